"""CPU: the Oxford / nuScenes restatement (tests/sample_prep_ds_oracle.py) against the reference's own functions
(tests/golden/sample_prep_ds_golden.npz), the centre-pick resize against the bilinear rule it is derived from, the shuffle and the range
rule at their borders, and the argument errors of deepi2p_amd.sample_prep with dataset=..., all raised before any device work."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deepi2p_amd import sample_prep
from tests import sample_prep_ds_oracle as dso
from tests import sample_prep_oracle as spo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "sample_prep_ds_golden.npz"))
EPS32 = 2.0 ** -24          # unit round-off of float32


def test_camera_matrix_against_reference():
    """The reference works in float32 throughout (float32 K, the Python scale cast to float32, float32 subtractions): up to three float32
    roundings of values no larger than the scaled principal point / focal length, where the oracle rounds an fp64 result once.  Bound: 4
    unit round-offs of the largest scaled entry -- absolute, because the window subtraction may cancel."""
    for name, top in (("ox", 0), ("nu", int(G["nu_top"]))):
        K, s = G[name + "_K_raw"].astype(np.float64), float(G[name + "_scale"])
        bound = 4 * EPS32 * np.abs(s * K).max()
        for w, want in zip(G[name + "_windows"], G[name + "_K_out"]):
            got = spo.camera_matrix(K, top, s, int(w[0]), int(w[1])).astype(np.float32)
            assert want.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= bound, (name, w)
    # the Oxford order (scale, crop) is the KITTI formula with no top crop: the bottom crop never enters K
    assert np.array_equal(spo.camera_matrix(G["ox_K_raw"], 0, 0.5, 3, 4), spo.camera_matrix(G["ox_K_raw"], 0.0, 0.5, 3, 4))


def test_pose_against_reference():
    """Pr: the reference rounds an fp64 rotation and translation to float32 -> one unit round-off of each entry.  P = P_cam_pc . inv(Pr) in
    float32 there (a float32 LU inverse of a rotation, condition 1, then a float32 product): every entry of P is a sum of four products of
    magnitude <= max(1, |t_r|, |t_c|), each factor carrying a few round-offs; 32 unit round-offs of (1 + |t_r| + |t_c|) covers it with room
    and is still 2e-6 relative."""
    for name in ("ox", "nu", "ox_val", "nu_val"):
        amp = G[name + "_amp"]
        for u, Pr_ref, Pcp, P_ref in zip(G[name + "_unit"], G[name + "_Pr"], G[name + "_P_cam_pc"], G[name + "_P"]):
            Pr = dso.pose_from_uniforms(u, amp)
            assert Pr_ref.dtype == np.float32 and np.abs(Pr - Pr_ref).max() <= EPS32 * max(1.0, np.abs(Pr).max())
            P = dso.assemble_pose(Pr, Pcp.astype(np.float64))
            scale = 1.0 + np.linalg.norm(Pr[:3, 3]) + np.linalg.norm(Pcp[:3, 3])
            assert np.abs(P.astype(np.float64) - P_ref[:3]).max() <= 32 * EPS32 * scale, name
    assert dso.val_amplitudes("oxford") == list(G["ox_val_amp"]) and dso.val_amplitudes("nuscenes") == list(G["nu_val_amp"])
    # val_random_Ry about y leaves y alone, about z leaves z alone
    for ds, axis in (("oxford", 1), ("nuscenes", 2)):
        Pr = dso.pose_from_uniforms([0.3] * 6, dso.val_amplitudes(ds))
        e = np.zeros(3)
        e[axis] = 1.0
        assert np.allclose(Pr[:3, :3] @ e, e, atol=1e-15) and abs(Pr[0, 0] - 1.0) > 0.1 and np.all(Pr[:3, 3] == 0)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_centre_pick_is_the_bilinear_rule(k):
    rng = np.random.default_rng(k)
    img = rng.integers(0, 256, (k * 11, k * 13, 3)).astype(np.uint8)
    pick = dso.resize(img, 1.0 / k)
    assert pick.shape == (11, 13, 3) and np.array_equal(pick, img[(k - 1) // 2::k, (k - 1) // 2::k])
    assert np.array_equal(dso.bilinear_f64(img, k), pick.astype(np.float64))          # weights exactly (1, 0): no rounding at all
    assert not np.array_equal(dso.bilinear_f64(img, 2)[:5, :6], img[::2, ::2][:5, :6].astype(np.float64))          # even k is NOT a pick


def test_shuffle_is_a_seeded_permutation():
    rng = np.random.default_rng(0)
    pts = rng.uniform(-10, 10, (777, 4)).astype(np.float32)
    out, order = dso.range_shuffle(pts, 5, 2, 0.0)
    assert sorted(order) == list(range(777)) and np.array_equal(out, pts[order]) and not np.array_equal(order, np.arange(777))
    assert np.array_equal(dso.range_shuffle(pts, 5, 2, 0.0)[1], order)
    assert not np.array_equal(dso.range_shuffle(pts, 6, 2, 0.0)[1], order) and not np.array_equal(dso.range_shuffle(pts, 5, 3, 0.0)[1], order)
    keys = dso.shuffle_keys(5, 2, 777)
    assert np.all(np.diff(keys[order].astype(np.float64)) >= 0) and keys.max() < np.uint64(1) << np.uint64(63)


def test_range_rule_at_its_borders():
    r = 50.0
    r2 = np.float32(r) * np.float32(r)
    below, above = np.nextafter(r2, np.float32(0)), np.nextafter(r2, np.float32(np.inf))
    rows = np.array([[30, 7, 40, 0],          # 900 + 1600 = 2500: not < 2500, dropped (the test is strict)
                     [30, -1000, np.sqrt(np.float32(1599.9)), 0],          # y does not count
                     [0, 0, np.sqrt(below.astype(np.float64)), 0], [0, 0, np.sqrt(above.astype(np.float64)), 0], [0, 0, 50, 0],
                     [-30, 0, -39.99, 0], [49.99, 0, 0, 0], [0, 99, 0, 0]], dtype=np.float32)
    keep = dso.range_keep(rows, r)
    x2z2 = rows[:, 0] * rows[:, 0] + rows[:, 2] * rows[:, 2]
    assert x2z2.dtype == np.float32 and np.array_equal(keep, x2z2 < r2)
    assert not keep[0] and keep[1] and not keep[4] and keep[5] and keep[6] and keep[7]
    # the float32 neighbours of r^2 themselves
    assert dso.range_keep(np.array([[np.sqrt(below), 0, 0, 0]], np.float32), r)[0] == (np.float32(np.sqrt(below)) ** 2 < r2)
    sq = np.array([below, r2, above], dtype=np.float32)
    assert list(sq < r2) == [True, False, False]
    assert dso.range_keep(rows, 0.0).all() and dso.range_keep(rows, -1.0).all()


def test_intensity_noise_is_its_own_stream():
    n = dso.intensity_noise(9, 1, 4096, 0.01, 0.05)
    pts, _ = spo.jitter_noise(9, 1, 4096, 0.01, 0.05)
    assert n.dtype == np.float32 and np.abs(n).max() <= np.float32(0.05)
    for w in range(2):
        for c in range(3):
            assert not np.array_equal(n, pts[w, c])
    assert np.array_equal(dso.intensity_noise(9, 1, 4096, 0.01, 0.05, slot=0), pts[0, 0])          # the same rule on the slots the oracle shares


def test_colour_enable_share_of_the_committed_seed():
    """256 frames of seed 2024: the enabled share within 5 binomial standard errors (0.5 / 16 each) of 1/2, i.e. in [0.34, 0.66]"""
    o = dict(top=0, scale=0.5, img_H=24, img_W=32, Hs=32, Ws=48, amp=[0.0] * 6, ranges=[(0.8, 1.2)] * 3 + [(-0.1, 0.1)])
    d = dso.sample_draws(2024, range(256), "train", "oxford", np.tile(np.eye(3), (256, 1, 1)), np.tile(np.eye(4), (256, 1, 1)), o)
    share = d["enable"].mean()
    assert abs(share - 0.5) <= 5 * math.sqrt(0.25 / 256) and 0.34 <= share <= 0.66
    assert np.all(d["ints"][:, 2] == 0)          # no flip
    v = dso.sample_draws(2024, range(8), "val", "oxford", np.tile(np.eye(3), (8, 1, 1)), np.tile(np.eye(4), (8, 1, 1)), o)
    assert not v["enable"].any() and np.all(v["ints"][:, :2] == [8, 4])


# ---------------------------------------------------------------------------------------------------------------- the public interface
def test_option_block_of_the_data_sets():
    ox = sample_prep.option_block(SimpleNamespace(), (960, 1280), "train", dataset="oxford")
    assert (ox.crop_top, ox.crop_bottom, ox.img_scale, ox.Hs, ox.Ws, ox.img_H, ox.img_W, ox.resize_k, ox.dataset) == (0, 0, 0.5, 480, 640, 384, 640, 0, 1)
    assert list(ox.amplitude) == [10.0, 5.0, 10.0, 0.0, 2.0 * math.pi, 0.0] and ox.max_range == 50.0
    nu = sample_prep.option_block(SimpleNamespace(), (900, 1600), "train", dataset="nuscenes")
    assert (nu.crop_top, nu.crop_bottom, nu.img_scale, nu.Hs, nu.Ws, nu.img_H, nu.img_W, nu.resize_k, nu.dataset) == (100, 0, 0.2, 160, 320, 160, 320, 5, 2)
    assert list(nu.amplitude) == [0.0] * 5 + [2.0 * math.pi] and nu.max_range == 0.0
    small = sample_prep.option_block(SimpleNamespace(crop_original_bottom_rows=8, img_H=24, img_W=32), (72, 96), "val", dataset="oxford")
    assert (small.crop_bottom, small.Hs, small.Ws) == (8, 32, 48)
    for name in ("crop_original_bottom_rows", "pc_max_range", "P_tx_amplitude", "img_H", "img_W", "img_scale"):
        assert name in sample_prep.DATASET_DEFAULTS["oxford"] and name in sample_prep.DATASET_DEFAULTS["nuscenes"]


def test_kitti_keyword_changes_nothing():
    for opt, hw, mode in ((SimpleNamespace(), (370, 1226), "train"), (SimpleNamespace(img_H=128, img_W=480, P_tx_amplitude=0.8), (370, 1226), "val")):
        a, b = sample_prep.option_block(opt, hw, mode), sample_prep.option_block(opt, hw, mode, dataset="kitti")
        assert bytes(a) == bytes(b) and (b.dataset, b.crop_bottom, b.resize_k, b.max_range) == (0, 0, 0, 0.0)
    with pytest.raises(ValueError, match="img_scale"):
        sample_prep.option_block(SimpleNamespace(img_scale=0.2), (370, 1225), "train")          # 1/k stays a data-set rule


def test_argument_errors_before_device_work():
    ns = SimpleNamespace
    with pytest.raises(ValueError, match="img_scale"):
        sample_prep.option_block(ns(img_scale=0.25), (900, 1600), "train", dataset="nuscenes")          # even k
    with pytest.raises(ValueError, match="img_scale"):
        sample_prep.option_block(ns(img_scale=0.3), (900, 1600), "train", dataset="nuscenes")
    with pytest.raises(ValueError, match="divides"):
        sample_prep.option_block(ns(), (901, 1600), "train", dataset="nuscenes")          # 801 rows, k = 5
    with pytest.raises(ValueError, match="divides"):
        sample_prep.option_block(ns(), (900, 1601), "train", dataset="nuscenes")
    with pytest.raises(ValueError, match="larger than the scaled image"):
        sample_prep.option_block(ns(img_H=161), (900, 1600), "train", dataset="nuscenes")
    with pytest.raises(ValueError, match="larger than the scaled image"):
        sample_prep.option_block(ns(crop_original_bottom_rows=200), (960, 1280), "train", dataset="oxford")          # 380 rows < 384
    for fn in (lambda: sample_prep.option_block(ns(), (960, 1280), "train", dataset="waymo"),
               lambda: sample_prep.prepare_images(np.zeros((1, 60, 100, 3), np.uint8), np.eye(3)[None], ns(), "val", dataset="waymo"),
               lambda: sample_prep.prepare_samples([], np.zeros((1, 60, 100, 3), np.uint8), np.eye(3)[None], np.eye(4)[None], ns(), dataset="waymo"),
               lambda: sample_prep.SamplePlan(ns(), 1, 16, 16, dataset="waymo"), lambda: sample_prep.ImagePlan(ns(), 1, dataset="waymo")):
        with pytest.raises(ValueError, match="unknown dataset"):
            fn()
    img = np.zeros((1, 60, 100, 3), np.uint8)
    opt = ns(img_H=8, img_W=16, crop_original_top_rows=10)
    rec = [np.zeros((4, 5), np.float32)]
    with pytest.raises(ValueError, match="Pji"):
        sample_prep.prepare_samples(rec, img, np.eye(3)[None], np.eye(4)[None], opt, "train", Pji=np.eye(4)[None], dataset="nuscenes")
    with pytest.raises(ValueError, match="no normals"):
        sample_prep.prepare_samples([np.zeros((7, 5), np.float32)], img, np.eye(3)[None], np.eye(4)[None], opt, "train", dataset="nuscenes")
    with pytest.raises(ValueError, match="no normals"):
        sample_prep.prepare_samples((torch.zeros(5, 4), torch.zeros(5, 3)), img, np.eye(3)[None], np.eye(4)[None], opt, "train",
                                    offsets=torch.tensor([0, 5], dtype=torch.int32), dataset="oxford")
    with pytest.raises(ValueError, match="img_scale"):
        sample_prep.prepare_samples(rec, img, np.eye(3)[None], np.eye(4)[None], ns(img_scale=0.25, crop_original_top_rows=10), "train", dataset="nuscenes")
    with pytest.raises(ValueError, match="images is None"):
        sample_prep.prepare_samples(rec, None, np.eye(3)[None], np.eye(4)[None], opt, "train", dataset="oxford")


def test_nuscenes_accumulation_transform():
    rng = np.random.default_rng(4)

    def pose():
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = spo.rotation(rng.uniform(-0.3, 0.3, 3)), rng.uniform(-20, 20, 3)
        return P
    P_oi, P_vl, P_oj = pose(), pose(), np.stack([pose() for _ in range(3)])
    T = sample_prep.accumulation_transforms_nuscenes(P_oi, P_oj, P_vl)
    assert T.shape == (3, 4, 4) and T.dtype == np.float64
    for j in range(3):          # :227-229 in the reference's association order
        P_ij = np.dot(np.linalg.inv(P_oi), P_oj[j])
        assert np.allclose(T[j], np.dot(np.dot(np.linalg.inv(P_vl), P_ij), P_vl), rtol=0, atol=1e-12)
    assert np.allclose(sample_prep.accumulation_transforms_nuscenes(P_oi, P_oi, P_vl), np.eye(4), rtol=0, atol=1e-12)
