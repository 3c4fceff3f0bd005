"""CPU: the numpy oracle of the training-sample preparation (tests/sample_prep_oracle.py) reproduces every array of
tests/golden/sample_prep_golden.npz (PIL's colour operations, the reference's camera-matrix, pose, jitter and accumulation code), the new
symbols are declared, exported and bound, and argument errors are reported before anything touches a device."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import sample_prep_oracle as spo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "sample_prep_golden.npz"))
NEW = ["di2p_sample_draws", "di2p_image_prepare", "di2p_image_prepare_workspace_bytes", "di2p_transform_segments", "di2p_gather_ragged_aug",
       "di2p_random_choice_dseed", "di2p_random_choice_ragged_dseed"]
IMAGE_SEED, CROPS = 2024, ((50, 0), (50, 202))


def _crops():
    from deepi2p_amd import synthetic
    raw = synthetic.make_camera_image(np.random.default_rng(IMAGE_SEED))
    return [spo.resize(raw[r:r + 320, c:c + 1024], 0.5) for r, c in CROPS]


def test_colour_chain_equals_pil_in_all_24_orders():
    cs = _crops()
    for ci, c in enumerate(cs):
        assert spo.checksum(c) == G["crop_checksum"][ci], "synthetic.make_camera_image drifted from the fixture's generator"
        for oi, order in enumerate(spo.PERMS):
            f = G["order_factors"][oi]
            got, _ = spo.color_jitter(c, order, f, spo.hue_shift_of(f[3]))
            assert np.array_equal(got[::16, ::16].transpose(2, 0, 1), G["order_sub"][ci, oi]), (ci, order)
            assert spo.checksum(got) == G["order_checksum"][ci, oi], (ci, order)


def test_hue_equals_pil_over_all_colours():
    allc, idx = spo.all_colours(), spo.colour_subsample()
    for k, h in enumerate(G["hue_values"]):
        got = spo.adjust_hue(allc, spo.hue_shift_of(h)).reshape(-1, 3)
        assert np.array_equal(got[idx].T, G["hue_sub"][k]), h
        assert spo.checksum(got) == G["hue_checksum"][k], h


def test_camera_matrix_and_rotation_bit_for_bit():
    for a, want in zip(G["K_args"], G["K_out"]):
        assert np.array_equal(spo.camera_matrix(G["K_raw"], int(a[0]), a[1], int(a[2]), int(a[3])), want)
    for a, want in zip(G["rot_angles"], G["rot_out"]):
        assert np.array_equal(spo.rotation(a), want)


def test_jitter_bit_for_bit():
    for tag, sigma in (("jit", 0.01), ("jit2", 0.03)):
        noise = spo.jitter_from_normals(G[tag + "_normals"], sigma, 0.05)
        got = spo.jitter(G[tag + "_in"], noise)
        assert got.dtype == np.float32 and np.array_equal(got, G[tag + "_out"])
        assert np.abs(noise).max() <= np.float32(0.05)


def test_getitem_block_all_modes():
    """Pr and K' bit for bit.  P: the oracle inverts Pr in closed form, the reference with np.linalg.inv (LU).  Bound: LAPACK's inverse of
    a well-conditioned (orthogonal rotation, |t| <= 1.4 m) 4x4 is accurate to a few eps = 2.2e-16 per entry, say 8 eps ~ 2e-15; P multiplies
    it by P_nwu_cam (a signed permutation: exact), Pc (|rotation entries| <= 1, |t| < 0.3) and Pji (rotation, |t| <= 7): each of the 12
    entries is a sum of at most 4 + 4 such products of magnitude O(1) .. O(7), so |dP| <= ~ (1 + 1 + 1 + 0.3) * 2e-15 + rounding of the
    sums (a few ulp of values below 16: 4 * 1.8e-15) < 1e-14 absolute."""
    from deepi2p_amd import synthetic
    raw = synthetic.make_camera_image(np.random.default_rng(IMAGE_SEED + 1))
    n_train = n_flip = 0
    for i, mode in enumerate(G["item_mode"]):
        d = G["item_draws"][i]
        if mode == 0:
            dx, dy, t, ang, flip = int(d[0]), int(d[1]), d[2:5], d[5:8], d[8] > 0.5
            n_train, n_flip = n_train + 1, n_flip + int(flip)
        elif mode == 2:
            dx, dy, t, ang, flip = 50, 0, d[0:3], d[3:6], False
            assert np.all(t == 0) and ang[0] == 0 and ang[2] == 0
        else:
            dx, dy, t, ang, flip = 50, 0, np.zeros(3), np.zeros(3), False
        Pr = spo.random_pose(ang, t, flip)
        assert np.array_equal(Pr, G["item_Pr"][i])
        assert np.array_equal(spo.camera_matrix(G["K_raw"], 50, 0.5, dx, dy), G["item_K"][i])
        PrPcn, P32 = spo.assemble_pose(Pr, G["item_Pc"], G["item_Pji"][i])
        P64 = np.dot(G["item_Pji"][i], np.dot(G["item_Pc"], np.dot(spo.P_NWU_CAM, spo.rigid_inverse(Pr))))
        assert np.abs(P64 - G["item_P"][i]).max() <= 1e-14
        assert np.array_equal(P32, P64[:3].astype(np.float32))
        pc, sn = G["item_pc_in"][i]
        # the reference moves points AND normals with the homogeneous transform_pc_np, i.e. it adds Pr's translation to the normals too; this
        # pins the oracle's Pr . P_cam_nwu against both.  The DEVICE applies the rotation only to normals (DESIGN.md section 3;
        # tests/test_gpu_sample_prep.py checks sn = R . sn_src), which agrees with the reference wherever the P_t*_amplitudes are zero.
        for x, want in ((pc, G["item_pc_out"][i]), (sn, G["item_sn_out"][i])):
            h = np.concatenate([x.astype(np.float64), np.ones((1, x.shape[1]))], 0)
            assert np.allclose(np.dot(PrPcn, h)[:3], want, rtol=0, atol=1e-12)
        ints = np.array([dx, dy, int(flip), 0, 1, 2, 3, 0])
        img, _ = spo.prepare_image(raw, 50, 0.5, 160, 512, ints, np.ones(4, np.float32), color=False)
        assert np.array_equal(img[:, ::8, ::8], G["item_img_sub"][i]) and spo.checksum(img.astype(np.uint8)) == G["item_img_sum"][i]
    assert n_train >= 3 and 0 < n_flip < n_train          # flipped and unflipped train frames are both in the fixture


def test_accumulation_against_reference():
    Pc = G["item_Pc"]
    for k in range(3):
        T = spo.accumulation_transform(Pc, G["acc_P_oi"], G["acc_P_oj"][k])          # float32 poses: the reference's own dtypes
        rec = G["acc_records"][k]
        h = np.concatenate([rec[0:3].astype(np.float64), np.ones((1, rec.shape[1]))], 0)
        assert np.array_equal(np.dot(T, h)[:3], G["acc_pc"][k])                          # same matrices, same np.dot: bit for bit
        R = T.copy()
        R[:3, 3] = 0
        hs = np.concatenate([rec[4:7].astype(np.float64), np.ones((1, rec.shape[1]))], 0)
        assert np.array_equal(np.dot(R, hs)[:3], G["acc_sn"][k])
        pts4 = np.ascontiguousarray(rec[0:4].T)
        p, n = spo.transform_segments(pts4, np.ascontiguousarray(rec[4:7].T), [0, pts4.shape[0]], T[None])
        assert np.allclose(p[:, :3], G["acc_pc"][k].T, rtol=2e-7, atol=1e-6) and np.allclose(n, G["acc_sn"][k].T, rtol=2e-7, atol=1e-6)
        assert np.array_equal(p[:, 3], pts4[:, 3])


def test_oracle_draws_are_a_function_of_seed_and_frame():
    o = dict(top=50, scale=0.5, img_H=160, img_W=512, Hs=160, Ws=613, amp=[0.5, 0.2, 1.0, 0.1, 2 * np.pi, 0.1], ranges=[(0.8, 1.2)] * 3 + [(-0.1, 0.1)])
    K, Pc = np.tile(G["K_raw"], (8, 1, 1)), np.tile(G["item_Pc"], (8, 1, 1))
    a = spo.sample_draws(9, range(8), "train", K, Pc, np.tile(np.eye(4), (8, 1, 1)), o)
    b = spo.sample_draws(9, [5], "train", K[5:6], Pc[5:6], np.eye(4)[None], o)
    for k in ("ints", "factors", "Pr", "P", "K"):
        assert np.array_equal(a[k][5], b[k][0])
    c = spo.sample_draws(10, range(8), "train", K, Pc, np.tile(np.eye(4), (8, 1, 1)), o)
    assert not np.array_equal(a["ints"], c["ints"])
    assert a["ints"][:, 0].min() >= 0 and a["ints"][:, 0].max() <= 101 and np.all(a["ints"][:, 1] == 0)
    assert all(sorted(r[3:7]) == [0, 1, 2, 3] for r in a["ints"])
    for Pr in a["Pr"]:
        assert np.abs(Pr[:3, :3] @ Pr[:3, :3].T - np.eye(3)).max() <= 1e-14


def test_new_symbols_declared_exported_and_bound():
    from deepi2p_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepi2p_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    ws = _lib.load().di2p_image_prepare_workspace_bytes
    assert ws(8) >= 32 and ws(8) % 256 == 0 and ws(-1) == 0


def test_python_argument_errors_before_any_device_work():
    from deepi2p_amd import sample_prep
    opt = SimpleNamespace()
    K = np.tile(G["K_raw"], (1, 1, 1))
    img = np.zeros((1, 370, 1226, 3), np.uint8)
    with pytest.raises(ValueError, match="images is None"):
        sample_prep.prepare_images(None, K, opt, "val")
    with pytest.raises(ValueError, match="images is None"):
        sample_prep.prepare_samples([np.zeros((7, 10), np.float32)], None, K, np.eye(4)[None], opt, "train")
    with pytest.raises(ValueError, match="odd scaled size"):
        sample_prep.prepare_images(np.zeros((1, 371, 1226, 3), np.uint8), K, opt, "val")
    with pytest.raises(ValueError, match="odd scaled size"):
        sample_prep.prepare_images(np.zeros((1, 370, 1225, 3), np.uint8), K, opt, "val")
    for scale in (0.2, 0.25, 2.0):
        with pytest.raises(ValueError, match="unsupported img_scale"):
            sample_prep.prepare_images(img, K, SimpleNamespace(img_scale=scale), "val")
    with pytest.raises(ValueError, match="larger than the scaled image"):
        sample_prep.prepare_images(img, K, SimpleNamespace(img_W=1024), "val")
    with pytest.raises(ValueError, match="larger than the scaled image"):
        sample_prep.prepare_images(img, K, SimpleNamespace(img_H=161), "train")
    with pytest.raises(ValueError, match="bad mode"):
        sample_prep.prepare_images(img, K, opt, "test")
    with pytest.raises(ValueError, match="bad mode"):
        sample_prep.option_block(opt, (370, 1226), "training")
    o = sample_prep.option_block(opt, (370, 1226), "train")          # defaults = kitti/options.py
    assert (o.crop_top, o.img_scale, o.img_H, o.img_W, o.Hs, o.Ws) == (50, 0.5, 160, 512, 160, 613)
    assert list(o.amplitude) == [0, 0, 0, 0, 2 * np.pi, 0] and list(o.color_range) == [0.8, 1.2, 0.8, 1.2, 0.8, 1.2, -0.1, 0.1]


def test_library_argument_errors():
    import concurrent.futures          # di2p_last_error is per thread; test_capi_and_host expects "ok" on the main thread
    with concurrent.futures.ThreadPoolExecutor(1) as ex:
        ex.submit(_library_argument_errors).result()


def _library_argument_errors():
    from deepi2p_amd import _lib, sample_prep
    E = _lib.DeepI2PHipError
    fake = 256          # never dereferenced: every call below fails its host-side checks first
    good = sample_prep.option_block(SimpleNamespace(), (370, 1226), "train")

    def img(o=good, images=fake, H0=370, W0=1226, B=1, ws=fake):
        _lib.call("di2p_image_prepare", images, B, H0, W0, o, fake, fake, 1, 1, 0, fake, ws, None)
    with pytest.raises(E, match="null pointer"):
        img(images=None)
    with pytest.raises(E, match="odd scaled size"):
        img(H0=371)
    with pytest.raises(E, match="does not match"):
        img(H0=372)
    img(B=0, images=None, ws=None)          # an empty batch is a valid no-op
    bad = sample_prep.option_block(SimpleNamespace(), (370, 1226), "train")
    bad.img_scale = 0.2
    with pytest.raises(E, match="unsupported img_scale"):
        img(o=bad)
    bad.img_scale, bad.img_W = 0.5, 614
    with pytest.raises(E, match="larger than the scaled image"):
        img(o=bad)
    bad.img_W, bad.mode = 512, 3
    with pytest.raises(E, match="bad mode"):
        _lib.call("di2p_sample_draws", 0, None, 1, 0, bad, fake, fake, None, fake, fake, fake, fake, fake, fake, None)
    with pytest.raises(E, match="null pointer"):
        _lib.call("di2p_sample_draws", 0, None, 1, 0, good, None, fake, None, fake, fake, fake, fake, fake, fake, None)
    _lib.call("di2p_sample_draws", 0, None, 0, 0, good, None, None, None, None, None, None, None, None, None, None)
    with pytest.raises(E, match="null pointer"):
        _lib.call("di2p_transform_segments", None, None, None, None, 2, 10, None, None, None)
    with pytest.raises(E, match="go together"):
        _lib.call("di2p_transform_segments", fake, fake, fake, fake, 2, 10, fake, None, None)
    _lib.call("di2p_transform_segments", None, None, None, None, 0, 0, None, None, None)
    with pytest.raises(E, match="clip > 0"):
        _lib.call("di2p_gather_ragged_aug", fake, fake, fake, fake, fake, None, 1, 8, 0, None, 0, 0.01, 0.0, fake, fake, fake, None)
    with pytest.raises(E, match="null"):
        _lib.call("di2p_gather_ragged_aug", None, None, None, None, None, None, 1, 8, 0, None, 0, 0.01, 0.05, None, None, None, None)
    with pytest.raises(E, match="null"):
        _lib.call("di2p_random_choice_ragged_dseed", None, 0, 2, fake, 100, 8, fake, fake, None)
