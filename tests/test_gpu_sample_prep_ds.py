"""GPU: sample preparation for the Oxford and nuScenes loaders (deepi2p_amd.sample_prep with dataset=..., di2p_range_shuffle,
di2p_gather_ragged_aug_intensity, di2p_sample_draws_ds, di2p_image_prepare_ds) against tests/sample_prep_ds_oracle.py, which
tests/test_sample_prep_ds_host.py pins against the reference's own functions.  Small shapes: input_pt_num 256, 16 nodes, frames of 0, 1, 257
and ~5000 points (only the last passes 2 * input_pt_num after the filter) and one frame wholly outside the range."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, sample_prep, scan_prep, synthetic
from tests import sample_prep_ds_oracle as dso
from tests import sample_prep_oracle as spo

pytestmark = pytest.mark.gpu
N, NODES, RANGE = 256, 16, 50.0
AMP = dict(P_tx_amplitude=10.0, P_ty_amplitude=5.0, P_tz_amplitude=10.0, P_Rx_amplitude=0.1, P_Ry_amplitude=2.0 * math.pi, P_Rz_amplitude=0.2)
OX = SimpleNamespace(crop_original_bottom_rows=8, img_H=24, img_W=32, input_pt_num=N, node_a_num=NODES, node_b_num=NODES, pc_max_range=RANGE, **AMP)
NU = SimpleNamespace(crop_original_top_rows=10, img_H=8, img_W=16, input_pt_num=N, node_a_num=NODES, node_b_num=NODES, **AMP)
CASES = {"oxford": (OX, (72, 96)), "nuscenes": (NU, (60, 100))}
RANGES = [(0.8, 1.2)] * 3 + [(-0.1, 0.1)]


def _np(t):
    return t.cpu().numpy()


def _odict(optb):
    return dict(top=optb.crop_top, scale=optb.img_scale, img_H=optb.img_H, img_W=optb.img_W, Hs=optb.Hs, Ws=optb.Ws, amp=list(optb.amplitude), ranges=RANGES)


@pytest.fixture(scope="module")
def clouds(dev):
    """five Oxford sub-maps (0, 1, 257, 5000 points, and 300 points shifted wholly outside the range) and four velodyne scans cut to the same
    counts; packed once, never modified"""
    rng = np.random.default_rng(3)
    ox = [synthetic.make_oxford_submap(rng, n) if n else np.zeros((4, 0), np.float32) for n in (0, 1, 257, 5000)]
    ox[1][:3, 0] = [1.0, 1.5, 20.0]          # the single point lies inside the range
    far = synthetic.make_oxford_submap(rng, 300)
    far[2] += 200.0
    ox.append(far)
    scan = synthetic.make_velodyne_scan(np.random.default_rng(4))
    nu = [np.ascontiguousarray(scan[i::11][:n].T) for i, n in enumerate((0, 1, 257, 5000))]
    out = {}
    for name, recs in (("oxford", ox), ("nuscenes", nu)):
        pts, off, host = scan_prep.pack([r.T for r in recs], dev)
        out[name] = (recs, pts, off, host)
    return out


@pytest.fixture(scope="module")
def cameras(dev):
    rng = np.random.default_rng(5)
    out = {}
    for name, (opt, hw) in CASES.items():
        raw = np.stack([synthetic.make_camera_image(np.random.default_rng(300 + b), hw[0], hw[1]) for b in range(5)])
        K = np.tile(np.array([[120.0, 0, hw[1] / 2 + 0.3], [0, 120.0, hw[0] / 2 - 0.7], [0, 0, 1]]), (5, 1, 1))
        Pcp = np.tile(np.eye(4), (5, 1, 1))
        for b in range(5):
            Pcp[b, :3, :3], Pcp[b, :3, 3] = spo.rotation(rng.uniform(-0.1, 0.1, 3)), rng.uniform(-6, 6, 3)
        out[name] = (raw, torch.from_numpy(raw).to(dev), K, torch.from_numpy(K).to(dev), Pcp, torch.from_numpy(Pcp).to(dev))
    return out


def test_filter_shuffle_bit_for_bit(dev, clouds):
    recs, pts, off, host = clouds["oxford"]
    cap = pts.shape[0]
    got = {}
    for seed in (7, 8):
        o_pts, o_off, st = scan_prep.range_shuffle(pts, off, RANGE, seed=seed, max_frame_points=5000)
        o_pts, o_off = _np(o_pts), _np(o_off)
        assert np.all(_np(st) == 0) and o_off[0] == 0
        for b, r in enumerate(recs):
            want, order = dso.range_shuffle(r.T, seed, b, RANGE)
            assert o_off[b + 1] - o_off[b] == len(order), (b, seed)
            assert np.array_equal(o_pts[o_off[b]:o_off[b + 1]], want), (b, seed)
        got[seed] = o_pts[:o_off[-1]].copy()
        counts = np.diff(o_off)
        assert counts[0] == 0 and counts[1] == 1 and counts[4] == 0 and 2 * N < counts[3] < 5000 and 0 < counts[2] <= 257
    assert got[7].shape == got[8].shape and not np.array_equal(got[7], got[8])          # two seeds, two orders of the same set
    assert np.array_equal(np.sort(got[7].view(np.uint32), 0), np.sort(got[8].view(np.uint32), 0))
    sd = torch.tensor([7], dtype=torch.int64, device=dev)
    again = scan_prep.range_shuffle(pts, off, RANGE, seed=99, seed_dev=sd, max_frame_points=5000)
    assert np.array_equal(_np(again[0])[:len(got[7])], got[7])          # the same seed (from device memory), the same order
    # r <= 0 keeps every point; a frame above max_frame_points is rejected through the status and writes nothing
    everything = scan_prep.range_shuffle(pts, off, 0.0, seed=7, max_frame_points=5000)
    assert np.array_equal(_np(everything[1]), np.array(host, dtype=np.int32))
    out = (torch.full((cap, 4), -7.0, device=dev), torch.zeros(6, dtype=torch.int32, device=dev), torch.zeros(5, dtype=torch.int32, device=dev))
    scan_prep.range_shuffle(pts, off, RANGE, seed=7, max_frame_points=1000, out=out)
    o_off = _np(out[1])
    kept = [len(dso.range_shuffle(r.T, 7, b, RANGE)[1]) for b, r in enumerate(recs)]
    kept[3] = 0          # the rejected frame has no output rows
    assert list(_np(out[2])) == [0, 0, 0, 1, 0] and np.array_equal(o_off, np.concatenate([[0], np.cumsum(kept)]))
    assert np.all(_np(out[0])[o_off[-1]:] == -7.0)
    want2, _ = dso.range_shuffle(recs[2].T, 7, 2, RANGE)
    assert np.array_equal(_np(out[0])[o_off[2]:o_off[3]], want2)


@pytest.mark.parametrize("name", ["oxford", "nuscenes"])
def test_image_path_bit_for_bit(dev, cameras, name):
    opt, hw = CASES[name]
    raw, dimg, K, dK, Pcp, dP = cameras[name]
    for mode in ("train", "val"):
        optb = sample_prep.option_block(opt, hw, mode, dataset=name)
        plan = sample_prep.ImagePlan(optb, 5, hw, mode, dev, dataset=name, color=True if mode == "train" else None)
        table = sample_prep.sample_draws_ds(optb, dK, dP, seed=21)
        ints, fac, drawn = _np(table.ints), _np(table.factors), _np(table.enable).copy()
        for forced in ((1, 0, None) if mode == "train" else (None,)):
            if forced is not None:
                table.enable.fill_(forced)
            else:
                table.enable.copy_(torch.from_numpy(drawn))
            en = _np(table.enable)
            got = _np(plan.run(dimg, table))
            want = np.stack([dso.prepare_image(raw[b], optb.crop_top, optb.crop_bottom, optb.img_scale, optb.img_H, optb.img_W, ints[b], fac[b], en[b],
                                               color=mode == "train") for b in range(5)])
            print("%s %s enable %s: %d differing floats" % (name, mode, forced, int((got != want).sum())))
            assert np.array_equal(got, want), (mode, forced)
        if mode == "val":
            assert np.all(ints[:, :3] == [(optb.Ws - optb.img_W) // 2, (optb.Hs - optb.img_H) // 2, 0]) and not drawn.any()
        else:
            assert 0 < drawn.sum() < 5, "seed 21 should enable some frames and not others"
    # a caller's table cannot flip these data sets' images
    table.ints[:, 2] = 1
    assert np.array_equal(_np(plan.run(dimg, table)), got)


def test_nuscenes_real_size_image(dev):
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(400 + b), 900, 1600) for b in range(2)])
    K = np.tile(np.array([[1266.4, 0, 816.3], [0, 1266.4, 491.5], [0, 0, 1]]), (2, 1, 1))
    img, Kp = sample_prep.prepare_images(raw, K, SimpleNamespace(), "val", dataset="nuscenes")
    assert tuple(img.shape) == (2, 3, 160, 320)
    want = np.stack([dso.prepare_image(raw[b], 100, 0, 0.2, 160, 320, [0, 0, 0, 0, 1, 2, 3, 0], np.ones(4), 0, False) for b in range(2)])
    assert np.array_equal(_np(img), want) and np.array_equal(want[0, :, 3, 7], raw[0, 100 + 17, 37].astype(np.float32))
    assert np.array_equal(_np(Kp)[0], spo.camera_matrix(K[0], 100, 0.2, 0, 0).astype(np.float32))
    optb = sample_prep.option_block(SimpleNamespace(img_H=96, img_W=200), (900, 1600), "train", dataset="nuscenes")
    dK, eye = torch.from_numpy(K).cuda(), torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1)
    table = sample_prep.sample_draws_ds(optb, dK, eye, seed=3)
    table.enable.fill_(1)
    got = _np(sample_prep.ImagePlan(optb, 2, (900, 1600), "train", dev, dataset="nuscenes").run(torch.from_numpy(raw).to(dev), table))
    ints, fac = _np(table.ints), _np(table.factors)
    assert np.array_equal(got, np.stack([dso.prepare_image(raw[b], 100, 0, 0.2, 96, 200, ints[b], fac[b], 1) for b in range(2)]))


@pytest.mark.parametrize("name", ["oxford", "nuscenes"])
def test_draws(dev, name):
    n = 256
    opt, hw = CASES[name]
    rng = np.random.default_rng(6)
    K = np.tile(np.array([[120.0, 0, 50.3], [0, 121.0, 29.3], [0, 0, 1]]), (n, 1, 1)) + rng.uniform(0, 1e-3, (n, 3, 3)) * [[1, 0, 1], [0, 1, 1], [0, 0, 0]]
    Pcp = np.tile(np.eye(4), (n, 1, 1))
    for b in range(n):
        Pcp[b, :3, :3], Pcp[b, :3, 3] = spo.rotation(rng.uniform(-0.1, 0.1, 3)), rng.uniform(-6, 6, 3)
    dK, dP = torch.from_numpy(K).to(dev), torch.from_numpy(Pcp).to(dev)
    for mode in ("train", "val", "val_random_Ry"):
        optb = sample_prep.option_block(opt, hw, mode, dataset=name)
        t = sample_prep.sample_draws_ds(optb, dK, dP, seed=2024)
        ora = dso.sample_draws(2024, range(n), mode, name, K, Pcp, _odict(optb))
        en = _np(t.enable)
        assert np.array_equal(_np(t.ints), ora["ints"]) and np.array_equal(_np(t.factors), ora["factors"]) and np.array_equal(en, ora["enable"])
        assert np.array_equal(_np(t.K), ora["K"])          # K' bit for bit
        Pr = _np(t.Pr)
        assert np.abs(Pr - ora["Pr"]).max() <= 1e-14
        R = Pr[:, :3, :3]
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14 and np.all(np.linalg.det(R) > 0) and np.all(Pr[:, 3] == [0, 0, 0, 1])
        assert np.abs(_np(t.P) - ora["P"]).max() <= 1e-6 * (1 + np.abs(ora["P"]).max())
        assert np.array_equal(_np(t.t_ij), Pcp[:, :3, 3].astype(np.float32)) and np.all(_np(t.ints)[:, 2] == 0)
        if mode == "train":
            # 256 frames of seed 2024: the enabled share within 5 binomial standard errors of 1/2 (the oracle's own draw passes, host test)
            assert abs(en.mean() - 0.5) <= 5 * math.sqrt(0.25 / n) and 0.34 <= en.mean() <= 0.66
            assert np.abs(Pr[:, :3, 3]).max(0) == pytest.approx([10.0, 5.0, 10.0], rel=0.05) and np.abs(Pr[:, 0, 3]).min() < 0.5
            kitti = sample_prep.sample_draws(sample_prep.option_block(SimpleNamespace(), (370, 1226), "train"), dK, dP, None, seed=2024)
            assert np.array_equal(_np(kitti.factors), ora["factors"])          # the frame's uniforms did not move
        elif mode == "val":
            assert np.array_equal(Pr, np.tile(np.eye(4), (n, 1, 1))) and np.array_equal(_np(t.P), Pcp[:, :3].astype(np.float32)) and not en.any()
        else:
            axis = 1 if name == "oxford" else 2
            e = np.zeros(3)
            e[axis] = 1.0
            assert np.abs(R @ e - e).max() <= 1e-15 and np.abs(R.transpose(0, 2, 1) @ e - e).max() <= 1e-15
            assert np.abs(R[:, 0, 0]).min() < 0.2 and np.all(Pr[:, :3, 3] == 0) and not en.any()
    t8 = sample_prep.sample_draws_ds(optb, dK[:1], dP[:1], seed=2024, frame0=5)          # a pure function of (seed, frame)
    assert np.array_equal(_np(t8.Pr)[0], _np(sample_prep.sample_draws_ds(optb, dK[5:6], dP[5:6], seed=2024, frame0=5).Pr)[0])
    assert np.array_equal(_np(t8.Pr)[0, :3, :3], Pr[5, :3, :3])


def test_jitter_coordinates_and_intensity(dev):
    B, n, sigma, clip, seed = 3, 4096, 0.01, 0.05, 31
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.uniform(-40, 40, (B * n, 3)).astype(np.float32)).to(dev)
    it = torch.from_numpy(rng.random(B * n).astype(np.float32)).to(dev)
    off = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
    idx = torch.from_numpy(np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32)).to(dev)
    T = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        T[b, :3, :3], T[b, :3, 3] = spo.rotation(rng.uniform(-1, 1, 3)), rng.uniform(-5, 5, 3)
    dT = torch.from_numpy(T).to(dev)

    def new(px, pi, tr):
        pc, oi = torch.empty((B, 3, n), device=dev), torch.empty((B, 1, n), device=dev)
        _lib.call("di2p_gather_ragged_aug_intensity", px.data_ptr(), pi.data_ptr(), off.data_ptr(), idx.data_ptr(), _lib.ptr(tr), B, n, seed, None, 0,
                  sigma, clip, pc.data_ptr(), oi.data_ptr(), _lib.stream())
        return _np(pc), _np(oi)[:, 0]
    old_pc, old_it = torch.empty((B, 3, n), device=dev), torch.empty((B, 1, n), device=dev)
    _lib.call("di2p_gather_ragged_aug", x.data_ptr(), it.data_ptr(), None, off.data_ptr(), idx.data_ptr(), dT.data_ptr(), B, n, seed, None, 0, sigma, clip,
              old_pc.data_ptr(), old_it.data_ptr(), None, _lib.stream())
    pc, inten = new(x, it, dT)
    assert np.array_equal(pc, _np(old_pc))          # coordinates: di2p_gather_ragged_aug's bits, transform included
    src = _np(it).reshape(B, n)[np.arange(B)[:, None], _np(idx)]
    assert np.array_equal(_np(old_it)[:, 0], src)          # the existing entry point leaves the intensity alone
    zpc, noise = new(torch.zeros_like(x), torch.zeros_like(it), None)          # in = 0: the float32 noise itself
    assert np.array_equal(inten, noise + src)          # float32 noise + float32 value
    assert np.abs(noise).max() <= np.float32(clip)
    # (clipping at 5 sigma costs 1.6e-7 of the variance, see test_gpu_sample_prep.test_jitter)
    m = noise.size
    assert abs(noise.astype(np.float64).mean()) <= 5 * sigma / math.sqrt(m) and abs(noise.astype(np.float64).std() - sigma) <= 5 * sigma / math.sqrt(2.0 * m)
    for b in range(B):
        want = dso.intensity_noise(seed, b, n, sigma, clip)
        assert (np.abs(noise[b].astype(np.float64) - want) / np.spacing(np.abs(want))).max() <= 1.0, b
        for c in range(3):
            assert not np.array_equal(noise[b], zpc[b, c])          # its own Philox slot


@pytest.mark.parametrize("name", ["oxford", "nuscenes"])
def test_plan_all_modes(dev, clouds, cameras, name):
    opt, hw = CASES[name]
    recs, pts, off, host = clouds[name]
    raw, dimg, K, dK, Pcp, dP = cameras[name]
    B = len(recs)
    for mode in ("train", "val", "val_random_Ry"):
        plan = sample_prep.SamplePlan(opt, B, pts.shape[0], 5000, hw, mode, dev, jitter=None, dataset=name)
        assert plan.sn is not None and not plan.sn.any()
        pc, inten, sn, na, nb, P, img, Kp, t_ij = [_np(t) for t in plan.run(pts, None, off, dimg[:B], dK[:B], dP[:B], seed=3)]
        assert np.all(_np(plan.status) == 0) and not sn.any() and sn.shape == pc.shape == (B, 3, N) and na.shape == (B, 3, NODES)
        idx, v_off, v_pts, v_int = _np(plan.points.idx), _np(plan.points.v_off), _np(plan.points.v_pts).astype(np.float64), _np(plan.points.v_int)
        counts = np.diff(v_off)
        src_counts = np.diff(_np(plan.filtered[1])) if name == "oxford" else np.diff(host)
        assert counts[3] < src_counts[3] and np.array_equal(counts[:3], src_counts[:3])          # both sides of the "> 2 * input_pt_num" voxel rule
        assert not pc[0].any() and not inten[0].any()          # an empty frame gives zeros
        if name == "oxford":
            assert counts[4] == 0 and not pc[4].any() and not na[4].any()          # a frame wholly outside the range: zeros, no fault
        Pr = _np(plan.table.Pr)
        for b in range(B):
            if counts[b] == 0:
                continue
            src = v_pts[v_off[b] + idx[b]].T
            assert np.allclose(pc[b], Pr[b, :3, :3] @ src + Pr[b, :3, 3:4], rtol=2e-7, atol=2e-7 * np.abs(Pr[b, :3, 3]).max())
            assert np.array_equal(inten[b, 0], v_int[v_off[b] + idx[b]])
            # P . [pc; 1] against P_cam_pc . [pc before Pr; 1]: 2e-7 of the larger norm per component, translations included
            lhs = P[b].astype(np.float64) @ np.concatenate([pc[b].astype(np.float64), np.ones((1, N))], 0)
            rhs = (Pcp[b] @ np.concatenate([src, np.ones((1, N))], 0))[:3]
            scale = np.maximum(np.linalg.norm(rhs, axis=0), np.linalg.norm(pc[b].astype(np.float64), axis=0))
            worst = (np.abs(lhs - rhs).max(0) / scale).max()
            print("%s %s frame %d: P bookkeeping worst relative error %.3g" % (name, mode, b, worst))
            assert worst <= 2e-7
        assert np.array_equal(t_ij, Pcp[:B, :3, 3].astype(np.float32)) and img.shape == (B, 3, opt.img_H, opt.img_W) and Kp.shape == (B, 3, 3)
        if mode == "val":          # a superset, not a second implementation: scan_prep.BatchPlan(voxel=0.2) fed the filter's output
            ref_plan = scan_prep.BatchPlan(B, pts.shape[0], 5000, N, NODES, voxel=0.2, device=dev, normals=False)
            fp, fo = (plan.filtered[0], plan.filtered[1]) if name == "oxford" else (pts, off)
            ref = ref_plan.run(fp, None, fo, 3)
            for a, r in zip((pc, inten, na, nb), (ref[0], ref[1], ref[3], ref[4])):
                assert np.array_equal(a, _np(r))
            assert np.array_equal(P, Pcp[:B, :3].astype(np.float32))
        if mode == "train":          # with the jitter: the same choice, noise on coordinates (before Pr) and on the intensity
            jplan = sample_prep.SamplePlan(opt, B, pts.shape[0], 5000, hw, mode, dev, dataset=name)
            jout = [_np(t) for t in jplan.run(pts, None, off, dimg[:B], dK[:B], dP[:B], seed=3)]
            assert np.array_equal(_np(jplan.points.idx), idx) and not jout[2].any()
            for b in range(B):
                if counts[b] == 0:
                    continue
                noise, _ = spo.jitter_noise(3, b, N, *sample_prep.JITTER)
                x = spo.jitter(v_pts[v_off[b] + idx[b]].T.astype(np.float32), noise[0]).astype(np.float64)
                want = Pr[b, :3, :3] @ x + Pr[b, :3, 3:4]
                err = np.abs(jout[0][b] - want).max(0) / np.maximum(np.linalg.norm(want, axis=0), 1e-3)
                assert err.max() <= 2e-7, (b, err.max())
                d = jout[1][b, 0].astype(np.float64) - inten[b, 0]
                ni = dso.intensity_noise(3, b, N, *sample_prep.JITTER)
                assert np.abs(d - ni).max() <= 2 * np.spacing(np.float32(1.0)) and np.abs(d).max() > 1e-3
    got = sample_prep.prepare_samples(recs, raw[:B], K[:B], Pcp[:B], opt, "val", seed=3, dataset=name)          # the convenience wrapper: the same nine
    assert got[2] is not None and not _np(got[2]).any() and tuple(got[0].shape) == (B, 3, N)


@pytest.mark.parametrize("name", ["oxford", "nuscenes"])
def test_graph_replay(dev, clouds, cameras, name):
    opt, hw = CASES[name]
    recs, pts, off, host = clouds[name]
    raw, dimg, K, dK, Pcp, dP = cameras[name]
    B = len(recs)
    plan = sample_prep.SamplePlan(opt, B, pts.shape[0], 5000, hw, "train", dev, dataset=name)
    args = (pts, None, off, dimg[:B], dK[:B], dP[:B])
    eager = {s: [t.clone() for t in plan.run(*args, seed=s)] for s in (11, 12)}
    assert not torch.equal(eager[11][0], eager[12][0]) and not torch.equal(eager[11][5], eager[12][5])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run(*args, seed=None)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = plan.run(*args, seed=None)
    for s in (12, 11):
        plan.seed.fill_(s)
        for t in (out[0], out[1], out[3], out[4], out[6]):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[s], out):
            assert torch.equal(a, b), s
    assert not out[2].any() and np.all(_np(plan.status) == 0)          # sn: exactly zero, before and after


def test_kitti_keyword_changes_nothing(dev):
    rng = np.random.default_rng(8)
    recs = []
    for n in (700, 300):
        p = np.stack([rng.uniform(2, 60, n), rng.uniform(-25, 25, n), rng.uniform(-2, 3, n)])
        recs.append(np.concatenate([p, rng.random((1, n)), rng.standard_normal((3, n))], 0).astype(np.float32))
    points, normals, offsets, host = scan_prep.pack_records(recs, dev)
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(500 + b), 74, 122) for b in range(2)])
    opt = SimpleNamespace(crop_original_top_rows=10, img_H=24, img_W=48, input_pt_num=N, node_a_num=NODES, node_b_num=NODES, **AMP)
    K = torch.from_numpy(np.tile(np.array([[90.0, 0, 60.2], [0, 90.0, 37.1], [0, 0, 1]]), (2, 1, 1))).to(dev)
    Pc = torch.from_numpy(np.tile(np.array([[0, -1, 0, 0], [0, 0, -1, -0.05], [1, 0, 0, -0.3], [0, 0, 0, 1.0]]), (2, 1, 1))).to(dev)
    outs = []
    for kw in ({}, {"dataset": "kitti"}):
        plan = sample_prep.SamplePlan(opt, 2, points.shape[0], 700, (74, 122), "train", dev, **kw)
        outs.append([t.clone() for t in plan.run(points, normals, offsets, torch.from_numpy(raw).to(dev), K, Pc, None, seed=5)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][2].any() and outs[0][0].any()
