"""GPU: training-sample preparation (deepi2p_amd.sample_prep, csrc/sample_prep.hip, the jittered gather of csrc/scan_prep.hip) against the
numpy restatement in tests/sample_prep_oracle.py, which tests/test_sample_prep_host.py pins against PIL and the reference's own code."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, sample_prep, scan_prep, synthetic
from tests import sample_prep_oracle as spo
from tests import scan_prep_oracle as vox

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "sample_prep_golden.npz"))
K_RAW, PC = G["K_raw"], G["item_Pc"]
OPT = SimpleNamespace(P_tx_amplitude=0.8, P_ty_amplitude=0.5, P_tz_amplitude=1.0, P_Rx_amplitude=0.1, P_Ry_amplitude=2.0 * math.pi, P_Rz_amplitude=0.2)
SMALL = SimpleNamespace(img_H=128, img_W=480)          # a window with room in both directions: dx in [0, 133], dy in [0, 32]


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def images(dev):
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(100 + i)) for i in range(8)])
    return raw, torch.from_numpy(raw).to(dev)


def _oracle_images(raw, optb, ints, factors, color=True):
    out = [spo.prepare_image(raw[b], optb.crop_top, optb.img_scale, optb.img_H, optb.img_W, ints[b], factors[b], color) for b in range(len(raw))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int64)


def _forced_table(dev, ints, factors):
    t = sample_prep.DrawTable(len(ints), dev)
    t.ints.copy_(torch.from_numpy(np.asarray(ints, dtype=np.int32)))
    t.factors.copy_(torch.from_numpy(np.asarray(factors, dtype=np.float32)))
    return t


def test_image_path_bit_for_bit_forced_draws(dev, images):
    """all 24 orders, both flip values, the four corner windows and the centred one, through a caller-supplied draw table"""
    raw, dimg = images
    rng = np.random.default_rng(1)
    for opt, windows in ((SimpleNamespace(), [(0, 0), (101, 0), (50, 0), (37, 0)]), (SMALL, [(0, 0), (133, 0), (0, 32), (133, 32), (66, 16)])):
        plan = sample_prep.ImagePlan(opt, 8, (370, 1226), "train", dev)
        for rep in range(3):
            ints = np.zeros((8, 8), np.int32)
            fac = np.concatenate([rng.uniform(0.8, 1.2, (8, 3)), rng.uniform(-0.1, 0.1, (8, 1))], 1).astype(np.float32)
            for b in range(8):
                dx, dy = windows[(rep * 8 + b) % len(windows)]
                ints[b] = [dx, dy, (b + rep) & 1, *spo.PERMS[rep * 8 + b], spo.hue_shift_of(fac[b, 3])]
            got = _np(plan.run(dimg, _forced_table(dev, ints, fac)))
            want, gsum = _oracle_images(raw, plan.optb, ints, fac)
            print("forced draws: window set %d rep %d: %d differing floats" % (len(windows), rep, int((got != want).sum())))
            assert np.array_equal(got, want)
            assert np.array_equal(plan.grey_sums(), gsum)          # 3. the contrast mean's integer sum, windows at every corner
            again = _np(plan.run(dimg, _forced_table(dev, ints, fac), reduce_blocks=(1, 37, 128)[rep])).copy()
            assert np.array_equal(again, got) and np.array_equal(plan.grey_sums(), gsum)          # another launch geometry, the same integers


def test_image_path_bit_for_bit_own_draws_and_validation_geometry(dev, images):
    raw, dimg = images
    K = torch.from_numpy(np.tile(K_RAW, (8, 1, 1))).to(dev)
    eye = torch.eye(4, dtype=torch.float64, device=dev).repeat(8, 1, 1)
    for mode in ("train", "val"):
        optb = sample_prep.option_block(SMALL, (370, 1226), mode)
        table = sample_prep.sample_draws(optb, K, eye, None, seed=77)
        plan = sample_prep.ImagePlan(optb, 8, (370, 1226), mode, dev)
        got = _np(plan.run(dimg, table))
        ints, fac = _np(table.ints), _np(table.factors)
        want, _ = _oracle_images(raw, optb, ints, fac, color=(mode == "train"))
        assert np.array_equal(got, want)
        if mode == "val":
            assert np.all(ints[:, :3] == [66, 16, 0])
    img, K2 = sample_prep.prepare_images(raw, np.tile(K_RAW, (8, 1, 1)), SimpleNamespace(), "val")
    want, _ = _oracle_images(raw, sample_prep.option_block(SimpleNamespace(), (370, 1226), "val"), np.tile([50, 0, 0, 0, 1, 2, 3, 0], (8, 1)), np.ones((8, 4)), False)
    assert np.array_equal(_np(img), want)
    assert np.array_equal(_np(K2)[0], spo.camera_matrix(K_RAW, 50, 0.5, 50, 0).astype(np.float32))


def test_hue_exhaustive(dev):
    """every RGB colour through the hue operation alone (the three blends with factor 1 are the identity) for the fixture's six shifts"""
    allc = spo.all_colours()
    d = torch.from_numpy(allc[None]).to(dev)
    opt = SimpleNamespace(crop_original_top_rows=0, img_scale=1.0, img_H=4096, img_W=4096)
    plan = sample_prep.ImagePlan(opt, 1, (4096, 4096), "train", dev, geometry=False, color=True)
    idx = spo.colour_subsample()
    for k, h in enumerate(G["hue_values"]):
        ints = [[0, 0, 0, *spo.PERMS[(5 * k) % 24], spo.hue_shift_of(h)]]
        out = plan.run(d, _forced_table(dev, ints, [[1.0, 1.0, 1.0, h]]))
        got = _np(out[0].to(torch.uint8).permute(1, 2, 0).contiguous()).reshape(-1, 3)
        assert np.array_equal(got[idx].T, G["hue_sub"][k]), h
        assert spo.checksum(got) == G["hue_checksum"][k], h


def test_draws(dev):
    n = 4096
    optb = sample_prep.option_block(SimpleNamespace(img_H=128, img_W=480, **vars(OPT)), (370, 1226), "train")
    K = torch.from_numpy(np.tile(K_RAW, (n, 1, 1))).to(dev)
    Pc = torch.from_numpy(np.tile(PC, (n, 1, 1))).to(dev)
    t = sample_prep.sample_draws(optb, K, Pc, None, seed=5)
    ints, fac, Pr, P, Kp = _np(t.ints), _np(t.factors), _np(t.Pr), _np(t.P), _np(t.K)
    # a pure function of (seed, frame)
    t8 = sample_prep.sample_draws(optb, K[:8], Pc[:8], None, seed=5)
    t1 = sample_prep.sample_draws(optb, K[:1], Pc[:1], None, seed=5, frame0=5)
    for name in ("ints", "factors", "Pr", "PrPcn", "P", "K"):
        a, b, c = _np(getattr(t, name)), _np(getattr(t8, name)), _np(getattr(t1, name))
        assert np.array_equal(a[:8], b[:8]) and np.array_equal(b[5], c[0]), name
    other = sample_prep.sample_draws(optb, K[:8], Pc[:8], None, seed=6)
    assert not np.array_equal(_np(other.ints)[:8], ints[:8]) and not np.array_equal(_np(other.factors)[:8], fac[:8])
    seed_dev = torch.tensor([5], dtype=torch.int64, device=dev)
    assert np.array_equal(_np(sample_prep.sample_draws(optb, K[:8], Pc[:8], None, seed=99, seed_dev=seed_dev).ints), ints[:8])
    # against the oracle: integers, factors and K' exactly; the matrices up to the libraries' sin / cos (a few fp64 ulp)
    ora = spo.sample_draws(5, range(64), "train", np.tile(K_RAW, (64, 1, 1)), np.tile(PC, (64, 1, 1)), np.tile(np.eye(4), (64, 1, 1)),
                           dict(top=50, scale=0.5, img_H=128, img_W=480, Hs=160, Ws=613, amp=list(optb.amplitude), ranges=[(0.8, 1.2)] * 3 + [(-0.1, 0.1)]))
    assert np.array_equal(ints[:64], ora["ints"]) and np.array_equal(fac[:64], ora["factors"]) and np.array_equal(Kp[:64], ora["K"])
    assert np.abs(Pr[:64] - ora["Pr"]).max() <= 1e-14 and np.abs(P[:64] - ora["P"]).max() <= 1e-6
    # ranges, both ends hit; all 24 orders
    assert ints[:, 0].min() == 0 and ints[:, 0].max() == 133 and ints[:, 1].min() == 0 and ints[:, 1].max() == 32
    assert len({tuple(r) for r in ints[:, 3:7]}) == 24 and all(sorted(r) == [0, 1, 2, 3] for r in ints[:, 3:7])
    # flip rate and factor means within 5 standard errors of the uniform's
    se = math.sqrt(0.25 / n)
    assert abs(ints[:, 2].mean() - 0.5) <= 5 * se
    for k, (lo, hi) in enumerate(((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))):
        assert fac[:, k].min() >= np.float32(lo) and fac[:, k].max() <= np.float32(hi)
        assert abs(fac[:, k].mean() - 0.5 * (lo + hi)) <= 5 * (hi - lo) / math.sqrt(12.0 * n), k
    for name, m in (("dx", 134), ("dy", 33)):
        v = ints[:, 0 if name == "dx" else 1]
        assert abs(v.mean() - (m - 1) / 2.0) <= 5 * math.sqrt((m * m - 1) / 12.0 / n), name
    R = Pr[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14
    assert np.array_equal(np.sign(np.linalg.det(R)), np.where(ints[:, 2] == 1, -1.0, 1.0))          # the flip mirrors Pr


def test_jitter(dev):
    B, N, sigma, clip, seed = 4, 20480, 0.01, 0.05, 31
    rng = np.random.default_rng(2)
    x = rng.uniform(-40, 40, (B * N, 3)).astype(np.float32)
    s = rng.standard_normal((B * N, 3)).astype(np.float32)
    off = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=dev)
    idx = torch.arange(N, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    inten = torch.zeros((B * N,), dtype=torch.float32, device=dev)

    def run(px, ps, sd=seed):
        out = [torch.empty((B, 3, N), dtype=torch.float32, device=dev), torch.empty((B, 1, N), dtype=torch.float32, device=dev),
               torch.empty((B, 3, N), dtype=torch.float32, device=dev)]
        _lib.call("di2p_gather_ragged_aug", px.data_ptr(), inten.data_ptr(), ps.data_ptr(), off.data_ptr(), idx.data_ptr(), None, B, N, sd, None, 0,
                  sigma, clip, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _lib.stream())
        return _np(out[0]), _np(out[2])
    zero = torch.zeros((B * N, 3), dtype=torch.float32, device=dev)
    n_pc, n_sn = run(zero, zero)          # out - in with in = 0: the float32 noise itself
    noise = np.concatenate([n_pc.reshape(-1), n_sn.reshape(-1)]).astype(np.float64)
    n = noise.size // 2          # B * 3 * N samples per stream (points, normals)
    assert np.abs(noise).max() <= np.float32(clip)
    # clipping at 5 sigma: the variance loses 2 * int_5^inf (z^2 - 25) phi(z) dz = 2 * (26 * Q(5) - 5 * phi(5)) ~ 1.6e-7 relative (< 1e-4),
    # far below the sampling error 5 * sigma / sqrt(2 n) ~ 7e-3 relative of the bound below
    for part in (noise[:n], noise[n:]):
        assert abs(part.mean()) <= 5 * sigma / math.sqrt(n)
        assert abs(part.std() - sigma) <= 5 * sigma / math.sqrt(2.0 * n)
    for b in range(B):
        ora, _ = spo.jitter_noise(seed, b, N, sigma, clip)
        for got, want in ((n_pc[b], ora[0]), (n_sn[b], ora[1])):
            ulp = np.spacing(np.abs(want))
            worst = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
            assert worst.max() <= 1.0, (b, worst.max())
    # (independent of the launch grid by construction: the Philox counter is (output index, frame, component), nothing of the grid)
    # float32 noise + float32 value, exactly; and another seed gives other noise
    j_pc, j_sn = run(torch.from_numpy(x).to(dev), torch.from_numpy(s).to(dev))
    assert np.array_equal(j_pc, n_pc + x.reshape(B, N, 3).transpose(0, 2, 1)) and np.array_equal(j_sn, n_sn + s.reshape(B, N, 3).transpose(0, 2, 1))
    assert not np.array_equal(run(zero, zero, seed + 1)[0], n_pc)


def _records(rng, counts):
    recs = []
    for n in counts:
        p = np.stack([rng.uniform(2, 60, n), rng.uniform(-25, 25, n), rng.uniform(-2, 3, n)])          # Velodyne frame: x forward
        sn = rng.standard_normal((3, n))
        recs.append(np.concatenate([p, rng.random((1, n)), sn / np.linalg.norm(sn, axis=0)], 0).astype(np.float32))
    return recs


def test_pose_bookkeeping_all_modes(dev, images):
    raw, dimg = images
    B = 4
    rng = np.random.default_rng(8)
    recs = _records(rng, (30000, 25000, 36000, 21000))          # below 2 * input_pt_num: the voxel pass copies them
    points, normals, offsets, host = scan_prep.pack_records(recs, dev)
    Pji = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        Pji[b, :3, :3], Pji[b, :3, 3] = spo.rotation(rng.uniform(-0.05, 0.05, 3)), rng.uniform(-4, 4, 3)
    K, Pc, Pj = [torch.from_numpy(a).to(dev) for a in (np.tile(K_RAW, (B, 1, 1)), np.tile(PC, (B, 1, 1)), Pji)]
    for mode in ("train", "val", "val_random_Ry"):
        plan = sample_prep.SamplePlan(OPT, B, points.shape[0], 36000, (370, 1226), mode, dev, jitter=None)
        pc, inten, sn, na, nb, P, img, Kp, t_ji = [_np(t) for t in plan.run(points, normals, offsets, dimg[:B], K, Pc, Pj, seed=3)]
        assert np.all(_np(plan.status) == 0)
        idx, v_off, v_pts = _np(plan.points.idx), _np(plan.points.v_off), _np(plan.points.v_pts).astype(np.float64)
        v_nrm = _np(plan.points.v_nrm).astype(np.float64)
        flips = _np(plan.table.ints)[:, 2]
        PrPcn = _np(plan.table.PrPcn)
        for b in range(B):
            src = v_pts[v_off[b] + idx[b]].T          # the points the gather chose, Velodyne frame
            # the device's own transform from its fp64 table, rounded once: element-wise rtol 2e-7 (the project's transform tolerance), no atol
            assert np.allclose(pc[b], PrPcn[b, :3, :3] @ src + PrPcn[b, :3, 3:4], rtol=2e-7, atol=0)
            # normals take the ROTATION of Pr . P_cam_nwu only (flipped frames included).  The reference's transform_pc_np is homogeneous and
            # would add Pr's translation to the normals when a P_t*_amplitude is non-zero (it is zero in kitti/options.py): not reproduced.
            assert np.allclose(sn[b], PrPcn[b, :3, :3] @ v_nrm[v_off[b] + idx[b]].T, rtol=2e-7, atol=0)
            # P . [pc; 1] against Pji . Pc . [pc_nwu; 1].  Both P and pc are float32 here (eps32 = 6e-8 relative on every entry of P and on
            # every coordinate), so a component of the product carries up to ~ 3 * 2 * eps32 * |P_ij| |pc_j| <= 3.6e-7 of the largest
            # coordinate, however small the component itself is: an element-wise rtol is unreachable for components near zero.  The bound is
            # therefore 2e-7 of the point's norm (the larger of the two sides), per component.
            lhs = P[b].astype(np.float64) @ np.concatenate([pc[b].astype(np.float64), np.ones((1, pc.shape[2]))], 0)
            rhs = (Pji[b] @ PC @ np.concatenate([src, np.ones((1, src.shape[1]))], 0))[:3]
            scale = np.maximum(np.linalg.norm(rhs, axis=0), np.linalg.norm(pc[b].astype(np.float64), axis=0))
            worst = (np.abs(lhs - rhs).max(0) / scale).max()
            print("pose bookkeeping %s frame %d flip %d: worst relative error %.3g" % (mode, b, flips[b], worst))
            assert worst <= 2e-7
        if mode == "train":
            # jitter and transform together: out = T . float32(x + noise), the noise added in float32 BEFORE the rigid transform.  The noise
            # depends on (seed, frame, output index, component) only -- the counter holds no launch geometry -- so the oracle's noise applies.
            # The device's noise may differ from the oracle's by one float32 ulp of the noise (test_jitter), which can move the float32 sum by
            # one ulp of the coordinate: bound 2e-7 of the point's norm.
            jplan = sample_prep.SamplePlan(OPT, B, points.shape[0], 36000, (370, 1226), mode, dev)
            assert jplan.jitter == sample_prep.JITTER
            jout = [_np(t) for t in jplan.run(points, normals, offsets, dimg[:B], K, Pc, Pj, seed=3)]
            assert np.array_equal(_np(jplan.points.idx), idx) and np.array_equal(_np(jplan.table.PrPcn), PrPcn)
            for b in range(B):
                noise, _ = spo.jitter_noise(3, b, pc.shape[2], *sample_prep.JITTER)
                for got, clean, srcv, w, trans in ((jout[0][b], pc[b], v_pts, 0, 1.0), (jout[2][b], sn[b], v_nrm, 1, 0.0)):
                    x = spo.jitter(srcv[v_off[b] + idx[b]].T.astype(np.float32), noise[w]).astype(np.float64)
                    want = PrPcn[b, :3, :3] @ x + trans * PrPcn[b, :3, 3:4]
                    err = np.abs(got - want).max(0) / np.maximum(np.linalg.norm(want, axis=0), 1e-3)
                    assert err.max() <= 2e-7, (b, w, err.max())
                    assert np.abs(got - clean).max() > 1e-3          # the jitter is there (up to 0.05 per component)
        assert np.array_equal(t_ji, Pji[:, :3, 3].astype(np.float32)) and img.shape == (B, 3, 160, 512) and Kp.shape == (B, 3, 3)
        if mode == "val":          # a superset, not a second implementation: bit-identical to scan_prep with P = P_cam_nwu
            ref_plan = scan_prep.BatchPlan(B, points.shape[0], 36000, 20480, 128, device=dev)
            Pcn = torch.from_numpy(np.tile(spo.P_CAM_NWU, (B, 1, 1))).to(dev)
            ref = scan_prep.prepare_batch_into(ref_plan, points, normals, offsets, 3, Pcn)
            for a, r in zip((pc, inten, sn, na, nb), ref):
                assert np.array_equal(a, _np(r))
        if mode == "train":
            assert 0 < flips.sum() < B, "seed 3 should give flipped and unflipped frames"


def test_accumulation(dev):
    rng = np.random.default_rng(12)
    frames, poses = [], []
    for f, k in enumerate((3, 1, 3)):
        scans, ps = [], []
        for j in range(k):
            s = synthetic.make_velodyne_scan(np.random.default_rng(60 + 4 * f + j))
            sn = rng.standard_normal((s.shape[0], 3)).astype(np.float32)
            scans.append(np.concatenate([s.T, sn.T], 0))
            P = np.eye(4)
            P[:3, :3], P[:3, 3] = spo.rotation([0.002 * j, 0.03 * j + 0.1 * f, -0.001 * j]), [0.9 * j + f, -0.02 * j, 5.0 * j]
            ps.append(P)
        frames.append(scans)
        poses.append(ps)
    Pcs = [PC] * 3
    flat = [r for f in frames for r in f]
    raw_p, raw_n, seg_off, seg_host = scan_prep.pack_records(flat, dev)
    raw_p, raw_n = _np(raw_p), _np(raw_n)
    points, normals, seg, frame_off = sample_prep.accumulate(frames, poses, Pcs, dev)
    T = np.concatenate(sample_prep.accumulation_transforms(poses, Pcs), 0)
    assert np.array_equal(T[0], np.eye(4)) and np.array_equal(T[3], np.eye(4))
    for s, (f, j) in enumerate([(f, j) for f in range(3) for j in range(len(frames[f]))]):
        assert np.allclose(T[s], spo.accumulation_transform(PC, poses[f][0], poses[f][j]), rtol=0, atol=1e-12)
    want_p, want_n = spo.transform_segments(raw_p, raw_n, seg_host, T)
    got_p, got_n = _np(points), _np(normals)
    assert np.allclose(got_p, want_p, rtol=2e-7, atol=0) and np.allclose(got_n, want_n, rtol=2e-7, atol=0)
    assert np.array_equal(got_p[:, 3], raw_p[:, 3])
    fo = _np(frame_off)
    assert list(fo) == [seg_host[0], seg_host[3], seg_host[4], seg_host[7]]
    # the 0.3 m voxel pass merges the scans of a frame exactly as it treats one scan: bit for bit on the device's own transformed points
    st = scan_prep.voxel_down_sample(points, frame_off, 0.3, normals=normals, want_keys=True)
    assert np.all(_np(st.status) == 0)
    vo = _np(st.offsets)
    for b in range(3):
        ref = vox.voxel_down_sample(got_p[fo[b]:fo[b + 1]], 0.3, normals=got_n[fo[b]:fo[b + 1]])
        sl = slice(vo[b], vo[b + 1])
        assert vo[b + 1] - vo[b] == len(ref["keys"])
        assert np.array_equal(_np(st.keys)[sl], ref["keys"]) and np.array_equal(_np(st.points)[sl], ref["points"])
        assert np.array_equal(_np(st.intensity)[sl], ref["intensity"]) and np.array_equal(_np(st.normals)[sl], ref["normals"])


def test_graph_replay_with_device_seed_and_training_step(dev, images):
    raw, dimg = images
    B = 2
    recs = _records(np.random.default_rng(21), (45000, 38000))          # above 2 * input_pt_num: the 0.3 m voxel pass runs
    points, normals, offsets, host = scan_prep.pack_records(recs, dev)
    K, Pc = [torch.from_numpy(a).to(dev) for a in (np.tile(K_RAW, (B, 1, 1)), np.tile(PC, (B, 1, 1)))]
    plan = sample_prep.SamplePlan(OPT, B, points.shape[0], 45000, (370, 1226), "train", dev)
    eager = {s: [t.clone() for t in plan.run(points, normals, offsets, dimg[:B], K, Pc, None, seed=s)] for s in (11, 12)}
    assert not torch.equal(eager[11][0], eager[12][0]) and not torch.equal(eager[11][6], eager[12][6])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run(points, normals, offsets, dimg[:B], K, Pc, None, seed=None)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = plan.run(points, normals, offsets, dimg[:B], K, Pc, None, seed=None)          # the seed stays in plan.seed: a device-side argument
    for s in (12, 11):
        plan.seed.fill_(s)
        for t in out[:8]:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[s], out):
            assert torch.equal(a, b), s
    # straight into one training step
    from deepi2p_amd import networks
    from deepi2p_amd.training import ClassifierTrainer
    got = sample_prep.prepare_samples(recs, raw[:B], np.tile(K_RAW, (B, 1, 1)), np.tile(PC, (B, 1, 1)), SimpleNamespace(), "train", seed=4)
    pc, inten, sn, na, nb, P, img, Kp, t_ji = got
    opt = synthetic.OptLike(20480, 160, 512, True)
    opt.lr, opt.coarse_loss_alpha = 1e-3, 50.0
    det = networks.KeypointDetector(opt)
    det.load_state_dict(synthetic.random_state_dict(opt, 5))
    tr = ClassifierTrainer(det.to(dev), opt)
    L = tr.optimize(pc, inten, sn, na, nb, img, Kp, P)
    assert math.isfinite(float(L["loss"]))
    lab = _np(L["coarse_labels"])
    assert lab.min() == 0 and lab.max() == 1, "the projected labels should contain both classes"


def test_graph_replay_above_2_20_points(dev, images):
    """SamplePlan.run replayed from a graph with more than 2^20 points in the batch (rocPRIM's radix sort changes algorithm there): the
    replay equals the eager launches bit for bit, for two seeds written into the plan's seed slot."""
    raw, dimg = images
    B = 20
    recs = _records(np.random.default_rng(33), [60000] * B)
    points, normals, offsets, host = scan_prep.pack_records(recs, dev)
    assert host[-1] > (1 << 20)
    big = dimg.repeat(3, 1, 1, 1)[:B].contiguous()
    K, Pc = [torch.from_numpy(a).to(dev) for a in (np.tile(K_RAW, (B, 1, 1)), np.tile(PC, (B, 1, 1)))]
    plan = sample_prep.SamplePlan(OPT, B, points.shape[0], 60000, (370, 1226), "train", dev)
    eager = {s: [t.clone() for t in plan.run(points, normals, offsets, big, K, Pc, None, seed=s)] for s in (1, 2)}
    torch.cuda.synchronize()
    assert np.all(_np(plan.status) == 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run(points, normals, offsets, big, K, Pc, None, seed=None)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = plan.run(points, normals, offsets, big, K, Pc, None, seed=None)
    for s in (2, 1):
        plan.seed.fill_(s)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[s], out):
            assert torch.equal(a, b), s
    assert np.all(_np(plan.status) == 0)


def test_prepare_images_into_registration_executor(dev, images):
    """prepare_images' outputs (float32 [B,3,H,W] image and float32 K', on the device) go into RegistrationExecutor.submit as they are"""
    from deepi2p_amd.networks import MMClassiferCoarse
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    raw, _ = images
    B, N, H, W = 3, 2048, 64, 128
    opt = synthetic.OptLike(N, H, W, False)
    opt.device = dev
    mm = MMClassiferCoarse(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    b = synthetic.make_batch(500, B, N=N, H=H, W=W)
    host = {k: torch.from_numpy(b[k]) for k in ("pc", "intensity", "sn", "node_a", "node_b", "img")}
    img, Kp = sample_prep.prepare_images(raw[:B], np.tile(K_RAW, (B, 1, 1)), SimpleNamespace(img_H=H, img_W=W), "val")
    assert img.dtype == torch.float32 and tuple(img.shape) == (B, 3, H, W) and img.is_cuda and Kp.dtype == torch.float32 and tuple(Kp.shape) == (B, 3, 3)
    pipe = RegistrationPipeline(H, W, R=6, seed=3)
    ex = RegistrationExecutor(mm, pipe, torch.from_numpy(b["K"]).to(dev), host, n_streams=1, restarts=pipe.draw(B, dev))
    batch = dict(host, img=img, K=Kp)
    got = {k: v.clone() for k, v in ex.result(ex.submit(batch)).items() if torch.is_tensor(v)}
    slot = ex.slots[0]
    assert torch.equal(slot.devs[slot.cur]["img"], img) and torch.equal(slot.devs[slot.cur]["K"], Kp.double())      # what the step read
    ref = {k: v.clone() for k, v in ex.result(ex.submit(dict(host, img=img.cpu(), K=Kp.cpu()))).items() if torch.is_tensor(v)}
    assert got.keys() == ref.keys() and "P" in got
    for k in got:
        assert torch.equal(got[k], ref[k]), k
    assert torch.isfinite(got["cost"]).all()
