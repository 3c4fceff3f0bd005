"""GPU: raw-scan preparation (deepi2p_amd.scan_prep, csrc/scan_prep.hip) against the numpy / scipy restatement in
tests/scan_prep_oracle.py, on full-size synthetic HDL-64 scans in a ragged batch of 4 (unequal counts, one frame empty)."""
import numpy as np
import pytest
import torch

from deepi2p_amd import prep, scan_prep, synthetic
from tests import scan_prep_oracle as spo

pytestmark = pytest.mark.gpu


def _scans():
    s = [synthetic.make_velodyne_scan(np.random.default_rng(10 + i)) for i in range(3)]
    return [s[0], s[1][:70_000], np.zeros((0, 4), np.float32), s[2]]


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def batch(dev):
    scans = _scans()
    points, offsets, host = scan_prep.pack(scans, dev)
    st = scan_prep.voxel_down_sample(points, offsets, 0.1, want_keys=True)
    normals, cnt, nbr = scan_prep.estimate_normals(st, 0.6, 30, want_neighbors=True)
    nn_idx, nn_int, nn_d2 = scan_prep.nearest_raw(st, points, offsets)
    torch.cuda.synchronize()
    vo = _np(st.offsets)
    out = dict(scans=scans, points=points, offsets=offsets, vo=vo, status=_np(st.status), keys=_np(st.keys), pts=_np(st.points),
               inten=_np(st.intensity), normals=_np(normals), cnt=_np(cnt), nbr=_np(nbr), nn_idx=_np(nn_idx), nn_int=_np(nn_int), nn_d2=_np(nn_d2))
    out["ref"] = [spo.voxel_down_sample(s, 0.1) for s in scans]
    return out


def _frame(batch, name, b):
    return batch[name][batch["vo"][b]:batch["vo"][b + 1]]


def test_voxel_grid_bit_exact(batch):
    assert np.all(batch["status"] == 0)
    for b, ref in enumerate(batch["ref"]):
        n = batch["vo"][b + 1] - batch["vo"][b]
        assert n == len(ref["keys"]), b
        assert np.array_equal(_frame(batch, "keys", b), ref["keys"])
        assert np.array_equal(_frame(batch, "pts", b), ref["points"])
        assert np.array_equal(_frame(batch, "inten", b), ref["intensity"])
    assert batch["vo"][3] == batch["vo"][2]                          # the empty frame


def test_voxel_attributes_and_pass_through_bit_exact(dev):
    """The loader's 0.3 m pass on 7 x n records: averaged intensity (fake colour) and normals; a frame at or below min_points is copied."""
    rng = np.random.default_rng(3)
    recs = []
    for i, n in enumerate((90_000, 30_000, 0, 60_000)):
        s = synthetic.make_velodyne_scan(np.random.default_rng(20 + i))[:n]
        sn = rng.standard_normal((s.shape[0], 3)).astype(np.float32)
        recs.append((s, sn))
    points, offsets, host = scan_prep.pack([r[0] for r in recs], dev)
    normals, _, _ = scan_prep.pack([r[1] for r in recs], dev, cols=3)
    st = scan_prep.voxel_down_sample(points, offsets, 0.3, normals=normals, min_points=40_960, want_keys=True)
    vo = _np(st.offsets)
    for b, (s, sn) in enumerate(recs):
        ref = spo.voxel_down_sample(s, 0.3, normals=sn, min_points=40_960)
        sl = slice(vo[b], vo[b + 1])
        assert vo[b + 1] - vo[b] == len(ref["keys"]), b
        for got, want in ((st.keys, ref["keys"]), (st.points, ref["points"]), (st.intensity, ref["intensity"]), (st.normals, ref["normals"])):
            assert np.array_equal(_np(got[sl]), want), b
    assert vo[2] - vo[1] == 30_000                                   # passed through unchanged


def test_voxel_edge_cases(dev):
    """points exactly on voxel faces, negative coordinates, duplicates, a one-point frame"""
    v = 0.25
    g = np.arange(-6, 7) * v              # with the extra minimum -1.625, min_bound = -1.75: every grid value lies on a voxel face
    face = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    face = np.concatenate([face, [[-1.625, -1.625, -1.625]]])
    neg = face - 1000.0
    dup = np.repeat(face[:50], 7, axis=0)
    frames = [face, neg, dup, face[5:6]]
    rng = np.random.default_rng(4)
    frames = [np.concatenate([f, rng.random((len(f), 1))], 1).astype(np.float32) for f in frames]
    points, offsets, _ = scan_prep.pack(frames, dev)
    st = scan_prep.voxel_down_sample(points, offsets, v, want_keys=True)
    vo = _np(st.offsets)
    for b, f in enumerate(frames):
        ref = spo.voxel_down_sample(f, v)
        sl = slice(vo[b], vo[b + 1])
        assert vo[b + 1] - vo[b] == len(ref["keys"])
        assert np.array_equal(_np(st.keys[sl]), ref["keys"]) and np.array_equal(_np(st.points[sl]), ref["points"])
        assert np.array_equal(_np(st.intensity[sl]), ref["intensity"])
    assert vo[4] - vo[3] == 1


def test_normals_against_oracle(batch):
    for b, ref in enumerate(batch["ref"]):
        cen = ref["cen"]
        cnt, nbr = spo.neighbors(cen, 0.6, 30)
        got_cnt, got_nbr = _frame(batch, "cnt", b), _frame(batch, "nbr", b)
        assert np.array_equal(got_cnt, cnt), b
        # the neighbour sets: identical except where the 30th and 31st distances tie exactly
        same = np.all(np.sort(got_nbr, 1) == np.sort(nbr, 1), axis=1)
        if not np.all(same):
            bad = np.nonzero(~same)[0]
            c2, n2 = spo.neighbors(cen[:], 0.6, 31)
            for q in bad:
                d = spo.d2(cen[n2[q]], cen[q])
                assert c2[q] == 31 and d[29] == d[30], (b, q)
        if len(cen):
            from scipy.spatial import cKDTree
            dd, ii = cKDTree(cen).query(cen, k=30, distance_upper_bound=0.6)
            kd_cnt = np.isfinite(dd).sum(1)
            assert np.mean(kd_cnt == cnt) > 0.999
        nref, lam = spo.normals(cen, cnt, nbr)
        n = _frame(batch, "normals", b).astype(np.float64)
        gap = (lam[:, 1] - lam[:, 0]) / np.maximum(lam[:, 2], 1e-300)
        well = (cnt >= 3) & (gap > 1e-3)
        dots = np.abs(np.sum(n * nref, 1))
        # the kernel's fp64 normal is rounded to f32 on output: 1 - 1e-9 on the fp64 direction is 1 - 1e-7 on the f32 one
        assert np.all(dots[well] >= 1 - 1e-7), (b, dots[well].min())
        sure = np.abs(nref[:, 2]) > 1e-6
        assert np.all(n[sure, 2] >= 0)
        lone = cnt < 3
        assert np.all(n[lone] == np.array([0, 0, 1]))


def test_normals_fallbacks_and_dense_patch(dev):
    rng = np.random.default_rng(5)
    iso = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0]], np.float64)              # isolated points
    pair = np.array([[0, 0, 0], [0.3, 0, 0], [30, 0, 0], [30, 0.3, 0]], np.float64)  # pairs
    xy = np.stack(np.meshgrid(np.arange(20) * 0.05, np.arange(20) * 0.05, indexing="ij"), -1).reshape(-1, 2)
    patch = np.concatenate([xy, 0.3 * xy[:, :1] + 0.01 * rng.standard_normal((len(xy), 1))], 1)   # 400 points in a 1 m tilted patch
    frames = [np.concatenate([f, np.full((len(f), 1), 0.5)], 1).astype(np.float32) for f in (iso, pair, patch)]
    points, offsets, _ = scan_prep.pack(frames, dev)
    st = scan_prep.voxel_down_sample(points, offsets, 0.01)         # below the spacing: every point is a voxel of its own
    normals, cnt, nbr = scan_prep.estimate_normals(st, 0.6, 30, want_neighbors=True)
    vo, normals, cnt, nbr = _np(st.offsets), _np(normals), _np(cnt), _np(nbr)
    assert np.all(normals[vo[0]:vo[2]] == np.array([0, 0, 1], np.float32))
    assert np.array_equal(cnt[vo[0]:vo[1]], [1, 1, 1]) and np.array_equal(cnt[vo[1]:vo[2]], [2, 2, 2, 2])
    ref = spo.voxel_down_sample(frames[2], 0.01)
    c, i = spo.neighbors(ref["cen"], 0.6, 30)
    assert np.all(c == 30)                                          # more than max_nn inside r everywhere: the 30 nearest are kept
    assert np.array_equal(cnt[vo[2]:vo[3]], c) and np.array_equal(nbr[vo[2]:vo[3]], i)
    n = normals[vo[2]:vo[3]]
    assert np.all(n[:, 2] > 0.9)


def test_nearest_raw_exact(batch):
    for b, ref in enumerate(batch["ref"]):
        s = batch["scans"][b]
        idx, d2 = spo.nearest_raw(s, ref["cen"])
        got_d2 = _frame(batch, "nn_d2", b)
        assert np.array_equal(got_d2, d2), b
        raw = s[:, :3].astype(np.float64)
        got = _frame(batch, "nn_idx", b)
        # both pick the lower index among exact ties, so the indices agree; where they did not, the distance would still have to tie
        eq = got == idx
        if not np.all(eq):
            assert np.array_equal(spo.d2(raw[got[~eq]], ref["cen"][~eq]), d2[~eq])
        assert len(eq) == 0 or np.mean(eq) > 0.999
        assert np.array_equal(_frame(batch, "nn_int", b)[eq], s[idx[eq], 3])


def test_ragged_downsample_matches_prep_downsample(dev):
    rng = np.random.default_rng(6)
    n_out = 4096
    # equal counts: bit for bit the existing call
    B, N = 3, 9000
    pc = torch.from_numpy(rng.standard_normal((B, 3, N)).astype(np.float32)).to(dev)
    it = torch.from_numpy(rng.random((B, 1, N)).astype(np.float32)).to(dev)
    sn = torch.from_numpy(rng.standard_normal((B, 3, N)).astype(np.float32)).to(dev)
    off = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=dev)
    flat = lambda t: t.permute(0, 2, 1).reshape(B * N, -1).contiguous()
    for n in (n_out, 20_000):
        idx = scan_prep.random_choice_ragged(7, off, N, n)
        got = scan_prep.gather_ragged(flat(pc), flat(it).reshape(-1), flat(sn), off, idx)
        want = prep.downsample(pc, it, sn, n, 7)
        assert torch.equal(idx, want[3])
        for g, w in zip(got, want[:3]):
            assert torch.equal(g, w)
    # unequal counts: frame b follows prep.downsample's rule for its own count (checked against that call on b + 1 equal frames)
    counts = [9000, 1500, 0, 4096, 5000]
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
    idx = _np(scan_prep.random_choice_ragged(11, off, max(counts), n_out))
    for b, c in enumerate(counts):
        if c == 0:
            assert np.all(idx[b] == -1)
            continue
        z = torch.zeros((b + 1, 3, c), device=dev)
        want = prep.downsample(z, torch.zeros((b + 1, 1, c), device=dev), z, n_out, 11)[3][b]
        assert np.array_equal(idx[b], _np(want)), b
    # the fused rigid transform: points by [R|t], normals by R
    T = np.zeros((len(counts), 4, 4))
    for b in range(len(counts)):
        a = rng.uniform(-np.pi, np.pi)
        T[b, :3, :3] = synthetic.ry_matrix(a) @ np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]])
        T[b, :3, 3] = rng.uniform(-5, 5, 3)
        T[b, 3, 3] = 1
    tot = sum(counts)
    P = rng.standard_normal((tot, 3)).astype(np.float32) * 20
    S = rng.standard_normal((tot, 3)).astype(np.float32)
    I = rng.random(tot).astype(np.float32)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    idx_t = td(idx)
    pc, it, sn = scan_prep.gather_ragged(td(P), td(I), td(S), off, idx_t, td(T))
    pc, it, sn = _np(pc), _np(it), _np(sn)
    ho = _np(off)
    for b, c in enumerate(counts):
        if c == 0:
            assert np.all(pc[b] == 0) and np.all(it[b] == 0)
            continue
        g = ho[b] + idx[b]
        wp = T[b, :3, :3] @ P[g].T.astype(np.float64) + T[b, :3, 3:4]
        ws = T[b, :3, :3] @ S[g].T.astype(np.float64)
        assert np.allclose(pc[b], wp, rtol=2e-7, atol=1e-6) and np.allclose(sn[b], ws, rtol=2e-7, atol=1e-7)
        assert np.array_equal(it[b, 0], I[g])


def test_frame_alone_equals_frame_in_batch_and_runs_repeat(dev, batch):
    s = batch["scans"][3]
    recs = scan_prep.preprocess_velodyne([s], device=dev)
    recs2 = scan_prep.preprocess_velodyne(batch["scans"], device=dev)
    recs3 = scan_prep.preprocess_velodyne(batch["scans"], device=dev)
    assert torch.equal(recs[0], recs2[3])
    assert all(torch.equal(a, b) for a, b in zip(recs2, recs3))
    assert recs2[2].shape == (7, 0)
    # the record is the offline script's: points, intensity of the nearest raw point, normals
    r = _np(recs2[3])
    ref = batch["ref"][3]
    assert np.array_equal(r[0:3].T, ref["points"])
    assert np.array_equal(r[3], _frame(batch, "nn_int", 3))
    assert np.array_equal(r[4:7].T, _frame(batch, "normals", 3))


def test_rejected_frames_report_status(dev):
    s = synthetic.make_velodyne_scan(np.random.default_rng(30))
    points, offsets, _ = scan_prep.pack([s[:1000], s[:5000]], dev)
    st = scan_prep.voxel_down_sample(points, offsets, 0.1, max_frame_points=2000)
    assert list(_np(st.status)) == [0, 1]
    vo = _np(st.offsets)
    assert vo[2] == vo[1] > 0
    with pytest.raises(scan_prep.DeepI2PHipError, match="frame 1"):
        scan_prep.check_status(st.status)
    st = scan_prep.voxel_down_sample(points, offsets, 0.1, max_extent=1.0)
    assert np.all(_np(st.status) == 2)


def _records(dev):
    scans = _scans()
    return scans, scan_prep.preprocess_velodyne(scans, device=dev)


def test_prepare_batch_graph_replay_equals_eager(dev):
    scans, recs = _records(dev)
    points, normals, offsets, host = scan_prep.pack_records(recs, dev)
    counts = np.diff(host)
    plan = scan_prep.BatchPlan(len(recs), points.shape[0], int(counts.max()), 20480, 128)
    T = torch.eye(4, dtype=torch.float64, device=dev).repeat(len(recs), 1, 1)
    T[:, 0, 3] = 1.5
    eager = [t.clone() for t in scan_prep.prepare_batch_into(plan, points, normals, offsets, 5, T)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        scan_prep.prepare_batch_into(plan, points, normals, offsets, 5, T)        # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = scan_prep.prepare_batch_into(plan, points, normals, offsets, 5, T)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    # and prepare_batch (the eager front end) computes the same
    got = scan_prep.prepare_batch(recs, 20480, 128, seed=5, P=T)
    for a, b in zip(eager, got):
        assert torch.equal(a, b)
    assert np.all(_np(plan.status) == 0)


def test_prepare_batch_end_to_end(dev):
    from deepi2p_amd.networks import KeypointDetector
    from deepi2p_amd.registration import RegistrationPipeline
    scans = [synthetic.make_velodyne_scan(np.random.default_rng(40 + i)) for i in range(2)]
    N, H, W = 20480, 160, 512
    P = np.stack([np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)] * 2)     # velodyne -> camera axes
    pc, it, sn, na, nb = scan_prep.prepare_batch(scans, N, 128, seed=1, P=P, raw=True)
    assert pc.shape == (2, 3, N) and it.shape == (2, 1, N) and sn.shape == (2, 3, N) and na.shape == (2, 3, 128) and nb.shape == (2, 3, 128)
    for t in (pc, it, sn, na, nb):
        assert torch.isfinite(t).all()
    opt = synthetic.OptLike(N, H, W, True)
    det = KeypointDetector(opt)
    det.load_state_dict(synthetic.synthetic_state_dict(opt))
    det = det.to(dev).eval()
    img = torch.from_numpy(np.random.default_rng(0).uniform(0, 255, (2, 3, H, W)).astype(np.float32)).to(dev)
    coarse, fine = det.predict_labels(pc, it, sn, na, nb, img)
    assert coarse.shape == (2, N) and fine.shape == (2, N)
    pipe = RegistrationPipeline(H, W, R=8, seed=0)
    K = torch.from_numpy(np.stack([synthetic.make_K(H, W)] * 2)).to(dev)
    out = pipe(pc, coarse, K, pipe.draw(2, dev))
    assert torch.isfinite(out["cost"]).all()
