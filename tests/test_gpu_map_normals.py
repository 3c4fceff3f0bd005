"""GPU: the normals of a map (csrc/map_normals.hip) against the brute-force oracle (tests/map_normals_oracle.py) on the map of
tests/map_normals_cases.py -- neighbour counts and lists EXACTLY, the normals by the rule of test_normals_against_oracle (DESIGN.md
section 6) -- for every up axis and orientation, on a translated grid, and bit for bit against scan_prep.estimate_normals on the same points;
di2p_map_crop_normals bit for bit against its restatement, with rejected frames, from a replayed graph; and MapRawPlan(dataset="kitti")
against CropPlan(want_normals=True) followed by sample_prep.SamplePlan(dataset="kitti")."""
import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, map_index, sample_prep, scan_prep, synthetic
from deepi2p_amd._lib import DeepI2PHipError, ptr, stream
from tests import map_cases as mc
from tests import map_index_oracle as index_oracle
from tests import map_normals_cases as cases
from tests import map_normals_oracle as oracle

pytestmark = pytest.mark.gpu
N, H, W = 2048, 64, 128
KITTI_RAW_HW = (180, 256)          # the KITTI loader cuts 50 rows off the top and halves: 65 x 128 for a 64 x 128 window


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


@pytest.fixture(scope="module")
def ref():
    return cases.reference()


# ---------------------------------------------------------------------------------------------------------------- di2p_map_normals
@pytest.mark.parametrize("up_axis,orient", [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)])
def test_normals_against_the_oracle(dev, ref, up_axis, orient):
    p, cnt, idx = ref["points"], ref["cnt"], ref["idx"]
    n, got_cnt, got_idx = map_index.estimate_normals(p, cases.RADIUS, cases.MAX_NN, up_axis, orient, want_neighbors=True, device=dev)
    assert n.shape == (len(p), 3) and n.dtype == torch.float32
    assert np.array_equal(_np(got_cnt), cnt)
    wrong = np.nonzero(np.any(_np(got_idx) != idx, axis=1))[0]
    assert len(wrong) == 0, (len(wrong), wrong[:5], int(ref["tie"][wrong].sum()))          # the lists do not depend on the axis: exact, ties included
    nref, lam = oracle.normals(p, cnt, idx, up_axis, orient)
    n = _np(n).astype(np.float64)
    well = oracle.well_conditioned(cnt, lam)
    dots = np.abs(np.sum(n * nref, 1))
    print("up %d orient %+d: %d well-conditioned rows, smallest |n . n_ref| = 1 - %.3e" % (up_axis, orient, well.sum(), 1 - dots[well].min()))
    assert np.all(dots[well] >= 1 - 1e-7), dots[well].min()
    sure = np.abs(nref[:, up_axis]) > 1e-6
    assert np.all(orient * n[sure, up_axis] >= 0)
    e = np.zeros(3)
    e[up_axis] = orient
    assert (cnt < 3).sum() >= 4 and np.all(n[cnt < 3] == e)
    alone = map_index.estimate_normals(p, cases.RADIUS, cases.MAX_NN, up_axis, orient, device=dev)          # without the lists: the same normals
    assert _np(alone).astype(np.float64).tobytes() == n.tobytes()


def test_the_lists_do_not_depend_on_where_the_grid_lands(dev, ref):
    p = ref["points"].copy()
    p[:, :3] += cases.SHIFT.astype(np.float32)          # exact: every difference of two rows is what it was
    _, cnt, idx = map_index.estimate_normals(p, cases.RADIUS, cases.MAX_NN, want_neighbors=True, device=dev)
    assert np.array_equal(_np(cnt), ref["cnt"]) and np.array_equal(_np(idx), ref["idx"])


@pytest.mark.parametrize("method", ["query", "cells"])
def test_one_implementation_with_scan_prep(dev, method):
    """a scan whose points are voxels of their own: the frame's centroids are the points, so both front ends select among the same
    positions with the same indices, and the shared selection and tail give the same bits"""
    scan = cases.lattice_scan()
    points, offsets, _ = scan_prep.pack([scan], dev)
    st = scan_prep.voxel_down_sample(points, offsets, 2.0 ** -7)
    n = int(st.offsets[1])
    assert n == len(scan) > 3000 and int(st.status[0]) == 0
    assert sorted(map(tuple, _np(st.points[:n]))) == sorted(map(tuple, scan[:, :3]))
    want = scan_prep.estimate_normals(st, cases.RADIUS, cases.MAX_NN, want_neighbors=True, method=method)
    as_map = torch.cat([st.points[:n], torch.zeros((n, 1), device=dev)], 1).contiguous()
    got = map_index.estimate_normals(as_map, cases.RADIUS, cases.MAX_NN, up_axis=2, orient=1, want_neighbors=True)
    for name, a, b in zip(("normals", "nn_count", "nn_idx"), got, want):
        assert _same(a, b[:n].contiguous()), name
    assert int(got[1].max()) == cases.MAX_NN and int(got[1].min()) < cases.MAX_NN


def test_status_and_a_capturing_stream(dev, ref):
    p = ref["points"].copy()
    bad = p.copy()
    bad[123, 2] = np.nan
    with pytest.raises(DeepI2PHipError, match="non-finite"):
        map_index.estimate_normals(bad, device=dev)
    wide = p.copy()
    wide[5, 0] = 3.0e6          # at radius 0.6 an edge of 3000 km is more than 2^21 - 4 cells
    with pytest.raises(DeepI2PHipError, match="bounds"):
        map_index.estimate_normals(wide, device=dev)
    lib = _lib.load()
    pts = torch.from_numpy(p).to(dev)
    M = len(p)
    normals = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.di2p_map_normals_workspace_bytes(M),), dtype=torch.uint8, device=dev)
    assert lib.di2p_map_normals_workspace_bytes(0) == 0 and lib.di2p_map_normals_workspace_bytes((1 << 27) + 1) == 0
    x = torch.zeros((8,), device=dev)
    args = lambda: (ptr(pts), M, 2, 1, cases.RADIUS, cases.MAX_NN, ptr(normals), None, None, ptr(status), ptr(ws), stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x.add_(1.0)
        rc = lib.di2p_map_normals(*args())
        x.add_(1.0)
    assert rc != 0 and b"capturing" in lib.di2p_last_error()
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 2.0 and float(normals.abs().sum()) == 0.0          # the capture recorded both adds and nothing of the normals
    assert lib.di2p_map_normals(*args()) == 0 and int(status.item()) == 0
    assert _same(normals, map_index.estimate_normals(p, device=dev))


# ---------------------------------------------------------------------------------------------------------------- di2p_map_crop_normals
SENTINEL = 7.25


@pytest.fixture(scope="module")
def maps(dev):
    """up_axis -> (points, arbitrary float32 normals, the oracle's index, the device's index carrying those normals)"""
    out = {}
    for up in (0, 1, 2):
        p = mc.grid_map(up)
        nm = np.random.default_rng(40 + up).standard_normal((len(p), 3)).astype(np.float32)
        index = map_index.MapIndex.build(p, mc.CELL, up, origin=mc.ORIGIN, shape=(mc.NX, mc.NY), device=dev, normals=nm)
        assert _np(index.normals).tobytes() == nm.tobytes()          # stored as given, in map-row order
        out[up] = (p, nm, index_oracle.build(p, mc.CELL, up, mc.ORIGIN, mc.NX, mc.NY), index)
    return out


def _check_plan(plan, ix, nm, T, r):
    """the plan's buffers after a run against the two oracles; rows past offsets[B] hold the sentinel"""
    want = index_oracle.crop(ix, T, r, plan.cap, plan.max_src, plan.max_cells)
    n = int(want[1][-1])
    assert list(_np(plan.offsets)) == list(want[1]) and list(_np(plan.status)) == list(want[3])
    assert _np(plan.rows)[:n].tobytes() == want[0].tobytes() and np.array_equal(_np(plan.index)[:n], want[2])
    got = _np(plan.normals)
    assert got[:n].tobytes() == oracle.crop_normals(nm, want[2], want[1], T).tobytes()
    assert np.all(got[n:] == SENTINEL) and len(got) > n
    return n


@pytest.mark.parametrize("up_axis", [0, 1, 2])
@pytest.mark.parametrize("kind", ["identity", "quarter", "generic"])
def test_crop_normals_equal_the_oracle(dev, maps, up_axis, kind):
    p, nm, ix, index = maps[up_axis]
    T, r = mc.grid_frames(up_axis, kind)          # frames 2 and 3 are rejected (off the grid, a NaN prior): they have no rows
    plan = map_index.CropPlan(index, 4, 2 * len(p), len(p), 40.0, want_normals=True)
    plan.normals.fill_(SENTINEL)
    out = plan.run(torch.from_numpy(T).to(dev), torch.from_numpy(r).to(dev))
    assert len(out) == 3
    n = _check_plan(plan, ix, nm, T, r)
    assert n > len(p) and list(_np(plan.status)) == [0, 0, 4, 5]
    if kind != "generic":          # an exact rotation: R^T n computed any way
        off = _np(plan.offsets)
        for f in (0, 1):
            sel = _np(plan.index)[off[f]:off[f + 1]]
            assert np.array_equal(_np(plan.normals)[off[f]:off[f + 1]], (nm[sel].astype(np.float64) @ T[f, :3, :3]).astype(np.float32))
    eager = index.crop(T, r, len(p), cap=plan.cap, want_index=True, want_normals=True)
    assert len(eager) == 5 and _np(eager[4])[:n].tobytes() == _np(plan.normals)[:n].tobytes() and np.all(_np(eager[4])[n:] == 0)


def test_crop_without_normals_is_unchanged(dev, maps):
    p, nm, ix, index = maps[1]
    plain = map_index.MapIndex.build(p, mc.CELL, 1, origin=mc.ORIGIN, shape=(mc.NX, mc.NY), device=dev)
    assert plain.normals is None
    T, r = mc.grid_frames(1, "generic")
    a, b = index.crop(T, r, len(p), want_index=True), plain.crop(T, r, len(p), want_index=True)
    n = int(a[1][-1])
    assert len(a) == len(b) == 4 and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert _np(a[0])[:n].tobytes() == _np(b[0])[:n].tobytes() and np.array_equal(_np(a[3])[:n], _np(b[3])[:n])
    want = index_oracle.crop(ix, T, r, 4 * len(p), len(p), mc.NX * mc.NY)
    assert _np(a[0])[:n].tobytes() == want[0].tobytes()
    assert map_index.CropPlan(index, 4, 100, 50, 5.0).normals is None
    with pytest.raises(ValueError, match="want_normals"):
        plain.crop(T, r, len(p), want_normals=True)


def test_crop_normals_replayed_from_a_graph_follow_the_priors(dev, maps):
    p, nm, ix, index = maps[1]
    T0, r0 = mc.grid_frames(1)
    T1, _ = mc.grid_frames(1, "generic")
    T1, r1 = T1[[1, 3, 0, 2]], r0[[1, 3, 0, 2]]
    plan = map_index.CropPlan(index, 4, 2 * len(p), len(p), 40.0, want_normals=True)
    T, r = torch.from_numpy(T0).to(dev), torch.from_numpy(r0).to(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        plan.run(T, r)          # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.run(T, r)
    seen = []
    for Th, rh in ((T1, r1), (T0, r0)):
        T.copy_(torch.from_numpy(Th))
        r.copy_(torch.from_numpy(rh))
        plan.normals.fill_(SENTINEL)
        plan.offsets.fill_(-1)
        g.replay()
        n = _check_plan(plan, ix, nm, Th, rh)
        seen.append(_np(plan.normals)[:n].copy())
    assert seen[0].tobytes() != seen[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- MapRawPlan(dataset="kitti")
def test_kitti_raw_plan_equals_the_crop_and_the_sample_stage(dev):
    world = mc.street()
    index = map_index.MapIndex.build(world["points"], mc.STREET_CELL, up_axis=1, device=dev, normals=True)
    nm = _np(index.normals)
    assert nm.shape == (mc.STREET_ROWS, 3) and np.all(nm[:, 1] <= 0)          # a camera-convention map: the normals point up, -y
    own = map_index.estimate_normals(world["points"], up_axis=1, orient=-1, device=dev)
    assert _same(index.normals, own)
    B, mode, opt = mc.STREET_B, "val_random_Ry", synthetic.OptLike(N, H, W, False)
    hb = mc.street_batches(world)[1]
    rng = np.random.default_rng(8)
    images = torch.from_numpy(np.stack([synthetic.make_camera_image(rng, *KITTI_RAW_HW) for _ in range(B)])).to(dev)
    K_raw = torch.from_numpy(np.tile(np.array([[200.0, 0, 128.3], [0, 200.0, 89.3], [0, 0, 1]]), (B, 1, 1))).to(dev)
    T = torch.from_numpy(np.ascontiguousarray(hb["T_map_prior"])).to(dev)
    r = torch.from_numpy(np.asarray(hb["radius"], np.float64)).to(dev)
    P_cam_pc = torch.from_numpy(np.linalg.inv(hb["T_map_cam_gt"]) @ hb["T_map_prior"]).to(dev)
    plan = map_index.MapRawPlan(index, opt, B, mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS, KITTI_RAW_HW, mode, dataset="kitti")
    got = [t.clone() for t in plan.run(T, r, images, K_raw, P_cam_pc, seed=31)]
    assert len(got) == 11 and list(_np(got[9])) == [0, 0]
    crop = map_index.CropPlan(index, B, mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS, want_normals=True)
    rows, offsets, _ = crop.run(T, r)
    assert int(offsets[-1]) > 2 * 2 * N          # both frames go through the loader's 0.3 m voxel pass
    sample = sample_prep.SamplePlan(opt, B, mc.STREET_CAP, mc.STREET_MFP, KITTI_RAW_HW, mode, dev, dataset="kitti")
    want = sample.run(rows, crop.normals, offsets, images, K_raw, P_cam_pc, seed=31)
    for name, a, b in zip(sample_prep.PREPARED[:9], got, want):
        assert _same(a, b), name
    sn = _np(got[2])
    assert sn.shape == (B, 3, N) and np.all(np.abs(sn).sum(1) > 0)          # every point has a normal
    assert _same(got[10], sample.table.Pr[:B])
    conv = map_index.prepare_map_raw(index, hb["T_map_prior"], hb["radius"], images.cpu(), K_raw.cpu(), P_cam_pc.cpu(), opt, mc.STREET_MFP, mode,
                                     seed=31, dataset="kitti")
    for name, a, b in zip(sample_prep.PREPARED[:9], conv, want):
        assert _same(a, b), name
