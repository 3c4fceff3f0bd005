"""GPU: csrc/map_index.hip against its numpy restatement (tests/map_index_oracle.py) with EXACT equality -- cell_start, order, sorted, rows,
offsets, index and status -- on the grid map of tests/map_cases.py: every up axis, an exact and a generic rotation, the three ways a frame
is rejected with the other frames bit-identical, run-to-run equality, a CropPlan replayed from a graph after its priors were overwritten in
place, the build refusing a capturing stream, and di2p_map_pose against fp64 numpy."""
import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, map_index
from deepi2p_amd._lib import DeepI2PHipError, ptr, stream
from tests import map_cases as mc
from tests import map_index_oracle as oracle

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def maps(dev):
    """up_axis -> (points, the oracle's index, the device's), built once and never modified"""
    out = {}
    for up in (0, 1, 2):
        p = mc.grid_map(up)
        out[up] = (p, oracle.build(p, mc.CELL, up, mc.ORIGIN, mc.NX, mc.NY),
                   map_index.MapIndex.build(p, mc.CELL, up, origin=mc.ORIGIN, shape=(mc.NX, mc.NY), device=dev))
    return out


def _crop_equals(index, ix, T, r, mfp, cap, max_cells):
    """the eager crop against the oracle, every output exactly -> the device outputs (numpy, up to the last row)"""
    rows, off, status, idx = index.crop(T, r, mfp, cap=cap, want_index=True, max_cells=max_cells)
    want = oracle.crop(ix, T, r, cap, mfp, max_cells)
    off = _np(off)
    n = int(off[-1])
    got = (_np(rows)[:n], off, _np(idx)[:n], _np(status))
    assert list(got[3]) == list(want[3]) and list(got[1]) == list(want[1])
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[2], want[2])
    return got


@pytest.mark.parametrize("up_axis", [0, 1, 2])
def test_build_and_crop_equal_the_oracle_on_every_up_axis(maps, up_axis):
    p, ix, index = maps[up_axis]
    assert (index.M, index.nx, index.ny, index.origin) == (len(p), mc.NX, mc.NY, mc.ORIGIN)
    assert np.array_equal(_np(index.cell_start), ix["cell_start"]) and np.array_equal(_np(index.order), ix["order"])
    assert _np(index.sorted).tobytes() == ix["sorted"].tobytes()
    T, r = mc.grid_frames(up_axis)
    rows, off, idx, status = _crop_equals(index, ix, T, r, len(p), 2 * len(p), mc.NX * mc.NY)
    assert list(status) == [0, 0, oracle.ST_EMPTY, oracle.ST_PRIOR] and off[2] - off[1] == len(p) and off[1] > 100


def test_build_with_its_own_origin(maps, dev):
    p, ix, _ = maps[1]
    index = map_index.MapIndex.build(torch.from_numpy(p).to(dev), mc.CELL, 1)
    assert (index.origin, index.nx, index.ny) == (mc.ORIGIN, mc.NX, mc.NY)
    assert np.array_equal(_np(index.cell_start), ix["cell_start"]) and np.array_equal(_np(index.order), ix["order"])
    with pytest.raises(DeepI2PHipError, match="outside"):
        map_index.MapIndex.build(p, mc.CELL, 1, origin=mc.ORIGIN, shape=(mc.NX - 1, mc.NY), device=dev)
    bad = p.copy()
    bad[17, 1] = np.inf          # the up coordinate: no cell depends on it, the row is refused all the same
    with pytest.raises(DeepI2PHipError, match="non-finite"):
        map_index.MapIndex.build(bad, mc.CELL, 1, origin=mc.ORIGIN, shape=(mc.NX, mc.NY), device=dev)


@pytest.mark.parametrize("kind", ["quarter", "generic"])
def test_rotated_priors(maps, kind):
    """a quarter turn keeps the transform exact: the rows equal R^T (p - t) computed any way; a generic rotation equals the stated order"""
    p, ix, index = maps[1]
    T, r = mc.grid_frames(1, kind)
    rows, off, idx, _ = _crop_equals(index, ix, T, r, len(p), 2 * len(p), mc.NX * mc.NY)
    if kind == "quarter":
        for f in (0, 1):
            sel = idx[off[f]:off[f + 1]]
            exact = (p[sel, :3].astype(np.float64) - T[f, :3, 3]) @ T[f, :3, :3]
            assert np.array_equal(rows[off[f]:off[f + 1], :3], exact.astype(np.float32))


def test_keep_rule_is_strict(maps):
    p, ix, index = maps[1]
    T = mc.prior((0.0, 0.0), 1)[None]
    _, off, idx, status = _crop_equals(index, ix, T, np.array([5.0]), len(p), len(p), 20)
    kept = p[idx][:, [0, 2]]
    assert status[0] == 0 and not np.all(kept == np.float32(mc.ON_CIRCLE), axis=1).any()
    assert np.all(kept == np.float32(mc.INSIDE_CIRCLE), axis=1).sum() == 1


def test_rejected_frames_leave_the_others_bit_identical(maps):
    """a frame over max_frame_points, too small a cap, too small a max_cells: status 1 for that frame, the frame before it as it was"""
    p, ix, index = maps[1]
    T, r = mc.grid_frames(1)
    cells = mc.NX * mc.NY
    full = _crop_equals(index, ix, T, r, len(p), 2 * len(p), cells)
    n0 = int(full[1][1])
    for mfp, cap, max_cells in ((len(p) - 1, 2 * len(p), cells), (len(p), n0 + len(p) - 1, cells), (len(p), 2 * len(p), cells - 1)):
        got = _crop_equals(index, ix, T, r, mfp, cap, max_cells)
        assert list(got[3]) == [0, 1, 4, 5] and list(got[1]) == [0, n0, n0, n0, n0]
        assert got[0].tobytes() == full[0][:n0].tobytes() and np.array_equal(got[2], full[2][:n0])
    # the wide frame first: the frame behind a rejected one starts where it would have started
    got = _crop_equals(index, ix, T[[1, 0]], r[[1, 0]], len(p) - 1, 2 * len(p), cells)
    assert list(got[3]) == [1, 0] and got[0].tobytes() == full[0][:n0].tobytes()
    # exactly at both limits nothing is rejected
    got = _crop_equals(index, ix, T, r, len(p), n0 + len(p), cells)
    assert list(got[3]) == [0, 0, 4, 5]


def test_two_runs_are_equal(maps):
    p, ix, index = maps[1]
    T, r = mc.grid_frames(1, "generic")
    a = index.crop(T, r, len(p), want_index=True)
    b = index.crop(T, r, len(p), want_index=True)
    n = int(a[1][-1])
    assert n > len(p) and all(_np(x)[:n].tobytes() == _np(y)[:n].tobytes() for x, y in ((a[0], b[0]), (a[3], b[3])))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_crop_plan_replayed_from_a_graph_reads_the_priors_in_place(maps, dev):
    p, ix, index = maps[1]
    T0, r0 = mc.grid_frames(1)
    T1, r1 = mc.grid_frames(1, "generic")
    T1, r1 = T1[[1, 3, 0, 2]], r0[[1, 3, 0, 2]]
    plan = map_index.CropPlan(index, 4, 2 * len(p), len(p), 40.0, want_index=True)
    assert plan.max_cells == mc.NX * mc.NY
    T, r = torch.from_numpy(T0).to(dev), torch.from_numpy(r0).to(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        plan.run(T, r)          # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.run(T, r)
    for Th, rh in ((T1, r1), (T0, r0)):
        T.copy_(torch.from_numpy(Th))
        r.copy_(torch.from_numpy(rh))
        plan.rows.fill_(float("nan"))
        plan.offsets.fill_(-1)
        g.replay()
        want = oracle.crop(ix, Th, rh, plan.cap, len(p), plan.max_cells)
        n = int(want[1][-1])
        assert list(_np(plan.offsets)) == list(want[1]) and list(_np(plan.status)) == list(want[3])
        assert _np(plan.rows)[:n].tobytes() == want[0].tobytes() and np.array_equal(_np(plan.index)[:n], want[2])
        eager = index.crop(Th, rh, len(p), cap=plan.cap)
        assert _np(eager[0])[:n].tobytes() == _np(plan.rows)[:n].tobytes()


def test_build_refuses_a_capturing_stream(maps, dev):
    """di2p_map_index_build returns its error with nothing enqueued; the capture goes on and its graph replays"""
    p, ix, index = maps[1]
    lib = _lib.load()
    pts = torch.from_numpy(p).to(dev)
    M, ncell = len(p), mc.NX * mc.NY
    cell_start = torch.zeros((ncell + 1,), dtype=torch.int32, device=dev)
    order = torch.zeros((M,), dtype=torch.int32, device=dev)
    rows = torch.zeros((M, 4), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.di2p_map_index_workspace_bytes(M, ncell),), dtype=torch.uint8, device=dev)
    x = torch.zeros((8,), device=dev)
    args = lambda: (ptr(pts), M, 1, mc.ORIGIN[0], mc.ORIGIN[1], mc.CELL, mc.NX, mc.NY, ptr(cell_start), ptr(order), ptr(rows), ptr(status), ptr(ws),
                    stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x.add_(1.0)
        rc = lib.di2p_map_index_build(*args())
        x.add_(1.0)
    assert rc != 0 and b"capturing" in lib.di2p_last_error()
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 2.0 and int(order.abs().sum()) == 0          # the capture recorded both adds and nothing of the build
    assert lib.di2p_map_index_build(*args()) == 0                       # and the same call outside a capture builds the index
    assert np.array_equal(_np(order), ix["order"]) and int(status.item()) == 0


def _pose_bound(A, P):
    """di2p_map_pose and the numpy reference both compute sum_k A_ik M_kj with M = [R^T | -R^T t]: a dot product of four terms whose last
    column is itself a dot product of three.  Each side is within gamma_7 sum_k |A_ik| Mabs_kj of the exact entry, Mabs = [|R^T| | |R^T| |t|]
    (gamma_n = n u / (1 - n u), u = 2^-53: any summation order, fused or not), so the two differ by at most twice that.  Built like
    _p_scan_bound of tests/test_gpu_raw_frames.py."""
    u = 2.0 ** -53
    Mabs = np.zeros_like(P)
    Mabs[:, :3, :3] = np.abs(P[:, :3, :3].transpose(0, 2, 1))
    Mabs[:, :3, 3] = np.einsum("nij,nj->ni", Mabs[:, :3, :3], np.abs(P[:, :3, 3]))
    Mabs[:, 3, 3] = 1.0
    return 2.0 * (7 * u / (1 - 7 * u)) * (np.abs(A) @ Mabs)


def rigid_inverse(P):
    M = np.tile(np.eye(4), (len(P), 1, 1))
    M[:, :3, :3] = P[:, :3, :3].transpose(0, 2, 1)
    M[:, :3, 3] = -np.einsum("nij,nj->ni", M[:, :3, :3], P[:, :3, 3])
    return M


def test_map_pose_against_fp64_numpy(dev):
    rng = np.random.default_rng(4)
    n = 70          # more than one 64-thread workgroup
    A = np.stack([mc.prior(rng.uniform(-500, 500, 2), 1, mc.rotation("generic", 1, s), rng.uniform(-2, 2)) for s in range(n)])
    P = np.stack([mc.prior(rng.uniform(-5, 5, 2), 1, mc.rotation("generic", 1, 100 + s), rng.uniform(-2, 2)) for s in range(n)])
    got = _np(map_index.map_pose(torch.from_numpy(A).to(dev), torch.from_numpy(P).to(dev)))
    assert got.tobytes() == oracle.pose(A, P).tobytes()
    diff = np.abs(got - A @ rigid_inverse(P))
    print("map_pose: largest |T_map_cam - T_map_prior @ inv(P_scan)| = %.3e" % diff.max())
    assert np.all(diff <= _pose_bound(A, P))
    assert np.abs(got @ P - A).max() < 1e-9                              # and it IS the inverse: T_map_cam . P_scan = T_map_prior
    same = torch.from_numpy(A).to(dev)
    map_index.map_pose(same, torch.from_numpy(P).to(dev), out=same)      # in place
    assert _np(same).tobytes() == got.tobytes()
