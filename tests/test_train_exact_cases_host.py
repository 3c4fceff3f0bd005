"""CPU: the premises of tests/test_gpu_train_exact.py.  For every case of tests/train_exact_cases.py: the sum of absolute products of every
output is at most 2^24 (so any fp32 evaluation in any order is exact), the operands are non-zero where losing them must show, the one-hot
operands of family ID cover the critical set of the chunk plan, the references agree with torch's own fp64 autograd, and -- through the
library's routing query (di2p_rc_route / di2p_rc_vec_ok, host code) -- the tables reach every kernel instance, tile, reduction width and
chunk-plan edge, and the query reproduces the workspace sizes the library asks for."""
import collections
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import train_exact_cases as tc

FAKE_BASE = 1 << 20          # the alignment of a fresh device allocation (at least 256 bytes)


def _vec_ok(placed, R):
    from deepi2p_amd import ops
    return ops.rc_vec_ok(FAKE_BASE + 4 * placed.offset, placed.ld, placed.batch_stride, R)


def rc_route_of(c, case):
    from deepi2p_amd import _lib, ops
    with _lib.option("rc_tile64", c.tile64):
        return ops.rc_route("strided", c.Z, c.rows, c.cols, c.R, _vec_ok(case["pa"], c.R), _vec_ok(case["pb"], c.R))


def instance_of(rt):
    if rt["tile"] == 128:
        return "rc_gemm_kernel<128,true,true>"
    return "rc_gemm_kernel<64,%s,%s>" % ("true" if rt["a_stager"] else "false", "true" if rt["b_stager"] else "false")


def _bounded(absum, what):
    assert float(absum.max()) <= tc.LIMIT, (what, float(absum.max()))


def _integers(*tensors):
    return all(bool((t == t.round()).all()) for t in tensors if t is not None)


# ------------------------------------------------------------------------------------------------ the routing query itself
def test_route_query_is_the_launchers_decision():
    from deepi2p_amd import _lib, ops
    lib = _lib.load()
    assert ops.rc_vec_ok(FAKE_BASE, 36, 36 * 5, 36) and ops.rc_vec_ok(FAKE_BASE, 40, 40 * 5 + 4, 36)
    for bad in ((FAKE_BASE + 4, 36, 180, 36), (FAKE_BASE, 37, 185, 36), (FAKE_BASE, 36, 181, 36), (FAKE_BASE, 33, 165, 33), (FAKE_BASE, 28, 140, 28)):
        assert not ops.rc_vec_ok(*bad), bad
    # a strided pair takes the 16-byte stagers together or not at all; the 128-row tile needs them, 128 rows and columns, and the knob off
    assert ops.rc_route("strided", 1, 130, 129, 36, True, True) == dict(tile=128, a_stager=1, b_stager=1, rch=64, chunks=1)
    assert ops.rc_route("strided", 1, 130, 129, 36, True, False) == dict(tile=64, a_stager=0, b_stager=0, rch=64, chunks=1)
    assert ops.rc_route("strided", 1, 130, 127, 36, True, True)["tile"] == 64
    with _lib.option("rc_tile64", 1):
        assert ops.rc_route("strided", 1, 130, 129, 36, True, True) == dict(tile=64, a_stager=1, b_stager=1, rch=64, chunks=1)
    assert ops.rc_route("wgrad", 3, 65, 63, 576, True, True) == dict(tile=64, a_stager=1, b_stager=0, rch=288, chunks=2)
    assert ops.rc_route("wgrad", 3, 255, 255, 576, False, False)["a_stager"] == 0
    assert ops.rc_route("gather", 3, 255, 255, 2305, True, True) == dict(tile=64, a_stager=0, b_stager=0, rch=288, chunks=9)
    # the chunk plans the issue names: last chunks of 1, 4 and 34 indices, and a plan that collapses from ten chunks to nine
    for R, chunks, last in ((2305, 9, 1), (2308, 9, 4), (2050, 8, 34), (2592, 9, 288)):
        rt = ops.rc_route("strided", 1, 5, 5, R)
        assert (rt["rch"], rt["chunks"], R - (rt["chunks"] - 1) * rt["rch"]) == (288, chunks, last), (R, rt)
    assert 2592 // 256 == 10

    def refused():          # in a thread of its own: di2p_last_error is per thread
        out = (ctypes.c_int32 * 5)()
        for args in ((3, 1, 1, 1, 1, 0, 0), (0, 0, 1, 1, 1, 0, 0), (0, 1, 1, 1, 0, 0, 0)):
            assert lib.di2p_rc_route(*args, out) != 0
        with pytest.raises(_lib.DeepI2PHipError, match="di2p_rc_route: bad args"):
            ops.rc_route("strided", 1, 0, 1, 1)
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(1) as ex:
        ex.submit(refused).result()


# ------------------------------------------------------------------------------------------------ di2p_bmm_rc
def test_rc_table_lists_every_edge_of_the_issue():
    cs = tc.RC_CASES
    assert len(cs) == len(set(cs))
    assert {c.Z for c in cs} == {1, 3} and {c.reduce_z for c in cs} == {0, 1} and {c.alpha for c in cs} == set(tc.ALPHAS)
    assert {c.rows for c in cs} >= set(tc.RC_DIMS) and {c.cols for c in cs} >= set(tc.RC_DIMS)
    assert {c.R for c in cs} == set(tc.RC_R) | set(tc.RC_R_EXTRA)
    for lay in ("ld4", "ld1", "off1", "bs4", "bs1"):
        for Z in {3}:          # (a batch stride only shows with more than one batch)
            assert any(c.layA == lay and c.layB == "c" and c.Z == Z for c in cs), lay
            assert any(c.layA == "c" and c.layB == lay and c.Z == Z for c in cs), lay
            assert any(c.layA == lay and c.layB == lay and c.Z == Z for c in cs), lay
    for fam in ("IDA", "IDB"):
        for c in cs:
            if c.family == fam:
                assert (c.cols if fam == "IDA" else c.rows) >= 40 and c.alpha == 1.0, c
    # every big case (128 x 128 tiles) runs again on 64 x 64 tiles
    routes = {c: rc_route_of(c, tc.rc_case(c)) for c in cs}
    big = [c for c in cs if routes[c]["tile"] == 128]
    assert len(big) >= 8
    for c in big:
        twin = c._replace(tile64=1)
        assert c.tile64 == 0 and twin in routes and routes[twin]["tile"] == 64 and routes[twin]["a_stager"] == routes[twin]["b_stager"] == 1, c
        assert min(c.rows, c.cols) >= 128


def test_rc_table_reaches_every_instance_and_plan_edge():
    from deepi2p_amd import _lib
    lib = _lib.load()
    seen, per_group, last, per_family = collections.Counter(), set(), set(), collections.defaultdict(set)
    for c in tc.RC_CASES:
        case = tc.rc_case(c)
        rt = rc_route_of(c, case)
        seen[instance_of(rt)] += 1
        per_family[c.family].add(instance_of(rt))
        per_group.add(rt["chunks"] * (c.Z if c.reduce_z else 1))
        last.add(c.R - (rt["chunks"] - 1) * rt["rch"])
        assert 0 < c.R - (rt["chunks"] - 1) * rt["rch"] <= rt["rch"] and rt["rch"] % tc.RC_BK == 0
        # the workspace the call needs is within what the library tells its callers to allocate, and is exactly that on its own tile
        need = c.Z * rt["chunks"] * c.rows * c.cols * 4
        assert need <= lib.di2p_bmm_rc_workspace_bytes(c.Z, c.rows, c.cols, c.R), c
        from deepi2p_amd import ops
        with _lib.option("rc_tile64", 0):
            both = [ops.rc_route("strided", c.Z, c.rows, c.cols, c.R, v, v) for v in (False, True)]
        assert lib.di2p_bmm_rc_workspace_bytes(c.Z, c.rows, c.cols, c.R) == max(c.Z * r["chunks"] * c.rows * c.cols * 4 for r in both), c
    print("di2p_bmm_rc cases per kernel instance:", dict(seen))
    assert set(seen) == {"rc_gemm_kernel<64,false,false>", "rc_gemm_kernel<64,true,true>", "rc_gemm_kernel<128,true,true>"}
    for fam in ("S", "IDA", "IDB"):
        assert per_family[fam] == set(seen), fam
    assert per_group >= {1, 7, 8, 9, 17} and last >= {1, 4, 34}


@pytest.mark.parametrize("c", tc.RC_CASES, ids=tc.rc_id)
def test_rc_case_is_exact_and_sensitive(c):
    case = tc.rc_case(c)
    A, B = case["A"], case["B"]
    assert A.shape == (c.Z, c.rows, c.R) and B.shape == (c.Z, c.cols, c.R) and _integers(A, B)
    _bounded(case["absum"] * max(1.0, abs(c.alpha)), c)
    assert case["ref"].shape == ((c.rows, c.cols) if c.reduce_z else (c.Z, c.rows, c.cols))
    assert torch.equal(case["ref"].float().double(), case["ref"])                  # the reference is an fp32 number
    # the placed operands: the values where they belong, NaN everywhere else
    for t, p, n in ((A, case["pa"], c.rows), (B, case["pb"], c.cols)):
        assert torch.equal(tc.unplace(p, c.Z, n, c.R), t)
        assert int((p.buf == p.buf).sum()) == t.numel() and p.ld >= c.R and p.batch_stride >= n * p.ld
        assert p.offset >= 2 * p.ld and p.buf.numel() - (p.offset + c.Z * p.batch_stride) >= 2 * p.ld
    rt = rc_route_of(c, case)
    if c.family == "S":
        for t in (A, B):
            assert bool((t[:, :, -1] != 0).all()) and bool((t[:, -1, :] != 0).all()), c
    else:
        coded, hot = (A, B) if c.family == "IDA" else (B, A)
        assert coded.unique().numel() == coded.numel() and float(coded.min()) == 1.0
        assert bool((hot.sum(2) == 1).all()) and bool(((hot == 0) | (hot == 1)).all())
        crit = tc.critical_set(c.R, rt["rch"], rt["chunks"])
        assert {0, c.R - 1} <= set(crit) and all(b in crit for ch in range(1, rt["chunks"]) for b in (ch * rt["rch"] - 1, ch * rt["rch"]))
        last_begin = (rt["chunks"] - 1) * rt["rch"]
        assert last_begin + (c.R - 1 - last_begin) // tc.RC_BK * tc.RC_BK in crit          # the first index of the last K-step
        for z in range(c.Z):
            assert set(crit) <= set(hot[z].argmax(1).tolist()), (c, z)
        # the output is the id of the element read
        if not c.reduce_z:
            idx = tc.first_mismatch(torch.zeros_like(case["ref"]), case["ref"])          # the first non-zero output
            assert tc.decode(float(case["ref"][idx]), tuple(coded.shape)) is not None


# ------------------------------------------------------------------------------------------------ di2p_bmm_km
def test_km_table_lists_every_edge_of_the_issue():
    cs = tc.KM_CASES
    assert {c.Z for c in cs} == {1, 3} and {c.alpha for c in cs} == set(tc.ALPHAS) and {c.K for c in cs} == set(tc.KM_K)
    assert {c.rows for c in cs} == set(tc.KM_DIMS) and {c.cols for c in cs} == set(tc.KM_DIMS)
    assert any(c.dlda > 0 for c in cs) and any(c.dldb > 0 for c in cs) and any(c.bpad > 0 and c.Z == 3 for c in cs)
    assert {c.family for c in cs} == {"S", "IDA", "IDB"}


@pytest.mark.parametrize("c", tc.KM_CASES, ids=tc.km_id)
def test_km_case_is_exact_and_sensitive(c):
    case = tc.km_case(c)
    A, B = case["A"], case["B"]
    assert A.shape == (c.Z, c.K, c.rows) and B.shape == (c.Z, c.K, c.cols) and _integers(A, B)
    _bounded(case["absum"] * max(1.0, abs(c.alpha)), c)
    assert torch.equal(tc.unplace(case["pa"], c.Z, c.K, c.rows), A) and torch.equal(tc.unplace(case["pb"], c.Z, c.K, c.cols), B)
    assert case["pa"].ld == c.rows + c.dlda and case["pb"].ld == c.cols + c.dldb
    if c.family == "S":
        for t in (A, B):
            assert bool((t[:, -1, :] != 0).all()) and bool((t[:, :, -1] != 0).all())
    else:
        coded, hot = (A, B) if c.family == "IDA" else (B, A)
        assert coded.unique().numel() == coded.numel() and bool((hot.sum(1) == 1).all())
        for z in range(c.Z):
            assert set(hot[z].argmax(0).tolist()) == set(range(c.K)), c          # every k is somebody's one-hot position


# ------------------------------------------------------------------------------------------------ convolutions
def _conv_grid_is_complete(cases):
    combos = {((c.KH, c.KW), c.stride, c.pad) for c in cases}
    assert combos >= {(f, s, p) for f in tc.FILTERS for s in tc.STRIDES for p in tc.PADS}
    assert {c.B for c in cases} == {1, 3}
    assert any(tc.uncovered(c) for c in cases) and any(c.pad > max(c.KH, c.KW) // 2 for c in cases)
    assert any(c.H * c.W == 1 for c in cases) and any(c.KH != c.KW for c in cases)


def test_wgrad_table_reaches_every_instance_and_edge():
    from deepi2p_amd import _lib, ops
    lib = _lib.load()
    cs = tc.WGRAD_CASES
    _conv_grid_is_complete(cs)
    seen = collections.Counter()
    spatial, chunks = set(), set()
    for c in cs:
        OH, OW = tc.conv_out(c)
        R, rows, cols = OH * OW, c.Cout, c.Cin * c.KH * c.KW
        rt = ops.rc_route("wgrad", c.B, rows, cols, R, ops.rc_vec_ok(FAKE_BASE, R, rows * R, R))
        seen[instance_of(rt)] += 1
        spatial.add(R)
        chunks.add(rt["chunks"])
        assert lib.di2p_conv2d_wgrad_workspace_bytes(c.B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW, c.stride, c.pad) == c.B * rt["chunks"] * rows * cols * 4, c
    # a filter that does not fit the padded input has no output, at any stride (C's division truncates toward zero: (2 - 3) / 2 + 1 == 1)
    for stride in (1, 2, 3):
        assert lib.di2p_conv2d_wgrad_workspace_bytes(1, 3, 2, 2, 5, 3, 3, stride, 0) == 0
        assert lib.di2p_conv2d_wgrad_workspace_bytes(1, 3, 9, 2, 5, 3, 3, stride, 0) == 0
    assert lib.di2p_conv2d_wgrad_workspace_bytes(1, 3, 3, 3, 5, 3, 3, 2, 0) == 5 * 27 * 4
    print("di2p_conv2d_wgrad cases per kernel instance:", dict(seen))
    assert set(seen) == {"rc_gemm_kernel<64,false,false>", "rc_gemm_kernel<64,true,false>"}
    assert spatial >= {1, 31, 32, 35, 36, 576} and chunks == {1, 2}
    for side in (lambda c: c.Cout, lambda c: c.Cin * c.KH * c.KW):
        assert any(side(c) < 64 for c in cs) and any(side(c) > 64 for c in cs) and any(side(c) in (63, 64, 65) for c in cs)
    assert {c.family for c in cs} == {"S", "IDX", "IDY"}


@pytest.mark.parametrize("c", tc.WGRAD_CASES, ids=tc.conv_id)
def test_wgrad_case_is_exact_and_agrees_with_autograd(c):
    case = tc.wgrad_case(c)
    x, dy = case["x"], case["dy"]
    assert _integers(x, dy) and dy.shape == (c.B, c.Cout) + tc.conv_out(c)
    _bounded(case["absum"], c)
    w = torch.zeros(c.Cout, c.Cin, c.KH, c.KW, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, stride=c.stride, padding=c.pad).backward(dy.double())
    assert torch.equal(w.grad, case["ref"]), c
    if c.family == "S":
        for t in (x, dy):
            assert bool((t[:, -1] != 0).all()) and bool((t[:, :, -1] != 0).all()) and bool((t[:, :, :, -1] != 0).all())
    elif c.family == "IDX":
        from deepi2p_amd import ops
        OH, OW = tc.conv_out(c)
        rt = ops.rc_route("wgrad", c.B, c.Cout, c.Cin * c.KH * c.KW, OH * OW)
        hot = dy.view(c.B, c.Cout, -1)
        assert bool((hot.sum(2) == 1).all()) and x.unique().numel() == x.numel()
        crit = tc.critical_set(OH * OW, rt["rch"], rt["chunks"])
        assert c.Cout < len(crit) or all(set(crit) <= set(hot[b].argmax(1).tolist()) for b in range(c.B)), c
    else:
        assert bool((x.view(c.B, c.Cin, -1).sum(2) == 1).all()) and dy.unique().numel() == dy.numel()


def test_dgrad_table_lists_every_edge_of_the_issue():
    cs = tc.DGRAD_CASES
    _conv_grid_is_complete(cs)
    assert {c.H for c in cs} >= set(tc.DGRAD_SIZES) and {c.W for c in cs} >= set(tc.DGRAD_SIZES)
    assert {c.Cin for c in cs} >= {1, 5, 65} and {c.Cout for c in cs} >= {1, 3, 17}
    assert any(c.H * c.W < 64 for c in cs) and any(c.H * c.W > 64 for c in cs)
    assert {c.Cout * c.KH * c.KW for c in cs} >= {1, 15, 16, 17}
    assert {c.family for c in cs} == {"S", "IDY", "IDW"}
    assert {c.family for c in cs if c.stride == 2} == {"S", "IDY", "IDW"}


@pytest.mark.parametrize("c", tc.DGRAD_CASES, ids=tc.conv_id)
def test_dgrad_case_is_exact_and_agrees_with_autograd(c):
    case = tc.dgrad_case(c)
    dy, w = case["dy"], case["w"]
    assert _integers(dy, w) and case["ref"].shape == (c.B, c.Cin, c.H, c.W)
    _bounded(case["absum"], c)
    x = torch.zeros(c.B, c.Cin, c.H, c.W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), stride=c.stride, padding=c.pad).backward(dy.double())
    assert torch.equal(x.grad, case["ref"]), c
    if c.family == "S":
        assert bool((w[-1] != 0).all()) and bool((w[:, -1] != 0).all()) and bool((w[:, :, -1] != 0).all()) and bool((w[..., -1] != 0).all())
        assert bool((dy[:, -1] != 0).all()) and bool((dy[:, :, -1] != 0).all()) and bool((dy[..., -1] != 0).all())
    elif c.family == "IDY":
        assert bool((w.transpose(0, 1).reshape(c.Cin, -1).sum(1) == 1).all()) and dy.unique().numel() == dy.numel()
    else:
        assert bool((dy.view(c.B, -1).sum(1) == 1).all()) and w.unique().numel() == w.numel()


# ------------------------------------------------------------------------------------------------ di2p_gather_backward
def test_gather_table_reaches_every_edge():
    from deepi2p_amd import _lib, ops
    lib = _lib.load()
    cs = tc.GATHER_CASES
    assert {c.mode for c in cs} == {"k1", "k1w", "k3w"} and {c.M for c in cs} >= set(tc.GATHER_M) and {c.C for c in cs} >= set(tc.GATHER_C)
    assert {c.J for c in cs} == set(tc.GATHER_J)
    for mode in ("k1", "k1w", "k3w"):
        assert {c.J for c in cs if c.mode == mode} == set(tc.GATHER_J)
        assert {c.pattern for c in cs if c.mode == mode and c.family == "S"} == set(tc.GATHER_PATTERNS if mode == "k3w" else tc.GATHER_PATTERNS[:3])
    seen = collections.Counter()
    for c in cs:
        rt = ops.rc_route("gather", c.B, c.C, c.M, c.J, True, True)
        seen[instance_of(rt)] += 1
        assert lib.di2p_gather_backward_workspace_bytes(c.B, c.C, c.J, c.M) == c.B * rt["chunks"] * c.C * c.M * 4, c
    print("di2p_gather_backward cases per kernel instance:", dict(seen))
    assert set(seen) == {"rc_gemm_kernel<64,false,false>"}


@pytest.mark.parametrize("c", tc.GATHER_CASES, ids=tc.gather_id)
def test_gather_case_is_exact_and_agrees_with_autograd(c):
    case = tc.gather_case(c)
    dy, idx, w, k = case["dy"], case["idx"].long(), case["w"], case["k"]
    assert _integers(dy, w) and idx.shape == (c.B, c.J, k) and int(idx.min()) >= 0 and int(idx.max()) < c.M
    _bounded(case["absum"], c)
    # torch's own backward of the gather (and of the weighted sum of three gathers) in fp64
    feats = torch.zeros(c.B, c.C, c.M, dtype=torch.float64, requires_grad=True)
    y = 0
    for kk in range(k):
        g = torch.gather(feats, 2, idx[:, :, kk].unsqueeze(1).expand(c.B, c.C, c.J))
        y = y + (g if w is None else g * w[:, :, kk].double().unsqueeze(1))
    y.backward(dy.double())
    assert torch.equal(feats.grad, case["ref"]), c
    assert bool((dy[:, :, -1] != 0).all()) and bool((dy[:, -1] != 0).all())
    unref = case["unreferenced"]
    assert bool((case["ref"].transpose(1, 2)[unref] == 0).all())
    if c.M >= 3:
        assert bool(unref.any(1).all()), c
    if c.pattern == "dup2":
        assert bool((idx[:, :, 0] == idx[:, :, 2]).all())
    if c.pattern == "dup3":
        assert bool((idx[:, :, 0] == idx[:, :, 1]).all()) and bool((idx[:, :, 0] == idx[:, :, 2]).all())
    if c.pattern == "one":
        assert idx.unique().numel() == 1
    if w is not None and c.J >= 31:
        assert bool((w == 0).any()) and bool((w < 0).any())
    if c.family == "ID":
        from deepi2p_amd import ops
        rt = ops.rc_route("gather", c.B, c.C, c.M, c.J)
        for j in tc.critical_set(c.J, rt["rch"], rt["chunks"]):
            assert int((idx[0, :, 0] == idx[0, j, 0]).sum()) == 1          # a node of its own: the output there is the id of (b, c, j)
            assert float(case["ref"][0, c.C - 1, idx[0, j, 0]]) == float(dy[0, c.C - 1, j])


# ------------------------------------------------------------------------------------------------ di2p_channel_sum
def test_sum_table_is_the_issues():
    assert len(tc.SUM_CASES) == 3 * 2 * 3 * 8
    for fam in ("S", "dyadic", "wide"):
        assert {(c.B, c.C, c.N) for c in tc.SUM_CASES if c.family == fam} == {(b, ch, n) for b in (1, 3) for ch in (1, 64, 65) for n in tc.SUM_N}


@pytest.mark.parametrize("c", tc.SUM_CASES, ids=tc.sum_id)
def test_sum_case_is_exact(c):
    x, ref = tc.sum_case(c)
    if c.family == "S":
        assert _integers(x) and float(x.abs().sum((0, 2)).max()) <= tc.LIMIT
        assert bool((x[-1] != 0).all()) and bool((x[:, :, -1] != 0).all())
    else:
        k = x.double() * 256.0
        assert _integers(k) and float(k.abs().max()) < 2 ** tc.SUM_BITS[c.family]
        # every partial sum, in any order, is a multiple of 2^-8 below 2^53 * 2^-8: the fp64 sum is exact
        assert float(k.abs().sum((0, 2)).max()) < 2.0 ** 53
        assert torch.equal((k.to(torch.int64).sum((0, 2)).double() / 256.0).float(), ref)
        if c.family == "wide" and c.N >= 255:          # already two elements often do not add exactly in fp32 (same sign, sum >= 2^24 and odd: 1/8)
            a, b = x[0, 0, :-1], x[0, 0, 1:]
            assert float(((a + b).double() != a.double() + b.double()).float().mean()) > 0.05
