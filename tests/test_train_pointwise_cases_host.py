"""The premises of tests/train_pointwise_cases.py, proved on the host (no GPU): the bit counts that make the BatchNorm sums exact in fp64 in any
order, the exactness of xhat and of every product of the backward cases, the restated chunk plan against the library's own workspace size, the
sentinels (losing or doubling one moves the fp32 result), the dispatch predicates against the shapes that are meant to cross them, the
integer bounds of the router cases, and the sensitivity of the loss cases to a lost point."""
import numpy as np
import pytest
import torch

from tests import train_pointwise_cases as pc


def _k(t):
    """t = k / 256 -> k as exact integers (asserting that t is such a value)"""
    k = (t.double() * 256.0)
    assert bool((k == k.round()).all())
    return k.long()


# ------------------------------------------------------------------------------------------------ the table and the chunk plan
def test_bn_table_covers_the_issue():
    cases = pc.BN_CASES
    assert {c.N for c in cases} == set(pc.BN_N) and len(cases) == 2 * len(pc.BN_N)
    assert {(c.B, c.C) for c in cases} >= {(B, C) for B in (1, 3) for C in (1, 64, 65)}
    assert all(c.B * c.N >= 2 for c in cases) and [c.B for c in cases if c.N == 1] == [2, 2]
    for bit in (1, 2, 4):                                  # every switch on and off, with one chunk and with several
        for many in (False, True):
            seen = {bool(c.flags & bit) for c in cases if (pc.red_plan(c.B, c.C, c.N)[0] > 1) == many}
            assert seen == {False, True}, (bit, many)
    assert any(pc.bn_backward_flags(c)["y_null"] for c in cases)
    # chunk counts: 1, 2, 3 (ragged last chunk), the cap of 16
    assert {pc.red_plan(1, 1, N)[0] for N in pc.BN_N} >= {1, 2, 3, 16}
    assert pc.red_plan(1, 1, 8193)[:2] == (2, 4097) and pc.red_plan(1, 1, 12289)[:2] == (3, 4097) and pc.red_plan(1, 1, 70001)[:2] == (16, 4376)


def test_restated_chunk_plan_matches_the_library():
    from deepi2p_amd import _lib
    lib = _lib.load()
    shapes = {(c.B, c.C, c.N) for c in pc.BN_CASES} | {(B, C, N) for B in (1, 3) for C in (1, 65) for N in (1, 4095, 4096, 8191, 8192, 8193, 65536, 70001, 200000)}
    for B, C, N in sorted(shapes):
        SN, per, S, nbytes = pc.red_plan(B, C, N)
        assert nbytes == lib.di2p_channel_reduce_workspace_bytes(B, C, N), (B, C, N)
        assert S == B * SN and (SN - 1) * per < N <= SN * per and 1 <= SN <= 16
        crit = pc.critical_positions(N)
        assert crit == sorted(set(crit)) and crit[0] == 0 and crit[-1] == N - 1
        for ch in range(1, SN):
            assert ch * per - 1 in crit and ch * per in crit
        assert (N <= 255) or (255 in crit and (N == 256 or 256 in crit))


def test_bn_bit_counts():
    """the largest case: 2^18 > B * N values of |k| < 2^12 per channel.  sum k < 2^30 and sum k^2 < 2^42, both far below 2^53; the backward
    products g * xhat are multiples of 2^-18 below 2^10 and their sums below 2^28: 46 bits"""
    count = max(c.B * c.N for c in pc.BN_CASES)
    assert count == 3 * 70001 and count < 2 ** 18
    assert count * (2 ** 12 - 1) < 2 ** 30 and count * (2 ** 12 - 1) ** 2 < 2 ** 42 < 2 ** 53
    max_xhat_k = (2 ** 12 - 1 + 256) * 4 * 2            # (k - j) / 256 * invstd <= 2, in units of 2^-10
    assert max_xhat_k < 2 ** 24                          # exact in fp32
    assert count * (2 ** 12 - 1) * max_xhat_k < 2 ** 53  # the sum of g * xhat in units of 2^-18
    # a lost or doubled sentinel (|x| >= 8) moves the mean by 8 / count, far more than the spacing of fp32 below 16 (2^-20)
    assert 8.0 / count > 16 * 2.0 ** -20


@pytest.mark.parametrize("c", pc.BN_CASES, ids=pc.bn_id)
def test_bn_forward_case_is_exact_and_sensitive(c):
    case = pc.bn_forward_case(c)
    x = case["x"]
    k = _k(x)
    assert int(k.abs().max()) < 2 ** 12
    # the fp64 sums are the integer sums: nothing was rounded on the way
    assert torch.equal(case["sum0"] * 256.0, k.sum((0, 2)).double()) and torch.equal(case["sum1"] * 65536.0, (k * k).sum((0, 2)).double())
    crit = case["crit"]
    assert bool((x[:, :, crit].abs() >= 8).all())
    mean32 = (case["sum0"] / case["count"]).float()
    for p in crit:                                         # losing or doubling any sentinel of any row changes the fp32 mean
        for sign in (-1.0, 1.0):
            moved = ((case["sum0"][None, :] + sign * x[:, :, p].double()) / case["count"]).float()
            assert bool((moved != mean32[None, :]).all()), (p, sign)
    if case["rm0"] is not None:
        assert bool((case["rv0"] > 0).all())
    assert bool((case["invstd"] > 0).all()) and bool(torch.isfinite(case["invstd"]).all())


@pytest.mark.parametrize("c", pc.BN_CASES, ids=pc.bn_id)
def test_bn_backward_case_is_exact_and_sensitive(c):
    case = pc.bn_backward_case(c)
    f = pc.bn_backward_flags(c)
    kx, kd, kj = _k(case["x"]), _k(case["dy"]), _k(case["mean"])
    assert int(kx.abs().max()) < 2 ** 12 and int(kd.abs().max()) < 2 ** 12 and int(kj.abs().max()) <= 256
    assert set(case["invstd"].tolist()) <= {0.25, 0.5, 1.0, 2.0}
    # xhat: the fp32 value is the exact one, (k - j) * invstd / 256
    exact = (kx - kj[None, :, None]).double() / 256.0 * case["invstd"].double()[None, :, None]
    assert torch.equal(case["xhat"].double(), exact)
    # the sums: integer arithmetic in units of 2^-8 and 2^-18
    g10 = torch.where(case["keep"], kd, torch.zeros((), dtype=torch.long))
    xh10 = (exact * 1024.0).long()
    assert torch.equal(xh10.double(), exact * 1024.0)
    assert torch.equal(case["a0"] * 256.0, g10.sum((0, 2)).double()) and torch.equal(case["a1"] * 262144.0, (g10 * xh10).sum((0, 2)).double())
    # y: the mask is `y > 0`: both zeros, negatives and NaN are masked, the tiny and the subnormal positives are not; all of them occur
    y = case["y"]
    if c.B * c.C * c.N >= 4096:
        bits = y.view(torch.int32)
        assert bool((bits == 0).any()) and bool((bits == -2 ** 31).any()) and bool(torch.isnan(y).any()) and bool((y < 0).any())
        assert bool(((y > 0) & (y < 1e-38)).any()) and bool((y == 1e-30).any())
        if f["relu"]:                                      # `y >= 0` instead of `y > 0` would change both sums of some channel
            loose = torch.where(y >= 0, kd, torch.zeros((), dtype=torch.long))
            assert bool((loose.sum((0, 2)) != g10.sum((0, 2))).any()) and bool(((loose * xh10).sum((0, 2)) != (g10 * xh10).sum((0, 2))).any())
    # the sentinels: present in g (never masked), large in dy and in dy * xhat; losing or doubling one changes fp32 dbeta and dgamma
    crit = case["crit"]
    assert bool(case["keep"][:, :, crit].all()) and bool((case["g"][:, :, crit].abs() >= 8).all()) and bool((case["xhat"][:, :, crit].abs() >= 1.75).all())
    for p in crit:
        for sign in (-1.0, 1.0):
            assert bool(((case["a0"][None, :] + sign * case["term0"][:, :, p]).float() != case["dbeta"][None, :]).all()), (p, sign)
            assert bool(((case["a1"][None, :] + sign * case["term1"][:, :, p]).float() != case["dgamma"][None, :]).all()), (p, sign)


# ------------------------------------------------------------------------------------------------ max-pool
def test_pool_cases_cross_the_dispatch_edges():
    fwd = pc.POOL_FWD_CASES
    vec = [c for c in fwd if pc.pool_forward_uses_vec4(c)]
    assert {(c.H, c.W) for c in vec} == {(1, 8), (5, 8), (7, 16), (33, 64)}
    misaligned = [c for c in fwd if c.W % 8 == 0 and not pc.pool_forward_uses_vec4(c)]
    assert {(c.xoff > 0, c.yoff > 0) for c in misaligned} == {(True, False), (False, True), (True, True)}
    assert {(c.H, c.W) for c in fwd if c.W % 8} == {(1, 1), (2, 2), (6, 2), (9, 7), (33, 65)}
    assert all(c.B * c.C >= 4 for c in fwd)                # the four special planes fit
    bwd = pc.POOL_BWD_CASES
    assert {c.H for c in bwd} >= {1, 2, 7, 8, 9, 33}
    # the LDS limit: 11 input rows and 5 window rows of OW = ceil(W / 2) ints in 64 KiB
    W = pc.POOL_LDS_MAX_W
    assert W == 1213 and (11 * W + 5 * 607) * 4 == 65512 <= 65536 < (11 * (W + 1) + 5 * 607) * 4 == 65556
    assert pc.maxpool_uses_lds((1, 2, 9, W)) and not pc.maxpool_uses_lds((1, 2, 9, W + 1))
    assert pc.maxpool_uses_lds((1, 65535, 2, 2)) and not pc.maxpool_uses_lds((1, 65536, 2, 2))
    routes = {(pc.maxpool_uses_lds((c.B, c.C, c.H, c.W)), c.B * c.C > 65535, c.W > W) for c in bwd}
    assert routes == {(True, False, False), (False, True, False), (False, False, True)}


@pytest.mark.parametrize("c", [c for c in pc.POOL_BWD_CASES if c.B * c.C < 100], ids=pc.pool_id)
def test_pool_backward_reference_takes_the_first_maximum(c):
    """torch's autograd against a literal scan of every window ((ky, kx) order, strict >) on the small cases"""
    x, dy, ref = pc.pool_backward_case(c)
    assert set(x.unique().tolist()) <= {0.0, 1.0, 2.0} and float(dy.abs().max()) <= 8 and float(dy.abs().min()) >= 1
    if c.H * c.W > 700:
        x, dy, ref = x[:1, :1], dy[:1, :1], ref[:1, :1]
    want = torch.zeros_like(x)
    OH, OW = pc.pool_out(c.H, c.W)
    xn, dn, wn = x.numpy(), dy.numpy(), want.numpy()
    ties = 0
    for b in range(x.shape[0]):
        for ch in range(x.shape[1]):
            for oy in range(OH):
                for ox in range(OW):
                    best, arg, n_best = None, None, 0
                    for yy in range(max(0, 2 * oy - 1), min(c.H, 2 * oy + 2)):
                        for xx in range(max(0, 2 * ox - 1), min(c.W, 2 * ox + 2)):
                            v = xn[b, ch, yy, xx]
                            if best is None or v > best:
                                best, arg, n_best = v, (yy, xx), 1
                            elif v == best:
                                n_best += 1
                    ties += n_best > 1
                    wn[b, ch, arg[0], arg[1]] += dn[b, ch, oy, ox]
    assert torch.equal(want, ref)
    assert c.H * c.W < 9 or ties > 0


# ------------------------------------------------------------------------------------------------ routers
@pytest.mark.parametrize("c", pc.GROUP_CASES, ids=pc.group_id)
def test_group_case(c):
    case = pc.group_case(c)
    x, arg = case["x"], case["arg"].long()
    for r in range(c.rows):                                # the kernel's rule, literally: strict >, and the first NaN wins and stays
        best, a = x[r, 0], 0
        for k in range(1, c.K):
            v = x[r, k]
            if v > best or (v != v and best == best):
                best, a = v, k
        assert a == int(arg[r])
    nan = torch.isnan(x)
    if bool(nan.any()):
        assert bool((x.view(torch.int32)[nan] == pc.NAN_PAYLOAD_BITS).all())          # an operand NaN is not the NaN of an unwritten output
    assert bool((case["dy"] != 0).all()) and int((case["dx"] != 0).sum()) == c.rows
    if c.rows > 3 and c.K > 1:
        assert int(arg[1]) == 0 and int(arg[2]) == 0 and int(arg[3]) == 0              # all -inf, all NaN, all equal: the first
    if c.rows >= 255 and c.K >= 16:
        assert bool((arg > 0).any()) and bool(nan.any()) and bool(torch.isinf(x).any())


@pytest.mark.parametrize("c", pc.SEG_CASES, ids=pc.seg_id)
def test_seg_case(c):
    case = pc.seg_case(c)
    idx, N = case["idx"], case["N"]
    assert case["absum"] <= 2 ** 24 and bool((case["dv"] != 0).all())
    assert bool(((case["ref"] * 2) == (case["ref"] * 2).round()).all())
    assert bool((idx == -1).any() or (idx == N).any()) and int(idx.min()) >= -1 and int(idx.max()) <= N
    if c.M > 1:
        assert bool((idx == -1).any()) and bool((idx == N).any())
        inside = [sorted(v for v in row.tolist() if 0 <= v < N) for row in idx.view(-1, c.M)]
        if c.pattern == "distinct":
            assert all(len(set(r)) == len(r) for r in inside)
        elif c.M >= 127:
            assert all(len(set(r)) < len(r) for r in inside)
        assert bool(case["unreferenced"].any()) and bool((~case["unreferenced"]).any())
    assert bool((case["ref"][case["unreferenced"]] == 0).all())
    if case["mask"] is not None:
        assert set(case["mask"].unique().tolist()) <= ({0.0, 1.0} if c.mask == "binary" else {0.0, 0.5, 1.0})


# ------------------------------------------------------------------------------------------------ masks
def test_mask_cases_cross_the_dispatch():
    assert {(c.n, c.align) for c in pc.MASK_CASES if pc.apply_mask_uses_vec8(c)} == {(8, "aligned"), (2048, "aligned"), (2056, "aligned")}
    for c in pc.MASK_CASES:
        x, mask, ref = pc.apply_mask_case(c)
        assert set(mask.unique().tolist()) <= {0, 1, 2, 255}
        assert not bool(torch.isnan(ref).any()) and bool((ref[mask == 0].view(torch.int32) == 0).all())          # exactly +0 under a zero byte
        if c.n >= 8:
            assert mask[:8].tolist() == [1, 0, 2, 0, 255, 0, 0, 1] and bool(torch.isnan(x[mask == 0]).any()) and bool((ref[:8][mask[:8] != 0] != 0).all())
        if c.n >= 2048:
            assert set(mask.unique().tolist()) == {0, 1, 2, 255} and bool(torch.isinf(x[mask == 0]).any()) and bool(torch.isinf(ref).any())


# ------------------------------------------------------------------------------------------------ loss
def test_loss_table_covers_the_issue():
    cases = pc.LOSS_CASES
    assert {(c.B, c.N, c.L) for c in cases} == {(B, N, L) for B in (1, 3) for N in (1, 255, 256, 257, 700) for L in (1, 2, 80)}
    assert {c.scenario for c in cases} == set(pc.LOSS_SCENARIOS) and {c.variant for c in cases} == set(pc.LOSS_VARIANTS)
    assert {c.scenario for c in cases if c.variant == "full" and c.L > 1} == set(pc.LOSS_SCENARIOS)


@pytest.mark.parametrize("c", pc.LOSS_CASES, ids=pc.loss_id)
def test_loss_case_is_sensitive_to_every_critical_point(c):
    """A kernel loses a point by not adding its terms (the ragged last block, the first thread of a block): the coarse divisor B * N stays,
    the inside count drops with the point.  Losing any one of points 0, 255, 256, N - 1 of any frame must move the loss by more than ten times
    the tolerance the GPU test allows.  (Not every point can be that heavy: a point the coarse head classifies correctly with a gap of 100
    has a focal term of 1e-18.  The critical points are confidently wrong; N is small, so each weighs more than 1e-4 of the sum.)"""
    case = pc.loss_case(c)
    with_fine = c.variant != "no_fine"
    full = pc.loss_reference(case, with_fine)["out"]
    inside = int((case["clab"] == 1).sum())
    assert (inside == 0) == (c.scenario == "none_inside") or c.N == 1
    if c.scenario == "all_inside":
        assert inside == c.B * c.N
    if c.scenario == "none_inside" and with_fine:
        assert np.isnan(full[2]) and np.isnan(full[0]) and np.isnan(full[4]) and full[5] == 0
    if c.scenario == "ties" and c.N > 200:
        assert bool((case["coarse"][:, 0] == case["coarse"][:, 1]).any())
        if c.L > 1:
            top = case["fine"].max(1, keepdim=True).values
            assert bool(((case["fine"] == top).sum(1) > 1).any())
    if c.scenario == "gaps" and c.N > 200:
        assert float((case["coarse"][:, 0] - case["coarse"][:, 1]).abs().max()) > 90
    if c.scenario == "big_fine":
        assert float(case["fine"].min()) > 9000
    for b in range(c.B):
        for p in case["crit"]:
            keep = torch.ones(c.B, c.N, dtype=torch.bool)
            keep[b, p] = False
            lost = pc.loss_reference(case, with_fine, keep)["out"]
            assert abs(lost[1] - full[1]) > 10 * pc.LOSS_TOL * abs(full[1]), (b, p, lost[1], full[1])
            if with_fine and case["clab"][b, p] == 1:
                assert lost[5] == full[5] - 1
                if c.L > 1 and full[5] > 1 and c.N > 1:       # (N = 1: every inside point has the same fine term, only the count notices)
                    assert abs(lost[2] - full[2]) > 10 * pc.LOSS_TOL * abs(full[2]), (b, p, lost[2], full[2])
                    assert abs(lost[0] - full[0]) > 10 * pc.LOSS_TOL * abs(full[0])


def test_loss_reference_with_every_point_kept_is_the_oracle():
    c = pc.LossCase(3, 257, 80, "mixed", "full")
    case = pc.loss_case(c)
    a, b = pc.loss_reference(case), pc.loss_reference(case, keep=torch.ones(3, 257, dtype=torch.bool))
    assert np.allclose(a["out"], b["out"], rtol=1e-13, atol=0) and torch.allclose(a["d_coarse"], b["d_coarse"], rtol=1e-12, atol=1e-18)


# ------------------------------------------------------------------------------------------------ the neighbours
@pytest.mark.parametrize("c", pc.IMAX_CASES, ids=pc.imax_id)
def test_imax_case(c):
    case = pc.imax_case(c)
    S, sl = pc.imax_slices(c)
    assert S == 2 and c.N % 4 != 0 and sl % 4 == 0 and sl < c.N <= 2 * sl             # two slices, the second one short; rows start misaligned
    data, index, idx = case["data"], case["index"], case["idx"]
    assert int(index.min()) == 0 and int(index.max()) < c.K - 1                        # the last cluster is empty
    none = case["none"]
    assert none[:, :, c.K - 1].all() and none[:, :, 0].all() and not none[:, :, 1:max(2, c.K - 2)].all()
    assert bool(torch.isnan(data).any()) and bool((data == -1000.0).any())
    # winners on both sides of the slice boundary and at N - 1 (values 4 and 5 exist only there)
    won = set(idx.reshape(-1).tolist())
    assert won & set(case["edges"]) and c.N - 1 in case["edges"] and sl - 1 in case["edges"] and sl in case["edges"]
    picked = torch.gather(data, 2, idx.long())
    assert not bool(torch.isnan(picked).any())
    assert bool((case["val_nomask"][torch.from_numpy(none)] == 0).all())


def test_avgpool_cases_are_exact():
    for B, C in pc.AVG_ROWS:
        for HW in pc.AVG_HW:
            x, ref = pc.avgpool_case(B, C, HW)
            assert float(x.abs().sum(2).max()) < 2 ** 24 and bool((x == x.round()).all())
            assert torch.equal(ref, (x.double().sum(2) / HW).float()) or HW not in (1, 64, 2560)          # a power-of-two count divides exactly
    assert any(B * C % 4 for B, C in pc.AVG_ROWS)


def test_adam_reference_is_torch():
    c = pc.AdamCase(257, 1)
    case = pc.adam_case(c)
    p = torch.nn.Parameter(case["p"].double())
    opt = torch.optim.Adam([p], lr=float(np.float32(pc.ADAM_LR)), betas=(float(np.float32(pc.ADAM_B1)), float(np.float32(pc.ADAM_B2))),
                           eps=float(np.float32(pc.ADAM_EPS)), weight_decay=0)
    # torch starts from zero moments: compare on a case with m = v = 0
    case0 = dict(case, m=torch.zeros(257), v=torch.zeros(257))
    lr, b1, b2, eps = (float(np.float32(h)) for h in (pc.ADAM_LR, pc.ADAM_B1, pc.ADAM_B2, pc.ADAM_EPS))
    m1 = (1.0 - b1) * case0["g"].double()
    v1 = (1.0 - b2) * case0["g"].double() ** 2
    want = case0["p"].double() - (lr / (1.0 - b1)) * (m1 / (v1.sqrt() / (1.0 - b2) ** 0.5 + eps))
    p.grad = case0["g"].double()
    opt.step()
    assert torch.allclose(p.detach(), want, rtol=1e-12, atol=0)
    assert bool((case["v"] >= 0).all()) and {a.step for a in pc.ADAM_CASES} == {1, 10000}
