"""GPU: the kernels of the training step that are not matrix products (csrc/train.hip: train-mode BatchNorm both ways, the max-pool backward, the
arg-max routers, the mask application; csrc/conv.hip: the max-pool and the global average pool; csrc/loss.hip: the classifier loss and Adam;
csrc/index_max.hip on its split path with a ragged N) on the operands of tests/train_pointwise_cases.py, whose premises
tests/test_train_pointwise_cases_host.py proves.  Every call goes through _lib.call on raw pointers; every output and every operand sits
between NaN guard bands, outputs pre-filled with NaN; every workspace is exactly as long as the library asks, with a NaN guard behind it;
every case runs twice and must give the same bits.  What can be exact is compared bit for bit; where the kernel rounds in fp32, the bound is
the one its roundings allow (stated at the reference) and nothing wider."""
import numpy as np
import pytest
import torch

from tests import train_pointwise_cases as pc
from tests.gpu_exact_harness import Guarded, gptr, put, same_bits, twice

pytestmark = pytest.mark.gpu


def _ws(nbytes, dev):
    return Guarded(nbytes, dev, compare=False)


def _within(got, ref64, bound, what):
    """|got - ref| <= bound everywhere (got f32 on the CPU, ref and bound f64); NaN fails"""
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = pc.first_mismatch(torch.where(bad, 1.0, 0.0), torch.zeros_like(err))
        raise AssertionError("%s: element %s: got %r, fp64 %r, error %.3g over the bound %.3g; %d of %d elements out of bound" % (
            what, idx, float(got[idx]), float(ref64[idx]), float(err[idx]), float(bound[idx]), int(bad.sum()), bad.numel()))


# ------------------------------------------------------------------------------------------------ di2p_bn_train_forward
def _bn_forward(c, case, unfused, dev):
    from deepi2p_amd import _lib
    f = pc.bn_forward_flags(c)
    nb = _lib.load().di2p_channel_reduce_workspace_bytes(c.B, c.C, c.N)
    assert nb == pc.red_plan(c.B, c.C, c.N)[3]
    x, gamma, beta, res = (put(case[k], dev) for k in ("x", "gamma", "beta", "res"))

    def run():
        y, mean, invstd, ws = Guarded(4 * c.B * c.C * c.N, dev), Guarded(4 * c.C, dev), Guarded(4 * c.C, dev), _ws(nb, dev)
        rm, rv = put(case["rm0"], dev), put(case["rv0"], dev)
        _lib.call("di2p_bn_train_forward", x.ptr, gamma.ptr, beta.ptr, gptr(res), y.ptr, mean.ptr, invstd.ptr, gptr(rm), gptr(rv), pc.BN_MOMENTUM, pc.BN_EPS,
                  int(f["relu"]), c.B, c.C, c.N, ws.ptr, _lib.stream())
        return [y, mean, invstd, ws] + ([rm, rv] if f["running"] else [])

    with _lib.option("bn_unfused", unfused):
        outs = twice(run)
    assert x.guards_untouched() and torch.equal(x.cpu(torch.float32), case["x"].reshape(-1))          # the operand was only read
    return outs


@pytest.mark.parametrize("c", pc.BN_CASES, ids=pc.bn_id)
def test_bn_train_forward(dev, c):
    case = pc.bn_forward_case(c)
    f = pc.bn_forward_flags(c)
    fused, unfused = _bn_forward(c, case, 0, dev), _bn_forward(c, case, 1, dev)
    for i, (a, b) in enumerate(zip(fused, unfused)):
        if a.compare:
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), "output %d differs between the fused and the unfused launches" % i
    y, mean, invstd = fused[0].cpu(torch.float32, c.B, c.C, c.N), fused[1].cpu(torch.float32), fused[2].cpu(torch.float32)
    same_bits(mean, (case["sum0"] / case["count"]).float(), "save_mean")
    assert bool(pc.within_one_ulp(invstd, case["invstd"]).all()), "save_invstd: %r against %r" % (invstd, case["invstd"])
    if f["running"]:
        rm, rv = fused[4].cpu(torch.float32), fused[5].cpu(torch.float32)
        assert bool(pc.within_one_ulp(rm, case["rm"]).all()), "running_mean: %r against %r" % (rm, case["rm"])
        assert bool(pc.within_one_ulp(rv, case["rv"]).all()), "running_var: %r against %r" % (rv, case["rv"])
    ref, bound = pc.bn_forward_y(case, f["relu"], mean, invstd)
    _within(y, ref, bound, "y")


# ------------------------------------------------------------------------------------------------ di2p_bn_train_backward
def _bn_backward(c, case, unfused, dev):
    from deepi2p_amd import _lib
    f = pc.bn_backward_flags(c)
    nb = _lib.load().di2p_channel_reduce_workspace_bytes(c.B, c.C, c.N)
    x, dy, gamma, mean, invstd = (put(case[k], dev) for k in ("x", "dy", "gamma", "mean", "invstd"))
    # relu off: y must not be read -- it is NULL, or a buffer of NaN
    y = put(case["y"], dev) if f["relu"] else (None if f["y_null"] else Guarded(4 * c.B * c.C * c.N, dev))

    def run():
        n = 4 * c.B * c.C * c.N
        dx, dgamma, dbeta, ws = Guarded(n, dev), Guarded(4 * c.C, dev), Guarded(4 * c.C, dev), _ws(nb, dev)
        dres = Guarded(n, dev) if f["dres"] else None
        _lib.call("di2p_bn_train_backward", x.ptr, gptr(y), dy.ptr, gamma.ptr, mean.ptr, invstd.ptr, int(f["relu"]), dx.ptr, gptr(dres), dgamma.ptr, dbeta.ptr,
                  c.B, c.C, c.N, ws.ptr, _lib.stream())
        return [dx, dgamma, dbeta, ws] + ([dres] if f["dres"] else [])

    with _lib.option("bn_unfused", unfused):
        return twice(run)


@pytest.mark.parametrize("c", pc.BN_CASES, ids=pc.bn_id)
def test_bn_train_backward(dev, c):
    case = pc.bn_backward_case(c)
    f = pc.bn_backward_flags(c)
    fused, unfused = _bn_backward(c, case, 0, dev), _bn_backward(c, case, 1, dev)
    for i, (a, b) in enumerate(zip(fused, unfused)):
        if a.compare:
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), "output %d differs between the fused and the unfused launches" % i
    same_bits(fused[2].cpu(torch.float32), case["dbeta"], "dbeta")
    same_bits(fused[1].cpu(torch.float32), case["dgamma"], "dgamma")
    if f["dres"]:
        same_bits(fused[4].cpu(torch.float32, c.B, c.C, c.N), case["g"], "dresidual")
    _within(fused[0].cpu(torch.float32, c.B, c.C, c.N), case["dx"], case["bound"], "dx")


# ------------------------------------------------------------------------------------------------ di2p_maxpool3x3s2 and its backward
@pytest.mark.parametrize("c", pc.POOL_FWD_CASES, ids=pc.pool_id)
def test_maxpool_forward(dev, c):
    from deepi2p_amd import _lib
    x_cpu, ref = pc.pool_forward_case(c)
    x = put(x_cpu, dev, 4 * c.xoff)
    assert (x.ptr % 16 == 0) == (c.xoff % 4 == 0)

    def run():
        y = Guarded(4 * ref.numel(), dev, 4 * c.yoff)
        _lib.call("di2p_maxpool3x3s2", x.ptr, y.ptr, c.B, c.C, c.H, c.W, _lib.stream())
        return [y]

    same_bits(twice(run)[0].cpu(torch.float32, *ref.shape), ref, pool_route(c))


def pool_route(c):
    return "%s on the %s kernel" % (pc.pool_id(c), "four-per-lane" if pc.pool_forward_uses_vec4(c) else "scalar")


@pytest.mark.parametrize("c", pc.POOL_BWD_CASES, ids=pc.pool_id)
def test_maxpool_backward(dev, c):
    from deepi2p_amd import _lib
    x_cpu, dy_cpu, ref = pc.pool_backward_case(c)
    x, dy = put(x_cpu, dev), put(dy_cpu, dev)

    def run():
        dx = Guarded(4 * ref.numel(), dev)
        _lib.call("di2p_maxpool3x3s2_backward", x.ptr, dy.ptr, dx.ptr, c.B, c.C, c.H, c.W, _lib.stream())
        return [dx]

    what = "%s on the %s kernel" % (pc.pool_id(c), "LDS" if pc.maxpool_uses_lds((c.B, c.C, c.H, c.W)) else "fallback")
    same_bits(twice(run)[0].cpu(torch.float32, *ref.shape), ref, what)


# ------------------------------------------------------------------------------------------------ di2p_group_max_forward / _backward
@pytest.mark.parametrize("c", pc.GROUP_CASES, ids=pc.group_id)
def test_group_max(dev, c):
    from deepi2p_amd import _lib
    case = pc.group_case(c)
    x, dy, arg_in = put(case["x"], dev), put(case["dy"], dev), put(case["arg"], dev)

    def forward():
        y, arg = Guarded(4 * c.rows, dev), Guarded(4 * c.rows, dev)
        _lib.call("di2p_group_max_forward", x.ptr, y.ptr, arg.ptr, c.rows, c.K, _lib.stream())
        return [y, arg]

    def backward():
        dx = Guarded(4 * c.rows * c.K, dev)
        _lib.call("di2p_group_max_backward", dy.ptr, arg_in.ptr, dx.ptr, c.rows, c.K, _lib.stream())
        return [dx]

    y, arg = twice(forward)
    same_bits(arg.cpu(torch.int32), case["arg"], "arg")
    same_bits(y.cpu(torch.float32), case["y"], "y")
    same_bits(twice(backward)[0].cpu(torch.float32, c.rows, c.K), case["dx"], "dx")


# ------------------------------------------------------------------------------------------------ di2p_segment_max_backward
@pytest.mark.parametrize("c", pc.SEG_CASES, ids=pc.seg_id)
def test_segment_max_backward(dev, c):
    from deepi2p_amd import _lib
    case = pc.seg_case(c)
    dv, idx, mask = put(case["dv"], dev), put(case["idx"], dev), put(case["mask"], dev)
    B, N = pc.SEG_B, case["N"]

    def run():
        dx = Guarded(4 * B * c.C * N, dev)
        _lib.call("di2p_segment_max_backward", dv.ptr, idx.ptr, gptr(mask), dx.ptr, B, c.C, N, c.M, _lib.stream())
        return [dx]

    got = twice(run)[0].cpu(torch.float32, B, c.C, N)
    same_bits(got, case["ref"], pc.seg_id(c))
    assert bool((got[case["unreferenced"]].view(torch.int32) == 0).all())          # +0, not -0, where nothing was added


# ------------------------------------------------------------------------------------------------ di2p_apply_mask
@pytest.mark.parametrize("c", pc.MASK_CASES, ids=pc.mask_id)
def test_apply_mask(dev, c):
    from deepi2p_amd import _lib
    x_cpu, mask_cpu, ref = pc.apply_mask_case(c)
    xo, yo, mo = pc.MASK_ALIGN[c.align]
    x, mask = put(x_cpu, dev, xo), put(mask_cpu, dev, mo)

    def run():
        y = Guarded(4 * c.n, dev, yo)
        _lib.call("di2p_apply_mask", x.ptr, mask.ptr, pc.MASK_SCALE, y.ptr, c.n, _lib.stream())
        return [y]

    what = "%s on the %s kernel" % (pc.mask_id(c), "eight-per-thread" if pc.apply_mask_uses_vec8(c) else "scalar")
    same_bits(twice(run)[0].cpu(torch.float32), ref, what)


# ------------------------------------------------------------------------------------------------ di2p_classifier_loss
@pytest.mark.parametrize("c", pc.LOSS_CASES, ids=pc.loss_id)
def test_classifier_loss(dev, c):
    from deepi2p_amd import _lib
    case = pc.loss_case(c)
    with_fine = c.variant != "no_fine"
    ref = pc.loss_reference(case, with_fine)
    coarse, clab, flab = put(case["coarse"], dev), put(case["clab"], dev), put(case["flab"], dev)
    fine = put(case["fine"], dev) if with_fine else None
    want_dc, want_df = c.variant != "no_dcoarse", c.variant == "full"
    nb = _lib.load().di2p_classifier_loss_workspace_bytes(c.B, c.N)

    def run():
        out, ws = Guarded(64, dev), _ws(nb, dev)
        out.view(torch.float64).fill_(pc.NAN)          # (two fp32 NaNs side by side are a finite double)
        dc = Guarded(4 * c.B * 2 * c.N, dev) if want_dc else None
        df = Guarded(4 * c.B * c.L * c.N, dev) if want_df else None
        _lib.call("di2p_classifier_loss", coarse.ptr, gptr(fine), clab.ptr, flab.ptr if with_fine else None, c.B, c.N, c.L, pc.LOSS_ALPHA, pc.LOSS_GAMMA,
                  pc.LOSS_COARSE_ALPHA, out.ptr, gptr(dc), gptr(df), ws.ptr, _lib.stream())
        return [out, ws] + [b for b in (dc, df) if b is not None]

    outs = twice(run)
    got, want = outs[0].cpu(torch.float64).numpy(), ref["out"]
    print("\n%s: loss %r / %r, coarse %r / %r, fine %r / %r" % (pc.loss_id(c), got[0], want[0], got[1], want[1], got[2], want[2]))
    for i, name in ((0, "loss"), (1, "coarse loss"), (2, "fine loss")):
        if np.isnan(want[i]):
            assert np.isnan(got[i]), "%s: %r, expected NaN (no point inside)" % (name, got[i])
        else:
            assert abs(got[i] - want[i]) <= pc.LOSS_TOL * abs(want[i]), "%s: %r against %r" % (name, got[i], want[i])
    for i, name in ((3, "coarse accuracy"), (4, "fine accuracy"), (5, "inside count")):       # quotients of exact integers: the same bits
        assert got[i:i + 1].tobytes() == want[i:i + 1].tobytes() or (np.isnan(got[i]) and np.isnan(want[i])), "%s: %r against %r" % (name, got[i], want[i])
    assert got[6] == 0.0 and got[7] == 0.0
    rest = outs[2:]
    if want_dc:
        d = rest.pop(0).cpu(torch.float32, c.B, 2, c.N).double()
        tol = pc.LOSS_TOL * float(ref["d_coarse"].abs().max())
        assert float((d - ref["d_coarse"]).abs().max()) <= tol, "d_coarse: %.3g over %.3g" % (float((d - ref["d_coarse"]).abs().max()), tol)
    if want_df:
        d = rest.pop(0).cpu(torch.float32, c.B, c.L, c.N)
        tol = pc.LOSS_TOL * float(ref["d_fine"].abs().max())
        assert float((d.double() - ref["d_fine"]).abs().max()) <= tol, "d_fine: %.3g over %.3g" % (float((d.double() - ref["d_fine"]).abs().max()), tol)
        outside = (case["clab"] != 1)[:, None, :].expand(c.B, c.L, c.N)
        assert bool((d[outside].view(torch.int32) == 0).all()), "d_fine is not exactly 0 at a point outside the image"


# ------------------------------------------------------------------------------------------------ di2p_adam_step
@pytest.mark.parametrize("c", pc.ADAM_CASES, ids=pc.adam_id)
def test_adam_step(dev, c):
    from deepi2p_amd import _lib
    case = pc.adam_case(c)
    g = put(case["g"], dev)

    def run():
        p, m, v = put(case["p"], dev), put(case["m"], dev), put(case["v"], dev)
        _lib.call("di2p_adam_step", p.ptr, g.ptr, m.ptr, v.ptr, c.n, c.step, pc.ADAM_LR, pc.ADAM_B1, pc.ADAM_B2, pc.ADAM_EPS, _lib.stream())
        return [p, m, v]

    outs = twice(run)
    assert g.guards_untouched() and torch.equal(g.cpu(torch.float32), case["g"])
    for buf, name in zip(outs, ("p1", "m1", "v1")):
        got, want = buf.cpu(torch.float32).double(), case[name]
        assert float((got - want).abs().max()) <= pc.ADAM_TOL * float(want.abs().max()), "%s: %.3g over %.3g" % (
            name, float((got - want).abs().max()), pc.ADAM_TOL * float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ index_max: split path, ragged N
@pytest.mark.parametrize("c", pc.IMAX_CASES, ids=pc.imax_id)
def test_index_max_split_ragged(dev, c):
    from deepi2p_amd import _lib
    case = pc.imax_case(c)
    data, index, mask = put(case["data"], dev), put(case["index"], dev), put(case["mask"], dev)
    n = c.B * c.C * c.K

    def launch(with_ws, values, with_mask, with_idx):
        def run():
            ws = _ws(8 * n, dev) if with_ws else None
            idx = Guarded(4 * n, dev) if with_idx else None
            val = Guarded(4 * n, dev) if values else None
            if values:
                _lib.call("di2p_index_max_values", data.ptr, index.ptr, mask.ptr if with_mask else None, val.ptr, gptr(idx), c.B, c.C, c.N, c.K, gptr(ws),
                          _lib.stream())
            else:
                _lib.call("di2p_index_max_forward", data.ptr, index.ptr, idx.ptr, c.B, c.C, c.N, c.K, gptr(ws), _lib.stream())
            return [b for b in (idx, val, ws) if b is not None]
        return run

    for values, with_mask, with_idx in ((False, False, True), (True, True, True), (True, False, True), (True, True, False)):
        per_ws = []
        for with_ws in (True, False):
            outs = twice(launch(with_ws, values, with_mask, with_idx))
            what = "%s %s %s %s" % (pc.imax_id(c), "split" if with_ws else "one pass", "values" if values else "indices", "mask" if with_mask else "no mask")
            if with_idx:
                same_bits(outs[0].cpu(torch.int32, c.B, c.C, c.K), case["idx"], what)
            if values:
                same_bits(outs[1 if with_idx else 0].cpu(torch.float32, c.B, c.C, c.K), case["val_mask" if with_mask else "val_nomask"], what)
            per_ws.append([b for b in outs if b.compare])
        for a, b in zip(*per_ws):
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), "with and without a workspace differ"


# ------------------------------------------------------------------------------------------------ di2p_global_avgpool
@pytest.mark.parametrize("HW", pc.AVG_HW)
def test_global_avgpool(dev, HW):
    from deepi2p_amd import _lib
    for B, C in pc.AVG_ROWS:
        x_cpu, ref = pc.avgpool_case(B, C, HW)
        x = put(x_cpu, dev)

        def run():
            y = Guarded(4 * B * C, dev)
            _lib.call("di2p_global_avgpool", x.ptr, y.ptr, B, C, HW, _lib.stream())
            return [y]

        same_bits(twice(run)[0].cpu(torch.float32, B, C), ref, "b%d c%d hw%d" % (B, C, HW))
