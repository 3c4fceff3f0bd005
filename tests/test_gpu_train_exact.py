"""GPU: the fp32 matrix kernels of the training step (csrc/train.hip: the rc-GEMM family behind every weight gradient, the gather /
interpolation backward, the km-GEMM, both convolution input-gradient kernels, the fp64 channel sum) on operands for which they are exact
(tests/train_exact_cases.py; the premises: tests/test_train_exact_cases_host.py).  Every call goes through _lib.call on raw pointers -- strided
operands inside NaN-filled buffers, the output between NaN guard bands, output and workspace pre-filled with NaN -- and must equal the fp64
reference bit for bit (torch.equal), leave every guard untouched, and give the same bits when it runs again.  There is no tolerance here."""
import concurrent.futures

import pytest
import torch

from tests import train_exact_cases as tc
from tests.gpu_exact_harness import _Out, _Workspace, _device, _same, _twice, _untouched

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ di2p_bmm_rc
@pytest.mark.parametrize("c", tc.RC_CASES, ids=tc.rc_id)
def test_bmm_rc_is_exact(dev, c):
    from deepi2p_amd import _lib, ops
    case = tc.rc_case(c)
    (abuf, aptr), (bbuf, bptr) = _device(case["pa"], dev), _device(case["pb"], dev)
    pa, pb = case["pa"], case["pb"]
    out_shape = (c.rows, c.cols) if c.reduce_z else (c.Z, c.rows, c.cols)
    nb = _lib.load().di2p_bmm_rc_workspace_bytes(c.Z, c.rows, c.cols, c.R)

    def launch(out, ws):
        _lib.call("di2p_bmm_rc", aptr, pa.ld, pa.batch_stride, bptr, pb.ld, pb.batch_stride, out.ptr, c.Z, c.rows, c.cols, c.R, c.alpha, c.reduce_z,
                  ws.ptr, ws.bytes, _lib.stream())

    with _lib.option("rc_tile64", c.tile64):
        rt = ops.rc_route("strided", c.Z, c.rows, c.cols, c.R, ops.rc_vec_ok(aptr, pa.ld, pa.batch_stride, c.R), ops.rc_vec_ok(bptr, pb.ld, pb.batch_stride, c.R))
        out = _twice(launch, case["ref"].numel(), nb, dev)
    _same(out.values(out_shape), case["ref"], "%s on %s" % (tc.rc_id(c), rt), lambda idx, got: tc.rc_explain(c, idx, got))
    # the operands were only read
    assert torch.equal(abuf.cpu().view(torch.int32), pa.buf.view(torch.int32)) and torch.equal(bbuf.cpu().view(torch.int32), pb.buf.view(torch.int32))


# ------------------------------------------------------------------------------------------------ di2p_bmm_km
@pytest.mark.parametrize("c", tc.KM_CASES, ids=tc.km_id)
def test_bmm_km_is_exact(dev, c):
    from deepi2p_amd import _lib
    case = tc.km_case(c)
    (abuf, aptr), (bbuf, bptr) = _device(case["pa"], dev), _device(case["pb"], dev)
    pa, pb = case["pa"], case["pb"]

    def launch(out, ws):
        _lib.call("di2p_bmm_km", aptr, pa.ld, pa.batch_stride, bptr, pb.ld, pb.batch_stride, out.ptr, c.Z, c.rows, c.cols, c.K, c.alpha, _lib.stream())

    out = _twice(launch, c.Z * c.rows * c.cols, 0, dev)
    _same(out.values((c.Z, c.rows, c.cols)), case["ref"], tc.km_id(c), lambda idx, got: tc.km_explain(c, got))


# ------------------------------------------------------------------------------------------------ di2p_conv2d_wgrad
@pytest.mark.parametrize("c", tc.WGRAD_CASES, ids=tc.conv_id)
def test_conv2d_wgrad_is_exact(dev, c):
    from deepi2p_amd import _lib, ops
    case = tc.wgrad_case(c)
    x, dy = case["x"].to(dev), case["dy"].to(dev)
    OH, OW = tc.conv_out(c)
    nb = _lib.load().di2p_conv2d_wgrad_workspace_bytes(c.B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW, c.stride, c.pad)

    def launch(out, ws):
        _lib.call("di2p_conv2d_wgrad", x.data_ptr(), dy.data_ptr(), out.ptr, c.B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW, c.stride, c.pad, ws.ptr, ws.bytes,
                  _lib.stream())

    rt = ops.rc_route("wgrad", c.B, c.Cout, c.Cin * c.KH * c.KW, OH * OW, ops.rc_vec_ok(dy.data_ptr(), OH * OW, c.Cout * OH * OW, OH * OW))
    out = _twice(launch, case["ref"].numel(), nb, dev)
    coded = tuple(case["x"].shape) if c.family == "IDX" else tuple(case["dy"].shape)
    _same(out.values(case["ref"].shape), case["ref"], "%s on %s" % (tc.conv_id(c), rt), lambda idx, got: tc.conv_explain(c, got, coded))


# ------------------------------------------------------------------------------------------------ di2p_conv2d_dgrad
DGRAD_RUNS = [(c, dense) for c in tc.DGRAD_CASES for dense in ((0, 1) if c.stride == 2 else (0,))]


@pytest.mark.parametrize("c,dense", DGRAD_RUNS, ids=lambda v: tc.conv_id(v) if isinstance(v, tc.ConvCase) else ("dense" if v else "default"))
def test_conv2d_dgrad_is_exact(dev, c, dense):
    """every stride-2 case on the parity-class kernel and on the dense kernel: both against the reference, not only each other"""
    from deepi2p_amd import _lib
    case = tc.dgrad_case(c)
    dy, w = case["dy"].to(dev), case["w"].to(dev)

    def launch(out, ws):
        _lib.call("di2p_conv2d_dgrad", dy.data_ptr(), w.data_ptr(), out.ptr, c.B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW, c.stride, c.pad, _lib.stream())

    with _lib.option("conv_dgrad_dense", dense):
        out = _twice(launch, case["ref"].numel(), 0, dev)
    coded = tuple(case["dy"].shape) if c.family == "IDY" else tuple(case["w"].shape)
    kernel = "conv_dgrad_s2_kernel" if c.stride == 2 and not dense else "conv_dgrad_kernel"
    _same(out.values(case["ref"].shape), case["ref"], "%s on %s" % (tc.conv_id(c), kernel), lambda idx, got: tc.conv_explain(c, got, coded))


# ------------------------------------------------------------------------------------------------ di2p_gather_backward
@pytest.mark.parametrize("c", tc.GATHER_CASES, ids=tc.gather_id)
def test_gather_backward_is_exact(dev, c):
    from deepi2p_amd import _lib
    case = tc.gather_case(c)
    dy, idx = case["dy"].to(dev), case["idx"].to(dev)
    w = None if case["w"] is None else case["w"].to(dev)
    nb = _lib.load().di2p_gather_backward_workspace_bytes(c.B, c.C, c.J, c.M)

    def launch(out, ws):
        _lib.call("di2p_gather_backward", dy.data_ptr(), idx.data_ptr(), _lib.ptr(w), case["k"], out.ptr, c.B, c.C, c.J, c.M, ws.ptr, ws.bytes, _lib.stream())

    out = _twice(launch, case["ref"].numel(), nb, dev)
    got = out.values(case["ref"].shape)

    def explain(idx_, value):
        return " (as an id of dy %s: element %s)" % (tuple(case["dy"].shape), tc.decode(value, tuple(case["dy"].shape))) if c.family == "ID" else ""
    _same(got, case["ref"], tc.gather_id(c), explain)
    # nodes nobody references get exactly zero
    assert bool((got.cpu().transpose(1, 2)[case["unreferenced"]] == 0).all())


# ------------------------------------------------------------------------------------------------ di2p_channel_sum
@pytest.mark.parametrize("c", tc.SUM_CASES, ids=tc.sum_id)
def test_channel_sum_is_exact(dev, c):
    from deepi2p_amd import _lib
    x_cpu, ref = tc.sum_case(c)
    x = x_cpu.to(dev)
    nb = _lib.load().di2p_channel_reduce_workspace_bytes(c.B, c.C, c.N)

    def launch(out, ws):
        _lib.call("di2p_channel_sum", x.data_ptr(), out.ptr, c.B, c.C, c.N, ws.ptr, _lib.stream())

    out = _twice(launch, c.C, nb + (-nb) % 4, dev)
    _same(out.values((c.C,)), ref, tc.sum_id(c))


# ------------------------------------------------------------------------------------------------ error returns: all before any launch
def _refused(match, name, out, *args):
    """the call raises with `match` in its message and the NaN-filled output stays untouched (in a thread of its own: di2p_last_error is per
    thread, and other tests expect "ok" on the main thread)"""
    from deepi2p_amd import _lib

    def run():
        with pytest.raises(_lib.DeepI2PHipError, match=match):
            _lib.call(name, *args)
    with concurrent.futures.ThreadPoolExecutor(1) as ex:
        ex.submit(run).result()
    torch.cuda.synchronize()
    assert _untouched(out.buf), name + " wrote its output although it refused the call"


def test_workspace_one_byte_short_is_refused(dev):
    from deepi2p_amd import _lib, ops
    lib = _lib.load()
    st = _lib.stream()
    Z, rows, cols, R = 3, 5, 65, 772
    a, b = torch.ones(Z, rows, R, device=dev), torch.ones(Z, cols, R, device=dev)
    rt = ops.rc_route("strided", Z, rows, cols, R, ops.rc_vec_ok(a.data_ptr(), R, rows * R, R), ops.rc_vec_ok(b.data_ptr(), R, cols * R, R))
    need = Z * rt["chunks"] * rows * cols * 4
    assert need == lib.di2p_bmm_rc_workspace_bytes(Z, rows, cols, R)
    out, ws = _Out(Z * rows * cols, dev), _Workspace(need, dev)
    _refused("di2p_bmm_rc: workspace too small \\(%d bytes needed\\)" % need, "di2p_bmm_rc", out, a.data_ptr(), R, rows * R, b.data_ptr(), R, cols * R,
             out.ptr, Z, rows, cols, R, 1.0, 0, ws.ptr, need - 1, st)
    _refused("workspace too small", "di2p_bmm_rc", out, a.data_ptr(), R, rows * R, b.data_ptr(), R, cols * R, out.ptr, Z, rows, cols, R, 1.0, 0, None, need, st)
    assert _untouched(ws.buf)
    # the gather backward
    B, C, J, M = 3, 5, 772, 65
    idx = torch.zeros(B, J, 1, dtype=torch.int32, device=dev)
    need = lib.di2p_gather_backward_workspace_bytes(B, C, J, M)
    assert need == B * ops.rc_route("gather", B, C, M, J)["chunks"] * C * M * 4
    out, ws = _Out(B * C * M, dev), _Workspace(need, dev)
    _refused("di2p_gather_backward: workspace too small", "di2p_gather_backward", out, a.data_ptr(), idx.data_ptr(), None, 1, out.ptr, B, C, J, M, ws.ptr,
             need - 1, st)
    assert _untouched(ws.buf)
    # the convolution weight gradient
    x, dy = torch.ones(1, 3, 24, 24, device=dev), torch.ones(1, 5, 24, 24, device=dev)
    need = lib.di2p_conv2d_wgrad_workspace_bytes(1, 3, 24, 24, 5, 3, 3, 1, 1)
    assert need == 2 * 5 * 27 * 4
    out, ws = _Out(5 * 27, dev), _Workspace(need, dev)
    _refused("di2p_conv2d_wgrad: workspace too small", "di2p_conv2d_wgrad", out, x.data_ptr(), dy.data_ptr(), out.ptr, 1, 3, 24, 24, 5, 3, 3, 1, 1, ws.ptr,
             need - 1, st)
    assert _untouched(ws.buf)


def test_too_many_reduction_chunks_is_refused(dev):
    from deepi2p_amd import _lib
    Z = 65536
    a, b = torch.ones(Z, device=dev), torch.ones(Z, device=dev)
    need = _lib.load().di2p_bmm_rc_workspace_bytes(Z, 1, 1, 1)
    assert need == Z * 4
    for reduce_z in (0, 1):
        out, ws = _Out(Z, dev), _Workspace(need, dev)
        _refused("di2p_bmm_rc: too many reduction chunks", "di2p_bmm_rc", out, a.data_ptr(), 1, 1, b.data_ptr(), 1, 1, out.ptr, Z, 1, 1, 1, 1.0, reduce_z,
                 ws.ptr, need, _lib.stream())
        assert _untouched(ws.buf)


def test_gather_with_two_neighbours_is_refused(dev):
    from deepi2p_amd import _lib
    B, C, J, M = 1, 3, 33, 5
    dy, idx, w = torch.ones(B, C, J, device=dev), torch.zeros(B, J, 2, dtype=torch.int32, device=dev), torch.ones(B, J, 2, device=dev)
    need = _lib.load().di2p_gather_backward_workspace_bytes(B, C, J, M)
    out, ws = _Out(B * C * M, dev), _Workspace(need, dev)
    _refused("k must be 1", "di2p_gather_backward", out, dy.data_ptr(), idx.data_ptr(), w.data_ptr(), 2, out.ptr, B, C, J, M, ws.ptr, need, _lib.stream())
    assert _untouched(ws.buf)


def test_convolution_gradients_of_an_empty_output_are_refused(dev):
    from deepi2p_amd import _lib
    x, dy, w = torch.ones(1, 3, 2, 2, device=dev), torch.ones(1, 5, 1, 1, device=dev), torch.ones(5, 3, 3, 3, device=dev)
    # a 3 x 3 filter on a 2 x 2 input without padding: no output at any stride ((2 - 3) / stride + 1 is 1 in truncating division for stride > 1)
    for stride in (1, 2, 3):
        out, ws = _Out(5 * 27, dev), _Workspace(1024, dev)
        _refused("di2p_conv2d_wgrad: empty output", "di2p_conv2d_wgrad", out, x.data_ptr(), dy.data_ptr(), out.ptr, 1, 3, 2, 2, 5, 3, 3, stride, 0, ws.ptr,
                 1024, _lib.stream())
        assert _untouched(ws.buf)
        out = _Out(3 * 2 * 2, dev)
        _refused("di2p_conv2d_dgrad: empty output", "di2p_conv2d_dgrad", out, dy.data_ptr(), w.data_ptr(), out.ptr, 1, 3, 2, 2, 5, 3, 3, stride, 0,
                 _lib.stream())
