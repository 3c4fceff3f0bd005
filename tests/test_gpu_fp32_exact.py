"""GPU: the fp32-MFMA inference kernels -- di2p_pointwise_gemm, di2p_conv2d / _ws, di2p_conv3x3_winograd with both weight transforms,
di2p_attention_pool, di2p_batch_gemv / _gemv2, di2p_point_chain, di2p_point_head, di2p_conv7x7s2_stem with its packer -- on operands for which their arithmetic is exact (tests/fp32_exact_cases.py;
the bounds are proven on the CPU by tests/test_fp32_exact_cases_host.py).  Every case
  * re-asserts on the device's own pointers the kernel instance the library's routing query names,
  * runs twice and must equal the fp64 reference, and itself, bit for bit,
  * writes into a NaN-filled buffer whose guard bands must stay NaN (dense sources of the pointwise cases live in NaN-filled buffers too),
  * and must give a frame alone what the frame gets in its batch.
A mismatch names the first differing index, what the identity-coded families decode it to, and whether it lies in the last tile."""
import ctypes
import types

import pytest
import torch

from tests import fp32_exact_cases as fc

pytestmark = pytest.mark.gpu


def _same(got, ref, what, decode_shape=None, tiles=None):
    """got (device or CPU) equals ref (fp64 or fp32) bit for bit; tiles: (axis, tile, name) triples for the message"""
    got, ref = got.detach().cpu(), ref.float()
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(ref.shape))
    idx = fc.first_mismatch(got, ref)
    if idx is not None:
        where = ["in the last %s tile" % name for axis, tile, name in (tiles or ()) if idx[axis] >= (ref.shape[axis] - 1) // tile * tile]
        dec = ""
        if decode_shape is not None:
            dec = "; as ids: read %s instead of %s of %s" % (fc.decode(got[idx], decode_shape), fc.decode(ref[idx], decode_shape), tuple(decode_shape))
        raise AssertionError("%s: first differing index %s of %s (got %r, expected %r; %d of %d differ)%s %s" % (
            what, idx, tuple(ref.shape), float(got[idx]), float(ref[idx]), int((got != ref).sum()), ref.numel(), dec, ", ".join(where)))
    assert torch.equal(got, ref)


def _out(dev, shape):
    buf, view = fc.guarded(shape)
    buf = buf.to(dev)
    n = view.numel()
    return buf, buf[fc.GUARD:fc.GUARD + n].view(*shape)


def _guards_intact(buf, what):
    g = torch.cat([buf[:fc.GUARD], buf[-fc.GUARD:]]).cpu()
    assert bool(torch.isnan(g).all()), "%s: wrote outside its output (%d guard floats changed)" % (what, int((~torch.isnan(g)).sum()))


# ===================================================================================================== di2p_pointwise_gemm
def _pw_sources(dev, _lib, c, d, frames):
    """the case's sources on the device (dense ones as strided views of NaN-filled buffers, gaps checked afterwards) -> (Src-like list, placed)"""
    out, placed = [], []
    for kind, t, gi, grp in d["parts"]:
        t = t[frames]
        if kind == "dense":
            p = fc.place(t, c.layout)
            buf = p.buf.to(dev)
            view = buf.as_strided(tuple(t.shape), (p.batch_stride, p.ld, 1), p.offset)
            placed.append((buf, p, tuple(t.shape)))
            out.append(types.SimpleNamespace(t=view, mode=_lib.SRC_DENSE, gidx=None, group=1))
        elif kind == "gather":
            out.append(types.SimpleNamespace(t=t.to(dev), mode=_lib.SRC_GATHER, gidx=gi[frames].contiguous().to(dev), group=1))
        else:
            out.append(types.SimpleNamespace(t=t.to(dev), mode=_lib.SRC_GROUP, gidx=None, group=grp))
    return out, placed


def _pw_run(dev, c, d, frames=slice(None)):
    """one di2p_pointwise_gemm launch of the case's frames -> list of (output on the device, fp64 reference) and the route it must have taken"""
    from deepi2p_amd import _lib, ops
    B, M, K, N = len(range(c.B)[frames]), c.M, c.K, c.N
    srcs, placed = _pw_sources(dev, _lib, c, d, frames)
    Wt = d["w"].t().contiguous().to(dev)
    kw = d["kw"]
    keep = [Wt, srcs]
    e = _lib.EpilogueT()
    for name in ("scale", "shift", "batch_bias"):
        t = kw.get(name)
        if t is not None:
            t = (t[frames] if name == "batch_bias" else t).contiguous().to(dev)
            keep.append(t)
        setattr(e, name, _lib.ptr(t))
    gm = kw.get("group_max", 1)
    e.relu, e.group_max, e.transpose_out = int(bool(kw.get("relu"))), gm, int(bool(kw.get("transpose_out")))
    gathered = [tuple(None if t is None else t[frames].contiguous().to(dev) for t in tab) for tab in kw.get("gathered", [])]
    ops._fill_gathered(e, gathered, B, M, N)
    keep.append(gathered)
    refs = d["ref"] if isinstance(d["ref"], tuple) else (d["ref"],)
    outs = [_out(dev, (B,) + tuple(r.shape[1:])) for r in refs]
    if kw.get("also_full"):
        e.group_max_out = _lib.ptr(outs[1][1])
    dense = all(s.mode == _lib.SRC_DENSE and s.t.stride(1) % 4 == 0 and s.t.stride(0) % 4 == 0 and s.t.data_ptr() % 16 == 0 for s in srcs)
    with fc.knobs(((c.knob, 1),) if c.knob else ()):
        rt = ops.pointwise_route(M, K, N, B, dense, Wt.data_ptr() % 16 == 0)
        _lib.call("di2p_pointwise_gemm", ops._fill_srcs(srcs), len(srcs), _lib.ptr(Wt), _lib.ptr(outs[0][1]), B, M, K, N, ctypes.byref(e), _lib.stream())
    torch.cuda.synchronize()
    for buf, p, shape in placed:          # the kernel wrote nothing into its sources' buffers
        mask = torch.ones_like(p.buf, dtype=torch.bool)
        mask.as_strided(shape, (p.batch_stride, p.ld, 1), p.offset).fill_(False)
        assert bool(torch.isnan(buf.cpu()[mask]).all()), "a source buffer's NaN gaps were written"
    return outs, [r[frames] for r in refs], rt


@pytest.mark.parametrize("c", fc.PW_CASES, ids=fc.pw_id)
def test_pointwise_gemm_is_exact(dev, c):
    d = fc.pw_case(c)
    what = fc.pw_id(c)
    outs, refs, rt = _pw_run(dev, c, d)
    assert rt == d["route"], "%s: on the device the route is %s, the case table expects %s" % (what, rt, d["route"])
    dec = {"IDA": (c.B, c.K, d["parts"][0][1].shape[2]), "IDB": (c.M, c.K)}.get(c.family)          # the ids of the stored source / of the weights
    tiles = None if c.epi in ("transpose", "gmax8") else ((1, rt["bm"], "M"), (2, rt["bn"], "N"))
    for (buf, y), ref in zip(outs, refs):
        _same(y, ref, what, dec, tiles)
        _guards_intact(buf, what)
    again, _, _ = _pw_run(dev, c, d)
    for (_, y), (_, y2) in zip(outs, again):
        assert torch.equal(y.cpu(), y2.cpu()), what + ": two runs differ"
    alone, refs1, _ = _pw_run(dev, c, d, slice(1, 2))
    for (buf, y), ref in zip(alone, refs1):
        _same(y, ref, what + " (frame 1 alone)", None, tiles)
        _guards_intact(buf, what + " (frame 1 alone)")


# ===================================================================================================== di2p_conv2d / di2p_conv2d_ws
def _conv_run(dev, c, d, frames=slice(None)):
    from deepi2p_amd import _lib, ops
    B = len(range(c.B)[frames])
    x = d["x"][frames].contiguous()
    xbuf = torch.full((x.numel() + 8,), fc.NAN)
    xbuf[c.xoff:c.xoff + x.numel()] = x.reshape(-1)
    xbuf = xbuf.to(dev)
    xv = xbuf[c.xoff:c.xoff + x.numel()].view(*x.shape)
    Wt, scale, shift = d["Wt"].to(dev), d["scale"].to(dev), d["shift"].to(dev)
    res = None if d["residual"] is None else d["residual"][frames].contiguous().to(dev)
    ref = d["ref"][frames]
    buf, y = _out(dev, tuple(ref.shape))
    need, given = fc.conv_ws_bytes(c, B)
    ws = torch.empty((max(given, 16),), dtype=torch.uint8, device=dev) if given else None
    args = (_lib.ptr(xv), _lib.ptr(Wt), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res), _lib.ptr(y), B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW, c.stride,
            c.pad, int(d["relu"]), int(c.tap_major))
    with fc.knobs(((c.knob, 1),) if c.knob else ()):
        rt = ops.conv2d_route((B, c.Cin, c.H, c.W), c.Cout, c.KH, c.KW, c.stride, c.pad, c.tap_major, x_aligned=xv.data_ptr() % 16 == 0,
                              wt_aligned=Wt.data_ptr() % 16 == 0, workspace_bytes=given if ws is not None and ws.data_ptr() % 16 == 0 else 0)
        if c.ws == "none":
            _lib.call("di2p_conv2d", *args, _lib.stream())
        else:
            _lib.call("di2p_conv2d_ws", *args, _lib.ptr(ws), given, _lib.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(torch.cat([xbuf[:c.xoff], xbuf[c.xoff + x.numel():]]).cpu()).all())
    return buf, y, ref, rt


@pytest.mark.parametrize("c", fc.CONV_CASES, ids=fc.conv_id)
def test_conv2d_is_exact(dev, c):
    d = fc.conv_case(c)
    what = fc.conv_id(c)
    buf, y, ref, rt = _conv_run(dev, c, d)
    assert rt == d["route"], "%s: on the device the route is %s, the case table expects %s" % (what, rt, d["route"])
    dec = tuple(d["x"].shape) if c.family == "TID" else None
    got = y.cpu()
    idx = fc.first_mismatch(got, ref.float())
    if idx is not None:
        OH, OW = ref.shape[2:]
        border = idx[2] in (0, OH - 1) or idx[3] in (0, OW - 1)
        pix = (idx[0] * OH + idx[2]) * OW + idx[3]
        Ntot = c.B * OH * OW
        where = "%sborder pixel; %slast M tile; %slast N tile" % ("" if border else "no ", "" if idx[1] >= (c.Cout - 1) // rt["bm"] * rt["bm"] else "not the ",
                                                                 "" if pix >= (Ntot - 1) // rt["bn"] * rt["bn"] else "not the ")
        _same(y, ref, what + " [" + where + "]", dec)
    _guards_intact(buf, what)
    _, y2, _, _ = _conv_run(dev, c, d)
    assert torch.equal(got, y2.cpu()), what + ": two runs differ"
    buf1, y1, ref1, _ = _conv_run(dev, c, d, slice(1, 2))
    _same(y1, ref1, what + " (frame 1 alone)", dec)
    _guards_intact(buf1, what + " (frame 1 alone)")


# ===================================================================================================== di2p_conv3x3_winograd
def _wino_run(dev, c, d, frames=slice(None)):
    from deepi2p_amd import _lib, ops
    x = d["x"][frames].contiguous().to(dev)
    B = x.shape[0]
    scale, shift = d["scale"].to(dev), d["shift"].to(dev)
    res = None if d["residual"] is None else d["residual"][frames].contiguous().to(dev)
    ref = d["ref"][frames]
    buf, y = _out(dev, tuple(ref.shape))
    with fc.knobs(c.knobs):
        U = (ops.winograd_weights_dgrad if c.dgrad else ops.winograd_weights)(d["weight"].to(dev))
        rt = ops.winograd_route((B, c.Cin, c.H, c.W), c.Cout)
        _lib.call("di2p_conv3x3_winograd", _lib.ptr(x), _lib.ptr(U), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res), _lib.ptr(y), B, c.Cin, c.H, c.W,
                  c.Cout, int(d["relu"]), _lib.stream())
    torch.cuda.synchronize()
    return buf, y, ref, rt, U


@pytest.mark.parametrize("c", fc.WINO_CASES, ids=fc.wino_id)
def test_conv3x3_winograd_is_exact(dev, c):
    d = fc.wino_case(c)
    what = fc.wino_id(c)
    buf, y, ref, rt, U = _wino_run(dev, c, d)
    assert rt == fc.wino_route(c), "%s: on the device the route is %s, the case table expects %s" % (what, rt, fc.wino_route(c))
    _same(U, fc.wino_pipeline(d["x"][:1], d["w"])[0], what + ": the transformed filter U = G g G^T")
    _same(y, ref, what, None, ((1, rt["cob"], "output-channel"),))
    _guards_intact(buf, what)
    _, y2, _, _, _ = _wino_run(dev, c, d)
    assert torch.equal(y.cpu(), y2.cpu()), what + ": two runs differ"
    buf1, y1, ref1, _, _ = _wino_run(dev, c, d, slice(1, 2))
    _same(y1, ref1, what + " (frame 1 alone)")
    _guards_intact(buf1, what + " (frame 1 alone)")


# ===================================================================================================== di2p_attention_pool
def _attn_run(dev, c, d, frames=slice(None)):
    from deepi2p_amd import _lib
    feat, score = d["feat"][frames].contiguous().to(dev), d["score"][frames].contiguous().to(dev)
    ref = d["ref"][frames]
    buf, y = _out(dev, tuple(ref.shape))
    _lib.call("di2p_attention_pool", _lib.ptr(feat), _lib.ptr(score), _lib.ptr(y), feat.shape[0], c.C, c.HW, c.Mn, _lib.stream())
    torch.cuda.synchronize()
    return buf, y, ref


@pytest.mark.parametrize("c", fc.ATTN_CASES, ids=fc.attn_id)
def test_attention_pool_is_exact(dev, c):
    d = fc.attn_case(c)
    what = fc.attn_id(c)
    buf, y, ref = _attn_run(dev, c, d)
    _same(y, ref, what, None, ((1, 64, "C"), (2, 64, "Mn")))
    _guards_intact(buf, what)
    assert torch.equal(y.cpu(), _attn_run(dev, c, d)[1].cpu()), what + ": two runs differ"
    buf1, y1, ref1 = _attn_run(dev, c, d, slice(1, 2))
    _same(y1, ref1, what + " (frame 1 alone)")
    _guards_intact(buf1, what + " (frame 1 alone)")


# ===================================================================================================== di2p_batch_gemv / di2p_batch_gemv2
def _gemv_run(dev, c, d, frames=slice(None)):
    from deepi2p_amd import _lib
    Wt = d["Wt"].to(dev)
    v = d["v"][frames].contiguous().to(dev)
    ref = d["ref"][frames]
    buf, y = _out(dev, tuple(ref.shape))
    if c.Kv1:
        v1 = d["v1"][frames].contiguous().to(dev)
        _lib.call("di2p_batch_gemv2", _lib.ptr(Wt), c.M, c.k0, _lib.ptr(v), c.Kv, c.k1, _lib.ptr(v1), c.Kv1, _lib.ptr(y), v.shape[0], _lib.stream())
    else:
        _lib.call("di2p_batch_gemv", _lib.ptr(Wt), c.M, c.k0, _lib.ptr(v), c.Kv, _lib.ptr(y), v.shape[0], _lib.stream())
    torch.cuda.synchronize()
    return buf, y, ref


@pytest.mark.parametrize("c", fc.GEMV_CASES, ids=fc.gemv_id)
def test_batch_gemv_is_exact(dev, c):
    d = fc.gemv_case(c)
    what = fc.gemv_id(c)
    buf, y, ref = _gemv_run(dev, c, d)
    _same(y, ref, what, tuple(d["Wt"].shape) if c.family == "IDB" and not c.Kv1 else None, ((1, 64, "M"),))
    _guards_intact(buf, what)
    assert torch.equal(y.cpu(), _gemv_run(dev, c, d)[1].cpu()), what + ": two runs differ"
    buf1, y1, ref1 = _gemv_run(dev, c, d, slice(1, 2))
    _same(y1, ref1, what + " (frame 1 alone)")
    _guards_intact(buf1, what + " (frame 1 alone)")


# ===================================================================================================== di2p_point_chain
def _chain_operands(dev, d, frames):
    layers = [(w.t().contiguous().to(dev), None if sc is None else sc.to(dev), None if sh is None else sh.to(dev), relu) for w, sc, sh, relu in d["layers"]]
    kw = {}
    if "batch_bias" in d["kw"]:
        kw["batch_bias"] = d["kw"]["batch_bias"][frames].contiguous().to(dev)
    if "gathered" in d["kw"]:
        kw["gathered"] = [tuple(t[frames].contiguous().to(dev) for t in tab) for tab in d["kw"]["gathered"]]
    return d["x"][frames].contiguous().to(dev), layers, kw


def _chain_run(dev, c, d, frames=slice(None)):
    from deepi2p_amd import _lib, ops
    x, layers, kw = _chain_operands(dev, d, frames)
    B, N = x.shape[0], d["N"]
    (W0, sc0, sh0, r0), (W1, sc1, sh1, r1) = layers[0], layers[1]
    W2, sc2, sh2, r2 = layers[2] if len(layers) == 3 else (None, None, None, False)
    e = _lib.EpilogueT()
    e.scale, e.shift, e.batch_bias = _lib.ptr(sc0), _lib.ptr(sh0), _lib.ptr(kw.get("batch_bias"))
    e.relu, e.group_max, e.transpose_out = int(bool(r0)), 1, 0
    ops._fill_gathered(e, kw.get("gathered"), B, c.M, N)
    ref = d["outs"][-1][frames]
    buf, y = _out(dev, tuple(ref.shape))
    _lib.call("di2p_point_chain", ops._fill_srcs([ops.Src(x)]), 1, _lib.ptr(W0), c.K0, ctypes.byref(e), _lib.ptr(W1), _lib.ptr(sc1), _lib.ptr(sh1),
              int(bool(r1)), _lib.ptr(W2), _lib.ptr(sc2), _lib.ptr(sh2), int(bool(r2)), _lib.ptr(y), B, c.M, N, _lib.stream())
    torch.cuda.synchronize()
    return buf, y, ref


@pytest.mark.parametrize("c", fc.CHAIN_CASES, ids=fc.chain_id)
def test_point_chain_is_exact(dev, c):
    from deepi2p_amd import ops
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    N = c.N or fc.chain_uneven_n(c.M, c.K0, c.layers, c.B, cus)
    d = fc.chain_case(c, N)
    what = fc.chain_id(c) + " (N = %d)" % N
    assert max(d["bounds"]) < fc.LIMIT, what          # the per-layer bound of the shape THIS device runs (CPU tensors)
    rt = fc.chain_route(c, cus, N)
    assert (rt["M"], rt["ks0"], rt["layers"]) in fc.CHAIN_INSTANCES
    if not c.N:
        assert rt["total"] % (4 * rt["wgs"]) and rt["total"] > 4 * rt["wgs"], "%s: the trips are equal on %d compute units (%s)" % (what, cus, rt)
    buf, y, ref = _chain_run(dev, c, d)
    _same(y, ref, what, tuple(d["x"].shape) if c.family == "ID" else None, ((2, 32 * rt["tn"], "N"),))
    _guards_intact(buf, what)
    assert torch.equal(y.cpu(), _chain_run(dev, c, d)[1].cpu()), what + ": two runs differ"
    # the documented promise: the same bits as the separate pointwise_gemm launches on the same operands
    x, layers, kw = _chain_operands(dev, d, slice(None))
    v = ops.pointwise_gemm([ops.Src(x)], layers[0][0], c.M, N, scale=layers[0][1], shift=layers[0][2], relu=layers[0][3], **kw)
    for Wt, sc, sh, relu in layers[1:]:
        v = ops.pointwise_gemm([ops.Src(v)], Wt, c.M, N, scale=sc, shift=sh, relu=relu)
    assert torch.equal(y.cpu(), v.cpu()), what + ": the chain differs from the separate launches"
    buf1, y1, ref1 = _chain_run(dev, c, d, slice(1, 2))
    _same(y1, ref1, what + " (frame 1 alone)")
    _guards_intact(buf1, what + " (frame 1 alone)")


# ===================================================================================================== di2p_point_head
def _head_operands(dev, d, frames):
    srcs = [t[frames].contiguous().to(dev) for t in d["srcs"]]
    gathered = [tuple(None if t is None else t[frames].contiguous().to(dev) for t in tab) for tab in d["gathered"]]
    dv = {k: (None if d[k] is None else d[k].to(dev)) for k in ("W0", "W1", "sc0", "sh0", "sc1", "sh1", "sc2", "sh2")}
    return srcs, gathered, dv


def _head_run(dev, c, d, N, W2, ref, frames=slice(None)):
    from deepi2p_amd import _lib, ops
    srcs, gathered, v = _head_operands(dev, d, frames)
    B = srcs[0].shape[0]
    W2 = W2.contiguous().to(dev)
    e = _lib.EpilogueT()
    e.scale, e.shift, e.batch_bias = _lib.ptr(v["sc0"]), _lib.ptr(v["sh0"]), None
    e.relu, e.group_max, e.transpose_out = int(bool(d["relu0"])), 1, 0
    ops._fill_gathered(e, gathered, B, 128, N)
    ref = ref[frames]
    buf, y = _out(dev, tuple(ref.shape))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    with fc.knobs((("head_reg", c.reg),)):
        rt = ops.point_head_route(c.K0, len(srcs), srcs[0].shape[1], B, N, cus, g33=len(gathered) == 2 and all(g[1].shape[2] == 3 for g in gathered),
                                  reg_range=all(t.shape[1] * t.stride(1) * 4 < 1 << 31 for t in srcs))
        _lib.call("di2p_point_head", ops._fill_srcs([ops.Src(t) for t in srcs]), len(srcs), _lib.ptr(v["W0"]), c.K0, ctypes.byref(e), _lib.ptr(v["W1"]),
                  _lib.ptr(v["sc1"]), _lib.ptr(v["sh1"]), int(bool(d["relu1"])), _lib.ptr(W2), _lib.ptr(v["sc2"]), _lib.ptr(v["sh2"]), int(bool(d["relu2"])),
                  _lib.ptr(y), B, 128, c.P, N, _lib.stream())
    torch.cuda.synchronize()
    return buf, y, ref, rt


@pytest.mark.parametrize("c", fc.HEAD_CASES, ids=fc.head_id)
def test_point_head_is_exact(dev, c):
    from deepi2p_amd import ops
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    N = c.N or fc.head_uneven_n(c.B, cus)
    d = fc.head_case(c, N)
    what = fc.head_id(c) + " (N = %d)" % N
    for name, _, bound in d["stages"]:
        assert float(bound.max()) < fc.LIMIT, "%s: stage %s" % (what, name)          # the per-layer bounds of the shape THIS device runs
    want = fc.head_route(c, cus, N)
    if not c.N:
        assert not want["reg"] or (want["total"] > 8 * want["wgs"] and want["total"] % (8 * want["wgs"])), "%s: equal trips (%s)" % (what, want)
    for i, (W2, ref) in enumerate(d["tails"]):
        buf, y, ref, rt = _head_run(dev, c, d, N, W2, ref)
        assert rt == want, "%s: on the device the route is %s, the case table expects %s" % (what, rt, want)
        _same(y, ref, what + ", output layer %d" % i, None, ((2, rt["bn"], "N"),))
        _guards_intact(buf, what)
    W2, ref = d["tails"][0]
    _, y, _, rt = _head_run(dev, c, d, N, W2, ref)
    assert torch.equal(y.cpu(), _head_run(dev, c, d, N, W2, ref)[1].cpu()), what + ": two runs differ"
    # the documented promise: the same bits as the three separate pointwise_gemm launches on the same operands
    srcs, gathered, v = _head_operands(dev, d, slice(None))
    h = ops.pointwise_gemm([ops.Src(t) for t in srcs], v["W0"], 128, N, scale=v["sc0"], shift=v["sh0"], relu=d["relu0"], gathered=gathered or None, x3=False)
    h = ops.pointwise_gemm([ops.Src(h)], v["W1"], 128, N, scale=v["sc1"], shift=v["sh1"], relu=d["relu1"], x3=False)
    h = ops.pointwise_gemm([ops.Src(h)], W2.contiguous().to(dev), c.P, N, scale=v["sc2"], shift=v["sh2"], relu=d["relu2"], x3=False)
    assert torch.equal(y.cpu(), h.cpu()), what + ": the fused head differs from the separate launches"
    buf1, y1, ref1, _ = _head_run(dev, c, d, N, W2, ref, slice(1, 2) if c.B > 1 else slice(0, 1))
    _same(y1, ref1, what + " (one frame alone)")
    _guards_intact(buf1, what + " (one frame alone)")


# ===================================================================================================== di2p_conv7x7s2_stem, di2p_stem_pack
def _stem_run(dev, c, d, frames=slice(None)):
    from deepi2p_amd import _lib, ops
    x = d["x"][frames].contiguous().to(dev)
    Wp = ops.stem_weights(d["w"].to(dev))
    scale, shift = d["scale"].to(dev), d["shift"].to(dev)
    ref = d["ref"][frames]
    buf, y = _out(dev, tuple(ref.shape))
    _lib.call("di2p_conv7x7s2_stem", _lib.ptr(x), _lib.ptr(Wp), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), x.shape[0], c.H, c.W, int(d["relu"]), _lib.stream())
    torch.cuda.synchronize()
    return buf, y, ref, Wp


@pytest.mark.parametrize("c", fc.STEM_CASES, ids=fc.stem_id)
def test_conv7x7s2_stem_is_exact(dev, c):
    d = fc.stem_case(c)
    what = fc.stem_id(c)
    buf, y, ref, Wp = _stem_run(dev, c, d)
    _same(Wp, fc.stem_packed(d["w"]), what + ": the packed filter bank")
    got = y.cpu()
    idx = fc.first_mismatch(got, ref.float())
    if idx is not None:
        OH, OW = ref.shape[2:]
        where = "border pixel: %s; last row pair: %s; last 128-pixel column tile: %s" % (
            idx[2] in (0, OH - 1) or idx[3] in (0, OW - 1), idx[2] >= (OH - 1) // 2 * 2, idx[3] >= (OW - 1) // 128 * 128)
        _same(y, ref, what + " [" + where + "]")
    _guards_intact(buf, what)
    assert torch.equal(got, _stem_run(dev, c, d)[1].cpu()), what + ": two runs differ"
    buf1, y1, ref1, _ = _stem_run(dev, c, d, slice(1, 2))
    _same(y1, ref1, what + " (frame 1 alone)")
    _guards_intact(buf1, what + " (frame 1 alone)")


def test_stem_pack_copies_any_float(dev):
    """the packer moves bit patterns: arbitrary normal finite floats arrive unchanged, the padding tap kx = 7 is zero"""
    from deepi2p_amd import ops
    w = fc.any_floats((64, 3, 7, 7), fc._gen("stem pack"))
    _same(ops.stem_weights(w.to(dev)), fc.stem_packed(w), "stem_weights")
