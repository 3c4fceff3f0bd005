"""GPU: the product launches what ops.conv_route names.  Entry points are counted with the per-launch hook of _lib.call (_lib.TIMED), for
train_net._Conv2d (forward + input gradient) on the smallest shapes that separate the branches of the rule, and for a whole ImageEncoder.forward;
and the two fall-back wrappers every route can land on (ops.conv2d, ops.conv3x3_winograd) refuse malformed operands before any launch."""
from collections import Counter

import pytest
import torch

from deepi2p_amd import _lib

pytestmark = pytest.mark.gpu

ENTRY = {"x3": "di2p_conv3x3_x3", "winograd": "di2p_conv3x3_winograd", "direct_tap": "di2p_conv2d", "direct": "di2p_conv2d"}
X3, X3_SMALL, WINO, TAP, DIRECT = ("x3", -1), ("x3", 3), ("winograd", None), ("direct_tap", None), ("direct", None)


def _launches(fn):
    """fn() with the launch hook on: (fn's result, {entry point: calls}) -- di2p_conv2d_ws (split-K with a workspace) counts as di2p_conv2d"""
    _lib.TIMED = {name: [] for name in ("di2p_conv3x3_x3", "di2p_conv3x3_winograd", "di2p_conv2d", "di2p_conv2d_ws")}
    try:
        out = fn()
        torch.cuda.synchronize()
        n = {name: len(v) for name, v in _lib.TIMED.items()}
    finally:
        _lib.TIMED = None
    n["di2p_conv2d"] += n.pop("di2p_conv2d_ws")
    return out, n


def _counts(routes):
    n = Counter({"di2p_conv3x3_x3": 0, "di2p_conv3x3_winograd": 0, "di2p_conv2d": 0})
    n.update(ENTRY[kernel] for kernel, _ in routes)
    return dict(n)


# x shape, Cout: the route of (inference, training forward, training input gradient)
CASES = [((2, 64, 8, 64), 128, X3, WINO, WINO),              # training: two frames of 128 channels stay on Winograd (the batch rule)
         ((16, 64, 8, 64), 128, X3, X3, X3),
         ((1, 512, 5, 16), 512, X3, X3_SMALL, X3_SMALL),      # few frames: the smallest tile configuration, forward and input gradient
         ((1, 64, 8, 24), 64, WINO, WINO, WINO),              # a width that is no multiple of 16
         ((1, 64, 8, 23), 64, TAP, TAP, TAP),                 # an odd width
         ((1, 8, 8, 32), 64, DIRECT, DIRECT, TAP)]            # Cin % 16 != 0 (the gradient contracts over Cout = 64)


@pytest.mark.parametrize("xs,Cout,infer,fwd,dgrad", CASES)
def test_training_conv_launches_the_routed_kernels(dev, xs, Cout, infer, fwd, dgrad):
    from deepi2p_amd import ops, train_net as tn
    B, Cin, H, W = xs
    ws = (Cout, Cin, 3, 3)
    assert ops.conv_route(xs, ws, 1, 1) == infer
    assert ops.conv_route(xs, ws, 1, 1, training=True) == fwd
    assert ops.conv_route((B, Cout, H, W), (Cin, Cout, 3, 3), 1, 1, training=True) == dgrad
    g = torch.Generator().manual_seed(Cin + W)
    x = torch.randn(xs, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(ws, generator=g) / (9 * Cin) ** 0.5).to(dev).requires_grad_(True)
    y, n = _launches(lambda: tn._Conv2d.apply(x, w, 1, 1))
    assert n == _counts([fwd]), (n, fwd)
    dy = torch.randn(y.shape, generator=g).to(dev)
    _, n = _launches(lambda: y.backward(dy))
    assert n == _counts([dgrad]), (n, dgrad)                  # (the weight gradient is di2p_conv2d_wgrad: none of the routed kernels)
    assert x.grad is not None and w.grad is not None


@pytest.mark.parametrize("knobs", [{}, {"conv_x3": 0}, {"conv_x3": 0, "conv_nowinograd": 1}], ids=["default", "conv_x3=0", "direct only"])
def test_image_encoder_launches_the_routed_kernels(dev, knobs):
    """One ImageEncoder.forward at B = 1 on a 32 x 128 image: per entry point, as many launches as walking its blocks with conv_route predicts."""
    from contextlib import ExitStack
    from deepi2p_amd import ops, synthetic as nt
    from deepi2p_amd.networks import ImageEncoder
    opt = nt.OptLike(1024, 32, 128, False)
    sd = {k[len("img_encoder."):]: v for k, v in nt.synthetic_state_dict(opt).items() if k.startswith("img_encoder.")}
    enc = ImageEncoder(opt)
    enc.load_state_dict(sd)
    enc = enc.to(dev)
    img = torch.rand(1, 3, 32, 128, generator=torch.Generator().manual_seed(2)).to(dev) * 255
    with ExitStack() as st:
        for name, v in knobs.items():
            st.enter_context(_lib.option(name, v))
        routes, shape = [], (1, 64, 8, 32)                   # the stem's output: 64 channels at a quarter of the image
        for blk in enc._pack()["blocks"]:
            Cout, s = blk["c1"][0].shape[1], blk["stride"]
            r1 = ops.conv_route(shape, (Cout, shape[1], 3, 3), s, 1)
            routes.append(r1)
            if "ds" in blk and not (r1[0] == "x3" and s == 2):            # the 1x1 branch: a launch of its own unless fused into the x3 launch
                routes.append(TAP)
            shape = (1, Cout, (shape[2] - 1) // s + 1, (shape[3] - 1) // s + 1)
            routes.append(ops.conv_route(shape, (Cout, Cout, 3, 3), 1, 1))
        out, n = _launches(lambda: enc(img))
    assert n == _counts(routes), (n, Counter(routes))
    assert sum(n.values()) >= 32 and tuple(out[1].shape) == (1, 512, 1, 4)
    if knobs.get("conv_nowinograd"):
        assert n["di2p_conv3x3_x3"] == n["di2p_conv3x3_winograd"] == 0
    elif not knobs:
        assert min(n.values()) > 0, n                          # this image size meets all three kernels


def _zero_launches(fn, match):
    """fn() raises a host-side RuntimeError (not the library's refusal) and nothing was launched"""
    def run():
        with pytest.raises(RuntimeError, match=match) as e:
            fn()
        assert not isinstance(e.value, _lib.DeepI2PHipError)
    _, n = _launches(run)
    assert not any(n.values()), n


def test_fallback_wrappers_reject_malformed_operands(dev):
    """A malformed operand is never smaller than the right one (a missed check could not read out of bounds), except the short scale."""
    from deepi2p_amd import ops
    B, Cin, H, W, Cout = 1, 32, 6, 8, 64
    x = torch.zeros(B, Cin, H, W, device=dev)
    Wt, U = torch.zeros(9 * Cin, Cout, device=dev), torch.zeros(16, Cin, Cout, device=dev)
    one, res = torch.ones(Cout, device=dev), torch.zeros(B, Cout, H, W, device=dev)

    def conv(x=x, Wt=Wt, scale=one, shift=one, residual=res):
        return ops.conv2d(x, Wt, scale, shift, 3, 3, 1, 1, True, residual=residual, tap_major=True)

    def wino(x=x, U=U, scale=one, shift=one, residual=res):
        return ops.conv3x3_winograd(x, U, scale, shift, True, residual=residual)

    (_, _), n = _launches(lambda: (conv(), wino()))
    assert n == {"di2p_conv3x3_x3": 0, "di2p_conv3x3_winograd": 1, "di2p_conv2d": 1}          # the well-formed calls run
    for f, weight in ((conv, "Wt"), (wino, "U")):
        _zero_launches(lambda: f(x=x.double()), "input must be torch.float32")
        _zero_launches(lambda: f(x=x.view(B * Cin, H, W)), r"takes x f32\[B,Cin,H,W\]")
        _zero_launches(lambda: f(scale=one[:Cout - 1]), "scale holds 63 values, needs 64")
        _zero_launches(lambda: f(shift=one.double()), "shift must be torch.float32")
        _zero_launches(lambda: f(residual=torch.zeros(B, Cout, H + 2, W, device=dev)), "residual must be")
        _zero_launches(lambda: f(residual=res.double()), "residual must be torch.float32")
        bigger = torch.zeros(9 * 2 * Cin, Cout, device=dev) if weight == "Wt" else torch.zeros(16, 2 * Cin, Cout, device=dev)
        _zero_launches(lambda: f(**{weight: bigger}), weight + " must be")
        _zero_launches(lambda: f(**{weight: (Wt if weight == "Wt" else U).double()}), weight + " must be torch.float32")
