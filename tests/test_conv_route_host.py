"""CPU: ops.conv_route, the one statement of which kernel runs a convolution layer (inference network, training forward, training input gradient).
The table pins its answers for every 3x3 layer shape of ResNet-34 at a 160 x 512 image under default knobs.  Its entries were recorded from the
dispatch code this function replaced (ImageEncoder.forward's ladder, train_net's _conv_forward and the three-branch ladder of _Conv2d.backward,
run on meta tensors with the kernel wrappers replaced by recorders), not from conv_route."""
import pytest

X3, X3_SMALL, WINO, TAP = ("x3", -1), ("x3", 3), ("winograd", None), ("direct_tap", None)
# (B, Cin, H, W, Cout, stride): (inference, training forward, training input gradient; None: the strided layers' gradient is di2p_conv2d_dgrad)
TABLE = {
    (8, 64, 40, 128, 64, 1): (X3, WINO, WINO),
    (8, 128, 20, 64, 128, 1): (X3, WINO, WINO),
    (8, 256, 10, 32, 256, 1): (X3, X3_SMALL, X3_SMALL),
    (8, 512, 5, 16, 512, 1): (X3, X3_SMALL, X3_SMALL),
    (8, 64, 40, 128, 128, 2): (X3, TAP, None),
    (8, 128, 20, 64, 256, 2): (X3, TAP, None),
    (8, 256, 10, 32, 512, 2): (X3, TAP, None),
    (16, 64, 40, 128, 64, 1): (X3, X3, X3),
    (16, 128, 20, 64, 128, 1): (X3, X3, X3),
    (16, 256, 10, 32, 256, 1): (X3, X3, X3),
    (16, 512, 5, 16, 512, 1): (X3, X3, X3),
    (16, 64, 40, 128, 128, 2): (X3, TAP, None),
    (16, 128, 20, 64, 256, 2): (X3, TAP, None),
    (16, 256, 10, 32, 512, 2): (X3, TAP, None),
    (32, 64, 40, 128, 64, 1): (X3, X3, X3),
    (32, 128, 20, 64, 128, 1): (X3, X3, X3),
    (32, 256, 10, 32, 256, 1): (X3, X3, X3),
    (32, 512, 5, 16, 512, 1): (X3, X3, X3),
    (32, 64, 40, 128, 128, 2): (X3, TAP, None),
    (32, 128, 20, 64, 256, 2): (X3, TAP, None),
    (32, 256, 10, 32, 512, 2): (X3, TAP, None),
}


def _routes(B, Cin, H, W, Cout, stride):
    """(inference, training forward, training input gradient) of the 3x3 / pad 1 layer: the gradient is the route of dY with Cin, Cout swapped"""
    from deepi2p_amd import ops
    xs, ws = (B, Cin, H, W), (Cout, Cin, 3, 3)
    dgrad = ops.conv_route((B, Cout, H, W), (Cin, Cout, 3, 3), 1, 1, training=True) if stride == 1 else None
    return ops.conv_route(xs, ws, stride, 1), ops.conv_route(xs, ws, stride, 1, training=True), dgrad


def test_resnet34_layers_under_default_knobs():
    for key, want in TABLE.items():
        assert _routes(*key) == want, key


def test_the_rule_outside_the_table():
    from deepi2p_amd import ops
    # what other tests assert of `supported`, seen through the route
    for cfg in range(4):
        assert ops.conv3x3_x3_supported((2, 64, 8, 64), 128, 1, cfg=cfg) == (cfg < 2)
        assert ops.conv3x3_x3_supported((1, 512, 5, 16), 512, 1, cfg=cfg) == (cfg >= 2)
    assert _routes(2, 64, 8, 64, 128, 1) == (X3, WINO, WINO)                  # two frames of 128 channels: training stays on Winograd
    assert _routes(16, 64, 8, 64, 128, 1) == (X3, X3, X3)
    assert _routes(1, 512, 5, 16, 512, 1) == (X3, X3_SMALL, X3_SMALL)
    assert _routes(1, 64, 8, 24, 64, 1) == (WINO, WINO, WINO)                 # width no multiple of 16: no x3 instance
    assert _routes(1, 64, 8, 23, 64, 1) == (TAP, TAP, TAP)                    # odd width: not Winograd either
    assert _routes(1, 64, 8, 2, 64, 1) == (TAP, TAP, TAP)                     # ... nor a width below 4
    assert _routes(1, 64, 8, 24, 24, 1)[:2] == (TAP, TAP)                     # Cout % 32 != 0
    assert _routes(1, 8, 8, 32, 64, 1)[:2] == (("direct", None),) * 2        # Cin % 16 != 0: the plain matrix
    assert _routes(1, 64, 7, 32, 64, 2)[:2] == (TAP, TAP)                     # odd height at stride 2: no x3 instance
    assert _routes(32, 64, 40, 128, 128, 2)[1] == TAP                         # training never routes a strided layer to x3
    # other filter sizes: by Cin only
    for ws, stride, pad in (((64, 3, 7, 7), 2, 3), ((64, 3, 7, 7), 1, 3)):
        assert ops.conv_route((8, 3, 160, 512), ws, stride, pad, training=True) == ("direct", None)
    for training in (False, True):
        assert ops.conv_route((32, 64, 40, 128), (128, 64, 1, 1), 2, 0, training=training) == TAP
        assert ops.conv_route((32, 64, 40, 128), (64, 64, 3, 3), 1, 0, training=training) == TAP      # 3x3 without its padding


def test_knob_conv_x3():
    from deepi2p_amd import _lib
    with _lib.option("conv_x3", 0):
        for key in TABLE:
            assert all(r is None or r[0] != "x3" for r in _routes(*key)), key
        assert _routes(32, 64, 40, 128, 64, 1) == (WINO, WINO, WINO) and _routes(32, 64, 40, 128, 128, 2)[0] == TAP
    with _lib.option("conv_x3", 16 | 2):                   # bit 4: the strided layers; bit s-1: Cout = 64 << (s-1)
        assert [_routes(32, C, 8, 64, C, 1)[0][0] for C in (64, 128, 256, 512)] == ["winograd", "x3", "winograd", "winograd"]
        assert _routes(32, 64, 40, 128, 128, 2)[0] == X3
    with _lib.option("conv_x3", 15):
        assert _routes(32, 64, 40, 128, 128, 2)[0] == TAP and _routes(32, 64, 40, 128, 64, 1)[0] == X3


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_knob_conv_x3_cfg(k):
    """A forced configuration: the route passes cfg = -1 (the knob decides in the library) and asks `supported` under the knob."""
    from deepi2p_amd import _lib, ops
    with _lib.option("conv_x3_cfg", k):
        for key in list(TABLE) + [(2, 64, 8, 64, 128, 1), (1, 512, 5, 16, 512, 1)]:
            B, Cin, H, W, Cout, stride = key
            for r in _routes(*key):
                assert r is None or r[0] != "x3" or r == X3, (key, r)
            on = ops.conv3x3_x3_supported((B, Cin, H, W), Cout, stride, cfg=k)
            assert ops.conv3x3_x3_supported((B, Cin, H, W), Cout, stride) == on
            assert (_routes(*key)[0] == X3) == on, key
        assert (_routes(1, 512, 5, 16, 512, 1)[1] == X3) == (k >= 2)
        assert (_routes(2, 64, 8, 64, 128, 1)[0] == X3) == (k < 2)


def test_knob_conv_nowinograd_is_read_by_inference_only():
    from deepi2p_amd import _lib
    key = (1, 64, 8, 24, 64, 1)
    assert _routes(*key) == (WINO, WINO, WINO)
    with _lib.option("conv_nowinograd", 1):
        assert _routes(*key) == (TAP, WINO, WINO)
        assert _routes(8, 64, 40, 128, 64, 1) == TABLE[(8, 64, 40, 128, 64, 1)]              # (x3 in inference; training as before)
        with _lib.option("conv_x3", 0):
            assert _routes(8, 64, 40, 128, 64, 1) == (TAP, WINO, WINO)
