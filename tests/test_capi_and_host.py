"""CPU: the C-ABI library loads and exports every symbol include/deepi2p_hip.h declares (no compute calls without
a GPU); host-side logic (state-dict layout, weight packing, error behaviour) without touching the device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "deepi2p_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(di2p_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from deepi2p_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "missing export " + n
    # and the python binding covers exactly the declared ABI
    assert sorted(_lib.EXPORTS) == names
    l = _lib.load()
    assert l.di2p_version() >= 1 and l.di2p_last_error() == b"ok"
    assert l.di2p_solve_workspace_bytes(32, 60, 20480) >= 32 * 20480 * 32


def test_documented_knobs_are_the_knob_table():
    """csrc/common.h's DI2P_OPTIONS is the one definition of the knobs; the lists in include/deepi2p_hip.h and INTEGRATION.md name exactly
    its entries, and the library knows each of them under that name."""
    table = re.findall(r'\bX\((\w+), "(\w+)", "(\w+)", (-?\d+)\)', open(os.path.join(ROOT, "deepi2p_amd", "csrc", "common.h")).read())
    names = [name for _, name, _, _ in table]
    assert len(names) >= 20 and len(set(names)) == len(names)
    for ident, name, env, _ in table:
        assert name == ident.lower() and env == "DI2P_" + ident
    header = open(os.path.join(ROOT, "include", "deepi2p_hip.h")).read()
    comment = header[header.index("/* Tuning / test knobs"):header.index("int di2p_set_option(")]
    assert sorted(re.findall(r'"(\w+)"', comment)) == sorted(names)
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = guide[guide.index("The knobs ("):]
    listed = listed[listed.index("\n") + 1:listed.index(".\n")]
    assert sorted(re.findall(r"`(\w+)`", listed)) == sorted(names)
    # in a thread of its own: the unknown name below sets di2p_last_error, which is per thread
    import concurrent.futures
    from deepi2p_amd import _lib

    def known():
        for name in names:
            _lib.set_option(name, _lib.get_option(name))
        with pytest.raises(_lib.DeepI2PHipError, match="unknown option"):
            _lib.set_option("no_such_knob", 1)
    with concurrent.futures.ThreadPoolExecutor(1) as ex:
        ex.submit(known).result()


def test_argument_errors_are_reported_not_crashed():
    from deepi2p_amd import _lib
    l = _lib.load()
    with pytest.raises(_lib.DeepI2PHipError, match="k must be"):
        _lib.call("di2p_knn_nodes", None, None, None, None, 1, 10, 8, 99, None)
    with pytest.raises(_lib.DeepI2PHipError, match="null"):
        _lib.call("di2p_conv2d", None, None, None, None, None, None, 1, 3, 8, 8, 4, 3, 3, 1, 1, 0, 0, None)
    # empty problems are valid no-ops (edge cases: B == 0)
    _lib.call("di2p_ball_query_forward", None, None, 0.5, 4, 0, 3, 10, None)
    _lib.call("di2p_index_max_forward", None, None, None, 0, 4, 10, 8, None, None)


def test_conv2d_refuses_a_filter_that_does_not_fit_the_padded_input():
    # in a thread of its own: di2p_last_error is per thread
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(1) as ex:
        ex.submit(_conv2d_empty_output_checks).result()


def _conv2d_empty_output_checks():
    """A filter larger than the padded input has no output at ANY stride (C's truncating division gives (H + 2 pad - KH) / stride + 1 = 1
    for -stride < H + 2 pad - KH < 0): di2p_conv2d, di2p_conv2d_ws, di2p_conv2d_workspace_bytes and di2p_conv2d_route refuse it before any
    device call -- the addresses below are made up and never dereferenced."""
    from deepi2p_amd import _lib, ops
    lib = _lib.load()
    fake = 4096

    def conv(H, W, KH, KW, stride, pad, ws=False, Cin=3, Cout=4, tap_major=0):
        args = (fake, fake, fake, fake, None, fake, 1, Cin, H, W, Cout, KH, KW, stride, pad, 0, tap_major)
        if ws:
            _lib.call("di2p_conv2d_ws", *args, fake, 1 << 30, None)
        else:
            _lib.call("di2p_conv2d", *args, None)

    # (H, W, KH, KW, stride, pad): too tall, too wide, both; by one and by stride - 1; with padding that still does not reach
    empty = [(2, 8, 3, 3, 2, 0), (8, 2, 3, 3, 2, 0), (2, 2, 3, 3, 2, 0), (1, 8, 3, 1, 3, 0), (8, 4, 1, 7, 4, 1), (5, 5, 7, 7, 2, 0), (3, 3, 7, 7, 2, 1),
             (2, 8, 3, 3, 1, 0), (1, 1, 4, 4, 3, 1), (6, 6, 9, 9, 100, 1)]
    for H, W, KH, KW, stride, pad in empty:
        assert H + 2 * pad < KH or W + 2 * pad < KW
        for ws in (False, True):
            with pytest.raises(_lib.DeepI2PHipError, match="conv2d_impl: empty output"):
                conv(H, W, KH, KW, stride, pad, ws)
        assert lib.di2p_conv2d_workspace_bytes(1, 3, H, W, 4, KH, KW, stride, pad, 0) == 0
        with pytest.raises(_lib.DeepI2PHipError, match="di2p_conv2d_route: empty output"):
            ops.conv2d_route((1, 3, H, W), 4, KH, KW, stride, pad)
    # the same refusal on a shape that would split K (the workspace query must not size a workspace for it): Cin 512, Cout 128, tap-major
    assert lib.di2p_conv2d_workspace_bytes(1, 512, 2, 9, 128, 3, 3, 2, 0, 1) == 0
    assert lib.di2p_conv2d_workspace_bytes(1, 512, 3, 9, 128, 3, 3, 2, 0, 1) == 3 * 128 * 4 * 4       # ... and does for the smallest that fits
    with pytest.raises(_lib.DeepI2PHipError, match="empty output"):
        conv(2, 9, 3, 3, 2, 0, ws=True, Cin=512, Cout=128, tap_major=1)
    # a filter that exactly fits is one output pixel, at any stride: the route query answers (nothing is launched)
    for H, W, KH, KW, stride, pad in ((3, 3, 3, 3, 2, 0), (1, 1, 3, 3, 5, 1), (7, 7, 7, 7, 2, 0), (2, 3, 2, 3, 9, 0)):
        assert ops.conv2d_route((1, 3, H, W), 4, KH, KW, stride, pad)["kernel"] == 0


def test_pointwise_entry_points_share_their_argument_checks():
    # in a thread of its own: di2p_last_error is per thread, and the export test above expects "ok" on the main thread
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(1) as ex:
        ex.submit(_pointwise_argument_checks).result()


def _pointwise_argument_checks():
    """The five pointwise entry points marshal their sources and their epilogue through one function each (gemm.hip: pw_sources,
    pw_epilogue): every argument error carries the entry point's own name, and comes before any device call -- the addresses below are
    made up and never dereferenced."""
    from deepi2p_amd import _lib
    E, SrcT, EpilogueT = _lib.DeepI2PHipError, _lib.SrcT, _lib.EpilogueT
    fake = 4096                                  # 16-byte aligned; fake + 4: addr % 16 == 4
    B, N = 2, 256

    def srcs(*specs):                            # (channels, mode, gidx, group)
        arr = (SrcT * 4)()                       # room for the n_src = 4 case
        for i, (c, mode, gidx, group) in enumerate(specs):
            arr[i].ptr, arr[i].gidx, arr[i].batch_stride, arr[i].row_stride = fake, gidx, c * N, N
            arr[i].channels, arr[i].mode, arr[i].group = c, mode, group
        return arr

    dense = lambda c: (c, _lib.SRC_DENSE, None, 0)

    def epi(**kw):
        e = EpilogueT()
        e.group_max = 1
        for k, v in kw.items():
            if isinstance(v, tuple):
                for t, x in enumerate(v):
                    getattr(e, k)[t] = x
            else:
                setattr(e, k, v)
        return e

    # every entry point as f(sources, n_src, epilogue, B) on a shape it accepts: M = 128 (chain: 64), K = 64, N = 256
    def gemm(s, n, e, B=B):
        _lib.call("di2p_pointwise_gemm", s, n, fake, fake, B, 128, 64, N, ctypes.byref(e), None)

    def gemm_x3(s, n, e, B=B):
        _lib.call("di2p_pointwise_gemm_x3", s, n, fake, fake, B, 128, 64, N, ctypes.byref(e), None)

    def gemm_x3p(s, n, e, B=B):
        _lib.call("di2p_pointwise_gemm_x3p", fake, fake, fake, B, 128, 64, N, ctypes.byref(e), None)

    def head(s, n, e, B=B):
        _lib.call("di2p_point_head", ctypes.cast(s, ctypes.c_void_p), n, fake, 64, ctypes.cast(ctypes.pointer(e), ctypes.c_void_p), fake, None, None, 1,
                  fake, None, None, 0, fake, B, 128, 2, N, None)

    def chain(s, n, e, B=B):
        _lib.call("di2p_point_chain", ctypes.cast(s, ctypes.c_void_p), n, fake, 64, ctypes.cast(ctypes.pointer(e), ctypes.c_void_p), fake, None, None, 1,
                  None, None, None, 0, fake, B, 64, N, None)

    entries = {"di2p_pointwise_gemm": gemm, "di2p_pointwise_gemm_x3": gemm_x3, "di2p_pointwise_gemm_x3p": gemm_x3p, "di2p_point_head": head,
               "di2p_point_chain": chain}

    def fails(name, text, s, n, e):
        with pytest.raises(E, match=re.escape(": %s: %s" % (name, text))):
            entries[name](s, n, e)

    one = srcs(dense(64))
    # ---- sources
    for name in ("di2p_pointwise_gemm", "di2p_pointwise_gemm_x3"):
        fails(name, "source channels do not sum to K", srcs(dense(32), dense(16)), 2, epi())
        fails(name, "gather source without index", srcs((64, _lib.SRC_GATHER, None, 0)), 1, epi())
        fails(name, "group source without group", srcs((64, _lib.SRC_GROUP, None, 0)), 1, epi())
        fails(name, "1..3 sources", one, 0, epi())
        fails(name, "1..3 sources", srcs(dense(16), dense(16), dense(16), dense(16)), 4, epi())
    fails("di2p_point_head", "source channels do not sum to K0", srcs(dense(32), dense(16)), 2, epi())
    fails("di2p_point_head", "fused head: dense sources only", srcs((64, _lib.SRC_GATHER, None, 0)), 1, epi())
    fails("di2p_point_head", "fused head: dense sources only", srcs((64, _lib.SRC_GROUP, None, 0)), 1, epi())
    fails("di2p_point_head", "null pointer", one, 0, epi())
    fails("di2p_point_head", "null pointer", srcs(dense(16), dense(16), dense(16), dense(16)), 4, epi())
    odd = srcs(dense(64))
    odd[0].ptr = fake + 4
    fails("di2p_point_head", "sources must be 16-byte addressable", odd, 1, epi())
    fails("di2p_point_chain", "fused chain: one dense source", one, 0, epi())
    fails("di2p_point_chain", "fused chain: one dense source of K0 channels", srcs((64, _lib.SRC_GATHER, None, 0)), 1, epi())
    # ---- epilogue
    for name in entries:
        fails(name, "g_k must be in [0, DI2P_MAX_GK]", one, 1, epi(g_table=(fake,), g_idx=(fake,), g_nodes=(8,), g_k=(17,)))
        fails(name, "gathered table without index / k / nodes", one, 1, epi(g_table=(fake,), g_nodes=(8,), g_k=(3,)))
        fails(name, "gathered tables must be 16-byte aligned", one, 1, epi(g_table=(fake + 4,), g_idx=(fake,), g_nodes=(8,), g_k=(3,)))
        entries[name](one, 1, epi(), B=0)                                    # an empty batch stays a valid no-op
    for name in ("di2p_pointwise_gemm", "di2p_pointwise_gemm_x3", "di2p_pointwise_gemm_x3p"):
        for g in (3, 64):
            fails(name, "group_max must be a power of two <= 32 dividing N", one, 1, epi(group_max=g))
    for name, what in (("di2p_point_head", "fused head"), ("di2p_point_chain", "fused chain")):
        for kw in (dict(group_max=16), dict(transpose_out=1), dict(planes_out=fake)):
            fails(name, what + ": layer 0 takes scale/shift/relu/bias/gathered only", one, 1, epi(**kw))
    fails("di2p_pointwise_gemm", "planes_out: only the bf16x3 entry points write split planes", one, 1, epi(planes_out=fake))
    # the bf16x3 kernels read the per-row operands 16 bytes at a time
    for name in ("di2p_pointwise_gemm_x3", "di2p_pointwise_gemm_x3p"):
        for field in ("scale", "shift", "batch_bias"):
            fails(name, "scale, shift and batch_bias must be 16-byte aligned", one, 1, epi(**{field: fake + 4}))


def test_host_side_shape_queries_of_the_bf16x3_entry_points_with_cfg():
    """Pure host logic behind the C ABI (no device needed): which shapes the round-5 kernels take, and the sizes of their packed operands.
    ABI 8: di2p_conv3x3_x3_supported takes the tile configuration (-1: the knob conv_x3_cfg, by default the cost model's choice)."""
    from deepi2p_amd import _lib
    lib = _lib.load()
    # stem + pool in one launch: H % 4 == 0, W % 128 == 0, W <= 512 (include/deepi2p_hip.h)
    assert lib.di2p_stem_x3_supported(160, 512) == 1 and lib.di2p_stem_x3_supported(4, 128) == 1
    for H, W in ((30, 512), (160, 640), (160, 192), (0, 128), (2, 128)):
        assert lib.di2p_stem_x3_supported(H, W) == 0, (H, W)
    assert lib.di2p_stem_x3_packed_bytes() == 11 * 2 * 3 * 64 * 16           # [K-step][channel tile][plane][lane] x 16 B
    # the head's fragment-ordered weights: [K / 16][4 row tiles][3 planes][64 lanes] x 16 B
    assert lib.di2p_head_x3_packed_bytes(96) == 6 * 4 * 3 * 1024 and lib.di2p_head_x3_packed_bytes(128) == 8 * 4 * 3 * 1024
    assert lib.di2p_head_x3_packed_bytes(100) == 0                           # K % 16 != 0: nothing to pack
    # the seven 3x3 layer shapes of ResNet-34 at 160 x 512 have a bf16x3 instance; odd sizes under stride 2 and Cin < 16 do not
    for Cin, H, W, Cout, s in ((64, 40, 128, 64, 1), (128, 20, 64, 128, 1), (256, 10, 32, 256, 1), (512, 5, 16, 512, 1),
                               (64, 40, 128, 128, 2), (128, 20, 64, 256, 2), (256, 10, 32, 512, 2)):
        assert lib.di2p_conv3x3_x3_supported(32, Cin, H, W, Cout, s, -1) == 1, (Cin, H, W, Cout, s)
    assert lib.di2p_conv3x3_x3_supported(32, 64, 41, 128, 128, 2, -1) == 0 and lib.di2p_conv3x3_x3_supported(32, 8, 40, 128, 64, 1, -1) == 0
    assert lib.di2p_conv3x3_x3_supported(1, 64, 40, 128, 64, 1, -1) == lib.di2p_conv3x3_x3_supported(64, 64, 40, 128, 64, 1, -1) == 1     # batch independent
    # a forced configuration answers for itself: 0 and 1 tile 32-pixel segments (OW = 16 does not divide), 2 and 3 16-pixel ones
    assert lib.di2p_conv3x3_x3_supported(32, 512, 5, 16, 512, 1, 0) == lib.di2p_conv3x3_x3_supported(32, 512, 5, 16, 512, 1, 1) == 0
    assert lib.di2p_conv3x3_x3_supported(32, 512, 5, 16, 512, 1, 2) == lib.di2p_conv3x3_x3_supported(32, 512, 5, 16, 512, 1, 3) == 1
    assert lib.di2p_conv3x3_x3_supported(32, 64, 40, 128, 64, 1, 4) == lib.di2p_conv3x3_x3_supported(32, 64, 40, 128, 64, 1, -2) == 0


def test_no_cpu_fallback_paths():
    from deepi2p_amd import ball_query, index_max, ops
    x = torch.zeros(1, 2, 8)
    idx = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        index_max.forward_cuda_shared_mem(x, idx, 4)
    with pytest.raises(NotImplementedError):
        index_max.forward_cpu(x, idx, 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        ball_query.forward_cuda_shared_mem(torch.zeros(1, 2, 8), 0.1, 2)
    with pytest.raises(RuntimeError):
        ops.knn_nodes(torch.zeros(1, 3, 8), torch.zeros(1, 3, 4), 2)
    if not torch.cuda.is_available():
        from deepi2p_amd import FrustumRegistration
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FrustumRegistration.solvePGivenK(np.zeros((3, 4)), np.zeros(4, np.int32), np.eye(3), 0.0, np.zeros(3), 160, 512,
                                             [-1, -1, -1], [1, 1, 1], 5, False, True)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "deepi2p_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("the oracle", "").replace("oracle's", "").replace("oracle/", "") \
                    or not f.endswith(".py"), f
                if f.endswith(".py"):
                    assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f


def test_state_dict_layout_and_packing():
    from deepi2p_amd import networks
    from oracle import network_torch as nt
    opt = nt.OptLike(256, 64, 64, True)
    det = networks.KeypointDetector(opt)
    spec = nt.state_dict_spec(opt)
    sd = det.state_dict()
    assert list(sd.keys()) == [k for k, _ in spec] and len(sd) == 361
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in spec)
    syn = nt.synthetic_state_dict(opt)
    det.load_state_dict(syn)
    # BN folding used by every kernel epilogue: y = scale * conv + shift == BN(conv + bias)
    Wt, scale, shift, act = networks._fold(syn, "pc_encoder.first_pointnet.layers.0.conv", "pc_encoder.first_pointnet.layers.0.norm")
    x = torch.randn(5, 7)
    ref = torch.nn.functional.batch_norm(x @ syn["pc_encoder.first_pointnet.layers.0.conv.weight"][:, :, 0].t()
                                         + syn["pc_encoder.first_pointnet.layers.0.conv.bias"],
                                         syn["pc_encoder.first_pointnet.layers.0.norm.running_mean"],
                                         syn["pc_encoder.first_pointnet.layers.0.norm.running_var"],
                                         syn["pc_encoder.first_pointnet.layers.0.norm.weight"],
                                         syn["pc_encoder.first_pointnet.layers.0.norm.bias"], False, 0.0, 1e-5)
    torch.testing.assert_close((x @ Wt) * scale + shift, ref, rtol=1e-5, atol=1e-6)
    assert act and Wt.shape == (7, 32)
    # last layers have no norm: identity scale, shift = bias, no activation
    Wt2, sc2, sh2, act2 = networks._fold(syn, "per_point_pn.layers.2.conv", "per_point_pn.layers.2.norm")
    assert sc2 is None and not act2 and torch.equal(sh2, syn["per_point_pn.layers.2.conv.bias"])
    # repacking is invalidated by load_state_dict
    det._packed = {"stale": True}
    det.load_state_dict(syn)
    assert det._packed is None
    # 'module.'-prefixed checkpoints (util/pytorch_helper.py:24-33)
    conv = networks.model_state_dict_convert_auto({"module." + k: v for k, v in syn.items()})
    assert list(conv.keys()) == list(syn.keys())


def test_shard_ranges():
    from deepi2p_amd.distributed import shard_range
    for n in (0, 1, 7, 60, 128, 256):
        for world in (1, 2, 3, 8):
            parts = [shard_range(n, r, world) for r in range(world)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in parts]
            assert max(sizes) - min(sizes) <= 1


def test_classifier_checkpoint_and_lr_helpers(tmp_path):
    """save_network / load_model / update_learning_rate of the MMClassifer mirror (multimodal_classifier.py:75-80,263-277): host logic
    only -- the 361-key state_dict round-trips through a file, the learning-rate rule clips at 1e-5."""
    import torch
    from deepi2p_amd import synthetic
    from deepi2p_amd.networks import MMClassifer
    opt = synthetic.OptLike(256, 32, 64, True)
    opt.device, opt.checkpoints_dir, opt.lr = torch.device("cpu"), str(tmp_path), 1e-3
    m = MMClassifer(opt)
    sd = synthetic.random_state_dict(opt, 1)
    m.detector.load_state_dict(sd)
    m.save_network(m.detector, "gpu0_0_net_detector.pth")
    m2 = MMClassifer(opt)
    m2.load_model(str(tmp_path / "gpu0_0_net_detector.pth"))
    got = m2.detector.state_dict()
    assert set(got) == set(sd) and len(got) == 361
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    m.update_learning_rate(0.5)
    assert abs(m.old_lr_detector - 5e-4) < 1e-12
    m.update_learning_rate(1e-6)
    assert m.old_lr_detector == 0.00001
