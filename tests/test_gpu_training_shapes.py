"""Every layer of the training step at the real training shapes (batch 8, 20480 points, 160 x 512, coarse + fine heads: bench.py --mode train)
against float64.

tests/test_gpu_training.py compares each autograd Function of deepi2p_amd/train_net.py with torch at toy shapes, where most of the production
dispatch never runs (the bf16x3 3x3 layers, the 128 x 128 weight-gradient tiles, the reduction plans of R = 8 x 20480), and the whole step only
through a loose bound set by the train-mode BatchNorm's ill-conditioning.  Here one real forward of the step is recorded -- every call of every
Function subclass of train_net, with its shapes, flags and integer operands -- and each distinct call is replayed in isolation on fresh seeded
floats: output and every input / parameter gradient against torch.autograd of the plain op in float64.

  bar          max |HIP - fp64| / max |fp64| <= max(floor, 4 * e32), e32 = torch's own fp32 CPU evaluation of the same op against the same
               reference; the floors are the per-op tolerances of tests/test_gpu_training.py
  sensitivity  every reduction-shaped gradient (weight gradients, bias sums, BatchNorm d gamma / d beta, gather / interpolate / attention
               backward): the fp64 contribution of the last 32 reduction indices of the last frame -- the final k-tile of the last, ragged
               chunk -- is at least 3 x the bar, so a kernel that lost that tile fails
  determinism  every replay runs twice: bit-identical outputs and gradients
  coverage     the kernel path of each case from the library's own predicates; the recorded step must reach every path listed in REQUIRED
  knobs        rc_tile64, bn_unfused, pw_x3, conv_x3, conv_x3_cfg, conv_dgrad_dense on the same recorded cases; the stride-1 3x3 layers of
               stages 1 and 2 at batch 16 (where ops.conv_route takes every stage)

Run with -s for the per-case table and the coverage manifest.
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_STEP, N_STEP, H_STEP, W_STEP = 8, 20480, 160, 512
TAIL = 32                                        # one k-tile of the reduction GEMMs (RC_BK)
FLOOR = {"_Linear": 2e-5, "_Conv2d": 3e-5, "_BatchNorm": 5e-5}
DEFAULT_FLOOR = 2e-5
# positions of the differentiable arguments of each Function's apply (all other tensors are recorded operands)
GRADS = {"_Linear": (0, 1, 2), "_Conv2d": (0, 1), "_BatchNorm": (0, 1, 2, 7), "_AttentionPool": (0, 1)}
# gradients that are reductions over the output positions (the sensitivity check applies)
REDUCED = {"_Linear": (1, 2), "_Conv2d": (1,), "_BatchNorm": (1, 2), "_GatherCols": (0,), "_Interpolate": (0,), "_AttentionPool": (0,)}
# argument names for the table
ARGN = {"_Linear": ("x", "W", "b"), "_Conv2d": ("x", "W"), "_BatchNorm": ("x", "gamma", "beta", None, None, None, None, "res"),
        "_AttentionPool": ("feat", "score")}
REQUIRED = ("x3 conv fwd", "x3 conv dgrad", "winograd conv fwd", "winograd conv dgrad", "s2 parity dgrad", "tap-major direct conv fwd",
            "stem conv fwd, not tap-major", "conv wgrad im2col", "rc_gemm128", "rc_gemm 64-tile", "gather bwd k=1",
            "gather bwd k=3", "bf16x3 linear fwd", "bf16x3 linear dx", "fp32 linear fwd")
GPU_REF_MACS = 1 << 30          # point layers with more multiply-adds than this take their fp64 reference as a float64 matmul on the GPU


# ------------------------------------------------------------------------------------------------ recording the step
def _function_classes(tn):
    return sorted(n for n, v in vars(tn).items()
                  if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == tn.__name__)


def _snapshot(name, args):
    """Per argument: ("f", shape) a differentiable float input (replayed fresh), ("stat", shape) a BatchNorm running buffer (fresh),
    ("t", clone) an operand replayed as recorded (indices, masks, interpolation weights), ("v", value) a Python value or None."""
    spec = []
    for pos, a in enumerate(args):
        if torch.is_tensor(a):
            if name == "_BatchNorm" and pos in (3, 4):
                spec.append(("stat", tuple(a.shape)))
            elif a.is_floating_point() and pos in GRADS.get(name, (0,)):
                spec.append(("f", tuple(a.shape)))
            else:
                spec.append(("t", a.detach().clone()))
        else:
            spec.append(("v", a))
    return spec


def _signature(name, spec):
    return (name,) + tuple((k, tuple(v.shape), str(v.dtype)) if k == "t" else (k, v) for k, v in spec)


@pytest.fixture(scope="module")
def step():
    """One train-mode forward of the step at the training configuration with every Function's apply wrapped: the distinct calls."""
    from deepi2p_amd import synthetic, train_net as tn
    opt = synthetic.OptLike(N_STEP, H_STEP, W_STEP, True)
    P = {k: v.to(DEV) for k, v in synthetic.random_state_dict(opt, 0).items()}
    b = synthetic.make_batch(2000, B_STEP, N=N_STEP, H=H_STEP, W=W_STEP)
    t = [torch.from_numpy(np.ascontiguousarray(b[k])).to(DEV) for k in ("pc", "intensity", "sn", "node_a", "node_b", "img")]
    masks = [tn.dropout_mask((B_STEP, c, N_STEP), 0.5, 0, i, DEV) for i, c in enumerate(tn.head_widths(P))]
    names = _function_classes(tn)
    calls = []

    def wrap(name, orig):
        def apply(*args):
            calls.append((name, _snapshot(name, args)))
            return orig(*args)
        return staticmethod(apply)

    with pytest.MonkeyPatch.context() as mp:
        for n in names:
            cls = getattr(tn, n)
            mp.setattr(cls, "apply", wrap(n, cls.apply))
        scores = tn.keypoint_detector(P, opt, *t, dropouts=masks)
    torch.cuda.synchronize()
    assert tuple(scores.shape) == (B_STEP, 2 + 80, N_STEP)
    cases, seen = [], {}
    for name, spec in calls:
        sig = _signature(name, spec)
        if sig in seen:
            seen[sig]["count"] += 1
            continue
        case = dict(op=name, spec=spec, seed=len(cases), count=1, key="step%d" % len(cases))
        seen[sig] = case
        cases.append(case)
    return dict(names=names, calls=len(calls), cases=cases)


# ------------------------------------------------------------------------------------------------ one case: inputs, HIP, references
def _fresh(op, pos, shape, g):
    v = torch.randn(shape, generator=g)
    if op == "_Linear" and pos == 1:
        return v / float(np.prod(shape[1:])) ** 0.5
    if op == "_Linear" and pos == 2:
        return 0.1 * v
    if op == "_Conv2d" and pos == 1:
        return v / float(np.prod(shape[1:])) ** 0.5
    if op == "_BatchNorm":
        return {0: v * 2 + 0.5, 1: torch.rand(shape, generator=g) + 0.5, 2: 0.1 * v}.get(pos, v)
    if op in ("_SegmentMax", "_GroupMax", "_MaxPool"):
        return torch.relu(v)                     # the step feeds them ReLU outputs: exact zeros, ties inside the windows / groups
    return v


def _inputs(case):
    if "inputs" not in case:
        g = torch.Generator().manual_seed(1000 + case["seed"])
        vals = {pos: _fresh(case["op"], pos, v, g) for pos, (k, v) in enumerate(case["spec"]) if k == "f"}
        if case["op"] == "_BatchNorm" and case["spec"][6][1] and 7 in vals:
            # relu(bn(x) + res) has a kink at 0 where the two summands cancel: a pre-activation within fp32 rounding of it switches its
            # gradient on in one precision and off in the other (an error of one whole cotangent, for torch's fp32 as for the kernel).
            # Moving the residual of those few elements 1e-4 away from the kink leaves the batch statistics as they are.
            z = F.batch_norm(vals[0].double(), None, None, vals[1].double(), vals[2].double(), True, 0.1, 1e-5) + vals[7].double()
            near = z.abs() < 1e-4
            vals[7][near] += torch.where(z[near] >= 0, 2e-4, -2e-4).float()
        case["inputs"] = vals
    return case["inputs"]


def _cotangent(case, shape):
    g = torch.Generator().manual_seed(5000 + case["seed"])
    return torch.randn(shape, generator=g, dtype=torch.float64)


def _args(case, device, dtype):
    leaves, args = [], []
    vals = _inputs(case)
    for pos, (k, v) in enumerate(case["spec"]):
        if k == "f":
            t = vals[pos].to(device=device, dtype=dtype, copy=True).requires_grad_(True)
            leaves.append((pos, t))
            args.append(t)
        elif k == "stat":
            args.append((torch.zeros if pos == 3 else torch.ones)(v, dtype=dtype, device=device))
        elif k == "t":
            args.append(v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device))
        else:
            args.append(v)
    return leaves, args


def _knobs(knobs):
    from deepi2p_amd import _lib
    stack = contextlib.ExitStack()
    for name, value in (knobs or {}).items():
        stack.enter_context(_lib.option(name, value))
    return stack


def _hip(case, knobs=None):
    """Forward + backward of the library's Function on DEV -> [output, gradient of each differentiable argument] (fp32, on DEV)."""
    from deepi2p_amd import train_net as tn
    leaves, args = _args(case, DEV, torch.float32)
    with _knobs(knobs):
        y = getattr(tn, case["op"]).apply(*args)
        y.backward(_cotangent(case, tuple(y.shape)).float().to(DEV))
    torch.cuda.synchronize()
    return [y.detach()] + [t.grad for _, t in leaves]


def _ref_linear(a):
    x, W, b = a[0], a[1], a[2]
    y = torch.matmul(W.reshape(W.shape[0], -1), x)
    return y + b[:, None] if b is not None else y


def _ref_bn(a):
    x, gamma, beta, _, _, momentum, relu, res = a
    y = F.batch_norm(x, None, None, gamma, beta, True, momentum, 1e-5)
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


def _ref_segment_max(a):
    from oracle.network_torch import index_max_torch
    d, index, Ma, mask = a
    gi = index_max_torch(d.detach().float(), index, Ma)
    return d.gather(2, gi) * mask.unsqueeze(1)


def _ref_gather(a):
    x, idx = a
    return x.gather(2, idx.long().unsqueeze(1).expand(x.shape[0], x.shape[1], idx.shape[1]))


def _ref_interpolate(a):
    f, idx, w = a
    B, C, _ = f.shape
    J = idx.shape[1]
    return sum(f.gather(2, idx[:, :, k].long().unsqueeze(1).expand(B, C, J)) * w[:, :, k].unsqueeze(1) for k in range(idx.shape[2]))


REF = {
    "_Linear": _ref_linear,
    "_Conv2d": lambda a: F.conv2d(a[0], a[1], None, stride=a[2], padding=a[3]),
    "_BatchNorm": _ref_bn,
    "_SegmentMax": _ref_segment_max,
    "_GatherCols": _ref_gather,
    "_Interpolate": _ref_interpolate,
    "_GroupMax": lambda a: a[0].max(dim=-1)[0],
    "_AttentionPool": lambda a: torch.bmm(a[0], a[1]) / a[0].shape[2],
    "_MaxPool": lambda a: F.max_pool2d(a[0], 3, 2, 1),
    "_AvgPool": lambda a: F.adaptive_avg_pool2d(a[0], (1, 1)),
    "_Dropout": lambda a: a[0] * a[1].to(a[0].dtype) * a[2],
}


def _ref_device(case):
    if case["op"] == "_Linear":
        (B, K, N), M = case["spec"][0][1], case["spec"][1][1][0]
        if B * K * M * N > GPU_REF_MACS:
            return DEV                           # float64 matmul (no MIOpen involved); the convolutions stay on the CPU
    return "cpu"


def _err(a, r):
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    return float((a - r).abs().max()) / max(float(r.abs().max()), 1e-30)


_REF_CACHE = {}


def _reference(case):
    """fp64 output and gradients (CPU), torch's fp32 CPU error e32 per tensor, the bars, and the tail sensitivity of the reduced gradients."""
    if case["key"] in _REF_CACHE:
        return _REF_CACHE[case["key"]]
    op = case["op"]
    dev = _ref_device(case)
    leaves, args = _args(case, dev, torch.float64)
    y = REF[op](args)
    ct = _cotangent(case, tuple(y.shape)).to(dev)
    grads = torch.autograd.grad(y, [t for _, t in leaves], ct, retain_graph=True)
    ref = [y.detach().cpu()] + [g.cpu() for g in grads]
    names = ["out"] + [(ARGN.get(op, ("x",))[p] or "arg%d" % p) for p, _ in leaves]
    # the contribution of the last TAIL output positions of the last frame (the reduction's final k-tile) to each reduced gradient
    sens = {}
    red = [(i + 1, t) for i, (p, t) in enumerate(leaves) if p in REDUCED.get(op, ())]
    if red:
        mask = torch.zeros_like(ct)
        mask.view(ct.shape[0], ct.shape[1], -1)[-1, :, -TAIL:] = 1.0
        tails = torch.autograd.grad(y, [t for _, t in red], ct * mask)
        for (i, _), tg in zip(red, tails):
            sens[i] = float(tg.abs().max()) / max(float(ref[i].abs().max()), 1e-30)
    del y, grads, args, leaves
    # torch's own fp32 evaluation on the CPU
    leaves, args = _args(case, "cpu", torch.float32)
    y = REF[op](args)
    g32 = torch.autograd.grad(y, [t for _, t in leaves], ct.cpu().float())
    e32 = [_err(a, r) for a, r in zip([y] + list(g32), ref)]
    floor = FLOOR.get(op, DEFAULT_FLOOR)
    out = dict(ref=ref, names=names, e32=e32, bars=[max(floor, 4.0 * e) for e in e32], sens=sens, ref_dev=dev)
    if op in ("_Linear", "_Conv2d", "_AttentionPool"):       # the knob variants replay these against the same reference
        _REF_CACHE[case["key"]] = out
    return out


# ------------------------------------------------------------------------------------------------ kernel paths (the library's own predicates)
def _rc_path(rows, cols, R):
    """di2p_bmm_rc on fresh (16-byte aligned) operands contiguous along R: rc_vec_ok and rc_big of train.hip."""
    from deepi2p_amd import _lib
    vec = R % 4 == 0 and R >= 32
    return "rc_gemm128" if vec and rows >= 128 and cols >= 128 and _lib.get_option("rc_tile64") == 0 else "rc_gemm 64-tile"


def _conv_path(xs, ws, stride, pad, what):
    """The kernel ops.conv_route names for the training step's convolution of xs with a filter bank ws (what = "fwd" / "dgrad"), as a label."""
    from deepi2p_amd import _lib, ops
    kernel, cfg = ops.conv_route(xs, ws, stride, pad, training=True)
    if kernel == "x3":
        knob = _lib.get_option("conv_x3_cfg")
        return "x3 conv %s [cfg %s]" % (what, knob if knob >= 0 else cfg if cfg >= 0 else "auto")
    if kernel == "winograd":
        return "winograd conv " + what
    p = "tap-major direct conv fwd" if kernel == "direct_tap" else "stem conv fwd, not tap-major"
    return "dgrad as " + p if what == "dgrad" else p


def _paths(case):
    """The kernels a case runs under the current knobs (the convolutions: by ops.conv_route, the rule train_net itself runs)."""
    from deepi2p_amd import _lib, train_net as tn
    op, sp = case["op"], case["spec"]
    if op == "_Conv2d":
        xs, ws, stride, pad = sp[0][1], sp[1][1], sp[2][1], sp[3][1]
        Cout, Cin, KH, KW = ws
        paths = [_conv_path(xs, ws, stride, pad, "fwd")]
        if stride == 1 and KH == KW and 2 * pad == KH - 1:
            paths.append(_conv_path((xs[0], Cout, xs[2], xs[3]), (Cin, Cout, KH, KW), 1, pad, "dgrad"))
        elif stride == 2 and _lib.get_option("conv_dgrad_dense") == 0:
            paths.append("s2 parity dgrad")
        else:
            paths.append("dense dgrad")
        paths += ["conv wgrad im2col", "rc_gemm 64-tile"]          # (RcIm2col operand: never the 128 x 128 tiles)
        return paths
    if op == "_Linear":
        (B, K, N), M = sp[0][1], sp[1][1][0]
        paths = ["bf16x3 linear fwd" if tn._x3_step(K, M, N) else "fp32 linear fwd",
                 "bf16x3 linear dx" if tn._x3_step(M, K, N) else "fp32 linear dx", _rc_path(M, K, N)]
        if sp[2][0] == "f":
            paths.append("channel_sum")
        return paths
    if op == "_AttentionPool":
        (B, C, HW), Mn = sp[0][1], sp[1][1][2]
        return [_rc_path(C, HW, Mn), "bmm_km"]
    if op == "_GatherCols":
        return ["gather bwd k=1", "rc_gemm 64-tile"]
    if op == "_Interpolate":
        return ["gather bwd k=3", "rc_gemm 64-tile"]
    if op == "_MaxPool":
        return ["maxpool bwd " + ("LDS" if _maxpool_uses_lds(sp[0][1]) else "fallback")]
    if op == "_BatchNorm":
        return ["bn " + ("unfused" if _lib.get_option("bn_unfused") else "fused")]
    return [op]


def _maxpool_uses_lds(shape):
    """di2p_maxpool3x3s2_backward's choice: the LDS kernel while its (2 R + 3) input rows and (R + 1) window rows (R = 4) fit 64 KiB."""
    B, C, H, W = shape
    OW = (W - 1) // 2 + 1
    return (11 * W + 5 * OW) * 4 <= 64 * 1024 and B * C <= 65535


def _describe(case):
    parts = []
    for k, v in case["spec"]:
        if k in ("f", "stat"):
            parts.append("x".join(str(s) for s in v))
        elif k == "t":
            parts.append("%s%s" % ({torch.int32: "i", torch.uint8: "u8", torch.float32: "f"}.get(v.dtype, "?"), "x".join(str(s) for s in v.shape)))
        elif v is None:
            parts.append("-")
        else:
            parts.append(str(v))
    return "%s(%s)" % (case["op"].lstrip("_"), " ".join(parts))


# ------------------------------------------------------------------------------------------------ the comparison
def _check(case, knobs=None, twice=True, label=""):
    """Replays `case` (under `knobs`) and returns (table row, failure messages)."""
    got = _hip(case, knobs)
    fails = []
    if twice:
        again = _hip(case, knobs)
        for name, a, b in zip(["out"] + ["g%d" % i for i in range(len(got) - 1)], got, again):
            if not torch.equal(a, b):
                fails.append("%s %s: two runs differ in %s" % (_describe(case), label, name))
    r = _reference(case)
    cells = []
    for i, (a, ref, name) in enumerate(zip(got, r["ref"], r["names"])):
        if a is None:
            fails.append("%s %s: no gradient for %s" % (_describe(case), label, name))
            continue
        if tuple(a.shape) != tuple(ref.shape):
            fails.append("%s %s: %s has shape %s, expected %s" % (_describe(case), label, name, tuple(a.shape), tuple(ref.shape)))
            continue
        e = _err(a, ref)
        cells.append("%s %.2g/%.2g" % ("d" + name if i else name, e, r["e32"][i]))
        if not e <= r["bars"][i]:
            fails.append("%s %s: %s error %.3g > bar %.3g (e32 %.3g)" % (_describe(case), label, "d" + name if i else name, e, r["bars"][i], r["e32"][i]))
        if i in r["sens"]:
            cells[-1] += " tail %.2g" % r["sens"][i]
            if not r["sens"][i] >= 3.0 * r["bars"][i]:
                fails.append("%s: the last %d reduction indices contribute only %.3g of d%s's abs-max (< 3 x bar %.3g): the test could not see "
                             "a lost tail tile" % (_describe(case), TAIL, r["sens"][i], name, r["bars"][i]))
    with _knobs(knobs):
        paths = _paths(case)
    row = "%-62s %-58s %s%s" % (_describe(case), ", ".join(paths), " | ".join(cells), ("  [%s]" % label) if label else "")
    return row, fails, got


def _run_cases(cases, title, knobs=None, twice=True):
    print("\n== %s (error / abs-max: HIP / torch fp32 CPU against float64; tail = share of the last %d reduction indices)" % (title, TAIL))
    fails = []
    for c in cases:
        row, f, _ = _check(c, knobs, twice, label=", ".join("%s=%s" % kv for kv in (knobs or {}).items()))
        print(row)
        fails += f
    return fails


def _by_op(step, *ops):
    return [c for c in step["cases"] if c["op"] in ops]


# ------------------------------------------------------------------------------------------------ 1 + 3: the recording and the coverage manifest
def test_step_records_every_function_and_covers_every_path(step):
    recorded = {c["op"] for c in step["cases"]}
    print("\n%d Function calls in one training forward, %d distinct" % (step["calls"], len(step["cases"])))
    # drift: a Function added to or renamed in train_net that the step does not call (or this file does not know) fails here
    assert recorded == set(step["names"]), "not recorded: %s" % sorted(set(step["names"]) - recorded)
    assert set(step["names"]) <= set(REF), "no float64 reference for %s" % sorted(set(step["names"]) - set(REF))
    manifest = {}
    for c in step["cases"]:
        for p in _paths(c):
            manifest.setdefault(p.split(" [")[0], []).append(_describe(c))
    print("coverage manifest (path: distinct cases)")
    for p in sorted(manifest):
        print("  %-40s %3d   e.g. %s" % (p, len(manifest[p]), manifest[p][0]))
    missing = [p for p in REQUIRED if p not in manifest]
    assert not missing, "the recorded training step does not reach: %s" % missing


# ------------------------------------------------------------------------------------------------ 2: every distinct call against float64
@pytest.mark.parametrize("ops", [("_Linear",), ("_Conv2d",), ("_BatchNorm",),
                                 ("_SegmentMax", "_GatherCols", "_Interpolate", "_GroupMax", "_AttentionPool", "_MaxPool", "_AvgPool", "_Dropout")],
                         ids=["linear", "conv2d", "batchnorm", "routers_pools"])
def test_replay_vs_float64(step, ops):
    cases = _by_op(step, *ops)
    assert cases
    fails = _run_cases(cases, "/".join(o.lstrip("_") for o in ops) + " at the step's shapes")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 4: knob variants of the same cases
def test_knob_rc_tile64(step):
    """64 x 64 tiles for the weight gradients that take 128 x 128 ones: other chunks, so the accuracy bar, not bit-equality."""
    from deepi2p_amd import _lib
    cases = [c for c in _by_op(step, "_Linear", "_AttentionPool") if "rc_gemm128" in _paths(c)]
    assert cases
    with _lib.option("rc_tile64", 1):
        assert all("rc_gemm128" not in _paths(c) for c in cases)
    fails = _run_cases(cases, "rc_tile64=1", {"rc_tile64": 1}, twice=False)
    assert not fails, "\n".join(fails)


def test_knob_bn_unfused_same_results(step):
    """The finalize of the BatchNorm statistics in a launch of its own (rounds 2-5) is documented as "same results": bit-identical output,
    input gradient, residual gradient, d gamma, d beta and running buffers."""
    from deepi2p_amd import train_net as tn
    cases = _by_op(step, "_BatchNorm")
    fails = []
    for c in cases:
        outs = []
        for unfused in (0, 1):
            leaves, args = _args(c, DEV, torch.float32)
            with _knobs({"bn_unfused": unfused}):
                y = tn._BatchNorm.apply(*args)
                y.backward(_cotangent(c, tuple(y.shape)).float().to(DEV))
            torch.cuda.synchronize()
            outs.append([y.detach()] + [t.grad for _, t in leaves] + [args[3], args[4]])
        for i, (a, b) in enumerate(zip(*outs)):
            if not torch.equal(a, b):
                fails.append("%s: tensor %d differs with bn_unfused=1 (max %.3g)" % (_describe(c), i, float((a - b).abs().max())))
    print("\nbn_unfused=1: %d BatchNorm cases compared bit for bit" % len(cases))
    assert not fails, "\n".join(fails)


def test_knob_pw_x3_off(step):
    cases = [c for c in _by_op(step, "_Linear") if any(p.startswith("bf16x3") for p in _paths(c))]
    assert cases
    fails = _run_cases(cases, "pw_x3=0 (fp32-MFMA point layers)", {"pw_x3": 0}, twice=False)
    assert not fails, "\n".join(fails)


def _x3_conv_cases(step):
    return [c for c in _by_op(step, "_Conv2d") if any(p.startswith("x3 conv") for p in _paths(c))]


def test_knob_conv_x3_off(step):
    cases = _x3_conv_cases(step)
    assert cases
    fails = _run_cases(cases, "conv_x3=0 (Winograd / direct kernels)", {"conv_x3": 0}, twice=False)
    assert not fails, "\n".join(fails)


def _batch16_cases():
    """The stride-1 3x3 layers of stages 1 and 2 at batch 16: from 16 frames on ops.conv_route takes every stage (forward and input gradient)."""
    cases = []
    for i, (C, H, W) in enumerate(((64, 40, 128), (128, 20, 64))):
        cases.append(dict(op="_Conv2d", spec=[("f", (16, C, H, W)), ("f", (C, C, 3, 3)), ("v", 1), ("v", 1)], seed=900 + i, count=1,
                          key="b16_%d" % i))
    return cases


_B16 = _batch16_cases()


def test_batch16_stage1_stage2_on_x3(step):
    for c in _B16:
        paths = _paths(c)
        assert paths[0].startswith("x3 conv fwd") and paths[1].startswith("x3 conv dgrad"), paths
    fails = _run_cases(_B16, "batch 16, stages 1 and 2")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_knob_conv_x3_cfg(step, cfg):
    """Each tile configuration of di2p_conv3x3_x3 on the x3 layers it supports.  A configuration that cannot run a shape (0 and 1 take 32-pixel
    segments: not the 16-pixel rows of the 512-channel stage; 1 to 3 do not fit the batch-16 stage-1 patch, 2 and 3 not the stage-2 one) leaves
    that layer on the Winograd kernel through ops.conv_route -- still held to the bar."""
    from deepi2p_amd import _lib
    cases = _x3_conv_cases(step) + _B16
    with _lib.option("conv_x3_cfg", cfg):
        on_x3 = [c for c in cases if any(p.startswith("x3 conv") for p in _paths(c))]
    print("\nconv_x3_cfg=%d runs di2p_conv3x3_x3 in %d of %d cases" % (cfg, len(on_x3), len(cases)))
    assert on_x3, "configuration %d supports none of the x3 layers" % cfg
    fails = _run_cases(cases, "conv_x3_cfg=%d" % cfg, {"conv_x3_cfg": cfg}, twice=False)
    assert not fails, "\n".join(fails)


def test_knob_conv_dgrad_dense_bit_identical(step):
    """The stride-2 input gradient per parity class must equal the dense kernel's bit for bit at the real layer shapes."""
    from deepi2p_amd import train_net as tn
    cases = [c for c in _by_op(step, "_Conv2d") if c["spec"][2][1] == 2]
    assert cases
    fails = []
    for c in cases:
        dx = []
        for dense in (0, 1):
            leaves, args = _args(c, DEV, torch.float32)
            with _knobs({"conv_dgrad_dense": dense}):
                y = tn._Conv2d.apply(*args)
                y.backward(_cotangent(c, tuple(y.shape)).float().to(DEV))
            torch.cuda.synchronize()
            dx.append(leaves[0][1].grad)
        if not torch.equal(dx[0], dx[1]):
            fails.append("%s: parity-class dgrad differs from the dense kernel (max %.3g)" % (_describe(c), float((dx[0] - dx[1]).abs().max())))
        print("conv_dgrad_dense=1 %s: %s" % (_describe(c), "bit-identical" if not fails else "DIFFERS"))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 5: small related cases
@pytest.mark.parametrize("shape", [(1, 2, 9, 1300), (2, 3, 12, 1301)])
def test_maxpool_backward_fallback_kernel(shape):
    """Planes too wide for the LDS kernel (its 11 input rows and 5 window rows need more than 64 KiB) take maxpool_backward_kernel; odd and
    even heights, ties from a ReLU input."""
    from deepi2p_amd import train_net as tn
    assert not _maxpool_uses_lds(shape)
    g = torch.Generator().manual_seed(shape[3])
    x = torch.relu(torch.randn(shape, generator=g))
    ct = torch.randn((shape[0], shape[1], (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1), generator=g, dtype=torch.float64)
    runs = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        y = tn._MaxPool.apply(xd)
        y.backward(ct.float().to(DEV))
        runs.append((y.detach(), xd.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    xr = x.double().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    yr.backward(ct)
    assert _err(runs[0][0], yr) == 0.0
    assert _err(runs[0][1], xr.grad) <= DEFAULT_FLOOR


def test_classifier_loss_at_production_size():
    """training.classifier_loss at B = 8, N = 20480 and the 80 fine classes of 160 x 512 against oracle/losses_torch in float64."""
    from deepi2p_amd.training import classifier_loss
    from oracle import losses_torch as lt
    B, N, L = B_STEP, N_STEP, 80
    g = torch.Generator().manual_seed(17)
    coarse = torch.randn(B, 2, N, generator=g) * 2
    fine = torch.randn(B, L, N, generator=g) * 2
    clab = (torch.rand(B, N, generator=g) < 0.4).to(torch.int32)
    flab = torch.randint(0, L, (B, N), generator=g, dtype=torch.int32)
    out = classifier_loss(coarse.to(DEV), clab.to(DEV), fine.to(DEV), flab.to(DEV), coarse_loss_alpha=50.0)
    out2 = classifier_loss(coarse.to(DEV), clab.to(DEV), fine.to(DEV), flab.to(DEV), coarse_loss_alpha=50.0)
    c64, f64 = coarse.double().requires_grad_(True), fine.double().requires_grad_(True)
    loss, cl, fl, _, _ = lt.classifier_loss(c64, f64, clab.long(), flab.long(), 50.0)
    loss.backward()
    print("\nclassifier loss B=%d N=%d L=%d: loss %.6f (fp64 %.6f), d_coarse %.2g, d_fine %.2g" % (
        B, N, L, float(out["loss"]), float(loss.detach()), _err(out["d_coarse"], c64.grad), _err(out["d_fine"], f64.grad)))
    for key, ref in (("loss", loss.detach()), ("coarse", cl.detach()), ("fine", fl.detach())):
        assert abs(float(out[key]) - float(ref)) <= 1e-5 * abs(float(ref)), key
    assert float(out["inside"]) == float((clab == 1).sum())
    assert _err(out["d_coarse"], c64.grad) <= 1e-5
    assert _err(out["d_fine"], f64.grad) <= 1e-5
    assert torch.equal(out["d_coarse"], out2["d_coarse"]) and torch.equal(out["d_fine"], out2["d_fine"])
    assert float(out["loss"]) == float(out2["loss"])
