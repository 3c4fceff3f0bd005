"""The exact-integer cases of the bf16x3 pointwise GEMMs (operand families of tests/x3_exact_cases.py): shapes, sources and epilogues, with
their fp64 references.  CPU only: tests/test_x3_exact_cases_host.py proves the bounds, tests/test_gpu_pointwise_x3_exact.py runs the kernels."""
import functools

import torch

from tests import x3_exact_cases as xc

B = 2
GROUP = 16
# (K, M, N): the smallest layer; ragged K-step and N tile; three 128-row tiles on a narrow N; a partial 128-row tile
SHAPES = [(32, 4, 4), (130, 128, 132), (128, 384, 20), (160, 260, 256)]
# source kinds per shape: one dense source; three concatenated dense sources (5 + 64 + the rest: 5 + 64 + 61 at K = 130); a gather source;
# a group source (one column per 16 output columns: N % 16 == 0)
SOURCE_CASES = ([(s, "dense") for s in SHAPES] + [(s, "concat") for s in SHAPES if s[0] >= 130] + [(s, "gather") for s in SHAPES]
                + [(s, "group") for s in SHAPES if s[2] % GROUP == 0])
# epilogues on family A: (shape, kind)
EPILOGUE_CASES = ([((130, 128, 132), k) for k in ("bias", "transpose", "gathered", "gathered_w")]
                  + [((160, 260, 256), k) for k in ("bias", "transpose", "gmax16", "gmax8_full", "gathered", "gathered_w")])
# planes hand-over: K, M1, N of the producer; M2 of the consumer (384: the 128-row kernel, 256: the 256-row kernel)
PLANES = dict(K=128, M1=128, N=128, M2=(384, 256), families=("A", "B"))
NODES, GK = 24, 3


def source_id(case):
    (K, M, N), kind = case
    return "%dx%dx%d-%s" % (K, M, N, kind)


@functools.lru_cache(maxsize=None)
def source_case(family, K, M, N, kind):
    """dict: w f32[M,K]; parts = [(kind, tensor, gidx | None)] to build ops.Src from; full f32[B,K,N] the virtual concatenation; ref / absum"""
    what = (family, K, M, N, kind)
    w = xc.weights(family, M, (K,), xc.seed_of("w", what))
    g = torch.Generator().manual_seed(xc.seed_of("i", what))
    if kind in ("dense", "concat"):
        full = xc.activations(family, (B, K, N), xc.seed_of("x", what), max_channels=63)
        split = (K,) if kind == "dense" else (5, 64, K - 69)
        parts = [("dense", t.contiguous(), None) for t in torch.split(full, split, dim=1)]
    elif kind == "gather":
        tab = xc.activations(family, (B, K, NODES), xc.seed_of("x", what), max_channels=63)
        gi = torch.randint(0, NODES, (B, N), generator=g, dtype=torch.int32)
        gi[:, 0], gi[:, -1] = NODES - 1, 0
        full = torch.gather(tab, 2, gi.long().unsqueeze(1).expand(B, K, N))
        parts = [("gather", tab, gi)]
    elif kind == "group":
        src = xc.activations(family, (B, K, N // GROUP), xc.seed_of("x", what), max_channels=63)
        full = src.repeat_interleave(GROUP, dim=2)
        parts = [("group", src, None)]
    else:
        raise ValueError(kind)
    ref, absum = xc.gemm_reference(full, w)
    return dict(w=w, parts=parts, full=full, ref=ref, absum=absum)


@functools.lru_cache(maxsize=None)
def epilogue_case(K, M, N, kind):
    """family A through one epilogue: dict with w, x, kw (the CPU tensors of pointwise_gemm's keyword arguments; `gathered` as a list of
    (table, idx, w | None)), ref (fp64, what the call returns; a tuple for also_full) and absum of the contraction"""
    what = ("A", K, M, N, kind)
    g = torch.Generator().manual_seed(xc.seed_of("e", what))
    w = xc.weights("A", M, (K,), xc.seed_of("w", what))
    x = xc.activations("A", (B, K, N), xc.seed_of("x", what))
    acc, absum = xc.gemm_reference(x, w)
    scale, shift, _ = xc.epilogue(M, (1,), xc.seed_of("s", what))
    kw = dict(scale=scale, shift=shift, relu=kind in ("gmax16", "gathered"))
    v = acc
    if kind == "bias":
        kw["batch_bias"] = torch.randint(-64, 65, (B, M), generator=g).to(torch.float32)
        v = v + kw["batch_bias"].double().unsqueeze(2)
    if kind in ("gathered", "gathered_w"):
        tab = torch.randint(-32, 33, (B, NODES, M), generator=g).to(torch.float32)
        gi = torch.randint(0, NODES, (B, N, GK), generator=g, dtype=torch.int32)
        gw = None if kind == "gathered" else torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])[torch.randint(0, 5, (B, N, GK), generator=g)]
        kw["gathered"] = [(tab, gi, gw)]
        rows = torch.gather(tab.double().unsqueeze(1).expand(B, N, NODES, M), 2, gi.long().unsqueeze(3).expand(B, N, GK, M))      # [B,N,GK,M]
        v = v + ((rows * gw.double().unsqueeze(3)) if gw is not None else rows).sum(2).transpose(1, 2)
    v = v * scale.double().view(1, M, 1) + shift.double().view(1, M, 1)
    if kw["relu"]:
        v = torch.relu(v)
    ref = v
    if kind == "transpose":
        kw["transpose_out"] = True
        ref = v.transpose(1, 2).contiguous()
    if kind == "gmax16":
        kw["group_max"] = 16
        ref = v.view(B, M, N // 16, 16).max(dim=3)[0]
    if kind == "gmax8_full":
        kw.update(group_max=8, also_full=True)
        ref = (v, v.view(B, M, N // 8, 8).max(dim=3)[0])
    return dict(w=w, x=x, kw=kw, ref=ref, absum=absum)


@functools.lru_cache(maxsize=None)
def planes_case(family, M2):
    """two layers, the first handing split planes to the second: x f32[B,K,N], w1 f32[M1,K], w2 f32[M2,M1]; ref1 / ref2 (fp64), absum1 / absum2.
    Family B's first layer has ONE +-1 per output row (a signed selection of input rows): its output is as wide as its input, |y1| < 2^18
    and odd, which is what family B asks of the activations of the second layer."""
    K, M1, N = PLANES["K"], PLANES["M1"], PLANES["N"]
    what = (family, M2, "planes")
    x = xc.activations(family, (B, K, N), xc.seed_of("x", what), max_channels=63)
    w1 = xc.weights(family, M1, (K,), xc.seed_of("w1", what), nnz=1)
    w2 = xc.weights(family, M2, (M1,), xc.seed_of("w2", what))
    ref1, absum1 = xc.gemm_reference(x, w1)
    ref2, absum2 = xc.gemm_reference(ref1, w2)
    return dict(x=x, w1=w1, w2=w2, ref1=ref1, ref2=ref2, absum1=absum1, absum2=absum2)
