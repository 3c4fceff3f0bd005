"""Thin torch-tensor front-ends of the C-ABI kernels (include/deepi2p_hip.h).

torch supplies device memory and the current HIP stream only.  Every function launches on
``torch.cuda.current_stream()`` (the reference launched on the legacy default stream,
index_max_cuda.cu:75,93) and never synchronises, so sequences of these calls can be captured in a
``torch.cuda.CUDAGraph``.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._lib import EpilogueT, SrcT, call, ptr, require_cuda, stream

_f32, _i32, _f64 = torch.float32, torch.int32, torch.float64
MAX_GK = 16          # DI2P_MAX_GK (include/deepi2p_hip.h)


def _chk(t, dtype, name):
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))


def _work(name, macs):
    """Add `macs` multiply-accumulates to the executed-work counter of entry point `name` (_lib.WORK; bench.py switches it on)."""
    if _lib.WORK is not None:
        _lib.WORK[name] = _lib.WORK.get(name, 0) + macs


# ------------------------------------------------------------------------------------ native ops
def index_max(data, index, K, return_values=False, mask=None):
    """data f32[B,C,N], index i32[B,N] -> max_idx i32[B,C,K] (and masked max values if asked)."""
    require_cuda(data, index, mask)
    _chk(data, _f32, "data")
    _chk(index, _i32, "index")
    B, C, N = data.shape
    K = int(K)
    if tuple(index.shape) != (B, N):
        raise RuntimeError("index must be i32[B, N] for data f32[B, C, N]")
    if mask is not None and tuple(mask.shape) != (B, K):
        raise RuntimeError("mask must be f32[B, K]")
    idx = torch.empty((B, C, K), dtype=_i32, device=data.device)
    ws = torch.empty((B * C * K,), dtype=torch.int64, device=data.device)
    if return_values:
        val = torch.empty((B, C, K), dtype=_f32, device=data.device)
        call("di2p_index_max_values", ptr(data), ptr(index), ptr(mask), ptr(val), ptr(idx), B, C, N, K, ptr(ws), stream())
        return idx, val
    call("di2p_index_max_forward", ptr(data), ptr(index), ptr(idx), B, C, N, K, ptr(ws), stream())
    return idx


def ball_query(node_to_point_dist, radius, K):
    require_cuda(node_to_point_dist)
    _chk(node_to_point_dist, _f32, "node_to_point_dist")
    B, M, N = node_to_point_dist.shape
    out = torch.empty((B, M, int(K)), dtype=_i32, device=node_to_point_dist.device)
    call("di2p_ball_query_forward", ptr(node_to_point_dist), ptr(out), float(radius), int(K), B, M, N, stream())
    return out


def _shape(t, shape, name, what):
    """shape: expected sizes, None = any; the operands of one call must agree on B / N / M / k before a pointer is handed over"""
    if t.dim() != len(shape) or any(e is not None and int(s) != int(e) for s, e in zip(t.shape, shape)):
        raise RuntimeError("%s must be %s, got %s" % (name, what, list(t.shape)))


def knn_nodes(query, nodes, k, want_weights=False):
    """query f32[B,3,Nq], nodes f32[B,3,M] -> idx i32[B,Nq,k] (+ weights f32[B,Nq,k])."""
    require_cuda(query, nodes)
    _chk(query, _f32, "query")
    _chk(nodes, _f32, "nodes")
    _shape(query, (None, 3, None), "query", "f32[B, 3, Nq]")
    B, _, Nq = query.shape
    _shape(nodes, (B, 3, None), "nodes", "f32[B, 3, M] for query f32[B, 3, Nq]")
    M, k = nodes.shape[2], int(k)             # the library checks 1 <= k <= 16, k <= M <= 4096 before it launches
    idx = torch.empty((B, Nq, k), dtype=_i32, device=query.device)
    w = torch.empty((B, Nq, k), dtype=_f32, device=query.device) if want_weights else None
    call("di2p_knn_nodes", ptr(query), ptr(nodes), ptr(idx), ptr(w), B, Nq, M, k, stream())
    return (idx, w) if want_weights else idx


def cluster_stats(pc, knn_idx, M):
    """pc f32[B,3,N], knn_idx i32[B,N,k] (column 0 = nearest node) -> mean f32[B,3,M], mask f32[B,M], min_idx i32[B,N]."""
    require_cuda(pc, knn_idx)
    _chk(pc, _f32, "pc")
    _chk(knn_idx, _i32, "knn_idx")
    _shape(pc, (None, 3, None), "pc", "f32[B, 3, N]")
    B, _, N = pc.shape
    _shape(knn_idx, (B, N, None), "knn_idx", "i32[B, N, k] for pc f32[B, 3, N]")
    M = int(M)
    mean = torch.empty((B, 3, M), dtype=_f32, device=pc.device)
    mask = torch.empty((B, M), dtype=_f32, device=pc.device)
    min_idx = torch.empty((B, N), dtype=_i32, device=pc.device)
    call("di2p_cluster_stats", ptr(pc), ptr(knn_idx), knn_idx.shape[2], ptr(mean), ptr(mask), ptr(min_idx), B, N, M, stream())
    return mean, mask, min_idx


def build_point_input(pc, intensity, sn, cluster_mean, min_idx):
    """pc f32[B,3,N], intensity f32[B,1,N], sn f32[B,3,N], cluster_mean f32[B,3,M], min_idx i32[B,N] -> centers f32[B,3,N], aug f32[B,7,N]."""
    require_cuda(pc, intensity, sn, cluster_mean, min_idx)
    for t, name in ((pc, "pc"), (intensity, "intensity"), (sn, "sn"), (cluster_mean, "cluster_mean")):
        _chk(t, _f32, name)
    _chk(min_idx, _i32, "min_idx")
    _shape(pc, (None, 3, None), "pc", "f32[B, 3, N]")
    B, _, N = pc.shape
    _shape(intensity, (B, 1, N), "intensity", "f32[B, 1, N] for pc f32[B, 3, N]")
    _shape(sn, (B, 3, N), "sn", "f32[B, 3, N] for pc f32[B, 3, N]")
    _shape(cluster_mean, (B, 3, None), "cluster_mean", "f32[B, 3, M] for pc f32[B, 3, N]")
    _shape(min_idx, (B, N), "min_idx", "i32[B, N] for pc f32[B, 3, N]")
    centers = torch.empty_like(pc)
    aug = torch.empty((B, 7, N), dtype=_f32, device=pc.device)
    call("di2p_build_point_input", ptr(pc), ptr(intensity), ptr(sn), ptr(cluster_mean), ptr(min_idx), ptr(centers),
         ptr(aug), B, N, cluster_mean.shape[2], stream())
    return centers, aug


def interpolate(feats, idx, weights):
    """feats f32[B,C,M], idx i32[B,Nq,k], weights f32[B,Nq,k] -> f32[B,C,Nq]."""
    require_cuda(feats, idx, weights)
    _chk(feats, _f32, "feats")
    _chk(idx, _i32, "idx")
    _chk(weights, _f32, "weights")
    _shape(feats, (None, None, None), "feats", "f32[B, C, M]")
    B, C, M = feats.shape
    _shape(idx, (B, None, None), "idx", "i32[B, Nq, k] for feats f32[B, C, M]")
    Nq, k = idx.shape[1], idx.shape[2]
    _shape(weights, (B, Nq, k), "weights", "f32[B, Nq, k] for idx i32[B, Nq, k]")
    out = torch.empty((B, C, Nq), dtype=_f32, device=feats.device)
    call("di2p_interpolate", ptr(feats), ptr(idx), ptr(weights), ptr(out), B, C, M, Nq, k, stream())
    return out


def gather_neighbors(database, query, idx):
    """database f32[B,3,Md], query f32[B,3,Mq], idx i32[B,Mq,K] -> f32[B,3,Mq*K] = database[:, idx] - query."""
    require_cuda(database, query, idx)
    _chk(database, _f32, "database")
    _chk(query, _f32, "query")
    _chk(idx, _i32, "idx")
    _shape(database, (None, 3, None), "database", "f32[B, 3, Md]")
    B, _, Md = database.shape
    _shape(query, (B, 3, None), "query", "f32[B, 3, Mq] for database f32[B, 3, Md]")
    _shape(idx, (B, query.shape[2], None), "idx", "i32[B, Mq, K] for query f32[B, 3, Mq]")
    Mq, K = idx.shape[1], idx.shape[2]
    out = torch.empty((B, 3, Mq * K), dtype=_f32, device=database.device)
    call("di2p_gather_neighbors", ptr(database), ptr(query), ptr(idx), ptr(out), B, Md, Mq, K, stream())
    return out


def argmax_channels(scores):
    """scores f32[B,C,N] (a channel slice of a larger [B,C',N] tensor is fine) -> i32[B,N]."""
    if not scores.is_cuda:
        raise RuntimeError("tensor must be a CUDA tensor/variable")
    B, C, N = scores.shape
    if scores.stride(2) != 1 or scores.stride(1) != N:
        raise RuntimeError("scores rows must be contiguous")
    out = torch.empty((B, N), dtype=_i32, device=scores.device)
    call("di2p_argmax_channels", ptr(scores), ptr(out), B, C, N, scores.stride(0), stream())
    return out


def channel_max(x):
    """x f32[B,C,N] -> f32[B,C], the maximum over N (NaN if the row holds one)."""
    require_cuda(x)
    _chk(x, _f32, "x")
    _shape(x, (None, None, None), "x", "f32[B, C, N]")
    B, C, N = x.shape
    out = torch.empty((B, C), dtype=_f32, device=x.device)
    call("di2p_channel_max", ptr(x), ptr(out), B, C, N, stream())
    return out


# ------------------------------------------------------------------------------------ contractions
class Src:
    """One operand source of the virtual concatenation (see di2p_src_t)."""

    def __init__(self, t, mode=_lib.SRC_DENSE, gidx=None, group=1):
        require_cuda(t, gidx)
        assert t.dim() == 3
        self.t, self.mode, self.gidx, self.group = t, mode, gidx, group


class X3Planes:
    """An activation f32[B,C,N] held ALREADY SPLIT for the bf16x3 kernel that contracts over its channels: u16[B,3,C/4,N,4], the three exact bf16
    terms of every value, four consecutive channels of one column per 8 bytes (di2p_epilogue_t.planes_out; include/deepi2p_hip.h).  Written
    by pointwise_gemm(..., planes_out=True), read by pointwise_gemm([X3Planes], ...); float() gives the fp32 values back (tests)."""

    def __init__(self, t, C, N):
        self.t, self.C, self.N = t, C, N
        self.shape = (t.shape[0], C, N)

    @staticmethod
    def ok(C, N):
        """Can a layer with C output rows and N columns hand its output on as planes (to a consumer with K = C)?"""
        return C % 32 == 0 and N % 128 == 0 and 3 * C * N * 2 < (1 << 31)

    def float(self):
        B = self.t.shape[0]
        w = self.t.view(torch.int16).view(B, 3, self.C // 4, self.N, 4).to(torch.int32) << 16
        f = w.view(torch.float32)
        return ((f[:, 2] + f[:, 1]) + f[:, 0]).permute(0, 1, 3, 2).reshape(B, self.C, self.N)


def _fill_srcs(srcs):
    arr = (SrcT * len(srcs))()
    for i, s in enumerate(srcs):
        arr[i].ptr = ptr(s.t)
        arr[i].gidx = ptr(s.gidx)
        arr[i].batch_stride = s.t.stride(0)
        arr[i].row_stride = s.t.stride(1)
        arr[i].channels = s.t.shape[1]
        arr[i].mode = s.mode
        arr[i].group = s.group
    return arr


def _fill_gathered(e, gathered, B, M, N):
    """Up to two gathered tables (table f32[B,nodes,M] node-major, idx i32[B,N,k_t], w f32[B,N,k_t] | None); each
    table carries its OWN k (opt.k_interp_point_a and k_interp_point_b may differ)."""
    e.g_k[0] = e.g_k[1] = 0
    if not gathered:
        return
    if len(gathered) > 2:
        raise RuntimeError("at most two gathered tables")
    for t, (tab, gi, gw) in enumerate(gathered):
        require_cuda(tab, gi, gw)
        _chk(tab, _f32, "gathered table")
        _chk(gi, _i32, "gathered index")
        if tab.dim() != 3 or tab.shape[0] != B or tab.shape[2] != M:
            raise RuntimeError("gathered table must be f32[B, nodes, M]")
        if gi.dim() != 3 or gi.shape[0] != B or gi.shape[1] != N:
            raise RuntimeError("gathered index must be i32[B, N, k]")
        k = gi.shape[2]
        if not 1 <= k <= MAX_GK:
            raise RuntimeError("gathered k must be in [1, %d]" % MAX_GK)
        if gw is not None:
            _chk(gw, _f32, "gathered weights")
            if gw.shape != gi.shape:
                raise RuntimeError("gathered weights must have the index's shape")
        e.g_table[t], e.g_idx[t], e.g_w[t] = ptr(tab), ptr(gi), ptr(gw)
        e.g_nodes[t] = tab.shape[1]
        e.g_k[t] = k


# bf16x3 operand cache: packed (split) weights of the GEMM-shaped layers, keyed by the fp32 operand they were made from.  An entry lives exactly
# as long as the fp32 operand's BASE tensor (a derived tensor owned by one networks._PackedModule's `_packed` container): a weak-reference
# finaliser drops it when that tensor is freed, so (i) a recycled address can never return a stale split, (ii) invalidating ONE module (its
# .to(), load_state_dict, an optimiser step) never touches another module's splits -- a holder of raw pointers (a captured hipGraph) keeps the
# module's packed operands referenced and thereby their splits (pipeline.RegistrationExecutor._packed_refs / _x3_refs).
# An entry is published only when it is COMPLETE: the packing stream is synchronised before the entry becomes visible, so another stream
# that finds it needs no ordering; under stream capture nothing can be waited for -- the pack becomes a node of THAT graph and is not
# cached (the executor runs one eager step before it captures, so this is the cold path only).
_X3_CACHE = {}            # (address, K, M, device) -> (weak reference to the fp32 operand's base tensor, split operand)
X3_MIN_K = 128


def x3_invalidate():
    """Drop every cached split (tests; never needed for correctness: entries die with the operand they were made from)."""
    _X3_CACHE.clear()


def x3_live_operands(owners=None):
    """The split operands currently cached (a holder of raw pointers to them keeps this list).  owners: packed-operand containers
    (networks._PackedModule.packed_operands()) -- only the splits whose fp32 operand lives in one of them, so that a holder pins the
    splits of ITS model and not those of every other model (or test) that happens to be alive in the process."""
    if owners is None:
        return [e[1] for e in _X3_CACHE.values()]
    mine = set()

    def walk(o):
        if isinstance(o, torch.Tensor):
            mine.add(id(o._base if o._base is not None else o))
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
        elif hasattr(o, "__dict__"):
            for v in vars(o).values():
                walk(v)

    walk(owners)
    out = []
    for ref, wp in list(_X3_CACHE.values()):
        base = ref()
        if base is not None and id(base) in mine:
            out.append(wp)
    return out


def bf16x3_pack(Wt):
    """Wt f32[K,M] (contiguous) -> the split operand of di2p_pointwise_gemm_x3 (uint8 storage)."""
    require_cuda(Wt)
    K, M = Wt.shape
    Wp = torch.empty((_lib.load().di2p_bf16x3_packed_bytes(K, M),), dtype=torch.uint8, device=Wt.device)
    call("di2p_bf16x3_pack", ptr(Wt), K, M, ptr(Wp), stream())
    return Wp


def bf16x3_pack_conv3x3(W, dgrad=False):
    """The split operand of conv3x3_x3 straight from a filter bank W f32[Cout,Cin,3,3] (contiguous): the forward filter, or (dgrad=True) the
    filter whose convolution with dY is the layer's input gradient -- the same bytes as bf16x3_pack of the permuted (and flipped, transposed)
    matrix, in one launch."""
    require_cuda(W)
    _chk(W, _f32, "bf16x3_pack_conv3x3 filter")
    if W.dim() != 4 or W.shape[2:] != (3, 3) or not W.is_contiguous():
        raise RuntimeError("bf16x3_pack_conv3x3 needs a contiguous f32[Cout,Cin,3,3]")
    Cout, Cin = int(W.shape[0]), int(W.shape[1])
    K, M = (9 * Cout, Cin) if dgrad else (9 * Cin, Cout)
    Wp = torch.empty((_lib.load().di2p_bf16x3_packed_bytes(K, M),), dtype=torch.uint8, device=W.device)
    call("di2p_bf16x3_pack_conv3x3", ptr(W), Cout, Cin, int(bool(dgrad)), ptr(Wp), stream())
    return Wp


def _x3_auto(Wt, M, N):
    """The automatic rule of _x3_operand: does the layer with weights Wt [K, M] on N columns per frame run on the bf16x3 kernel?"""
    return (Wt.shape[0] >= X3_MIN_K and M % 128 == 0 and N % 4 == 0 and ((N + 127) // 128) * (M // 128) >= 8 and not Wt.requires_grad
            and _lib.get_option("pw_x3") != 0)


def _x3_operand(Wt, B, M, N, x3):
    """The packed operand if this layer runs on the bf16x3 kernel, else None.  x3: None = by shape and the library knob `pw_x3`; True / False force.
    Automatic rule: K >= 128, M % 128 == 0 and at least eight 128 x 128 workgroups PER FRAME -- a rule on the layer's shape only: a frame's
    result must not depend on the batch it is in (measured per layer of a 32-frame step,
    tools/call_times.py: 256x256x2048 135 -> 124 us, 512x256x2048 198 -> 139, 256x512x2048 211 -> 166, 1024x768x128 70 -> 55; the node-level
    layers with 128 workgroups or fewer are FASTER on the fp32 kernel's 64 x 64 tiles: 512x1024x128 48 vs 63 us, 128x512x128 19 vs 35)."""
    if x3 is None:
        x3 = _x3_auto(Wt, M, N)
    if not x3:
        return None
    K = Wt.shape[0]
    if x3 == "step":
        # training: the operand is this step's transposed copy of a parameter -- split it on the stream, use it once, cache nothing (no
        # host synchronisation: the split, the launch that reads it and the allocator's reuse of its memory are ordered by the stream)
        if M % 4 or N % 4 or not Wt.is_contiguous():
            raise RuntimeError("bf16x3 needs M % 4 == 0, N % 4 == 0 and a contiguous [K,M] weight")
        return bf16x3_pack(Wt)
    if M % 4 or N % 4 or not Wt.is_contiguous():
        raise RuntimeError("bf16x3 needs M % 4 == 0, N % 4 == 0 and a contiguous [K,M] weight")
    # an address is only an identity while the tensor that owns it is alive: the entry remembers (weakly) the base tensor it was made from --
    # a deleted module's operand whose memory the allocator hands to the next module must not find the old split
    base = Wt._base if Wt._base is not None else Wt
    key = (Wt.data_ptr(), K, M, Wt.device.index)
    ent = _X3_CACHE.get(key)
    if ent is not None and ent[0]() is base:
        return ent[1]
    Wp = bf16x3_pack(Wt)
    if torch.cuda.is_current_stream_capturing():
        return Wp                                    # a node of this graph only: never visible to another stream or graph
    torch.cuda.current_stream(Wt.device).synchronize()   # complete before it is published (once per layer and weights version)

    def _expired(ref, key=key):
        ent = _X3_CACHE.get(key)
        if ent is not None and ent[0] is ref:
            del _X3_CACHE[key]

    _X3_CACHE[key] = (weakref.ref(base, _expired), Wp)
    return Wp


def x3_planes_link(producer, consumer_Wt, B, N):
    """Should `producer` (a (Wt, scale, shift, act) layer) hand its [B, M, N] output to the layer with weights consumer_Wt [K = M, M2] as
    split planes?  Both must run on the bf16x3 kernel by the automatic rule, the shapes must fit X3Planes, and the knob `pw_x3_planes` be on."""
    Wt = producer[0]
    M = Wt.shape[1]
    if _lib.get_option("pw_x3_planes") == 0 or consumer_Wt.shape[0] != M or not X3Planes.ok(M, N):
        return False
    return all(_x3_auto(W, W.shape[1], N) and W.is_contiguous() for W in (Wt, consumer_Wt))


def pointwise_gemm(srcs, Wt, M, N, scale=None, shift=None, batch_bias=None, relu=False, group_max=1, gathered=None,
                   transpose_out=False, also_full=False, x3=None, planes_out=False):
    """Y[b] = epi(Wt^T @ concat(srcs)[b]).  srcs: list of Src; Wt f32[K,M].  gathered: optional list of up
    to two (table f32[B,nodes,M] node-major, idx i32[B,N,k], w f32[B,N,k]).  transpose_out: Y is f32[B,N,M].
    group_max > 1 returns the group maxima; with also_full=True it returns (full Y, maxima) from the same launch.
    x3: run the contraction on the bf16x3 kernel (exact three-way bf16 split of both operands, fp32 accumulation; None = for the GEMM-shaped
    layers, K >= 128 and M % 128 == 0, unless the knob `pw_x3` is 0; "step" = yes, with the weights split for this call only -- the
    training step, whose operand is a fresh transposed copy of a parameter every time).
    planes_out (bf16x3 layers only): the full-size output comes back as X3Planes -- already split for the bf16x3 layer that consumes it as
    `srcs=[planes]` (bit-identical to handing the fp32 output on; the split leaves the consumer's K loop)."""
    B = srcs[0].t.shape[0]
    K = Wt.shape[0]
    from_planes = any(isinstance(s, X3Planes) for s in srcs)
    if from_planes:
        if len(srcs) != 1 or srcs[0].C != K or srcs[0].N != N or srcs[0].t.device != Wt.device:
            raise RuntimeError("a split-planes source must be the only source, with K channels and N columns, on the weights' device")
        x3 = True
    if planes_out and (transpose_out or not X3Planes.ok(M, N)):
        raise RuntimeError("planes_out needs M % 32 == 0, N % 128 == 0 and no transpose_out")
    if x3 is not False and any(t is not None and t.data_ptr() % 16 for t in (scale, shift, batch_bias)):
        # the bf16x3 kernels read the per-row operands 16 bytes at a time (a bias that is a view at an odd offset of a flat parameter buffer)
        if x3 is not None and x3 != "step":
            raise RuntimeError("bf16x3 needs 16-byte aligned scale, shift and batch_bias")
        x3 = False
    Wp = _x3_operand(Wt, B, M, N, x3)
    if planes_out and Wp is None:
        raise RuntimeError("planes_out: only the bf16x3 kernels write split planes")
    arr = None if from_planes else _fill_srcs(srcs)
    e = EpilogueT()
    e.scale, e.shift, e.batch_bias = ptr(scale), ptr(shift), ptr(batch_bias)
    e.relu, e.group_max = int(bool(relu)), int(group_max)
    _fill_gathered(e, gathered, B, M, N)
    e.transpose_out = int(bool(transpose_out))
    Nout = N // group_max if group_max > 1 else N
    Ymax = None
    if planes_out:
        # the full-size output as split planes; with group_max > 1 the maxima come out of the same launch (also_full or not: there is no
        # maxima-only planes output)
        if group_max > 1 and not also_full:
            raise RuntimeError("planes_out with group_max > 1 returns (planes, maxima): pass also_full=True")
        Y = X3Planes(torch.empty((_lib.load().di2p_bf16x3_planes_bytes(B, M, N),), dtype=torch.uint8, device=Wt.device).view(B, -1), M, N)
        e.planes_out = ptr(Y.t)
        if group_max > 1:
            Ymax = torch.empty((B, M, Nout), dtype=_f32, device=Wt.device)
            e.group_max_out = ptr(Ymax)
        y_ptr = None
    elif also_full and group_max > 1:
        Y = torch.empty((B, M, N), dtype=_f32, device=Wt.device)
        Ymax = torch.empty((B, M, Nout), dtype=_f32, device=Wt.device)
        e.group_max_out = ptr(Ymax)
        y_ptr = ptr(Y)
    else:
        Y = torch.empty((B, Nout, M) if transpose_out else (B, M, Nout), dtype=_f32, device=Wt.device)
        y_ptr = ptr(Y)
    if Wp is not None:
        _work("di2p_pointwise_gemm_x3", B * M * K * N)
        if from_planes:
            call("di2p_pointwise_gemm_x3p", ptr(srcs[0].t), ptr(Wp), y_ptr, B, M, K, N, ctypes.byref(e), stream())
        else:
            call("di2p_pointwise_gemm_x3", arr, len(srcs), ptr(Wp), y_ptr, B, M, K, N, ctypes.byref(e), stream())
        return (Y, Ymax) if Ymax is not None else Y
    _work("di2p_pointwise_gemm", B * M * K * N)
    call("di2p_pointwise_gemm", arr, len(srcs), ptr(Wt), ptr(Y), B, M, K, N, ctypes.byref(e), stream())
    return (Y, Ymax) if Ymax is not None else Y


def point_head(srcs, layer0, layer1, layer2, N, batch_bias=None, gathered=None):
    """Fused three-layer per-point head (di2p_point_head): layers are (Wt[K,M], scale, shift, relu) tuples with hidden
    width 128 and at most 4 outputs; layer0's Wt holds only the rows of the dense `srcs`.  -> f32[B, P, N]."""
    Wt0, sc0, sh0, act0 = layer0
    Wt1, sc1, sh1, act1 = layer1
    Wt2, sc2, sh2, act2 = layer2
    B = srcs[0].t.shape[0]
    M, P = Wt0.shape[1], Wt2.shape[1]
    require_cuda(Wt0, Wt1, Wt2, sc0, sh0, sc1, sh1, sc2, sh2, batch_bias)
    e = EpilogueT()
    e.scale, e.shift, e.batch_bias = ptr(sc0), ptr(sh0), ptr(batch_bias)
    e.relu, e.group_max, e.transpose_out = int(bool(act0)), 1, 0
    _fill_gathered(e, gathered, B, M, N)
    out = torch.empty((B, P, N), dtype=_f32, device=Wt0.device)
    _work("di2p_point_head", B * N * (Wt0.shape[0] * M + M * M + M * P))
    call("di2p_point_head", _fill_srcs(srcs), len(srcs), ptr(Wt0), Wt0.shape[0], ctypes.byref(e), ptr(Wt1), ptr(sc1), ptr(sh1),
         int(bool(act1)), ptr(Wt2), ptr(sc2), ptr(sh2), int(bool(act2)), ptr(out), B, M, P, N, stream())
    return out


def head_x3_pack(Wt):
    """Wt f32[K,128] (contiguous, K % 16 == 0) -> the fragment-ordered split operand of di2p_point_head_x3 (uint8 storage)."""
    require_cuda(Wt)
    K, M = Wt.shape
    if M != 128 or K % 16 or not Wt.is_contiguous():
        raise RuntimeError("head_x3_pack needs a contiguous f32[K,128] with K % 16 == 0")
    Wp = torch.empty((_lib.load().di2p_head_x3_packed_bytes(K),), dtype=torch.uint8, device=Wt.device)
    call("di2p_head_x3_pack", ptr(Wt), K, ptr(Wp), stream())
    return Wp


def point_head_x3(src0, src1, packed, gathered, N):
    """The coarse per-point head in one launch on the bf16 matrix instructions (di2p_point_head_x3).  src0 / src1: dense f32[B,ch,N];
    packed: dict W0p, W1p (head_x3_pack), ss f32[4,128] (scale0, shift0, scale1, shift1), relu0, relu1, W2t f32[128,P], sc2, sh2, relu2;
    gathered: [(table f32[B,nodes,128], idx i32[B,N,3], w f32[B,N,3] | None)] x 2.  -> f32[B,P,N]."""
    require_cuda(src0, src1, packed["W0p"], packed["W1p"], packed["ss"], packed["W2t"], packed["sc2"], packed["sh2"])
    B = src0.shape[0]
    P = packed["W2t"].shape[1]
    # raw pointers below: the packs must be the ones made for THIS head (layer 0's dense rows, layer 1), the small operands fp32 of the right size
    k0 = int(src0.shape[1]) + int(src1.shape[1])
    hb = _lib.load().di2p_head_x3_packed_bytes
    if k0 % 16 or packed["W0p"].numel() * packed["W0p"].element_size() != hb(k0) or packed["W1p"].numel() * packed["W1p"].element_size() != hb(128):
        raise RuntimeError("point_head_x3: W0p / W1p must be head_x3_pack of the [%d,128] dense rows and of the [128,128] second layer" % k0)
    for name, n in (("ss", 4 * 128), ("W2t", 128 * P), ("sc2", P), ("sh2", P)):
        if packed[name] is None and name in ("sc2", "sh2"):          # the output layer may come without scale / shift
            continue
        _chk(packed[name], _f32, "point_head_x3 " + name)
        if packed[name].numel() < n:
            raise RuntimeError("point_head_x3: %s holds %d values, needs %d" % (name, packed[name].numel(), n))
    if tuple(packed["W2t"].shape) != (128, P) or not 1 <= P <= 4:
        raise RuntimeError("point_head_x3: W2t must be f32[128,P] with P <= 4")
    h = _lib.HeadX3T()
    for t, x in enumerate((src0, src1)):
        _chk(x, _f32, "head source")
        if x.dim() != 3 or x.shape[2] != N or x.stride(2) != 1:
            raise RuntimeError("head sources must be [B, ch, N] with unit column stride")
        h.src[t], h.batch_stride[t], h.row_stride[t], h.channels[t] = ptr(x), x.stride(0), x.stride(1), x.shape[1]
    for t, (tab, gi, gw) in enumerate(gathered):
        require_cuda(tab, gi, gw)
        _chk(tab, _f32, "gathered table")
        _chk(gi, _i32, "gathered index")
        if tuple(tab.shape[0::2]) != (B, 128) or tuple(gi.shape) != (B, N, 3) or (gw is not None and tuple(gw.shape) != (B, N, 3)):
            raise RuntimeError("the head takes node tables [B,nodes,128] with three neighbours per point")
        h.tab[t], h.idx[t], h.w[t], h.nodes[t] = ptr(tab), ptr(gi), ptr(gw), tab.shape[1]
    h.W0p, h.W1p, h.scale_shift = ptr(packed["W0p"]), ptr(packed["W1p"]), ptr(packed["ss"])
    h.relu0, h.relu1, h.relu2, h.P = int(bool(packed["relu0"])), int(bool(packed["relu1"])), int(bool(packed["relu2"])), P
    h.W2t, h.scale2, h.shift2 = ptr(packed["W2t"]), ptr(packed["sc2"]), ptr(packed["sh2"])
    out = torch.empty((B, P, N), dtype=_f32, device=src0.device)
    _work("di2p_point_head_x3", B * N * ((src0.shape[1] + src1.shape[1]) * 128 + 128 * 128 + 128 * P))
    call("di2p_point_head_x3", ctypes.byref(h), ptr(out), B, N, stream())
    return out


def head_labels_pack(Wt):
    """Wt f32[K,M] (contiguous, K % 16 == 0) -> the fragment-ordered split operand of di2p_point_head_labels_x3 (uint8 storage; rows padded to
    a multiple of 32 with zeros)."""
    require_cuda(Wt)
    _chk(Wt, _f32, "head_labels_pack weights")
    if Wt.dim() != 2 or Wt.shape[0] % 16 or Wt.shape[0] < 16:
        raise RuntimeError("head_labels_pack needs a contiguous f32[K,M] with K % 16 == 0")
    K, M = int(Wt.shape[0]), int(Wt.shape[1])
    Wp = torch.empty((_lib.load().di2p_head_labels_x3_packed_bytes(K, M),), dtype=torch.uint8, device=Wt.device)
    call("di2p_head_labels_x3_pack", ptr(Wt), K, M, ptr(Wp), stream())
    return Wp


def point_head_labels(y0, packed, N, scores_out=None):
    """Layers 1-2 of the fine per-point head and both argmaxes in one launch (di2p_point_head_labels_x3).  y0: layer 0's output f32[B,256,N]
    (unit column stride); packed: dict W1p, W2p (head_labels_pack of W1t f32[256,256] and W2t f32[256,P]), P, sc1, sh1 f32[256], relu1,
    sc2 / sh2 f32[P] or None.  scores_out: an f32[B,P,N] tensor the kernel also writes the scores into (None: no scores).
    -> (coarse i32[B,N], fine i32[B,N]) with the argmax semantics of argmax_channels on the same scores."""
    require_cuda(y0, packed["W1p"], packed["W2p"], packed["sc1"], packed["sh1"], packed["sc2"], packed["sh2"], scores_out)
    _chk(y0, _f32, "point_head_labels y0")
    P = int(packed["P"])
    if y0.dim() != 3 or y0.shape[1] != 256 or y0.shape[2] != N or y0.stride(2) != 1:
        raise RuntimeError("point_head_labels: y0 must be f32[B,256,N] with unit column stride")
    B = int(y0.shape[0])
    # raw pointers below: the packs must be the ones made for THIS head, the small operands fp32 of the right size
    hb = _lib.load().di2p_head_labels_x3_packed_bytes
    if P < 3 or packed["W1p"].numel() * packed["W1p"].element_size() != hb(256, 256) or packed["W2p"].numel() * packed["W2p"].element_size() != hb(256, P):
        raise RuntimeError("point_head_labels: W1p / W2p must be head_labels_pack of the [256,256] layer 1 and of the [256,%d] layer 2 (P >= 3)" % P)
    for name, n in (("sc1", 256), ("sh1", 256), ("sc2", P), ("sh2", P)):
        if packed[name] is None:
            if name in ("sc2", "sh2"):                    # the output layer may come without scale / shift
                continue
            raise RuntimeError("point_head_labels: %s is required" % name)
        _chk(packed[name], _f32, "point_head_labels " + name)
        if packed[name].numel() != n:
            raise RuntimeError("point_head_labels: %s holds %d values, needs %d" % (name, packed[name].numel(), n))
    if scores_out is not None:
        _chk(scores_out, _f32, "point_head_labels scores_out")
        if tuple(scores_out.shape) != (B, P, N) or scores_out.device != y0.device:
            raise RuntimeError("point_head_labels: scores_out must be f32[%d,%d,%d] on the device of y0" % (B, P, N))
    h = _lib.HeadLabelsX3T()
    h.y0, h.batch_stride, h.row_stride, h.K = ptr(y0), y0.stride(0), y0.stride(1), 256
    h.W1p, h.scale1, h.shift1, h.relu1 = ptr(packed["W1p"]), ptr(packed["sc1"]), ptr(packed["sh1"]), int(bool(packed["relu1"]))
    h.W2p, h.scale2, h.shift2, h.P = ptr(packed["W2p"]), ptr(packed["sc2"]), ptr(packed["sh2"]), P
    coarse = torch.empty((B, N), dtype=_i32, device=y0.device)
    fine = torch.empty((B, N), dtype=_i32, device=y0.device)
    h.scores, h.coarse, h.fine = ptr(scores_out), ptr(coarse), ptr(fine)
    _work("di2p_point_head_labels_x3", B * N * 256 * (256 + P))
    call("di2p_point_head_labels_x3", ctypes.byref(h), B, N, stream())
    return coarse, fine


def point_chain_ok(srcs, layers, N):
    """Can di2p_point_chain run these layers ((Wt, scale, shift, relu) tuples; layers[0].Wt holds the rows of the dense `srcs`)?"""
    if len(layers) not in (2, 3) or len(srcs) != 1 or _lib.get_option("pw_nochain"):
        return False
    M = layers[0][0].shape[1]
    if M not in (32, 64) or layers[0][0].shape[0] > M or any(tuple(l[0].shape) != (M, M) for l in layers[1:]):
        return False
    if any(l[0].requires_grad or not l[0].is_contiguous() for l in layers):
        return False
    return srcs[0].mode == _lib.SRC_DENSE and srcs[0].t.stride(2) == 1


def point_chain(srcs, layers, N, batch_bias=None, gathered=None):
    """Fused narrow PointNet chain (di2p_point_chain): two or three (Wt[K,M], scale, shift, relu) layers of one width
    M in {32, 64}; layers[0]'s Wt holds only the rows of the dense `srcs`.  -> f32[B, M, N], bit-identical to the
    separate pointwise_gemm calls."""
    Wt0, sc0, sh0, act0 = layers[0]
    Wt1, sc1, sh1, act1 = layers[1]
    Wt2, sc2, sh2, act2 = layers[2] if len(layers) == 3 else (None, None, None, False)
    B = srcs[0].t.shape[0]
    M = Wt0.shape[1]
    require_cuda(Wt0, Wt1, Wt2, sc0, sh0, sc1, sh1, sc2, sh2, batch_bias)
    e = EpilogueT()
    e.scale, e.shift, e.batch_bias = ptr(sc0), ptr(sh0), ptr(batch_bias)
    e.relu, e.group_max, e.transpose_out = int(bool(act0)), 1, 0
    _fill_gathered(e, gathered, B, M, N)
    out = torch.empty((B, M, N), dtype=_f32, device=Wt0.device)
    _work("di2p_point_chain", B * N * (Wt0.shape[0] * M + (len(layers) - 1) * M * M))
    call("di2p_point_chain", _fill_srcs(srcs), len(srcs), ptr(Wt0), Wt0.shape[0], ctypes.byref(e), ptr(Wt1), ptr(sc1), ptr(sh1),
         int(bool(act1)), ptr(Wt2), ptr(sc2), ptr(sh2), int(bool(act2)), ptr(out), B, M, N, stream())
    return out


def batch_gemv(Wt, k0, v):
    """out[b,m] = sum_k Wt[k0+k, m] v[b,k]."""
    require_cuda(Wt, v)
    B, Kv = v.shape
    M = Wt.shape[1]
    out = torch.empty((B, M), dtype=_f32, device=Wt.device)
    call("di2p_batch_gemv", ptr(Wt), M, int(k0), ptr(v), Kv, ptr(out), B, stream())
    return out


def batch_gemv2(Wt, k0, v0, k1, v1):
    """out[b,m] = sum_k Wt[k0+k, m] v0[b,k] + sum_k Wt[k1+k, m] v1[b,k]  (one launch)."""
    require_cuda(Wt, v0, v1)
    B = v0.shape[0]
    M = Wt.shape[1]
    out = torch.empty((B, M), dtype=_f32, device=Wt.device)
    call("di2p_batch_gemv2", ptr(Wt), M, int(k0), ptr(v0), v0.shape[1], int(k1), ptr(v1), v1.shape[1], ptr(out), B, stream())
    return out


def attention_pool(feat, score):
    """feat f32[B,C,HW], score f32[B,HW,Mn] -> f32[B,C,Mn] = feat@score / HW."""
    require_cuda(feat, score)
    B, C, HW = feat.shape
    Mn = score.shape[2]
    out = torch.empty((B, C, Mn), dtype=_f32, device=feat.device)
    call("di2p_attention_pool", ptr(feat), ptr(score), ptr(out), B, C, HW, Mn, stream())
    return out


def _conv_operands(who, x, Cout, KH, KW, stride, pad, scale, shift, residual):
    """The operand checks the convolution wrappers share -- the kernels read through raw pointers, so a short scale / shift or a smaller
    residual would be read out of bounds: x f32[B,Cin,H,W], scale / shift f32 with at least Cout values, residual (if any) f32 of exactly
    the output shape.  -> (B, Cin, H, W, OH, OW); the caller checks its weight operand against Cin."""
    _chk(x, _f32, who + " input")
    if x.dim() != 4:
        raise RuntimeError("%s takes x f32[B,Cin,H,W]" % who)
    B, Cin, H, W = x.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    for name, v in (("scale", scale), ("shift", shift)):
        if v is None or v.dtype != _f32:
            raise RuntimeError("%s %s must be %s, got %s" % (who, name, _f32, None if v is None else v.dtype))
        if v.numel() < Cout:
            raise RuntimeError("%s: %s holds %d values, needs %d" % (who, name, v.numel(), Cout))
    if residual is not None:
        _chk(residual, _f32, who + " residual")
        if residual.shape != (B, Cout, OH, OW):
            raise RuntimeError("%s: residual must be f32%s, got %s" % (who, (B, Cout, OH, OW), tuple(residual.shape)))
    return B, Cin, H, W, OH, OW


def conv_route(x_shape, w_shape, stride, pad, training=False):
    """Which kernel runs the convolution layer x f32[B,Cin,H,W] * W f32[Cout,Cin,KH,KW]: -> (kernel, cfg), THE statement of the rule for the
    inference network (networks.ImageEncoder), the training step and its input gradient (train_net._Conv2d; the gradient of a stride-1 "same"
    layer is the route of dY with Cin and Cout swapped) and the tests.  A function of the shapes and the library knobs only (host code).
      "x3"         conv3x3_x3 (bf16x3): 3x3 / pad 1, Cin % 16 == 0, the layer's bit of the knob `conv_x3` (bit 4: stride 2; else bit 0..3 for
                   Cout 64 / 128 / 256 / 512 and beyond -- ResNet stage 1..4) and a kernel instance for the shape.  cfg: the tile configuration
                   to pass (-1: the library's choice, which the knob `conv_x3_cfg` overrides).  Inference: stride 2 too (the caller fuses the
                   block's 1x1 downsample branch into the launch).  Training: stride 1, from 16 frames on every such layer, below (the
                   reference's batch of 8) only Cout >= 256 -- the workgroup tiles are sized for whole rounds of the chip at 32 frames; at 8
                   frames the Winograd kernel's smaller tiles win on the two large-image stages (tools/bench_conv_x3.py, B=8: 30.8 / 38.7 us
                   against 29.2 / 42.7) and lose on the small-image ones (48.2 / 73.2 against 29.2 / 46.0 us with the smallest tile
                   configuration, cfg = 3, which the route then names where it runs the shape and the knob forces none)
      "winograd"   conv3x3_winograd: 3x3 / stride 1 / pad 1, Cin % 16 == 0, Cout % 32 == 0, an even width of at least 4.  The knob
                   `conv_nowinograd` takes it away from INFERENCE only: the training step has never read that knob
      "direct_tap" conv2d on the tap-major matrix (16-byte staged): any other layer with Cin % 16 == 0
      "direct"     conv2d on the plain matrix: the rest (the 7x7 stem in training)
    cfg is None for every kernel but "x3"."""
    B, Cin, H, W = x_shape
    Cout, _, KH, KW = w_shape
    if KH == KW == 3 and pad == 1 and Cin % 16 == 0 and stride in (1, 2):
        bit = 4 if stride == 2 else max(0, min(3, int(Cout).bit_length() - 7))
        wanted = not training or (stride == 1 and (B >= 16 or Cout >= 256))
        if wanted and _lib.get_option("conv_x3") >> bit & 1 and conv3x3_x3_supported(x_shape, Cout, stride):
            small = training and B < 16 and _lib.get_option("conv_x3_cfg") < 0 and conv3x3_x3_supported(x_shape, Cout, stride, cfg=3)
            return "x3", 3 if small else -1
        if stride == 1 and Cout % 32 == 0 and W % 2 == 0 and W >= 4 and (training or not _lib.get_option("conv_nowinograd")):
            return "winograd", None
    return ("direct_tap" if Cin % 16 == 0 else "direct"), None


def conv2d(x, Wt, scale, shift, KH, KW, stride, pad, relu, residual=None, tap_major=False):
    """y = relu?(scale * conv(x) + shift + residual) on the implicit-GEMM kernels (di2p_conv2d); Wt f32[KH*KW*Cin, Cout], rows ordered
    (ci,kh,kw) or, tap_major, (kh,kw,ci)."""
    require_cuda(x, Wt, scale, shift, residual)
    _chk(Wt, _f32, "conv2d Wt")
    Cout = Wt.shape[-1]
    B, Cin, H, W, OH, OW = _conv_operands("conv2d", x, Cout, KH, KW, stride, pad, scale, shift, residual)
    if tuple(Wt.shape) != (KH * KW * Cin, Cout):
        raise RuntimeError("conv2d: Wt must be f32[KH*KW*Cin, Cout] = [%d, %d], got %s" % (KH * KW * Cin, Cout, tuple(Wt.shape)))
    y = torch.empty((B, Cout, OH, OW), dtype=_f32, device=x.device)
    args = (ptr(x), ptr(Wt), ptr(scale), ptr(shift), ptr(residual), ptr(y), B, Cin, H, W, Cout, KH, KW,
            stride, pad, int(bool(relu)), int(bool(tap_major)))
    nws = _lib.load().di2p_conv2d_workspace_bytes(B, Cin, H, W, Cout, KH, KW, stride, pad, int(bool(tap_major)))
    if nws > 0:       # split-K scratch (stream-ordered: the caching allocator hands it out per stream)
        ws = torch.empty((nws,), dtype=torch.uint8, device=x.device)
        call("di2p_conv2d_ws", *args, ptr(ws), nws, stream())
    else:
        call("di2p_conv2d", *args, stream())
    return y


def conv3x3_x3_supported(x_shape, Cout, stride, cfg=-1):
    """True if di2p_conv3x3_x3 has a kernel instance for this layer shape (x_shape = (B, Cin, H, W)) in tile configuration cfg (0..3;
    -1: the knob conv_x3_cfg, by default the cheapest)."""
    B, Cin, H, W = x_shape
    return bool(_lib.load().di2p_conv3x3_x3_supported(int(B), int(Cin), int(H), int(W), int(Cout), int(stride), int(cfg)))


CONV_X3_PLAN_FIELDS = ("cfg", "instance", "instances", "fallback", "dbuf", "plan_items", "instance_items", "pwt", "tiles_per_frame", "n_mt",
                       "max_rows", "ragged_segments", "partial_cout", "chunks")


def conv3x3_x3_plan(x_shape, Cout, stride, cfg=-1):
    """What di2p_conv3x3_x3 would launch for this layer (di2p_conv3x3_x3_plan; host code, no GPU needed): None where conv3x3_x3_supported
    is False, else a dict of CONV_X3_PLAN_FIELDS -- the configuration, the kernel instance (index, of `instances`), whether the
    double-buffered plan fell back to a single-buffered instance, the staging items of plan and instance, the instance's compile-time patch
    row length, and the tile geometry (ragged_segments = nseg % NSEG, partial_cout = Cout % MT, chunks = Cin / KS)."""
    B, Cin, H, W = (int(v) for v in x_shape)
    out = (ctypes.c_int32 * len(CONV_X3_PLAN_FIELDS))()
    if not _lib.load().di2p_conv3x3_x3_plan(B, Cin, H, W, int(Cout), int(stride), int(cfg), out):
        return None
    return dict(zip(CONV_X3_PLAN_FIELDS, (int(v) for v in out)))


RC_KINDS = ("strided", "wgrad", "gather")
RC_ROUTE_FIELDS = ("tile", "a_stager", "b_stager", "rch", "chunks")


def rc_vec_ok(ptr, ld, batch_stride, R):
    """True if the reduction GEMMs of the training step may read this strided operand with 16-byte loads (di2p_rc_vec_ok; host code)."""
    return bool(_lib.load().di2p_rc_vec_ok(ptr, int(ld), int(batch_stride), int(R)))


def rc_route(kind, Z, rows, cols, R, a_vec=False, b_vec=False):
    """What a reduction GEMM of the training step would launch (di2p_rc_route: the launcher's own routing function; host code, no GPU
    needed): a dict of RC_ROUTE_FIELDS -- tile (64 / 128), the stagers of A and B (0 scalar, 1 16-byte), reduction indices per chunk and
    chunks.  kind: "strided" (di2p_bmm_rc), "wgrad" (di2p_conv2d_wgrad: rows = Cout, cols = Cin*KH*KW, R = OH*OW), "gather"
    (di2p_gather_backward: rows = C, cols = M, R = J); a_vec / b_vec: rc_vec_ok of the strided operands."""
    out = (ctypes.c_int32 * len(RC_ROUTE_FIELDS))()
    _lib.call("di2p_rc_route", RC_KINDS.index(kind), int(Z), int(rows), int(cols), int(R), int(bool(a_vec)), int(bool(b_vec)), out)
    return dict(zip(RC_ROUTE_FIELDS, (int(v) for v in out)))


PW_ROUTE_FIELDS = ("vec", "bm", "bn", "dense", "depth", "bk")
CONV2D_ROUTE_FIELDS = ("kernel", "bm", "bn", "bk", "variant", "depth", "splits")
CONV2D_KERNELS = ("scalar", "vec", "stem_row")
WINO_ROUTE_FIELDS = ("reg", "cob", "kc", "waves", "n_tb", "tiles", "n_cb", "grid")
CHAIN_ROUTE_FIELDS = ("M", "ks0", "layers", "tn", "nblk", "total", "wgs", "w")
HEAD_ROUTE_FIELDS = ("reg", "g33", "bn", "nblk", "total", "wgs")


def _route(name, fields, *args):
    out = (ctypes.c_int32 * len(fields))()
    _lib.call(name, *(int(a) for a in args), out)
    return dict(zip(fields, (int(v) for v in out)))


def pointwise_route(M, K, N, B=1, dense=True, wt_aligned=True):
    """What di2p_pointwise_gemm would launch (di2p_pointwise_route: the entry's own routing function; host code, no GPU needed): a dict of
    PW_ROUTE_FIELDS -- stager (vec 0 scalar / 1 16-byte), tile bm x bn, the dense loader, prefetch depth and K-step.  dense: every source
    dense with strides % 4 == 0 and a 16-byte aligned base; wt_aligned: Wt 16-byte aligned."""
    return _route("di2p_pointwise_route", PW_ROUTE_FIELDS, M, K, N, B, bool(dense), bool(wt_aligned))


def conv2d_route(x_shape, Cout, KH, KW, stride, pad, tap_major=False, x_aligned=True, wt_aligned=True, workspace_bytes=0):
    """What di2p_conv2d / di2p_conv2d_ws would launch (di2p_conv2d_route; host code): a dict of CONV2D_ROUTE_FIELDS -- kernel (an index
    into CONV2D_KERNELS), tile, K-step, stride variant (1, 2, 22 = aligned windows; 0 off the 16-byte stager), prefetch depth and the
    K-slices actually used with a 16-byte aligned workspace of workspace_bytes (0: none)."""
    B, Cin, H, W = x_shape
    return _route("di2p_conv2d_route", CONV2D_ROUTE_FIELDS, B, Cin, H, W, Cout, KH, KW, stride, pad, bool(tap_major), bool(x_aligned),
                  bool(wt_aligned), workspace_bytes)


def conv2d_workspace_bytes(x_shape, Cout, KH, KW, stride, pad, tap_major=False):
    """The split-K workspace conv2d wants for this shape (di2p_conv2d_workspace_bytes; 0: no split, or a shape conv2d refuses)."""
    B, Cin, H, W = x_shape
    return int(_lib.load().di2p_conv2d_workspace_bytes(int(B), int(Cin), int(H), int(W), int(Cout), int(KH), int(KW), int(stride), int(pad),
                                                       int(bool(tap_major))))


def winograd_route(x_shape, Cout):
    """What di2p_conv3x3_winograd would launch (di2p_winograd_route; host code): a dict of WINO_ROUTE_FIELDS -- kernel (reg 0 LDS-panel /
    1 register-resident), output channels per workgroup, K-step, waves, tile blocks, tiles per block, co-blocks, workgroups."""
    B, Cin, H, W = x_shape
    return _route("di2p_winograd_route", WINO_ROUTE_FIELDS, B, Cin, H, W, Cout)


def point_chain_route(M, K0, layers, B, N, cus):
    """What di2p_point_chain would launch on `cus` compute units (di2p_point_chain_route; host code): a dict of CHAIN_ROUTE_FIELDS."""
    return _route("di2p_point_chain_route", CHAIN_ROUTE_FIELDS, M, K0, layers, B, N, cus)


def point_head_route(K0, n_src, c0, B, N, cus, g33=False, reg_range=True):
    """What di2p_point_head would launch on `cus` compute units (di2p_point_head_route; host code): a dict of HEAD_ROUTE_FIELDS."""
    return _route("di2p_point_head_route", HEAD_ROUTE_FIELDS, K0, n_src, c0, bool(reg_range), bool(g33), B, N, cus)


def conv3x3_x3(x, Wp, Cout, scale, shift, stride, relu, residual=None, downsample=None, cfg=-1):
    """3x3 / pad 1 convolution on the bf16 matrix instructions with exact three-way fp32 splits (di2p_conv3x3_x3):
    y = relu?(scale * conv(x) + shift + residual).  Wp = bf16x3_pack(tap-major Wt[9 Cin, Cout]).  stride 2 takes
    downsample = (Wp_ds, scale_ds, shift_ds) -- the BasicBlock's 1x1 / stride-2 branch of the same input (resnet.py:160-164) -- and
    returns (y, y_ds).  cfg: the tile configuration, as for conv3x3_x3_supported."""
    require_cuda(x, Wp, scale, shift, residual)
    B, Cin, H, W, OH, OW = _conv_operands("conv3x3_x3", x, Cout, 3, 3, stride, 1, scale, shift, residual)
    # a pack made for another layer shape would be read out of bounds like a short scale or a smaller residual
    packed_bytes = _lib.load().di2p_bf16x3_packed_bytes
    if Wp.numel() * Wp.element_size() != packed_bytes(9 * Cin, int(Cout)):
        raise RuntimeError("conv3x3_x3: Wp is not bf16x3_pack of a [9*%d, %d] matrix (%d bytes, expected %d)" % (Cin, Cout, Wp.numel() * Wp.element_size(), packed_bytes(9 * Cin, int(Cout))))
    y = torch.empty((B, Cout, OH, OW), dtype=_f32, device=x.device)
    Wd = sd = hd = yd = None
    if downsample is not None:
        Wd, sd, hd = downsample
        require_cuda(Wd, sd, hd)
        if Wd.numel() * Wd.element_size() != packed_bytes(Cin, int(Cout)):
            raise RuntimeError("conv3x3_x3: the downsample pack is not bf16x3_pack of a [%d, %d] matrix" % (Cin, Cout))
        _chk(sd, _f32, "conv3x3_x3 downsample scale"); _chk(hd, _f32, "conv3x3_x3 downsample shift")
        if sd.numel() < Cout or hd.numel() < Cout:
            raise RuntimeError("conv3x3_x3: downsample scale / shift need %d values" % Cout)
        yd = torch.empty((B, Cout, OH, OW), dtype=_f32, device=x.device)
    _work("di2p_conv3x3_x3", B * Cout * Cin * (9 + (1 if downsample is not None else 0)) * OH * OW)
    call("di2p_conv3x3_x3", ptr(x), ptr(Wp), ptr(scale), ptr(shift), ptr(residual), ptr(y), B, Cin, H, W, Cout, int(stride), int(bool(relu)),
         ptr(Wd), ptr(sd), ptr(hd), ptr(yd), int(cfg), stream())
    return (y, yd) if downsample is not None else y


def stem_weights(weight):
    """weight f32[64,3,7,7] -> Wp f32[168,64]: the packed filter bank of conv_stem."""
    require_cuda(weight)
    if tuple(weight.shape) != (64, 3, 7, 7) or weight.dtype != _f32:
        raise RuntimeError("stem_weights needs the f32[64,3,7,7] ResNet stem filter")
    w = weight.detach().contiguous()
    Wp = torch.empty((168, 64), dtype=_f32, device=w.device)
    call("di2p_stem_pack", ptr(w), ptr(Wp), stream())
    return Wp


def conv_stem(x, Wp, scale, shift, relu=True):
    """ResNet stem: y = relu?(scale * conv7x7/2(x) + shift); x f32[B,3,H,W] -> f32[B,64,OH,OW]."""
    require_cuda(x, Wp, scale, shift)
    B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError("the stem takes 3 input channels")
    y = torch.empty((B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=_f32, device=x.device)
    call("di2p_conv7x7s2_stem", ptr(x), ptr(Wp), ptr(scale), ptr(shift), ptr(y), B, H, W, int(bool(relu)), stream())
    return y


def stem_x3_weights(weight):
    """weight f32[64,3,7,7] -> the split, fragment-ordered operand of stem_x3 (uint8 storage)."""
    require_cuda(weight)
    if tuple(weight.shape) != (64, 3, 7, 7) or weight.dtype != _f32:
        raise RuntimeError("stem_x3_weights needs the f32[64,3,7,7] ResNet stem filter")
    w = weight.detach().contiguous()
    Wp = torch.empty((_lib.load().di2p_stem_x3_packed_bytes(),), dtype=torch.uint8, device=w.device)
    call("di2p_stem_x3_pack", ptr(w), ptr(Wp), stream())
    return Wp


def stem_x3_supported(H, W):
    return bool(_lib.load().di2p_stem_x3_supported(int(H), int(W)))


def stem_x3(x, Wp, scale, shift):
    """conv1 + bn1 + relu + maxpool of the image branch in one launch (di2p_stem_x3): x f32[B,3,H,W] -> f32[B,64,H/4,W/4]."""
    require_cuda(x, Wp, scale, shift)
    _chk(x, _f32, "stem_x3 input"); _chk(scale, _f32, "stem_x3 scale"); _chk(shift, _f32, "stem_x3 shift")
    if x.dim() != 4:
        raise RuntimeError("stem_x3 takes x f32[B,3,H,W]")
    B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError("the stem takes 3 input channels")
    if Wp.numel() * Wp.element_size() != _lib.load().di2p_stem_x3_packed_bytes() or scale.numel() < 64 or shift.numel() < 64:
        raise RuntimeError("stem_x3: Wp must be stem_x3_weights(...) and scale / shift hold 64 values")
    y = torch.empty((B, 64, H // 4, W // 4), dtype=_f32, device=x.device)
    _work("di2p_stem_x3", B * 64 * 147 * (H // 2) * (W // 2))
    call("di2p_stem_x3", ptr(x), ptr(Wp), ptr(scale), ptr(shift), ptr(y), B, H, W, stream())
    return y


def winograd_weights(weight):
    """weight f32[Cout,Cin,3,3] -> U f32[16,Cin,Cout] = G g G^T per (ci, co): the operand of conv3x3_winograd."""
    Cout, Cin, KH, KW = weight.shape
    if (KH, KW) != (3, 3) or weight.dtype != _f32:
        raise RuntimeError("winograd_weights needs an f32 3x3 filter bank")
    w = weight.detach().contiguous()          # (a flipped / transposed view is fine: the training path passes one)
    require_cuda(w)
    U = torch.empty((16, Cin, Cout), dtype=_f32, device=w.device)
    call("di2p_winograd_weight_transform", ptr(w), ptr(U), Cin, Cout, stream())
    return U


def winograd_weights_dgrad(weight):
    """weight f32[Cout,Cin,3,3] of a stride-1 3x3 layer -> U f32[16,Cout,Cin]: the transformed filter of the layer's INPUT GRADIENT (the
    convolution of dY with the flipped, channel-transposed filter), in one launch."""
    Cout, Cin, KH, KW = weight.shape
    if (KH, KW) != (3, 3) or weight.dtype != _f32:
        raise RuntimeError("winograd_weights_dgrad needs an f32 3x3 filter bank")
    w = weight.detach().contiguous()
    require_cuda(w)
    U = torch.empty((16, Cout, Cin), dtype=_f32, device=w.device)
    call("di2p_winograd_weight_transform_dgrad", ptr(w), ptr(U), Cout, Cin, stream())
    return U


def conv3x3_winograd(x, U, scale, shift, relu, residual=None):
    """3x3 / stride 1 / pad 1 convolution via Winograd F(2x2,3x3): y = relu?(scale * conv(x) + shift + residual)."""
    require_cuda(x, U, scale, shift, residual)
    _chk(U, _f32, "conv3x3_winograd U")
    Cout = U.shape[-1]
    B, Cin, H, W, _, _ = _conv_operands("conv3x3_winograd", x, Cout, 3, 3, 1, 1, scale, shift, residual)
    if tuple(U.shape) != (16, Cin, Cout):
        raise RuntimeError("U must be f32[16, Cin, Cout] = [16, %d, %d], got %s" % (Cin, Cout, tuple(U.shape)))
    y = torch.empty((B, Cout, H, W), dtype=_f32, device=x.device)
    _work("di2p_conv3x3_winograd", B * Cout * Cin * 16 * ((H + 1) // 2) * ((W + 1) // 2))
    call("di2p_conv3x3_winograd", ptr(x), ptr(U), ptr(scale), ptr(shift), ptr(residual), ptr(y), B, Cin, H, W, Cout, int(bool(relu)), stream())
    return y


def maxpool3x3s2(x):
    require_cuda(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=_f32, device=x.device)
    call("di2p_maxpool3x3s2", ptr(x), ptr(y), B, C, H, W, stream())
    return y


def global_avgpool(x):
    require_cuda(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, 1, 1), dtype=_f32, device=x.device)
    call("di2p_global_avgpool", ptr(x), ptr(y), B, C, H * W, stream())
    return y


# ------------------------------------------------------------------------------------ solver
def _dbl3(v):
    a = (ctypes.c_double * 3)()
    for i in range(3):
        a[i] = float(v[i])      # IndexError on short lists, like the reference's .at(i)
    return a


def initial_guess(points64, labels):
    require_cuda(points64, labels)
    F, _, N = points64.shape
    yaw0 = torch.empty((F,), dtype=_f64, device=points64.device)
    labels_out = torch.empty_like(labels)
    has_inside = torch.empty((F,), dtype=_i32, device=points64.device)
    call("di2p_initial_guess", ptr(points64), ptr(labels), ptr(yaw0), ptr(labels_out), ptr(has_inside), F, N, stream())
    return yaw0, labels_out, has_inside


def solve_batched(points, labels, K, init_y, init_T, H, W, lb, ub, max_iter, is_2d, yaw0=None, sweeps=None, workspace=None):
    """points f64|f32 [F,3,N], labels i32[F,N], K f64[F,3,3], init_y f64[F,R], init_T f64[F,R,3]
    -> params f64[F,R,np], cost f64[F,R], iters i32[F,R].
    workspace: caller-owned uint8 tensor of at least di2p_solve_workspace_bytes(F, R, N) bytes on the points' device, used instead of
    the internal allocation (the C API takes it from the caller anyway; tests read the prepared frames back from it)."""
    require_cuda(points, labels, K, init_y, init_T, yaw0, workspace)
    _chk(labels, _i32, "labels")
    _chk(K, _f64, "K")
    _chk(init_y, _f64, "init_y")
    _chk(init_T, _f64, "init_T")
    F, _, N = points.shape
    R = init_y.shape[1]
    npar = 4 if is_2d else 6
    params = torch.empty((F, R, npar), dtype=_f64, device=points.device)
    cost = torch.empty((F, R), dtype=_f64, device=points.device)
    iters = torch.empty((F, R), dtype=_i32, device=points.device)
    name = "di2p_solve_batched" if points.dtype == _f64 else "di2p_solve_batched_f32"
    if points.dtype not in (_f64, _f32):
        raise RuntimeError("points must be float64 or float32")
    need = _lib.load().di2p_solve_workspace_bytes(F, R, N)
    if workspace is None:
        ws = torch.empty((need,), dtype=torch.uint8, device=points.device)
    else:
        ws = workspace
        _chk(ws, torch.uint8, "workspace")
        if ws.device != points.device:
            raise RuntimeError("workspace must be on the points' device")
        if ws.numel() < need:
            raise RuntimeError("workspace has %d bytes, di2p_solve_workspace_bytes(%d, %d, %d) = %d" % (ws.numel(), F, R, N, need))
    call(name, ptr(points), ptr(labels), ptr(K), ptr(init_y), ptr(init_T), ptr(yaw0), float(H), float(W), _dbl3(lb),
         _dbl3(ub), int(max_iter), int(bool(is_2d)), F, R, N, ptr(params), ptr(cost), ptr(iters), ptr(sweeps), ptr(ws), stream())
    return params, cost, iters


def select_best(params, cost, is_2d, has_inside=None):
    require_cuda(params, cost, has_inside)
    F, R = cost.shape
    best = torch.empty((F,), dtype=_i32, device=cost.device)
    P = torch.empty((F, 4, 4), dtype=_f64, device=cost.device)
    bc = torch.empty((F,), dtype=_f64, device=cost.device)
    call("di2p_select_best", ptr(params), ptr(cost), ptr(has_inside), int(bool(is_2d)), F, R, ptr(best), ptr(P), ptr(bc), stream())
    return best, P, bc


def solver_residuals(points64, labels, K, params, H, W, is_2d):
    require_cuda(points64, labels, K, params)
    F, _, N = points64.shape
    res = torch.empty((F, 3 * N), dtype=_f64, device=points64.device)
    counts = torch.empty((F,), dtype=_i32, device=points64.device)
    cost = torch.empty((F,), dtype=_f64, device=points64.device)
    call("di2p_solver_residuals", ptr(points64), ptr(labels), ptr(K), ptr(params), float(H), float(W), int(bool(is_2d)),
         F, N, ptr(res), ptr(counts), ptr(cost), stream())
    return res, counts, cost


# ------------------------------------------------------------------------------------ pose confidence
def _npar(is_2d):
    return 4 if is_2d else 6


def pose_information_workspace(F, N, device):
    """A workspace for pose_information_into: di2p_pose_information_workspace_bytes(F, N) bytes as a uint8 tensor"""
    need = int(_lib.load().di2p_pose_information_workspace_bytes(int(F), int(N)))
    return torch.empty((max(need, 8),), dtype=torch.uint8, device=device)


def pose_information_into(points, labels, K, params, H, W, is_2d, info, grad, cost, active, workspace):
    """pose_information with the outputs and the workspace supplied: two launches, no allocation -- the form graphs capture."""
    require_cuda(points, labels, K, params, info, grad, cost, active, workspace)
    _chk(points, _f32, "points")
    _chk(labels, _i32, "labels")
    _chk(K, _f64, "K")
    _chk(params, _f64, "params")
    if points.dim() != 3 or points.shape[1] != 3:
        raise ValueError("pose_information: points must be f32 [F,3,N]")
    F, _, N = points.shape
    npar = _npar(is_2d)
    if tuple(labels.shape) != (F, N) or tuple(K.shape) != (F, 3, 3) or tuple(params.shape) != (F, npar):
        raise ValueError("pose_information: labels must be i32 [F,N], K f64 [F,3,3] and params f64 [F,%d]" % npar)
    if (info.dtype, grad.dtype, cost.dtype, active.dtype) != (_f64, _f64, _f64, _i32) or tuple(info.shape) != (F, npar, npar) \
            or tuple(grad.shape) != (F, npar) or tuple(cost.shape) != (F,) or tuple(active.shape) != (F, 2):
        raise ValueError("pose_information: outputs must be info f64[F,np,np], grad f64[F,np], cost f64[F], active i32[F,2]")
    need = int(_lib.load().di2p_pose_information_workspace_bytes(F, N))
    if workspace.dtype != torch.uint8 or workspace.numel() < need:
        raise ValueError("pose_information: the workspace must be uint8 with at least di2p_pose_information_workspace_bytes(%d, %d) = %d bytes"
                         % (F, N, need))
    call("di2p_pose_information", ptr(points), ptr(labels), ptr(K), ptr(params), float(H), float(W), int(bool(is_2d)), F, N, ptr(info),
         ptr(grad), ptr(cost), ptr(active), ptr(workspace), stream())
    return info, grad, cost, active


def pose_information(points, labels, K, params, H, W, is_2d, workspace=None):
    """The Cauchy-weighted normal matrix, gradient and cost of the registration problem at GIVEN parameters (csrc/solver_aux.hip).
    points f32[F,3,N], labels i32[F,N] (labels outside {0, 1} are skipped), K f64[F,3,3], params f64[F,np]
    -> info f64[F,np,np] = sum rho'(s) J^T J, grad f64[F,np] = sum rho'(s) J^T r, cost f64[F] = 1/2 sum log1p(s), active i32[F,2] (label-1 /
    label-0 points with a non-zero residual block).  In the solver's parameterisation; deterministic (no atomics), independent of F."""
    F, _, N = points.shape
    npar = _npar(is_2d)
    dev = points.device
    info = torch.empty((F, npar, npar), dtype=_f64, device=dev)
    grad = torch.empty((F, npar), dtype=_f64, device=dev)
    cost = torch.empty((F,), dtype=_f64, device=dev)
    active = torch.empty((F, 2), dtype=_i32, device=dev)
    ws = workspace if workspace is not None else pose_information_workspace(F, N, dev)
    return pose_information_into(points, labels, K, params, H, W, is_2d, info, grad, cost, active, ws)


def gather_best_params(params, best, is_2d):
    """params f64[F,R,np], best i32[F] -> f64[F,np] = params[f, best[f]] (best outside [0, R): restart 0), on the device"""
    require_cuda(params, best)
    _chk(params, _f64, "params")
    _chk(best, _i32, "best")
    npar = _npar(is_2d)
    if params.dim() != 3 or params.shape[2] != npar or best.numel() != params.shape[0] or params.shape[1] < 1:
        raise ValueError("gather_best_params: params must be f64 [F,R,%d] with R >= 1 and best i32 [F]" % npar)
    F, R = int(params.shape[0]), int(params.shape[1])
    out = torch.empty((F, npar), dtype=_f64, device=params.device)
    call("di2p_gather_best_params", ptr(params), ptr(best), int(bool(is_2d)), F, R, ptr(out), stream())
    return out


def pose_covariance(info, params, lb, ub, is_2d, has_inside=None):
    """The bounded inverse of the information matrix.  info f64[F,np,np], params f64[F,np], lb / ub: the solve's translation bounds (3 values
    each), has_inside i32[F] | None -> (cov f64[F,np,np], free_mask i32[F], status i32[F], sigma_t f64[F], sigma_r f64[F] in degrees).
    A translation parameter exactly on a bound is fixed (removed before the inversion, 0 in cov); status 0 ok, 1 not positive definite, 2
    has_inside == 0 or non-finite input (then cov and the sigmas are NaN).  The sigmas carry no fitted noise scale: they compare frames of one
    configuration with each other, they are not metres or degrees of expected error (include/deepi2p_hip.h)."""
    require_cuda(info, params, has_inside)
    _chk(info, _f64, "info")
    _chk(params, _f64, "params")
    npar = _npar(is_2d)
    F = int(info.shape[0])
    if tuple(info.shape) != (F, npar, npar) or tuple(params.shape) != (F, npar):
        raise ValueError("pose_covariance: info must be f64 [F,%d,%d] and params f64 [F,%d]" % (npar, npar, npar))
    if has_inside is not None and (has_inside.dtype != _i32 or has_inside.numel() != F):
        raise ValueError("pose_covariance: has_inside must be i32 [F]")
    dev = info.device
    cov = torch.empty((F, npar, npar), dtype=_f64, device=dev)
    free_mask = torch.empty((F,), dtype=_i32, device=dev)
    status = torch.empty((F,), dtype=_i32, device=dev)
    sigma_t = torch.empty((F,), dtype=_f64, device=dev)
    sigma_r = torch.empty((F,), dtype=_f64, device=dev)
    call("di2p_pose_covariance", ptr(info), ptr(params), ptr(has_inside), _dbl3(lb), _dbl3(ub), int(bool(is_2d)), F, ptr(cov), ptr(free_mask),
         ptr(status), ptr(sigma_t), ptr(sigma_r), stream())
    return cov, free_mask, status, sigma_t, sigma_r


def restart_consensus(params, cost, best, is_2d, t_tol=2.0, r_tol_deg=5.0, has_inside=None):
    """What the other restarts of a multi-start solve say about the selected one.  params f64[F,R,np], cost f64[F,R], best i32[F]
    -> (finite i32[F]: restarts with a finite cost; agree i32[F]: those within t_tol / r_tol_deg of the best pose by get_P_diff's rule on
    P_r^-1 P_best, the best included; gap f64[F]: the cheapest disagreeing restart's cost minus the best's, +inf when all agree).
    Frames with has_inside == 0 (or best outside [0, R)) get 0, 0, NaN."""
    require_cuda(params, cost, best, has_inside)
    _chk(params, _f64, "params")
    _chk(cost, _f64, "cost")
    _chk(best, _i32, "best")
    npar = _npar(is_2d)
    if cost.dim() != 2 or cost.shape[1] < 1 or tuple(params.shape) != (cost.shape[0], cost.shape[1], npar) or best.numel() != cost.shape[0]:
        raise ValueError("restart_consensus: params must be f64 [F,R,%d], cost f64 [F,R] with R >= 1 and best i32 [F]" % npar)
    F, R = int(cost.shape[0]), int(cost.shape[1])
    if has_inside is not None and (has_inside.dtype != _i32 or has_inside.numel() != F):
        raise ValueError("restart_consensus: has_inside must be i32 [F]")
    dev = cost.device
    finite = torch.empty((F,), dtype=_i32, device=dev)
    agree = torch.empty((F,), dtype=_i32, device=dev)
    gap = torch.empty((F,), dtype=_f64, device=dev)
    call("di2p_restart_consensus", ptr(params), ptr(cost), ptr(best), ptr(has_inside), int(bool(is_2d)), F, R, float(t_tol), float(r_tol_deg),
         ptr(finite), ptr(agree), ptr(gap), stream())
    return finite, agree, gap
