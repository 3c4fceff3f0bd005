"""Raw LiDAR scan preparation on the device (csrc/scan_prep.hip, include/deepi2p_hip.h).

Open3D voxel_down_sample + estimate_normals     data/kitti/kitti_pc_bin_to_npy_with_downsample_sn.py:50-74
  + orient_normals_to_align_with_direction + cKDTree 1-NN intensity                             (voxel 0.1, sn_radius 0.6, max_nn 30)
downsample_with_intensity_sn (0.3 m) + downsample_np + the rigid transform into the camera frame
                                                data/kitti_pc_img_pose_loader.py:26-44,158-171,296-306,380

A batch is ragged: one device buffer f32[total, 4] of KITTI .bin rows (x, y, z, intensity) and i32[B+1] frame offsets.  The wrappers
here synchronise only to trim ragged outputs and to check the per-frame status; BatchPlan.run (prepare_batch_into) never does.
"""
import numpy as np
import torch

from . import _lib, _ragged
from ._lib import DeepI2PHipError, call, ptr, require_cuda, stream
from ._ragged import MAX_FRAME_POINTS, _dev

MAX_EXTENT = 2048.0          # default bound (m) on the bounding-box edge of a frame: frames above it are rejected (status 2)
NORMALS_METHODS = {"query": "di2p_estimate_normals", "cells": "di2p_estimate_normals_cells"}
NORMALS_CELL_CANDIDATES = 960          # di2p_normals_cells_candidates(): the LDS candidate capacity of a cell of the "cells" kernel
_STATUS = {1: "more than max_frame_points points", 2: "bounding box above max_extent / voxel index span above 2^21", 3: "bad frame offsets"}


def pack(frames, device=None, cols=4):
    """list of [n_b, cols] arrays / tensors -> (f32[total, cols] device, i32[B+1] device offsets, host offsets list)"""
    device = device or _dev()
    parts = [torch.as_tensor(np.asarray(f, dtype=np.float32) if not torch.is_tensor(f) else f).to(device, torch.float32).reshape(-1, cols)
             for f in frames]
    counts = [int(p.shape[0]) for p in parts]
    host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat = torch.cat(parts, 0).contiguous() if parts and host[-1] > 0 else torch.zeros((max(1, int(host[-1])), cols), dtype=torch.float32, device=device)
    return flat, torch.tensor(host, dtype=torch.int32, device=device), [int(x) for x in host]


def workspace(B, cap, device=None):
    return _ragged.workspace("di2p_scan_prep_workspace_bytes", B, cap, device)


def check_status(status):
    """Raise DeepI2PHipError for a rejected frame (synchronises)."""
    _ragged.check_status("scan_prep", "frame", _STATUS, status)


class VoxelState:
    """Outputs of voxel_down_sample, ragged with device offsets; ws carries the batch on to estimate_normals / nearest_raw."""

    def __init__(self, B, cap, voxel, ws, offsets, points, intensity, normals, keys, status):
        self.B, self.cap, self.voxel, self.ws = B, cap, voxel, ws
        self.offsets, self.points, self.intensity, self.normals, self.keys, self.status = offsets, points, intensity, normals, keys, status


def voxel_down_sample(points, offsets, voxel, normals=None, min_points=0, want_keys=False, cap=None, ws=None,
                      max_frame_points=MAX_FRAME_POINTS, max_extent=MAX_EXTENT):
    """points f32[total,4], offsets i32[B+1] (device) -> VoxelState (points f32[cap,3], intensity f32[cap], normals f32[cap,3] when
    `normals` f32[total,3] is given, keys i64[cap] on request; rows out.offsets[b] .. out.offsets[b+1] belong to frame b)."""
    require_cuda(points, offsets, normals)
    B = offsets.shape[0] - 1
    cap = int(points.shape[0]) if cap is None else int(cap)
    dev = points.device
    ws = workspace(B, cap, dev) if ws is None else ws
    out_off = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    pts = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=dev)
    inten = torch.empty((max(cap, 1),), dtype=torch.float32, device=dev)
    nrm = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=dev) if normals is not None else None
    keys = torch.empty((max(cap, 1),), dtype=torch.int64, device=dev) if want_keys else None
    status = torch.empty((max(B, 1),), dtype=torch.int32, device=dev)
    call("di2p_voxel_down_sample", ptr(points), ptr(offsets), B, cap, int(max_frame_points), float(voxel), float(max_extent), int(min_points),
         ptr(normals), ptr(out_off), ptr(pts), ptr(inten), ptr(nrm), ptr(keys), ptr(status), ptr(ws), stream())
    return VoxelState(B, cap, float(voxel), ws, out_off, pts, inten, nrm, keys, status)


def _normals_entry(method):
    if method not in NORMALS_METHODS:
        raise ValueError("scan_prep: unknown normals method %r (query, cells)" % (method,))
    return NORMALS_METHODS[method]


def estimate_normals(state, radius=0.6, max_nn=30, want_neighbors=False, max_extent=MAX_EXTENT, method="query"):
    """-> normals f32[cap,3] (+ nn_count i32[cap], nn_idx i32[cap,max_nn] with want_neighbors) for the points of `state`.
    method "query": one wave per query point (di2p_estimate_normals); "cells": one workgroup per occupied grid cell
    (di2p_estimate_normals_cells) -- the same outputs bit for bit."""
    entry = _normals_entry(method)
    dev = state.points.device
    normals = torch.empty((max(state.cap, 1), 3), dtype=torch.float32, device=dev)
    cnt = torch.empty((max(state.cap, 1),), dtype=torch.int32, device=dev) if want_neighbors else None
    idx = torch.empty((max(state.cap, 1), int(max_nn)), dtype=torch.int32, device=dev) if want_neighbors else None
    call(entry, ptr(state.offsets), state.B, state.cap, float(radius), int(max_nn), float(max_extent), ptr(normals), ptr(cnt),
         ptr(idx), ptr(state.ws), stream())
    return (normals, cnt, idx) if want_neighbors else normals


def nearest_raw(state, points, offsets):
    """-> (index i32[cap] frame-local, intensity f32[cap], d2 f64[cap]) of the nearest raw point of every output point of `state`."""
    dev = state.points.device
    idx = torch.empty((max(state.cap, 1),), dtype=torch.int32, device=dev)
    inten = torch.empty((max(state.cap, 1),), dtype=torch.float32, device=dev)
    d2 = torch.empty((max(state.cap, 1),), dtype=torch.float64, device=dev)
    call("di2p_nearest_raw", ptr(points), ptr(offsets), ptr(state.offsets), state.B, state.cap, state.voxel, ptr(idx), ptr(inten), ptr(d2),
         ptr(state.ws), stream())
    return idx, inten, d2


def range_shuffle(points, offsets, max_range, seed=0, seed_dev=None, max_frame_points=MAX_FRAME_POINTS, cap=None, out=None, ws=None):
    """di2p_range_shuffle (the Oxford loader's shuffle and horizontal range filter): points f32[>=total,4], offsets i32[B+1] (device) ->
    (points f32[cap,4], offsets i32[B+1], status i32[B]): per frame the points with x^2 + z^2 < max_range^2 (float32; max_range <= 0: all) in
    the order of their Philox keys.  out = (points, offsets, status) preallocated, ws the scan_prep workspace of (B, cap).  No synchronisation."""
    require_cuda(points, offsets, seed_dev)
    B = offsets.shape[0] - 1
    cap = int(points.shape[0]) if cap is None else int(cap)
    dev = points.device
    if out is None:
        out = (torch.zeros((max(cap, 1), 4), dtype=torch.float32, device=dev), torch.zeros((B + 1,), dtype=torch.int32, device=dev),
               torch.zeros((max(B, 1),), dtype=torch.int32, device=dev))
    ws = workspace(B, cap, dev) if ws is None else ws
    call("di2p_range_shuffle", ptr(points), ptr(offsets), B, cap, int(max_frame_points), float(max_range), 0 if seed_dev is not None else int(seed),
         ptr(seed_dev), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws), stream())
    return out


def random_choice_ragged(seed, offsets, max_src, n_out, stream_id=0, out=None, ws=None):
    """-> i32[B, n_out] frame-local indices: prep.downsample's draw per frame with that frame's own count (device offsets)."""
    B = offsets.shape[0] - 1
    out = torch.empty((B, n_out), dtype=torch.int32, device=offsets.device) if out is None else out
    if ws is None:
        ws = torch.empty((_lib.load().di2p_random_choice_ragged_workspace_bytes(B, max_src),), dtype=torch.uint8, device=offsets.device)
    call("di2p_random_choice_ragged", int(seed), int(stream_id), B, ptr(offsets), int(max_src), int(n_out), ptr(out), ptr(ws), stream())
    return out


def gather_ragged(points, intensity, normals, offsets, idx, transform=None, out=None):
    """-> (pc f32[B,3,n], intensity f32[B,1,n], sn f32[B,3,n]); transform f64[B,4,4] (device) moves points by [R|t], normals by R."""
    B, n = idx.shape
    dev = idx.device
    if out is None:
        out = (torch.empty((B, 3, n), dtype=torch.float32, device=dev), torch.empty((B, 1, n), dtype=torch.float32, device=dev),
               torch.empty((B, 3, n), dtype=torch.float32, device=dev) if normals is not None else None)
    pc, it, sn = out
    call("di2p_gather_ragged", ptr(points), ptr(intensity), ptr(normals), ptr(offsets), ptr(idx), ptr(transform), B, n, ptr(pc), ptr(it), ptr(sn),
         stream())
    return pc, it, sn



def preprocess_velodyne(scans, voxel=0.1, sn_radius=0.6, sn_max_nn=30, device=None, method="query"):
    """The offline script's record per raw scan ([n,4] f32 rows x, y, z, intensity): a list of f32[7, m] device tensors (points, the
    intensity of the nearest raw point, oriented normals), rows in ascending voxel key.  Synchronises (ragged trim, status).
    method: the normals kernel (estimate_normals)."""
    _normals_entry(method)
    points, offsets, _ = pack(scans, device)
    st = voxel_down_sample(points, offsets, voxel, cap=points.shape[0])
    normals = estimate_normals(st, sn_radius, sn_max_nn, method=method)
    _, inten, _ = nearest_raw(st, points, offsets)
    check_status(st.status[:st.B])
    host = st.offsets.cpu().tolist()
    rec = torch.cat((st.points, inten[:, None], normals), 1)
    return [rec[host[b]:host[b + 1]].t().contiguous() for b in range(st.B)]


class BatchPlan:
    """Fixed-capacity, preallocated form of prepare_batch: run() launches every stage on the current stream with no host
    synchronisation and no allocation, so it can be captured in a hipGraph (torch.cuda.graph).  status (i32[B]) stays on the device."""

    def __init__(self, B, cap, max_frame_points, input_pt_num=20480, node_num=128, voxel=0.3, device=None, normals=True):
        """normals=False (the Oxford / nuScenes records have none): no normal buffers, run() takes normals=None and returns sn = None"""
        dev = device or _dev()
        self.B, self.cap, self.max_src, self.n, self.node_num, self.voxel = B, int(cap), int(max_frame_points), int(input_pt_num), int(node_num), voxel
        self.ws = workspace(B, self.cap, dev)
        c = max(self.cap, 1)
        self.v_off = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
        self.v_pts = torch.empty((c, 3), dtype=torch.float32, device=dev)
        self.v_int = torch.empty((c,), dtype=torch.float32, device=dev)
        self.v_nrm = torch.empty((c, 3), dtype=torch.float32, device=dev) if normals else None
        self.status = torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)
        self.idx = torch.empty((B, self.n), dtype=torch.int32, device=dev)
        self.choice_ws = torch.empty((_lib.load().di2p_random_choice_ragged_workspace_bytes(B, max(1, self.max_src)),), dtype=torch.uint8, device=dev)
        self.pc = torch.empty((B, 3, self.n), dtype=torch.float32, device=dev)
        self.intensity = torch.empty((B, 1, self.n), dtype=torch.float32, device=dev)
        self.sn = torch.empty((B, 3, self.n), dtype=torch.float32, device=dev) if normals else None
        self.m = min(self.n, self.node_num * 8)
        self.cand_ws = torch.empty((_lib.load().di2p_random_choice_workspace_bytes(B, self.n),), dtype=torch.uint8, device=dev)
        self.cand_idx = [torch.empty((B, self.m), dtype=torch.int32, device=dev) for _ in range(2)]
        self.cand = [torch.empty((B, 3, self.m), dtype=torch.float32, device=dev) for _ in range(2)]
        self.fps_idx = [torch.empty((B, self.node_num), dtype=torch.int32, device=dev) for _ in range(2)]
        self.nodes = [torch.empty((B, 3, self.node_num), dtype=torch.float32, device=dev) for _ in range(2)]

    def run(self, points, normals, offsets, seed, P=None, seed_dev=None, jitter=None, jitter_intensity=False):
        """points f32[>=total,4] (x, y, z, intensity), normals f32[>=total,3], offsets i32[B+1] (device; total <= cap, every frame
        <= max_frame_points), P f64[B,4,4] or None -> (pc, intensity, sn, node_a, node_b), views of the plan's buffers.
        seed_dev (i64[1] device, sample_prep.SamplePlan): every draw reads its seed from there when it runs, `seed` is ignored -- the same
        draws as seed = seed_dev's value.  jitter (sigma, clip): Gaussian noise on points and normals before P (di2p_gather_ragged_aug);
        jitter_intensity (a plan without normals only): the noise on the intensity too (di2p_gather_ragged_aug_intensity)."""
        require_cuda(points, normals, offsets, P, seed_dev)
        if (normals is None) != (self.v_nrm is None):
            raise ValueError("scan_prep: normals must be given to a plan with normals and be None for a plan without (BatchPlan(normals=...))")
        if jitter_intensity and (jitter is None or normals is not None):
            raise ValueError("scan_prep: jitter_intensity needs jitter and a plan without normals")
        B, s = self.B, stream()
        call("di2p_voxel_down_sample", ptr(points), ptr(offsets), B, self.cap, self.max_src, float(self.voxel), MAX_EXTENT, 2 * self.n, ptr(normals),
             ptr(self.v_off), ptr(self.v_pts), ptr(self.v_int), ptr(self.v_nrm), None, ptr(self.status), ptr(self.ws), s)
        if seed_dev is None:
            call("di2p_random_choice_ragged", int(seed), 0, B, ptr(self.v_off), self.max_src, self.n, ptr(self.idx), ptr(self.choice_ws), s)
        else:
            call("di2p_random_choice_ragged_dseed", ptr(seed_dev), 0, B, ptr(self.v_off), self.max_src, self.n, ptr(self.idx), ptr(self.choice_ws), s)
        if jitter_intensity:
            call("di2p_gather_ragged_aug_intensity", ptr(self.v_pts), ptr(self.v_int), ptr(self.v_off), ptr(self.idx), ptr(P), B, self.n,
                 0 if seed_dev is not None else int(seed), ptr(seed_dev), 0, float(jitter[0]), float(jitter[1]), ptr(self.pc), ptr(self.intensity), s)
        elif jitter is None:
            call("di2p_gather_ragged", ptr(self.v_pts), ptr(self.v_int), ptr(self.v_nrm), ptr(self.v_off), ptr(self.idx), ptr(P), B, self.n,
                 ptr(self.pc), ptr(self.intensity), ptr(self.sn), s)
        else:
            call("di2p_gather_ragged_aug", ptr(self.v_pts), ptr(self.v_int), ptr(self.v_nrm), ptr(self.v_off), ptr(self.idx), ptr(P), B, self.n,
                 0 if seed_dev is not None else int(seed), ptr(seed_dev), 0, float(jitter[0]), float(jitter[1]), ptr(self.pc), ptr(self.intensity),
                 ptr(self.sn), s)
        for k in range(2):          # node_a (stream 1), node_b (stream 2): prep.sample_nodes_device with preallocated buffers
            if seed_dev is None:
                call("di2p_random_choice", int(seed), k + 1, B, self.n, self.m, ptr(self.cand_idx[k]), ptr(self.cand_ws), s)
            else:
                call("di2p_random_choice_dseed", ptr(seed_dev), k + 1, B, self.n, self.m, ptr(self.cand_idx[k]), ptr(self.cand_ws), s)
            call("di2p_gather_points", ptr(self.pc), ptr(self.cand_idx[k]), ptr(self.cand[k]), B, 3, self.n, self.m, s)
            call("di2p_farthest_point_sampling", ptr(self.cand[k]), None, ptr(self.fps_idx[k]), ptr(self.nodes[k]), B, self.m, self.node_num, s)
        return self.pc, self.intensity, self.sn, self.nodes[0], self.nodes[1]


def prepare_batch_into(plan, points, normals, offsets, seed, P=None):
    """Graph-safe prepare_batch: see BatchPlan.run."""
    return plan.run(points, normals, offsets, seed, P)


def pack_records(records, device=None):
    """list of f32[7, n] records -> (points f32[total,4], normals f32[total,3], offsets i32[B+1], host offsets)"""
    rows = [torch.as_tensor(r).to(device or _dev(), torch.float32) for r in records]
    points, offsets, host = pack([r[0:4].t() for r in rows], device)
    normals, _, _ = pack([r[4:7].t() for r in rows], device, cols=3)
    return points, normals, offsets, host


def prepare_batch(records, input_pt_num=20480, node_num=128, seed=0, P=None, raw=False, device=None):
    """The loader's per-sample path for a batch: records f32[7, n] (the offline record; raw=True: [n, 4] scans, run through
    preprocess_velodyne first) -> the loader's 0.3 m voxel pass where n > 2 * input_pt_num, the random down-sample to input_pt_num,
    the optional per-frame transform P (f64[B,4,4], numpy or device) and node sampling: (pc f32[B,3,N], intensity f32[B,1,N],
    sn f32[B,3,N], node_a f32[B,3,node_num], node_b f32[B,3,node_num]) device tensors, the shapes KeypointDetector takes.  An empty
    frame gives zeros."""
    if raw:
        records = preprocess_velodyne(records, device=device)
    points, normals, offsets, host = pack_records(records, device)
    B = len(host) - 1
    counts = np.diff(host)
    if counts.max(initial=0) > MAX_FRAME_POINTS:
        raise DeepI2PHipError("scan_prep: a frame has more than 2^20 points")
    plan = BatchPlan(B, points.shape[0], int(counts.max()), input_pt_num, node_num, device=points.device)
    if P is not None:
        P = torch.as_tensor(np.asarray(P, dtype=np.float64) if not torch.is_tensor(P) else P).to(points.device, torch.float64).reshape(B, 4, 4).contiguous()
    out = plan.run(points, normals, offsets, seed, P)
    check_status(plan.status[:B])
    return out
