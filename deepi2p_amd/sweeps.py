"""nuScenes sweep accumulation on the device (csrc/sweeps.hip, include/deepi2p_hip.h): the raw stage of nuScenesLoader.__getitem__,
data/nuscenes_pc_img_pose_loader.py.

  poses        get_sample_data_ego_pose_P / get_calibration_P (:58-78)   (quaternion wxyz, translation) -> 4x4 of float32 values   di2p_pose_matrices
  transforms   lidar_frame_accumulation (:227-229, :249-252)             T_j = inv(P_vehicle_lidar) . (inv(P_oi) . P_oj) . P_vehicle_lidar
               __getitem__ (:292-293, :324-325, :351-354)                P_cam_pc = inv(cam_calib) . (inv(cam_pose) . (lidar_pose . lidar_calib))
                                                                                                                                  di2p_sweep_transforms
  accumulate   get_lidar_pc_intensity_by_token (:194-210)                the ego-box filter of every sweep (float32 compares)
               accumulate_lidar_points (:242-267)                        key sweep | next picks | prev picks, each moved by its T_j     di2p_sweep_accumulate

A batch is B frames, ragged on two levels: rows f32[P,cols] (cols 4: x, y, z, intensity; cols 5: the .pcd.bin rows as they are, the ring is
not read), sweep_offsets i32[S+1] (sweep -> rows), frame_offsets i32[B+1] (frame -> sweeps, the key sweep first).  Records are f64[.,7] rows
(w, x, y, z, tx, ty, tz): `ego` one per sweep (the ego pose of its sample_data), `lidar_calib`, `cam_pose`, `cam_calib` one per frame (the
LiDAR's calibrated_sensor, the camera frame's ego pose and calibrated_sensor).  Token look-ups, the choice of the camera and file reading
stay with the caller; sweep_picks says which neighbours the reference's walk takes.

The cloud comes out as sample_prep(dataset="nuscenes") takes it: (points f32[total,4], offsets i32[B+1]).  One documented fork:
the cloud is rounded to float32 when it is written; the reference keeps float64 coordinates when its voxel pass is not taken.

status per frame: 0 ok, 1 more than max_frame_points surviving rows (or more than the capacity), 2 (voxel pass of the sample stage) bounding
box above its limit, 3 bad offsets, 4 no sweep or no surviving row.  A frame with a status has no rows.
"""
import numpy as np
import torch

from . import _lib, _ragged, sample_prep, scan_prep
from ._lib import DeepI2PHipError, call, ptr, require_cuda, stream
from ._ragged import _dev

MAX_FRAME_POINTS = scan_prep.MAX_FRAME_POINTS
BOX = (0.8, 2.7)          # half-extents (x, y) of the ego car's box, get_lidar_pc_intensity_by_token
_STATUS = dict(scan_prep._STATUS)
_STATUS.update({1: "more than max_frame_points surviving rows", 4: "no sweep or no surviving row"})


def check_status(status):
    """Raise DeepI2PHipError for a rejected frame (synchronises)."""
    _ragged.check_status("sweeps", "frame", _STATUS, status)


def sweep_picks(available_next, available_prev, frame_num=3, frame_skip=4):
    """lidar_frame_accumulation's walk as index arithmetic: with available_next / available_prev sweeps after / before the key sweep in its
    linked list -> (next, prev), the distances from the key sweep (1 = its direct neighbour) of the sweeps the reference accumulates, in the
    order it appends them: every frame_skip-th one, at most frame_num per side, until the list ends."""
    frame_num, frame_skip = int(frame_num), int(frame_skip)
    if frame_num < 0 or frame_skip < 1:
        raise ValueError("sweeps: accumulation_frame_num must be >= 0 and accumulation_frame_skip >= 1")
    if int(available_next) < 0 or int(available_prev) < 0:
        raise ValueError("sweeps: available_next and available_prev must be >= 0")
    walk = lambda n: [k * frame_skip for k in range(1, frame_num + 1) if k * frame_skip <= int(n)]
    return walk(available_next), walk(available_prev)


def _check_cols(cols):
    if cols not in (4, 5):
        raise ValueError("sweeps: cols must be 4 (x, y, z, intensity) or 5 (the .pcd.bin rows)")
    return int(cols)


def _box(box):
    try:
        bx, by = (float(v) for v in box)
    except (TypeError, ValueError):
        raise ValueError("sweeps: box must be the two half-extents (x, y) of the ego box") from None
    if not (bx >= 0.0 and by >= 0.0):
        raise ValueError("sweeps: box must be the two half-extents (x, y) of the ego box, numbers >= 0")
    return bx, by


def _records(x, n, name, dev):
    """f64[n,7] on the device; n=None: any number of rows"""
    if torch.is_tensor(x) and x.is_cuda:
        if x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != 7 or (n is not None and x.shape[0] != n) or not x.is_contiguous():
            raise ValueError("sweeps: %s must be a contiguous float64 tensor [%s, 7] (w, x, y, z, tx, ty, tz)" % (name, "n" if n is None else n))
        return x
    if x is None:
        raise ValueError("sweeps: %s is None ([n, 7] records: w, x, y, z, tx, ty, tz)" % name)
    a = np.asarray(x.numpy() if torch.is_tensor(x) else x, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 7 or (n is not None and a.shape[0] != n):
        raise ValueError("sweeps: %s must be [%s, 7] (w, x, y, z, tx, ty, tz), got %s" % (name, "n" if n is None else n, list(a.shape)))
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev or _dev())


def _m44(x, n, name):
    """contiguous f64 [n,4,4]; n a string: any number of matrices"""
    return _ragged._check_tensor("sweeps", x, name, torch.float64, (n, 4, 4), "tensor")


def _check_rows(rows, cols=None, P_cap=None):
    if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] not in (4, 5) or not rows.is_contiguous():
        raise ValueError("sweeps: rows must be a contiguous float32 tensor [P, 4] (x, y, z, intensity) or [P, 5] (the .pcd.bin rows)")
    if cols is not None and (rows.shape[1] != cols or rows.shape[0] != P_cap):
        raise ValueError("sweeps: the plan takes rows [%d, %d] (fixed capacity; unused tail rows are never read)" % (P_cap, cols))
    return int(rows.shape[0]), int(rows.shape[1])


def pose_matrices(records, out=None):
    """records [n,7] (w, x, y, z, tx, ty, tz; host array or device tensor) -> f64[n,4,4] on the device: the reference's pose / calibration
    matrix, whose rotation and translation entries are float32 values.  No synchronisation."""
    if out is not None and not torch.is_tensor(out):
        raise ValueError("sweeps: out must be a contiguous float64 tensor [n, 4, 4]")
    rec = _records(records, None, "records", out.device if out is not None else None)
    n = int(rec.shape[0])
    out = torch.empty((n, 4, 4), dtype=torch.float64, device=rec.device) if out is None else _m44(out, n, "out")
    require_cuda(rec, out)
    call("di2p_pose_matrices", ptr(rec), n, ptr(out), stream())
    return out


def sweep_transforms(P_ego, frame_offsets, P_vehicle_lidar, P_ego_cam, P_vehicle_cam):
    """P_ego f64[S,4,4] (per sweep), frame_offsets [B+1], P_vehicle_lidar / P_ego_cam / P_vehicle_cam f64[B,4,4] (device) ->
    (T f64[S,4,4]: identity for each frame's first sweep, P_cam_pc f64[B,4,4]).  No synchronisation."""
    B = len(frame_offsets) - 1
    if B < 0:
        raise ValueError("sweeps: frame_offsets must have at least one entry")
    _m44(P_ego, "S", "P_ego")
    for t, name in ((P_vehicle_lidar, "P_vehicle_lidar"), (P_ego_cam, "P_ego_cam"), (P_vehicle_cam, "P_vehicle_cam")):
        _m44(t, B, name)
    S, dev = int(P_ego.shape[0]), P_ego.device
    off = _ragged._offsets("sweeps", frame_offsets, "frame_offsets", B + 1, dev)
    require_cuda(P_ego, off, P_vehicle_lidar, P_ego_cam, P_vehicle_cam)
    T = torch.zeros((max(S, 1), 4, 4), dtype=torch.float64, device=dev)
    P_cam_pc = torch.zeros((max(B, 1), 4, 4), dtype=torch.float64, device=dev)
    call("di2p_sweep_transforms", ptr(P_ego), ptr(off), ptr(P_vehicle_lidar), ptr(P_ego_cam), ptr(P_vehicle_cam), B, S, ptr(T), ptr(P_cam_pc), stream())
    return T[:S], P_cam_pc[:B]


def host_sweeps(frames, cols=None):
    """frames: per frame a list of float32 arrays [n, 4] or [n, 5], the key sweep first -> (parts: the arrays to lay end to end,
    sweep_offsets i64[S+1], frame_offsets i64[B+1], cols); host only, nothing is cast silently."""
    parts, counts, fo = [], [], [0]
    for b, sweeps in enumerate(frames):
        if not isinstance(sweeps, (list, tuple)):
            raise ValueError("sweeps: frame %d must be a list of sweeps (the key sweep first)" % b)
        for s in sweeps:
            a = s if torch.is_tensor(s) else np.asarray(s)
            if len(a.shape) != 2 or a.shape[1] not in (4, 5) or a.dtype != (torch.float32 if torch.is_tensor(a) else np.float32):
                raise ValueError("sweeps: a sweep must be a float32 array [n, 4] (x, y, z, intensity) or [n, 5] (the .pcd.bin rows)")
            if cols is None:
                cols = int(a.shape[1])
            if a.shape[1] != cols:
                raise ValueError("sweeps: every sweep of a batch must have the same number of columns (%d)" % cols)
            parts.append(a)
            counts.append(int(a.shape[0]))
        fo.append(fo[-1] + len(sweeps))
    so = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    if so[-1] >= 2 ** 31:
        raise ValueError("sweeps: more than 2^31 - 1 rows in a batch")
    return parts, so, np.asarray(fo, dtype=np.int64), 4 if cols is None else cols


def host_ego(ego, S):
    """ego records of a batch, all of them [S, 7] or per frame an [S_b, 7] array -> f64[S,7] (host)"""
    if isinstance(ego, (list, tuple)):
        ego = np.concatenate([np.asarray(e, dtype=np.float64).reshape(-1, 7) for e in ego]) if len(ego) else np.zeros((0, 7))
    ego = np.asarray(ego, dtype=np.float64)
    if ego.shape != (S, 7):
        raise ValueError("sweeps: ego must hold one record (w, x, y, z, tx, ty, tz) per sweep: [%d, 7], got %s" % (S, list(ego.shape)))
    return ego


def pack_sweeps(frames, device=None, cols=None):
    """host_sweeps' form -> (rows f32[P,cols], sweep_offsets i32[S+1], frame_offsets i32[B+1]) on the device (P >= 1: an empty batch gets one
    unused row)."""
    parts, so, fo, cols = host_sweeps(frames, cols)
    dev = device or _dev()
    rows = np.concatenate([np.asarray(p) for p in parts]) if parts else np.zeros((0, cols), np.float32)
    if rows.shape[0] == 0:
        rows = np.zeros((1, cols), np.float32)
    t = torch.as_tensor
    return t(np.ascontiguousarray(rows)).to(dev), t(so.astype(np.int32)).to(dev), t(fo.astype(np.int32)).to(dev)


def workspace(B, S_cap, device=None):
    return _ragged.workspace("di2p_sweep_workspace_bytes", B, S_cap, device)


def _launch(rows, sweep_off, frame_off, T, B, S_cap, P_cap, cols, cap, mfp, box, kept, out_off, out_pts, status, ws):
    call("di2p_sweep_accumulate", ptr(rows), ptr(sweep_off), ptr(frame_off), ptr(T), B, S_cap, P_cap, cols, cap, mfp, box[0], box[1], ptr(kept),
         ptr(out_off), ptr(out_pts), ptr(status), ptr(ws), stream())


def accumulate_sweeps(rows, sweep_offsets, frame_offsets, T, box=BOX, max_frame_points=MAX_FRAME_POINTS, cap=None):
    """Eager: rows f32[P,4|5], T f64[S,4,4] (device), the offsets host arrays (checked here) or device tensors (checked on the device: status
    3) -> (points f32[cap,4] rows (x, y, z, intensity) in each frame's key-sweep LiDAR frame, offsets i32[B+1], kept i32[S] surviving rows per
    sweep, status i32[B]).  No synchronisation."""
    mfp, box = _ragged._check_max_frame_points("sweeps", max_frame_points), _box(box)
    P, cols = _check_rows(rows)
    B = len(frame_offsets) - 1
    if B < 0:
        raise ValueError("sweeps: frame_offsets must have at least one entry")
    _m44(T, "S", "T")
    S, dev = int(T.shape[0]), rows.device
    frame_off = _ragged._offsets("sweeps", frame_offsets, "frame_offsets", B + 1, dev)
    sweep_off = _ragged._offsets("sweeps", sweep_offsets, "sweep_offsets", S + 1, dev)
    cap = P if cap is None else int(cap)
    if cap < 0:
        raise ValueError("sweeps: cap must be >= 0")
    require_cuda(rows, sweep_off, frame_off, T)
    b = max(B, 1)
    kept = torch.zeros((max(S, 1),), dtype=torch.int32, device=dev)
    out_off = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
    out_pts = torch.zeros((max(cap, 1), 4), dtype=torch.float32, device=dev)
    status = torch.zeros((b,), dtype=torch.int32, device=dev)
    _launch(rows, sweep_off, frame_off, T, B, S, P, cols, cap, mfp, box, kept, out_off, out_pts, status, workspace(B, S, dev))
    return out_pts, out_off, kept[:S], status[:B]


class SweepPlan:
    """Fixed-capacity, preallocated form of pose_matrices + sweep_transforms + accumulate_sweeps: run() launches them on the current stream
    with no allocation and no host synchronisation, so it can be captured in a hipGraph (the style of submap.SubmapPlan).  S_cap / P_cap:
    sweeps / rows of the input buffers; cap_raw: surviving rows of the whole batch; max_frame_points: of one frame (a longer one: status 1, no
    rows, the others unaffected).  ws: a workspace of at least workspace(B, S_cap) bytes to use instead of an own one."""

    def __init__(self, B, S_cap, P_cap, cap_raw, max_frame_points, cols=4, box=BOX, device=None, ws=None):
        self.max_src, self.box, self.cols = _ragged._check_max_frame_points("sweeps", max_frame_points), _box(box), _check_cols(cols)
        if min(int(B), int(S_cap), int(P_cap), int(cap_raw)) < 0:
            raise ValueError("sweeps: B, S_cap, P_cap and cap_raw must be >= 0")
        dev = device or _dev()
        self.B, self.S_cap, self.P_cap, self.cap = int(B), int(S_cap), int(P_cap), int(cap_raw)
        b, s = max(self.B, 1), max(self.S_cap, 1)
        need = max(256, _lib.load().di2p_sweep_workspace_bytes(self.B, self.S_cap))
        self.ws = ws if ws is not None and ws.numel() * ws.element_size() >= need else workspace(self.B, self.S_cap, dev)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.P_ego, self.T = f64(s, 4, 4), f64(s, 4, 4)
        self.P_vehicle_lidar, self.P_ego_cam, self.P_vehicle_cam, self.P_cam_pc = f64(b, 4, 4), f64(b, 4, 4), f64(b, 4, 4), f64(b, 4, 4)
        self.kept = torch.zeros((s,), dtype=torch.int32, device=dev)
        self.offsets = torch.zeros((self.B + 1,), dtype=torch.int32, device=dev)
        self.points = torch.zeros((max(self.cap, 1), 4), dtype=torch.float32, device=dev)
        self.status = torch.zeros((b,), dtype=torch.int32, device=dev)

    def run(self, rows, sweep_offsets, frame_offsets, ego, lidar_calib, cam_pose, cam_calib):
        """rows f32[P_cap,cols], sweep_offsets i32[S_cap+1], frame_offsets i32[B+1], ego f64[S_cap,7], lidar_calib / cam_pose / cam_calib
        f64[B,7] (all device) -> (points f32[cap_raw,4], offsets i32[B+1], kept i32[S_cap], status i32[B], P_cam_pc f64[B,4,4]), views of the
        plan's buffers."""
        B, S = self.B, self.S_cap
        _check_rows(rows, self.cols, self.P_cap)
        for t, name, dtype, shape in ((sweep_offsets, "sweep_offsets", torch.int32, (S + 1,)), (frame_offsets, "frame_offsets", torch.int32, (B + 1,)),
                                      (ego, "ego", torch.float64, (S, 7)), (lidar_calib, "lidar_calib", torch.float64, (B, 7)),
                                      (cam_pose, "cam_pose", torch.float64, (B, 7)), (cam_calib, "cam_calib", torch.float64, (B, 7))):
            _ragged._check_tensor("sweeps", t, name, dtype, shape)
        require_cuda(rows, sweep_offsets, frame_offsets, ego, lidar_calib, cam_pose, cam_calib)
        s = stream()
        for rec, n, out in ((ego, S, self.P_ego), (lidar_calib, B, self.P_vehicle_lidar), (cam_pose, B, self.P_ego_cam), (cam_calib, B, self.P_vehicle_cam)):
            call("di2p_pose_matrices", ptr(rec), n, ptr(out), s)
        call("di2p_sweep_transforms", ptr(self.P_ego), ptr(frame_offsets), ptr(self.P_vehicle_lidar), ptr(self.P_ego_cam), ptr(self.P_vehicle_cam), B, S,
             ptr(self.T), ptr(self.P_cam_pc), s)
        _launch(rows, sweep_offsets, frame_offsets, self.T, B, S, self.P_cap, self.cols, self.cap, self.max_src, self.box, self.kept, self.offsets,
                self.points, self.status, self.ws)
        return self.points, self.offsets, self.kept[:S], self.status[:B], self.P_cam_pc[:B]


class NuScenesRawPlan:
    """SweepPlan + sample_prep.SamplePlan(dataset="nuscenes"): raw sweeps, the data set's records and camera frames to the nuScenes loader's
    sample in one graph-safe call.  The accumulation uses the sample stage's workspace (it is done before the 0.2 m pass starts) when that is
    large enough.  The result equals pose_matrices, sweep_transforms and accumulate_sweeps followed by
    sample_prep.prepare_samples(dataset="nuscenes", offsets=...) bit for bit."""

    def __init__(self, opt, B, S_cap, P_cap, cap_raw, max_frame_points, raw_hw=None, mode="val", cols=4, box=BOX, device=None,
                 jitter=sample_prep.JITTER, color=None):
        _ragged._check_max_frame_points("sweeps", max_frame_points)
        _check_cols(cols)
        _box(box)
        sample_prep.option_block(opt, sample_prep.RAW_HW["nuscenes"] if raw_hw is None else raw_hw, mode, dataset="nuscenes")      # argument errors first
        dev = device or _dev()
        self.sample = sample_prep.SamplePlan(opt, B, int(cap_raw), int(max_frame_points), raw_hw, mode, dev, jitter=jitter, color=color, dataset="nuscenes")
        self.sweeps = SweepPlan(B, S_cap, P_cap, cap_raw, max_frame_points, cols, box, dev, ws=self.sample.points.ws)
        self.B = int(B)
        self.status = torch.zeros((max(self.B, 1),), dtype=torch.int32, device=dev)

    @property
    def seed(self):
        """i64[1] device: the seed slot of the draws (sample_prep.SamplePlan.seed)"""
        return self.sample.seed

    @property
    def T_scan(self):
        """f64[B,4,4] device: the Pr the last run's draw applied to the accumulated cloud"""
        return self.sample.table.Pr[:self.B]

    @property
    def P_cam_pc(self):
        return self.sweeps.P_cam_pc[:self.B]

    def run(self, rows, sweep_offsets, frame_offsets, ego, lidar_calib, cam_pose, cam_calib, images_u8, K_raw, seed=None):
        """the batch and its records (SweepPlan.run), images u8[B,H0,W0,3], K_raw f64[B,3,3] (all device) -> SamplePlan.run's nine tensors +
        (status i32[B], T_scan f64[B,4,4]), views of the plans' buffers.  seed=None leaves the seed slot as it is (graph replays)."""
        sample_prep._check_images(images_u8, self.B, self.sample.image.raw_hw)
        points, offsets, _, _, P_cam_pc = self.sweeps.run(rows, sweep_offsets, frame_offsets, ego, lidar_calib, cam_pose, cam_calib)
        out = self.sample.run(points, None, offsets, images_u8, K_raw, self.sweeps.P_cam_pc, seed=seed)
        torch.maximum(self.sweeps.status, self.sample.status, out=self.status)
        return tuple(out) + (self.status[:self.B], self.T_scan)


def prepare_nuscenes_raw(frames, ego, lidar_calib, cam_pose, cam_calib, images, K_raw, opt, mode="val", seed=0, box=BOX, device=None):
    """Convenience: packs the frames (host_sweeps' form; ego: per frame an [S_b, 7] array, or all of them [S, 7]), builds a plan, runs it and
    checks the status (synchronises).  images u8[B,H0,W0,3]; K_raw [B,3,3]; lidar_calib / cam_pose / cam_calib [B,7] -> NuScenesRawPlan.run's
    tuple."""
    images, raw_hw = sample_prep._host_images(images, len(frames), "sweeps", "frame")
    sample_prep.option_block(opt, raw_hw, mode, dataset="nuscenes")          # argument errors before anything touches the device
    _box(box)
    parts, so, fo, cols = host_sweeps(frames)
    B, S = len(frames), int(fo[-1])
    ego = host_ego(ego, S)
    recs = []
    for name, r in (("lidar_calib", lidar_calib), ("cam_pose", cam_pose), ("cam_calib", cam_calib)):
        if r is None or tuple(np.shape(r)) != (B, 7):
            raise ValueError("sweeps: %s must be [%d, 7] (w, x, y, z, tx, ty, tz)" % (name, B))
        recs.append(np.asarray(r, dtype=np.float64))
    per_frame = [int(so[fo[b + 1]] - so[fo[b]]) for b in range(B)]
    if max(per_frame, default=0) > MAX_FRAME_POINTS:
        raise DeepI2PHipError("sweeps: a frame has more than 2^20 rows")
    dev = device or _dev()
    rows, sweep_off, frame_off = pack_sweeps(frames, dev, cols)
    s = max(S, 1)
    ego_d = torch.zeros((s, 7), dtype=torch.float64)
    ego_d[:S] = torch.as_tensor(ego)
    pad = lambda a: torch.as_tensor(np.ascontiguousarray(a if B else np.zeros((1, 7)))).to(dev)
    sweep_off = sweep_off if S else torch.zeros((2,), dtype=torch.int32, device=dev)
    plan = NuScenesRawPlan(opt, B, s, rows.shape[0], rows.shape[0], max(max(per_frame, default=1), 1), raw_hw, mode, cols, box, dev)
    out = plan.run(rows, sweep_off, frame_off, ego_d.to(dev), pad(recs[0]), pad(recs[1]), pad(recs[2]), images.to(dev).contiguous(),
                   sample_prep._f64(K_raw, (B, 3, 3), dev), seed=seed)
    check_status(plan.status[:B])
    return out
