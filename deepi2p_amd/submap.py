"""Oxford sub-maps from LMS push-broom profiles on the device (csrc/submap.hip, include/deepi2p_hip.h): the raw stage of the Oxford data set,
data/oxford/build_dataset.py.

  A-C  my_build_pointcloud (:79-148)   per profile the keep rule (missing file; skipped when the vehicle moved less than skip_threshold since
                                       the last KEPT profile), the ground filter x < threshold, pose . G_posesource_laser applied to (x, y, 0, 1),
                                       stacked in profile order with the reflectance                                    di2p_submap_build
  D    downsample (:151-166)           the 0.1 m voxel pass with the reflectance as a fake colour                       di2p_voxel_down_sample
  E    :310, :319-321                  G_camera_image^-1 . G_camera_posesource on the voxel means, the float32 record   di2p_submap_to_camera

A batch is B sub-maps of one traversal, ragged on two levels: scan_xyr f64[P,3] (the rows of the .bin files: x, y, reflectance), scan_offsets
i32[S+1] (profile -> rows), submap_offsets i32[B+1] (sub-map -> profiles), poses f64[S,4,4] (what vo_manager.interpolate_vo_poses(timestamps,
origin_time) returns for the profiles of each sub-map), present u8[S] (0: the scan file does not exist).  Poses, G_posesource_laser and
G_cam = inv(G_camera_image) . G_camera_posesource are arguments: the SDK's interpolate_poses / build_se3_transform, timestamps, file discovery
and the velocity rule of save_pc_img_for_traversal are out of scope.  The reference's call site passes skip_threshold = voxel / 16.

The record comes out in the layout sample_prep(dataset="oxford") takes: (points f32[total,4], offsets i32[B+1]); rows of a sub-map in
ascending voxel (ix, iy, iz).  One documented fork: the cloud is rounded to float32 before the voxel pass.

status per sub-map: 0 ok, 1 more than max_frame_points surviving rows (or more than the capacity), 2 (voxel pass) bounding box above its limit,
3 bad offsets, 4 no profile or no surviving row (the reference raises ValueError / IOError there).  A sub-map with a status has no rows.
"""
import numpy as np
import torch

from . import _lib, _ragged, sample_prep, scan_prep
from ._lib import DeepI2PHipError, call, ptr, require_cuda, stream
from ._ragged import _dev

MAX_FRAME_POINTS = scan_prep.MAX_FRAME_POINTS
VOXEL = 0.1          # voxel_grid_downsample_size of build_dataset.py
_STATUS = dict(scan_prep._STATUS)
_STATUS.update({1: "more than max_frame_points surviving rows", 4: "no profile or no surviving row"})


def check_status(status):
    """Raise DeepI2PHipError for a rejected sub-map (synchronises)."""
    _ragged.check_status("submap", "sub-map", _STATUS, status)


def _threshold(value, name):
    if value is None:
        return None
    v = float(value)
    if v != v:
        raise ValueError("submap: %s must be a number or None" % name)
    return v


def _skip_arg(skip_threshold):
    v = _threshold(skip_threshold, "skip_threshold")
    if v is not None and v < 0:
        raise ValueError("submap: skip_threshold must be >= 0 or None (no skip rule)")
    return -1.0 if v is None else v


def _ground_args(ground_threshold):
    """the reference removes ground only when the threshold is not None and > -1"""
    v = _threshold(ground_threshold, "ground_threshold")
    return (0.0, 0) if v is None or not v > -1 else (v, 1)


def _check_batch(scan_xyr, poses, present, B, S_cap=None, P_cap=None):
    """shapes and dtypes of the device tensors of a batch; -> (S_cap, P_cap)"""
    if not torch.is_tensor(scan_xyr) or scan_xyr.dtype != torch.float64 or scan_xyr.dim() != 2 or scan_xyr.shape[1] != 3 or not scan_xyr.is_contiguous():
        raise ValueError("submap: scan_xyr must be a contiguous float64 tensor [P, 3] (x, y, reflectance)")
    if not torch.is_tensor(poses) or poses.dtype != torch.float64 or poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or not poses.is_contiguous():
        raise ValueError("submap: poses must be a contiguous float64 tensor [S, 4, 4]")
    S, P = int(poses.shape[0]), int(scan_xyr.shape[0])
    if S_cap is not None and (S != S_cap or P != P_cap):
        raise ValueError("submap: the plan takes poses [%d, 4, 4] and scan_xyr [%d, 3] (fixed capacities; unused tail entries are never read)" % (S_cap, P_cap))
    if present is not None and (not torch.is_tensor(present) or present.dtype != torch.uint8 or tuple(present.shape) != (S,) or not present.is_contiguous()):
        raise ValueError("submap: present must be a contiguous uint8 tensor [%d] or None" % S)
    if B < 0:
        raise ValueError("submap: submap_offsets must have at least one entry")
    return S, P


def _g44(G, name, dev, batch=None):
    shape = (4, 4) if batch is None else (batch, 4, 4)
    if torch.is_tensor(G) and G.is_cuda:
        if G.dtype != torch.float64 or tuple(G.shape) != shape or not G.is_contiguous():
            raise ValueError("submap: %s must be a contiguous float64 tensor %s" % (name, list(shape)))
        return G
    a = np.asarray(G.numpy() if torch.is_tensor(G) else G, dtype=np.float64)
    if batch is not None and a.shape == (4, 4):
        a = np.tile(a, (batch, 1, 1))
    if a.shape != shape:
        raise ValueError("submap: %s must be %s" % (name, list(shape)))
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def pack_scans(submaps, device=None):
    """submaps: list of (scans, poses) per sub-map -- scans a list of [n, 3] float64 arrays (x, y, reflectance; None: the file is missing),
    poses [S_b, 4, 4] -> (scan_xyr f64[P,3], scan_offsets i32[S+1], submap_offsets i32[B+1], poses f64[S,4,4], present u8[S]) on the device."""
    rows, counts, present, pose_parts, sub = [], [], [], [], [0]
    for b, (scans, poses) in enumerate(submaps):
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        if len(scans) != poses.shape[0]:
            raise ValueError("submap: sub-map %d has %d scans and %d poses" % (b, len(scans), poses.shape[0]))
        for s in scans:
            if s is None:
                present.append(0)
                counts.append(0)
                continue
            a = np.asarray(s)
            if a.dtype != np.float64 or a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("submap: a scan must be a float64 array [n, 3] (x, y, reflectance) or None")
            present.append(1)
            counts.append(a.shape[0])
            rows.append(a)
        pose_parts.append(poses)
        sub.append(sub[-1] + len(scans))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if off[-1] >= 2 ** 31:
        raise ValueError("submap: more than 2^31 - 1 rows in a batch")
    dev = device or _dev()
    S = sub[-1]
    xyr = np.concatenate(rows) if rows else np.zeros((0, 3))
    if xyr.shape[0] == 0:
        xyr = np.zeros((1, 3))
    P = np.concatenate(pose_parts) if S else np.zeros((1, 4, 4))
    pres = np.asarray(present, dtype=np.uint8) if S else np.zeros((1,), np.uint8)
    soff = off.astype(np.int32) if S else np.zeros((2,), np.int32)
    t = torch.as_tensor
    return (t(np.ascontiguousarray(xyr)).to(dev), t(soff).to(dev), t(np.asarray(sub, dtype=np.int32)).to(dev), t(np.ascontiguousarray(P)).to(dev),
            t(pres).to(dev))


def workspace(B, S_cap, device=None):
    return _ragged.workspace("di2p_submap_workspace_bytes", B, S_cap, device)


def voxel_centroids(state):
    """f64[cap,3]: the fp64 means scan_prep.voxel_down_sample left in its workspace, in output point order (a view; valid until the workspace's
    next use)"""
    return _centroids(state.ws, state.B, state.cap)


def _centroids(ws, B, cap):
    off = int(_lib.load().di2p_scan_prep_centroids_offset(B, cap))
    return ws[off:off + 24 * cap].view(torch.float64).view(-1, 3)


def _launch_build(xyr, scan_off, sub_off, poses, present, G, B, S_cap, P_cap, cap, mfp, skip, ground, kept, skip_count, out_off, out_pts, status, ws):
    call("di2p_submap_build", ptr(xyr), ptr(scan_off), ptr(sub_off), ptr(poses), ptr(present), ptr(G), B, S_cap, P_cap, cap, mfp, skip, ground[0],
         ground[1], ptr(kept), ptr(skip_count), ptr(out_off), ptr(out_pts), ptr(status), ptr(ws), stream())


def build_raw(scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, skip_threshold=None, ground_threshold=None,
              max_frame_points=MAX_FRAME_POINTS, cap=None):
    """Stages A-C, eager: -> (points f32[cap,4] rows (x, y, z, reflectance) in the frame of each sub-map's origin, offsets i32[B+1],
    kept i32[S] (1 kept, 0 skipped, -1 missing), skip_count i32[B], status i32[B]).  Offsets may be host arrays (checked here) or device
    tensors (checked on the device: status 3).  No synchronisation."""
    mfp = _ragged._check_max_frame_points("submap", max_frame_points)
    skip, ground = _skip_arg(skip_threshold), _ground_args(ground_threshold)
    B = len(submap_offsets) - 1
    S, P = _check_batch(scan_xyr, poses, present, B)
    dev = scan_xyr.device
    sub_off = _ragged._offsets("submap", submap_offsets, "submap_offsets", B + 1, dev)
    scan_off = _ragged._offsets("submap", scan_offsets, "scan_offsets", S + 1, dev)
    G = _g44(G_posesource_laser, "G_posesource_laser", dev)
    require_cuda(scan_xyr, scan_off, sub_off, poses, present, G)
    cap = P if cap is None else int(cap)
    b = max(B, 1)
    kept = torch.empty((S,), dtype=torch.int32, device=dev)
    skip_count = torch.zeros((b,), dtype=torch.int32, device=dev)
    out_off = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
    out_pts = torch.zeros((max(cap, 1), 4), dtype=torch.float32, device=dev)
    status = torch.zeros((b,), dtype=torch.int32, device=dev)
    _launch_build(scan_xyr, scan_off, sub_off, poses, present, G, B, S, P, cap, mfp, skip, ground, kept, skip_count, out_off, out_pts, status,
                  workspace(B, S, dev))
    return out_pts, out_off, kept, skip_count[:B], status[:B]


def to_camera(state, G_cam, out=None):
    """Stage E on a scan_prep.VoxelState: -> f32[cap,4] rows (G_cam[b] . mean in fp64, intensity); G_cam f64[B,4,4] (device)."""
    out = torch.zeros((max(state.cap, 1), 4), dtype=torch.float32, device=state.points.device) if out is None else out
    call("di2p_submap_to_camera", ptr(voxel_centroids(state)), ptr(state.intensity), ptr(state.offsets), ptr(G_cam), state.B, state.cap, ptr(out),
         stream())
    return out


def build_submaps(scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, skip_threshold=None, ground_threshold=None,
                  max_frame_points=MAX_FRAME_POINTS, cap=None, voxel=VOXEL, G_cam=None):
    """Stages A-E, eager: -> (record f32[cap,4] rows (x, y, z, intensity) in the camera frame, offsets i32[B+1], status i32[B]).
    G_cam: [4,4] or [B,4,4], inv(G_camera_image) . G_camera_posesource."""
    if G_cam is None:
        raise ValueError("submap: G_cam is None (inv(G_camera_image) . G_camera_posesource)")
    if not 0.0 < float(voxel) < 1e30:
        raise ValueError("submap: voxel must be positive and finite")
    B = len(submap_offsets) - 1
    _check_batch(scan_xyr, poses, present, B)
    Gc = _g44(G_cam, "G_cam", scan_xyr.device, batch=max(B, 1))
    pts, off, _, _, status = build_raw(scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, skip_threshold, ground_threshold,
                                       max_frame_points, cap)
    st = scan_prep.voxel_down_sample(pts, off, float(voxel), cap=pts.shape[0] if cap is None else int(cap), max_frame_points=int(max_frame_points))
    return to_camera(st, Gc), st.offsets, torch.maximum(status, st.status[:B])


class SubmapPlan:
    """Fixed-capacity, preallocated form of build_submaps: run() launches stages A-E on the current stream with no allocation and no host
    synchronisation, so it can be captured in a hipGraph (the style of scan_prep.BatchPlan).  S_cap / P_cap: profiles / rows of the input
    buffers; cap_raw: surviving rows of the whole batch; max_frame_points: of one sub-map (a longer one: status 1, no rows, the others
    unaffected).  ws: a scan_prep workspace of (B, cap_raw) to share."""

    def __init__(self, B, S_cap, P_cap, cap_raw, max_frame_points, voxel=VOXEL, skip_threshold=None, ground_threshold=None, device=None, ws=None):
        self.max_src = _ragged._check_max_frame_points("submap", max_frame_points)
        self.skip, self.ground = _skip_arg(skip_threshold), _ground_args(ground_threshold)
        if not 0.0 < float(voxel) < 1e30:
            raise ValueError("submap: voxel must be positive and finite")
        if min(int(B), int(S_cap), int(P_cap), int(cap_raw)) < 0:
            raise ValueError("submap: B, S_cap, P_cap and cap_raw must be >= 0")
        dev = device or _dev()
        self.B, self.S_cap, self.P_cap, self.cap, self.voxel = int(B), int(S_cap), int(P_cap), int(cap_raw), float(voxel)
        b, c = max(self.B, 1), max(self.cap, 1)
        self.sub_ws = workspace(self.B, self.S_cap, dev)
        self.ws = scan_prep.workspace(self.B, self.cap, dev) if ws is None else ws
        self.cen = _centroids(self.ws, self.B, self.cap)          # the fp64 means of the voxel pass, inside its workspace
        self.kept = torch.zeros((max(self.S_cap, 1),), dtype=torch.int32, device=dev)
        self.skip_count = torch.zeros((b,), dtype=torch.int32, device=dev)
        self.raw_off = torch.zeros((self.B + 1,), dtype=torch.int32, device=dev)
        self.raw_pts = torch.zeros((c, 4), dtype=torch.float32, device=dev)
        self.raw_status = torch.zeros((b,), dtype=torch.int32, device=dev)
        self.v_off = torch.zeros((self.B + 1,), dtype=torch.int32, device=dev)
        self.v_pts = torch.empty((c, 3), dtype=torch.float32, device=dev)
        self.v_int = torch.empty((c,), dtype=torch.float32, device=dev)
        self.v_status = torch.zeros((b,), dtype=torch.int32, device=dev)
        self.record = torch.zeros((c, 4), dtype=torch.float32, device=dev)
        self.status = torch.zeros((b,), dtype=torch.int32, device=dev)

    def run(self, scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, G_cam):
        """scan_xyr f64[P_cap,3], scan_offsets i32[S_cap+1], submap_offsets i32[B+1], poses f64[S_cap,4,4], present u8[S_cap] | None,
        G_posesource_laser f64[4,4], G_cam f64[B,4,4] (all device) -> (record f32[cap_raw,4], offsets i32[B+1], status i32[B]), views of the
        plan's buffers."""
        B = self.B
        _check_batch(scan_xyr, poses, present, B, self.S_cap, self.P_cap)
        for t, name, dtype, shape in ((scan_offsets, "scan_offsets", torch.int32, (self.S_cap + 1,)), (submap_offsets, "submap_offsets", torch.int32, (B + 1,)),
                                      (G_posesource_laser, "G_posesource_laser", torch.float64, (4, 4)), (G_cam, "G_cam", torch.float64, (max(B, 1), 4, 4))):
            _ragged._check_tensor("submap", t, name, dtype, shape)
        require_cuda(scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, G_cam)
        s = stream()
        _launch_build(scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, B, self.S_cap, self.P_cap, self.cap, self.max_src,
                      self.skip, self.ground, self.kept, self.skip_count, self.raw_off, self.raw_pts, self.raw_status, self.sub_ws)
        call("di2p_voxel_down_sample", ptr(self.raw_pts), ptr(self.raw_off), B, self.cap, self.max_src, self.voxel, scan_prep.MAX_EXTENT, 0, None,
             ptr(self.v_off), ptr(self.v_pts), ptr(self.v_int), None, None, ptr(self.v_status), ptr(self.ws), s)
        call("di2p_submap_to_camera", ptr(self.cen), ptr(self.v_int), ptr(self.v_off), ptr(G_cam), B, self.cap, ptr(self.record), s)
        torch.maximum(self.raw_status, self.v_status, out=self.status)
        return self.record, self.v_off, self.status[:B]


class OxfordRawPlan:
    """SubmapPlan + sample_prep.SamplePlan(dataset="oxford"): LMS profiles and camera frames to the Oxford loader's sample in one graph-safe
    call.  The two voxel stages share one workspace (same B and capacity; the 0.1 m stage's means are last read by the camera transform, before
    the loader's filter starts).  The result equals build_submaps followed by sample_prep.prepare_samples(dataset="oxford") bit for bit."""

    def __init__(self, opt, B, S_cap, P_cap, cap_raw, max_frame_points, raw_hw=None, mode="val", voxel=VOXEL, skip_threshold=None,
                 ground_threshold=None, device=None, jitter=sample_prep.JITTER, color=None):
        _ragged._check_max_frame_points("submap", max_frame_points)
        _skip_arg(skip_threshold)
        sample_prep.option_block(opt, sample_prep.RAW_HW["oxford"] if raw_hw is None else raw_hw, mode, dataset="oxford")          # argument errors first
        dev = device or _dev()
        # a voxel has at least one raw row: the record needs no more rows, and no sub-map more points, than the raw batch
        self.sample = sample_prep.SamplePlan(opt, B, int(cap_raw), int(max_frame_points), raw_hw, mode, dev, jitter=jitter, color=color, dataset="oxford")
        self.submap = SubmapPlan(B, S_cap, P_cap, cap_raw, max_frame_points, voxel, skip_threshold, ground_threshold, dev, ws=self.sample.points.ws)
        self.B = int(B)
        self.status = torch.zeros((max(self.B, 1),), dtype=torch.int32, device=dev)
        self._T_scan = torch.zeros((max(self.B, 1), 4, 4), dtype=torch.float64, device=dev)

    @property
    def seed(self):
        """i64[1] device: the seed slot of the draws (sample_prep.SamplePlan.seed)"""
        return self.sample.seed

    @property
    def T_scan(self):
        """f64[B,4,4] device: Pr . G_cam of the last run(with_T_scan=True) -- from the sub-map's origin vehicle frame (what build_raw writes)
        onto the prepared points.  The record is already in the camera's frame, so the draw's Pr alone maps the RECORD onto them."""
        return self._T_scan[:self.B]

    def run(self, scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, G_cam, images_u8, K_raw, P_cam_pc, seed=None,
            with_T_scan=False):
        """the batch (SubmapPlan.run), images u8[B,H0,W0,3], K_raw f64[B,3,3], P_cam_pc f64[B,4,4] (all device) -> SamplePlan.run's nine
        tensors + status i32[B], views of the plans' buffers.  seed=None leaves the seed slot as it is (graph replays).
        with_T_scan=True: one launch more (di2p_compose_poses) and T_scan as an eleventh entry: sample_prep.PREPARED."""
        sample_prep._check_images(images_u8, self.B, self.sample.image.raw_hw)
        record, offsets, _ = self.submap.run(scan_xyr, scan_offsets, submap_offsets, poses, present, G_posesource_laser, G_cam)
        out = self.sample.run(record, None, offsets, images_u8, K_raw, P_cam_pc, seed=seed)
        torch.maximum(self.submap.status, self.sample.status, out=self.status)
        if not with_T_scan:
            return tuple(out) + (self.status[:self.B],)
        call("di2p_compose_poses", ptr(self.sample.table.Pr), ptr(G_cam), self.B, ptr(self._T_scan), stream())
        return tuple(out) + (self.status[:self.B], self.T_scan)


def prepare_oxford_raw(submaps, G_posesource_laser, G_cam, images, K_raw, P_cam_pc, opt, mode="val", seed=0, skip_threshold=None,
                       ground_threshold=None, voxel=VOXEL, device=None):
    """Convenience: packs the sub-maps (pack_scans' host form), builds a plan, runs it and checks the status (synchronises).
    images u8[B,H0,W0,3]; K_raw [B,3,3]; P_cam_pc [B,4,4] -> OxfordRawPlan.run's tuple."""
    images, raw_hw = sample_prep._host_images(images, len(submaps), "submap", "sub-map")
    sample_prep.option_block(opt, raw_hw, mode, dataset="oxford")          # argument errors before anything touches the device
    _skip_arg(skip_threshold)
    _ground_args(ground_threshold)
    B = len(submaps)
    for name, G, shape in (("G_posesource_laser", G_posesource_laser, [(4, 4)]), ("G_cam", G_cam, [(4, 4), (B, 4, 4)])):
        if G is None or tuple(np.shape(G)) not in shape:
            raise ValueError("submap: %s must be %s" % (name, " or ".join(str(list(s)) for s in shape)))
    rows = [sum(0 if s is None else len(s) for s in scans) for scans, _ in submaps]
    if max(rows, default=0) > MAX_FRAME_POINTS:
        raise DeepI2PHipError("submap: a sub-map has more than 2^20 rows")
    dev = device or _dev()
    xyr, scan_off, sub_off, poses, present = pack_scans(submaps, dev)
    plan = OxfordRawPlan(opt, B, poses.shape[0], xyr.shape[0], xyr.shape[0], max(max(rows, default=1), 1), raw_hw, mode, voxel, skip_threshold,
                         ground_threshold, dev)
    f64 = sample_prep._f64
    out = plan.run(xyr, scan_off, sub_off, poses, present, _g44(G_posesource_laser, "G_posesource_laser", dev), _g44(G_cam, "G_cam", dev, batch=max(B, 1)),
                   images.to(dev).contiguous(), f64(K_raw, (B, 3, 3), dev), f64(P_cam_pc, (B, 4, 4), dev), seed=seed)
    check_status(plan.status[:B])
    return out
