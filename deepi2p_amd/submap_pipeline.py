"""Oxford raw executor: "here are a traversal's LMS push-broom profiles, their poses and a camera frame, give me the pose" on
raw_pipeline.PreparedFrameExecutor.

One STEP = H2D copy of the raw batch -> submap.OxfordRawPlan (keep rule, ground filter and transform of every profile, the 0.1 m voxel pass,
the camera-frame record, the loader's sample preparation, image path) -> classifier -> pose solve (Gauss-Newton restarts or PnP-RANSAC) ->
P_scan = P . T_scan.  The staging, the step and the evaluation mode are the base class's, shared with raw_pipeline.RawFrameExecutor and
sweep_pipeline.SweepFrameExecutor; this module has the host check of a sub-map batch (host_submap_frames) and the subclass that names the
staged inputs, the plan and P_cam_pc.  The Oxford record is in a camera frame (y down): build the pipeline with the default frame="cam".
"""
import numpy as np
import torch

from . import _ragged, sample_prep, submap
from .raw_pipeline import PreparedFrameExecutor

ROWS_LIST, ROWS_FLAT = ("submaps",), ("scan_xyr", "scan_offsets", "submap_offsets", "poses", "present")
KEYS = ("G_posesource_laser", "G_cam", "image", "K_raw", "P_cam_pc")


def _host_submaps(submaps):
    """submap.pack_scans' host form, kept on the host -> (parts: the float64 [n,3] arrays to lay end to end, scan_offsets i64[S+1],
    submap_offsets i64[B+1], poses f64[S,4,4], present u8[S]); nothing is cast silently"""
    parts, counts, present, pose_parts, sub = [], [], [], [], [0]
    for b, entry in enumerate(submaps):
        if not isinstance(entry, (list, tuple)) or len(entry) != 2:
            raise ValueError("raw sub-map batch: sub-map %d must be the pair (scans, poses)" % b)
        scans, poses = entry
        poses = np.asarray(poses, dtype=np.float64)
        if poses.ndim != 3 or poses.shape[1:] != (4, 4) or len(scans) != poses.shape[0]:
            raise ValueError("raw sub-map batch: sub-map %d has %d scans and poses %s ([S_b, 4, 4] needed)" % (b, len(scans), list(poses.shape)))
        for s in scans:
            if s is None:
                present.append(0)
                counts.append(0)
                continue
            a = s if torch.is_tensor(s) else np.asarray(s)
            if len(a.shape) != 2 or a.shape[1] != 3 or a.dtype != (torch.float64 if torch.is_tensor(a) else np.float64):
                raise ValueError("raw sub-map batch: a scan must be a float64 array [n, 3] (x, y, reflectance) or None")
            present.append(1)
            counts.append(int(a.shape[0]))
            parts.append(a)
        pose_parts.append(poses)
        sub.append(sub[-1] + len(scans))
    so = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    P = np.concatenate(pose_parts) if pose_parts else np.zeros((0, 4, 4))
    return parts, so, np.asarray(sub, dtype=np.int64), P, np.asarray(present, dtype=np.uint8)


def host_submap_frames(host_batch, B, S_cap, P_cap, raw_hw):
    """Check a raw host batch against the shapes an executor was built for and bring it to its staged form; host-only, raises ValueError
    before anything is enqueued, and modifies nothing it is given.  host_batch: dict with `submaps` (submap.pack_scans' host form: per
    sub-map (scans, poses), scans a list of float64 [n,3] arrays or None for a missing file; or the flat form: `scan_xyr` f64[P,3] plus
    `scan_offsets` [S+1], `submap_offsets` [B+1], `poses` f64[S,4,4] and `present` u8[S]), `G_posesource_laser` [4,4], `G_cam` [4,4] or
    [B,4,4], `image` u8[B,H0,W0,3], `K_raw` [B,3,3], `P_cam_pc` [B,4,4] and optionally `seed`.  Rows of another dtype than float64 raise in
    both forms: the .bin files hold doubles and di2p_submap_build takes doubles.
    -> (parts: list of f64 tensors [n,3] to lay end to end, scan_offsets i32[S+1], submap_offsets i32[B+1], poses f64[S,4,4], present u8[S],
        G_posesource_laser f64[4,4], G_cam f64[B,4,4], image, K_raw, P_cam_pc f64[B,4,4], seed int)"""
    flat = host_batch.get("submaps") is None and host_batch.get("scan_xyr") is not None
    for k in (ROWS_FLAT if flat else ROWS_LIST) + KEYS:
        if host_batch.get(k) is None:
            raise ValueError("raw sub-map batch has no %r (submaps | scan_xyr, scan_offsets, submap_offsets, poses, present; G_posesource_laser, G_cam, "
                             "image, K_raw, P_cam_pc[, seed])" % k)
    if not flat:
        parts, so, mo, poses, present = _host_submaps(host_batch["submaps"])
        parts = [torch.as_tensor(p) for p in parts]
    else:
        xyr = torch.as_tensor(host_batch["scan_xyr"])
        if xyr.dim() != 2 or xyr.shape[1] != 3:
            raise ValueError("raw sub-map batch: flat scan_xyr must be [P, 3] (x, y, reflectance), got %s" % (tuple(xyr.shape),))
        if xyr.dtype != torch.float64:
            raise ValueError("raw sub-map batch: scan_xyr must be float64")
        so = np.asarray(host_batch["scan_offsets"]).astype(np.int64).reshape(-1)
        mo = np.asarray(host_batch["submap_offsets"]).astype(np.int64).reshape(-1)
        if len(so) < 1 or so[0] != 0 or np.any(np.diff(so) < 0) or so[-1] > xyr.shape[0]:
            raise ValueError("raw sub-map batch: scan_offsets must start at 0, not decrease and end within the %d rows of scan_xyr" % xyr.shape[0])
        if len(mo) < 1 or mo[0] != 0 or np.any(np.diff(mo) < 0) or mo[-1] != len(so) - 1:
            raise ValueError("raw sub-map batch: submap_offsets must start at 0, not decrease and end at the %d profiles of scan_offsets" % (len(so) - 1))
        S = len(so) - 1
        poses = np.asarray(host_batch["poses"])
        present = np.asarray(host_batch["present"])
        if poses.dtype != np.float64 or poses.shape != (S, 4, 4):
            raise ValueError("raw sub-map batch: poses must be float64 [%d, 4, 4] (one per profile), got %s %s" % (S, poses.dtype, list(poses.shape)))
        if present.dtype != np.uint8 or present.shape != (S,):
            raise ValueError("raw sub-map batch: present must be uint8 [%d] (one per profile), got %s %s" % (S, present.dtype, list(present.shape)))
        parts = [xyr[:int(so[-1])]]
    if len(mo) != B + 1:
        raise ValueError("raw sub-map batch has %d sub-maps, this executor was built (and its graphs captured) for B = %d" % (len(mo) - 1, B))
    S, total = int(mo[-1]), int(so[-1])
    if S > S_cap:
        raise ValueError("raw sub-map batch has %d profiles in all, above the S_cap = %d this executor stages" % (S, S_cap))
    if total > P_cap:
        raise ValueError("raw sub-map batch has %d rows in all, above the P_cap = %d rows this executor stages" % (total, P_cap))
    Gl = np.asarray(host_batch["G_posesource_laser"], dtype=np.float64)
    if Gl.shape != (4, 4):
        raise ValueError("raw sub-map batch: G_posesource_laser must be [4, 4], got %s" % list(Gl.shape))
    Gc = np.asarray(host_batch["G_cam"], dtype=np.float64)
    if Gc.shape == (4, 4):
        Gc = np.tile(Gc, (B, 1, 1))
    if Gc.shape != (B, 4, 4):
        raise ValueError("raw sub-map batch: G_cam must be [4, 4] or [%d, 4, 4] (inv(G_camera_image) . G_camera_posesource), got %s" % (B, list(Gc.shape)))
    image = torch.as_tensor(host_batch["image"])
    want = (B, int(raw_hw[0]), int(raw_hw[1]), 3)
    if image.dtype != torch.uint8 or tuple(image.shape) != want:
        raise ValueError("raw sub-map batch: image must be uint8 %s (this executor's graphs were captured for that shape), got %s %s"
                         % (want, image.dtype, tuple(image.shape)))
    K_raw = torch.as_tensor(host_batch["K_raw"])
    P_cam_pc = torch.as_tensor(host_batch["P_cam_pc"])
    if tuple(K_raw.shape) != (B, 3, 3) or tuple(P_cam_pc.shape) != (B, 4, 4):
        raise ValueError("raw sub-map batch: K_raw must be [%d,3,3] and P_cam_pc [%d,4,4], got %s and %s"
                         % (B, B, tuple(K_raw.shape), tuple(P_cam_pc.shape)))
    seed = host_batch.get("seed")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
    return (parts, t(so, np.int32), t(mo, np.int32), t(poses, np.float64), t(present, np.uint8), t(Gl, np.float64), t(Gc, np.float64), image, K_raw,
            P_cam_pc, 0 if seed is None else int(seed))


class OxfordFrameExecutor(PreparedFrameExecutor):
    """executor = OxfordFrameExecutor(mm, pipe, opt, example_batch, S_cap, P_cap, cap_raw, max_frame_points, n_streams=4)
    ticket = executor.submit(host_batch)          # dict: submaps | the flat form, G_posesource_laser, G_cam, image, K_raw, P_cam_pc[, seed]
    out = executor.result(ticket)                 # the base executor's outputs + status i32[B], T_scan, P_cam_pc, P_scan f64[B,4,4]

    opt: the option bag of sample_prep(dataset="oxford") (img_H / img_W / input_pt_num / node numbers must be the classifier's).  Fixed per
    executor: B, the raw image shape, S_cap (profiles of a batch), P_cap (rows of the pinned staging buffer: a batch with more profiles or
    rows in all raises), cap_raw (surviving rows of the whole batch) and max_frame_points (a sub-map that keeps more rows is rejected ON THE
    DEVICE: status != 0, its pose is whatever the solver makes of zeros, the other sub-maps are unaffected); voxel, skip_threshold and
    ground_threshold are submap.OxfordRawPlan's.  T_scan = Pr . G_cam maps coordinates in the sub-map's origin vehicle frame (what
    submap.build_raw writes) onto the prepared points, so P_scan = P . T_scan maps them into the camera frame; P_cam_pc is the staged one.
    The seed of the preparation's draws is staged with the batch and read from device memory inside the graph.

    evaluate=True: the base executor's evaluation mode with the ground truth the preparation produces itself -- the pose P of the prepared
    points (the sample's f32 [B,3,4]) against the solver's out["P"] -- and status == 0 as the frame mask: a sub-map with status 1 or 4 is
    absent from the statistics.  visualize: passed through; the overlays are drawn over the PREPARED image from the prepared points, with
    the prepared K."""

    BATCH, ROWS = "raw sub-map batch", "scan_xyr"

    def __init__(self, mm, pipe, opt, example_batch, S_cap, P_cap, cap_raw, max_frame_points, n_streams=4, use_graph=True, restarts=None,
                 samples=None, labels_override=None, mode="val", voxel=submap.VOXEL, skip_threshold=None, ground_threshold=None,
                 h2d_mode="copy_stream", post_fn=None, evaluate=False, visualize=None, confidence=False):
        self._check_h2d_mode(h2d_mode)
        _ragged._check_max_frame_points("submap", max_frame_points)
        submap._skip_arg(skip_threshold)
        submap._ground_args(ground_threshold)
        self._read_example(example_batch.get("image"))
        self.opt, self.mode, self.voxel, self.skip_threshold, self.ground_threshold = opt, mode, voxel, skip_threshold, ground_threshold
        self.S_cap, self.P_cap, self.cap_raw, self.max_frame_points = int(S_cap), int(P_cap), int(cap_raw), int(max_frame_points)
        sample_prep.option_block(opt, self.raw_hw, mode, dataset="oxford")
        self._check_batch(example_batch)
        super().__init__(mm, pipe, example_batch, n_streams=n_streams, use_graph=use_graph, restarts=restarts, labels_override=labels_override,
                         post_fn=post_fn, h2d_mode=h2d_mode, samples=samples, evaluate=evaluate, visualize=visualize, confidence=confidence)

    def _check_batch(self, host_batch):
        return host_submap_frames(host_batch, self.B, self.S_cap, self.P_cap, self.raw_hw)

    def _staged_inputs(self, example_batch, B):
        H, W = self.raw_hw
        S = max(self.S_cap, 1)
        return [("submap_offsets", (B + 1,), torch.int32), ("scan_offsets", (S + 1,), torch.int32), ("seed", (1,), torch.int64),
                ("K_raw", (B, 3, 3), torch.float64), ("P_cam_pc", (B, 4, 4), torch.float64), ("G_posesource_laser", (4, 4), torch.float64),
                ("G_cam", (B, 4, 4), torch.float64), ("present", (S,), torch.uint8), ("poses", (S, 4, 4), torch.float64),
                ("image", (B, H, W, 3), torch.uint8), ("scan_xyr", (max(self.P_cap, 1), 3), torch.float64)]

    def _copy_staged(self, h, staged):
        parts, so, mo, poses, present, Gl, Gc, image, K_raw, P_cam_pc, seed = staged
        S = int(mo[-1])
        h["submap_offsets"].copy_(mo)
        h["scan_offsets"][:S + 1].copy_(so)
        h["scan_offsets"][S + 1:].fill_(int(so[-1]))           # profiles past submap_offsets[B] are never read; they hold the end of the rows
        h["seed"].fill_(seed)
        h["K_raw"].copy_(K_raw)
        h["P_cam_pc"].copy_(P_cam_pc)
        h["G_posesource_laser"].copy_(Gl)
        h["G_cam"].copy_(Gc)
        h["present"][:S].copy_(present)
        h["present"][S:].fill_(0)
        h["poses"][:S].copy_(poses)
        h["poses"][S:] = torch.eye(4, dtype=torch.float64)
        h["image"].copy_(image)
        return self._lay_rows(h["scan_xyr"], parts)

    def _make_plan(self):
        return submap.OxfordRawPlan(self.opt, self.B, max(self.S_cap, 1), max(self.P_cap, 1), self.cap_raw, self.max_frame_points, self.raw_hw,
                                    self.mode, self.voxel, self.skip_threshold, self.ground_threshold, self.device)

    def _run_plan(self, plan, d):
        return plan.run(d["scan_xyr"], d["scan_offsets"], d["submap_offsets"], d["poses"], d["present"], d["G_posesource_laser"], d["G_cam"],
                        d["image"], d["K_raw"], d["P_cam_pc"], seed=None, with_T_scan=True)

    def _normals(self, plan):
        return plan.sample.sn          # the Oxford records have no normals: the plan's zero buffer

    def _extra_outputs(self, slot):
        return dict(P_cam_pc=slot.dev["P_cam_pc"])
