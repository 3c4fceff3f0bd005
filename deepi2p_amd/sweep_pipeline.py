"""Raw-sweep executor: "here are a nuScenes sample's LiDAR sweeps, its records and a camera frame, give me the pose" on
raw_pipeline.PreparedFrameExecutor.

One STEP = H2D copy of the raw batch -> sweeps.NuScenesRawPlan (pose matrices, sweep transforms and P_cam_pc, ego-box filter and
accumulation, the loader's sample preparation, image path) -> classifier -> pose solve (Gauss-Newton restarts or PnP-RANSAC) ->
P_scan = P . T_scan.  The staging, the step and the evaluation mode are the base class's, shared with raw_pipeline.RawFrameExecutor; this
module has the host check of a sweep batch (host_sweep_frames) and the subclass that names the staged inputs, the plan and P_cam_pc.
nuScenes clouds are z-up: build the pipeline with frame="enu".
"""
import numpy as np
import torch

from . import _ragged, sample_prep, sweeps
from .raw_pipeline import PreparedFrameExecutor

RECORDS = ("lidar_calib", "cam_pose", "cam_calib")


def host_sweep_frames(host_batch, B, S_cap, cap_raw, raw_hw, cols=None):
    """Check a raw host batch against the shapes an executor was built for and bring it to its staged form; host-only, raises ValueError
    before anything is enqueued.  host_batch: dict with `sweeps` (per frame a list of float32 arrays [n, cols], the key sweep first, then the
    `next` picks, then the `prev` picks; or a flat [total, cols] array plus `sweep_offsets` [S+1] and `frame_offsets` [B+1]), `ego` (one
    record (w, x, y, z, tx, ty, tz) per sweep: [S, 7], or per frame an [S_b, 7] array), `lidar_calib`, `cam_pose`, `cam_calib` [B, 7],
    `image` u8[B,H,W,3], `K_raw` [B,3,3] and optionally `seed`.  Rows of another dtype than float32 raise in both forms.  cols: the columns the executor was built
    for; None (the example batch): whatever the batch has, 4 or 5.
    -> (parts: list of f32 tensors to lay end to end, sweep_offsets i32[S+1], frame_offsets i32[B+1], ego f64[S,7], three f64[B,7] records,
        image, K_raw, seed int, cols)"""
    for k in ("sweeps", "ego") + RECORDS + ("image", "K_raw"):
        if k not in host_batch:
            raise ValueError("raw sweep batch has no %r (sweeps, ego, lidar_calib, cam_pose, cam_calib, image, K_raw[, sweep_offsets, frame_offsets, "
                             "seed])" % k)
    sw = host_batch["sweeps"]
    if isinstance(sw, (list, tuple)):
        parts, so, fo, cols = sweeps.host_sweeps(sw, cols)
        parts = [torch.as_tensor(p) for p in parts]
    else:
        if host_batch.get("sweep_offsets") is None or host_batch.get("frame_offsets") is None:
            raise ValueError("raw sweep batch: a flat `sweeps` array needs `sweep_offsets` [S+1] and `frame_offsets` [B+1]")
        flat = torch.as_tensor(sw)
        if flat.dim() != 2 or flat.shape[1] != (cols or flat.shape[1]) or flat.shape[1] not in (4, 5):
            raise ValueError("raw sweep batch: flat sweeps must be [total, %s], got %s" % (cols or "4 | 5", tuple(flat.shape)))
        cols = int(flat.shape[1])
        if flat.dtype != torch.float32:
            raise ValueError("raw sweep batch: sweeps must be float32")
        so = np.asarray(host_batch["sweep_offsets"]).astype(np.int64).reshape(-1)
        fo = np.asarray(host_batch["frame_offsets"]).astype(np.int64).reshape(-1)
        if len(so) < 1 or so[0] != 0 or np.any(np.diff(so) < 0) or so[-1] > flat.shape[0]:
            raise ValueError("raw sweep batch: sweep_offsets must start at 0, not decrease and end within the %d rows of sweeps" % flat.shape[0])
        if len(fo) < 1 or fo[0] != 0 or np.any(np.diff(fo) < 0) or fo[-1] != len(so) - 1:
            raise ValueError("raw sweep batch: frame_offsets must start at 0, not decrease and end at the %d sweeps of sweep_offsets" % (len(so) - 1))
        parts = [flat[:int(so[-1])]]
    if len(fo) != B + 1:
        raise ValueError("raw sweep batch has %d frames, this executor was built (and its graphs captured) for B = %d" % (len(fo) - 1, B))
    S, total = int(fo[-1]), int(so[-1])
    if S > S_cap:
        raise ValueError("raw sweep batch has %d sweeps in all, above the S_cap = %d this executor stages" % (S, S_cap))
    if total > cap_raw:
        raise ValueError("raw sweep batch has %d rows in all, above the cap_raw = %d rows this executor stages" % (total, cap_raw))
    ego = sweeps.host_ego(host_batch["ego"], S)
    recs = []
    for k in RECORDS:
        r = np.asarray(host_batch[k], dtype=np.float64)
        if r.shape != (B, 7):
            raise ValueError("raw sweep batch: %s must be [%d, 7] (w, x, y, z, tx, ty, tz), got %s" % (k, B, list(r.shape)))
        recs.append(torch.from_numpy(np.ascontiguousarray(r)))
    image = torch.as_tensor(host_batch["image"])
    want = (B, int(raw_hw[0]), int(raw_hw[1]), 3)
    if image.dtype != torch.uint8 or tuple(image.shape) != want:
        raise ValueError("raw sweep batch: image must be uint8 %s (this executor's graphs were captured for that shape), got %s %s"
                         % (want, image.dtype, tuple(image.shape)))
    K_raw = torch.as_tensor(host_batch["K_raw"])
    if tuple(K_raw.shape) != (B, 3, 3):
        raise ValueError("raw sweep batch: K_raw must be [%d,3,3], got %s" % (B, tuple(K_raw.shape)))
    seed = host_batch.get("seed")
    return (parts, torch.from_numpy(so.astype(np.int32)), torch.from_numpy(fo.astype(np.int32)), torch.from_numpy(np.ascontiguousarray(ego)), recs,
            image, K_raw, 0 if seed is None else int(seed), cols)


class SweepFrameExecutor(PreparedFrameExecutor):
    """executor = SweepFrameExecutor(mm, pipe, opt, example_batch, S_cap, cap_raw, max_frame_points, n_streams=4)
    ticket = executor.submit(host_batch)          # dict: sweeps, ego, lidar_calib, cam_pose, cam_calib, image, K_raw[, offsets, seed]
    out = executor.result(ticket)                 # the base executor's outputs + status i32[B], T_scan, P_cam_pc, P_scan f64[B,4,4]

    opt: the option bag of sample_prep(dataset="nuscenes") (img_H / img_W / input_pt_num / node numbers must be the classifier's).  Fixed per
    executor: B, the raw image shape, the columns of a row (4 or 5, the example's), S_cap (sweeps of a batch), cap_raw (rows of the pinned
    staging buffer and of the accumulated cloud: a batch with more sweeps or rows in all raises) and max_frame_points (a frame that keeps more
    rows is rejected ON THE DEVICE: status != 0, its pose is whatever the solver makes of zeros, the other frames are unaffected).
    P_scan = P . T_scan maps the accumulated cloud (the key sweep's LiDAR frame) into the camera frame; P_cam_pc is the data set's own
    transform between the two.  The seed of the preparation's draws is staged with the batch and read from device memory inside the graph.

    evaluate=True: the base executor's evaluation mode with the ground truth the preparation produces itself -- the pose P of the prepared
    points (the sample's f32 [B,3,4]) against the solver's out["P"] -- and status == 0 as the frame mask.  visualize: passed through; the
    overlays are drawn over the PREPARED image from the prepared points, with the prepared K."""

    BATCH, ROWS = "raw sweep batch", "rows"
    cols = None          # while the example batch itself is checked: whatever it has

    def __init__(self, mm, pipe, opt, example_batch, S_cap, cap_raw, max_frame_points, n_streams=4, use_graph=True, restarts=None, samples=None,
                 labels_override=None, mode="val", box=sweeps.BOX, h2d_mode="copy_stream", post_fn=None, evaluate=False, visualize=None, confidence=False):
        self._check_h2d_mode(h2d_mode)
        _ragged._check_max_frame_points("sweeps", max_frame_points)
        sweeps._box(box)
        self._read_example(example_batch.get("image"))
        self.opt, self.mode, self.box = opt, mode, box
        self.S_cap, self.cap_raw, self.max_frame_points = int(S_cap), int(cap_raw), int(max_frame_points)
        sample_prep.option_block(opt, self.raw_hw, mode, dataset="nuscenes")
        self.cols = self._check_batch(example_batch)[-1]          # 4 or 5: the example's
        super().__init__(mm, pipe, example_batch, n_streams=n_streams, use_graph=use_graph, restarts=restarts, labels_override=labels_override,
                         post_fn=post_fn, h2d_mode=h2d_mode, samples=samples, evaluate=evaluate, visualize=visualize, confidence=confidence)

    def _check_batch(self, host_batch):
        return host_sweep_frames(host_batch, self.B, self.S_cap, self.cap_raw, self.raw_hw, self.cols)

    def _staged_inputs(self, example_batch, B):
        H, W = self.raw_hw
        S = max(self.S_cap, 1)
        return [("frame_offsets", (B + 1,), torch.int32), ("sweep_offsets", (S + 1,), torch.int32), ("seed", (1,), torch.int64),
                ("K_raw", (B, 3, 3), torch.float64), ("lidar_calib", (B, 7), torch.float64), ("cam_pose", (B, 7), torch.float64),
                ("cam_calib", (B, 7), torch.float64), ("ego", (S, 7), torch.float64), ("image", (B, H, W, 3), torch.uint8),
                ("rows", (max(self.cap_raw, 1), self.cols), torch.float32)]

    def _copy_staged(self, h, staged):
        parts, so, fo, ego, recs, image, K_raw, seed, _ = staged
        S = int(fo[-1])
        h["frame_offsets"].copy_(fo)
        h["sweep_offsets"][:S + 1].copy_(so)
        h["sweep_offsets"][S + 1:].fill_(int(so[-1]))          # sweeps past frame_offsets[B] are never read; they hold the end of the rows
        h["seed"].fill_(seed)
        h["K_raw"].copy_(K_raw)
        for k, r in zip(RECORDS, recs):
            h[k].copy_(r)
        h["ego"][:S].copy_(ego)
        h["ego"][S:] = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], dtype=torch.float64)
        h["image"].copy_(image)
        return self._lay_rows(h["rows"], parts)

    def _make_plan(self):
        return sweeps.NuScenesRawPlan(self.opt, self.B, max(self.S_cap, 1), max(self.cap_raw, 1), self.cap_raw, self.max_frame_points, self.raw_hw,
                                      self.mode, self.cols, self.box, self.device)

    def _run_plan(self, plan, d):
        return plan.run(d["rows"], d["sweep_offsets"], d["frame_offsets"], d["ego"], d["lidar_calib"], d["cam_pose"], d["cam_calib"], d["image"],
                        d["K_raw"], seed=None)

    def _normals(self, plan):
        return plan.sample.sn          # the nuScenes records have no normals: the plan's zero buffer

    def _extra_outputs(self, slot):
        return dict(P_cam_pc=slot.plan.P_cam_pc)
