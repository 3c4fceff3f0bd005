"""Raw-sweep executor: "here are a nuScenes sample's LiDAR sweeps, its records and a camera frame, give me the pose" on the machinery of
pipeline.RegistrationExecutor.

One STEP = H2D copy of the raw batch -> sweeps.NuScenesRawPlan (pose matrices, sweep transforms and P_cam_pc, ego-box filter and
accumulation, the loader's sample preparation, image path) -> classifier -> pose solve (Gauss-Newton restarts or PnP-RANSAC) ->
P_scan = P . T_scan.  Streams, slots, pinned staging, copy streams, one captured graph per slot, weight following and submit / result tickets
are the base class's; this class only describes other staged inputs and puts the preparation in front of the step, as
raw_pipeline.RawFrameExecutor does for KITTI scans.  nuScenes clouds are z-up: build the pipeline with frame="enu".
"""
import numpy as np
import torch

from . import sweeps
from ._lib import call, ptr, stream
from .pipeline import INPUT_NAMES, K_NAME, RegistrationExecutor

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


class SweepFrameExecutor(RegistrationExecutor):
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

    def __init__(self, mm, pipe, opt, example_batch, S_cap, cap_raw, max_frame_points, n_streams=4, use_graph=True, restarts=None, samples=None,
                 labels_override=None, mode="val", box=sweeps.BOX, h2d_mode="copy_stream", post_fn=None, evaluate=False, visualize=None):
        if h2d_mode not in ("copy_stream", "eager"):
            raise ValueError("SweepFrameExecutor: h2d_mode must be 'copy_stream' or 'eager' (a captured copy has a fixed size; the raw copy has not)")
        sweeps._check_max_frame_points(max_frame_points)
        sweeps._box(box)
        if "image" not in example_batch or torch.as_tensor(example_batch["image"]).dim() != 4:
            raise ValueError("raw sweep batch: image must be uint8 [B, H, W, 3]")
        image = torch.as_tensor(example_batch["image"])
        self.opt, self.mode, self.box = opt, mode, box
        self.B, self.raw_hw = int(image.shape[0]), (int(image.shape[1]), int(image.shape[2]))
        self.S_cap, self.cap_raw, self.max_frame_points = int(S_cap), int(cap_raw), int(max_frame_points)
        from . import sample_prep
        sample_prep.option_block(opt, self.raw_hw, mode, dataset="nuscenes")
        self.cols = host_sweep_frames(example_batch, self.B, self.S_cap, self.cap_raw, self.raw_hw)[-1]          # 4 or 5: the example's
        super().__init__(mm, pipe, torch.eye(3, dtype=torch.float64), example_batch, n_streams=n_streams, use_graph=use_graph, restarts=restarts,
                         labels_override=labels_override, post_fn=post_fn, h2d_mode=h2d_mode, samples=samples, evaluate=evaluate, visualize=visualize)

    # ---------------------------------------------------------------------------------------------------------- staged inputs
    def _batch_size(self, example_batch):
        return self.B

    def _staged_inputs(self, example_batch, B):
        H, W = self.raw_hw
        S = max(self.S_cap, 1)
        # rows LAST: a step copies the buffer only up to its last row in use
        return [("frame_offsets", (B + 1,), torch.int32), ("sweep_offsets", (S + 1,), torch.int32), ("seed", (1,), torch.int64),
                ("K_raw", (B, 3, 3), torch.float64), ("lidar_calib", (B, 7), torch.float64), ("cam_pose", (B, 7), torch.float64),
                ("cam_calib", (B, 7), torch.float64), ("ego", (S, 7), torch.float64), ("image", (B, H, W, 3), torch.uint8),
                ("rows", (max(self.cap_raw, 1), self.cols), torch.float32)]

    def _check(self, host_batch):
        return host_sweep_frames(host_batch, self.B, self.S_cap, self.cap_raw, self.raw_hw, self.cols)

    def _validate(self, slot, host_batch):
        self._checked = (host_batch, self._check(host_batch))      # submit stages it next: converted once

    def _stage(self, slot, host_batch):
        checked, self._checked = getattr(self, "_checked", None), None
        staged = checked[1] if checked is not None and checked[0] is host_batch else self._check(host_batch)
        parts, so, fo, ego, recs, image, K_raw, seed, _ = staged
        h = slot.host
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
        row = 0
        for p in parts:
            h["rows"][row:row + p.shape[0]].copy_(p)
            row += int(p.shape[0])
        # rows past the last sweep offset stay stale: they are not copied and no kernel reads them
        slot.copy_bytes = h["rows"].data_ptr() - slot.host_flat.data_ptr() + 4 * self.cols * row

    def _stage_example(self, slot, example_batch):
        slot.host["rows"].zero_()
        self._stage(slot, example_batch)

    def _slot_ready(self, slot):
        d = slot.devs[0]
        plan = sweeps.NuScenesRawPlan(self.opt, self.B, max(self.S_cap, 1), max(self.cap_raw, 1), self.cap_raw, self.max_frame_points, self.raw_hw,
                                      self.mode, self.cols, self.box, self.device)
        plan.sample.seed = d["seed"]          # the draws read the staged seed where the copy puts it
        slot.plan = plan
        slot.K64 = torch.zeros((self.B, 3, 3), dtype=torch.float64, device=self.device)
        slot.P_scan = torch.zeros((self.B, 4, 4), dtype=torch.float64, device=self.device)
        if self.evaluate:
            slot.P_gt64 = torch.zeros((self.B, 3, 4), dtype=torch.float64, device=self.device)
            slot.mask = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        p = plan.sample
        # what _net_part / _solve_part read: the plan's outputs, in place (the nuScenes records have no normals: sn is the plan's zero buffer)
        d.update(zip(INPUT_NAMES, (p.points.pc, p.points.intensity, p.sn, p.points.nodes[0], p.points.nodes[1], p.image.img)))
        d[K_NAME] = slot.K64

    # ---------------------------------------------------------------------------------------------------------- one step
    def _step(self, slot, with_h2d):
        if with_h2d:
            slot.copy_in()
        d = slot.dev
        prepared = slot.plan.run(d["rows"], d["sweep_offsets"], d["frame_offsets"], d["ego"], d["lidar_calib"], d["cam_pose"], d["cam_calib"],
                                 d["image"], d["K_raw"], seed=None)
        slot.K64.copy_(prepared[7])                                          # the prepared f32 K, as the base executor stages it: f64
        slot.prepared = prepared
        out = self._solve_part(slot, self._net_part(slot))
        P = out["P"]
        if P.dtype != torch.float64 or tuple(P.shape) != (self.B, 4, 4) or not P.is_contiguous():
            raise ValueError("SweepFrameExecutor: the pose solve must return P as contiguous f64 [B,4,4]")
        call("di2p_compose_poses", ptr(P), ptr(prepared[10]), self.B, ptr(slot.P_scan), stream())
        out.update(status=prepared[9], T_scan=prepared[10], P_cam_pc=slot.plan.P_cam_pc, P_scan=slot.P_scan)
        return out

    def _eval_truth(self, slot):
        prepared = slot.prepared
        slot.P_gt64.copy_(prepared[5])                                       # the sample's own pose of the prepared points, f32 -> f64
        slot.mask.copy_(prepared[9] == 0)                                    # a rejected frame (status != 0) is skipped entirely
        return slot.P_gt64, prepared[5], prepared[7], slot.mask
