"""Raw-frame executors: "here is what the sensors wrote, give me the pose" on the machinery of pipeline.RegistrationExecutor.

One STEP = H2D copy of the raw batch -> a preparation plan -> classifier -> pose solve (Gauss-Newton restarts or PnP-RANSAC) ->
P_scan = P . T_scan.  Streams, slots, pinned staging, copy streams, one captured graph per slot, weight following and submit / result
tickets are RegistrationExecutor's.  PreparedFrameExecutor puts a preparation plan in front of the step: the checked-once staging of a
host batch, the plan's outputs wired in place of the staged network inputs, the step, the composed pose and the ground truth of the
evaluation mode.  A front end is a subclass that names its staged inputs, its host check and its plan:
  RawFrameExecutor                        a KITTI scan and a camera frame          raw_prep.RawFramePlan (voxel grid, normals, nearest-raw
                                                                                   intensity, the loader's sample preparation, image path)
  sweep_pipeline.SweepFrameExecutor       a nuScenes sample's sweeps and records   sweeps.NuScenesRawPlan
  submap_pipeline.OxfordFrameExecutor     an Oxford traversal's LMS profiles       submap.OxfordRawPlan
"""
import numpy as np
import torch

from . import raw_prep, scan_prep
from ._lib import call, ptr, stream
from .pipeline import INPUT_NAMES, K_NAME, RegistrationExecutor
from .sample_prep import I_K, I_P, I_STATUS, I_T_SCAN


def host_frames(host_batch, B, cap_raw, raw_hw):
    """Check a raw host batch against the shapes an executor was built for and bring it to its staged form; host-only, raises ValueError
    before anything is enqueued.  host_batch: dict with `scans` (a list of B [n_b,4] float32 arrays, or a flat [total,4] array plus
    `offsets` [B+1]), `image` u8[B,H,W,3], `K_raw` [B,3,3], `Pc` [B,4,4] and optionally `seed`.  Scans of another dtype than float32 raise
    in both forms (nothing is cast silently).
    -> (points: list of f32 tensors [n,4] to lay end to end, offsets i32[B+1] tensor, image, K_raw f64, Pc f64, seed int)"""
    for k in ("scans", "image", "K_raw", "Pc"):
        if k not in host_batch:
            raise ValueError("raw host batch has no %r (scans, image, K_raw, Pc[, offsets, seed])" % k)
    scans = host_batch["scans"]
    if isinstance(scans, (list, tuple)):
        parts = [torch.as_tensor(s) for s in scans]
        if any(p.dim() != 2 or p.shape[1] != 4 for p in parts):
            raise ValueError("raw host batch: every scan must be [n, 4] (x, y, z, intensity)")
        counts = [int(p.shape[0]) for p in parts]
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    else:
        if host_batch.get("offsets") is None:
            raise ValueError("raw host batch: a flat `scans` array needs `offsets` [B+1]")
        flat = torch.as_tensor(scans)
        if flat.dim() != 2 or flat.shape[1] != 4:
            raise ValueError("raw host batch: flat scans must be [total, 4], got %s" % (tuple(flat.shape),))
        offsets = torch.as_tensor(np.asarray(host_batch["offsets"])).to(torch.int32).reshape(-1)
        o = offsets.tolist()
        if len(o) < 1 or o[0] != 0 or any(b < a for a, b in zip(o, o[1:])) or o[-1] > flat.shape[0]:
            raise ValueError("raw host batch: offsets must start at 0, not decrease and end within the %d rows of scans" % flat.shape[0])
        parts = [flat[:o[-1]]]
    if offsets.shape[0] != B + 1:
        raise ValueError("raw host batch has %d frames, this executor was built (and its graphs captured) for B = %d" % (offsets.shape[0] - 1, B))
    total = int(offsets[-1])
    if total > cap_raw:
        raise ValueError("raw host batch has %d points in all, above the cap_raw = %d rows this executor stages" % (total, cap_raw))
    for p in parts:
        if p.dtype != torch.float32:
            raise ValueError("raw host batch: scans must be float32")
    image = torch.as_tensor(host_batch["image"])
    want = (B, int(raw_hw[0]), int(raw_hw[1]), 3)
    if image.dtype != torch.uint8 or tuple(image.shape) != want:
        raise ValueError("raw host batch: image must be uint8 %s (this executor's graphs were captured for that shape), got %s %s"
                         % (want, image.dtype, tuple(image.shape)))
    K_raw, Pc = torch.as_tensor(host_batch["K_raw"]), torch.as_tensor(host_batch["Pc"])
    if tuple(K_raw.shape) != (B, 3, 3) or tuple(Pc.shape) != (B, 4, 4):
        raise ValueError("raw host batch: K_raw must be [%d,3,3] and Pc [%d,4,4], got %s and %s" % (B, B, tuple(K_raw.shape), tuple(Pc.shape)))
    seed = host_batch.get("seed")
    return parts, offsets, image, K_raw, Pc, 0 if seed is None else int(seed)


class PreparedFrameExecutor(RegistrationExecutor):
    """RegistrationExecutor with a preparation plan in front of the step.  The plan (slot.plan, one per slot) has a `sample`
    (sample_prep.SamplePlan) and a run() that returns SamplePlan.run's nine tensors + (status i32[B], T_scan f64[B,4,4]): sample_prep.PREPARED.

    A subclass sets BATCH (its host batch's name in messages) and ROWS (the staged row buffer), checks its own arguments and calls
    _check_h2d_mode and _read_example in the order its constructor documents, then this constructor; and defines
      _check_batch(host_batch) -> the staged form (host-only; raises ValueError for a batch the executor was not built for)
      _staged_inputs(example_batch, B)      with a "seed" i64[1] and the ROWS buffer last: a step copies that one only up to its last row in use
      _copy_staged(h, staged) -> rows       copies a staged form into the pinned views h, returns the rows written to h[ROWS]
      _make_plan() -> plan,  _run_plan(plan, d) -> the prepared tuple from the slot's device inputs d,  _normals(plan) -> sn f32[B,3,N]
      _extra_outputs(slot) -> dict          results beside status, T_scan and P_scan (default: none)"""
    BATCH = ROWS = None
    _checked = None          # (host batch, its staged form) between _validate and _stage

    def __init__(self, mm, pipe, example_batch, **kw):
        super().__init__(mm, pipe, torch.eye(3, dtype=torch.float64), example_batch, **kw)

    def _check_h2d_mode(self, h2d_mode):
        if h2d_mode not in ("copy_stream", "eager"):
            raise ValueError("%s: h2d_mode must be 'copy_stream' or 'eager' (a captured copy has a fixed size; the raw copy has not)" % type(self).__name__)

    def _read_example(self, image):
        """B and the raw image shape are the example image's"""
        image = None if image is None else torch.as_tensor(image)
        if image is None or image.dim() != 4:
            raise ValueError("%s: image must be uint8 [B, H, W, 3]" % self.BATCH)
        self.B, self.raw_hw = int(image.shape[0]), (int(image.shape[1]), int(image.shape[2]))

    def _extra_outputs(self, slot):
        return {}

    @staticmethod
    def _lay_rows(dst, parts):
        """for _copy_staged: the row arrays of a staged form end to end into the pinned row buffer -> rows written"""
        row = 0
        for p in parts:
            dst[row:row + p.shape[0]].copy_(p)
            row += int(p.shape[0])
        return row

    # ---------------------------------------------------------------------------------------------------------- staged inputs
    def _batch_size(self, example_batch):
        return self.B

    def _validate(self, slot, host_batch):
        self._checked = (host_batch, self._check_batch(host_batch))      # submit stages it next: converted once

    def _stage(self, slot, host_batch):
        checked, self._checked = self._checked, None
        staged = checked[1] if checked is not None and checked[0] is host_batch else self._check_batch(host_batch)
        rows = slot.host[self.ROWS]
        n = self._copy_staged(slot.host, staged)
        # rows past the last one written stay stale: they are not copied and no kernel reads them
        slot.copy_bytes = rows.data_ptr() - slot.host_flat.data_ptr() + rows.element_size() * rows.shape[1] * n

    def _stage_example(self, slot, example_batch):
        slot.host[self.ROWS].zero_()
        self._stage(slot, example_batch)

    def _slot_ready(self, slot):
        d = slot.devs[0]
        plan = self._make_plan()
        plan.sample.seed = d["seed"]          # the draws read the staged seed where the copy puts it
        slot.plan = plan
        slot.K64 = torch.zeros((self.B, 3, 3), dtype=torch.float64, device=self.device)
        slot.P_scan = torch.zeros((self.B, 4, 4), dtype=torch.float64, device=self.device)
        if self.evaluate:
            slot.P_gt64 = torch.zeros((self.B, 3, 4), dtype=torch.float64, device=self.device)
            slot.mask = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        p = plan.sample
        # what _net_part / _solve_part read: the plan's outputs, in place
        d.update(zip(INPUT_NAMES, (p.points.pc, p.points.intensity, self._normals(plan), p.points.nodes[0], p.points.nodes[1], p.image.img)))
        d[K_NAME] = slot.K64

    # ---------------------------------------------------------------------------------------------------------- one step
    def _step(self, slot, with_h2d):
        if with_h2d:
            slot.copy_in()
        prepared = self._run_plan(slot.plan, slot.dev)
        slot.K64.copy_(prepared[I_K])                                        # the prepared f32 K, as the base executor stages it: f64
        slot.prepared = prepared
        out = self._solve_part(slot, self._net_part(slot))
        P = out["P"]
        if P.dtype != torch.float64 or tuple(P.shape) != (self.B, 4, 4) or not P.is_contiguous():
            raise ValueError("%s: the pose solve must return P as contiguous f64 [B,4,4]" % type(self).__name__)
        call("di2p_compose_poses", ptr(P), ptr(prepared[I_T_SCAN]), self.B, ptr(slot.P_scan), stream())
        out.update(status=prepared[I_STATUS], T_scan=prepared[I_T_SCAN], **self._extra_outputs(slot), P_scan=slot.P_scan)
        return out

    def _eval_truth(self, slot):
        prepared = slot.prepared
        slot.P_gt64.copy_(prepared[I_P])                                     # the sample's own pose of the prepared points, f32 -> f64
        slot.mask.copy_(prepared[I_STATUS] == 0)                             # a rejected frame (status != 0) is skipped entirely
        return slot.P_gt64, prepared[I_P], prepared[I_K], slot.mask


class RawFrameExecutor(PreparedFrameExecutor):
    """executor = RawFrameExecutor(mm, pipe, opt, example_batch, cap_raw, max_frame_points, n_streams=4)
    ticket = executor.submit(host_batch)          # dict: scans, image, K_raw, Pc[, offsets, seed] (host_frames)
    out = executor.result(ticket)                 # the base executor's outputs + status i32[B], T_scan, P_scan f64[B,4,4]

    opt: the option bag of sample_prep (img_H / img_W / input_pt_num / node numbers must be the classifier's).  Fixed per executor: B, the
    raw image shape, cap_raw (rows of the pinned staging buffer: a batch with more points in all raises) and max_frame_points (a longer
    frame is rejected ON THE DEVICE: status != 0, its pose is whatever the solver makes of zeros, the other frames are unaffected).
    P_scan = P . T_scan maps raw-scan coordinates into the camera frame.  The seed of the preparation's draws is staged with the batch and
    read from device memory inside the graph.

    evaluate=True: the base executor's evaluation mode with the ground truth the preparation produces itself -- the pose P of the prepared
    points (the sample's f32 [B,3,4]) against the solver's out["P"] -- and status != 0 as the frame mask: a rejected frame is absent from
    the statistics.  No host "P" is needed.

    visualize: the base executor's option, passed through; the overlays are drawn over the PREPARED image (the network's input) from the
    prepared points, with the prepared K."""
    BATCH, ROWS = "raw host batch", "points"

    def __init__(self, mm, pipe, opt, example_batch, cap_raw, max_frame_points, n_streams=4, use_graph=True, restarts=None, samples=None,
                 labels_override=None, mode="val", dataset="kitti", normals_method="query", h2d_mode="copy_stream", post_fn=None, evaluate=False,
                 visualize=None, confidence=False):
        raw_prep._check_dataset(dataset)
        scan_prep._normals_entry(normals_method)
        self._check_h2d_mode(h2d_mode)
        self._read_example(example_batch["image"])
        self.opt, self.mode, self.dataset, self.normals_method = opt, mode, dataset, normals_method
        self.cap_raw, self.max_frame_points = int(cap_raw), int(max_frame_points)
        self._check_batch(example_batch)
        super().__init__(mm, pipe, example_batch, n_streams=n_streams, use_graph=use_graph, restarts=restarts, labels_override=labels_override,
                         post_fn=post_fn, h2d_mode=h2d_mode, samples=samples, evaluate=evaluate, visualize=visualize, confidence=confidence)

    def _check_batch(self, host_batch):
        return host_frames(host_batch, self.B, self.cap_raw, self.raw_hw)

    def _staged_inputs(self, example_batch, B):
        H, W = self.raw_hw
        return [("offsets", (B + 1,), torch.int32), ("seed", (1,), torch.int64), ("K_raw", (B, 3, 3), torch.float64), ("Pc", (B, 4, 4), torch.float64),
                ("image", (B, H, W, 3), torch.uint8), ("points", (max(self.cap_raw, 1), 4), torch.float32)]

    def _copy_staged(self, h, staged):
        parts, offsets, image, K_raw, Pc, seed = staged
        h["offsets"].copy_(offsets)
        h["seed"].fill_(seed)
        h["K_raw"].copy_(K_raw)
        h["Pc"].copy_(Pc)
        h["image"].copy_(image)
        return self._lay_rows(h["points"], parts)

    def _make_plan(self):
        return raw_prep.RawFramePlan(self.opt, self.B, self.cap_raw, self.max_frame_points, self.raw_hw, self.mode, self.dataset, self.normals_method,
                                     self.device)

    def _run_plan(self, plan, d):
        return plan.run(d["points"], d["offsets"], d["image"], d["K_raw"], d["Pc"], None, seed=None)

    def _normals(self, plan):
        return plan.sample.points.sn
