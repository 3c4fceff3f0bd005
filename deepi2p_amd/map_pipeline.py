"""Map executor: "here is a camera frame and roughly where it was taken, give me the camera's pose in the map" on
raw_pipeline.PreparedFrameExecutor.

One STEP = H2D copy of the priors, radii and camera frames -> map_index.MapRawPlan (the crop of the resident map around every prior, in
the prior's frame; the loader's sample preparation; image path) -> classifier -> pose solve (Gauss-Newton restarts or PnP-RANSAC) ->
P_scan = P . T_scan -> T_map_cam = T_map_prior . P_scan^-1.  The map (map_index.MapIndex) stays on the device, is shared by all slots and is
never staged: a step copies 128 bytes of prior per frame where the other raw front ends copy a cloud.  The staging, the step and the
evaluation mode are the base class's; this module has the host check of a batch (host_map_frames) and the subclass that names the staged
inputs, the plan, the composed pose and the evaluation's ground truth.
"""
import numpy as np
import torch

from . import _ragged, map_index, sample_prep
from ._lib import call, ptr, stream
from .raw_pipeline import PreparedFrameExecutor
from .sample_prep import I_K, I_P, I_STATUS

KEYS = ("T_map_prior", "radius", "image", "K_raw")
BATCH = "map batch"


def host_map_frames(host_batch, B, raw_hw, max_radius=None):
    """Check a host batch against the shapes an executor was built for and bring it to its staged form; host-only, raises ValueError before
    anything is enqueued, and modifies nothing it is given.  host_batch: dict with `T_map_prior` [B,4,4] (map <- prior frame; a finite prior
    must be rigid to map_index.RIGID_TOL, a non-finite one is rejected on the device: status 5), `radius` (a number or [B]; a finite one above
    max_radius raises), `image` u8[B,H0,W0,3], `K_raw` [B,3,3], optionally `T_map_cam_gt` [B,4,4] (the camera's true pose in the map) and
    `seed`.  With ground truth the sample stage's P_cam_pc is inv(T_map_cam_gt) . T_map_prior, computed here in fp64; without, the identity.
    -> (T_map_prior f64[B,16], radius f64[B], image, K_raw, P_cam_pc f64[B,4,4], T_map_cam_gt f64[B,4,4] | None, seed int)"""
    for k in KEYS:
        if host_batch.get(k) is None:
            raise ValueError("%s has no %r (T_map_prior, radius, image, K_raw[, T_map_cam_gt, seed])" % (BATCH, k))
    T = map_index.check_priors(host_batch["T_map_prior"], B, prefix=BATCH)
    r = map_index.check_radius(host_batch["radius"], B, prefix=BATCH)
    if max_radius is not None and np.any(r[np.isfinite(r)] > max_radius):
        raise ValueError("%s: a radius above the max_radius = %g this executor's crop workspace was sized for" % (BATCH, max_radius))
    image = torch.as_tensor(host_batch["image"])
    want = (B, int(raw_hw[0]), int(raw_hw[1]), 3)
    if image.dtype != torch.uint8 or tuple(image.shape) != want:
        raise ValueError("%s: image must be uint8 %s (this executor's graphs were captured for that shape), got %s %s"
                         % (BATCH, want, image.dtype, tuple(image.shape)))
    K_raw = torch.as_tensor(host_batch["K_raw"])
    if tuple(K_raw.shape) != (B, 3, 3):
        raise ValueError("%s: K_raw must be [%d,3,3], got %s" % (BATCH, B, tuple(K_raw.shape)))
    gt = host_batch.get("T_map_cam_gt")
    P_cam_pc = np.tile(np.eye(4), (B, 1, 1))
    if gt is not None:
        gt = map_index.check_priors(gt, B, "T_map_cam_gt", BATCH)
        if not np.isfinite(gt).all():
            raise ValueError("%s: T_map_cam_gt must be finite" % BATCH)
        for b in range(B):
            if np.isfinite(T[b]).all():          # a non-finite prior has no rows: its P_cam_pc stays the identity
                inv = np.eye(4)
                inv[:3, :3] = gt[b, :3, :3].T
                inv[:3, 3] = -gt[b, :3, :3].T @ gt[b, :3, 3]
                P_cam_pc[b] = inv @ T[b]
        gt = torch.from_numpy(gt)
    seed = host_batch.get("seed")
    return (torch.from_numpy(T.reshape(B, 16)), torch.from_numpy(r), image, K_raw, torch.from_numpy(P_cam_pc), gt, 0 if seed is None else int(seed))


class MapFrameExecutor(PreparedFrameExecutor):
    """executor = MapFrameExecutor(mm, pipe, opt, index, example_batch, cap, max_frame_points, max_radius, n_streams=4)
    ticket = executor.submit(host_batch)          # dict: T_map_prior, radius, image, K_raw[, T_map_cam_gt, seed] (host_map_frames)
    out = executor.result(ticket)                 # the base executor's outputs + status i32[B], T_scan, P_scan, T_map_prior, T_map_cam f64[B,4,4]

    index: the map_index.MapIndex the frames are localised in.  opt: the option bag of sample_prep(dataset) (img_H / img_W / input_pt_num /
    node numbers must be the classifier's); dataset "oxford" (camera-convention maps, up_axis=1, pipeline frame="cam"), "nuscenes" (z-up
    maps, up_axis=2, frame="enu") or "kitti" (the index must carry normals, MapIndex.build(..., normals=...): the crop rotates them into
    the prior frame and the KITTI sample stage hands the classifier its `sn`).  Fixed per executor: B, the raw image shape, cap (kept rows of the whole batch), max_frame_points (a frame
    that keeps more rows is rejected ON THE DEVICE: status != 0, its pose is whatever the solver makes of zeros, the other frames are
    unaffected) and max_radius (the crop's window workspace).  P_scan = P . T_scan maps PRIOR-frame coordinates into the camera frame, so
    T_map_cam = T_map_prior . P_scan^-1 is the camera's pose in the map.

    evaluate=True needs `T_map_cam_gt` in every batch (ValueError otherwise).  The label accuracies are measured against the prepared sample's
    own pose as in the other raw executors; the pose errors are get_P_diff's rule on (T_map_cam, T_map_cam_gt) -- the RTE is the distance
    between the solved and the true camera position in the map -- with status == 0 as the frame mask: a frame whose prior lies off the map is
    absent from the statistics.  visualize: passed through."""

    BATCH, ROWS = BATCH, "T_map_prior"

    def __init__(self, mm, pipe, opt, index, example_batch, cap, max_frame_points, max_radius, n_streams=4, use_graph=True, restarts=None,
                 samples=None, labels_override=None, mode="val", dataset="oxford", h2d_mode="copy_stream", post_fn=None, evaluate=False,
                 visualize=None, confidence=False):
        self._check_h2d_mode(h2d_mode)
        map_index._check_dataset(dataset, index)
        _ragged._check_max_frame_points("map_index", max_frame_points)
        if not isinstance(index, map_index.MapIndex):
            raise ValueError("MapFrameExecutor: index must be a map_index.MapIndex (MapIndex.build)")
        self._read_example(example_batch.get("image"))
        self.opt, self.mode, self.dataset, self.index = opt, mode, dataset, index
        self.cap, self.max_frame_points, self.max_radius = int(cap), int(max_frame_points), float(max_radius)
        map_index.max_window_cells(index, max_radius)
        sample_prep.option_block(opt, self.raw_hw, mode, dataset=dataset)
        self.with_truth = bool(evaluate)
        self._check_batch(example_batch)
        super().__init__(mm, pipe, example_batch, n_streams=n_streams, use_graph=use_graph, restarts=restarts, labels_override=labels_override,
                         post_fn=post_fn, h2d_mode=h2d_mode, samples=samples, evaluate=evaluate, visualize=visualize, confidence=confidence)

    def _check_batch(self, host_batch):
        staged = host_map_frames(host_batch, self.B, self.raw_hw, self.max_radius)
        if self.with_truth and staged[5] is None:
            raise ValueError("evaluate=True: the %s has no ground-truth pose 'T_map_cam_gt' ([B,4,4])" % BATCH)
        return staged

    def _staged_inputs(self, example_batch, B):
        H, W = self.raw_hw
        truth = [("T_map_cam_gt", (B, 4, 4), torch.float64)] if self.with_truth else []
        return [("seed", (1,), torch.int64), ("radius", (B,), torch.float64), ("K_raw", (B, 3, 3), torch.float64),
                ("P_cam_pc", (B, 4, 4), torch.float64)] + truth + [("image", (B, H, W, 3), torch.uint8), ("T_map_prior", (B, 16), torch.float64)]

    def _copy_staged(self, h, staged):
        T, r, image, K_raw, P_cam_pc, gt, seed = staged
        h["seed"].fill_(seed)
        h["radius"].copy_(r)
        h["K_raw"].copy_(K_raw)
        h["P_cam_pc"].copy_(P_cam_pc)
        if self.with_truth:
            h["T_map_cam_gt"].copy_(gt)
        h["image"].copy_(image)
        h["T_map_prior"].copy_(T)
        return self.B          # the prior buffer's length does not vary

    def _make_plan(self):
        return map_index.MapRawPlan(self.index, self.opt, self.B, self.cap, self.max_frame_points, self.max_radius, self.raw_hw, self.mode,
                                    self.dataset)

    def _slot_ready(self, slot):
        super()._slot_ready(slot)
        slot.T_map_prior = slot.devs[0]["T_map_prior"].view(self.B, 4, 4)
        slot.T_map_cam = torch.zeros((self.B, 4, 4), dtype=torch.float64, device=self.device)

    def _run_plan(self, plan, d):
        return plan.run(d["T_map_prior"].view(self.B, 4, 4), d["radius"], d["image"], d["K_raw"], d["P_cam_pc"], seed=None)

    def _normals(self, plan):
        if self.dataset == "kitti":
            return plan.sample.points.sn          # the crop's normals through the KITTI sample stage, as RawFrameExecutor's
        return plan.sample.sn          # the Oxford and nuScenes models read no normals: the plan's zero buffer

    def _map_pose(self, slot):
        call("di2p_map_pose", ptr(slot.T_map_prior), ptr(slot.P_scan), self.B, ptr(slot.T_map_cam), stream())
        return slot.T_map_cam

    def _extra_outputs(self, slot):          # called behind the launch that writes slot.P_scan
        return dict(T_map_prior=slot.T_map_prior, T_map_cam=self._map_pose(slot))

    def _eval_truth(self, slot):
        prepared = slot.prepared
        slot.mask.copy_(prepared[I_STATUS] == 0)
        return slot.dev["T_map_cam_gt"], prepared[I_P], prepared[I_K], slot.mask

    def _eval_part(self, slot, out):
        """The base evaluation with the pose it measures exchanged: T_map_cam against T_map_cam_gt.  It runs inside the pose solve, before
        the step composes P_scan, so the two compositions are launched here first (and once more by the step: the same bits)."""
        P = out["P"]
        call("di2p_compose_poses", ptr(P), ptr(slot.prepared[sample_prep.I_T_SCAN]), self.B, ptr(slot.P_scan), stream())
        out["P"] = self._map_pose(slot)
        try:
            return super()._eval_part(slot, out)
        finally:
            out["P"] = P
