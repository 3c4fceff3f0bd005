"""Training-sample preparation on the device (csrc/sample_prep.hip, include/deepi2p_hip.h): what KittiLoader.__getitem__
(data/kitti_pc_img_pose_loader.py:289-446) does per sample besides reading files, in `train`, `val` and `val_random_Ry` mode.

  image     top-row crop, x0.5 resize, random / centred crop window, ColorJitter (PIL arithmetic), flip, uint8 HWC -> float32 CHW    :326-349,:120-134,:361-362,:439
  K         camera_matrix_cropping / _scaling for the same window                                                                  kitti_helper.py:193-203
  pose      the random Pr (times P_flip), Pr . P_cam_nwu for the points, the ground-truth P = Pji . Pc . P_nwu_cam . Pr^-1           :136-156,:352-384
  points    scan_prep.BatchPlan (0.3 m voxel pass, random down-sample, node sampling) with the Gaussian jitter fused into its gather :108-118
  scans     multi-scan accumulation: one rigid transform per scan, then the voxel pass merges them                                  :199-282

Every random draw is a pure function of (seed, frame[, index]) on the library's Philox generator.  SamplePlan keeps the seed in DEVICE
memory (plan.seed, i64[1]): a captured graph holds the pointer, not the value, so one capture replays with any seed written into the slot.
The resize supports img_scale 1.0, 0.5 (rounded 2x2 mean on even dimensions) and, for the Oxford / nuScenes data sets, 1/k for odd k >= 3
(see option_block); any other scale raises ValueError.

dataset="oxford" / "nuscenes" (data/oxford_pc_img_pose_loader.py:220-380, data/nuscenes_pc_img_pose_loader.py:273-408) differ from KITTI in:
  image     Oxford removes bottom rows (K untouched), nuScenes top rows; scale 0.5 / 0.2; ColorJitter only when a uniform draw > 0.5; no flip
  points    Oxford: random permutation of the record, then keep x^2 + z^2 < pc_max_range^2 in float32 (di2p_range_shuffle); no normals
            (sn is a zero buffer); 0.2 m voxel pass; the jitter also on the intensity
  pose      Pr = [Rz Ry Rx | t] from all six amplitudes, applied to the cloud in the frame it is stored in; P = P_cam_pc . Pr^-1,
            t_ij = P_cam_pc[:3, 3]; val_random_Ry about y (Oxford) / z (nuScenes)
  scans     nuScenes sweep accumulation: accumulation_transforms_nuscenes + transform_segments
Dataset indexing, the camera-timestamp rejection loop, token look-ups, file reading, P_cam_pc and the sweep poses stay arguments.
"""
import math

import numpy as np
import torch

from . import _lib, scan_prep
from ._lib import call, ptr, require_cuda, stream
from ._ragged import _dev

MODES = {"train": 0, "val": 1, "val_random_Ry": 2}
# the loader fields of kitti/options.py; an option bag without them gets these
DEFAULTS = dict(crop_original_top_rows=50, img_scale=0.5, img_H=160, img_W=512, input_pt_num=20480, node_a_num=128, node_b_num=128,
                P_tx_amplitude=0.0, P_ty_amplitude=0.0, P_tz_amplitude=0.0, P_Rx_amplitude=0.0, P_Ry_amplitude=2.0 * math.pi, P_Rz_amplitude=0.0)
DATASETS = {"kitti": 0, "oxford": 1, "nuscenes": 2}
# the loader fields of oxford/options.py and nuscenes_t/options.py (a field a loader does not have is its neutral value)
DATASET_DEFAULTS = {
    "kitti": DEFAULTS,
    "oxford": dict(crop_original_top_rows=0, crop_original_bottom_rows=0, pc_max_range=50.0, img_scale=0.5, img_H=384, img_W=640,
                   input_pt_num=20480, node_a_num=128, node_b_num=128, P_tx_amplitude=10.0, P_ty_amplitude=5.0, P_tz_amplitude=10.0,
                   P_Rx_amplitude=0.0, P_Ry_amplitude=2.0 * math.pi, P_Rz_amplitude=0.0),
    "nuscenes": dict(crop_original_top_rows=100, crop_original_bottom_rows=0, pc_max_range=0.0, img_scale=0.2, img_H=160, img_W=320,
                     input_pt_num=20480, node_a_num=128, node_b_num=128, P_tx_amplitude=0.0, P_ty_amplitude=0.0, P_tz_amplitude=0.0,
                     P_Rx_amplitude=0.0, P_Ry_amplitude=0.0, P_Rz_amplitude=2.0 * math.pi),
}
RAW_HW = {"kitti": (370, 1226), "oxford": (960, 1280), "nuscenes": (900, 1600)}
VOXEL = {"kitti": 0.3, "oxford": 0.2, "nuscenes": 0.2}
COLOR_RANGES = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))          # brightness, contrast, saturation, hue (augment_img)
JITTER = (0.01, 0.05)                                                     # sigma, clip (augment_pc)


def _get(opt, name, dataset="kitti"):
    return getattr(opt, name, DATASET_DEFAULTS[dataset][name])


def _check_dataset(dataset):
    if dataset not in DATASETS:
        raise ValueError("sample_prep: unknown dataset %r (kitti, oxford, nuscenes)" % (dataset,))


def _resize_k(scale):
    """0 for the scales of the KITTI path (1.0, 0.5), odd k >= 3 for scale 1/k, ValueError otherwise"""
    if scale in (0.5, 1.0):
        return 0
    k = int(round(1.0 / scale)) if 0.0 < scale < 1.0 else 0
    if k < 3 or k % 2 == 0 or abs(1.0 / k - scale) > 1e-12:
        raise ValueError("sample_prep: unsupported img_scale %r: only 1.0, 0.5 (the rounded 2x2 mean) and 1/k for odd k >= 3 (the centre pixel) are "
                         "implemented; any other scale, even k included, has fractional bilinear weights and would have to reproduce OpenCV's "
                         "fixed-point coefficients and intermediate rounding, which cannot be checked here" % (scale,))
    return k


def option_block(opt, raw_hw, mode, color_ranges=COLOR_RANGES, dataset="kitti"):
    """The di2p_sample_opt_t of an option bag for H0 x W0 source images; every argument error is raised here, before any device work.

    dataset "oxford" / "nuscenes": fields the bag lacks come from DATASET_DEFAULTS; the block carries dataset, crop_bottom, resize_k and
    max_range beside the C struct.  Besides 1.0 and 0.5 these data sets take img_scale 1/k for ODD k >= 3 dividing both cropped source
    dimensions; output pixel (y, x) is then the source pixel (k y + (k-1)/2, k x + (k-1)/2).  Derivation: cv2.resize is called with an explicit
    dsize, for which OpenCV uses scale = src / dst = k exactly; the sample coordinate of destination index d is (d + 0.5) k - 0.5, the integer
    k d + (k - 1) / 2 for odd k, so the bilinear weights are exactly (1, 0) and the fixed-point path returns that pixel itself.  OpenCV is
    not available where this was written: the rule is derived from OpenCV's documented coordinate mapping, NOT checked against OpenCV.  Even k
    (half-half weights, OpenCV's intermediate rounding) and every other scale raise ValueError."""
    if mode not in MODES:
        raise ValueError("sample_prep: bad mode %r (train, val, val_random_Ry)" % (mode,))
    _check_dataset(dataset)
    if dataset != "kitti":
        return _option_block_ds(opt, raw_hw, mode, color_ranges, dataset)
    H0, W0 = int(raw_hw[0]), int(raw_hw[1])
    top, scale, H, W = int(_get(opt, "crop_original_top_rows")), float(_get(opt, "img_scale")), int(_get(opt, "img_H")), int(_get(opt, "img_W"))
    if scale not in (0.5, 1.0):
        raise ValueError("sample_prep: unsupported img_scale %r: only 0.5 (the rounded 2x2 mean) and 1.0 are implemented; a general bilinear "
                         "resize would have to reproduce OpenCV's fixed-point coefficients, which cannot be checked here" % (scale,))
    if top < 0 or top >= H0:
        raise ValueError("sample_prep: crop_original_top_rows %d leaves nothing of a %d-row image" % (top, H0))
    if scale == 0.5 and ((H0 - top) % 2 or W0 % 2):
        raise ValueError("sample_prep: odd scaled size: img_scale 0.5 needs even cropped source dimensions, got %d x %d" % (H0 - top, W0))
    Hs, Ws = int(round((H0 - top) * scale)), int(round(W0 * scale))
    if H < 1 or W < 1 or H > Hs or W > Ws:
        raise ValueError("sample_prep: crop window %d x %d larger than the scaled image %d x %d" % (H, W, Hs, Ws))
    o = _lib.SampleOptT()
    o.mode, o.crop_top, o.img_scale, o.img_H, o.img_W, o.Hs, o.Ws = MODES[mode], top, scale, H, W, Hs, Ws
    for k, n in enumerate(("P_tx_amplitude", "P_ty_amplitude", "P_tz_amplitude", "P_Rx_amplitude", "P_Ry_amplitude", "P_Rz_amplitude")):
        o.amplitude[k] = float(_get(opt, n))
    for k, (lo, hi) in enumerate(color_ranges):
        o.color_range[2 * k], o.color_range[2 * k + 1] = float(lo), float(hi)
    return o


def _option_block_ds(opt, raw_hw, mode, color_ranges, dataset):
    H0, W0 = int(raw_hw[0]), int(raw_hw[1])
    g = lambda name: _get(opt, name, dataset)
    top, bottom, scale, H, W = int(g("crop_original_top_rows")), int(g("crop_original_bottom_rows")), float(g("img_scale")), int(g("img_H")), int(g("img_W"))
    if dataset == "oxford":
        top = 0          # the Oxford loader has no top crop
    else:
        bottom = 0       # nor the nuScenes loader a bottom crop
    k = _resize_k(scale)
    if top < 0 or bottom < 0 or top + bottom >= H0:
        raise ValueError("sample_prep: crop_original_top_rows %d / crop_original_bottom_rows %d leave nothing of a %d-row image" % (top, bottom, H0))
    Hc, div = H0 - top - bottom, (k if k else 2 if scale == 0.5 else 1)
    if Hc % div or W0 % div:
        raise ValueError("sample_prep: img_scale 1/%d needs cropped source dimensions it divides, got %d x %d" % (div, Hc, W0))
    Hs, Ws = Hc // div, W0 // div
    if H < 1 or W < 1 or H > Hs or W > Ws:
        raise ValueError("sample_prep: crop window %d x %d larger than the scaled image %d x %d" % (H, W, Hs, Ws))
    o = _lib.SampleOptT()
    o.mode, o.crop_top, o.img_scale, o.img_H, o.img_W, o.Hs, o.Ws = MODES[mode], top, scale, H, W, Hs, Ws
    for i, n in enumerate(("P_tx_amplitude", "P_ty_amplitude", "P_tz_amplitude", "P_Rx_amplitude", "P_Ry_amplitude", "P_Rz_amplitude")):
        o.amplitude[i] = float(g(n))
    for i, (lo, hi) in enumerate(color_ranges):
        o.color_range[2 * i], o.color_range[2 * i + 1] = float(lo), float(hi)
    o.dataset, o.crop_bottom, o.resize_k, o.max_range = DATASETS[dataset], bottom, k, float(g("pc_max_range")) if dataset == "oxford" else 0.0
    return o


def _check_images(images, B, raw_hw):
    if images is None:
        raise ValueError("sample_prep: images is None")
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or tuple(images.shape) != (B, raw_hw[0], raw_hw[1], 3):
        raise ValueError("sample_prep: images must be a uint8 tensor [%d, %d, %d, 3] (HWC)" % (B, raw_hw[0], raw_hw[1]))


def _host_images(images, n, prefix, unit):
    """the images of a convenience call (prepare_raw and its Oxford / nuScenes kin): [B, H0, W0, 3], one per `unit` of the n -> (tensor, raw_hw)"""
    if images is None:
        raise ValueError("%s: images is None" % prefix)
    images = torch.as_tensor(images)
    if images.dim() != 4 or images.shape[0] != n:
        raise ValueError("%s: images must be [B, H0, W0, 3] with one image per %s" % (prefix, unit))
    return images, (images.shape[1], images.shape[2])


def _f64(a, shape, dev):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t.to(dev, torch.float64).reshape(shape).contiguous()


class DrawTable:
    """Device tables of di2p_sample_draws for B frames (tests may fill ints / factors themselves and hand the table to ImagePlan.run)."""

    def __init__(self, B, device=None):
        dev = device or _dev()
        b = max(B, 1)
        self.B = B
        self.ints = torch.zeros((b, 8), dtype=torch.int32, device=dev)          # dx, dy, flip, op0..op3, hue shift
        self.factors = torch.ones((b, 4), dtype=torch.float32, device=dev)      # brightness, contrast, saturation, hue
        self.Pr = torch.zeros((b, 4, 4), dtype=torch.float64, device=dev)
        self.PrPcn = torch.zeros((b, 4, 4), dtype=torch.float64, device=dev)
        self.P = torch.zeros((b, 3, 4), dtype=torch.float32, device=dev)
        self.K = torch.zeros((b, 3, 3), dtype=torch.float32, device=dev)
        self.enable = torch.ones((b,), dtype=torch.int32, device=dev)           # per-frame colour enable (Oxford / nuScenes image path only)
        self.t_ij = torch.zeros((b, 3), dtype=torch.float32, device=dev)        # P_cam_pc[:3, 3] (Oxford / nuScenes draws only)


def sample_draws(optb, K_raw, Pc, Pji=None, seed=0, seed_dev=None, frame0=0, table=None):
    """di2p_sample_draws: K_raw f64[B,3,3], Pc f64[B,4,4], Pji f64[B,4,4] | None (device) -> DrawTable.  No synchronisation."""
    require_cuda(K_raw, Pc, Pji, seed_dev)
    B = K_raw.shape[0]
    table = table or DrawTable(B, K_raw.device)
    call("di2p_sample_draws", int(seed), ptr(seed_dev), B, int(frame0), optb, ptr(K_raw), ptr(Pc), ptr(Pji), ptr(table.ints), ptr(table.factors),
         ptr(table.Pr), ptr(table.PrPcn), ptr(table.P), ptr(table.K), stream())
    return table


def sample_draws_ds(optb, K_raw, P_cam_pc, seed=0, seed_dev=None, frame0=0, table=None):
    """di2p_sample_draws_ds for an Oxford / nuScenes option block: K_raw f64[B,3,3], P_cam_pc f64[B,4,4] (device) -> DrawTable with ints
    (no flip), factors, enable, Pr, PrPcn (the SAME tensor as Pr: the point kernels apply Pr itself), P, K and t_ij.  No synchronisation."""
    require_cuda(K_raw, P_cam_pc, seed_dev)
    if not optb.dataset:
        raise ValueError("sample_prep: sample_draws_ds needs an option block of dataset oxford or nuscenes")
    B = K_raw.shape[0]
    table = table or DrawTable(B, K_raw.device)
    table.PrPcn = table.Pr
    call("di2p_sample_draws_ds", int(seed), ptr(seed_dev), B, int(frame0), optb, optb.dataset, ptr(K_raw), ptr(P_cam_pc), ptr(table.ints),
         ptr(table.factors), ptr(table.enable), ptr(table.Pr), ptr(table.P), ptr(table.K), ptr(table.t_ij), stream())
    return table


class ImagePlan:
    """The image half, preallocated: run() is three launches, no allocation, no synchronisation."""

    def __init__(self, opt, B, raw_hw=(370, 1226), mode="train", device=None, geometry=True, color=None, dataset="kitti"):
        """dataset "oxford" / "nuscenes": bottom / top crop, the block's resize rule, no flip, and the colour chain only on the frames whose
        table.enable is non-zero (a DrawTable starts with every frame enabled)."""
        _check_dataset(dataset)
        dev = device or _dev()
        self.optb = opt if isinstance(opt, _lib.SampleOptT) else option_block(opt, raw_hw, mode, dataset=dataset)
        if self.optb.dataset != DATASETS[dataset]:
            raise ValueError("sample_prep: the option block was made for another data set than %r" % (dataset,))
        if self.optb.dataset and not geometry:
            raise ValueError("sample_prep: geometry=False is a KITTI-path option")
        self.B, self.raw_hw = B, (int(raw_hw[0]), int(raw_hw[1]))
        self.geometry = bool(geometry)
        self.color = (self.optb.mode == 0) if color is None else bool(color)          # validation: geometry only
        self.ws = torch.zeros((_lib.load().di2p_image_prepare_workspace_bytes(B) // 4,), dtype=torch.int32, device=dev)
        self.img = torch.empty((B, 3, self.optb.img_H, self.optb.img_W), dtype=torch.float32, device=dev)

    def run(self, images_u8, table, reduce_blocks=0):
        _check_images(images_u8, self.B, self.raw_hw)
        require_cuda(images_u8)
        if self.optb.dataset:
            call("di2p_image_prepare_ds", ptr(images_u8), self.B, self.raw_hw[0], self.raw_hw[1], self.optb, self.optb.crop_bottom, self.optb.resize_k,
                 ptr(table.ints), ptr(table.factors), ptr(table.enable), int(self.color), int(reduce_blocks), ptr(self.img), ptr(self.ws), stream())
            return self.img
        call("di2p_image_prepare", ptr(images_u8), self.B, self.raw_hw[0], self.raw_hw[1], self.optb, ptr(table.ints), ptr(table.factors),
             int(self.geometry), int(self.color), int(reduce_blocks), ptr(self.img), ptr(self.ws), stream())
        return self.img

    def grey_sums(self):
        """i64[B]: the grey sums the contrast operation of the last run used (synchronises)"""
        return self.ws[:self.B].cpu().numpy().astype(np.int64) & 0xFFFFFFFF


# SamplePlan.run's nine tensors in order, then the two a raw plan's run (raw_prep.RawFramePlan, sweeps.NuScenesRawPlan) appends; the positions
# the executors of raw_pipeline read by name
PREPARED = ("pc", "intensity", "sn", "node_a", "node_b", "P", "img", "K", "t_ji", "status", "T_scan")
I_P, I_K, I_STATUS, I_T_SCAN = (PREPARED.index(k) for k in ("P", "K", "status", "T_scan"))


class SamplePlan:
    """scan_prep.BatchPlan + draws + image path, preallocated.  run() launches everything on the current stream with no host
    synchronisation and no allocation (torch.cuda.graph-safe); plan.status (i32[B]) stays on the device (scan_prep.check_status).

    The seed lives in plan.seed (i64[1], device).  run(seed=s) writes s there first (a fill launch); run(seed=None) leaves the slot alone,
    which is how a captured graph is replayed with other seeds: plan.seed.fill_(s); graph.replay()."""

    def __init__(self, opt, B, cap, max_frame_points, raw_hw=None, mode="train", device=None, jitter=JITTER, color=None, dataset="kitti"):
        """dataset "oxford" / "nuscenes": range filter + shuffle (Oxford) -> 0.2 m voxel pass and ragged choice -> gather with the jitter on
        coordinates and intensity -> node sampling; run() takes normals=None and P_cam_pc where KITTI takes Pc, and no Pji; sn is a zero
        buffer written here once and never again."""
        _check_dataset(dataset)
        dev = device or _dev()
        raw_hw = RAW_HW[dataset] if raw_hw is None else raw_hw
        self.optb = option_block(opt, raw_hw, mode, dataset=dataset)
        if int(_get(opt, "node_a_num", dataset)) != int(_get(opt, "node_b_num", dataset)):
            raise ValueError("sample_prep: node_a_num != node_b_num is not supported by scan_prep.BatchPlan")
        if int(max_frame_points) > scan_prep.MAX_FRAME_POINTS:
            raise ValueError("sample_prep: max_frame_points above 2^20")
        self.B, self.mode, self.dataset = B, mode, dataset
        n, nodes = int(_get(opt, "input_pt_num", dataset)), int(_get(opt, "node_a_num", dataset))
        self.points = scan_prep.BatchPlan(B, cap, max_frame_points, n, nodes, voxel=VOXEL[dataset], device=dev, normals=dataset == "kitti")
        self.image = ImagePlan(self.optb, B, raw_hw, mode, dev, color=color, dataset=dataset)
        self.sn = torch.zeros((B, 3, n), dtype=torch.float32, device=dev) if dataset != "kitti" else None
        self.filtered = None
        if dataset == "oxford":          # (points f32[cap,4], offsets i32[B+1], status i32[B]) of the filter; the workspace is the voxel pass's
            self.filtered = (torch.zeros((max(int(cap), 1), 4), dtype=torch.float32, device=dev), torch.zeros((B + 1,), dtype=torch.int32, device=dev),
                             torch.zeros((max(B, 1),), dtype=torch.int32, device=dev))
        self.table = DrawTable(B, dev)
        self.jitter = tuple(jitter) if (mode == "train" and jitter is not None and jitter[0] > 0) else None
        self.seed = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.t_ji = torch.zeros((max(B, 1), 3), dtype=torch.float32, device=dev)
        self.status = self.points.status if self.filtered is None else torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)

    def _run_ds(self, points, normals, offsets, images_u8, K_raw, P_cam_pc, Pji):
        if normals is not None:
            raise ValueError("sample_prep: the %s records have no normals: pass normals=None (sn is returned as zeros)" % self.dataset)
        if Pji is not None:
            raise ValueError("sample_prep: Pji is a KITTI argument; the %s ground truth is P_cam_pc . Pr^-1" % self.dataset)
        require_cuda(points, offsets, images_u8, K_raw, P_cam_pc)
        sample_draws_ds(self.optb, K_raw, P_cam_pc, seed_dev=self.seed, table=self.table)
        if self.filtered is not None:
            points, offsets, fstat = scan_prep.range_shuffle(points, offsets, self.optb.max_range, seed_dev=self.seed, max_frame_points=self.points.max_src,
                                                             cap=self.points.cap, out=self.filtered, ws=self.points.ws)
        pc, intensity, _, node_a, node_b = self.points.run(points, None, offsets, 0, self.table.Pr, seed_dev=self.seed, jitter=self.jitter,
                                                           jitter_intensity=self.jitter is not None)
        if self.filtered is not None:          # a frame the filter rejected looks empty (and fine) to the voxel pass: keep the worse status
            torch.maximum(self.points.status, fstat, out=self.status)
        img = self.image.run(images_u8, self.table)
        B = self.B
        return pc, intensity, self.sn, node_a, node_b, self.table.P[:B], img, self.table.K[:B], self.table.t_ij[:B]          # PREPARED[:9]

    def run(self, points, normals, offsets, images_u8, K_raw, Pc, Pji=None, seed=None):
        """points f32[>=total,4], normals f32[>=total,3], offsets i32[B+1], images u8[B,H0,W0,3], K_raw f64[B,3,3], Pc f64[B,4,4] (camera
        calibration x Tr), Pji f64[B,4,4] | None (all device) -> (pc f32[B,3,N], intensity f32[B,1,N], sn f32[B,3,N], node_a, node_b
        f32[B,3,M], P f32[B,3,4], img f32[B,3,H,W], K f32[B,3,3], t_ji f32[B,3]): __getitem__'s nine, batched, views of the plan's buffers."""
        _check_images(images_u8, self.B, self.image.raw_hw)
        if self.dataset != "kitti" and (normals is not None or Pji is not None):
            return self._run_ds(points, normals, offsets, images_u8, K_raw, Pc, Pji)          # raises
        require_cuda(points, normals, offsets, images_u8, K_raw, Pc, Pji)
        if seed is not None:
            self.seed.fill_(int(seed))
        if self.dataset != "kitti":
            return self._run_ds(points, None, offsets, images_u8, K_raw, Pc, None)
        sample_draws(self.optb, K_raw, Pc, Pji, seed_dev=self.seed, table=self.table)
        pc, intensity, sn, node_a, node_b = self.points.run(points, normals, offsets, 0, self.table.PrPcn, seed_dev=self.seed, jitter=self.jitter)
        img = self.image.run(images_u8, self.table)
        if Pji is not None:
            self.t_ji.copy_(Pji[:, :3, 3])
        B = self.B
        return pc, intensity, sn, node_a, node_b, self.table.P[:B], img, self.table.K[:B], self.t_ji[:B]          # PREPARED[:9]


def prepare_images(images_u8, K_raw, opt, mode="val", seed=0, dataset="kitti"):
    """The image half alone (RegistrationExecutor users): images u8[B,H0,W0,3] (numpy or tensor), K_raw [B,3,3] ->
    (img f32[B,3,img_H,img_W], K f32[B,3,3]) on the device."""
    if images_u8 is None:
        raise ValueError("sample_prep: images is None")
    images = torch.as_tensor(images_u8)
    if images.dim() != 4:
        raise ValueError("sample_prep: images must be [B, H0, W0, 3]")
    B, raw_hw = images.shape[0], (images.shape[1], images.shape[2])
    optb = option_block(opt, raw_hw, mode, dataset=dataset)
    _check_images(images, B, raw_hw)
    dev = images.device if images.is_cuda else _dev()
    images = images.to(dev).contiguous()
    eye = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1)
    if dataset == "kitti":
        table = sample_draws(optb, _f64(K_raw, (B, 3, 3), dev), eye, None, seed=seed)
    else:
        table = sample_draws_ds(optb, _f64(K_raw, (B, 3, 3), dev), eye, seed=seed)
    plan = ImagePlan(optb, B, raw_hw, mode, dev, dataset=dataset)
    return plan.run(images, table), table.K[:B]


def accumulation_transforms(poses, Pc):
    """poses: per frame a list of 4x4 world poses, the frame's own scan first; Pc: per-frame 4x4 -> per frame f64[S_b,4,4]:
    Pc^-1 . (P_oi^-1 . P_oj) . Pc (identity for the frame's own scan).  fp64 host arithmetic on the arguments (the reference computes it on
    float32 poses cast from disk; take the file's values in fp64 to reproduce a result to about 1e-7 relative)."""
    out = []
    for ps, pc in zip(poses, Pc):
        pc = np.asarray(pc, dtype=np.float64)
        pci, pio = np.linalg.inv(pc), np.linalg.inv(np.asarray(ps[0], dtype=np.float64))
        out.append(np.stack([np.eye(4) if j == 0 else np.dot(pci, np.dot(np.dot(pio, np.asarray(p, dtype=np.float64)), pc)) for j, p in enumerate(ps)]))
    return out


def accumulation_transforms_nuscenes(P_oi, P_oj, P_vehicle_lidar):
    """lidar_frame_accumulation (data/nuscenes_pc_img_pose_loader.py:227-229): P_vehicle_lidar^-1 . (P_oi^-1 . P_oj) . P_vehicle_lidar, the
    transform that moves sweep j into the LiDAR frame of sweep i.  P_oi, P_vehicle_lidar 4x4; P_oj 4x4 or [S,4,4] -> f64 of P_oj's shape.
    Feed the result to transform_segments (identity for the frame's own sweep).  fp64 host arithmetic, as accumulation_transforms."""
    P_oj = np.asarray(P_oj, dtype=np.float64)
    vl = np.asarray(P_vehicle_lidar, dtype=np.float64)
    lv, io = np.linalg.inv(vl), np.linalg.inv(np.asarray(P_oi, dtype=np.float64))
    out = np.stack([np.dot(np.dot(lv, np.dot(io, p)), vl) for p in P_oj.reshape(-1, 4, 4)])
    return out.reshape(P_oj.shape)


def accumulate(scans_per_frame, poses, Pc, device=None):
    """Multi-scan accumulation (get_accumulated_pc): scans_per_frame: per frame a list of f32[7, n] records, the frame's own first, then the
    previous / next scans; poses: their 4x4 world poses; Pc: per-frame 4x4.  Every scan is moved into its frame's Velodyne frame on the
    device (di2p_transform_segments).  -> (points f32[total,4], normals f32[total,3], seg_offsets i32[S+1], frame_offsets i32[B+1]); the
    frame offsets are what SamplePlan.run / scan_prep take, whose 0.3 m voxel pass then merges the scans."""
    dev = device or _dev()
    flat = [r for f in scans_per_frame for r in f]
    points, normals, seg_off, host = scan_prep.pack_records(flat, dev)
    T = np.concatenate(accumulation_transforms(poses, Pc), 0) if flat else np.zeros((0, 4, 4))
    counts = np.cumsum([0] + [len(f) for f in scans_per_frame])
    frame_off = torch.tensor([host[c] for c in counts], dtype=torch.int32, device=dev)
    transform_segments(points, normals, seg_off, _f64(T, (-1, 4, 4), dev), total=host[-1])
    return points, normals, seg_off, frame_off


def transform_segments(points, normals, seg_offsets, transforms, total=None, out=None):
    """In place (out=None) or into out = (points_out, normals_out)."""
    require_cuda(points, normals, seg_offsets, transforms)
    S = seg_offsets.shape[0] - 1
    total = int(points.shape[0]) if total is None else int(total)
    po, no = (points, normals) if out is None else out
    call("di2p_transform_segments", ptr(points), ptr(normals), ptr(seg_offsets), ptr(transforms), S, total, ptr(po), ptr(no), stream())
    return po, no


def prepare_samples(records, images, K_raw, Pc, opt, mode="train", seed=0, Pji=None, device=None, offsets=None, dataset="kitti"):
    """Convenience: packs, plans, runs, checks the status (synchronises).  records: list of f32[7, n] records, or with `offsets`
    the (points, normals) pair of accumulate() and its frame offsets.  -> SamplePlan.run's nine tensors.
    dataset "oxford" / "nuscenes": records are f32[4, n] (x, y, z, intensity; with `offsets` the pair (points f32[total,4], None)), Pc is
    P_cam_pc, Pji is not accepted."""
    _check_dataset(dataset)
    if dataset != "kitti":
        return _prepare_samples_ds(records, images, K_raw, Pc, opt, mode, seed, Pji, device, offsets, dataset)
    if images is None:
        raise ValueError("sample_prep: images is None")
    images = torch.as_tensor(images)
    if images.dim() != 4:
        raise ValueError("sample_prep: images must be [B, H0, W0, 3]")
    raw_hw = (images.shape[1], images.shape[2])
    option_block(opt, raw_hw, mode)          # argument errors before anything touches the device
    dev = device or _dev()
    if offsets is None:
        points, normals, offsets, host = scan_prep.pack_records(records, dev)
    else:
        points, normals = records
        host = offsets.cpu().tolist()
    B = len(host) - 1
    plan = SamplePlan(opt, B, points.shape[0], int(np.diff(host).max(initial=1)), raw_hw, mode, dev)
    out = plan.run(points, normals, offsets, images.to(dev).contiguous(), _f64(K_raw, (B, 3, 3), dev), _f64(Pc, (B, 4, 4), dev),
                   None if Pji is None else _f64(Pji, (B, 4, 4), dev), seed=seed)
    scan_prep.check_status(plan.status[:B])
    return out


def _prepare_samples_ds(records, images, K_raw, P_cam_pc, opt, mode, seed, Pji, device, offsets, dataset):
    if images is None:
        raise ValueError("sample_prep: images is None")
    if Pji is not None:
        raise ValueError("sample_prep: Pji is a KITTI argument; the %s ground truth is P_cam_pc . Pr^-1" % dataset)
    images = torch.as_tensor(images)
    if images.dim() != 4:
        raise ValueError("sample_prep: images must be [B, H0, W0, 3]")
    raw_hw = (images.shape[1], images.shape[2])
    option_block(opt, raw_hw, mode, dataset=dataset)          # argument errors before anything touches the device
    if offsets is None:
        if any(np.ndim(r) != 2 or r.shape[0] != 4 for r in records):
            raise ValueError("sample_prep: %s records are f32[4, n] (x, y, z, intensity): they have no normals" % dataset)
        dev = device or _dev()
        points, offsets, host = scan_prep.pack([torch.as_tensor(r).t() for r in records], dev)
    else:
        points, normals = records
        if normals is not None:
            raise ValueError("sample_prep: the %s records have no normals: pass (points, None)" % dataset)
        dev = device or _dev()
        host = offsets.cpu().tolist()
    B = len(host) - 1
    plan = SamplePlan(opt, B, points.shape[0], int(np.diff(host).max(initial=1)), raw_hw, mode, dev, dataset=dataset)
    out = plan.run(points, None, offsets, images.to(dev).contiguous(), _f64(K_raw, (B, 3, 3), dev), _f64(P_cam_pc, (B, 4, 4), dev), seed=seed)
    scan_prep.check_status(plan.status[:B])
    return out
