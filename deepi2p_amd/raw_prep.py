"""Raw frames to network inputs on the device: a Velodyne scan ([n,4] rows x, y, z, intensity) and a camera frame (uint8 HWC) through

  scan_prep     voxel grid 0.1 m -> normals (radius 0.6, max_nn 30) -> intensity of the nearest raw point     (the offline script's record,
                data/kitti/kitti_pc_bin_to_npy_with_downsample_sn.py:50-74)
  sample_prep   SamplePlan.run on that record: 0.3 m voxel pass, down-sample, pose draws, image path          (KittiLoader.__getitem__)

in one call.  RawFramePlan is the fixed-capacity, preallocated form (the style of scan_prep.BatchPlan / sample_prep.SamplePlan): run()
launches everything on the current stream with no allocation and no host synchronisation, so it can be captured in a hipGraph.  The
result equals scan_prep.preprocess_velodyne followed by sample_prep.prepare_samples bit for bit.  This plan is the KITTI raw stage (a
record with normals from one Velodyne scan): other data sets raise ValueError.  The Oxford loader reads offline records without normals;
the raw stage that writes them -- sub-maps from LMS profiles, data/oxford/build_dataset.py -- is deepi2p_amd.submap (SubmapPlan,
OxfordRawPlan).  The nuScenes loader reads no offline record: its __getitem__ reads up to seven raw LiDAR sweeps per sample, cuts the ego car
out of each and accumulates them in the key sweep's frame; that raw stage is deepi2p_amd.sweeps (SweepPlan, NuScenesRawPlan).
"""
import numpy as np
import torch

from . import sample_prep, scan_prep
from ._lib import call, ptr, require_cuda, stream

VOXEL, SN_RADIUS, SN_MAX_NN = 0.1, 0.6, 30          # kitti_pc_bin_to_npy_with_downsample_sn.py


def _check_dataset(dataset):
    if dataset != "kitti":
        raise ValueError("raw_prep: only dataset 'kitti' has a raw-scan stage (the Oxford / nuScenes loaders read offline records without "
                         "normals), got %r" % (dataset,))


class RawFramePlan:
    """plan = RawFramePlan(opt, B, cap_raw, max_frame_points, raw_hw); out = plan.run(points_raw, offsets, images_u8, K_raw, Pc)

    cap_raw: capacity in raw points of the whole batch; max_frame_points: of one frame (a longer frame is rejected: status 1, its
    outputs are zeros, the other frames are unaffected).  normals_method: scan_prep.estimate_normals' method; "query" until the
    cell-cooperative kernel has been measured faster ("Raw-scan preparation")."""

    def __init__(self, opt, B, cap_raw, max_frame_points, raw_hw=None, mode="val", dataset="kitti", normals_method="query", device=None,
                 jitter=sample_prep.JITTER, color=None):
        _check_dataset(dataset)
        self.normals_entry = scan_prep._normals_entry(normals_method)
        if int(max_frame_points) > scan_prep.MAX_FRAME_POINTS:
            raise ValueError("raw_prep: max_frame_points above 2^20")
        dev = device or scan_prep._dev()
        self.B, self.cap, self.max_src = int(B), int(cap_raw), int(max_frame_points)
        c, b = max(self.cap, 1), max(self.B, 1)
        # a voxel has at least one raw point: the record needs no more rows, and no frame more points, than the raw batch
        self.sample = sample_prep.SamplePlan(opt, B, self.cap, self.max_src, raw_hw, mode, dev, jitter=jitter, color=color, dataset=dataset)
        # one workspace for both voxel stages (same B and cap): the 0.1 m stage's state is last read by the 1-NN call, before the 0.3 m pass starts
        self.ws = self.sample.points.ws
        self.v_off = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
        self.v_pts = torch.empty((c, 3), dtype=torch.float32, device=dev)
        self.nn_int = torch.empty((c,), dtype=torch.float32, device=dev)
        self.rec_points = torch.empty((c, 4), dtype=torch.float32, device=dev)          # the record: x, y, z, intensity of the nearest raw point
        self.rec_normals = torch.empty((c, 3), dtype=torch.float32, device=dev)
        self.raw_status = torch.zeros((b,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((b,), dtype=torch.int32, device=dev)

    @property
    def seed(self):
        """i64[1] device: the seed slot of the draws (sample_prep.SamplePlan.seed)"""
        return self.sample.seed

    @property
    def T_scan(self):
        """f64[B,4,4] device: the rigid transform the last run applied to the stored points (the matrix handed to the ragged gather)"""
        return self.sample.table.PrPcn[:self.B]

    def run(self, points_raw, offsets, images_u8, K_raw, Pc, Pji=None, seed=None):
        """points_raw f32[>=total,4], offsets i32[B+1], images u8[B,H0,W0,3], K_raw f64[B,3,3], Pc f64[B,4,4], Pji f64[B,4,4] | None (all
        device; rows past offsets[B] are never read) -> SamplePlan.run's nine tensors + (status i32[B], T_scan f64[B,4,4]), views of the
        plan's buffers.  seed=None leaves the seed slot as it is (graph replays: plan.seed.fill_(s); graph.replay())."""
        require_cuda(points_raw, offsets, images_u8, K_raw, Pc, Pji)
        if points_raw.dim() != 2 or points_raw.shape[1] != 4 or points_raw.dtype != torch.float32 or not points_raw.is_contiguous():
            raise ValueError("raw_prep: points_raw must be a contiguous float32 tensor [total, 4]")
        if tuple(offsets.shape) != (self.B + 1,) or offsets.dtype != torch.int32:
            raise ValueError("raw_prep: offsets must be int32 [%d]" % (self.B + 1))
        B, s = self.B, stream()
        call("di2p_voxel_down_sample", ptr(points_raw), ptr(offsets), B, self.cap, self.max_src, VOXEL, scan_prep.MAX_EXTENT, 0, None,
             ptr(self.v_off), ptr(self.v_pts), None, None, None, ptr(self.raw_status), ptr(self.ws), s)
        call(self.normals_entry, ptr(self.v_off), B, self.cap, SN_RADIUS, SN_MAX_NN, scan_prep.MAX_EXTENT, ptr(self.rec_normals), None, None,
             ptr(self.ws), s)
        call("di2p_nearest_raw", ptr(points_raw), ptr(offsets), ptr(self.v_off), B, self.cap, VOXEL, None, ptr(self.nn_int), None, ptr(self.ws), s)
        torch.cat((self.v_pts, self.nn_int[:, None]), 1, out=self.rec_points)
        out = self.sample.run(self.rec_points, self.rec_normals, self.v_off, images_u8, K_raw, Pc, Pji, seed=seed)
        torch.maximum(self.raw_status, self.sample.status, out=self.status)
        return tuple(out) + (self.status[:B], self.T_scan)


def prepare_raw(scans, images, K_raw, Pc, opt, mode="val", seed=0, Pji=None, device=None, normals_method="query", dataset="kitti"):
    """Convenience: packs the frames, builds a plan, runs it and checks the status (synchronises).  scans: list of [n_b,4] float32
    arrays; images u8[B,H0,W0,3]; K_raw [B,3,3]; Pc [B,4,4] -> RawFramePlan.run's tuple."""
    _check_dataset(dataset)
    scan_prep._normals_entry(normals_method)
    images, raw_hw = sample_prep._host_images(images, len(scans), "raw_prep", "scan")
    sample_prep.option_block(opt, raw_hw, mode)          # argument errors before anything touches the device
    dev = device or scan_prep._dev()
    points, offsets, host = scan_prep.pack(scans, dev)
    B = len(host) - 1
    counts = np.diff(host)
    if counts.max(initial=0) > scan_prep.MAX_FRAME_POINTS:
        raise scan_prep.DeepI2PHipError("raw_prep: a frame has more than 2^20 points")
    plan = RawFramePlan(opt, B, points.shape[0], int(counts.max(initial=1)), raw_hw, mode, dataset, normals_method, dev)
    f64 = sample_prep._f64
    out = plan.run(points, offsets, images.to(dev).contiguous(), f64(K_raw, (B, 3, 3), dev), f64(Pc, (B, 4, 4), dev),
                   None if Pji is None else f64(Pji, (B, 4, 4), dev), seed=seed)
    scan_prep.check_status(plan.status[:B])
    return out
