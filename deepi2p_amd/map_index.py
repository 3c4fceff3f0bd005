"""Map localisation, the front of it (csrc/map_index.hip, include/deepi2p_hip.h): a LiDAR map that stays on the device, a uniform cell index
over it, and the crop of one disc per camera frame around a rough pose prior (GPS and a compass, or the last frame's pose).

  MapIndex.build   once per map, eager      cell of every row -> stable sort -> cell_start, order, sorted             di2p_map_index_build
  estimate_normals once per map, eager      3-D cell keys -> stable sort -> radius-bounded kNN -> PCA normal of every row  di2p_map_normals
  MapIndex.crop    per batch, allocating    frame -> window cells -> rows inside the disc, in the prior frame         di2p_map_crop
  CropPlan         per batch, graph-safe    the same, preallocated: the priors and radii are read from device memory;
                                            want_normals: the map's normals of the kept rows, R^T n, behind the crop     di2p_map_crop_normals
  MapRawPlan       CropPlan + sample_prep.SamplePlan(dataset="oxford" | "nuscenes" | "kitti"): priors and camera frames to the loader's sample
  map_pose         T_map_cam = T_map_prior . P_scan^-1                                                                di2p_map_pose

The map is f32[M,4] rows (x, y, z, intensity) in a map frame.  Coordinates are float32: the caller keeps them small, relative to a map origin
of its own (at 10 km from that origin a float32 coordinate resolves 1 mm).  up_axis names the vertical axis, the ground axes (a, b) are the
other two in ascending order: camera-convention maps (y down, the Oxford record) have up_axis=1 and the ground plane x-z; z-up maps
(nuScenes, ENU) up_axis=2.  T_map_prior f64[B,4,4] maps prior-frame coordinates into the map; a frame keeps the rows with
dx^2 + dy^2 < radius^2 on the ground plane around the prior's translation (strict, as the Oxford loader's range filter) and gets them in the
PRIOR frame, R^T (p - t).  The arithmetic is fp64 with every operation rounded once, so the tests restate it in numpy bit for bit.

The KITTI model reads surface normals (`sn`), so a map it is to be localised in carries one normal per row: MapIndex.build(..., normals=...)
takes the user's own f32[M,3] (Open3D's, computed offline) or computes them with estimate_normals -- scan_prep.estimate_normals' rule (the
at most max_nn nearest rows inside `radius`, PCA, oriented along orient . e_up_axis) on the whole map as one cloud.  Normals are computed
once per map, as the index is; a step gathers 12 more bytes per kept row.  A raw, unthinned map can hold its 30 nearest rows within 0.6 m in
a very small patch: thin the map first (a voxel pass), as the KITTI records are.

status per frame: 0 ok, 1 more than max_frame_points kept rows (or more than the capacity, or a window of more than max_cells cells), 2 (voxel
pass of the sample stage) bounding box above its limit, 4 no kept row (also a disc off the map), 5 a non-finite prior or a radius that is not
finite and positive.  A frame with a status has no rows and leaves the others as they are without it.
"""
import numpy as np
import torch

from . import _lib, _ragged, sample_prep, scan_prep
from ._lib import DeepI2PHipError, call, ptr, require_cuda, stream
from ._ragged import _dev

MAX_FRAME_POINTS = scan_prep.MAX_FRAME_POINTS
MAX_ROWS, MAX_CELLS = 1 << 27, 1 << 24
RIGID_TOL = 1e-6          # largest |R^T R - I| entry a prior checked on the host may have
NORMALS_RADIUS, NORMALS_MAX_NN, NORMALS_NN_LIMIT = 0.6, 30, 64          # the offline KITTI script's radius and max_nn; the kernel's limit
_NORMALS_STATUS = {1: "the map has a non-finite coordinate", 2: "an edge of the map's bounds is above radius * (2^21 - 4)"}
_STATUS = dict(scan_prep._STATUS)
_STATUS.update({1: "more than max_frame_points kept rows, more than the capacity, or a window of more than max_cells cells",
                4: "no map row inside the disc", 5: "non-finite prior, or a radius that is not finite and positive"})


def check_status(status):
    """Raise DeepI2PHipError for a rejected frame (synchronises)."""
    _ragged.check_status("map_index", "frame", _STATUS, status)


def ground_axes(up_axis):
    if up_axis not in (0, 1, 2):
        raise ValueError("map_index: up_axis must be 0, 1 or 2 (the vertical axis of the map frame)")
    return [k for k in range(3) if k != up_axis]


def _check_cell(cell):
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError("map_index: cell must be a finite number > 0 (metres)")
    return cell


def _check_grid(nx, ny):
    nx, ny = int(nx), int(ny)
    if nx < 1 or ny < 1 or nx * ny > MAX_CELLS:
        raise ValueError("map_index: the grid must have nx, ny >= 1 and nx * ny <= 2^24 cells, got %d x %d (a larger cell?)" % (nx, ny))
    return nx, ny


def _check_points(points):
    """host array or tensor -> float32 tensor [M,4] with 1 <= M <= 2^27 (ValueError otherwise)"""
    if not torch.is_tensor(points):
        arr = np.asarray(points)
        if arr.dtype != np.float32:
            raise ValueError("map_index: points must be float32 [M, 4] (x, y, z, intensity), got %s" % arr.dtype)
        points = torch.from_numpy(np.ascontiguousarray(arr))
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4:
        raise ValueError("map_index: points must be float32 [M, 4] (x, y, z, intensity), got %s %s" % (points.dtype, list(points.shape)))
    M = int(points.shape[0])
    if M < 1 or M > MAX_ROWS:
        raise ValueError("map_index: a map has 1 to 2^27 rows, got %d" % M)
    return points


def _check_normals_args(radius, max_nn, up_axis, orient):
    ground_axes(up_axis)
    radius = float(radius)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError("map_index: the normals' radius must be a finite number > 0 (metres)")
    if int(max_nn) != max_nn or not 1 <= int(max_nn) <= NORMALS_NN_LIMIT:
        raise ValueError("map_index: the normals' max_nn must be an integer in [1, %d], got %r" % (NORMALS_NN_LIMIT, max_nn))
    if orient not in (1, -1):
        raise ValueError("map_index: orient must be +1 or -1 (the sign of the up axis the normals point along), got %r" % (orient,))
    return radius, int(max_nn), int(up_axis), int(orient)


def _check_normals(normals, M):
    """the user's own normals -> float32 tensor [M,3], as given (ValueError for another dtype or shape)"""
    t = normals if torch.is_tensor(normals) else None
    if t is None:
        arr = np.asarray(normals)
        if arr.dtype != np.float32:
            raise ValueError("map_index: normals must be float32 [%d, 3] (one per map row), got %s" % (M, arr.dtype))
        t = torch.from_numpy(np.ascontiguousarray(arr))
    if t.dtype != torch.float32 or tuple(t.shape) != (M, 3):
        raise ValueError("map_index: normals must be float32 [%d, 3] (one per map row), got %s %s" % (M, t.dtype, list(t.shape)))
    return t


def estimate_normals(points, radius=NORMALS_RADIUS, max_nn=NORMALS_MAX_NN, up_axis=2, orient=1, want_neighbors=False, device=None):
    """points f32[M,4] (host array or tensor, any device) -> normals f32[M,3] on `device`, row i the normal of row i (+ nn_count i32[M] and
    nn_idx i32[M,max_nn], -1 past the count, with want_neighbors).  scan_prep.estimate_normals' rule on the map as one cloud: the at most max_nn
    rows inside `radius` in ascending (d2, row), the row itself included; the eigenvector of the smallest eigenvalue of their covariance,
    flipped so that orient * n[up_axis] >= 0; orient * e_up_axis below 3 neighbours.  orient=-1 for camera-convention maps (up is -y).
    ValueError for bad arguments before anything touches the device; DeepI2PHipError for a non-finite coordinate or bounds above
    radius * (2^21 - 4) (one synchronisation)."""
    points = _check_points(points)
    radius, max_nn, up_axis, orient = _check_normals_args(radius, max_nn, up_axis, orient)
    M = int(points.shape[0])
    dev = device or (points.device if points.is_cuda else _dev())
    pts = points.to(dev).contiguous()
    normals = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros((M,), dtype=torch.int32, device=dev) if want_neighbors else None
    idx = torch.zeros((M, max_nn), dtype=torch.int32, device=dev) if want_neighbors else None
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(256, int(_lib.load().di2p_map_normals_workspace_bytes(M))),), dtype=torch.uint8, device=dev)
    require_cuda(pts)
    call("di2p_map_normals", ptr(pts), M, up_axis, orient, radius, max_nn, ptr(normals), ptr(cnt), ptr(idx), ptr(status), ptr(ws), stream())
    st = int(status.item())
    if st != 0:
        raise DeepI2PHipError("map_index: estimate_normals: %s" % _NORMALS_STATUS.get(st, "status %d" % st))
    return (normals, cnt, idx) if want_neighbors else normals


def check_priors(T_map_prior, B=None, name="T_map_prior", prefix="map_index"):
    """host priors [B,4,4] -> f64 array; ValueError for a wrong shape or a finite prior whose rotation block is further than RIGID_TOL from
    orthonormal.  A prior with a non-finite entry passes: the device gives its frame status 5."""
    T = np.asarray(T_map_prior.numpy() if torch.is_tensor(T_map_prior) else T_map_prior)
    if T.dtype.kind != "f" or T.ndim != 3 or T.shape[1:] != (4, 4) or (B is not None and T.shape[0] != B):
        raise ValueError("%s: %s must be a floating-point array [%s, 4, 4], got %s %s" % (prefix, name, "B" if B is None else B, T.dtype, list(T.shape)))
    T = np.ascontiguousarray(T, dtype=np.float64)
    for b in range(T.shape[0]):
        if np.isfinite(T[b]).all():
            R = T[b, :3, :3]
            if np.abs(R.T @ R - np.eye(3)).max() > RIGID_TOL or np.abs(T[b, 3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > RIGID_TOL:
                raise ValueError("%s: %s[%d] is not a rigid transform (|R^T R - I| or its last row off by more than %g)" % (prefix, name, b, RIGID_TOL))
    return T


def check_radius(radius, B, prefix="map_index"):
    """host radius, a scalar or [B] -> f64[B]; its values are checked on the device (status 5)"""
    r = np.asarray(radius.numpy() if torch.is_tensor(radius) else radius)
    if r.dtype.kind not in "fiu" or r.shape not in ((), (B,)):
        raise ValueError("%s: radius must be a number or a numeric array [%d], got %s %s" % (prefix, B, r.dtype, list(r.shape)))
    return np.broadcast_to(r.astype(np.float64), (B,)).copy()


def _checked_priors(T_map_prior, radius, B):
    """(T f64[B,4,4], r f64[B]) tensors: device tensors are taken as they are (shape and dtype only), host values are checked and stay on the
    host"""
    if torch.is_tensor(T_map_prior) and T_map_prior.is_cuda:
        T = _ragged._check_tensor("map_index", T_map_prior, "T_map_prior", torch.float64, ("B" if B is None else B, 4, 4))
    else:
        T = torch.from_numpy(check_priors(T_map_prior, B))
    B = int(T.shape[0])
    if torch.is_tensor(radius) and radius.is_cuda:
        r = _ragged._check_tensor("map_index", radius, "radius", torch.float64, (B,))
    else:
        r = torch.from_numpy(check_radius(radius, B))
    return T, r


def max_window_cells(index, max_radius):
    """the window cells a disc of at most max_radius can touch: per axis floor(2 r / cell) + 2, at most the grid's"""
    r = float(max_radius)
    if not (r > 0.0 and np.isfinite(r)):
        raise ValueError("map_index: max_radius must be a finite number > 0")
    per_axis = int(np.floor(2.0 * r / index.cell)) + 2
    return max(1, min(per_axis, index.nx) * min(per_axis, index.ny))


class MapIndex:
    """The resident map: sorted f32[M,4] (the rows cell after cell, inside a cell in map-row order), cell_start i32[nx ny + 1], order i32[M]
    (the map row of every stored row), and the grid (origin, cell, nx, ny, up_axis); normals f32[M,3] | None in MAP-ROW order (row i belongs
    to row i of the points given to build: what the crop's `index` output addresses).  Built by MapIndex.build; never modified afterwards."""

    def __init__(self, sorted_rows, cell_start, order, origin, cell, nx, ny, up_axis, normals=None):
        self.sorted, self.cell_start, self.order, self.normals = sorted_rows, cell_start, order, normals
        self.origin, self.cell, self.nx, self.ny, self.up_axis = (float(origin[0]), float(origin[1])), float(cell), int(nx), int(ny), int(up_axis)
        self.M, self.device = int(order.shape[0]), sorted_rows.device

    def _grid_args(self):
        return (self.M, self.up_axis, self.origin[0], self.origin[1], self.cell, self.nx, self.ny)

    @staticmethod
    def build(points, cell=8.0, up_axis=1, origin=None, device=None, shape=None, normals=None):
        """points f32[M,4] (host array or tensor, any device) -> MapIndex on `device`.  origin=None: origin = floor(min / cell) cell on the
        two ground axes and (nx, ny) from the map's own extent; with an origin, shape=(nx, ny) or again the extent.  Raises ValueError for bad
        arguments before anything touches the device, DeepI2PHipError for a non-finite coordinate or a row outside the grid (one
        synchronisation).  normals: None (index.normals is None: the Oxford and nuScenes models); a float32 [M,3] array or tensor, the
        user's own normals, stored as given; or True / a dict of radius, max_nn, orient: estimate_normals on the points (orient defaults
        to -1 for up_axis=1, camera-convention maps, else +1).  The KITTI model needs them."""
        a, b = ground_axes(up_axis)
        cell = _check_cell(cell)
        points = _check_points(points)
        M = int(points.shape[0])
        own, estimate = None, None
        if normals is True or isinstance(normals, dict):
            estimate = {} if normals is True else dict(normals)
            unknown = set(estimate) - {"radius", "max_nn", "orient"}
            if unknown:
                raise ValueError("map_index: normals=dict(...) takes radius, max_nn and orient, got %s" % sorted(unknown))
            estimate = _check_normals_args(estimate.get("radius", NORMALS_RADIUS), estimate.get("max_nn", NORMALS_MAX_NN), up_axis,
                                           estimate.get("orient", -1 if up_axis == 1 else 1))
        elif normals is not None and normals is not False:
            own = _check_normals(normals, M)
        if origin is not None:
            origin = np.asarray(origin, dtype=np.float64)
            if origin.shape != (2,) or not np.isfinite(origin).all():
                raise ValueError("map_index: origin must be two finite numbers (the grid's corner on the ground axes)")
        if shape is not None:
            if origin is None:
                raise ValueError("map_index: shape=(nx, ny) goes with an origin")
            shape = _check_grid(*shape)
        if origin is None or shape is None:
            ground = points[:, [a, b]].double()
            lo, hi = ground.min(dim=0).values.cpu().numpy(), ground.max(dim=0).values.cpu().numpy()
            if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                raise DeepI2PHipError("map_index: the map has a non-finite coordinate")
            if origin is None:
                origin = np.floor(lo / cell) * cell
            n = np.floor((hi - origin) / cell) + 1
            shape = _check_grid(*np.clip(n, 1, 2.0 ** 31 - 1).astype(np.int64))
        nx, ny = shape
        dev = device or (points.device if points.is_cuda else _dev())
        pts = points.to(dev).contiguous()
        cell_start = torch.zeros((nx * ny + 1,), dtype=torch.int32, device=dev)
        order = torch.zeros((M,), dtype=torch.int32, device=dev)
        sorted_rows = torch.zeros((M, 4), dtype=torch.float32, device=dev)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        ws = _ragged.workspace("di2p_map_index_workspace_bytes", M, nx * ny, dev)
        require_cuda(pts)
        call("di2p_map_index_build", ptr(pts), M, int(up_axis), float(origin[0]), float(origin[1]), cell, nx, ny, ptr(cell_start), ptr(order),
             ptr(sorted_rows), ptr(status), ptr(ws), stream())
        if int(status.item()) != 0:
            raise DeepI2PHipError("map_index: the map has a non-finite coordinate or a row outside the %d x %d grid at origin (%g, %g)"
                                  % (nx, ny, origin[0], origin[1]))
        if estimate is not None:
            own = estimate_normals(pts, estimate[0], estimate[1], estimate[2], estimate[3], device=dev)
        elif own is not None:
            own = own.to(dev).contiguous()
        return MapIndex(sorted_rows, cell_start, order, origin, cell, nx, ny, up_axis, own)

    def crop(self, T_map_prior, radius, max_frame_points, cap=None, want_index=False, max_cells=None, want_normals=False):
        """Eager: T_map_prior [B,4,4], radius a number or [B] (host values, checked here; or f64 device tensors, checked on the device) ->
        (rows f32[cap,4] in each frame's prior frame, offsets i32[B+1], status i32[B][, index i32[cap]: the map row of every kept row]).
        cap: rows of the whole batch (default B * max_frame_points); max_cells: window cells per frame the workspace is sized for (default:
        the whole grid).  want_normals appends normals f32[cap,3], the map's normals of the kept rows in the prior frame (R^T n; the index
        must carry normals).  No synchronisation."""
        mfp = _ragged._check_max_frame_points("map_index", max_frame_points)
        T, r = _checked_priors(T_map_prior, radius, None)
        B = int(T.shape[0])
        cap = B * mfp if cap is None else int(cap)
        max_cells = self.nx * self.ny if max_cells is None else int(max_cells)
        if cap < 0 or max_cells < 1:
            raise ValueError("map_index: cap must be >= 0 and max_cells >= 1")
        plan = CropPlan(self, B, cap, mfp, None, want_index=want_index, max_cells=max_cells, want_normals=want_normals)
        out = plan.run(T.to(self.device), r.to(self.device))
        return out[:3] + ((plan.index,) if want_index else ()) + ((plan.normals,) if want_normals else ())


class CropPlan:
    """Fixed-capacity, preallocated form of MapIndex.crop: run() launches di2p_map_crop on the current stream with no allocation and no host
    synchronisation, so it can be captured in a hipGraph; a replay reads the priors and radii the tensors hold THEN.  cap: rows of the whole
    batch; max_frame_points: of one frame; max_radius: the largest radius a frame will ask for (a wider window: status 1).  want_normals: the
    index must carry normals; run() then launches di2p_map_crop_normals behind the crop and fills plan.normals f32[cap,3], row k the normal of
    kept row k in its frame's prior frame (rows past offsets[B] keep what they held); run() returns the same three tensors."""

    def __init__(self, index, B, cap, max_frame_points, max_radius, want_index=False, max_cells=None, want_normals=False):
        if not isinstance(index, MapIndex):
            raise ValueError("map_index: index must be a MapIndex (MapIndex.build)")
        if want_normals and index.normals is None:
            raise ValueError("map_index: want_normals needs an index that carries normals (MapIndex.build(..., normals=...))")
        self.max_src = _ragged._check_max_frame_points("map_index", max_frame_points)
        if int(B) < 0 or int(cap) < 0:
            raise ValueError("map_index: B and cap must be >= 0")
        self.index_map, self.B, self.cap = index, int(B), int(cap)
        self.max_cells = int(max_cells) if max_cells is not None else max_window_cells(index, max_radius)
        if self.max_cells < 1 or max(self.B, 1) * self.max_cells > 1 << 28:
            raise ValueError("map_index: B * max_cells must be at most 2^28 (a larger cell, or a smaller radius)")
        dev = index.device
        b = max(self.B, 1)
        self.ws = _ragged.workspace("di2p_map_crop_workspace_bytes", self.B, self.max_cells, dev)
        self.rows = torch.zeros((max(self.cap, 1), 4), dtype=torch.float32, device=dev)
        self.offsets = torch.zeros((self.B + 1,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((b,), dtype=torch.int32, device=dev)
        self.index = torch.zeros((max(self.cap, 1),), dtype=torch.int32, device=dev) if want_index or want_normals else None
        self.normals = torch.zeros((max(self.cap, 1), 3), dtype=torch.float32, device=dev) if want_normals else None

    def run(self, T_map_prior, radius):
        """T_map_prior f64[B,4,4], radius f64[B] (device) -> (rows f32[cap,4], offsets i32[B+1], status i32[B]), views of the plan's buffers"""
        B, ix = self.B, self.index_map
        _ragged._check_tensor("map_index", T_map_prior, "T_map_prior", torch.float64, (B, 4, 4))
        _ragged._check_tensor("map_index", radius, "radius", torch.float64, (B,))
        require_cuda(T_map_prior, radius)
        call("di2p_map_crop", ptr(ix.sorted), ptr(ix.cell_start), ptr(ix.order), *ix._grid_args(), ptr(T_map_prior), ptr(radius), B, self.cap,
             self.max_src, self.max_cells, ptr(self.rows), ptr(self.offsets), ptr(self.index), ptr(self.status), ptr(self.ws), stream())
        if self.normals is not None:
            call("di2p_map_crop_normals", ptr(ix.normals), ptr(self.index), ptr(self.offsets), ptr(T_map_prior), B, self.cap, ptr(self.normals),
                 stream())
        return self.rows, self.offsets, self.status[:B]


def map_pose(T_map_prior, P_scan, out=None):
    """T_map_prior, P_scan f64[B,4,4] (device) -> T_map_cam = T_map_prior . P_scan^-1 (the rigid inverse): with P_scan from prior-frame
    coordinates into the camera frame, the camera's pose in the map.  No synchronisation."""
    _ragged._check_tensor("map_index", T_map_prior, "T_map_prior", torch.float64, ("B", 4, 4))
    B = int(T_map_prior.shape[0])
    _ragged._check_tensor("map_index", P_scan, "P_scan", torch.float64, (B, 4, 4))
    out = torch.empty_like(T_map_prior) if out is None else _ragged._check_tensor("map_index", out, "out", torch.float64, (B, 4, 4))
    require_cuda(T_map_prior, P_scan, out)
    call("di2p_map_pose", ptr(T_map_prior), ptr(P_scan), B, ptr(out), stream())
    return out


def _check_dataset(dataset, index=None):
    """`index`: the map the data set's model is to be localised in; the KITTI model reads normals, so its map must carry them"""
    if dataset not in ("oxford", "nuscenes", "kitti"):
        raise ValueError("map_index: dataset must be 'oxford', 'nuscenes' or 'kitti', got %r" % (dataset,))
    if dataset == "kitti" and getattr(index, "normals", None) is None:
        raise ValueError("map_index: dataset 'kitti': the KITTI model reads normals, so a KITTI map needs MapIndex.build(..., normals=...) "
                         "(True, a dict of radius / max_nn / orient, or the user's own f32[M,3])")


class MapRawPlan:
    """CropPlan + sample_prep.SamplePlan(dataset): pose priors and camera frames to the loader's sample in one graph-safe call.  The crop is
    in the prior frame, so P_cam_pc maps PRIOR-frame coordinates into the camera frame and T_scan, the draw's Pr, maps them onto the prepared
    points.  The result equals CropPlan.run followed by sample_prep.SamplePlan.run bit for bit."""

    def __init__(self, index, opt, B, cap, max_frame_points, max_radius, raw_hw, mode="val", dataset="oxford", jitter=sample_prep.JITTER, color=None):
        _check_dataset(dataset, index)
        _ragged._check_max_frame_points("map_index", max_frame_points)
        sample_prep.option_block(opt, sample_prep.RAW_HW[dataset] if raw_hw is None else raw_hw, mode, dataset=dataset)      # argument errors first
        self.crop = CropPlan(index, B, cap, max_frame_points, max_radius, want_normals=dataset == "kitti")
        self.sample = sample_prep.SamplePlan(opt, B, int(cap), int(max_frame_points), raw_hw, mode, index.device, jitter=jitter, color=color,
                                             dataset=dataset)
        self.B = int(B)
        self.status = torch.zeros((max(self.B, 1),), dtype=torch.int32, device=index.device)

    @property
    def seed(self):
        """i64[1] device: the seed slot of the draws (sample_prep.SamplePlan.seed)"""
        return self.sample.seed

    @property
    def T_scan(self):
        """f64[B,4,4] device: the Pr the last run's draw applied to the crop"""
        return self.sample.table.Pr[:self.B]

    def run(self, T_map_prior, radius, images_u8, K_raw, P_cam_pc, seed=None):
        """T_map_prior f64[B,4,4], radius f64[B], images u8[B,H0,W0,3], K_raw f64[B,3,3], P_cam_pc f64[B,4,4] (all device) -> SamplePlan.run's
        nine tensors + (status i32[B], T_scan f64[B,4,4]): sample_prep.PREPARED, views of the plans' buffers.  status is the elementwise maximum
        of the crop's and the sample's.  seed=None leaves the seed slot as it is (graph replays)."""
        sample_prep._check_images(images_u8, self.B, self.sample.image.raw_hw)
        rows, offsets, _ = self.crop.run(T_map_prior, radius)
        out = self.sample.run(rows, self.crop.normals, offsets, images_u8, K_raw, P_cam_pc, seed=seed)          # KITTI: P_cam_pc for Pc, no Pji
        torch.maximum(self.crop.status, self.sample.status, out=self.status)
        return tuple(out) + (self.status[:self.B], self.T_scan)


def prepare_map_raw(index, T_map_prior, radius, images, K_raw, P_cam_pc, opt, max_frame_points, mode="val", seed=0, dataset="oxford", cap=None):
    """Convenience: builds a plan for this batch, runs it and checks the status (synchronises).  T_map_prior [B,4,4], radius a number or [B],
    images u8[B,H0,W0,3], K_raw [B,3,3], P_cam_pc [B,4,4] (host values) -> MapRawPlan.run's tuple."""
    _check_dataset(dataset, index)
    T = check_priors(T_map_prior)
    B = int(T.shape[0])
    r = check_radius(radius, B)
    images, raw_hw = sample_prep._host_images(images, B, "map_index", "frame")
    sample_prep.option_block(opt, raw_hw, mode, dataset=dataset)          # argument errors before anything touches the device
    mfp = _ragged._check_max_frame_points("map_index", max_frame_points)
    if not isinstance(index, MapIndex):
        raise ValueError("map_index: index must be a MapIndex (MapIndex.build)")
    finite = r[np.isfinite(r) & (r > 0)]
    dev = index.device
    plan = MapRawPlan(index, opt, B, B * mfp if cap is None else int(cap), mfp, float(finite.max()) if len(finite) else 1.0, raw_hw, mode, dataset)
    f64 = sample_prep._f64
    out = plan.run(torch.from_numpy(T).to(dev), torch.from_numpy(r).to(dev), images.to(dev).contiguous(), f64(K_raw, (B, 3, 3), dev),
                   f64(P_cam_pc, (B, 4, 4), dev), seed=seed)
    check_status(plan.status[:B])
    return out
