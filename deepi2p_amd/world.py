"""Synthetic worlds on the device (csrc/world.hip): one analytic scene per frame, ray-cast twice through ONE trace function -- for the camera
(a uint8 HWC raw frame) and for an HDL-64-like LiDAR (ragged [n,4] rows) -- so that image and point cloud show the same scene.  The outputs
are the tensors raw_prep.RawFramePlan.run and sample_prep.SamplePlan.run take; WorldPlan is the preallocated, graph-safe form.
synthetic.make_velodyne_scan / make_frame / make_camera_image are untouched: this module is the generator they are not (a rendered image).

The scene (make_world; the scene rule of synthetic.make_velodyne_scan, drawn in its order, z-up sensor frame): table f64[B, 32, 16] and
count i32[B] (at most MAX_PRIMS = 32; 0 is legal: all sky, no return).  A row:
    0      type: 0 ground plane z = z0, 1 axis-aligned box, 2 vertical cylinder
    1-6    ground z0 | box lo x y z, hi x y z | cylinder cx, cy, radius, z0, z1
    7-9    albedo r g b in [0, 1]        10  LiDAR reflectance = the albedo's luminance 0.299 r + 0.587 g + 0.114 b (the common cue)
    11     texture cell size (m, > 0)    12-15 unused (0)

trace(o, d) -> (t, prim): the fp64 arithmetic of synthetic._ray_box / _ray_pole, operation for operation (slab test with 1 / d, NaN products
skipped as np.nanmax / np.nanmin do; smaller cylinder root with disc >= 0, t > 0 and the height test; ground (z0 - o.z) / min(d.z, -1e-12)
for d.z < 0 and t > 0).  The nearest hit wins, ties go to the lowest index, a miss is (inf, -1).

The camera: pixel (u, v) casts d_cam = ((u - cx) / fx, (v - cy) / fy, 1) through cam_to_world (formed on the host in fp64: [T .] inv(Pc)), so t
is the camera-frame depth.  The colour, in fp64, every operation rounded on its own:
    hit      c = (((albedo * shade) * tex) * fade) * 255 per channel, at the hit point h = o + t d
             shade   ground 1;  box 0.80 on the x faces, 0.65 on the y faces, 1 on top (the face is the slab the entry parameter came from,
                     the first of equal ones);  cylinder 0.6 + 0.4 max(0, n . l), n = ((h.x - cx) / r, (h.y - cy) / r), l = (0.6, 0.8)
             tex     TEX[k & 7], k an integer hash of q = floor(h / cell) (the low 32 bits, after a clamp to +-2^52) without the axis the
                     surface is normal to (ground: z; box: the face's axis; cylinder: x and y) and of the primitive's index:
                     k = qx 73856093 ^ qy 19349663 ^ qz 83492791 ^ prim 2654435761;  k ^= k >> 13;  k *= 0x5bd1e995;  k ^= k >> 15  (mod 2^32)
             fade    1 - 0.5 min(t / max_range, 1)
    miss     c = SKY_TOP + SKY_SPAN (v + 0.5) / H0 per channel (a gradient in v)
    byte     floor(clamp(c, 0, 255) + 0.5)
Optional outputs: depth f32 (t; 0 on a miss) and prim i32 (-1 on a miss).  No transcendental function is on the camera path.

The scan: ray r = beam * azimuths + azimuth has the sensor-frame direction (cE cA, cE sA, sE) from host tables of cosines and sines
(hdl64_pattern: the elevations and the per-frame azimuth phase of make_velodyne_scan), cast from the sensor pose T (identity by default).
Kept iff t < max_range and u >= dropout, decided before the noise; t += range_sigma g; intensity = clip(reflectance + intensity_sigma g', 0,
1); rows (x, y, z, intensity) float32 in the sensor frame, in ray order.  u, g, g' come from Philox counter (r, frame0 + b, 0 | 1 | 2, 7):
u53 of the first two words, Box-Muller (cosine branch) of the two u53 of a block.

Push-broom profiles (the section at the end): the same worlds seen by a 2-D laser with one pose per profile -- make_street, make_trajectory,
traversal_inputs, render_profiles and TraversalPlan, whose outputs are the arguments of submap.OxfordRawPlan.run.
"""
import numpy as np
import torch

from . import _ragged
from ._lib import call, ptr, require_cuda, stream
from ._ragged import _dev

MAX_PRIMS, SLOTS = 32, 16
GROUND, BOX, CYLINDER = 0, 1, 2
LUMA = np.array([0.299, 0.587, 0.114])
TEX = np.array([0.70, 0.78, 0.86, 0.92, 1.00, 0.96, 0.82, 0.74])
SHADE = np.array([0.80, 0.65, 1.00])
LIGHT = np.array([0.6, 0.8])
SKY_TOP, SKY_SPAN = np.array([90.0, 140.0, 230.0]), np.array([110.0, 80.0, 15.0])
MAX_RANGE, DROPOUT, RANGE_SIGMA, INTENSITY_SIGMA = 120.0, 0.03, 0.02, 0.05          # make_velodyne_scan's defaults


# ---------------------------------------------------------------------------------------------------------------- scene and pattern (host)
def _row(kind, geom, albedo, cell):
    r = np.zeros(SLOTS)
    r[0] = kind
    r[1:1 + len(geom)] = geom
    r[7:10] = albedo
    r[10] = float(np.dot(LUMA, albedo))
    r[11] = cell
    return r


def _albedo(refl, tint):
    """a colour of luminance `refl` (up to the clip at 1) in the direction of `tint`"""
    return np.clip(tint * (refl / float(np.dot(LUMA, tint))), 0.0, 1.0)


def make_world(rng, B, sensor_height=1.73):
    """B scenes in the z-up sensor frame (sensor at the origin, `sensor_height` above the ground) -> (table f64[B,32,16], count i32[B]).
    Per frame the draws of synthetic.make_velodyne_scan's scene in its order (6-9 boxes, 4-8 poles, three far walls, nothing within 6 m),
    so a generator in the same state gives the same geometry; the tints and cell sizes are drawn after them."""
    table, count = np.zeros((int(B), MAX_PRIMS, SLOTS)), np.zeros((int(B),), np.int32)
    z0 = -float(sensor_height)
    for b in range(int(B)):
        geom, refl = [(GROUND, [z0])], [0.25]
        for _ in range(int(rng.integers(6, 10))):
            c = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40)])
            if np.hypot(*c) < 6.0:
                c *= 6.0 / max(np.hypot(*c), 1e-6)
            half = np.array([rng.uniform(0.8, 6.0), rng.uniform(0.8, 6.0)])
            hgt = rng.uniform(1.2, 8.0)
            geom.append((BOX, [c[0] - half[0], c[1] - half[1], z0, c[0] + half[0], c[1] + half[1], z0 + hgt]))
            refl.append(rng.uniform(0.1, 0.9))
        for _ in range(int(rng.integers(4, 9))):
            r = rng.uniform(5, 30)
            a = rng.uniform(-np.pi, np.pi)
            geom.append((CYLINDER, [r * np.cos(a), r * np.sin(a), rng.uniform(0.08, 0.3), z0, rng.uniform(2.0, 6.0)]))
            refl.append(rng.uniform(0.3, 1.0))
        wx, wy = rng.uniform(45, 70), rng.uniform(45, 70)
        for lo, hi in (([wx, -wy, z0], [wx + 1, wy, z0 + 10.0]), ([-wx - 1, wy, z0], [wx, wy + 1, z0 + 10.0]),
                       ([-wx - 1, -wy - 1, z0], [wx, -wy, z0 + 10.0])):
            geom.append((BOX, lo + hi))
            refl.append(rng.uniform(0.05, 0.5))
        n = len(geom)
        tints = rng.uniform(0.35, 1.0, (n, 3))
        tints[0] = 1.0                                           # the ground is grey
        cells = rng.uniform(0.4, 1.5, n)
        for i, ((kind, g), rf) in enumerate(zip(geom, refl)):
            table[b, i] = _row(kind, g, _albedo(rf, tints[i]), cells[i])
        count[b] = n
    return table, count


def hdl64_pattern(rng, B, beams=64, azimuths=1800):
    """-> (elevation f64[beams,2], azimuth f64[B,azimuths,2]): (cos, sin) of make_velodyne_scan's elevations (-24.8 .. +2 degrees) and of its
    azimuths with one phase draw per frame"""
    elev = np.deg2rad(np.linspace(-24.8, 2.0, int(beams)))
    azim = np.stack([np.linspace(-np.pi, np.pi, int(azimuths), endpoint=False) + rng.uniform(0, 2 * np.pi / max(int(azimuths), 1))
                     for _ in range(int(B))]) if B else np.zeros((0, int(azimuths)))
    return np.stack([np.cos(elev), np.sin(elev)], -1), np.stack([np.cos(azim), np.sin(azim)], -1)


# ---------------------------------------------------------------------------------------------------------------- argument checks (host)
def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def check_world(world):
    """(table, count), numpy arrays or tensors -> B; host values are checked in full, device tensors by shape and dtype (the device clamps
    a count to [0, 32])"""
    if not isinstance(world, (tuple, list)) or len(world) != 2:
        raise ValueError("world: a world is the pair (table f64[B,32,16], count i32[B])")
    table, count = world
    for a, name, kind, shape in ((table, "table", "f", (None, MAX_PRIMS, SLOTS)), (count, "count", "i", (None,))):
        dt = a.dtype if torch.is_tensor(a) else np.asarray(a).dtype
        ok = dt in (torch.float64, np.dtype(np.float64)) if kind == "f" else dt in (torch.int32, np.dtype(np.int32))
        sh = tuple(a.shape) if torch.is_tensor(a) else np.shape(a)
        if not ok or len(sh) != len(shape) or any(n is not None and m != n for m, n in zip(sh, shape)):
            raise ValueError("world: %s must be %s [%s]" % (name, "float64" if kind == "f" else "int32", ", ".join("B" if n is None else str(n) for n in shape)))
    B = int(table.shape[0])
    if int(count.shape[0]) != B:
        raise ValueError("world: table and count must have the same number of frames")
    if B > 65535:
        raise ValueError("world: at most 65535 frames in a batch")
    if not (torch.is_tensor(count) and count.is_cuda):
        c = _host(count)
        if c.size and (c.min() < 0 or c.max() > MAX_PRIMS):
            raise ValueError("world: a primitive count must be in [0, %d]" % MAX_PRIMS)
        if not (torch.is_tensor(table) and table.is_cuda):
            t = _host(table)
            for b in range(B):
                rows = t[b, :c[b]]
                if np.any((rows[:, 0] != GROUND) & (rows[:, 0] != BOX) & (rows[:, 0] != CYLINDER)) or not np.all(rows[:, 11] > 0):
                    raise ValueError("world: frame %d has a primitive of unknown type or a texture cell size that is not positive" % b)
    return B


def _world_dev(world, dev):
    B = check_world(world)
    table, count = (a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a)) for a in world)
    return table.to(dev).contiguous(), count.to(dev).contiguous(), B


def _mats(a, B, n, name):
    """host f64[B,n,n]"""
    m = np.ascontiguousarray(_host(a), dtype=np.float64)
    if m.shape != (B, n, n) or not np.all(np.isfinite(m)):
        raise ValueError("world: %s must be a finite array [%d, %d, %d]" % (name, B, n, n))
    return m


def camera_pose(Pc, T=None):
    """cam_to_world f64[B,4,4] = [T .] inv(Pc), on the host in fp64.  Pc: sensor frame -> camera frame (RawFramePlan's Pc); T: the sensor's
    pose in the world (None: the world is given in the sensor frame)."""
    Pc = np.asarray(Pc, dtype=np.float64)
    try:
        inv = np.linalg.inv(Pc)
    except np.linalg.LinAlgError:
        raise ValueError("world: Pc must be invertible")
    return np.ascontiguousarray(inv if T is None else np.matmul(np.asarray(T, dtype=np.float64), inv))


def _check_scan_opt(max_range, dropout, range_sigma, intensity_sigma, frame0=0):
    if not (0.0 < float(max_range) < 1e300) or not (0.0 <= float(dropout) <= 1.0):
        raise ValueError("world: max_range must be positive and dropout in [0, 1]")
    if not (0.0 <= float(range_sigma) < 1e300) or not (0.0 <= float(intensity_sigma) < 1e300):
        raise ValueError("world: range_sigma and intensity_sigma must be >= 0")
    if int(frame0) < 0:
        raise ValueError("world: frame0 must be >= 0")
    return float(max_range), float(dropout), float(range_sigma), float(intensity_sigma)


def _check_hw(B, H0, W0):
    if int(H0) < 0 or int(W0) < 0 or int(H0) * int(W0) >= 1 << 29:
        raise ValueError("world: H0, W0 must be >= 0 and H0 * W0 below 2^29")
    return int(H0), int(W0)


def _check_pattern(pattern, B):
    if not isinstance(pattern, (tuple, list)) or len(pattern) != 2:
        raise ValueError("world: a pattern is the pair (elevation f64[beams,2], azimuth f64[B,azimuths,2])")
    elev, azim = (np.ascontiguousarray(_host(a), dtype=np.float64) for a in pattern)
    if elev.ndim != 2 or elev.shape[1] != 2 or azim.ndim != 3 or azim.shape[0] != B or azim.shape[2] != 2:
        raise ValueError("world: pattern must be (elevation [beams, 2], azimuth [%d, azimuths, 2]) of (cos, sin)" % B)
    if not (np.all(np.isfinite(elev)) and np.all(np.isfinite(azim))):
        raise ValueError("world: pattern must be finite")
    if B * elev.shape[0] * azim.shape[1] >= 2 ** 31:
        raise ValueError("world: the capacity B * beams * azimuths must stay below 2^31")
    return elev, azim


def workspace(B, R, device=None):
    return _ragged.workspace("di2p_world_workspace_bytes", B, R, device)


# ---------------------------------------------------------------------------------------------------------------- eager calls
def trace(world, origin, dirs, device=None):
    """origin [B,3], dirs [B,R,3] (fp64; host arrays or tensors) -> (t f64[B,R], prim i32[B,R]) on the device.  No synchronisation."""
    B = check_world(world)
    o, d = (a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)) for a in (origin, dirs))
    if o.dtype != torch.float64 or tuple(o.shape) != (B, 3) or d.dtype != torch.float64 or d.dim() != 3 or d.shape[0] != B or d.shape[2] != 3:
        raise ValueError("world: origin must be float64 [%d, 3] and dirs float64 [%d, R, 3]" % (B, B))
    R = int(d.shape[1])
    if B * R >= 2 ** 31:
        raise ValueError("world: B * R must stay below 2^31")
    dev = device or _dev()
    table, count, _ = _world_dev(world, dev)
    o, d = o.to(dev).contiguous(), d.to(dev).contiguous()
    t = torch.empty((B, R), dtype=torch.float64, device=dev)
    prim = torch.empty((B, R), dtype=torch.int32, device=dev)
    call("di2p_world_trace", ptr(table), ptr(count), B, MAX_PRIMS, ptr(o), ptr(d), R, ptr(t), ptr(prim), stream())
    return t, prim


def render_camera(world, K_raw, Pc, H0, W0, T=None, depth=False, prim=False, max_range=MAX_RANGE, device=None):
    """K_raw [B,3,3], Pc [B,4,4], T [B,4,4] | None (host) -> image u8[B,H0,W0,3] on the device, or the tuple (image[, depth f32[B,H0,W0]][,
    prim i32[B,H0,W0]]) when asked for.  No synchronisation."""
    B = check_world(world)
    H0, W0 = _check_hw(B, H0, W0)
    K = _mats(K_raw, B, 3, "K_raw")
    if np.any(K[:, 0, 0] == 0) or np.any(K[:, 1, 1] == 0):
        raise ValueError("world: K_raw needs focal lengths that are not 0")
    M = camera_pose(_mats(Pc, B, 4, "Pc"), None if T is None else _mats(T, B, 4, "T"))
    max_range = _check_scan_opt(max_range, 0.0, 0.0, 0.0)[0]
    dev = device or _dev()
    table, count, _ = _world_dev(world, dev)
    Kd, Md = torch.as_tensor(K).to(dev), torch.as_tensor(M).to(dev)
    img = torch.empty((B, H0, W0, 3), dtype=torch.uint8, device=dev)
    dep = torch.empty((B, H0, W0), dtype=torch.float32, device=dev) if depth else None
    pr = torch.empty((B, H0, W0), dtype=torch.int32, device=dev) if prim else None
    call("di2p_world_render_camera", ptr(table), ptr(count), B, MAX_PRIMS, ptr(Kd), ptr(Md), H0, W0, max_range, ptr(img), ptr(dep), ptr(pr), stream())
    out = (img,) + ((dep,) if depth else ()) + ((pr,) if prim else ())
    return out if len(out) > 1 else img


def render_scan(world, pattern, seed, T=None, max_range=MAX_RANGE, dropout=DROPOUT, range_sigma=RANGE_SIGMA, intensity_sigma=INTENSITY_SIGMA,
                frame0=0, device=None):
    """pattern: hdl64_pattern's pair; T [B,4,4] | None: the sensor pose -> (points f32[B * beams * azimuths, 4], offsets i32[B+1],
    count i32[B]) on the device: frame b's rows are points[offsets[b]:offsets[b+1]].  No synchronisation."""
    B = check_world(world)
    elev, azim = _check_pattern(pattern, B)
    opt = _check_scan_opt(max_range, dropout, range_sigma, intensity_sigma, frame0)
    pose = np.tile(np.eye(4), (B, 1, 1)) if T is None else _mats(T, B, 4, "T")
    dev = device or _dev()
    table, count, _ = _world_dev(world, dev)
    beams, azimuths = elev.shape[0], azim.shape[1]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    e, a, p = t(elev), t(azim), t(pose)
    points = torch.zeros((max(B * beams * azimuths, 1), 4), dtype=torch.float32, device=dev)
    offsets = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
    cnt = torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)
    call("di2p_world_render_scan", ptr(table), ptr(count), B, MAX_PRIMS, ptr(e), ptr(a), ptr(p), beams, azimuths, *opt, int(seed) & (2 ** 64 - 1), None,
         int(frame0), ptr(points), ptr(offsets), ptr(cnt), ptr(workspace(B, beams * azimuths, dev)), stream())
    return points, offsets, cnt[:B]


# ---------------------------------------------------------------------------------------------------------------- the plan
class WorldPlan:
    """Fixed-capacity, preallocated camera render + scan of B frames: run() launches five kernels on the current stream with no allocation
    and no host synchronisation, so it can be captured in the same hipGraph as raw_prep.RawFramePlan.run, which takes its outputs:

        wp = WorldPlan(B, H0, W0, beams, azimuths, dev, seed_slot=raw_plan.seed); wp.set_pattern(hdl64_pattern(rng, B, beams, azimuths))
        points, offsets, images = wp.run(world, K_raw, Pc)          # host arrays: uploaded into the plan's buffers (not capturable)
        raw_plan.run(points, offsets, images, wp.K_raw, wp.Pc)      # cap_raw = wp.cap
        ... capture: wp.run(None, None, None) reuses the buffers; wp.seed.fill_(s); graph.replay()

    The seed lives in plan.seed (i64[1], device; seed_slot: another plan's slot to share).  run(seed=None) leaves it alone."""

    def __init__(self, B, H0, W0, beams, azimuths, device=None, seed_slot=None, max_range=MAX_RANGE, dropout=DROPOUT, range_sigma=RANGE_SIGMA,
                 intensity_sigma=INTENSITY_SIGMA, frame0=0):
        if int(B) < 0 or int(B) > 65535 or int(beams) < 0 or int(azimuths) < 0:
            raise ValueError("world: B must be in [0, 65535], beams and azimuths >= 0")
        self.B, self.beams, self.azimuths, self.frame0 = int(B), int(beams), int(azimuths), int(frame0)
        self.H0, self.W0 = _check_hw(B, H0, W0)
        self.cap = self.B * self.beams * self.azimuths
        if self.cap >= 2 ** 31:
            raise ValueError("world: the capacity B * beams * azimuths must stay below 2^31")
        self.opt = _check_scan_opt(max_range, dropout, range_sigma, intensity_sigma, frame0)
        if seed_slot is not None and (not torch.is_tensor(seed_slot) or seed_slot.dtype != torch.int64 or seed_slot.numel() != 1):
            raise ValueError("world: seed_slot must be an int64 tensor with one element")
        dev = device or _dev()
        b = max(self.B, 1)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.table, self.count = f64(b, MAX_PRIMS, SLOTS), torch.zeros((b,), dtype=torch.int32, device=dev)
        self.K_raw, self.Pc, self.cam_to_world, self.pose = f64(b, 3, 3), f64(b, 4, 4), f64(b, 4, 4), f64(b, 4, 4)
        self.K_raw[:] = torch.eye(3, dtype=torch.float64)
        for m in (self.Pc, self.cam_to_world, self.pose):
            m[:] = torch.eye(4, dtype=torch.float64)
        self.elevation, self.azimuth = f64(max(self.beams, 1), 2), f64(b, max(self.azimuths, 1), 2)
        self.seed = seed_slot if seed_slot is not None else torch.zeros((1,), dtype=torch.int64, device=dev)
        self.images = torch.zeros((self.B, self.H0, self.W0, 3), dtype=torch.uint8, device=dev)
        self.points = torch.zeros((max(self.cap, 1), 4), dtype=torch.float32, device=dev)
        self.offsets = torch.zeros((self.B + 1,), dtype=torch.int32, device=dev)
        self.kept = torch.zeros((b,), dtype=torch.int32, device=dev)
        self.ws = workspace(self.B, self.beams * self.azimuths, dev)

    def set_pattern(self, pattern):
        elev, azim = _check_pattern(pattern, self.B)
        if elev.shape[0] != self.beams or azim.shape[1] != self.azimuths:
            raise ValueError("world: the plan was made for %d beams x %d azimuths" % (self.beams, self.azimuths))
        if self.B and self.cap:
            self.elevation.copy_(torch.as_tensor(elev))
            self.azimuth.copy_(torch.as_tensor(azim))

    def set_world(self, world):
        if check_world(world) != self.B:
            raise ValueError("world: the plan was made for %d frames" % self.B)
        if self.B:
            self.table.copy_(world[0] if torch.is_tensor(world[0]) else torch.as_tensor(np.ascontiguousarray(world[0])))
            self.count.copy_(world[1] if torch.is_tensor(world[1]) else torch.as_tensor(np.ascontiguousarray(world[1])))

    def set_cameras(self, K_raw, Pc, T=None):
        """K_raw [B,3,3], Pc [B,4,4], T [B,4,4] | None (host, or brought to the host): the inverse is formed here, in fp64"""
        B = self.B
        K, P = _mats(K_raw, B, 3, "K_raw"), _mats(Pc, B, 4, "Pc")
        if np.any(K[:, 0, 0] == 0) or np.any(K[:, 1, 1] == 0):
            raise ValueError("world: K_raw needs focal lengths that are not 0")
        Tm = None if T is None else _mats(T, B, 4, "T")
        M = camera_pose(P, Tm)
        if B:
            for dst, src in ((self.K_raw, K), (self.Pc, P), (self.cam_to_world, M), (self.pose, np.tile(np.eye(4), (B, 1, 1)) if Tm is None else Tm)):
                dst.copy_(torch.as_tensor(src))

    def run(self, world=None, K_raw=None, Pc=None, T=None, seed=None):
        """world / K_raw, Pc[, T]: given -> checked on the host and uploaded into the plan's buffers first (set_world / set_cameras); None ->
        the buffers as they are (the capturable form).  -> (points_raw f32[cap,4], offsets i32[B+1], images u8[B,H0,W0,3]), views of the
        plan's buffers; plan.kept i32[B] has the rows per frame."""
        if (K_raw is None) != (Pc is None) or (T is not None and Pc is None):
            raise ValueError("world: K_raw and Pc go together (and T only with them)")
        if world is not None:
            self.set_world(world)
        if K_raw is not None:
            self.set_cameras(K_raw, Pc, T)
        if seed is not None:
            self.seed.fill_(int(seed))
        B, s = self.B, stream()
        require_cuda(self.table, self.images, self.points, self.seed)
        call("di2p_world_render_camera", ptr(self.table), ptr(self.count), B, MAX_PRIMS, ptr(self.K_raw), ptr(self.cam_to_world), self.H0, self.W0,
             self.opt[0], ptr(self.images), None, None, s)
        call("di2p_world_render_scan", ptr(self.table), ptr(self.count), B, MAX_PRIMS, ptr(self.elevation), ptr(self.azimuth), ptr(self.pose),
             self.beams, self.azimuths, *self.opt, 0, ptr(self.seed), self.frame0, ptr(self.points), ptr(self.offsets), ptr(self.kept), ptr(self.ws), s)
        return self.points, self.offsets, self.images


# ---------------------------------------------------------------------------------------------------------------- push-broom profiles
# An Oxford traversal from the same kind of world: a 2-D laser (the LMS of deepi2p_amd.submap) carried along a street, one scene per
# sub-map, one pose per profile, and the camera frame of the same scene.  World frame: z up, the ground at z = 0, the street along x.
# Vehicle frame: x forward, y right, z down (the fixed flip is inside T_world_vehicle).  Laser frame: x to the ground, the scan plane
# across the direction of travel (synthetic.make_lms_traversal's G_posesource_laser).
#
# The profile render (di2p_world_render_profiles): beam k of profile s casts R_s . (c_k, s_k, 0) from the translation of laser_to_world[s]
# (every entry (R_i0 c + R_i1 s) + R_i2 0, each product rounded).  Kept iff t < max_range and u >= dropout, decided before the noise;
# t += range_sigma g; the row is (t c_k, t s_k, clip(255 (reflectance + reflectance_sigma g'), 0, 255)) in float64 -- the reflectance is
# NOT rounded to an integer.  u, g, g' come from Philox counter (k, frame0 + s, 0 | 1 | 2, 8), s the profile's index in the batch.  Kept
# rays in beam order, profile after profile: scan_xyr f64[S * beams, 3] and scan_offsets i32[S+1], the first two arguments of
# di2p_submap_build.
LMS_MAX_RANGE, LMS_DROPOUT, LMS_RANGE_SIGMA, REFLECTANCE_SIGMA = 50.0, 0.05, 0.01, 0.1          # make_lms_traversal's (25 / 255 ~ 0.1)


def lms_pattern(beams=541, fov_deg=270.0):
    """-> beam f64[beams,2]: (cos, sin) of linspace(-fov / 2, fov / 2, beams); angle 0 points along laser x, the axis that points to the ground"""
    if int(beams) < 0 or not (0.0 <= float(fov_deg) <= 360.0):
        raise ValueError("world: beams must be >= 0 and fov_deg in [0, 360]")
    a = np.deg2rad(np.linspace(-float(fov_deg) / 2.0, float(fov_deg) / 2.0, int(beams)))
    return np.stack([np.cos(a), np.sin(a)], -1)


def make_street(rng, B, length, clearance=4.0):
    """B streets along world x (z up, the ground at z = 0) -> (table f64[B,32,16], count i32[B]) in make_world's row format: the ground,
    buildings (boxes) on both sides of a corridor, poles at the corridor's edge, two end walls; at most MAX_PRIMS primitives, and nothing
    but the ground closer (in x-y) than `clearance` to the centre line y = 0 over [-length / 2, length / 2]."""
    length, clearance = float(length), float(clearance)
    if not (length > 0.0 and clearance > 0.0):
        raise ValueError("world: length and clearance must be positive")
    table, count = np.zeros((int(B), MAX_PRIMS, SLOTS)), np.zeros((int(B),), np.int32)
    half = length / 2.0
    for b in range(int(B)):
        geom, refl = [(GROUND, [0.0])], [0.25]
        n_poles = int(rng.integers(4, 7))
        per_side = int(min((MAX_PRIMS - 3 - n_poles) // 2, max(1, round(length / 12.0))))
        for side in (1.0, -1.0):
            cuts = np.concatenate([[-half - clearance], np.sort(rng.uniform(-half, half, per_side - 1)), [half + clearance]])
            for x0, x1 in zip(cuts[:-1], cuts[1:]):
                gap = rng.uniform(0.0, 0.3) * (x1 - x0)
                near, depth, hgt = clearance + rng.uniform(0.5, 4.0), rng.uniform(5.0, 12.0), rng.uniform(3.0, 12.0)
                ys = sorted([side * near, side * (near + depth)])
                geom.append((BOX, [x0 + gap / 2, ys[0], 0.0, x1 - gap / 2, ys[1], hgt]))
                refl.append(rng.uniform(0.1, 0.9))
        for _ in range(n_poles):
            r = rng.uniform(0.08, 0.3)
            side = 1.0 if rng.random() < 0.5 else -1.0
            geom.append((CYLINDER, [rng.uniform(-half, half), side * (clearance + r + rng.uniform(0.0, 0.4)), r, 0.0, rng.uniform(2.0, 6.0)]))
            refl.append(rng.uniform(0.3, 1.0))
        wide = clearance + 20.0
        for x0 in (half + clearance, -half - clearance - 1.0):
            geom.append((BOX, [x0, -wide, 0.0, x0 + 1.0, wide, 10.0]))
            refl.append(rng.uniform(0.05, 0.5))
        n = len(geom)
        tints = rng.uniform(0.35, 1.0, (n, 3))
        tints[0] = 1.0                                           # the ground is grey
        cells = rng.uniform(0.4, 1.5, n)
        for i, ((kind, g), rf) in enumerate(zip(geom, refl)):
            table[b, i] = _row(kind, g, _albedo(rf, tints[i]), cells[i])
        count[b] = n
    return table, count


def make_trajectory(rng, B, S, speed=10.0, rate=50.0, creep=True, height=0.3, clearance=4.0, skip_threshold=0.1 / 16.0):
    """-> T_world_vehicle f64[B,S,4,4]: per sub-map S vehicle poses (x forward, y right, z down; the flip to the z-up world is inside the
    pose) `height` above the ground, along a gentle S-curve centred on x = 0 whose origin stays within clearance / 4 of the centre line y = 0
    (a laser mounted within clearance / 4 of the vehicle's origin therefore stays within clearance / 2), at about `speed` m/s and `rate`
    profiles per second; creep: with stretches slower than `skip_threshold` per profile, as in synthetic.make_lms_traversal."""
    B, S = int(B), int(S)
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    T = np.tile(np.eye(4), (B, max(S, 0), 1, 1))
    for b in range(B):
        step = np.full(S, float(speed) / float(rate))
        if creep:
            for _ in range(max(1, S // 25)):
                a = int(rng.integers(0, max(S - 1, 1)))
                step[a:a + int(rng.integers(2, 9))] = skip_threshold * rng.uniform(0.05, 0.45)
        dist = np.cumsum(step) - (step[0] if S else 0.0)
        x = dist - (dist[-1] / 2.0 if S else 0.0)
        amp, wave, phase = float(clearance) / 4.0, 35.0, rng.uniform(0.0, 2.0 * np.pi)
        y = amp * np.sin(x / wave + phase)
        yaw = np.arctan(amp / wave * np.cos(x / wave + phase))          # the tangent of the curve
        for i in range(S):
            c, s = np.cos(yaw[i]), np.sin(yaw[i])
            Rz = np.array([[c, -s, 0, x[i]], [s, c, 0, y[i]], [0, 0, 1.0, float(height)], [0, 0, 0, 1.0]])
            T[b, i] = Rz @ flip
    return T


def traversal_inputs(T_world_vehicle, origin, cam, G_posesource_laser, G_cam):
    """T_world_vehicle f64[B,S,4,4]; origin / cam: the index (an int, or one per sub-map) of the profile whose vehicle frame is the
    sub-map's origin / at which the camera frame is taken; G_cam [4,4] or [B,4,4].  Host, fp64 ->
    (laser_to_world f64[B,S,4,4] = T_wv[s] . G_posesource_laser,  poses f64[B,S,4,4] = inv(T_wv[origin]) . T_wv[s],
     cam_to_world f64[B,4,4] = T_wv[cam] . inv(G_cam),  P_cam_pc f64[B,4,4] = G_cam . inv(T_wv[cam]) . T_wv[origin] . inv(G_cam))"""
    T = np.asarray(T_world_vehicle, dtype=np.float64)
    if T.ndim != 4 or T.shape[2:] != (4, 4) or T.shape[1] < 1:
        raise ValueError("world: T_world_vehicle must be [B, S, 4, 4] with S >= 1")
    B, S = T.shape[:2]
    idx = []
    for v, name in ((origin, "origin"), (cam, "cam")):
        i = np.broadcast_to(np.asarray(v, dtype=np.int64), (B,)) if np.ndim(v) <= 1 and np.size(v) in (1, B) else None
        if i is None or (B and (i.min() < 0 or i.max() >= S)):
            raise ValueError("world: %s must be a profile index in [0, %d), one or one per sub-map" % (name, S))
        idx.append(i)
    Gl = np.asarray(G_posesource_laser, dtype=np.float64)
    Gc = np.asarray(G_cam, dtype=np.float64)
    Gc = np.tile(Gc, (B, 1, 1)) if Gc.shape == (4, 4) else Gc
    if Gl.shape != (4, 4) or Gc.shape != (B, 4, 4):
        raise ValueError("world: G_posesource_laser must be [4, 4] and G_cam [4, 4] or [%d, 4, 4]" % B)
    ar = np.arange(B)
    T_o, T_c, Gc_inv = T[ar, idx[0]], T[ar, idx[1]], np.linalg.inv(Gc)
    laser_to_world = np.matmul(T, Gl)
    poses = np.matmul(np.linalg.inv(T_o)[:, None], T)
    cam_to_world = np.matmul(T_c, Gc_inv)
    P_cam_pc = np.matmul(np.matmul(np.matmul(Gc, np.linalg.inv(T_c)), T_o), Gc_inv)
    return tuple(np.ascontiguousarray(a) for a in (laser_to_world, poses, cam_to_world, P_cam_pc))


def _check_profiles(submap_offsets, laser_to_world, beam, B):
    off = np.ascontiguousarray(_host(submap_offsets)).reshape(-1)
    if off.shape[0] != B + 1 or off.dtype.kind not in "iu":
        raise ValueError("world: submap_offsets must be %d integers (one scene per sub-map)" % (B + 1))
    L = np.ascontiguousarray(_host(laser_to_world), dtype=np.float64)
    if L.ndim != 3 or L.shape[1:] != (4, 4) or not np.all(np.isfinite(L)):
        raise ValueError("world: laser_to_world must be a finite array [S, 4, 4] (one pose per profile)")
    bm = _check_beam(beam)
    if L.shape[0] * bm.shape[0] >= 2 ** 31:
        raise ValueError("world: the capacity S * beams must stay below 2^31")
    return off.astype(np.int32), L, bm


def _check_beam(beam, beams=None):
    bm = np.ascontiguousarray(_host(beam), dtype=np.float64)
    if bm.ndim != 2 or bm.shape[1] != 2 or not np.all(np.isfinite(bm)) or (beams is not None and bm.shape[0] != beams):
        raise ValueError("world: beam must be a finite array [%s, 2] of (cos, sin)" % ("beams" if beams is None else beams))
    return bm


def profiles_workspace(S_cap, beams, device=None):
    return _ragged.workspace("di2p_world_profiles_workspace_bytes", S_cap, beams, device)


def render_profiles(world, submap_offsets, laser_to_world, beam, seed, max_range=LMS_MAX_RANGE, dropout=LMS_DROPOUT, range_sigma=LMS_RANGE_SIGMA,
                    reflectance_sigma=REFLECTANCE_SIGMA, frame0=0, device=None):
    """world: one scene per sub-map; submap_offsets [B+1] (host: uploaded as given, checked on the device -> status 3); laser_to_world
    [S,4,4]; beam [beams,2] (lms_pattern) -> (scan_xyr f64[S * beams, 3], scan_offsets i32[S+1], count i32[S], status i32[B]) on the device:
    profile s's rows are scan_xyr[scan_offsets[s]:scan_offsets[s+1]].  No synchronisation."""
    B = check_world(world)
    off, L, bm = _check_profiles(submap_offsets, laser_to_world, beam, B)
    opt = _check_scan_opt(max_range, dropout, range_sigma, reflectance_sigma, frame0)
    dev = device or _dev()
    table, count, _ = _world_dev(world, dev)
    S, beams = L.shape[0], bm.shape[0]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    o, l, m = t(off), t(L if S else np.zeros((1, 4, 4))), t(bm if beams else np.zeros((1, 2)))
    xyr = torch.zeros((max(S * beams, 1), 3), dtype=torch.float64, device=dev)
    scan_off = torch.zeros((S + 1,), dtype=torch.int32, device=dev)
    cnt = torch.zeros((max(S, 1),), dtype=torch.int32, device=dev)
    status = torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)
    call("di2p_world_render_profiles", ptr(table), ptr(count), B, MAX_PRIMS, ptr(o), ptr(l), ptr(m), S, beams, *opt, int(seed) & (2 ** 64 - 1), None,
         int(frame0), ptr(xyr), ptr(scan_off), ptr(cnt), ptr(status), ptr(profiles_workspace(S, beams, dev)), stream())
    return xyr, scan_off, cnt[:S], status[:B]


class TraversalPlan:
    """Fixed-capacity, preallocated camera render + profile render of B sub-maps of S profiles: run() launches seven kernels on the current
    stream with no allocation and no host synchronisation, so it can be captured in the same hipGraph as submap.OxfordRawPlan.run, which
    takes its outputs in their order:

        tp = TraversalPlan(B, S, beams, H0, W0, dev, seed_slot=oxford_plan.seed)
        tp.set_world(make_street(rng, B, length)); tp.set_calibration(G_posesource_laser, G_cam); tp.set_camera(K_raw)
        tp.set_traversal(*traversal_inputs(make_trajectory(rng, B, S), S // 2, S // 2, G_posesource_laser, G_cam))
        oxford_plan.run(*tp.run(), seed=None)          # S_cap = tp.S_cap = B S, P_cap = tp.P_cap = B S beams

    Every profile is present; the camera frame of sub-map b is rendered at cam_to_world[b].  The seed lives in plan.seed (i64[1], device;
    seed_slot: another plan's slot to share).  run(seed=None) leaves it alone."""

    def __init__(self, B, S, beams, H0, W0, device=None, seed_slot=None, beam=None, max_range=LMS_MAX_RANGE, dropout=LMS_DROPOUT,
                 range_sigma=LMS_RANGE_SIGMA, reflectance_sigma=REFLECTANCE_SIGMA, frame0=0, camera_range=MAX_RANGE):
        if int(B) < 0 or int(B) > 65535 or int(S) < 0 or int(beams) < 0:
            raise ValueError("world: B must be in [0, 65535], S and beams >= 0")
        self.B, self.S, self.beams, self.frame0 = int(B), int(S), int(beams), int(frame0)
        self.H0, self.W0 = _check_hw(B, H0, W0)
        self.S_cap, self.P_cap = self.B * self.S, self.B * self.S * self.beams
        if self.P_cap >= 2 ** 31:
            raise ValueError("world: the capacity B * S * beams must stay below 2^31")
        self.opt = _check_scan_opt(max_range, dropout, range_sigma, reflectance_sigma, frame0)
        self.camera_range = _check_scan_opt(camera_range, 0.0, 0.0, 0.0)[0]
        if seed_slot is not None and (not torch.is_tensor(seed_slot) or seed_slot.dtype != torch.int64 or seed_slot.numel() != 1):
            raise ValueError("world: seed_slot must be an int64 tensor with one element")
        dev = device or _dev()
        b, s = max(self.B, 1), max(self.S_cap, 1)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        eye = lambda *lead: torch.eye(4, dtype=torch.float64, device=dev).repeat(*lead, 1, 1).contiguous()
        self.table, self.count = f64(b, MAX_PRIMS, SLOTS), torch.zeros((b,), dtype=torch.int32, device=dev)
        self.K_raw = torch.eye(3, dtype=torch.float64, device=dev).repeat(b, 1, 1).contiguous()
        self.laser_to_world, self.poses, self.cam_to_world, self.P_cam_pc, self.G_cam = eye(s), eye(s), eye(b), eye(b), eye(b)
        self.G_posesource_laser = torch.eye(4, dtype=torch.float64, device=dev)
        self.present = torch.ones((s,), dtype=torch.uint8, device=dev)
        self.submap_offsets = (torch.arange(self.B + 1, dtype=torch.int32) * self.S).to(dev)
        self.beam = f64(max(self.beams, 1), 2)
        self.set_pattern(lms_pattern(self.beams) if beam is None else beam)
        self.seed = seed_slot if seed_slot is not None else torch.zeros((1,), dtype=torch.int64, device=dev)
        self.images = torch.zeros((self.B, self.H0, self.W0, 3), dtype=torch.uint8, device=dev)
        self.scan_xyr = f64(max(self.P_cap, 1), 3)
        self.scan_offsets = torch.zeros((self.S_cap + 1,), dtype=torch.int32, device=dev)
        self.kept = torch.zeros((s,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((b,), dtype=torch.int32, device=dev)
        self.ws = profiles_workspace(self.S_cap, self.beams, dev)

    def set_pattern(self, beam):
        bm = _check_beam(beam, self.beams)
        if self.beams:
            self.beam.copy_(torch.as_tensor(bm))

    def set_world(self, world):
        if check_world(world) != self.B:
            raise ValueError("world: the plan was made for %d sub-maps" % self.B)
        if self.B:
            self.table.copy_(world[0] if torch.is_tensor(world[0]) else torch.as_tensor(np.ascontiguousarray(world[0])))
            self.count.copy_(world[1] if torch.is_tensor(world[1]) else torch.as_tensor(np.ascontiguousarray(world[1])))

    def set_calibration(self, G_posesource_laser, G_cam):
        """G_posesource_laser [4,4], G_cam [4,4] or [B,4,4] (host): handed on to OxfordRawPlan.run as they are"""
        Gl = np.ascontiguousarray(_host(G_posesource_laser), dtype=np.float64)
        Gc = np.ascontiguousarray(_host(G_cam), dtype=np.float64)
        Gc = np.tile(Gc, (self.B, 1, 1)) if Gc.shape == (4, 4) else Gc
        if Gl.shape != (4, 4) or Gc.shape != (self.B, 4, 4) or not (np.all(np.isfinite(Gl)) and np.all(np.isfinite(Gc))):
            raise ValueError("world: G_posesource_laser must be a finite array [4, 4] and G_cam [4, 4] or [%d, 4, 4]" % self.B)
        self.G_posesource_laser.copy_(torch.as_tensor(Gl))
        if self.B:
            self.G_cam.copy_(torch.as_tensor(Gc))

    def set_traversal(self, laser_to_world, poses, cam_to_world, P_cam_pc):
        """traversal_inputs' four arrays (host): [B,S,4,4], [B,S,4,4], [B,4,4], [B,4,4]"""
        B, S = self.B, self.S
        per_profile = []
        for a, name in ((laser_to_world, "laser_to_world"), (poses, "poses")):
            m = np.ascontiguousarray(_host(a), dtype=np.float64)
            if m.shape != (B, S, 4, 4) or not np.all(np.isfinite(m)):
                raise ValueError("world: %s must be a finite array [%d, %d, 4, 4]" % (name, B, S))
            per_profile.append(m.reshape(B * S, 4, 4))
        per_map = [_mats(cam_to_world, B, 4, "cam_to_world"), _mats(P_cam_pc, B, 4, "P_cam_pc")]
        if self.S_cap:
            self.laser_to_world.copy_(torch.as_tensor(per_profile[0]))
            self.poses.copy_(torch.as_tensor(per_profile[1]))
        if B:
            self.cam_to_world.copy_(torch.as_tensor(per_map[0]))
            self.P_cam_pc.copy_(torch.as_tensor(per_map[1]))

    def set_camera(self, K_raw):
        K = _mats(K_raw, self.B, 3, "K_raw")
        if np.any(K[:, 0, 0] == 0) or np.any(K[:, 1, 1] == 0):
            raise ValueError("world: K_raw needs focal lengths that are not 0")
        if self.B:
            self.K_raw.copy_(torch.as_tensor(K))

    def run(self, seed=None):
        """-> (scan_xyr f64[P_cap,3], scan_offsets i32[S_cap+1], submap_offsets i32[B+1], poses f64[S_cap,4,4], present u8[S_cap] (all ones),
        G_posesource_laser f64[4,4], G_cam f64[B,4,4], images u8[B,H0,W0,3], K_raw f64[B,3,3], P_cam_pc f64[B,4,4]): the arguments of
        submap.OxfordRawPlan.run in their order, views of the plan's buffers; plan.kept i32[S_cap] has the rows per profile, plan.status
        i32[B] the status of the offsets (always 0 here)."""
        if seed is not None:
            self.seed.fill_(int(seed))
        B, s = self.B, stream()
        require_cuda(self.table, self.images, self.scan_xyr, self.seed)
        call("di2p_world_render_camera", ptr(self.table), ptr(self.count), B, MAX_PRIMS, ptr(self.K_raw), ptr(self.cam_to_world), self.H0, self.W0,
             self.camera_range, ptr(self.images), None, None, s)
        call("di2p_world_render_profiles", ptr(self.table), ptr(self.count), B, MAX_PRIMS, ptr(self.submap_offsets), ptr(self.laser_to_world),
             ptr(self.beam), self.S_cap, self.beams, *self.opt, 0, ptr(self.seed), self.frame0, ptr(self.scan_xyr), ptr(self.scan_offsets),
             ptr(self.kept), ptr(self.status), ptr(self.ws), s)
        return (self.scan_xyr, self.scan_offsets, self.submap_offsets, self.poses, self.present, self.G_posesource_laser, self.G_cam, self.images,
                self.K_raw, self.P_cam_pc)
