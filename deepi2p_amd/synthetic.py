"""Synthetic KITTI-shaped frames: no datasets are available, so bench and
tests use this seeded generator.  numpy only; nothing here touches the reference or the oracle.

Input contract mirrored: data/kitti_pc_img_pose_loader.py:431-446 (pc 3xN f32 camera frame,
intensity 1xN, sn 3xN unit normals, node_a/node_b = FPS of 1024 random points
(:416-423, data/kitti_helper.py:224-243), img 3xHxW f32 0..255, K 3x3).
"""
import math

import numpy as np
import torch


def farthest_point_sampling(pts, k, start=0):
    """pts 3xM -> k column indices; greedy max-min distance (data/kitti_helper.py:224-243)."""
    M = pts.shape[1]
    sel = np.zeros(k, dtype=np.int64)
    sel[0] = start
    d = np.full(M, np.inf)
    for i in range(1, k):
        d = np.minimum(d, np.sum((pts - pts[:, sel[i - 1]:sel[i - 1] + 1]) ** 2, axis=0))
        sel[i] = int(np.argmax(d))
    return sel


def ry_matrix(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def make_K(H, W, fx_scale=0.7):
    fx = fx_scale * W
    return np.array([[fx, 0, W / 2.0], [0, fx, H / 2.0], [0, 0, 1.0]])


def inside_mask(pc, P, K, H, W):
    """Frustum labels as evaluation/registration_lsq.py:67-84 (<= W-1, z > 0.1)."""
    cam = P[:3, :3] @ pc + P[:3, 3:4]
    px = K[0, 0] * cam[0] / cam[2] + K[0, 2]
    py = K[1, 1] * cam[1] / cam[2] + K[1, 2]
    return (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1) & (cam[2] > 0.1)


def make_scene(rng, N, r_min=2.0, r_max=80.0):
    ang = rng.uniform(-math.pi, math.pi, N)
    r = np.sqrt(rng.uniform(r_min ** 2, r_max ** 2, N))          # uniform over the annulus area
    y = rng.uniform(-2.0, 3.0, N)
    return np.stack([r * np.cos(ang), y, r * np.sin(ang)], axis=0)  # x right, y down, z forward


def make_frame(rng, N=20480, H=160, W=512, Ma=128, Mb=128, flip=0.05, with_image=True):
    """One frame: network inputs (f32) + GT pose + solver labels (exact frustum labels with `flip`
    random flips emulating classifier error)."""
    pc = make_scene(rng, N)
    yaw = rng.uniform(-math.pi, math.pi)
    t = np.array([rng.uniform(-5, 5), rng.uniform(-0.1, 0.1), rng.uniform(-10, 10)])
    P = np.eye(4)
    P[:3, :3] = ry_matrix(yaw)
    P[:3, 3] = t
    K = make_K(H, W)
    labels = inside_mask(pc, P, K, H, W).astype(np.int32)
    flips = rng.random(N) < flip
    labels_noisy = np.where(flips, 1 - labels, labels).astype(np.int32)
    sub = rng.choice(N, size=min(1024, N), replace=False)
    na = sub[farthest_point_sampling(pc[:, sub], Ma)]
    sub2 = rng.choice(N, size=min(1024, N), replace=False)
    nb = sub2[farthest_point_sampling(pc[:, sub2], Mb)]
    sn = rng.standard_normal((3, N))
    sn /= np.linalg.norm(sn, axis=0, keepdims=True)
    out = dict(pc=pc.astype(np.float32), intensity=rng.random((1, N)).astype(np.float32),
               sn=sn.astype(np.float32), node_a=np.ascontiguousarray(pc[:, na], dtype=np.float32), node_b=np.ascontiguousarray(pc[:, nb], dtype=np.float32),
               K=K, P_gt=P, yaw_gt=yaw, t_gt=t, labels_gt=labels, labels=labels_noisy)
    if with_image:
        out["img"] = rng.uniform(0, 255, (3, H, W)).astype(np.float32)
    return out


def make_batch(seed, B, **kw):
    rng = np.random.default_rng(seed)
    frames = [make_frame(rng, **kw) for _ in range(B)]
    return {k: np.ascontiguousarray(np.stack([np.asarray(f[k]) for f in frames], axis=0)) for k in frames[0]}

# ----------------------------------------------------------------------------------------
# Option bag + closed-form ("synthetic") weights: no checkpoints can be downloaded, so bench and tests use
# deterministic formula weights (SURVEY.md 8c fixture policy).  Pure data generation, no network compute.
# ----------------------------------------------------------------------------------------
class OptLike:
    """Attribute bag with the field names of kitti/options.py:6-60 used on the path."""

    def __init__(self, input_pt_num=20480, img_H=160, img_W=512, is_fine_resolution=False,
                 node_a_num=128, node_b_num=128, k_ab=16, k_interp_ab=3, k_interp_point_a=3,
                 k_interp_point_b=3, img_fine_resolution_scale=32, batch_size=8):
        self.input_pt_num = input_pt_num
        self.img_H, self.img_W = img_H, img_W
        self.is_fine_resolution = is_fine_resolution
        self.node_a_num, self.node_b_num = node_a_num, node_b_num
        self.k_ab, self.k_interp_ab = k_ab, k_interp_ab
        self.k_interp_point_a, self.k_interp_point_b = k_interp_point_a, k_interp_point_b
        self.img_fine_resolution_scale = img_fine_resolution_scale
        self.batch_size = batch_size
        self.normalization, self.activation, self.norm_momentum = "batch", "relu", 0.1
        self.gpu_ids = [0]


def state_dict_spec(opt):
    """(key, shape) list of the reference KeypointDetector state_dict, in its own order
    (networks_united.py:19-74, networks_pc.py:19-42, resnet.py:125-152)."""
    spec = []

    def pn(prefix, cin, couts, norm_last):
        c = cin
        for i, co in enumerate(couts):
            q = "%s.layers.%d" % (prefix, i)
            spec.append((q + ".conv.weight", (co, c, 1)))
            spec.append((q + ".conv.bias", (co,)))
            if i < len(couts) - 1 or norm_last:
                for s in ("weight", "bias", "running_mean", "running_var"):
                    spec.append((q + ".norm." + s, (co,)))
                spec.append((q + ".norm.num_batches_tracked", ()))
            c = co

    def c2d(prefix, cin, co):
        spec.append((prefix + ".conv.weight", (co, cin, 1, 1)))
        spec.append((prefix + ".conv.bias", (co,)))
        for s in ("weight", "bias", "running_mean", "running_var"):
            spec.append((prefix + ".norm." + s, (co,)))
        spec.append((prefix + ".norm.num_batches_tracked", ()))

    def bn(prefix, c):
        for s in ("weight", "bias", "running_mean", "running_var"):
            spec.append((prefix + "." + s, (c,)))
        spec.append((prefix + ".num_batches_tracked", ()))

    Ca, Cb, Cg = 64, 256, 512
    pn("pc_encoder.first_pointnet", 7, [Ca // 2] * 3, True)
    pn("pc_encoder.second_pointnet", Ca, [Ca, Ca], True)
    c2d("pc_encoder.knnlayer.layers_before.0", 3 + Ca, Cb)
    c2d("pc_encoder.knnlayer.layers_before.1", Cb, Cb)
    c2d("pc_encoder.knnlayer.layers_after.0", 2 * Cb, 2 * Cb)
    c2d("pc_encoder.knnlayer.layers_after.1", 2 * Cb, Cb)
    pn("pc_encoder.final_pointnet", 3 + Cb, [Cg // 2, Cg], True)
    r = "img_encoder.backbone"
    spec.append((r + ".conv1.weight", (64, 3, 7, 7)))
    bn(r + ".bn1", 64)
    inpl = 64
    for li, (planes, nb) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3)), start=1):
        for bi in range(nb):
            q = "%s.layer%d.%d" % (r, li, bi)
            spec.append((q + ".conv1.weight", (planes, inpl, 3, 3)))
            bn(q + ".bn1", planes)
            spec.append((q + ".conv2.weight", (planes, planes, 3, 3)))
            bn(q + ".bn2", planes)
            if bi == 0 and li > 1:
                spec.append((q + ".downsample.0.weight", (planes, inpl, 1, 1)))
                bn(q + ".downsample.1", planes)
            inpl = planes
    spec.append((r + ".fc.weight", (1000, 512)))
    spec.append((r + ".fc.bias", (1000,)))
    L = int(round(opt.img_H / opt.img_fine_resolution_scale)) * int(round(opt.img_W / opt.img_fine_resolution_scale))
    pn("node_b_attention_pn", 256 + 512, [256, L], False)
    pn("node_b_pn", 256 + 512 + 512 + 512, [1024, 512, 512], False)
    pn("node_a_attention_pn", 64 + 512, [256, L * 4], False)
    pn("node_a_pn", 64 + 256 + 512, [512, 128, 128], False)
    if opt.is_fine_resolution:
        pn("per_point_pn", 736, [256, 256, 2 + L], False)
    else:
        pn("per_point_pn", 736, [128, 128, 2], False)
    return spec


def synthetic_state_dict(opt, seed=0):
    """Closed-form deterministic weights (no RNG state, reproducible anywhere):
    w[i] = amp * sin(a*i + b) with per-tensor (a, b) from the tensor's ordinal.
    conv weights get He-like amplitude so activations stay O(1) through 34 layers;
    BN running_var in [0.5, 1.5], gamma in [0.8, 1.2]; small biases / means."""
    sd = {}
    for t, (key, shape) in enumerate(state_dict_spec(opt)):
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(1, dtype=torch.long)
            continue
        n = 1
        for s in shape:
            n *= s
        i = torch.arange(n, dtype=torch.float64)
        a = 0.731 + 0.0137 * ((t * 7 + seed) % 53)
        b = 0.37 * t + 0.11 * seed
        base = torch.sin(a * i + b)
        if key.endswith("conv.weight") or key.endswith(".conv1.weight") or key.endswith(".conv2.weight") \
                or key.endswith("downsample.0.weight") or key.endswith("fc.weight"):
            fan_in = n // shape[0]
            v = base * math.sqrt(3.0 / fan_in) * 1.3
        elif key.endswith("running_var"):
            v = 1.0 + 0.5 * base
        elif key.endswith("running_mean"):
            v = 0.1 * base
        elif key.endswith("norm.weight") or key.endswith("bn1.weight") or key.endswith("bn2.weight") \
                or key.endswith("downsample.1.weight"):
            v = 1.0 + 0.2 * base
        else:  # biases
            v = 0.05 * base
        sd[key] = v.to(torch.float32).reshape(shape)
    return sd


def random_state_dict(opt, seed=0):
    """He-normal weights, BN gamma in [0.9, 1.1], small biases, fresh running buffers: a freshly initialised network as the
    reference's constructors leave it (layers_pc.py:308-323, resnet.py:148-160), drawn from a seeded CPU generator (the
    training-parity fixtures use it: train-mode gradients of the closed-form weights above are ill-conditioned in fp32)."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in state_dict_spec(opt):
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(0, dtype=torch.long)
        elif key.endswith("running_var"):
            sd[key] = torch.ones(shape)
        elif key.endswith("running_mean"):
            sd[key] = torch.zeros(shape)
        elif len(shape) >= 2:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            sd[key] = torch.randn(shape, generator=gen) * math.sqrt(2.0 / fan_in)
        elif key.endswith("weight"):
            sd[key] = 1.0 + 0.2 * (torch.rand(shape, generator=gen) - 0.5)
        else:
            sd[key] = 0.1 * torch.randn(shape, generator=gen)
    return sd


# ----------------------------------------------------------------------------------------
# Raw Velodyne scans (the input of deepi2p_amd.scan_prep): no KITTI .bin files are available, so tests and
# tools/bench_scan_prep.py ray-cast an HDL-64-like sensor into a seeded scene.
# ----------------------------------------------------------------------------------------
def _ray_box(o, d, lo, hi):
    """slab test of rays o + t d (d [n,3]) against an axis-aligned box; -> entry t (inf on a miss)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0 = (lo[None] - o[None]) * inv
        t1 = (hi[None] - o[None]) * inv
    tmin = np.nanmax(np.minimum(t0, t1), axis=1)
    tmax = np.nanmin(np.maximum(t0, t1), axis=1)
    return np.where((tmax >= tmin) & (tmin > 0.0), tmin, np.inf)


def _ray_pole(o, d, cx, cy, radius, z0, z1):
    """vertical cylinder (centre cx, cy) between heights z0 and z1; -> entry t (inf on a miss)"""
    ox, oy = o[0] - cx, o[1] - cy
    a = d[:, 0] ** 2 + d[:, 1] ** 2
    bq = 2.0 * (ox * d[:, 0] + oy * d[:, 1])
    c = ox * ox + oy * oy - radius * radius
    disc = bq * bq - 4.0 * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (-bq - np.sqrt(disc)) / (2.0 * a)
    z = o[2] + t * d[:, 2]
    ok = (disc >= 0) & (t > 0) & (z >= z0) & (z <= z1)
    return np.where(ok, t, np.inf)


def make_velodyne_scan(rng, beams=64, azimuths=1800, max_range=120.0, dropout=0.03, range_sigma=0.02):
    """One raw scan in the velodyne frame (x forward, y left, z up; sensor at the origin, 1.73 m above a ground plane):
    f32[n, 4] rows (x, y, z, intensity) like a KITTI .bin, n ~ 100-130 k for the defaults.  HDL-64-like elevations from -24.8 to
    +2 degrees; the scene is the ground, a handful of boxes and poles and far walls; per-surface intensity in [0, 1], Gaussian range
    noise, randomly dropped returns and no-hit rays (nothing within max_range) removed."""
    elev = np.deg2rad(np.linspace(-24.8, 2.0, beams))
    azim = np.linspace(-np.pi, np.pi, azimuths, endpoint=False) + rng.uniform(0, 2 * np.pi / azimuths)
    ee, aa = np.meshgrid(elev, azim, indexing="ij")
    d = np.stack([np.cos(ee) * np.cos(aa), np.cos(ee) * np.sin(aa), np.sin(ee)], axis=-1).reshape(-1, 3)
    o = np.zeros(3)
    hits = [np.where(d[:, 2] < 0, -1.73 / np.minimum(d[:, 2], -1e-12), np.inf)]     # ground z = -1.73
    refl = [0.25]
    for _ in range(int(rng.integers(6, 10))):                                       # boxes: cars, buildings
        c = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40)])
        if np.hypot(*c) < 6.0:
            c *= 6.0 / max(np.hypot(*c), 1e-6)
        half = np.array([rng.uniform(0.8, 6.0), rng.uniform(0.8, 6.0)])
        hgt = rng.uniform(1.2, 8.0)
        hits.append(_ray_box(o, d, np.array([c[0] - half[0], c[1] - half[1], -1.73]), np.array([c[0] + half[0], c[1] + half[1], -1.73 + hgt])))
        refl.append(rng.uniform(0.1, 0.9))
    for _ in range(int(rng.integers(4, 9))):                                        # poles
        r = rng.uniform(5, 30)
        a = rng.uniform(-np.pi, np.pi)
        hits.append(_ray_pole(o, d, r * np.cos(a), r * np.sin(a), rng.uniform(0.08, 0.3), -1.73, rng.uniform(2.0, 6.0)))
        refl.append(rng.uniform(0.3, 1.0))
    wx, wy = rng.uniform(45, 70), rng.uniform(45, 70)                               # far walls on three sides, 10 m high
    for lo, hi in (([wx, -wy, -1.73], [wx + 1, wy, 8.27]), ([-wx - 1, wy, -1.73], [wx, wy + 1, 8.27]),
                   ([-wx - 1, -wy - 1, -1.73], [wx, -wy, 8.27])):
        hits.append(_ray_box(o, d, np.array(lo), np.array(hi)))
        refl.append(rng.uniform(0.05, 0.5))
    T = np.stack(hits, axis=1)
    which = np.argmin(T, axis=1)
    t = T[np.arange(T.shape[0]), which]
    keep = (t < max_range) & (rng.random(t.shape[0]) >= dropout)
    t, which, dk = t[keep], which[keep], d[keep]
    t = t + rng.normal(0.0, range_sigma, t.shape[0])
    pts = dk * t[:, None]
    inten = np.clip(np.asarray(refl)[which] + rng.normal(0.0, 0.05, t.shape[0]), 0.0, 1.0)
    return np.concatenate([pts, inten[:, None]], axis=1).astype(np.float32)


def make_oxford_submap(rng, n, length=100.0, half_width=8.0, far_share=0.2, max_range=50.0):
    """A push-broom sub-map as the Oxford loader stores it: f32[4, n] rows (x, y, z, intensity) in the CAMERA frame (x right, y down, z
    forward), built from a 2-D LMS-like scanner swept along z, so it is much longer (`length`, along z) than wide (+- half_width in x) and
    its points are stored in SCAN ORDER: profile after profile, ascending z -- which is why the loader shuffles before it down-samples.
    About `far_share` of the points lie beyond `max_range` in the x-z plane (the loader's horizontal range filter removes them)."""
    per = 64                                                    # points per scanner profile
    profiles = -(-n // per)
    zmax = max_range + far_share * length                        # uniform in z: the share beyond max_range is about far_share
    z0 = np.sort(rng.uniform(zmax - length, zmax, profiles))
    ang = np.linspace(-1.2, 1.2, per)
    zz = np.repeat(z0, per)[:n] + rng.normal(0.0, 0.01, n)
    a = np.tile(ang, profiles)[:n]
    road = np.abs(a) < 0.9                                       # road surface below the camera, walls at the sides
    x = np.where(road, 1.6 * np.tan(a), np.sign(a) * half_width) + rng.normal(0.0, 0.02, n)
    y = np.where(road, 1.6, 1.6 - (np.abs(a) - 0.9) * 20.0) + rng.normal(0.0, 0.02, n)
    inten = np.clip(np.where(road, 0.3, 0.6) + rng.normal(0.0, 0.05, n), 0.0, 1.0)
    return np.stack([x, y, zz, inten]).astype(np.float32)


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(4)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def make_lms_traversal(rng, submaps, scans, points_per_scan, speed=10.0, skip_threshold=0.1 / 16.0, missing=0.03, rate=50.0):
    """A stretch of an Oxford traversal as the raw stage reads it (deepi2p_amd.submap): `submaps` sub-maps of `scans` 2-D LMS profiles each
    (an int, or one count per sub-map) with up to `points_per_scan` rows (x, y, reflectance) in the LASER frame (x to the ground, the
    scan plane across the direction of travel): a road `height` below, walls at the sides, ragged row counts (returns drop out; now and
    then a profile is cut short or empty).  The vehicle (x forward, y right, z down) drives a gentle S-curve at about `speed` m/s and
    `rate` profiles per second, with stretches of every sub-map where it creeps slower than `skip_threshold` per profile; the poses are
    relative to the middle profile of each sub-map.  About `missing` of the profiles have no scan file (None).
    -> dict(submaps=[(scans, poses f64[S,4,4]), ...] (submap.pack_scans' host form), G_posesource_laser f64[4,4], G_cam f64[4,4])"""
    counts = [int(scans)] * int(submaps) if np.ndim(scans) == 0 else [int(c) for c in scans]
    # laser x (down) = vehicle z, laser y = vehicle y, laser z = - vehicle x; a small mounting error on top
    G_laser = np.array([[0.0, 0.0, -1.0, 1.6], [0.0, 1.0, 0.0, 0.05], [1.0, 0.0, 0.0, -1.1], [0.0, 0.0, 0.0, 1.0]]) @ _rot(0, 0.02) @ _rot(1, -0.015)
    # camera (x right, y down, z forward) from the vehicle frame, then the image convention of the camera model
    G_cam = np.array([[0.0, 1.0, 0.0, 0.1], [0.0, 0.0, 1.0, 1.2], [1.0, 0.0, 0.0, -1.4], [0.0, 0.0, 0.0, 1.0]]) @ _rot(2, 0.01)
    height, half_width, max_range = 1.1, 7.5, 50.0
    out = []
    for S in counts:
        step = np.full(S, speed / rate)
        for _ in range(max(1, S // 25)):                         # creeping stretches: well below the threshold per profile
            a = int(rng.integers(0, max(S - 1, 1)))
            step[a:a + int(rng.integers(2, 9))] = skip_threshold * rng.uniform(0.05, 0.45)
        dist = np.cumsum(step) - step[0]
        yaw = 0.15 * np.sin(dist / 35.0 + rng.uniform(0, 6.0))
        pitch = 0.01 * np.sin(dist / 9.0)
        xy = np.cumsum(np.stack([np.cos(yaw) * step, np.sin(yaw) * step], 1), 0)
        T = np.tile(np.eye(4), (S, 1, 1))
        for i in range(S):
            T[i] = _rot(2, yaw[i]) @ _rot(1, pitch[i])
            T[i, :3, 3] = [xy[i, 0], xy[i, 1], 0.02 * math.sin(dist[i] / 5.0)]
        origin = np.linalg.inv(T[S // 2]) if S else np.eye(4)
        poses = np.stack([origin @ T[i] for i in range(S)]) if S else np.zeros((0, 4, 4))
        prof = []
        for i in range(S):
            if rng.random() < missing:
                prof.append(None)
                continue
            n = int(points_per_scan)
            r = rng.random()
            if r < 0.04:
                n = 0
            elif r < 0.2:
                n = int(rng.integers(0, n + 1))
            ang = np.sort(rng.uniform(-2.2, 2.2, n))              # from straight down (x) past the horizon on both sides (y)
            rng_road = np.where(np.cos(ang) > 1e-3, height / np.maximum(np.cos(ang), 1e-3), np.inf)
            rng_wall = half_width / np.maximum(np.abs(np.sin(ang)), 1e-3)
            d = np.minimum(rng_road, rng_wall) + rng.normal(0.0, 0.01, n)
            keep = (d < max_range) & (rng.random(n) > 0.05)
            refl = np.rint(np.clip(np.where(rng_road < rng_wall, 60.0, 140.0) + rng.normal(0.0, 25.0, n), 0.0, 255.0))
            prof.append(np.ascontiguousarray(np.stack([d * np.cos(ang), d * np.sin(ang), refl], 1)[keep]))
        out.append((prof, poses))
    return dict(submaps=out, G_posesource_laser=G_laser, G_cam=G_cam)


def _quat_mul(a, b):
    """Hamilton product of two quaternions (w, x, y, z)"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _quat_axis(axis, a):
    q = np.zeros(4)
    q[0], q[1 + axis] = math.cos(a / 2.0), math.sin(a / 2.0)
    return q


def _quat_matrix(q, t):
    """the 4x4 of a record in fp64 (no float32 rounding: the scene is built from the exact poses)"""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    P = np.eye(4)
    P[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    P[:3, 3] = t
    return P


def make_nuscenes_sweeps(rng, B, sweeps_per_frame, rows, frame_skip=4, speed=8.0, rate=20.0, ego_share=0.04):
    """B nuScenes samples as the raw stage reads them (deepi2p_amd.sweeps): per frame `sweeps_per_frame` LiDAR sweeps (an int, or one count per
    frame; the key sweep first, then the `next` picks, then the `prev` picks, `frame_skip` sweeps of 1 / `rate` s apart) of `rows` rows (an int,
    or one count per sweep of the batch) with the five float32 columns of a .pcd.bin file (x, y, z, intensity, ring) in the LiDAR frame
    (x right, y forward, z up).  The scene is z-up and static: a road, walls along it, seen from an ego vehicle (x forward, y left, z up) that
    drives a gentle curve at about `speed` m/s a few thousand metres from the map's origin, so the float32 rounding of the pose translations
    matters.  About `ego_share` of the rows are returns on the ego car, inside the box the loader cuts out.  Every pose and calibration is a
    record (w, x, y, z, tx, ty, tz) as the data set stores it.
    -> dict(frames=[[f32[n,5], ...], ...], ego=[f64[S_b,7], ...], lidar_calib, cam_pose, cam_calib f64[B,7])"""
    counts = [int(sweeps_per_frame)] * int(B) if np.ndim(sweeps_per_frame) == 0 else [int(c) for c in sweeps_per_frame]
    n_rows = [int(rows)] * sum(counts) if np.ndim(rows) == 0 else [int(r) for r in rows]
    if len(counts) != B or len(n_rows) != sum(counts):
        raise ValueError("make_nuscenes_sweeps: one sweep count per frame and one row count per sweep")
    lidar_q = _quat_mul(_quat_axis(2, -math.pi / 2 + 0.004), _quat_mul(_quat_axis(1, 0.003), _quat_axis(0, -0.002)))
    lidar_t = np.array([0.943713, 0.0, 1.84023])
    cam_q = _quat_mul(np.array([0.5, -0.5, 0.5, -0.5]), _quat_axis(1, 0.006))          # x right, y down, z forward; a small mounting error
    cam_t = np.array([1.70079, 0.0159, 1.51095])
    origin = np.array([2100.0, 1650.0, 0.0]) + rng.uniform(-400.0, 400.0, 3) * [1, 1, 0]
    heading0 = rng.uniform(0, 2 * math.pi)

    def ego_at(time):
        """record of the ego pose `time` seconds along the drive"""
        d = speed * time
        yaw = heading0 + 0.2 * math.sin(d / 40.0)
        pos = origin + d * np.array([math.cos(heading0), math.sin(heading0), 0.0]) + 8.0 * (1 - math.cos(d / 40.0)) * np.array(
            [-math.sin(heading0), math.cos(heading0), 0.0])
        q = _quat_mul(_quat_axis(2, yaw), _quat_mul(_quat_axis(1, 0.004 * math.sin(d / 7.0)), _quat_axis(0, 0.003 * math.cos(d / 5.0))))
        return np.concatenate([q, pos + [0.0, 0.0, 0.01 * math.sin(d / 3.0)]])

    axis, side = np.array([math.cos(heading0), math.sin(heading0), 0.0]), np.array([-math.sin(heading0), math.cos(heading0), 0.0])
    frames, ego, cam_pose, k = [], [], [], 0
    for b, S in enumerate(counts):
        t0 = 2.0 + 1.5 * b
        n_next = min(S - 1, (S - 1 + 1) // 2) if S else 0
        times = [t0] + [t0 + (j + 1) * frame_skip / rate for j in range(n_next)] + [t0 - (j + 1) * frame_skip / rate for j in range(max(S - 1 - n_next, 0))]
        recs, sweeps = [], []
        for time in times[:S]:
            rec = ego_at(time)
            n = n_rows[k]
            k += 1
            world_from_lidar = _quat_matrix(rec[:4], rec[4:]) @ _quat_matrix(lidar_q, lidar_t)
            centre = world_from_lidar[:3, 3]
            n_car = int(round(ego_share * n))
            n_wall = int(0.4 * (n - n_car))
            n_road = n - n_car - n_wall
            r, az = 3.0 + 57.0 * rng.random(n_road) ** 1.5, rng.uniform(0, 2 * math.pi, n_road)
            road = centre + np.stack([r * np.cos(az), r * np.sin(az), np.zeros(n_road)], 1)
            road[:, 2] = 0.0
            along = np.dot(centre - origin, axis) + rng.uniform(-60.0, 60.0, n_wall)
            wall = origin + along[:, None] * axis + (np.where(rng.random(n_wall) < 0.5, -9.0, 17.0))[:, None] * side
            wall[:, 2] = rng.uniform(0.0, 6.0, n_wall)
            world = np.concatenate([road, wall]) + rng.normal(0.0, 0.01, (n_road + n_wall, 3))
            inv = np.linalg.inv(world_from_lidar)
            local = world @ inv[:3, :3].T + inv[:3, 3]
            car = np.stack([rng.uniform(-0.78, 0.78, n_car), rng.uniform(-2.6, 2.6, n_car), rng.uniform(-1.6, -0.4, n_car)], 1)
            pts = np.concatenate([local, car])[rng.permutation(n)] if n else np.zeros((0, 3))
            inten = np.rint(rng.uniform(0.0, 255.0, n))
            ring = rng.integers(0, 32, n).astype(np.float64)
            sweeps.append(np.ascontiguousarray(np.concatenate([pts, inten[:, None], ring[:, None]], 1).astype(np.float32)))
            recs.append(rec)
        frames.append(sweeps)
        ego.append(np.stack(recs) if recs else np.zeros((0, 7)))
        cam_pose.append(ego_at(t0 + 0.012))          # the camera frame closest in time has an ego pose of its own
    lidar_calib = np.tile(np.concatenate([lidar_q, lidar_t]), (B, 1))
    cam_calib = np.tile(np.concatenate([cam_q, cam_t]), (B, 1))
    return dict(frames=frames, ego=ego, lidar_calib=lidar_calib, cam_pose=np.stack(cam_pose) if B else np.zeros((0, 7)), cam_calib=cam_calib)


def make_camera_image(rng, H0=370, W0=1226):
    """A synthetic camera frame u8[H0, W0, 3] (HWC, as np.load gives the loader's images) that reaches every branch of the colour code:
    smooth gradients (every hue sector), per-pixel texture, saturated primaries, pure black / white, and exactly grey patches."""
    y, x = np.mgrid[0:H0, 0:W0].astype(np.float64)
    img = np.stack([127.5 + 127.5 * np.sin(x / 97.0 + y / 211.0), 127.5 + 127.5 * np.sin(x / 61.0 - y / 83.0 + 2.0),
                    127.5 + 127.5 * np.cos(x / 173.0 + y / 47.0 + 4.0)], -1)
    img += rng.normal(0.0, 12.0, img.shape)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    ph, pw = max(H0 // 8, 1), max(W0 // 16, 1)
    patches = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255), (128, 128, 128),
               (37, 37, 37), (254, 255, 254), (1, 0, 0)]
    for k, c in enumerate(patches):
        r0, c0 = int(rng.integers(0, max(H0 - ph, 1))), int(rng.integers(0, max(W0 - pw, 1)))
        img[r0:r0 + ph, c0:c0 + pw] = c
    g = rng.integers(0, 256, (ph, pw)).astype(np.uint8)          # a textured but exactly grey patch: S = 0 pixels next to each other
    img[H0 // 2:H0 // 2 + ph, W0 // 3:W0 // 3 + pw] = g[: img[H0 // 2:H0 // 2 + ph].shape[0], : img[:, W0 // 3:W0 // 3 + pw].shape[1], None]
    return img


def make_map(rng, n, length=300.0, half_width=8.0, bend=12.0, boxes=6, poses=16, camera_height=1.6):
    """A street-like LiDAR map in camera convention (x right, y DOWN, z forward; up_axis=1 for map_index.MapIndex.build), host only and
    deterministic for a given rng: ground, two walls and a few boxes along a gently curved path of `length` metres (its centre line is
    x = bend sin(pi z / length), z in [0, length]).  The rows are in SCAN ORDER, profile after profile along the path, 64 points per profile
    across it, as a push-broom traversal lays a map down.
    -> dict(points f32[n,4] rows (x, y, z, intensity), poses f64[poses,4,4] map <- camera at even steps along the path: the camera
    `camera_height` above the ground, looking along the path's tangent, s f64[poses] their arc parameter z)"""
    per = 64
    profiles = -(-n // per)
    centre = lambda z: bend * np.sin(np.pi * z / length)
    slope = lambda z: bend * np.pi / length * np.cos(np.pi * z / length)          # dx / dz of the centre line
    z0 = np.repeat(np.linspace(0.0, length, profiles), per)[:n]
    a = np.tile(np.linspace(-1.35, 1.35, per), profiles)[:n]                      # the beam's angle across the path
    road = np.abs(a) < 1.2
    lateral = np.where(road, camera_height * np.tan(a), np.sign(a) * half_width)
    y = np.where(road, camera_height, camera_height - (np.abs(a) - 1.2) * 30.0)  # y down: the walls rise towards negative y
    inten = np.where(road, 0.3, 0.6)
    # boxes: stretches of the path where one side's returns stop 3 m short of the wall, on the face of a 2 m high box
    starts = rng.uniform(0.05 * length, 0.9 * length, boxes)
    sides = rng.integers(0, 2, boxes) * 2 - 1
    for s0, side in zip(starts, sides):
        hit = (z0 >= s0) & (z0 < s0 + 4.0) & (np.sign(a) == side) & (np.abs(lateral) > half_width - 3.0)
        lateral = np.where(hit, side * (half_width - 3.0), lateral)
        y = np.where(hit, camera_height - 2.0 * rng.uniform(0.0, 1.0, n), y)
        inten = np.where(hit, 0.85, inten)
    x = centre(z0) + lateral + rng.normal(0.0, 0.02, n)
    z = z0 + rng.normal(0.0, 0.01, n)
    y = y + rng.normal(0.0, 0.02, n)
    inten = np.clip(inten + rng.normal(0.0, 0.05, n), 0.0, 1.0)
    points = np.stack([x, y, z, inten], axis=1).astype(np.float32)
    s = np.linspace(0.1 * length, 0.9 * length, poses)
    T = np.tile(np.eye(4), (poses, 1, 1))
    for k, zk in enumerate(s):
        T[k, :3, :3] = ry_matrix(math.atan2(slope(zk), 1.0))                             # camera z along the tangent (dx/dz, 0, 1)
        T[k, :3, 3] = (centre(zk), 0.0, zk)
    return dict(points=points, poses=T, s=s)
