"""numpy restatement of the training-sample preparation (deepi2p_amd/sample_prep.py, csrc/sample_prep.hip).

Colour: the four operations of torchvision's ColorJitter on PIL images (ImageEnhance.Brightness / Contrast / Color = Image.blend with a
black / mean-grey / per-pixel-grey image, and the HSV round trip of adjust_hue), restated from PIL's behaviour and pinned against PIL
itself by tests/golden/sample_prep_golden.npz.  Resize: the rounded 2x2 mean (OpenCV INTER_LINEAR at an exact factor of two) -- restated
only, OpenCV is not available.  Geometry, pose bookkeeping, jitter and accumulation follow data/kitti_pc_img_pose_loader.py; the draws
follow csrc/sample_prep.hip (Philox stream tags 4 and 5) word for word."""
import math

import numpy as np

from oracle import rng_np

MODES = {"train": 0, "val": 1, "val_random_Ry": 2}
TAG_DRAWS, TAG_JITTER = 4, 5
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
# columns of the integer draw table i32[B, 8] and of the factor table f32[B, 4]
I_DX, I_DY, I_FLIP, I_OP0, I_HUE_SHIFT = 0, 1, 2, 3, 7
P_CAM_NWU = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=np.float64)
P_NWU_CAM = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)
PERMS = [p for p in __import__("itertools").permutations(range(4))]          # lexicographic: index = the draw's floor(24 u)


# ---------------------------------------------------------------------------------------------------------------- colour
def grey(rgb):
    """PIL's RGB -> L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    c = rgb.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(d, p, factor):
    """Image.blend(degenerate, image, factor): float32, multiply and add rounded separately, clipped, truncated."""
    f = np.float32(factor)
    d32 = np.asarray(d).astype(np.float32)
    t = d32 + f * (p.astype(np.float32) - d32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.uint8)


def grey_mean(rgb):
    """ImageEnhance.Contrast: int(mean of L + 0.5)"""
    L = grey(rgb)
    return int(float(L.astype(np.int64).sum()) / L.size + 0.5)


def rgb_to_hsv(rgb):
    r, g, b = [rgb[..., k].astype(np.int64) for k in range(3)]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    cr = np.maximum(maxc - minc, 1).astype(np.float32)
    s = cr / np.maximum(maxc, 1).astype(np.float32)
    rc, gc, bc = [((maxc - c).astype(np.float32) / cr) for c in (r, g, b)]
    h = np.where(r == maxc, (bc - gc).astype(np.float64),
                 np.where(g == maxc, 2.0 + rc.astype(np.float64) - bc.astype(np.float64), 4.0 + gc.astype(np.float64) - rc.astype(np.float64)))
    h = np.fmod(h.astype(np.float32).astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    flat = maxc == minc
    return np.stack([np.where(flat, 0, uh), np.where(flat, 0, us), maxc], -1).astype(np.uint8)


def _round(x):
    return np.floor(x + 0.5)          # C round() for x >= 0


def hsv_to_rgb(hsv):
    h, s, v = [hsv[..., k].astype(np.float32).astype(np.float64) for k in range(3)]
    h6 = h * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(np.float32).astype(np.float64)
    fs = (s / 255.0).astype(np.float32).astype(np.float64)
    p = np.clip(_round(v * (1.0 - fs)), 0, 255)
    q = np.clip(_round(v * (1.0 - fs * f)), 0, 255)
    t = np.clip(_round(v * (1.0 - fs * (1.0 - f))), 0, 255)
    k = i.astype(np.int64) % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    out = np.stack([r, g, b], -1)
    return np.where((hsv[..., 1] == 0)[..., None], hsv[..., 2:3].astype(np.float64), out).astype(np.uint8)


def hue_shift_of(hue):
    """torchvision's np.uint8(hue_factor * 255): truncation towards zero, then wrap-around"""
    return int(float(hue) * 255.0) & 255


def adjust_hue(rgb, shift):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + int(shift)) & 255
    return hsv_to_rgb(hsv)


def apply_op(rgb, op, factors, shift, mean=None):
    if op == OP_BRIGHTNESS:
        return blend(np.float32(0), rgb, factors[0])
    if op == OP_CONTRAST:
        return blend(np.float32(grey_mean(rgb) if mean is None else mean), rgb, factors[1])
    if op == OP_SATURATION:
        return blend(grey(rgb)[..., None], rgb, factors[2])
    return adjust_hue(rgb, shift)


def color_jitter(rgb, order, factors, shift):
    """rgb u8[H,W,3] -> (u8[H,W,3], the grey sum the contrast operation saw)"""
    gsum = 0
    for op in order:
        if op == OP_CONTRAST:
            gsum = int(grey(rgb).astype(np.int64).sum())
        rgb = apply_op(rgb, int(op), factors, shift)
    return rgb, gsum


# ---------------------------------------------------------------------------------------------------------------- geometry
def scaled_size(H0, W0, top, scale):
    return int(round((H0 - top) * scale)), int(round(W0 * scale))


def resize(img, scale):
    """scale 0.5 on even dimensions: (a + b + c + d + 2) >> 2; scale 1.0: identity"""
    if scale == 1.0:
        return img
    assert scale == 0.5 and img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0
    a = img.astype(np.int64)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def camera_matrix(K, top, scale, dx, dy):
    K = np.array(K, dtype=np.float64)
    K[1, 2] -= top
    K = scale * K
    K[2, 2] = 1
    K[0, 2] -= dx
    K[1, 2] -= dy
    return K


def prepare_image(img_u8, top, scale, img_H, img_W, ints, factors, color=True):
    """One frame: u8[H0,W0,3] + its rows of the draw tables -> (f32[3,img_H,img_W], grey sum of the contrast operation)"""
    dx, dy, flip = int(ints[I_DX]), int(ints[I_DY]), int(ints[I_FLIP])
    win = resize(img_u8[top:], scale)[dy:dy + img_H, dx:dx + img_W]
    gsum = 0
    if color:
        win, gsum = color_jitter(win, [int(o) for o in ints[I_OP0:I_OP0 + 4]], factors, int(ints[I_HUE_SHIFT]))
    if flip:
        win = win[:, ::-1]
    return np.ascontiguousarray(win.astype(np.float32).transpose(2, 0, 1)), gsum


# ---------------------------------------------------------------------------------------------------------------- draws
def _uniforms(seed, frames, blocks):
    """u f64[len(frames), 2 * blocks]: block k of frame b is Philox counter (b, k, 0, TAG_DRAWS), two 53-bit uniforms per block"""
    b = np.asarray(frames, dtype=np.uint64)
    out = []
    for k in range(blocks):
        r = rng_np.philox4x32_10(b, np.full_like(b, k), np.zeros_like(b), np.full_like(b, TAG_DRAWS), seed & rng_np.MASK, (seed >> 32) & rng_np.MASK)
        out += [rng_np.u53(r[0], r[1]), rng_np.u53(r[2], r[3])]
    return np.stack(out, 1)


def rotation(angles):
    """Rz . Ry . Rx (augmentation.angles2rotation_matrix)"""
    cx, sx, cy, sy, cz, sz = np.cos(angles[0]), np.sin(angles[0]), np.cos(angles[1]), np.sin(angles[1]), np.cos(angles[2]), np.sin(angles[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.dot(Rz, np.dot(Ry, Rx))


def random_pose(angles, t, flip):
    """generate_random_transform's matrix from its six draws, times P_flip = diag(-1, 1, 1, 1) when flipped"""
    Pr = np.identity(4)
    Pr[0:3, 0:3] = rotation(angles)
    Pr[0:3, 3] = t
    if flip:
        Pr = np.dot(Pr, np.diag([-1.0, 1.0, 1.0, 1.0]))
    return Pr


def checksum(a):
    """64-bit position-weighted checksum of a uint8 array (wraps modulo 2^64)"""
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1).astype(np.uint64)
    w = (np.arange(a.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(11) | np.uint64(1)
    with np.errstate(over="ignore"):
        return np.uint64(((a + np.uint64(1)) * w).sum(dtype=np.uint64))


def all_colours():
    """u8[4096, 4096, 3]: every RGB colour once, colour index = (R << 16 | G << 8 | B) in row-major order"""
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def colour_subsample():
    """65 536 colour indices at stride 255: every channel varies"""
    return np.arange(65536, dtype=np.int64) * 255


def rigid_inverse(P):
    """[R | t]^-1 = [R^T | -R^T t] for orthogonal R (det -1 after the mirror flip included)"""
    out = np.eye(4)
    out[:3, :3] = P[:3, :3].T
    out[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
    return out


def assemble_pose(Pr, Pc, Pji):
    """-> (Pr . P_cam_nwu f64[4,4], P = Pji . Pc . P_nwu_cam . Pr^-1 f32[3,4]) in the reference's association order"""
    P = np.dot(Pji, np.dot(Pc, np.dot(P_NWU_CAM, rigid_inverse(Pr))))
    return np.dot(Pr, P_CAM_NWU), P[:3].astype(np.float32)


def sample_draws(seed, frames, mode, K, Pc, Pji, o):
    """The draw tables of di2p_sample_draws for the given frame indices.  o: dict(top, scale, img_H, img_W, Hs, Ws, amp[6] = tx ty tz Rx Ry Rz,
    ranges[4][2]).  -> dict(ints i32[n,8], factors f32[n,4], Pr, PrPcn f64[n,4,4], P f32[n,3,4], K f32[n,3,3], u f64[n,14])"""
    n = len(frames)
    u = _uniforms(seed, frames, 7)
    ints, fac = np.zeros((n, 8), np.int32), np.ones((n, 4), np.float32)
    Pr_all, PrPcn, P_all, K_all = np.zeros((n, 4, 4)), np.zeros((n, 4, 4)), np.zeros((n, 3, 4), np.float32), np.zeros((n, 3, 3), np.float32)
    m = MODES[mode]
    for j in range(n):
        nx, ny = o["Ws"] - o["img_W"] + 1, o["Hs"] - o["img_H"] + 1
        if m == 0:
            dx, dy = min(int(u[j, 0] * nx), nx - 1), min(int(u[j, 1] * ny), ny - 1)
            flip = 1 if u[j, 2] > 0.5 else 0
            order = PERMS[min(int(u[j, 3] * 24), 23)]
            f = [o["ranges"][k][0] + (o["ranges"][k][1] - o["ranges"][k][0]) * u[j, 4 + k] for k in range(4)]
            t = [o["amp"][k] * (2.0 * u[j, 8 + k] - 1.0) for k in range(3)]
            ang = [o["amp"][3 + k] * (2.0 * u[j, 11 + k] - 1.0) for k in range(3)]
        else:
            dx, dy, flip, order, f = int((o["Ws"] - o["img_W"]) / 2), int((o["Hs"] - o["img_H"]) / 2), 0, (0, 1, 2, 3), [1.0, 1.0, 1.0, 0.0]
            t, ang = [0.0, 0.0, 0.0], [0.0, (2.0 * math.pi) * (2.0 * u[j, 12] - 1.0) if m == 2 else 0.0, 0.0]
        ints[j] = [dx, dy, flip, order[0], order[1], order[2], order[3], hue_shift_of(f[3])]
        fac[j] = f
        Pr = random_pose(ang, t, flip)
        Pr_all[j] = Pr
        PrPcn[j], P_all[j] = assemble_pose(Pr, Pc[j], Pji[j])
        K_all[j] = camera_matrix(K[j], o["top"], o["scale"], dx, dy).astype(np.float32)
    return dict(ints=ints, factors=fac, Pr=Pr_all, PrPcn=PrPcn, P=P_all, K=K_all, u=u)


# ---------------------------------------------------------------------------------------------------------------- jitter
def jitter_noise(seed, frame, n_out, sigma, clip, stream_id=0):
    """f32[2, 3, n_out] (points, normals): element (which, c, n) from Philox counter (n, frame, stream_id * 8 + which * 4 + c, TAG_JITTER),
    Box-Muller (cosine branch) in fp64, clipped, rounded to float32.  Also returns the two uniforms."""
    n = np.arange(n_out, dtype=np.uint64)
    out, us = np.zeros((2, 3, n_out), np.float32), np.zeros((2, 3, n_out, 2))
    for w in range(2):
        for c in range(3):
            r = rng_np.philox4x32_10(n, np.full_like(n, frame), np.full_like(n, stream_id * 8 + w * 4 + c), np.full_like(n, TAG_JITTER),
                                     seed & rng_np.MASK, (seed >> 32) & rng_np.MASK)
            u1, u2 = rng_np.u53(r[0], r[1]), rng_np.u53(r[2], r[3])
            z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925 * u2)
            out[w, c] = np.clip(sigma * z, -clip, clip).astype(np.float32)
            us[w, c, :, 0], us[w, c, :, 1] = u1, u2
    return out, us


def jitter_from_normals(z, sigma, clip):
    """augmentation.jitter_point_cloud's noise from standard normals: clip(sigma * z, +-clip) cast to float32"""
    return np.clip(sigma * np.asarray(z, dtype=np.float64), -1 * clip, clip).astype(np.float32)


def jitter(x, noise):
    """the reference casts the noise to float32, then adds: float32 + float32"""
    return (noise.astype(np.float32) + x.astype(np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- accumulation
def accumulation_transform(Pc, P_oi, P_oj):
    """Pc^-1 . (P_oi^-1 . P_oj) . Pc in the dtypes given: float32 poses reproduce the reference (which casts the poses it reads from disk to
    float32, so its two pose inverses and their product are float32), fp64 poses give what deepi2p_amd.sample_prep computes"""
    return np.dot(np.linalg.inv(Pc), np.dot(np.dot(np.linalg.inv(P_oi), P_oj), Pc))


def transform_segments(points4, normals, seg_offsets, T):
    """points f32[total,4], normals f32[total,3]: segment s by T[s] (normals by its rotation), fp64 in the kernel's order, rounded once"""
    p_out, n_out = points4.copy(), normals.copy()
    for s in range(len(seg_offsets) - 1):
        a, b = seg_offsets[s], seg_offsets[s + 1]
        M = np.asarray(T[s], dtype=np.float64)
        p, q = points4[a:b, :3].astype(np.float64), normals[a:b].astype(np.float64)
        for r in range(3):
            p_out[a:b, r] = (((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]).astype(np.float32)
            n_out[a:b, r] = ((M[r, 0] * q[:, 0] + M[r, 1] * q[:, 1]) + M[r, 2] * q[:, 2]).astype(np.float32)
    return p_out, n_out
