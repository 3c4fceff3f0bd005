"""numpy restatement of csrc/sweeps.hip, value for value: every product and every sum is rounded on its own (numpy's elementwise fp64
arithmetic has no fused multiply-add), dot products run in ascending k, and the row transform is ((T0 x + T1 y) + T2 z) + T3.  The box test
is float32, as the reference's comparison of a float32 column with a Python constant is under numpy 2."""
import numpy as np

BOX = (0.8, 2.7)
MAX_FRAME_POINTS = 1 << 20


def sweep_picks(available, frame_num=3, frame_skip=4):
    """distances from the key sweep of one direction's picks"""
    return [k * frame_skip for k in range(1, frame_num + 1) if k * frame_skip <= available]


def pose_matrices(records):
    """[n,7] (w, x, y, z, tx, ty, tz) -> f64[n,4,4] with float32-valued rotation and translation"""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, 7)
    w, x, y, z = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = np.stack([1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
                  2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
                  2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)], 1).reshape(-1, 3, 3)
    P = np.tile(np.eye(4), (len(rec), 1, 1))
    P[:, :3, :3] = R.astype(np.float32)
    P[:, :3, 3] = rec[:, 4:].astype(np.float32)
    return P


def mul44(A, B):
    """row-major 4x4 product, ascending k"""
    C = A[:, 0:1] * B[0:1, :]
    for k in range(1, 4):
        C = C + A[:, k:k + 1] * B[k:k + 1, :]
    return C


def inv_affine(A):
    """adj(M) / det(M), then -(M^-1 . t); the last row of A is not read"""
    c = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[i, j] = A[i1, j1] * A[i2, j2] - A[i1, j2] * A[i2, j1]
    det = (A[0, 0] * c[0, 0] + A[0, 1] * c[0, 1]) + A[0, 2] * c[0, 2]
    Ai = np.eye(4)
    for i in range(3):
        for j in range(3):
            Ai[i, j] = c[j, i] / det
        Ai[i, 3] = -((Ai[i, 0] * A[0, 3] + Ai[i, 1] * A[1, 3]) + Ai[i, 2] * A[2, 3])
    return Ai


def sweep_transforms(P_ego, frame_offsets, P_vehicle_lidar, P_ego_cam, P_vehicle_cam):
    """-> (T f64[S,4,4], P_cam_pc f64[B,4,4]) for valid frame offsets"""
    S, B = len(P_ego), len(frame_offsets) - 1
    T, Pcp = np.zeros((S, 4, 4)), np.zeros((B, 4, 4))
    for b in range(B):
        s0, s1 = int(frame_offsets[b]), int(frame_offsets[b + 1])
        if s1 == s0:
            continue
        vl = P_vehicle_lidar[b]
        Pcp[b] = mul44(inv_affine(P_vehicle_cam[b]), mul44(inv_affine(P_ego_cam[b]), mul44(P_ego[s0], vl)))
        T[s0] = np.eye(4)
        for s in range(s0 + 1, s1):
            T[s] = mul44(mul44(inv_affine(vl), mul44(inv_affine(P_ego[s0]), P_ego[s])), vl)
    return T, Pcp


def keep_mask(rows, box=BOX):
    x, y = rows[:, 0].astype(np.float32), rows[:, 1].astype(np.float32)
    bx, by = np.float32(box[0]), np.float32(box[1])
    inside = (x < bx) & (x > -bx) & (y < by) & (y > -by)
    return ~inside


def transform_rows(T, rows):
    """f32 rows [n, >=4] -> (f32[n,4], f64[n,3]): the coordinates in fp64, in the kernel's order, and rounded once"""
    x, y, z = (rows[:, k].astype(np.float64) for k in range(3))
    p64 = np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], 1)
    return np.concatenate([p64.astype(np.float32), rows[:, 3:4].astype(np.float32)], 1), p64


def accumulate(rows, sweep_offsets, frame_offsets, T, box=BOX, max_frame_points=MAX_FRAME_POINTS, cap=None):
    """-> dict(points f32[total,4], points64 f64[total,3] (the key sweep's rows as they are), offsets i32[B+1], kept i32[S], status i32[B])"""
    rows = np.asarray(rows)
    S, B, P = len(sweep_offsets) - 1, len(frame_offsets) - 1, len(rows)
    cap = P if cap is None else cap
    kept, status, off = np.zeros(S, np.int32), np.zeros(B, np.int32), np.zeros(B + 1, np.int32)
    out, out64 = [], []
    frames_ok = True
    for b in range(B):
        s0, s1 = int(frame_offsets[b]), int(frame_offsets[b + 1])
        frames_ok = frames_ok and 0 <= s0 <= s1 <= S and (b > 0 or s0 == 0)
        ok = frames_ok and all(0 <= sweep_offsets[s] <= sweep_offsets[s + 1] <= P for s in range(s0, s1))
        off[b + 1] = off[b]
        if not ok:
            status[b] = 3
            continue
        parts, parts64 = [], []
        for s in range(s0, s1):
            r = rows[sweep_offsets[s]:sweep_offsets[s + 1], :4]
            r = r[keep_mask(r, box)]
            kept[s] = len(r)
            if s == s0:
                parts.append(r.astype(np.float32))
                parts64.append(r[:, :3].astype(np.float64))
            else:
                p, p64 = transform_rows(T[s], r)
                parts.append(p)
                parts64.append(p64)
        n = int(kept[s0:s1].sum())
        if n > max_frame_points or off[b] + n > cap:
            status[b] = 1
        elif n == 0:
            status[b] = 4
        else:
            out += parts
            out64 += parts64
            off[b + 1] = off[b] + n
    points = np.concatenate(out) if out else np.zeros((0, 4), np.float32)
    points64 = np.concatenate(out64) if out64 else np.zeros((0, 3))
    return dict(points=points, points64=points64, offsets=off, kept=kept, status=status)


U53 = 2.0 ** -53
K_INVERSE, K_PRODUCT = 13, 4


def gamma(k):
    return k * U53 / (1.0 - k * U53)


def chain_bounds(P_ego, frame_offsets, P_vehicle_lidar, P_ego_cam, P_vehicle_cam):
    """Componentwise fp64 bounds on T and P_cam_pc as csrc/sweeps.hip computes them: gamma_k times the product of the absolute matrices of
    the chain, -> (k, bound_T [S,4,4], bound_P_cam_pc [B,4,4]).

    k counts the roundings on the longest path of the kernel's arithmetic.  A 4x4 product: one product and three sums per entry, 4.  An
    inverse: a cofactor is two products and a difference (3); the determinant adds a product and two sums (6); an entry of M^-1 is a cofactor
    over the determinant (3 + 6 + 1 = 10); a translation entry -(M^-1 . t) adds a product and two sums: 13.  A computed inverse X of A
    carries its rounding error as X dA X with |dA| <= gamma |A|, so its place in the product of absolute matrices is |X| |A| |X| (which is
    at least |X|).  Both chains are two inverses and three products: k = 2 * 13 + 3 * 4 = 38."""
    k = 2 * K_INVERSE + 3 * K_PRODUCT
    a = np.abs
    inv_abs = lambda A: a(np.linalg.inv(A)) @ a(A) @ a(np.linalg.inv(A))
    S, B = len(P_ego), len(frame_offsets) - 1
    bT, bP = np.zeros((S, 4, 4)), np.zeros((B, 4, 4))
    for b in range(B):
        s0, s1 = int(frame_offsets[b]), int(frame_offsets[b + 1])
        if s1 == s0:
            continue
        vl = P_vehicle_lidar[b]
        bP[b] = gamma(k) * (inv_abs(P_vehicle_cam[b]) @ inv_abs(P_ego_cam[b]) @ a(P_ego[s0]) @ a(vl))
        for s in range(s0 + 1, s1):
            bT[s] = gamma(k) * (inv_abs(vl) @ inv_abs(P_ego[s0]) @ a(P_ego[s]) @ a(vl))
    return k, bT, bP
