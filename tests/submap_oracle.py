"""numpy restatement of csrc/submap.hip (stages A-C and E of deepi2p_amd.submap), with the operation order written out: every product and
sum below is one IEEE fp64 operation (numpy's elementwise arithmetic never fuses), in the order the kernels use.  The voxel pass between
them is tests/scan_prep_oracle.voxel_down_sample.  tests/test_submap_host.py pins this file against the reference's own
my_build_pointcloud / downsample (tests/golden/submap_golden.npz)."""
import numpy as np

from tests import scan_prep_oracle as spo

ST_OK, ST_TOO_MANY, ST_OFFSETS, ST_EMPTY = 0, 1, 3, 4


def keep_chain(poses, present, skip_threshold):
    """-> (kept i32[S]: 1 kept, 0 skipped, -1 missing; skip_count).  Skipped iff a previous KEPT profile exists and
    |R_prev^T (t - t_prev)|^2 < skip_threshold^2 (squares compared; sums in ascending index)."""
    S = len(poses)
    kept = np.full(S, -1, np.int32)
    prev, skipped = None, 0
    thr2 = None if skip_threshold is None else np.float64(skip_threshold) * np.float64(skip_threshold)
    for s in range(S):
        if present is not None and not present[s]:
            continue
        P = np.asarray(poses[s], dtype=np.float64)
        if prev is not None and thr2 is not None:
            d = [P[0, 3] - prev[0, 3], P[1, 3] - prev[1, 3], P[2, 3] - prev[2, 3]]
            n2 = np.float64(0.0)
            for i in range(3):
                e = (prev[0, i] * d[0] + prev[1, i] * d[1]) + prev[2, i] * d[2]
                n2 = n2 + e * e
            if n2 < thr2:
                kept[s] = 0
                skipped += 1
                continue
        kept[s] = 1
        prev = P
    return kept, skipped


def pose_times_G(P, G):
    """M[i][j] = sum_k P[i][k] G[k][j], k ascending, the first product not added to a zero"""
    M = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            a = P[i, 0] * G[0, j]
            for k in range(1, 4):
                a = a + P[i, k] * G[k, j]
            M[i, j] = a
    return M


def transform_rows(M, x, y):
    """p = (M[:,0] x + M[:,1] y) + M[:,3] for arrays x, y -> f64[n,3]"""
    return np.stack([(M[i, 0] * x + M[i, 1] * y) + M[i, 3] for i in range(3)], 1)


def build_raw(scan_xyr, scan_offsets, submap_offsets, poses, present, G, skip_threshold=None, ground_threshold=None, max_frame_points=1 << 20,
              cap=None):
    """-> dict(points f32[total,4], points64 f64[total,3], offsets i32[B+1], kept i32[S], skip_count i32[B], status i32[B])"""
    xyr = np.asarray(scan_xyr, dtype=np.float64)
    so, mo = np.asarray(scan_offsets, dtype=np.int64), np.asarray(submap_offsets, dtype=np.int64)
    poses, G = np.asarray(poses, dtype=np.float64), np.asarray(G, dtype=np.float64)
    S_cap, P_cap, B = poses.shape[0], xyr.shape[0], len(mo) - 1
    cap = P_cap if cap is None else cap
    remove_ground = ground_threshold is not None and ground_threshold > -1
    kept = np.full(S_cap, -1, np.int32)
    skip_count, status, offsets = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B + 1, np.int32)
    rows64, rows32 = [], []
    for b in range(B):
        head = mo[:b + 2]
        ok = head[0] == 0 and np.all(head >= 0) and np.all(np.diff(head) >= 0) and np.all(head <= S_cap)
        if ok:
            s0, s1 = int(mo[b]), int(mo[b + 1])
            lo, hi = so[s0:s1], so[s0 + 1:s1 + 1]
            ok = bool(np.all(lo >= 0) and np.all(hi >= lo) and np.all(hi <= P_cap))
        offsets[b + 1] = offsets[b]
        if not ok:
            status[b] = ST_OFFSETS
            continue
        kept[s0:s1], skip_count[b] = keep_chain(poses[s0:s1], None if present is None else present[s0:s1], skip_threshold)
        parts64, refl = [], []
        for s in range(s0, s1):
            if kept[s] != 1:
                continue
            rows = xyr[so[s]:so[s + 1]]
            if remove_ground:
                rows = rows[rows[:, 0] < np.float64(ground_threshold)]
            parts64.append(transform_rows(pose_times_G(poses[s], G), rows[:, 0], rows[:, 1]))
            refl.append(rows[:, 2])
        n = sum(len(p) for p in parts64)
        if n > max_frame_points or offsets[b] + n > cap:
            status[b] = ST_TOO_MANY
        elif n == 0:
            status[b] = ST_EMPTY
        else:
            p64 = np.concatenate(parts64)
            rows64.append(p64)
            rows32.append(np.concatenate([p64.astype(np.float32), np.concatenate(refl).astype(np.float32)[:, None]], 1))
            offsets[b + 1] = offsets[b] + n
    points = np.concatenate(rows32) if rows32 else np.zeros((0, 4), np.float32)
    points64 = np.concatenate(rows64) if rows64 else np.zeros((0, 3))
    return dict(points=points, points64=points64, offsets=offsets, kept=kept, skip_count=skip_count, status=status)


def to_camera(cen, intensity, G_cam):
    """q = ((G[i,0] x + G[i,1] y) + G[i,2] z) + G[i,3] in fp64, rounded once -> f32[m,4] (q, intensity)"""
    cen, G = np.asarray(cen, dtype=np.float64).reshape(-1, 3), np.asarray(G_cam, dtype=np.float64)
    x, y, z = cen[:, 0], cen[:, 1], cen[:, 2]
    q = np.stack([((G[i, 0] * x + G[i, 1] * y) + G[i, 2] * z) + G[i, 3] for i in range(3)], 1)
    return np.concatenate([q.astype(np.float32), np.asarray(intensity, np.float32).reshape(-1, 1)], 1)


def build_submaps(scan_xyr, scan_offsets, submap_offsets, poses, present, G, G_cam, skip_threshold=None, ground_threshold=None, voxel=0.1,
                  max_frame_points=1 << 20):
    """-> dict(record f32[total,4], offsets i32[B+1], voxel_counts i32[B], status i32[B]) + build_raw's kept / skip_count"""
    raw = build_raw(scan_xyr, scan_offsets, submap_offsets, poses, present, G, skip_threshold, ground_threshold, max_frame_points)
    B = len(raw["status"])
    G_cam = np.asarray(G_cam, dtype=np.float64)
    G_cam = np.tile(G_cam, (B, 1, 1)) if G_cam.ndim == 2 else G_cam
    recs, offsets = [], np.zeros(B + 1, np.int32)
    for b in range(B):
        v = spo.voxel_down_sample(raw["points"][raw["offsets"][b]:raw["offsets"][b + 1]], voxel)
        recs.append(to_camera(v["cen"], v["intensity"], G_cam[b]))
        offsets[b + 1] = offsets[b] + len(recs[-1])
    return dict(record=np.concatenate(recs) if recs else np.zeros((0, 4), np.float32), offsets=offsets, voxel_counts=np.diff(offsets).astype(np.int32),
                status=raw["status"], kept=raw["kept"], skip_count=raw["skip_count"])
