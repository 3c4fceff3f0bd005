"""The maps and frames the map localisation tests share (tests/test_map_index_host.py, tests/test_gpu_map_index.py,
tests/test_gpu_map_executor.py); host only.

grid_map: about 6 k rows on a 5 x 4 grid of 4 m cells whose coordinates are multiples of 2^-6, so is every centre and radius of
grid_frames: dx dx + dy dy and r r are then exact in fp64 and the keep rule gives the same answer in any operation order.  The map holds one
cell with about 700 rows (eleven 64-row wave iterations), one empty cell, rows exactly on cell borders and on the grid's low corner, and the
pair (3, 4) / (3 - 2^-6, 4) on the ground plane: at distance exactly 5 and just inside it from the centre (0, 0).

street: synthetic.make_map's street of about 40 k rows with the batches of priors the executor tests submit."""
import numpy as np

from deepi2p_amd import synthetic
from tests import map_index_oracle as oracle

Q = 2.0 ** -6
CELL, NX, NY, ORIGIN = 4.0, 5, 4, (-8.0, -8.0)
DENSE, EMPTY = (2, 2), (4, 0)          # (ix, iy) of the cell with about 700 rows and of the one without any
ON_CIRCLE, INSIDE_CIRCLE = (3.0, 4.0), (3.0 - Q, 4.0)


def _place(g0, g1, h, inten, up_axis):
    a, b = oracle.ground_axes(up_axis)
    p = np.zeros((len(g0), 4), np.float32)
    p[:, a], p[:, b], p[:, up_axis], p[:, 3] = g0, g1, h, inten
    return p


def grid_map(up_axis=1, seed=5):
    """f32[M,4] rows in a shuffled order (so that `order` is no identity anywhere)"""
    rng = np.random.default_rng(seed)
    n = 5600
    g0 = ORIGIN[0] + rng.integers(0, NX * 256, n) * Q
    g1 = ORIGIN[1] + rng.integers(0, NY * 256, n) * Q
    ix, iy = np.floor((g0 - ORIGIN[0]) / CELL), np.floor((g1 - ORIGIN[1]) / CELL)
    free = ~((ix == EMPTY[0]) & (iy == EMPTY[1])) & ~((ix == DENSE[0]) & (iy == DENSE[1]))
    g0, g1 = g0[free], g1[free]
    d0 = ORIGIN[0] + DENSE[0] * CELL + rng.integers(0, 256, 700) * Q
    d1 = ORIGIN[1] + DENSE[1] * CELL + rng.integers(0, 256, 700) * Q
    # rows exactly on cell borders (they belong to the cell that starts there) and on the grid's low corner
    b0 = np.array([ORIGIN[0], -4.0, 0.0, 0.0, 4.0, 8.0, 4.0, 0.5])
    b1 = np.array([ORIGIN[1], -4.0, 0.0, 1.0, 4.0, 4.0, -8.0, 2.0])
    s0, s1 = np.array([ON_CIRCLE[0], INSIDE_CIRCLE[0]]), np.array([ON_CIRCLE[1], INSIDE_CIRCLE[1]])
    g0, g1 = np.concatenate([g0, d0, b0, s0]), np.concatenate([g1, d1, b1, s1])
    h = rng.integers(-128, 128, len(g0)) * Q
    inten = rng.random(len(g0))
    p = _place(g0, g1, h, inten, up_axis)
    return p[rng.permutation(len(p))]


def rotation(kind, up_axis, seed=3):
    """3x3: "identity", "quarter" (a quarter turn about the up axis: the transform stays exact) or "generic" (a random rotation)"""
    if kind == "identity":
        return np.eye(3)
    if kind == "quarter":
        a, b = oracle.ground_axes(up_axis)
        R = np.zeros((3, 3))
        R[up_axis, up_axis] = 1.0
        R[a, b], R[b, a] = -1.0, 1.0
        return R
    q = np.random.default_rng(seed).standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def prior(centre, up_axis, R=None, height=0.25):
    a, b = oracle.ground_axes(up_axis)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) if R is None else R
    T[a, 3], T[b, 3], T[up_axis, 3] = centre[0], centre[1], height
    return T


def grid_frames(up_axis=1, kind="identity"):
    """B = 4: a disc inside the dense cell, a disc that covers the grid and passes it on all four sides, a disc off the grid (status 4), a
    NaN prior (status 5) -> (T_map_prior f64[4,4,4], radius f64[4])"""
    R = rotation(kind, up_axis)
    T = np.stack([prior((2.0, 2.0), up_axis, R), prior((2.0, 0.0), up_axis, R), prior((100.0, 100.0), up_axis, R), prior((1.0, 1.0), up_axis, R)])
    T[3, 1, 2] = np.nan
    return T, np.array([1.5, 40.0, 5.0, 3.0])


def grid_index(up_axis=1):
    return oracle.build(grid_map(up_axis), CELL, up_axis, ORIGIN, NX, NY)


# ---------------------------------------------------------------------------------------------------------------- the executor's street
STREET_ROWS, STREET_B, STREET_CELL = 40000, 2, 8.0
STREET_RADIUS, STREET_MFP = 30.0, 16384          # a 30 m disc of the 300 m street holds about 8 k of its rows
STREET_CAP = STREET_B * STREET_MFP
OFF_MAP = np.array([5000.0, 0.0, 5000.0])        # where a test puts a prior off the map on purpose


def street():
    return synthetic.make_map(np.random.default_rng(21), STREET_ROWS)


def _perturbed(rng, T_map_cam, shift=1.0, yaw=0.1):
    """a prior: the true pose moved by up to `shift` metres on the ground plane and turned by up to `yaw` radians about y"""
    T = np.array(T_map_cam)
    D = np.eye(4)
    D[:3, :3] = synthetic.ry_matrix(float(rng.uniform(-yaw, yaw)))
    D[0, 3], D[2, 3] = rng.uniform(-shift, shift, 2)
    return T @ D


def street_batches(world=None, off_map=()):
    """three batches of STREET_B frames with different poses, priors, radii and seeds -> list of dict(T_map_prior, radius, T_map_cam_gt, seed);
    off_map: (batch, frame) pairs whose prior is moved off the map"""
    world = street() if world is None else world
    rng = np.random.default_rng(77)
    out = []
    for i, (picks, radius) in enumerate((((3, 9), STREET_RADIUS), ((12, 5), np.array([25.0, 28.0])), ((1, 14), 22.0))):
        gt = world["poses"][list(picks)]
        T = np.stack([_perturbed(rng, g) for g in gt])
        for bi, f in off_map:
            if bi == i:
                T[f, :3, 3] = OFF_MAP
        out.append(dict(T_map_prior=T, radius=radius, T_map_cam_gt=gt, seed=90 + i))
    return out
