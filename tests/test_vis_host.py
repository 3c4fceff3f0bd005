"""CPU: the host side of the result overlays.  tests/golden/vis_golden.npz holds what the REFERENCE's three drawing functions give, run
against a stub cv2 that restates only the radius-1 filled circle and the axis-aligned one-pixel line (tests/golden/make_vis_golden.py):
the conditions the generator promises, checked on the committed file; tests/vis_oracle.py (the max-key restatement the GPU tests use where
the golden has no case) against every golden canvas, exactly; overlay_grid against the reference's grid and a numpy restatement; the
argument errors, raised from CPU tensors before any device work; the new entry points in the header, the library and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, visualization
from tests import vis_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["di2p_vis_workspace_bytes", "di2p_vis_classification", "di2p_vis_registration"]
N_CASES = 6


@pytest.fixture(scope="module")
def G(golden):
    return golden("vis_golden.npz")


def _case(G, kind, i):
    k = "%s%d_" % (kind, i)
    return {n[len(k):]: G[n] for n in G.files if n.startswith(k)}


def test_exports():
    from deepi2p_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepi2p_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "vis.hip" in build.SOURCES and build.PER_FILE_FLAGS["vis.hip"] == ["-ffp-contract=off"]
    l = _lib.load()
    assert l.di2p_version() == 9                      # purely additive
    for args in ((3, 24, 40, 6, 6), (32, 160, 512, 100, 100), (1, 1, 1, 0, 0)):
        B, H, W, Hd, Wd = args
        want = (4 * B * (H + 2 * Hd) * (W + 2 * Wd) + 255) // 256 * 256
        assert visualization.library_workspace_bytes(*args) == visualization.workspace_bytes(*args) == want
    assert l.di2p_vis_workspace_bytes(1, 0, 4, 0, 0) == -1 and l.di2p_vis_workspace_bytes(1, 4, 4, -1, 0) == -1


def _centres(p, delta):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (np.abs(p) < 1e6)
    return set((np.rint(p[ok]).astype(np.int64) + delta).tolist())


def test_golden_conditions_classification(G):
    sizes, deltas, cells = set(), set(), set()
    for i in range(N_CASES):
        c = _case(G, "cls", i)
        H, W, Hd, Wd, N, s = (int(v) for v in c["dims"])
        HL, WL = H + 2 * Hd, W + 2 * Wd
        sizes.add((H, W)), deltas.update((Hd, Wd)), cells.add(s)
        assert c["img"].shape == (H, W, 3) and c["pxpy"].shape == (2, N) and c["pxpy"].dtype == np.float32
        assert c["fine"].shape == c["coarse"].shape == (HL, WL, 3)
        if N < 63:
            continue
        p = c["pxpy"]
        for axis, delta, side in ((0, Wd, WL), (1, Hd, HL)):
            v = p[axis]
            assert np.isposinf(v).any() and np.isneginf(v).any() and np.isnan(v).any() and (v == np.float32(1e30)).any() and (v == np.float32(-1e30)).any()
            with np.errstate(invalid="ignore"):
                half = np.isfinite(v) & (np.abs(v) < 1e6) & (v - np.floor(v) == 0.5)
            assert (np.floor(v[half]) % 2 == 0).any() and (np.floor(v[half]) % 2 == 1).any()      # both parities of an exact .5
            assert {-1, 0, side - 2, side - 1} <= _centres(v, delta)
        if N >= 300:                                   # a "nothing drawn" point after a drawn one on the same centre
            assert (p[:, N - 1] == p[:, N - 2]).all() and c["coarse_gt"][N - 2] == 1
            assert c["coarse_pred"][N - 1] == 0 and c["coarse_gt"][N - 1] == 0
            cx, cy = int(p[0, N - 1]) + Wd, int(p[1, N - 1]) + Hd
            assert tuple(c["coarse"][cy, cx]) == (255, 0, 0)
    assert sizes == {(24, 40), (16, 32)} and deltas == {0, 6, 100} and cells == {8, 16}
    assert sorted(int(_case(G, "cls", i)["dims"][4]) for i in range(N_CASES)) == [1, 63, 64, 65, 300, 3000]
    assert round(24 / 16) == 2 and round(40 / 16) == 2                          # the half-to-even line counts of case 0
    # the dense case: most painted pixels are covered by more than one stamp
    c = _case(G, "cls", 0)
    H, W, Hd, Wd, N, s = (int(v) for v in c["dims"])
    cover = np.zeros((H + 2 * Hd, W + 2 * Wd), np.int64)
    drawn = (c["coarse_pred"] == 1) | (c["coarse_gt"] == 1)
    with np.errstate(invalid="ignore"):
        rx, ry = np.rint(c["pxpy"][0]), np.rint(c["pxpy"][1])
        ok = drawn & np.isfinite(rx) & np.isfinite(ry) & (rx >= -Wd) & (rx < W + Wd - 1) & (ry >= -Hd) & (ry < H + Hd - 1)
    for dx, dy in vis_oracle.STAMP:
        x, y = rx[ok].astype(int) + Wd + dx, ry[ok].astype(int) + Hd + dy
        inside = (x >= 0) & (x < cover.shape[1]) & (y >= 0) & (y < cover.shape[0])
        np.add.at(cover, (y[inside], x[inside]), 1)
    assert (cover > 1).sum() > 0.5 * (cover > 0).sum()


def test_golden_conditions_registration(G):
    seen_exact = 0
    for i in range(N_CASES):
        c = _case(G, "reg", i)
        H, W, Hd, Wd, N, exact = (int(v) for v in c["dims"])
        HL, WL = H + 2 * Hd, W + 2 * Wd
        assert c["pc"].shape == (3, N) and c["pc"].dtype == np.float32 and c["P"].dtype == np.float64 and c["canvas"].shape == (HL, WL, 3)
        assert not vis_oracle.near_tie(c["pc"], c["P"], c["K"]).any()              # the margin: 1e-6 px from every tie, |z| >= 1e-6 or z == 0
        px, py, z = vis_oracle.project(c["pc"], c["P"], c["K"])
        if exact:
            seen_exact += 1
            assert (z == 0).sum() >= 3 and np.isnan(px[z == 0]).any() and np.isinf(px[z == 0]).any()
            with np.errstate(invalid="ignore"):
                behind = (z < 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)      # finite, inside the image, and skipped for z alone
            assert behind.any()
            assert {-1, 0, WL - 2, WL - 1} <= _centres(px[z > 0], Wd) and {-1, 0, HL - 2, HL - 1} <= _centres(py[z > 0], Hd)
        if N >= 63:
            assert (z < 0).any() and (z > 0).any()
    assert seen_exact == 2
    assert sorted(int(_case(G, "reg", i)["dims"][4]) for i in range(N_CASES)) == [1, 63, 64, 65, 300, 3000]


def test_oracle_equals_every_golden_canvas(G):
    for i in range(N_CASES):
        c = _case(G, "cls", i)
        H, W, Hd, Wd, N, s = (int(v) for v in c["dims"])
        args = (c["pxpy"], c["coarse_pred"], c["coarse_gt"])
        for img in (c["img"], c["img"].transpose(2, 0, 1).astype(np.float32)):
            assert np.array_equal(vis_oracle.classification(*args, c["fine_pred"], c["fine_gt"], img, s, Hd, Wd), c["fine"]), i
            assert np.array_equal(vis_oracle.classification(*args, None, None, img, 0, Hd, Wd), c["coarse"]), i
        assert not np.array_equal(c["fine"], c["coarse"]) and not np.array_equal(c["fine"], vis_oracle.base_canvas(c["img"], Hd, Wd, s))
        c = _case(G, "reg", i)
        H, W, Hd, Wd, N, exact = (int(v) for v in c["dims"])
        assert np.array_equal(vis_oracle.registration(c["pc"], c["P"], c["K"], c["labels"], c["img"], Hd, Wd), c["canvas"]), i
        assert not np.array_equal(c["canvas"], vis_oracle.base_canvas(c["img"], Hd, Wd))


def _grid_numpy(items, col):
    if len(items) == 0:
        return np.zeros((3, 3), np.uint8)
    h, w, c = items[0].shape
    rows = -(-len(items) // col)
    sheet = np.full((rows * h, col * w, c), 255, np.uint8)
    for idx, it in enumerate(items):
        i, j = divmod(idx, col)
        sheet[i * h:(i + 1) * h, j * w:(j + 1) * w] = it
    return sheet


def test_overlay_grid_layout(G):
    assert np.array_equal(visualization.overlay_grid(torch.from_numpy(G["grid_in"]), col=2).numpy(), G["grid_out"])
    rng = np.random.default_rng(4)
    for B, col in ((1, 2), (4, 2), (5, 3), (3, 1), (2, 5)):
        items = rng.integers(0, 256, (B, 4, 6, 3), dtype=np.uint8)
        want = _grid_numpy(list(items), col)
        assert np.array_equal(visualization.overlay_grid(torch.from_numpy(items), col=col).numpy(), want), (B, col)
        assert np.array_equal(visualization.overlay_grid([torch.from_numpy(a) for a in items], col=col).numpy(), want), (B, col)
    for empty in ([], torch.zeros((0, 4, 6, 3), dtype=torch.uint8)):
        out = visualization.overlay_grid(empty)
        assert tuple(out.shape) == (3, 3) and out.dtype == torch.uint8 and int(out.sum()) == 0
    with pytest.raises(ValueError, match="col"):
        visualization.overlay_grid(torch.zeros((2, 4, 6, 3), dtype=torch.uint8), col=0)


def _cls_args(B=2, N=5, H=8, W=12):
    i32 = lambda: torch.zeros((B, N), dtype=torch.int32)      # noqa: E731
    return dict(pxpy=torch.zeros((B, 2, N)), coarse_pred=i32(), coarse_gt=i32(), fine_pred=i32(), fine_gt=i32(),
                img=torch.zeros((B, H, W, 3), dtype=torch.uint8))


def _reg_args(B=2, N=5, H=8, W=12):
    return dict(pc=torch.zeros((B, 3, N)), P=torch.zeros((B, 4, 4), dtype=torch.float64), K=torch.zeros((B, 3, 3), dtype=torch.float64),
                labels=torch.zeros((B, N), dtype=torch.int32), img=torch.zeros((B, 3, H, W)))


def test_argument_errors_come_before_any_device_work():
    """every operand is a CPU tensor: a ValueError here was raised before the library was asked for anything (a valid call on CPU tensors
    gets as far as the CUDA check and raises RuntimeError there)"""
    fine, coarse, reg = visualization.classification_overlay, visualization.classification_overlay_coarse, visualization.registration_overlay
    bad_cls = [dict(pxpy=torch.zeros((2, 2, 5), dtype=torch.float64)), dict(pxpy=torch.zeros((2, 3, 5))), dict(pxpy=torch.zeros((3, 2, 5))),
               dict(coarse_pred=torch.zeros((2, 5), dtype=torch.int64)), dict(coarse_gt=torch.zeros((2, 6), dtype=torch.int32)),
               dict(fine_gt=torch.zeros((2, 5))), dict(fine_pred=None), dict(img=torch.zeros((2, 8, 12, 3))),
               dict(img=torch.zeros((2, 3, 8, 12), dtype=torch.uint8)), dict(img=torch.zeros((8, 12, 3), dtype=torch.uint8)),
               dict(H_delta=-1), dict(W_delta=2.5), dict(W_delta=-3), dict(fine_scale=0), dict(fine_scale=32.0), dict(fine_scale=-8),
               dict(circle_size=2), dict(circle_size=0)]
    for kw in bad_cls:
        with pytest.raises(ValueError):
            fine(**dict(_cls_args(), **kw))
    for kw in (dict(pxpy=torch.zeros((2, 2, 4))), dict(coarse_gt=torch.zeros((2, 5))), dict(H_delta=1.0), dict(circle_size=3),
               dict(img=torch.zeros((2, 3, 8, 12), dtype=torch.float64))):
        a = _cls_args()
        del a["fine_pred"], a["fine_gt"]
        with pytest.raises(ValueError):
            coarse(**dict(a, **kw))
    for kw in (dict(pc=torch.zeros((2, 3, 5), dtype=torch.float64)), dict(pc=torch.zeros((2, 4, 5))), dict(P=torch.zeros((2, 4, 4))),
               dict(P=torch.zeros((2, 3, 4), dtype=torch.float64)), dict(K=torch.zeros((2, 3, 3))), dict(K=torch.zeros((3, 3), dtype=torch.float64)),
               dict(labels=torch.zeros((2, 5), dtype=torch.int64)), dict(labels=torch.zeros((2, 4), dtype=torch.int32)), dict(H_delta=-100),
               dict(W_delta="100"), dict(circle_size=2)):
        with pytest.raises(ValueError):
            reg(**dict(_reg_args(), **kw))
    # the *_into forms: canvas and workspace
    canvas, ws = torch.zeros((2, 12, 16, 3), dtype=torch.uint8), torch.zeros((visualization.workspace_bytes(2, 8, 12, 2, 2),), dtype=torch.uint8)
    for kw in (dict(canvas=canvas[:, :11]), dict(canvas=canvas.float()), dict(workspace=ws[:-1]), dict(workspace=ws.view(torch.int32))):
        common = dict(dict(canvas=canvas, workspace=ws, H_delta=2, W_delta=2), **kw)
        with pytest.raises(ValueError):
            visualization.registration_overlay_into(**_reg_args(), **common)
        with pytest.raises(ValueError):
            visualization.classification_overlay_into(**_cls_args(), **common)
    # valid arguments on the CPU: past every ValueError, stopped by the CUDA check
    with pytest.raises(RuntimeError, match="CUDA"):
        visualization.registration_overlay_into(**_reg_args(), canvas=canvas, workspace=ws, H_delta=2, W_delta=2)
    with pytest.raises(RuntimeError, match="CUDA"):
        fine(**_cls_args())
    assert visualization.grid_lines(24, 40, 16) == (1, 1) and visualization.grid_lines(160, 512, 32) == (4, 15)


def test_executor_option_errors():
    """the option is checked before the executor touches the device or the model"""
    from deepi2p_amd.pipeline import VISUALIZE, RegistrationExecutor
    assert VISUALIZE == (None, "registration", "classification", "both")
    for kw, match in ((dict(visualize="all"), "visualize must be"), (dict(visualize="classification"), "evaluate=True"),
                      (dict(visualize="both"), "evaluate=True"), (dict(visualize="registration", step_fn=lambda s, d: {}), "step_fn"),
                      (dict(visualize="both", evaluate=True, step_fn=lambda s, d: {}), "step_fn")):
        with pytest.raises(ValueError, match=match):
            RegistrationExecutor(None, None, None, None, **kw)
