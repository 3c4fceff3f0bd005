"""CPU: the window on the PnP workspace.  registration_pnp.workspace_views must describe the layout both RANSAC entry points use
(csrc/pnp.hip: corr, hyp, inliers, mask, each region rounded up to 256 bytes) and must stay inside di2p_pnp_workspace_bytes; the views
are views.  Needs the library only, no GPU."""
import os

import pytest
import torch

from deepi2p_amd import _lib
from deepi2p_amd import registration_pnp as rp

GRID = [(1, 1, 1), (3, 700, 301), (64, 20480, 500), (7, 130, 70), (2, 255, 64), (1, 257, 3), (5, 4096, 200)]


@pytest.fixture(scope="module")
def lib():
    from deepi2p_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("F,N,iters", GRID)
def test_workspace_views_inside_the_workspace(lib, F, N, iters):
    total = lib.di2p_pnp_workspace_bytes(F, N, iters)
    ws = torch.empty((total,), dtype=torch.uint8)
    v = rp.workspace_views(ws, F, N, iters)
    assert list(v) == ["corr", "hyp", "inliers", "mask"]
    want = dict(corr=((F, N, 8), torch.float32), hyp=((F, iters, 13), torch.float64), inliers=((F, iters), torch.int32), mask=((F, N), torch.uint8))
    base, end = ws.data_ptr(), 0
    for name, (shape, dtype) in want.items():
        t = v[name]
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
        off = t.data_ptr() - base
        # the launch code's own walk: every region starts at the 256-byte round-up of the end of the one before it
        assert off == (end + 255) // 256 * 256, (name, off, end)
        end = off + t.numel() * t.element_size()
    assert end <= total, (end, total)
    # views, not copies: a write through the view lands in the workspace
    ws.zero_()
    v["mask"][F - 1, N - 1] = 7
    v["inliers"][0, 0] = -1
    assert int(ws[end - 1]) == 7 and int(ws[v["inliers"].data_ptr() - base]) == 255


def test_workspace_views_refuse_a_short_or_typed_workspace(lib):
    F, N, iters = 3, 700, 301
    total = lib.di2p_pnp_workspace_bytes(F, N, iters)
    v = rp.workspace_views(torch.empty((total,), dtype=torch.uint8), F, N, iters)
    need = v["mask"].data_ptr() + F * N - v["corr"].data_ptr()
    rp.workspace_views(torch.empty((need,), dtype=torch.uint8), F, N, iters)
    with pytest.raises(ValueError):
        rp.workspace_views(torch.empty((need - 1,), dtype=torch.uint8), F, N, iters)
    with pytest.raises(ValueError):
        rp.workspace_views(torch.empty((total,), dtype=torch.int8), F, N, iters)
