"""CPU: the argument errors of the raw-frame path (scan_prep's normals method, raw_prep, raw_pipeline.host_frames) are raised on the host,
before anything touches a device, and the three entry points it adds are declared, exported and bound."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, raw_pipeline, raw_prep, scan_prep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["di2p_estimate_normals_cells", "di2p_normals_cells_candidates", "di2p_compose_poses"]


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
    assert _lib.load().di2p_normals_cells_candidates() == scan_prep.NORMALS_CELL_CANDIDATES
    # the grown workspace still scales with the capacity, and the version number is the one the other tests pin
    l = _lib.load()
    assert l.di2p_scan_prep_workspace_bytes(4, 200_000) > l.di2p_scan_prep_workspace_bytes(4, 100_000) >= 100_000 * 112
    assert l.di2p_version() == 9


def test_bad_normals_method():
    with pytest.raises(ValueError, match="normals method"):
        scan_prep.estimate_normals(None, method="cell")
    with pytest.raises(ValueError, match="normals method"):
        scan_prep.preprocess_velodyne([np.zeros((4, 4), np.float32)], method="wave")
    with pytest.raises(ValueError, match="normals method"):
        raw_prep.RawFramePlan(SimpleNamespace(), 1, 100, 100, normals_method="fast")
    with pytest.raises(ValueError, match="normals method"):
        raw_prep.prepare_raw([np.zeros((4, 4), np.float32)], np.zeros((1, 370, 1226, 3), np.uint8), np.eye(3)[None], np.eye(4)[None],
                             SimpleNamespace(), normals_method="")


@pytest.mark.parametrize("dataset", ["oxford", "nuscenes", "kitty"])
def test_only_kitti_has_a_raw_stage(dataset):
    with pytest.raises(ValueError, match="raw-scan stage"):
        raw_prep.RawFramePlan(SimpleNamespace(), 1, 100, 100, dataset=dataset)
    with pytest.raises(ValueError, match="raw-scan stage"):
        raw_prep.prepare_raw([np.zeros((4, 4), np.float32)], np.zeros((1, 370, 1226, 3), np.uint8), np.eye(3)[None], np.eye(4)[None],
                             SimpleNamespace(), dataset=dataset)
    with pytest.raises(ValueError, match="raw-scan stage"):
        raw_pipeline.RawFrameExecutor(None, None, SimpleNamespace(), {}, 100, 100, dataset=dataset)


def _batch(counts=(30, 0, 50), hw=(8, 10)):
    rng = np.random.default_rng(0)
    B = len(counts)
    return dict(scans=[rng.standard_normal((n, 4)).astype(np.float32) for n in counts], image=np.zeros((B,) + hw + (3,), np.uint8),
                K_raw=np.tile(np.eye(3), (B, 1, 1)), Pc=np.tile(np.eye(4), (B, 1, 1)))


def test_host_frames_accepts_both_forms():
    b = _batch()
    parts, off, image, K, Pc, seed = raw_pipeline.host_frames(b, 3, 80, (8, 10))
    assert off.dtype == torch.int32 and off.tolist() == [0, 30, 30, 80] and seed == 0 and len(parts) == 3
    flat = dict(b, scans=np.concatenate(b["scans"] + [np.zeros((9, 4), np.float32)]), offsets=[0, 30, 30, 80], seed=7)
    parts, off, image, K, Pc, seed = raw_pipeline.host_frames(flat, 3, 80, (8, 10))
    assert off.tolist() == [0, 30, 30, 80] and seed == 7 and len(parts) == 1 and parts[0].shape == (80, 4)
    assert np.array_equal(parts[0].numpy(), np.concatenate(b["scans"]))


def test_oversize_batch_and_shape_mismatch():
    b = _batch()
    hf = raw_pipeline.host_frames
    with pytest.raises(ValueError, match="cap_raw = 79"):
        hf(b, 3, 79, (8, 10))
    with pytest.raises(ValueError, match="B = 2"):
        hf(b, 2, 80, (8, 10))
    with pytest.raises(ValueError, match="image"):
        hf(b, 3, 80, (8, 12))
    with pytest.raises(ValueError, match="image"):
        hf(dict(b, image=b["image"].astype(np.float32)), 3, 80, (8, 10))
    with pytest.raises(ValueError, match="K_raw"):
        hf(dict(b, K_raw=np.eye(3)), 3, 80, (8, 10))
    with pytest.raises(ValueError, match="offsets"):
        hf(dict(b, scans=np.zeros((80, 4), np.float32)), 3, 80, (8, 10))
    with pytest.raises(ValueError, match="offsets"):
        hf(dict(b, scans=np.zeros((80, 4), np.float32), offsets=[0, 50, 30, 80]), 3, 80, (8, 10))
    with pytest.raises(ValueError, match="offsets"):
        hf(dict(b, scans=np.zeros((80, 4), np.float32), offsets=[0, 30, 30, 81]), 3, 80, (8, 10))
    with pytest.raises(ValueError, match="float32"):
        hf(dict(b, scans=np.zeros((80, 4), np.float64), offsets=[0, 30, 30, 80]), 3, 80, (8, 10))
    with pytest.raises(ValueError, match="float32"):
        hf(dict(b, scans=[x.astype(np.float64) for x in b["scans"]]), 3, 80, (8, 10))
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        hf(dict(b, scans=[x[:, :3] for x in b["scans"]]), 3, 80, (8, 10))
    with pytest.raises(ValueError, match="no 'Pc'"):
        hf({k: v for k, v in b.items() if k != "Pc"}, 3, 80, (8, 10))
