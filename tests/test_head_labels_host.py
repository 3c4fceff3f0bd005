"""CPU: the host side of the fine head's labels-only kernel (di2p_point_head_labels_x3, ABI version 7) -- packed operand sizes and argument
checks, which return before anything touches a device."""
import ctypes
import threading

import pytest


def test_head_labels_packed_bytes_and_abi_version():
    from deepi2p_amd import _lib
    lib = _lib.load()
    assert lib.di2p_version() == 9
    # [ceil(P / 32) row tiles][K / 16 K-steps][3 planes][64 lanes] x 16 B
    assert lib.di2p_head_labels_x3_packed_bytes(256, 256) == 8 * 16 * 3 * 1024
    assert lib.di2p_head_labels_x3_packed_bytes(256, 82) == 3 * 16 * 3 * 1024
    assert lib.di2p_head_labels_x3_packed_bytes(256, 1402) == 44 * 16 * 3 * 1024
    assert lib.di2p_head_labels_x3_packed_bytes(100, 82) == 0 and lib.di2p_head_labels_x3_packed_bytes(256, 0) == 0


def test_head_labels_argument_errors_are_reported():
    """(on a thread of its own: the library's last-error message is per thread, and the ABI test expects "ok" on the main thread)"""
    errors = []

    def body():
        try:
            _argument_errors()
        except BaseException as exc:      # noqa: BLE001 -- re-raised on the test's thread
            errors.append(exc)

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if errors:
        raise errors[0]


def _argument_errors():
    from deepi2p_amd import _lib
    _lib.load()
    with pytest.raises(_lib.DeepI2PHipError, match="null"):
        _lib.call("di2p_point_head_labels_x3", None, 1, 64, None)
    h = _lib.HeadLabelsX3T()
    h.K, h.P = 256, 2
    with pytest.raises(_lib.DeepI2PHipError, match="P >= 3"):
        _lib.call("di2p_point_head_labels_x3", ctypes.byref(h), 1, 64, None)
    h.K, h.P = 128, 82
    with pytest.raises(_lib.DeepI2PHipError, match="hidden width of 256"):
        _lib.call("di2p_point_head_labels_x3", ctypes.byref(h), 1, 64, None)
    h.K = 256
    with pytest.raises(_lib.DeepI2PHipError, match="null operand"):
        _lib.call("di2p_point_head_labels_x3", ctypes.byref(h), 1, 64, None)
    with pytest.raises(_lib.DeepI2PHipError, match="K % 16"):
        _lib.call("di2p_head_labels_x3_pack", 16, 100, 82, 16, None)
