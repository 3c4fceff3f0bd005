"""CPU: the host side of evaluation mode.  tests/golden/eval_golden.npz holds 67 pose pairs with the errors the REFERENCE's get_P_diff
(and enu2cam) gives for them and the summary statistics restated with numpy (tests/golden/make_eval_golden.py): the golden against a
live call of scipy's route here, EvalState.merge / summary / line against the restated statistics, the argument errors of the new
options, and the four new entry points in the header, the library and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from deepi2p_amd import _lib, evaluation, registration, registration_pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["di2p_pose_errors", "di2p_eval_accumulate", "di2p_eval_acc_reset", "di2p_eval_acc_bytes", "di2p_enu2cam_points"]


@pytest.fixture(scope="module")
def G(golden):
    return golden("eval_golden.npz")


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
    l = _lib.load()
    assert l.di2p_eval_acc_bytes() == 8 * (16 + 2 * evaluation.BINS)
    assert l.di2p_version() == 9                      # purely additive


def test_golden_shape_and_conditions(G):
    """what the generator promises, checked on the committed file: 67 pairs, invalid costs of both kinds, thresholds and bin edges at
    least 1e-6 away, a success, a failure and an overflow of each kind among the valid frames"""
    assert G["P_pred"].shape == (67, 4, 4) and G["P_gt"].shape == (67, 4, 4) and G["gt_is3"].any() and not G["gt_is3"].all()
    cost = G["cost"]
    assert (cost == 0).any() and (cost == 1e-7).any() and cost[cost > 1e-6].min() >= 1e-3
    for s in ("", "_enu"):
        t, r = G["rte" + s], G["rre" + s]
        assert np.abs(t - 2.0).min() > 1e-6 and np.abs(r - 5.0).min() > 1e-6
        assert np.abs(t[:, None] - np.linspace(0, 15, 61)[None, 1:]).min() > 1e-6
        assert np.abs(r[:, None] - np.linspace(0, 30, 61)[None, 1:]).min() > 1e-6
    for f in ("cam", "enu"):
        assert 0 < G[f + "_n_success"] < G[f + "_n_valid"] == 60 and G[f + "_rte_over"] > 0 and G[f + "_rre_over"] > 0


def test_golden_agrees_with_scipy_here(G):
    """registration.get_P_diff (numpy + scipy, live) against the reference's recorded values, plain and in the converted frame"""
    Ci = np.linalg.inv(evaluation.P_CONVERT)
    for i in range(67):
        t, r = registration.get_P_diff(G["P_pred"][i], G["P_gt"][i])
        assert abs(t - G["rte"][i]) <= 1e-12 and abs(r - G["rre"][i]) <= 1e-12, i
        t, r = registration.get_P_diff(G["P_pred"][i] @ Ci, G["P_gt"][i] @ Ci)
        assert abs(t - G["rte_enu"][i]) <= 1e-12 and abs(r - G["rre_enu"][i]) <= 1e-12, i
    # the points: (x, y, z) -> (x, -z, y)
    pc = G["pc"]
    assert np.array_equal(G["pc_enu2cam"], np.stack([pc[0], -pc[2], pc[1]]))


@pytest.mark.parametrize("frame", ["cam", "enu"])
def test_state_merge_summary_line(G, frame):
    """the golden's error lists split into three uneven parts, folded on the host and merged: counts and histograms exact, means and
    sigmas to 1e-12 relative, the line string-equal to the reference's format on the restated numbers"""
    s = "" if frame == "cam" else "_enu"
    rte, rre, cost = G["rte" + s], G["rre" + s], G["cost"]
    flags = (cost > 1e-6).astype(np.int32) | (np.logical_and(rte < 2.0, rre < 5.0).astype(np.int32) << 1)
    state = evaluation.EvalState()
    for a, b in ((0, 5), (5, 48), (48, 67)):
        state = state.merge(evaluation.EvalState.from_errors(rte[a:b], rre[a:b], flags[a:b]))
    out = state.summary()
    p = frame + "_"
    assert out["n"] == 67 and out["n_valid"] == int(G[p + "n_valid"])
    assert np.array_equal(out["rte_hist"], G[p + "rte_hist"]) and np.array_equal(out["rre_hist"], G[p + "rre_hist"])
    assert out["rte_overflow"] == int(G[p + "rte_over"]) and out["rre_overflow"] == int(G[p + "rre_over"])
    assert state.n_success == int(G[p + "n_success"])
    for k in ("rte_mean", "rte_sigma", "rre_mean", "rre_sigma", "success_rate"):
        assert abs(out[k] - float(G[p + k])) <= 1e-12 * abs(float(G[p + k])), k
    assert np.isnan(out["coarse_accuracy"]) and np.isnan(out["fine_accuracy"])
    want = "RTE %.2f +- %.2f, RRE %.2f +- %.2f, success rate %.2f" % (G[p + "rte_mean"], G[p + "rte_sigma"], G[p + "rre_mean"],
                                                                       G[p + "rre_sigma"], G[p + "success_rate"] * 100)
    assert state.line() == want


def test_state_words_mask_and_accuracy():
    """from_words reads the layout the header documents; a masked frame is absent from everything; NaN accuracies are not counted"""
    words = np.zeros(136, np.int64)
    words[:7] = [9, 7, 3, 9, 8, 1, 2]
    words[8:14] = np.array([7.0, 9.0, 21.0, 70.0, 4.5, 2.0]).view(np.int64)
    words[16 + 4], words[76 + 59] = 6, 5
    st = evaluation.EvalState.from_words(words.view(np.uint8))
    assert (st.n, st.n_valid, st.n_success, st.n_coarse, st.n_fine, st.rte_over, st.rre_over) == (9, 7, 3, 9, 8, 1, 2)
    assert (st.rte_sum, st.rte_sq, st.rre_sum, st.rre_sq, st.coarse_sum, st.fine_sum) == (7.0, 9.0, 21.0, 70.0, 4.5, 2.0)
    assert st.rte_hist[4] == 6 and st.rre_hist[59] == 5 and st.rte_hist.sum() == 6
    out = st.summary()
    assert out["rte_mean"] == 1.0 and out["coarse_accuracy"] == 0.5 and out["fine_accuracy"] == 0.25 and out["success_rate"] == 3 / 7
    with pytest.raises(ValueError):
        evaluation.EvalState.from_words(np.zeros(135, np.int64))
    acc = np.array([[0.5, np.nan], [1.0, 0.25], [0.0, 0.75]], np.float32)
    st = evaluation.EvalState.from_errors([1.0, 20.0, 3.0], [1.0, 2.0, 40.0], frame_mask=[1, 0, 1], accuracy=acc)
    assert (st.n, st.n_valid, st.n_success, st.n_coarse, st.n_fine, st.rte_over, st.rre_over) == (2, 2, 1, 2, 1, 0, 1)
    assert st.coarse_sum == 0.5 and st.fine_sum == 0.75
    empty = evaluation.EvalState().summary()
    assert empty["n"] == 0 and np.isnan(empty["rte_mean"]) and np.isnan(empty["success_rate"])


def test_bad_frame_raises_on_the_host():
    with pytest.raises(ValueError, match="frame"):
        registration.RegistrationPipeline(64, 128, frame="sideways")
    with pytest.raises(ValueError, match="frame"):
        registration_pnp.PnPPipeline(64, 128, frame="sideways")
    assert registration.RegistrationPipeline(64, 128).frame == "cam" and registration_pnp.PnPPipeline(64, 128, frame="enu").enu
    with pytest.raises(ValueError, match="frame"):
        evaluation.check_frame("ENU")
