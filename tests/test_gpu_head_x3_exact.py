"""GPU: di2p_point_head_x3 with operands for which all three layers are exact (tests/head_x3_cases.py): the output must equal the fp64
evaluation BIT FOR BIT, under every value of the head_x3_tab knob (node tables from memory, in LDS with eight waves, in LDS with four).
What only a tolerance pinned before: the register split of layer 0's operand, the v_permlane32_swap that builds layer 1's operand and its
re-split, which of the six products each layer issues, the fma chain over the gathered node rows, the meeting of the two half-waves in the
output layer, the walk of a workgroup over its frame's blocks and the prefetch of the next block.  tests/test_x3_fused_cases_host.py asserts
the bounds and the families' claims on the reference alone.  Reference: per_point_pn of models/networks_united.py:57-74, applied at
:188-197, in fp64 on the CPU."""
import pytest
import torch

from deepi2p_amd import _lib
from tests import head_x3_cases as hc
from tests import x3_exact_cases as xc

pytestmark = pytest.mark.gpu


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _describe(idx, N):
    b, p, n = idx
    return ("first differing index (b, p, n) = %s: point %d of 32-point block %d of its frame (the last block: %s, a ragged one: %s)"
            % (idx, n % 32, n // 32, n // 32 == (N - 1) // 32, N % 32 != 0))


def _run_all(dev, d, N, what):
    from deepi2p_amd import ops
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items() if k not in ("stages", "tails")}
    packed = {"W0p": ops.head_x3_pack(t["W0"].contiguous()), "W1p": ops.head_x3_pack(t["W1"].contiguous()),
              "ss": torch.stack((t["sc0"], t["sh0"], t["sc1"], t["sh1"])).contiguous(), "relu0": d["relu0"], "relu1": d["relu1"],
              "sc2": t["sc2"], "sh2": t["sh2"], "relu2": d["relu2"]}
    gathered = [(t["Ga"], t["ia"], t["wa"]), (t["Gb"], t["ib"], t["wb"])]
    for name, _, bound in d["stages"]:
        assert float(bound.max()) < hc.LIMIT, (what, name)          # on the reference alone (the host test, for this device's sizes)
    for tab in (0, 1, 2):
        with _lib.option("head_x3_tab", tab):
            outs = [ops.point_head_x3(t["first"], t["second"], dict(packed, W2t=W2.to(dev).contiguous()), gathered, N) for W2, _ in d["tails"]]
        for i, (got, (_, ref)) in enumerate(zip(outs, d["tails"])):
            got = got.cpu()
            idx = xc.first_mismatch(got, ref)
            assert idx is None, "head_x3 %s, head_x3_tab = %d, output layer %d of %d: %s (got %r, expected %r; %d of %d differ)" % (
                what, tab, i, len(outs), _describe(idx, N), float(got[idx]), float(ref[idx]), int((got != ref).sum()), ref.numel())
            assert torch.equal(got, ref)


@pytest.mark.parametrize("family", hc.HEAD_FAMILIES)
@pytest.mark.parametrize("config", hc.HEAD_CONFIGS, ids=hc.head_config_id)
def test_head_x3_equals_fp64_bit_for_bit(dev, config, family):
    B, N, P, nodes = config
    cus = _cus(dev)
    if N is None:
        N = hc.head_big_n(cus)
        for tab in (0, 1, 2):
            lo, hi = hc.head_trips(B, N, cus, tab)
            assert hi >= 2 and lo < hi          # waves with unequal trip counts, the frame's last block a later trip of its wave
    _run_all(dev, hc.head_case(family, B, N, P, nodes), N, (family, hc.head_config_id(config)))
