"""CPU: the case tables of tests/fp32_exact_cases.py are what they claim -- every bound below 2^24 (per layer, per Winograd transform position,
the whole epilogue counted in), the edges non-zero, the critical sets covered, every fp64 reference equal to torch's own, and every kernel
instance the library's routing queries can return reached by a minimal case (one K-step, ragged tiles) and a pipelined one (three or more
K-steps).  Instances no admissible shape can reach are listed by name (UNREACHABLE) with the inequality that shows why."""
import collections
import concurrent.futures

import pytest
import torch
import torch.nn.functional as F

from tests import fp32_exact_cases as fc

# instances of the source no shape reaches ("Exact-integer tests of the fp32-MFMA inference family"); each inequality is swept
# through the routing queries by test_unreachable_instances_are_unreachable_by_the_route_queries
UNREACHABLE = {
    "pointwise_gemm_vec_kernel<*, *, DEPTH2 = true>: one K-step": "depth 2 is chosen for K > 64: three K-steps or more",
    "pointwise_gemm_vec_kernel<64 x 64, *>: a ragged N tile": "the 64 x 64 tile is chosen for N % 64 == 0",
    "point_chain_kernel<*>: three K-steps in layer 0": "K0 <= M and M <= 2 KS0 in all eight instances: at most two K-steps (both LDS buffers written once)",
    "point_chain_kernel<64, 32, *>: one K-step in layer 0": "K-step 32 is chosen for K0 > 32",
    "conv2d_kernel<*k32, tap_major = false> (4 instances)": "K-step 32 is chosen as tap_major && Cin % 32 == 0: never without tap_major",
    "conv2d_vec_kernel<*, 22, *> refused for W % 8 != 0 alone": "the 16-byte stager needs OW % 4 == 0 and variant 22 needs W == 2 OW: W % 8 == 0 follows",
}


def _is_multiple(t, unit):
    return bool((t * unit == (t * unit).round()).all())


# ===================================================================================================== routing queries
def test_route_queries_answer_without_a_device_and_refuse_what_the_entries_refuse():
    from deepi2p_amd import _lib, ops

    def checks():
        assert ops.pointwise_route(130, 3, 8193, 2, True, True) == dict(vec=0, bm=128, bn=128, dense=0, depth=1, bk=16)
        assert ops.pointwise_route(130, 3, 8193, 1, True, True)["bm"] == 64                  # 130 workgroups: below 256
        assert ops.pointwise_route(132, 65, 132, 2, False, True) == dict(vec=1, bm=64, bn=128, dense=0, depth=2, bk=32)
        assert ops.pointwise_route(132, 64, 128, 2, True, True) == dict(vec=1, bm=64, bn=64, dense=1, depth=1, bk=32)
        assert ops.pointwise_route(132, 65, 128, 2, True, False)["vec"] == 0                 # misaligned weights
        with _lib.option("pw_novec", 1):
            assert ops.pointwise_route(132, 65, 128, 2, True, True)["vec"] == 0
        with _lib.option("conv_depth1", 1):
            assert ops.pointwise_route(132, 65, 128, 2, True, True)["depth"] == 1
        x = (3, 96, 5, 8)
        need = ops.conv2d_workspace_bytes(x, 128, 3, 3, 1, 1, True)
        assert need == 3 * 128 * 3 * 40 * 4
        full = dict(kernel=1, bm=64, bn=64, bk=32, variant=1, depth=2, splits=3)
        assert ops.conv2d_route(x, 128, 3, 3, 1, 1, True, workspace_bytes=need) == full
        for given in (0, need - 4):                                                           # the silent fallback to one slice
            assert ops.conv2d_route(x, 128, 3, 3, 1, 1, True, workspace_bytes=given) == dict(full, splits=1)
        with _lib.option("conv_nosplit", 1):
            assert ops.conv2d_route(x, 128, 3, 3, 1, 1, True, workspace_bytes=need)["splits"] == 1
        assert ops.conv2d_route((3, 96, 23, 32), 128, 3, 3, 1, 1, True, workspace_bytes=1 << 40)["splits"] == 2
        s2 = ((3, 32, 5, 16), 68, 3, 3, 2, 1, True)
        assert ops.conv2d_route(*s2)["variant"] == 22 and ops.conv2d_route(*s2, x_aligned=False)["variant"] == 2
        assert ops.conv2d_route((3, 32, 5, 7), 68, 3, 3, 2, 1, True)["variant"] == 2          # W != 2 OW
        with _lib.option("conv_s2scalar", 1):
            assert ops.conv2d_route(*s2)["variant"] == 2
        assert ops.conv2d_route(*s2, wt_aligned=False)["kernel"] == 0
        assert ops.conv2d_route((3, 3, 9, 16), 8, 7, 7, 2, 3)["kernel"] == 2 and ops.conv2d_route((3, 3, 9, 14), 8, 7, 7, 2, 3)["kernel"] == 0
        # the 128 x 64 scalar tile exists in a narrow window only
        assert [(ops.conv2d_route((1, 1, 1, n), 129, 1, 1, 1, 0)["bm"], ops.conv2d_route((1, 1, 1, n), 129, 1, 1, 1, 0)["bn"])
                for n in (16320, 16321, 21760, 21761, 32640, 32641)] == [(64, 64), (128, 64), (128, 64), (64, 128), (64, 128), (128, 128)]
        with pytest.raises(_lib.DeepI2PHipError, match="di2p_conv2d_route: tap-major weights need Cin % 16 == 0"):
            ops.conv2d_route((1, 8, 4, 4), 8, 3, 3, 1, 1, True)
        with pytest.raises(_lib.DeepI2PHipError, match="di2p_winograd_route: needs Cin % 8 == 0"):
            ops.winograd_route((1, 4, 4, 4), 32)
        with pytest.raises(_lib.DeepI2PHipError, match="di2p_point_chain_route: bad args"):
            ops.point_chain_route(48, 8, 2, 1, 64, 256)
        with pytest.raises(_lib.DeepI2PHipError, match="di2p_pointwise_route: bad args"):
            ops.pointwise_route(0, 1, 1)
        assert ops.winograd_route((3, 8, 64, 170), 64)["reg"] == 1 and ops.winograd_route((3, 8, 5, 6), 64)["reg"] == 0
        assert ops.winograd_route((3, 8, 64, 342), 32)["reg"] == 1 and ops.winograd_route((3, 8, 64, 168), 64)["reg"] == 0      # 256 workgroups of 64 tiles x 32 channels
        with _lib.option("wino_reg", 1):          # co-block 64 from 768 workgroups on
            assert [ops.winograd_route((3, 8, 128, W), 64)["cob"] for W in (254, 256)] == [32, 64]
            assert ops.winograd_route((3, 8, 128, 256), 96)["cob"] == 32 and ops.winograd_route((3, 512, 8, 8), 64)["kc"] == 8
        # the chain's grid for any device size; the head's two kernels
        for cus in (1, 8, 256):
            rt = ops.point_chain_route(32, 8, 3, 3, 65, cus)
            assert (rt["ks0"], rt["layers"], rt["tn"], rt["nblk"], rt["total"]) == (4, 3, 2, 2, 6) and rt["wgs"] == min(cus * rt["w"], 2)
            assert ops.point_head_route(96, 2, 64, 3, 64, cus)["reg"] == 0                    # the knob head_reg is 0 by default
            with _lib.option("head_reg", 1):
                assert ops.point_head_route(96, 2, 64, 3, 64, cus, g33=True) == dict(reg=1, g33=1, bn=32, nblk=2, total=6, wgs=1)
                assert ops.point_head_route(96, 2, 63, 3, 64, cus)["reg"] == 0                # an odd first source of two
                assert ops.point_head_route(96, 2, 64, 3, 64, cus, reg_range=False)["reg"] == 0
                assert ops.point_head_route(100, 1, 100, 3, 64, cus) == dict(reg=0, g33=0, bn=64, nblk=1, total=3, wgs=3)
                assert ops.point_head_route(4, 1, 4, 3, 4096, cus)["wgs"] == min(cus, 48)     # 384 blocks of 32 columns, 8 waves per workgroup
    with concurrent.futures.ThreadPoolExecutor(1) as ex:          # di2p_last_error is per thread
        ex.submit(checks).result()


# ===================================================================================================== di2p_pointwise_gemm
def test_pointwise_cases_are_exact_and_reach_every_instance():
    reached = collections.defaultdict(lambda: [0, 0, 0])          # instance -> cases, minimal, pipelined
    for c in fc.PW_CASES:
        d = fc.pw_case(c)
        rt, what = d["route"], fc.pw_id(c)
        assert rt["vec"] or not rt["dense"]
        assert bool((d["full"] == d["full"]).all()) and d["full"].shape == (c.B, c.K, c.N)
        # the reference is torch's own contraction of the virtual concatenation
        assert torch.equal(d["acc"], torch.einsum("km,bkn->bmn", d["w"].t().double(), d["full"].double())), what
        if c.family in ("S", "IDA", "IDB"):
            assert float(d["bound"].max()) < fc.LIMIT, what
            for t in [d["w"], d["full"]] + [v for v in d["kw"].values() if torch.is_tensor(v)]:
                assert _is_multiple(t, fc.UNIT), what
            for tab, gi, gw in d["kw"].get("gathered", []):
                assert _is_multiple(tab, 1.0) and (gw is None or set(gw.unique().tolist()) <= set(fc.GW)), what
        if c.family == "S":
            assert bool((d["w"][-1] != 0).all()) and bool((d["w"][:, -1] != 0).all()), what
            stored = d["parts"][0][1] if c.src == "gather" else d["full"]          # a gather source: the table's last row and column
            assert bool((stored[:, -1] != 0).all()) and bool((stored[:, :, -1] != 0).all()), what
        else:
            hot = d["w"] if c.family in ("IDA", "P") else d["full"].transpose(1, 2)
            assert bool(((hot != 0).sum(-1) == 1).all()) and bool((hot.abs().sum(-1) == 1).all()), what
            if c.family in ("P", "Pw"):          # a signed copy of one operand element: exact for any float
                other = d["full"] if c.family == "P" else d["w"]
                assert bool(torch.isfinite(other).all()) and float(other.abs().min()) >= 2.0 ** -126, what
                assert torch.equal(d["acc"].float().double(), d["acc"]), what
            used = set(d["pos"].reshape(-1).tolist())
            n_hot = d["pos"].numel() // (1 if c.family in ("IDA", "P") else c.B)
            want = set(d["crit"]) if n_hot >= len(d["crit"]) else None
            assert want is None or want <= used, "%s: critical indices %s not covered" % (what, sorted(want - used))
        steps = -(-c.K // rt["bk"])
        r = reached[fc.pw_instance(rt)]
        r[0] += 1
        ragged_n = c.N % rt["bn"] != 0 or (rt["vec"] and rt["bn"] == 64)          # the 16-byte stager takes 64-column tiles only for N % 64 == 0
        r[1] += steps == 1 and c.M % rt["bm"] != 0 and ragged_n
        r[2] += steps >= 3 and c.K % rt["bk"] == 1
    assert sorted(reached) == sorted(fc.PW_INSTANCES)
    for inst, (n, minimal, pipelined) in reached.items():
        assert (minimal >= 1 or inst[4] == 2) and pipelined >= 1, "instance %s: %d cases, %d minimal, %d pipelined" % (inst, n, minimal, pipelined)


def test_pointwise_critical_sets():
    assert fc.critical_k(97, 32, [5, 69]) == [0, 4, 5, 31, 32, 63, 64, 68, 69, 95, 96]
    assert fc.critical_k(33, 16) == [0, 15, 16, 31, 32] and fc.critical_k(1, 16) == [0] and fc.critical_k(16, 16) == [0, 15]
    for c in fc.PW_CASES:
        if c.src == "concat":
            assert {4, 5, 68, 69} <= set(fc.pw_case(c)["crit"])


# ===================================================================================================== di2p_conv2d
def test_conv2d_cases_are_exact_and_reach_every_instance():
    reached = collections.defaultdict(lambda: [0, 0, 0])
    splits = collections.Counter()
    fallback = 0
    for c in fc.CONV_CASES:
        d = fc.conv_case(c)
        rt, what = d["route"], fc.conv_id(c)
        K = c.Cin * c.KH * c.KW
        # Wt is the weight in the case's row order; the reference is F.conv2d
        order = d["w"].permute(2, 3, 1, 0) if c.tap_major else d["w"].permute(1, 2, 3, 0)
        assert torch.equal(d["Wt"], order.reshape(K, c.Cout)), what
        assert torch.equal(d["acc"], F.conv2d(d["x"].double(), d["w"].double(), stride=c.stride, padding=c.pad)), what
        assert d["acc"].shape[2:] == (fc.conv_out(c.H, c.KH, c.stride, c.pad), fc.conv_out(c.W, c.KW, c.stride, c.pad))
        if c.family in ("S", "TID"):
            assert float(d["bound"].max()) < fc.LIMIT, what
        if c.family == "S":
            assert bool((d["Wt"][-1] != 0).all()) and bool((d["Wt"][:, -1] != 0).all()) and bool((d["x"][:, -1] != 0).all()), what
            assert _is_multiple(d["scale"], 2.0) and _is_multiple(d["shift"], 1.0), what
        else:
            assert bool(((d["Wt"] != 0).sum(0) == 1).all()) and bool((d["Wt"].abs().sum(0) == 1).all()), what
            assert torch.equal(d["Wt"].abs().argmax(0), d["pos"]), what
            used = set(d["pos"].tolist())
            assert c.Cout < len(d["crit"]) or set(d["crit"]) <= used, what
            if c.family == "T":
                assert float(d["x"].abs().min()) >= 2.0 ** -126 and torch.equal(d["acc"].float().double(), d["acc"]), what
        need, given = fc.conv_ws_bytes(c)
        if c.ws != "full" and need:
            assert rt["splits"] == 1 and given < need, what
            fallback += 1
        splits[rt["splits"]] += 1
        if rt["splits"] > 1:          # both sides of every slice boundary are in the critical set
            T = K // rt["bk"]
            for z in range(1, rt["splits"]):
                b = T * z // rt["splits"] * rt["bk"]
                assert {b - 1, b} <= set(d["crit"]), what
        steps = -(-K // rt["bk"])
        Ntot = c.B * d["acc"].shape[2] * d["acc"].shape[3]
        r = reached[fc.conv_instance(rt)]
        r[0] += 1
        r[1] += steps == 1 and Ntot % rt["bn"] != 0 and c.Cout % rt["bm"] != 0
        assert rt["kernel"] != 1 or K % 32 == 0          # the 16-byte stager never sees a ragged last K-step
        r[2] += steps >= 3
    want = sorted(fc.CONV_SCALAR + fc.CONV_VEC + [(2,)])
    assert sorted(reached) == want, "unreached: %s" % sorted(set(want) - set(reached))
    for inst, (n, minimal, pipelined) in reached.items():
        if inst == (2,):          # the 7x7 / 2 stager: at least 49 rows, two K-steps
            assert pipelined >= 1
        else:
            assert minimal >= 1 and pipelined >= 1, "instance %s: %d cases, %d minimal, %d pipelined" % (inst, n, minimal, pipelined)
    assert splits[2] >= 1 and splits[3] >= 1 and fallback >= 4


# ===================================================================================================== di2p_conv3x3_winograd
def test_winograd_cases_are_exact_in_the_transform_domain_and_reach_every_instance():
    reached = collections.Counter()
    for c in fc.WINO_CASES:
        d = fc.wino_case(c)
        what = fc.wino_id(c)
        U, V, m_abs, y_abs, y = fc.wino_pipeline(d["x"], d["w"])
        assert bool((d["w"] % 4 == 0).all()) and _is_multiple(U, 1.0) and _is_multiple(V, 1.0), what
        assert m_abs < fc.LIMIT and y_abs < fc.LIMIT, what                       # sum_ci |U||V| per position, then A^T |M| A
        assert (y_abs * 2.0 + d["epi_bound"]) * fc.UNIT < fc.LIMIT, what         # scale <= 2, shift, residual; halves
        assert torch.equal(y, d["acc"]) and torch.equal(d["acc"], F.conv2d(d["x"].double(), d["w"].double(), padding=1)), what
        if c.dgrad:
            assert torch.equal(d["acc"], torch.nn.grad.conv2d_input(tuple(d["acc"].shape), d["weight"].double(), d["x"].double(), padding=1)), what
        rt = fc.wino_route(c)
        tiles = c.B * ((c.H + 1) // 2) * ((c.W + 1) // 2)
        assert rt["n_tb"] == -(-tiles // rt["tiles"])
        reached[fc.wino_instance(rt)] += 1
        reached[fc.wino_instance(rt) + ("partial last block",)] += tiles % rt["tiles"] != 0
        reached[fc.wino_instance(rt) + ("steps", c.Cin // 8)] += 1
    for inst in fc.WINO_INSTANCES:
        assert reached[inst] >= 1 and reached[inst + ("partial last block",)] >= 1, inst
        assert all(reached[inst + ("steps", s)] >= 1 for s in (1, 2, 3)), inst
    assert any(not c.knobs and fc.wino_route(c)["reg"] for c in fc.WINO_CASES) and any(not c.knobs and not fc.wino_route(c)["reg"] for c in fc.WINO_CASES)


# ===================================================================================================== attention_pool, batch_gemv
def test_attention_and_gemv_cases_are_exact():
    assert {(c.C, c.HW, c.Mn) for c in fc.ATTN_CASES} == set(fc.ATTN_SHAPES)
    assert any(c.HW & (c.HW - 1) == 0 and c.HW > 1 for c in fc.ATTN_CASES) and any(c.HW % 2 == 1 and c.HW > 1 for c in fc.ATTN_CASES)
    for c in fc.ATTN_CASES:
        d = fc.attn_case(c)
        assert float(d["absum"].max()) < fc.LIMIT and c.HW < fc.LIMIT
        assert torch.equal(d["acc"], torch.einsum("bch,bhm->bcm", d["feat"].double(), d["score"].double()))
        assert d["ref"].dtype == torch.float32 and torch.equal(d["ref"], (d["acc"] / c.HW).to(torch.float32))
        if c.family != "S":
            assert c.HW > len(fc.critical_k(c.HW, 16)) or set(fc.critical_k(c.HW, 16)) <= set(d["pos"].reshape(-1).tolist())
    for c in fc.GEMV_CASES:
        d = fc.gemv_case(c)
        assert float(d["absum"].max()) < fc.LIMIT
        ref = d["v"].double() @ d["Wt"][c.k0:c.k0 + c.Kv].double()
        if c.Kv1:
            ref = ref + d["v1"].double() @ d["Wt"][c.k1:c.k1 + c.Kv1].double()
        assert torch.equal(d["ref"], ref)
        per = (c.Kv + 3) // 4
        assert {s * per + o for s in range(1, 4) for o in (-1, 0) if 0 < s * per < c.Kv} <= set(fc.gemv_critical(c.Kv))
    assert {(c.M, c.Kv, c.k0) for c in fc.GEMV_CASES} == set(fc.GEMV_GRID)


# ===================================================================================================== di2p_point_chain
@pytest.mark.parametrize("cus", (1, 8, 256))
def test_chain_cases_are_exact_per_layer_and_reach_every_instance(cus):
    reached = collections.Counter()
    for c in fc.CHAIN_CASES:
        N = c.N or fc.chain_uneven_n(c.M, c.K0, c.layers, c.B, cus)
        rt = fc.chain_route(c, cus, N)
        inst = (rt["M"], rt["ks0"], rt["layers"])
        reached[inst] += 1
        if not c.N:
            assert rt["total"] > 4 * rt["wgs"] and rt["total"] % (4 * rt["wgs"]) != 0
            reached[inst + ("uneven",)] += 1
        # layer 0 has at most TWO K-steps by construction (K0 <= M <= 2 KS0 in every instance), and the K-step-32 instances (K0 > 32) never one
        reached[inst + ("minimal",)] += c.K0 <= rt["ks0"] and N % (32 * rt["tn"]) != 0
        reached[inst + ("pipelined",)] += c.K0 > rt["ks0"]
        d = fc.chain_case(c, N)
        assert len(d["outs"]) == c.layers and max(d["bounds"]) < fc.LIMIT, fc.chain_id(c)
        v = d["x"].double()
        for l, (w, sc, sh, relu) in enumerate(d["layers"]):
            if c.family == "ID" or c.epi in ("none", "relu0"):
                a = torch.einsum("mk,bkn->bmn", w.double(), v)
                a = a * (1 if sc is None else sc.double().view(1, -1, 1)) + (0 if sh is None else sh.double().view(1, -1, 1))
                assert torch.equal(torch.relu(a) if relu else a, d["outs"][l]), fc.chain_id(c)
            v = d["outs"][l]
        if c.family == "ID":          # every hidden row is observed: the later layers are permutations
            assert all(bool(((w != 0).sum(0) == 1).all()) and bool(((w != 0).sum(1) == 1).all()) for w, _, _, _ in d["layers"][1:])
            assert c.M < len(fc.critical_k(c.K0, rt["ks0"])) or set(fc.critical_k(c.K0, rt["ks0"])) <= set(d["pos"].tolist())
    for inst in fc.CHAIN_INSTANCES:
        assert reached[inst] >= 1 and reached[inst + ("uneven",)] >= 1 and reached[inst + ("pipelined",)] >= 1, (inst, reached)
        assert reached[inst + ("minimal",)] >= 1 or inst[:2] == (64, 32), (inst, reached)


# ===================================================================================================== di2p_point_head
@pytest.mark.parametrize("cus", (1, 8, 256))
def test_head_cases_are_exact_per_layer_and_reach_every_instance(cus):
    reached = collections.Counter()
    for c in fc.HEAD_CASES:
        N = c.N or fc.head_uneven_n(c.B, cus)
        assert N % 4 == 0 and sum(c.split) == c.K0
        rt = fc.head_route(c, cus, N)
        inst = (rt["reg"], rt["g33"])
        reached[inst] += 1
        want_reg = c.reg and c.K0 <= 96 and len(c.split) <= 2 and (len(c.split) == 1 or c.split[0] % 2 == 0)
        assert rt["reg"] == int(bool(want_reg)) and rt["g33"] == int(fc.head_g33(c)), fc.head_id(c)
        ks = 48 if rt["reg"] else 16
        reached[inst + ("minimal",)] += c.K0 <= ks and N % rt["bn"] != 0
        reached[inst + ("pipelined",)] += (c.K0 > ks) if rt["reg"] else (c.K0 > 2 * ks and c.K0 % ks == 4)
        if not c.N:
            reached[inst + ("uneven",)] += rt["total"] > 8 * rt["wgs"] and rt["total"] % (8 * rt["wgs"]) != 0
        if c.N or cus == 8:          # every listed N; the route-chosen N at one device size here, at the device's own in the GPU test
            d = fc.head_case(c, N)
            assert [n for n, _, _ in d["stages"]][:2] == ["y0", "y1"] and len(d["stages"]) == 2 + len(d["tails"])
            for name, _, bound in d["stages"]:
                assert float(bound.max()) < fc.LIMIT, (fc.head_id(c), name)
            if not c.family.startswith("x3:"):          # the reference is torch's own: three einsums with the epilogues between
                x = torch.cat(d["srcs"], 1).double()
                g = torch.zeros(c.B, 128, N, dtype=torch.float64)
                for G, idx, w in d["gathered"]:
                    for j in range(3):
                        rows = torch.gather(G.double(), 1, idx[:, :, j].long().unsqueeze(2).expand(c.B, N, 128)).transpose(1, 2)
                        g += rows * (1.0 if w is None else w[:, :, j].double().unsqueeze(1))
                v = (torch.einsum("km,bkn->bmn", d["W0"].double(), x) + g) * d["sc0"].double().view(1, -1, 1) + d["sh0"].double().view(1, -1, 1)
                v = torch.relu(v) if d["relu0"] else v
                v = torch.einsum("km,bkn->bmn", d["W1"].double(), v) * d["sc1"].double().view(1, -1, 1) + d["sh1"].double().view(1, -1, 1)
                v = torch.relu(v) if d["relu1"] else v
                v = torch.einsum("km,bkn->bmn", d["tails"][0][0].double(), v) * d["sc2"].double().view(1, -1, 1) + d["sh2"].double().view(1, -1, 1)
                assert torch.equal(torch.relu(v) if d["relu2"] else v, d["tails"][0][1]), fc.head_id(c)
                assert bool((d["W0"][-1] != 0).all()) and bool((d["W0"][:, -1] != 0).all()) and bool((x[:, -1] != 0).all()) and bool((x[:, :, -1] != 0).all())
    for inst in fc.HEAD_INSTANCES:
        assert reached[inst] >= 1 and reached[inst + ("minimal",)] >= 1 and reached[inst + ("pipelined",)] >= 1, (inst, reached)
        assert not inst[0] or reached[inst + ("uneven",)] >= 1, (inst, reached)          # trips exist on the wave-autonomous kernel only
    # every hidden row of layer 1 is observed by some one-hot output layer of the head_x3_cases families
    c = next(c for c in fc.HEAD_CASES if c.family == "x3:B" and c.N)
    assert torch.stack([W2.abs().sum(1) for W2, _ in fc.head_case(c)["tails"]]).sum(0).min() >= 1


# ===================================================================================================== di2p_conv7x7s2_stem
def test_stem_cases_are_exact_and_cover_the_launch_rule():
    from tests import stem_x3_cases as sx
    assert set(sx.SHAPES) <= set(fc.STEM_SHAPES)
    taps = set()
    items = [fc.stem_items(c) for c in fc.STEM_CASES]
    assert any(t == g == 3 for t, g in items) and any(t > g == 512 for t, g in items)          # one item per frame; more items than workgroups
    assert any(((c.W - 1) // 2 + 1) % 128 == 1 and c.W > 256 for c in fc.STEM_CASES) and any(((c.H - 1) // 2 + 1) % 2 == 1 for c in fc.STEM_CASES)
    for c in fc.STEM_CASES:
        d = fc.stem_case(c)
        assert float(d["x"].min()) >= 0 and float(d["x"].max()) <= 255 and _is_multiple(d["x"], 1.0) and _is_multiple(d["scale"], 2.0)
        assert float(d["bound"].max()) < fc.LIMIT, fc.stem_id(c)
        assert torch.equal(d["acc"], F.conv2d(d["x"].double(), d["w"].double(), stride=2, padding=3))
        assert d["acc"].shape == (c.B, 64, (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1)
        Wp = fc.stem_packed(d["w"])
        assert Wp.shape == (168, 64) and bool((Wp.view(21, 8, 64)[:, 7] == 0).all()) and torch.equal(Wp.view(3, 7, 8, 64)[:, :, :7].permute(3, 0, 1, 2), d["w"])
        if c.family != "S":
            flat = d["w"].view(64, 147)
            assert bool(((flat != 0).sum(1) == 1).all()) and flat.abs().argmax(1).tolist() == sx.d_taps(int(c.family[1]))
            taps |= set(flat.abs().argmax(1).tolist())
            assert bool((d["w"].sum((1, 2, 3)) < 0).any()) and bool((d["w"].sum((1, 2, 3)) > 0).any())
        else:
            assert bool((d["w"].view(64, 147)[:, -1] != 0).all()) and bool((d["w"][-1] != 0).all())
    assert taps == set(range(147))


# ===================================================================================================== what no shape reaches
def test_unreachable_instances_are_unreachable_by_the_route_queries():
    """Every entry of UNREACHABLE as a sweep through the routing queries: no admissible shape returns the instance."""
    from deepi2p_amd import _lib, ops
    assert len(UNREACHABLE) == 6
    pw = [ops.pointwise_route(M, K, N, B, dense, True) for M in (68, 132, 260) for K in (1, 32, 64, 65, 97, 300) for N in (4, 60, 64, 128, 132, 192, 1000)
          for B in (1, 3) for dense in (False, True)]
    assert any(r["vec"] and r["depth"] == 2 for r in pw) and any(r["vec"] and r["bn"] == 64 for r in pw)
    for M in (68, 132):
        for K in range(1, 200):
            for N in (4, 60, 64, 128, 132, 192):
                r = ops.pointwise_route(M, K, N, 3, True, True)
                assert r["vec"] == 1 and (r["depth"] == 2) == (K > 2 * r["bk"]) and (r["bn"] == 64) == (N % 64 == 0)          # depth 2: >= 3 K-steps; 64 columns: no ragged tile
    for M, kss in ((32, (4, 16)), (64, (16, 32))):
        for K0 in range(1, M + 1):
            for layers in (2, 3):
                r = ops.point_chain_route(M, K0, layers, 3, 65, 8)
                assert r["ks0"] in kss and -(-K0 // r["ks0"]) <= 2 and (r["ks0"] != 32 or K0 > 32)
    for tap in (False, True):
        for Cin in (16, 32, 48, 64, 96) if tap else (1, 3, 32, 33, 64, 96):
            for Cout in (8, 65, 129):
                for W in (8, 7, 10881):
                    for k, stride, pad in ((1, 1, 0), (3, 1, 1), (3, 2, 1), (3, 3, 1)):
                        r = ops.conv2d_route((3, Cin, 5 if W < 100 else 1, W), Cout, k if W < 100 else 1, k if W < 100 else 1, stride, pad if W < 100 else 0, tap)
                        assert r["bk"] == (32 if tap and Cin % 32 == 0 else 16)          # K-step 32 never without tap_major
    for W in range(4, 200):          # variant 22's own W % 8 test never decides alone
        for k, pad in ((3, 1), (1, 0)):
            OW = (W + 2 * pad - k) // 2 + 1
            r = ops.conv2d_route((3, 32, 5, W), 68, k, k, 2, pad, True)
            if r["kernel"] == 1 and W == 2 * OW:
                assert W % 8 == 0 and r["variant"] == 22
            assert r["kernel"] != 1 or (r["variant"] == 22) == (W == 2 * OW)
