"""CPU: tests/conv_x3_cases.py covers every kernel instance of conv_x3.hip, checked against the plan entry (di2p_conv3x3_x3_plan: host code, the
same cx_best call as the launch; without a GPU the cost model prices for 256 compute units).  A new instance without a row in the table, or a
plan change that moves a row to another instance, fails here."""
import pytest

from tests import conv_x3_cases as cx


@pytest.fixture(scope="module")
def plans():
    from deepi2p_amd import ops
    return [ops.conv3x3_x3_plan((cx.B, c.Cin, c.H, c.W), c.Cout, c.stride, cfg=c.cfg) for c in cx.CASES]


def test_plan_entry_agrees_with_supported():
    from deepi2p_amd import ops
    assert ops.conv3x3_x3_plan((1, 64, 8, 24), 64, 1) is None and not ops.conv3x3_x3_supported((1, 64, 8, 24), 64, 1)
    assert ops.conv3x3_x3_plan((1, 64, 7, 32), 64, 2) is None and ops.conv3x3_x3_plan((1, 512, 5, 16), 512, 1, cfg=0) is None
    p = ops.conv3x3_x3_plan((32, 64, 40, 128), 64, 1)
    assert p is not None and sorted(p) == sorted(ops.CONV_X3_PLAN_FIELDS)
    # the first ResNet layer: configuration 0 on its compile-time row length, four chunks of 16 channels -- and the same in any batch
    assert (p["cfg"], p["instance"], p["pwt"], p["dbuf"], p["fallback"], p["chunks"]) == (0, 0, 130, 1, 0, 4)
    assert ops.conv3x3_x3_plan((1, 64, 40, 128), 64, 1) == p == ops.conv3x3_x3_plan((3, 64, 40, 128), 64, 1)
    # a forced configuration is the one that runs, where it has an instance for the shape (16-pixel segments of a 64-pixel row: none)
    for cfg in range(4):
        q = ops.conv3x3_x3_plan((2, 64, 8, 64), 128, 1, cfg=cfg)
        assert (q is not None) == ops.conv3x3_x3_supported((2, 64, 8, 64), 128, 1, cfg=cfg) == (cfg < 2)
        assert q is None or q["cfg"] == cfg


def test_every_row_runs_on_the_instance_it_names(plans):
    for c, p in zip(cx.CASES, plans):
        assert p is not None, cx.case_id(c)
        assert (p["instance"], p["fallback"], p["cfg"]) == (c.instance, c.fallback, c.cfg), (cx.case_id(c), p)
        assert p["fallback"] == 0 or p["dbuf"] == 0, (cx.case_id(c), p)


def test_every_row_has_the_edges_it_claims(plans):
    for c, p in zip(cx.CASES, plans):
        assert cx.plan_flags(p, c) == set(c.flags), (cx.case_id(c), p)
        assert {"ragged", "partial"} <= set(c.flags), cx.case_id(c)                       # every layer: ragged last tile, partial Cout tile
        if c.kind == "minimal":
            assert p["chunks"] == 1, cx.case_id(c)
        else:
            assert "chunks3" in c.flags, cx.case_id(c)
        assert 4 * cx.B * max(c.Cin * c.H * c.W, c.Cout * c.H * c.W) < (1 << 20), cx.case_id(c)      # a layer stays under a megabyte


def test_every_instance_and_every_fallback_is_reached(plans):
    count = plans[0]["instances"]
    assert count == 13 and all(p["instances"] == count for p in plans)
    direct = {p["instance"] for p in plans if not p["fallback"]}
    by_fallback = {p["instance"] for p in plans if p["fallback"]}
    assert direct | by_fallback == set(range(count))
    single = {p["instance"] for p in plans if p["dbuf"] == 0}
    assert single == {4, 5, 11, 12} and single <= by_fallback          # every single-buffered instance also through the fallback
    pipelined = {p["instance"] for p in plans if p["chunks"] >= 3}
    assert pipelined == set(range(count))
    # each (instance, route) has its minimal and its pipelined layer
    routes = {(c.instance, c.fallback) for c in cx.CASES}
    for r in routes:
        assert sorted(c.kind for c in cx.CASES if (c.instance, c.fallback) == r) == ["minimal", "pipelined"], r
    # surplus staging items wherever an instance can have them: every instance but the 8-item single-buffered ones on their own plan
    surplus = {(c.instance, c.fallback) for c in cx.CASES if "surplus" in c.flags}
    assert routes - surplus == {(4, 0), (5, 0), (12, 0)}
