"""The layer shapes that put every kernel instance of conv_x3.hip (DI2P_CX_INSTANCES) under the exact tests -- and every single-buffered
instance additionally through cx_best's fallback (a double-buffered plan without a double-buffered instance).  No GPU code.

The plan entry (ops.conv3x3_x3_plan = di2p_conv3x3_x3_plan) is the authority on what a shape runs on: tests/test_conv_x3_plan_host.py asserts
every row's claims against it, so a new instance without a row, or a plan change that moves a row, fails before a GPU is needed.

Each (instance, route) has two layers, run with B = 2:
  minimal    one chunk (Cin == KS): ragged last tile (nseg % NSEG != 0), a partial Cout tile and, where the instance has more staging items
             than the plan needs, surplus items (they land in the dump entry);
  pipelined  at least 3 chunks (both patch buffers are written twice, chunk(c, true_type) runs twice), and where the geometry allows at least
             2 tiles per frame with 3 output rows under a tile.  The fallback routes of instances 4, 5 and 12 cannot have that: a patch with 3
             output rows at their row length does not fit the LDS twice, and then the plan is single-buffered itself and not a fallback.
"""
from collections import namedtuple

Case = namedtuple("Case", "instance fallback kind Cin H W Cout stride cfg flags")

# flags a row claims of its plan: ragged (nseg % NSEG != 0), partial (Cout % MT != 0 with 2 Cout tiles), surplus (instance items > plan
# items), chunks3 (Cin / KS >= 3), tiles2 (>= 2 tiles per frame), rows3 (>= 3 output rows under a tile)
_MIN, _PIPE = "minimal", "pipelined"
_R, _P, _S, _C, _T, _W = "ragged", "partial", "surplus", "chunks3", "tiles2", "rows3"

CASES = [
    # instance, via fallback, kind, Cin, H, W, Cout, stride, cfg
    Case(0, 0, _MIN, 16, 1, 128, 72, 1, 0, (_R, _P, _S)),
    Case(0, 0, _PIPE, 48, 3, 128, 72, 1, 0, (_R, _P, _C, _T, _W)),
    Case(1, 0, _MIN, 16, 1, 64, 136, 1, 1, (_R, _P, _S)),
    Case(1, 0, _PIPE, 48, 3, 64, 136, 1, 1, (_R, _P, _C, _T, _W)),
    Case(2, 0, _MIN, 32, 1, 32, 136, 1, 2, (_R, _P, _S)),
    Case(2, 0, _PIPE, 96, 3, 32, 136, 1, 2, (_R, _P, _C, _T, _W)),
    Case(3, 0, _MIN, 32, 1, 16, 72, 1, 3, (_R, _P, _S)),
    Case(3, 0, _PIPE, 96, 6, 16, 72, 1, 3, (_R, _P, _C, _T, _W)),
    Case(4, 0, _MIN, 16, 6, 128, 136, 2, 1, (_R, _P, _T, _W)),
    Case(4, 0, _PIPE, 48, 6, 128, 136, 2, 1, (_R, _P, _C, _T, _W)),
    Case(4, 1, _MIN, 16, 2, 128, 136, 2, 1, (_R, _P, _S)),
    Case(4, 1, _PIPE, 48, 4, 128, 136, 2, 1, (_R, _P, _S, _C)),
    Case(5, 0, _MIN, 32, 6, 64, 136, 2, 2, (_R, _P, _T, _W)),
    Case(5, 0, _PIPE, 96, 6, 64, 136, 2, 2, (_R, _P, _C, _T, _W)),
    Case(5, 1, _MIN, 32, 2, 64, 136, 2, 2, (_R, _P, _S)),
    Case(5, 1, _PIPE, 96, 4, 64, 136, 2, 2, (_R, _P, _S, _C)),
    Case(6, 0, _MIN, 32, 2, 32, 72, 2, 3, (_R, _P, _S)),
    Case(6, 0, _PIPE, 96, 12, 32, 72, 2, 3, (_R, _P, _C, _T, _W)),
    Case(7, 0, _MIN, 16, 11, 32, 72, 1, 0, (_R, _P, _S, _T, _W)),
    Case(7, 0, _PIPE, 48, 11, 32, 72, 1, 0, (_R, _P, _S, _C, _T, _W)),
    Case(8, 0, _MIN, 16, 6, 32, 136, 1, 1, (_R, _P, _S, _T, _W)),
    Case(8, 0, _PIPE, 48, 6, 32, 136, 1, 1, (_R, _P, _S, _C, _T, _W)),
    Case(9, 0, _MIN, 32, 6, 16, 136, 1, 2, (_R, _P, _S, _T, _W)),
    Case(9, 0, _PIPE, 96, 6, 16, 136, 1, 2, (_R, _P, _S, _C, _T, _W)),
    Case(10, 0, _MIN, 32, 3, 32, 72, 1, 3, (_R, _P, _S, _T, _W)),
    Case(10, 0, _PIPE, 96, 3, 32, 72, 1, 3, (_R, _P, _S, _C, _T, _W)),
    Case(11, 1, _MIN, 16, 12, 64, 136, 2, 1, (_R, _P, _S, _T, _W)),          # instance 11 is reachable through the fallback only
    Case(11, 1, _PIPE, 48, 12, 64, 136, 2, 1, (_R, _P, _S, _C, _T, _W)),
    Case(12, 0, _MIN, 32, 6, 64, 72, 2, 3, (_R, _P, _T, _W)),
    Case(12, 0, _PIPE, 96, 6, 64, 72, 2, 3, (_R, _P, _C, _T, _W)),
    Case(12, 1, _MIN, 32, 2, 64, 72, 2, 3, (_R, _P, _S)),
    Case(12, 1, _PIPE, 96, 4, 64, 72, 2, 3, (_R, _P, _S, _C)),
]

B = 2          # frames per layer in the exact tests


def case_id(c):
    return "i%d%s-%s-%dx%dx%d-%d-s%d" % (c.instance, "fb" if c.fallback else "", c.kind[:3], c.Cin, c.H, c.W, c.Cout, c.stride)


def plan_flags(p, c):
    """the flags of `Case.flags` that the plan p (ops.conv3x3_x3_plan) of case c has"""
    have = set()
    if p["ragged_segments"] != 0:
        have.add(_R)
    if p["partial_cout"] != 0 and p["n_mt"] == 2:
        have.add(_P)
    if p["instance_items"] > p["plan_items"]:
        have.add(_S)
    if p["chunks"] >= 3:
        have.add(_C)
    if p["tiles_per_frame"] >= 2:
        have.add(_T)
    if p["max_rows"] >= 3:
        have.add(_W)
    return have


def geometry(c):
    """(MF, NSEG, MT) of the case's tile configuration (kCfgs of conv_x3.hip): pixels per segment, segments and output channels per workgroup"""
    MF, TM, TN, WM, WN = ((32, 1, 5, 2, 2), (32, 1, 5, 4, 1), (16, 2, 5, 4, 1), (16, 1, 5, 4, 1))[c.cfg]
    return MF, TN * WN, MF * TM * WM


def describe(c, idx):
    """where an output index (b, co, oh, ow) of case c lies: the four facts the exact tests report with a mismatch"""
    b, co, oh, ow = idx
    MF, NSEG, MT = geometry(c)
    OH, OW = (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    seg = oh * (OW // MF) + ow // MF
    return ("first differing index (b, co, oh, ow) = %s; border row/column: %s; first/last pixel of its segment: %s; in the last Cout tile: %s; "
            "segment %d of the frame = segment %d of workgroup tile %d"
            % (idx, oh in (0, OH - 1) or ow in (0, OW - 1), ow % MF in (0, MF - 1), co // MT == (c.Cout - 1) // MT, seg, seg % NSEG, seg // NSEG))
