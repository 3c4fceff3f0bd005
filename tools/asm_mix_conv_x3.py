#!/usr/bin/env python3
"""Instruction mix of every conv3x3_x3_kernel instance, from hipcc's assembly (host only: cross-compiles, runs nothing).

Compiles deepi2p_amd/csrc/conv_x3.hip for gfx950 with the flags deepi2p_amd/build.py uses and splits each instance into regions:
  prologue  kernel entry up to the first matrix instruction (set-up, first patch, first weights)
  first     a chunk peeled in front of the loop, where there is one: from the first matrix instruction to the loop
  loop      the chunk loop (the backward branch that spans the most matrix instructions): one chunk of nine taps WITH staging
  last      the chunk peeled behind the loop (no staging): from the loop's end to the last matrix instruction
  epilogue  everything behind the last matrix instruction (both branches of it, with and without a residual: the counts are static)
and counts per region: matrix instructions (v_mfma*), other vector instructions (v_* except v_mfma* / v_accvgpr*), and moves through the
accumulator file, v_accvgpr_*, in two kinds: `acc`, whose AGPR some matrix instruction of the kernel accumulates in (plus every v_mov_b32
that touches such a register), and `oth`, the rest: vector registers hipcc parks in free AGPRs.  "out" = all but the loop.  Registers and
spills come from the kernel's metadata.

    python tools/asm_mix_conv_x3.py [--label TEXT] [--src conv_x3.hip] [--asm file.s]
--src: another version of the file (say `git show HEAD~1:deepi2p_amd/csrc/conv_x3.hip` written somewhere), compiled against this tree's headers.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepi2p_amd import build as B  # noqa: E402

SRC = "conv_x3.hip"
REGIONS = ("prologue", "first", "loop", "last", "epilogue")
PARAMS = ("MF", "TM", "TN", "WM", "WN", "STRIDE", "DS", "DBUF", "ITEMS", "PWT", "SA")


def compile_asm(src):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    slp = [] if SRC in B.SLP_ON else ["-fno-slp-vectorize"]
    cmd = [B.HIPCC] + B.FLAGS + slp + B.PER_FILE_FLAGS.get(SRC, []) + ["-I", B.CSRC, "-x", "hip", "--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return out


def regs(tok):
    """'a[0:15]' / 'v7' -> set of (file, index); anything else -> empty"""
    m = re.fullmatch(r"([av])\[(\d+):(\d+)\]", tok)
    if m:
        return {(m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    m = re.fullmatch(r"([av])(\d+)", tok)
    return {(m.group(1), int(m.group(2)))} if m else set()


def instr(line):
    s = line.split(";")[0].strip()
    if not s or s.startswith((".", "//")) or s.endswith(":"):
        return None, []
    parts = s.split(None, 1)
    ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
    return parts[0], ops


def metadata(text):
    meta = {}
    for chunk in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", chunk)
        if not name:
            continue
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, chunk).group(1)) if re.search(r"\.%s:\s+(\d+)" % k, chunk) else -1
        meta[name.group(1)] = {k: get(k) for k in ("agpr_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return meta


def analyse(lines, start):
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end + 1]
    dec = [instr(l) for l in body]
    label_at = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    is_mfma = [bool(op) and op.startswith("v_mfma") for op, _ in dec]
    loops = []
    for i, (op, ops) in enumerate(dec):
        if op and op.startswith(("s_cbranch", "s_branch")) and ops and ops[0] in label_at and label_at[ops[0]] <= i:
            loops.append((sum(is_mfma[label_at[ops[0]]:i + 1]), label_at[ops[0]], i))
    n_mfma, lo, hi = max(loops) if loops else (0, 0, -1)
    last_mfma = max(i for i, m in enumerate(is_mfma) if m)
    acc_regs = set()
    for (op, ops), m in zip(dec, is_mfma):
        if m:
            acc_regs |= regs(ops[0])
    first_mfma = min(i for i, m in enumerate(is_mfma) if m)
    region = lambda i: "prologue" if i < min(first_mfma, lo) else "first" if i < lo else "loop" if i <= hi else "last" if i <= last_mfma else "epilogue"
    cnt = {r: {"mfma": 0, "vector": 0, "acc": 0, "oth": 0, "scratch": 0} for r in REGIONS}
    for i, (op, ops) in enumerate(dec):
        if not op:
            continue
        c = cnt[region(i)]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_accvgpr"):
            c["acc" if any(regs(o.split()[0]) & acc_regs for o in ops[:2]) else "oth"] += 1
        elif op.startswith("v_"):
            c["vector"] += 1
            if op.startswith("v_mov_b32") and any(regs(o.split()[0]) & acc_regs for o in ops[:2]):
                c["acc"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
    return cnt, len(acc_regs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--src", default=os.path.join(B.CSRC, SRC))
    ap.add_argument("--asm", default=None, help="an assembly file already made (skips the compile)")
    a = ap.parse_args()
    path = a.asm or compile_asm(a.src)
    text = open(path).read()
    lines = text.splitlines()
    meta = metadata(text)
    if a.label:
        print("== " + a.label)
    print("per region: mfma / vec / acc / oth (see the head of tools/asm_mix_conv_x3.py); out = all but the loop")
    print("%-34s | %-19s | %-19s | %-19s | %-14s | %-14s | %-14s | %s" % ("instance MF,TM,TN,WM,WN,stride,ITEMS,PWT", "first", "loop", "last",
          "prologue", "epilogue", "out", "accregs agpr vgpr spill scratch"))
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w*conv3x3_x3_kernel\w*):", l)
        if not m:
            continue
        t = dict(zip(PARAMS, [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1))]))
        cnt, nacc = analyse(lines, i)
        md = meta.get(m.group(1), {})
        cnt["out"] = {k: sum(cnt[r][k] for r in REGIONS if r != "loop") for k in ("vector", "acc", "oth")}
        name = "%d,%d,%d,%d,%d,%d,%d,%d" % tuple(t[k] for k in ("MF", "TM", "TN", "WM", "WN", "STRIDE", "ITEMS", "PWT"))
        chunk = lambda r: "%4d %5d %4d %3d" % (cnt[r]["mfma"], cnt[r]["vector"], cnt[r]["acc"], cnt[r]["oth"])
        rest = lambda r: "%5d %4d %3d" % (cnt[r]["vector"], cnt[r]["acc"], cnt[r]["oth"])
        print("%-34s | %s | %s | %s | %s | %s | %s | %7d %4d %4d %5d %7d" % (
            name, chunk("first"), chunk("loop"), chunk("last"), rest("prologue"), rest("epilogue"), rest("out"), nacc, md.get("agpr_count", -1),
            md.get("vgpr_count", -1), md.get("vgpr_spill_count", -1), sum(cnt[r]["scratch"] for r in REGIONS)))
    if not a.asm:
        os.unlink(path)


if __name__ == "__main__":
    main()
