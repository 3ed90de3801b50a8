"""Generate tests/golden/conv_plans.npz: what the fp32 forward planner answers over a grid of descriptors.

plan_fwd (csrc/s2i_conv.hip) is host code and the library loads without a device, so the table is the three queries
s2i_conv_workspace_bytes / s2i_conv_stat_parts / s2i_conv_split_eligible for every descriptor of GRID under every knob
setting of KNOBS, refused rows included: their sentinel results and which S2I_REQUIRE family said so (ERRORS, matched
against s2i_last_error()).  The file holds integers only.  It pins the planner across changes that must not move a plan:
run this once BEFORE such a change, commit the file, and tests/test_conv_plan_cpu.py recomputes the table with the
functions below and compares row by row.

main() also asserts that the grid reaches the planner's branches worth guarding (both tile heights, split K, the thin
layers' workspace, the small-N exclusion of the split-bf16 path, every refusal family of ERRORS).

Usage:  python tests/golden/make_golden_conv_plans.py            (writes next to this file; needs the built library)
"""
import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

K1, K3S1, K4S2, TCONV, C1D = 0, 1, 2, 3, 4       # s2i_conv_kind of include/s2i_hip.h
KINDS = (K1, K3S1, K4S2, TCONV, C1D)
BATCHES = (1, 5, 24, 72, 144)
EXTENTS = (1, 4, 16, 64, 128)                    # H = W
CXS = (4, 32, 40, 64, 136)
NS = (4, 40, 64, 136)
CCS = (0, 32, 128)
STATS_GROUPS = ((0, 1), (1, 1), (1, 3))
NOSPLIT = (0, 1)
WMODES = (0, 1)
KNOBS = ({}, {"fwd_bm": 96}, {"fwd_bm": 128}, {"fwd_min_cps": 2})       # {}: the defaults
GRID = tuple(itertools.product(KINDS, BATCHES, EXTENTS, CXS, NS, CCS, STATS_GROUPS, NOSPLIT, WMODES))
# the S2I_REQUIRE families of plan_fwd this grid reaches (code = index + 1; 0 = the plan was made)
ERRORS = ("extent < 2", "conv1d: forward only", "BatchNorm groups of whole row tiles", "no tile height fits")
COLUMNS = ("workspace", "parts", "split_eligible", "error")


def describe(row, knobs):
    kind, B, HW, Cx, N, Cc, (stats, groups), nosplit, wmode = row
    return "kind=%d B=%d H=W=%d Cx=%d N=%d Cc=%d stats=%d groups=%d nosplit=%d wmode=%d knobs=%r" % (
        kind, B, HW, Cx, N, Cc, stats, groups, nosplit, wmode, knobs)


def descriptor(_lib, row):
    kind, B, HW, Cx, N, Cc, (stats, groups), nosplit, wmode = row
    ca = Cx + Cc
    return _lib.ConvDesc(kind=kind, B=B, H=HW, W=HW, Cx=Cx, Cc=Cc, N=N, wmode=wmode, flip=0, wR=N if wmode else ca,
                         ldw=ca if wmode else N, act=0, stats=stats, ldy=N, groups=groups, nosplit=nosplit, kw=5, stride=1,
                         pad=2)


def compute():
    """int64 array [len(KNOBS)][len(GRID)][len(COLUMNS)]"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    out = np.zeros((len(KNOBS), len(GRID), len(COLUMNS)), dtype=np.int64)
    for k, knobs in enumerate(KNOBS):
        with _lib.tuning(**knobs):
            for i, row in enumerate(GRID):
                d = ctypes.byref(descriptor(_lib, row))
                parts = lib.s2i_conv_stat_parts(d)
                err = 0
                if parts < 0:
                    msg = lib.s2i_last_error().decode()
                    hits = [j + 1 for j, e in enumerate(ERRORS) if e in msg]
                    assert len(hits) == 1, "%s: unexpected refusal %r" % (describe(row, knobs), msg)
                    err = hits[0]
                out[k, i] = (lib.s2i_conv_workspace_bytes(d), parts, lib.s2i_conv_split_eligible(d), err)
    return out


def reached(table):
    """the planner branches the table shows, from the stored results alone: the row of the same layer with nosplit = 1 holds
    the thin layers' workspace and the row-tile count, so a larger workspace without it is K-split slabs"""
    seen = set()
    col = {c: j for j, c in enumerate(COLUMNS)}
    index = {row: i for i, row in enumerate(GRID)}
    for k in range(len(KNOBS)):
        for i, row in enumerate(GRID):
            kind, B, HW, Cx, N, Cc, (stats, groups), nosplit, wmode = row
            r = table[k, i]
            if r[col["error"]]:
                seen.add("refused: " + ERRORS[r[col["error"]] - 1])
                continue
            whole = table[k, index[row[:7] + (1, wmode)]]
            Ho = HW // 2 if kind == K4S2 else HW
            M, nph = B * Ho * Ho, 4 if kind == TCONV else 1
            if whole[col["workspace"]]:
                seen.add("thin workspace")
            if r[col["workspace"]] > whole[col["workspace"]]:
                assert r[col["workspace"]] % (M * nph * N * 4) == 0, describe(row, KNOBS[k])
                seen.add("splitk > 1")
            t96, t128 = -(-M // 96) * nph, -(-M // 128) * nph
            if nosplit and t96 != t128:
                assert r[col["parts"]] in (t96, t128), describe(row, KNOBS[k])
                seen.add("bm = %d%s" % (96 if r[col["parts"]] == t96 else 128, " forced" if "fwd_bm" in KNOBS[k] else ""))
            if (Cx + Cc) % 32 == 0 and Cc % 32 == 0 and not r[col["split_eligible"]]:
                seen.add("small-N stream excluded from split-bf16")
    return seen


REQUIRED = ("splitk > 1", "thin workspace", "bm = 96", "bm = 128", "bm = 96 forced", "bm = 128 forced",
            "small-N stream excluded from split-bf16") + tuple("refused: " + e for e in ERRORS)


def main():
    table = compute()
    seen = reached(table)
    missing = [b for b in REQUIRED if b not in seen]
    assert not missing, "the grid does not reach: %s" % missing
    assert table.min() >= -1 and table[..., 3].max() <= len(ERRORS)
    path = os.path.join(HERE, "conv_plans.npz")
    np.savez_compressed(path, **{c: table[..., j] for j, c in enumerate(COLUMNS)})
    print("%d rows x %d knob settings -> %s (%d bytes); reached: %s" % (len(GRID), len(KNOBS), path, os.path.getsize(path),
                                                                         sorted(seen)))


if __name__ == "__main__":
    main()
