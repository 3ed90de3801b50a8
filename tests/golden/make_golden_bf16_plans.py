"""Generate tests/golden/bf16_plans.npz: what the bf16 convolution planner answers over a grid of descriptors.

The planner (plan_bf16) is host code and the library loads without a device, so the table is the five queries
s2i_conv_bf16_eligible / _weight_layout / _workspace_bytes / _stat_parts / _weight_elems for every descriptor of GRID
under every knob setting of KNOBS, ineligible rows included: their sentinel results and, where the plan itself refused
the descriptor, which S2I_REQUIRE family said so (ERRORS, matched against s2i_last_error()).  The file holds integers
only.  It pins the planner across changes that must not move a plan: run this once BEFORE such a change, commit the
file, and tests/test_bf16_plan_cpu.py recomputes the table with the functions below and compares row by row.

main() also asserts that the grid reaches the planner's branches worth guarding (both kernels, the 66-pixel padded
patch, split-K under both slot counts, the 16-channel fallback of the wide stride-2 plan, a BatchNorm-groups straddle).

Usage:  python tests/golden/make_golden_bf16_plans.py            (writes next to this file; needs the built library)
"""
import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

K3S1, K4S2, TCONV = 1, 2, 3                      # s2i_conv_kind of include/s2i_hip.h
KINDS = (K3S1, K4S2, TCONV)
BATCHES = (1, 5, 9, 24, 48, 144)
EXTENTS = (4, 8, 16, 32, 64, 128)                # H = W
CXS = (32, 64, 96, 256, 512)
NS = (32, 64, 96, 128, 256, 512)
STATS_GROUPS = ((0, 1), (1, 1), (1, 3))
NOSPLIT = (0, 1)
KNOBS = ({}, {"b16_v2": 0}, {"b16_v2": 2})       # {}: the defaults
GRID = tuple(itertools.product(KINDS, BATCHES, EXTENTS, CXS, NS, STATS_GROUPS, NOSPLIT))
# the S2I_REQUIRE families of plan_bf16 this grid reaches (code = index + 1; 0 = the plan was made)
ERRORS = ("exceeds the LDS plan", "straddles", "output too large")
COLUMNS = ("eligible", "layout", "workspace", "parts", "elems", "error")


def describe(row, knobs):
    kind, B, HW, Cx, N, (stats, groups), nosplit = row
    return "kind=%d B=%d H=W=%d Cx=%d N=%d stats=%d groups=%d nosplit=%d knobs=%r" % (kind, B, HW, Cx, N, stats, groups,
                                                                                      nosplit, knobs)


def descriptor(_lib, row):
    kind, B, HW, Cx, N, (stats, groups), nosplit = row
    return _lib.ConvDesc(kind=kind, B=B, H=HW, W=HW, Cx=Cx, Cc=0, N=N, act=0, stats=stats, ldy=N, groups=groups,
                         nosplit=nosplit)


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
                layout = lib.s2i_conv_bf16_weight_layout(d)
                err = 0
                if layout < 0:
                    msg = lib.s2i_last_error().decode()
                    hits = [j + 1 for j, e in enumerate(ERRORS) if e in msg]
                    assert len(hits) == 1, "%s: unexpected refusal %r" % (describe(row, knobs), msg)
                    err = hits[0]
                out[k, i] = (lib.s2i_conv_bf16_eligible(d), layout, lib.s2i_conv_bf16_workspace_bytes(d),
                             lib.s2i_conv_bf16_stat_parts(d), lib.s2i_conv_bf16_weight_elems(d), err)
    return out


def tiles(row, bm):
    """(tile count, patch width) of a bm-pixel tile, restated from the planner's geometry: as wide as the map (up to 32),
    then rows, then images"""
    kind, B, HW = row[:3]
    Ho = Wo = HW // 2 if kind == K4S2 else HW
    tw = min(Wo, 32)
    th = min(bm // tw, Ho)
    tb = bm // (tw * th)
    pw = tw + 2 if kind == K3S1 else (2 * tw + 2 if kind == K4S2 else tw + 1)
    return (Wo // tw) * (Ho // th) * -(-B // tb), pw


def reached(table):
    """the planner branches the table shows, from the stored results and the restated tile geometry"""
    seen = set()
    col = {c: j for j, c in enumerate(COLUMNS)}
    index = {row: i for i, row in enumerate(GRID)}
    for k in range(len(KNOBS)):
        for i, row in enumerate(GRID):
            kind, B, HW, Cx, N, (stats, groups), nosplit = row
            r = table[k, i]
            if r[col["error"]]:
                seen.add("refused: " + ERRORS[r[col["error"]] - 1])
                continue
            if not r[col["eligible"]] or N <= 64:
                continue
            # which kernel: the unsplit, ungrouped statistics rows of the same layer are its tile count (x 4 phases)
            base = table[k, index[(kind, B, HW, Cx, N, (1, 1), 1)]]
            if base[col["error"]]:
                continue
            grid_m = base[col["parts"]] // (4 if kind == TCONV else 1)
            (t128, _), (t256, pw256) = tiles(row, 128), tiles(row, 256)
            if t128 == t256:
                continue
            assert grid_m in (t128, t256), describe(row, KNOBS[k])
            v2 = grid_m == t256
            ck = r[col["layout"]] & 0xff
            seen.add("v2=%d" % v2)
            if v2 and kind == K4S2 and pw256 == 66 and ck == 32:
                seen.add("padded PW == 66")
            if r[col["workspace"]]:
                seen.add("splitk > 1, %d slots" % (256 if v2 else 512))
            if not v2 and kind == K4S2 and ck == 16:
                seen.add("ck = 16 fallback")
    return seen


REQUIRED = ("v2=0", "v2=1", "padded PW == 66", "splitk > 1, 256 slots", "splitk > 1, 512 slots", "ck = 16 fallback",
            "refused: straddles", "refused: exceeds the LDS plan", "refused: output too large")


def main():
    table = compute()
    seen = reached(table)
    missing = [b for b in REQUIRED if b not in seen]
    assert not missing, "the grid does not reach: %s" % missing
    assert table[..., :5].min() >= -1 and table[..., 5].max() <= len(ERRORS)
    path = os.path.join(HERE, "bf16_plans.npz")
    np.savez_compressed(path, **{c: table[..., j] for j, c in enumerate(COLUMNS)})
    print("%d rows x %d knob settings -> %s (%d bytes); reached: %s" % (len(GRID), len(KNOBS), path, os.path.getsize(path),
                                                                         sorted(seen)))


if __name__ == "__main__":
    main()
