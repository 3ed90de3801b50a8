"""Generate tests/golden/bf16_plans.npz: what the bf16 convolution planner answers over a grid of descriptors.

The planner (plan_bf16) is host code and the library loads without a device, so the table is what
s2i_conv_bf16_plan_query says for every descriptor of GRID under every knob setting of KNOBS, ineligible rows included:
whether the plan names a kernel, the weight layout key CK | Npad << 8, workspace bytes, statistics rows, weight elements,
the kernel (index into _lib.B16_KERNELS), the grid along x (the persistent form's block slots included) and the tile
count; for a descriptor the plan itself refused, sentinels and which S2I_REQUIRE family said so (ERRORS, matched against
s2i_last_error()).  The file holds integers only.  It pins the planner across changes that must not move a plan: run
this once BEFORE such a change, commit the file, and tests/test_bf16_plan_cpu.py recomputes the table with the functions
below and compares row by row.

main() also asserts that the grid reaches the planner's branches worth guarding (every kernel, split-K under both slot
counts, a persistent grid whose blocks walk different numbers of tiles, a BatchNorm-groups straddle and the other
refusals).

Usage:  python tests/golden/make_golden_bf16_plans.py            (writes next to this file; needs the built library)
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from speech_to_image_translation_without_text_amd import _lib  # noqa: E402  (binds nothing until compute() loads the library)

K3S1, K4S2, TCONV = 1, 2, 3                      # s2i_conv_kind of include/s2i_hip.h
KINDS = (K3S1, K4S2, TCONV)
BATCHES = (1, 5, 9, 24, 48, 144)
EXTENTS = (4, 8, 16, 32, 64, 128)                # H = W
CXS = (32, 64, 96, 256, 512)
NS = (32, 64, 96, 128, 256, 512)
STATS_GROUPS = ((0, 1), (1, 1), (1, 3))
NOSPLIT = (0, 1)
# {}: the defaults; the last setting is the one the GPU tests force (four block slots for the persistent form)
KNOBS = ({}, {"b16_v2": 0}, {"b16_v2": 2}, {"b16_v2": 2, "b16_persist": 4})
GRID = tuple(itertools.product(KINDS, BATCHES, EXTENTS, CXS, NS, STATS_GROUPS, NOSPLIT))
# the S2I_REQUIRE families of plan_bf16 this grid reaches (code = index + 1; 0 = the plan was made)
ERRORS = ("exceeds the LDS plan", "straddles", "output too large")
COLUMNS = ("eligible", "layout", "workspace", "parts", "elems", "error", "kernel", "gx", "tiles")
REFUSED = (0, -1, 0, -1, 0, None, -1, 0, 0)      # what a refused descriptor records beside its error code


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
    lib = _lib.load()
    out = np.zeros((len(KNOBS), len(GRID), len(COLUMNS)), dtype=np.int64)
    for k, knobs in enumerate(KNOBS):
        with _lib.tuning(**knobs):
            for i, row in enumerate(GRID):
                p = _lib.conv_bf16_plan(descriptor(_lib, row))
                if p is None:
                    msg = lib.s2i_last_error().decode()
                    hits = [j + 1 for j, e in enumerate(ERRORS) if e in msg]
                    assert len(hits) == 1, "%s: unexpected refusal %r" % (describe(row, knobs), msg)
                    out[k, i] = tuple(hits[0] if v is None else v for v in REFUSED)
                    continue
                named = p["kernel"] is not None
                out[k, i] = (int(named), p["ck"] | p["npad"] << 8, p["ws_bytes"], p["parts"], p["w_elems"], 0,
                             _lib.B16_KERNELS.index(p["kernel"]) if named else -1, p["gx"], p["tiles"])
    return out


def reached(table):
    """the planner branches the table shows, from the stored columns alone"""
    seen = set()
    col = {c: j for j, c in enumerate(COLUMNS)}
    for r in table.reshape(-1, len(COLUMNS)):
        if r[col["error"]]:
            seen.add("refused: " + ERRORS[r[col["error"]] - 1])
            continue
        if not r[col["eligible"]]:
            continue
        name = _lib.B16_KERNELS[r[col["kernel"]]]
        v2 = name.startswith("b16v2-")
        seen.update((name, "v2=%d" % v2))
        if r[col["workspace"]]:
            seen.add("splitk > 1, %d slots" % (256 if v2 else 512))
        if r[col["gx"]] < r[col["tiles"]] and r[col["tiles"]] % r[col["gx"]]:
            seen.add("persistent, uneven")
    return seen


REQUIRED = _lib.B16_KERNELS + ("v2=0", "v2=1", "splitk > 1, 256 slots", "splitk > 1, 512 slots", "persistent, uneven",
                               "refused: straddles", "refused: exceeds the LDS plan", "refused: output too large")


def main():
    table = compute()
    seen = reached(table)
    missing = [b for b in REQUIRED if b not in seen]
    assert not missing, "the grid does not reach: %s" % missing
    assert table.min() >= -1 and table[..., 5].max() <= len(ERRORS)
    path = os.path.join(HERE, "bf16_plans.npz")
    np.savez_compressed(path, **{c: table[..., j] for j, c in enumerate(COLUMNS)})
    print("%d rows x %d knob settings -> %s (%d bytes); reached: %s" % (len(GRID), len(KNOBS), path, os.path.getsize(path),
                                                                         sorted(seen)))


if __name__ == "__main__":
    main()
