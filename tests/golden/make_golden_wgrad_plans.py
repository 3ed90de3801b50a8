"""Generate tests/golden/wgrad_plans.npz: what the weight-gradient planner answers over a grid of descriptors.

plan_wgrad (csrc/s2i_wgrad_plan.hip) is host code and the library loads without a device, so the table is, for every
descriptor of GRID under every (operand mode, knob setting) of SETTINGS: the three workspace queries
s2i_wgrad_workspace_bytes / _dt / _split (as the number of K x N fp32 slabs: the bytes must be a whole number of them),
s2i_conv_wgrad_in_eligible, the twelve outputs of s2i_wgrad_plan_query (kernel,
tile, block, grid, stage pixels, slabs launched and held, K, M) and, where the plan refuses the layer in that mode, which
S2I_REQUIRE family said so (ERRORS, matched against s2i_last_error()).  The file holds integers only.  It pins the planner
across changes that must not move a plan: run this once BEFORE such a change, commit the file, and
tests/test_wgrad_plan_cpu.py recomputes the table with the functions below and compares row by row.

main() also asserts that the grid reaches what is worth guarding: every kernel, the 256 x 128 and 256 x 256 tiles each chosen
by the cost model alone (fp32 and bf16), a bf16 launch that writes fewer slabs than the workspace holds, the first
discriminator convolution's one-block grid, every refusal family of ERRORS.

Usage:  python tests/golden/make_golden_wgrad_plans.py            (writes next to this file; needs the built library)
"""
import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

K1, K3S1, K4S2, UP = 0, 1, 2, -1                 # s2i_conv_kind of include/s2i_hip.h; UP: the up layer's K4S2 with swap + fold
KINDS = (K1, K3S1, K4S2, UP)
BATCHES = (1, 3, 5, 24, 48, 72, 144)
EXTENTS = (1, 8, 32, 128)                        # H = W (the stride-2 kinds start at 2: their output map must not be empty)
CAS = (4, 16, 32, 40, 64, 96, 128, 160, 256, 512)
NS = (4, 8, 32, 40, 64, 96, 128, 136, 256, 512)
# rows: (kind, B, H = W, Ca, N, Cc, ldg - N)
GRID = tuple(r + (0, 0) for r in itertools.product(KINDS, BATCHES, EXTENTS, CAS, NS)) + \
    tuple(r + (32, 0) for r in itertools.product((K1, K3S1), (3, 24), (8, 32), CAS, NS)) + \
    tuple(r + (0, 8) for r in itertools.product((K3S1, K4S2), (5, 48), (8, 128), CAS, NS)) + \
    tuple(r + (0, -4) for r in itertools.product((K3S1,), (5,), (8,), (32,), NS))
F32, BF16, LRELU = 0, 1, 2
# operand modes: (name, a_dtype, g_dtype, planes, in_act, a_groups)
MODES = {"f32": (F32, F32, 0, 0, 0), "a16": (BF16, F32, 0, 0, 0), "g16": (F32, BF16, 0, 0, 0), "b16": (BF16, BF16, 0, 0, 0),
         "planes1": (F32, F32, 1, 0, 0), "planes2": (F32, F32, 2, 0, 0), "planes3": (F32, F32, 3, 0, 0),
         "in-g1": (F32, F32, 0, LRELU, 1), "in-g3": (F32, F32, 0, LRELU, 3)}
# the knobs act on one mode each: wgrad_bm on fp32 operands, wgrad16_bm on two bf16 operands
SETTINGS = tuple([("f32", {})] + [("f32", {"wgrad_bm": v}) for v in (1, 128, 256, 512)] +
                 [("b16", {})] + [("b16", {"wgrad16_bm": v}) for v in (128, 256, 512)] +
                 [(m, {}) for m in MODES if m not in ("f32", "b16")])
# the S2I_REQUIRE families this grid reaches (code = index + 1; 0 = the plan was made)
ERRORS = ("ldg < N", "expects an fp32 output gradient", "apply-on-load")
PLAN = ("kernel", "bm", "bn", "threads", "gx", "gy", "gz", "stage", "slabs", "ws_slabs", "K", "M")
COLUMNS = ("workspace", "workspace_dt", "workspace_split", "in_eligible") + PLAN + ("error",)
# the WgKernel values of csrc/s2i_igemm.h, in order
KERNELS = ("f32-128x128", "f32-128x64", "f32-128x32", "f32-64x64", "f32-256x128", "f32-256x256", "f32-96x64", "f32-96x32",
           "f32in-128x128", "b16-128x128", "b16-128x64", "b16-128x32", "b16-64x64", "b16-256x128", "b16-256x256",
           "b16d1-64x64", "split-128x128", "split-128x64", "split-128x32", "split-64x64", "rows3-32x64", "rows3-32x32",
           "rows3-64x128", "rows3-64x64", "rows3-64x32", "smalln-16", "smalln-32", "smalln-64")


def describe(row, setting):
    return "kind=%d B=%d H=W=%d Ca=%d N=%d Cc=%d ldg=N%+d mode=%s knobs=%r" % (row + setting)


def descriptor(_lib, row, mode):
    kind, B, HW, Ca, N, Cc, dldg = row
    a_act, a_groups = MODES[mode][3:]
    if kind == UP:      # a is the output gradient (Ca = O channels), g the layer's input (N = I channels), 3x3 parameter
        return _lib.WgradDesc(K4S2, B, max(HW, 2), max(HW, 2), Ca, 0, N, N + dldg, 1, 1, Ca, N, 3, 3, 0, 0, 0, a_act, a_groups)
    if kind == K4S2:
        HW = max(HW, 2)
    k = {K1: 1, K3S1: 3, K4S2: 4}[kind]
    return _lib.WgradDesc(kind, B, HW, HW, Ca, Cc, N, N + dldg, 0, 0, N, Ca + Cc, k, k, 0, 0, 0, a_act, a_groups)


def compute():
    """int64 array [len(GRID)][len(SETTINGS)][len(COLUMNS)]"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    out = np.zeros((len(GRID), len(SETTINGS), len(COLUMNS)), dtype=np.int64)
    plan = (ctypes.c_int * 12)()
    for k, (mode, knobs) in enumerate(SETTINGS):
        a_dt, g_dt, planes, in_act, _ = MODES[mode]
        with _lib.tuning(**knobs):
            for i, row in enumerate(GRID):
                desc = descriptor(_lib, row, mode)
                d = ctypes.byref(desc)
                slab = {K1: 1, K3S1: 9, K4S2: 16}[desc.kind] * (desc.Ca + desc.Cc) * desc.N * 4
                err = 0
                if lib.s2i_wgrad_plan_query(d, a_dt, g_dt, planes, in_act, ctypes.byref(plan)):
                    msg = lib.s2i_last_error().decode()
                    hits = [j + 1 for j, e in enumerate(ERRORS) if e in msg]
                    assert len(hits) == 1, "%s: unexpected refusal %r" % (describe(row, SETTINGS[k]), msg)
                    err = hits[0]
                ws = (lib.s2i_wgrad_workspace_bytes(d), lib.s2i_wgrad_workspace_bytes_dt(d, a_dt, g_dt),
                      lib.s2i_wgrad_workspace_bytes_split(d, planes))
                assert not any(b % slab for b in ws), "%s: workspaces %r are not whole slabs" % (describe(row, SETTINGS[k]), ws)
                out[i, k] = tuple(b // slab for b in ws) + (lib.s2i_conv_wgrad_in_eligible(d),) + tuple(plan) + (err,)
    return out


def reached(table):
    """what the table shows, from the stored results alone"""
    seen = set()
    col = {c: j for j, c in enumerate(COLUMNS)}
    default = {mode: k for k, (mode, knobs) in enumerate(SETTINGS) if not knobs}
    for k, (mode, knobs) in enumerate(SETTINGS):
        for i, row in enumerate(GRID):
            r = table[i, k]
            if r[col["error"]]:
                seen.add("refused: " + ERRORS[r[col["error"]] - 1])
                continue
            name = KERNELS[r[col["kernel"]]]
            seen.add(name)
            if not knobs and name.endswith(("256x128", "256x256")):
                seen.add("model picks " + name)
            if r[col["slabs"]] < r[col["ws_slabs"]]:
                assert r[col["stage"]] == 64, describe(row, SETTINGS[k])
                seen.add("fewer slabs launched than held")
            if name == "b16d1-64x64":
                # the same layer with an fp32 gradient keeps the 32-pixel plan; this one re-cuts it in 64-pixel stages
                other = table[i, default["f32"]]
                assert r[col["ws_slabs"]] == other[col["slabs"]] == other[col["gz"]], describe(row, SETTINGS[k])
                if (r[col["gx"]], r[col["gy"]]) == (1, 1) and r[col["gz"]] == r[col["slabs"]] < other[col["gz"]]:
                    seen.add("first-D-conv override")
    return seen


REQUIRED = KERNELS + ("model picks f32-256x128", "model picks f32-256x256", "model picks b16-256x128", "model picks b16-256x256",
                      "fewer slabs launched than held", "first-D-conv override") + tuple("refused: " + e for e in ERRORS)


def main():
    table = compute()
    seen = reached(table)
    missing = [b for b in REQUIRED if b not in seen]
    assert not missing, "the grid does not reach: %s" % missing
    assert table.min() >= 0 and table[..., -1].max() <= len(ERRORS)
    path = os.path.join(HERE, "wgrad_plans.npz")
    assert table.max() < 2 ** 31
    np.savez_compressed(path, **{c: table[..., j].astype(np.int32) for j, c in enumerate(COLUMNS)})
    print("%d rows x %d settings -> %s (%d bytes); reached: %s" % (len(GRID), len(SETTINGS), path, os.path.getsize(path),
                                                                  sorted(seen)))


if __name__ == "__main__":
    main()
