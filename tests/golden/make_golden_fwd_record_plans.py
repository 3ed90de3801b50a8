"""How tests/golden/fwd_record_plans.json was made: what every forward record of the edge suites reaches, frozen at the
parent commit (90a2933b; the file's "recorded_at" holds the full hash).

Until s2i_conv_plan_query existed no host query named the kernel a forward convolution launches, and the only record of
which kernel, tile and K split each record of tests/conv_edges.py and tests/image_layer_edges.py reaches was a Python
restatement of the dispatch in those two helper modules (conv_plan in each).  This script froze their answers before the
restatements were deleted: it was run ONCE, in a checkout of that commit with its library built, and wrote for every
fp32-path forward record (fn conv_raw / conv_any, not the bf16 unit's `fast` records, which s2i_conv_bf16_plan_query describes)

  conv_edges          i, id, M, nphases, K, nchunks, splitk, cps, bm (null where the parent could not tell 96 from 128
                      rows), BN, reach (sorted)
  image_layer_edges   i, id, branch, M, nphases, splitk, ppb, blocks, Ho, Wo, reach (sorted)

The file holds integers and names only.  tests/test_fwd_plan_cpu.py compares the helpers' answers, which now come from the
query, with it field by field.  Run today the script would only write down what the query says, so it is kept as
documentation of how the file was made and is not to be run again; a new record is added to the file by hand together with
the reasoning that says which kernel it must reach.

Usage (at the parent commit only):  python tests/golden/make_golden_fwd_record_plans.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)

EDGE_FIELDS = ("M", "nphases", "K", "nchunks", "splitk", "cps", "bm", "BN")
IMAGE_FIELDS = ("branch", "M", "nphases", "splitk", "ppb", "blocks", "Ho", "Wo")


def record(suite, fields):
    rows = []
    for i, rec in enumerate(suite.RECORDS):
        if not rec["fn"].startswith("conv") or rec["fast"]:
            continue
        plan = suite.conv_plan(rec)
        row = dict(i=i, id=suite.record_id(i, rec))
        row.update((f, plan[f]) for f in fields)
        row["reach"] = sorted(plan["reach"])
        rows.append(row)
    return rows


def main():
    import subprocess
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import conv_edges
    import image_layer_edges
    head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
    out = dict(recorded_at=head, conv_edges=record(conv_edges, EDGE_FIELDS),
               image_layer_edges=record(image_layer_edges, IMAGE_FIELDS))
    path = os.path.join(HERE, "fwd_record_plans.json")
    with open(path, "w") as f:
        f.write("{\n \"recorded_at\": %s,\n" % json.dumps(head))
        for k, name in enumerate(("conv_edges", "image_layer_edges")):
            f.write(" %s: [\n%s\n ]%s\n" % (json.dumps(name), ",\n".join("  " + json.dumps(r) for r in out[name]),
                                            "," if k == 0 else ""))
        f.write("}\n")
    print("%d + %d records at %s -> %s (%d bytes)" % (len(out["conv_edges"]), len(out["image_layer_edges"]), head, path,
                                                     os.path.getsize(path)))


if __name__ == "__main__":
    main()
