#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libs2i_hip.so kernel by kernel (no GPU needed).

    python tools/compare_code_objects.py OLD/libs2i_hip.so NEW/libs2i_hip.so [--arch gfx950] [--show N]

For a change that only moves source between translation units the device code must not change at all.  Every kernel of
both libraries is keyed by its demangled name with `(anonymous namespace)::` removed (a kernel or a parameter type that
moves between an unnamed namespace and a header changes its mangled name, not its code) and the check is:
  * the two sets of kernel names are equal, and no name occurs twice in one library (a kernel compiled in two units);
  * per kernel, the instruction stream is identical (mnemonics, operands and encoding words; addresses and the symbol
    annotations of branch targets are layout, not code, and are dropped);
  * per kernel, the resources are identical: the code object metadata (VGPR / AGPR / SGPR counts, LDS and scratch bytes,
    spill counts, kernarg size, workgroup size limit, argument layout) and the 64-byte kernel descriptor except its
    entry-point offset.
Prints one summary line and exits 1 on any difference, naming the kernels and showing both resource lines.

Needs llvm-objdump and llvm-readelf of the ROCm LLVM ($ROCM_PATH/lib/llvm/bin, default /opt/rocm) and c++filt."""
import argparse
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
RESOURCE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                 "vgpr_spill_count", "sgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size",
                 "uses_dynamic_stack", "wavefront_size")


def llvm_tool(name):
    path = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", name)
    return path if os.path.exists(path) else (shutil.which(name) or sys.exit("%s not found" % name))


def code_objects(lib, arch):
    """The device ELF images for `arch` in the library's offload bundles, one per translation unit that has kernels."""
    data = open(lib, "rb").read()
    if b"CCOB" in data and MAGIC not in data:
        sys.exit("%s: compressed offload bundles; rebuild with --no-offload-compress" % lib)
    out, at = [], data.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        o = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tlen].decode()
            o += 24 + tlen
            if triple.startswith("hip") and triple.endswith(arch) and size:
                out.append(data[at + off:at + off + size])
        at = data.find(MAGIC, at + 1)
    if not out:
        sys.exit("%s: no %s code object found" % (lib, arch))
    return out


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True, **kw).stdout


def instructions(elf):
    """mangled symbol -> list of 'mnemonic operands | encoding words'"""
    syms, cur = {}, None
    for line in run(llvm_tool("llvm-objdump"), "-d", elf).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t") and line.strip() != "...":   # "...": elided padding after a section's last function
            text, _, enc = line.partition("//")
            enc = re.sub(r"<[^>]*>", "", enc.partition(":")[2])        # drop the address and the branch-target annotation
            cur.append(" ".join(text.split()) + " | " + " ".join(enc.split()))
    return syms


def metadata(elf):
    """mangled kernel name -> {key: value of the kernel's metadata map, 'args': argument layout lines} from the
    NT_AMDGPU_METADATA note (a kernel is a list item at indent 2, its keys at indent 4, its argument list deeper)"""
    kernels, cur, in_args = [], None, False
    for line in run(llvm_tool("llvm-readelf"), "--notes", elf).splitlines():
        if line.startswith("  - ."):
            cur = {"args": []}
            kernels.append(cur)
            line = "    " + line[4:]
        if cur is None:
            continue
        if not line.startswith("    "):
            cur = None                                   # the next top-level key ends the kernel list
        elif line.startswith("      "):
            if in_args and ".name:" not in line:
                cur["args"].append(" ".join(line.split()))
        else:
            key, _, val = line.strip().partition(":")
            in_args = key == ".args"
            if not in_args:
                cur[key.lstrip(".")] = val.strip().strip("'")
    return {k["name"]: k for k in kernels}


def descriptors(elf):
    """mangled kernel name -> the 64 descriptor bytes, entry-point offset zeroed"""
    data = open(elf, "rb").read()
    sections = {}
    for line in run(llvm_tool("llvm-readelf"), "-S", "-W", elf).splitlines():
        m = re.match(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            sections[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))
    out = {}
    for line in run(llvm_tool("llvm-readelf"), "-s", "-W", elf).splitlines():
        f = line.split()
        if len(f) == 8 and f[7].endswith(".kd") and f[6].isdigit():
            addr, off = sections[int(f[6])]
            at = off + int(f[1], 16) - addr
            kd = bytearray(data[at:at + 64])
            kd[16:24] = bytes(8)
            out[f[7][:-3]] = bytes(kd)
    return out


def demangle(names):
    names = list(names)
    out = run(shutil.which("c++filt") or llvm_tool("llvm-cxxfilt"), input="\n".join(names) + "\n").splitlines()
    return {n: d.replace("(anonymous namespace)::", "") for n, d in zip(names, out)}


def kernels_of(lib, arch, tmp, tag):
    """normalised demangled name -> list (one entry per defining unit) of (instructions, resources, args, descriptor)"""
    table = {}
    for i, blob in enumerate(code_objects(lib, arch)):
        elf = os.path.join(tmp, "%s_%d.elf" % (tag, i))
        with open(elf, "wb") as fh:
            fh.write(blob)
        ins, meta, kds = instructions(elf), metadata(elf), descriptors(elf)
        if set(meta) != set(kds):
            sys.exit("%s: metadata and descriptor symbols disagree in code object %d" % (lib, i))
        names = demangle(meta)
        for mangled, m in meta.items():
            res = tuple((k, m.get(k)) for k in RESOURCE_KEYS)
            table.setdefault(names[mangled], []).append((ins[mangled], res, tuple(m["args"]), kds[mangled]))
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--show", type=int, default=20, help="differing kernels to print in full")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels_of(args.old, args.arch, tmp, "old"), kernels_of(args.new, args.arch, tmp, "new")
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    dup = sorted(["old: " + n for n in a if len(a[n]) > 1] + ["new: " + n for n in b if len(b[n]) > 1])
    diff_ins, diff_res = [], []
    for n in sorted(set(a) & set(b)):
        (ia, ra, aa, ka), (ib, rb, ab, kb) = a[n][0], b[n][0]
        if ia != ib:
            diff_ins.append(n)
        if (ra, aa, ka) != (rb, ab, kb):
            diff_res.append(n)
    for title, names in (("only in old", only_a), ("only in new", only_b), ("compiled in two units", dup)):
        for n in names:
            print("%s: %s" % (title, n))
    for n in sorted(set(diff_ins) | set(diff_res))[:args.show]:
        (ia, ra, aa, ka), (ib, rb, ab, kb) = a[n][0], b[n][0]
        print("DIFFERS: %s" % n)
        print("  old: %d instructions, %s" % (len(ia), " ".join("%s=%s" % kv for kv in ra)))
        print("  new: %d instructions, %s" % (len(ib), " ".join("%s=%s" % kv for kv in rb)))
        if aa != ab:
            print("  argument layout differs")
        if ka != kb:
            print("  descriptor old %s\n  descriptor new %s" % (ka.hex(), kb.hex()))
        for k, (x, y) in enumerate(zip(ia, ib)):
            if x != y:
                print("  first differing instruction #%d:\n    old %s\n    new %s" % (k, x, y))
                break
    n_ins = sum(len(v[0][0]) for v in a.values())
    print("compare_code_objects: %d kernels old, %d new, %d in both (%d instructions compared); only-old %d, only-new %d, "
          "in two units %d, instruction streams differ %d, resources differ %d"
          % (len(a), len(b), len(set(a) & set(b)), n_ins, len(only_a), len(only_b), len(dup), len(diff_ins), len(diff_res)))
    return 1 if (only_a or only_b or dup or diff_ins or diff_res) else 0


if __name__ == "__main__":
    sys.exit(main())
