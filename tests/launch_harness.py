"""The harness the launch-replay suites share (test_step_launches_gpu, test_step_elementwise_gpu,
test_encoder_launches_gpu, test_eval_launches_gpu): launch records and census files, the recorders that take a census,
the element-wise comparison against fp64, and the ledger of worst measured values each suite prints at its end.

A suite owns one Ledger and passes it to every replay it runs, so a value measured during a test of a module is printed
by that module, whichever module the replay code lives in."""
import ctypes
import functools
import json
import os
import time
import zlib

import pytest
import torch

from helpers import CASES, build_nets, make_batch
from speech_to_image_translation_without_text_amd import _lib

BF16_ROUND = 2.0 ** -8       # round to nearest bf16 (8 significant bits): |rounded - v| <= 2^-8 |v|
U = 2.0 ** -24               # fp32 unit roundoff
GUARD_BYTES = 256            # margin on both sides of a guarded output buffer (a multiple of every alignment in use)
GUARD_BYTE = 0xA5            # its fill: a fixed bit pattern compared as integers (no NaN, and any float added to it shows)

# the train step's workloads, mode name -> (case, bf16 activations): BASELINE configs 2 and 4
STEP_MODES = {
    "fp32_b24": (dict(CASES["full3_fwd"], B=24), False),
    "bf16_b48": (dict(CASES["full3_fwd"], B=48), True),
}


# ---- records and census files ----------------------------------------------------------------------------------------
def canon(rec):
    return json.dumps(rec, sort_keys=True)


def dedup(recs):
    """The distinct records, sorted by their canonical JSON."""
    return [json.loads(s) for s in sorted({canon(r) for r in recs})]


@functools.lru_cache(maxsize=None)
def load_census(path):
    if not os.path.exists(path):
        return {}
    with open(path) as fp:
        return json.load(fp)


def write_census(path, census):
    with open(path, "w") as fp:
        fp.write("{\n" + ",\n".join('  "%s": [\n%s\n  ]' % (m, ",\n".join("    " + canon(r) for r in recs))
                                    for m, recs in census.items()) + "\n}\n")
    load_census.cache_clear()


def assert_census_equal(live, committed, keys, filename):
    for key in keys:
        have = {canon(r) for r in committed.get(key, [])}
        now = {canon(r) for r in live[key]}
        assert now == have, "%s: launches not in tests/%s: %s; listed but not launched: %s" % (
            key, filename, sorted(now - have)[:5], sorted(have - now)[:5])


def gen_rec(dev, rec):
    """The generator a record's replay draws its operands from."""
    return torch.Generator(device=dev).manual_seed(zlib.crc32(canon(rec).encode()))


def gen_key(dev, *key):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(repr(key).encode()))


# ---- recording -------------------------------------------------------------------------------------------------------
class LibRecorder:
    """Stands in for the ctypes library: every s2i_* entry point that `passed` does not let through is wrapped and its
    call appended to recs as {"fn": name, argument: value, ...}.  args[name] lists the argument names (include/s2i_hip.h
    order, the trailing stream left out); arguments named in skip are not recorded.  A pointer is recorded as whether it
    is non-NULL, or with null_ok=False required to be non-NULL and left out; a descriptor passed by reference field by
    field; a scalar by value."""

    def __init__(self, lib, recs, args, passed, skip=(), null_ok=True,
                 unlisted="entry point %s has no argument list in ARGS (and no replay)"):
        self._lib, self._recs, self._args, self._passed = lib, recs, args, passed
        self._skip, self._null_ok, self._unlisted = skip, null_ok, unlisted

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("s2i_") or self._passed(name):
            return fn
        assert name in self._args, self._unlisted % name
        names = self._args[name].split()
        types = _lib._SIGNATURES[name][1]

        def call(*args):
            assert len(args) == len(names) + 1, (name, len(args))
            rec = {"fn": name}
            for n, t, v in zip(names, types, args):
                if n in self._skip:
                    continue
                if t is ctypes.c_void_p:
                    if self._null_ok:
                        rec[n] = not (v is None or (isinstance(v, int) and v == 0))
                    else:
                        assert v, "%s: NULL %s" % (name, n)
                elif hasattr(v, "_obj"):                 # byref(descriptor): field by field
                    rec[n] = {f: int(getattr(v._obj, f)) for f, _ in v._obj._fields_}
                elif t is ctypes.c_float:
                    rec[n] = float(ctypes.c_float(v).value)
                else:
                    rec[n] = int(v)
            self._recs.append(rec)
            return fn(*args)
        return call


class ModuleSpy:
    """A module's view of the _lib module, with load() handing out the recording library."""

    def __init__(self, lib):
        self._spy = lib

    def load(self):
        return self._spy

    def __getattr__(self, name):
        return getattr(_lib, name)


def install(mp, proxy, *modules):
    """Every library call of ops.py, and of the modules given (which load the library themselves), goes through proxy."""
    from speech_to_image_translation_without_text_amd import ops
    mp.setattr(ops, "_lib_ready", lambda: (_lib.require_device(), proxy)[1])
    for m in modules:
        mp.setattr(m, "_lib", ModuleSpy(proxy))


def record_train_step(gpu, case, bf16, mp, install_recorder):
    """One eager train_step (the pattern of test_bf16_gpu._run_steps) with install_recorder(mp, recs) in place -> recs."""
    from speech_to_image_translation_without_text_amd import ops, trainer as T
    recs = []
    install_recorder(mp, recs)
    mp.setattr(ops, "ACT_BF16", bf16)
    netG, netsD = build_nets(case)
    batch = make_batch(case)
    netG.to(gpu)
    for d in netsD:
        d.to(gpu)
    tr = T.condGANTrainer(None, None, 256, False)
    tr.build(netG, netsD)
    b = {k: ([t.to(gpu) for t in v] if isinstance(v, list) and torch.is_tensor(v[0]) else
             (v.to(gpu) if torch.is_tensor(v) else v)) for k, v in batch.items()}
    emb = b["emb"].clone().requires_grad_(True)
    tr.train_step(b["real"], b["wrong"], emb, batch["labels"], b["noise"], b["eps"])
    torch.cuda.synchronize()
    return recs


def take_step_census(gpu, modes, install_recorder):
    """{mode: deduplicated, sorted list of records}, and {mode: recorded calls per step}; modes maps a name to
    (case, bf16 activations)."""
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0 and not ops.DEFER_ACT, "census needs the default paths"
    out, calls = {}, {}
    for mode, (case, bf16) in modes.items():
        with pytest.MonkeyPatch.context() as mp:
            recs = record_train_step(gpu, case, bf16, mp, install_recorder)
        calls[mode] = len(recs)
        out[mode] = dedup(recs)
        torch.cuda.empty_cache()
    return out, calls


# ---- ledger ----------------------------------------------------------------------------------------------------------
class Ledger:
    """What one suite measured: the worst value per family with the bound in use there, and how often each mutation was
    rejected."""

    def __init__(self):
        self.worst, self.rejected, self.t0 = {}, {}, time.time()

    def start(self):
        self.t0 = time.time()

    def note(self, fam, value, what="", bound=None):
        if fam not in self.worst or value > self.worst[fam][0]:
            self.worst[fam] = (value, bound, what)

    def reject(self, mutation):
        self.rejected[mutation] = self.rejected.get(mutation, 0) + 1

    def report(self, title):
        print("\n%s, %.0f s: worst measured value per family (bound in use)" % (title, time.time() - self.t0))
        for fam in sorted(self.worst):
            value, bound, what = self.worst[fam]
            print("  %-28s %.3e  (%s)  %s" % (fam, value, "-" if bound is None else "%.3e" % bound, what))
        print("mutations rejected (family: mutation, cases):")
        for k in sorted(self.rejected):
            print("  %-64s %d" % (k, self.rejected[k]))


# ---- comparison ------------------------------------------------------------------------------------------------------
def compare(out, ref, absref, rnd, gamma):
    """(ratio, ok): ratio = max (|out - ref| - rnd |ref|) / absref, the gamma this element needs."""
    err = (out - ref).abs() - rnd * ref.abs()
    ratio = float((err / absref.clamp_min(1e-300)).clamp_min(0).max()) if err.numel() else 0.0
    return ratio, bool((err <= gamma * absref).all())


def fails(out, mref, absref, rnd, gamma):
    return not compare(out, mref, absref, rnd, gamma)[1]


class Check:
    """Collects the comparisons of one test against the gamma table of its suite, notes them in the ledger; done() raises
    with every failure, a write into the margins of a watched buffer among them."""

    def __init__(self, what, gammas, ledger):
        self.what, self.gammas, self.ledger, self.bad, self.watched = what, gammas, ledger, [], []

    def watch(self, buf, margin, nbytes):
        """buf: uint8, GUARD_BYTE throughout when handed out; the bytes [margin, margin + nbytes) belong to the test."""
        self.watched.append((buf, margin, nbytes))

    def close(self, fam, name, out, ref, absref, rnd=0.0, mutants=None):
        out, ref, absref = out.double(), ref.double(), torch.as_tensor(absref, dtype=torch.float64, device=ref.device)
        absref = absref.expand_as(ref)
        gamma = self.gammas[fam]
        ratio, ok = compare(out, ref, absref, rnd, gamma)
        self.ledger.note(fam, ratio, "%s %s" % (self.what, name), gamma)
        print("%s %s: ratio %.3e (gamma %.1e)" % (self.what, name, ratio, gamma))
        if not ok:
            self.bad.append("%s: element error %.3e x absref > gamma %.1e" % (name, ratio, gamma))
        for mname, mref in (mutants or {}).items():
            if compare(out, mref.double(), absref, rnd, gamma)[1]:
                self.bad.append("%s: the bound cannot see the mutation '%s'" % (name, mname))
            else:
                self.ledger.reject("%s: %s" % (fam, mname))

    def equal(self, name, out, ref):
        if not torch.equal(out, ref):
            n = int((out != ref).sum()) if out.shape == ref.shape else -1
            self.bad.append("%s: not bit-identical (%d elements differ)" % (name, n))

    def done(self):
        for i, (buf, margin, nbytes) in enumerate(self.watched):
            for side, m in (("before", buf[:margin]), ("past the end of", buf[margin + nbytes:])):
                hit = int((m != GUARD_BYTE).sum())
                if hit:
                    self.bad.append("%d guard bytes %s output %d (%d bytes) were written" % (hit, side, i, nbytes))
        assert not self.bad, "%s: %s" % (self.what, "; ".join(self.bad))


# ---- small operand helpers -------------------------------------------------------------------------------------------
def dyadic(shape, gen, dev):
    """Integers in [-16, 16] times 2^-6: exact in bf16, and so are the sums of four of them."""
    return torch.randint(-16, 17, tuple(shape), generator=gen, device=dev).float() * 2.0 ** -6


def P(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args, _lib.stream()), name)
    torch.cuda.synchronize()


def nchw(t):
    return t.permute(0, 3, 1, 2)
