"""The weight re-pack kernels, single and batched, bit for bit against plain references.

Every convolution reads weights that went OIHW -> P[tap][Ip][Op] (pack_weight_kernel, or pack_weight_batched_kernel for a
whole network) and, in bf16 mode, P -> Wb[phase][chunk][tap][Npad][CK] (pack_bf16_kernel / pack_bf16_batched_kernel).  The
replay suites set the s2i_pack* launches aside and prepare their operands with the single-weight kernels; after its first
iteration training runs only the batched ones, whose bodies (pack_bf16_strip, the item lookup, the tables ops.refresh_packed
and ops._refresh_bf16 build) nothing else runs, and which only whole-step tolerance tests reached.  A block, strip tile or
tail that is not written keeps last step's weights, within lr of the right ones: only an exact comparison over a poisoned
destination sees that.  Both operations are permutations plus zero padding, one RNE rounding (bf16) or a sum of at most four
terms (UPFOLD), so every comparison here is bit for bit, with one derived exception (standard normal values under UPFOLD).

  * Single fp32 packer: every record of weight_pack_ref.CASES_F32 x index-coded, dyadic and standard normal values.
  * Single bf16 packer, and the batched kernel on a table of that one item through the C entry points: every record of
    CASES_B16, standard normal P with the rounding specials of the splitter test at both ends of the matrix.
  * Network: parameters over CASES_F32 (the misaligned views and the masters packed in both modes among them) and the
    masters of CASES_B16 with the forward and, where the kernels take it, the input-gradient descriptor, through
    ops.packed_weight / ops.bf16_weight / ops.refresh_packed: masters overwritten, every copy poisoned, one refresh, every
    copy equal to the reference and to the single-weight kernels; twice, the second time from the cached device tables.
  * Item lookup: the same procedure on a table of one item, on a table whose first and last fp32 items own one block (the
    smallest bf16 item owns nine: one strip x nine taps), and on a table of 34 parameters.
  * Cache bookkeeping: ops.bf16_weight hands out the refreshed tensor; a conv_any forward through it equals the forward on
    freshly packed weights and differs from the one on the previous masters; ops.invalidate_derived re-derives the same bits;
    a table is not reused for other shapes at the same addresses.
  * Power: the kernels are never broken; each comparison must FAIL against wrong references (flip ignored, wmode ignored,
    parities exchanged, chunk and tap exchanged, padding left at the sentinel, the pack of the previous masters).

Destinations lie between guard margins; destination and margins hold a sentinel (a NaN pattern for fp32, 0x5A5A for bf16)
before each call and the whole buffer is compared, so padding must come out zero and the margins untouched.

Measured on one MI355X: 19 fp32 and 23 bf16 records; a network of 37 parameters, 39 packed tensors and 33 bf16 copies; lookup
tables of 1, 7 and 37 fp32 items (1, 6 and 42 bf16 items); 936 bit-exact comparisons; 882 wrong references rejected, none
accepted (fp32 single 81, bf16 single 69, one-item table 69, network 280, item lookup 380, cache 3); standard normal values
under UPFOLD at most 1.3e-7 of sum |terms| (bound 4 x 2^-24 = 2.4e-7).  The four kernels agreed with the references and with
each other at first contact.  One host bug was found: ops.refresh_packed and ops._refresh_bf16 cached their device tables
by addresses alone, so parameters and packed copies at the addresses of a dead network of other shapes were re-packed with
the dead network's shapes (558 of 576 elements wrong in test_tables_are_not_reused_for_other_shapes_at_the_same_addresses);
the shapes are part of the key now.  50 tests, about 4 s."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import launch_harness as LH  # noqa: E402
import split_planes as S  # noqa: E402
import weight_pack_ref as W  # noqa: E402
from launch_harness import P  # noqa: E402
from speech_to_image_translation_without_text_amd._lib import PACK_PLAIN, PACK_UPFOLD  # noqa: E402

pytestmark = pytest.mark.gpu

LEDGER = LH.Ledger()
COUNTS = {}                 # family -> [records, bit-exact comparisons]
GUARD = 256                 # elements of margin on both sides of a destination
F32_IDS = [W.f32_id(i) for i in range(len(W.CASES_F32))]
B16_IDS = [W.b16_id(i) for i in range(len(W.CASES_B16))]
SPECIALS = [0.0, -0.0, 1 + 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8, (1 + 2.0 ** -8) * 2.0 ** -9,
            1 + 2.0 ** -8 + 2.0 ** -16, 1 + 2.0 ** -8 + 2.0 ** -23, S.PROBE_C, -S.PROBE_C]


@pytest.fixture(scope="module", autouse=True)
def _report():
    LEDGER.start()
    yield
    LEDGER.report("weight re-pack kernels")
    print("family: records, bit-exact comparisons")
    for fam in sorted(COUNTS):
        print("  %-28s %4d %6d" % (fam, COUNTS[fam][0], COUNTS[fam][1]))


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _count(fam, records=0, comparisons=0):
    c = COUNTS.setdefault(fam, [0, 0])
    c[0] += records
    c[1] += comparisons


def _bits(t):
    """The elements of a tensor as integers (NaN patterns and the sign of zero compare)."""
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).reshape(-1)


def _same(chk, fam, name, out, ref):
    chk.equal(name, _bits(out), _bits(ref).to(out.device))
    _count(fam, comparisons=1)


def _differs(chk, fam, name, out, wrong, mutation):
    """The comparison that holds the kernel must fail against a wrong reference."""
    if torch.equal(_bits(out), _bits(wrong).to(out.device)):
        chk.bad.append("%s: the comparison cannot see the mutation '%s'" % (name, mutation))
    else:
        LEDGER.reject("%s: %s" % (fam, mutation))


def _guarded(n, dtype, dev):
    """(whole, dest): dest is a tensor of n elements of dtype between two margins, all of it filled with the sentinel."""
    itype, fill = (torch.int32, W.SENTINEL_F32) if dtype == torch.float32 else (torch.int16, W.SENTINEL_B16)
    whole = torch.full((n + 2 * GUARD,), fill, dtype=itype, device=dev)
    dest = whole[GUARD:GUARD + n].view(dtype)
    assert dest.data_ptr() % 16 == 0
    return whole, dest


def _framed(ref, whole):
    """The reference of a whole guarded buffer: the sentinel margins around the reference of the destination."""
    ref = _bits(ref).to(whole.device)
    fill = W.SENTINEL_F32 if whole.dtype == torch.int32 else W.SENTINEL_B16
    m = torch.full((GUARD,), fill, dtype=whole.dtype, device=whole.device)
    assert ref.dtype == whole.dtype
    return torch.cat((m, ref, m))


def _poison(t):
    _bits(t).fill_(W.SENTINEL_F32 if t.element_size() == 4 else W.SENTINEL_B16)      # a view: t is filled


def _sentinels(t):
    return int((_bits(t) == (W.SENTINEL_F32 if t.element_size() == 4 else W.SENTINEL_B16)).sum())


def _place(shape, values, misaligned, dev):
    """A contiguous fp32 tensor of this shape holding values; misaligned: a view one float into a larger buffer."""
    n = values.numel()
    if misaligned:
        t = torch.zeros(n + 8, dtype=torch.float32, device=dev)[1:1 + n].view(shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    else:
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        assert t.data_ptr() % 16 == 0
    t.copy_(values.view(shape))
    return t


def _fine(shape, gen, dev):
    """Integers in [-2^20, 2^20] times 2^-22: 21 significant bits, so the bf16 rounding is a real one, and every sum of four
    of them is exact in fp32 in any order."""
    return torch.randint(-2 ** 20, 2 ** 20 + 1, tuple(shape), generator=gen, device=dev).float() * 2.0 ** -22


def _pad_sentinel_f32(ref, O, I):
    bad = _bits(ref.float()).view(ref.shape).clone()
    bad[:, I:, :] = W.SENTINEL_F32
    bad[:, :, O:] = W.SENTINEL_F32
    return bad


def _b16_source(c, gen, dev, specials=True):
    """Standard normal P[Tsrc][R][C] of a record, the rounding specials at the first and the last elements of the matrix the
    kernel reads (tap 0 and the last tap)."""
    Tsrc, R, C = W.b16_source_shape(c)
    Pt = _place((Tsrc, R, C), torch.randn(Tsrc * R * C, generator=gen, device=dev), c.misaligned, dev)
    if specials:
        rows, cols = (c.N, c.Cx) if c.wmode else (c.Cx, c.N)
        for j, v in enumerate(SPECIALS):
            r, q = divmod(j, cols)
            Pt[0, c.Cc + r, q] = v
            r, q = divmod(rows * cols - len(SPECIALS) + j, cols)
            Pt[Tsrc - 1, c.Cc + r, q] = v
    return Pt


def _b16_ref(c, plan, Pt, mutate=None):
    return W.pack_bf16_ref(Pt.cpu(), c.kind, c.wmode, c.flip, c.Cx, c.N, plan["npad"], plan["ck"], w_offset=W.b16_w_offset(c),
                           mutate=mutate)


def _single_bf16(c, Pt, out):
    _, R, C = W.b16_source_shape(c)
    LH.call("s2i_pack_conv_weight_bf16", ctypes.byref(W.b16_desc(c)), P(Pt) + 4 * W.b16_w_offset(c), R, C, P(out))


# ---- the single fp32 packer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(W.CASES_F32)), ids=F32_IDS)
def test_single_fp32_packer(gpu, index):
    c = W.CASES_F32[index]
    fam = "fp32 single"
    shape = W.f32_shape(c)
    n = c.O * c.I * c.KH * c.KW
    gen = LH.gen_key(gpu, "pack f32", index)
    Ip, Op = W.roundup4(c.I), W.roundup4(c.O)
    T = 16 if c.mode == PACK_UPFOLD else c.KH * c.KW
    chk = LH.Check("pack %s" % F32_IDS[index], {}, LEDGER)
    other = W.pack_ref(torch.randn(shape, generator=gen, device=gpu), c.mode)[0]
    for name, values in (("index coded", torch.arange(n, dtype=torch.float32, device=gpu)),
                         ("dyadic", LH.dyadic((n,), gen, gpu)),
                         ("normal", torch.randn(n, generator=gen, device=gpu))):
        w = _place(shape, values, c.misaligned, gpu)
        whole, out = _guarded(T * Ip * Op, torch.float32, gpu)
        LH.call("s2i_pack_conv_weight", P(w), P(out), c.O, c.I, c.KH, c.KW, Ip, c.mode)
        val, mag = W.pack_ref(w, c.mode)
        exact = c.mode == PACK_PLAIN or name != "normal"      # integers below 2^20 and dyadic values: every sum is exact
        if exact:
            assert torch.equal(val.float().double(), val)
            _same(chk, fam, name, whole, _framed(val.float(), whole))
            if Ip > c.I or Op > c.O:
                _differs(chk, fam, name, whole, _framed(_pad_sentinel_f32(val, c.O, c.I), whole), "padding left at the sentinel")
            _differs(chk, fam, name, whole, _framed(other.float(), whole), "the pack of other masters")
        else:
            # up to four terms added in fp32: three additions to first order and one for slack, 4 u sum |terms|; where there
            # are no terms (padding) the bound is zero
            bound = 4 * LH.U * mag
            got = out.view(T, Ip, Op).double()
            err = (got - val).abs()
            ratio = float((err / mag.clamp_min(1e-300)).max())
            print("pack %s %s: worst |error| / sum |terms| %.3e (bound %.3e)" % (F32_IDS[index], name, ratio, 4 * LH.U))
            LEDGER.note("fp32 upfold, normal values", ratio, F32_IDS[index], 4 * LH.U)
            if not bool((err <= bound).all()):
                chk.bad.append("%s: %d elements beyond 4 u sum |terms|" % (name, int((~(err <= bound)).sum())))
            chk.equal(name + ": padding", _bits(out)[(mag == 0).reshape(-1)], torch.zeros(int((mag == 0).sum()), dtype=torch.int32,
                                                                                      device=gpu))
            chk.equal(name + ": margins", torch.cat((whole[:GUARD], whole[-GUARD:])),
                      torch.full((2 * GUARD,), W.SENTINEL_F32, dtype=torch.int32, device=gpu))
            if bool(((other - val).abs() <= bound).all()):
                chk.bad.append("%s: the bound cannot see the pack of other masters" % name)
            else:
                LEDGER.reject("%s: the pack of other masters" % fam)
    _count(fam, records=1)
    chk.done()


# ---- the single bf16 packer, and the batched kernel on a table of that item ------------------------------------------
@pytest.mark.parametrize("index", range(len(W.CASES_B16)), ids=B16_IDS)
def test_single_and_one_item_bf16_packer(gpu, index):
    from speech_to_image_translation_without_text_amd import _lib
    c = W.CASES_B16[index]
    plan = W.b16_plan(c)
    gen = LH.gen_key(gpu, "pack b16", index)
    n = plan["w_elems"]
    _, R, C = W.b16_source_shape(c)
    Pt = _b16_source(c, gen, gpu)
    ref = _b16_ref(c, plan, Pt)
    wrong = {m: _b16_ref(c, plan, Pt, mutate=m) for m in W.b16_mutations(c, plan)}
    wrong["the pack of other masters"] = _b16_ref(c, plan, _b16_source(c, gen, gpu, specials=False))
    chk = LH.Check("pack bf16 %s" % B16_IDS[index], {}, LEDGER)

    def judge(fam, whole):
        _same(chk, fam, fam, whole, _framed(ref, whole))
        for m, bad in wrong.items():
            _differs(chk, fam, fam, whole, _framed(bad, whole), m)
        _count(fam, records=1)

    whole, out = _guarded(n, torch.bfloat16, gpu)
    _single_bf16(c, Pt, out)
    judge("bf16 single", whole)
    # the strip kernel on a table of this one item, as ops._refresh_bf16 builds it
    whole2, out2 = _guarded(n, torch.bfloat16, gpu)
    item = _lib.Pack16Item()
    nb = _lib.load().s2i_pack16_item_fill(ctypes.byref(W.b16_desc(c)), P(Pt) + 4 * W.b16_w_offset(c), R, C, P(out2),
                                          ctypes.byref(item))
    assert nb == item.gx * item.gy * item.nphase * item.T and item.block0 == 0, nb
    table = torch.frombuffer(bytearray(bytes(item)), dtype=torch.uint8).to(gpu)
    LH.call("s2i_pack_conv_weights_bf16_batched", P(table), 1, nb)
    judge("bf16 one-item table", whole2)
    chk.equal("strip kernel == block kernel", whole2, whole)
    chk.done()


# ---- batched == single == reference through the production entry points ---------------------------------------------
def _f32_specs():
    """One parameter per distinct master of CASES_F32, packed in every mode the table asks of it."""
    specs = {}
    for c in W.CASES_F32:
        specs.setdefault((W.f32_shape(c), c.misaligned), []).append(c.mode)
    return [dict(shape=s, misaligned=m, modes=sorted(set(modes)), b16=[]) for (s, m), modes in specs.items()]


def _b16_specs(cases):
    """One parameter per in-network record of CASES_B16, with the record and its other direction where the kernels take it."""
    specs = []
    for c in cases:
        if W.b16_in_network(c):
            shape, mode = W.b16_master(c)
            o = W.b16_counterpart(c)
            specs.append(dict(shape=shape, misaligned=False, modes=[mode], b16=[c] + ([o] if o is not None else [])))
    return specs


def _run_network(gpu, what, fam, specs, rounds=2):
    """Steps 1 - 10 of the procedure in the module docstring on the parameters of specs."""
    from speech_to_image_translation_without_text_amd import ops
    gen = LH.gen_key(gpu, "network", what)
    chk = LH.Check(what, {}, LEDGER)
    params, packs, copies = [], [], []       # packs: (param index, mode, packed); copies: (pack index, record, plan, desc, ent)
    for s in specs:
        p = torch.nn.Parameter(_place(s["shape"], _fine((int(torch.Size(s["shape"]).numel()),), gen, gpu), s["misaligned"], gpu))
        assert p.data_ptr() % 16 == (4 if s["misaligned"] else 0)
        params.append(p)
        for mode in s["modes"]:
            packed = ops.packed_weight(p, mode)
            packs.append((len(params) - 1, mode, packed))
            for c in s["b16"]:
                assert tuple(packed.shape) == W.b16_source_shape(c), (c, packed.shape)
                d = W.b16_desc(c)
                ent = ops.bf16_weight(packed, d, W.b16_w_offset(c))
                copies.append((len(packs) - 1, c, W.b16_plan(c), d, ent))
    assert len({e.data_ptr() for *_, e in copies}) == len(copies), "every descriptor has a copy of its own"
    torch.cuda.synchronize()
    prev = [p.detach().clone() for p in params]
    tables = None
    for rnd in range(rounds):
        with torch.no_grad():
            for p in params:
                p.copy_(_fine(p.shape, gen, gpu))                   # masters overwritten in place
        for _, _, packed in packs:
            _poison(packed)
        for *_, ent in copies:
            _poison(ent)
        ops.refresh_packed(params)                                  # ONE fp32 launch and ONE bf16 launch
        torch.cuda.synchronize()
        if tables is None:
            tables = (len(ops._pack_tables), len(ops._pack16_tables))
        else:
            assert tables == (len(ops._pack_tables), len(ops._pack16_tables)), "the second refresh builds no new table"
        refs, stale = [], []                                        # on the host, where pack_bf16_ref rounds
        for k, (pi, mode, packed) in enumerate(packs):
            tag = "round %d pack %d %s mode %d" % (rnd, k, tuple(params[pi].shape), mode)
            val, _ = W.pack_ref(params[pi], mode)
            assert torch.equal(val.float().double(), val)
            old = W.pack_ref(prev[pi], mode)[0].float()
            refs.append(val.float().cpu())
            stale.append(old.cpu())
            _same(chk, fam, tag + " vs reference", packed, val.float())
            _same(chk, fam, tag + " vs single kernel", packed, ops.pack_weight(params[pi].detach(), mode))
            _differs(chk, fam, tag, packed, old, "the pack of the previous masters")
            if _sentinels(packed):
                chk.bad.append("%s: %d sentinels left" % (tag, _sentinels(packed)))
        for pk, c, plan, d, ent in copies:
            pi, mode, packed = packs[pk]
            tag = "round %d copy %s of pack %d" % (rnd, W.b16_name(c), pk)
            ref = _b16_ref(c, plan, refs[pk])
            _same(chk, fam, tag + " vs reference", ent, ref)
            fresh = torch.empty_like(ent)
            _single_bf16(c, ops.pack_weight(params[pi].detach(), mode), fresh)
            _same(chk, fam, tag + " vs single kernels", ent, fresh)
            for m in W.b16_mutations(c, plan):
                _differs(chk, fam, tag, ent, _b16_ref(c, plan, refs[pk], mutate=m), m)
            _differs(chk, fam, tag, ent, _b16_ref(c, plan, stale[pk]), "the pack of the previous masters")
            if _sentinels(ent):
                chk.bad.append("%s: %d sentinels left" % (tag, _sentinels(ent)))
            # the cache hands out the refreshed tensor itself, untouched
            if ops.bf16_weight(packed, d, W.b16_w_offset(c)) is not ent:
                chk.bad.append("%s: bf16_weight does not return the refreshed tensor" % tag)
            _same(chk, fam, tag + " after bf16_weight", ent, ref)
        prev = [p.detach().clone() for p in params]
    _count(fam, records=len(packs) + len(copies))
    print("%s: %d parameters, %d packed tensors, %d bf16 copies, %d rounds" % (what, len(params), len(packs), len(copies), rounds))
    chk.done()
    return params, packs, copies


def test_network_refresh_equals_single_kernels_and_reference(gpu):
    specs = _f32_specs() + _b16_specs(W.CASES_B16)
    params, packs, copies = _run_network(gpu, "network", "network refresh", specs)
    assert sum(1 for s in specs if s["misaligned"]) >= 2 and sum(1 for s in specs if len(s["modes"]) == 2) >= 2
    assert len(packs) >= len(W.CASES_F32) and len(copies) >= len([c for c in W.CASES_B16 if W.b16_in_network(c)]) + 8


SMALL_F32 = dict(shape=(10, 5, 3, 3), misaligned=False, modes=[PACK_PLAIN], b16=[])      # one block of the fp32 kernel


def _smallest_b16():
    c = W.CASES_B16[3]
    assert (c.Cx, c.N, c.wmode) == (32, 8, 0)                                             # one strip x nine taps
    return _b16_specs([c])[0]


def test_item_lookup_on_a_table_of_one_item(gpu):
    _run_network(gpu, "lookup: one item", "item lookup", [_smallest_b16()])


def test_item_lookup_with_single_block_items_at_both_ends(gpu):
    specs = [SMALL_F32, _smallest_b16()] + _b16_specs(W.CASES_B16[0:2]) + [dict(SMALL_F32, modes=[PACK_UPFOLD]), _smallest_b16(),
                                                                         dict(SMALL_F32)]
    # the fp32 table begins and ends with one-block items; the bf16 table with the smallest item there is
    _run_network(gpu, "lookup: small items at both ends", "item lookup", specs)


def test_item_lookup_on_a_table_of_34_parameters(gpu):
    pool = [W.CASES_B16[i] for i in (3, 15, 4, 11)]               # small weights of the three kinds, both directions
    specs = [_b16_specs([pool[i % len(pool)]])[0] for i in range(34)]
    specs = [dict(SMALL_F32)] + specs[:17] + [dict(SMALL_F32, shape=(65, 8, 4, 4))] + specs[17:] + [dict(SMALL_F32)]
    params, packs, copies = _run_network(gpu, "lookup: 34 parameters", "item lookup", specs)
    assert len(packs) >= 33 and len(copies) >= 33, (len(packs), len(copies))


# ---- cache bookkeeping -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", (0, 9, 12), ids=[B16_IDS[i] for i in (0, 9, 12)])
def test_forward_through_refreshed_copies(gpu, index):
    from speech_to_image_translation_without_text_amd import ops
    c = W.CASES_B16[index]
    fam = "cache"
    assert c.wmode == 0 and W.b16_in_network(c)
    gen = LH.gen_key(gpu, "pack cache", index)
    shape, mode = W.b16_master(c)
    w1, w2 = _fine(shape, gen, gpu), _fine(shape, gen, gpu)
    x = torch.randn((3, c.H, c.H, c.Cx), generator=gen, device=gpu).bfloat16()
    chk = LH.Check("cache %s" % B16_IDS[index], {}, LEDGER)

    def forward(packed):
        y = ops.conv_any(c.kind, x, packed, c.N, out_dtype=torch.bfloat16)[0]
        torch.cuda.synchronize()
        assert y.dtype == torch.bfloat16 and len(packed._s2i_b16[1]) == 1, "the bf16 kernels took the layer"
        return y.clone()

    p = torch.nn.Parameter(w1.clone())
    packed = ops.packed_weight(p, mode)
    y1 = forward(packed)
    (ent,) = packed._s2i_b16[1].values()
    chk.equal("first use", y1, forward(ops.pack_weight(w1, mode)))
    with torch.no_grad():
        p.copy_(w2)
    _poison(packed)
    _poison(ent)
    ops.refresh_packed([p])
    y2 = forward(packed)
    (ent2,) = packed._s2i_b16[1].values()
    assert ent2 is ent, "the forward runs on the refreshed tensor"
    _same(chk, fam, "forward after refresh vs fresh packs", y2, forward(ops.pack_weight(w2, mode)))
    _differs(chk, fam, "forward after refresh", y2, y1, "the forward on the previous masters")
    # invalidate_derived: the copy is derived again, by the single-weight kernel, to the same bits
    kept = ent.clone()
    _poison(ent)
    ops.invalidate_derived([p])
    d = W.b16_desc(c, B=3)
    again = ops.bf16_weight(packed, d, 0)
    torch.cuda.synchronize()
    _same(chk, fam, "copy after invalidate_derived", again, kept)
    _same(chk, fam, "forward after invalidate_derived", forward(packed), y2)
    _count(fam, records=1)
    chk.done()


def test_tables_are_not_reused_for_other_shapes_at_the_same_addresses(gpu):
    """The allocator gives the addresses of a dead network to the next one.  Two parameters of different shapes at the same
    address, with packed copies at the same address: each refresh packs its own shape."""
    from speech_to_image_translation_without_text_amd import ops
    fam = "cache"
    gen = LH.gen_key(gpu, "pack table key")
    chk = LH.Check("table key", {}, LEDGER)
    store = torch.zeros(8 * 8 * 9, dtype=torch.float32, device=gpu)
    dest = torch.zeros(9 * 8 * 8, dtype=torch.float32, device=gpu)
    for shape in ((8, 8, 3, 3), (4, 16, 3, 3)):                   # both pack into 9 x 8 x 8 = 9 x 16 x 4 floats
        p = torch.nn.Parameter(store.view(shape))
        with torch.no_grad():
            p.copy_(_fine(shape, gen, gpu))
        packed = dest.view(9, W.roundup4(shape[1]), W.roundup4(shape[0]))
        p._s2i_packs = {PACK_PLAIN: (packed, p._version, p.data_ptr())}   # as ops.packed_weight files it
        _poison(packed)
        ops.refresh_packed([p])
        torch.cuda.synchronize()
        _same(chk, fam, "refresh of %s" % (shape,), packed, W.pack_ref(p, PACK_PLAIN)[0].float())
    _count(fam, records=1)
    chk.done()
