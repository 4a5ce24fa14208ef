"""Content oracles for every production scatter policy of both radix passes.

ops.net_scatter_slices / ops.local_scatter_slices run the sampled network pass
and the local pass exactly as the engine does (same kernels:: calls, same
order) into sentinel-filled outputs.  What they write is compared with plain
uint64 numpy references (helpers.expected_net / expected_local).

Network pass, asserted in every case (fill = final gcur - gstart):
  1. Demand   fill[g, d] equals the reference count of (claim group g, digit d)
              exactly, overflowed or not; the sum is n (kept tuples of a range pass).
  2. Content  per slice, the first min(fill, gend - gstart) values, read through
              the returned round map, are the reference multiset of (g, d); in an
              overflowed slice a sub-multiset of it, of exactly the slice capacity.
  3. Sentinel every other window element, guard included, still holds the sentinel
              (strays, writes past a bounded end, dropped range tuples).
  4. Layout   slices are disjoint, inside capacity_used <= capacity, capacities are
              multiples of 16 and, with an exact histogram, roundup16(count) before
              `shrink`; with rounds on, gstart[i] == i << lv and 2^lv >= every capacity.

Local pass, asserted in every case:
  1. Sizes    final-partition sizes equal the reference histogram of (lp,
              sub-partition); so does the pre-clamp claim demand of the sampled path.
  2. Content  per final partition the multiset of output rows equals the reference
              (lo / hi columns read as pairs at the same index).
  3. Sentinel everything outside [begin, end) of every partition, in every column,
              still holds the sentinel.
  4. Overflow the flag is set iff some demand exceeds its slot; after claimOverflow
              gcur <= gend everywhere.

A kernel change must keep all eight.
"""
import numpy as np
import pytest
import torch

import helpers as H

G = H.CLAIM_GROUPS
SIZES = [1, 4095, 8191, 8192, 8193, 12_289, 70_001]
TWO_SIZES = [12_289, 70_001]
GUARD = 64


# --------------------------------------------------------------- host tests
@pytest.mark.parametrize("bits", [7, 27, 32, 33, 63, 64])
def test_key_mix_matches_native(C, bits):
    g = torch.Generator().manual_seed(100 + bits)
    k = torch.randint(-(1 << 63), (1 << 63) - 1, (100_000,), generator=g, dtype=torch.int64)
    if bits < 64:
        k = torch.from_numpy((H.u64(k) >> np.uint64(64 - bits)).view(np.int64).copy())
    k[:3] = torch.tensor([0, 1, -1 if bits == 64 else (1 << bits) - 1])
    assert np.array_equal(H.key_mix(k, bits), H.u64(C.ops.key_mix(k, bits)))


@pytest.mark.parametrize("bits", [1, 7, 16, 17])
def test_key_mix_is_bijection(C, bits):
    k = np.arange(1 << bits, dtype=np.uint64)
    m = H.key_mix(k, bits)
    assert np.array_equal(np.sort(m), k)
    assert np.array_equal(m, H.u64(C.ops.key_mix(torch.arange(1 << bits), bits)))


@pytest.mark.parametrize("lp,lv,lns", [(0, 0, 0), (4, 4, 6), (4, 9, 8), (5, 13, 14), (1, 20, 3), (16, 30, 17)])
def test_round_slot_matches_native(C, lp, lv, lns):
    rng = np.random.default_rng(lp * 100 + lv)
    top = 1 << (lv + lns) if lv else 1 << 40
    L = rng.integers(0, top, 2000, dtype=np.int64)
    L[:2] = [0, top - 1]
    ref = H.round_slot(L, lp, lv, lns)
    assert [int(x) for x in ref] == [C.ops.round_slot(int(x), lp, lv, lns) for x in L]


@pytest.mark.parametrize("lp,lv,lns", [(2, 5, 3), (4, 4, 6), (1, 6, 0), (3, 9, 4)])
def test_round_slot_is_bijection(lp, lv, lns):
    slots = H.round_slot(np.arange(1 << (lv + lns), dtype=np.int64), lp, lv, lns)
    assert np.array_equal(np.sort(slots), np.arange(1 << (lv + lns), dtype=np.uint64))


# ------------------------------------------------------------------- inputs
def _randint(gen, hi, n):
    return torch.randint(0, min(hi, (1 << 63) - 1), (n,), generator=gen, dtype=torch.int64)


def make_keys(shape, n, key_bits, bits, mix_bits, seed):
    """Keys < 2^key_bits whose (mixed) digits follow `shape`."""
    gen = torch.Generator().manual_seed(seed)
    F = 1 << bits
    if shape == "uniform":
        return _randint(gen, 1 << key_bits, n)
    if shape == "dense":
        return torch.randperm(n, generator=gen)
    digits = {"one": [F // 3], "two": [0, F - 1]}[shape]
    if not mix_bits:
        pick = torch.tensor(digits)[torch.randint(0, len(digits), (n,), generator=gen)]
        return (_randint(gen, 1 << (key_bits - bits), n) << bits) | pick
    got, have = [], 0
    while have < n:  # a few rounds of rejection on whole arrays
        cand = _randint(gen, 1 << key_bits, 2 * n * F // len(digits) + 1024)
        d = (H.key_mix(cand, mix_bits) & np.uint64(F - 1)).astype(np.int64)
        sel = cand[torch.from_numpy(np.isin(d, digits))]
        got.append(sel)
        have += sel.numel()
    return torch.cat(got)[:n].contiguous()


def make_tuples(keys):
    return torch.stack([keys, torch.arange(keys.numel())], dim=1).contiguous()


# format, key_bits (None: 32 + bits), mixed, id
POLICIES = [
    ("frag", 27, False, "frag27"),
    ("frag", 27, True, "frag27-mix"),
    ("frag", None, False, "fragdig"),
    ("frag", None, True, "fragdig-mix"),
    ("key_only", 63, False, "keyonly63"),
    ("key_only", 63, True, "keyonly63-mix"),
    ("compressed", 30, False, "compressed30"),
    ("compressed", 64, False, "compressed64"),
    ("wide", 40, False, "wide"),
]
POL_IDS = [p[3] for p in POLICIES]


def policy_args(pol, bits):
    fmt, kb, mixed, _ = pol
    key_bits = 32 + bits if kb is None else kb
    gen_bits = 30 if fmt == "compressed" else key_bits  # compressed64: the digit array, same keys
    return fmt, key_bits, gen_bits, (key_bits if mixed else 0)


# ------------------------------------------------------------ network oracle
def sentinel_rows(C, width_bits, cols):
    s = np.uint64(C.ops.scatter_sentinel() & ((1 << 64) - 1)) & np.uint64((1 << width_bits) - 1)
    return np.full((1, cols), s, dtype=np.uint64)


def run_net(C, t, fmt, bits, **kw):
    return C.ops.net_scatter_slices(t.cuda(), bits, fmt, guard=GUARD, **kw)


def check_net(C, t, res, fmt, bits, *, key_shift=32, mix_bits=0, d_lo=0, rng=0, shrink=0, exact=True,
              expect_overflow=None, expect_rounds=None, mutate=None):
    Fp = rng or (1 << bits)
    m = G * Fp
    gstart, gcur, gend = (res[k].numpy().astype(np.int64) for k in ("gstart", "gcur", "gend"))
    assert gstart.shape == (G, Fp)
    fill, cap = (gcur - gstart).ravel(), (gend - gstart).ravel()
    tpb, ptile = res["tiles_per_block"], C.ops.partition_tile()
    if mutate == "digit_shift":  # a deliberately wrong reference must fail
        group, digit, _ = H.expected_net(t, fmt, bits, tpb, ptile, key_shift, mix_bits, d_lo, rng)
        vals = H.expected_net(t, fmt, bits + 1, tpb, ptile, key_shift, mix_bits, d_lo, rng)[2]  # value >> (bits + 1)
    elif mutate == "group_boundary":
        group, digit, vals = H.expected_net(t, fmt, bits, tpb, ptile, key_shift, mix_bits, d_lo, rng)
        group = H.claim_group(np.arange(t.shape[0]) + 1, tpb, ptile)[:group.size]
    else:
        group, digit, vals = H.expected_net(t, fmt, bits, tpb, ptile, key_shift, mix_bits, d_lo, rng)
    ref_sid = group * Fp + digit
    count = np.bincount(ref_sid, minlength=m)
    # 1. demand
    assert np.array_equal(fill, count), "claim demand differs from the reference histogram"
    assert int(fill.sum()) == ref_sid.size
    # 4. layout
    lp, lv, lns = res["round_map"]
    capacity, used = res["capacity"], res["capacity_used"]
    assert used <= capacity
    assert (cap >= 0).all() and (cap % 16 == 0).all()
    if exact:
        full = (count + 15) // 16 * 16
        assert np.array_equal(cap, np.where(full >= shrink + 16, full - shrink, full))
    if expect_rounds is not None:
        assert (lv > 0) == expect_rounds, (lp, lv, lns)
    if lv:
        assert np.array_equal(gstart.ravel(), np.arange(m, dtype=np.int64) << lv)
        assert (1 << lv) >= int(cap.max()) + shrink and (1 << lns) == m and lp <= lv
        assert C.ops.round_slots(int(cap.max()), lp, lns) <= used
    else:
        order = np.lexsort((gend.ravel(), gstart.ravel()))  # empty slices before the one they start with
        s, e = gstart.ravel()[order], gend.ravel()[order]
        assert (e[:-1] <= s[1:]).all() and int(e.max()) <= used
    # 2. content
    stored = np.minimum(fill, cap)
    over = fill > cap
    if expect_overflow is not None:
        assert bool(over.any()) == expect_overflow
    window = res["window"].cpu()
    assert window.shape[0] == capacity + GUARD
    sid, got, slots = H.slice_contents(window, gstart, stored, (lp, lv, lns))
    assert np.unique(slots).size == slots.size and (slots.size == 0 or int(slots.max()) < capacity)
    if not over.any():
        a, b = H.canonical(sid, got), H.canonical(ref_sid, vals)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "slice contents differ"
    else:
        assert H.multiset_excess(sid, got, ref_sid, vals) == 0, "a slice holds values outside its reference multiset"
    # 3. sentinel
    rows = H.rows_of(window)
    untouched = np.ones(rows.shape[0], dtype=bool)
    untouched[slots] = False
    sent = sentinel_rows(C, 32 if fmt == "frag" else 64, rows.shape[1])
    assert (rows[untouched] == sent).all(), "a store landed outside the filled slice ranges"


def net_case(C, pol, n, bits, *, shape="uniform", seed=1, mutate=None, expect_overflow=False, **kw):
    fmt, key_bits, gen_bits, mix_bits = policy_args(pol, bits)
    t = make_tuples(make_keys(shape, n, gen_bits, bits, mix_bits, seed))
    res = run_net(C, t, fmt, bits, key_bits=key_bits, mix_bits=mix_bits, **kw)
    check_net(C, t, res, fmt, bits, mix_bits=mix_bits, shrink=kw.get("shrink", 0),
              exact=kw.get("sample_stride", 1) == 1, expect_overflow=expect_overflow, mutate=mutate,
              d_lo=kw.get("d_lo", 0), rng=kw.get("range", 0))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pol", POLICIES, ids=POL_IDS)
def test_net_policy_sizes(C, cuda, pol, n):
    net_case(C, pol, n, 5, narrow=1, seed=n)


@pytest.mark.gpu
@pytest.mark.parametrize("pol", POLICIES, ids=POL_IDS)
def test_net_policy_few_blocks(C, cuda, pol):
    res = net_case(C, pol, 262_161, 5, narrow=1, max_blocks=7, seed=7)
    assert res["blocks"] == 7 and res["tiles_per_block"] == 10


@pytest.mark.gpu
@pytest.mark.parametrize("n", TWO_SIZES)
@pytest.mark.parametrize("bits,narrow", [(1, 1), (10, 0), (11, 1), (11, 0)])
@pytest.mark.parametrize("pol", POLICIES, ids=POL_IDS)
def test_net_policy_bits(C, cuda, pol, bits, narrow, n):
    if pol[0] == "wide" and bits == 11:
        # 8192 staged 16-byte tuples plus 2048-entry digit arrays exceed the 160 KiB of
        # LDS: the launcher refuses (plans pick at most 10 bits per pass on their own).
        with pytest.raises(RuntimeError, match="LDS .* too large"):
            net_case(C, pol, n, bits, narrow=narrow, seed=bits)
        return
    net_case(C, pol, n, bits, narrow=narrow, seed=bits)


@pytest.mark.gpu
@pytest.mark.parametrize("n", TWO_SIZES)
@pytest.mark.parametrize("pol", POLICIES, ids=POL_IDS)
def test_net_policy_wide_cursors(C, cuda, pol, n):
    net_case(C, pol, n, 5, narrow=0, seed=3)


@pytest.mark.gpu
@pytest.mark.parametrize("n", TWO_SIZES)
@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("pol", POLICIES[:-1], ids=POL_IDS[:-1])  # the wide scatter keeps linear slices
def test_net_policy_rounds(C, cuda, pol, narrow, n):
    res = net_case(C, pol, n, 5, narrow=narrow, round_lp=4, seed=4)
    assert res["round_map"][1] > 0, "uniform keys must get round-interleaved slices"


@pytest.mark.gpu
@pytest.mark.parametrize("pol,shape,round_lp", [
    pytest.param(p, s, r, id=f"{p[3]}-{s}-lp{r}") for p in POLICIES for s in ("one", "two", "dense")
    for r in ((0,) if p[0] == "wide" else (0, 4))])  # the wide scatter keeps linear slices
def test_net_policy_key_shapes(C, cuda, pol, shape, round_lp):
    net_case(C, pol, 70_001, 5, shape=shape, narrow=1 if shape != "two" else 0, round_lp=round_lp, seed=5)


@pytest.mark.gpu
@pytest.mark.parametrize("pol,shape,bits", [
    pytest.param(p, s, b, id=f"{p[3]}-{s}-{b}") for p in POLICIES if not p[2] for s in ("one", "two") for b in (1, 11)
    if not (p[0] == "wide" and b == 11)])  # digits 0 and F - 1 at both ends of the digit arrays
def test_net_policy_key_shapes_edge_bits(C, cuda, pol, shape, bits):
    net_case(C, pol, 70_001, bits, shape=shape, narrow=1, seed=6)


@pytest.mark.gpu
@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("pol,n,bits", [
    pytest.param(p, n, b, id=f"{p[3]}-{n}-{b}") for p in POLICIES for n, b in ((12_289, 5), (70_001, 5), (70_001, 11))
    if not (p[0] == "wide" and b == 11)])
def test_net_policy_unbounded(C, cuda, pol, n, bits, narrow):
    # No slice ends (the exact multi-rank pass): exact slices hold every tuple.
    rounds = n == 70_001 and bits == 5 and pol[0] != "wide"
    net_case(C, pol, n, bits, narrow=narrow, unbounded=True, round_lp=4 if rounds else 0, seed=8)


@pytest.mark.gpu
@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("d_lo,rng", [(0, 1), (256, 256), (1023, 1), (1, 1023)])
@pytest.mark.parametrize("pol", [POLICIES[0], POLICIES[2]], ids=["frag27", "fragdig"])
@pytest.mark.parametrize("n", TWO_SIZES)
def test_net_frag_range(C, cuda, n, pol, d_lo, rng, narrow):
    net_case(C, pol, n, 10, narrow=narrow, d_lo=d_lo, range=rng, seed=rng)


@pytest.mark.gpu
@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("pol", [POLICIES[1], POLICIES[3]], ids=["frag27-mix", "fragdig-mix"])
def test_net_frag_range_mixed(C, cuda, pol, narrow):
    net_case(C, pol, 70_001, 10, narrow=narrow, d_lo=256, range=256, seed=9)


@pytest.mark.gpu
@pytest.mark.parametrize("pol,round_lp", [(POLICIES[0], 0), (POLICIES[0], 4), (POLICIES[4], 0), (POLICIES[4], 4)],
                         ids=["frag27", "frag27-rounds", "keyonly63", "keyonly63-rounds"])
def test_net_sampled(C, cuda, pol, round_lp):
    # 2^20 uniform keys, 32 digits: ~4096 tuples per (group, digit), ~1024 of them
    # sampled; the margin (6 sigma + 2 % + 256 > 1000) is far above the cell's
    # standard deviation (~64), and tile sampling with a fixed seed is deterministic.
    res = net_case(C, pol, 1 << 20, 5, narrow=1, sample_stride=4, round_lp=round_lp, seed=20, expect_overflow=False)
    assert res["sample_stride"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("pol", [POLICIES[0], POLICIES[3]], ids=["frag27", "fragdig-mix"])
def test_net_sampled_range(C, cuda, pol):
    # Sampled totals laid out for a digit range (the spill plan's partition-group pass);
    # whether a slice overflows is left to the oracle, which holds either way.
    res = net_case(C, pol, 1 << 20, 10, narrow=1, sample_stride=4, d_lo=512, range=384, seed=21, expect_overflow=None)
    assert res["sample_stride"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("pol,kw", [
    (POLICIES[0], dict()), (POLICIES[1], dict(round_lp=4)), (POLICIES[4], dict()), (POLICIES[5], dict(narrow=0)),
    (POLICIES[0], dict(d_lo=256, range=256)), (POLICIES[2], dict(d_lo=1, range=1023)),
    (POLICIES[6], dict()), (POLICIES[8], dict()),
], ids=["frag27", "frag27-mix-rounds", "keyonly63", "keyonly63-mix-wide", "range256", "range1023-dig", "compressed30",
        "wide"])
def test_net_forced_overflow(C, cuda, pol, kw):
    # shrink moves gend, never the allocation: slices of >= 32 slots lose their last line.
    # 5 bits: ~270 tuples per (group, digit); range passes (10 bits): 7 workgroups, ~36 per cell.
    kw = dict(dict(narrow=1), **kw)
    if "range" in kw:
        net_case(C, pol, 262_161, 10, max_blocks=7, shrink=16, seed=16, expect_overflow=True, **kw)
    else:
        net_case(C, pol, 70_001, 5, shrink=16, seed=16, expect_overflow=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("mutate", ["digit_shift", "group_boundary"])
def test_net_oracle_rejects_wrong_reference(C, cuda, mutate):
    with pytest.raises(AssertionError):
        net_case(C, POLICIES[0], 70_001, 5, narrow=1, seed=11, mutate=mutate)


# -------------------------------------------------------------- local oracle
def run_local(C, window, runs, owned, shift, bits, mode, **kw):
    return C.ops.local_scatter_slices(window, runs, owned, shift, bits, mode, guard=GUARD, **kw)


def check_local(C, res, part, rows, P, mode, *, sampled, expect_overflow=None, mutate=None):
    begin = res["part_begin"].numpy().astype(np.int64)[:P]
    end, slot_end, demand = (res[k].numpy().astype(np.int64) for k in ("part_end", "slot_end", "demand"))
    if mutate == "partition_shift":
        part = (part + 1) % max(P, 1)
    hist = np.bincount(part, minlength=P)
    slot = slot_end - begin
    # 1. sizes
    assert np.array_equal(demand, hist), "claim demand differs from the reference histogram"
    assert np.array_equal(end - begin, np.minimum(hist, slot))
    # 4. overflow
    assert res["overflow"] == bool((hist > slot).any())
    if expect_overflow is not None:
        assert res["overflow"] == expect_overflow
    assert (end <= slot_end).all() and (begin <= end).all()
    if not sampled:
        assert np.array_equal(slot_end, res["part_begin"].numpy()[1:]) and int(begin[0] if P else 0) == 0
    order = np.lexsort((slot_end, begin))
    assert (slot_end[order][:-1] <= begin[order][1:]).all() and (P == 0 or int(slot_end.max()) <= res["capacity"])
    # 2. content
    cols = [res["out"].cpu()] + ([res["hi"].cpu()] if mode == "split" else [])
    assert all(c.shape[0] == res["capacity"] + GUARD for c in cols)
    pid, slots = H.slice_slots(begin, end - begin)
    got = np.concatenate([H.rows_of(c)[slots] for c in cols], axis=1)
    assert np.unique(slots).size == slots.size
    if not res["overflow"]:
        a, b = H.canonical(pid, got), H.canonical(part, rows)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "partition contents differ"
    else:
        assert H.multiset_excess(pid, got, part, rows) == 0
    # 3. sentinel
    untouched = np.ones(cols[0].shape[0], dtype=bool)
    untouched[slots] = False
    widths = {"compressed": [64], "wide": [64], "split": [32, 16], "frag": [16]}[mode]
    for c, w in zip(cols, widths):
        r = H.rows_of(c)
        assert (r[untouched] == sentinel_rows(C, w, r.shape[1])).all(), "a store landed outside every partition"


# One partition of several items (and, exact path, several claim streams),
# empty partitions, a single tuple, a whole tile, a tail tile.
LOCAL_SIZES = [70_001, 0, 1, 0, 5000, 8192, 0, 12_289]


def local_words(mode, seed):
    gen = torch.Generator().manual_seed(seed)
    n = sum(LOCAL_SIZES)
    w = torch.randint(0, (1 << 63) - 1, (n,), generator=gen, dtype=torch.int64)
    window = make_tuples(w) if mode == "wide" else w
    pb = np.concatenate([[0], np.cumsum(LOCAL_SIZES)])
    runs = torch.tensor([[lp, int(pb[lp]), LOCAL_SIZES[lp]] for lp in range(len(LOCAL_SIZES))])
    lp_of = np.repeat(np.arange(len(LOCAL_SIZES)), LOCAL_SIZES)
    return window, runs, lp_of


LOCAL_VARIANTS = [dict(narrow=1), dict(narrow=0), dict(sample_stride=4)]
LOCAL_VARIANT_IDS = ["exact32", "exact64", "sampled"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", LOCAL_VARIANTS, ids=LOCAL_VARIANT_IDS)
@pytest.mark.parametrize("shift", [0, 27, 32])
@pytest.mark.parametrize("mode", ["compressed", "wide"])
def test_local_plain(C, cuda, mode, shift, variant):
    window, runs, lp_of = local_words(mode, 40 + shift)
    owned, bits = len(LOCAL_SIZES), 9
    res = run_local(C, window.cuda(), runs, owned, shift, bits, mode, **variant)
    assert res["items"] == 2 + 4  # 70_001 = 65536 + 4465
    part, rows = H.expected_local(H.rows_of(window), lp_of, shift, bits, mode)
    check_local(C, res, part, rows, owned << bits, mode, sampled="sample_stride" in variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", LOCAL_VARIANTS, ids=LOCAL_VARIANT_IDS)
@pytest.mark.parametrize("bits", [0, 4, 11])
@pytest.mark.parametrize("mode", ["compressed", "wide"])
def test_local_plain_bits(C, cuda, mode, bits, variant):
    window, runs, lp_of = local_words(mode, 50 + bits)
    owned = len(LOCAL_SIZES)
    if mode == "wide" and bits == 11:  # as in the network pass: no LDS for 16-byte tuples x 2048 digits
        with pytest.raises(RuntimeError, match="LDS .* too large"):
            run_local(C, window.cuda(), runs, owned, 27, bits, mode, **variant)
        return
    res = run_local(C, window.cuda(), runs, owned, 27, bits, mode, **variant)
    part, rows = H.expected_local(H.rows_of(window), lp_of, 27, bits, mode)
    check_local(C, res, part, rows, owned << bits, mode, sampled="sample_stride" in variant)


# Local passes fed from a network window, as in a join: the filled [gstart, gcur)
# run of every (group, digit) slice, digit-major, read through its round map.
NET_BITS = 3


def skewed_keys(n, key_bits, seed):
    """Digit 0 holds 70 % (slices longer than LOCAL_ITEM_MAX), digits 1 and 5 are empty, digit 2 holds one tuple."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=gen)
    rest = torch.tensor([3, 4, 6, 7])[torch.randint(0, 4, (n,), generator=gen)]
    d = torch.where(u < 0.7, torch.zeros(n, dtype=torch.int64), rest)
    d[n // 2] = 2
    return (_randint(gen, 1 << (key_bits - NET_BITS), n) << NET_BITS) | d


def net_feed(C, fmt, key_bits, rounds, seed):
    n = 200_001
    if rounds:
        keys = make_keys("uniform", n, key_bits, NET_BITS, 0, seed)
    else:
        keys = skewed_keys(n, key_bits, seed)
    t = make_tuples(keys)
    res = run_net(C, t, fmt, NET_BITS, key_bits=key_bits, narrow=1, max_blocks=2, round_lp=4 if rounds else 0)
    check_net(C, t, res, fmt, NET_BITS, expect_overflow=False, expect_rounds=rounds)
    F = 1 << NET_BITS
    gstart = res["gstart"].numpy()
    fill = res["gcur"].numpy() - gstart
    runs = torch.tensor([[d, int(gstart[g, d]), int(fill[g, d])] for d in range(F) for g in range(G)])
    sid, words, _ = H.slice_contents(res["window"].cpu(), gstart, fill, res["round_map"])
    if not rounds:
        assert int(fill.max()) > C.ops.local_item_max() and (fill.sum(axis=0) == 0).any() and (fill.sum(axis=0) == 1).any()
    return res, runs, words, sid % F


FEEDS = [
    # mode, network format, key bits, shift, (lo_shift, frag_shift) from the local bits
    ("split", "compressed", 30, 32, lambda b: (0, 32)),
    ("split", "key_only", 63, 0, lambda b: (b, b + 32)),
    ("frag", "frag", 35, 0, lambda b: (0, b)),
]
FEED_IDS = ["split-compressed", "split-keyonly", "frag"]


def local_fed(C, feed, rounds, bits, variant, seed, **check):
    mode, fmt, key_bits, shift, shifts = feed
    lo_shift, frag_shift = shifts(bits)
    net, runs, words, lp_of = net_feed(C, fmt, key_bits, rounds, seed)
    F = 1 << NET_BITS
    res = run_local(C, net["window"], runs, F, shift, bits, mode, round_map=net["round_map"], lo_shift=lo_shift,
                    frag_shift=frag_shift, **variant)
    part, rows = H.expected_local(words, lp_of, shift, bits, mode, frag_shift, lo_shift)
    check_local(C, res, part, rows, F << bits, mode, sampled="sample_stride" in variant, **check)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("variant", LOCAL_VARIANTS, ids=LOCAL_VARIANT_IDS)
@pytest.mark.parametrize("rounds", [False, True], ids=["linear", "rounds"])
@pytest.mark.parametrize("feed", FEEDS, ids=FEED_IDS)
def test_local_fed(C, cuda, feed, rounds, variant):
    local_fed(C, feed, rounds, 9, variant, 60)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", LOCAL_VARIANTS[1:], ids=LOCAL_VARIANT_IDS[1:])
@pytest.mark.parametrize("bits", [0, 4, 11])
@pytest.mark.parametrize("feed", FEEDS, ids=FEED_IDS)
def test_local_fed_bits(C, cuda, feed, bits, variant):
    local_fed(C, feed, bits == 4, bits, variant, 61)


@pytest.mark.gpu
@pytest.mark.parametrize("feed", FEEDS, ids=FEED_IDS)
def test_local_sampled_no_overflow(C, cuda, feed):
    # Uniform keys, 8 network partitions of ~25000 tuples into 16 sub-partitions:
    # ~1560 tuples per final partition (>= 256 asked), ~512 of them sampled (the
    # first tile of each of the two ~12500-tuple runs); the slot margin (8 sigma +
    # 2 % + 64 ~ 650) is ~9 standard deviations (~70) of the estimate.
    local_fed(C, feed, True, 4, dict(sample_stride=4), 62, expect_overflow=False)


@pytest.mark.gpu
@pytest.mark.parametrize("feed", FEEDS, ids=FEED_IDS)
def test_local_forced_overflow(C, cuda, feed):
    # Every slot loses 1024 of its ~2200 slots and ~1560 tuples claim it.
    local_fed(C, feed, True, 4, dict(sample_stride=4, shrink=1024), 63, expect_overflow=True)


@pytest.mark.gpu
def test_local_oracle_rejects_wrong_reference(C, cuda):
    with pytest.raises(AssertionError):
        local_fed(C, FEEDS[0], False, 4, dict(narrow=1), 64, mutate="partition_shift")
