"""Packed fragment windows of the headline plan (JoinConfig.packed_fragments).

A window element is one u64 word: bits 0-19, 20-39 and 40-59 hold fragments 0,
1 and 2, bits 60-63 the number of valid fragments (0-3, filled from fragment 0
upwards).  A chunk is 8 consecutive words on a 64-byte boundary; the scatter
(netScatterFragPackedKernel) writes whole chunks only, carrying every digit's
partial tail in LDS across its tiles, so only the last chunk a workgroup writes
for a digit may be partial.  Slice tables, round-map positions and capacities
count words.

Scatter, asserted in every case (numpy references below; the sentinel, the
claim groups and the round map come from tests/helpers.py):
  1. Demand   per (group, digit): gcur - gstart is 8 words for every chunk the
              workgroups of the group need, sum over blocks of ceil(count / 24),
              overflowed or not, and the decoded fragment count equals the
              reference count when nothing overflowed.
  2. Content  the decoded multiset per slice equals the reference multiset (an
              overflowed slice holds a sub-multiset); every count nibble is <= 3,
              a word's fields above its count are zero, and a slice has at most
              8 x (workgroups of the group) words with count < 3.
  3. Sentinel every word outside [gstart, min(gcur, gend)) still holds the
              sentinel, guard included.
  4. Layout   slices are disjoint, inside the capacity, start and end on multiples
              of 8 words; with an exact histogram a capacity is roundup16(ceil(count
              / 3)) + 8 x ceil(blocks / 8) before `shrink`.
"""
import numpy as np
import pytest
import torch

import helpers as H

G = H.CLAIM_GROUPS
GUARD = 64
FB, FMASK = 20, (1 << 20) - 1
SIZES = [1, 23, 24, 25, 8191, 8192, 8193, 24_577, 70_001]


# ------------------------------------------------------------ numpy format
def np_pack(frags, counts):
    """[m, 3] fragments (< 2^20) and [m] counts (0-3) -> [m] uint64 words."""
    f = np.asarray(frags, dtype=np.uint64)
    c = np.asarray(counts, dtype=np.uint64)
    return f[:, 0] | (f[:, 1] << np.uint64(FB)) | (f[:, 2] << np.uint64(2 * FB)) | (c << np.uint64(60))


def np_unpack(words):
    w = np.asarray(words, dtype=np.uint64)
    f = np.stack([(w >> np.uint64(FB * e)) & np.uint64(FMASK) for e in range(3)], axis=1)
    return f, (w >> np.uint64(60))


def decode(words):
    """(index of the word, fragment) of every valid fragment, and the counts."""
    f, c = np_unpack(words)
    valid = np.arange(3)[None, :] < c[:, None].astype(np.int64)
    idx = np.repeat(np.arange(w_len(words)), 3).reshape(-1, 3)
    return idx[valid], f[valid], c.astype(np.int64), f, valid


def w_len(words):
    return int(np.asarray(words).shape[0])


def pack_runs(runs):
    """Packed words of one slice written by several 'workgroups': every run of
    fragments is packed 3 per word and padded with count-0 words to whole chunks."""
    out = []
    for r in runs:
        r = np.asarray(r, dtype=np.uint64)
        if r.size == 0:
            continue
        words = (r.size + 2) // 3
        padded = (words + 7) // 8 * 8
        f = np.zeros((padded, 3), dtype=np.uint64)
        f.ravel()[:r.size] = r
        c = np.clip(r.size - 3 * np.arange(padded), 0, 3)
        out.append(np_pack(f, c))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


# ------------------------------------------------------------- format, CPU
def test_numpy_pack_unpack_bijection():
    rng = np.random.default_rng(1)
    f = rng.integers(0, 1 << FB, (50_000, 3), dtype=np.int64)
    c = rng.integers(0, 4, 50_000, dtype=np.int64)
    f[:4] = [[0, 0, 0], [FMASK, FMASK, FMASK], [FMASK, 0, FMASK], [1, 2, 3]]
    w = np_pack(f, c)
    f2, c2 = np_unpack(w)
    assert np.array_equal(f2, f.astype(np.uint64)) and np.array_equal(c2, c.astype(np.uint64))
    assert np.array_equal(np_pack(f2, c2), w)
    assert int(w.max() >> np.uint64(60)) <= 3


def test_native_pack_unpack_agree(C):
    rng = np.random.default_rng(2)
    f = rng.integers(0, 1 << FB, (20_000, 3), dtype=np.int64)
    c = rng.integers(0, 4, 20_000, dtype=np.int64)
    f[:2] = [[FMASK, FMASK, FMASK], [0, 0, 0]]
    c[:2] = [3, 0]
    w = C.ops.pack_fragments(torch.from_numpy(f), torch.from_numpy(c))
    assert np.array_equal(H.u64(w), np_pack(f, c))
    f2, c2 = C.ops.unpack_fragments(w)
    assert np.array_equal(f2.numpy(), f) and np.array_equal(c2.numpy(), c)
    with pytest.raises(RuntimeError):
        C.ops.pack_fragments(torch.tensor([[1 << FB, 0, 0]]), torch.tensor([1]))
    with pytest.raises(RuntimeError):
        C.ops.pack_fragments(torch.tensor([[1, 0, 0]]), torch.tensor([4]))


# ----------------------------------------------------------- scatter, GPU
def make_keys(shape, n, bits, seed, mix_bits=0):
    """Keys whose fragment above `bits` radix bits fits 20 bits."""
    gen = torch.Generator().manual_seed(seed)
    F = 1 << bits
    if shape == "uniform":
        return torch.randint(0, 1 << (bits + FB), (n,), generator=gen, dtype=torch.int64)
    if shape == "dense":
        return torch.randperm(n, generator=gen)
    assert shape == "one" and not mix_bits
    return (torch.randint(0, 1 << FB, (n,), generator=gen, dtype=torch.int64) << bits) | (F // 3)


def tuples_of(keys):
    return torch.stack([keys, torch.arange(keys.numel())], dim=1).contiguous()


def check_packed(C, t, res, bits, *, mix_bits=0, shrink=0, exact=True, expect_overflow=False, saturate=False):
    F = 1 << bits
    m = G * F
    gstart, gcur, gend = (res[k].numpy().astype(np.int64) for k in ("gstart", "gcur", "gend"))
    assert gstart.shape == (G, F)
    claimed, cap = (gcur - gstart).ravel(), (gend - gstart).ravel()
    tpb, ptile, blocks = res["tiles_per_block"], C.ops.partition_tile(), res["blocks"]
    group, digit, vals = H.expected_net(t, "frag", bits, tpb, ptile, 32, mix_bits)
    vals = vals[:, 0]
    if saturate:  # a fragment above 20 bits is stored saturated, never truncated
        vals = np.where(vals > np.uint64(FMASK), np.uint64(FMASK), vals)
    ref_sid = group * F + digit
    count = np.bincount(ref_sid, minlength=m)
    # 1. demand: one chunk per started 24 fragments of every (block, digit)
    block = np.arange(t.shape[0], dtype=np.int64) // (tpb * ptile)
    per_block = np.bincount(block * F + digit, minlength=blocks * F).reshape(blocks, F)
    chunks = np.zeros((G, F), dtype=np.int64)
    for b in range(blocks):
        chunks[b % G] += (per_block[b] + 23) // 24
    assert (claimed % 8 == 0).all()
    assert np.array_equal(claimed, 8 * chunks.ravel()), "claimed words differ from the chunks the reference needs"
    # 4. layout
    lp, lv, lns = res["round_map"]
    capacity, used = res["capacity"], res["capacity_used"]
    assert used <= capacity
    assert (gstart % 8 == 0).all() and (cap >= 0).all() and (cap % 8 == 0).all()
    tail = 8 * ((blocks + G - 1) // G)
    if exact:
        full = ((count + 2) // 3 + 15) // 16 * 16 + tail
        assert np.array_equal(cap, np.where(full >= shrink + 16, full - shrink, full))
    if lv:
        assert np.array_equal(gstart.ravel(), np.arange(m, dtype=np.int64) << lv)
        assert (1 << lv) >= int(cap.max()) + shrink and (1 << lns) == m and 3 <= lp <= lv
    else:
        order = np.lexsort((gend.ravel(), gstart.ravel()))
        s, e = gstart.ravel()[order], gend.ravel()[order]
        assert (e[:-1] <= s[1:]).all() and int(e.max()) <= used
    # 2. content
    over = claimed > cap
    assert bool(over.any()) == expect_overflow
    stored = np.minimum(claimed, cap)
    window = res["window"].cpu()
    assert window.shape[0] == capacity + GUARD
    sid_w, words, slots = H.slice_contents(window, gstart, stored, (lp, lv, lns))
    words = words[:, 0]
    assert np.unique(slots).size == slots.size and (slots.size == 0 or int(slots.max()) < capacity)
    widx, frags, cnts, fields, valid = decode(words)
    assert (cnts <= 3).all(), "a count nibble above 3 (a sentinel read as data?)"
    assert (fields[~valid] == 0).all(), "a word carries bits above its count"
    got_sid = sid_w[widx]
    if not over.any():
        assert np.array_equal(np.bincount(got_sid, minlength=m), count), "decoded fragments per slice"
        a, b = H.canonical(got_sid, frags[:, None]), H.canonical(ref_sid, vals[:, None])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "slice contents differ"
    else:
        assert H.multiset_excess(got_sid, frags[:, None], ref_sid, vals[:, None]) == 0
    partial = np.bincount(sid_w[cnts < 3], minlength=m).reshape(G, F)
    wgs = np.array([len(range(g, blocks, G)) for g in range(G)])
    assert (partial <= 8 * wgs[:, None]).all(), "partial words beyond one chunk per workgroup"
    # 3. sentinel
    rows = H.rows_of(window)
    untouched = np.ones(rows.shape[0], dtype=bool)
    untouched[slots] = False
    sent = np.uint64(C.ops.scatter_sentinel() & ((1 << 64) - 1))
    assert (rows[untouched] == sent).all(), "a store landed outside the filled slice ranges"


def packed_case(C, n, bits, *, shape="uniform", seed=1, mix_bits=0, expect_overflow=False, **kw):
    t = tuples_of(make_keys(shape, n, bits, seed, mix_bits))
    res = C.ops.net_scatter_slices(t.cuda(), bits, "frag_packed", guard=GUARD, key_bits=bits + FB, mix_bits=mix_bits,
                                   **kw)
    assert res["wide_flag"] == 0
    check_packed(C, t, res, bits, mix_bits=mix_bits, shrink=kw.get("shrink", 0),
                 exact=kw.get("sample_stride", 1) == 1, expect_overflow=expect_overflow)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("max_blocks", [3, 2048])  # several tiles per workgroup (the carry) / several workgroups per group
@pytest.mark.parametrize("round_lp", [0, 9])
@pytest.mark.parametrize("shape", ["uniform", "dense", "one"])
@pytest.mark.parametrize("bits", [3, 10])
@pytest.mark.parametrize("n", SIZES)
def test_packed_scatter(C, cuda, n, bits, shape, round_lp, max_blocks):
    packed_case(C, n, bits, shape=shape, round_lp=round_lp, max_blocks=max_blocks, seed=n + bits)


@pytest.mark.gpu
@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("shape", ["uniform", "one"])
def test_packed_scatter_rounds_and_cursors(C, cuda, shape, narrow):
    """Small pieces, so that uniform keys really get round-interleaved slices; both cursor widths."""
    res = packed_case(C, 70_001, 3, shape=shape, round_lp=4, max_blocks=3, narrow=narrow, seed=11)
    if shape == "uniform":
        assert res["round_map"][1] > 0
    assert res["narrow"] == bool(narrow)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [3, 10])
def test_packed_scatter_mixed_keys(C, cuda, bits):
    packed_case(C, 70_001, bits, mix_bits=bits + FB, max_blocks=3, seed=12)


@pytest.mark.gpu
def test_packed_scatter_sampled(C, cuda):
    res = packed_case(C, 1 << 20, 5, sample_stride=4, round_lp=9, seed=13)
    assert res["sample_stride"] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("round_lp", [0, 4])
def test_packed_scatter_bounded_overflow(C, cuda, round_lp):
    """Slices 1024 words too small: nothing is written at or past gend, the demand is exact, the overflow shows."""
    packed_case(C, 1 << 18, 3, shrink=1024, max_blocks=16, round_lp=round_lp, seed=14, expect_overflow=True)


@pytest.mark.gpu
def test_packed_scatter_wide_fragment(C, cuda):
    """A key whose fragment needs 21 bits raises the flag and is stored saturated: the truncated value
    (fragment & 0xFFFFF = 5 here, a fragment no other key of the digit has) is not written."""
    bits, n = 10, 30_000
    keys = make_keys("uniform", n, bits, 15)
    keys[keys >> bits == 5] += 1 << bits  # no honest fragment 5
    keys[12_345] = (((1 << FB) | 5) << bits) | 7
    t = tuples_of(keys)
    res = C.ops.net_scatter_slices(t.cuda(), bits, "frag_packed", guard=GUARD, key_bits=bits + FB + 1, max_blocks=3)
    assert res["wide_flag"] >= 1
    check_packed(C, t, res, bits, saturate=True)
    gstart, gcur = res["gstart"].numpy(), res["gcur"].numpy()
    _, words, _ = H.slice_contents(res["window"].cpu(), gstart, (gcur - gstart).ravel(), res["round_map"])
    _, frags, _, _, _ = decode(words[:, 0])
    assert not (frags == 5).any() and (frags == FMASK).any()


# -------------------------------------------------------- join kernel, GPU
class PackedSide:
    """Packed windows laid out by hand: slice (g, d) holds runs[g][d], a list of fragment arrays (one per
    'workgroup', each ending in its own partial chunk), at a chunk-aligned start behind a poisoned gap."""

    def __init__(self, runs, F, poison_frag, gap=8):
        self.F = F
        self.start = np.zeros((G, F), dtype=np.int64)
        self.cur = np.zeros((G, F), dtype=np.int64)
        parts, at = [], 0
        poison = np_pack(np.full((gap, 3), poison_frag), np.full(gap, 3))
        for g in range(G):
            for d in range(F):
                parts.append(poison)
                at += gap
                w = pack_runs(runs[g][d])
                self.start[g, d] = at
                self.cur[g, d] = at + w.size
                parts.append(w)
                at += w.size
        parts.append(poison)
        self.window = np.concatenate(parts)
        self.end = self.cur.copy()

    def device(self, prefix):
        kw = {prefix + k: torch.from_numpy(v.astype(np.int32)).cuda() for k, v in
              (("start", self.start), ("cur", self.cur), ("end", self.end))}
        return torch.from_numpy(self.window.view(np.int64)).cuda(), kw


def split_runs(frags, rng):
    """One slice's fragments as 1-3 workgroup runs."""
    k = int(rng.integers(1, 4))
    cuts = np.sort(rng.integers(0, frags.size + 1, k - 1))
    return np.split(frags, cuts)


def join_reference(inner, outer, F):
    """searchsorted count per partition: outer fragments with a partner among the (unique) inner ones."""
    total = 0
    for d in range(F):
        r = np.sort(np.concatenate([inner[g][d] for g in range(G)]))
        s = np.concatenate([outer[g][d] for g in range(G)])
        if r.size == 0:
            continue
        i = np.clip(np.searchsorted(r, s), 0, r.size - 1)
        total += int((r[i] == s).sum())
    return total


def join_sides(bits, rng, F=3, per_part=6000):
    limit = 1 << bits
    inner = [[None] * F for _ in range(G)]
    outer = [[None] * F for _ in range(G)]
    for d in range(F):
        n_in = min(per_part, limit // 2)
        r = rng.choice(limit, n_in, replace=False).astype(np.uint64)  # unique per partition, half the range at most
        hits = rng.choice(r, 2 * n_in)  # duplicates among the outer tuples
        s = np.concatenate([hits, rng.integers(0, limit, n_in).astype(np.uint64)])  # and misses
        rng.shuffle(s)
        rc = np.sort(rng.integers(0, r.size + 1, G - 1))
        sc = np.sort(rng.integers(0, s.size + 1, G - 1))
        for g, (a, b) in enumerate(zip(np.split(r, rc), np.split(s, sc))):
            inner[g][d], outer[g][d] = a, b
    return inner, outer


def run_join(C, inner, outer, F, bits, rng, **shape):
    R = PackedSide([[split_runs(inner[g][d], rng) for d in range(F)] for g in range(G)], F, FMASK)
    S = PackedSide([[split_runs(outer[g][d], rng) for d in range(F)] for g in range(G)], F, FMASK)
    rw, rkw = R.device("r_")
    sw, skw = S.device("s_")
    return C.ops.bitmap_join(rw, sw, F, bits, **rkw, **skw, packed=True, **shape)


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [0, 1])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("bits", [12, 18, 20])
def test_packed_bitmap_join_counts(C, cuda, bits, threads, flat):
    rng = np.random.default_rng(bits * 10 + threads + flat)
    F = 3
    inner, outer = join_sides(bits, rng, F)
    exp = join_reference(inner, outer, F)
    assert 0 < exp < sum(outer[g][d].size for g in range(G) for d in range(F))
    got = run_join(C, inner, outer, F, bits, rng, threads=threads, flat=flat)
    assert (got["matches"], got["dup"], got["overflow"]) == (exp, 0, 0), got


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [0, 1])
def test_packed_bitmap_join_flags(C, cuda, flat):
    """A repeated inner fragment raises dup (inside one slice and across two groups); so does a fragment
    >= 2^bits when bits < 20; an overflowed slice (cur > end) raises overflow."""
    bits, F = 12, 3
    rng = np.random.default_rng(7 + flat)
    inner, outer = join_sides(bits, rng, F, per_part=900)
    assert run_join(C, inner, outer, F, bits, rng, flat=flat)["dup"] == 0

    def edited(edit):
        copy = [[inner[g][d].copy() for d in range(F)] for g in range(G)]
        edit(copy)
        return run_join(C, copy, outer, F, bits, rng, flat=flat)

    def repeat_in_slice(x):
        g = max(range(G), key=lambda g: x[g][1].size)
        x[g][1] = np.append(x[g][1], x[g][1][0])

    def repeat_across_groups(x):
        gs = [g for g in range(G) if x[g][2].size]
        x[gs[0]][2] = np.append(x[gs[0]][2], x[gs[-1]][2][-1])

    def out_of_range(x):
        x[3][0] = np.append(x[3][0], np.uint64(1 << bits))

    for edit in (repeat_in_slice, repeat_across_groups, out_of_range):
        assert edited(edit)["dup"] > 0, edit.__name__
    R = PackedSide([[split_runs(inner[g][d], rng) for d in range(F)] for g in range(G)], F, FMASK)
    S = PackedSide([[split_runs(outer[g][d], rng) for d in range(F)] for g in range(G)], F, FMASK)
    S.cur[2, 1] = S.end[2, 1] + 8
    rw, rkw = R.device("r_")
    sw, skw = S.device("s_")
    got = C.ops.bitmap_join(rw, sw, F, bits, **rkw, **skw, packed=True, flat=flat)
    assert got["overflow"] > 0 and got["dup"] == 0 and got["matches"] == join_reference(inner, outer, F)


# --------------------------------------------------------------- engine, GPU
def dense_tuples(n, seed):
    g = torch.Generator().manual_seed(seed)
    return tuples_of(torch.randperm(n, generator=g)).cuda()


def zipf_tuples(C, n, domain, seed):
    return H.gen(C, n, seed=seed, dist="ZIPF", domain=domain, device="cuda")


def engine(C, R, S, **cfg_fields):
    cfg = C.JoinConfig()
    for k, v in cfg_fields.items():
        setattr(cfg, k, v)
    ctx = C.ExecContext("device", 0, C.LocalCommunicator())
    return C.HashJoin(C.Relation.from_tensor(R, R.shape[0]), C.Relation.from_tensor(S, S.shape[0]), ctx, cfg)


@pytest.fixture(scope="module")
def engine_inputs(C, cuda):
    n = 1 << 20
    R = dense_tuples(n, 21)
    sets = {"dense": (R, dense_tuples(n, 22)), "zipf": (R, zipf_tuples(C, 3 * n, n, 23))}
    return {k: (r, s, H.ref_join_count(r[:, 0].contiguous(), s[:, 0].contiguous())) for k, (r, s) in sets.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dense", "zipf"])
def test_engine_packed_on_off(C, cuda, engine_inputs, which):
    R, S, exp = engine_inputs[which]
    got = {}
    for choice in ("ON", "OFF"):
        j = engine(C, R, S, packed_fragments=getattr(C.PlanChoice, choice))
        assert j.plan.bitmap_join and j.plan.packed_fragments == (choice == "ON"), j.plan
        assert (" packed" in repr(j.plan)) == (choice == "ON")
        res = j.run()
        assert res["bitmap_join"] and res["local_fallbacks"] == 0, res
        got[choice] = res["global_matches"]
        assert j.run()["global_matches"] == got[choice]  # a second join on the same engine
    assert got["ON"] == got["OFF"] == exp


@pytest.mark.gpu
def test_engine_duplicate_inner_falls_back(C, cuda, engine_inputs):
    """Repeated inner keys with replicate_bitmap = On force the bitmap plan; the packed join flags the
    repeat and the two-level fallback is exact."""
    R, S, _ = engine_inputs["dense"]
    R2 = R.clone()
    R2[:1000, 0] = R2[1000:2000, 0]
    exp = H.ref_join_count(R2[:, 0].contiguous(), S[:, 0].contiguous())
    j = engine(C, R2, S, replicate_bitmap=C.PlanChoice.ON, packed_fragments=C.PlanChoice.ON)
    assert j.plan.packed_fragments
    res = j.run()
    assert res["local_fallbacks"] == 1 and res["global_matches"] == exp
    assert not j.plan.packed_fragments and not j.plan.bitmap_join
    assert j.run()["global_matches"] == exp


@pytest.mark.gpu
def test_engine_slice_overflow_reruns_exactly(C, cuda):
    """Every 4096-tuple tile holds one network digit, so the sample misses most digits (the layout of
    test_join_engine.py's sampled-overflow tests, at a key range the bitmaps hold): the packed slices
    overflow and the exact re-run, still packed, is right."""
    n = 1 << 20
    i = torch.arange(n, device="cuda")
    keys = i * 512 + (i // 4096) % 512  # unique; 29 bits: 20-bit fragments above 9 radix bits
    R = torch.stack([keys, i], 1).contiguous()
    S = torch.stack([keys.flip(0), i], 1).contiguous()
    j = engine(C, R, S, network_histogram=C.HistogramMode.SAMPLED, key_hashing=C.KeyHashing.OFF, network_bits=9,
               max_partition_blocks=16, packed_fragments=C.PlanChoice.ON)
    assert j.plan.bitmap_join and j.plan.packed_fragments and j.plan.bitmap_bits == 20, j.plan
    res = j.run()
    assert res["network_fallbacks"] == 1 and res["local_fallbacks"] == 0 and res["global_matches"] == n, res
    assert j.run()["global_matches"] == n


@pytest.mark.gpu
def test_engine_eligibility(C, cuda, engine_inputs):
    R, S, _ = engine_inputs["dense"]
    n = R.shape[0]
    wide_keys = R.clone()
    wide_keys[0, 0] = (1 << 32) + 5  # 33-bit keys: the digit-array fragment policy
    cases = {
        "semi": dict(kind=C.JoinKind.SEMI, semi_bitmap=True),
        "group": dict(kind=C.JoinKind.GROUP),
        "33-bit keys": dict(),
    }
    for name, fields in cases.items():
        r = wide_keys if name == "33-bit keys" else R
        j = engine(C, r, S, **fields)
        assert not j.plan.packed_fragments and " packed" not in repr(j.plan), name
        with pytest.raises(RuntimeError, match="packed"):
            engine(C, r, S, packed_fragments=C.PlanChoice.ON, **fields)
    # A workspace budget below the two fragment windows forces partition-group passes.
    budget = dict(workspace_budget=6 << 20)
    j = engine(C, R, S, **budget)
    assert j.plan.bitmap_join and not j.plan.packed_fragments, j.plan
    res = j.run()
    assert res["group_passes"] > 1 and res["global_matches"] == n, res
    with pytest.raises(RuntimeError, match="packed"):
        engine(C, R, S, packed_fragments=C.PlanChoice.ON, **budget)


@pytest.mark.gpu
def test_engine_auto(C, cuda, engine_inputs):
    """Auto packs the eligible plan (the headline passed its A/B: profiles/r7/packed_fragments/README.md)."""
    R, S, exp = engine_inputs["dense"]
    j = engine(C, R, S)
    assert j.plan.bitmap_join and j.plan.packed_fragments and " packed" in repr(j.plan), j.plan
    assert j.run()["global_matches"] == exp


def test_config_knob(C, monkeypatch):
    from hpcjoin.utils import config_from_dict, config_to_dict
    assert config_to_dict(C.JoinConfig())["packed_fragments"] == "AUTO"
    assert config_from_dict({"packed_fragments": "off"}).packed_fragments == C.PlanChoice.OFF
    monkeypatch.setenv("HPCJOIN_PACKED_FRAGMENTS", "OFF")
    cfg = config_from_dict({})
    assert cfg.packed_fragments == C.PlanChoice.OFF and config_to_dict(cfg)["packed_fragments"] == "OFF"
