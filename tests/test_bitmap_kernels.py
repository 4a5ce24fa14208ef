"""Content oracles of the three LDS bitmap kernels (kernels/bitmap_join.hip) and
of the direct-addressed 8-byte count table (kernels/build_probe.hip), called at
kernel level on windows this file lays out itself.

Inner sets: every build window here holds a seeded random subset of each
partition's fragment range (never the whole range), and the probe tests do not
build their bitmaps from any inner side at all: the bitmaps are seeded random
words.  A dense inner side cannot test a probe, because it sets every bit of
every bitmap: whatever word, bit, piece or partition the probe then reads, it
finds a 1 and counts |S|, exactly like a correct probe.  With random bits a
wrong read is right only half of the time per outer element.

Windows: slice starts sit on 16-element boundaries (the engine's contract; the
u32 walks read 16-byte vectors), the gaps between slices hold a poison fragment
that changes the counters if it is ever read (inner: 0xFFFFFFFF, outside every
bitmap, raises dup; outer: a fragment whose bit is set in every bitmap).

The sharpness check at the top is pure numpy: the key sets that
test_selective_inner.py joins tell a correct probe from the wrong ones.
"""
import numpy as np
import pytest
import torch

import helpers as H
from conftest import devices

G = H.CLAIM_GROUPS
POISON_R = 0xFFFFFFFF  # no bitmap holds it: an inner read of a gap raises dup
POISON_S = 1  # outer gaps: bit 1 of every bitmap is set, a read of a gap adds a match


# ---- sharpness of the selective inputs (numpy only) ---------------------------
# (D, network_bits, patterns): the sets of test_selective_inner.py.
SELECTIVE_SETS = [(1 << 20, 10, H.INNER_PATTERNS), (1 << 22, 1, H.PIECE_PATTERNS)]
# Which wrong probes each pattern exposes with its complement or uniform outer side, by construction:
#   bit        a set bit next to a clear one inside a word (whole words hide it)
#   word       word w differs from word w + 1 (a bitmap whose words are all alike hides it)
#   partition  partition d's bitmap differs from partition d ^ 1's
# The complement side exposes every read that lands on a set bit (its true count is 0, or 1 for the carried
# key D - 1), the uniform side every read that leaves a set bit for a clear one.
EXPOSES = {
    "half": {"bit", "word", "partition"},
    "one_bit_per_word": {"bit"},
    "one_word_in_k": {"word"},
    "even_partitions": {"partition"},
    "edges": {"bit", "word", "partition"},
    "low_piece": {"word"},
    "high_piece": {"word"},
}


def test_selective_inputs_are_sharp():
    """For every (inner, outer) pair of the selective tests except `same`, the count of an every-bit-set
    bitmap (all that a dense inner side can check) differs from the true count; for every pattern except
    the single key, the probes reading bit + 1, word + 1 or partition ^ 1 differ from the true count,
    with one outer side or the other, exactly where EXPOSES says: every pattern exposes at least one of
    them and every wrong probe is exposed by some pattern.  (No pattern but `half` and `edges` can expose
    all three: whole words hide a bit shift, equal partitions hide a partition swap.)"""
    exposed = set()
    for D, nb, patterns in SELECTIVE_SETS:
        bits = (D >> nb).bit_length() - 1
        for pattern in patterns:
            inner = H.inner_keys(pattern, D, nb)
            assert np.unique(inner).size == inner.size and 0 < inner.size < D
            rw, rs = H.key_slices(inner, nb)
            ref = H.bitmap_reference(rw, rs, 1 << nb, bits)
            assert not ref["dup"]
            differ = set()
            for kind in ("complement", "uniform"):
                outer = H.outer_keys(kind, inner, D)
                sw, ss = H.key_slices(outer, nb)
                count = {w: H.bitmap_probe_reference(ref["bitmaps"], sw, ss, bits, wrong=w)[0]
                         for w in (None, "all_ones", "bit", "word", "partition")}
                assert count[None] == H.ref_join_count(torch.from_numpy(inner), torch.from_numpy(outer))
                if kind == "complement":
                    assert count[None] == int(D - 1 in inner)
                assert count["all_ones"] == outer.size != count[None], (pattern, kind)
                differ |= {w for w in ("bit", "word", "partition") if count[w] != count[None]}
            if pattern != "single":
                assert differ == EXPOSES[pattern], (pattern, differ)
                exposed |= differ
    assert exposed == {"bit", "word", "partition"}


# ---- window layout -------------------------------------------------------------
def up16(x):
    return (np.asarray(x, dtype=np.int64) + 15) // 16 * 16


class Side:
    """One side's fragment window with claim slices [8, F] (numpy, then device tensors)."""

    def __init__(self, lengths, frags, poison, round_lp=0, wide=False, overflow=(), lv=0):
        lengths = np.asarray(lengths, dtype=np.int64)
        F = lengths.shape[1]
        cap = up16(lengths).ravel() + 16  # a poisoned gap after every slice
        if round_lp:  # slice i owns logical positions i << lv | k (lv: common to both sides of a kernel)
            lns = (G * F).bit_length() - 1
            assert 1 << lns == G * F and cap.max() <= 1 << lv and lv >= round_lp
            self.round_map = (round_lp, lv, lns)
            start = np.arange(G * F, dtype=np.int64) << lv
            size = int(-(-int(cap.max()) // (1 << round_lp))) << (lns + round_lp)
        else:
            self.round_map = (0, 0, 0)
            start = np.cumsum(cap) - cap
            size = int(cap.sum())
        fill = lengths.ravel()
        cur = start + fill
        end = start + up16(fill)
        for i in overflow:  # the claims ran past the slice end: only [start, end) holds fragments
            end[i] = start[i] + fill[i]
            cur[i] = end[i] + 7
        window = np.full(size, poison, dtype=np.uint32)
        _, slots = H.slice_slots(start, fill, self.round_map)
        assert np.unique(slots).size == slots.size and (slots.size == 0 or slots.max() < size)
        window[slots] = frags
        self.F, self.window, self.wide = F, window, wide
        self.start, self.cur, self.end = (x.reshape(G, F) for x in (start, cur, end))
        self.slices = H.claim_slices(self.start, self.cur, self.end)

    def device(self):
        ct = torch.int64 if self.wide else torch.int32
        dev = lambda a: torch.from_numpy(a.astype(np.int64)).to(ct).cuda().contiguous()
        kw = {"start": dev(self.start), "cur": dev(self.cur), "end": dev(self.end)}
        return torch.from_numpy(self.window.view(np.int32)).cuda(), kw

    def round_meta(self):
        if not self.round_map[1]:
            return None
        return torch.tensor(list(self.round_map) + [0], dtype=torch.int32).cuda()


def slice_lengths(F, batch, rng, small=False):
    """[8, F] slice lengths from the walks' own batch size (u32 elements per batch = threads * 16): 0, 1, 3,
    4, 5, one batch -1 / +0 / +1, two batches + 7, partitions mixing empty and sub-vector slices, an empty
    partition; `small`: the same edges below one vector and around 16 / 32 (bitmaps of 128 or 256 bits)."""
    if small:
        menu = [[0, 1, 3, 4, 5, 16, 17, 33], [0, 0, 2, 0, 1, 0, 3, 0], [0] * 8, [5, 0, 0, 0, 0, 0, 0, 4]]
    else:
        menu = [[0, 1, 3, 4, 5, batch - 1, batch, batch + 1], [2 * batch + 7, 0, 0, 2, 0, 1, 0, 3], [0] * 8,
                [5, 16, 17, 0, 4, 4, 1, 0]]
    L = rng.integers(0, 12 if small else 40, size=(G, F))
    L[rng.random((G, F)) < 0.3] = 0
    for j, m in enumerate(menu):
        for d in {j, F - 1 - j} if F >= 2 * len(menu) else {j} if j < F else ():
            L[:, d] = m
    return L.astype(np.int64)


def inner_fragments(L, limit, rng, anchor=None):
    """Unique fragments below `limit` per partition, in slice order i = g * F + d; `anchor` is among them
    wherever the partition is not empty."""
    F = L.shape[1]
    per = [[None] * F for _ in range(G)]
    for d in range(F):
        n = int(L[:, d].sum())
        assert n < limit, "a selective build leaves bits clear"
        f = rng.permutation(limit)[:n].astype(np.uint32)
        if anchor is not None and n and anchor not in f:
            f[0] = anchor
        f = rng.permutation(f)
        off = np.cumsum(L[:, d]) - L[:, d]
        for g in range(G):
            per[g][d] = f[off[g]:off[g] + L[g, d]]
    return np.concatenate([per[g][d] for g in range(G) for d in range(F)]) if L.sum() else np.zeros(0, np.uint32)


def outer_fragments(L, limit, rng, inner=None):
    """Draws with repeats over [0, 2 * limit): about half lie outside the bitmap and count nothing; a few
    sit on the boundaries.  With `inner` (some side's fragments) every other draw is one of those, so a
    join against a sparsely filled bitmap still has many hits to lose."""
    n = int(L.sum())
    f = rng.integers(0, 2 * limit, size=n, dtype=np.int64)
    if inner is not None and inner.size:
        f[::2] = rng.choice(inner, f[::2].size)
    edge = np.array([0, 31, 32, limit - 1, limit, 2 * limit - 1, 0xFFFFFFFF], dtype=np.int64)
    f[rng.integers(0, max(n, 1), size=min(n, 64))] = edge[rng.integers(0, edge.size, size=min(n, 64))]
    return f.astype(np.uint32)


def random_bitmaps(P, words, rng):
    bm = rng.integers(0, 1 << 32, size=(P, words), dtype=np.uint64).astype(np.uint32)
    bm[:, 0] |= np.uint32(1 << POISON_S)
    return bm


def as_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


# bits x (threads, flat); F, cursor width and window layout rotate so that every value meets every walk.
# bits 5: the 4-word minimum; 18 / 19: the 256 / 1024-thread switch; 21: two pieces per partition.
# round_lp 10 is the production piece of u32 fragment windows (JoinConfig.round_lp 9 + 1), 4 a smaller legal one.
SHAPES = []
for bi, bits in enumerate((5, 8, 18, 19, 20, 21)):
    for vi, (threads, flat) in enumerate(((256, 0), (256, 1), (1024, 0), (1024, 1))):
        F = (1024, 1, 2, 1024)[(bi + vi) % 4] if bits <= 8 else (2, 1, 2, 1)[(bi + vi) % 4]
        SHAPES.append(pytest.param(bits, threads, flat, F, (vi + bi) % 2 == 1, (0, 10, 4)[(bi + 2 * vi) % 3],
                                   id=f"b{bits}-t{threads}-f{flat}-F{F}"))
for bits in (18, 19):  # the kernels' own choice of threads and walk on both sides of the switch
    SHAPES.append(pytest.param(bits, 0, -1, 2, False, 0, id=f"b{bits}-auto"))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,threads,flat,F,wide,round_lp", SHAPES)
def test_bitmap_kernels_match_reference(C, cuda, bits, threads, flat, F, wide, round_lp):
    """Build: bitmaps equal the numpy reference word for word, dup stays 0.  Probe: seeded random bitmaps
    (built from no inner side), matches and popcount over a partition sub-range that does not start at 0.
    Join: the fused kernel equals reference build + probe.  Narrow and wide cursors, linear and
    round-interleaved windows, every slice-length edge of the walks."""
    rng = np.random.default_rng(1000 * bits + threads + flat + F)
    words = H.bitmap_words(bits)
    assert C.ops.bitmap_words(bits) == words
    limit = 32 * words
    batch = (threads or (256 if bits <= 18 else 1024)) * 16
    if F == 1024:
        round_lp = 0  # a round holds a piece of all 2^13 slices: the long slices would need a 1 GiB window
    Lr = slice_lengths(F, batch, rng, small=limit < 4 * batch + 64)
    Ls = slice_lengths(F, batch, rng)
    lv = max(round_lp, int(up16(max(Lr.max(), Ls.max())) + 15).bit_length())  # as the layout kernel picks it
    fr = inner_fragments(Lr, limit, rng, anchor=POISON_S)
    R = Side(Lr, fr, POISON_R, round_lp, wide, lv=lv)
    S = Side(Ls, outer_fragments(Ls, limit, rng, inner=fr), POISON_S, round_lp, wide, lv=lv)
    meta = R.round_meta()
    shape = dict(threads=threads, flat=flat, round_meta=meta)
    rw, rkw = R.device()
    sw, skw = S.device()

    ref = H.bitmap_reference(R.window, R.slices, F, bits, round_map=R.round_map)
    assert not ref["dup"] and not ref["overflow"]
    got = C.ops.bitmap_build(rw, F, bits, **rkw, **shape)
    assert (got["matches"], got["popcount"], got["dup"], got["overflow"]) == (0, 0, 0, 0)
    built = got["bitmaps"].cpu().numpy().view(np.uint32)
    assert built.shape == (F, words) and np.array_equal(built, ref["bitmaps"])

    bm = random_bitmaps(F, words, rng)
    first, count = (0, 1) if F == 1 else (1, 1) if F == 2 else (3, 700)
    for fc in ((0, F), (first, count)):
        m, p = H.bitmap_probe_reference(bm, S.window, S.slices, bits, round_map=S.round_map, first=fc[0], count=fc[1])
        got = C.ops.bitmap_probe(sw, as_i32(bm), F, bits, **skw, **shape, first=fc[0], count=fc[1])
        assert (got["matches"], got["popcount"], got["dup"], got["overflow"]) == (m, p, 0, 0), (fc, m, p)
    assert 0 < m < int(Ls[:, first:first + count].sum())

    m, _ = H.bitmap_probe_reference(ref["bitmaps"], S.window, S.slices, bits, round_map=S.round_map)
    got = C.ops.bitmap_join(rw, sw, F, bits, **{"r_" + k: v for k, v in rkw.items()},
                            **{"s_" + k: v for k, v in skw.items()}, **shape)
    assert (got["matches"], got["popcount"], got["dup"], got["overflow"]) == (m, 0, 0, 0)
    assert 0 < m < int(Ls.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [0, 1])
def test_bitmap_build_flags_repeats_and_range(C, cuda, flat):
    """dup is 0 exactly when no fragment repeats inside a partition: the same fragment in two partitions
    does not flag; a pair inside one slice, a pair across two claim groups of one partition, and a
    fragment >= 2^bits (21 bits: >= 2^21) each do.  A build of a partition sub-range flags only what the
    range holds and leaves the other partitions' words zero."""
    F, bits = 4, 10
    base = np.zeros((G, F), dtype=np.int64)
    base[0, :] = 40
    base[5, :] = 23

    def run(edit, bits=bits, **kw):
        rng = np.random.default_rng(5)
        fr = inner_fragments(base, 700, rng)  # 777 is in no partition
        side = Side(base, fr, POISON_R)
        w = side.window
        s = lambda g, d: int(side.start[g, d])
        edit(w, s)
        ref = H.bitmap_reference(w, side.slices, F, bits)
        rw, rkw = side.device()
        got = C.ops.bitmap_build(rw, F, bits, **rkw, flat=flat, **kw)
        return ref, got

    def same_in_two_partitions(w, s):
        w[s(0, 1) + 2] = 777
        w[s(0, 2) + 9] = 777
        w[s(5, 3) + 1] = 777

    def pair_in_slice(w, s):
        w[s(0, 2) + 7] = w[s(0, 2) + 30]

    def pair_across_groups(w, s):
        w[s(5, 1) + 22] = w[s(0, 1) + 3]

    def out_of_range(w, s):
        w[s(5, 3) + 4] = 1 << bits

    for edit, dup in ((same_in_two_partitions, False), (pair_in_slice, True), (pair_across_groups, True),
                      (out_of_range, True)):
        ref, got = run(edit)
        assert ref["dup"] == dup == (got["dup"] > 0), edit.__name__
        assert np.array_equal(got["bitmaps"].cpu().numpy().view(np.uint32), ref["bitmaps"]), edit.__name__
    # 21 bits: 2^20 lies in the second piece and is no error; 2^21 is outside both
    for frag, dup in ((1 << 20, False), (1 << 21, True)):
        ref, got = run(lambda w, s: w.__setitem__(s(0, 0) + 5, frag), bits=21)
        assert ref["dup"] == dup == (got["dup"] > 0), frag
        assert np.array_equal(got["bitmaps"].cpu().numpy().view(np.uint32), ref["bitmaps"])
    # sub-range [1, 3): the repeat in partition 3 is not seen, the one in partition 2 is
    for edit, dup in ((lambda w, s: w.__setitem__(s(0, 3) + 1, w[s(5, 3) + 2]), False), (pair_in_slice, True)):
        ref, got = run(edit, first=1, count=2)
        assert (got["dup"] > 0) == dup
        exp = ref["bitmaps"].copy()
        exp[[0, 3]] = 0
        assert np.array_equal(got["bitmaps"].cpu().numpy().view(np.uint32), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("threads,flat", [(256, 0), (256, 1), (1024, 0), (1024, 1)])
def test_bitmap_join_overflowed_slices(C, cuda, threads, flat):
    """overflow is set exactly when some cur > end, and only [start, end) of such a slice is read: what lies
    between end and cur is poison that would raise dup (inner) or add matches (outer)."""
    F, bits = 2, 12
    rng = np.random.default_rng(threads + flat)
    L = np.array([[37, 0], [5, 1000], [0, 0], [16, 3], [640, 0], [1, 1], [0, 18], [4, 33]], dtype=np.int64)
    fr = inner_fragments(L, 1 << bits, rng, anchor=POISON_S)
    fs = outer_fragments(L, 1 << bits, rng)
    for over_r, over_s in (((), ()), ((0, 3), ()), ((), (9,)), ((14,), (0, 15))):
        R, S = Side(L, fr, POISON_R, overflow=over_r), Side(L, fs, POISON_S, overflow=over_s)
        ref = H.bitmap_reference(R.window, R.slices, F, bits)
        assert ref["overflow"] == bool(over_r) and S.slices[3] == bool(over_s) and not ref["dup"]
        m, _ = H.bitmap_probe_reference(ref["bitmaps"], S.window, S.slices, bits)
        (rw, rkw), (sw, skw) = R.device(), S.device()
        got = C.ops.bitmap_join(rw, sw, F, bits, **{"r_" + k: v for k, v in rkw.items()},
                                **{"s_" + k: v for k, v in skw.items()}, threads=threads, flat=flat)
        assert got["matches"] == m and got["dup"] == 0, (over_r, over_s, got, m)
        assert (got["overflow"] > 0) == bool(over_r or over_s)
        b = C.ops.bitmap_build(rw, F, bits, **rkw, threads=threads, flat=flat)
        assert (b["overflow"] > 0) == bool(over_r) and b["dup"] == 0
        p = C.ops.bitmap_probe(sw, b["bitmaps"], F, bits, **skw, threads=threads, flat=flat)
        assert p["matches"] == m and (p["overflow"] > 0) == bool(over_s)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
def test_bitmap_kernels_segment_table(C, cuda, threads):
    """The 8-byte path: CompressedTuple words (fragment = value >> key_shift, rid bits below) addressed by a
    host-built segment table [F, groups] (TableSrc).  It is compiled public API with no production caller
    (the engine's bitmap plans read u32 fragments through claim slices) and had no test.  One batch is
    threads * 8 words here."""
    F, groups, bits, shift = 3, 3, 16, 40
    rng = np.random.default_rng(threads)
    limit, batch = 1 << bits, threads * 8
    lens = {"r": np.array([[0, 1, 3], [batch - 1, 0, batch + 1], [2 * batch + 7, 5, 0]], dtype=np.int64),
            "s": np.array([[batch + 1, 0, 2 * batch + 7], [3, batch, 1], [0, batch - 1, 4]], dtype=np.int64)}
    sides = {}
    for k, L in lens.items():
        gap = 5  # unread words between segments: no alignment contract on this path
        start = (np.cumsum(L.ravel() + gap) - L.ravel() - gap).reshape(F, groups) + 2
        poison = (1 << (64 - shift)) - 1 if k == "r" else POISON_S  # inner: the largest fragment, outside the bitmap
        window = np.full(int(start.max() + L.max() + gap), poison << shift, dtype=np.uint64)
        for d in range(F):
            n = int(L[d].sum())
            f = rng.permutation(limit)[:n] if k == "r" else rng.integers(0, 2 * limit, size=n)
            if k == "r" and n:
                f[0] = POISON_S if POISON_S not in f else f[0]
            f = f.astype(np.uint64) << np.uint64(shift) | rng.integers(0, 1 << shift, size=n).astype(np.uint64)
            off = 0
            for g in range(groups):
                window[start[d, g]:start[d, g] + L[d, g]] = f[off:off + L[d, g]]
                off += L[d, g]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
        sides[k] = (window, H.table_slices(start, L), dev(window), dev(start), dev(L))
    (rwin, rsl, rw, rst, rln), (swin, ssl, sw, sst, sln) = sides["r"], sides["s"]
    ref = H.bitmap_reference(rwin, rsl, F, bits, key_shift=shift)
    assert not ref["dup"]
    kw = dict(key_shift=shift, threads=threads)
    b = C.ops.bitmap_build(rw, F, bits, seg_start=rst, seg_len=rln, **kw)
    assert b["dup"] == 0 and np.array_equal(b["bitmaps"].cpu().numpy().view(np.uint32), ref["bitmaps"])
    bm = random_bitmaps(F, H.bitmap_words(bits), rng)
    m, p = H.bitmap_probe_reference(bm, swin, ssl, bits, key_shift=shift, first=1, count=2)
    got = C.ops.bitmap_probe(sw, as_i32(bm), F, bits, seg_start=sst, seg_len=sln, first=1, count=2, **kw)
    assert (got["matches"], got["popcount"]) == (m, p) and 0 < m
    m, _ = H.bitmap_probe_reference(ref["bitmaps"], swin, ssl, bits, key_shift=shift)
    got = C.ops.bitmap_join(rw, sw, F, bits, r_seg_start=rst, r_seg_len=rln, s_seg_start=sst, s_seg_len=sln, **kw)
    assert (got["matches"], got["dup"], got["overflow"]) == (m, 0, 0) and 0 < m < int(lens["s"].sum())
    # a repeated fragment with another rid is still a repeated key
    rwin2 = rwin.copy()
    a, c = int(rsl[1][3]), int(rsl[1][5])  # partition 1, groups 0 and 2
    rwin2[c + 7] = (rwin2[a + 11] >> np.uint64(shift) << np.uint64(shift)) | np.uint64(12345)
    assert H.bitmap_reference(rwin2, rsl, F, bits, key_shift=shift)["dup"]
    rw2 = torch.from_numpy(rwin2.view(np.int64)).cuda()
    assert C.ops.bitmap_build(rw2, F, bits, seg_start=rst, seg_len=rln, **kw)["dup"] > 0


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("frag_bits", [8, 13])
def test_build_probe_direct_count_selective(C, dev, frag_bits):
    """The direct-addressed count table over 8-byte words (frag_bits <= 13; the host twin hashes): the inner
    side is a random half of every partition's fragment range plus repeats, both sides repeat, and r_chunk
    / s_chunk split every partition into several items.  Slots of absent fragments must read 0 and
    repeated ones their multiplicity; a dense unique inner side makes every slot 1."""
    P, shift = 5, 32
    rng = np.random.default_rng(frag_bits)
    lim = 1 << frag_bits
    words, keys, begins = {}, {}, {}
    for side, reps in (("r", 3 * lim // 4), ("s", 9 * lim)):
        vals, ks, begin = [], [], [0]
        for p in range(P):
            half = rng.permutation(lim)[:lim // 2]
            f = np.concatenate([half, rng.choice(half, reps)]) if side == "r" else rng.integers(0, lim, reps)
            if p == 3:
                f = f[:0]  # an empty partition beside full ones
            f = rng.permutation(f).astype(np.int64)
            vals.append((f << shift) | rng.integers(0, 1 << 31, size=f.size))
            ks.append(f * P + p)
            begin.append(begin[-1] + f.size)
        words[side], keys[side], begins[side] = np.concatenate(vals), np.concatenate(ks), begin
    ref = H.ref_join_count(torch.from_numpy(keys["r"]), torch.from_numpy(keys["s"]))
    assert 0 < ref != keys["s"].size
    R, S = (torch.from_numpy(words[k]).contiguous().to(dev) for k in "rs")
    pr, ps = (torch.tensor(begins[k], dtype=torch.int64) for k in "rs")
    for r_chunk, s_chunk in ((1 << 18, 65536), (lim // 3 + 1, 4 * lim + 5)):
        res = C.ops.build_probe(R, S, pr, ps, shift, shift, r_chunk=r_chunk, s_chunk=s_chunk, frag_bits=frag_bits)
        assert res["matches"] == ref, (r_chunk, s_chunk, res["matches"], ref)
        if dev == "cuda" and r_chunk < lim:
            assert res["work_items"] > 2 * P
    with pytest.raises(RuntimeError, match="frag_bits"):
        C.ops.build_probe(R, S, pr, ps, shift, shift, frag_bits=frag_bits - 1)
