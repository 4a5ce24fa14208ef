"""Shared test helpers: plain PyTorch references for every kernel."""
import numpy as np
import torch


def gen(C, n, seed=1234, dist="UNIQUE", domain=0, device="cpu", offset=0, global_size=None, theta=0.75):
    spec = C.GenSpec(distribution=getattr(C.KeyDistribution, dist), seed=seed, domain=domain, zipf_theta=theta)
    return C.ops.generate(n, offset, global_size or n, spec, device)


def unpack(values, bits, key_shift, part_begin):
    """CompressedTuple -> (key, rid) using the partition each value lives in."""
    F = part_begin.numel() - 1
    sizes = (part_begin[1:] - part_begin[:-1]).to(values.device)
    part = torch.repeat_interleave(torch.arange(F, device=values.device), sizes)
    key = ((values >> key_shift) << bits) | part
    rid = values & ((1 << key_shift) - 1)
    return key, rid


def sorted_pairs(keys, rids):
    k = keys * (1 << 32) + rids  # keys and rids < 2^31 in tests
    return torch.sort(k).values


# ---- references of the scatter policies (test_scatter_policies.py) -----------
# Plain numpy in uint64 arithmetic: 64-bit mixing and 63-bit keys never pass
# through a signed shift.
CLAIM_GROUPS = 8


def u64(x):
    """int64 torch tensor / any integer array -> uint64 numpy array (bit pattern kept)."""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    if x.dtype == np.int64:
        return x.view(np.uint64)
    if x.dtype == np.int32:
        return x.view(np.uint32).astype(np.uint64)
    if x.dtype == np.int16:
        return x.view(np.uint16).astype(np.uint64)
    return x.astype(np.uint64)


def key_mix(k, bits):
    """KeyMix{1, bits}.apply: a bijection of [0, 2^bits)."""
    k = u64(k).copy()
    m = np.uint64(0xFFFFFFFFFFFFFFFF if bits >= 64 else (1 << bits) - 1)
    h = np.uint64((bits + 1) // 2)
    k = (k * np.uint64(0x9E3779B97F4A7C15)) & m
    k ^= k >> h
    k = (k * np.uint64(0xC2B2AE3D27D4EB4F)) & m
    k ^= k >> h
    return k


def round_slot(L, lp, lv, lns):
    """Physical slot of logical position L in a round-interleaved window (RoundMap)."""
    L = u64(L)
    lp, lv, lns = np.uint64(lp), np.uint64(lv), np.uint64(lns)
    one = np.uint64(1)
    k = L & ((one << lv) - one)
    return ((k >> lp) << (lns + lp)) | ((L >> lv) << lp) | (k & ((one << lp) - one))


def slice_slots(gstart, fill, round_map=(0, 0, 0)):
    """(slice id, physical slot) of the first fill[i] positions of every slice i."""
    gstart = np.asarray(gstart, dtype=np.int64).ravel()
    fill = np.asarray(fill, dtype=np.int64).ravel()
    sid = np.repeat(np.arange(fill.size, dtype=np.int64), fill)
    first = np.cumsum(fill) - fill
    L = gstart[sid] + (np.arange(sid.size, dtype=np.int64) - first[sid])
    lp, lv, lns = round_map
    slots = round_slot(L, lp, lv, lns).astype(np.int64) if lv else L
    return sid, slots


def rows_of(t):
    """A window / output column as uint64 rows [n, columns]."""
    a = u64(t)
    return a.reshape(a.shape[0], -1)


def slice_contents(window, gstart, fill, round_map=(0, 0, 0)):
    """Flat (slice id, value rows, slots) list of what the slices hold."""
    sid, slots = slice_slots(gstart, fill, round_map)
    return sid, rows_of(window)[slots], slots


def claim_group(i, tiles_per_block, partition_tile):
    return (np.asarray(i, dtype=np.int64) // (tiles_per_block * partition_tile)) % CLAIM_GROUPS


def expected_net(tuples, fmt, bits, tiles_per_block, partition_tile, key_shift=32, mix_bits=0, d_lo=0, rng=0):
    """(group, digit, staged value rows) of every tuple the network pass keeps."""
    t = u64(tuples)
    key, rid = t[:, 0], t[:, 1]
    mk = key_mix(key, mix_bits) if mix_bits else key
    b = np.uint64(bits)
    digit = (mk & np.uint64((1 << bits) - 1)).astype(np.int64)
    if fmt == "compressed":
        vals = (rid | ((mk >> b) << np.uint64(key_shift)))[:, None]
    elif fmt == "key_only":
        vals = (mk >> b)[:, None]
    elif fmt == "frag":
        vals = ((mk >> b) & np.uint64(0xFFFFFFFF))[:, None]
    elif fmt == "wide":
        vals = np.stack([mk, rid], axis=1)
    else:
        raise ValueError(fmt)
    group = claim_group(np.arange(key.size), tiles_per_block, partition_tile)
    if rng:
        keep = (digit >= d_lo) & (digit < d_lo + rng)
        group, digit, vals = group[keep], digit[keep] - d_lo, vals[keep]
    return group, digit, vals


def expected_local(rows, lp, shift, bits, mode, frag_shift=32, lo_shift=0):
    """(final partition, output rows) of input rows (word, or key and rid) of owned partition lp."""
    w = rows[:, 0]
    sub = ((w >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    part = np.asarray(lp, dtype=np.int64) * (1 << bits) + sub
    if mode in ("compressed", "wide"):
        out = rows
    elif mode == "split":
        out = np.stack([(w >> np.uint64(lo_shift)) & np.uint64(0xFFFFFFFF),
                        (w >> np.uint64(frag_shift)) & np.uint64(0xFFFF)], axis=1)
    elif mode == "frag":
        out = ((w >> np.uint64(frag_shift)) & np.uint64(0xFFFF))[:, None]
    else:
        raise ValueError(mode)
    return part, out


def canonical(ids, rows):
    """(ids, rows) sorted by id, then row: equal multisets per id <=> equal arrays."""
    order = np.lexsort(tuple(rows[:, c] for c in reversed(range(rows.shape[1]))) + (ids,))
    return ids[order], rows[order]


def multiset_excess(ids, rows, ref_ids, ref_rows):
    """Number of (id, row) occurrences that are not covered by the reference multiset."""
    a = np.concatenate([ids[:, None].astype(np.uint64), rows], axis=1)
    b = np.concatenate([ref_ids[:, None].astype(np.uint64), ref_rows], axis=1)
    _, inv = np.unique(np.concatenate([a, b]), axis=0, return_inverse=True)
    inv = inv.ravel()
    ca = np.bincount(inv[:a.shape[0]], minlength=inv.max() + 1 if inv.size else 0)
    cb = np.bincount(inv[a.shape[0]:], minlength=ca.size)
    return int(np.maximum(ca - cb, 0).sum())


def ref_join_count(r_keys, s_keys):
    """Exact |R join S| with torch: sum over S of multiplicity in R."""
    uk, cnt = torch.unique(r_keys, return_counts=True)
    idx = torch.searchsorted(uk, s_keys)
    idx = idx.clamp(max=uk.numel() - 1)
    hit = uk[idx] == s_keys
    return int(cnt[idx][hit].sum().item())


# ---- selective inner key sets (test_bitmap_kernels.py, test_selective_inner.py)
# A key of [0, D) is (fragment << network_bits) | digit: the network pass sends
# it to partition `digit`, whose bitmap (or count table) is indexed by
# `fragment`.  An inner side that holds every key sets every bit of every
# bitmap, so a probe that tests the wrong bit, word, piece or partition still
# counts |S|; the sets below leave gaps where such a probe lands.
INNER_PATTERNS = ("half", "one_bit_per_word", "one_word_in_k", "even_partitions", "edges", "single")
PIECE_PATTERNS = ("low_piece", "high_piece", "half")  # 21 fragment bits: two 2^20-bit pieces per partition
OUTER_KINDS = ("complement", "same", "uniform")


def inner_keys(pattern, D, network_bits, seed=7, bit=5, k=3, word=1):
    """Sorted unique int64 keys of [0, D) (D a power of two) of one pattern."""
    keys = np.arange(D, dtype=np.int64)
    frag, digit = keys >> network_bits, keys & ((1 << network_bits) - 1)
    limit, F = D >> network_bits, 1 << network_bits
    if pattern == "half":
        return np.sort(np.random.default_rng(seed).permutation(D)[:D // 2]).astype(np.int64)
    if pattern == "one_bit_per_word":
        return keys[(frag & 31) == bit]
    if pattern == "one_word_in_k":
        return keys[((frag >> 5) % k) == word]
    if pattern == "even_partitions":
        return keys[(digit & 1) == 0]
    if pattern == "low_piece":
        return keys[frag < (1 << 20)]
    if pattern == "high_piece":
        return keys[frag >= (1 << 20)]
    if pattern == "edges":
        f = np.array([0, 31, 32, limit - 1], dtype=np.int64)
        d = np.array([0, F - 1], dtype=np.int64)
        return np.sort(((f[:, None] << network_bits) | d[None, :]).ravel())
    if pattern == "single":
        return np.array([D - 1], dtype=np.int64)
    raise ValueError(pattern)


def outer_keys(kind, inner, D, n=0, seed=11):
    """Outer keys for a unique inner set.  complement: every key outside it (count 0, or 1 when the inner set
    holds D - 1: that key is always carried, so the planned key width is the pattern's own only for `same`);
    same: the inner keys permuted (count |R|); uniform: n seeded draws with repeats over [0, D)."""
    rng = np.random.default_rng(seed)
    if kind == "complement":
        mask = np.ones(D, dtype=bool)
        mask[inner] = False
        mask[D - 1] = True
        return rng.permutation(np.flatnonzero(mask)).astype(np.int64)
    if kind == "same":
        return rng.permutation(inner).astype(np.int64)
    if kind == "uniform":
        out = rng.integers(0, D, size=n or D // 2, dtype=np.int64)
        out[0] = D - 1
        return out
    raise ValueError(kind)


def key_tuples(keys, device="cpu", rid0=0):
    """[n, 2] int64 (key, rid) tensor for Relation.from_tensor."""
    k = torch.from_numpy(np.array(keys, dtype=np.int64))  # a copy: the shared key sets stay read-only
    return torch.stack([k, torch.arange(rid0, rid0 + k.numel(), dtype=torch.int64)], 1).contiguous().to(device)


# ---- numpy reference of the LDS bitmap kernels (kernels/bitmap_join.hip) ------
BITMAP_MAX_BITS = 20


def bitmap_words(bits):
    """u32 words of one partition's bitmap: 2^bits bits, at least 4 words; 21 bits are two 2^20-bit pieces."""
    split = max(bits - BITMAP_MAX_BITS, 0)
    return (1 << (bits - split - 5) if bits - split > 7 else 4) << split


def claim_slices(start, cur, end):
    """[groups, F] claim slices -> flat (partition, begin, length) and whether any cur > end (overflow)."""
    start, cur, end = (np.asarray(x, dtype=np.int64) for x in (start, cur, end))
    part = np.broadcast_to(np.arange(start.shape[1], dtype=np.int64), start.shape)
    return part.ravel(), start.ravel(), (np.minimum(cur, end) - start).ravel(), bool((cur > end).any())


def table_slices(seg_start, seg_len):
    """[F, groups] segment table -> flat (partition, begin, length); a table cannot overflow."""
    seg_start, seg_len = np.asarray(seg_start, dtype=np.int64), np.asarray(seg_len, dtype=np.int64)
    part = np.broadcast_to(np.arange(seg_start.shape[0], dtype=np.int64)[:, None], seg_start.shape)
    return part.ravel(), seg_start.ravel(), seg_len.ravel(), False


def slice_fragments(window, slices, key_shift=0, round_map=(0, 0, 0)):
    """(partition, fragment) of every element the slices hold, fragments as uint64."""
    part, begin, length, _ = slices
    sid, slots = slice_slots(begin, length, round_map)
    return part[sid], u64(window)[slots] >> np.uint64(key_shift)


def bitmap_reference(window, slices, partitions, bits, key_shift=0, round_map=(0, 0, 0)):
    """Build reference: bitmaps [partitions, bitmap_words(bits)] uint32, and the dup / overflow flags.
    Bit f of partition d is set iff fragment f < 32 * words occurs in d; dup iff a fragment repeats inside
    a partition or lies outside the bitmap."""
    words = bitmap_words(bits)
    limit = np.uint64(32 * words)
    part, frag = slice_fragments(window, slices, key_shift, round_map)
    inside = frag < limit
    idx = part[inside].astype(np.uint64) * limit + frag[inside]
    uniq = np.unique(idx)
    w = np.zeros(partitions * words, dtype=np.uint64)
    np.add.at(w, (uniq >> np.uint64(5)).astype(np.int64), np.uint64(1) << (uniq & np.uint64(31)))
    assert int(w.max(initial=0)) < (1 << 32)
    return {"bitmaps": w.astype(np.uint32).reshape(partitions, words),
            "dup": bool((~inside).any() or uniq.size != idx.size), "overflow": slices[3]}


def bitmap_probe_reference(bitmaps, window, slices, bits, key_shift=0, round_map=(0, 0, 0), first=0, count=None,
                           wrong=None):
    """(matches, popcount) of probing `bitmaps` [partitions, words] over partitions [first, first + count).
    wrong = "all_ones" | "bit" | "word" | "partition": what a kernel computes that sets every bit, tests
    bit + 1 of the word, word + 1 of the bitmap (the last word: word - 1), or partition ^ 1's bitmap (the sharpness check)."""
    bm = np.ascontiguousarray(bitmaps, dtype=np.uint32)
    P, words = bm.shape
    assert words == bitmap_words(bits)
    count = P - first if count is None else count
    limit = np.uint64(32 * words)
    part, frag = slice_fragments(window, slices, key_shift, round_map)
    keep = (part >= first) & (part < first + count) & (frag < limit)
    part, frag = part[keep], frag[keep]
    if wrong == "bit":
        frag = (frag & ~np.uint64(31)) | ((frag + np.uint64(1)) & np.uint64(31))
    elif wrong == "word":
        frag = np.where(frag + np.uint64(32) < limit, frag + np.uint64(32), frag - np.uint64(32))  # last word: w - 1
    elif wrong == "partition":
        part = np.minimum(part ^ 1, P - 1)
    word = bm[part, (frag >> np.uint64(5)).astype(np.int64)].astype(np.uint64)
    hit = (word >> (frag & np.uint64(31))) & np.uint64(1)
    if wrong == "all_ones":
        hit = np.ones_like(hit)
    sel = bm[first:first + count].view(np.uint8)
    return int(hit.sum()), int(np.unpackbits(sel).sum())


def key_slices(keys, network_bits):
    """Keys as a (window of fragments, one slice per partition) pair for the references above."""
    keys = np.asarray(keys, dtype=np.int64)
    F = 1 << network_bits
    digit = keys & (F - 1)
    order = np.argsort(digit, kind="stable")
    cnt = np.bincount(digit, minlength=F).astype(np.int64)
    begin = np.cumsum(cnt) - cnt
    return (keys[order] >> network_bits), (np.arange(F, dtype=np.int64), begin, cnt, False)
