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
