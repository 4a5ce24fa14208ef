"""Key-column relations: a plain int64 key column whose rids are positions.

Three layers are covered.

Kernel content (gpu).  ops.net_scatter_slices over a 1-D key tensor runs the
key-column instantiations of the rid-free scatter policies (u32 fragments,
packed fragment words, key-only words).  Per digit, over the digit's eight
group slices, what they write must be the same multiset as what the tuple
instantiations write for torch.stack([k, arange], 1), and as the numpy
reference (digit = mix(k) & mask, fragment = mix(k) >> bits); every other
window element, guard included, keeps the sentinel.

Engine, native (gpu).  A key-column side of a join whose network pass carries
no rid is read in place: the count is right, equals the same join on tuple
relations, repeats, the result says "native" and no expansion exists.

Expansion (cpu and gpu).  Everything that needs a rid runs on the relation's
tuple expansion {keys[i], rid_offset + i} and says "expanded".
"""
import threading

import numpy as np
import pytest
import torch

import helpers as H
from conftest import devices

G = H.CLAIM_GROUPS
GUARD = 64
TILE = 8192  # elements per scatter tile
SIZES = [1000, TILE, 3 * TILE + 5, 1 << 18]
FB, FMASK = 20, (1 << 20) - 1


def tuples_of(keys, rid0=0):
    return torch.stack([keys, torch.arange(rid0, rid0 + keys.numel(), dtype=torch.int64, device=keys.device)],
                       1).contiguous()


# ------------------------------------------------------------ kernel content
# format, bits of the generated keys (None: bits + 20, what a packed fragment holds), key_bits argument
FORMATS = {"frag": 27, "frag_packed": None, "key_only": 63}


def random_keys(n, key_bits, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, min(1 << key_bits, (1 << 63) - 1), (n,), generator=gen, dtype=torch.int64)


def digit_contents(C, res, fmt, Fp):
    """(digit, value) of everything the slices hold, the slots they occupy, and the window rows."""
    gstart, gcur, gend = (res[k].numpy().astype(np.int64) for k in ("gstart", "gcur", "gend"))
    assert gstart.shape == (G, Fp)
    fill, cap = (gcur - gstart).ravel(), (gend - gstart).ravel()
    assert (fill <= cap).all(), "a slice overflowed: its content would depend on the order of the claims"
    window = res["window"].cpu()
    assert window.shape[0] == res["capacity"] + GUARD
    sid, rows, slots = H.slice_contents(window, gstart, fill, res["round_map"])
    assert np.unique(slots).size == slots.size and (slots.size == 0 or int(slots.max()) < res["capacity"])
    digit, vals = sid % Fp, rows[:, 0]
    if fmt == "frag_packed":
        frags, counts = C.ops.unpack_fragments(torch.from_numpy(vals.view(np.int64).copy()))
        frags, counts = frags.numpy(), counts.numpy()
        valid = np.arange(3)[None, :] < counts[:, None]
        digit, vals = np.repeat(digit, 3).reshape(-1, 3)[valid], frags[valid].astype(np.uint64)
    return digit, vals, slots, H.rows_of(window), (gstart, gcur, gend)


def check_column_scatter(C, keys, fmt, bits, key_bits, *, mix_bits=0, d_lo=0, rng=0, **kw):
    """Key column vs tuples vs numpy, per digit; sentinels everywhere else."""
    assert keys.is_cuda and keys.dim() == 1
    Fp = rng or (1 << bits)
    args = dict(guard=GUARD, key_bits=key_bits, mix_bits=mix_bits, max_blocks=16, **kw)
    if rng:
        args.update(d_lo=d_lo, range=rng)
    col = C.ops.net_scatter_slices(keys, bits, fmt, **args)
    tup = C.ops.net_scatter_slices(tuples_of(keys), bits, fmt, **args)
    dc, vc, slots, rows, cursors_c = digit_contents(C, col, fmt, Fp)
    dt, vt, _, _, cursors_t = digit_contents(C, tup, fmt, Fp)
    for a, b in zip(cursors_c, cursors_t):  # the same histogram laid out the same slices, filled alike
        assert np.array_equal(a, b)
    for k in ("round_map", "capacity", "capacity_used", "blocks", "tiles_per_block", "sample_stride", "narrow"):
        assert col[k] == tup[k], k
    if fmt == "frag_packed":
        assert col["wide_flag"] == 0 and tup["wide_flag"] == 0
    _, rd, rv = H.expected_net(tuples_of(keys.cpu()), "frag" if fmt == "frag_packed" else fmt, bits,
                               col["tiles_per_block"], C.ops.partition_tile(), 32, mix_bits, d_lo, rng)
    a, b, r = H.canonical(dc, vc[:, None]), H.canonical(dt, vt[:, None]), H.canonical(rd, rv)
    assert np.array_equal(a[0], r[0]) and np.array_equal(a[1], r[1]), "key column differs from the reference"
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "key column differs from the tuple scatter"
    untouched = np.ones(rows.shape[0], dtype=bool)
    untouched[slots] = False
    width = 32 if fmt == "frag" else 64
    sent = np.uint64(C.ops.scatter_sentinel() & ((1 << 64) - 1)) & np.uint64((1 << width) - 1)
    assert (rows[untouched] == sent).all(), "a store landed outside the filled slice ranges"
    return col


def format_keys(fmt, n, bits, seed):
    gen_bits = bits + FB if FORMATS[fmt] is None else FORMATS[fmt]
    return random_keys(n, gen_bits, seed).cuda(), gen_bits


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("sample_stride", [1, 4])
@pytest.mark.parametrize("bits", [5, 10])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_column_scatter_matches_tuples(C, cuda, fmt, n, bits, sample_stride, mixed):
    keys, key_bits = format_keys(fmt, n, bits, n + bits)
    res = check_column_scatter(C, keys, fmt, bits, key_bits, mix_bits=key_bits if mixed else 0,
                               sample_stride=sample_stride)
    if n == 1 << 18:  # 16 workgroups of two scatter tiles each: the prefetch crosses a tile end and a range end
        assert res["blocks"] == 16 and res["tiles_per_block"] * C.ops.partition_tile() == 2 * TILE


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("bits", [5, 10])
def test_column_scatter_33_bit_keys(C, cuda, bits, mixed):
    """Keys of 32 + bits bits: the fragment fills the u32 and the digit goes to the tile's digit array."""
    key_bits = 32 + bits
    keys = random_keys(3 * TILE + 5, key_bits, 33 + bits).cuda()
    keys[0] = (1 << key_bits) - 1
    check_column_scatter(C, keys, "frag", bits, key_bits, mix_bits=key_bits if mixed else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("key_bits", [27, 37])
@pytest.mark.parametrize("bits,d_lo,rng", [(5, 3, 7), (10, 100, 300)])
def test_column_scatter_range_pass(C, cuda, bits, d_lo, rng, key_bits):
    """A partition-group pass: only digits [d_lo, d_lo + range) are written, renumbered from 0."""
    keys = random_keys(3 * TILE + 5, key_bits, 7 + bits).cuda()
    check_column_scatter(C, keys, "frag", bits, key_bits, d_lo=d_lo, rng=rng)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_column_scatter_unaligned_base(C, cuda, fmt):
    """A column that starts 8 bytes past a 16-byte boundary."""
    bits, n = 5, 3 * TILE + 5
    buf, key_bits = format_keys(fmt, n + 1, bits, 99)
    keys = buf[1:]
    assert keys.is_contiguous() and keys.data_ptr() % 16 == 8
    check_column_scatter(C, keys, fmt, bits, key_bits)
    assert torch.equal(C.ops.net_histogram(keys, bits), C.ops.net_histogram(tuples_of(keys), bits))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [5, 10])
@pytest.mark.parametrize("n", SIZES)
def test_column_histogram_matches_tuples(C, cuda, n, bits):
    keys = random_keys(n, 40, n).cuda()
    got = C.ops.net_histogram(keys, bits)
    assert torch.equal(got, C.ops.net_histogram(tuples_of(keys), bits))
    ref = np.bincount((H.u64(keys) & np.uint64((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
    assert np.array_equal(got.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_column_scatter_empty(C, cuda, fmt):
    res = C.ops.net_scatter_slices(torch.empty(0, dtype=torch.int64, device="cuda"), 5, fmt, guard=GUARD, key_bits=25)
    assert torch.equal(res["gcur"], res["gstart"]), "an empty column claimed slots"
    rows = H.rows_of(res["window"].cpu())
    width = 32 if fmt == "frag" else 64
    sent = np.uint64(C.ops.scatter_sentinel() & ((1 << 64) - 1)) & np.uint64((1 << width) - 1)
    assert (rows == sent).all()


# ------------------------------------------------------------ engine, native
N = 1 << 20


def config(C, **fields):
    cfg = C.JoinConfig()
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def relation(C, keys, column, rid_offset=0, global_size=None):
    g = global_size or keys.numel()
    if column:
        return C.Relation.from_keys(keys, g, rid_offset)
    return C.Relation.from_tensor(tuples_of(keys, rid_offset), g)


def native_case(C, kR, kS, expected, columns=(True, True), **fields):
    """The five assertions every native case makes; returns the key-column engine and its first result."""
    ctx = C.ExecContext("device", 0, C.LocalCommunicator())
    R, S = relation(C, kR, columns[0]), relation(C, kS, columns[1])
    j = C.HashJoin(R, S, ctx, config(C, **fields))
    assert "keyColumns=" in repr(j.plan) and "(in place)" in repr(j.plan), j.plan
    res = j.run()
    again = j.run()
    tj = C.HashJoin(relation(C, kR, False), relation(C, kS, False), C.ExecContext("device", 0, C.LocalCommunicator()),
                    config(C, **fields))
    tuples = tj.run()
    assert "keyColumns" not in repr(tj.plan) and tuples["key_columns"] == ("tuples", "tuples")
    assert res["global_matches"] == expected, (res["global_matches"], expected)
    assert res["global_matches"] == tuples["global_matches"]
    assert again["global_matches"] == res["global_matches"]
    want = tuple("native" if c else "tuples" for c in columns)
    assert res["key_columns"] == want and again["key_columns"] == want, (res["key_columns"], again["key_columns"])
    assert not R.expanded and not S.expanded
    assert R.is_key_column == columns[0] and S.is_key_column == columns[1]
    return j, res, tuples


@pytest.fixture(scope="module")
def dense_keys(C, cuda):
    gen = torch.Generator().manual_seed(5)
    kR = torch.randperm(N, generator=gen).cuda()
    kS = torch.randperm(N, generator=gen).cuda()
    zipf = H.gen(C, 3 * N, seed=23, dist="ZIPF", domain=N, device="cuda")[:, 0].contiguous()
    return {"dense": (kR, kS, N), "zipf": (kR, zipf, H.ref_join_count(kR, zipf))}


@pytest.mark.gpu
@pytest.mark.parametrize("packed", ["ON", "OFF"])
@pytest.mark.parametrize("which", ["dense", "zipf"])
def test_native_bitmap_plan(C, cuda, dense_keys, which, packed):
    kR, kS, exp = dense_keys[which]
    j, res, _ = native_case(C, kR, kS, exp, packed_fragments=getattr(C.PlanChoice, packed))
    assert j.plan.bitmap_join and j.plan.packed_fragments == (packed == "ON"), j.plan
    assert res["bitmap_join"] and res["local_fallbacks"] == 0, res


@pytest.mark.gpu
@pytest.mark.parametrize("columns", [(True, False), (False, True)], ids=["inner", "outer"])
def test_native_one_side_tuples(C, cuda, dense_keys, columns):
    kR, kS, exp = dense_keys["zipf"]
    j, res, _ = native_case(C, kR, kS, exp, columns=columns)
    assert ("keyColumns=inner(" in repr(j.plan)) == columns[0] and ("keyColumns=outer(" in repr(j.plan)) == columns[1]


@pytest.mark.gpu
def test_native_duplicate_inner_falls_back_to_fragments(C, cuda, dense_keys):
    """Repeated inner keys under replicate_bitmap = ON: the bitmap join flags them and the two-level fragments
    plan, still reading the columns in place, is exact."""
    kR, kS, _ = dense_keys["dense"]
    kR = kR.clone()
    kR[:1000] = kR[1000:2000]
    exp = H.ref_join_count(kR, kS)
    j, res, tuples = native_case(C, kR, kS, exp, replicate_bitmap=C.PlanChoice.ON,
                                 network_histogram=C.HistogramMode.SAMPLED)
    assert res["local_fallbacks"] == 1 and tuples["local_fallbacks"] == 1, res
    assert not j.plan.bitmap_join and " fragments" in repr(j.plan) and "(in place)" in repr(j.plan), j.plan


@pytest.mark.gpu
def test_native_slice_overflow_reruns_exactly(C, cuda):
    """Every 4096-tuple tile holds one network digit, so the sample misses most digits: the slices overflow
    and the exact re-run still reads the columns in place."""
    i = torch.arange(N, device="cuda")
    keys = i * 512 + (i // 4096) % 512
    j, res, _ = native_case(C, keys, keys.flip(0).contiguous(), N, network_histogram=C.HistogramMode.SAMPLED,
                            key_hashing=C.KeyHashing.OFF, network_bits=9, max_partition_blocks=16)
    assert j.plan.bitmap_join, j.plan
    assert res["network_fallbacks"] == 1 and res["local_fallbacks"] == 0, res


@pytest.mark.gpu
def test_native_key_only_path(C, cuda):
    """Random 63-bit keys: key-only words through the sampled two-level pass."""
    gen = torch.Generator().manual_seed(63)
    kR = torch.unique(torch.randint(0, (1 << 63) - 1, (N,), generator=gen, dtype=torch.int64))
    kR = kR[torch.randperm(kR.numel(), generator=gen)].cuda()
    kS = torch.cat([kR[: N // 2], torch.randint(0, (1 << 63) - 1, (N // 2,), generator=gen, dtype=torch.int64).cuda()])
    kS = kS[torch.randperm(kS.numel(), device="cuda")].contiguous()
    j, res, _ = native_case(C, kR, kS, H.ref_join_count(kR, kS), network_histogram=C.HistogramMode.SAMPLED)
    assert j.plan.key_only and j.plan.sampled_network and not j.plan.bitmap_join, j.plan
    assert res["sampled_network"] and res["network_fallbacks"] == 0, res


def overflow_keys(high=0):
    """Every 4096-tuple tile holds one network digit (of 512): the sample misses most digits."""
    i = torch.arange(N, device="cuda")
    keys = (i * 512 + (i // 4096) % 512) | high
    return keys, keys.flip(0).contiguous()


@pytest.mark.gpu
def test_native_key_only_overflow_stays_in_place(C, cuda):
    """63-bit keys on the two-level key-only plan: the sampled slices overflow, and the exact re-run (exact
    histogram, unbounded key-only scatter) and every later, exact join still read the columns in place."""
    kR, kS = overflow_keys(1 << 62)
    j, res, _ = native_case(C, kR, kS, N, network_histogram=C.HistogramMode.SAMPLED, key_hashing=C.KeyHashing.OFF,
                            network_bits=9, max_partition_blocks=16)
    assert j.plan.key_only and not j.plan.bitmap_join, j.plan
    assert res["network_fallbacks"] == 1 and not res["sampled_network"], res
    assert "(in place)" in repr(j.plan), j.plan
    later = j.run()
    assert later["network_fallbacks"] == 0 and not later["sampled_network"] and later["global_matches"] == N
    assert later["key_columns"] == ("native", "native")


@pytest.mark.gpu
def test_fragments_overflow_expands_and_says_so(C, cuda):
    """The two-level fragments plan writes u32 fragments in its sampled pass only: after a slice overflow the exact
    pass writes CompressedTuples with rids, so the columns are expanded -- and result and plan both say it."""
    kR, kS = overflow_keys()
    ctx = C.ExecContext("device", 0, C.LocalCommunicator())
    R, S = relation(C, kR, True), relation(C, kS, True)
    j = C.HashJoin(R, S, ctx, config(C, network_histogram=C.HistogramMode.SAMPLED, key_hashing=C.KeyHashing.OFF,
                                     network_bits=9, local_bits=6, bitmap_join=False, max_partition_blocks=16))
    assert j.plan.fragments and "(in place)" in repr(j.plan), j.plan
    res = j.run()
    assert res["network_fallbacks"] == 1 and res["global_matches"] == N, res
    assert res["key_columns"] == ("expanded", "expanded") and R.expanded and S.expanded
    assert "(expanded)" in repr(j.plan), j.plan
    assert j.run()["global_matches"] == N


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["SEMI", "ANTI"])
def test_native_semi_bitmap_count(C, cuda, dense_keys, kind):
    """Count-only semi / anti joins on the set plan: unique inner keys, so the semi count is the join count."""
    kR = dense_keys["dense"][0]
    kS = torch.randint(0, 2 * N, (N,), generator=torch.Generator().manual_seed(9), dtype=torch.int64).cuda()
    hits = H.ref_join_count(kR, kS)
    assert 0 < hits < N
    j, res, _ = native_case(C, kR, kS, hits if kind == "SEMI" else N - hits, kind=getattr(C.JoinKind, kind),
                            semi_bitmap=True)
    assert j.plan.bitmap_join and j.plan.bitmap_set, j.plan


@pytest.mark.gpu
def test_native_partition_group_passes(C, cuda, dense_keys):
    """A workspace budget below the two fragment windows forces partition-group passes (range scatters)."""
    kR, kS, exp = dense_keys["dense"]
    j, res, _ = native_case(C, kR, kS, exp, workspace_budget=6 << 20)
    assert j.plan.bitmap_join and res["group_passes"] > 1, res


# ---------------------------------------------------------------- expansion
RID0 = 1_000_003


def small_keys(dev, seed=3):
    gen = torch.Generator().manual_seed(seed)
    kR = torch.randperm(20_000, generator=gen)
    kS = torch.randint(0, 30_000, (50_000,), generator=gen, dtype=torch.int64)
    return kR.to(dev), kS.to(dev)


def engines(C, dev, kR, kS, rid0, **fields):
    """(engine, relations, context) over key columns and over tuples with the same rids."""
    out = []
    for column in (True, False):
        loc = "device" if dev == "cuda" else "host"
        ctx = C.ExecContext(loc, 0 if dev == "cuda" else -1, C.LocalCommunicator())
        R, S = relation(C, kR, column, rid0), relation(C, kS, column, rid0)
        out.append((C.HashJoin(R, S, ctx, config(C, **fields)), R, S, ctx))
    return out


def sorted_rows(t):
    t = t.cpu()
    keys = [t[:, c].numpy() for c in reversed(range(t.shape[1]))]
    return t[torch.from_numpy(np.lexsort(keys))]


@pytest.mark.parametrize("dev", devices())
def test_expanded_materialize(C, dev):
    kR, kS = small_keys(dev)
    (j, R, S, _), (tj, _, _, _) = engines(C, dev, kR, kS, RID0, materialize=True)
    assert "(expanded)" in repr(j.plan), j.plan
    res, ref = j.run(), tj.run()
    assert res["key_columns"] == ("expanded", "expanded") and R.expanded and S.expanded
    assert res["global_matches"] == ref["global_matches"] == H.ref_join_count(kR, kS)
    pairs = sorted_rows(j.output())
    assert torch.equal(pairs, sorted_rows(tj.output()))
    assert int(pairs.min()) >= RID0
    assert torch.equal(kR.cpu()[pairs[:, 0] - RID0], kS.cpu()[pairs[:, 1] - RID0])
    assert torch.equal(R.to_tensor().cpu(), tuples_of(kR.cpu(), RID0))


@pytest.mark.parametrize("dev", devices())
def test_expanded_semi_rids(C, dev):
    kR, kS = small_keys(dev)
    (j, R, S, _), (tj, _, _, _) = engines(C, dev, kR, kS, RID0, kind=C.JoinKind.SEMI, materialize=True)
    res = j.run()
    tj.run()
    assert res["key_columns"] == ("expanded", "expanded")
    rids = torch.sort(j.output_rids().cpu()).values
    assert torch.equal(rids, torch.sort(tj.output_rids().cpu()).values)
    member = torch.isin(kS.cpu(), kR.cpu())
    assert torch.equal(rids, torch.nonzero(member).ravel() + RID0)


@pytest.mark.parametrize("dev", devices())
def test_expanded_group_values(C, dev):
    """join_group with a value column indexed by the outer rid offset."""
    kR, kS = small_keys(dev)
    values = torch.arange(kS.numel(), dtype=torch.int64, device=kS.device) * 3 + 1
    rows = []
    for j, R, S, ctx in engines(C, dev, kR, kS, RID0, kind=C.JoinKind.GROUP, materialize=True):
        res, r = j.join_group(ctx, values, RID0, values.shape[0])
        rows.append(sorted_rows(r))
        if R.is_key_column:
            assert res["key_columns"] == ("expanded", "expanded")
    assert torch.equal(rows[0], rows[1])
    got = rows[0]
    assert got.shape == (kR.numel(), 3) and torch.equal(got[:, 0], torch.arange(kR.numel()) + RID0)
    count = torch.bincount(kS.cpu(), minlength=30_000)
    sums = torch.zeros(30_000, dtype=torch.int64).index_add_(0, kS.cpu(), values.cpu())
    assert torch.equal(got[:, 1], count[kR.cpu()]) and torch.equal(got[:, 2], sums[kR.cpu()])


def test_expanded_host_count(C):
    kR, kS = small_keys("cpu")
    (j, R, S, _), (tj, _, _, _) = engines(C, "cpu", kR, kS, 0)
    res = j.run()
    assert res["global_matches"] == tj.run()["global_matches"] == H.ref_join_count(kR, kS)
    assert res["key_columns"] == ("expanded", "expanded") and R.expanded and S.expanded
    assert "keyColumns=inner,outer(expanded)" in repr(j.plan), j.plan  # the host path never reads in place
    assert j.run()["global_matches"] == res["global_matches"]


def test_expanded_two_host_ranks(C):
    """Each in-process rank holds a slice of the key columns; its rids start at the slice's global offset."""
    kR, kS = small_keys("cpu")
    group = C.InProcessGroup(2)
    results, errors = [None, None], []

    def rank_main(r):
        try:
            ctx = C.ExecContext("host", -1, group.communicator(r))
            rels = []
            for keys in (kR, kS):
                g = keys.numel()
                off, n = C.Relation.local_offset_for(g, r, 2), C.Relation.local_size_for(g, r, 2)
                rels.append(C.Relation.from_keys(keys[off:off + n].contiguous(), g, off))
            res = C.HashJoin(rels[0], rels[1], ctx, C.JoinConfig()).run()
            results[r] = (res, rels[0].expanded and rels[1].expanded)
        except Exception as e:  # surface in the main thread
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    exp = H.ref_join_count(kR, kS)
    for res, expanded in results:
        assert res["global_matches"] == exp and res["key_columns"] == ("expanded", "expanded") and expanded
    assert sum(res["local_matches"] for res, _ in results) == exp


@pytest.mark.parametrize("dev", devices())
def test_ops_accept_key_columns(C, dev):
    from hpcjoin import ops
    kR, kS = small_keys(dev)
    tR, tS = tuples_of(kR), tuples_of(kS)
    exp = H.ref_join_count(kR, kS)
    assert ops.join_count(kR, kS) == ops.join_count(tR, tS) == exp
    assert ops.join_count(kR, tS) == ops.join_count(tR, kS) == exp
    pairs = sorted_rows(ops.join(kR, kS))
    assert torch.equal(pairs, sorted_rows(ops.join(tR, tS))) and pairs.shape == (exp, 2)
    assert torch.equal(kR.cpu()[pairs[:, 0]], kS.cpu()[pairs[:, 1]])  # rids are positions


@pytest.mark.parametrize("dev", devices())
def test_ops_kinds_accept_key_columns(C, dev):
    from hpcjoin import ops
    kR, kS = small_keys(dev)
    tR, tS = tuples_of(kR), tuples_of(kS)
    assert ops.semi_join_count(kR, kS) == ops.semi_join_count(tR, tS)
    assert ops.anti_join_count(kR, kS) == kS.numel() - ops.semi_join_count(kR, kS)
    assert torch.equal(torch.sort(ops.semi_join(kR, kS).cpu()).values, torch.sort(ops.semi_join(tR, tS).cpu()).values)
    assert ops.full_outer_join_count(kR, kS) == ops.full_outer_join_count(tR, tS)
    assert torch.equal(sorted_rows(ops.left_outer_join(kR, kS)), sorted_rows(ops.left_outer_join(tR, tS)))
    assert torch.equal(sorted_rows(ops.group_join_count(kR, kS)), sorted_rows(ops.group_join_count(tR, tS)))
    values = torch.arange(kS.numel(), dtype=torch.int64, device=kS.device)
    assert torch.equal(sorted_rows(ops.group_join_sum(kR, kS, values)), sorted_rows(ops.group_join_sum(tR, tS, values)))
    assert torch.equal(ops.radix_histogram(kR, 5).cpu(), ops.radix_histogram(tR, 5).cpu())


# ----------------------------------------------------------------- refusals
def test_from_keys_refuses_other_input(C):
    k = torch.arange(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"dtype Int with shape \[10\]"):
        C.Relation.from_keys(k.int(), 10)
    with pytest.raises(RuntimeError, match=r"dtype Long with shape \[5, 2\]"):
        C.Relation.from_keys(k.reshape(5, 2), 5)
    with pytest.raises(RuntimeError, match=r"shape \[5\] \(not contiguous\)"):
        C.Relation.from_keys(k[::2], 5)
    R = C.Relation.from_keys(k, 10, 7)
    assert R.is_key_column and not R.expanded and R.local_size() == 10 and R.location() == "host"
    assert torch.equal(R.to_tensor(), tuples_of(k, 7)) and R.expanded
    assert not C.Relation.from_tensor(tuples_of(k), 10).is_key_column


def test_key_column_cannot_be_rewritten(C):
    """Generators and distribute() rewrite tuples in place; a key column is a view of the caller's keys."""
    R = C.Relation.from_keys(torch.arange(100, dtype=torch.int64), 100)
    for call in (lambda: R.generate(C.GenSpec(seed=1), 0), lambda: R.fill_unique_values(0, 0),
                 lambda: R.fill_modulo_values(0, 0, 10), lambda: R.distribute(0, 2, C.LocalCommunicator())):
        with pytest.raises(RuntimeError, match="key column"):
            call()
    assert not R.expanded


@pytest.mark.parametrize("fmt", ["compressed", "wide"])
def test_scatter_slices_refuses_columns_for_rid_formats(C, fmt):
    with pytest.raises(RuntimeError, match="carries a rid"):
        C.ops.net_scatter_slices(torch.arange(100, dtype=torch.int64), 5, fmt)
