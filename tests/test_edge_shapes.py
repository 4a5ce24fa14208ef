"""Edge shapes: tiny and empty relations through every plan and kind, ranks that
own nothing, and keys one bit below, at and above every width at which the
planner switches layout (core/JoinConfig.cpp, operators/HashJoin.cpp).

Every expected value is plain torch on CPU copies of the (key, rid) tensors:
the inner keys sorted, ``searchsorted`` left / right of the outer keys gives
each outer tuple's partners, ``repeat_interleave`` expands them into the pair
list, ``torch.isin`` both ways gives the unmatched tuples (class ``Ref``); group
aggregates come from ``test_group_typed.TypedOracle`` (whose constructor has no
share guard).  The oracles of test_outer_join / test_semi_join / test_group_join
assert ">= 5 % matched" and the like in their constructors, which (0, 1) tuples
cannot satisfy, so ``Ref`` is local; their row checks (sorted rows, no row
twice) are imported as they are.  Nothing is taken from the host engine, from
``Relation.expected_matches`` or from another plan.

Rids start at 1,000,003 so that a rid is never a position.  Every join is run
twice on the same ``HashJoin`` object (marks, counters and identities are
re-initialised between runs), with ``reserve_workspace = False``.

A. ``test_sizes_*``: 17 (|R|, |S|) pairs around 0, 1, the wave (64), the
   workgroup (256) and the 4096-tuple tile, two key shapes (mixed, one key), a
   unique-inner and a sparse 63-bit variant.  ``test_sizes_plan_coverage`` asserts
   that over the pairs with both sides >= 63 the device really took every plan
   the matrix is meant to reach.
B. ``test_ranks_*``: 4 in-process ranks, global sizes that leave ranks empty.
C. ``test_width_*``: 3,005 inner keys below 2^kb with the zero and the all-ones
   fragment planted, 4 + 4 radix bits, kb on both sides of every flip.
D. ``test_scan_u32_edges``, ``test_kernels_on_sixteen_partitions``.
"""
import functools
import threading

import pytest
import torch

from conftest import devices
from test_group_join import _check_rows as check_group_rows
from test_group_typed import TypedOracle, _bits, _typed_columns
from test_outer_join import KEEP, NULL, _check_rows as check_pair_rows, _sorted_rows
from test_semi_join import _check_rids

OFF = 1_000_003
INF_BITS = _bits(float("inf"))
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 4097), (4097, 0), (1, 4097), (4097, 1), (63, 65), (64, 64), (65, 63),
         (255, 257), (256, 256), (257, 255), (4095, 4097), (4096, 4096), (4097, 4095)]
BIG = [p for p in PAIRS if min(p) >= 63]
NONEMPTY = [p for p in PAIRS if min(p) >= 1]
SPARSE_MUL = (1 << 50) + 0x9E3779B1  # keys below 5,120 become keys of up to 63 bits
OUTER_KINDS = ["LEFT_OUTER", "RIGHT_OUTER", "FULL_OUTER"]
PACKED_REFUSAL = "not the single-pass counting bitmap"  # HashJoin::planPackedFragments (test_packed_fragments pins it)


def _loc(dev):
    return "device" if dev == "cuda" else "host"


def _ctx(C, dev, comm=None):
    return C.ExecContext(_loc(dev), 0 if dev == "cuda" else -1, comm or C.LocalCommunicator())


def _cfg(C, **fields):
    cfg = C.JoinConfig()
    cfg.reserve_workspace = False
    for k, v in fields.items():
        setattr(cfg, k, getattr(C.JoinKind, v) if k == "kind" else v)
    return cfg


def _tuples(keys, rid0=OFF):
    return torch.stack([keys, torch.arange(rid0, rid0 + keys.numel(), dtype=torch.int64)], 1).contiguous()


# ---------------------------------------------------------------------- oracle
class Ref:
    """Brute force on CPU tensors: pair list, qualifying outer rids, unmatched tuples, per-inner counts."""

    def __init__(self, R, S):
        assert R.device.type == "cpu" and S.device.type == "cpu"
        self.R, self.S = R, S
        self.n_r, self.n_s = R.shape[0], S.shape[0]
        rk, order = torch.sort(R[:, 0], stable=True)
        rr = R[:, 1][order]
        sk, sr = S[:, 0].contiguous(), S[:, 1]
        lo = torch.searchsorted(rk, sk, right=False)
        self.partners = torch.searchsorted(rk, sk, right=True) - lo  # per outer tuple
        self.count = int(self.partners.sum())
        first = torch.cumsum(self.partners, 0) - self.partners
        within = torch.arange(self.count) - torch.repeat_interleave(first, self.partners)
        pairs = torch.stack([rr[torch.repeat_interleave(lo, self.partners) + within],
                             torch.repeat_interleave(sr, self.partners)], 1)
        self.pairs = _sorted_rows(pairs)
        self.outer_hit = self.partners > 0
        self.inner_hit = torch.isin(R[:, 0], sk)
        assert torch.equal(self.outer_hit, torch.isin(sk, R[:, 0]))
        self.rids = {"SEMI": sr[self.outer_hit].sort().values, "ANTI": sr[~self.outer_hit].sort().values}
        self.un_inner, self.un_outer = R[:, 1][~self.inner_hit], sr[~self.outer_hit]
        self.group = TypedOracle(R, S, OFF)  # counts per inner tuple from the outer keys sorted
        assert int(self.group.counts.sum()) == self.count
        self._rows = {}

    def guard(self):
        """What a mixed case with both sides >= 63 must hold for the kinds to differ (asserted before any engine runs)."""
        fig = (self.count, int((~self.inner_hit).sum()), int((~self.outer_hit).sum()),
               self.n_r - torch.unique(self.R[:, 0]).numel(), int((self.partners >= 2).sum()))
        assert all(f >= 1 for f in fig), fig
        return self

    def outer_counts(self, kind):
        keep_r, keep_s = KEEP[kind]
        return self.count, self.un_inner.numel() if keep_r else 0, self.un_outer.numel() if keep_s else 0

    def outer_rows(self, kind):
        if kind not in self._rows:
            keep_r, keep_s = KEEP[kind]
            parts = [self.pairs]
            if keep_r:
                parts.append(torch.stack([self.un_inner, torch.full_like(self.un_inner, NULL)], 1))
            if keep_s:
                parts.append(torch.stack([torch.full_like(self.un_outer, NULL), self.un_outer], 1))
            self._rows[kind] = _sorted_rows(torch.cat(parts))
        return self._rows[kind]

    def group_rows(self, columns=(), aggs=()):
        return self.group.rows(list(columns), list(aggs))


def _pair_histogram(rows, n_r, n_s):
    """Occurrences of every possible (inner rid or NULL, outer rid or NULL) row: rows are equal as multisets exactly
    when these are equal, and a row emitted twice shows as a 2."""
    rows = rows.cpu()
    r = torch.where(rows[:, 0] == NULL, torch.zeros_like(rows[:, 0]), rows[:, 0] - OFF + 1)
    s = torch.where(rows[:, 1] == NULL, torch.zeros_like(rows[:, 1]), rows[:, 1] - OFF + 1)
    assert bool(((r >= 0) & (r <= n_r) & (s >= 0) & (s <= n_s)).all()), "a rid outside the relations"
    return torch.bincount(r * (n_s + 1) + s, minlength=(n_r + 1) * (n_s + 1))


def _check_pairs(rows, expected, ref):
    """test_outer_join._check_rows (sorted rows, none twice); above 2^17 rows -- the one-key cross products of the
    4096-tuple pairs, 16.7M rows -- the same equality through _pair_histogram, which needs no sort."""
    if expected.shape[0] <= 1 << 17:
        return check_pair_rows(rows, expected)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == tuple(expected.shape), (rows.shape, expected.shape)
    key = ("histogram", id(expected))
    if key not in ref._rows:
        ref._rows[key] = (expected, _pair_histogram(expected, ref.n_r, ref.n_s))
    want = ref._rows[key][1]
    assert int(want.max()) == 1
    assert torch.equal(_pair_histogram(rows, ref.n_r, ref.n_s), want)


class Case:
    def __init__(self, rk, sk, guard=False, tuples=None):
        """From key tensors (rids OFF + position), or from ready (R, S) tuple tensors."""
        self.R, self.S = tuples if tuples is not None else (_tuples(rk), _tuples(sk))
        self.ref = Ref(self.R, self.S)
        if guard:
            self.ref.guard()
        self._dev = {}

    def on(self, dev):
        """(R, S) tuple tensors on the device, moved once."""
        if dev not in self._dev:
            self._dev[dev] = (self.R.to(dev), self.S.to(dev))
        return self._dev[dev]

    def relations(self, C, dev, columns=False):
        R, S = self.on(dev)
        if columns:  # 1-D key columns read in place; fresh objects, since an expansion would stick to them
            return (C.Relation.from_keys(R[:, 0].contiguous(), R.shape[0], OFF),
                    C.Relation.from_keys(S[:, 0].contiguous(), S.shape[0], OFF))
        return C.Relation.from_tensor(R, R.shape[0]), C.Relation.from_tensor(S, S.shape[0])


@functools.lru_cache(maxsize=None)
def _size_case(shape, n_r, n_s):
    """mixed: inner uniform over D = max(1, |R| // 2) keys, outer uniform over 2 D keys from D // 2.  one: key 5
    everywhere.  unique: inner a random subset of [0, 2 |R|), outer as for mixed over that range.  sparse: mixed
    times SPARSE_MUL.  Seeds depend on the sizes only; the guards of Ref.guard hold for every pair >= 63 (asserted)."""
    g = torch.Generator().manual_seed(7919 * n_r + n_s + 1)
    D = max(1, n_r // 2)
    if shape == "one":
        return Case(torch.full((n_r,), 5, dtype=torch.int64), torch.full((n_s,), 5, dtype=torch.int64))
    if shape == "unique":
        rk = torch.randperm(2 * n_r, generator=g)[:n_r]
        sk = torch.randint(n_r // 2, n_r // 2 + 2 * max(1, n_r), (n_s,), generator=g)
        case = Case(rk, sk)
        assert torch.unique(rk).numel() == n_r
        if min(n_r, n_s) >= 63:
            assert 0 < case.ref.count < n_s
        return case
    rk = torch.randint(0, D, (n_r,), generator=g)
    sk = torch.randint(D // 2, D // 2 + 2 * D, (n_s,), generator=g)
    if shape == "sparse":
        rk, sk = rk * SPARSE_MUL, sk * SPARSE_MUL
        assert int(sk.max() if n_s else 0) < 2**63 and int(rk.min() if n_r else 0) >= 0
    return Case(rk, sk, guard=min(n_r, n_s) >= 63)


def test_oracle_guards_hold():
    """The guards are part of the host run: every mixed / sparse / unique case >= 63 can tell the kinds apart."""
    for n_r, n_s in PAIRS:
        for shape in ("mixed", "sparse", "unique", "one"):
            case = _size_case(shape, n_r, n_s)
            assert case.ref.pairs.shape[0] == case.ref.count
            if shape == "one":
                assert case.ref.count == n_r * n_s
    assert len(BIG) == 9 and len(NONEMPTY) == 12


# ------------------------------------------------------------- engine runners
TAKEN = {}  # plan flag -> (|R|, |S|, config) of the first device case >= 63 that took it
DONE = set()  # matrix functions that ran to the end on the device in this session (_done)


def _done(dev, key):
    if dev == "cuda":
        DONE.add(key)


def _record(dev, case, j, res, tag):
    if dev != "cuda" or min(case.ref.n_r, case.ref.n_s) < 63:
        return
    p = j.plan
    flags = {"bitmap": res["bitmap_join"] and not p.bitmap_set, "packed": res["bitmap_join"] and p.packed_fragments,
             "bitmap_set": res["bitmap_join"] and p.bitmap_set, "fragments": p.fragments and not res["bitmap_join"],
             "key_only": p.key_only, "wide": p.wide, "split_local": p.split_local and not res["bitmap_join"],
             "single_level": not p.two_level and not p.bitmap_join,
             "key_columns": res["key_columns"] == ("native", "native")}
    for name, on in flags.items():
        if on:
            TAKEN.setdefault(name, (case.ref.n_r, case.ref.n_s, tag))


def _engine(C, dev, ctx, case, columns=False, **fields):
    R, S = case.relations(C, dev, columns)
    return C.HashJoin(R, S, ctx, _cfg(C, **fields))


def _run_count(C, dev, ctx, case, tag, expected, columns=False, **fields):
    j = _engine(C, dev, ctx, case, columns, **fields)
    for _ in range(2):
        res = j.run()
        assert res["global_matches"] == res["local_matches"] == expected, (tag, res["global_matches"], expected, j.plan)
        assert res["output_pairs"] == 0 and res["output_rids"] == 0
    _record(dev, case, j, res, tag)
    return j, res


def _run_pairs(C, dev, ctx, case, tag, **fields):
    j = _engine(C, dev, ctx, case, materialize=True, **fields)
    for _ in range(2):
        res = j.run()
        assert res["global_matches"] == res["output_pairs"] == case.ref.count, (tag, res["global_matches"], j.plan)
        _check_pairs(j.output(), case.ref.pairs, case.ref)
    _record(dev, case, j, res, tag)
    return j, res


def _run_rids(C, dev, ctx, case, tag, kind, **fields):
    want = case.ref.rids[kind]
    j = _engine(C, dev, ctx, case, kind=kind, materialize=True, **fields)
    for _ in range(2):
        res = j.run()
        assert res["global_matches"] == res["local_matches"] == res["output_rids"] == want.numel(), (tag, kind, j.plan)
        _check_rids(j.output_rids(), want)
    _record(dev, case, j, res, tag)
    return j, res


def _run_outer(C, dev, ctx, case, tag, kind, materialize, **fields):
    j = _engine(C, dev, ctx, case, kind=kind, materialize=materialize, **fields)
    pairs, un_r, un_s = case.ref.outer_counts(kind)
    for _ in range(2):
        res = j.run()
        assert (res["matched_pairs"], res["unmatched_inner"], res["unmatched_outer"]) == (pairs, un_r, un_s), (tag, kind)
        assert res["global_matches"] == res["local_matches"] == pairs + un_r + un_s
        if materialize:
            _check_pairs(j.output(), case.ref.outer_rows(kind), case.ref)
        else:
            assert res["output_pairs"] == 0
    _record(dev, case, j, res, tag)
    return j, res


def _check_group_result(res, ref, tag):
    assert (res["matched_pairs"], res["unmatched_inner"], res["unmatched_outer"]) == (
        ref.count, int((ref.group.counts == 0).sum()), 0), (tag, res)
    assert res["global_matches"] == res["local_matches"] == ref.n_r


def _run_group(C, dev, ctx, case, tag, materialize, **fields):
    j = _engine(C, dev, ctx, case, kind="GROUP", materialize=materialize, **fields)
    for _ in range(2):
        res = j.run()
        _check_group_result(res, case.ref, tag)
        if materialize:
            check_group_rows(j.output_groups(), case.ref.group_rows())
        else:
            assert res["output_groups"] == 0
    _record(dev, case, j, res, tag)
    return j, res


# ------------------------------------------------------------ A. size matrix
INNER_CONFIGS = ["default", "hash-exact-exact", "hash-exact-sampled", "hash-sampled-exact", "hash-sampled-sampled",
                 "single", "wide", "no-split", "no-direct", "r-chunk-512"]


def _inner_config(C, name):
    """Default = split_local on, direct_count on, r_chunk 0: the other value of each is listed, the default once."""
    modes = {"exact": C.HistogramMode.EXACT, "sampled": C.HistogramMode.SAMPLED}
    if name.startswith("hash-"):
        _, net, local = name.split("-")
        return dict(bitmap_join=False, network_histogram=modes[net], local_histogram=modes[local])
    return {"default": {}, "single": dict(two_level=False), "wide": dict(format=C.TupleFormat.WIDE),
            "no-split": dict(split_local=False), "no-direct": dict(direct_count=False),
            "r-chunk-512": dict(r_chunk=512)}[name]


def _matrix_inner(C, dev, shape, what, config, pairs):
    ctx = _ctx(C, dev)
    fields = _inner_config(C, config)
    for n_r, n_s in pairs:
        case = _size_case(shape, n_r, n_s)
        tag = (shape, n_r, n_s, config, what)
        if what == "count":
            _run_count(C, dev, ctx, case, tag, case.ref.count, **fields)
        else:
            j, _ = _run_pairs(C, dev, ctx, case, tag, **fields)
            assert not j.plan.bitmap_join and not j.plan.key_only and not j.plan.fragments, (tag, j.plan)


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("config", INNER_CONFIGS)
@pytest.mark.parametrize("what", ["count", "pairs"])
@pytest.mark.parametrize("shape", ["mixed", "one"])
def test_sizes_inner(C, dev, shape, what, config):
    _matrix_inner(C, dev, shape, what, config, PAIRS)
    _done(dev, ("inner", shape, what, config))


def _matrix_sparse(C, dev, pairs):
    ctx = _ctx(C, dev)
    for n_r, n_s in pairs:
        case = _size_case("sparse", n_r, n_s)
        tag = ("sparse", n_r, n_s)
        j, _ = _run_count(C, dev, ctx, case, tag + ("count",), case.ref.count)
        # makePlan: more than 32 key bits above the network digit cannot sit in a CompressedTuple (keyShift 32) --
        # key-only words for the count, the wide format for pairs.  The keys are 0 or at least 2^50.
        top = max(int(case.R[:, 0].max()) if n_r else 0, int(case.S[:, 0].max()) if n_s else 0)
        assert j.plan.key_bits == top.bit_length()
        assert j.plan.key_only == (j.plan.key_bits - j.plan.network_bits > 32) == (top > 0), (tag, j.plan)
        assert not j.plan.wide, (tag, j.plan)
        j, _ = _run_pairs(C, dev, ctx, case, tag + ("pairs",))
        assert j.plan.wide == (j.plan.key_bits - j.plan.network_bits > 32) == (top > 0), (tag, j.plan)
        assert not j.plan.key_only, (tag, j.plan)


@pytest.mark.parametrize("dev", devices())
def test_sizes_sparse(C, dev):
    _matrix_sparse(C, dev, PAIRS)
    _done(dev, ("sparse",))


def _unique_configs(C):
    S, ON, OFFC = C.HistogramMode.SAMPLED, C.PlanChoice.ON, C.PlanChoice.OFF
    return [("bitmap", dict(bitmap_join=True, network_histogram=S, packed_fragments=OFFC)),
            ("packed", dict(bitmap_join=True, network_histogram=S, packed_fragments=ON)),
            ("replicated", dict(replicate_bitmap=ON)),
            ("fragments", dict(bitmap_join=False, network_histogram=S))]


def _count_or_packed_refusal(C, dev, ctx, case, tag, columns, fields):
    """Runs the count.  packed_fragments = ON is refused at construction where the plan is not eligible (pinned by
    test_packed_fragments.test_engine_eligibility): that refusal alone is accepted, by its message, and only when
    the same plan without the demand is indeed not packed."""
    try:
        return _run_count(C, dev, ctx, case, tag, case.ref.count, columns, **fields)
    except RuntimeError as e:
        assert fields.get("packed_fragments") == C.PlanChoice.ON and PACKED_REFUSAL in str(e), (tag, str(e))
    auto = dict(fields, packed_fragments=C.PlanChoice.AUTO)
    j, res = _run_count(C, dev, ctx, case, tag + ("refused",), case.ref.count, columns, **auto)
    assert not j.plan.packed_fragments, (tag, j.plan)
    return j, res


def _matrix_unique(C, dev, pairs):
    ctx = _ctx(C, dev)
    for n_r, n_s in pairs:
        case = _size_case("unique", n_r, n_s)
        for name, fields in _unique_configs(C):
            for columns in (False, True):
                tag = ("unique", n_r, n_s, name, "columns" if columns else "tuples")
                j, res = _count_or_packed_refusal(C, dev, ctx, case, tag, columns, fields)
                if dev == "cuda" and name == "packed":
                    # one device rank, counting bitmap plan, keys below 2^14: eligible at every size
                    assert j.plan.bitmap_join and j.plan.packed_fragments and res["bitmap_join"], (tag, j.plan)
                if dev == "cpu" and name == "packed":
                    assert not j.plan.packed_fragments  # the host engine never packs: refused, then run unpacked


@pytest.mark.parametrize("dev", devices())
def test_sizes_unique_inner(C, dev):
    _matrix_unique(C, dev, PAIRS)
    _done(dev, ("unique",))


def _matrix_semi_anti(C, dev, shape, pairs):
    ctx = _ctx(C, dev)
    for n_r, n_s in pairs:
        case = _size_case(shape, n_r, n_s)
        for kind in ("SEMI", "ANTI"):
            for semi_bitmap in (False, True):
                tag = (shape, n_r, n_s, kind, "set" if semi_bitmap else "marks")
                j, _ = _run_count(C, dev, ctx, case, tag, case.ref.rids[kind].numel(), kind=kind,
                                  semi_bitmap=semi_bitmap)
                assert j.plan.bitmap_set == semi_bitmap, (tag, j.plan)  # keys below 2^13: the set plan always fits
                j, _ = _run_rids(C, dev, ctx, case, tag, kind, semi_bitmap=semi_bitmap)
                assert j.plan.bitmap_set == semi_bitmap, (tag, j.plan)


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("shape", ["mixed", "one"])
def test_sizes_semi_anti(C, dev, shape):
    _matrix_semi_anti(C, dev, shape, PAIRS)
    _done(dev, ("semi", shape))


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("kind", OUTER_KINDS)
@pytest.mark.parametrize("shape", ["mixed", "one"])
def test_sizes_outer(C, dev, shape, kind):
    ctx = _ctx(C, dev)
    for n_r, n_s in PAIRS:
        case = _size_case(shape, n_r, n_s)
        for materialize in (False, True):
            _run_outer(C, dev, ctx, case, (shape, n_r, n_s, kind, materialize), kind, materialize)


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("shape", ["mixed", "one"])
def test_sizes_group(C, dev, shape):
    ctx = _ctx(C, dev)
    for n_r, n_s in PAIRS:
        case = _size_case(shape, n_r, n_s)
        ref = case.ref
        tag = (shape, n_r, n_s)
        _run_group(C, dev, ctx, case, tag + ("count",), False)
        _run_group(C, dev, ctx, case, tag + ("rows",), True)
        # int64 SUM and float64 MIN: k / 8 values (exact in any order), an empty group carries 0 and +inf
        f64, _, _ = _typed_columns(n_s, 300 + n_s, dev)
        i64 = torch.randint(-2**40, 2**40, (n_s,), generator=torch.Generator().manual_seed(n_s)).to(dev)
        want = ref.group_rows([i64, f64], ["sum", "min"])
        empty = want[:, 1] == 0
        assert bool((want[empty, 2] == 0).all()) and bool((want[empty, 3] == INF_BITS).all())
        assert int(empty.sum()) == int((~ref.inner_hit).sum())
        j = _engine(C, dev, ctx, case, kind="GROUP", materialize=True, group_columns=2)
        for _ in range(2):
            res, rows = j.join_group_agg(ctx, [i64, f64], ["sum", "min"], OFF, n_s)
            _check_group_result(res, ref, tag)
            assert list(res["group_dtypes"]) == ["int64", "float64"]
            check_group_rows(rows, want)
            check_group_rows(j.output_groups(), want)
            got_empty = rows.cpu()[rows.cpu()[:, 1] == 0]
            assert bool((got_empty[:, 2] == 0).all()) and bool((got_empty[:, 3] == INF_BITS).all()), tag


def _payload(n, seed, dev):
    return torch.randint(-2**62, 2**62, (n, 4), generator=torch.Generator().manual_seed(seed)).to(dev)


def _check_payload_words(rows, rid_col, first_word, payload):
    """Words [first_word, first_word + 4) of every row are payload[rid - OFF], or four NULL words for a NULL rid:
    plain indexing of the payload tensor (on the device the rows are on)."""
    rid = rows[:, rid_col]
    words = rows[:, first_word:first_word + 4]
    real = rid != NULL
    if bool(real.all()):  # (no masked copies of 16.7M-row results)
        assert torch.equal(words, payload[rid - OFF])
        return
    assert torch.equal(words[real], payload[rid[real] - OFF])
    assert bool((words[~real] == NULL).all())


# The one-key cross products of the three 4096-tuple pairs are 16.7M rows of 80 bytes each: one function each.
PAYLOAD_SIZES = {"to-4097x1": [p for p in NONEMPTY if min(p) <= 257], "4095x4097": [(4095, 4097)],
                 "4096x4096": [(4096, 4096)], "4097x4095": [(4097, 4095)]}


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("sizes", list(PAYLOAD_SIZES))
@pytest.mark.parametrize("kind", ["INNER", "SEMI", "FULL_OUTER"])
@pytest.mark.parametrize("shape", ["mixed", "one"])
def test_sizes_payload_rows(C, dev, shape, kind, sizes):
    """Fused rows of the inner join (join_materialized) and the row forms of the semi and the full outer join
    (HashJoin.join_rows, which ops.semi_join_rows / ops.full_outer_join_rows call): the rid columns against the
    oracle's rows, the payload words against indexing the payload tensors with the row's own rids."""
    from hpcjoin import ops
    ctx = _ctx(C, dev)
    for n_r, n_s in PAYLOAD_SIZES[sizes]:
        case = _size_case(shape, n_r, n_s)
        ref = case.ref
        dr, ds = _payload(n_r, 41, dev), _payload(n_s, 43, dev)
        tag = (shape, n_r, n_s, kind)
        j = _engine(C, dev, ctx, case, kind=kind, materialize=True)
        for _ in range(2):
            if kind == "INNER":
                res, rows = j.join_materialized(ctx, dr, OFF, n_r, ds, OFF, n_s)
            else:
                res, rows = j.join_rows(ctx, dr, OFF, n_r, ds, OFF, n_s)
            assert res["global_matches"] == rows.shape[0], tag
            if kind == "SEMI":
                assert rows.shape[1] == 5, tag
                _check_rids(rows[:, 0], ref.rids["SEMI"])
                _check_payload_words(rows, 0, 1, ds)
            else:
                assert rows.shape[1] == 10, tag
                _check_pairs(rows[:, :2].contiguous(), ref.pairs if kind == "INNER" else ref.outer_rows(kind), ref)
                _check_payload_words(rows, 0, 2, dr)
                _check_payload_words(rows, 1, 6, ds)
        if (n_r, n_s) == (65, 63) and kind == "SEMI":  # the ops entry points themselves, once
            R, S = case.on(dev)
            rows = ops.semi_join_rows(R, S, ds, OFF, _cfg(C))
            _check_rids(rows[:, 0], ref.rids["SEMI"])
            _check_payload_words(rows, 0, 1, ds)
        if (n_r, n_s) == (65, 63) and kind == "FULL_OUTER":
            R, S = case.on(dev)
            rows = ops.full_outer_join_rows(R, S, dr, ds, OFF, _cfg(C))
            _check_pairs(rows[:, :2].contiguous(), ref.outer_rows("FULL_OUTER"), ref)
            _check_payload_words(rows, 0, 2, dr)
            _check_payload_words(rows, 1, 6, ds)


@pytest.mark.gpu
def test_sizes_plan_coverage(C, cuda):
    """Over the pairs with both sides >= 63, the device took each plan at least once: the matrix does not quietly
    run one plan many times.  Reads what the matrix functions above recorded; one that has not run in this session
    is run here over those pairs."""
    dev = "cuda"

    def ensure(key, fn):
        if key not in DONE:
            fn(BIG)

    for shape in ("mixed", "one"):
        for what in ("count", "pairs"):
            for config in INNER_CONFIGS:
                ensure(("inner", shape, what, config), lambda pairs: _matrix_inner(C, dev, shape, what, config, pairs))
    ensure(("sparse",), lambda pairs: _matrix_sparse(C, dev, pairs))
    ensure(("unique",), lambda pairs: _matrix_unique(C, dev, pairs))
    ensure(("semi", "mixed"), lambda pairs: _matrix_semi_anti(C, dev, "mixed", pairs))
    need = ["bitmap", "packed", "bitmap_set", "fragments", "key_only", "wide", "split_local", "single_level",
            "key_columns"]
    assert all(n in TAKEN for n in need), ([n for n in need if n not in TAKEN], TAKEN)


# ------------------------------------------------- B. size matrix across ranks
RANK_SIZES = [(3, 3), (1, 5000), (5000, 1), (37, 5000), (1000, 0), (0, 1000)]
N_RANKS = 4


@functools.lru_cache(maxsize=None)
def _rank_case(G_R, G_S):
    g = torch.Generator().manual_seed(31 * G_R + G_S)
    D = max(1, G_R // 2)
    return Case(torch.randint(0, D, (G_R,), generator=g), torch.randint(D // 2, D // 2 + 2 * D, (G_S,), generator=g))


def _run_ranks(C, dev, case, fields, fetch):
    """One thread per rank over contiguous slices of the global relations (Relation.local_size_for); the join
    timeout is the one of the rank runners of test_outer_join / test_semi_join."""
    G_R, G_S = case.ref.n_r, case.ref.n_s
    group = C.InProcessGroup(N_RANKS)
    results, errors = [None] * N_RANKS, []
    Rd, Sd = case.on(dev)

    def rank_main(r):
        try:
            ctx = _ctx(C, dev, group.communicator(r))
            parts = []
            for t, G in ((Rd, G_R), (Sd, G_S)):
                b, n = C.Relation.local_offset_for(G, r, N_RANKS), C.Relation.local_size_for(G, r, N_RANKS)
                parts.append(C.Relation.from_tensor(t[b:b + n].contiguous(), G))
            j = C.HashJoin(parts[0], parts[1], ctx, _cfg(C, **fields))
            res = j.run()
            res = j.run()  # repeatable
            results[r] = (res, j.plan, fetch(j), parts[0].local_size(), parts[1].local_size())
        except Exception as e:  # surface in the main thread
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(N_RANKS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in threads), "a rank is still waiting"
    assert not errors, errors
    return results




def test_rank_sizes_leave_ranks_empty(C):
    empty = 0
    for G_R, G_S in RANK_SIZES:
        sizes = [(C.Relation.local_size_for(G_R, r, N_RANKS), C.Relation.local_size_for(G_S, r, N_RANKS))
                 for r in range(N_RANKS)]
        assert sum(s[0] for s in sizes) == G_R and sum(s[1] for s in sizes) == G_S
        empty += sum(1 for s in sizes if s[0] == 0 or s[1] == 0)
    assert empty >= 12


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("name", ["RCCL", "ONE_SIDED"])
@pytest.mark.parametrize("kind", ["count", "pairs", "SEMI", "FULL_OUTER", "GROUP"])
def test_ranks_sizes(C, dev, kind, name, chunks):
    fields = dict(exchange=getattr(C.ExchangeMode, name), chunks=chunks)
    for G_R, G_S in RANK_SIZES:
        case = _rank_case(G_R, G_S)
        ref = case.ref
        tag = (G_R, G_S, kind, name, fields["chunks"])
        if kind == "count":
            out = _run_ranks(C, dev, case, dict(fields, wire_codec=C.WireCodecMode.ON), lambda j: None)
            assert all(o[0]["global_matches"] == ref.count for o in out), tag
            assert sum(o[0]["local_matches"] for o in out) == ref.count, tag
        elif kind == "pairs":
            out = _run_ranks(C, dev, case, dict(fields, materialize=True), lambda j: j.output())
            assert all(o[0]["global_matches"] == ref.count for o in out), tag
            assert all(o[2].shape[0] == o[0]["local_matches"] == o[0]["output_pairs"] for o in out), tag
            check_pair_rows(torch.cat([o[2] for o in out]), ref.pairs)
        elif kind == "SEMI":
            out = _run_ranks(C, dev, case, dict(fields, kind="SEMI", materialize=True), lambda j: j.output_rids())
            assert all(o[0]["global_matches"] == ref.rids["SEMI"].numel() for o in out), tag
            assert all(o[2].numel() == o[0]["local_matches"] == o[0]["output_rids"] for o in out), tag
            _check_rids(torch.cat([o[2] for o in out]), ref.rids["SEMI"])
        elif kind == "FULL_OUTER":
            out = _run_ranks(C, dev, case, dict(fields, kind=kind, materialize=True), lambda j: j.output())
            want = ref.outer_rows(kind)
            assert all(o[0]["global_matches"] == want.shape[0] for o in out), tag
            for i, f in enumerate(("matched_pairs", "unmatched_inner", "unmatched_outer")):
                assert sum(o[0][f] for o in out) == ref.outer_counts(kind)[i], (tag, f)
            check_pair_rows(torch.cat([o[2] for o in out]), want)
        else:
            out = _run_ranks(C, dev, case, dict(fields, kind="GROUP", materialize=True), lambda j: j.output_groups())
            assert all(o[0]["global_matches"] == G_R for o in out), tag
            assert sum(o[0]["matched_pairs"] for o in out) == ref.count, tag
            assert sum(o[0]["local_matches"] for o in out) == G_R, tag
            check_group_rows(torch.cat([o[2] for o in out]), ref.group_rows())
        assert all(o[1].number_of_nodes == N_RANKS for o in out)
        assert all(o[1].one_sided == (name == "ONE_SIDED") for o in out), tag


# ------------------------------------------------ C. keys at the width limits
NB, LB = 4, 4  # fixed radix bits: passBits = 8


@functools.lru_cache(maxsize=None)
def _width_case(kb, unique=False, extra=()):
    """3,000 random inner keys below 2^kb plus 0, 15, 2^kb - 16 and 2^kb - 1 twice (the zero fragment in partition 0,
    the all-ones fragment in the all-ones partition); outer: every second inner key, 3,000 fresh keys, both extremes.
    unique: the inner keys once each.  extra: further keys (int64 bit patterns) on both sides."""
    g = torch.Generator().manual_seed(100 + kb)
    top = (1 << kb) - 1
    rk = torch.cat([torch.randint(0, top, (3000,), generator=g), torch.tensor([0, 15, top - 15, top, top])])
    if unique:
        rk = torch.unique(rk)[torch.randperm(torch.unique(rk).numel(), generator=g)]
    ex = torch.tensor(list(extra), dtype=torch.int64)
    rk = torch.cat([rk, ex])
    sk = torch.cat([rk[::2], torch.randint(0, top, (3000,), generator=g), torch.tensor([0, top]), ex])
    case = Case(rk, sk)
    ref = case.ref
    # both extremes are matched on both sides, fresh outer keys miss, every second inner key stays alone
    assert bool(ref.inner_hit[rk == top].all()) and bool(ref.inner_hit[rk == 0].all())
    assert int(ref.partners[-2 - len(extra)]) >= 1 and int(ref.partners[-1 - len(extra)]) == (1 if unique else 2)
    assert int((~ref.inner_hit).sum()) > 1000 and int((~ref.outer_hit).sum()) > (2000 if kb > 14 else 0)
    return case


def _width_cfg(**fields):
    return dict(network_bits=NB, local_bits=LB, **fields)


def _width_kinds(C, dev, ctx, case, tag, fields, wide):
    """SEMI rids, FULL OUTER rows and GROUP rows at a limit; `wide`: the format these rid-carrying kinds must take."""
    for kind in ("SEMI", "FULL_OUTER", "GROUP"):
        if kind == "SEMI":
            j, _ = _run_rids(C, dev, ctx, case, tag + (kind,), kind, **fields)
        elif kind == "FULL_OUTER":
            j, _ = _run_outer(C, dev, ctx, case, tag + (kind,), kind, True, **fields)
        else:
            j, _ = _run_group(C, dev, ctx, case, tag + (kind,), True, **fields)
        assert j.plan.wide == wide and not j.plan.key_only, (tag, kind, j.plan)
    return j


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("levels", ["two-level", "single-level"])
def test_width_compressed_limit(C, dev, levels):
    """keyBits - networkBits <= 64 - keyShift (32) and <= 31 + localBits.  Two levels, 4 + 4 bits: 32 bits above the
    network digit at kb = 36 is the last compressed width, 37 flips.  Single level: the fragment must stay below the
    LDS empty marker 0xFFFFFFFF, so 31 bits (kb = 35, fragments up to 0x7FFFFFFF) is the last and 36 flips.  The
    flip is key_only for a count and wide for everything that carries rids (makePlan, same on host and device)."""
    OFFH = C.KeyHashing.OFF
    two = levels == "two-level"
    ctx = _ctx(C, dev)
    for kb in ((35, 36, 37) if two else (34, 35, 36)):
        flipped = kb > (36 if two else 35)
        case = _width_case(kb)
        fields = _width_cfg(two_level=two, key_hashing=OFFH)
        tag = (levels, kb)
        j, _ = _run_count(C, dev, ctx, case, tag + ("count",), case.ref.count, **fields)
        assert j.plan.key_only == flipped and not j.plan.wide and j.plan.key_bits == kb, (tag, j.plan)
        assert (j.plan.network_bits, j.plan.local_bits) == (NB, LB if two else 0) and not j.plan.key_mix
        j, _ = _run_pairs(C, dev, ctx, case, tag + ("pairs",), **fields)
        assert j.plan.wide == flipped and not j.plan.key_only, (tag, j.plan)
        if not flipped:
            assert j.plan.key_shift == 32 and j.plan.frag_shift == 32 + (LB if two else 0)
        _width_kinds(C, dev, ctx, case, tag, fields, flipped)


@pytest.mark.parametrize("dev", devices())
def test_width_split_local_limit(C, dev):
    """Split local output holds the fragment above both digits in a u16 column: kb - 8 <= 16, so 24 is the last split
    width and 25 flips to u64 words (device only: the host path has no split layout).  The all-ones key at kb = 24 is
    fragment 0xFFFF."""
    ctx = _ctx(C, dev)
    for kb in (23, 24, 25):
        case = _width_case(kb)
        split = dev == "cuda" and kb <= 24
        fields = _width_cfg(key_hashing=C.KeyHashing.OFF, bitmap_join=False)
        tag = ("split", kb)
        j, _ = _run_count(C, dev, ctx, case, tag + ("count",), case.ref.count, **fields)
        assert j.plan.split_local == split and not j.plan.key_only and not j.plan.fragments, (tag, j.plan)
        j, _ = _run_pairs(C, dev, ctx, case, tag + ("pairs",), **fields)
        assert j.plan.split_local == split and not j.plan.wide, (tag, j.plan)
        j = _width_kinds(C, dev, ctx, case, tag, fields, False)
        assert j.plan.split_local == split, (tag, j.plan)
        # the same widths with the split layout off: the u64 path at 23 and 24 bits
        off = dict(fields, split_local=False)
        j, _ = _run_count(C, dev, ctx, case, tag + ("count", "off"), case.ref.count, **off)
        assert not j.plan.split_local
        _run_pairs(C, dev, ctx, case, tag + ("pairs", "off"), **off)


@pytest.mark.parametrize("dev", devices())
def test_width_key_only_split_limit(C, dev):
    """Key-only words split into u32 + u16 while the fragment above both digits has at most 48 bits: kb = 56 is the
    last, 57 flips.  These keys are sparse by construction (3,005 keys below 2^55 and up)."""
    ctx = _ctx(C, dev)
    for kb in (55, 56, 57):
        case = _width_case(kb)
        fields = _width_cfg(key_hashing=C.KeyHashing.OFF)
        tag = ("key-only split", kb)
        j, _ = _run_count(C, dev, ctx, case, tag + ("count",), case.ref.count, **fields)
        assert j.plan.key_only and j.plan.key_bits == kb, (tag, j.plan)
        assert j.plan.split_local == (dev == "cuda" and kb <= 56), (tag, j.plan)
        j, _ = _run_pairs(C, dev, ctx, case, tag + ("pairs",), **fields)
        assert j.plan.wide and not j.plan.split_local, (tag, j.plan)


@pytest.mark.parametrize("dev", devices())
def test_width_direct_count_limit(C, dev):
    """The count-only build/probe addresses an LDS count array by the fragment while it has at most 13 bits
    (BP_DIRECT_MAX_BITS): kb - 8 <= 13, so 21 is the last direct width and 22 hashes.  No plan flag shows the
    choice; direct_count on and off must agree with the oracle on both sides of it."""
    ctx = _ctx(C, dev)
    for kb in (20, 21, 22):
        case = _width_case(kb)
        counts = []
        for direct in (True, False):
            fields = _width_cfg(key_hashing=C.KeyHashing.OFF, bitmap_join=False, direct_count=direct)
            tag = ("direct", kb, direct)
            j, res = _run_count(C, dev, ctx, case, tag + ("count",), case.ref.count, **fields)
            assert j.plan.split_local == (dev == "cuda")
            counts.append(res["global_matches"])
            _run_group(C, dev, ctx, case, tag + ("group",), False, **fields)  # bpGroup has the same direct path
            _run_pairs(C, dev, ctx, case, tag + ("pairs",), **fields)
        assert counts[0] == counts[1] == case.ref.count


@pytest.mark.parametrize("dev", devices())
def test_width_bitmap_limit(C, dev):
    """Unique inner keys, sampled network pass, 4 network bits: the bitmap holds kb - 4 fragment bits, up to 21 (two
    2^20-bit pieces), so kb = 23, 24, 25 take the bitmap plan with 19, 20, 21 bits and 26 does not.  Packed
    fragments hold 20 bits: ON is taken up to kb = 24 and refused from 25.  At kb = 26 the u32-fragment two-level
    plan needs kb <= 4 + 4 + 16 as well, so the plan is the plain two-level one (compressed words).  The host engine
    takes the bitmap plan only under replicate_bitmap = ON, run here as well."""
    S, ON, OFFC = C.HistogramMode.SAMPLED, C.PlanChoice.ON, C.PlanChoice.OFF
    ctx = _ctx(C, dev)
    for kb in (23, 24, 25, 26):
        case = _width_case(kb, unique=True)
        fits = kb - NB <= 21
        for columns in (False, True):
            base = _width_cfg(key_hashing=C.KeyHashing.OFF, network_histogram=S)
            tag = ("bitmap", kb, "columns" if columns else "tuples")
            j, res = _run_count(C, dev, ctx, case, tag + ("u32",), case.ref.count, columns, packed_fragments=OFFC, **base)
            if dev == "cuda":
                assert j.plan.bitmap_join == res["bitmap_join"] == fits and not j.plan.packed_fragments, (tag, j.plan)
                # (plan.fragments describes the two-level plan a bitmap join would fall back to: kb <= 24 only)
                assert j.plan.bitmap_bits == (kb - NB if fits else 0) and j.plan.fragments == (kb <= 24), (tag, j.plan)
                assert res["key_columns"] == (("native", "native") if columns and fits else
                                              ("expanded", "expanded") if columns else ("tuples", "tuples")), tag
            j, res = _count_or_packed_refusal(C, dev, ctx, case, tag + ("packed",), columns,
                                              dict(base, packed_fragments=ON))
            if dev == "cuda":
                assert j.plan.packed_fragments == (kb - NB <= 20) and j.plan.bitmap_join == fits, (tag, j.plan)
            j, res = _run_count(C, dev, ctx, case, tag + ("replicated",), case.ref.count, columns,
                                replicate_bitmap=ON, **base)
            assert j.plan.bitmap_join == res["bitmap_join"] == fits, (tag, j.plan)
        _run_pairs(C, dev, ctx, case, ("bitmap", kb, "pairs"), **base)


@pytest.mark.parametrize("dev", devices())
def test_width_wide_limit(C, dev):
    """63-bit keys with 2^63 - 1 (the all-ones key of kb = 63) planted, next to 2^64 - 2 (int64 -2) on both sides:
    the wide format carries whole keys and reserves only 2^64 - 1 as its empty slot, which is refused when the plan
    is made.  The oracle sorts and compares the keys as signed int64 on both sides alike, so -2 matches only -2."""
    ctx = _ctx(C, dev)
    case = _width_case(63, extra=(-2,))
    top = 2**63 - 1
    assert int((case.R[:, 0] == -2).sum()) == 1 and int((case.R[:, 0] == top).sum()) == 2
    assert int(case.ref.partners[-1]) == 1 and int(case.S[-1, 0]) == -2  # 2^64 - 2 has exactly its one partner
    assert int(case.ref.partners[case.S[:, 0] == top].min()) == 2
    fields = _width_cfg(key_hashing=C.KeyHashing.OFF)
    j, _ = _run_pairs(C, dev, ctx, case, ("wide", "pairs"), **fields)
    assert j.plan.wide and j.plan.key_bits == 64, j.plan
    j, _ = _run_pairs(C, dev, ctx, case, ("wide", "pairs", "asked"), format=C.TupleFormat.WIDE, **fields)
    assert j.plan.wide
    j, _ = _run_count(C, dev, ctx, case, ("wide", "count"), case.ref.count, **fields)
    assert j.plan.key_only and not j.plan.wide and j.plan.key_bits == 64, j.plan
    _width_kinds(C, dev, ctx, case, ("wide",), fields, True)
    reserved = Case(torch.cat([case.R[:, 0], torch.tensor([-1])]), case.S[:, 0])
    for extra in (dict(materialize=True), dict(format=C.TupleFormat.WIDE), dict(kind="SEMI", materialize=True)):
        with pytest.raises(RuntimeError, match="wide format reserves key 0xFFFFFFFFFFFFFFFF"):
            _engine(C, dev, ctx, reserved, **extra, **fields)


@pytest.mark.parametrize("dev", devices())
def test_width_rid_limit(C, dev):
    """A rid of 2^32 - 1 still fits the 32-bit rid field of a CompressedTuple (key_shift 32, split output on the
    device); 2^32 moves key_shift to 33 and turns the split output (u32 rid column) off."""
    ctx = _ctx(C, dev)
    base = _width_case(20)
    for top_rid in (2**32 - 1, 2**32):
        R, S = base.R.clone(), base.S.clone()
        R[-1, 1] = top_rid  # the second copy of the all-ones key
        S[-1, 1] = top_rid  # the outer all-ones key
        case = Case(None, None, tuples=(R, S))
        assert int((case.ref.pairs == top_rid).sum()) >= 3
        fields = _width_cfg(key_hashing=C.KeyHashing.OFF)
        tag = ("rid", top_rid)
        j, _ = _run_pairs(C, dev, ctx, case, tag + ("pairs",), **fields)
        assert not j.plan.wide and j.plan.key_shift == (32 if top_rid < 2**32 else 33), (tag, j.plan)
        assert j.plan.split_local == (dev == "cuda" and top_rid < 2**32), (tag, j.plan)
        j, _ = _run_count(C, dev, ctx, case, tag + ("count",), case.ref.count, bitmap_join=False, **fields)
        assert j.plan.key_shift == (32 if top_rid < 2**32 else 33)
        _run_rids(C, dev, ctx, case, tag, "SEMI", **fields)
        _run_outer(C, dev, ctx, case, tag, "FULL_OUTER", True, **fields)


# ------------------------------------------------------ D. small kernel edges
@pytest.mark.gpu
def test_scan_u32_edges(C, cuda):
    """Exclusive scan and total, mod 2^32, around one block (256), one tile (2048) and 256 / 257 block sums."""
    g = torch.Generator().manual_seed(3)
    cases = [(n, torch.randint(0, 2**32, (n,), generator=g)) for n in
             (0, 1, 255, 256, 257, 2047, 2048, 2049, 524_288, 524_289)]
    cases.append((1, torch.tensor([2**32 - 1])))
    big = torch.randint(0, 2**32, (2049,), generator=g)
    big[-1] = 2**32 - 1
    cases.append((2049, big))
    for n, v in cases:
        got = C.ops.scan_u32(v.to(torch.int32).cuda()).cpu().to(torch.int64) & 0xFFFFFFFF  # int32 view of the u32 words
        want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(v, 0)]) & 0xFFFFFFFF
        assert got.shape == (n + 1,) and torch.equal(got, want), n


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_kernels_on_sixteen_partitions(C, dev, wide):
    """build_probe_marks / _outer / _group_agg over 16 final partitions of which 15 are empty on both sides and one
    holds a single tuple per side -- once with equal keys (a pair), once with different keys of the same partition."""
    from hpcjoin import ops
    from test_group_join import _partitioned
    b1, b2 = 3, 1
    for r_key, s_key in ((0x2D, 0x2D), (0x2D, 0x3D)):  # same low 4 bits: the same final partition
        R = torch.tensor([[r_key, 0]], dtype=torch.int64).to(dev)
        S = torch.tensor([[s_key, 0]], dtype=torch.int64).to(dev)
        hit = r_key == s_key
        rv, rpb = _partitioned(ops, R, b1, b2, wide)
        sv, spb = _partitioned(ops, S, b1, b2, wide)
        sizes_r, sizes_s = (rpb[1:] - rpb[:-1]).cpu(), (spb[1:] - spb[:-1]).cpu()
        assert sizes_r.numel() == 16 and int(sizes_r.sum()) == 1 and torch.equal(sizes_r, sizes_s)
        shifts = (64 if wide else 32 + b2, 64 if wide else 32)
        res = ops.build_probe_marks(rv, sv, rpb, spb, *shifts, wide=wide, r_chunk=512, s_chunk=1024)
        assert res["marks"].cpu().tolist() == [hit] and (res["semi_count"], res["anti_count"]) == (int(hit), int(not hit))
        assert res["semi_rids"].cpu().tolist() == ([0] if hit else []) and res["anti_rids"].cpu().tolist() == ([] if hit else [0])
        for kind in OUTER_KINDS:
            keep_r, keep_s = KEEP[kind]
            res = ops.build_probe_outer(rv, sv, rpb, spb, *shifts, wide=wide, r_chunk=512, s_chunk=1024,
                                        keep_inner=keep_r, keep_outer=keep_s)
            want = [[0, 0]] if hit else [[0, NULL]] * keep_r + [[NULL, 0]] * keep_s
            assert (res["matched_pairs"], res["unmatched_inner"], res["unmatched_outer"]) == (
                int(hit), int(keep_r and not hit), int(keep_s and not hit)), (kind, res)
            check_pair_rows(res["pairs"], _sorted_rows(torch.tensor(want, dtype=torch.int64).reshape(-1, 2)))
        f64 = torch.tensor([-2.625], dtype=torch.float64).to(dev)
        i64 = torch.tensor([-7], dtype=torch.int64).to(dev)
        res = ops.build_probe_group_agg(rv, sv, rpb, spb, *shifts, wide=wide, r_chunk=512, s_chunk=1024,
                                        columns=[i64, f64], aggs=["sum", "min"], rid_offset=0)
        want = [[0, 1, -7, _bits(-2.625)]] if hit else [[0, 0, 0, INF_BITS]]
        assert (res["matched_pairs"], res["unmatched_inner"]) == (int(hit), int(not hit))
        check_group_rows(res["rows"].cpu(), torch.tensor(want, dtype=torch.int64))
