"""Group joins with aggregates (JoinKind.GROUP, ``join_group_agg``): per inner
tuple the count of the outer tuples with its key and, over C = 1 ... 4 outer
value columns, each column's int64 SUM (wrapping), signed MIN or signed MAX --
one row ``(rid, count, agg_0, ..., agg_{C-1})`` per inner tuple, also for tuples
without a partner (count 0, each aggregate's identity: 0, INT64_MAX, INT64_MIN).

Every comparison is exact.  The oracle is plain torch on CPU copies of the
inputs: the pair list of ``test_group_join.Oracle.sums`` (outer keys sorted,
``searchsorted`` of the inner keys), then ``index_add_`` for sums and
``torch.full(identity).scatter_reduce_(..., "amin" / "amax", include_self=True)``
for minima and maxima.  Rows are compared sorted by rid, and no rid may repeat.

Every case first asserts, on the oracle alone: >= 5 % of the inner tuples have
count 0; >= 5 % have count >= 2 with min != max and a sum different from both;
>= 20 % share their key with another inner tuple; >= 5 % have min < 0 < max (an
unsigned compare fails).
"""
import functools
import threading

import pytest
import torch

from conftest import devices
from test_group_join import _case, _check_rows, _ctx, _hot_input, _loc, _partitioned, _rid_by_position

I64_MAX, I64_MIN = 2**63 - 1, -2**63
IDENTITY = {"sum": 0, "min": I64_MAX, "max": I64_MIN}


# ---------------------------------------------------------------------- oracle
class AggOracle:
    """Counts and aggregates per inner tuple (by input position of R), on CPU copies of the (key, rid) tensors."""

    def __init__(self, R, S, rid_offset=0):
        R, S = R.cpu(), S.cpu()
        rk = R[:, 0].contiguous()
        sk, order = torch.sort(S[:, 0])
        lo = torch.searchsorted(sk, rk, right=False)
        self.counts = torch.searchsorted(sk, rk, right=True) - lo
        self.rids = R[:, 1]
        self.n_r, self.n_s = R.shape[0], S.shape[0]
        self.matched_pairs = int(self.counts.sum())
        self.unmatched_inner = int((self.counts == 0).sum())
        # the pair list (inner position, outer rid - offset), as test_group_join.Oracle.sums
        cnt, total = self.counts, self.matched_pairs
        first = torch.cumsum(cnt, 0) - cnt
        within = torch.arange(total) - torch.repeat_interleave(first, cnt)
        self.r_pos = torch.repeat_interleave(torch.arange(self.n_r), cnt)
        self.s_row = S[:, 1][order[torch.repeat_interleave(lo, cnt) + within]] - rid_offset
        _, inv, copies = torch.unique(rk, return_inverse=True, return_counts=True)
        self.shared = int((copies[inv] > 1).sum())  # inner tuples whose key another inner tuple has
        self._aggs = {}
        assert self.rids.numel() == torch.unique(self.rids).numel()

    def agg(self, values, how):
        """values: the column by outer rid - offset (any device / stride; read through a CPU copy)."""
        key = (id(values), how)
        if key not in self._aggs:
            vals = values.cpu()[self.s_row]
            if how == "sum":
                out = torch.zeros(self.n_r, dtype=torch.int64).index_add_(0, self.r_pos, vals)  # wraps
            else:
                out = torch.full((self.n_r,), IDENTITY[how], dtype=torch.int64).scatter_reduce_(
                    0, self.r_pos, vals, "amin" if how == "min" else "amax", include_self=True)
            self._aggs[key] = (values, out)  # (keeps `values` alive: the key is its id)
        return self._aggs[key][1]

    def guard(self, values):
        """The guards of the module docstring, with the aggregates of one column."""
        s, lo, hi = (self.agg(values, h) for h in ("sum", "min", "max"))
        rich = (self.counts >= 2) & (lo != hi) & (s != lo) & (s != hi)
        signs = (self.counts > 0) & (lo < 0) & (hi > 0)
        fig = (self.unmatched_inner, int(rich.sum()), self.shared, int(signs.sum()), self.n_r)
        assert self.unmatched_inner >= 0.05 * self.n_r, fig
        assert int(rich.sum()) >= 0.05 * self.n_r, fig
        assert self.shared >= 0.20 * self.n_r, fig
        assert int(signs.sum()) >= 0.05 * self.n_r, fig
        empty = self.counts == 0  # the oracle itself: empty groups carry the identities
        assert bool((lo[empty] == I64_MAX).all()) and bool((hi[empty] == I64_MIN).all()) and bool((s[empty] == 0).all())
        return self

    def rows(self, columns, aggs):
        cols = [self.rids, self.counts] + [self.agg(v, h) for v, h in zip(columns, aggs)]
        rows = torch.stack(cols, 1)
        return rows[torch.sort(rows[:, 0]).indices]


def _check_result(res, oracle, n_cols):
    assert (res["matched_pairs"], res["unmatched_inner"], res["unmatched_outer"]) == (
        oracle.matched_pairs, oracle.unmatched_inner, 0), res
    assert res["local_matches"] == res["global_matches"] == res["output_groups"] == oracle.n_r
    assert res["output_pairs"] == 0 and res["output_rids"] == 0
    assert res["group_columns"] == n_cols


# ------------------------------------------------------------------ 1. kernels
def _check_agg_kernels(oracle, R, S, b1, b2, wide, cases, r_chunk=512, s_chunk=1024):
    """cases: [(columns, aggs)]; rows and the raw accumulators by position.  Rids are input positions (arange)."""
    from hpcjoin import ops
    rv, rpb = _partitioned(ops, R, b1, b2, wide)
    sv, spb = _partitioned(ops, S, b1, b2, wide)
    rid_at = _rid_by_position(rv, wide).cpu()
    for columns, aggs in cases:
        res = ops.build_probe_group_agg(rv, sv, rpb, spb, 64 if wide else 32 + b2, 64 if wide else 32, wide=wide,
                                        r_chunk=r_chunk, s_chunk=s_chunk, columns=columns, aggs=aggs, rid_offset=0)
        assert (res["matched_pairs"], res["unmatched_inner"]) == (oracle.matched_pairs, oracle.unmatched_inner)
        assert res["rows"].shape == (oracle.n_r, 2 + len(columns))
        _check_rows(res["rows"].cpu(), oracle.rows(columns, aggs))
        assert torch.equal(res["counts"].cpu(), oracle.counts[rid_at])
        got = res["aggs"].cpu()
        assert got.shape == (len(columns), oracle.n_r)
        for c, (v, how) in enumerate(zip(columns, aggs)):
            assert torch.equal(got[c], oracle.agg(v, how)[rid_at]), (c, how)
    return rpb, spb


@functools.lru_cache(maxsize=None)
def _hot_agg_input(dev):
    """The 60,000 x 200,000 hot-key input of test_group_join with three value columns uniform in +-2^40, a column
    of ties and a column over the whole int64 range with both extremes planted on matched outer tuples."""
    R, S, values, full, _ = _hot_input(dev)
    g = torch.Generator().manual_seed(77)
    n_s = S.shape[0]
    b = torch.randint(-2**40, 2**40, (n_s,), generator=g).to(dev)
    c = torch.randint(-2**40, 2**40, (n_s,), generator=g).to(dev)
    ties = torch.randint(-3, 4, (n_s,), generator=g).to(dev)
    oracle = AggOracle(R, S).guard(values)
    for v in (b, c, ties, full):
        oracle.guard(v)
    hot = R[:, 0].cpu() == 20_011
    assert int(hot.sum()) == 2 and bool((oracle.counts[hot] == 20_006).all())
    # both extremes on outer tuples that have a partner (one of them the hot key's), then the oracle of that column
    extremes = full.clone()
    matched = torch.unique(oracle.s_row)
    assert matched.numel() > 1000
    hot_rows = torch.nonzero(S[:, 0].cpu() == 20_011).flatten()
    assert int(matched[-9]) >= 20_000  # (the first 20,000 outer rows are the hot key's)
    extremes[matched[-9]] = I64_MIN
    extremes[matched[-7]] = I64_MAX
    extremes[hot_rows[3]] = I64_MAX
    extremes[hot_rows[5]] = I64_MIN
    oracle.guard(extremes)
    assert int((oracle.agg(extremes, "min") == I64_MIN).sum()) >= 3 and int((oracle.agg(extremes, "max") == I64_MAX).sum()) >= 3
    return R, S, (values, b, c), ties, extremes, oracle


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_build_probe_group_agg(C, dev, wide):
    """8 final partitions, r_chunk = 512 and s_chunk = 1024: every inner tuple is combined from many items through the
    global atomics and the hot key's LDS slot takes 20,006 updates; partition sizes off the 64-lane rows, so every
    row width from 3 to 6 words is emitted on ragged units."""
    R, S, (a, b, c), _, _, oracle = _hot_agg_input(dev)
    cases = [([a, b, c], ["sum", "min", "max"]),
             ([a, b, c, b], ["min", "max", "sum", "sum"]),
             ([b], ["max"]),
             ([a, a], ["sum", "min"])]
    rpb, spb = _check_agg_kernels(oracle, R, S, 2, 1, wide, cases)
    r_sizes, s_sizes = rpb[1:] - rpb[:-1], spb[1:] - spb[:-1]
    assert rpb.numel() == 9 and int((r_sizes % 64 != 0).sum()) > 0 and int(r_sizes.min()) > 4 * 512
    assert int(s_sizes.min()) > 20 * 1024 and int(s_sizes.max()) > 40 * 1024


# -------------------------------------------------------- 2. extremes and ties
@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_build_probe_group_agg_extremes_and_ties(C, dev, wide):
    """Values from {-3 ... 3} (many ties), and the whole int64 range with INT64_MIN and INT64_MAX on matched outer
    tuples: signed compares, and sums that wrap as index_add_ does."""
    R, S, _, ties, extremes, oracle = _hot_agg_input(dev)
    hot = R[:, 0].cpu() == 20_011
    exact = sum(int(v) for v in extremes.cpu()[S[:, 0].cpu() == 20_011].tolist())
    assert abs(exact) >= 2**63  # the hot key's true sum does not fit int64
    assert int(oracle.agg(extremes, "sum")[hot][0]) == (exact + 2**63) % 2**64 - 2**63
    assert int(oracle.agg(extremes, "min")[hot][0]) == I64_MIN and int(oracle.agg(extremes, "max")[hot][0]) == I64_MAX
    assert int(oracle.agg(ties, "min")[hot][0]) == -3 and int(oracle.agg(ties, "max")[hot][0]) == 3
    cases = [([ties, ties, extremes, extremes], ["min", "max", "min", "max"]),
             ([extremes, ties, ties], ["sum", "sum", "max"]),
             ([extremes], ["min"])]
    _check_agg_kernels(oracle, R, S, 2, 1, wide, cases)


# -------------------------------------------------------------- 3. empty sides
@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_build_probe_group_agg_empty_sides(C, dev, wide):
    """The 16-partition input of test_build_probe_group_empty_sides: tuples of inner-only partitions get no work
    item, and still carry MIN = INT64_MAX and MAX = INT64_MIN (a zeroed accumulator would not)."""
    g = torch.Generator().manual_seed(5)
    n_r, n_s, D = 20_000, 60_000, 1_000
    r_digits, s_digits = torch.tensor([0, 1, 2, 5]), torch.tensor([0, 1, 2, 3, 4, 6])
    rk = torch.randint(0, D, (n_r,), generator=g) * 8 + r_digits[torch.randint(0, 4, (n_r,), generator=g)]
    sk = torch.randint(0, 2 * D, (n_s,), generator=g) * 8 + s_digits[torch.randint(0, 6, (n_s,), generator=g)]
    a = torch.randint(-2**40, 2**40, (n_s,), generator=g).to(dev)
    b = torch.randint(-2**40, 2**40, (n_s,), generator=g).to(dev)
    R = torch.stack([rk, torch.arange(n_r)], 1).contiguous().to(dev)
    S = torch.stack([sk, torch.arange(n_s)], 1).contiguous().to(dev)
    oracle = AggOracle(R, S).guard(a)
    oracle.guard(b)
    cases = [([a, b, a], ["min", "max", "sum"]), ([b, a], ["max", "min"]), ([a], ["min"])]
    rpb, spb = _check_agg_kernels(oracle, R, S, 3, 1, wide, cases)
    r_sizes, s_sizes = (rpb[1:] - rpb[:-1]).cpu(), (spb[1:] - spb[:-1]).cpu()
    assert r_sizes.numel() == 16 and int(((r_sizes > 0) & (s_sizes == 0)).sum()) >= 2
    inner_only = (R[:, 0].cpu() % 8) == 5  # digit 5: no outer tuple at all
    assert int(inner_only.sum()) > 0.05 * n_r and bool((oracle.counts[inner_only] == 0).all())
    assert bool((oracle.agg(a, "min")[inner_only] == I64_MAX).all()) and bool((oracle.agg(b, "max")[inner_only] == I64_MIN).all())


# ------------------------------------------------------------- 4. engine, N = 1
class AggCase:
    """The generated relations of test_group_join._case with three value columns and their CPU oracle."""

    def __init__(self, C, loc, G_R, G_S, outer_dist, sparse):
        base = _case(C, loc, G_R, G_S, outer_dist, sparse)
        self.R, self.S, self.inner, self.outer = base.R, base.S, base.inner, base.outer
        Rt, St = self.R.to_tensor(), self.S.to_tensor()
        g = torch.Generator().manual_seed(19)
        self.cols = [torch.randint(-2**40, 2**40, (G_S,), generator=g).to(Rt.device) for _ in range(3)]
        self.oracle = AggOracle(Rt, St)
        for v in self.cols:
            self.oracle.guard(v)


@functools.lru_cache(maxsize=None)
def _agg_case(C, loc, G_R, G_S, outer_dist="ZIPF", sparse=False):
    return AggCase(C, loc, G_R, G_S, outer_dist, sparse)


def _group_cfg(C, group_columns, **kw):
    cfg = C.JoinConfig()
    cfg.kind = C.JoinKind.GROUP
    cfg.materialize = True
    cfg.group_columns = group_columns
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _run_agg(C, case, loc, cfg, columns, aggs, runs=2):
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, cfg)
    assert j.plan.kind == C.JoinKind.GROUP and j.plan.group_columns == cfg.group_columns
    assert not j.plan.bitmap_join and not j.plan.key_only and not j.plan.fragments and not j.plan.pipeline_outer
    want = case.oracle.rows(columns, aggs)
    for _ in range(runs):  # the identity fill is repeated: a second run on the same object gives the same answer
        res, rows = j.join_group_agg(ctx, columns, aggs, 0, columns[0].shape[0])
        _check_result(res, case.oracle, len(columns))
        _check_rows(rows, want)
        out = j.output_groups()
        assert out.shape[1] == 2 + len(columns)
        _check_rows(out, want)
    return j, res


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("fmt", ["COMPRESSED", "WIDE"])
@pytest.mark.parametrize("outer_dist", ["ZIPF", "UNIFORM"])
def test_engine_single_rank(C, dev, outer_dist, fmt):
    loc = _loc(dev)
    case = _agg_case(C, loc, 150_000, 400_000, outer_dist)
    for r_chunk in (0, 512):  # 512: several inner chunks per final partition
        cfg = _group_cfg(C, 3, format=getattr(C.TupleFormat, fmt), r_chunk=r_chunk)
        j, res = _run_agg(C, case, loc, cfg, case.cols, ["sum", "min", "max"])
        assert res["group_columns"] == 3 and j.output_groups().shape[1] == 5
        assert j.plan.wide == (fmt == "WIDE") and j.plan.r_chunk == (512 if r_chunk else 1024)
        if r_chunk and dev == "cuda":
            assert res["build_probe_items"] > (1 << (j.plan.network_bits + j.plan.local_bits))


# ---------------------------------------------------------------------- 5. plan
def test_plan_sizes_the_table_with_the_columns(C):
    """The automatic rChunk is the largest power of two whose table with group_columns accumulators per slot fits
    80 KiB (two workgroups per CU); the default of one column gives the plans of a join without the field."""
    case = _case(C, "host", 150_000, 400_000)
    want = {"COMPRESSED": {1: 2048, 2: 1024, 3: 1024, 4: 512}, "WIDE": {1: 1024, 2: 1024, 3: 1024, 4: 512}}
    for fmt, key_bytes in (("COMPRESSED", 4), ("WIDE", 8)):
        for gc in (1, 2, 3, 4):
            cfg = _group_cfg(C, gc, format=getattr(C.TupleFormat, fmt))
            p = C.HashJoin(case.R, case.S, _ctx(C, "host"), cfg).plan
            slots = 1 << max(6, (2 * p.r_chunk - 1).bit_length())
            entry = key_bytes + 4 + 8 * gc
            assert p.r_chunk == want[fmt][gc] and p.group_columns == gc, (fmt, gc, p.r_chunk)
            assert slots * entry + 64 <= 80 * 1024 and 2 * slots * entry + 64 > 80 * 1024, (fmt, gc, slots)
        cfg = C.JoinConfig()  # group_columns untouched
        cfg.kind = C.JoinKind.GROUP
        cfg.format = getattr(C.TupleFormat, fmt)
        p = C.HashJoin(case.R, case.S, _ctx(C, "host"), cfg).plan
        assert cfg.group_columns == 1 and p.group_columns == 1 and p.r_chunk == (2048 if fmt == "COMPRESSED" else 1024)
        explicit = _group_cfg(C, 4, format=getattr(C.TupleFormat, fmt), r_chunk=777)  # taken as given
        assert C.HashJoin(case.R, case.S, _ctx(C, "host"), explicit).plan.r_chunk == 777


# ------------------------------------------- 6. strided views and the rid offset
@pytest.mark.parametrize("dev", devices())
def test_columns_as_strided_views(C, dev):
    """Columns 1, 2, 3 of an [n, 4] payload tensor (element stride 4, read in place), rids from 1,000,003, and a
    fourth column from a separate contiguous tensor: the result of the contiguous copies."""
    from hpcjoin import ops
    OFF, n_r, n_s = 1_000_003, 30_000, 70_000
    g = torch.Generator().manual_seed(31)
    R = torch.stack([torch.randint(0, n_r // 2, (n_r,), generator=g), torch.arange(n_r) + OFF], 1).contiguous().to(dev)
    S = torch.stack([torch.randint(n_r // 4, n_r + n_r // 4, (n_s,), generator=g), torch.arange(n_s) + OFF],
                    1).contiguous().to(dev)
    payload = C.ops.generate_payload(n_s, OFF, 77, dev)
    views = [payload[:, 1], payload[:, 2], payload[:, 3]]
    other = torch.randint(-2**40, 2**40, (n_s,), generator=g).to(dev)
    assert payload.shape == (n_s, 4) and all(v.stride(0) == 4 and not v.is_contiguous() for v in views)
    oracle = AggOracle(R, S, OFF)
    for v in views + [other]:
        oracle.guard(v)
    aggs = ["sum", "min", "max", "min"]
    a = ops.group_join_agg(R, S, views + [other], aggs, OFF)
    b = ops.group_join_agg(R, S, [v.contiguous() for v in views] + [other], aggs, OFF)
    assert a.shape == (n_r, 6)
    _check_rows(a, oracle.rows(views + [other], aggs))
    assert torch.equal(a[torch.sort(a[:, 0]).indices], b[torch.sort(b[:, 0]).indices])
    assert [v.data_ptr() for v in views] == [payload.data_ptr() + 8 * k for k in (1, 2, 3)]  # never copied by the test


# ----------------------------------------- 7. split columns, sampled local pass
@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False], ids=["split", "u64"])
def test_split_and_sampled_local(C, cuda, split):
    """The sampled local pass leaves gaps between the final partitions: gap positions are never read or emitted."""
    G = 1 << 22
    case = _agg_case(C, "device", G, G + 12345)
    cfg = _group_cfg(C, 2, split_local=split, local_histogram=C.HistogramMode.SAMPLED)
    j, res = _run_agg(C, case, "device", cfg, case.cols[:2], ["min", "sum"], runs=1)
    assert j.plan.split_local == split and res["sampled_local"] and res["local_fallbacks"] == 0
    assert res["output_groups"] == G


# --------------------------------------------------------- 8. sparse 63-bit keys
@pytest.mark.parametrize("dev", devices())
def test_sparse_keys_take_wide(C, dev):
    loc = _loc(dev)
    case = _agg_case(C, loc, 150_000, 400_000, "ZIPF", True)
    j, _ = _run_agg(C, case, loc, _group_cfg(C, 3), case.cols, ["max", "sum", "min"], runs=1)
    assert j.plan.key_bits == 63 and j.plan.wide and not j.plan.key_only


# ----------------------------------------------------------------- 9. equivalence
@pytest.mark.parametrize("dev", devices())
def test_one_sum_column_is_join_group(C, dev):
    """join_group_agg(ctx, [v], ["sum"]) returns exactly the rows of join_group(ctx, v)."""
    loc = _loc(dev)
    case = _agg_case(C, loc, 150_000, 400_000)
    v = case.cols[0]
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, _group_cfg(C, 1))
    res_a, rows_a = j.join_group_agg(ctx, [v], ["SUM"], 0, v.shape[0])  # (any letter case)
    res_b, rows_b = j.join_group(ctx, v, 0, v.shape[0])
    assert rows_a.shape == (150_000, 3)  # (the row order follows the partitioning, which differs from run to run)
    assert torch.equal(rows_a[torch.sort(rows_a[:, 0]).indices], rows_b[torch.sort(rows_b[:, 0]).indices])
    assert res_a["group_columns"] == res_b["group_columns"] == 1 and j.run()["group_columns"] == 0
    _check_rows(rows_a, case.oracle.rows([v], ["sum"]))


# ------------------------------------------------------------------ 10. rejections
def test_rejections(C):
    case = _agg_case(C, "host", 150_000, 400_000)
    n_s = 400_000
    a, b, c = case.cols
    ctx = _ctx(C, "host")
    j = C.HashJoin(case.R, case.S, ctx, _group_cfg(C, 2))
    _, good = j.join_group_agg(ctx, [a, b], ["min", "max"], 0, n_s)
    want = case.oracle.rows([a, b], ["min", "max"])
    _check_rows(good, want)

    def refused(fn, *words):
        with pytest.raises(RuntimeError) as e:
            fn()
        assert "join_group_agg" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: j.join_group_agg(ctx, [a, b, c], ["sum", "min", "max"], 0, n_s), "group_columns")
    refused(lambda: j.join_group_agg(ctx, [a, b, c, a, b], ["sum"] * 5, 0, n_s), "5", "columns")
    refused(lambda: j.join_group_agg(ctx, [a, b], ["sum"], 0, n_s), "aggregates")
    refused(lambda: j.join_group_agg(ctx, [a, b], ["sum", "avg"], 0, n_s), "avg", "aggregate")
    refused(lambda: j.join_group_agg(ctx, [a, b[: n_s - 1]], ["sum", "min"], 0, n_s), "cover")
    refused(lambda: j.join_group_agg(ctx, [a[: n_s - 1]], ["sum"], 0, n_s - 1), "cover")
    _check_rows(j.output_groups(), want)  # the refusals left the last run's rows alone

    cfg = C.JoinConfig()
    cfg.materialize = True
    refused(lambda: C.HashJoin(case.R, case.S, ctx, cfg).join_group_agg(ctx, [a], ["min"], 0, n_s), "GROUP")
    cfg = C.JoinConfig()
    cfg.kind = C.JoinKind.GROUP
    cfg.passes = 2  # (count-only: a materializing spill is refused at construction)
    refused(lambda: C.HashJoin(case.R, case.S, ctx, cfg).join_group_agg(ctx, [a], ["min"], 0, n_s), "spill", "2 passes")
    with pytest.raises(RuntimeError) as e:  # the field's range
        C.HashJoin(case.R, case.S, ctx, _group_cfg(C, 5))
    assert "group_columns" in str(e.value)


def test_in_process_ranks_refuse_columns(C):
    """The values of outer tuples received from other ranks live on those ranks."""
    G_R, G_S, n_ranks = 150_000, 400_000, 2
    case = _agg_case(C, "host", G_R, G_S)
    group = C.InProcessGroup(n_ranks)
    errors = []

    def rank_main(r):
        try:
            ctx = _ctx(C, "host", group.communicator(r))
            R = C.Relation(C.Relation.local_size_for(G_R, r, n_ranks), G_R, "host", 0)
            S = C.Relation(C.Relation.local_size_for(G_S, r, n_ranks), G_S, "host", 0)
            R.generate(case.inner, C.Relation.local_offset_for(G_R, r, n_ranks))
            S.generate(case.outer, C.Relation.local_offset_for(G_S, r, n_ranks))
            j = C.HashJoin(R, S, ctx, _group_cfg(C, 2))
            j.join_group_agg(ctx, case.cols[:2], ["min", "max"], 0, G_S)
        except Exception as e:  # surface in the main thread
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert len(errors) == 2 and all("join_group_agg" in e and "single rank" in e for _, e in errors), errors


# ----------------------------------------------------------------------- 11. config
def test_config_group_columns(C, monkeypatch):
    from hpcjoin.utils import config_from_dict, config_to_dict
    assert C.JoinConfig().group_columns == 1 and config_to_dict(C.JoinConfig())["group_columns"] == 1
    cfg = config_from_dict({"kind": "group", "group_columns": 3})
    assert cfg.group_columns == 3 and config_to_dict(cfg)["group_columns"] == 3
    assert "groupColumns=3" in repr(cfg)
    case = _case(C, "host", 150_000, 400_000)
    plan = C.HashJoin(case.R, case.S, _ctx(C, "host"), cfg).plan
    assert plan.group_columns == 3 and "groupColumns=3" in repr(plan)
    monkeypatch.setenv("HPCJOIN_GROUP_COLUMNS", "4")
    assert config_from_dict({"group_columns": 2}).group_columns == 4  # the environment overrides


# ------------------------------------------------------------ 12. Python surface
@pytest.mark.parametrize("dev", devices())
def test_ops_group_join_agg(C, dev):
    from hpcjoin import ops
    n_r, n_s = 30_000, 70_000
    spec_r = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=3, domain=n_r // 2)
    spec_s = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=4, domain=n_r, key_offset=n_r // 4)
    R, S = C.ops.generate(n_r, 0, n_r, spec_r, dev), C.ops.generate(n_s, 0, n_s, spec_s, dev)
    g = torch.Generator().manual_seed(2)
    a, b = (torch.randint(-2**40, 2**40, (n_s,), generator=g).to(dev) for _ in range(2))
    oracle = AggOracle(R, S).guard(a)
    oracle.guard(b)
    rows = ops.group_join_agg(R, S, [a, b, b], ["sum", "min", "max"])
    assert rows.shape == (n_r, 5)
    _check_rows(rows, oracle.rows([a, b, b], ["sum", "min", "max"]))
    one = ops.group_join_agg(R, S, [b], ["max"])
    _check_rows(one, oracle.rows([b], ["max"]))
    _check_rows(ops.group_join_agg(R, S, [a], ["sum"]), oracle.rows([a], ["sum"]))
    _check_rows(ops.group_join_sum(R, S, a), oracle.rows([a], ["sum"]))
    assert int(rows[:, 1].sum()) == ops.join_count(R, S) == oracle.matched_pairs
