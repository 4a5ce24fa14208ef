"""Group joins with typed value columns: each of the 1 ... 4 columns of one join is
int64, int32, float64 or float32.  Integer columns accumulate as int64 (int32 is
sign-extended on load), float columns as IEEE binary64 (float32 converts exactly);
the rows stay int64 ``[n, 2 + C]`` and the word of a float column holds the bit
pattern of its aggregate.  Empty groups carry 0 / INT64_MAX / INT64_MIN, or the bits
of +0.0 / +inf / -inf.

The oracle is plain torch on CPU copies, from the pair list of ``AggOracle``:
``index_add_`` / ``scatter_reduce_`` on int64 after ``.to(int64)``, or on float64
after ``.to(float64)`` with the identities +inf / -inf.  Rows are compared sorted by
rid, float words as bit patterns.

The float inputs are exact in their dtype: ``k / 8`` with ``k`` uniform in +-2^36
(float64) or +-2^20 (float32), so every partial sum is a multiple of 1/8 below
2^53 / 8, the same in any order, and every comparison is exact equality.  The one
exception is ``test_float_sum_rounding_bound``, which derives its bound there.
"""
import functools
import threading

import pytest
import torch

from conftest import devices
from test_group_agg import AggOracle
from test_group_join import _case, _check_rows, _ctx, _hot_input, _loc, _partitioned, _rid_by_position

I64_MAX, I64_MIN = 2**63 - 1, -2**63
I32_MAX, I32_MIN = 2**31 - 1, -2**31
INF = float("inf")
IDENT = {False: {"sum": 0, "min": I64_MAX, "max": I64_MIN}, True: {"sum": 0.0, "min": INF, "max": -INF}}
WORD = {torch.int64: "int64", torch.int32: "int64", torch.float64: "float64", torch.float32: "float64"}


def _bits(x: float) -> int:
    return int(torch.tensor([x], dtype=torch.float64).view(torch.int64)[0])


# ---------------------------------------------------------------------- oracle
class TypedOracle(AggOracle):
    """AggOracle whose aggregates follow the column's dtype; a float aggregate is returned as its int64 bits."""

    def agg(self, values, how):
        key = (id(values), how)
        if key not in self._aggs:
            fl = values.dtype.is_floating_point
            vals = values.cpu().to(torch.float64 if fl else torch.int64)[self.s_row]
            out = torch.full((self.n_r,), IDENT[fl][how], dtype=vals.dtype)
            if how == "sum":
                out.index_add_(0, self.r_pos, vals)
            else:
                out.scatter_reduce_(0, self.r_pos, vals, "amin" if how == "min" else "amax", include_self=True)
            self._aggs[key] = (values, out.view(torch.int64) if fl else out)  # (keeps `values` alive: the key is its id)
        return self._aggs[key][1]

    def fagg(self, values, how):
        return self.agg(values, how).view(torch.float64)

    def per_group(self, flags):
        """Per inner tuple: how many of its pairs have the flag (flags by outer row)."""
        return torch.zeros(self.n_r, dtype=torch.int64).index_add_(0, self.r_pos, flags.cpu()[self.s_row].to(torch.int64))


def _typed_columns(n_s, seed, dev):
    """k, k32, i32 in this order from one generator: float64 k / 8, float32 k32 / 8, int32 over the whole range."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-2**36, 2**36, (n_s,), generator=g)
    k32 = torch.randint(-2**20, 2**20, (n_s,), generator=g)
    i32 = torch.randint(-2**31, 2**31, (n_s,), generator=g).to(torch.int32)
    f64, f32 = k.to(torch.float64) / 8, k32.to(torch.float32) / 8
    assert torch.equal(f32.to(torch.float64) * 8, k32.to(torch.float64))  # exact in float32
    return f64.to(dev), f32.to(dev), i32.to(dev)


def _guard(oracle, f64, f32, i32):
    """The guards of the issue, on the oracle alone (fractions of the inner tuples)."""
    n = oracle.n_r
    cnt = oracle.counts
    fig = {"empty": oracle.unmatched_inner / n}
    for name, col in (("f64", f64), ("f32", f32)):
        neg = oracle.per_group(col < 0)
        fig[name + "_two_negative"] = int((neg >= 2).sum()) / n  # an integer compare of the bits gives a wrong MIN
        fig[name + "_all_negative"] = int(((cnt >= 2) & (neg == cnt)).sum()) / n  # ... a wrong MAX
        s = oracle.fagg(col, "sum")
        fig[name + "_sum_not_integer"] = int((s != s.round()).sum()) / n
        bits_added = torch.zeros(n, dtype=torch.int64).index_add_(
            0, oracle.r_pos, col.cpu().to(torch.float64).view(torch.int64)[oracle.s_row])
        fig[name + "_integer_add_differs"] = int((bits_added != oracle.agg(col, "sum")).sum()) / n
    s32 = oracle.agg(i32, "sum")
    fig["i32_sum_outside_int32"] = int(((s32 > I32_MAX) | (s32 < I32_MIN)).sum()) / n
    assert fig["empty"] >= 0.05, fig
    for name in ("f64", "f32"):
        assert fig[name + "_two_negative"] >= 0.20, fig
        assert fig[name + "_all_negative"] >= 0.01, fig
        assert fig[name + "_sum_not_integer"] >= 0.20, fig
        assert fig[name + "_integer_add_differs"] >= 0.20, fig
    assert fig["i32_sum_outside_int32"] >= 0.10, fig
    empty = cnt == 0  # the oracle itself: empty groups carry the typed identities, bit for bit
    for col in (f64, f32):
        assert bool((oracle.agg(col, "sum")[empty] == 0).all())  # +0.0
        assert bool((oracle.agg(col, "min")[empty] == _bits(INF)).all())
        assert bool((oracle.agg(col, "max")[empty] == _bits(-INF)).all())
    assert bool((oracle.agg(i32, "min")[empty] == I64_MAX).all()) and bool((oracle.agg(i32, "max")[empty] == I64_MIN).all())
    return fig


# ------------------------------------------------------------------ 1. kernels
def _check_typed_kernels(oracle, R, S, b1, b2, wide, cases, r_chunk=512, s_chunk=1024):
    """cases: [(columns, aggs)]; rows, raw counts, raw accumulators by position and group_dtypes.  Rids are input
    positions (arange)."""
    from hpcjoin import ops
    rv, rpb = _partitioned(ops, R, b1, b2, wide)
    sv, spb = _partitioned(ops, S, b1, b2, wide)
    rid_at = _rid_by_position(rv, wide).cpu()
    for columns, aggs in cases:
        res = ops.build_probe_group_agg(rv, sv, rpb, spb, 64 if wide else 32 + b2, 64 if wide else 32, wide=wide,
                                        r_chunk=r_chunk, s_chunk=s_chunk, columns=columns, aggs=aggs, rid_offset=0)
        tag = ([str(v.dtype) for v in columns], aggs)
        assert (res["matched_pairs"], res["unmatched_inner"]) == (oracle.matched_pairs, oracle.unmatched_inner), tag
        assert list(res["group_dtypes"]) == [WORD[v.dtype] for v in columns], tag
        assert res["rows"].shape == (oracle.n_r, 2 + len(columns)) and res["rows"].dtype == torch.int64, tag
        _check_rows(res["rows"].cpu(), oracle.rows(columns, aggs))
        assert torch.equal(res["counts"].cpu(), oracle.counts[rid_at]), tag
        got = res["aggs"].cpu()
        assert got.shape == (len(columns), oracle.n_r) and got.dtype == torch.int64, tag
        for c, (v, how) in enumerate(zip(columns, aggs)):
            assert torch.equal(got[c], oracle.agg(v, how)[rid_at]), (c, how, tag)
    return rpb, spb


@functools.lru_cache(maxsize=None)
def _typed_hot_input(dev):
    """The 60,000 x 200,000 hot-key input of test_group_join (seed 21) with typed columns from seed 91."""
    R, S, i64, _, _ = _hot_input(dev)
    f64, f32, i32 = _typed_columns(S.shape[0], 91, dev)
    oracle = TypedOracle(R, S)
    _guard(oracle, f64, f32, i32)
    hot = R[:, 0].cpu() == 20_011
    assert int(hot.sum()) == 2 and bool((oracle.counts[hot] == 20_006).all())
    return R, S, (i64, i32, f64, f32), oracle


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_build_probe_group_agg_typed(C, dev, wide):
    """8 final partitions, r_chunk = 512, s_chunk = 1024: every inner tuple is combined from many items through the
    global atomics (f64 add / min / max next to the integer forms) and the hot key's LDS slot takes 20,006 updates
    per column."""
    R, S, (i64, i32, f64, f32), oracle = _typed_hot_input(dev)
    cases = [([f64, f32, i32], ["sum", "min", "max"]),
             ([i64, f64, i32, f32], ["min", "sum", "sum", "max"]),
             ([f64], ["sum"]),
             ([f32], ["max"]),
             ([i32], ["sum"]),
             ([f64, f64], ["min", "max"])]
    rpb, spb = _check_typed_kernels(oracle, R, S, 2, 1, wide, cases)
    r_sizes, s_sizes = rpb[1:] - rpb[:-1], spb[1:] - spb[:-1]
    assert rpb.numel() == 9 and int((r_sizes % 64 != 0).sum()) > 0 and int(r_sizes.min()) > 4 * 512
    assert int(s_sizes.min()) > 20 * 1024


# ----------------------------------------------------------------- 2. extremes
def _plant_rows(oracle, S, n):
    """n matched outer rows outside the hot key, each of a different key, and two rows of the hot key."""
    sk = S[:, 0].cpu()
    matched = torch.unique(oracle.s_row)
    rows, keys = [], set()
    for r in reversed(matched.tolist()):
        if r >= 20_000 and int(sk[r]) not in keys:  # (the first 20,000 outer rows are the hot key's)
            rows.append(r)
            keys.add(int(sk[r]))
        if len(rows) == n:
            break
    assert len(rows) == n and 20_011 not in keys
    hot_rows = torch.nonzero(sk == 20_011).flatten()
    return rows, (int(hot_rows[3]), int(hot_rows[5]))


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_build_probe_group_agg_typed_extremes(C, dev, wide):
    """INT32_MIN / INT32_MAX (sign extension), +-1.7e308, a float64 subnormal and +-inf, FLT_MAX and the smallest
    float32 subnormal (its conversion to binary64 is exact), each on a matched outer tuple.  The float columns are
    compared for MIN / MAX only: a sum with both infinities is NaN."""
    R, S, (_, i32, f64, f32), oracle = _typed_hot_input(dev)
    rows, (h0, h1) = _plant_rows(oracle, S, 6)
    x32 = i32.clone()
    x32[rows[0]], x32[rows[1]], x32[h0], x32[h1] = I32_MIN, I32_MAX, I32_MAX, I32_MIN
    # positive base values (>= 1), so that a planted subnormal is its group's minimum
    e64 = f64.abs() + 1
    tiny64, tiny32, flt_max = 5e-324, 2.0**-149, 3.4028234663852886e38
    for r, v in zip(rows + [h0, h1], [1.7e308, -1.7e308, tiny64, INF, -INF, 1.0, -INF, INF]):
        e64[r] = v
    e32 = f32.abs() + 1
    for r, v in zip(rows[:3] + [h0, h1], [flt_max, -flt_max, tiny32, flt_max, tiny32]):
        e32[r] = v
    assert float(e64[rows[2]]) == tiny64 and float(e64[rows[2]]) > 0 and float(e32[rows[2]]) == tiny32 > 0
    hot = R[:, 0].cpu() == 20_011
    assert oracle.agg(x32, "min")[hot].tolist() == [I32_MIN] * 2 and oracle.agg(x32, "max")[hot].tolist() == [I32_MAX] * 2
    lo64, hi64 = oracle.fagg(e64, "min"), oracle.fagg(e64, "max")
    assert lo64[hot].tolist() == [-INF] * 2 and hi64[hot].tolist() == [INF] * 2
    for v in (-1.7e308, tiny64, -INF):
        assert int((lo64 == v).sum()) >= 1, v
    for v in (1.7e308, INF):
        assert int((hi64 == v).sum()) >= 1, v
    lo32, hi32 = oracle.fagg(e32, "min"), oracle.fagg(e32, "max")
    assert lo32[hot].tolist() == [tiny32] * 2 and hi32[hot].tolist() == [flt_max] * 2
    assert int((lo32 == -flt_max).sum()) >= 1 and int((lo32 == tiny32).sum()) >= 3 and int((hi32 == flt_max).sum()) >= 3
    cases = [([e64, e64, x32, x32], ["min", "max", "min", "max"]),
             ([e32, e32, x32], ["min", "max", "sum"]),
             ([e32], ["min"])]
    _check_typed_kernels(oracle, R, S, 2, 1, wide, cases)


# -------------------------------------------------------------- 3. empty sides
@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_build_probe_group_agg_typed_empty_sides(C, dev, wide):
    """The 16-partition input of test_build_probe_group_agg_empty_sides: tuples of inner-only partitions get no work
    item, and carry +inf / -inf / +0.0 bit for bit and the integer identities for the int32 column."""
    g = torch.Generator().manual_seed(5)
    n_r, n_s, D = 20_000, 60_000, 1_000
    r_digits, s_digits = torch.tensor([0, 1, 2, 5]), torch.tensor([0, 1, 2, 3, 4, 6])
    rk = torch.randint(0, D, (n_r,), generator=g) * 8 + r_digits[torch.randint(0, 4, (n_r,), generator=g)]
    sk = torch.randint(0, 2 * D, (n_s,), generator=g) * 8 + s_digits[torch.randint(0, 6, (n_s,), generator=g)]
    R = torch.stack([rk, torch.arange(n_r)], 1).contiguous().to(dev)
    S = torch.stack([sk, torch.arange(n_s)], 1).contiguous().to(dev)
    f64, f32, i32 = _typed_columns(n_s, 92, dev)
    oracle = TypedOracle(R, S)
    inner_only = (R[:, 0].cpu() % 8) == 5  # digit 5: no outer tuple at all
    assert int(inner_only.sum()) > 0.05 * n_r and bool((oracle.counts[inner_only] == 0).all())
    assert bool((oracle.agg(f64, "min")[inner_only] == _bits(INF)).all())
    assert bool((oracle.agg(f32, "max")[inner_only] == _bits(-INF)).all())
    assert bool((oracle.agg(f64, "sum")[inner_only] == 0).all()) and _bits(0.0) == 0 and _bits(-0.0) != 0
    assert bool((oracle.agg(i32, "min")[inner_only] == I64_MAX).all()) and bool((oracle.agg(i32, "max")[inner_only] == I64_MIN).all())
    cases = [([f64, f32, i32], ["min", "max", "min"]),
             ([f32, f64, i32, f64], ["min", "max", "max", "sum"]),
             ([f32], ["sum"]),
             ([f64], ["max"])]
    rpb, spb = _check_typed_kernels(oracle, R, S, 3, 1, wide, cases)
    r_sizes, s_sizes = (rpb[1:] - rpb[:-1]).cpu(), (spb[1:] - spb[:-1]).cpu()
    assert r_sizes.numel() == 16 and int(((r_sizes > 0) & (s_sizes == 0)).sum()) >= 2


# ----------------------------------------------------------- 4. rounding bound
@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_float_sum_rounding_bound(C, dev, wide):
    """One float64 column of randn * 1e6, "sum": the sum is taken in the order the atomics land, so it is compared
    against |got - oracle| <= count * 2^-51 * sum|v| per group.  Both sums carry at most (n - 1) * 2^-53 * sum|v| of
    rounding error; the factor 4 over their sum covers the oracle's own sum|v|.  A lost or doubled update is orders
    of magnitude above that."""
    from hpcjoin import ops
    R, S, _, oracle = _typed_hot_input(dev)
    n_s = S.shape[0]
    v = (torch.randn(n_s, generator=torch.Generator().manual_seed(93), dtype=torch.float64) * 1e6).to(dev)
    want = oracle.fagg(v, "sum")
    absum = torch.zeros(oracle.n_r, dtype=torch.float64).index_add_(0, oracle.r_pos, v.cpu().abs()[oracle.s_row])
    rev = torch.zeros(oracle.n_r, dtype=torch.float64).index_add_(0, oracle.r_pos.flip(0), v.cpu()[oracle.s_row].flip(0))
    rv, rpb = _partitioned(ops, R, 2, 1, wide)
    sv, spb = _partitioned(ops, S, 2, 1, wide)
    res = ops.build_probe_group_agg(rv, sv, rpb, spb, 64 if wide else 33, 64 if wide else 32, wide=wide, r_chunk=512,
                                    s_chunk=1024, columns=[v], aggs=["sum"], rid_offset=0)
    rows = res["rows"].cpu()
    rows = rows[torch.sort(rows[:, 0]).indices]
    assert torch.equal(rows[:, 0], torch.arange(oracle.n_r)) and torch.equal(rows[:, 1], oracle.counts)
    got = ops.group_agg_values(rows, 0, v)
    assert got.dtype == torch.float64
    err, bound = (got - want).abs(), oracle.counts.to(torch.float64) * 2.0**-51 * absum
    worst = float((err / bound.clamp_min(1e-300)).max())
    differs = int((got != want).sum()) / oracle.n_r
    differs_rev = int((rev != want).sum()) / oracle.n_r
    print(f"rounding: worst err / bound = {worst:.3g}, groups != oracle {differs:.3f}, oracle != reversed {differs_rev:.3f}")
    assert bool((err <= bound).all()), worst
    assert bool((got[oracle.counts == 0].view(torch.int64) == 0).all())
    assert max(differs, differs_rev) >= 0.20, (differs, differs_rev)  # the case is not secretly exact


# ------------------------------------------------------------- 5. engine, N = 1
class TypedCase:
    """The generated relations of test_group_join._case with float64, int32 and float32 columns and their oracle."""

    def __init__(self, C, loc, G_R, G_S, outer_dist):
        base = _case(C, loc, G_R, G_S, outer_dist, False)  # (the cached relations of test_group_agg)
        self.R, self.S, self.inner, self.outer = base.R, base.S, base.inner, base.outer
        Rt, St = self.R.to_tensor(), self.S.to_tensor()
        f64, f32, i32 = _typed_columns(G_S, 94, Rt.device)
        self.cols = [f64, i32, f32]
        self.oracle = TypedOracle(Rt, St)
        assert self.oracle.unmatched_inner >= 0.05 * G_R and self.oracle.matched_pairs >= 0.05 * G_S


@functools.lru_cache(maxsize=None)
def _typed_case(C, loc, G_R, G_S, outer_dist="ZIPF"):
    return TypedCase(C, loc, G_R, G_S, outer_dist)


def _group_cfg(C, group_columns, **kw):
    cfg = C.JoinConfig()
    cfg.kind = C.JoinKind.GROUP
    cfg.materialize = True
    cfg.group_columns = group_columns
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _run_typed(C, case, loc, cfg, columns, aggs, runs=2):
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, cfg)
    want = case.oracle.rows(columns, aggs)
    for _ in range(runs):  # the identity fill is repeated: a second run on the same object gives the same answer
        res, rows = j.join_group_agg(ctx, columns, aggs, 0, columns[0].shape[0])
        assert (res["matched_pairs"], res["unmatched_inner"], res["unmatched_outer"]) == (
            case.oracle.matched_pairs, case.oracle.unmatched_inner, 0), res
        assert res["output_groups"] == case.oracle.n_r and res["group_columns"] == len(columns)
        assert list(res["group_dtypes"]) == [WORD[v.dtype] for v in columns]
        _check_rows(rows, want)
        _check_rows(j.output_groups(), want)
    return j, res


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("fmt", ["COMPRESSED", "WIDE"])
@pytest.mark.parametrize("outer_dist", ["ZIPF", "UNIFORM"])
def test_engine_single_rank_typed(C, dev, outer_dist, fmt):
    loc = _loc(dev)
    case = _typed_case(C, loc, 150_000, 400_000, outer_dist)
    for r_chunk in (0, 512):  # 512: several inner chunks per final partition
        cfg = _group_cfg(C, 3, format=getattr(C.TupleFormat, fmt), r_chunk=r_chunk)
        j, res = _run_typed(C, case, loc, cfg, case.cols, ["sum", "min", "max"])
        assert res["group_columns"] == 3 and res["group_dtypes"] == ["float64", "int64", "float64"]
        assert j.plan.wide == (fmt == "WIDE") and j.plan.r_chunk == (512 if r_chunk else 1024)


@pytest.mark.gpu
def test_split_and_sampled_local_typed(C, cuda):
    """Split columns and the sampled local pass (gaps between the final partitions) with a float64 and an int32
    column."""
    G = 1 << 22
    case = _typed_case(C, "device", G, G + 12345)
    cfg = _group_cfg(C, 2, split_local=True, local_histogram=C.HistogramMode.SAMPLED)
    j, res = _run_typed(C, case, "device", cfg, case.cols[:2], ["sum", "max"], runs=1)
    assert j.plan.split_local and res["sampled_local"] and res["local_fallbacks"] == 0
    assert res["output_groups"] == G and res["group_dtypes"] == ["float64", "int64"]


# ------------------------------------------- 6. strided views and the rid offset
@pytest.mark.parametrize("dev", devices())
def test_typed_columns_as_strided_views(C, dev):
    """Columns 1, 3, 5 of an [n, 8] int32 tensor (element stride 8, 4-byte loads in place) and columns 1, 2 of an
    [n, 4] float32 tensor, rids from 1,000,003: the result of the contiguous copies, and the oracle's."""
    from hpcjoin import ops
    OFF, n_r, n_s = 1_000_003, 30_000, 70_000
    g = torch.Generator().manual_seed(31)
    R = torch.stack([torch.randint(0, n_r // 2, (n_r,), generator=g), torch.arange(n_r) + OFF], 1).contiguous().to(dev)
    S = torch.stack([torch.randint(n_r // 4, n_r + n_r // 4, (n_s,), generator=g), torch.arange(n_s) + OFF],
                    1).contiguous().to(dev)
    rows32 = torch.randint(-2**31, 2**31, (n_s, 8), generator=g).to(torch.int32).to(dev)
    rowsf = (torch.randint(-2**20, 2**20, (n_s, 4), generator=g).to(torch.float32) / 8).to(dev)
    iv = [rows32[:, 1], rows32[:, 3], rows32[:, 5]]
    fv = [rowsf[:, 1], rowsf[:, 2]]
    assert all(v.stride(0) == 8 and not v.is_contiguous() for v in iv) and all(v.stride(0) == 4 for v in fv)
    oracle = TypedOracle(R, S, OFF)
    assert oracle.unmatched_inner >= 0.05 * n_r and oracle.matched_pairs >= 0.05 * n_s
    for columns, aggs in ((iv + [fv[0]], ["sum", "min", "max", "sum"]), (fv + [iv[2]], ["min", "max", "sum"])):
        a = ops.group_join_agg(R, S, columns, aggs, OFF)
        b = ops.group_join_agg(R, S, [v.contiguous() for v in columns], aggs, OFF)
        assert a.shape == (n_r, 2 + len(columns))
        _check_rows(a, oracle.rows(columns, aggs))
        assert torch.equal(a[torch.sort(a[:, 0]).indices], b[torch.sort(b[:, 0]).indices])
    # never copied by the test: the views still point into their tensors
    assert [v.data_ptr() for v in iv] == [rows32.data_ptr() + 4 * k for k in (1, 3, 5)]
    assert [v.data_ptr() for v in fv] == [rowsf.data_ptr() + 4 * k for k in (1, 2)]


# --------------------------------------------------------------- 7. equivalences
@pytest.mark.parametrize("dev", devices())
def test_typed_equivalences(C, dev):
    from hpcjoin import ops
    n_r, n_s = 30_000, 70_000
    spec_r = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=3, domain=n_r // 2)
    spec_s = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=4, domain=n_r, key_offset=n_r // 4)
    R, S = C.ops.generate(n_r, 0, n_r, spec_r, dev), C.ops.generate(n_s, 0, n_s, spec_s, dev)
    f64, f32, i32 = _typed_columns(n_s, 95, dev)
    oracle = TypedOracle(R, S)
    assert oracle.unmatched_inner >= 0.05 * n_r and oracle.matched_pairs >= 0.05 * n_s

    def by_rid(rows):
        return rows[torch.sort(rows[:, 0]).indices]

    # group_join_sum with a float64 column is group_join_agg with one "sum" column
    one = by_rid(ops.group_join_sum(R, S, f64))
    assert one.shape == (n_r, 3) and torch.equal(one, by_rid(ops.group_join_agg(R, S, [f64], ["sum"])))
    _check_rows(one, oracle.rows([f64], ["sum"]))
    _check_rows(ops.group_join_sum(R, S, i32), oracle.rows([i32], ["sum"]))
    _check_rows(ops.group_join_sum(R, S, f32), oracle.rows([f32], ["sum"]))
    # a 4-byte column gives the rows of its widened copy, for all three aggregates
    aggs = ["sum", "min", "max"]
    as_i64, as_f64 = i32.to(torch.int64), f32.to(torch.float64)
    assert torch.equal(by_rid(ops.group_join_agg(R, S, [i32] * 3, aggs)), by_rid(ops.group_join_agg(R, S, [as_i64] * 3, aggs)))
    rows = by_rid(ops.group_join_agg(R, S, [f32] * 3, aggs))
    assert torch.equal(rows, by_rid(ops.group_join_agg(R, S, [as_f64] * 3, aggs)))
    _check_rows(rows, oracle.rows([f32] * 3, aggs))
    # group_agg_values: a float64 view of the same words for float columns, int64 otherwise
    for like in (f32, f64, torch.float32, torch.float64):
        v = ops.group_agg_values(rows, 1, like)
        assert v.dtype == torch.float64 and v.shape == (n_r,) and v.data_ptr() == rows[:, 3].data_ptr()
        assert torch.equal(v.view(torch.int64), rows[:, 3]) and torch.equal(v.cpu(), oracle.fagg(f32, "min"))
    for like in (None, i32, torch.int64):
        v = ops.group_agg_values(rows, 1, like)
        assert v.dtype == torch.int64 and torch.equal(v, rows[:, 3])
    avg = ops.group_agg_values(rows, 0, f32) / rows[:, 1]  # AVG: one division on the caller's side
    matched = (rows[:, 1] > 0).cpu()
    assert bool(torch.isfinite(avg.cpu()[matched]).all())


# ------------------------------------------------------------ 8. int64 untouched
@pytest.mark.parametrize("dev", devices())
def test_int64_columns_report_their_dtype(C, dev):
    loc = _loc(dev)
    case = _typed_case(C, loc, 150_000, 400_000)
    g = torch.Generator().manual_seed(96)
    cols = [torch.randint(-2**40, 2**40, (400_000,), generator=g).to(case.cols[0].device) for _ in range(3)]
    aggs = ["sum", "min", "max"]
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, _group_cfg(C, 3))
    res, rows = j.join_group_agg(ctx, cols, aggs, 0, 400_000)
    assert res["group_dtypes"] == ["int64"] * 3 and res["group_columns"] == 3
    _check_rows(rows, AggOracle.rows(case.oracle, cols, aggs))
    res1, _ = j.join_group(ctx, cols[0], 0, 400_000)
    assert res1["group_dtypes"] == ["int64"] and res1["group_columns"] == 1


# ------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("dev", devices())
def test_typed_refusals(C, dev):
    loc = _loc(dev)
    case = _typed_case(C, loc, 150_000, 400_000)
    n_s = 400_000
    f64, i32, f32 = case.cols
    assert f64.is_cuda == (dev == "cuda")
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, _group_cfg(C, 2))
    _, good = j.join_group_agg(ctx, [f64, i32], ["min", "max"], 0, n_s)
    want = case.oracle.rows([f64, i32], ["min", "max"])
    _check_rows(good, want)

    def refused(fn, *words, who="join_group_agg"):
        with pytest.raises(RuntimeError) as e:
            fn()
        assert who in str(e.value) and all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: j.join_group_agg(ctx, [f64, f32.to(torch.float16)], ["sum", "min"], 0, n_s), "column 1", "float16")
    refused(lambda: j.join_group_agg(ctx, [i32 > 0, f64], ["sum", "min"], 0, n_s), "column 0", "bool")
    refused(lambda: j.join_group_agg(ctx, [f64, i32.to(torch.uint8)], ["max", "max"], 0, n_s), "column 1", "uint8")
    refused(lambda: j.join_group_agg(ctx, [f32, f32.reshape(-1, 2)], ["sum", "sum"], 0, n_s), "column 1", "float32", "2 dim")
    refused(lambda: j.join_group_agg(ctx, [f64, f32], ["sum", "avg"], 0, n_s), "avg", "aggregate")
    refused(lambda: j.join_group_agg(ctx, [f64, i32, f32], ["sum", "min", "max"], 0, n_s), "group_columns")
    refused(lambda: j.join_group(ctx, f32.to(torch.float16), 0, n_s), "column 0", "float16", who="join_group")
    refused(lambda: j.join_group(ctx, i32 > 0, 0, n_s), "column 0", "bool", who="join_group")
    _check_rows(j.output_groups(), want)  # the refusals left the last run's rows alone

    cfg = C.JoinConfig()
    cfg.kind = C.JoinKind.GROUP
    cfg.passes = 2  # (count-only: a materializing spill is refused at construction)
    refused(lambda: C.HashJoin(case.R, case.S, ctx, cfg).join_group_agg(ctx, [f64], ["sum"], 0, n_s), "spill", "2 passes")


@pytest.mark.parametrize("dev", devices())
def test_in_process_ranks_refuse_typed_columns(C, dev):
    """The values of outer tuples received from other ranks live on those ranks, whatever their dtype."""
    G_R, G_S, n_ranks = 150_000, 400_000, 2
    loc = _loc(dev)
    case = _typed_case(C, loc, G_R, G_S)
    group = C.InProcessGroup(n_ranks)
    errors = []

    def rank_main(r):
        try:
            ctx = _ctx(C, loc, group.communicator(r))
            R = C.Relation(C.Relation.local_size_for(G_R, r, n_ranks), G_R, loc, 0)
            S = C.Relation(C.Relation.local_size_for(G_S, r, n_ranks), G_S, loc, 0)
            R.generate(case.inner, C.Relation.local_offset_for(G_R, r, n_ranks))
            S.generate(case.outer, C.Relation.local_offset_for(G_S, r, n_ranks))
            j = C.HashJoin(R, S, ctx, _group_cfg(C, 2))
            j.join_group_agg(ctx, case.cols[:2], ["sum", "max"], 0, G_S)
        except Exception as e:  # surface in the main thread
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert len(errors) == 2 and all("join_group_agg" in e and "single rank" in e for _, e in errors), errors
