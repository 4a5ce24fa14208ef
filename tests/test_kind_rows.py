"""Payload rows of semi, anti and outer joins (HashJoin.join_rows /
materialize_rows, kernels/kind_rows.hip and the host twins).

Formats.  SEMI / ANTI: int64 [m, 5] = [outer rid, outer payload row (4)], one
row per qualifying outer tuple.  LEFT / RIGHT / FULL_OUTER: int64 [m, 10] =
[rid_inner, rid_outer, inner row (4), outer row (4)]; in a padded row the
missing side's rid and its four payload words are all NULL_RID (-1).

Every comparison is exact, after sorting the rows by rid.  Payload rows come
from ``C.ops.generate_payload`` with two different seeds, and every relation's
rids start at OFF = 1000 (``rows[rid - OFF]``), so an offset bug cannot pass.
Inputs follow the recipe of test_semi_join.py: inner UNIFORM over G_R // 4
keys, outer ZIPF / UNIFORM over 2 * G_R keys.  Each case asserts from its torch
oracle that between 5 % and 95 % of every preserved side is unmatched and that
the inner-join count differs from the semi count: a join that returns nothing,
everything or the inner join cannot pass.
"""
import functools
import threading

import numpy as np
import pytest
import torch

import helpers as H
from conftest import devices
from helpers import gen, ref_join_count

OFF = 1000
SEED_R, SEED_S = 9001, 9002
NULL = -1
RID_KINDS = ["SEMI", "ANTI"]
OUTER_KINDS = ["LEFT_OUTER", "RIGHT_OUTER", "FULL_OUTER"]
KINDS = RID_KINDS + OUTER_KINDS
KEEP = {"LEFT_OUTER": (True, False), "RIGHT_OUTER": (False, True), "FULL_OUTER": (True, True)}


def _loc(dev):
    return "device" if dev == "cuda" else "host"


def _ctx(C, loc, comm=None):
    return C.ExecContext(loc, 0 if loc == "device" else -1, comm or C.LocalCommunicator())


# ---------------------------------------------------------------------- oracle
def _by_rid(rows):
    """[m, 5] rows in rid order."""
    return rows[torch.sort(rows[:, 0], stable=True).indices]


def _by_pair(rows):
    """[m, 10] (or [m, 2]) rows in (rid_inner, rid_outer) order (two stable sorts)."""
    rows = rows[torch.sort(rows[:, 1], stable=True).indices]
    return rows[torch.sort(rows[:, 0], stable=True).indices]


def _rid_rows(rids, rows_s):
    """Expected [m, 5] rows of a rid list, in rid order."""
    rids = rids.sort().values
    return torch.cat([rids[:, None], rows_s[rids - OFF]], 1)


def _pair_rows(pairs, rows_r, rows_s, off_r=OFF, off_s=OFF):
    """Expected [m, 10] rows of a NULL-padded pair list, in the pairs' order; NULL rids index nothing."""
    out = torch.full((pairs.shape[0], 10), NULL, dtype=torch.int64, device=pairs.device)
    out[:, :2] = pairs
    a, b = pairs[:, 0] != NULL, pairs[:, 1] != NULL
    out[a, 2:6] = rows_r[pairs[a, 0] - off_r]
    out[b, 6:10] = rows_s[pairs[b, 1] - off_s]
    return out


def _check_rid_rows(rows, expected):
    assert rows.dtype == torch.int64 and rows.dim() == 2 and rows.shape[1] == 5
    assert rows.shape[0] == expected.shape[0], (rows.shape[0], expected.shape[0])
    rows = _by_rid(rows.to(expected.device))
    assert rows.shape[0] < 2 or bool((rows[1:, 0] != rows[:-1, 0]).all()), "an outer rid was emitted twice"
    assert torch.equal(rows, expected)


def _check_pair_rows(rows, expected):
    assert rows.dtype == torch.int64 and rows.dim() == 2 and rows.shape[1] == 10
    assert rows.shape[0] == expected.shape[0], (rows.shape[0], expected.shape[0])
    rows = _by_pair(rows.to(expected.device))
    assert rows.shape[0] < 2 or bool((rows[1:, :2] != rows[:-1, :2]).any(1).all()), "a row was emitted twice"
    assert torch.equal(rows, expected)


class Case:
    """Two relations with rids from OFF, their payload rows and the oracle, computed once per shape.

    The oracle lives on the CPU: semi / anti from ``torch.isin``, the outer kinds from the already-tested
    ``ops.full_outer_join`` pairs of the host engine (left = its rows with an inner rid, right = those with an
    outer rid)."""

    def __init__(self, C, dev, G_R, G_S, outer_dist):
        from hpcjoin import ops
        self.G_R, self.G_S = G_R, G_S
        self.Rt = gen(C, G_R, seed=1234, dist="UNIFORM", domain=max(1, G_R // 4), device=dev, offset=OFF)
        self.St = gen(C, G_S, seed=4321, dist=outer_dist, domain=2 * G_R, device=dev, offset=OFF)
        self.R = C.Relation.from_tensor(self.Rt, G_R)
        self.S = C.Relation.from_tensor(self.St, G_S)
        self.rows_r = C.ops.generate_payload(G_R, OFF, SEED_R, dev)
        self.rows_s = C.ops.generate_payload(G_S, OFF, SEED_S, dev)
        rt, st, rows_r, rows_s = self.Rt.cpu(), self.St.cpu(), self.rows_r.cpu(), self.rows_s.cpu()
        assert int(rt[:, 1].min()) == OFF and int(st[:, 1].min()) == OFF
        assert not torch.equal(rows_r[:1000], rows_s[:1000])
        isin = torch.isin(st[:, 0], rt[:, 0])
        self.count = {"SEMI": int(isin.sum()), "ANTI": G_S - int(isin.sum())}
        self.expected = {"SEMI": _rid_rows(st[:, 1][isin], rows_s), "ANTI": _rid_rows(st[:, 1][~isin], rows_s)}
        self.inner_count = ref_join_count(rt[:, 0], st[:, 0])
        full = ops.full_outer_join(rt, st)
        pairs = {"FULL_OUTER": full, "LEFT_OUTER": full[full[:, 0] != NULL], "RIGHT_OUTER": full[full[:, 1] != NULL]}
        self.unmatched_inner = int((full[:, 1] == NULL).sum())
        self.unmatched_outer = int((full[:, 0] == NULL).sum())
        assert full.shape[0] == self.inner_count + self.unmatched_inner + self.unmatched_outer
        assert self.unmatched_outer == self.count["ANTI"]
        for k in OUTER_KINDS:
            self.expected[k] = _pair_rows(_by_pair(pairs[k]), rows_r, rows_s)
            self.count[k] = pairs[k].shape[0]
        # a join that returned nothing, everything or the inner join cannot pass
        assert 0.05 * G_S < self.unmatched_outer < 0.95 * G_S, (self.unmatched_outer, G_S)
        assert 0.05 * G_R < self.unmatched_inner < 0.95 * G_R, (self.unmatched_inner, G_R)
        assert self.inner_count != self.count["SEMI"] and self.inner_count > 0

    def check(self, kind, rows):
        (_check_rid_rows if kind in RID_KINDS else _check_pair_rows)(rows, self.expected[kind])

    def check_result(self, kind, res, rows):
        m = rows.shape[0]
        assert res["local_matches"] == res["global_matches"] == m == self.count[kind], (res, self.count[kind])
        assert not res["output_overflow"]
        if kind in RID_KINDS:
            assert res["output_rids"] == m and res["output_pairs"] == 0
            return
        keep_r, keep_s = KEEP[kind]
        assert res["output_pairs"] == m and res["output_rids"] == 0
        assert res["matched_pairs"] == self.inner_count
        assert res["unmatched_inner"] == (self.unmatched_inner if keep_r else 0)
        assert res["unmatched_outer"] == (self.unmatched_outer if keep_s else 0)
        assert res["matched_pairs"] + res["unmatched_inner"] + res["unmatched_outer"] == m
        rows = rows.cpu()
        assert int((rows[:, 0] == NULL).sum()) == res["unmatched_outer"]
        assert int((rows[:, 1] == NULL).sum()) == res["unmatched_inner"]

    def args(self, ctx, inner_rows=None):
        return (ctx, self.rows_r if inner_rows is None else inner_rows, OFF, self.G_R, self.rows_s, OFF, self.G_S)


@functools.lru_cache(maxsize=None)
def _case(C, dev, G_R, G_S, outer_dist="ZIPF"):
    return Case(C, dev, G_R, G_S, outer_dist)


# ------------------------------------------------------------------ 1. kernels
def _partitioned(ops, t, b1, b2, wide):
    """Network pass, then a local pass on the b2 key bits above the network digit."""
    v, b = ops.radix_partition(t, b1, 64 if wide else 32, wide)
    return ops.local_partition(v, b, b1 if wide else 32, b2, wide)


def _keys_by_position(v, pb, b1, b2, wide):
    if wide:
        return v[:, 0]
    sizes = (pb[1:] - pb[:-1]).to(v.device)
    part = torch.repeat_interleave(torch.arange(pb.numel() - 1, device=v.device), sizes)
    return ((v >> 32) << b1) | (part >> b2)


def _rids_by_position(v, wide):
    return v[:, 1] if wide else v & 0xFFFFFFFF


def _mark_rows(ops, R, S, rows_s, b1, b2, wide, r_chunk, s_chunk, out_capacity=0):
    """build_probe_mark_rows over the two-pass partitioned relations; also the oracle's selection and rids by
    outer position."""
    rv, rpb = _partitioned(ops, R, b1, b2, wide)
    sv, spb = _partitioned(ops, S, b1, b2, wide)
    res = ops.build_probe_mark_rows(rv, sv, rpb, spb, 64 if wide else 32 + b2, 64 if wide else 32, wide=wide,
                                    r_chunk=r_chunk, s_chunk=s_chunk, outer_rows=rows_s, rid_offset=OFF,
                                    out_capacity=out_capacity)
    marked = torch.isin(_keys_by_position(sv, spb, b1, b2, wide), R[:, 0])
    return res, marked, _rids_by_position(sv, wide), spb


def _check_mark_rows(res, kind, sel, rid, rows_s, n_s, capacity=None):
    """The buffer of one kind: rows below min(count, capacity) exact and in position order, sentinel beyond."""
    count = int(sel.sum())
    cap = n_s if capacity is None else capacity
    assert res[kind + "_count"] == count and res["capacity"] == cap and res["guard_rows"] == 64
    buf = res[kind + "_rows"]
    assert buf.dtype == torch.int64 and tuple(buf.shape) == (cap + 64, 5)
    stored = min(count, cap)
    want = rid[sel]  # a unit's rows land in position order, units in partition order
    got = buf[:stored]
    assert torch.equal(got[:, 0], want[:stored])
    assert torch.equal(got[:, 1:], rows_s[want[:stored] - OFF])
    uniq = torch.unique(got[:, 0])
    assert uniq.numel() == stored, "an outer rid was emitted twice"
    assert bool((buf[stored:] == res["sentinel"]).all()), "a row was written at or beyond the capacity / the count"
    return count


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_mark_place_rows(C, dev, wide):
    """The shape of test_build_probe_marks: 60,000 x 200,000 over 8 final partitions, r_chunk = 512, s_chunk =
    1024: ~25 ragged units per partition with boundaries off the 64-bit words.  Then with out_capacity = count -
    37: the count is reported in full, the rows below the capacity are exact, nothing beyond is written."""
    from hpcjoin import ops
    n_r, n_s = 60_000, 200_000
    R = gen(C, n_r, device=dev, seed=11, dist="UNIFORM", domain=n_r // 4, offset=OFF)
    S = gen(C, n_s, device=dev, seed=12, dist="UNIFORM", domain=2 * n_r, offset=OFF)
    rows_s = C.ops.generate_payload(n_s, OFF, SEED_S, dev)
    res, marked, rid, spb = _mark_rows(ops, R, S, rows_s, 2, 1, wide, 512, 1024)
    counts = {}
    for kind, sel in (("semi", marked), ("anti", ~marked)):
        counts[kind] = _check_mark_rows(res, kind, sel, rid, rows_s, n_s)
        got = res[kind + "_rows"][:counts[kind]]
        _check_rid_rows(got, _rid_rows(rid[sel].cpu(), rows_s.cpu()))
    assert 0.05 * n_s < counts["semi"] < 0.95 * n_s and counts["semi"] + counts["anti"] == n_s
    assert counts["semi"] != ref_join_count(R[:, 0].cpu(), S[:, 0].cpu())
    sizes = spb[1:] - spb[:-1]
    assert int((sizes % 64 != 0).sum()) > 0 and int(sizes.min()) > 1024  # several units each, ragged ends
    for kind in ("semi", "anti"):
        cap = counts[kind] - 37
        # (the device partition passes place tuples in no fixed order: positions are those of this call)
        clipped, marked, rid, _ = _mark_rows(ops, R, S, rows_s, 2, 1, wide, 512, 1024, out_capacity=cap)
        _check_mark_rows(clipped, kind, marked if kind == "semi" else ~marked, rid, rows_s, n_s, capacity=cap)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 1 / 4096, 1 / 64, 0.5, 1.0], ids=["0", "1/4096", "1/64", "1/2", "1"])
def test_mark_place_rows_selectivity(C, cuda, p):
    """A share p of the outer keys is drawn from the inner key set, the rest from a disjoint range; semi and
    anti cover p and 1 - p: units with nothing selected, queue flushes that straddle many mark words, flushes
    of exactly 64 rows.  (The 5 %-95 % guard is waived here: the oracle counts are asserted instead.)"""
    from hpcjoin import ops
    n_r, n_s = 40_000, 100_003
    g = torch.Generator().manual_seed(1 + int(p * 8192))
    R = gen(C, n_r, device="cpu", seed=21, dist="UNIFORM", domain=n_r // 4, offset=OFF)
    take = torch.rand(n_s, generator=g) < p
    inside = R[:, 0][torch.randint(0, n_r, (n_s,), generator=g)]
    outside = (1 << 20) + torch.randint(0, 2 * n_r, (n_s,), generator=g)  # no inner key is this large
    S = torch.stack([torch.where(take, inside, outside), OFF + torch.arange(n_s)], 1).contiguous()
    R, S = R.cuda(), S.cuda()
    rows_s = C.ops.generate_payload(n_s, OFF, SEED_S, "cuda")
    res, marked, rid, _ = _mark_rows(ops, R, S, rows_s, 2, 1, False, 512, 1024)
    n_in = int(take.sum())
    assert int(marked.sum()) == n_in and (p not in (0.0, 1.0) or n_in == int(p) * n_s)
    assert _check_mark_rows(res, "semi", marked, rid, rows_s, n_s) == n_in
    assert _check_mark_rows(res, "anti", ~marked, rid, rows_s, n_s) == n_s - n_in


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("wide", [False, True], ids=["compressed", "wide"])
def test_outer_pad_rows(C, dev, wide):
    """The 10-word shapes of the row-writing place pass in the unsplit layouts (the engine fuses outer kinds
    over the split layout only): the shape of test_build_probe_outer, 60,000 x 200,000 over 8 final partitions,
    r_chunk = 512, s_chunk = 1024.  The padded rows land behind the pairs' rows from the pairs' bases."""
    from hpcjoin import ops
    n_r, n_s = 60_000, 200_000
    R = gen(C, n_r, device=dev, seed=11, dist="UNIFORM", domain=30_000, offset=OFF)
    spec = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=12, domain=30_000, key_offset=15_000)
    S = C.ops.generate(n_s, OFF, n_s, spec, dev)
    rows_r = C.ops.generate_payload(n_r, OFF, SEED_R, dev)
    rows_s = C.ops.generate_payload(n_s, OFF, SEED_S, dev)
    rv, rpb = _partitioned(ops, R, 2, 1, wide)
    sv, spb = _partitioned(ops, S, 2, 1, wide)
    for kind in OUTER_KINDS:
        keep_r, keep_s = KEEP[kind]
        res = ops.build_probe_outer_rows(rv, sv, rpb, spb, 64 if wide else 33, 64 if wide else 32, wide=wide,
                                         r_chunk=512, s_chunk=1024, keep_inner=keep_r, keep_outer=keep_s,
                                         inner_rows=rows_r, inner_rid_offset=OFF, outer_rows=rows_s,
                                         outer_rid_offset=OFF)
        pairs, buf = res["pairs"], res["rows"]  # the pairs of the already-tested pair path, same call
        m, matched = pairs.shape[0], res["matched_pairs"]
        assert m == matched + res["unmatched_inner"] + res["unmatched_outer"] and tuple(buf.shape) == (m + 64, 10)
        assert 0.05 * n_s < res["unmatched_outer"] < 0.95 * n_s or not keep_s
        assert 0.05 * n_r < res["unmatched_inner"] < 0.95 * n_r or not keep_r
        assert matched > 0.05 * n_s and bool((pairs[:matched] != NULL).all())
        # the padded rows of a side keep the pair path's position order; the matched rows are the pairs' own
        assert torch.equal(buf[:m], _pair_rows(pairs, rows_r, rows_s))
        assert bool((buf[m:] == res["sentinel"]).all())


SIZES = [0, 1, 63, 64, 65, 100_003]


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("n", SIZES)
def test_rid_rows(C, dev, n):
    from hpcjoin import ops
    n_rows = 50_000
    rows = C.ops.generate_payload(n_rows, OFF, SEED_S, dev)
    g = torch.Generator().manual_seed(n)
    rids = (OFF + torch.randint(0, n_rows, (n,), generator=g)).to(dev)
    if n:
        rids[0], rids[-1] = OFF + n_rows - 1, OFF  # the last and the first row
    out = ops.rid_rows(rids, rows, OFF)
    assert out.dtype == torch.int64 and tuple(out.shape) == (n, 5) and out.device == rids.device
    assert torch.equal(out, torch.cat([rids[:, None], rows[rids - OFF]], 1))


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("n", SIZES)
def test_pair_rows_nulls(C, dev, n):
    """NULL_RID on either side at pseudo-random positions, and every row NULL on one side; variants 0-3."""
    from hpcjoin import ops
    n_a, n_b, off_a, off_b = 30_000, 50_000, OFF, OFF + 77
    rows_a = C.ops.generate_payload(n_a, off_a, SEED_R, dev)
    rows_b = C.ops.generate_payload(n_b, off_b, SEED_S, dev)
    g = torch.Generator().manual_seed(100 + n)
    base = torch.stack([off_a + torch.randint(0, n_a, (n,), generator=g),
                        off_b + torch.randint(0, n_b, (n,), generator=g)], 1)
    mixed = base.clone()
    mixed[torch.rand(n, generator=g) < 0.3, 0] = NULL
    mixed[torch.rand(n, generator=g) < 0.3, 1] = NULL
    no_inner, no_outer = base.clone(), base.clone()
    no_inner[:, 0] = NULL
    no_outer[:, 1] = NULL
    for pairs in (mixed, no_inner, no_outer):
        pairs = pairs.contiguous().to(dev)
        want = _pair_rows(pairs, rows_a, rows_b, off_a, off_b)
        if n:
            assert bool((want[pairs[:, 0] == NULL][:, [0, 2, 3, 4, 5]] == NULL).all())  # five -1 words
            assert bool((want[pairs[:, 1] == NULL][:, [1, 6, 7, 8, 9]] == NULL).all())
        for variant in range(4):
            out = ops.pair_rows(pairs, rows_a, off_a, rows_b, off_b, variant=variant)
            assert out.dtype == torch.int64 and tuple(out.shape) == (n, 10)
            assert torch.equal(out, want), variant
    if n > 1:
        assert int((mixed[:, 0] == NULL).sum()) + int((mixed[:, 1] == NULL).sum()) > 0


@pytest.mark.parametrize("dev", devices())
def test_pair_rows_equal_materialize_payloads(C, dev):
    """Pairs without NULLs: bit-identical to the existing materialize_payloads path, every variant."""
    from hpcjoin import ops
    case = _case(C, dev, 20_000, 50_000, "UNIFORM")
    loc = _loc(dev)
    cfg = C.JoinConfig()
    cfg.materialize = True
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, cfg)
    res = j.run()
    pairs = j.output().to(dev)
    ref = j.materialize_payloads(*case.args(ctx))
    assert res["output_pairs"] == case.inner_count == pairs.shape[0] and not bool((pairs == NULL).any())
    for variant in range(4):
        assert torch.equal(ops.pair_rows(pairs, case.rows_r, OFF, case.rows_s, OFF, variant=variant), ref)


# ------------------------------------------------------------- 2. engine, N = 1
@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("outer_dist", ["ZIPF", "UNIFORM"])
@pytest.mark.parametrize("fmt", ["COMPRESSED", "WIDE"])
@pytest.mark.parametrize("kind", KINDS)
def test_engine_rows(C, dev, kind, fmt, outer_dist):
    loc = _loc(dev)
    case = _case(C, dev, 150_000, 400_000, outer_dist)
    cfg = C.JoinConfig()
    cfg.kind = getattr(C.JoinKind, kind)
    cfg.format = getattr(C.TupleFormat, fmt)
    cfg.materialize = True
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, cfg)
    assert j.plan.kind == cfg.kind and j.plan.wide == (fmt == "WIDE") and not j.plan.bitmap_join
    for kind_rows in (None, 1):  # the default (outer kinds unfused), then fused wherever the plan can
        if kind_rows is not None:
            cfg.kind_rows = kind_rows
            j = C.HashJoin(case.R, case.S, ctx, cfg)
        fusable = kind in RID_KINDS or (kind_rows == 1 and j.plan.split_local and not j.plan.wide)
        assert j.can_fuse_kind_rows == (dev == "cuda" and fusable)
        for _ in range(2):  # marks and counts are re-zeroed: a second run gives the same rows
            res, rows = j.join_rows(*case.args(ctx))
            assert res["rows_fused"] == (j.can_fuse_kind_rows if dev == "cuda" else False)
            case.check_result(kind, res, rows)
            case.check(kind, rows)
    res = j.run()
    assert not res["rows_fused"]
    rows = j.materialize_rows(*case.args(ctx))
    case.check_result(kind, res, rows)
    case.check(kind, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_engine_rows_split_fused(C, cuda, kind):
    """The split layout: every kind fuses.  Outer kinds with r_chunk 0 / 512 / 2048 (the matched rows come from
    the LDS-cached and the staged row kernels) and output_capacity 0 / 1000 (too small: one exactly sized
    re-run, no overflow left); kind_rows = 0 gives the same rows unfused."""
    case = _case(C, "cuda", 160_000, 300_000)
    ctx = _ctx(C, "device")
    shapes = [(r, cap) for r in (0, 512, 2048) for cap in (0, 1000)] if kind in OUTER_KINDS else [(0, 0)]
    for kind_rows in (1, 0):
        for r_chunk, cap in shapes if kind_rows else shapes[:1]:
            cfg = C.JoinConfig()
            cfg.kind = getattr(C.JoinKind, kind)
            cfg.materialize = True
            cfg.split_local = True
            cfg.r_chunk = r_chunk
            cfg.output_capacity = cap
            cfg.kind_rows = kind_rows
            j = C.HashJoin(case.R, case.S, ctx, cfg)
            assert j.plan.split_local and not j.plan.wide and j.can_fuse_kind_rows == bool(kind_rows)
            res, rows = j.join_rows(*case.args(ctx))
            assert res["rows_fused"] == bool(kind_rows) and not res["output_overflow"], (r_chunk, cap, res)
            case.check_result(kind, res, rows)
            case.check(kind, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RID_KINDS)
def test_semi_bitmap_rows(C, cuda, kind):
    """The set-bitmap plan (semi_bitmap, dense keys): its rids come from bitmapSemiRidsKernel, the rows unfused."""
    D, nb = 1 << 20, 10
    base = H.inner_keys("half", D, nb)
    inner = np.random.default_rng(3).permutation(np.concatenate([base, base[::3]]))  # repeated inner keys
    outer = H.outer_keys("uniform", base, D)
    Rt, St = H.key_tuples(inner, "cuda", OFF), H.key_tuples(outer, "cuda", OFF)
    rows_s = C.ops.generate_payload(outer.size, OFF, SEED_S, "cuda")
    isin = torch.isin(St[:, 0], Rt[:, 0])
    sel = isin if kind == "SEMI" else ~isin
    assert 0.05 * outer.size < int(sel.sum()) < 0.95 * outer.size
    assert ref_join_count(Rt[:, 0].cpu(), St[:, 0].cpu()) != int(isin.sum())
    cfg = C.JoinConfig()
    cfg.network_bits = nb
    cfg.key_hashing = C.KeyHashing.OFF
    cfg.network_histogram = C.HistogramMode.EXACT
    cfg.kind = getattr(C.JoinKind, kind)
    cfg.materialize = True
    cfg.semi_bitmap = True
    ctx = _ctx(C, "device")
    j = C.HashJoin(C.Relation.from_tensor(Rt, inner.size), C.Relation.from_tensor(St, outer.size), ctx, cfg)
    assert j.plan.bitmap_join and j.plan.bitmap_set and not j.can_fuse_kind_rows
    empty = torch.empty((0, 4), dtype=torch.int64, device="cuda")
    expected = _rid_rows(St[:, 1][sel].cpu(), rows_s.cpu())
    for _ in range(2):
        res, rows = j.join_rows(ctx, empty, 0, 0, rows_s, OFF, outer.size)
        assert res["bitmap_join"] and not res["rows_fused"] and res["output_rids"] == expected.shape[0]
        _check_rid_rows(rows, expected)


# ------------------------------------------------------------ 3. host-only checks
def _host_join(C, case, kind, materialize=True, comm=None):
    cfg = C.JoinConfig()
    cfg.kind = getattr(C.JoinKind, kind)
    cfg.materialize = materialize
    ctx = _ctx(C, "host", comm)
    return C.HashJoin(case.R, case.S, ctx, cfg), ctx


def test_join_rows_needs_materialize(C):
    case = _case(C, "cpu", 20_000, 50_000, "UNIFORM")
    j, ctx = _host_join(C, case, "SEMI", materialize=False)
    with pytest.raises(RuntimeError) as e:
        j.join_rows(*case.args(ctx))
    assert "join_rows" in str(e.value) and "materialize" in str(e.value)


@pytest.mark.parametrize("kind", ["ANTI", "RIGHT_OUTER"])
def test_outer_payload_too_short(C, kind):
    """One payload row short of the outer rids: refused before anything runs."""
    case = _case(C, "cpu", 20_000, 50_000, "UNIFORM")
    j, ctx = _host_join(C, case, kind)
    with pytest.raises(RuntimeError) as e:
        j.join_rows(ctx, case.rows_r, OFF, case.G_R, case.rows_s[:-1], OFF, case.G_S)
    assert "outer payload rows" in str(e.value) and "cover" in str(e.value)
    assert j.run()["global_matches"] == case.count[kind]
    with pytest.raises(RuntimeError) as e:  # the same rows, one rid further on
        j.materialize_rows(ctx, case.rows_r, OFF, case.G_R, case.rows_s, OFF + 1, case.G_S)
    assert "outer payload rows" in str(e.value)


def test_inner_payload_checked_for_outer_kinds_only(C):
    case = _case(C, "cpu", 20_000, 50_000, "UNIFORM")
    empty = torch.empty((0, 4), dtype=torch.int64)
    j, ctx = _host_join(C, case, "SEMI")
    res, rows = j.join_rows(*case.args(ctx, inner_rows=empty))  # the inner payload is never read
    case.check_result("SEMI", res, rows)
    case.check("SEMI", rows)
    j, ctx = _host_join(C, case, "LEFT_OUTER")
    with pytest.raises(RuntimeError) as e:
        j.join_rows(*case.args(ctx, inner_rows=empty))
    assert "inner payload rows" in str(e.value)


def test_two_ranks_refused(C):
    """kind != INNER at N = 2: refused on both ranks before any communication, naming the entry point."""
    case = _case(C, "cpu", 20_000, 50_000, "UNIFORM")
    group = C.InProcessGroup(2)
    messages, errors = [None, None], []

    def rank_main(r):
        try:
            cfg = C.JoinConfig()
            cfg.kind = C.JoinKind.SEMI
            cfg.materialize = True
            ctx = _ctx(C, "host", group.communicator(r))
            h_r, h_s = case.G_R // 2, case.G_S // 2
            R = C.Relation.from_tensor(case.Rt[r * h_r:(r + 1) * h_r].contiguous(), case.G_R)
            S = C.Relation.from_tensor(case.St[r * h_s:(r + 1) * h_s].contiguous(), case.G_S)
            j = C.HashJoin(R, S, ctx, cfg)
            for entry in (j.join_rows, j.materialize_rows):
                try:
                    entry(*case.args(ctx))
                    messages[r] = "no error from " + entry.__name__
                    return
                except RuntimeError as e:
                    if entry.__name__ not in str(e) or "2" not in str(e) or "SEMI" not in str(e).upper():
                        messages[r] = "unexpected message: " + str(e)
                        return
            messages[r] = "ok"
        except Exception as e:  # surface in the main thread
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    assert messages == ["ok", "ok"], messages


@pytest.mark.parametrize("dev", devices())
def test_inner_kind_delegates(C, dev):
    """kind INNER through the new entry points: join_materialized / materialize_payloads, row for row."""
    case = _case(C, dev, 20_000, 50_000, "UNIFORM")
    loc = _loc(dev)
    cfg = C.JoinConfig()
    cfg.materialize = True
    ctx = _ctx(C, loc)
    j = C.HashJoin(case.R, case.S, ctx, cfg)
    res_a, rows_a = j.join_rows(*case.args(ctx))
    res_b, rows_b = j.join_materialized(*case.args(ctx))
    assert res_a["output_pairs"] == res_b["output_pairs"] == case.inner_count == rows_a.shape[0]
    assert res_a["rows_fused"] == res_b["rows_fused"]
    assert torch.equal(_by_pair(rows_a.cpu()), _by_pair(rows_b.cpu()))
    j.run()
    assert torch.equal(_by_pair(j.materialize_rows(*case.args(ctx)).cpu()), _by_pair(rows_b.cpu()))


# ----------------------------------------------------------- 4. Python surface
@pytest.mark.parametrize("dev", devices())
def test_ops_rows(C, dev):
    from hpcjoin import ops
    case = _case(C, dev, 20_000, 50_000, "UNIFORM")
    R, S, rows_r, rows_s = case.Rt, case.St, case.rows_r, case.rows_s
    case.check("SEMI", ops.semi_join_rows(R, S, rows_s, rid_offset=OFF))
    case.check("ANTI", ops.anti_join_rows(R, S, rows_s, rid_offset=OFF))
    case.check("LEFT_OUTER", ops.left_outer_join_rows(R, S, rows_r, rows_s, rid_offset=OFF))
    case.check("RIGHT_OUTER", ops.right_outer_join_rows(R, S, rows_r, rows_s, rid_offset=OFF))
    cfg = C.JoinConfig()
    cfg.kind_rows = 0
    case.check("FULL_OUTER", ops.full_outer_join_rows(R, S, rows_r, rows_s, rid_offset=OFF, config=cfg))
    case.check("FULL_OUTER", ops.full_outer_join_rows(R, S, rows_r, rows_s, rid_offset=OFF))


def test_config_kind_rows_from_dict_and_env(C, monkeypatch):
    from hpcjoin.utils import config_from_dict, config_to_dict
    assert config_to_dict(C.JoinConfig())["kind_rows"] in (0, 1, 2)
    assert config_from_dict({"kind_rows": 0}).kind_rows == 0
    monkeypatch.setenv("HPCJOIN_KIND_ROWS", "1")
    assert config_from_dict({"kind_rows": 0}).kind_rows == 1  # the environment overrides
