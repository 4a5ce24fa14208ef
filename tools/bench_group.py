#!/usr/bin/env python3
"""Group joins (kind = GROUP) against what answers the same question without
them, same relations, one process on one GPU.

    python tools/bench_group.py [--workload gpu_128m] [--scale 1.0] [--steps 5] [--warmup 2]
                                [--value-dtype int64|int32|float64|float32]

Runs the workload's Zipf-outer variant (theta 0.75 over the inner key domain)
and prints one JSON line per configuration -- join_ms, the device build/probe
span and (a only) the torch reduction as min / median / max over the timed
iterations:

  a  what a user does today: a materializing LEFT_OUTER join, then
     torch.bincount over the inner rids of its pairs (count) and index_add_ of
     the gathered value column (sum).  The pairs are brought to the device
     outside the timed part; the torch part is timed with device events.
  b  a count-only LEFT_OUTER join (bpOuterCount: the same key reads, marks in
     place of counters).
  c  a materializing GROUP join without a value column.
  d  a materializing GROUP join with a value column (join_group).
  e  three join_group runs, one per value column: today's engine route for the
     sums of three columns (join_ms and build/probe spans added up).
  f  one GROUP join over the three columns, [sum, sum, sum] (join_group_agg).
  g  one GROUP join over the three columns, [sum, min, max] (join_group_agg),
     next to a's pair list reduced by torch: gathers of the three columns,
     index_add_ and scatter_reduce_ amin / amax (timed with device events).
  h1 ... h4  join_group_agg over C = 1 ... 4 columns ([min], [min, sum], ...):
     the build/probe span per column count, next to d's.

Every result is checked against oracle counts (sorted outer keys, searchsorted
of the inner keys), sums (wrapping prefix sums of the values in outer key
order) and minima / maxima (scatter_reduce_ over the matching outer tuples).
--value-dtype generates the value columns in that dtype (still strided views of
one payload tensor): int32 over the whole range, float64 as k / 8 with |k| < 2^30
and float32 as k / 8 with |k| < 2^20, so that every float sum is exact in
binary64 whatever the order and the check stays exact equality.  Integer columns
accumulate as int64, float columns as binary64; the torch baselines gather in the
column's dtype, widen the gathered values the same way and reduce with
index_add_ / scatter_reduce_.  For the float dtypes the oracle uses no float
scatter operation (sums from integer prefix sums of k, minima / maxima from
int64 scatter_reduce_ on an order-preserving image of the bits), and the torch
reductions of a (its sum and g's [sum, min, max] baseline) run only with
--float-torch-baseline; without it a's torch_sum / total_sum / *_sum_min_max
fields and the comparisons built on them are null
(profiles/group_typed/README.md says why).  The last lines compare the medians: c and d must lie below a by more than a's
own min-to-max spread; c / b, f / e and g against a's torch route are reported.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _spread(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gpu_128m")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--value-dtype", default="int64", choices=["int64", "int32", "float64", "float32"])
    ap.add_argument("--float-torch-baseline", action="store_true",
                    help="float dtypes: also time torch's float64 index_add_ / scatter_reduce_ (see the module docstring)")
    a = ap.parse_args()
    assert a.steps >= 5, "at least 5 timed steps per configuration"

    import torch
    import hpcjoin
    from hpcjoin.models import workloads as W
    C = hpcjoin.require_native()
    assert torch.cuda.is_available(), "bench_group.py measures the device engine"
    torch.cuda.set_device(0)
    wl = W.get(a.workload, a.scale)
    G_R, G_S = wl.inner_size, wl.outer_size
    ctx = C.ExecContext("device", 0, C.LocalCommunicator())
    inner = C.GenSpec(seed=1234)
    outer = C.GenSpec(distribution=C.KeyDistribution.ZIPF, seed=4321, domain=G_R, zipf_theta=0.75)
    R, S = C.Relation(G_R, G_R, "device", 0), C.Relation(G_S, G_S, "device", 0)
    R.generate(inner, 0)
    S.generate(outer, 0)
    vdt = getattr(torch, a.value_dtype)
    is_float = vdt.is_floating_point
    acc = torch.float64 if is_float else torch.int64  # what the accumulators and the row words hold
    IDENT = {"min": float("inf"), "max": float("-inf")} if is_float else {"min": 2**63 - 1, "max": -2**63}

    def gen(shape, seed):  # int64 as ever; the other dtypes as the module docstring says
        span = {"int64": 2**40, "int32": 2**31, "float64": 2**30, "float32": 2**20}[a.value_dtype]
        k = torch.randint(-span, span, shape, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
        return (k.to(vdt) / 8) if is_float else k.to(vdt)

    torch_reduce = not is_float or a.float_torch_baseline

    def ordered(b):  # int64 bits of binary64 values <-> int64 keys in the values' order (its own inverse)
        return torch.where(b < 0, b ^ 0x7FFFFFFFFFFFFFFF, b)

    def bits(t):  # the int64 words of an accumulator tensor
        return t.view(torch.int64) if t.dtype == torch.float64 else t

    values = gen((G_S,), 9)
    # Two more value columns: with `values` the columns 1, 2, 3 of one [n, 4] payload tensor, read in place.
    payload = gen((G_S, 4), 10)
    payload[:, 1] = values
    cols = [payload[:, 1], payload[:, 2], payload[:, 3]]

    # ---- oracle, by inner rid (rids are 0 .. G_R - 1)
    Rt, St = R.to_tensor(), S.to_tensor()
    sk, order = torch.sort(St[:, 0])
    lo = torch.searchsorted(sk, Rt[:, 0].contiguous(), right=False)
    hi = torch.searchsorted(sk, Rt[:, 0].contiguous(), right=True)
    want_counts = torch.empty(G_R, dtype=torch.int64, device="cuda")
    want_counts[Rt[:, 1]] = hi - lo
    pairs_total, empty = int(want_counts.sum()), int((want_counts == 0).sum())

    def want_agg(col, how):  # by inner rid, from the outer tuples in key order; dtype `acc`
        v = col[St[:, 1][order]].to(acc)
        if how == "sum":
            if is_float:  # integer prefix sums of k = 8 v: exact, and no float atomics
                k = (v * 8).to(torch.int64)
                assert torch.equal(k.to(acc) / 8, v)
                v = k
            p = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(v, 0)])
            per_pos = p[hi] - p[lo]  # int64 wraps both ways
            if is_float:
                assert int(per_pos.abs().max()) < 2**53
                per_pos = per_pos.to(acc) / 8
        else:
            seg = torch.repeat_interleave(torch.arange(G_R, device="cuda"), hi - lo)  # inner position of every pair
            src = v[torch.repeat_interleave(lo, hi - lo) + torch.arange(seg.numel(), device="cuda") -
                    torch.repeat_interleave(torch.cumsum(hi - lo, 0) - (hi - lo), hi - lo)]
            ident = torch.tensor([IDENT[how]], dtype=acc, device="cuda")
            if is_float:  # int64 scatter_reduce_ on keys ordered as the values
                src, ident = ordered(src.view(torch.int64)), ordered(ident.view(torch.int64))
            per_pos = ident.repeat(G_R).scatter_reduce_(0, seg, src, "amin" if how == "min" else "amax", include_self=True)
            if is_float:
                per_pos = ordered(per_pos).view(acc)
        out = torch.empty(G_R, dtype=acc, device="cuda")
        out[Rt[:, 1]] = per_pos
        return out

    want_sums = want_agg(values, "sum")
    want = {(c, how): want_agg(cols[c], how) for c, how in ((0, "sum"), (1, "sum"), (2, "sum"), (0, "min"), (1, "min"),
                                                             (2, "max"))}
    assert torch.equal(want[(0, "sum")], want_sums)
    del sk, order, lo, hi, Rt, St
    torch.cuda.empty_cache()

    def join(kind, materialize):
        cfg = C.JoinConfig()
        cfg.kind = getattr(C.JoinKind, kind)
        cfg.materialize = materialize
        return C.HashJoin(R, S, ctx, cfg)

    def report(name, what, j, runs, extra=None):
        line = {"workload": wl.name, "config": name, "what": what, "value_dtype": a.value_dtype, "inner": G_R, "outer": G_S,
                "join_ms": _spread([r["join_ms"] for r in runs]),
                "dev_build_probe_ms": _spread([r["dev_build_probe_ms"] for r in runs]),
                "matched_pairs": runs[-1]["matched_pairs"], "unmatched_inner": runs[-1]["unmatched_inner"],
                "build_probe_items": runs[-1]["build_probe_items"], "reruns": runs[-1]["reruns"], "plan": repr(j.plan)}
        line.update(extra or {})
        print(json.dumps(line), flush=True)
        return line

    def by_rid(rows, col):
        out = torch.empty(G_R, dtype=torch.int64, device="cuda")
        out[rows[:, 0]] = rows[:, col]
        return out

    lines = {}
    # ---- a: LEFT_OUTER pairs, then torch
    j = join("LEFT_OUTER", True)
    for _ in range(a.warmup):
        j.run()
    runs = [j.run() for _ in range(a.steps)]
    pairs = j.output().cuda()
    assert pairs.shape[0] == pairs_total + empty and runs[-1]["matched_pairs"] == pairs_total
    torch_ms = {"count": [], "sum": []}
    for it in range(a.warmup + a.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        m = pairs[:, 1] != hpcjoin.NULL_RID
        rid, srid = pairs[:, 0][m], pairs[:, 1][m]
        counts = torch.bincount(rid, minlength=G_R)
        ev[1].record()
        if torch_reduce:
            sums = torch.zeros(G_R, dtype=acc, device="cuda").index_add_(0, rid, values[srid].to(acc))
        ev[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            torch_ms["count"].append(ev[0].elapsed_time(ev[1]))
            torch_ms["sum"].append(ev[1].elapsed_time(ev[2]))
    assert torch.equal(counts, want_counts)
    if torch_reduce:
        assert torch.equal(sums, want_sums)
    else:
        sums = None
    # the same pair list reduced to [sum, min, max] of the three columns (configuration g's baseline)
    torch_agg_ms = []
    for it in range(a.warmup + a.steps if torch_reduce else 0):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        m = pairs[:, 1] != hpcjoin.NULL_RID
        rid, srid = pairs[:, 0][m], pairs[:, 1][m]
        counts = torch.bincount(rid, minlength=G_R)
        t_sum = torch.zeros(G_R, dtype=acc, device="cuda").index_add_(0, rid, cols[0][srid].to(acc))
        t_min = torch.full((G_R,), IDENT["min"], dtype=acc, device="cuda").scatter_reduce_(
            0, rid, cols[1][srid].to(acc), "amin", include_self=True)
        t_max = torch.full((G_R,), IDENT["max"], dtype=acc, device="cuda").scatter_reduce_(
            0, rid, cols[2][srid].to(acc), "amax", include_self=True)
        ev[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            torch_agg_ms.append(ev[0].elapsed_time(ev[1]))
    if torch_reduce:
        assert torch.equal(t_sum, want[(0, "sum")]) and torch.equal(t_min, want[(1, "min")]) and torch.equal(t_max, want[(2, "max")])
        del t_sum, t_min, t_max
    total = {k: [r["join_ms"] + t for r, t in zip(runs, torch_ms[k])] for k in ("count", "sum")}
    total["sum"] = [x + c for x, c in zip(total["sum"], torch_ms["count"])]  # the mask and rids are shared
    total["agg"] = [r["join_ms"] + t for r, t in zip(runs, torch_agg_ms)]

    def timed(v):  # null where the torch reduction was not run
        return _spread(v) if torch_reduce else None
    lines["a"] = report("a", "LEFT_OUTER materialize + torch bincount / index_add_", j, runs, {
        "rows": int(pairs.shape[0]), "torch_count_ms": _spread(torch_ms["count"]), "torch_sum_ms": timed(torch_ms["sum"]),
        "total_count_ms": _spread(total["count"]), "total_sum_ms": timed(total["sum"]),
        "torch_sum_min_max_ms": timed(torch_agg_ms), "total_sum_min_max_ms": timed(total["agg"]),
        "torch_reductions_timed": torch_reduce})
    del j, pairs, m, rid, srid, counts, sums
    ctx.trim_workspace()
    torch.cuda.empty_cache()

    # ---- b: count-only LEFT_OUTER
    j = join("LEFT_OUTER", False)
    for _ in range(a.warmup):
        j.run()
    runs = [j.run() for _ in range(a.steps)]
    assert runs[-1]["matched_pairs"] == pairs_total and runs[-1]["unmatched_inner"] == empty
    lines["b"] = report("b", "LEFT_OUTER count-only (bpOuterCount)", j, runs)
    del j
    ctx.trim_workspace()

    # ---- c: GROUP rows (rid, count)
    j = join("GROUP", True)
    for _ in range(a.warmup):
        j.run()
    runs = [j.run() for _ in range(a.steps)]
    rows = j.output_groups().cuda()
    assert rows.shape == (G_R, 2) and torch.equal(by_rid(rows, 1), want_counts)
    assert runs[-1]["matched_pairs"] == pairs_total and runs[-1]["unmatched_inner"] == empty
    lines["c"] = report("c", "GROUP materialize, counts", j, runs, {"rows": G_R})
    del rows

    # ---- d: GROUP rows (rid, count, sum)
    runs = []
    for it in range(a.warmup + a.steps):
        res, rows = j.join_group(ctx, values, 0, G_S)
        if it >= a.warmup:
            runs.append(res)
    rows = rows.cuda()
    assert rows.shape == (G_R, 3) and torch.equal(by_rid(rows, 1), want_counts) and torch.equal(by_rid(rows, 2), bits(want_sums))
    lines["d"] = report("d", "GROUP materialize, counts and sums (join_group)", j, runs, {"rows": G_R})

    del rows, j
    ctx.trim_workspace()

    # ---- e: the sums of three columns today: one join_group per column
    j = join("GROUP", True)
    runs = []
    for it in range(a.warmup + a.steps):
        step = []
        for c in range(3):
            res, rows = j.join_group(ctx, cols[c], 0, G_S)
            step.append(res)
            if it == a.warmup + a.steps - 1:
                assert torch.equal(by_rid(rows.cuda(), 2), bits(want[(c, "sum")]))
        if it >= a.warmup:
            merged = dict(step[-1])
            merged["join_ms"] = sum(r["join_ms"] for r in step)
            merged["dev_build_probe_ms"] = sum(r["dev_build_probe_ms"] for r in step)
            runs.append(merged)
    lines["e"] = report("e", "GROUP, three join_group runs (one per column)", j, runs, {"rows": G_R})
    del j, rows
    ctx.trim_workspace()

    def agg_join(name, what, columns, aggs, wanted):
        cfg = C.JoinConfig()
        cfg.kind = C.JoinKind.GROUP
        cfg.materialize = True
        cfg.group_columns = len(columns)
        jj = C.HashJoin(R, S, ctx, cfg)
        rr = []
        for it in range(a.warmup + a.steps):
            res, rows = jj.join_group_agg(ctx, columns, aggs, 0, G_S)
            if it >= a.warmup:
                rr.append(res)
        rows = rows.cuda()
        assert rows.shape == (G_R, 2 + len(columns)) and torch.equal(by_rid(rows, 1), want_counts)
        for k, w in enumerate(wanted):
            assert torch.equal(by_rid(rows, 2 + k), bits(want[w])), (name, k)
        assert rr[-1]["group_dtypes"] == ["float64" if is_float else "int64"] * len(columns)
        lines[name] = report(name, what, jj, rr, {"rows": G_R, "columns": len(columns), "aggs": aggs})
        del rows, jj
        ctx.trim_workspace()

    agg_join("f", "GROUP join_group_agg [sum, sum, sum]", cols, ["sum", "sum", "sum"], [(0, "sum"), (1, "sum"), (2, "sum")])
    agg_join("g", "GROUP join_group_agg [sum, min, max]", cols, ["sum", "min", "max"], [(0, "sum"), (1, "min"), (2, "max")])
    agg_join("h1", "GROUP join_group_agg [min]", cols[:1], ["min"], [(0, "min")])
    agg_join("h2", "GROUP join_group_agg [min, sum]", cols[:2], ["min", "sum"], [(0, "min"), (1, "sum")])
    agg_join("h3", "GROUP join_group_agg [min, sum, max]", cols, ["min", "sum", "max"], [(0, "min"), (1, "sum"), (2, "max")])
    agg_join("h4", "GROUP join_group_agg [min, sum, max, sum]", cols + [cols[0]], ["min", "sum", "max", "sum"],
             [(0, "min"), (1, "sum"), (2, "max"), (0, "sum")])
    a_agg = lines["a"]["total_sum_min_max_ms"]
    print(json.dumps({
        "workload": wl.name, "value_dtype": a.value_dtype, "comparison": "aggregated columns, join_ms medians",
        "e_three_join_group": lines["e"]["join_ms"]["median"], "f_sum_sum_sum": lines["f"]["join_ms"]["median"],
        "e_over_f": round(lines["e"]["join_ms"]["median"] / lines["f"]["join_ms"]["median"], 3),
        "e_over_f_build_probe": round(lines["e"]["dev_build_probe_ms"]["median"] / lines["f"]["dev_build_probe_ms"]["median"], 3),
        "a_sum_min_max": a_agg, "g_sum_min_max": lines["g"]["join_ms"]["median"],
        "a_over_g": round(a_agg["median"] / lines["g"]["join_ms"]["median"], 3) if a_agg else None,
        "torch_reductions_timed": torch_reduce,
        "build_probe_ms_by_columns": {"join_group": lines["d"]["dev_build_probe_ms"]["median"],
                                      **{str(k): lines["h%d" % k]["dev_build_probe_ms"]["median"] for k in (1, 2, 3, 4)}},
        "checked": "counts, sums, minima and maxima equal the oracle"}), flush=True)

    a_count, a_sum = lines["a"]["total_count_ms"], lines["a"]["total_sum_ms"]
    c_med, d_med, b_med = (lines[k]["join_ms"]["median"] for k in ("c", "d", "b"))
    print(json.dumps({
        "workload": wl.name, "value_dtype": a.value_dtype, "comparison": "join_ms medians (a: join_ms + torch part)",
        "a_count": a_count, "a_sum": a_sum, "b": b_med, "c": c_med, "d": d_med,
        "c_below_a_beyond_spread": a_count["median"] - c_med > a_count["max"] - a_count["min"],
        "d_below_a_beyond_spread": (a_sum["median"] - d_med > a_sum["max"] - a_sum["min"]) if a_sum else None,
        "torch_reductions_timed": torch_reduce,
        "c_over_b": round(c_med / b_med, 3),
        "c_over_b_build_probe": round(lines["c"]["dev_build_probe_ms"]["median"] / lines["b"]["dev_build_probe_ms"]["median"], 3),
        "checked": "counts and sums equal the oracle"}), flush=True)


if __name__ == "__main__":
    main()
