#!/usr/bin/env python3
"""Payload rows of semi, anti and outer joins: what a user did before
HashJoin.join_rows existed against the unfused and the fused row paths, in one
process on one GPU, on the same relations.

    python tools/bench_kind_rows.py [--workload gpu_128m] [--scale 1.0] [--steps 5] [--warmup 2]
                                    [--kinds semi,anti,left_outer,right_outer,full_outer]
                                    [--modes baseline,unfused,fused] [--baseline-only] [--repeat 1]

Inner keys UNIFORM over |R| / 4, outer keys Zipf(0.75) over 2 |R|; 32-byte
payload rows of both sides on the device.  Per kind and mode one JSON line:

  baseline  run() with materialize, output_rids() / output() brought back to the
            device, torch indexing of the payload tensors; outer kinds add the
            masked fill of the NULL sides and the cat.  Only the API that
            existed before join_rows: --baseline-only runs on older trees.
  unfused   run() + materialize_rows (ridRows / NULL-aware materializeLocal).
  fused     join_rows (markPlaceRows from the place pass where the plan fuses).

Each line carries the median wall ms of a whole join + rows ending in a device
synchronise (and every step's), the device build/probe span, the row count,
`rows_fused`, and the bytes the algorithm has to move, from the shapes alone:
32 B per payload row read, 40 B (semi / anti) or 80 B (outer kinds) per row
written.  --repeat N measures every (kind, mode) N times in turn, for the
run-to-run spread of identical runs.

    rocprofv3 --kernel-trace --stats -- python tools/bench_kind_rows.py --kinds semi --modes fused

gives the markPlaceRows kernel time (tools/rocprof_summary.py).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NULL = -1
RID_KINDS = ("semi", "anti")


def baseline_rows(torch, j, kind, rows_r, rows_s):
    """The rows through the API that predates join_rows."""
    res = j.run()
    if kind in RID_KINDS:
        rids = j.output_rids().cuda()
        return res, torch.cat([rids[:, None], rows_s[rids]], 1)
    pairs = j.output().cuda()
    a, b = pairs[:, 0], pairs[:, 1]
    ra = rows_r[a.clamp(min=0)]
    ra[a == NULL] = NULL
    rb = rows_s[b.clamp(min=0)]
    rb[b == NULL] = NULL
    return res, torch.cat([pairs, ra, rb], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gpu_128m")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", default="semi,anti,left_outer,right_outer,full_outer")
    ap.add_argument("--modes", default="baseline,unfused,fused")
    ap.add_argument("--baseline-only", action="store_true", help="only the mode that needs no join_rows")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--tag", default="", help="copied into every line (e.g. the tree measured)")
    a = ap.parse_args()
    modes = ["baseline"] if a.baseline_only else a.modes.split(",")

    import torch
    import hpcjoin
    from hpcjoin.models import workloads as W
    C = hpcjoin.require_native()
    assert torch.cuda.is_available(), "bench_kind_rows.py measures the device engine"
    torch.cuda.set_device(0)
    wl = W.get(a.workload, a.scale)
    G_R, G_S = wl.inner_size, wl.outer_size
    ctx = C.ExecContext("device", 0, C.LocalCommunicator())
    inner = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=1234, domain=max(1, G_R // 4))
    outer = C.GenSpec(distribution=C.KeyDistribution.ZIPF, seed=4321, domain=2 * G_R, zipf_theta=0.75)
    R, S = C.Relation(G_R, G_R, "device", 0), C.Relation(G_S, G_S, "device", 0)
    R.generate(inner, 0)
    S.generate(outer, 0)
    rows_r = C.ops.generate_payload(G_R, 0, 9001, "cuda")
    rows_s = C.ops.generate_payload(G_S, 0, 9002, "cuda")
    args = (ctx, rows_r, 0, G_R, rows_s, 0, G_S)
    for rep in range(a.repeat):
        for kind in a.kinds.split(","):
            for mode in modes:
                cfg = C.JoinConfig()
                cfg.kind = getattr(C.JoinKind, kind.upper())
                cfg.materialize = True
                if mode != "baseline":
                    cfg.kind_rows = 1 if mode == "fused" else 0
                j = C.HashJoin(R, S, ctx, cfg)
                wall, span, res, rows = [], [], None, None
                for step in range(a.warmup + a.steps):
                    rows = None  # the previous step's rows are freed before the next join
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if mode == "baseline":
                        res, rows = baseline_rows(torch, j, kind, rows_r, rows_s)
                    elif mode == "unfused":
                        res = j.run()
                        rows = j.materialize_rows(*args)
                    else:
                        res, rows = j.join_rows(*args)
                    torch.cuda.synchronize()
                    if step >= a.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                        span.append(res["dev_build_probe_ms"])
                m = rows.shape[0]
                if kind in RID_KINDS:
                    must = m * (32 + 40)
                else:
                    nulls = int((rows[:, 0] == NULL).sum()) + int((rows[:, 1] == NULL).sum())
                    must = m * 80 + (2 * m - nulls) * 32
                line = {"workload": wl.name, "kind": kind, "mode": mode, "rep": rep, "inner": G_R, "outer": G_S,
                        "wall_ms": round(statistics.median(wall), 3), "step_wall_ms": [round(x, 3) for x in wall],
                        "dev_build_probe_ms": round(statistics.median(span), 3),
                        "rows": m, "row_words": rows.shape[1], "must_move_bytes": must,
                        "rows_fused": bool(res["rows_fused"]),
                        "plan": repr(j.plan)}
                if a.tag:
                    line["tag"] = a.tag
                print(json.dumps(line), flush=True)
                del j, rows
                torch.cuda.empty_cache()
                ctx.trim_workspace()


if __name__ == "__main__":
    main()
