#!/usr/bin/env python3
"""Semi- and anti-join against the materializing inner join of the same inputs,
in one process on one GPU.

    python tools/bench_semi.py [--workload gpu_128m] [--scale 1.0] [--steps 5] [--warmup 2] [--kinds inner,semi,anti]
                               [--plans mark,bitmap] [--materialize 0|1] [--inner-repeats K]

Runs the workload as generated (unique outer keys) and its Zipf-outer variant
(theta 0.75 over the inner key domain), each as kind = INNER / SEMI / ANTI with
materialize = True, and prints one JSON line per (variant, kind): median
join_ms, the device build/probe span, the result count and the plan.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_semi.py --kinds semi`
the kernel statistics give the bpMark / markCount / markPlace split
(tools/rocprof_summary.py).

--plans mark,bitmap runs every semi / anti join twice on the same relations in
this process: on the mark plan (the default) and on the set-semantics bitmap
plan (JoinConfig.semi_bitmap); --materialize 0 makes the joins count-only;
--inner-repeats K draws the inner keys UNIFORM over |R| / K keys (repeats and
gaps; 0 = unique keys as generated).  The lines then carry `plan_choice`,
`materialize` and the device network / local-pass spans as well.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gpu_128m")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", default="inner,semi,anti")
    ap.add_argument("--variants", default="unique,zipf")
    ap.add_argument("--plans", default="mark", help="mark,bitmap: the semi / anti plans to run (same relations)")
    ap.add_argument("--materialize", type=int, default=1, choices=[0, 1])
    ap.add_argument("--inner-repeats", type=int, default=0)
    a = ap.parse_args()

    import torch
    import hpcjoin
    from hpcjoin.models import workloads as W
    C = hpcjoin.require_native()
    assert torch.cuda.is_available(), "bench_semi.py measures the device engine"
    torch.cuda.set_device(0)
    wl = W.get(a.workload, a.scale)
    G_R, G_S = wl.inner_size, wl.outer_size
    ctx = C.ExecContext("device", 0, C.LocalCommunicator())
    for variant in a.variants.split(","):
        inner = C.GenSpec(seed=1234) if a.inner_repeats < 1 else C.GenSpec(
            distribution=C.KeyDistribution.UNIFORM, seed=1234, domain=max(1, G_R // a.inner_repeats))
        outer = C.GenSpec(seed=4321) if variant == "unique" else C.GenSpec(
            distribution=C.KeyDistribution.ZIPF, seed=4321, domain=G_R, zipf_theta=0.75)
        R, S = C.Relation(G_R, G_R, "device", 0), C.Relation(G_S, G_S, "device", 0)
        R.generate(inner, 0)
        S.generate(outer, 0)
        extended = a.plans != "mark" or a.materialize != 1 or a.inner_repeats > 0
        for kind in a.kinds.split(","):
            for plan in a.plans.split(","):
                if plan == "bitmap" and kind == "inner":
                    continue  # the set plan answers semi / anti joins only
                cfg = C.JoinConfig()
                cfg.kind = getattr(C.JoinKind, kind.upper())
                cfg.materialize = bool(a.materialize)
                cfg.semi_bitmap = plan == "bitmap"
                j = C.HashJoin(R, S, ctx, cfg)
                assert j.plan.bitmap_set == (plan == "bitmap"), j.plan
                for _ in range(a.warmup):
                    j.run()
                runs = [j.run() for _ in range(a.steps)]
                res = runs[-1]
                med = lambda k: round(statistics.median(r[k] for r in runs), 3)
                line = {
                    "workload": wl.name, "variant": variant, "kind": kind, "inner": G_R, "outer": G_S,
                    "join_ms": med("join_ms"), "dev_build_probe_ms": med("dev_build_probe_ms"),
                    "dev_span_ms": med("dev_span_ms"),
                    "matches": res["global_matches"], "output_pairs": res["output_pairs"],
                    "output_rids": res["output_rids"], "reruns": res["reruns"], "plan": repr(j.plan)}
                if extended:
                    line.update({"plan_choice": plan, "materialize": a.materialize, "inner_repeats": a.inner_repeats,
                                 "dev_network_ms": med("dev_network_ms"),
                                 "dev_local_partition_ms": med("dev_local_partition_ms"),
                                 "bitmap_join": res["bitmap_join"], "local_fallbacks": res["local_fallbacks"],
                                 "network_fallbacks": res["network_fallbacks"],
                                 "step_join_ms": [round(r["join_ms"], 3) for r in runs]})
                print(json.dumps(line), flush=True)
                del j
                ctx.trim_workspace()
        del R, S


if __name__ == "__main__":
    main()
