#!/usr/bin/env python3
"""Semi- and anti-join against the materializing inner join of the same inputs,
in one process on one GPU.

    python tools/bench_semi.py [--workload gpu_128m] [--scale 1.0] [--steps 5] [--warmup 2] [--kinds inner,semi,anti]

Runs the workload as generated (unique outer keys) and its Zipf-outer variant
(theta 0.75 over the inner key domain), each as kind = INNER / SEMI / ANTI with
materialize = True, and prints one JSON line per (variant, kind): median
join_ms, the device build/probe span, the result count and the plan.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_semi.py --kinds semi`
the kernel statistics give the bpMark / markCount / markPlace split
(tools/rocprof_summary.py).
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
        inner = C.GenSpec(seed=1234)
        outer = C.GenSpec(seed=4321) if variant == "unique" else C.GenSpec(
            distribution=C.KeyDistribution.ZIPF, seed=4321, domain=G_R, zipf_theta=0.75)
        R, S = C.Relation(G_R, G_R, "device", 0), C.Relation(G_S, G_S, "device", 0)
        R.generate(inner, 0)
        S.generate(outer, 0)
        for kind in a.kinds.split(","):
            cfg = C.JoinConfig()
            cfg.kind = getattr(C.JoinKind, kind.upper())
            cfg.materialize = True
            j = C.HashJoin(R, S, ctx, cfg)
            for _ in range(a.warmup):
                j.run()
            runs = [j.run() for _ in range(a.steps)]
            res = runs[-1]
            print(json.dumps({
                "workload": wl.name, "variant": variant, "kind": kind, "inner": G_R, "outer": G_S,
                "join_ms": round(statistics.median(r["join_ms"] for r in runs), 3),
                "dev_build_probe_ms": round(statistics.median(r["dev_build_probe_ms"] for r in runs), 3),
                "dev_span_ms": round(statistics.median(r["dev_span_ms"] for r in runs), 3),
                "matches": res["global_matches"], "output_pairs": res["output_pairs"],
                "output_rids": res["output_rids"], "reruns": res["reruns"], "plan": repr(j.plan)}), flush=True)
            del j
            ctx.trim_workspace()
        del R, S


if __name__ == "__main__":
    main()
