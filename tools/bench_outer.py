#!/usr/bin/env python3
"""Left / right / full outer joins against the composition the inner and anti
joins allow, same inputs, one process on one GPU.

    python tools/bench_outer.py [--workload gpu_128m] [--scale 1.0] [--steps 5] [--warmup 2]
                                [--kinds inner,anti,left_outer,right_outer,full_outer] [--variants zipf]

Runs the workload's Zipf-outer variant (theta 0.75 over the inner key domain;
`--variants unique,zipf` adds the workload as generated), each kind with
materialize = True, and prints one JSON line per (variant, kind): join_ms and
the device build/probe span as min / median / max over the timed iterations,
the result counts and the plan.  The last line per variant compares each outer
kind's build/probe span with its baseline, the spans of the joins that would
compose it: INNER + ANTI (left, right; for left the ANTI span stands in for
the inner side's), INNER + 2 x ANTI (full).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _spread(runs, field):
    v = [r[field] for r in runs]
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gpu_128m")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", default="inner,anti,left_outer,right_outer,full_outer")
    ap.add_argument("--variants", default="zipf")
    a = ap.parse_args()

    import torch
    import hpcjoin
    from hpcjoin.models import workloads as W
    C = hpcjoin.require_native()
    assert torch.cuda.is_available(), "bench_outer.py measures the device engine"
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
        spans = {}
        for kind in a.kinds.split(","):
            cfg = C.JoinConfig()
            cfg.kind = getattr(C.JoinKind, kind.upper())
            cfg.materialize = True
            j = C.HashJoin(R, S, ctx, cfg)
            for _ in range(a.warmup):
                j.run()
            runs = [j.run() for _ in range(a.steps)]
            res = runs[-1]
            spans[kind] = _spread(runs, "dev_build_probe_ms")
            print(json.dumps({
                "workload": wl.name, "variant": variant, "kind": kind, "inner": G_R, "outer": G_S,
                "join_ms": _spread(runs, "join_ms"), "dev_build_probe_ms": spans[kind],
                "dev_span_ms": _spread(runs, "dev_span_ms"),
                "matches": res["global_matches"], "matched_pairs": res["matched_pairs"],
                "unmatched_inner": res["unmatched_inner"], "unmatched_outer": res["unmatched_outer"],
                "output_pairs": res["output_pairs"], "output_rids": res["output_rids"], "reruns": res["reruns"],
                "plan": repr(j.plan)}), flush=True)
            del j
            ctx.trim_workspace()
        if "inner" in spans and "anti" in spans:
            cmp = {"workload": wl.name, "variant": variant, "comparison": "dev_build_probe_ms, fused vs composed"}
            for kind, antis in (("left_outer", 1), ("right_outer", 1), ("full_outer", 2)):
                if kind not in spans:
                    continue
                base = {k: round(spans["inner"][k] + antis * spans["anti"][k], 3) for k in ("min", "median", "max")}
                # faster only when even the slowest fused iteration beats the fastest composed one
                cmp[kind] = {"fused": spans[kind], "composed": base, "faster": spans[kind]["max"] < base["min"]}
            print(json.dumps(cmp), flush=True)
        del R, S


if __name__ == "__main__":
    main()
