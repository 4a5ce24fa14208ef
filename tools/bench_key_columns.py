#!/usr/bin/env python3
"""Key-column relations against tuple relations of the same keys, in one process on one GPU.

    python tools/bench_key_columns.py [--sizes 128e6,1e9] [--keys dense,sparse] [--steps 7] [--warmup 2]

For every size and key kind (dense unique keys: the headline bitmap plan with packed fragments; sparse random
63-bit keys: the general key-only path) three engines are built on the same context: tuple relations (A),
key-column relations over the key column of the same tuples (K), and the tuple configuration a second time (A').
They run alternately, A, K, A', step after step, so that drift hits all three alike and A against A' gives the
run-to-run spread that a difference between A and K has to exceed.  Every count is checked against the oracle.

One JSON line per (size, keys): median join_ms and device span of A, K and A', the medians of the timeline's
histogram (HILOCAL, HOLOCAL), scatter (MIMAINPART, MOMAINPART), local-pass and build/probe spans, how each
engine read its sides (`key_columns`) and whether a key column was expanded.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPANS = ("HILOCAL", "HOLOCAL", "MIMAINPART", "MOMAINPART", "LPPART", "BPTASKTIME")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128e6,1e9")
    ap.add_argument("--keys", default="dense,sparse")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import torch
    import hpcjoin
    C = hpcjoin.require_native()
    assert torch.cuda.is_available(), "bench_key_columns.py measures the device engine"
    torch.cuda.set_device(0)
    ctx = C.ExecContext("device", 0, C.LocalCommunicator())
    for size in a.sizes.split(","):
        G = int(float(size))
        for keys in a.keys.split(","):
            inner, outer = C.GenSpec(seed=1234), C.GenSpec(seed=4321)
            inner.sparse64 = outer.sparse64 = keys == "sparse"
            expected = C.Relation.expected_matches(inner, G, outer, G)
            tR, tS = (C.ops.generate(G, 0, G, s, "cuda") for s in (inner, outer))
            kR, kS = tR[:, 0].contiguous(), tS[:, 0].contiguous()
            rels = {"A": (C.Relation.from_tensor(tR, G), C.Relation.from_tensor(tS, G)),
                    "K": (C.Relation.from_keys(kR, G), C.Relation.from_keys(kS, G)),
                    "A2": (C.Relation.from_tensor(tR, G), C.Relation.from_tensor(tS, G))}
            joins = {k: C.HashJoin(r, s, ctx, C.JoinConfig()) for k, (r, s) in rels.items()}
            runs = {k: [] for k in joins}
            spans = {k: [] for k in joins}
            for step in range(a.warmup + a.steps):
                for k, j in joins.items():
                    res = j.run()
                    assert res["global_matches"] == expected, (k, res["global_matches"], expected)
                    if step >= a.warmup:
                        snap = C.measurements.snapshot()
                        runs[k].append(res)
                        spans[k].append({s: snap[s] for s in SPANS if s in snap})
            med = lambda k, f: round(statistics.median(r[f] for r in runs[k]), 3)
            line = {"size": G, "keys": keys, "matches": expected, "steps": a.steps, "plan": repr(joins["K"].plan)}
            for k in joins:
                line[k] = {"join_ms": med(k, "join_ms"), "dev_span_ms": med(k, "dev_span_ms"),
                           "step_join_ms": [round(r["join_ms"], 3) for r in runs[k]],
                           "key_columns": runs[k][-1]["key_columns"],
                           "spans_us": {s: round(statistics.median(x[s] for x in spans[k]), 1)
                                        for s in SPANS if all(s in x for x in spans[k])}}
            line["K"]["expanded"] = [r.expanded for r in rels["K"]]
            line["AA_spread_ms"] = round(abs(line["A"]["join_ms"] - line["A2"]["join_ms"]), 3)
            line["K_minus_A_ms"] = round(line["K"]["join_ms"] - min(line["A"]["join_ms"], line["A2"]["join_ms"]), 3)
            print(json.dumps(line), flush=True)
            del joins, rels, tR, tS, kR, kS
            ctx.reset_scratch()
            ctx.trim_workspace(0)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
