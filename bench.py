#!/usr/bin/env python3
"""Headline benchmark: distributed radix hash join throughput on MI355X.

BASELINE metric: billion tuples/s (whole node) for a 1B x 1B join of unique
int64 keys on 1/2/4/8 MI355X (strong scaling: the 1B x 1B total is fixed).
One step = one complete join (histogram -> fused all-gather -> LDS scatter +
RCCL all-to-allv -> local radix pass -> LDS build/probe -> match count), the
reference's JTOTAL span (operators/HashJoin.cpp:51,212).  Data generation is
outside the timed region, as in the reference.  Every step's match count is
checked against the exact oracle (|R| for unique keys).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--inner 1e9] [--outer 1e9]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run measures the headline only.  --full adds the secondary
measurements (general_path, scale_model and, at N > 1, shuffle_path), each a
run of its own.  --dump-outputs DIR writes what the last timed join returned
(its match counts) as DIR/matches.npy.
"""
import argparse
import gc
import json
import os
import signal
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
T_START = time.time()
# Multi-GPU runs: the engine's watchdog (every blocking wait on a collective or
# a stream) fires well before the driver's own 600 s limit, so a stuck rank
# ends the run with a message naming its rank, phase, wait site and last
# completed collective instead of a silent kill (HPCJOIN_COMM_TIMEOUT_S
# overrides).  Set before the ranks are spawned: they inherit it.
if int(os.environ.get("WORLD_SIZE", "1")) > 1 or any(a.startswith("--gpus") for a in sys.argv[1:]):
    os.environ.setdefault("HPCJOIN_COMM_TIMEOUT_S", "120")


def _spawn_ranks_if_needed():
    """``python bench.py --gpus N`` without a launcher: start N fresh rank
    processes (one per GPU, torchrun-style env) and exit with their status.

    Runs before torch/HIP are imported, so this process never touches the GPU
    (no exec of a GPU-initialised process).  Rank 0's JSON line reaches
    stdout unchanged (children inherit it); a failing rank makes the whole job
    fail and the other ranks are killed, so nothing hangs in a collective.
    """
    if "WORLD_SIZE" in os.environ:
        return
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gpus", type=int, default=1)
    known, _ = ap.parse_known_args()
    n = known.gpus
    if n <= 1:
        return
    # A free port below the kernel's ephemeral range: an ephemeral one can be
    # handed out again as the local port of the ranks' own outgoing sockets
    # (RCCL bootstrap) before rank 0 binds it (EADDRINUSE).
    import random
    port = 0
    for cand in random.Random(os.getpid()).sample(range(20000, 32000), 200):
        with socket.socket() as s:
            try:
                s.bind(("127.0.0.1", cand))
            except OSError:
                continue
            port = cand
            break
    if not port:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    base = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(n),
                LOCAL_WORLD_SIZE=str(n), HPCJOIN_SPAWNED="1")
    procs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r), GROUP_RANK="0")
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      start_new_session=True))
    def signal_all(sig):
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)
                except ProcessLookupError:
                    pass

    rc, killed_at = 0, None
    pending = set(range(n))
    while pending:
        for r in list(pending):
            code = procs[r].poll()
            if code is None:
                continue
            pending.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py: rank {r} exited with {code}; stopping the other ranks", file=sys.stderr, flush=True)
                signal_all(signal.SIGTERM)
                killed_at = time.time()
        if killed_at is not None and time.time() - killed_at > 15:
            signal_all(signal.SIGKILL)
            killed_at = time.time()
        time.sleep(0.05)
    sys.exit(rc)


if __name__ == "__main__":
    _spawn_ranks_if_needed()
# Host<->device copies of a join are small (plan uploads, cursor and counter
# read-backs): run them as blit kernels on the compute queue, not on the SDMA
# engines.  With SDMA on, about every second process stalled one join (the
# 4th) by 17-45 ms inside the first small copy; with it off 5/5 runs were
# clean (profiles/archive/r1_sdma_outlier.md).  Must be set before HIP initialises.
# Single-process runs only: multi-rank runs keep the runtime default (their
# RCCL rehearsals over the socket transport were measured with SDMA on).
if int(os.environ.get("WORLD_SIZE", "1")) == 1:
    os.environ.setdefault("HSA_ENABLE_SDMA", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import hpcjoin  # noqa: E402
from hpcjoin.parallel import init_distributed, make_context  # noqa: E402


DIST = {"unique": "UNIQUE", "uniform": "UNIFORM", "zipf": "ZIPF", "modulo": "MODULO"}
PHASES = ("histogram_ms", "network_ms", "local_ms", "dev_histogram_ms", "dev_network_ms", "dev_local_partition_ms",
          "dev_build_probe_ms")


def link_prediction(info, plan, results):
    """The plan's own link-traffic prediction (both N > 1 alternatives), so a
    measured multi-GPU step can be checked against what the links allow."""
    if info.world <= 1:
        return None
    gbps = plan.link_gbps
    return {"chosen": "replicated_bitmap" if plan.bitmap_replicated else "shuffle",
            "replicated_bytes_per_rank": int(plan.replicated_link_bytes),
            "shuffle_bytes_per_rank": int(plan.shuffle_link_bytes),
            "link_GBps_per_rank": gbps,
            "predicted_replicated_ms": round(plan.replicated_link_bytes / gbps / 1e6, 3) if gbps else None,
            "predicted_shuffle_ms": round(plan.shuffle_link_bytes / gbps / 1e6, 3) if gbps else None,
            "measured_wire_bytes_rank0": results[-1]["wire_bytes"]}


def scale_model(C, info, ctx, comm, on_gpu, G_R, G_S, specs, cfg, rel_loc, general_cfg_ok):
    """Predicted N = 2/4/8 step times of the three N > 1 paths, from one
    GPU: a rank's kernel work at N is measured directly as the same join on
    its share (G/N x G/N tuples); the link bytes per rank follow from the
    wire format the planner picks at that N (HashJoin.codec_pays: packed
    w-bit words when the link time saved exceeds the codec's extra passes,
    else raw 8-byte words gathered from the claim slices); the codec (pack +
    unpack) or gather passes cost their measured rates.
      value      replicated bitmaps: all-reduce of 2 (N-1)/N x 2^keyBits / 8 B
      shuffle    hash-partition shuffle of the dense keys: w = keyBits - net bits
      general    the same shuffle of 63-bit keys (key-only words, w = 53)
    Overlap (the chunked pipeline, chunks = 4 at N > 1): chunk k's exchange
    runs while chunk k + 1 is scattered and, for the outer relation, while
    chunk k - 1 is local-partitioned and probed, so a step is bounded by
      compute = rank share + codec/gather passes, and
      links   = first chunk's scatter + link time + last chunk's local work,
    predicted = max(compute, links).  The driver's SCALE run is the
    measurement this is checked against."""
    if info.world != 1 or not on_gpu:
        return None
    import math
    from hpcjoin.utils import config_from_dict
    per_peer = cfg.link_gbps_per_peer if cfg.link_gbps_per_peer > 0 else 64.0
    extra_ps = cfg.codec_extra_ps_per_tuple
    # pass rates (ms per tuple), 64M tuples: pack + unpack at the two codec
    # widths, and the raw gather (a 64-bit "pack" is a copy of the runs)
    raw = torch.randint(0, 1 << 62, (1 << 26,), dtype=torch.int64, device="cuda")
    codec = {}
    for w in (20, 53):
        r = C.ops.bench_wire(raw, w, 0, 0, 5)
        codec[w] = (r["pack_ms"] + r["unpack_ms"]) / raw.numel()
    gather = C.ops.bench_wire(raw, 64, 0, 0, 5)["pack_ms"] / raw.numel()
    del raw
    torch.cuda.empty_cache()
    key_bits = max(1, math.ceil(math.log2(max(G_R, 2))))
    chunks = 4
    out = {"link_GBps_per_peer": per_peer, "codec_extra_ps_per_tuple": extra_ps, "chunks": chunks,
           "source": "measured per-rank share on one GPU + codec / gather rates + link model + chunk pipeline",
           "paths": {}}
    for path in ("value", "shuffle", "general"):
        if path == "general" and not general_cfg_ok:
            continue
        rows = []
        for N in (2, 4, 8):
            gr, gs = G_R // N, G_S // N
            c = config_from_dict({}) if path != "shuffle" else config_from_dict({"bitmap_join": False})
            c.chunks = 1
            m = measure(C, info, ctx, comm, on_gpu, gr, gs, *specs(path == "general"), c, rel_loc, 3, 1)
            m.pop("join"), m.pop("results")
            ctx.reset_scratch()
            link_gbps = per_peer * min(N - 1, 7)
            share = (N - 1) / N
            net_ms = m["phases_ms"]["dev_network_ms"]
            if path == "value":
                link_bytes = 2 * share * (1 << key_bits) / 8
                codec_ms, wire = 0.0, "bitmap all-reduce"
                # ranges of the all-reduce overlap the outer scatter (half the network pass)
                pred_links = net_ms / 2 + link_bytes / link_gbps / 1e6
            else:
                w = (key_bits - 10) if path == "shuffle" else 53
                packed = C.HashJoin.codec_pays(w, N, per_peer, extra_ps)
                bits = w if packed else 64
                link_bytes = share * (gr + gs) * bits / 8
                codec_ms = share * (gr + gs) * (codec[20 if path == "shuffle" else 53] if packed else gather)
                wire = f"packed {w}-bit" if packed else "raw 64-bit (gathered runs, no unpack)"
                rest = max(0.0, m["ms_per_step"] - net_ms)
                pred_links = net_ms / (2 * chunks) + link_bytes / link_gbps / 1e6 + rest / chunks
            link_ms = link_bytes / link_gbps / 1e6
            pred = max(m["ms_per_step"] + codec_ms, pred_links)
            rows.append({"n_gpus": N, "rank_share_ms": m["ms_per_step"], "wire": wire, "codec_ms": round(codec_ms, 3),
                         "link_bytes_per_rank": int(link_bytes), "link_ms": round(link_ms, 3),
                         "compute_bound_ms": round(m["ms_per_step"] + codec_ms, 3),
                         "link_bound_ms": round(pred_links, 3), "predicted_ms": round(pred, 3),
                         "predicted_value": round((G_R + G_S) / pred / 1e6, 2), "rank_share_correct": m["correct"]})
        out["paths"][path] = rows
    return out


def rccl_debug_env(info):
    """Ask RCCL to log its transport choices to a per-rank file (not stdout:
    rank 0 prints one JSON line; this overrides an inherited NCCL_DEBUG level,
    HPCJOIN_RCCL_LOG=0 keeps it).  Must run before any RCCL communicator exists."""
    if info.world <= 1 or os.environ.get("HPCJOIN_RCCL_LOG") == "0":
        return None
    import tempfile
    path = os.path.join(tempfile.gettempdir(), f"hpcjoin_rccl.{os.getpid()}.log")
    os.environ["NCCL_DEBUG"] = "INFO"
    os.environ["NCCL_DEBUG_SUBSYS"] = "INIT,P2P,SHM,NET"
    os.environ["NCCL_DEBUG_FILE"] = path
    return path


def rccl_transports(path):
    """Counts of RCCL channel connections by transport in this rank's log."""
    out = {"P2P": 0, "SHM": 0, "NET": 0}
    if not path or not os.path.exists(path):
        return {"log": None}
    with open(path, errors="replace") as f:
        for line in f:
            if " via " not in line:
                continue
            for k in out:
                if f"via {k}" in line:
                    out[k] += 1
    try:
        os.unlink(path)
    except OSError:
        pass
    return out


def topology(C, info, on_gpu):
    """Per-rank device identity (ordinal, PCI bus id, host), gathered on every
    rank.  Two ranks on one device of one host are refused unless the run is
    an explicit shared-GPU rehearsal (HPCJOIN_SHARE_GPU=1)."""
    me = {"rank": info.rank, "local_rank": info.local_rank, "host": socket.gethostname()}
    if on_gpu:
        d = C.device_info(torch.cuda.current_device())
        me.update(device=d["device"], pci_bus_id=d["pci_bus_id"], arch=d["arch"], compute_units=d["compute_units"],
                  visible_devices=d["visible_devices"])
    ranks = [me]
    if info.world > 1:
        ranks = [None] * info.world
        dist.all_gather_object(ranks, me)
    seen = {}
    for r in ranks:
        key = (r["host"], r.get("pci_bus_id"))
        if on_gpu and key in seen and os.environ.get("HPCJOIN_SHARE_GPU") != "1":
            raise SystemExit(f"bench.py: ranks {seen[key]} and {r['rank']} share device {key[1]} on {key[0]}; "
                             "one rank per GPU (set HPCJOIN_SHARE_GPU=1 only for a shared-GPU rehearsal)")
        seen.setdefault(key, r["rank"])
    return {"ranks": ranks, "distinct_devices": len(seen), "shared_gpu_rehearsal": os.environ.get("HPCJOIN_SHARE_GPU") == "1"}


def calibrate_links(comm, info, on_gpu, mb_per_peer=256, iters=5):
    """Measured link bandwidth for the plan's link model: an RCCL all-to-allv
    on the engine's own communicator (each rank sends mb_per_peer MiB to every
    peer) and a torch.distributed RCCL all-reduce of 128 MiB."""
    if info.world <= 1 or not on_gpu:
        return None
    n = info.world
    words = (mb_per_peer << 20) // 8
    send = torch.ones(words * n, dtype=torch.int64, device="cuda")
    recv = torch.empty_like(send)
    counts = [words] * n
    for _ in range(2):
        comm.all_to_all_v(send, counts, recv, counts)
    comm.barrier()
    t0 = time.perf_counter()
    for _ in range(iters):
        comm.all_to_all_v(send, counts, recv, counts)
    t_a2a = (time.perf_counter() - t0) / iters
    red = torch.ones((128 << 20) // 4, dtype=torch.float32, device="cuda")
    for _ in range(2):
        dist.all_reduce(red)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        dist.all_reduce(red)
    torch.cuda.synchronize()
    t_ar = (time.perf_counter() - t0) / iters
    mine = [int(t_a2a * 1e9), int(t_ar * 1e9)]
    allv = comm.all_gather(mine)
    t_a2a, t_ar = max(allv[0::2]) / 1e9, max(allv[1::2]) / 1e9
    peer_bytes = words * 8
    del send, recv, red
    torch.cuda.empty_cache()
    return {"source": f"measured: RCCL all-to-allv of {mb_per_peer} MiB per peer on the engine communicator, "
                      f"torch.distributed all-reduce of 128 MiB, {iters} iterations each (max over ranks)",
            "all_to_all_GBps_per_peer": round(peer_bytes / t_a2a / 1e9, 2),
            "all_to_all_GBps_per_rank": round((n - 1) * peer_bytes / t_a2a / 1e9, 2),
            "all_reduce_busbw_GBps": round(2 * (n - 1) / n * (128 << 20) / t_ar / 1e9, 2),
            "all_to_all_ms": round(t_a2a * 1e3, 3), "all_reduce_ms": round(t_ar * 1e3, 3)}


def measure(C, info, ctx, comm, on_gpu, G_R, G_S, inner, outer, cfg, rel_loc, steps, warmup):
    """Generate this rank's slices, build the join (timed with its first run:
    the cold-join cost incl. planning), warm up, then time `steps` joins
    between barriers; the max over ranks is the step time."""
    lr, ls = (C.Relation.local_size_for(G, info.rank, info.world) for G in (G_R, G_S))
    R = C.Relation(lr, G_R, rel_loc, info.local_rank)
    S = C.Relation(ls, G_S, rel_loc, info.local_rank)
    R.generate(inner, C.Relation.local_offset_for(G_R, info.rank, info.world))
    S.generate(outer, C.Relation.local_offset_for(G_S, info.rank, info.world))
    expected = C.Relation.expected_matches(inner, G_R, outer, G_S)

    def barrier():
        if info.world > 1:
            comm.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    barrier()
    # Construction plans the join and grows the engine's workspace to the
    # plan's estimate (pages touched once): reported as setup_ms.  The first
    # run() after it is the cold join (first kernel launches, first use of the
    # arena): first_join_ms.
    t0 = time.perf_counter()
    join = C.HashJoin(R, S, ctx, cfg)
    barrier()
    setup_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    first = join.run()
    barrier()
    first_ms = (time.perf_counter() - t0) * 1e3
    if os.environ.get("HPCJOIN_TRACE_FIRST") == "1":
        keys = ("join_ms", "setup_ms", "teardown_ms") + PHASES
        print(json.dumps({"first_join": {k: round(first[k], 3) for k in keys if k in first},
                          "setup_ms": round(setup_ms, 3), "first_ms": round(first_ms, 3)}),
              file=sys.stderr, flush=True)
    # If the first join still spilled past the reserved workspace, the arena
    # adds a chunk for it here (never inside a timed join).
    ctx.reset_scratch()
    # No Python garbage collection inside the timed joins (host noise only:
    # the joins allocate nothing the collector tracks beyond their result dicts).
    # Collected before the last warmup joins, so the GPU goes from them straight
    # into the timed ones (a collection between them left it idle for tens of
    # ms, and the first timed join ran ~5 % slower).
    gc.collect()
    gc.disable()
    try:
        for _ in range(max(0, warmup - 1)):
            join.run()
        barrier()
        results = []
        t0 = time.perf_counter()
        for _ in range(steps):
            results.append(join.run())
        barrier()
        elapsed = time.perf_counter() - t0
    finally:
        gc.enable()
    mine = [int(elapsed * 1e9), int(first_ms * 1e6), int(setup_ms * 1e6), int(join.plan_ms * 1e6)]
    plan_ms = join.plan_ms
    if info.world > 1:
        allv = comm.all_gather(mine)
        elapsed, first_ms, setup_ms = max(allv[0::4]) / 1e9, max(allv[1::4]) / 1e6, max(allv[2::4]) / 1e6
        plan_ms = max(allv[3::4]) / 1e6
    ms = elapsed * 1e3 / steps
    out = {
        "ms_per_step": round(ms, 3),
        "value": round((G_R + G_S) * steps / elapsed / 1e9, 4),
        "first_join_ms": round(first_ms, 3),
        "setup_ms": round(setup_ms, 3),
        "plan_ms": round(plan_ms, 3),
        "workspace_reserved_GB": round(join.reserved_bytes / 1e9, 2),
        "matches": results[-1]["global_matches"],
        "expected_matches": expected,
        "correct": all(r["global_matches"] == expected for r in [first] + results) if expected is not None else None,
        "plan": repr(join.plan),
        "sampled_network": bool(results[-1]["sampled_network"]),
        "network_fallbacks": sum(r["network_fallbacks"] for r in [first] + results),
        # two-level plans: network windows (N > 1: send buffers) with round-interleaved slices
        "round_windows": results[-1].get("round_windows", 0),
        "phases_ms": {k: round(sum(r[k] for r in results) / len(results), 3) for k in PHASES},
        "results": results,
        "join": join,
    }
    del R, S
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=float, default=1e9)
    ap.add_argument("--outer", type=float, default=1e9)
    ap.add_argument("--dist", default="unique", choices=list(DIST))
    ap.add_argument("--theta", type=float, default=0.75)
    ap.add_argument("--chunks", type=int, default=0, help="exchange pipeline slices (0 = auto)")
    ap.add_argument("--input", default="device", choices=["device", "pinned"],
                    help="where the relations live: HBM, or pinned host memory read in place over the host link")
    ap.add_argument("--general", default="on", choices=["on", "off", "only"],
                    help="with --full, also time the general path: the same join on sparse random 63-bit keys "
                         "(only: the headline itself runs on those keys, for sweeps)")
    ap.add_argument("--scale-model", default="on", choices=["on", "off"],
                    help="with --full, N = 1 only: predicted N = 2/4/8 step times of the three N > 1 paths "
                         "(scale_model)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (shuffle_path, general_path, scale_model); a plain "
                         "run times the headline join only")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed join returned as DIR/matches.npy "
                         "(float64: global_matches, local_matches, output_pairs of rank 0)")
    ap.add_argument("--json-out", default="")
    ap.add_argument("--budget-s", type=float, default=float(os.environ.get("HPCJOIN_BENCH_BUDGET_S", "420")),
                    help="wall budget of the whole run: the secondary measurements (shuffle_path, general_path, "
                         "scale_model) are skipped once half of it is spent, so the headline line is always printed "
                         "inside the driver's limit")
    args = ap.parse_args()

    C = hpcjoin.require_native()
    from hpcjoin.parallel import DistInfo
    rccl_log = rccl_debug_env(DistInfo(world=int(os.environ.get("WORLD_SIZE", "1"))))
    info = init_distributed()
    if info.world != args.gpus and not (args.gpus == 1 and info.world == 1):
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={info.world}")
    on_gpu = torch.cuda.is_available()
    loc = "device" if on_gpu else "host"
    topo = topology(C, info, on_gpu)
    ctx, comm = make_context(info, loc)
    topo["communicator"] = {"name": comm.name(), "size": comm.size()}
    calib = calibrate_links(comm, info, on_gpu)

    G_R, G_S = int(args.inner), int(args.outer)
    if not on_gpu:  # CPU fallback for plumbing only: keep it small
        G_R, G_S = min(G_R, 1 << 20), min(G_S, 1 << 20)
    rel_loc = "pinned" if on_gpu and args.input == "pinned" else loc

    from hpcjoin.utils import config_from_dict  # HPCJOIN_<FIELD> env overrides (sweeps)
    cfg = config_from_dict({})
    if args.chunks > 0:
        cfg.chunks = args.chunks
    elif "HPCJOIN_CHUNKS" not in os.environ:
        cfg.chunks = 1 if info.world == 1 else 4
    if calib:
        cfg.link_gbps_per_peer = calib["all_to_all_GBps_per_peer"]

    def specs(sparse):
        inner = C.GenSpec(distribution=C.KeyDistribution.UNIQUE, seed=1234)
        outer = C.GenSpec(distribution=getattr(C.KeyDistribution, DIST[args.dist]), seed=4321,
                          domain=0 if args.dist == "unique" else G_R, zipf_theta=args.theta)
        inner.sparse64 = outer.sparse64 = sparse
        return inner, outer

    head = measure(C, info, ctx, comm, on_gpu, G_R, G_S, *specs(args.general == "only"), cfg, rel_loc, args.steps,
                   args.warmup)
    join, results = head.pop("join"), head.pop("results")
    if args.dump_outputs and info.rank == 0:
        # What a caller of HashJoin.run() receives from the last timed join:
        # its match counts (exact in float64 up to 2^53).
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        last = results[-1]
        np.save(os.path.join(args.dump_outputs, "matches.npy"),
                np.array([last["global_matches"], last["local_matches"], last["output_pairs"]], dtype=np.float64))
    plan = join.plan
    engine = {"reruns": results[-1]["reruns"], "build_probe_items": results[-1]["build_probe_items"],
              "network_fallbacks": sum(r["network_fallbacks"] for r in results),
              "local_fallbacks": sum(r["local_fallbacks"] for r in results),
              "wire_bytes": results[-1]["wire_bytes"],
              "local_items": results[-1]["local_items"], "workspace_GB": round(ctx.workspace_capacity() / 1e9, 2),
              "workspace_peak_GB": round(ctx.workspace_peak() / 1e9, 2),
              "step_ms": [round(r["join_ms"], 2) for r in results],
              # Per step: device span (first -> last event of the join) and
              # what the host added around it (join_ms - dev_span_ms), split
              # into enqueue (start -> last kernel enqueued) and the wait for
              # the result after it.  A stall shows as a large host gap with
              # an unchanged device span.
              "step_dev_span_ms": [round(r["dev_span_ms"], 3) for r in results],
              "step_host_gap_ms": [round(r["join_ms"] - r["dev_span_ms"], 3) for r in results],
              "step_enqueue_ms": [round(r["enqueue_ms"], 3) for r in results],
              "step_host_wait_ms": [round(r["host_wait_ms"], 3) for r in results],
              "step_phases_ms": [[round(r[k], 2) for k in PHASES] for r in results]}
    links = link_prediction(info, plan, results)
    if links is not None:
        links["bandwidth"] = calib or {"source": "model: 64 GB/s per peer (no calibration run)"}
    del join
    ctx.reset_scratch()

    def budget_left(what):
        """True while less than half the wall budget is spent (same answer on
        every rank: rank 0's clock decides)."""
        spent = time.time() - T_START
        ok = spent < 0.5 * args.budget_s
        if info.world > 1:
            ok = bool(comm.all_gather([int(ok)])[0])
        if not ok:
            skipped[what] = f"wall budget: {spent:.0f} s of {args.budget_s:.0f} s spent before it"
        return ok

    skipped = {}
    shuffle = None
    comm_ok = True
    if args.full and info.world > 1 and plan.bitmap_replicated and budget_left("shuffle_path"):
        # The reference's own N > 1 algorithm on the headline workload: hash-
        # partition shuffle (claim scatter + chunked RCCL all-to-allv, the
        # MPI_Put analog) instead of the replicated bitmaps the planner prefers.
        try:
            cfg_sh = config_from_dict({"replicate_bitmap": "OFF"})
            cfg_sh.chunks = cfg.chunks
            cfg_sh.link_gbps_per_peer = cfg.link_gbps_per_peer
            sh = measure(C, info, ctx, comm, on_gpu, G_R, G_S, *specs(args.general == "only"), cfg_sh, rel_loc,
                         max(2, args.steps // 2), max(1, args.warmup))
            sj, sres = sh.pop("join"), sh.pop("results")
            sh["links"] = link_prediction(info, sj.plan, sres)
            sh["wire_bytes_rank0"] = sres[-1]["wire_bytes"]
            sh["received_tuples_rank0"] = [sres[-1]["inner_received"], sres[-1]["outer_received"]]
            del sj
            shuffle = {"data": "same relations as the headline, plan forced to the hash-partition shuffle (the "
                               "reference's N > 1 algorithm: the radix-join scaling curve)", **sh}
            ctx.reset_scratch()
        except Exception as e:  # noqa: BLE001
            shuffle = {"error": f"{type(e).__name__}: {e}"[:500], "correct": False}
            comm_ok = False
            print(f"bench.py: shuffle path failed on rank {info.rank}: {e}", file=sys.stderr, flush=True)

    general = None
    if (args.full and args.general == "on" and args.dist in ("unique", "uniform", "zipf") and comm_ok
            and budget_left("general_path")):
        # The secondary measurement must not cost the headline line: a failure
        # here (the engine aborts the communicator on every rank) is reported
        # in general_path and the headline is still printed.
        try:
            g = measure(C, info, ctx, comm, on_gpu, G_R, G_S, *specs(True), cfg, rel_loc,
                        max(2, args.steps // 2), max(1, args.warmup))
            gj, gres = g.pop("join"), g.pop("results")
            g["links"] = link_prediction(info, gj.plan, gres)
            del gj
            general = {"data": "synthetic: unique random 63-bit keys (a fixed bijection of 0..G-1 over [0, 2^63)), "
                               "same join, generated on device",
                       **g}
            ctx.reset_scratch()
        except Exception as e:  # noqa: BLE001
            general = {"error": f"{type(e).__name__}: {e}"[:500], "correct": False}
            comm_ok = info.world == 1
            print(f"bench.py: general path failed on rank {info.rank}: {e}", file=sys.stderr, flush=True)

    model = None
    if (args.full and args.scale_model == "on" and info.world == 1 and on_gpu and args.dist == "unique" and comm_ok
            and budget_left("scale_model")):
        try:
            model = scale_model(C, info, ctx, comm, on_gpu, G_R, G_S, specs, cfg, rel_loc, args.general != "off")
        except Exception as e:  # noqa: BLE001
            model = {"error": f"{type(e).__name__}: {e}"[:500]}
            print(f"bench.py: scale model failed: {e}", file=sys.stderr, flush=True)

    correct = head["correct"] is not False
    if info.world > 1:
        tr = [None] * info.world
        dist.all_gather_object(tr, rccl_transports(rccl_log))
        topo["rccl_transports"] = tr
    if info.rank == 0:
        line = {
            "metric": "billion tuples/sec (whole node), 1B x 1B uniform int64 keys, 1/2/4/8 MI355X",
            "value": head["value"],
            "unit": "billion tuples/s",
            "n_gpus": info.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"],
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "int64 keys (u32 key fragments / 8-byte CompressedTuples after the network pass)",
            "data": "synthetic: unique int64 keys 0..G-1 in a keyed pseudo-random order (the reference generator, "
                    "Relation.cpp:63-97), generated on device",
            "config": {
                "model": f"distributed radix hash join, {args.dist} keys, |R|={G_R}, |S|={G_S}",
                "global_batch": G_R + G_S,
                "seq_len": 1,
                "parallelism": (f"{'replicated bitmap' if plan.bitmap_replicated else 'hash-partition shuffle'} "
                                f"x{info.world} (RCCL over xGMI)") if info.world > 1 else "single MI355X",
                "plan": head["plan"],
                "chunks": cfg.chunks,
                "input": rel_loc,
            },
            "value_note": ("N > 1: `value` is the planner's choice for this workload, replicated LDS bitmaps (one "
                           "all-reduce of the inner key bitmap, each rank probes its own outer slice) -- not the "
                           "reference's radix shuffle; `shuffle_path` is the same join through the hash-partition "
                           "shuffle (the radix-join scaling curve) and `general_path` the random 63-bit key join"
                           if info.world > 1 and plan.bitmap_replicated else
                           "N = 1: single-level LDS bitmap join over the claim-scatter partitions (no exchange); "
                           "`general_path` is the two-level radix hash join on random 63-bit keys"
                           if plan.bitmap_join else "two-level radix hash join"),
            "first_join_ms": head["first_join_ms"],
            "setup_ms": head["setup_ms"],
            "plan_ms": head["plan_ms"],
            "matches": head["matches"],
            "expected_matches": head["expected_matches"],
            "correct": head["correct"],
            "phases_ms": head["phases_ms"],
            "links": links,
            "shuffle_path": shuffle,
            "general_path": general,
            "scale_model": model,
            "engine": engine,
            "full": args.full,
            "skipped": skipped or None,
            "wall_s": round(time.time() - T_START, 1),
            "comm_timeout_s": float(os.environ.get("HPCJOIN_COMM_TIMEOUT_S", "600")),
            "topology": topo,
            "device": torch.cuda.get_device_name(0) if on_gpu else "cpu",
        }
        print(json.dumps(line), flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                json.dump(line, f, indent=1)
    # Deterministic teardown: engine objects (HIP streams, arenas, the RCCL
    # communicator) go before torch.distributed and before interpreter exit.
    del ctx
    if on_gpu:
        torch.cuda.synchronize()
    if info.world > 1 and comm_ok:
        comm.barrier()
    del comm
    if info.world > 1 and comm_ok:
        dist.barrier()
        dist.destroy_process_group()
    if not correct:
        sys.exit(3)
    if general is not None and general.get("correct") is False:  # reported in general_path; the headline stands
        print("bench.py: general path incorrect or failed (see general_path)", file=sys.stderr, flush=True)


def run_rank():
    """Multi-rank runs: a failing rank (watchdog, RCCL error, wrong result)
    prints its message and exits non-zero at once, without the teardown that
    would wait on peers stuck in a collective; the launcher (bench.py's own
    spawner or torchrun) then stops the other ranks."""
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        main()
        return
    try:
        main()
    except SystemExit:
        raise
    except BaseException as e:  # noqa: BLE001
        print(f"bench.py: rank {os.environ.get('RANK', '?')} failed after {time.time() - T_START:.1f} s: "
              f"{type(e).__name__}: {e}", file=sys.stderr, flush=True)
        os._exit(4)


if __name__ == "__main__":
    run_rank()
