"""Every count-only plan, end to end, with inner key sets that leave gaps.

Inner sets: unique keys of [0, D) chosen by helpers.inner_keys -- a random half,
one bit of every bitmap word, one word in three, the even network partitions,
one piece of a 21-bit fragment range, a few boundary fragments, a single key --
each probed by its complement (count 0: any false positive shows), by itself
permuted (count |R|: any false negative shows) and by uniform draws with
repeats (count from ref_join_count).  A key is (fragment << network_bits) |
digit, so every test sets network_bits and checks that the plan kept it.

A dense inner side (a permutation of 0..G-1) cannot test a probe: it sets every
bit of every partition's bitmap and every slot of a direct-addressed count table
to exactly 1, so a probe that reads the wrong bit, word, piece, 16-bit lane,
partition or all-reduce range still finds a 1 and counts |S|, like a correct
one.  test_bitmap_kernels.py::test_selective_inputs_are_sharp shows that these
sets do tell such probes apart.

Structured patterns run with key_hashing = OFF (AUTO may mix their skewed low
bits away); one `half` case runs with key_hashing = ON.
"""
import functools

import numpy as np
import pytest
import torch

import helpers as H
from conftest import devices
from test_bitmap_plans import run_ranks


@functools.lru_cache(maxsize=None)
def case(pattern, kind, D, nb, n=0):
    """(inner keys, outer keys, exact count), computed once per session and never written to."""
    inner = H.inner_keys(pattern, D, nb)
    outer = H.outer_keys(kind, inner, D, n)
    ref = H.ref_join_count(torch.from_numpy(inner), torch.from_numpy(outer))
    if kind == "complement":
        assert ref == int(D - 1 in inner)
    if kind == "same":
        assert ref == inner.size
    inner.setflags(write=False)
    outer.setflags(write=False)
    return inner, outer, ref


def context(C, dev):
    loc = "device" if dev == "cuda" else "host"
    return C.ExecContext(loc, 0 if loc == "device" else -1, C.LocalCommunicator())


def relation(C, dev, keys, G=None):
    return C.Relation.from_tensor(H.key_tuples(keys, dev), G or len(keys))


def bitmap_cfg(C, nb, hist="EXACT", hashing="OFF"):
    cfg = C.JoinConfig()
    cfg.network_bits = nb
    cfg.key_hashing = getattr(C.KeyHashing, hashing)
    cfg.network_histogram = getattr(C.HistogramMode, hist)
    cfg.replicate_bitmap = C.PlanChoice.ON  # the host path takes the bitmap plan only when forced
    return cfg


def run_bitmap(C, dev, inner, outer, ref, cfg, nb, sampled=False):
    """One N = 1 bitmap join, twice; the plan under test really ran."""
    j = C.HashJoin(relation(C, dev, inner), relation(C, dev, outer), context(C, dev), cfg)
    key_bits = max(int(inner.max()), int(outer.max())).bit_length()
    p = j.plan
    assert p.bitmap_join and not p.bitmap_replicated and p.network_bits == nb, p
    assert p.key_bits == key_bits and p.bitmap_bits == max(key_bits - nb, 0), p
    assert p.sampled_network == sampled
    assert p.key_mix == (cfg.key_hashing == C.KeyHashing.ON)
    res = None
    for _ in range(2):
        res = j.run()
        assert res["global_matches"] == ref, (res["global_matches"], ref)
        assert res["bitmap_join"] and res["local_fallbacks"] == 0
        if not sampled:
            assert res["network_fallbacks"] == 0
    return res, j


# ---- bitmap plan, N = 1 ---------------------------------------------------------
D1, NB1 = 1 << 20, 10  # 1024 partitions of 2^10 fragments: 32 bitmap words each


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("kind", H.OUTER_KINDS)
@pytest.mark.parametrize("pattern", H.INNER_PATTERNS)
def test_bitmap_plan_selective(C, dev, pattern, kind):
    """Every pattern x every outer side on the single-level bitmap plan with exact slices."""
    inner, outer, ref = case(pattern, kind, D1, NB1)
    run_bitmap(C, dev, inner, outer, ref, bitmap_cfg(C, NB1), NB1)


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("kind", H.OUTER_KINDS)
def test_bitmap_plan_selective_mixed_keys(C, dev, kind):
    """key_hashing = ON: the bitmaps are indexed by the mixed key's fragment; a random half stays selective."""
    inner, outer, ref = case("half", kind, D1, NB1)
    run_bitmap(C, dev, inner, outer, ref, bitmap_cfg(C, NB1, hashing="ON"), NB1)


@pytest.mark.gpu
@pytest.mark.parametrize("round_lp", [9, 0])
@pytest.mark.parametrize("kind", H.OUTER_KINDS)
def test_bitmap_plan_selective_sampled(C, cuda, kind, round_lp):
    """Sampled claim slices (the production path), round-interleaved and linear windows."""
    inner, outer, ref = case("half", kind, D1, NB1)
    cfg = bitmap_cfg(C, NB1, hist="SAMPLED")
    cfg.round_lp = round_lp
    run_bitmap(C, "cuda", inner, outer, ref, cfg, NB1, sampled=True)


@pytest.mark.gpu
@pytest.mark.parametrize("threads,flat", [(256, 0), (256, 1), (1024, 0), (1024, 1)])
@pytest.mark.parametrize("pattern", ["half", "even_partitions"])
def test_bitmap_plan_selective_walks(C, cuda, pattern, threads, flat):
    """Both workgroup sizes x both slice walks of the fused kernel."""
    for kind in ("complement", "uniform"):
        inner, outer, ref = case(pattern, kind, D1, NB1)
        cfg = bitmap_cfg(C, NB1)
        cfg.bm_threads, cfg.bm_flat = threads, flat
        run_bitmap(C, "cuda", inner, outer, ref, cfg, NB1)


D21, NB21 = 1 << 22, 1  # 2 partitions of 2^21 fragments: two 128 KiB pieces each


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("kind", H.OUTER_KINDS)
@pytest.mark.parametrize("pattern", H.PIECE_PATTERNS)
def test_bitmap_plan_selective_split_pieces(C, dev, pattern, kind):
    """21 fragment bits: a partition is joined by two workgroups, each with one piece of the range.  With
    only one piece populated, a workgroup that reads the other piece's bits counts wrongly.  (`same` over
    low_piece has 21-bit keys: one piece, the plan says so.)"""
    inner, outer, ref = case(pattern, kind, D21, NB21)
    res, j = run_bitmap(C, dev, inner, outer, ref, bitmap_cfg(C, NB21), NB21)
    assert j.plan.bitmap_bits == (20 if (pattern, kind) == ("low_piece", "same") else 21)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["half", "even_partitions"])
def test_bitmap_plan_selective_group_spill(C, cuda, pattern):
    """Partition-group spill (workspace_budget below the estimate): a group pass joins at most 512 network
    partitions, so 2^20 keys over 1024 partitions is the smallest set with two passes.  even_partitions:
    every other partition of a group has an empty inner side beside a full outer one."""
    inner, outer, ref = case(pattern, "uniform", D1, NB1)
    ctx = context(C, "cuda")
    R, S = relation(C, "cuda", inner), relation(C, "cuda", outer)
    est = C.HashJoin(R, S, ctx, bitmap_cfg(C, NB1, hist="AUTO")).workspace_estimate()
    cfg = bitmap_cfg(C, NB1, hist="AUTO")
    cfg.workspace_budget = est // 2
    j = C.HashJoin(R, S, ctx, cfg)
    assert j.plan.bitmap_join and j.plan.network_bits == NB1 and j.plan.bitmap_bits == 10
    for _ in range(2):
        res = j.run()
        assert res["global_matches"] == ref and res["bitmap_join"] and res["local_fallbacks"] == 0
        assert res["group_passes"] >= 2, (res["group_passes"], est)


# ---- replicated bitmaps, in-process ranks -----------------------------------------
def rank_of_inner(keys, nb, n):
    """Rank of every inner key: the upper half of the partitions belongs to rank digit % n alone (the other
    ranks hold no key of such a partition), the lower half is assembled from all ranks."""
    F = 1 << nb
    digit, frag = keys & (F - 1), keys >> nb
    return np.where(digit >= F // 2, digit % n, (digit + (frag >> 3)) % n)


def rank_relations(C, dev, keys, rank, n):
    tdev = "cuda" if dev == "cuda" else "cpu"
    rid0 = np.concatenate([[0], np.cumsum(np.bincount(rank, minlength=n))])
    return lambda r: C.Relation.from_tensor(H.key_tuples(keys[rank == r], tdev, int(rid0[r])), len(keys))


@pytest.mark.parametrize("dev", devices())
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("pattern", ["half", "even_partitions"])
def test_replicated_bitmap_selective(C, dev, pattern, n_ranks, chunks):
    """Every rank builds the bitmaps of its own inner keys (none at all for some partitions), the all-reduce
    in 1 or 3 partition ranges assembles them, every rank probes its own outer keys: global count and the
    sum of the ranks' local counts equal the reference."""
    loc = "device" if dev == "cuda" else "host"

    def cfg(c):
        c.replicate_bitmap = C.PlanChoice.ON
        c.network_bits = NB1
        c.key_hashing = C.KeyHashing.OFF
        c.network_histogram = C.HistogramMode.EXACT
        c.reduce_chunks = chunks

    for kind in ("uniform", "complement"):
        inner, outer, ref = case(pattern, kind, D1, NB1)
        r_rank = rank_of_inner(inner, NB1, n_ranks)
        assert all((np.bincount(inner[r_rank == r] & 1023, minlength=1024) == 0).any() for r in range(n_ranks))
        s_rank = np.arange(outer.size) * n_ranks // outer.size
        out = run_ranks(C, n_ranks, loc, rank_relations(C, dev, inner, r_rank, n_ranks),
                        rank_relations(C, dev, outer, s_rank, n_ranks), inner.size, outer.size, cfg)
        for res_list, plan in out:
            assert plan.bitmap_join and plan.bitmap_replicated and plan.network_bits == NB1 and plan.bitmap_bits == 10
            assert not plan.sampled_network and not plan.key_mix
            for res in res_list:
                assert res["bitmap_join"] and res["global_matches"] == ref, (kind, res["global_matches"], ref)
                assert res["local_fallbacks"] == 0 and res["network_fallbacks"] == 0
        for run in (0, 1):
            assert sum(o[0][run]["local_matches"] for o in out) == ref


@pytest.mark.parametrize("dev", devices())
def test_replicated_bitmap_sparse_cross_rank_duplicate(C, dev):
    """A key held by two ranks of a sparse inner side (one bit per word): the all-reduced sum carries into
    the clear neighbouring bit instead of a set one, so no further carry hides it.  The set-bit count
    still falls short of |R|, and the join falls back with the exact count."""
    loc = "device" if dev == "cuda" else "host"
    inner, outer, _ = case("one_bit_per_word", "uniform", D1, NB1)
    r_rank = (np.arange(inner.size) * 2 // inner.size).astype(np.int64)
    dup = inner[r_rank == 0][1234]
    keys = np.concatenate([inner, [dup]])
    r_rank = np.concatenate([r_rank, [1]])
    ref = H.ref_join_count(torch.from_numpy(keys), torch.from_numpy(outer.copy()))
    assert ref > case("one_bit_per_word", "uniform", D1, NB1)[2]
    s_rank = np.arange(outer.size) * 2 // outer.size

    def cfg(c):
        c.replicate_bitmap = C.PlanChoice.ON
        c.network_bits = NB1
        c.key_hashing = C.KeyHashing.OFF

    out = run_ranks(C, 2, loc, rank_relations(C, dev, keys, r_rank, 2), rank_relations(C, dev, outer, s_rank, 2),
                    keys.size, outer.size, cfg)
    for (first, second), plan in out:
        assert first["local_fallbacks"] == 1 and not first["bitmap_join"] and first["global_matches"] == ref
        assert second["local_fallbacks"] == 0 and not second["bitmap_join"] and second["global_matches"] == ref
        assert not plan.bitmap_join


# ---- two-level count-only plans (bitmap_join = False) --------------------------------
# 2^23 keys: 9 network bits + 1 local bit leave 1024 final partitions of 13-bit fragments, the widest a direct
# count table takes.  A random half puts 4096 +- 45 inner fragments into each (one batch of the count kernels
# is 4096: about half of the items run a second, short batch; half plus repeats: 4900), and 2^23 uniform outer
# keys 8192 into each, two to three batches.
D2, NB2 = 1 << 23, 9


def two_level_cfg(C):
    cfg = C.JoinConfig()
    cfg.bitmap_join = False
    cfg.network_bits = NB2
    cfg.key_hashing = C.KeyHashing.OFF
    return cfg


def run_two_level(C, inner, outer, ref, cfg, check):
    j = C.HashJoin(relation(C, "cuda", inner), relation(C, "cuda", outer), context(C, "cuda"), cfg)
    assert not j.plan.bitmap_join and j.plan.network_bits == NB2 and not j.plan.key_mix, j.plan
    check(j.plan)
    for _ in range(2):
        res = j.run()
        assert res["global_matches"] == ref and not res["bitmap_join"] and res["local_fallbacks"] == 0, res
        if not j.plan.sampled_network:
            assert res["network_fallbacks"] == 0
    return j


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("pattern", ["half", "one_word_in_k"])
def test_two_level_count_selective(C, cuda, pattern, direct, split):
    """direct_count x split_local: the direct-addressed count tables (u16 fragment column and 8-byte words)
    and the hash tables they replace, with slots that must stay 0."""
    inner, outer, ref = case(pattern, "uniform", D2, NB2, D2)
    cfg = two_level_cfg(C)
    cfg.network_histogram = C.HistogramMode.EXACT
    cfg.direct_count, cfg.split_local = direct, split

    def check(p):
        assert p.split_local == split and not p.sampled_network and not p.fragments
        assert p.key_bits == 23 and p.key_bits - p.network_bits - p.local_bits <= 13

    run_two_level(C, inner, outer, ref, cfg, check)
    inner, outer, ref = case(pattern, "complement", D2, NB2)
    run_two_level(C, inner, outer, ref, cfg, check)


@pytest.mark.gpu
@pytest.mark.parametrize("local", ["SAMPLED", "EXACT"])
@pytest.mark.parametrize("pattern", ["half", "one_word_in_k"])
def test_fragment_plan_selective(C, cuda, pattern, local):
    """The fragment plan (u32 fragments from the sampled network pass, u16 fragment column from the local
    pass): a wrong 16-bit lane of an 8-byte word of that column reads a neighbour's fragment."""
    inner, outer, ref = case(pattern, "uniform", D2, NB2, D2)
    cfg = two_level_cfg(C)
    cfg.network_histogram = C.HistogramMode.SAMPLED
    cfg.local_histogram = getattr(C.HistogramMode, local)

    def check(p):
        assert p.fragments and p.sampled_network and p.split_local, p

    run_two_level(C, inner, outer, ref, cfg, check)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False])
def test_two_level_count_selective_with_repeats(C, cuda, split):
    """A random half plus a million copies of a thousand of its keys, bitmap_join and replicate_bitmap left
    alone: the planner sees the repeats and takes the two-level plan by itself; count slots hold 0, 1 and
    about a thousand."""
    half, outer, _ = case("half", "uniform", D2, NB2, D2)
    rng = np.random.default_rng(3)
    inner = rng.permutation(np.concatenate([half, rng.choice(half[:1000], 1_000_000)]))
    ref = H.ref_join_count(torch.from_numpy(inner), torch.from_numpy(outer.copy()))
    cfg = C.JoinConfig()
    cfg.network_bits = NB2
    cfg.key_hashing = C.KeyHashing.OFF
    cfg.network_histogram = C.HistogramMode.EXACT
    cfg.split_local = split

    def check(p):
        assert p.inner_repeats and p.split_local == split, p

    run_two_level(C, inner, outer, ref, cfg, check)
