"""Tensor-level entry points of the gfx950 kernels (device tensors) and their
host twins (CPU tensors).  Tuples are int64 tensors of shape [n, 2] holding
(key, rid) — the 16-byte ``hpcjoin::data::Tuple`` layout.  The whole-engine
ops (``join_count``, ``join``, the semi / anti / outer / group joins) also take
a 1-D int64 key column for either side: its rids are the positions, and the
plans that carry no rid read it in place (``Relation.from_keys``).

    values, begin = radix_partition(tuples, bits=10)      # network pass
    v2, begin2 = local_partition(values, begin, 32, 9)   # local pass
    n = build_probe_count(rv, sv, rbeg, sbeg, 41, 32)    # LDS build/probe
    join_count(R, S)                                      # whole engine
    semi_join(R, S), anti_join(R, S)                      # outer rids with / without an inner partner
    left_outer_join(R, S), right_outer_join(R, S), full_outer_join(R, S)   # pairs + NULL_RID-padded rows
    semi_join_rows(R, S, S_rows), anti_join_rows(R, S, S_rows)            # [m, 5]: outer rid + its payload row
    full_outer_join_rows(R, S, R_rows, S_rows)                            # [m, 10]: rids + both rows, NULL_RID-padded
    group_join_count(R, S), group_join_sum(R, S, values)   # per inner tuple: [|R|, 2] (rid, count) / [|R|, 3] (+ sum)
    group_join_agg(R, S, [a, b, b], ["sum", "min", "max"])  # [|R|, 2 + C]: (rid, count, agg_0, ...), C = 1 ... 4 columns
                                                           # (AVG is sum / count on the caller's side)
"""
from __future__ import annotations

import torch

from .._native import require_native
from .tuples import compress, decompress, make_tuples  # noqa: F401


def _C():
    return require_native()


def generate(n: int, distribution: str = "UNIQUE", seed: int = 1234, domain: int = 0, global_offset: int = 0,
             global_size: int | None = None, zipf_theta: float = 0.75, device: str = "cpu") -> torch.Tensor:
    """Slice [global_offset, global_offset + n) of a synthetic relation (see Relation.generate)."""
    C = _C()
    spec = C.GenSpec(distribution=getattr(C.KeyDistribution, distribution.upper()), seed=seed, domain=domain,
                     zipf_theta=zipf_theta)
    return C.ops.generate(n, global_offset, global_size or n, spec, str(device))


def radix_histogram(tuples: torch.Tensor, bits: int) -> torch.Tensor:
    """Counts of ``key & (2^bits - 1)`` (LocalHistogram); ``tuples`` may be a 1-D key column."""
    return _C().ops.net_histogram(tuples.contiguous(), bits)


def radix_partition(tuples: torch.Tensor, bits: int, key_shift: int = 32, wide: bool = False,
                    key_bits: int = 64):
    """Network pass: returns (values, part_begin[F+1]); values are packed
    CompressedTuples (int64) unless ``wide`` (then [n, 2] tuples)."""
    return _C().ops.net_partition(tuples.contiguous(), bits, key_shift, wide, 2048, key_bits)


def local_partition(values: torch.Tensor, part_begin: torch.Tensor, shift: int, bits: int, wide: bool = False):
    """Local pass over a partition-major buffer: every input partition is split
    by ``(word >> shift) & (2^bits - 1)``; returns (values, part_begin[P*2^bits+1])."""
    return _C().ops.local_partition(values.contiguous(), part_begin, shift, bits, wide)


def build_probe(R, S, part_r, part_s, frag_shift: int, key_shift: int, wide=False, materialize=False,
                r_chunk=4096, s_chunk=65536, out_capacity=0) -> dict:
    """LDS hash build/probe over matching partitions; returns a dict with
    ``matches`` (and ``pairs`` / ``output_count`` when materializing)."""
    return _C().ops.build_probe(R, S, part_r, part_s, frag_shift, key_shift, wide, materialize, r_chunk, s_chunk,
                                out_capacity)


def build_probe_count(R, S, part_r, part_s, frag_shift: int, key_shift: int) -> int:
    return build_probe(R, S, part_r, part_s, frag_shift, key_shift)["matches"]


def build_probe_marks(R, S, part_r, part_s, frag_shift: int, key_shift: int, wide=False, r_chunk=4096,
                      s_chunk=65536) -> dict:
    """Semi-join marks over matching partitions: ``marks`` (bool [len(S)], by
    outer position: the tuple's key occurs on the inner side of its partition)
    and ``semi_count``; also ``anti_count`` and the compacted ``semi_rids`` /
    ``anti_rids``."""
    return _C().ops.build_probe_marks(R, S, part_r, part_s, frag_shift, key_shift, wide, r_chunk, s_chunk)


def build_probe_outer(R, S, part_r, part_s, frag_shift: int, key_shift: int, wide=False, r_chunk=4096,
                      s_chunk=65536, keep_inner=True, keep_outer=True) -> dict:
    """Outer join over matching partitions: ``pairs`` (int64 [m, 2]: the inner
    join's (inner rid, outer rid) pairs, then ``(rid, NULL_RID)`` per unmatched
    inner tuple if ``keep_inner`` and ``(NULL_RID, rid)`` per unmatched outer
    tuple if ``keep_outer``), ``matched_pairs``, ``unmatched_inner``,
    ``unmatched_outer`` and ``inner_marks`` / ``outer_marks`` (bool per
    position of R / S: the tuple has a partner; all false for a side not kept)."""
    return _C().ops.build_probe_outer(R, S, part_r, part_s, frag_shift, key_shift, wide, r_chunk, s_chunk,
                                      keep_inner, keep_outer)


def build_probe_mark_rows(R, S, part_r, part_s, frag_shift: int, key_shift: int, wide=False, r_chunk=4096,
                          s_chunk=65536, outer_rows=None, rid_offset=0, out_capacity=0) -> dict:
    """``build_probe_marks`` with the row-writing place pass: ``semi_rows`` / ``anti_rows`` are the whole
    ``[capacity + guard_rows, 5]`` buffers (``capacity`` = ``out_capacity`` or ``len(S)``) holding
    ``[rid, outer_rows[rid - rid_offset]]`` per selected tuple below the capacity and ``sentinel`` words everywhere
    else; ``semi_count`` / ``anti_count`` are the full counts."""
    return _C().ops.build_probe_mark_rows(R, S, part_r, part_s, frag_shift, key_shift, wide, r_chunk, s_chunk,
                                          outer_rows, rid_offset, out_capacity)


def build_probe_group(R, S, part_r, part_s, frag_shift: int, key_shift: int, wide=False, r_chunk=4096,
                      s_chunk=65536, values=None, rid_offset=0) -> dict:
    """Group join over matching partitions: ``rows`` (int64 ``[|R|, 2]`` of (inner rid, count), or ``[|R|, 3]``
    of (inner rid, count, sum) with ``values``, a 1-D int64 tensor with ``values[rid - rid_offset]`` the value
    of outer tuple ``rid``; any positive element stride), ``matched_pairs`` (the sum of the counts),
    ``unmatched_inner`` (groups with count 0) and the raw accumulators ``counts`` / ``sums`` (int64, by position
    of R).  int32, float64 or float32 ``values`` run ``build_probe_group_agg`` with one ``"sum"`` column (``sums``
    then holds binary64 bits for the float dtypes, and ``group_dtypes`` says so)."""
    return _C().ops.build_probe_group(R, S, part_r, part_s, frag_shift, key_shift, wide, r_chunk, s_chunk, values,
                                      rid_offset)


def build_probe_group_agg(R, S, part_r, part_s, frag_shift: int, key_shift: int, wide=False, r_chunk=4096,
                          s_chunk=65536, columns=(), aggs=(), rid_offset=0) -> dict:
    """Group join with aggregates over matching partitions: ``columns`` are 1 ... 4 1-D int64 tensors (any positive
    element stride each, ``column[rid - rid_offset]`` the value of outer tuple ``rid``), ``aggs`` one of ``"sum"``
    (int64, wraps), ``"min"``, ``"max"`` (signed) per column.  ``rows`` (int64 ``[|R|, 2 + C]`` of (inner rid, count,
    agg_0, ...); a tuple without a partner has count 0 and each aggregate's identity: 0, INT64_MAX, INT64_MIN),
    ``matched_pairs``, ``unmatched_inner`` and the raw accumulators ``counts`` (``[|R|]``) and ``aggs``
    (``[C, |R|]``), by position of R.  Columns may also be int32, float64 or float32 (see ``group_join_agg``):
    ``aggs`` and ``rows`` stay int64 and hold binary64 bits for float columns (identities ``+0.0``, ``+inf``,
    ``-inf``); ``group_dtypes`` lists the row-word dtype per column, ``"int64"`` or ``"float64"``."""
    return _C().ops.build_probe_group_agg(R, S, part_r, part_s, frag_shift, key_shift, wide, r_chunk, s_chunk,
                                          list(columns), [str(a) for a in aggs], rid_offset)


def build_probe_outer_rows(R, S, part_r, part_s, frag_shift: int, key_shift: int, wide=False, r_chunk=4096,
                           s_chunk=65536, keep_inner=True, keep_outer=True, inner_rows=None, inner_rid_offset=0,
                           outer_rows=None, outer_rid_offset=0) -> dict:
    """``build_probe_outer`` plus ``rows``: the whole ``[m + guard_rows, 10]`` buffer with the 10-word row of
    every pair and, behind them, the NULL_RID-padded rows of the kept sides written by the row-writing place
    pass; ``sentinel`` words in the guard rows."""
    return _C().ops.build_probe_outer_rows(R, S, part_r, part_s, frag_shift, key_shift, wide, r_chunk, s_chunk,
                                           keep_inner, keep_outer, inner_rows, inner_rid_offset, outer_rows,
                                           outer_rid_offset)


def rid_rows(rids: torch.Tensor, rows: torch.Tensor, rid_offset: int = 0) -> torch.Tensor:
    """int64 [n, 5]: ``[rid, rows[rid - rid_offset]]`` per rid."""
    return _C().ops.rid_rows(rids.contiguous(), rows, rid_offset)


def pair_rows(pairs: torch.Tensor, rows_a: torch.Tensor, off_a: int, rows_b: torch.Tensor, off_b: int,
              variant: int = 1) -> torch.Tensor:
    """int64 [n, 10]: ``[rid_a, rid_b, rows_a[rid_a - off_a], rows_b[rid_b - off_b]]`` per pair; a ``NULL_RID``
    side gives four ``NULL_RID`` words and reads no row."""
    return _C().ops.pair_rows(pairs.contiguous(), rows_a, off_a, rows_b, off_b, variant)


def npj_count(R: torch.Tensor, S: torch.Tensor) -> int:
    """No-partitioning join baseline (one global hash table)."""
    return _C().ops.npj_count(R.contiguous(), S.contiguous())


def npj_join(R: torch.Tensor, S: torch.Tensor) -> torch.Tensor:
    """(inner rid, outer rid) pairs of the no-partitioning hash join, [matches, 2] int64."""
    return _C().ops.npj_join(R.contiguous(), S.contiguous())


def _relation(C, t: torch.Tensor):
    """``[n, 2]`` (key, rid) tuples, or a 1-D int64 key column whose rids are the positions (read in place by the
    plans that carry no rid, ``Relation.from_keys``)."""
    if t.dim() == 1:
        return C.Relation.from_keys(t.contiguous(), t.shape[0], 0)
    return C.Relation.from_tensor(t.contiguous(), t.shape[0])


def _engine(inner: torch.Tensor, outer: torch.Tensor, config=None):
    C = _C()
    on_dev = inner.is_cuda
    dev = (inner.device.index or 0) if on_dev else -1
    ctx = C.ExecContext("device" if on_dev else "host", dev, C.LocalCommunicator())
    R = _relation(C, inner)
    S = _relation(C, outer)
    return C.HashJoin(R, S, ctx, config or C.JoinConfig())


def join_count(inner: torch.Tensor, outer: torch.Tensor, config=None) -> int:
    """|inner join outer| on key, single process, full engine."""
    return _engine(inner, outer, config).run()["global_matches"]


def join(inner: torch.Tensor, outer: torch.Tensor, config=None) -> torch.Tensor:
    """Materialized join: int64 [m, 2] of (inner rid, outer rid)."""
    C = _C()
    cfg = config or C.JoinConfig()
    cfg.materialize = True
    j = _engine(inner, outer, cfg)
    j.run()
    return j.output()


def _kind_join(inner, outer, kind: str, materialize: bool, config=None):
    C = _C()
    cfg = config or C.JoinConfig()
    cfg.kind = getattr(C.JoinKind, kind)
    cfg.materialize = materialize
    j = _engine(inner, outer, cfg)
    res = j.run()
    return j.output_rids() if materialize else res["global_matches"]


def semi_join(inner: torch.Tensor, outer: torch.Tensor, config=None) -> torch.Tensor:
    """Rids (int64 [m], any order) of the outer tuples whose key occurs in ``inner``: each once."""
    return _kind_join(inner, outer, "SEMI", True, config)


def anti_join(inner: torch.Tensor, outer: torch.Tensor, config=None) -> torch.Tensor:
    """Rids (int64 [m], any order) of the outer tuples whose key does not occur in ``inner``."""
    return _kind_join(inner, outer, "ANTI", True, config)


def semi_join_count(inner: torch.Tensor, outer: torch.Tensor, config=None) -> int:
    """Number of outer tuples with at least one inner partner (not the inner-join count)."""
    return _kind_join(inner, outer, "SEMI", False, config)


def anti_join_count(inner: torch.Tensor, outer: torch.Tensor, config=None) -> int:
    """Number of outer tuples with no inner partner."""
    return _kind_join(inner, outer, "ANTI", False, config)


# Padding rid of an outer join's unmatched rows (~0 as uint64, -1 as int64).
NULL_RID = -1


def _outer_join(inner, outer, kind: str, materialize: bool, config=None):
    C = _C()
    cfg = config or C.JoinConfig()
    cfg.kind = getattr(C.JoinKind, kind)
    cfg.materialize = materialize
    j = _engine(inner, outer, cfg)
    res = j.run()
    return j.output() if materialize else res["global_matches"]


def left_outer_join(inner: torch.Tensor, outer: torch.Tensor, config=None) -> torch.Tensor:
    """int64 [m, 2]: the join's (inner rid, outer rid) pairs plus ``(rid, NULL_RID)`` per inner tuple without a
    partner; any order."""
    return _outer_join(inner, outer, "LEFT_OUTER", True, config)


def right_outer_join(inner: torch.Tensor, outer: torch.Tensor, config=None) -> torch.Tensor:
    """int64 [m, 2]: the join's pairs plus ``(NULL_RID, rid)`` per outer tuple without a partner; any order."""
    return _outer_join(inner, outer, "RIGHT_OUTER", True, config)


def full_outer_join(inner: torch.Tensor, outer: torch.Tensor, config=None) -> torch.Tensor:
    """int64 [m, 2]: the join's pairs plus the NULL_RID-padded rows of both sides' tuples without a partner."""
    return _outer_join(inner, outer, "FULL_OUTER", True, config)


def left_outer_join_count(inner: torch.Tensor, outer: torch.Tensor, config=None) -> int:
    """Rows of ``left_outer_join``: pairs + inner tuples without a partner."""
    return _outer_join(inner, outer, "LEFT_OUTER", False, config)


def right_outer_join_count(inner: torch.Tensor, outer: torch.Tensor, config=None) -> int:
    """Rows of ``right_outer_join``: pairs + outer tuples without a partner."""
    return _outer_join(inner, outer, "RIGHT_OUTER", False, config)


def full_outer_join_count(inner: torch.Tensor, outer: torch.Tensor, config=None) -> int:
    """Rows of ``full_outer_join``."""
    return _outer_join(inner, outer, "FULL_OUTER", False, config)


def _group_join(inner, outer, values, rid_offset: int, config=None) -> torch.Tensor:
    C = _C()
    cfg = config or C.JoinConfig()
    cfg.kind = C.JoinKind.GROUP
    cfg.materialize = True
    on_dev = inner.is_cuda
    ctx = C.ExecContext("device" if on_dev else "host", (inner.device.index or 0) if on_dev else -1,
                        C.LocalCommunicator())
    R = _relation(C, inner)
    S = _relation(C, outer)
    j = C.HashJoin(R, S, ctx, cfg)
    if values is None:
        j.run()
        return j.output_groups()
    _, rows = j.join_group(ctx, values, rid_offset, values.shape[0])
    return rows


def group_join_count(inner: torch.Tensor, outer: torch.Tensor, config=None) -> torch.Tensor:
    """int64 [|inner|, 2]: ``(inner rid, count)`` per inner tuple, count = outer tuples with its key (0 for a
    tuple without a partner; copies of a key each get the key's count); any order."""
    return _group_join(inner, outer, None, 0, config)


def group_join_sum(inner: torch.Tensor, outer: torch.Tensor, values: torch.Tensor, rid_offset: int = 0,
                   config=None) -> torch.Tensor:
    """int64 [|inner|, 3]: ``(inner rid, count, sum)`` per inner tuple, sum = the int64 (wrapping) sum of
    ``values[rid - rid_offset]`` over the outer tuples with its key.  ``values`` is a 1-D int64 tensor of any
    positive element stride (a column view such as ``S_rows[:, 2]`` is read in place).

    ``values`` may also be int32 (sign-extended, summed as int64), float64 or float32 (converted exactly, summed
    as IEEE binary64): the stride then counts elements of that dtype, and for the float dtypes the sum word holds
    the bit pattern of the binary64 sum (``group_agg_values(rows, 0, values)`` views it as float64).  A float sum
    is taken in the order the updates land -- exact whenever every partial sum is representable, otherwise
    within the usual rounding bound; an empty group carries ``+0.0``.  NaN inputs give an unspecified result."""
    return _group_join(inner, outer, values, rid_offset, config)


def group_join_agg(inner: torch.Tensor, outer: torch.Tensor, columns, aggs, rid_offset: int = 0,
                   config=None) -> torch.Tensor:
    """int64 [|inner|, 2 + C]: ``(inner rid, count, agg_0, ..., agg_{C-1})`` per inner tuple over the outer tuples
    with its key.  ``columns``: C = 1 ... 4 1-D int64 tensors with ``column[rid - rid_offset]`` the value of outer
    tuple ``rid`` (views such as ``S_rows[:, 1]`` are read in place; the same view may come twice); ``aggs``: one
    of ``"sum"`` (wraps), ``"min"``, ``"max"`` (signed) per column.  A tuple without a partner has count 0 and each
    aggregate's identity (0, INT64_MAX, INT64_MIN).  AVG is ``sum / count`` on the caller's side.

    Each column may independently be int64, int32, float64 or float32; its stride counts elements of its own
    dtype (``rows32[:, 3]`` of an ``[n, 8]`` int32 tensor is read in place with 4-byte loads).  int32 values are
    sign-extended and aggregate as int64 (a sum cannot wrap).  float64 / float32 values aggregate as IEEE
    binary64 (float32 converts exactly) and the row word holds the binary64 bit pattern -- read it with
    ``group_agg_values(rows, c, column)``.  Float identities: ``+0.0`` (sum), ``+inf`` (min), ``-inf`` (max).  A
    float sum is the sum in whatever order the updates land: exact whenever every partial sum is representable,
    otherwise within the usual rounding bound.  Float MIN / MAX compare as IEEE numbers; NaN inputs give an
    unspecified result, and so does the relative order of ``-0.0`` and ``+0.0``.  With a float64 sum, AVG is one
    division on the caller's side.  Any other dtype (float16, bool, uint8, ...) is refused."""
    C = _C()
    cfg = config or C.JoinConfig()
    cfg.kind = C.JoinKind.GROUP
    cfg.materialize = True
    cfg.group_columns = max(1, min(len(columns), 4))  # (more than four: refused by join_group_agg)
    on_dev = inner.is_cuda
    ctx = C.ExecContext("device" if on_dev else "host", (inner.device.index or 0) if on_dev else -1,
                        C.LocalCommunicator())
    R = _relation(C, inner)
    S = _relation(C, outer)
    j = C.HashJoin(R, S, ctx, cfg)
    _, rows = j.join_group_agg(ctx, list(columns), [str(a) for a in aggs], rid_offset, outer.shape[0])
    return rows


def group_agg_values(rows: torch.Tensor, c: int, like=None) -> torch.Tensor:
    """Aggregate column ``c`` of group-join rows (``rows[:, 2 + c]``) as a 1-D tensor: int64, or -- when ``like``
    is a float32 / float64 tensor or dtype, i.e. the value column was a float column -- float64, a bit-level view
    of the same words (no conversion pass, no copy)."""
    assert rows.dim() == 2 and rows.dtype == torch.int64 and 0 <= c < rows.shape[1] - 2, (rows.shape, rows.dtype, c)
    col = rows[:, 2 + c]
    dtype = like.dtype if isinstance(like, torch.Tensor) else like
    if dtype in (torch.float32, torch.float64):
        return col.view(torch.float64)
    return col


def _kind_join_rows(inner, outer, kind: str, inner_rows, outer_rows, rid_offset: int, config=None) -> torch.Tensor:
    C = _C()
    cfg = config or C.JoinConfig()
    cfg.kind = getattr(C.JoinKind, kind)
    cfg.materialize = True
    on_dev = inner.is_cuda
    ctx = C.ExecContext("device" if on_dev else "host", (inner.device.index or 0) if on_dev else -1,
                        C.LocalCommunicator())
    R = _relation(C, inner)
    S = _relation(C, outer)
    j = C.HashJoin(R, S, ctx, cfg)
    if inner_rows is None:  # semi / anti: the inner payload is never read
        inner_rows = torch.empty((0, 4), dtype=torch.int64, device=outer_rows.device)
    _, rows = j.join_rows(ctx, inner_rows, rid_offset, inner_rows.shape[0], outer_rows, rid_offset,
                          outer_rows.shape[0])
    return rows


def semi_join_rows(inner: torch.Tensor, outer: torch.Tensor, outer_rows: torch.Tensor, rid_offset: int = 0,
                   config=None) -> torch.Tensor:
    """int64 [m, 5]: ``[outer rid, outer_rows[rid - rid_offset]]`` of the outer tuples whose key occurs in
    ``inner``, each once, any order."""
    return _kind_join_rows(inner, outer, "SEMI", None, outer_rows, rid_offset, config)


def anti_join_rows(inner: torch.Tensor, outer: torch.Tensor, outer_rows: torch.Tensor, rid_offset: int = 0,
                   config=None) -> torch.Tensor:
    """int64 [m, 5]: ``[outer rid, outer row]`` of the outer tuples whose key does not occur in ``inner``."""
    return _kind_join_rows(inner, outer, "ANTI", None, outer_rows, rid_offset, config)


def left_outer_join_rows(inner: torch.Tensor, outer: torch.Tensor, inner_rows: torch.Tensor,
                         outer_rows: torch.Tensor, rid_offset: int = 0, config=None) -> torch.Tensor:
    """int64 [m, 10]: ``[rid_inner, rid_outer, inner row, outer row]`` of ``left_outer_join``'s rows; the outer
    half of an unmatched inner tuple's row is five ``NULL_RID`` words.  Both payloads start at ``rid_offset``."""
    return _kind_join_rows(inner, outer, "LEFT_OUTER", inner_rows, outer_rows, rid_offset, config)


def right_outer_join_rows(inner: torch.Tensor, outer: torch.Tensor, inner_rows: torch.Tensor,
                          outer_rows: torch.Tensor, rid_offset: int = 0, config=None) -> torch.Tensor:
    """int64 [m, 10]: the rows of ``right_outer_join``; the inner half of an unmatched outer tuple's row is
    ``NULL_RID`` words."""
    return _kind_join_rows(inner, outer, "RIGHT_OUTER", inner_rows, outer_rows, rid_offset, config)


def full_outer_join_rows(inner: torch.Tensor, outer: torch.Tensor, inner_rows: torch.Tensor,
                         outer_rows: torch.Tensor, rid_offset: int = 0, config=None) -> torch.Tensor:
    """int64 [m, 10]: the rows of ``full_outer_join``, NULL_RID-padded on either side."""
    return _kind_join_rows(inner, outer, "FULL_OUTER", inner_rows, outer_rows, rid_offset, config)
