"""Every instantiation of the group-join kernels against the host twin, bit for bit.

``ops.build_probe_group`` / ``ops.build_probe_group_agg`` run on the device and on ``"cpu"`` (host::buildProbeGroup /
host::groupEmit) over the same partition-major inputs; ``rows`` (sorted by rid), ``counts``, ``aggs`` / ``sums``,
``matched_pairs`` and ``unmatched_inner`` must be equal, with no tolerance.  The host twin itself is first checked, on
the CPU alone, against a plain torch group-by of the same inputs.

The ops take compressed u64 words and wide tuples and never know the fragment width, so they reach the hashed tables
of those two layouts: count only (emit C = 0), one int64 SUM column (the single-column kernel, emit C = 1), C = 1 ... 4
int64 columns mixing SUM / MIN / MAX, and C = 1 ... 4 typed columns (int32, float64, float32 and int64 next to them,
element strides 1 ... 3).  The split layout and the direct-addressed count table (fragments of at most 13 bits) exist
only behind the engine's local pass, so they are driven through ``HashJoin`` with ``kind = GROUP``: ``split_local`` on
and off, ``direct_count`` on and off, the same column sets, the device's rows against the host engine's.

Shapes (the smallest at which the kernels can still go wrong):
 * ``main``: P = 5 final partitions -- 1100 x 9300 (three inner chunks of r_chunk = 512, two outer chunks of s_chunk =
   5000: more than one batch of 4096 with a ragged tail), 0 x 700, 333 x 0, 777 x 1500 and 97 x 515; inner units of
   512, 76, 333, 265 and 97 positions (no multiple of 64 among the tails).
 * ``many``: 1300 partitions of about 6 x 12 tuples, 1/16 of them empty on either side: more work items than the
   persistent grid has workgroups (at most 256 * 4), so every workgroup takes a second trip.
Inner keys repeat (copies read the first slot of their key), half of the outer key domain has no partner.  int64 and
int32 values span their whole range (the int64 sums wrap); float values are integers of magnitude <= 1024, so every
partial sum is exact in binary64 in whatever order the atomics land.
"""
import functools

import pytest
import torch

from test_group_join import _check_rows, _ctx

RID_OFFSET = 1000
R_CHUNK, S_CHUNK = 512, 5000
I64_MAX, I64_MIN = 2**63 - 1, -2**63
F64_INF, F64_NINF = 0x7FF0000000000000, 0xFFF0000000000000 - 2**64  # the bits, as int64
DTYPES = {"i64": torch.int64, "i32": torch.int32, "f64": torch.float64, "f32": torch.float32}

# name -> [(dtype, aggregate, element stride)]; "count" has no column, "sum" goes through build_probe_group(values=)
CASES = {
    "count": [],
    "sum": [("i64", "sum", 2)],
    "u1": [("i64", "max", 1)],
    "u2": [("i64", "sum", 2), ("i64", "min", 1)],
    "u3": [("i64", "sum", 1), ("i64", "min", 3), ("i64", "max", 1)],
    "u4": [("i64", "min", 1), ("i64", "max", 3), ("i64", "sum", 1), ("i64", "sum", 2)],
    "t1": [("f32", "sum", 2)],
    "t2": [("i32", "max", 3), ("f64", "min", 1)],
    "t3": [("f64", "sum", 2), ("f32", "min", 2), ("i32", "max", 3)],
    "t4": [("i32", "sum", 1), ("f32", "max", 3), ("f64", "sum", 1), ("i64", "min", 2)],
}
SHAPES = {
    "main": [(1100, 9300), (0, 700), (333, 0), (777, 1500), (97, 515)],
}


def _many_sizes():
    g = torch.Generator().manual_seed(3)
    nr, ns = torch.randint(1, 12, (1300,), generator=g), torch.randint(1, 24, (1300,), generator=g)
    hole = torch.randint(0, 16, (1300,), generator=g)
    nr[hole == 0] = 0
    ns[hole == 1] = 0
    return list(zip(nr.tolist(), ns.tolist()))


SHAPES["many"] = _many_sizes()


class Inputs:
    """Partition-major (key, rid) tuples of both sides on the CPU: key = (fragment << bits) | partition."""

    def __init__(self, shape):
        sizes = SHAPES[shape]
        g = torch.Generator().manual_seed(len(sizes))
        self.P = len(sizes)
        self.bits = max(1, (self.P - 1).bit_length())
        rk, sk = [], []
        for p, (nr, ns) in enumerate(sizes):
            D = max(1, nr // 2)  # inner keys repeat; outer fragments >= D have no partner
            rk.append((torch.randint(0, D, (nr,), generator=g) << self.bits) | p)
            sk.append((torch.randint(0, 2 * D + 1, (ns,), generator=g) << self.bits) | p)
        self.rk, self.sk = torch.cat(rk), torch.cat(sk)
        self.n_r, self.n_s = self.rk.numel(), self.sk.numel()
        self.r_rid = torch.randperm(self.n_r, generator=g) + 7  # scattered: the gathers are no stream
        self.s_rid = torch.randperm(self.n_s, generator=g) + RID_OFFSET
        self.part_r = torch.tensor([0] + [s[0] for s in sizes]).cumsum(0)
        self.part_s = torch.tensor([0] + [s[1] for s in sizes]).cumsum(0)
        self._base = {}
        # what the docstring promises of the inputs
        assert torch.unique(self.rk).numel() < 0.8 * self.n_r
        assert int((~torch.isin(self.sk, self.rk)).sum()) > 0.2 * self.n_s
        assert any(nr == 0 and ns > 0 for nr, ns in sizes) and any(ns == 0 and nr > 0 for nr, ns in sizes)

    def tuples(self, wide, dev):
        """(R, S, frag_shift, key_shift) as the ops take them."""
        if wide:
            R, S = torch.stack([self.rk, self.r_rid], 1), torch.stack([self.sk, self.s_rid], 1)
            return R.contiguous().to(dev), S.contiguous().to(dev), 64, 64
        return ((self.rk << 32) | self.r_rid).to(dev), ((self.sk << 32) | self.s_rid).to(dev), 32 + self.bits, 32

    def column(self, i, dtype, stride, dev):
        """Column i by outer rid - RID_OFFSET: a view with the given element stride into its own tensor."""
        key = (i, dtype, stride)
        if key not in self._base:
            g = torch.Generator().manual_seed(1000 + 10 * i + stride)
            n = self.n_s * stride
            if dtype == "i64":
                base = torch.randint(I64_MIN, I64_MAX, (n,), generator=g)
            elif dtype == "i32":
                base = torch.randint(-2**31, 2**31, (n,), generator=g).to(torch.int32)
            else:
                base = torch.randint(-1024, 1025, (n,), generator=g).to(DTYPES[dtype])
            self._base[key] = base
        view = self._base[key].to(dev)[stride - 1::stride]
        assert view.shape == (self.n_s,) and (self.n_s < 2 or view.stride(0) == stride)
        return view


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return Inputs(shape)


def _run_ops(shape, wide, case, dev):
    from hpcjoin import ops
    x = _inputs(shape)
    R, S, frag_shift, key_shift = x.tuples(wide, dev)
    spec = CASES[case]
    cols = [x.column(i, d, st, dev) for i, (d, _, st) in enumerate(spec)]
    kw = dict(wide=wide, r_chunk=R_CHUNK, s_chunk=S_CHUNK, rid_offset=RID_OFFSET)
    if case in ("count", "sum"):
        res = ops.build_probe_group(R, S, x.part_r, x.part_s, frag_shift, key_shift, values=cols[0] if cols else None, **kw)
    else:
        res = ops.build_probe_group_agg(R, S, x.part_r, x.part_s, frag_shift, key_shift, columns=cols,
                                        aggs=[a for _, a, _ in spec], **kw)
    out = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    out["rows"] = out["rows"][torch.sort(out["rows"][:, 0]).indices]
    return out


@functools.lru_cache(maxsize=None)
def _host(shape, wide, case):
    """The host twin's result, computed once and shared by the CPU check and the device comparison."""
    return _run_ops(shape, wide, case, "cpu")


def _identity(dtype, how):
    if dtype in ("f64", "f32"):
        return {"sum": 0.0, "min": float("inf"), "max": float("-inf")}[how]
    return {"sum": 0, "min": I64_MAX, "max": I64_MIN}[how]


def _group_by(x, spec):
    """counts [n_r] and the aggregate words [C, n_r] by position of R, from a plain torch group-by of the outer side."""
    uk, inv = torch.unique(x.sk, return_inverse=True)
    pos = torch.searchsorted(uk, x.rk).clamp(max=uk.numel() - 1)
    hit = uk[pos] == x.rk
    cnt = torch.zeros(uk.numel(), dtype=torch.int64).index_add_(0, inv, torch.ones_like(inv))
    counts = torch.where(hit, cnt[pos], torch.zeros_like(pos))
    words = []
    for i, (dtype, how, stride) in enumerate(spec):
        acc_t = torch.float64 if dtype in ("f64", "f32") else torch.int64
        v = x.column(i, dtype, stride, "cpu")[x.s_rid - RID_OFFSET].to(acc_t)  # widened as the kernels do
        ident = _identity(dtype, how)
        if how == "sum":
            acc = torch.zeros(uk.numel(), dtype=acc_t).index_add_(0, inv, v)  # int64 wraps
        else:
            acc = torch.full((uk.numel(),), ident, dtype=acc_t).scatter_reduce_(
                0, inv, v, "amin" if how == "min" else "amax", include_self=True)
        out = torch.where(hit, acc[pos], torch.full((x.n_r,), ident, dtype=acc_t))
        words.append(out.view(torch.int64))
    return counts, (torch.stack(words) if words else torch.zeros((0, x.n_r), dtype=torch.int64))


def _grid():
    return [(s, w, c) for s in SHAPES for w in (False, True) for c in CASES]


def _ids(v):
    return f"{v[0]}-{'wide' if v[1] else 'compressed'}-{v[2]}"


# ------------------------------------------------ 1. host twin vs torch group-by
@pytest.mark.parametrize("shape,wide,case", _grid(), ids=[_ids(v) for v in _grid()])
def test_host_twin_is_a_group_by(C, shape, wide, case):
    x, spec, got = _inputs(shape), CASES[case], _host(shape, wide, case)
    counts, words = _group_by(x, spec)
    assert int((counts == 0).sum()) > 0 and int((counts > 1).sum()) > 0
    assert (got["matched_pairs"], got["unmatched_inner"]) == (int(counts.sum()), int((counts == 0).sum()))
    assert torch.equal(got["counts"], counts)
    assert got["aggs"].shape == words.shape and torch.equal(got["aggs"], words)
    if case in ("count", "sum"):
        assert torch.equal(got["sums"], words[0] if spec else torch.zeros(x.n_r, dtype=torch.int64))
    _check_rows(got["rows"], torch.stack([x.r_rid, counts, *words], 1)[torch.sort(x.r_rid).indices])
    word = lambda d: "float64" if d in ("f64", "f32") else "int64"
    assert got["group_dtypes"] == [word(d) for d, _, _ in spec]
    empty = counts == 0  # empty groups carry the identities, in the accumulators' own bits
    for c, (dtype, how, _) in enumerate(spec):
        bits = {"sum": 0, "min": F64_INF, "max": F64_NINF}[how] if dtype in ("f64", "f32") else _identity(dtype, how)
        assert bool((got["aggs"][c][empty] == bits).all()), (c, dtype, how)
    if shape == "main" and case == "sum":  # the whole int64 range: some group's true sum does not fit
        v = x.column(0, "i64", 2, "cpu")[x.s_rid - RID_OFFSET]
        k = x.rk[int(torch.argmax(counts))]
        exact = sum(int(t) for t in v[x.sk == k].tolist())
        assert int(counts.max()) >= 8 and int(got["sums"][int(torch.argmax(counts))]) == (exact + 2**63) % 2**64 - 2**63


# -------------------------------------------- 2. device kernels vs the host twin
@pytest.mark.gpu
@pytest.mark.parametrize("shape,wide,case", _grid(), ids=[_ids(v) for v in _grid()])
def test_device_matches_host_twin(C, cuda, shape, wide, case):
    want, got = _host(shape, wide, case), _run_ops(shape, wide, case, "cuda")
    assert sorted(got) == sorted(want)
    for k in want:
        if isinstance(want[k], torch.Tensor):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
        else:
            assert got[k] == want[k], k
    if shape == "many":  # more items than workgroups: the persistent loop takes a second trip
        assert sum(1 for nr, ns in SHAPES["many"] if nr and ns) > 256 * 4


# ------------------------- 3. split columns and the direct-addressed count table
G_R, G_S = 40_000, 100_000


class Engine:
    """One generated 40,000 x 100,000 input per location and the value columns by outer rid (rids from 0)."""

    def __init__(self, C, loc):
        D = G_R // 2  # repeated inner keys; outer keys from D // 2 to 5 D / 2: partly without a partner
        inner = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=1234, domain=D)
        outer = C.GenSpec(distribution=C.KeyDistribution.UNIFORM, seed=4321, domain=2 * D, key_offset=D // 2)
        self.R, self.S = C.Relation(G_R, G_R, loc, 0), C.Relation(G_S, G_S, loc, 0)
        self.R.generate(inner, 0)
        self.S.generate(outer, 0)
        self.dev = "cuda" if loc == "device" else "cpu"
        self._base = {}

    def column(self, i, dtype, stride):
        key = (i, dtype, stride)
        if key not in self._base:
            g = torch.Generator().manual_seed(2000 + 10 * i + stride)
            n = G_S * stride
            base = (torch.randint(I64_MIN, I64_MAX, (n,), generator=g) if dtype == "i64" else
                    torch.randint(-2**31, 2**31, (n,), generator=g).to(torch.int32) if dtype == "i32" else
                    torch.randint(-1024, 1025, (n,), generator=g).to(DTYPES[dtype]))
            self._base[key] = base.to(self.dev)
        return self._base[key][stride - 1::stride]

    def rows(self, C, case, split=False, direct=True):
        spec = CASES[case]
        loc = "device" if self.dev == "cuda" else "host"
        cfg = C.JoinConfig()
        cfg.kind, cfg.materialize, cfg.r_chunk = C.JoinKind.GROUP, True, R_CHUNK
        cfg.split_local, cfg.direct_count, cfg.group_columns = split, direct, max(1, len(spec))
        ctx = _ctx(C, loc)
        j = C.HashJoin(self.R, self.S, ctx, cfg)
        cols = [self.column(i, d, st) for i, (d, _, st) in enumerate(spec)]
        if case == "count":
            res, rows = j.run(), j.output_groups()
        elif case == "sum":
            res, rows = j.join_group(ctx, cols[0], 0, G_S)
        else:
            res, rows = j.join_group_agg(ctx, cols, [a for _, a, _ in spec], 0, G_S)
        rows = rows.cpu()
        return j.plan, res, rows[torch.sort(rows[:, 0]).indices]


@functools.lru_cache(maxsize=None)
def _engine(C, loc):
    return Engine(C, loc)


@functools.lru_cache(maxsize=None)
def _engine_host_rows(C, case):
    return _engine(C, "host").rows(C, case)[1:]


@pytest.mark.parametrize("case", list(CASES))
def test_host_engine_is_a_group_by(C, case):
    """The host engine's rows -- the reference of the device runs below -- against the torch group-by."""
    e, spec = _engine(C, "host"), CASES[case]
    res, rows = _engine_host_rows(C, case)
    R, S = e.R.to_tensor(), e.S.to_tensor()

    class X:  # the fields _group_by reads
        rk, sk, s_rid, n_r = R[:, 0].contiguous(), S[:, 0].contiguous(), S[:, 1] + RID_OFFSET, G_R
        column = staticmethod(lambda i, d, st, dev: e.column(i, d, st))
    counts, words = _group_by(X, spec)
    assert 0.05 * G_R < int((counts == 0).sum()) < 0.95 * G_R and int(counts.max()) > 2
    _check_rows(rows, torch.stack([R[:, 1], counts, *words], 1)[torch.sort(R[:, 1]).indices])
    assert (res["matched_pairs"], res["unmatched_inner"]) == (int(counts.sum()), int((counts == 0).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES) + ["count-hashed"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "u64"])
def test_device_engine_matches_host_engine(C, cuda, split, case):
    """compressed and split layout; count only with fragments of at most 13 bits takes the direct-addressed table,
    with direct_count off (``count-hashed``) the hashed one."""
    direct, case = case != "count-hashed", case.split("-")[0]
    dev, (want_res, want) = _engine(C, "device"), _engine_host_rows(C, case)
    assert torch.equal(dev.R.to_tensor().cpu(), _engine(C, "host").R.to_tensor())
    assert torch.equal(dev.S.to_tensor().cpu(), _engine(C, "host").S.to_tensor())
    plan, res, rows = dev.rows(C, case, split, direct)
    frag_bits = plan.key_bits - plan.network_bits - plan.local_bits
    assert plan.split_local == split and not plan.wide and plan.r_chunk == R_CHUNK and 0 < frag_bits <= 13, plan
    _check_rows(rows, want)
    for k in ("matched_pairs", "unmatched_inner", "output_groups", "group_columns"):
        assert res[k] == want_res[k], k
