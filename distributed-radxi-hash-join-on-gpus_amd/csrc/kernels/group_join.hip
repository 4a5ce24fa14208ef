// Group joins (core::JoinKind::Group): per inner tuple r the number of outer
// tuples with r's key and the aggregates of C = 0 ... 4 outer value columns
// over those tuples -- the join followed by COUNT / SUM / MIN / MAX ... GROUP BY
// the build side, without ever forming a pair.  The columns are one
// GroupColumns (kernels.h: base pointer, element stride, aggregate and element
// type per column; n = 0 counts only) and the rows are (rid, count, agg_0, ...,
// agg_{C-1}), 2 + C words.  AVG is sum / count on the caller's side.
//
// Build/probe.  Both kernels are a persistent grid over the BPItem list with
// the geometry of bpOuterCountKernel: 256 threads, 16 tuples per thread and
// batch, the first inner and outer batch in flight while the table is cleared.
// Their phases are the same; groupHash, groupLoad, groupRid, groupInnerSlot and
// groupAggAtomic are shared, the batch dispatch, the build loop and the slot
// search are written out in both (why: profiles/group_unify/README.md).
//  * table: the key slots of the outer-join count, every inner copy in a slot
//    of its own (the only ds_cmpst of this file), next to one u32 counter and C
//    u64 accumulators per slot (column-major in LDS); only the *first* slot of
//    a key aggregates.  The clear writes each accumulator's identity.
//  * probe: an outer tuple stops at the first slot holding its key and does one
//    u32 LDS atomic and one 64-bit LDS atomic per column: it never walks the
//    chain of copies.  The rids come in with the keys (one 8-byte load per
//    compressed tuple instead of its high dword); wide tuples read the rid
//    word only of a tuple that found a slot (16 preloaded 8-byte rids next to
//    16 8-byte keys of either side spilled to scratch).  Column c's value is
//    element (rid - offset) * stride[c], loaded non-temporally; the C * G
//    gathers of G tuples are all issued before the first one is consumed, and
//    a tuple that found no slot forms no address.
//  * inner side: after a barrier every inner tuple (still in registers when the
//    item has one batch) looks up the first slot of its own key and applies
//    that slot's count and aggregates to the global accumulators at its
//    position rb + idx of the partitioned inner buffer, accAgg[c * accSlots +
//    position]: consecutive lanes hold consecutive positions.  An inner chunk
//    is shared by all outer chunks of its partition, so these are global
//    atomics, skipped when the item counted nothing for the tuple.  (A plain
//    store for partitions of a single outer chunk was not built: it needs a
//    second code path per item and nothing has measured the atomics as the
//    bottleneck.)  The item's pair total is the sum of the counts its inner
//    tuples read; *a.result gets one 64-bit atomic per workgroup.
// bpGroup() alone decides which kernel runs:
//  * bpGroupKernel<LAYOUT, DIRECT, SUM> -- no column, or one int64 column with
//    SUM: no run-time branch on an aggregate or a type, G = 16 (wide tuples with
//    SUM: 8).  DIRECT (4-byte fragments of at most 13 bits, count only):
//    table[fragment] is the number of outer tuples of the fragment; no build,
//    the probe adds one per outer tuple, the inner tuples read their fragment's
//    counter.  DIRECT is not built with columns: the accumulators would be 12 B
//    per fragment (96 KiB + 64 B at 13 bits, one workgroup per CU) and an outer
//    tuple without a partner would still gather its value.
//  * bpGroupAggKernel<LAYOUT, C, TYPED> -- everything else.  The aggregate code
//    (and with TYPED the element type) of each column is a kernel argument,
//    wave-uniform and branched on in scalar code.  G shrinks with C (16, 8, 4,
//    4; wide tuples 8, 4, 2, 2) so that nothing spills.  TYPED = false: every
//    column is int64.  TYPED = true (any column int32, float64 or float32): the
//    gather is a 4- or 8-byte load into a dword pair kept as loaded, so the
//    gathers are still issued before the first wait; the widening happens at
//    the atomic: int32 sign-extended, float32 converted to binary64
//    (v_cvt_f64_f32, exact).  Accumulators stay 8 bytes per column and slot, so
//    the LDS layout, the planned rChunk and G do not depend on TYPED.
// Arithmetic: integer columns accumulate as int64 (SUM wraps, MIN / MAX signed);
// float columns hold binary64 bits -- SUM in the order the atomics land, MIN /
// MAX as IEEE numbers, NaN inputs and the order of -0.0 / +0.0 unspecified.
// Identities (groupAggIdentity): 0, INT64_MAX, INT64_MIN; +0.0, +inf, -inf.
// The global accumulators must hold them before the launch: groupAggInit (a
// zeroWords clear when every column is a SUM, groupAggFillKernel otherwise).
// All 64-bit atomics are native on gfx950 -- ds_add_u64 / ds_min_i64 / ds_max_i64 /
// ds_add_f64 / ds_min_f64 / ds_max_f64 and global_atomic_add_x2 / smin_x2 /
// smax_x2 / add_f64 / min_f64 / max_f64, no compare-and-swap loop and no
// -munsafe-fp-atomics (read once in the assembly, hipcc of ROCm 7).  The
// hardware float atomics are valid on coarse-grained memory only: the global
// accumulators live in the engine's Arena or a torch tensor (hipMalloc) and
// must stay there.
//
// Rows.  groupUnitLengths / groupEmitKernel<LAYOUT, C> -- one wave per unit of
// the inner side (markPlanUnits / markEmitUnits over outerSwapSides(a, unit),
// also for partitions without outer tuples, which got no work item).  Every
// valid position is selected, so a unit's row count is its length and the row
// offsets come from the u32-to-u64 scan.  C = 0 stores one 16-byte row per
// lane; C >= 1 stores word q of the wave's run from lane q % 64, the columns
// interleaved through lane shuffles, so the stores stay consecutive 8-byte
// words although W = 2 + C is no power of two.  The kernel only moves 8-byte
// words: the bits of a float column pass through unchanged, and empty groups
// carry the identities.  Zero counts are added to *a.result; without `out` the
// kernel only counts them.  Positions outside [partS, partSEnd) -- the gaps of
// a sampled local pass -- are never read.
//
// Count accumulators are u32: the caller refuses a global outer size of 2^32
// or more (HashJoin, ops.build_probe_group).
//
// Layouts (template LAYOUT): u64 CompressedTuples, split columns, wide 16-byte
// tuples.  Key-only words are refused (no rid to report).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// kernel uses scratch; per kernel in profiles/group_unify/README.md):
//   bpGroupKernel<compressed>        121 VGPRs hashed, 120 direct; 3 workgroups per CU
//   bpGroupKernel<split>             108 VGPRs hashed and direct; 4 workgroups per CU
//   bpGroupKernel<wide>              176 VGPRs; 2 workgroups per CU
//   bpGroupKernel<compressed, SUM>   234 VGPRs; 2 workgroups per CU
//   bpGroupKernel<split, SUM>        186 VGPRs; 2 workgroups per CU
//   bpGroupKernel<wide, SUM>         192 VGPRs; 2 workgroups per CU
//   bpGroupAggKernel<compressed, C>  238 / 240 / 234 / 248 VGPRs for C = 1 / 2 / 3 / 4; 2 workgroups per CU
//   bpGroupAggKernel<split, C>       186 / 188 / 182 / 196 VGPRs; 2 workgroups per CU
//   bpGroupAggKernel<wide, C>        212 / 206 / 200 / 206 VGPRs; 2 workgroups per CU
//   bpGroupAggKernel<*, C, TYPED>    the VGPRs of TYPED = false (split, C = 3: 183) and 5 - 17 more SGPRs (at most
//                                    106).  The C = 4 instantiations keep 12 (compressed), 15 (split) and 13 (wide)
//                                    SGPRs in VGPR lanes, split C = 3 keeps 2 (SGPR spills inside the VGPR counts
//                                    above: no scratch, no VGPR spill)
//   groupEmitKernel<*, C>            28-30 / 52-54 / 62-64 / 73-76 / 86-87 VGPRs for C = 0 ... 4; 32 B LDS
//   groupUnitLengthsKernel           12 VGPRs, no LDS
//   groupAggFillKernel               10 VGPRs, no LDS
//   LDS (dynamic, bpGroupLdsBytes): slots * (key + 4 + 8 C) + 64 B, slots = groupMaxSlots(rChunk).  4-byte keys at
//   the planned rChunk 2048 / 2048 / 1024 / 1024 / 512 for C = 0 ... 4: 32 / 64 / 48 / 64 / 40 KiB + 64 B; 8-byte
//   keys at 1024 / 1024 / 1024 / 1024 / 512: 24 / 40 / 56 / 72 / 44 KiB + 64 B; direct 4 B << fragBits + 64 B (32
//   KiB + 64 B at 13 bits).  A request above 160 KiB is refused by bpGroup.
#include "kernels.h"
#include "device_common.h"
#include "mark_units.h"

#include <algorithm>
#include <type_traits>

namespace hpcjoin {
namespace kernels {

constexpr int GJ_T = 256;
constexpr int GJ_K = 16;  // tuples per thread per batch (as the counting build/probe)
constexpr uint32_t GJ_BATCH = GJ_T * GJ_K;
constexpr uint32_t GJ_EMPTY32 = 0xFFFFFFFFu;
constexpr unsigned long long GJ_EMPTY64 = ~0ull;
constexpr uint32_t GJ_NONE = 0xFFFFFFFFu;  // probe: no slot holds the key
constexpr uint32_t GJ_DIRECT_MAX_BITS = 13;

template <int LAYOUT>
struct GroupKey {
  using type = typename std::conditional<LAYOUT == MK_WIDE, unsigned long long, uint32_t>::type;
  static constexpr type EMPTY = LAYOUT == MK_WIDE ? (type)GJ_EMPTY64 : (type)GJ_EMPTY32;
};
// Rid registers of the outer side: the whole CompressedTuple, the u32 rid column, the Tuple's rid.
template <int LAYOUT>
struct GroupRid {
  using type = typename std::conditional<LAYOUT == MK_SPLIT, uint32_t, unsigned long long>::type;
};

template <int LAYOUT, typename K>
__device__ __forceinline__ uint32_t groupHash(K key, uint32_t tbits) {
  if constexpr (LAYOUT == MK_WIDE)
    return (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> (64 - tbits));
  else
    return ((uint32_t)key * 2654435761u) >> (32 - tbits);
}

// ------------------------------------------------- phases of the build/probe
// One batch of an item's keys into registers; RIDS: the rids as well.
template <int LAYOUT, bool FULL, bool RIDS, typename K, typename R, int NR>
__device__ __forceinline__ void groupLoad(const void *__restrict__ src, const uint16_t *__restrict__ hi, uint64_t off,
                                          uint32_t n, uint32_t b0, uint32_t fragShift, K (&v)[GJ_K], R (&r)[NR]) {
  static_assert(!RIDS || NR == GJ_K, "one rid register per tuple");
#pragma unroll
  for (int k = 0; k < GJ_K; ++k) {
    const uint32_t idx = b0 + k * GJ_T + threadIdx.x;
    if (FULL || idx < n) {
      if constexpr (LAYOUT == MK_SPLIT) {
        v[k] = hi[off + idx];
        if constexpr (RIDS) r[k] = reinterpret_cast<const uint32_t *>(src)[off + idx];
      } else if constexpr (LAYOUT == MK_COMPRESSED) {
        if constexpr (RIDS) {  // one 8-byte load: the fragment is taken from it, the rid field masked at use
          r[k] = reinterpret_cast<const unsigned long long *>(src)[off + idx];
          v[k] = (uint32_t)(r[k] >> fragShift);
        } else {  // fragShift >= keyShift >= 32: the fragment lies in the high dword
          v[k] = reinterpret_cast<const uint32_t *>(src)[2 * (off + idx) + 1] >> (fragShift - 32);
        }
      } else {
        v[k] = reinterpret_cast<const unsigned long long *>(src)[2 * (off + idx)];
        if constexpr (RIDS) r[k] = reinterpret_cast<const unsigned long long *>(src)[2 * (off + idx) + 1];
      }
    }
  }
}
// The rid in a register groupLoad<.., RIDS> filled.
template <int LAYOUT, typename R>
__device__ __forceinline__ uint64_t groupRid(R r, uint64_t ridMask) {
  return LAYOUT == MK_COMPRESSED ? ((uint64_t)r & ridMask) : (uint64_t)r;
}

// Inner side: the first slot of the key (it is in the table: this tuple inserted it).
template <int LAYOUT, bool DIRECT, typename K>
__device__ __forceinline__ uint32_t groupInnerSlot(const K *table, K key, uint32_t tbits, uint32_t mask) {
  if constexpr (DIRECT) {
    return (uint32_t)key & mask;
  } else {
    uint32_t h = groupHash<LAYOUT>(key, tbits);
    while (table[h] != key) h = (h + 1) & mask;
    return h;
  }
}

static bool groupDirect(const BPArgs &a, bool columns) {
  return !columns && !a.wide && a.fragBits > 0 && a.fragBits <= GJ_DIRECT_MAX_BITS;
}

// (HIP launch bounds: the second value is workgroups per CU, as bpOuterCountKernel; SUM holds the rids and 16
// gathered values next to the keys.)
template <int LAYOUT, bool DIRECT, bool SUM>
__global__ __launch_bounds__(GJ_T, LAYOUT == MK_WIDE || SUM ? 2 : LAYOUT == MK_SPLIT ? 4 : 3) void bpGroupKernel(
    BPArgs a, const BPItem *__restrict__ items, const uint32_t *__restrict__ nItemsPtr, uint32_t capacity,
    const unsigned long long *__restrict__ values, uint64_t ridOffset, uint64_t stride, uint32_t *accCount,
    unsigned long long *accSum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using K = typename GroupKey<LAYOUT>::type;
  using R = typename GroupRid<LAYOUT>::type;
  constexpr K EMPTY = GroupKey<LAYOUT>::EMPTY;
  constexpr bool PRE_RID = SUM && LAYOUT != MK_WIDE;  // wide tuples read their rid when a slot was found
  static_assert(!DIRECT || (LAYOUT != MK_WIDE && !SUM), "direct-addressed tables count 4-byte fragments");
  const uint64_t maxSlots = DIRECT ? (uint64_t(1) << a.fragBits) : groupMaxSlots(a.rChunk);
  // [sum u64 x slots][key x slots][count u32 x slots][8 x u64 reduction words]; DIRECT: [count u32 x slots][...]
  unsigned long long *sums = reinterpret_cast<unsigned long long *>(smem);
  K *table = reinterpret_cast<K *>(smem + (SUM ? maxSlots * 8 : 0));
  uint32_t *cnt = DIRECT ? reinterpret_cast<uint32_t *>(smem)
                         : reinterpret_cast<uint32_t *>(smem + (SUM ? maxSlots * 8 : 0) + maxSlots * sizeof(K));
  unsigned long long *wsum = reinterpret_cast<unsigned long long *>(
      smem + (DIRECT ? maxSlots * 4 : maxSlots * ((SUM ? 8 : 0) + sizeof(K) + 4)));
  const uint32_t t = threadIdx.x;
  const uint32_t nItems = min(*nItemsPtr, capacity);
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  unsigned long long matches = 0;
  for (uint32_t w = blockIdx.x; w < nItems; w += gridDim.x) {
    const BPItem it = items[w];
    const uint64_t rb = a.partR[it.part] + (uint64_t)it.rChunk * a.rChunk;
    const uint64_t re = min(a.partREnd[it.part], rb + a.rChunk);
    const uint64_t sb = a.partS[it.part] + (uint64_t)it.sChunk * a.sChunk;
    const uint64_t se = min(a.partSEnd[it.part], sb + a.sChunk);
    const uint32_t nr = (uint32_t)(re - rb), ns = (uint32_t)(se - sb);
    uint32_t tbits = DIRECT ? a.fragBits : ceilLog2(2ull * nr);
    if (!DIRECT && tbits < 6) tbits = 6;
    const uint32_t slots = 1u << tbits, mask = slots - 1;

    // First inner batch and first outer batch are in flight while the table is cleared.
    K rv[GJ_K], sv[GJ_K];
    R rr[PRE_RID ? GJ_K : 1], nor[1];
    if (nr >= GJ_BATCH) groupLoad<LAYOUT, true, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv, nor);
    else groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv, nor);
    if (ns >= GJ_BATCH) groupLoad<LAYOUT, true, PRE_RID>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
    else groupLoad<LAYOUT, false, PRE_RID>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
    for (uint32_t i = t; i < slots; i += GJ_T) {
      cnt[i] = 0;
      if constexpr (!DIRECT) table[i] = EMPTY;
      if constexpr (SUM) sums[i] = 0;
    }
    __syncthreads();

    // ---- build: every inner copy takes a slot (DIRECT: nothing to build)
    if constexpr (!DIRECT) {
      for (uint32_t b0 = 0; b0 < nr; b0 += GJ_BATCH) {
        if (b0) groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv, nor);
#pragma unroll
        for (int k = 0; k < GJ_K; ++k) {
          if (b0 + k * GJ_T + t < nr) {
            const K key = rv[k];
            uint32_t h = groupHash<LAYOUT>(key, tbits);
            while (atomicCAS(&table[h], EMPTY, key) != EMPTY) h = (h + 1) & mask;
          }
        }
      }
      __syncthreads();
    }

    // ---- probe: the first slot of the key, one LDS atomic (SUM: two)
    for (uint32_t b0 = 0; b0 < ns; b0 += GJ_BATCH) {
      if (b0) {
        if (b0 + GJ_BATCH <= ns) groupLoad<LAYOUT, true, PRE_RID>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
        else groupLoad<LAYOUT, false, PRE_RID>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
      }
      if constexpr (DIRECT) {
#pragma unroll
        for (int k = 0; k < GJ_K; ++k)
          if (b0 + k * GJ_T + t < ns) atomicAdd(&cnt[sv[k] & mask], 1u);  // (fragments are < 2^fragBits)
      } else {
        // G tuples at a time: their slots, then (SUM) all G gathers issued before the first value is consumed.
        constexpr int G = SUM && LAYOUT == MK_WIDE ? 8 : GJ_K;
#pragma unroll
        for (int g0 = 0; g0 < GJ_K; g0 += G) {
          uint32_t slot[G];
#pragma unroll
          for (int j = 0; j < G; ++j) {
            slot[j] = GJ_NONE;
            if (b0 + (g0 + j) * GJ_T + t < ns) {
              const K key = sv[g0 + j];
              uint32_t h = groupHash<LAYOUT>(key, tbits);
              K e;
              while ((e = table[h]) != EMPTY) {
                if (e == key) {
                  slot[j] = h;
                  break;
                }
                h = (h + 1) & mask;
              }
            }
          }
          if constexpr (SUM) {
            unsigned long long val[G];
            if constexpr (!PRE_RID) {
#pragma unroll
              for (int j = 0; j < G; ++j)
                if (slot[j] != GJ_NONE)
                  val[j] = reinterpret_cast<const unsigned long long *>(a.S)[2 * (sb + b0 + (g0 + j) * GJ_T + t) + 1];
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
              if (slot[j] != GJ_NONE) {  // a tuple that found no slot forms no address
                uint64_t rid;
                if constexpr (!PRE_RID) rid = val[j];
                else rid = groupRid<LAYOUT>(rr[g0 + j], ridMask);
                val[j] = __builtin_nontemporal_load(values + (rid - ridOffset) * stride);
              }
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
              if (slot[j] != GJ_NONE) {
                atomicAdd(&cnt[slot[j]], 1u);
                atomicAdd(&sums[slot[j]], val[j]);
              }
            }
          } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
              if (slot[j] != GJ_NONE) atomicAdd(&cnt[slot[j]], 1u);
          }
        }
      }
    }
    __syncthreads();

    // ---- inner side: count and sum of the first slot of every inner tuple's key
    for (uint32_t b0 = 0; b0 < nr; b0 += GJ_BATCH) {
      if (nr > GJ_BATCH) groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv, nor);  // else in registers
#pragma unroll
      for (int k = 0; k < GJ_K; ++k) {
        const uint32_t idx = b0 + k * GJ_T + t;
        if (idx < nr) {
          const uint32_t h = groupInnerSlot<LAYOUT, DIRECT>(table, rv[k], tbits, mask);
          const uint32_t c = cnt[h];
          if (c) {
            matches += c;
            atomicAdd(&accCount[rb + idx], c);
            if constexpr (SUM) atomicAdd(&accSum[rb + idx], sums[h]);
          }
        }
      }
    }
    __syncthreads();  // the next item clears the table
  }
  const unsigned long long total = blockReduceSum<GJ_T, unsigned long long>(matches, wsum);
  if (t == 0 && total) atomicAdd(a.result, total);
}

// ------------------------------------------------------ aggregated columns
// Values of one column in flight per thread before the first is consumed: 16 (wide tuples 8) divided by the
// columns, as a power of two -- C * G 8-byte values next to the keys and rids of both sides.
constexpr int groupAggBatch(int layout, int c) {
  const int g = (layout == MK_WIDE ? 8 : GJ_K) / c;
  return g >= 16 ? 16 : g >= 8 ? 8 : g >= 4 ? 4 : 2;
}

// One accumulator update in LDS (SCOPE workgroup) or on the global accumulators (agent).  The aggregate code is
// wave-uniform (a kernel argument): one scalar branch per atomic.  TYPED: so is the column's type; a floating-point
// accumulator holds the bits of a binary64 and takes the f64 atomics (add, IEEE min, IEEE max).
template <int SCOPE, bool TYPED>
__device__ __forceinline__ void groupAggAtomic(unsigned long long *p, unsigned long long v, uint32_t agg, uint32_t dtype) {
  if (TYPED && groupDtypeIsFloat(dtype)) {
    double *d = reinterpret_cast<double *>(p);
    const double x = __longlong_as_double((long long)v);
    if (agg == GROUP_SUM) __hip_atomic_fetch_add(d, x, __ATOMIC_RELAXED, SCOPE);
    else if (agg == GROUP_MIN) __hip_atomic_fetch_min(d, x, __ATOMIC_RELAXED, SCOPE);
    else __hip_atomic_fetch_max(d, x, __ATOMIC_RELAXED, SCOPE);
  } else {
    long long *i = reinterpret_cast<long long *>(p);
    if (agg == GROUP_SUM) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE);
    else if (agg == GROUP_MIN) __hip_atomic_fetch_min(i, (long long)v, __ATOMIC_RELAXED, SCOPE);
    else __hip_atomic_fetch_max(i, (long long)v, __ATOMIC_RELAXED, SCOPE);
  }
}

// TYPED gather: element idx of a column of 8- or 4-byte elements, as loaded, in two dwords; a 4-byte element leaves
// `hi` alone (writing a zero there would have to wait for the gathers still in flight).  groupWiden turns the pair
// into the accumulator's word when it is consumed, so no load is waited for early.
__device__ __forceinline__ void groupGather(const void *col, uint64_t idx, uint32_t dtype, uint32_t &lo, uint32_t &hi) {
  if (groupDtypeBytes(dtype) == 4) {
    lo = __builtin_nontemporal_load(static_cast<const uint32_t *>(col) + idx);
  } else {
    const unsigned long long v = __builtin_nontemporal_load(static_cast<const unsigned long long *>(col) + idx);
    lo = (uint32_t)v;
    hi = (uint32_t)(v >> 32);
  }
}
__device__ __forceinline__ unsigned long long groupWiden(uint32_t lo, uint32_t hi, uint32_t dtype) {
  if (dtype == GROUP_I32) return (unsigned long long)(long long)(int32_t)lo;                          // sign-extended
  if (dtype == GROUP_F32) return (unsigned long long)__double_as_longlong((double)__uint_as_float(lo));  // exact
  return ((unsigned long long)hi << 32) | lo;
}

// Every column's identity over its accSlots accumulators (column-major).
__global__ __launch_bounds__(GJ_T) void groupAggFillKernel(GroupColumns cols, unsigned long long *__restrict__ accAgg,
                                                          uint64_t accSlots) {
  for (uint32_t c = 0; c < cols.n; ++c) {
    const unsigned long long ident = groupAggIdentity(cols.agg[c], cols.dtype[c]);
    for (uint64_t i = (uint64_t)blockIdx.x * GJ_T + threadIdx.x; i < accSlots; i += (uint64_t)gridDim.x * GJ_T)
      accAgg[c * accSlots + i] = ident;
  }
}

template <int LAYOUT, int C, bool TYPED>
__global__ __launch_bounds__(GJ_T, 2) void bpGroupAggKernel(BPArgs a, const BPItem *__restrict__ items,
                                                            const uint32_t *__restrict__ nItemsPtr, uint32_t capacity,
                                                            GroupColumns cols, uint32_t *accCount,
                                                            unsigned long long *accAgg, uint64_t accSlots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using K = typename GroupKey<LAYOUT>::type;
  using R = typename GroupRid<LAYOUT>::type;
  constexpr K EMPTY = GroupKey<LAYOUT>::EMPTY;
  constexpr bool PRE_RID = LAYOUT != MK_WIDE;  // wide tuples read their rid when a slot was found
  constexpr int G = groupAggBatch(LAYOUT, C);  // (TYPED holds the values as loaded: no more VGPRs, the same G)
  const uint64_t maxSlots = groupMaxSlots(a.rChunk);
  // [agg u64 x slots] x C (column-major) [key x slots][count u32 x slots][8 x u64 reduction words]
  unsigned long long *aggs = reinterpret_cast<unsigned long long *>(smem);
  K *table = reinterpret_cast<K *>(smem + maxSlots * 8 * C);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(smem + maxSlots * (8 * C + sizeof(K)));
  unsigned long long *wsum = reinterpret_cast<unsigned long long *>(smem + maxSlots * (8 * C + sizeof(K) + 4));
  const uint32_t t = threadIdx.x;
  const uint32_t nItems = min(*nItemsPtr, capacity);
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  unsigned long long ident[C];
#pragma unroll
  for (int c = 0; c < C; ++c) ident[c] = groupAggIdentity(cols.agg[c], TYPED ? cols.dtype[c] : (uint32_t)GROUP_I64);
  unsigned long long matches = 0;
  for (uint32_t w = blockIdx.x; w < nItems; w += gridDim.x) {
    const BPItem it = items[w];
    const uint64_t rb = a.partR[it.part] + (uint64_t)it.rChunk * a.rChunk;
    const uint64_t re = min(a.partREnd[it.part], rb + a.rChunk);
    const uint64_t sb = a.partS[it.part] + (uint64_t)it.sChunk * a.sChunk;
    const uint64_t se = min(a.partSEnd[it.part], sb + a.sChunk);
    const uint32_t nr = (uint32_t)(re - rb), ns = (uint32_t)(se - sb);
    uint32_t tbits = ceilLog2(2ull * nr);
    if (tbits < 6) tbits = 6;
    const uint32_t slots = 1u << tbits, mask = slots - 1;

    // First inner batch and first outer batch are in flight while the table is cleared.
    K rv[GJ_K], sv[GJ_K];
    R rr[PRE_RID ? GJ_K : 1], nor[1];
    if (nr >= GJ_BATCH) groupLoad<LAYOUT, true, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv, nor);
    else groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv, nor);
    if (ns >= GJ_BATCH) groupLoad<LAYOUT, true, PRE_RID>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
    else groupLoad<LAYOUT, false, PRE_RID>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
    for (uint32_t i = t; i < slots; i += GJ_T) {
      cnt[i] = 0;
      table[i] = EMPTY;
#pragma unroll
      for (int c = 0; c < C; ++c) aggs[c * maxSlots + i] = ident[c];  // not all zeros: MIN and MAX
    }
    __syncthreads();

    // ---- build: every inner copy takes a slot
    for (uint32_t b0 = 0; b0 < nr; b0 += GJ_BATCH) {
      if (b0) groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv, nor);
#pragma unroll
      for (int k = 0; k < GJ_K; ++k) {
        if (b0 + k * GJ_T + t < nr) {
          const K key = rv[k];
          uint32_t h = groupHash<LAYOUT>(key, tbits);
          while (atomicCAS(&table[h], EMPTY, key) != EMPTY) h = (h + 1) & mask;
        }
      }
    }
    __syncthreads();

    // ---- probe: the first slot of the key, one u32 LDS atomic and one 64-bit LDS atomic per column
    for (uint32_t b0 = 0; b0 < ns; b0 += GJ_BATCH) {
      if (b0) {
        if (b0 + GJ_BATCH <= ns) groupLoad<LAYOUT, true, PRE_RID>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
        else groupLoad<LAYOUT, false, PRE_RID>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
      }
      // G tuples at a time: their slots, then all C * G gathers issued before the first value is consumed.
#pragma unroll
      for (int g0 = 0; g0 < GJ_K; g0 += G) {
        uint32_t slot[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
          slot[j] = GJ_NONE;
          if (b0 + (g0 + j) * GJ_T + t < ns) {
            const K key = sv[g0 + j];
            uint32_t h = groupHash<LAYOUT>(key, tbits);
            K e;
            while ((e = table[h]) != EMPTY) {
              if (e == key) {
                slot[j] = h;
                break;
              }
              h = (h + 1) & mask;
            }
          }
        }
        unsigned long long wrid[PRE_RID ? 1 : G];
        if constexpr (!PRE_RID) {
#pragma unroll
          for (int j = 0; j < G; ++j)
            if (slot[j] != GJ_NONE)
              wrid[j] = reinterpret_cast<const unsigned long long *>(a.S)[2 * (sb + b0 + (g0 + j) * GJ_T + t) + 1];
        }
        unsigned long long val[TYPED ? 1 : C][TYPED ? 1 : G];
        uint32_t vlo[TYPED ? C : 1][TYPED ? G : 1], vhi[TYPED ? C : 1][TYPED ? G : 1];  // TYPED: as loaded
#pragma unroll
        for (int j = 0; j < G; ++j) {
          if (slot[j] != GJ_NONE) {  // a tuple that found no slot forms no address
            uint64_t rid;
            if constexpr (!PRE_RID) rid = wrid[j];
            else rid = groupRid<LAYOUT>(rr[g0 + j], ridMask);
            const uint64_t row = rid - cols.offset;
#pragma unroll
            for (int c = 0; c < C; ++c) {
              if constexpr (TYPED)
                groupGather(cols.col[c], row * cols.stride[c], cols.dtype[c], vlo[c][j], vhi[c][j]);
              else
                val[c][j] = __builtin_nontemporal_load(static_cast<const unsigned long long *>(cols.col[c]) +
                                                       row * cols.stride[c]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
          if (slot[j] != GJ_NONE) {
            atomicAdd(&cnt[slot[j]], 1u);
#pragma unroll
            for (int c = 0; c < C; ++c) {
              unsigned long long v;
              if constexpr (TYPED) v = groupWiden(vlo[c][j], vhi[c][j], cols.dtype[c]);
              else v = val[c][j];
              groupAggAtomic<__HIP_MEMORY_SCOPE_WORKGROUP, TYPED>(&aggs[c * maxSlots + slot[j]], v, cols.agg[c],
                                                                  cols.dtype[c]);
            }
          }
        }
      }
    }
    __syncthreads();

    // ---- inner side: count and aggregates of the first slot of every inner tuple's key
    for (uint32_t b0 = 0; b0 < nr; b0 += GJ_BATCH) {
      if (nr > GJ_BATCH) groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv, nor);  // else in registers
#pragma unroll
      for (int k = 0; k < GJ_K; ++k) {
        const uint32_t idx = b0 + k * GJ_T + t;
        if (idx < nr) {
          const uint32_t h = groupInnerSlot<LAYOUT, false>(table, rv[k], tbits, mask);
          const uint32_t c0 = cnt[h];
          if (c0) {
            matches += c0;
            atomicAdd(&accCount[rb + idx], c0);
#pragma unroll
            for (int c = 0; c < C; ++c)
              groupAggAtomic<__HIP_MEMORY_SCOPE_AGENT, TYPED>(&accAgg[c * accSlots + rb + idx], aggs[c * maxSlots + h],
                                                              cols.agg[c], cols.dtype[c]);
          }
        }
      }
    }
    __syncthreads();  // the next item clears the table
  }
  const unsigned long long total = blockReduceSum<GJ_T, unsigned long long>(matches, wsum);
  if (t == 0 && total) atomicAdd(a.result, total);
}

// ------------------------------------------------------------------- units
__global__ __launch_bounds__(GJ_T) void groupUnitLengthsKernel(BPArgs a, const MarkUnit *__restrict__ units,
                                                              const uint32_t *__restrict__ nUnitsPtr, uint32_t capacity,
                                                              uint32_t *__restrict__ unitCounts) {
  const uint32_t nUnits = min(*nUnitsPtr, capacity);
  for (uint32_t u = blockIdx.x * GJ_T + threadIdx.x; u < nUnits; u += gridDim.x * GJ_T) {
    uint64_t ub, ue;
    unitRange(a, units[u], ub, ue);
    unitCounts[u] = (uint32_t)(ue - ub);
  }
}

// One wave per unit of a.S (the inner relation: sides swapped by the caller); rows of W = 2 + C words.
template <int LAYOUT, int C>
__global__ __launch_bounds__(GJ_T) void groupEmitKernel(BPArgs a, const MarkUnit *__restrict__ units,
                                                       const uint32_t *__restrict__ nUnitsPtr, uint32_t capacity,
                                                       const uint32_t *__restrict__ accCount,
                                                       const unsigned long long *__restrict__ accAgg, uint64_t accSlots,
                                                       const unsigned long long *__restrict__ unitOffsets,
                                                       unsigned long long *__restrict__ out, uint64_t outCapacity) {
  constexpr uint32_t W = 2 + C;
  __shared__ unsigned long long wsum[GJ_T / WAVE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  const uint32_t nUnits = min(*nUnitsPtr, capacity);
  const uint32_t wavesPerGrid = gridDim.x * (GJ_T / WAVE);
  unsigned long long zeros = 0;
  for (uint32_t u = blockIdx.x * (GJ_T / WAVE) + threadIdx.x / WAVE; u < nUnits; u += wavesPerGrid) {
    uint64_t ub, ue;
    unitRange(a, units[u], ub, ue);
    const unsigned long long base = out ? unitOffsets[u] : 0ull;
    for (uint64_t p0 = ub; p0 < ue; p0 += WAVE) {  // wave-uniform
      const uint32_t m = (uint32_t)min((uint64_t)WAVE, ue - p0);
      const bool valid = lane < m;
      const uint32_t c = valid ? accCount[p0 + lane] : 1u;
      zeros += c == 0;
      if (!out) continue;
      const unsigned long long row0 = base + (p0 - ub);  // the wave's first output row
      const unsigned long long rid = valid ? markRid<LAYOUT>(a, p0 + lane, ridMask) : 0ull;
      if constexpr (C == 0) {
        if (valid && row0 + lane < outCapacity)
          reinterpret_cast<ulonglong2 *>(out)[row0 + lane] = make_ulonglong2(rid, (unsigned long long)c);
      } else {
        unsigned long long g[C];
#pragma unroll
        for (int j = 0; j < C; ++j) g[j] = valid ? accAgg[j * accSlots + p0 + lane] : 0ull;
        // word q of the run (row q / W, column q % W) is stored by lane q % 64: consecutive 8-byte stores
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) {
          const uint32_t q = WAVE * k + lane, src = q / W, col = q - src * W;
          const unsigned long long vr = __shfl(rid, src, WAVE);
          const uint32_t vc = __shfl(c, src, WAVE);
          unsigned long long v = col == 0 ? vr : (unsigned long long)vc;
#pragma unroll
          for (int j = 0; j < C; ++j) {
            const unsigned long long vg = __shfl(g[j], src, WAVE);
            if (col == 2u + j) v = vg;
          }
          if (src < m && row0 + src < outCapacity) out[row0 * W + q] = v;
        }
      }
    }
  }
  const unsigned long long total = blockReduceSum<GJ_T, unsigned long long>(zeros, wsum);
  if (threadIdx.x == 0 && total) atomicAdd(a.result, total);
}

// --------------------------------------------------------------- launchers
// Small units are latency-bound per wave: the grid fills every CU with waves (as semi_join.hip).
static uint32_t groupUnitGrid(uint32_t capacity) {
  const uint32_t perBlock = GJ_T / WAVE;
  return std::max<uint32_t>(1, std::min<uint32_t>(256 * 8, (capacity + perBlock - 1) / perBlock));
}

// The arguments with both end arrays set, after the checks every group kernel needs.
static BPArgs groupArgs(const BPArgs &args, const char *who) {
  BPArgs a = args;
  if (!a.partREnd) a.partREnd = a.partR + 1;
  if (!a.partSEnd) a.partSEnd = a.partS + 1;
  HJ_CHECK(!a.keyOnly, "%s: key-only words carry no rid (group joins use rid-carrying layouts)", who);
  HJ_CHECK(!(a.split && a.wide), "%s: the split layout holds compressed tuples", who);
  return a;
}

static void groupColumnsCheck(const GroupColumns &cols, const char *who) {
  HJ_CHECK(cols.n <= GROUP_MAX_COLUMNS, "%s: %u value columns (0 to %u)", who, cols.n, GROUP_MAX_COLUMNS);
  for (uint32_t c = 0; c < cols.n; ++c)
    // (cols.rows == 0: a column without storage; the callers' cover checks then admit no outer tuple to read it for.)
    HJ_CHECK((cols.col[c] || cols.rows == 0) && cols.stride[c] >= 1 && cols.agg[c] <= GROUP_MAX &&
                 cols.dtype[c] <= GROUP_DTYPE_MAX &&
                 reinterpret_cast<uintptr_t>(cols.col[c]) % groupDtypeBytes(cols.dtype[c]) == 0,
             "%s: column %u needs aligned values, a stride >= 1, an aggregate (sum, min, max) and an element type "
             "(int64, int32, float64, float32)",
             who, c);
}

size_t bpGroupLdsBytes(const BPArgs &a, uint32_t columns) {
  if (groupDirect(a, columns != 0)) return (size_t(4) << a.fragBits) + 64;
  return groupTableBytes(a.rChunk, a.wide, columns);
}

void groupAggInit(const GroupColumns &cols, unsigned long long *accAgg, uint64_t accSlots, hipStream_t s) {
  if (cols.n == 0 || accSlots == 0) return;
  groupColumnsCheck(cols, "groupAggInit");
  HJ_CHECK(accAgg, "groupAggInit: needs the accumulators");
  bool zero = true;
  for (uint32_t c = 0; c < cols.n; ++c) zero = zero && groupAggIdentity(cols.agg[c], cols.dtype[c]) == 0;
  if (zero) {  // (the engine's own clear, as ExecContext::zero)
    zeroWords(accAgg, cols.n * accSlots, s);
    return;
  }
  const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(256 * 8, (accSlots + GJ_T - 1) / GJ_T));
  hipLaunchKernelGGL(groupAggFillKernel, dim3(blocks), dim3(GJ_T), 0, s, cols, accAgg, accSlots);
  HIP_CHECK_LAUNCH();
}

void bpGroup(const BPArgs &args, const BPItem *items, const uint32_t *nItems, uint32_t capacity,
             const GroupColumns &cols, uint32_t *accCount, unsigned long long *accAgg, uint64_t accSlots,
             hipStream_t s) {
  if (capacity == 0) return;
  groupColumnsCheck(cols, "bpGroup");
  const BPArgs a = groupArgs(args, "bpGroup");
  const size_t lds = bpGroupLdsBytes(a, cols.n);
  HJ_CHECK(lds <= 160 * 1024, "bpGroup: LDS request %zu exceeds 160 KiB (rChunk=%u, %u value columns)", lds, a.rChunk,
           cols.n);
  HJ_CHECK(!a.split || (a.Rhi && a.Shi), "bpGroup: split layout without fragment columns");
  HJ_CHECK(a.wide || a.fragShift >= 32, "bpGroup: fragShift=%u < 32 (the rid field of a CompressedTuple is >= 32 bits)",
           a.fragShift);
  HJ_CHECK(a.result && accCount && (cols.n == 0 || accAgg), "bpGroup: needs the pair counter and the accumulators");
  const bool typed = groupColumnsTyped(cols);
  // No column, or one int64 SUM: the kernel without run-time aggregate branches.
  const bool single = cols.n == 0 || (cols.n == 1 && cols.agg[0] == GROUP_SUM && !typed);
  const bool direct = groupDirect(a, cols.n != 0);
  const size_t bound = a.wide || cols.n ? 2 : a.split ? 4 : 3;  // the kernels' launch bounds
  const uint32_t perCu = (uint32_t)std::max<size_t>(1, std::min<size_t>(bound, (160 * 1024) / lds));
  const dim3 grid(std::min<uint32_t>(capacity, 256 * perCu)), block(GJ_T);
#define HJ_GJ(LAYOUT, DIRECT, SUM)                                                                            \
  hipLaunchKernelGGL((bpGroupKernel<LAYOUT, DIRECT, SUM>), grid, block, lds, s, a, items, nItems, capacity,    \
                     static_cast<const unsigned long long *>(cols.col[0]), cols.offset, cols.stride[0], accCount, \
                     accAgg)
#define HJ_GJ_AGG(LAYOUT, C, TYPED)                                                                                 \
  hipLaunchKernelGGL((bpGroupAggKernel<LAYOUT, C, TYPED>), grid, block, lds, s, a, items, nItems, capacity, cols, \
                     accCount, accAgg, accSlots)
#define HJ_GJ_AGG_C(LAYOUT, C)           \
  if (typed) HJ_GJ_AGG(LAYOUT, C, true); \
  else HJ_GJ_AGG(LAYOUT, C, false)
#define HJ_GJ_LAYOUT(LAYOUT, DIRECT_BUILT)                                   \
  if (single && cols.n) HJ_GJ(LAYOUT, false, true);                          \
  else if (single && direct) HJ_GJ(LAYOUT, DIRECT_BUILT, false);             \
  else if (single) HJ_GJ(LAYOUT, false, false);                              \
  else if (cols.n == 1) { HJ_GJ_AGG_C(LAYOUT, 1); }                          \
  else if (cols.n == 2) { HJ_GJ_AGG_C(LAYOUT, 2); }                          \
  else if (cols.n == 3) { HJ_GJ_AGG_C(LAYOUT, 3); }                          \
  else { HJ_GJ_AGG_C(LAYOUT, 4); }
  switch (markLayout(a)) {
    case MK_COMPRESSED: HJ_GJ_LAYOUT(MK_COMPRESSED, true); break;
    case MK_SPLIT: HJ_GJ_LAYOUT(MK_SPLIT, true); break;
    default: HJ_GJ_LAYOUT(MK_WIDE, false); break;  // (groupDirect is false for wide tuples)
  }
#undef HJ_GJ_LAYOUT
#undef HJ_GJ_AGG_C
#undef HJ_GJ_AGG
#undef HJ_GJ
  HIP_CHECK_LAUNCH();
}

void groupUnitLengths(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
                      uint32_t *unitCounts, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = groupArgs(args, "groupUnitLengths");
  const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(1024, (capacity + GJ_T - 1) / GJ_T));
  hipLaunchKernelGGL(groupUnitLengthsKernel, dim3(blocks), dim3(GJ_T), 0, s, a, units, nUnits, capacity, unitCounts);
  HIP_CHECK_LAUNCH();
}

void groupEmit(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
               const uint32_t *accCount, const unsigned long long *accAgg, uint64_t accSlots, uint32_t columns,
               const unsigned long long *unitOffsets, unsigned long long *out, uint64_t outCapacity, hipStream_t s) {
  if (capacity == 0) return;
  HJ_CHECK(columns <= GROUP_MAX_COLUMNS, "groupEmit: %u value columns (0 to %u)", columns, GROUP_MAX_COLUMNS);
  const BPArgs a = groupArgs(args, "groupEmit");
  HJ_CHECK(a.result && accCount && (columns == 0 || accAgg),
           "groupEmit: needs the empty-group counter and the accumulators");
  HJ_CHECK(!out || unitOffsets, "groupEmit: rows need the unit offsets");
  HJ_CHECK(!out || columns || reinterpret_cast<uintptr_t>(out) % 16 == 0,
           "groupEmit: rows of (rid, count) must be 16-byte aligned");
  const dim3 grid(groupUnitGrid(capacity)), block(GJ_T);
#define HJ_GJ_EMIT(LAYOUT, C)                                                                                         \
  hipLaunchKernelGGL((groupEmitKernel<LAYOUT, C>), grid, block, 0, s, a, units, nUnits, capacity, accCount, accAgg, \
                     accSlots, unitOffsets, out, outCapacity)
#define HJ_GJ_EMIT_C(LAYOUT)                 \
  switch (columns) {                         \
    case 0: HJ_GJ_EMIT(LAYOUT, 0); break;    \
    case 1: HJ_GJ_EMIT(LAYOUT, 1); break;    \
    case 2: HJ_GJ_EMIT(LAYOUT, 2); break;    \
    case 3: HJ_GJ_EMIT(LAYOUT, 3); break;    \
    default: HJ_GJ_EMIT(LAYOUT, 4); break;   \
  }
  switch (markLayout(a)) {
    case MK_COMPRESSED: HJ_GJ_EMIT_C(MK_COMPRESSED); break;
    case MK_SPLIT: HJ_GJ_EMIT_C(MK_SPLIT); break;
    default: HJ_GJ_EMIT_C(MK_WIDE); break;
  }
#undef HJ_GJ_EMIT_C
#undef HJ_GJ_EMIT
  HIP_CHECK_LAUNCH();
}

// Loads this file's code object at engine start (kernels::preloadCodeObjects).
void preloadGroupJoin() {
  hipFuncAttributes a;
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&groupUnitLengthsKernel)));
}

}  // namespace kernels
}  // namespace hpcjoin
