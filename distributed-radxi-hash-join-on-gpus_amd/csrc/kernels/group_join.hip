// Group joins (core::JoinKind::Group): per inner tuple r the number of outer
// tuples with r's key, and optionally the int64 sum (two's complement, wraps)
// of one outer value column over those tuples -- the join followed by COUNT /
// SUM ... GROUP BY the build side, without ever forming a pair.
//
//  * bpGroupKernel<LAYOUT, DIRECT, SUM> -- persistent grid over the BPItem
//    list, geometry of bpOuterCountKernel (256 threads, 16 tuples per thread
//    and batch, the first inner and outer batch in flight while the table is
//    cleared).  Hashed table: the key slots of the outer-join count, every
//    inner copy in a slot of its own, next to one u32 counter per slot and
//    with SUM one u64 accumulator per slot; only the *first* slot of a key
//    aggregates.  An outer tuple stops at the first slot holding its key and
//    does one LDS atomic add (with SUM a second, 64-bit one): it never walks
//    the chain of copies.  The value is values[(rid - ridOffset) * stride],
//    loaded non-temporally; the rids come in with the keys (one 8-byte load
//    per compressed tuple instead of its high dword; wide tuples read the rid
//    word of a tuple that found a slot), and the gathers of a
//    thread's 16 tuples (wide tuples: 8) are all issued before the first one is consumed.  A
//    tuple that found no slot forms no address.  After a barrier every inner
//    tuple (still in registers when the item has one batch) looks up the first
//    slot of its own key and adds that slot's count and sum to the global
//    accumulators at its position rb + idx of the partitioned inner buffer:
//    consecutive lanes hold consecutive positions.  An inner chunk is shared
//    by all outer chunks of its partition, so the add is a global atomic,
//    skipped when the item counted nothing for the tuple.  (A plain store for
//    partitions of a single outer chunk was not built: it needs a second code
//    path per item and nothing has measured the atomics as the bottleneck.)
//    The item's pair total is the sum of the counts its inner tuples read;
//    *a.result gets one 64-bit atomic per workgroup.
//  * DIRECT (4-byte fragments of at most 13 bits, count only): table[fragment]
//    is the number of outer tuples of the fragment.  No build: the probe adds
//    one per outer tuple, the inner tuples read their fragment's counter.
//    DIRECT is not built for SUM: the accumulators would be 12 B per fragment
//    (96 KiB + 64 B at 13 bits, one workgroup per CU) and an outer tuple
//    without a partner would still gather its value; SUM always takes the
//    hashed table, whose size follows rChunk.  bpGroup() chooses accordingly.
//  * groupUnitLengths / groupEmitKernel<LAYOUT, SUM> -- one wave per unit of
//    the inner side (markPlanUnits / markEmitUnits over outerSwapSides(a,
//    unit), also for partitions without outer tuples, which got no work item).
//    Every valid position is selected, so a unit's row count is its length and
//    the row offsets come from the u32-to-u64 scan.  Per position the row
//    (rid, count[, sum]) is written; the wave's stores are consecutive 8-byte
//    words of the unit's run (the three columns are interleaved through lane
//    shuffles).  Zero counts are added to *a.result; without `out` the kernel
//    only counts them.  Positions outside [partS, partSEnd) -- the gaps of a
//    sampled local pass -- are never read.
//
// Count accumulators are u32: the caller refuses a global outer size of 2^32
// or more (HashJoin, ops.build_probe_group).
//
// Layouts (template LAYOUT): u64 CompressedTuples, split columns, wide 16-byte
// tuples.  Key-only words are refused (no rid to report).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// kernel uses scratch):
//   bpGroupKernel<compressed>        121 VGPRs hashed, 120 direct; 3 workgroups per CU
//   bpGroupKernel<split>             108 VGPRs hashed and direct; 4 workgroups per CU
//   bpGroupKernel<wide>              176 VGPRs; 2 workgroups per CU
//   bpGroupKernel<compressed, SUM>   234 VGPRs; 2 workgroups per CU
//   bpGroupKernel<split, SUM>        186 VGPRs; 2 workgroups per CU
//   bpGroupKernel<wide, SUM>         192 VGPRs; 2 workgroups per CU
//   groupEmitKernel                  28-30 VGPRs (rid, count), 52-54 (rid, count, sum); 32 B LDS
//   groupUnitLengthsKernel           12 VGPRs, no LDS
//   LDS of bpGroupKernel (dynamic, bpGroupLdsBytes): hashed 4-byte keys + counters 32 KiB + 64 B at the
//   planned rChunk 2048 (4096 slots), with sums 64 KiB + 64 B; 8-byte keys at the planned rChunk 1024 (2048
//   slots) 24 KiB + 64 B, with sums 40 KiB + 64 B; direct 4 B << fragBits + 64 B (32 KiB + 64 B at 13 bits).
//   A request above 160 KiB (a configured rChunk of 8192 with sums) is refused by bpGroup.
#include "kernels.h"
#include "device_common.h"
#include "mark_units.h"

#include <algorithm>
#include <type_traits>

namespace hpcjoin {
namespace kernels {

constexpr int GJ_T = 256;
constexpr int GJ_K = 16;  // tuples per thread per batch (as the counting build/probe)
constexpr uint32_t GJ_EMPTY32 = 0xFFFFFFFFu;
constexpr unsigned long long GJ_EMPTY64 = ~0ull;
constexpr uint32_t GJ_NONE = 0xFFFFFFFFu;  // probe: no slot holds the key
constexpr uint32_t GJ_DIRECT_MAX_BITS = 13;

template <int LAYOUT>
struct GroupKey {
  using type = typename std::conditional<LAYOUT == MK_WIDE, unsigned long long, uint32_t>::type;
};
// Rid registers of the outer side (SUM): the whole CompressedTuple, the u32 rid column, the Tuple's rid.
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

static bool groupDirect(const BPArgs &a, bool sum) {
  return !sum && !a.wide && a.fragBits > 0 && a.fragBits <= GJ_DIRECT_MAX_BITS;
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
  constexpr K EMPTY = LAYOUT == MK_WIDE ? (K)GJ_EMPTY64 : (K)GJ_EMPTY32;
  constexpr uint32_t BATCH = GJ_T * GJ_K;
  // The outer rids come in with the keys; wide tuples read theirs when a slot was found (see the probe).
  constexpr bool PRE_RID = SUM && LAYOUT != MK_WIDE;
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
    if (nr >= BATCH) groupLoad<LAYOUT, true, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv, nor);
    else groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv, nor);
    if constexpr (PRE_RID) {
      if (ns >= BATCH) groupLoad<LAYOUT, true, true>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
      else groupLoad<LAYOUT, false, true>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
    } else {
      if (ns >= BATCH) groupLoad<LAYOUT, true, false>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
      else groupLoad<LAYOUT, false, false>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv, rr);
    }
    for (uint32_t i = t; i < slots; i += GJ_T) {
      cnt[i] = 0;
      if constexpr (!DIRECT) table[i] = EMPTY;
      if constexpr (SUM) sums[i] = 0;
    }
    __syncthreads();

    // ---- build: every inner copy takes a slot (DIRECT: nothing to build)
    if constexpr (!DIRECT) {
      for (uint32_t b0 = 0; b0 < nr; b0 += BATCH) {
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
    for (uint32_t b0 = 0; b0 < ns; b0 += BATCH) {
      if (b0) {
        if constexpr (PRE_RID) {
          if (b0 + BATCH <= ns) groupLoad<LAYOUT, true, true>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
          else groupLoad<LAYOUT, false, true>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
        } else {
          if (b0 + BATCH <= ns) groupLoad<LAYOUT, true, false>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
          else groupLoad<LAYOUT, false, false>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv, rr);
        }
      }
      if constexpr (DIRECT) {
#pragma unroll
        for (int k = 0; k < GJ_K; ++k)
          if (b0 + k * GJ_T + t < ns) atomicAdd(&cnt[sv[k] & mask], 1u);  // (fragments are < 2^fragBits)
      } else {
        // G tuples at a time: their slots, then (SUM) all G gathers issued before the first value is consumed.
        // (Wide tuples with a value column take 8, and read the rid -- the second word of the 16-byte tuple whose
        // key they hold -- only for tuples with a slot: with 16 preloaded 8-byte rids next to 16 8-byte keys of
        // either side the kernel spilled 52 bytes per lane to scratch.)
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
                else rid = LAYOUT == MK_COMPRESSED ? ((uint64_t)rr[g0 + j] & ridMask) : (uint64_t)rr[g0 + j];
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
    for (uint32_t b0 = 0; b0 < nr; b0 += BATCH) {
      if (nr > BATCH) groupLoad<LAYOUT, false, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv, nor);  // else in registers
#pragma unroll
      for (int k = 0; k < GJ_K; ++k) {
        const uint32_t idx = b0 + k * GJ_T + t;
        if (idx < nr) {
          const K key = rv[k];
          uint32_t h;
          if constexpr (DIRECT) {
            h = (uint32_t)key & mask;
          } else {
            h = groupHash<LAYOUT>(key, tbits);
            while (table[h] != key) h = (h + 1) & mask;  // the key is in the table: this tuple inserted it
          }
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

// One wave per unit of a.S (the inner relation: sides swapped by the caller).
template <int LAYOUT, bool SUM>
__global__ __launch_bounds__(GJ_T) void groupEmitKernel(BPArgs a, const MarkUnit *__restrict__ units,
                                                       const uint32_t *__restrict__ nUnitsPtr, uint32_t capacity,
                                                       const uint32_t *__restrict__ accCount,
                                                       const unsigned long long *__restrict__ accSum,
                                                       const unsigned long long *__restrict__ unitOffsets,
                                                       unsigned long long *__restrict__ out, uint64_t outCapacity) {
  constexpr uint32_t W = SUM ? 3 : 2;
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
      if constexpr (!SUM) {
        if (valid && row0 + lane < outCapacity)
          reinterpret_cast<ulonglong2 *>(out)[row0 + lane] = make_ulonglong2(rid, (unsigned long long)c);
      } else {
        const unsigned long long s = valid ? accSum[p0 + lane] : 0ull;
        // word q of the run (row q / 3, column q % 3) is stored by lane q % 64: consecutive 8-byte stores
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) {
          const uint32_t q = WAVE * k + lane, src = q / W, col = q - src * W;
          const unsigned long long vr = __shfl(rid, src, WAVE), vs = __shfl(s, src, WAVE);
          const uint32_t vc = __shfl(c, src, WAVE);
          const unsigned long long v = col == 0 ? vr : col == 1 ? (unsigned long long)vc : vs;
          if (src < m && row0 + src < outCapacity) out[row0 * W + q] = v;
        }
      }
    }
  }
  const unsigned long long total = blockReduceSum<GJ_T, unsigned long long>(zeros, wsum);
  if (threadIdx.x == 0 && total) atomicAdd(a.result, total);
}

// Small units are latency-bound per wave: the grid fills every CU with waves (as semi_join.hip).
static uint32_t groupUnitGrid(uint32_t capacity) {
  const uint32_t perBlock = GJ_T / WAVE;
  return std::max<uint32_t>(1, std::min<uint32_t>(256 * 8, (capacity + perBlock - 1) / perBlock));
}

static BPArgs groupArgs(const BPArgs &args) {
  BPArgs a = args;
  if (!a.partREnd) a.partREnd = a.partR + 1;
  if (!a.partSEnd) a.partSEnd = a.partS + 1;
  return a;
}

size_t bpGroupLdsBytes(const BPArgs &a, bool sum) {
  if (groupDirect(a, sum)) return (size_t(4) << a.fragBits) + 64;
  return groupTableBytes(a.rChunk, a.wide, sum);
}

void bpGroup(const BPArgs &args, const BPItem *items, const uint32_t *nItems, uint32_t capacity,
             const unsigned long long *values, uint64_t ridOffset, uint64_t strideWords, uint32_t *accCount,
             unsigned long long *accSum, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = groupArgs(args);
  const bool sum = values != nullptr;
  const size_t lds = bpGroupLdsBytes(a, sum);
  HJ_CHECK(lds <= 160 * 1024, "bpGroup: LDS request %zu exceeds 160 KiB (rChunk=%u%s)", lds, a.rChunk,
           sum ? ", with a value column" : "");
  HJ_CHECK(!a.keyOnly, "bpGroup: key-only words carry no rid (group joins use rid-carrying layouts)");
  HJ_CHECK(!(a.split && a.wide), "bpGroup: the split layout holds compressed tuples");
  HJ_CHECK(!a.split || (a.Rhi && a.Shi), "bpGroup: split layout without fragment columns");
  HJ_CHECK(a.wide || a.fragShift >= 32, "bpGroup: fragShift=%u < 32 (the rid field of a CompressedTuple is >= 32 bits)",
           a.fragShift);
  HJ_CHECK(a.result && accCount, "bpGroup: needs the pair counter and the count accumulators");
  HJ_CHECK(!sum || (accSum && strideWords >= 1), "bpGroup: a value column needs the sum accumulators and a stride >= 1");
  const size_t bound = a.wide || sum ? 2 : a.split ? 4 : 3;
  const uint32_t perCu = (uint32_t)std::max<size_t>(1, std::min<size_t>(bound, (160 * 1024) / lds));
  const uint32_t blocks = std::min<uint32_t>(capacity, 256 * perCu);
#define HJ_GJ(LAYOUT, DIRECT, SUM)                                                                                 \
  hipLaunchKernelGGL((bpGroupKernel<LAYOUT, DIRECT, SUM>), dim3(blocks), dim3(GJ_T), lds, s, a, items, nItems, capacity, \
                     values, ridOffset, strideWords, accCount, accSum)
  const bool direct = groupDirect(a, sum);
  switch (markLayout(a)) {
    case MK_COMPRESSED:
      if (sum) HJ_GJ(MK_COMPRESSED, false, true);
      else if (direct) HJ_GJ(MK_COMPRESSED, true, false);
      else HJ_GJ(MK_COMPRESSED, false, false);
      break;
    case MK_SPLIT:
      if (sum) HJ_GJ(MK_SPLIT, false, true);
      else if (direct) HJ_GJ(MK_SPLIT, true, false);
      else HJ_GJ(MK_SPLIT, false, false);
      break;
    default:
      if (sum) HJ_GJ(MK_WIDE, false, true);
      else HJ_GJ(MK_WIDE, false, false);
      break;
  }
#undef HJ_GJ
  HIP_CHECK_LAUNCH();
}

void groupUnitLengths(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
                      uint32_t *unitCounts, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = groupArgs(args);
  const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(1024, (capacity + GJ_T - 1) / GJ_T));
  hipLaunchKernelGGL(groupUnitLengthsKernel, dim3(blocks), dim3(GJ_T), 0, s, a, units, nUnits, capacity, unitCounts);
  HIP_CHECK_LAUNCH();
}

void groupEmit(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
               const uint32_t *accCount, const unsigned long long *accSum, const unsigned long long *unitOffsets,
               unsigned long long *out, uint64_t outCapacity, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = groupArgs(args);
  HJ_CHECK(!a.keyOnly, "groupEmit: key-only words carry no rid");
  HJ_CHECK(!(a.split && a.wide), "groupEmit: the split layout holds compressed tuples");
  HJ_CHECK(a.result && accCount, "groupEmit: needs the empty-group counter and the count accumulators");
  HJ_CHECK(!out || unitOffsets, "groupEmit: rows need the unit offsets");
  HJ_CHECK(!out || reinterpret_cast<uintptr_t>(out) % 16 == 0, "groupEmit: the rows must be 16-byte aligned");
  const dim3 grid(groupUnitGrid(capacity)), block(GJ_T);
#define HJ_GJ_EMIT(LAYOUT, SUM)                                                                                    \
  hipLaunchKernelGGL((groupEmitKernel<LAYOUT, SUM>), grid, block, 0, s, a, units, nUnits, capacity, accCount, accSum, \
                     unitOffsets, out, outCapacity)
  const bool sum = accSum != nullptr;
  switch (markLayout(a)) {
    case MK_COMPRESSED:
      if (sum) HJ_GJ_EMIT(MK_COMPRESSED, true); else HJ_GJ_EMIT(MK_COMPRESSED, false);
      break;
    case MK_SPLIT:
      if (sum) HJ_GJ_EMIT(MK_SPLIT, true); else HJ_GJ_EMIT(MK_SPLIT, false);
      break;
    default:
      if (sum) HJ_GJ_EMIT(MK_WIDE, true); else HJ_GJ_EMIT(MK_WIDE, false);
      break;
  }
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
