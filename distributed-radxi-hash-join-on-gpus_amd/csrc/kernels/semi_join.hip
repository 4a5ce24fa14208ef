// Semi- and anti-joins (core::JoinKind): which outer tuples have an inner
// partner, each answered once however many inner copies its key has.
//
// The build/probe's work items cannot answer that on their own: a partition
// with more than rChunk inner tuples is expanded into several (R-chunk,
// S-chunk) items (bpPlanCounts), so an outer tuple may match in two inner
// chunks, and is known to be unmatched only after every item of its
// partition has run.  Hence mark, then compact:
//
//  * bpMarkKernel -- persistent grid over the BPItem list, like
//    buildProbeKernel.  The LDS open-addressing table holds keys only and is
//    built set-wise (a CAS that meets its own key stops: repeated inner keys
//    take one slot, chains stay short); the probe stops at the first hit.
//    Per batch row the wave's 64 hit flags become one __ballot mask over 64
//    consecutive positions of the partitioned outer buffer, OR-ed by one lane
//    into the device bit array `marks` (at most two atomicOr per wave and
//    row, none when nothing hit; no per-tuple global atomic).  The OR is
//    needed because the items of one partition cover the same positions and
//    neighbouring items share boundary words.
//  * markCountKernel / markPlaceKernel -- over outer units: one run of
//    a.sChunk positions (the engine passes min(sChunk, MARK_UNIT)) of one
//    final partition's valid range [partS[p], partSEnd[p]) (the
//    sampled local pass leaves gaps between partitions; gap positions are
//    never read).  Units exist for every partition with outer tuples, also
//    those without inner tuples, which get no work item and are exactly what
//    an anti-join emits.  One wave per unit: the count is a popcount of the
//    unit's words (semi) or its complement within the valid range (anti);
//    the place kernel ranks each lane with popcount(mask & lanes below) and
//    stores the selected rids of a word contiguously from the unit's offset
//    (exclusive scan of the unit counts).  A wave walks its unit in position
//    order with its cursor in a register: no atomic, and the rids of a unit
//    come out in position order.
//
// Layouts (template LAYOUT): u64 CompressedTuples (key = high dword >>
// (fragShift - 32)), split columns (key = the u16 fragment; the rid column is
// read only by markPlace), wide 16-byte tuples (64-bit keys).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// kernel uses scratch):
//   bpMarkKernel<compressed>  117 VGPRs, 32 KiB + 64 B LDS at rChunk 4096, 4 workgroups per CU
//   bpMarkKernel<split>        98 VGPRs, same LDS
//   bpMarkKernel<wide>        170 VGPRs, 64 KiB + 64 B LDS at rChunk 4096, 2 workgroups per CU
//   markCountKernel            42 VGPRs, 32 B LDS
//   markPlaceKernel            72 VGPRs (all layouts), no LDS
#include "kernels.h"
#include "device_common.h"
#include "mark_units.h"

#include <algorithm>
#include <type_traits>

namespace hpcjoin {
namespace kernels {

constexpr int MK_T = 256;
constexpr int MK_K = 16;  // tuples per thread per batch (as the counting build/probe)
constexpr uint32_t MK_EMPTY32 = 0xFFFFFFFFu;
constexpr unsigned long long MK_EMPTY64 = ~0ull;

// (MarkLayout, unitRange, unitSelect and markRid: mark_units.h, shared with kind_rows.hip)

template <int LAYOUT>
struct MarkKey {
  using type = typename std::conditional<LAYOUT == MK_WIDE, unsigned long long, uint32_t>::type;
};

template <int LAYOUT, typename K>
__device__ __forceinline__ uint32_t markHash(K key, uint32_t tbits) {
  if constexpr (LAYOUT == MK_WIDE)
    return (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> (64 - tbits));
  else
    return ((uint32_t)key * 2654435761u) >> (32 - tbits);
}

// One batch of an item's keys into registers (only the key: no rid is read).
template <int LAYOUT, bool FULL, typename K>
__device__ __forceinline__ void markLoad(const void *__restrict__ src, const uint16_t *__restrict__ hi, uint64_t off,
                                         uint32_t n, uint32_t b0, uint32_t fragShift, K (&v)[MK_K]) {
#pragma unroll
  for (int k = 0; k < MK_K; ++k) {
    const uint32_t idx = b0 + k * MK_T + threadIdx.x;
    if (FULL || idx < n) {
      if constexpr (LAYOUT == MK_SPLIT)
        v[k] = hi[off + idx];
      else if constexpr (LAYOUT == MK_COMPRESSED)  // fragShift >= keyShift >= 32: the fragment lies in the high dword
        v[k] = reinterpret_cast<const uint32_t *>(src)[2 * (off + idx) + 1] >> (fragShift - 32);
      else
        v[k] = reinterpret_cast<const unsigned long long *>(src)[2 * (off + idx)];
    }
  }
}

// (HIP launch bounds: the second value is workgroups per CU, bound by the LDS
// table as for buildProbeKernel: 4-byte keys 4 per CU, 8-byte keys 2.)
template <int LAYOUT>
__global__ __launch_bounds__(MK_T, LAYOUT == MK_WIDE ? 2 : 4) void bpMarkKernel(BPArgs a,
                                                                               const BPItem *__restrict__ items,
                                                                               const uint32_t *__restrict__ nItemsPtr,
                                                                               uint32_t capacity,
                                                                               unsigned long long *marks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using K = typename MarkKey<LAYOUT>::type;
  constexpr K EMPTY = LAYOUT == MK_WIDE ? (K)MK_EMPTY64 : (K)MK_EMPTY32;
  constexpr uint32_t BATCH = MK_T * MK_K;
  K *table = reinterpret_cast<K *>(smem);
  const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
  const uint32_t nItems = min(*nItemsPtr, capacity);
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
    K rv[MK_K], sv[MK_K];
    if (nr >= BATCH) markLoad<LAYOUT, true>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv);
    else markLoad<LAYOUT, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv);
    if (ns >= BATCH) markLoad<LAYOUT, true>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv);
    else markLoad<LAYOUT, false>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv);
    for (uint32_t i = t; i < slots; i += MK_T) table[i] = EMPTY;
    __syncthreads();

    // ---- build: a set of keys
    for (uint32_t b0 = 0; b0 < nr; b0 += BATCH) {
      if (b0) markLoad<LAYOUT, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv);
#pragma unroll
      for (int k = 0; k < MK_K; ++k) {
        if (b0 + k * MK_T + t < nr) {
          const K key = rv[k];
          uint32_t h = markHash<LAYOUT>(key, tbits);
          for (;;) {
            const K old = atomicCAS(&table[h], EMPTY, key);
            if (old == EMPTY || old == key) break;
            h = (h + 1) & mask;
          }
        }
      }
    }
    __syncthreads();

    // ---- probe: first hit, one mask per wave and batch row
    for (uint32_t b0 = 0; b0 < ns; b0 += BATCH) {
      if (b0) {
        if (b0 + BATCH <= ns) markLoad<LAYOUT, true>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv);
        else markLoad<LAYOUT, false>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv);
      }
#pragma unroll
      for (int k = 0; k < MK_K; ++k) {
        const uint32_t row0 = b0 + k * MK_T + (t - lane);  // the wave's first tuple of this row (wave-uniform)
        if (row0 >= ns) break;
        bool hit = false;
        if (row0 + lane < ns) {
          const K key = sv[k];
          uint32_t h = markHash<LAYOUT>(key, tbits);
          K e;
          while ((e = table[h]) != EMPTY) {
            if (e == key) {
              hit = true;
              break;
            }
            h = (h + 1) & mask;
          }
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0 && m) {
          // Bits of positions p0 .. p0 + 63; only lanes below ns set one, so
          // the spill-over word is touched only when it holds a valid position.
          const uint64_t p0 = sb + row0;
          const uint32_t sh = (uint32_t)(p0 & 63);
          const unsigned long long lo = m << sh;
          if (lo) atomicOr(&marks[p0 >> 6], lo);
          if (sh) {
            const unsigned long long hi = m >> (64 - sh);
            if (hi) atomicOr(&marks[(p0 >> 6) + 1], hi);
          }
        }
      }
    }
    __syncthreads();  // the next item clears the table
  }
}

// ------------------------------------------------------------------- units
__global__ __launch_bounds__(MK_T) void markPlanUnitsKernel(const uint64_t *__restrict__ partS,
                                                           const uint64_t *__restrict__ partSEnd, uint32_t P,
                                                           uint32_t sc, uint32_t *counts) {
  const uint32_t p = blockIdx.x * MK_T + threadIdx.x;
  if (p >= P) return;
  counts[p] = (uint32_t)ceilDiv(partSEnd[p] - partS[p], (uint64_t)sc);
}

__global__ __launch_bounds__(MK_T) void markEmitUnitsKernel(uint32_t P, const uint32_t *__restrict__ counts,
                                                           const uint32_t *__restrict__ offsets, MarkUnit *units,
                                                           uint32_t capacity) {
  const uint32_t p = blockIdx.x * MK_T + threadIdx.x;
  if (p >= P) return;
  const uint32_t c = counts[p], o = offsets[p];
  for (uint32_t i = 0; i < c && o + i < capacity; ++i) {
    MarkUnit u;
    u.part = p;
    u.chunk = i;
    units[o + i] = u;
  }
}

__global__ __launch_bounds__(MK_T) void markCountKernel(BPArgs a, const MarkUnit *__restrict__ units,
                                                       const uint32_t *__restrict__ nUnitsPtr, uint32_t capacity,
                                                       const unsigned long long *__restrict__ marks, bool anti,
                                                       uint32_t *__restrict__ unitCounts) {
  __shared__ unsigned long long wsum[MK_T / WAVE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t nUnits = min(*nUnitsPtr, capacity);
  const uint32_t wavesPerGrid = gridDim.x * (MK_T / WAVE);
  unsigned long long mine = 0;
  for (uint32_t u = blockIdx.x * (MK_T / WAVE) + threadIdx.x / WAVE; u < nUnits; u += wavesPerGrid) {
    uint64_t ub, ue;
    unitRange(a, units[u], ub, ue);
    const uint64_t w0 = ub >> 6, wl = (ue - 1) >> 6;
    uint32_t c = 0;
    for (uint64_t w = w0 + lane; w <= wl; w += WAVE) c += __popcll(unitSelect(marks, w, ub, ue, anti));
    c = waveReduceSum<uint32_t>(c);
    if (lane == 0) {
      unitCounts[u] = c;
      mine += c;
    }
  }
  const unsigned long long total = blockReduceSum<MK_T, unsigned long long>(mine, wsum);
  if (threadIdx.x == 0 && total) atomicAdd(a.result, total);
}

// One wave per unit.  Per round a lane reads one of the unit's next 64 mark
// words; a wave scan of their popcounts gives every word its offset in the
// unit's output run, and the words are then placed four at a time (the four
// rid loads issued before the first store).
template <int LAYOUT>
__global__ __launch_bounds__(MK_T) void markPlaceKernel(BPArgs a, const MarkUnit *__restrict__ units,
                                                       const uint32_t *__restrict__ nUnitsPtr, uint32_t capacity,
                                                       const unsigned long long *__restrict__ marks, bool anti,
                                                       const unsigned long long *__restrict__ unitOffsets,
                                                       unsigned long long *__restrict__ out, uint64_t outCapacity) {
  constexpr int U = 4;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const unsigned long long below = (1ull << lane) - 1;
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  const uint32_t nUnits = min(*nUnitsPtr, capacity);
  const uint32_t wavesPerGrid = gridDim.x * (MK_T / WAVE);
  for (uint32_t u = blockIdx.x * (MK_T / WAVE) + threadIdx.x / WAVE; u < nUnits; u += wavesPerGrid) {
    uint64_t ub, ue;
    unitRange(a, units[u], ub, ue);
    const uint64_t w0 = ub >> 6, wl = (ue - 1) >> 6;
    unsigned long long base = unitOffsets[u];
    for (uint64_t wb = w0; wb <= wl; wb += WAVE) {
      const unsigned long long sel = wb + lane <= wl ? unitSelect(marks, wb + lane, ub, ue, anti) : 0ull;
      const uint32_t c = (uint32_t)__popcll(sel);
      const uint32_t incl = waveInclusiveScan<uint32_t>(c);
      const uint32_t excl = incl - c;
      const uint32_t nw = (uint32_t)min((uint64_t)WAVE, wl - wb + 1);  // wave-uniform
      for (uint32_t i = 0; i < nw; i += U) {
        unsigned long long s[U], rid[U];
        uint32_t o[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
          const uint32_t src = min(i + j, nw - 1);
          const uint32_t lo = __shfl((uint32_t)sel, src, WAVE), hi = __shfl((uint32_t)(sel >> 32), src, WAVE);
          s[j] = i + j < nw ? ((unsigned long long)hi << 32) | lo : 0ull;
          o[j] = __shfl(excl, src, WAVE);
          rid[j] = 0;
          if ((s[j] >> lane) & 1) rid[j] = markRid<LAYOUT>(a, ((wb + i + j) << 6) + lane, ridMask);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
          if ((s[j] >> lane) & 1) {
            const unsigned long long at = base + o[j] + (uint32_t)__popcll(s[j] & below);
            if (at < outCapacity) out[at] = rid[j];
          }
        }
      }
      base += __shfl(incl, WAVE - 1, WAVE);
    }
  }
}

// Small units (one final partition's outer side is a few thousand positions)
// are latency-bound per wave: the grid fills every CU with waves.
static uint32_t unitGrid(uint32_t capacity) {
  const uint32_t perBlock = MK_T / WAVE;
  return std::max<uint32_t>(1, std::min<uint32_t>(256 * 8, (capacity + perBlock - 1) / perBlock));
}

static BPArgs markArgs(const BPArgs &args) {
  BPArgs a = args;
  if (!a.partREnd) a.partREnd = a.partR + 1;
  if (!a.partSEnd) a.partSEnd = a.partS + 1;
  return a;
}

size_t bpMarkLdsBytes(const BPArgs &a) {
  const uint64_t slots = uint64_t(1) << ceilLog2(2ull * a.rChunk);
  return slots * (a.wide ? 8 : 4) + 64;
}

uint64_t markWords(uint64_t positions) { return positions / 64 + 2; }

void bpMark(const BPArgs &args, const BPItem *items, const uint32_t *nItems, uint32_t capacity,
            unsigned long long *marks, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = markArgs(args);
  const size_t lds = bpMarkLdsBytes(a);
  HJ_CHECK(lds <= 160 * 1024, "bpMark: LDS request %zu exceeds 160 KiB (rChunk=%u)", lds, a.rChunk);
  HJ_CHECK(!a.keyOnly, "bpMark: key-only words carry no rid (semi- and anti-joins use rid-carrying layouts)");
  HJ_CHECK(!(a.split && a.wide), "bpMark: the split layout holds compressed tuples");
  HJ_CHECK(!a.split || (a.Rhi && a.Shi), "bpMark: split layout without fragment columns");
  HJ_CHECK(a.wide || a.fragShift >= 32, "bpMark: fragShift=%u < 32 (the rid field of a CompressedTuple is >= 32 bits)",
           a.fragShift);
  const uint32_t perCu = (uint32_t)std::max<size_t>(1, std::min<size_t>(a.wide ? 2 : 4, (160 * 1024) / lds));
  const uint32_t blocks = std::min<uint32_t>(capacity, 256 * perCu);
  switch (markLayout(a)) {
    case MK_COMPRESSED:
      hipLaunchKernelGGL(bpMarkKernel<MK_COMPRESSED>, dim3(blocks), dim3(MK_T), lds, s, a, items, nItems, capacity, marks);
      break;
    case MK_SPLIT:
      hipLaunchKernelGGL(bpMarkKernel<MK_SPLIT>, dim3(blocks), dim3(MK_T), lds, s, a, items, nItems, capacity, marks);
      break;
    default:
      hipLaunchKernelGGL(bpMarkKernel<MK_WIDE>, dim3(blocks), dim3(MK_T), lds, s, a, items, nItems, capacity, marks);
      break;
  }
  HIP_CHECK_LAUNCH();
}

void markPlanUnits(const BPArgs &args, uint32_t *counts, hipStream_t s) {
  if (args.P == 0) return;
  const BPArgs a = markArgs(args);
  hipLaunchKernelGGL(markPlanUnitsKernel, dim3(ceilDiv(a.P, MK_T)), dim3(MK_T), 0, s, a.partS, a.partSEnd, a.P,
                     a.sChunk, counts);
  HIP_CHECK_LAUNCH();
}

void markEmitUnits(const BPArgs &a, const uint32_t *counts, const uint32_t *offsets, MarkUnit *units,
                   uint32_t capacity, hipStream_t s) {
  if (a.P == 0) return;
  hipLaunchKernelGGL(markEmitUnitsKernel, dim3(ceilDiv(a.P, MK_T)), dim3(MK_T), 0, s, a.P, counts, offsets, units,
                     capacity);
  HIP_CHECK_LAUNCH();
}

void markCount(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
               const unsigned long long *marks, bool anti, uint32_t *unitCounts, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = markArgs(args);
  hipLaunchKernelGGL(markCountKernel, dim3(unitGrid(capacity)), dim3(MK_T), 0, s, a, units, nUnits, capacity, marks,
                     anti, unitCounts);
  HIP_CHECK_LAUNCH();
}

void markPlace(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
               const unsigned long long *marks, bool anti, const unsigned long long *unitOffsets,
               unsigned long long *out, uint64_t outCapacity, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = markArgs(args);
  const dim3 grid(unitGrid(capacity)), block(MK_T);
  switch (markLayout(a)) {
    case MK_COMPRESSED:
      hipLaunchKernelGGL(markPlaceKernel<MK_COMPRESSED>, grid, block, 0, s, a, units, nUnits, capacity, marks, anti,
                         unitOffsets, out, outCapacity);
      break;
    case MK_SPLIT:
      hipLaunchKernelGGL(markPlaceKernel<MK_SPLIT>, grid, block, 0, s, a, units, nUnits, capacity, marks, anti,
                         unitOffsets, out, outCapacity);
      break;
    default:
      hipLaunchKernelGGL(markPlaceKernel<MK_WIDE>, grid, block, 0, s, a, units, nUnits, capacity, marks, anti,
                         unitOffsets, out, outCapacity);
      break;
  }
  HIP_CHECK_LAUNCH();
}

// Loads this file's code object at engine start (kernels::preloadCodeObjects).
void preloadSemiJoin() {
  hipFuncAttributes a;
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&markPlanUnitsKernel)));
}

}  // namespace kernels
}  // namespace hpcjoin
