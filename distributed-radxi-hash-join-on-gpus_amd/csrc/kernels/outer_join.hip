// Left, right and full outer joins (core::JoinKind): the inner join's
// (rid_inner, rid_outer) pairs plus one NULL-padded row per tuple of a
// preserved side that found no partner.
//
// A tuple is known to be unmatched only after every work item of its
// partition has run: a partition with more than rChunk inner tuples or more
// than sChunk outer tuples is expanded into several (R-chunk, S-chunk) items
// (bpPlanCounts), so an outer tuple may hit in several inner chunks and an
// inner tuple may be hit from several outer chunks.  Hence one fused pass and
// the compaction of semi_join.hip per preserved side:
//
//  * bpOuterCountKernel -- persistent grid over the BPItem list.  It replaces
//    the count pre-pass of the two-pass pair materialization and reads the
//    item's inner and outer keys once.  Fragments of at most 13 bits use a
//    direct-addressed table (copies and hit flag per fragment, see DIRECT
//    below); otherwise the LDS open-addressing table holds keys only, every inner copy in a slot of its own (the pairs are counted
//    with multiplicity: the probe walks its whole chain), next to one hit bit
//    per slot.  Per item it produces
//      - itemCounts[w]: the pairs the place pass (buildProbe with item
//        offsets, unchanged) will write for this item;
//      - S preserved: per batch row the wave's 64 hit flags as one __ballot
//        mask, OR-ed into marksS exactly as bpMark does;
//      - R preserved: the probe sets the hit bit of the *first* slot holding
//        its key; after a barrier every inner tuple (still in registers when
//        the item has one batch) looks up the first slot of its own key, and
//        the wave's ballot of those bits is OR-ed into marksR, a bit array
//        over the positions of the partitioned inner buffer.
//    No per-tuple global atomic: at most two 64-bit atomicOr per wave and row.
//    The OR is required on both sides: the items of one partition share inner
//    chunks across outer chunks and vice versa, and neighbouring items share
//    boundary words.
//  * The unmatched tuples of a preserved side come from the unit machinery of
//    semi_join.hip (markPlanUnits / markEmitUnits / markCount with anti =
//    true); for the inner side the caller passes BPArgs with the sides swapped.
//  * markPlacePairsKernel -- the pair-writing twin of markPlaceKernel: one wave
//    per unit, cursor in a register, one 16-byte store {rid, NULL_RID} or
//    {NULL_RID, rid} per unmarked tuple, from unitOffsets[u] + the row count
//    written before this side (device words, no host round trip).
//
// Layouts (template LAYOUT): u64 CompressedTuples, split columns, wide 16-byte
// tuples, as semi_join.hip.  Key-only words are refused (no rid to emit).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// kernel uses scratch):
//   bpOuterCountKernel<compressed>  140 VGPRs (hashed and direct), 3 workgroups per CU
//   bpOuterCountKernel<split>       126 VGPRs (hashed and direct), 4 workgroups per CU
//   bpOuterCountKernel<wide>        190 VGPRs, 2 workgroups per CU
//   markPlacePairsKernel             76 VGPRs (all layouts), no LDS
//   LDS of bpOuterCountKernel (dynamic): hashed 4-byte keys 16.5 KiB + 64 B at
//   rChunk 2048 (33 KiB + 64 B at 4096), 8-byte keys 32.5 KiB + 64 B at 2048;
//   direct 4 B << fragBits + 64 B (4 KiB + 64 B at 10 fragment bits).
#include "kernels.h"
#include "device_common.h"

#include <algorithm>
#include <type_traits>

namespace hpcjoin {
namespace kernels {

constexpr int OJ_T = 256;
constexpr int OJ_K = 16;  // tuples per thread per batch (as the counting build/probe)
constexpr uint32_t OJ_EMPTY32 = 0xFFFFFFFFu;
constexpr unsigned long long OJ_EMPTY64 = ~0ull;

enum OuterLayout : int { OJ_COMPRESSED = 0, OJ_SPLIT = 1, OJ_WIDE = 2 };

static int outerLayout(const BPArgs &a) { return a.wide ? OJ_WIDE : a.split ? OJ_SPLIT : OJ_COMPRESSED; }

template <int LAYOUT>
struct OuterKey {
  using type = typename std::conditional<LAYOUT == OJ_WIDE, unsigned long long, uint32_t>::type;
};

template <int LAYOUT, typename K>
__device__ __forceinline__ uint32_t outerHash(K key, uint32_t tbits) {
  if constexpr (LAYOUT == OJ_WIDE)
    return (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> (64 - tbits));
  else
    return ((uint32_t)key * 2654435761u) >> (32 - tbits);
}

// One batch of an item's keys into registers (only the key: no rid is read).
template <int LAYOUT, bool FULL, typename K>
__device__ __forceinline__ void outerLoad(const void *__restrict__ src, const uint16_t *__restrict__ hi, uint64_t off,
                                          uint32_t n, uint32_t b0, uint32_t fragShift, K (&v)[OJ_K]) {
#pragma unroll
  for (int k = 0; k < OJ_K; ++k) {
    const uint32_t idx = b0 + k * OJ_T + threadIdx.x;
    if (FULL || idx < n) {
      if constexpr (LAYOUT == OJ_SPLIT)
        v[k] = hi[off + idx];
      else if constexpr (LAYOUT == OJ_COMPRESSED)  // fragShift >= keyShift >= 32: the fragment lies in the high dword
        v[k] = reinterpret_cast<const uint32_t *>(src)[2 * (off + idx) + 1] >> (fragShift - 32);
      else
        v[k] = reinterpret_cast<const unsigned long long *>(src)[2 * (off + idx)];
    }
  }
}

// Slots of the largest table of a launch (an item's table has at least 64).
HJ_HD uint64_t outerMaxSlots(uint32_t rChunk) {
  const uint32_t b = ceilLog2(2ull * rChunk);
  return uint64_t(1) << (b < 6 ? 6 : b);
}

// The wave's hit mask of 64 consecutive positions from p0 into a bit array
// (only lanes of valid positions set a bit, so the spill-over word is touched
// only when it holds a valid position).
__device__ __forceinline__ void outerOrMask(unsigned long long *marks, uint64_t p0, unsigned long long m) {
  const uint32_t sh = (uint32_t)(p0 & 63);
  const unsigned long long lo = m << sh;
  if (lo) atomicOr(&marks[p0 >> 6], lo);
  if (sh) {
    const unsigned long long hi = m >> (64 - sh);
    if (hi) atomicOr(&marks[(p0 >> 6) + 1], hi);
  }
}

// (HIP launch bounds: the second value is workgroups per CU.  8-byte keys get
// the 2-per-CU budget of the wide mark kernel; the u16 fragment column 4;
// CompressedTuples 3, as the per-item count variant of buildProbeKernel: at 4
// per CU (128 VGPRs) that instantiation spilled 44 bytes per lane to scratch.)
//
// DIRECT (4-byte keys whose fragments span at most 2^fragBits <= 2^13 values,
// as the direct-addressed count of build_probe.hip): table[fragment] holds the
// inner copies of the fragment in its low 31 bits and the hit flag in bit 31
// -- no hashing, no chains, no separate hit bits.
constexpr uint32_t OJ_DIRECT_MAX_BITS = 13;
constexpr uint32_t OJ_HIT = 0x80000000u;
static bool outerDirect(const BPArgs &a) { return !a.wide && a.fragBits > 0 && a.fragBits <= OJ_DIRECT_MAX_BITS; }

template <int LAYOUT, bool DIRECT>
__global__ __launch_bounds__(OJ_T, LAYOUT == OJ_WIDE ? 2 : LAYOUT == OJ_SPLIT ? 4 : 3) void bpOuterCountKernel(
    BPArgs a, const BPItem *__restrict__ items, const uint32_t *__restrict__ nItemsPtr, uint32_t capacity,
    unsigned long long *marksR, unsigned long long *marksS) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using K = typename OuterKey<LAYOUT>::type;
  constexpr K EMPTY = LAYOUT == OJ_WIDE ? (K)OJ_EMPTY64 : (K)OJ_EMPTY32;
  constexpr uint32_t BATCH = OJ_T * OJ_K;
  static_assert(!DIRECT || LAYOUT != OJ_WIDE, "direct-addressed tables hold 4-byte fragments");
  const uint64_t maxSlots = DIRECT ? (uint64_t(1) << a.fragBits) : outerMaxSlots(a.rChunk);
  K *table = reinterpret_cast<K *>(smem);
  uint32_t *hitBits = reinterpret_cast<uint32_t *>(smem + maxSlots * sizeof(K));  // one bit per slot (not DIRECT)
  unsigned long long *wsum =
      reinterpret_cast<unsigned long long *>(smem + maxSlots * sizeof(K) + (DIRECT ? 0 : maxSlots / 8));
  const uint32_t t = threadIdx.x, lane = t & (WAVE - 1);
  const uint32_t nItems = min(*nItemsPtr, capacity);
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
    const unsigned long long matchesBefore = matches;

    // First inner batch and first outer batch are in flight while the table is cleared.
    K rv[OJ_K], sv[OJ_K];
    if (nr >= BATCH) outerLoad<LAYOUT, true>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv);
    else outerLoad<LAYOUT, false>(a.R, a.Rhi, rb, nr, 0, a.fragShift, rv);
    if (ns >= BATCH) outerLoad<LAYOUT, true>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv);
    else outerLoad<LAYOUT, false>(a.S, a.Shi, sb, ns, 0, a.fragShift, sv);
    for (uint32_t i = t; i < slots; i += OJ_T) table[i] = DIRECT ? (K)0 : EMPTY;
    if constexpr (!DIRECT)
      for (uint32_t i = t; i < (slots >> 5); i += OJ_T) hitBits[i] = 0;
    __syncthreads();

    // ---- build: every inner copy takes a slot
    for (uint32_t b0 = 0; b0 < nr; b0 += BATCH) {
      if (b0) outerLoad<LAYOUT, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv);
#pragma unroll
      for (int k = 0; k < OJ_K; ++k) {
        if (b0 + k * OJ_T + t < nr) {
          const K key = rv[k];
          if constexpr (DIRECT) {
            atomicAdd(&table[key], (K)1);
          } else {
            uint32_t h = outerHash<LAYOUT>(key, tbits);
            while (atomicCAS(&table[h], EMPTY, key) != EMPTY) h = (h + 1) & mask;
          }
        }
      }
    }
    __syncthreads();

    // ---- probe: the whole chain (pairs with multiplicity), one mask per wave and batch row
    for (uint32_t b0 = 0; b0 < ns; b0 += BATCH) {
      if (b0) {
        if (b0 + BATCH <= ns) outerLoad<LAYOUT, true>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv);
        else outerLoad<LAYOUT, false>(a.S, a.Shi, sb, ns, b0, a.fragShift, sv);
      }
#pragma unroll
      for (int k = 0; k < OJ_K; ++k) {
        const uint32_t row0 = b0 + k * OJ_T + (t - lane);  // the wave's first tuple of this row (wave-uniform)
        if (row0 >= ns) break;
        uint32_t found = 0;
        if (row0 + lane < ns) {
          const K key = sv[k];
          if constexpr (DIRECT) {
            const uint32_t e = (uint32_t)table[key];  // the counts are final: the probe only ever sets bit 31
            found = e & ~OJ_HIT;
            if (found && marksR && !(e & OJ_HIT)) atomicOr(reinterpret_cast<uint32_t *>(&table[key]), OJ_HIT);
          } else {
            uint32_t h = outerHash<LAYOUT>(key, tbits);
            K e;
            while ((e = table[h]) != EMPTY) {
              if (e == key) {
                // the first slot of the key carries its hit bit (set once: later probes of the key see it)
                if (found == 0 && marksR && !((hitBits[h >> 5] >> (h & 31)) & 1))
                  atomicOr(&hitBits[h >> 5], 1u << (h & 31));
                ++found;
              }
              h = (h + 1) & mask;
            }
          }
        }
        matches += found;
        if (marksS) {
          const unsigned long long m = __ballot(found != 0);
          if (lane == 0 && m) outerOrMask(marksS, sb + row0, m);
        }
      }
    }

    // ---- inner side: the hit bit of the first slot of every inner tuple's key
    if (marksR) {
      __syncthreads();
      for (uint32_t b0 = 0; b0 < nr; b0 += BATCH) {
        if (nr > BATCH) outerLoad<LAYOUT, false>(a.R, a.Rhi, rb, nr, b0, a.fragShift, rv);  // else still in registers
#pragma unroll
        for (int k = 0; k < OJ_K; ++k) {
          const uint32_t row0 = b0 + k * OJ_T + (t - lane);
          if (row0 >= nr) break;
          bool hit = false;
          if (row0 + lane < nr) {
            const K key = rv[k];
            if constexpr (DIRECT) {
              hit = ((uint32_t)table[key] & OJ_HIT) != 0;
            } else {
              uint32_t h = outerHash<LAYOUT>(key, tbits);
              while (table[h] != key) h = (h + 1) & mask;  // the key is in the table: this tuple inserted it
              hit = (hitBits[h >> 5] >> (h & 31)) & 1;
            }
          }
          const unsigned long long m = __ballot(hit);
          if (lane == 0 && m) outerOrMask(marksR, rb + row0, m);
        }
      }
    }
    const unsigned long long im = blockReduceSum<OJ_T, unsigned long long>(matches - matchesBefore, wsum);
    if (t == 0) a.itemCounts[w] = (uint32_t)im;
    __syncthreads();  // the next item clears the table
  }
  const unsigned long long total = blockReduceSum<OJ_T, unsigned long long>(matches, wsum);
  if (t == 0 && total) atomicAdd(a.result, total);
}

// ------------------------------------------------------------------- units
// (unit geometry and selection as semi_join.hip)
__device__ __forceinline__ void outerUnitRange(const BPArgs &a, const MarkUnit u, uint64_t &ub, uint64_t &ue) {
  ub = a.partS[u.part] + (uint64_t)u.chunk * a.sChunk;
  ue = min(a.partSEnd[u.part], ub + a.sChunk);
}

// Unmarked positions of mark word w within [ub, ue).
__device__ __forceinline__ unsigned long long outerUnitUnmarked(const unsigned long long *__restrict__ marks,
                                                                uint64_t w, uint64_t ub, uint64_t ue) {
  unsigned long long valid = ~0ull;
  if (w == (ub >> 6)) valid &= ~0ull << (ub & 63);
  if (w == ((ue - 1) >> 6)) valid &= ~0ull >> (63 - ((ue - 1) & 63));
  return ~marks[w] & valid;
}

template <int LAYOUT>
__device__ __forceinline__ unsigned long long outerRid(const BPArgs &a, uint64_t pos, uint64_t ridMask) {
  if constexpr (LAYOUT == OJ_SPLIT)
    return reinterpret_cast<const uint32_t *>(a.S)[pos];
  else if constexpr (LAYOUT == OJ_COMPRESSED)
    return reinterpret_cast<const unsigned long long *>(a.S)[pos] & ridMask;
  else
    return reinterpret_cast<const unsigned long long *>(a.S)[2 * pos + 1];
}

// One wave per unit of a.S (the preserved side; the inner one with the sides
// swapped), as markPlaceKernel: per round a lane reads one of the unit's next
// 64 mark words, a wave scan of their popcounts gives every word its offset,
// and the words are placed four at a time.
template <int LAYOUT>
__global__ __launch_bounds__(OJ_T) void markPlacePairsKernel(BPArgs a, const MarkUnit *__restrict__ units,
                                                            const uint32_t *__restrict__ nUnitsPtr, uint32_t capacity,
                                                            const unsigned long long *__restrict__ marks,
                                                            const unsigned long long *__restrict__ unitOffsets,
                                                            const unsigned long long *__restrict__ base0,
                                                            const unsigned long long *__restrict__ base1, bool innerSide,
                                                            ulonglong2 *__restrict__ out, uint64_t outCapacity) {
  constexpr int U = 4;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const unsigned long long below = (1ull << lane) - 1;
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  const uint32_t nUnits = min(*nUnitsPtr, capacity);
  const uint32_t wavesPerGrid = gridDim.x * (OJ_T / WAVE);
  const unsigned long long first = *base0 + (base1 ? *base1 : 0ull);  // rows written before this side
  for (uint32_t u = blockIdx.x * (OJ_T / WAVE) + threadIdx.x / WAVE; u < nUnits; u += wavesPerGrid) {
    uint64_t ub, ue;
    outerUnitRange(a, units[u], ub, ue);
    const uint64_t w0 = ub >> 6, wl = (ue - 1) >> 6;
    unsigned long long base = first + unitOffsets[u];
    for (uint64_t wb = w0; wb <= wl; wb += WAVE) {
      const unsigned long long sel = wb + lane <= wl ? outerUnitUnmarked(marks, wb + lane, ub, ue) : 0ull;
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
          if ((s[j] >> lane) & 1) rid[j] = outerRid<LAYOUT>(a, ((wb + i + j) << 6) + lane, ridMask);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
          if ((s[j] >> lane) & 1) {
            const unsigned long long at = base + o[j] + (uint32_t)__popcll(s[j] & below);
            if (at < outCapacity)
              out[at] = innerSide ? make_ulonglong2(rid[j], NULL_RID) : make_ulonglong2(NULL_RID, rid[j]);
          }
        }
      }
      base += __shfl(incl, WAVE - 1, WAVE);
    }
  }
}

// Small units are latency-bound per wave: the grid fills every CU with waves (as semi_join.hip).
static uint32_t outerUnitGrid(uint32_t capacity) {
  const uint32_t perBlock = OJ_T / WAVE;
  return std::max<uint32_t>(1, std::min<uint32_t>(256 * 8, (capacity + perBlock - 1) / perBlock));
}

static BPArgs outerArgs(const BPArgs &args) {
  BPArgs a = args;
  if (!a.partREnd) a.partREnd = a.partR + 1;
  if (!a.partSEnd) a.partSEnd = a.partS + 1;
  return a;
}

size_t bpOuterLdsBytes(const BPArgs &a) {
  if (outerDirect(a)) return (size_t(4) << a.fragBits) + 64;
  const uint64_t slots = outerMaxSlots(a.rChunk);
  return slots * (a.wide ? 8 : 4) + slots / 8 + 64;
}

void bpOuterCount(const BPArgs &args, const BPItem *items, const uint32_t *nItems, uint32_t capacity,
                  unsigned long long *marksR, unsigned long long *marksS, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = outerArgs(args);
  const size_t lds = bpOuterLdsBytes(a);
  HJ_CHECK(lds <= 160 * 1024, "bpOuterCount: LDS request %zu exceeds 160 KiB (rChunk=%u)", lds, a.rChunk);
  HJ_CHECK(!a.keyOnly, "bpOuterCount: key-only words carry no rid (outer joins use rid-carrying layouts)");
  HJ_CHECK(!(a.split && a.wide), "bpOuterCount: the split layout holds compressed tuples");
  HJ_CHECK(!a.split || (a.Rhi && a.Shi), "bpOuterCount: split layout without fragment columns");
  HJ_CHECK(a.wide || a.fragShift >= 32,
           "bpOuterCount: fragShift=%u < 32 (the rid field of a CompressedTuple is >= 32 bits)", a.fragShift);
  HJ_CHECK(a.itemCounts && a.result, "bpOuterCount: needs the per-item counts and the pair counter");
  const uint32_t perCu = (uint32_t)std::max<size_t>(1, std::min<size_t>(a.wide ? 2 : a.split ? 4 : 3, (160 * 1024) / lds));
  const uint32_t blocks = std::min<uint32_t>(capacity, 256 * perCu);
#define HJ_OJ_COUNT(LAYOUT, DIRECT)                                                                              \
  hipLaunchKernelGGL((bpOuterCountKernel<LAYOUT, DIRECT>), dim3(blocks), dim3(OJ_T), lds, s, a, items, nItems, capacity, \
                     marksR, marksS)
  const bool direct = outerDirect(a);
  switch (outerLayout(a)) {
    case OJ_COMPRESSED:
      if (direct) HJ_OJ_COUNT(OJ_COMPRESSED, true); else HJ_OJ_COUNT(OJ_COMPRESSED, false);
      break;
    case OJ_SPLIT:
      if (direct) HJ_OJ_COUNT(OJ_SPLIT, true); else HJ_OJ_COUNT(OJ_SPLIT, false);
      break;
    default:
      HJ_OJ_COUNT(OJ_WIDE, false);
      break;
  }
#undef HJ_OJ_COUNT
  HIP_CHECK_LAUNCH();
}

void markPlacePairs(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
                    const unsigned long long *marks, const unsigned long long *unitOffsets,
                    const unsigned long long *base0, const unsigned long long *base1, bool innerSide, ulonglong2 *out,
                    uint64_t outCapacity, hipStream_t s) {
  if (capacity == 0) return;
  const BPArgs a = outerArgs(args);
  HJ_CHECK(!a.keyOnly, "markPlacePairs: key-only words carry no rid");
  HJ_CHECK(base0, "markPlacePairs: needs the row count written before this side");
  const dim3 grid(outerUnitGrid(capacity)), block(OJ_T);
  switch (outerLayout(a)) {
    case OJ_COMPRESSED:
      hipLaunchKernelGGL(markPlacePairsKernel<OJ_COMPRESSED>, grid, block, 0, s, a, units, nUnits, capacity, marks,
                         unitOffsets, base0, base1, innerSide, out, outCapacity);
      break;
    case OJ_SPLIT:
      hipLaunchKernelGGL(markPlacePairsKernel<OJ_SPLIT>, grid, block, 0, s, a, units, nUnits, capacity, marks,
                         unitOffsets, base0, base1, innerSide, out, outCapacity);
      break;
    default:
      hipLaunchKernelGGL(markPlacePairsKernel<OJ_WIDE>, grid, block, 0, s, a, units, nUnits, capacity, marks,
                         unitOffsets, base0, base1, innerSide, out, outCapacity);
      break;
  }
  HIP_CHECK_LAUNCH();
}

BPArgs outerSwapSides(const BPArgs &a, uint32_t unit) {
  BPArgs u = a;
  u.S = a.R;
  u.Shi = a.Rhi;
  u.partS = a.partR;
  u.partSEnd = a.partREnd;
  u.sChunk = unit;
  return u;
}

// Loads this file's code object at engine start (kernels::preloadCodeObjects).
void preloadOuterJoin() {
  hipFuncAttributes a;
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&markPlacePairsKernel<OJ_COMPRESSED>)));
}

}  // namespace kernels
}  // namespace hpcjoin
