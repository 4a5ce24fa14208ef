// Payload rows of semi, anti and outer joins at N = 1 (core::JoinKind): the
// rows a user of those kinds wants, written without the detour over a rid or
// pair list and a generic gather.
//
// Row shapes (kernels.h, KindRowShape):
//   Rid       5 words  {rid, row}                      one per qualifying outer tuple of a semi / anti join
//   InnerPad 10 words  {rid, NULL_RID, row, NULL x 4}   unmatched inner tuple of an outer join
//   OuterPad 10 words  {NULL_RID, rid, NULL x 4, row}   unmatched outer tuple of an outer join
// The matched rows of an outer join are the inner join's and come from its
// fused row kernels (build_probe.hip); a NULL rid never forms an address.
//
//  * markPlaceRowsKernel -- the row-writing twin of markPlaceKernel /
//    markPlacePairsKernel: one wave per MarkUnit, same marks, unit offsets and
//    base counters, the three layouts through markRid<LAYOUT>.  A lane reads
//    one of the unit's next 64 mark words; the words are then taken four at a
//    time (the four rid loads issued first) and the selected rids appended, by
//    popcount rank, to a wave-private ring of 128 rids in LDS.  Whenever 64 are
//    queued the wave writes 64 rows (the rest at the unit's end), so every
//    gather and store has its lanes busy whatever the selectivity: a word with
//    one selected position would otherwise cost a whole gather instruction.
//  * writing up to 64 rows (krWriteRows): the payload is gathered by lane
//    pairs, lanes 2j and 2j + 1 loading the two 16-byte halves of row j
//    (non-temporal: each row is read once), the rows are assembled in a
//    wave-private staging buffer and stored as consecutive pieces, so each
//    store instruction of the wave covers one contiguous run.  10-word rows
//    start 16-byte aligned and go out as 16-byte pieces; 5-word rows start
//    16-byte aligned only at even row indices and unit offsets are arbitrary,
//    so they go out as 8-byte pieces.  Staging writes and reads are ordered by
//    the wavefront fence + wave_barrier idiom of materializeLocalKernel (no
//    __syncthreads: the waves of a block walk different units).
//  * ridRowsKernel -- unfused: out[i] = {rids[i], rows[rids[i] - rowOffset]}
//    over a rid list (the set-bitmap plan's rids, the host-planned paths), 64
//    rids per wave and step through the same row writer.
// The NULL-aware pair rows of an unfused outer join are materializeLocalKernel
// with its NULLS flag (materialize.hip).
//
// A unit's rows land at [base + unitOffsets[u], + unitCounts[u]) in position
// order; rows at or beyond outCapacity are not stored.
//
// Measured (MI355X, 128M x 128M, inner UNIFORM over |R| / 4, outer Zipf(0.75)
// over 2 |R|, split layout, wall ms per join + rows, median of 5, two rounds;
// tools/bench_kind_rows.py, profiles/kind_rows/README.md), fused vs unfused:
//   semi   15.7M rows   3.69 / 3.62 vs  3.72 / 3.66     anti  112.3M rows   6.93 / 6.76 vs  7.00 / 7.05
//   left  158.0M rows  15.71 / 15.59 vs 12.36 / 12.37   right 176.0M rows  30.97 / 31.02 vs 17.09 / 17.21
//   full  270.3M rows  40.18 / 40.36 vs 22.63 / 22.95
// Semi / anti: fused is level with or ahead of unfused (it skips the rid list)
// and is the default.  Outer kinds: fused loses.  Its build/probe span is 13.2
// ms (left) against 4.3 ms + ~5.3 ms of materializeLocal over the pair list --
// markPlaceRows moves ~2.3 TB/s of row bytes (anti: 8.1 GB in the 3.6 ms it
// adds to the span) where materializeLocal streams the dense pair list at ~3.7
// TB/s -- and right / full overflow the caller's default buffer (outer rows +
// 1024, plus the inner rows when the inner side is preserved), so every such
// join runs twice.  Outer kinds therefore stay unfused unless
// variants.kindRows = 1 asks for the fused path (kept selectable).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// kernel uses scratch):
//   markPlaceRowsKernel<*, Rid>       80 VGPRs (all layouts), 14 KiB LDS per block (3.5 KiB per wave)
//   markPlaceRowsKernel<*, InnerPad>  88 VGPRs (split: 90), 24 KiB LDS per block (6 KiB per wave)
//   markPlaceRowsKernel<*, OuterPad>  88 VGPRs (split: 90), 24 KiB LDS per block
//   ridRowsKernel                     41 VGPRs, 10 KiB LDS per block
#include "kernels.h"
#include "device_common.h"
#include "mark_units.h"

#include <algorithm>

namespace hpcjoin {
namespace kernels {

constexpr int KR_T = 256;
constexpr int KR_WAVES = KR_T / WAVE;
constexpr uint32_t KR_QUEUE = 128;  // rids per wave: 63 left over + one mark word of 64 always fit
constexpr int KR_RID = (int)KindRowShape::Rid, KR_INNER = (int)KindRowShape::InnerPad,
              KR_OUTER = (int)KindRowShape::OuterPad;
using kr_u64x2 = unsigned long long __attribute__((ext_vector_type(2)));

template <int SHAPE>
struct KindRow {
  static constexpr uint32_t W = SHAPE == KR_RID ? RID_ROW_WORDS : PAIR_ROW_WORDS;  // words per output row
  static constexpr uint32_t ROW_AT = SHAPE == KR_RID ? 1 : SHAPE == KR_INNER ? 2 : 6;  // word of the payload row
  static constexpr uint32_t PAD_AT = SHAPE == KR_INNER ? 6 : 2;                        // word of the NULL row (pads)
};

__device__ __forceinline__ void krWaveSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave writes rows [0, m) of one run (m <= 64), of which the first mStore
// are stored to dst (the run's first output word).  ridLane: rid of row
// `lane`; ridHalf[k]: rid of row (lane >> 1) + 32 k, whose 16-byte half
// (lane & 1) this lane loads.  w: the wave's staging buffer, W * 64 words.
template <int SHAPE>
__device__ __forceinline__ void krWriteRows(unsigned long long *w, unsigned long long ridLane,
                                            const unsigned long long (&ridHalf)[2], uint32_t m, uint32_t mStore,
                                            const ulonglong2 *__restrict__ rows, uint64_t rowOffset,
                                            unsigned long long *__restrict__ dst, uint32_t lane) {
  constexpr uint32_t W = KindRow<SHAPE>::W, ROW_AT = KindRow<SHAPE>::ROW_AT, PAD_AT = KindRow<SHAPE>::PAD_AT;
  const uint32_t half = lane & 1;
  kr_u64x2 r[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t j = (lane >> 1) + 32 * k;
    if (j < m)
      r[k] = __builtin_nontemporal_load(reinterpret_cast<const kr_u64x2 *>(rows + 2 * (ridHalf[k] - rowOffset) + half));
  }
  if (lane < m) {
    if constexpr (SHAPE == KR_RID) {
      w[W * lane] = ridLane;
    } else {
      w[W * lane] = SHAPE == KR_INNER ? ridLane : NULL_RID;
      w[W * lane + 1] = SHAPE == KR_INNER ? NULL_RID : ridLane;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t j = (lane >> 1) + 32 * k;
    if (j < m) {
      w[W * j + ROW_AT + 2 * half] = r[k].x;
      w[W * j + ROW_AT + 2 * half + 1] = r[k].y;
      if constexpr (SHAPE != KR_RID) {
        w[W * j + PAD_AT + 2 * half] = NULL_RID;
        w[W * j + PAD_AT + 2 * half + 1] = NULL_RID;
      }
    }
  }
  krWaveSync();
  if constexpr (SHAPE == KR_RID) {  // 8-byte pieces: a 40-byte row is 16-byte aligned at even row indices only
#pragma unroll
    for (uint32_t k = 0; k < W; ++k) {
      const uint32_t q = 64 * k + lane;
      if (q < W * mStore) __builtin_nontemporal_store(w[q], dst + q);
    }
  } else {  // 16-byte pieces: 80-byte rows keep every run 16-byte aligned
    const kr_u64x2 *w2 = reinterpret_cast<const kr_u64x2 *>(w);
    kr_u64x2 *d2 = reinterpret_cast<kr_u64x2 *>(dst);
#pragma unroll
    for (uint32_t k = 0; k < W / 2; ++k) {
      const uint32_t q = 64 * k + lane;
      if (q < W / 2 * mStore) __builtin_nontemporal_store(w2[q], d2 + q);
    }
  }
  krWaveSync();  // the staging buffer (and the caller's rid queue) may be rewritten
}

template <int LAYOUT, int SHAPE>
__global__ __launch_bounds__(KR_T) void markPlaceRowsKernel(BPArgs a, const MarkUnit *__restrict__ units,
                                                           const uint32_t *__restrict__ nUnitsPtr, uint32_t capacity,
                                                           const unsigned long long *__restrict__ marks, bool anti,
                                                           const unsigned long long *__restrict__ unitOffsets,
                                                           const unsigned long long *__restrict__ base0,
                                                           const unsigned long long *__restrict__ base1,
                                                           const ulonglong2 *__restrict__ rows, uint64_t rowOffset,
                                                           unsigned long long *__restrict__ out, uint64_t outCapacity) {
  constexpr int U = 4;
  constexpr uint32_t W = KindRow<SHAPE>::W;
  __shared__ unsigned long long queue[KR_WAVES][KR_QUEUE];
  __shared__ ulonglong2 stage[KR_WAVES][W * 32];  // 64 rows of W words
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  unsigned long long *q = queue[wave];
  unsigned long long *w = reinterpret_cast<unsigned long long *>(stage[wave]);
  const unsigned long long below = (1ull << lane) - 1;
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  const uint32_t nUnits = min(*nUnitsPtr, capacity);
  const uint32_t wavesPerGrid = gridDim.x * KR_WAVES;
  const unsigned long long first = (base0 ? *base0 : 0ull) + (base1 ? *base1 : 0ull);  // rows written before these
  for (uint32_t u = blockIdx.x * KR_WAVES + wave; u < nUnits; u += wavesPerGrid) {
    uint64_t ub, ue;
    unitRange(a, units[u], ub, ue);
    const uint64_t w0 = ub >> 6, wl = (ue - 1) >> 6;
    unsigned long long base = first + unitOffsets[u];  // output row of the queue's head
    uint32_t qh = 0, qn = 0;                           // ring head and fill (wave-uniform)
    // Rows [0, m) of the queue -> output rows base ..., clipped at outCapacity.
    auto flush = [&](uint32_t m) {
      krWaveSync();  // the queue writes of this wave
      const unsigned long long ridLane = q[(qh + lane) & (KR_QUEUE - 1)];
      const unsigned long long ridHalf[2] = {q[(qh + (lane >> 1)) & (KR_QUEUE - 1)],
                                             q[(qh + (lane >> 1) + 32) & (KR_QUEUE - 1)]};
      const uint32_t mStore =
          base >= outCapacity ? 0u : (uint32_t)min((unsigned long long)m, (unsigned long long)outCapacity - base);
      krWriteRows<SHAPE>(w, ridLane, ridHalf, m, mStore, rows, rowOffset, out + base * W, lane);
      qh = (qh + m) & (KR_QUEUE - 1);
      qn -= m;
      base += m;
    };
    for (uint64_t wb = w0; wb <= wl; wb += WAVE) {
      const unsigned long long sel = wb + lane <= wl ? unitSelect(marks, wb + lane, ub, ue, anti) : 0ull;
      const uint32_t nw = (uint32_t)min((uint64_t)WAVE, wl - wb + 1);  // wave-uniform
      for (uint32_t i = 0; i < nw; i += U) {
        unsigned long long s[U], rid[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
          const uint32_t src = min(i + j, nw - 1);
          const uint32_t lo = __shfl((uint32_t)sel, src, WAVE), hi = __shfl((uint32_t)(sel >> 32), src, WAVE);
          s[j] = i + j < nw ? ((unsigned long long)hi << 32) | lo : 0ull;
          rid[j] = 0;
          if ((s[j] >> lane) & 1) rid[j] = markRid<LAYOUT>(a, ((wb + i + j) << 6) + lane, ridMask);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
          if ((s[j] >> lane) & 1) q[(qh + qn + (uint32_t)__popcll(s[j] & below)) & (KR_QUEUE - 1)] = rid[j];
          qn += (uint32_t)__builtin_amdgcn_readfirstlane(__popcll(s[j]));  // s[j] is the same in every lane
          if (qn >= WAVE) flush(WAVE);
        }
      }
    }
    if (qn) flush(qn);
  }
}

__global__ __launch_bounds__(KR_T) void ridRowsKernel(const unsigned long long *__restrict__ rids, uint64_t n,
                                                     const ulonglong2 *__restrict__ rows, uint64_t rowOffset,
                                                     unsigned long long *__restrict__ out) {
  __shared__ ulonglong2 stage[KR_WAVES][RID_ROW_WORDS * 32];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  unsigned long long *w = reinterpret_cast<unsigned long long *>(stage[wave]);
  const uint64_t steps = ceilDiv(n, WAVE), waveStride = (uint64_t)gridDim.x * KR_WAVES;
  for (uint64_t st = (uint64_t)blockIdx.x * KR_WAVES + wave; st < steps; st += waveStride) {
    const uint64_t base = st * WAVE;
    const uint32_t m = (uint32_t)(n - base < WAVE ? n - base : WAVE);
    const unsigned long long ridLane = lane < m ? rids[base + lane] : rowOffset;
    const unsigned long long ridHalf[2] = {__shfl(ridLane, lane >> 1, WAVE), __shfl(ridLane, (lane >> 1) + 32, WAVE)};
    krWriteRows<KR_RID>(w, ridLane, ridHalf, m, m, rows, rowOffset, out + base * RID_ROW_WORDS, lane);
  }
}

// Small units are latency-bound per wave: the grid fills every CU with waves (as semi_join.hip).
static uint32_t kindUnitGrid(uint32_t capacity) {
  return std::max<uint32_t>(1, std::min<uint32_t>(256 * 8, (capacity + KR_WAVES - 1) / KR_WAVES));
}

void markPlaceRows(const BPArgs &args, const MarkUnit *units, const uint32_t *nUnits, uint32_t capacity,
                   const unsigned long long *marks, bool anti, const unsigned long long *unitOffsets,
                   const unsigned long long *base0, const unsigned long long *base1, KindRowShape shape,
                   const uint64_t *rows, uint64_t rowOffset, uint64_t *out, uint64_t outCapacity, hipStream_t s) {
  if (capacity == 0) return;
  BPArgs a = args;
  if (!a.partREnd) a.partREnd = a.partR + 1;
  if (!a.partSEnd) a.partSEnd = a.partS + 1;
  HJ_CHECK(!a.keyOnly, "markPlaceRows: key-only words carry no rid");
  HJ_CHECK(!(a.split && a.wide), "markPlaceRows: the split layout holds compressed tuples");
  HJ_CHECK(rows && out, "markPlaceRows: needs the payload rows and the output");
  HJ_CHECK(reinterpret_cast<uintptr_t>(rows) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
           "markPlaceRows: payload rows and output must be 16-byte aligned");
  const dim3 grid(kindUnitGrid(capacity)), block(KR_T);
  const auto *r = reinterpret_cast<const ulonglong2 *>(rows);
  auto *o = reinterpret_cast<unsigned long long *>(out);
#define HJ_KR_PLACE(LAYOUT, SHAPE)                                                                                  \
  hipLaunchKernelGGL((markPlaceRowsKernel<LAYOUT, SHAPE>), grid, block, 0, s, a, units, nUnits, capacity, marks, anti, \
                     unitOffsets, base0, base1, r, rowOffset, o, outCapacity)
#define HJ_KR_SHAPES(LAYOUT)                                      \
  switch (shape) {                                                \
    case KindRowShape::Rid: HJ_KR_PLACE(LAYOUT, KR_RID); break;   \
    case KindRowShape::InnerPad: HJ_KR_PLACE(LAYOUT, KR_INNER); break; \
    default: HJ_KR_PLACE(LAYOUT, KR_OUTER); break;                \
  }
  switch (markLayout(a)) {
    case MK_COMPRESSED: HJ_KR_SHAPES(MK_COMPRESSED) break;
    case MK_SPLIT: HJ_KR_SHAPES(MK_SPLIT) break;
    default: HJ_KR_SHAPES(MK_WIDE) break;
  }
#undef HJ_KR_SHAPES
#undef HJ_KR_PLACE
  HIP_CHECK_LAUNCH();
}

void ridRows(const uint64_t *rids, uint64_t n, const uint64_t *rows, uint64_t rowOffset, uint64_t *out,
             hipStream_t s) {
  if (!n) return;
  HJ_CHECK(reinterpret_cast<uintptr_t>(rows) % 16 == 0, "ridRows: payload rows must be 16-byte aligned");
  const uint64_t blocks = ceilDiv(ceilDiv(n, WAVE), KR_WAVES);
  hipLaunchKernelGGL(ridRowsKernel, dim3((uint32_t)std::min<uint64_t>(blocks, 8192)), dim3(KR_T), 0, s,
                     reinterpret_cast<const unsigned long long *>(rids), n, reinterpret_cast<const ulonglong2 *>(rows),
                     rowOffset, reinterpret_cast<unsigned long long *>(out));
  HIP_CHECK_LAUNCH();
}

// Loads this file's code object at engine start (kernels::preloadCodeObjects).
void preloadKindRows() {
  hipFuncAttributes a;
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&ridRowsKernel)));
}

}  // namespace kernels
}  // namespace hpcjoin
