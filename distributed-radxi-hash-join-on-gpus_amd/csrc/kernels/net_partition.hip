// Pass 1 (network partitioning) for MI355X (gfx950): replaces the CPU
// software-write-combining loop of the reference's tasks/NetworkPartitioning.cpp:74-222
// and the LocalHistogram pass of its histograms/LocalHistogram.cpp:35-53.
//
// Design (CDNA4-first, not a translation):
//  * Histogram: one workgroup (4 wave64s) owns a contiguous run of 4096-tuple
//    tiles; each wave counts into its own LDS sub-histogram (4 x F u32), which
//    cuts LDS atomic contention 4x, then the block writes a digit-major
//    [F][blocks] histogram so ONE exclusive scan per digit yields every
//    block's private output cursor (no global atomics, no inter-WG hand-off).
//  * Scatter = LDS write-combining in claim mode (scatter_core.h).
#include "scatter_core.h"

#include <algorithm>
#include <cstdlib>
#include <cmath>

namespace hpcjoin {
namespace kernels {

PartitionGeometry partitionGeometry(uint64_t n, uint32_t maxBlocks) {
  PartitionGeometry g;
  const uint64_t tiles = ceilDiv(n, PART_TILE);
  if (tiles == 0) {
    g.blocks = 1;
    g.tilesPerBlock = 1;
    return g;
  }
  g.tilesPerBlock = (uint32_t)ceilDiv(tiles, maxBlocks);
  g.blocks = (uint32_t)ceilDiv(tiles, g.tilesPerBlock);
  return g;
}

// Calls fn with the typed element pointer of a key source: 16-byte tuples or
// a key column (kernels.h, KeySource).
template <class Fn>
static void withKeyElements(const char *who, const KeySource &in, Fn &&fn) {
  HJ_CHECK(in.strideWords == 1 || in.strideWords == 2, "%s: keys %u words apart", who, in.strideWords);
  if (in.isColumn())
    fn(reinterpret_cast<const uint64_t *>(in.base));
  else
    fn(reinterpret_cast<const ulonglong2 *>(in.base));
}
__device__ __forceinline__ uint64_t keyOf(const ulonglong2 &x) { return x.x; }
__device__ __forceinline__ uint64_t keyOf(const uint64_t &x) { return x; }

// ------------------------------------------------------- histogram (pass 1)
template <typename InT>
__device__ __forceinline__ void netHistogramBody(const InT *__restrict__ in, uint64_t n, uint32_t tpb,
                                                 uint32_t bits, uint32_t *__restrict__ blockHist, KeyMix mix,
                                                 uint32_t stride, uint32_t *hsh) {
  const uint32_t F = 1u << bits, mask = F - 1;
  const int wid = threadIdx.x / WAVE;
  for (uint32_t i = threadIdx.x; i < 4 * F; i += NT) hsh[i] = 0;
  __syncthreads();
  uint32_t *wh = hsh + wid * F;
  const uint64_t begin = (uint64_t)blockIdx.x * tpb * PART_TILE;
  const uint64_t end = min(n, begin + (uint64_t)tpb * PART_TILE);
  for (uint64_t base = begin; base < end; base += (uint64_t)PART_TILE * stride) {
    uint64_t k[PART_ITEMS];
#pragma unroll
    for (int i = 0; i < (int)PART_ITEMS; ++i) {
      const uint64_t idx = base + (uint64_t)i * NT + threadIdx.x;
      k[i] = idx < end ? mix.apply(keyOf(in[idx])) : 0;
    }
#pragma unroll
    for (int i = 0; i < (int)PART_ITEMS; ++i) {
      const uint64_t idx = base + (uint64_t)i * NT + threadIdx.x;
      if (idx < end) atomicAdd(&wh[k[i] & mask], 1u);
    }
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < F; d += NT)
    blockHist[(uint64_t)d * gridDim.x + blockIdx.x] = hsh[d] + hsh[F + d] + hsh[2 * F + d] + hsh[3 * F + d];
}

// Exact (every tile) and sampled (1 tile in `stride`) launches are separate
// kernels so that a trace tells a full pre-read from a sample.
template <typename InT>
__global__ __launch_bounds__(NT) void netHistogramKernel(const InT *__restrict__ in, uint64_t n, uint32_t tpb,
                                                         uint32_t bits, uint32_t *__restrict__ blockHist,
                                                         KeyMix mix) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hsh[];
  netHistogramBody(in, n, tpb, bits, blockHist, mix, 1, hsh);
}

template <typename InT>
__global__ __launch_bounds__(NT) void netSampledHistogramKernel(const InT *__restrict__ in, uint64_t n, uint32_t tpb,
                                                                uint32_t bits, uint32_t *__restrict__ blockHist,
                                                                KeyMix mix, uint32_t stride) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hsh[];
  netHistogramBody(in, n, tpb, bits, blockHist, mix, stride, hsh);
}

void netHistogram(KeySource in, uint64_t n, uint32_t bits, const PartitionGeometry &g, uint32_t *blockHist,
                  hipStream_t s, KeyMix mix, uint32_t sampleStride) {
  HJ_CHECK(bits >= 1 && bits <= MAX_PART_BITS, "netHistogram: bits=%u out of range", bits);
  HJ_CHECK(sampleStride >= 1, "netHistogram: sampleStride must be >= 1");
  const size_t lds = size_t(4) << bits << 2;
  withKeyElements("netHistogram", in, [&](auto *src) {
    using InT = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
    if (sampleStride > 1)
      hipLaunchKernelGGL(netSampledHistogramKernel<InT>, dim3(g.blocks), dim3(NT), lds, s, src, n, g.tilesPerBlock,
                         bits, blockHist, mix, sampleStride);
    else
      hipLaunchKernelGGL(netHistogramKernel<InT>, dim3(g.blocks), dim3(NT), lds, s, src, n, g.tilesPerBlock, bits,
                         blockHist, mix);
  });
  HIP_CHECK_LAUNCH();
}

// ---------------------------------------- sampled per-(group, digit) totals
// A sampled pass only needs per-(XCD group, digit) totals.  Group g's tiles
// (those of blocks b = g mod NGROUPS, block by block) are numbered 0, 1, ...;
// every stride-th of them is sampled, one workgroup per sampled tile, and its
// LDS histogram is added into totals[g][d] with one device atomic per
// non-empty digit.  Against netHistogram + netGroupTotals (every block of the
// geometry runs, samples its own tiles and writes F block counts) this reads
// 1/stride of the input at every size -- a block range shorter than stride
// tiles still sampled one full tile, 1/15 of a 125M-tuple input -- and writes
// no per-block array (47-57 us -> see profiles at 125M).  sampleScale()
// computes the same tile set on the host.
__host__ __device__ inline uint64_t sampledTile(uint64_t local, uint32_t g, uint32_t tpb) {
  return ((local / tpb) * NGROUPS + g) * tpb + local % tpb;
}

struct SampledSideArgs {
  const uint64_t *in;  // key i at in[i << wordShift]: 1 = tuples, 0 = a key column
  uint32_t wordShift;
  uint64_t n;
  uint32_t tpb, blocks, stride;
  unsigned long long *totals;  // [NGROUPS][F]
};

// Workgroups [0, wgA) sample side a, the rest side b (both sides of a join
// in one launch).
__global__ __launch_bounds__(NT) void netSampledTotalsKernel(SampledSideArgs a, SampledSideArgs b, uint32_t wgA,
                                                             uint32_t bits, KeyMix mix) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hsh[];
  const bool onB = blockIdx.x >= wgA;
  const SampledSideArgs &sd = onB ? b : a;
  const uint32_t w = onB ? blockIdx.x - wgA : blockIdx.x;
  const uint32_t g = w % NGROUPS;
  const uint64_t local = (uint64_t)(w / NGROUPS) * sd.stride;
  const uint64_t tile = sampledTile(local, g, sd.tpb);
  const uint64_t begin = tile * PART_TILE, n = sd.n;
  if (tile / sd.tpb >= sd.blocks || begin >= n) return;  // uniform over the workgroup
  const uint64_t end = min(n, begin + PART_TILE);
  const uint64_t *__restrict__ in = sd.in;
  const uint32_t F = 1u << bits, mask = F - 1, ws = sd.wordShift;
  for (uint32_t i = threadIdx.x; i < 4 * F; i += NT) hsh[i] = 0;
  __syncthreads();
  uint32_t *wh = hsh + (threadIdx.x / WAVE) * F;
  uint64_t k[PART_ITEMS];
#pragma unroll
  for (int i = 0; i < (int)PART_ITEMS; ++i) {
    const uint64_t idx = begin + (uint64_t)i * NT + threadIdx.x;
    k[i] = idx < end ? mix.apply(in[idx << ws]) : 0;
  }
#pragma unroll
  for (int i = 0; i < (int)PART_ITEMS; ++i) {
    const uint64_t idx = begin + (uint64_t)i * NT + threadIdx.x;
    if (idx < end) atomicAdd(&wh[k[i] & mask], 1u);
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < F; d += NT) {
    const uint32_t c = hsh[d] + hsh[F + d] + hsh[2 * F + d] + hsh[3 * F + d];
    if (c) atomicAdd(&sd.totals[(uint64_t)g * F + d], (unsigned long long)c);
  }
}

// Tiles of XCD group g in geometry gm (blocks b = g mod NGROUPS).
static uint64_t groupTiles(const PartitionGeometry &gm, uint64_t n, uint32_t g) {
  const uint64_t tiles = ceilDiv(n, PART_TILE);
  uint64_t t = 0;
  for (uint32_t b = g; b < gm.blocks; b += NGROUPS) {
    const uint64_t b0 = (uint64_t)b * gm.tilesPerBlock;
    if (b0 < tiles) t += std::min<uint64_t>(gm.tilesPerBlock, tiles - b0);
  }
  return t;
}

uint32_t sampleStrideFor(const PartitionGeometry &g, uint64_t n, uint32_t F, uint32_t stride) {
  uint64_t minTiles = UINT64_MAX;
  for (uint32_t gr = 0; gr < NGROUPS; ++gr) {
    const uint64_t t = groupTiles(g, n, gr);
    if (t) minTiles = std::min(minTiles, t);
  }
  if (minTiles == UINT64_MAX || stride <= 1) return 1;
  const uint64_t most = minTiles * PART_TILE / (32ull * std::max<uint32_t>(F, 1));
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(stride, most));
}

// Workgroups one side needs (sampled tiles of its largest XCD group x groups).
static uint32_t sampledWorkgroups(const PartitionGeometry &g, uint64_t n, uint32_t stride) {
  uint64_t perGroup = 0;
  for (uint32_t gr = 0; gr < NGROUPS; ++gr) perGroup = std::max(perGroup, ceilDiv(groupTiles(g, n, gr), stride));
  HJ_CHECK(perGroup * NGROUPS < (1ull << 30), "netSampledTotals: %llu sampled tiles", (unsigned long long)perGroup);
  return (uint32_t)(perGroup * NGROUPS);
}

static SampledSideArgs sampledSide(const SampledInput &x) {
  HJ_CHECK(x.stride >= 1, "netSampledTotals: sampleStride must be >= 1");
  HJ_CHECK(x.data.strideWords == 1 || x.data.strideWords == 2, "netSampledTotals: keys %u words apart",
           x.data.strideWords);
  return SampledSideArgs{x.data.base, x.data.strideWords - 1, x.n, x.geom.tilesPerBlock, x.geom.blocks,
                         x.stride, reinterpret_cast<unsigned long long *>(x.totals)};
}

void netSampledTotals(const SampledInput *sides, uint32_t count, uint32_t bits, hipStream_t s, KeyMix mix,
                      bool preZeroed) {
  HJ_CHECK(bits >= 1 && bits <= MAX_PART_BITS, "netSampledTotals: bits=%u out of range", bits);
  HJ_CHECK(count == 1 || count == 2, "netSampledTotals: %u sides", count);
  const uint32_t F = 1u << bits;
  const size_t bytes = (size_t)NGROUPS * F * sizeof(uint64_t);
  // Both sides' totals adjacent: one clear.
  if (preZeroed) {
    // DeviceControl totals: the layout kernel that read them last cleared them.
  } else if (count == 2 && sides[1].totals == sides[0].totals + (size_t)NGROUPS * F) {
    HIP_CHECK(hipMemsetAsync(sides[0].totals, 0, 2 * bytes, s));
  } else {
    for (uint32_t i = 0; i < count; ++i) HIP_CHECK(hipMemsetAsync(sides[i].totals, 0, bytes, s));
  }
  const SampledSideArgs a = sampledSide(sides[0]), b = count == 2 ? sampledSide(sides[1]) : a;
  const uint32_t wgA = sampledWorkgroups(sides[0].geom, sides[0].n, sides[0].stride);
  const uint32_t wgB = count == 2 ? sampledWorkgroups(sides[1].geom, sides[1].n, sides[1].stride) : 0;
  if (wgA + wgB == 0) return;
  const size_t lds = size_t(4) << bits << 2;
  hipLaunchKernelGGL(netSampledTotalsKernel, dim3(wgA + wgB), dim3(NT), lds, s, a, b, wgA, bits, mix);
  HIP_CHECK_LAUNCH();
}

void netSampledTotals(KeySource in, uint64_t n, uint32_t bits, const PartitionGeometry &g,
                      uint64_t *totals, hipStream_t s, KeyMix mix, uint32_t sampleStride) {
  const SampledInput one{in, n, g, sampleStride, totals};
  netSampledTotals(&one, 1, bits, s, mix);
}

// --------------------------------------------------- digit totals / cursors
__global__ __launch_bounds__(NT) void digitTotalsKernel(const uint32_t *__restrict__ blockHist, uint32_t F,
                                                        uint32_t blocks, uint32_t bpc, uint64_t *totals) {
  __shared__ uint64_t wt[NT / WAVE];
  const uint32_t d = blockIdx.x, c = blockIdx.y;
  const uint32_t b0 = c * bpc, b1 = min(blocks, b0 + bpc);
  uint64_t s = 0;
  for (uint32_t b = b0 + threadIdx.x; b < b1; b += NT) s += blockHist[(uint64_t)d * blocks + b];
  s = blockReduceSum<NT, uint64_t>(s, wt);
  if (threadIdx.x == 0) totals[(uint64_t)c * F + d] = s;
}

void digitTotals(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t blocksPerChunk,
                 uint32_t chunks, uint64_t *totals, hipStream_t s) {
  hipLaunchKernelGGL(digitTotalsKernel, dim3(F, chunks), dim3(NT), 0, s, blockHist, F, blocks, blocksPerChunk,
                     totals);
  HIP_CHECK_LAUNCH();
}

__global__ __launch_bounds__(NT) void netCursorsKernel(const uint32_t *__restrict__ blockHist, uint32_t F,
                                                       uint32_t blocks, uint32_t bpc, const uint64_t *base,
                                                       uint64_t *cursors) {
  __shared__ uint64_t wt[NT / WAVE];
  const uint32_t d = blockIdx.x;
  const uint32_t chunks = (blocks + bpc - 1) / bpc;
  for (uint32_t c = 0; c < chunks; ++c) {
    const uint32_t b0 = c * bpc, nb = min(blocks, b0 + bpc) - b0;
    const uint64_t off = (uint64_t)d * blocks + b0;
    const uint64_t bse = base[(uint64_t)c * F + d];
    // exclusive scan of blockHist[d][b0..b0+nb) (global) -> cursors (global)
    const int per = (nb + NT - 1) / NT;
    const int b = threadIdx.x * per;
    uint64_t local = 0;
    for (int i = 0; i < per; ++i)
      if (b + i < (int)nb) local += blockHist[off + b + i];
    const uint64_t incl = waveInclusiveScan<uint64_t>(local);
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    __syncthreads();
    if (lane == WAVE - 1) wt[wid] = incl;
    __syncthreads();
    uint64_t prefix = 0;
    for (int w = 0; w < wid; ++w) prefix += wt[w];
    uint64_t run = bse + prefix + incl - local;
    for (int i = 0; i < per; ++i)
      if (b + i < (int)nb) {
        const uint64_t v = blockHist[off + b + i];
        cursors[off + b + i] = run;
        run += v;
      }
  }
}

void netCursors(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t blocksPerChunk,
                const uint64_t *base, uint64_t *cursors, hipStream_t s) {
  hipLaunchKernelGGL(netCursorsKernel, dim3(F), dim3(NT), 0, s, blockHist, F, blocks, blocksPerChunk, base,
                     cursors);
  HIP_CHECK_LAUNCH();
}

// Group cursors for claim-mode scatter: the workgroups of a chunk are split
// into NGROUPS groups by (block - chunkBegin) % NGROUPS, which is the XCD
// round-robin of the dispatcher (a speed assumption only).  Each group owns a
// contiguous slice of every digit's region, sized by the group's histogram,
// and its workgroups claim space from the slice with one device atomic per
// digit per tile.  gcur[c][g][d] = base[c][d] + sum of the earlier groups.
template <typename CurT>
__global__ __launch_bounds__(NT) void netGroupCursorsKernel(const uint32_t *__restrict__ blockHist, uint32_t F,
                                                            uint32_t blocks, uint32_t bpc, const uint64_t *base,
                                                            CurT *gcur) {
  __shared__ unsigned long long gs[NGROUPS];
  const uint32_t d = blockIdx.x;
  const uint32_t chunks = (blocks + bpc - 1) / bpc;
  for (uint32_t c = 0; c < chunks; ++c) {
    if (threadIdx.x < NGROUPS) gs[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t b0 = c * bpc, b1 = min(blocks, b0 + bpc);
    unsigned long long mine = 0;  // NT % NGROUPS == 0: thread t only sees group t % NGROUPS
    for (uint32_t b = b0 + threadIdx.x; b < b1; b += NT) mine += blockHist[(uint64_t)d * blocks + b];
    atomicAdd(&gs[threadIdx.x % NGROUPS], mine);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long run = base[(uint64_t)c * F + d];
      for (uint32_t g = 0; g < NGROUPS; ++g) {
        gcur[((uint64_t)c * NGROUPS + g) * F + d] = (CurT)run;
        run += gs[g];
      }
    }
    __syncthreads();
  }
}

void netGroupCursors(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t blocksPerChunk,
                     const uint64_t *base, void *gcur, bool narrow, hipStream_t s) {
  if (narrow)
    hipLaunchKernelGGL(netGroupCursorsKernel<uint32_t>, dim3(F), dim3(NT), 0, s, blockHist, F, blocks, blocksPerChunk,
                       base, reinterpret_cast<uint32_t *>(gcur));
  else
    hipLaunchKernelGGL(netGroupCursorsKernel<unsigned long long>, dim3(F), dim3(NT), 0, s, blockHist, F, blocks,
                       blocksPerChunk, base, reinterpret_cast<unsigned long long *>(gcur));
  HIP_CHECK_LAUNCH();
}

// totals[c][g][d]: one workgroup per (digit, chunk); thread t only sees
// blocks of group t % NGROUPS (NT % NGROUPS == 0, b0 is where the groups start).
__global__ __launch_bounds__(NT) void netChunkGroupTotalsKernel(const uint32_t *__restrict__ blockHist, uint32_t F,
                                                                uint32_t blocks, uint32_t bpc,
                                                                unsigned long long *totals) {
  __shared__ unsigned long long gs[NGROUPS];
  const uint32_t d = blockIdx.x, c = blockIdx.y;
  const uint32_t b0 = c * bpc, b1 = min(blocks, b0 + bpc);
  if (threadIdx.x < NGROUPS) gs[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (uint32_t b = b0 + threadIdx.x; b < b1; b += NT) mine += blockHist[(uint64_t)d * blocks + b];
  atomicAdd(&gs[threadIdx.x % NGROUPS], mine);
  __syncthreads();
  if (threadIdx.x < NGROUPS) totals[((uint64_t)c * NGROUPS + threadIdx.x) * F + d] = gs[threadIdx.x];
}

void netChunkGroupTotals(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t blocksPerChunk,
                         uint32_t chunks, uint64_t *totals, hipStream_t s) {
  HJ_CHECK(blocksPerChunk >= 1 && (uint64_t)chunks * blocksPerChunk >= blocks, "netChunkGroupTotals: %u x %u < %u",
           chunks, blocksPerChunk, blocks);
  hipLaunchKernelGGL(netChunkGroupTotalsKernel, dim3(F, chunks), dim3(NT), 0, s, blockHist, F, blocks,
                     blocksPerChunk, reinterpret_cast<unsigned long long *>(totals));
  HIP_CHECK_LAUNCH();
}

// totals[g][d] = sum of blockHist[d][b] over the blocks b of XCD group g (b % NGROUPS == g).
__global__ __launch_bounds__(NT) void netGroupTotalsKernel(const uint32_t *__restrict__ blockHist, uint32_t F,
                                                           uint32_t blocks, unsigned long long *totals) {
  __shared__ unsigned long long gs[NGROUPS];
  const uint32_t d = blockIdx.x;
  if (threadIdx.x < NGROUPS) gs[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long mine = 0;  // NT % NGROUPS == 0: thread t only sees group t % NGROUPS
  for (uint32_t b = threadIdx.x; b < blocks; b += NT) mine += blockHist[(uint64_t)d * blocks + b];
  atomicAdd(&gs[threadIdx.x % NGROUPS], mine);
  __syncthreads();
  if (threadIdx.x < NGROUPS) totals[(uint64_t)threadIdx.x * F + d] = gs[threadIdx.x];
}

void netGroupTotals(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint64_t *totals, hipStream_t s) {
  hipLaunchKernelGGL(netGroupTotalsKernel, dim3(F), dim3(NT), 0, s, blockHist, F, blocks,
                     reinterpret_cast<unsigned long long *>(totals));
  HIP_CHECK_LAUNCH();
}

// True when key >> bits, shifted to keyShift, leaves `bits` spare top bits.
static bool digitFitsOnTop(uint32_t bits, uint32_t keyShift, uint32_t keyBits) {
  const uint32_t high = keyBits > bits ? keyBits - bits : 0;
  return keyShift + high + bits <= 64;
}

// The claim scatter runs 8192-tuple tiles (1024 threads x 8, CL_NTH x CL_IPT)
// with the early prefetch (earlyPrefetch: the next tile's loads overlap the
// scan and staging).  Measured alternatives, all retired: 16384-tuple tiles of
// 4-byte staged words (longer runs per partition and tile, but too many
// registers for the early prefetch: 1B x 1B 10.08 ms vs 9.56 with 8192 +
// early prefetch, same box, profiles/r5/README.md); 12288-tuple tiles (4.73 ->
// 5.14 ms, profiles/r6/README.md); 512-thread workgroups (docs/ROUND5.md).
// Only 1024 x 8 compiles without scratch for every policy.
// digits: claim slices per group (filtered range passes); else 2^bits.
template <class Pol>
static void launchNetClaim(const Pol &pol, const void *in, uint64_t n, uint32_t bits,
                           const PartitionGeometry &g, uint32_t blockBegin, uint32_t blockEnd, void *gcur,
                           void *out, hipStream_t s, const void *gend, bool narrow,
                           const uint32_t *roundMeta = nullptr, uint32_t digits = 0) {
  const uint32_t F = digits ? digits : 1u << bits;
  const auto *src = static_cast<const typename Pol::InT *>(in);
  auto *dst = reinterpret_cast<typename Pol::OutT *>(out);
  const dim3 grid(blockEnd - blockBegin);
  auto go = [&](auto cur, auto maxd) {
    using C = decltype(cur);
    constexpr int M = decltype(maxd)::value;
    const size_t lds = ScatterLayout<Pol, C, CL_NTH * CL_IPT>::bytes(F);
    HJ_CHECK(lds <= 160 * 1024, "scatter LDS %zu too large", lds);
    auto *gc = reinterpret_cast<C *>(gcur);
    if (gend)
      hipLaunchKernelGGL((netScatterClaimKernel<Pol, C, CL_NTH, CL_IPT, 0, true, M>), grid, dim3(CL_NTH), lds, s, src,
                         n, g.tilesPerBlock, F, pol, blockBegin, gc, dst, reinterpret_cast<const C *>(gend),
                         roundMeta);
    else if constexpr (!FilterOf<Pol>::value)  // filtered passes are bounded only (netScatterFragRange)
      hipLaunchKernelGGL((netScatterClaimKernel<Pol, C, CL_NTH, CL_IPT, 0, false, M>), grid, dim3(CL_NTH), lds, s,
                         src, n, g.tilesPerBlock, F, pol, blockBegin, gc, dst, nullptr, roundMeta);
  };
  withMaxd<CL_NTH>(F, [&](auto maxd) {
    if (narrow)
      go(uint32_t(), maxd);
    else
      go((unsigned long long)0, maxd);
  });
  HIP_CHECK_LAUNCH();
}

void scatterProfile(unsigned long long out[10], bool reset) {
  HIP_CHECK(hipDeviceSynchronize());
  for (int i = 0; i < 10; ++i) out[i] = 0;
  scatterProfileNet(out, reset);
  scatterProfileLocal(out, reset);
  scatterProfileAblation(out, reset);
}
void scatterProfileNet(unsigned long long acc[10], bool reset) { scatterProfileAdd(acc, reset); }

bool scatterProfileBuilt() {
#ifdef HPCJOIN_SCATTER_PROF
  return true;
#else
  return false;
#endif
}

// Argument checks shared by the netScatter* entry points; false = nothing to scatter.
static bool netScatterArgs(const char *who, uint64_t n, uint32_t bits, const PartitionGeometry &g,
                           uint32_t blockBegin, uint32_t blockEnd) {
  HJ_CHECK(bits >= 1 && bits <= MAX_PART_BITS, "%s: bits=%u out of range", who, bits);
  HJ_CHECK(blockBegin <= blockEnd && blockEnd <= g.blocks, "%s: block range [%u,%u) of %u", who, blockBegin, blockEnd,
           g.blocks);
  return n != 0 && blockEnd != blockBegin;
}

template <class Pol>
static void setDigits(Pol &pol, uint32_t bits, KeyMix mix) {
  pol.mask = (1ull << bits) - 1;
  pol.mix = mix;
  if constexpr (!std::is_same_v<Pol, NetWidePol>) pol.bits = bits;  // wide tuples keep the whole key
}

// Calls fn with the fragment policy of kb-bit (mixed) keys: the digit rides on
// top of the staged u32 when fragment + digit fit it, else in the tile's digit array.
// In: the input element (ulonglong2 tuples or a uint64_t key column).
template <bool FILT, typename In, class Fn>
static void withFragPol(uint32_t kb, KeyMix mix, Fn &&fn) {
  const bool digitOnTop = kb <= 32;
  if (mix.on && digitOnTop)
    fn(NetFragPolT<true, FILT, In>());
  else if (digitOnTop)
    fn(NetFragPolT<false, FILT, In>());
  else if (mix.on)
    fn(NetFragDigPolT<true, FILT, In>());
  else
    fn(NetFragDigPolT<false, FILT, In>());
}

void netScatter(KeySource in, uint64_t n, uint32_t bits, uint32_t keyShift, const PartitionGeometry &g,
                uint32_t blockBegin, uint32_t blockEnd, void *gcur, uint64_t *out, hipStream_t s, uint32_t keyBits,
                KeyMix mix, const void *gend, int narrowMode, bool withRids, const uint32_t *roundMeta) {
  const bool narrow = narrowMode < 0 ? cursorsNarrow(n) : narrowMode != 0;
  if (!netScatterArgs("netScatter", n, bits, g, blockBegin, blockEnd)) return;
  HJ_CHECK(withRids || keyShift == 0, "netScatter: key-only words need keyShift 0 (got %u)", keyShift);
  if (!withRids) {  // key >> bits always leaves `bits` spare top bits
    withKeyElements("netScatter", in, [&](auto *src) {
      using In = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
      auto go = [&](auto kpol) {
        setDigits(kpol, bits, mix);
        launchNetClaim(kpol, src, n, bits, g, blockBegin, blockEnd, gcur, out, s, gend, narrow, roundMeta);
      };
      if (mix.on)
        go(NetKeyPol<true, In>());
      else
        go(NetKeyPol<false, In>());
    });
    return;
  }
  HJ_CHECK(!in.isColumn(), "netScatter: CompressedTuples carry a rid; a key column has none to read");
  NetCompressedPol pol;
  setDigits(pol, bits, mix);
  pol.keyShift = keyShift;
  if (digitFitsOnTop(bits, keyShift, mix.on ? std::max(keyBits, mix.bits) : keyBits)) {
    launchNetClaim(pol, in.base, n, bits, g, blockBegin, blockEnd, gcur, out, s, gend, narrow, roundMeta);
  } else {
    NetCompressedDigPol dpol;
    static_cast<NetCompressedPol &>(dpol) = pol;
    launchNetClaim(dpol, in.base, n, bits, g, blockBegin, blockEnd, gcur, out, s, gend, narrow, roundMeta);
  }
}

void netScatterWide(const data::Tuple *in, uint64_t n, uint32_t bits, const PartitionGeometry &g,
                    uint32_t blockBegin, uint32_t blockEnd, void *gcur, data::Tuple *out, hipStream_t s,
                    KeyMix mix, const void *gend, int narrowMode) {
  const bool narrow = narrowMode < 0 ? cursorsNarrow(n) : narrowMode != 0;
  if (!netScatterArgs("netScatterWide", n, bits, g, blockBegin, blockEnd)) return;
  NetWidePol pol;
  setDigits(pol, bits, mix);
  launchNetClaim(pol, in, n, bits, g, blockBegin, blockEnd, gcur, out, s, gend, narrow);
}

void netScatterFrag(KeySource in, uint64_t n, uint32_t bits, const PartitionGeometry &g, uint32_t blockBegin,
                    uint32_t blockEnd, void *gcur, uint32_t *out, hipStream_t s, uint32_t keyBits, KeyMix mix,
                    const void *gend, int narrowMode, const uint32_t *roundMeta) {
  const bool narrow = narrowMode < 0 ? cursorsNarrow(n) : narrowMode != 0;
  const bool any = netScatterArgs("netScatterFrag", n, bits, g, blockBegin, blockEnd);
  const uint32_t kb = mix.on ? std::max(keyBits, mix.bits) : keyBits;
  HJ_CHECK(fragWordFits(kb, bits), "netScatterFrag: %u-bit keys leave a fragment wider than %u bits above %u radix bits",
           kb, 32 - bits, bits);
  if (!any) return;
  withKeyElements("netScatterFrag", in, [&](auto *src) {
    using In = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
    withFragPol<false, In>(kb, mix, [&](auto pol) {
      setDigits(pol, bits, mix);
      launchNetClaim(pol, src, n, bits, g, blockBegin, blockEnd, gcur, out, s, gend, narrow, roundMeta);
    });
  });
}

void netScatterFragPacked(KeySource in, uint64_t n, uint32_t bits, const PartitionGeometry &g, void *gcur,
                          uint64_t *out, hipStream_t s, KeyMix mix, const void *gend, bool narrow,
                          const uint32_t *roundMeta, unsigned long long *wideFlag) {
  const bool any = netScatterArgs("netScatterFragPacked", n, bits, g, 0, g.blocks);
  HJ_CHECK(bits <= PK_MAX_PART_BITS, "netScatterFragPacked: %u radix bits, the LDS carry holds 2^%u digits", bits,
           PK_MAX_PART_BITS);
  HJ_CHECK(gend && wideFlag, "netScatterFragPacked: bounded slices and a flag word are required");
  if (!any) return;
  const uint32_t F = 1u << bits;
  auto *dst = reinterpret_cast<unsigned long long *>(out);
  auto go = [&](auto mixed, auto cur) {
    using C = decltype(cur);
    constexpr bool MIX = decltype(mixed)::value;
    constexpr size_t lds = packedScatterLds<C>();
    static_assert(lds <= 160 * 1024, "packed scatter: LDS carve exceeds a CU");
    withKeyElements("netScatterFragPacked", in, [&](auto *src) {
      using In = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
      hipLaunchKernelGGL((netScatterFragPackedKernel<MIX, C, In>), dim3(g.blocks), dim3(CL_NTH), lds, s, src, n,
                         g.tilesPerBlock, F, bits, mix, reinterpret_cast<C *>(gcur), dst,
                         reinterpret_cast<const C *>(gend), roundMeta, wideFlag);
    });
  };
  auto width = [&](auto mixed) {
    if (narrow)
      go(mixed, uint32_t());
    else
      go(mixed, (unsigned long long)0);
  };
  if (mix.on)
    width(std::true_type());
  else
    width(std::false_type());
  HIP_CHECK_LAUNCH();
}

void netScatterFragRange(KeySource in, uint64_t n, uint32_t bits, const PartitionGeometry &g, void *gcur,
                         uint32_t *out, hipStream_t s, uint32_t keyBits, KeyMix mix, const void *gend, bool narrow,
                         uint32_t dLo, uint32_t range) {
  const bool any = netScatterArgs("netScatterFragRange", n, bits, g, 0, g.blocks);
  const uint32_t kb = mix.on ? std::max(keyBits, mix.bits) : keyBits;
  HJ_CHECK(fragWordFits(kb, bits), "netScatterFragRange: %u-bit keys above %u radix bits", kb, bits);
  // The sentinel digit `range` needs an LDS counter of its own: range < padDigits(range).
  HJ_CHECK(range >= 1 && range < padDigits(range) && dLo + range <= (1u << bits) && gend,
           "netScatterFragRange: digits [%u, %u) of %u (at most %u per pass, bounded slices)", dLo, dLo + range,
           1u << bits, padDigits(1) - 1);
  if (!any) return;
  withKeyElements("netScatterFragRange", in, [&](auto *src) {
    using In = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
    withFragPol<true, In>(kb, mix, [&](auto pol) {
      setDigits(pol, bits, mix);
      pol.dLo = dLo;
      pol.range = range;
      launchNetClaim(pol, src, n, bits, g, 0, g.blocks, gcur, out, s, gend, narrow, nullptr, range);
    });
  });
}

// ------------------------------------------------ device-side sampled layout
// Turns the sampled per-(XCD group, digit) counts into bounded claim slices
// on the device, so a sampled network pass needs no host round trip between
// its histogram and its scatter (the whole count-only join is then one
// stream of kernels with a single synchronisation at the end).  Entry
// j = d * G + g (partition-major, groups inside) is stored at i = g * F + d,
// the claim-cursor layout.  cap = roundup16(min(est + margin, total_g)),
// est = sampled * total_g / seen_g, margin = sigmas * sqrt(max(est, 1) *
// total_g / seen_g) + frac * est + floor (sigmas = frac = floor = 0 with an
// exact histogram: the slices are then exactly the counts, rounded to lines).
constexpr int LAY_NT = 1024;
template <typename CurT>
struct LayoutSideArgs {
  const unsigned long long *sampled;
  SampleScale sc;
  CurT *gstart, *gcur, *gend;
  unsigned long long *capacityUsed;
  unsigned long long *clear;  // = sampled when it is DeviceControl scratch, else nullptr
  uint32_t *roundMeta;        // LayoutInput::roundMeta
  uint32_t roundLp, roundMaxLv;
  unsigned long long roundCapacity;
  uint32_t packDiv, packTail;  // LayoutInput::packed: fragments per word (else 1), tail words per slice
};

// Workgroup i lays out side i (one or two sides per launch).
// Digits [dLo, dLo + F) of totals laid out as [G][Fsrc] (a partition-group
// pass lays out its range only; F = Fsrc, dLo = 0 otherwise).
template <typename CurT>
__global__ __launch_bounds__(LAY_NT) void netSampledLayoutKernel(LayoutSideArgs<CurT> s0, LayoutSideArgs<CurT> s1,
                                                                  uint32_t F, uint32_t Fsrc, uint32_t dLo) {
  const LayoutSideArgs<CurT> &ls = blockIdx.x ? s1 : s0;
  const unsigned long long *__restrict__ sampled = ls.sampled;
  const SampleScale &sc = ls.sc;
  CurT *__restrict__ gstart = ls.gstart;
  CurT *__restrict__ gcur = ls.gcur;
  CurT *__restrict__ gend = ls.gend;
  unsigned long long *__restrict__ capacityUsed = ls.capacityUsed;
  __shared__ unsigned long long wt[LAY_NT / WAVE];
  __shared__ unsigned long long maxCapS;
  constexpr uint32_t G = NGROUPS;
  const uint32_t n = F * G;
  const uint32_t per = (n + LAY_NT - 1) / LAY_NT, t = threadIdx.x;
  const uint32_t j0 = t * per;
  constexpr int MAXPER = ((1u << MAX_PART_BITS) * NGROUPS + LAY_NT - 1) / LAY_NT;
  unsigned long long cap[MAXPER];
  unsigned long long local = 0;
#pragma unroll
  for (int k = 0; k < MAXPER; ++k) {
    cap[k] = 0;
    const uint32_t j = j0 + k;
    if (k < (int)per && j < n) {
      const uint32_t d = j / G, g = j % G;
      const double seen = sc.seen[g], total = sc.total[g];
      double c = 0;
      if (seen > 0) {
        const double scale = total / seen;
        const double est = (double)sampled[(size_t)g * Fsrc + dLo + d] * scale;
        // sigma of a count scaled by `scale` from k samples: scale * sqrt(k);
        // at least one sample's worth (k = 0 says little about a cell).
        const double margin = sc.sigmas * sqrt(fmax(est, scale) * scale) + sc.frac * est + sc.floor;
        c = fmin(ceil(est + margin), total);
      }
      if (ls.clear) ls.clear[(size_t)g * Fsrc + dLo + d] = 0;  // read once (above), by this thread
      // Packed windows count words: ceil(fragments / 3), plus the workgroups' tail chunks.
      const unsigned long long slots = ((unsigned long long)c + ls.packDiv - 1) / ls.packDiv;
      cap[k] = ((slots + 15ull) & ~15ull) + ls.packTail;
      local += cap[k];
    }
  }
  // Round-interleaved slices (RoundMap) when the largest slice allows them.
  uint32_t lv = 0, lns = 0;
  unsigned long long roundUsed = 0;
  if (ls.roundMeta) {  // uniform per workgroup
    if (t == 0) maxCapS = 0;
    __syncthreads();
    unsigned long long m = 0;
#pragma unroll
    for (int k = 0; k < MAXPER; ++k) m = cap[k] > m ? cap[k] : m;
    atomicMax(&maxCapS, m);
    __syncthreads();
    const unsigned long long maxCap = maxCapS;
    while ((1u << lns) < n) ++lns;
    uint32_t v = ls.roundLp;
    while ((1ull << v) < maxCap) ++v;
    roundUsed = roundSlots(maxCap, ls.roundLp, lns);
    if ((1u << lns) == n && v <= ls.roundMaxLv && roundUsed <= ls.roundCapacity) lv = v;
    if (t == 0) {
      ls.roundMeta[0] = lv ? ls.roundLp : 0;
      ls.roundMeta[1] = lv;
      ls.roundMeta[2] = lv ? lns : 0;
      ls.roundMeta[3] = 0;
    }
  }
  const unsigned long long incl = waveInclusiveScan<unsigned long long>(local);
  const int lane = t & (WAVE - 1), wid = t / WAVE;
  if (lane == WAVE - 1) wt[wid] = incl;
  __syncthreads();
  unsigned long long run = incl - local;
  for (int w = 0; w < wid; ++w) run += wt[w];
#pragma unroll
  for (int k = 0; k < MAXPER; ++k) {
    const uint32_t j = j0 + k;
    if (k < (int)per && j < n) {
      const uint32_t i = (j % G) * F + j / G;
      const unsigned long long b = lv ? (unsigned long long)i << lv : run;
      gstart[i] = (CurT)b;
      gcur[i] = (CurT)b;
      gend[i] = (CurT)(b + cap[k]);
      run += cap[k];
    }
  }
  if (t == LAY_NT - 1) *capacityUsed = lv ? roundUsed : run;
}

template <typename CurT>
static LayoutSideArgs<CurT> layoutSide(const LayoutInput &x) {
  auto *sampled = reinterpret_cast<const unsigned long long *>(x.sampled);
  return LayoutSideArgs<CurT>{sampled, x.sc,
                              static_cast<CurT *>(x.gstart), static_cast<CurT *>(x.gcur), static_cast<CurT *>(x.gend),
                              x.capacityUsed,
                              x.clearSampled ? const_cast<unsigned long long *>(sampled) : nullptr,
                              x.roundMeta, x.roundLp, x.roundMaxLv, (unsigned long long)x.roundCapacity,
                              x.packed ? PK_WORD_FRAGS : 1u, x.packed ? x.packedTail : 0u};
}

void netSampledLayout(const LayoutInput *sides, uint32_t count, uint32_t F, bool narrow, hipStream_t s, uint32_t dLo,
                      uint32_t range) {
  HJ_CHECK(F >= 1 && F <= (1u << MAX_PART_BITS), "netSampledLayout: F=%u", F);
  HJ_CHECK(count == 1 || count == 2, "netSampledLayout: %u sides", count);
  const uint32_t R = range ? range : F;
  HJ_CHECK(dLo + R <= F, "netSampledLayout: digits [%u, %u) of %u", dLo, dLo + R, F);
  for (uint32_t k = 0; k < count; ++k)
    HJ_CHECK(!sides[k].roundMeta || (range == 0 && sides[k].roundLp >= 1 && sides[k].roundLp <= 16),
             "netSampledLayout: round slices need a whole-range layout and 1 <= lp <= 16 (lp %u, range %u)",
             sides[k].roundLp, range);
  const LayoutInput &b = sides[count - 1];
  if (narrow)
    hipLaunchKernelGGL(netSampledLayoutKernel<uint32_t>, dim3(count), dim3(LAY_NT), 0, s,
                       layoutSide<uint32_t>(sides[0]), layoutSide<uint32_t>(b), R, F, dLo);
  else
    hipLaunchKernelGGL(netSampledLayoutKernel<unsigned long long>, dim3(count), dim3(LAY_NT), 0, s,
                       layoutSide<unsigned long long>(sides[0]), layoutSide<unsigned long long>(b), R, F, dLo);
  HIP_CHECK_LAUNCH();
}

void netSampledLayout(const uint64_t *sampled, uint32_t F, const SampleScale &sc, void *gstart, void *gcur, void *gend,
                      bool narrow, unsigned long long *capacityUsed, hipStream_t s) {
  const LayoutInput one{sampled, sc, gstart, gcur, gend, capacityUsed};
  netSampledLayout(&one, 1, F, narrow, s);
}

SampleScale sampleScale(const PartitionGeometry &g, uint64_t n, uint32_t sampleStride, bool exact) {
  SampleScale sc{};
  const uint64_t span = (uint64_t)g.tilesPerBlock * PART_TILE;
  for (uint32_t b = 0; b < g.blocks; ++b) {
    const uint64_t begin = (uint64_t)b * span, end = std::min(n, begin + span);
    if (begin < end) sc.total[b % NGROUPS] += (double)(end - begin);
  }
  // The tiles netSampledTotals reads (every tile when sampleStride == 1).
  for (uint32_t gr = 0; gr < NGROUPS; ++gr) {
    const uint64_t tiles = groupTiles(g, n, gr);
    for (uint64_t local = 0; local < tiles; local += sampleStride) {
      const uint64_t begin = sampledTile(local, gr, g.tilesPerBlock) * PART_TILE;
      if (begin < n) sc.seen[gr] += (double)std::min<uint64_t>(PART_TILE, n - begin);
    }
  }
  if (exact) {
    sc.sigmas = sc.frac = sc.floor = 0;
  } else {  // 6 sigma + 2% + 256 (tasks/SampledNetworkPartitioning.cpp, same statistics)
    sc.sigmas = 6.0;
    sc.frac = 0.02;
    sc.floor = 256.0;
  }
  return sc;
}

uint64_t sampledWindowCapacity(const SampleScale &sc, uint32_t F, uint32_t roundLp) {
  const uint64_t bound = sampledLayoutCapacityBound(sc, F);
  if (!roundLp) return bound;
  double maxCap = 0;
  for (uint32_t g = 0; g < NGROUPS; ++g) {
    if (sc.total[g] <= 0) continue;
    const double scale = sc.seen[g] > 0 ? sc.total[g] / sc.seen[g] : 1.0;
    // The largest slice: its sampled estimate up to 5 sigma above the mean,
    // plus the layout kernel's margin taken at that estimate.
    const double mean = sc.total[g] / F;
    const double hi = mean + 5.0 * std::sqrt(std::max(mean, scale) * scale);
    maxCap = std::max(maxCap, hi + sc.sigmas * std::sqrt(std::max(hi, scale) * scale) + sc.frac * hi + sc.floor + 16.0);
  }
  uint32_t lns = 0;
  while ((1u << lns) < NGROUPS * F) ++lns;
  return std::max<uint64_t>(bound, roundSlots((uint64_t)std::ceil(maxCap), roundLp, lns));
}

uint64_t sampledPackedWindowCapacity(const SampleScale &sc, uint32_t F, uint32_t roundLp, uint32_t tailWords) {
  // Per slice: ceil(c / 3) rounded up to 16 words, plus the tail chunks.
  const uint64_t perSlice = 17 + tailWords;
  const uint64_t bound = sampledLayoutCapacityBound(sc, F) / PK_WORD_FRAGS + perSlice * NGROUPS * F + 4096;
  if (!roundLp) return bound;
  double maxCap = 0;  // the largest slice's fragments, as sampledWindowCapacity
  for (uint32_t g = 0; g < NGROUPS; ++g) {
    if (sc.total[g] <= 0) continue;
    const double scale = sc.seen[g] > 0 ? sc.total[g] / sc.seen[g] : 1.0;
    const double mean = sc.total[g] / F;
    const double hi = mean + 5.0 * std::sqrt(std::max(mean, scale) * scale);
    maxCap = std::max(maxCap, hi + sc.sigmas * std::sqrt(std::max(hi, scale) * scale) + sc.frac * hi + sc.floor + 16.0);
  }
  uint32_t lns = 0;
  while ((1u << lns) < NGROUPS * F) ++lns;
  const uint64_t maxWords = (uint64_t)std::ceil(maxCap) / PK_WORD_FRAGS + perSlice;
  return std::max<uint64_t>(bound, roundSlots(maxWords, roundLp, lns));
}

uint64_t sampledLayoutCapacityBound(const SampleScale &sc, uint32_t F) {
  // Per group: sum_d est_d = total_g; sum_d sqrt(max(est_d,scale) * scale) <=
  // sqrt(F * scale * (total_g + F * scale)) (Cauchy-Schwarz); + ceil and the 16-tuple
  // line rounding per slice.
  double b = 0;
  for (uint32_t g = 0; g < NGROUPS; ++g) {
    if (sc.total[g] <= 0) continue;
    const double scale = sc.seen[g] > 0 ? sc.total[g] / sc.seen[g] : 1.0;
    b += (1.0 + sc.frac) * sc.total[g] + sc.sigmas * std::sqrt((double)F * scale * (sc.total[g] + F * scale)) +
         (sc.floor + 17.0) * F;
  }
  return (uint64_t)(b * 1.0001) + 4096;
}

// Loads this file's code object at engine start (kernels::preloadCodeObjects).
void preloadNetPartition() {
  hipFuncAttributes a;
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&netHistogramKernel<ulonglong2>)));
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&netScatterFragPackedKernel<false, uint32_t>)));
}

}  // namespace kernels
}  // namespace hpcjoin
