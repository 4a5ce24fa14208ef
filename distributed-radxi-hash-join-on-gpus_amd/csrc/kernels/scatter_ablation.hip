// Scatter ablation matrix (tools/microbench.py, tools/round_probe.py): the
// network scatter of scatter_core.h over mode x workgroup geometry, with
// per-workgroup cursors or claim slices, and the per-tuple global-atomic
// baseline.  A benchmark, not a join path: joins launch only the production
// geometry (net_partition.hip, local_partition.hip).
#include "scatter_core.h"

namespace hpcjoin {
namespace kernels {

// Per-workgroup cursors (ablation baseline): F <= NTH * MAXD digits, no claims.
template <class Pol, typename CurT, int NTH, int IPT, int MODE>
__global__ __launch_bounds__(NTH, ScatterOcc<NTH>::value) void netScatterKernel(
    const typename Pol::InT *__restrict__ in, uint64_t n, uint32_t tpb, uint32_t F, Pol pol, uint32_t totalBlocks,
    uint32_t blockBegin, const uint64_t *__restrict__ cursors, typename Pol::OutT *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t blk = blockBegin + blockIdx.x;
  const uint32_t FP = padDigits(F);
  CurT *cursor = reinterpret_cast<CurT *>(smem);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(cursor + 2 * FP);
  for (uint32_t d = threadIdx.x; d < FP; d += NTH) {
    if (d < F) cursor[d] = (CurT)cursors[(uint64_t)d * totalBlocks + blk];
    cnt[d] = 0;
  }
  __syncthreads();
  const uint64_t begin = (uint64_t)blk * tpb * PART_TILE;  // geometry is in PART_TILE units
  const uint64_t end = min(n, begin + (uint64_t)tpb * PART_TILE);
  scatterRange<Pol, CurT, NTH, IPT, MODE>(in, begin, end, F, smem, pol, out);
}

// Default geometry (measured on MI355X, tools/microbench.py ablation).
constexpr int SC_NTH = 256;
constexpr int SC_IPT = 16;

template <class Pol, typename CurT, int NTH = SC_NTH, int IPT = SC_IPT, int MODE = 0>
static void launchNet(const Pol &pol, const data::Tuple *in, uint64_t n, uint32_t bits, const PartitionGeometry &g,
                      uint32_t blockBegin, uint32_t blockEnd, const uint64_t *cursors, void *out, hipStream_t s) {
  const uint32_t F = 1u << bits;
  const size_t lds = ScatterLayout<Pol, CurT, NTH * IPT>::bytes(F);
  HJ_CHECK(lds <= 160 * 1024, "scatter LDS %zu too large", lds);
  hipLaunchKernelGGL((netScatterKernel<Pol, CurT, NTH, IPT, MODE>), dim3(blockEnd - blockBegin), dim3(NTH), lds, s,
                     reinterpret_cast<const typename Pol::InT *>(in), n, g.tilesPerBlock, F, pol, g.blocks,
                     blockBegin, cursors, reinterpret_cast<typename Pol::OutT *>(out));
  HIP_CHECK_LAUNCH();
}

// Per-workgroup cursors at NTH x IPT: mode 0 real, 1 coalesced write-out, 2 none.
template <int NTH, int IPT, class P>
static void ablationCursors(const P &p, const data::Tuple *in, uint64_t n, uint32_t bits, const PartitionGeometry &g,
                            const uint64_t *cursors, uint64_t *out, int mode, hipStream_t s) {
  if (mode == 1)
    launchNet<P, uint32_t, NTH, IPT, 1>(p, in, n, bits, g, 0, g.blocks, cursors, out, s);
  else if (mode == 2)
    launchNet<P, uint32_t, NTH, IPT, 2>(p, in, n, bits, g, 0, g.blocks, cursors, out, s);
  else
    launchNet<P, uint32_t, NTH, IPT, 0>(p, in, n, bits, g, 0, g.blocks, cursors, out, s);
}

// Claim mode at NTH x IPT (u32 group cursors): mode 1 coalesced write-out,
// 3 real scatter into round-interleaved slices, else real scatter.
template <int NTH, int IPT>
static void ablationClaim(const NetCompressedPol &pol, const data::Tuple *in, uint64_t n, uint32_t bits,
                          const PartitionGeometry &g, void *gcur, uint64_t *out, int mode, const uint32_t *roundMeta,
                          hipStream_t s) {
  const uint32_t F = 1u << bits;
  withMaxd<NTH>(F, [&](auto maxd) {
    constexpr int M = decltype(maxd)::value;
    const size_t lds = ScatterLayout<NetCompressedPol, uint32_t, NTH * IPT>::bytes(F);
    const auto *src = reinterpret_cast<const ulonglong2 *>(in);
    auto *gc = reinterpret_cast<uint32_t *>(gcur);
    if (mode == 1)
      hipLaunchKernelGGL((netScatterClaimKernel<NetCompressedPol, uint32_t, NTH, IPT, 1, false, M>), dim3(g.blocks),
                         dim3(NTH), lds, s, src, n, g.tilesPerBlock, F, pol, 0u, gc, out);
    else
      hipLaunchKernelGGL((netScatterClaimKernel<NetCompressedPol, uint32_t, NTH, IPT, 0, false, M>), dim3(g.blocks),
                         dim3(NTH), lds, s, src, n, g.tilesPerBlock, F, pol, 0u, gc, out, nullptr,
                         mode == 3 ? roundMeta : nullptr);
  });
}

// The count-only fragment scatter at 1024 x 16 in mode MODE.
template <int MODE>
static void ablationFrag(const NetFragPol &fpol, const data::Tuple *in, uint64_t n, uint32_t bits,
                         const PartitionGeometry &g, void *gcur, uint64_t *out, hipStream_t s) {
  const uint32_t F = 1u << bits;
  const size_t lds = ScatterLayout<NetFragPol, uint32_t, 1024 * 16>::bytes(F);
  withMaxd<1024>(F, [&](auto maxd) {
    hipLaunchKernelGGL((netScatterClaimKernel<NetFragPol, uint32_t, 1024, 16, MODE, false, decltype(maxd)::value>),
                       dim3(g.blocks), dim3(1024), lds, s, reinterpret_cast<const ulonglong2 *>(in), n,
                       g.tilesPerBlock, F, fpol, 0u, reinterpret_cast<uint32_t *>(gcur),
                       reinterpret_cast<uint32_t *>(out));
  });
}

void scatterAblation(const data::Tuple *in, uint64_t n, uint32_t bits, uint32_t keyShift, const PartitionGeometry &g,
                     const uint64_t *cursors, uint64_t *out, int mode, int geometry, hipStream_t s, void *gcur,
                     const uint32_t *roundMeta) {
  NetCompressedPol pol;
  pol.mask = (1ull << bits) - 1;
  pol.bits = bits;
  pol.keyShift = keyShift;
  NetCompressedDigPol dpol;
  static_cast<NetCompressedPol &>(dpol) = pol;
  // 10: the count-only fragment scatter of the bitmap plan (4-byte output,
  // 1024 x 16 tiles): mode 0 real, 1 coalesced write-out, 2 no write-out.
  // Measured at 1B tuples, bits 8/9/10/11: 4.18/4.30/4.45/4.70 ms real against
  // ~3.87 coalesced and ~2.6 without writes (streaming ceiling of the byte mix
  // 3.47 ms, tools/stream_mix_bench.py): the scatter pays for runs of ~16
  // fragments per partition and tile.  Key-only loads with 24-key tiles
  // (longer runs) spilled and ran 4.56 ms at bits 10; key-only loads through a
  // buffer resource with two register tiles (the next tile's loads issued
  // before this one is ranked) ran 2 % slower in the 1B join (network pass
  // 8.78 vs 8.60 ms): the pass is bound by the scattered writes, not by load
  // latency.
  HJ_CHECK(mode != 3 || (geometry >= 6 && geometry <= 9 && roundMeta), "scatterAblation: mode 3 needs a claim geometry");
  if (geometry == 10) {
    NetFragPol fpol;
    fpol.mask = (1ull << bits) - 1;
    fpol.bits = bits;
    if (mode == 1)
      ablationFrag<1>(fpol, in, n, bits, g, gcur, out, s);
    else if (mode == 2)
      ablationFrag<2>(fpol, in, n, bits, g, gcur, out, s);
    else
      ablationFrag<0>(fpol, in, n, bits, g, gcur, out, s);
    HIP_CHECK_LAUNCH();
    return;
  }
  switch (geometry) {
    case 1: ablationCursors<512, 16>(pol, in, n, bits, g, cursors, out, mode, s); break;
    case 2: ablationCursors<1024, 8>(pol, in, n, bits, g, cursors, out, mode, s); break;
    case 3: ablationCursors<1024, 16>(pol, in, n, bits, g, cursors, out, mode, s); break;
    case 4: ablationCursors<256, 16>(dpol, in, n, bits, g, cursors, out, mode, s); break;
    case 5: ablationCursors<256, 8>(pol, in, n, bits, g, cursors, out, mode, s); break;
    case 6: ablationClaim<256, 16>(pol, in, n, bits, g, gcur, out, mode, roundMeta, s); break;
    case 7: ablationClaim<512, 16>(pol, in, n, bits, g, gcur, out, mode, roundMeta, s); break;
    case 8: ablationClaim<1024, 16>(pol, in, n, bits, g, gcur, out, mode, roundMeta, s); break;
    case 9: ablationClaim<1024, 8>(pol, in, n, bits, g, gcur, out, mode, roundMeta, s); break;
    default: ablationCursors<SC_NTH, SC_IPT>(pol, in, n, bits, g, cursors, out, mode, s); break;
  }
}

// Ablation: per-tuple global atomics on a per-digit cursor (no LDS staging).
__global__ __launch_bounds__(NT) void netScatterGlobalAtomicKernel(const ulonglong2 *__restrict__ in, uint64_t n,
                                                                   uint32_t bits, uint32_t keyShift,
                                                                   unsigned long long *cursor, uint64_t *out) {
  const uint64_t mask = (1ull << bits) - 1;
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) {
    const ulonglong2 x = in[i];
    const unsigned long long pos = atomicAdd(&cursor[x.x & mask], 1ull);
    out[pos] = x.y | ((x.x >> bits) << keyShift);
  }
}

void netScatterGlobalAtomic(const data::Tuple *in, uint64_t n, uint32_t bits, uint32_t keyShift,
                            uint64_t *digitCursor, uint64_t *out, hipStream_t s) {
  if (n == 0) return;
  const uint64_t want = ceilDiv(n, NT);
  const uint32_t blocks = (uint32_t)(want < 4096 ? want : 4096);
  hipLaunchKernelGGL(netScatterGlobalAtomicKernel, dim3(blocks), dim3(NT), 0, s,
                     reinterpret_cast<const ulonglong2 *>(in), n, bits, keyShift,
                     reinterpret_cast<unsigned long long *>(digitCursor), out);
  HIP_CHECK_LAUNCH();
}

void scatterProfileAblation(unsigned long long acc[10], bool reset) { scatterProfileAdd(acc, reset); }

// Loads this file's code object at engine start (kernels::preloadCodeObjects).
void preloadScatterAblation() {
  hipFuncAttributes a;
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&netScatterGlobalAtomicKernel)));
}

}  // namespace kernels
}  // namespace hpcjoin
