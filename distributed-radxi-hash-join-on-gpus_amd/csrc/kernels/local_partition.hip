// Pass 2 (local partitioning) for MI355X (gfx950): replaces the reference's
// tasks/LocalPartitioning.cpp:138-250.  Item histograms and
// cursors (exact or sampled layout), then the persistent claim scatter over
// the work items (scatter_core.h).
#include "scatter_core.h"

#include <algorithm>
#include <cstdlib>
#include <cmath>

namespace hpcjoin {
namespace kernels {

// ------------------------------------------------------ pass 2 (local) kernels
// KIND: 0 = 8-byte CompressedTuple / key-only word, 1 = 16-byte tuple (its
// key), 2 = u32 key fragment (JoinPlan::fragments).
template <int KIND>
__device__ __forceinline__ uint64_t localWord(const void *in, uint64_t i) {
  if constexpr (KIND == 1)
    return reinterpret_cast<const ulonglong2 *>(in)[i].x;
  else if constexpr (KIND == 2)
    return reinterpret_cast<const uint32_t *>(in)[i];
  else
    return reinterpret_cast<const uint64_t *>(in)[i];
}

template <int WIDE>
__global__ __launch_bounds__(NT) void localHistogramKernel(const void *__restrict__ in,
                                                           const LocalItem *__restrict__ items, uint32_t shift,
                                                           uint32_t bits, uint32_t *__restrict__ itemHist,
                                                           uint32_t stride, RoundMap rm) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hsh[];
  const uint32_t F = 1u << bits;
  const uint64_t mask = F - 1;
  const int wid = threadIdx.x / WAVE;
  for (uint32_t i = threadIdx.x; i < 4 * F; i += NT) hsh[i] = 0;
  __syncthreads();
  const LocalItem it = items[blockIdx.x];
  uint32_t *wh = hsh + wid * F;
  for (uint32_t base = 0; base < it.len; base += PART_TILE * stride) {
    uint64_t w[PART_ITEMS];
#pragma unroll
    for (int i = 0; i < (int)PART_ITEMS; ++i) {
      const uint32_t idx = base + i * NT + threadIdx.x;
      w[i] = idx < it.len ? localWord<WIDE>(in, rm(it.begin + idx)) : 0;
    }
#pragma unroll
    for (int i = 0; i < (int)PART_ITEMS; ++i) {
      const uint32_t idx = base + i * NT + threadIdx.x;
      if (idx < it.len) atomicAdd(&wh[(w[i] >> shift) & mask], 1u);
    }
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < F; d += NT)
    itemHist[(uint64_t)blockIdx.x * F + d] = hsh[d] + hsh[F + d] + hsh[2 * F + d] + hsh[3 * F + d];
}

// 8-byte words whose digit lies inside one 32-bit half (HALF 0 = low word,
// 1 = high word; shift is then relative to that half): every thread loads
// only that half, and both of a batch's two sampled tiles are in flight
// before the first is counted (an item of the 1B x 1B general path holds two
// sampled tiles: one HBM round trip instead of two).
template <int HALF>
__global__ __launch_bounds__(NT) void localHistogramHalfKernel(const uint32_t *__restrict__ in,
                                                               const LocalItem *__restrict__ items, uint32_t shift,
                                                               uint32_t bits, uint32_t *__restrict__ itemHist,
                                                               uint32_t stride, RoundMap rm) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hsh[];
  const uint32_t F = 1u << bits, mask = F - 1;
  const int wid = threadIdx.x / WAVE;
  for (uint32_t i = threadIdx.x; i < 4 * F; i += NT) hsh[i] = 0;
  __syncthreads();
  const LocalItem it = items[blockIdx.x];
  uint32_t *wh = hsh + wid * F;
  const uint32_t step = PART_TILE * stride;
  for (uint32_t base = 0; base < it.len; base += 2 * step) {
    uint32_t w[2][PART_ITEMS];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < (int)PART_ITEMS; ++i) {
        const uint32_t idx = base + t * step + i * NT + threadIdx.x;
        w[t][i] = idx < it.len ? __builtin_nontemporal_load(in + 2 * rm(it.begin + idx) + HALF) : 0u;
      }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < (int)PART_ITEMS; ++i) {
        const uint32_t idx = base + t * step + i * NT + threadIdx.x;
        if (idx < it.len) atomicAdd(&wh[(w[t][i] >> shift) & mask], 1u);
      }
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < F; d += NT)
    itemHist[(uint64_t)blockIdx.x * F + d] = hsh[d] + hsh[F + d] + hsh[2 * F + d] + hsh[3 * F + d];
}

void localHistogram(const void *in, bool wide, const LocalItem *items, uint32_t nItems, uint32_t shift,
                    uint32_t bits, uint32_t *itemHist, hipStream_t s, uint32_t sampleStride, bool frag, RoundMap rm) {
  HJ_CHECK(bits <= MAX_PART_BITS, "localHistogram: bits=%u out of range", bits);
  HJ_CHECK(sampleStride >= 1, "localHistogram: sampleStride must be >= 1");
  HJ_CHECK(!(wide && frag), "localHistogram: fragments are not wide tuples");
  if (nItems == 0) return;
  const size_t lds = size_t(4) << bits << 2;
  const char *hv = std::getenv("HPCJOIN_LH_HALF");  // "0": the whole-word kernel (A/B)
  if (!wide && !frag && (shift + bits <= 32 || shift >= 32) && !(hv && hv[0] == '0')) {
    const auto *w = static_cast<const uint32_t *>(in);
    if (shift >= 32)
      hipLaunchKernelGGL(localHistogramHalfKernel<1>, dim3(nItems), dim3(NT), lds, s, w, items, shift - 32, bits,
                         itemHist, sampleStride, rm);
    else
      hipLaunchKernelGGL(localHistogramHalfKernel<0>, dim3(nItems), dim3(NT), lds, s, w, items, shift, bits,
                         itemHist, sampleStride, rm);
  } else if (frag)
    hipLaunchKernelGGL(localHistogramKernel<2>, dim3(nItems), dim3(NT), lds, s, in, items, shift, bits, itemHist,
                       sampleStride, rm);
  else if (wide)
    hipLaunchKernelGGL(localHistogramKernel<1>, dim3(nItems), dim3(NT), lds, s, in, items, shift, bits, itemHist,
                       sampleStride, rm);
  else
    hipLaunchKernelGGL(localHistogramKernel<0>, dim3(nItems), dim3(NT), lds, s, in, items, shift, bits, itemHist,
                       sampleStride, rm);
  HIP_CHECK_LAUNCH();
}

uint32_t assignLocalStreams(LocalItem *items, uint32_t nItems) {
  // Block b of the local scatter runs item (b % NGROUPS) * q + b / NGROUPS, so
  // the items of group g = item / q are one contiguous run of the (lp-sorted)
  // list and share an XCD; a stream = one (lp, group) run.
  const uint32_t q = (nItems + NGROUPS - 1) / NGROUPS;
  uint32_t streams = 0, prevLp = ~0u, prevG = ~0u;
  for (uint32_t i = 0; i < nItems; ++i) {
    const uint32_t g = i / (q ? q : 1);
    if (items[i].lp != prevLp || g != prevG) {
      ++streams;
      prevLp = items[i].lp;
      prevG = g;
    }
    items[i].stream = streams - 1;
  }
  return streams;
}

// One workgroup per owned partition lp: turns the [item][F] histograms of its
// items into the start of every (stream, sub-partition) claim slice and the
// final partition begin offsets partBegin[lp*F + q].
template <typename CurT>
__global__ __launch_bounds__(NT) void localCursorsKernel(const uint32_t *__restrict__ itemHist,
                                                         const uint32_t *__restrict__ lpItemBegin, uint32_t owned,
                                                         uint32_t bits, const uint64_t *__restrict__ lpBase,
                                                         const LocalItem *__restrict__ items, CurT *__restrict__ gcur,
                                                         uint64_t *__restrict__ partBegin) {
  extern __shared__ __attribute__((aligned(16))) uint64_t csh[];
  const uint32_t F = 1u << bits;
  uint64_t *tot = csh;     // [F]
  uint64_t *wt = csh + F;  // [NT/64]
  const uint32_t lp = blockIdx.x;
  const uint32_t ib = lpItemBegin[lp], ie = lpItemBegin[lp + 1];
  for (uint32_t q = threadIdx.x; q < F; q += NT) {
    uint64_t s = 0;
    for (uint32_t it = ib; it < ie; ++it) s += itemHist[(uint64_t)it * F + q];
    tot[q] = s;
  }
  __syncthreads();
  blockExclusiveScanLds<NT, uint64_t, uint64_t>(tot, tot, (int)F, wt);
  const uint64_t base = lpBase[lp];
  for (uint32_t q = threadIdx.x; q < F; q += NT) {
    uint64_t run = base + tot[q];
    partBegin[(uint64_t)lp * F + q] = run;
    uint32_t prev = ~0u;
    for (uint32_t it = ib; it < ie; ++it) {
      const uint32_t st = items[it].stream;
      if (st != prev) {
        gcur[(uint64_t)st * F + q] = (CurT)run;
        prev = st;
      }
      run += itemHist[(uint64_t)it * F + q];
    }
  }
  if (lp == owned - 1 && threadIdx.x == 0) partBegin[(uint64_t)owned * F] = lpBase[owned];
}

void localCursors(const uint32_t *itemHist, const uint32_t *lpItemBegin, uint32_t owned, uint32_t bits,
                  const uint64_t *lpBase, const LocalItem *items, void *gcur, bool narrow, uint64_t *partBegin,
                  hipStream_t s) {
  if (owned == 0) return;
  const size_t lds = (size_t(1) << bits) * 8 + 64;
  if (narrow)
    hipLaunchKernelGGL(localCursorsKernel<uint32_t>, dim3(owned), dim3(NT), lds, s, itemHist, lpItemBegin, owned, bits,
                       lpBase, items, reinterpret_cast<uint32_t *>(gcur), partBegin);
  else
    hipLaunchKernelGGL(localCursorsKernel<unsigned long long>, dim3(owned), dim3(NT), lds, s, itemHist, lpItemBegin,
                       owned, bits, lpBase, items, reinterpret_cast<unsigned long long *>(gcur), partBegin);
  HIP_CHECK_LAUNCH();
}

// Sampled local pass: tuples of item it the histogram read (tiles 0, S, 2S...).
__device__ __forceinline__ uint32_t sampledLen(uint32_t len, uint32_t stride) {
  uint32_t seen = 0;
  for (uint32_t b = 0; b < len; b += PART_TILE * stride) seen += min((uint32_t)PART_TILE, len - b);
  return seen;
}

// One workgroup per owned partition lp: capacity of each final partition
// (lp, q) = sampled estimate + LOCAL_SIGMAS sigma of the sampling error + 2% + 64.
// With ~240 sampled tuples per final partition (1 tile in 16), a low sample
// shrinks both the estimate and its margin: at 6 sigma a slot overflows with
// probability ~1e-7 (Poisson lower tail), i.e. a few percent of 1B x 1B joins
// (2^19 slots) would take the exact re-run; at 8 sigma ~1e-11.  The price is
// memory only (gaps are never read): ~+15% of the local output allocation.
constexpr double LOCAL_SIGMAS = 8.0;
__global__ __launch_bounds__(NT) void localCapacityKernel(const uint32_t *__restrict__ itemHist,
                                                          const uint32_t *__restrict__ lpItemBegin,
                                                          const LocalItem *__restrict__ items, uint32_t bits,
                                                          uint32_t stride, uint32_t align, uint32_t *__restrict__ caps) {
  const uint32_t F = 1u << bits, lp = blockIdx.x;
  const uint32_t ib = lpItemBegin[lp], ie = lpItemBegin[lp + 1];
  double len = 0, seen = 0;
  for (uint32_t it = ib; it < ie; ++it) {
    len += items[it].len;
    seen += sampledLen(items[it].len, stride);
  }
  const double scale = seen > 0 ? len / seen : 1.0;
  for (uint32_t q = threadIdx.x; q < F; q += NT) {
    double est = 0;
    for (uint32_t it = ib; it < ie; ++it) {
      const uint32_t s = sampledLen(items[it].len, stride);
      if (s) est += (double)itemHist[(uint64_t)it * F + q] * ((double)items[it].len / s);
    }
    const double cap = est + LOCAL_SIGMAS * sqrt(fmax(est, 1.0) * scale) + 0.02 * est + 64.0;
    // Whole 128-byte lines per slot (align = 16 tuples of 8 bytes, or 64 of
    // 6 bytes): partitions never share a cache line, so the scatter's partial
    // lines at slot edges are not split across XCDs and every build/probe read
    // starts line-aligned.
    const uint32_t c = (uint32_t)min(ceil(cap), 4294967040.0);
    caps[(uint64_t)lp * F + q] = (c + align - 1) / align * align;
  }
}

// gcur = partBegin = exclusive prefix of caps; gend = start + cap.  Both are
// clamped to the allocated capacity, so no write or later read can leave the
// buffer even if the host-side bound were ever too small (the slot would
// just overflow and trigger the exact re-run).
__global__ __launch_bounds__(NT) void localSampledCursorsKernel(const uint32_t *__restrict__ caps,
                                                                const unsigned long long *__restrict__ starts,
                                                                uint64_t P, unsigned long long capacity,
                                                                unsigned long long *__restrict__ gcur,
                                                                unsigned long long *__restrict__ gend,
                                                                uint64_t *__restrict__ partBegin) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < P; i += stride) {
    const unsigned long long s = min(starts[i], capacity);
    gcur[i] = s;
    gend[i] = min(s + (unsigned long long)caps[i], capacity);
    partBegin[i] = s;
  }
}

// flag |= some final claim cursor passed its slice end (the run is redone
// exactly); gcur is clamped to the slice end so that, used as partition ends,
// it never points past what was written.
__global__ __launch_bounds__(NT) void claimOverflowKernel(unsigned long long *__restrict__ gcur,
                                                          const unsigned long long *__restrict__ gend, uint64_t P,
                                                          unsigned int *flag) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  bool over = false;
  for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < P; i += stride) {
    const unsigned long long g = gcur[i], e = gend[i];
    if (g > e) {
      over = true;
      gcur[i] = e;
    }
  }
  if (__any(over) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(flag, 1u);
}

void localSampledLayout(const uint32_t *itemHist, const uint32_t *lpItemBegin, const LocalItem *items,
                        uint32_t owned, uint32_t bits, uint32_t sampleStride, uint32_t *caps,
                        unsigned long long *starts, void *scanWorkspace, unsigned long long *gcur,
                        unsigned long long *gend, uint64_t *partBegin, uint64_t capacity, hipStream_t s,
                        uint32_t align) {
  if (owned == 0) return;
  HJ_CHECK(align >= 1 && align <= 256, "localSampledLayout: align=%u", align);
  const uint64_t P = (uint64_t)owned << bits;
  hipLaunchKernelGGL(localCapacityKernel, dim3(owned), dim3(NT), 0, s, itemHist, lpItemBegin, items, bits,
                     sampleStride, align, caps);
  HIP_CHECK_LAUNCH();
  scanExclusiveU32to64(caps, starts, P, nullptr, scanWorkspace, s);
  const uint32_t grid = (uint32_t)std::min<uint64_t>(ceilDiv(P, NT), 4096);
  hipLaunchKernelGGL(localSampledCursorsKernel, dim3(grid), dim3(NT), 0, s, caps, starts, P,
                     (unsigned long long)capacity, gcur, gend, partBegin);
  HIP_CHECK_LAUNCH();
}

uint64_t localSampledCapacityBound(uint64_t n, uint64_t partitions, uint32_t sampleStride, uint32_t align) {
  // Sum of the per-partition capacities: estimates sum to n; by Cauchy-Schwarz
  // the sigma terms sum to at most LOCAL_SIGMAS sqrt(n * S * P); + per partition for
  // the constant, the ceil and float rounding.
  // (an item's len/seen ratio is at most ~sampleStride; +1 covers the rounding)
  const double bound = 1.02 * (double)n +
                       LOCAL_SIGMAS * std::sqrt(((double)n + (double)partitions) * (sampleStride + 1.0) * (double)partitions) +
                       (66.0 + align) * (double)partitions;  // 64 + ceil + line rounding + float slack
  return (uint64_t)(bound * 1.001) + 1024;
}

void claimOverflow(unsigned long long *gcur, const unsigned long long *gend, uint64_t P, unsigned int *flag,
                   hipStream_t s) {
  if (P == 0) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(ceilDiv(P, NT), 4096);
  hipLaunchKernelGGL(claimOverflowKernel, dim3(grid), dim3(NT), 0, s, gcur, gend, P, flag);
  HIP_CHECK_LAUNCH();
}

// Persistent local claim scatter.  Work items are short (1B x 1B: a network
// partition's slice of one claim group, ~120K tuples = 15 tiles) and the
// production workgroup owns its CU (1024 threads, ~90 KB of LDS), so a
// workgroup per item drained the tile pipeline at every item end (the last
// tile's write-out overlapped nothing) and refilled it at the next item's
// start (workgroup launch, LDS init, first tile's loads exposed).  Here a
// workgroup walks the items of its XCD's contiguous run with a stride of the
// workgroups on that XCD, and the prefetch issued while an item's last tile
// is staged already loads the next item's first tile.  Between items only
// the bounded slot ends are swapped (after an LDS barrier: the last
// write-out read them).
template <class Pol, typename CurT, int NTH, int IPT, bool BOUNDED, int MAXD>
__global__ __launch_bounds__(NTH, ScatterOcc<NTH>::value) void localScatterPersistKernel(
    const typename Pol::InT *__restrict__ in, const LocalItem *__restrict__ items, uint32_t nItems, uint32_t F,
    Pol pol, CurT *__restrict__ gcur, typename Pol::OutT *out, const CurT *__restrict__ gend, uint32_t perXcd,
    RoundMap im) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t TILE = NTH * IPT;
  const uint32_t q = (nItems + NGROUPS - 1) / NGROUPS;
  const uint32_t first = (blockIdx.x % NGROUPS) * q, last = min(nItems, first + q);  // this XCD's items
  uint32_t cur = first + blockIdx.x / NGROUPS;
  if (cur >= last) return;  // uniform per workgroup
  const uint32_t FP = padDigits(F);
  const ScatterSmem<Pol, CurT, TILE> l(smem, F);
  LocalItem it = items[cur];
  for (uint32_t d = threadIdx.x; d < FP; d += NTH) {
    l.cnt[d] = 0;
    if constexpr (BOUNDED)
      if (d < F) l.cursor[d] = gend[(uint64_t)it.stream * F + d];
  }
  __syncthreads();
  typename Pol::LoadT v[IPT];
  ScatterProf pf;
  prefetchTile<Pol, NTH, IPT>(in, it.begin, it.begin + it.len - 1, v, im);
  for (;;) {
    const uint32_t nxt = cur + perXcd;
    const bool more = nxt < last;
    const LocalItem nit = more ? items[nxt] : it;
    const uint64_t end = it.begin + it.len;
    CurT *gc = gcur + (uint64_t)it.stream * F;
    for (uint64_t base = it.begin; base < end; base += TILE) {
      const bool lastTile = base + TILE >= end;
      const uint64_t nb = lastTile ? nit.begin : base + TILE;
      const uint64_t nl = lastTile ? nit.begin + nit.len - 1 : end - 1;
      if (base + TILE <= end)
        scatterTile<Pol, CurT, NTH, IPT, 0, true, true, BOUNDED, MAXD>(in, base, end, TILE, F, l, pol, out, v, gc,
                                                                       pf, nb, nl, im);
      else
        scatterTile<Pol, CurT, NTH, IPT, 0, false, true, BOUNDED, MAXD>(in, base, end, (uint32_t)(end - base), F, l,
                                                                        pol, out, v, gc, pf, nb, nl, im);
    }
    if (!more) break;
    if constexpr (BOUNDED) {
      CurT e[MAXD];
#pragma unroll
      for (int k = 0; k < MAXD; ++k) {
        const uint32_t d = threadIdx.x + k * NTH;
        e[k] = d < F ? gend[(uint64_t)nit.stream * F + d] : (CurT)0;
      }
      ldsBarrier();  // every wave's last write-out has read the old slot ends
#pragma unroll
      for (int k = 0; k < MAXD; ++k) {
        const uint32_t d = threadIdx.x + k * NTH;
        if (d < F) l.cursor[d] = e[k];
      }
      // visible to the next tile's write-out through its barriers A and B
    }
    it = nit;
    cur = nxt;
  }
  pf.flush();
}

// Workgroups per XCD of the persistent local scatter: what stays resident.
template <class K>
static uint32_t persistPerXcd(K kernel, uint32_t nth, size_t lds, uint32_t nItems) {
  static thread_local int cus = 0;
  if (!cus) {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  int per = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, reinterpret_cast<const void *>(kernel), (int)nth, lds));
  const uint32_t q = (nItems + NGROUPS - 1) / NGROUPS;
  const uint32_t want = (uint32_t)std::max(1, per) * (uint32_t)std::max(1, cus / (int)NGROUPS);
  return std::max<uint32_t>(1, std::min<uint32_t>(want, q));
}

template <class P, typename C, int NTH, int IPT>
static void launchLocalClaimPersist(const void *in, const LocalItem *items, uint32_t nItems, uint32_t F, const P &pol,
                                    void *gcur, void *out, const void *gend, hipStream_t s, RoundMap rm) {
  const size_t lds = ScatterLayout<P, C, NTH * IPT>::bytes(F);
  HJ_CHECK(lds <= 160 * 1024, "local scatter LDS %zu too large", lds);
  withMaxd<NTH>(F, [&](auto maxd) {
    constexpr int M = decltype(maxd)::value;
    auto go = [&](auto kernel, const C *ge) {
      const uint32_t per = persistPerXcd(kernel, NTH, lds, nItems);
      hipLaunchKernelGGL(kernel, dim3(per * NGROUPS), dim3(NTH), lds, s, reinterpret_cast<const typename P::InT *>(in),
                         items, nItems, F, pol, reinterpret_cast<C *>(gcur), reinterpret_cast<typename P::OutT *>(out),
                         ge, per, rm);
    };
    if (gend)
      go(localScatterPersistKernel<P, C, NTH, IPT, true, M>, reinterpret_cast<const C *>(gend));
    else
      go(localScatterPersistKernel<P, C, NTH, IPT, false, M>, nullptr);
  });
}

template <class P>
static void setSplit(P &, const SplitLayout &) {}
static void setSplit(LocalFragPol &p, const SplitLayout &sl) { p.fragShift = sl.fragShift; }
static void setSplit(LocalSplitPol &p, const SplitLayout &sl) {
  p.hi = sl.hi;
  p.fragShift = sl.fragShift;
  p.loShift = sl.loShift;
}

// Always the persistent 1024 x 8 kernel.  Retired after measurement: one
// workgroup per item at the same shape (6.29 ms against 5.96-6.01 persistent),
// persistent 12 / 10 tuples per thread (6.10-6.11 ms; profiles/r6/README.md)
// and the 512- / 256-thread and 1024 x 16 shapes (docs/ROUND4.md).
void localScatter(const void *in, bool wide, const LocalItem *items, uint32_t nItems, uint32_t shift, uint32_t bits,
                  void *gcur, bool narrow, void *out, hipStream_t s, const void *gend, SplitLayout split, bool frag,
                  RoundMap rm) {
  HJ_CHECK(!(wide && split.on), "localScatter: the split layout needs compressed input");
  HJ_CHECK(!split.on || frag || split.hi, "localScatter: split layout without a fragment column");
  HJ_CHECK(!(frag && wide), "localScatter: fragments are not wide tuples");
  HJ_CHECK(bits <= MAX_PART_BITS, "localScatter: bits=%u out of range", bits);
  if (nItems == 0) return;
  const uint32_t F = 1u << bits;
  auto go = [&](auto pol) {
    using P = decltype(pol);
    pol.mask = F - 1;
    pol.shift = shift;
    setSplit(pol, split);
    if (narrow)
      launchLocalClaimPersist<P, uint32_t, CL_NTH, CL_IPT>(in, items, nItems, F, pol, gcur, out, gend, s, rm);
    else
      launchLocalClaimPersist<P, unsigned long long, CL_NTH, CL_IPT>(in, items, nItems, F, pol, gcur, out, gend, s,
                                                                     rm);
  };
  if (frag)
    go(LocalFragPol());
  else if (wide)
    go(LocalWidePol());
  else if (split.on)
    go(LocalSplitPol());
  else
    go(LocalCompressedPol());
  HIP_CHECK_LAUNCH();
}

void scatterProfileLocal(unsigned long long acc[10], bool reset) { scatterProfileAdd(acc, reset); }

// Loads this file's code object at engine start (kernels::preloadCodeObjects).
void preloadLocalPartition() {
  hipFuncAttributes a;
  HIP_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&claimOverflowKernel)));
}

}  // namespace kernels
}  // namespace hpcjoin

