// LDS write-combining scatter of both radix passes: device templates shared
// by net_partition.hip, local_partition.hip and scatter_ablation.hip.
//
// Each tile is ranked per digit with LDS atomics, block-scanned, reordered
// through LDS so that consecutive lanes hold consecutive tuples of the same
// digit, then streamed out.  Because a workgroup's tiles are contiguous, a
// digit's output run continues across tiles and the L2 / Infinity Cache merge
// the partial lines (the GPU analog of the reference's 64-byte cache-line
// buffers + non-temporal flushes).  The packed CompressedTuple (8 B) halves
// everything written after pass 1.
//
// Every including file is its own code object: the trash line and the profile
// counters below are per file (static).
#pragma once

#include "kernels.h"
#include "device_common.h"

#include <type_traits>

namespace hpcjoin {
namespace kernels {

constexpr int NT = PART_THREADS;
constexpr uint32_t NGROUPS = 8;  // XCDs on MI355X

// ------------------------------------------------------------------ loads
// Input streams are read exactly once: non-temporal loads keep them from
// evicting the partially filled output lines the L2 is write-combining.
using u64x2 = unsigned long long __attribute__((ext_vector_type(2)));
template <typename InT>
struct Loader;
template <>
struct Loader<ulonglong2> {
  static __device__ __forceinline__ ulonglong2 load(const ulonglong2 *p) {
    const u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p));
    return make_ulonglong2(v.x, v.y);
  }
};
template <>
struct Loader<uint64_t> {
  static __device__ __forceinline__ uint64_t load(const uint64_t *p) { return __builtin_nontemporal_load(p); }
};
template <>
struct Loader<uint32_t> {
  static __device__ __forceinline__ uint32_t load(const uint32_t *p) { return __builtin_nontemporal_load(p); }
};

// What a scatter policy loads per element.  PlainLoad: the whole input
// element.  KeyLoad: only the key of a 16-byte tuple, for policies whose
// output never carries the rid (count-only fragments, key-only words): half
// the VGPRs per element in flight.  With whole tuples the frag scatter sat at
// 121 VGPRs and the compiler reused the dead rid halves of pending loads for
// address arithmetic, which put an s_waitcnt vmcnt(0) after every second
// load of the next tile's prefetch (three serial HBM round trips per tile).
template <typename In>
struct PlainLoad {
  using LoadT = In;
  static __device__ __forceinline__ LoadT load(const In *p) { return Loader<In>::load(p); }
};
// In = uint64_t: the input is a key column (kernels.h, KeySource), the same
// 8-byte load from elements 8 bytes apart: a wave's load instruction then
// covers 512 contiguous bytes instead of every other 8 of 1024.
template <typename In = ulonglong2>
struct KeyLoad {
  using LoadT = uint64_t;
  static __device__ __forceinline__ LoadT load(const In *p) {
    return __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(p));
  }
};

// -------------------------------------------------- LDS write-combining scatter
// A scatter policy says how a tuple is ranked (digit), what is staged in LDS
// (the packed output word, possibly carrying its digit in spare top bits),
// how the digit is recovered from the staged word and what is finally
// written.  Only the compressed network pass may need a separate LDS digit
// array: the local pass and wide tuples recompute the digit from the staged
// word, and compressed words carry it in their top bits whenever the key
// range leaves `bits` spare bits (JoinPlan knows; the 1B config does).
struct NetCompressedPol : PlainLoad<ulonglong2> {  // 16 B tuple -> 8 B CompressedTuple, digit in the top bits
  using InT = ulonglong2;
  using StageT = uint64_t;
  using OutT = uint64_t;
  static constexpr bool kDigArray = false;
  uint64_t mask;
  uint32_t bits, keyShift;
  KeyMix mix;
  // ~0 = keep the rid below keyShift; 0 = key-only words (count-only joins of
  // keys too wide for a CompressedTuple: value = key >> bits, keyShift = 0).
  uint64_t ridMask = ~0ull;
  __device__ __forceinline__ uint32_t digit(const InT &x) const { return (uint32_t)(mix.apply(x.x) & mask); }
  __device__ __forceinline__ StageT stage(const InT &x, uint32_t d) const {
    return (x.y & ridMask) | ((mix.apply(x.x) >> bits) << keyShift) | ((uint64_t)d << (64 - bits));
  }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &v) const { return (uint32_t)(v >> (64 - bits)); }
  __device__ __forceinline__ OutT out(const StageT &v) const { return v & (~0ull >> bits); }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
struct NetCompressedDigPol : NetCompressedPol {  // no spare bits: digits staged separately
  static constexpr bool kDigArray = true;
  __device__ __forceinline__ StageT stage(const InT &x, uint32_t) const {
    return (x.y & ridMask) | ((mix.apply(x.x) >> bits) << keyShift);
  }
  __device__ __forceinline__ OutT out(const StageT &v) const { return v; }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
// Key-only words (count-only joins of keys too wide for a CompressedTuple,
// JoinPlan::keyOnly): value = mixed key >> bits, digit in the top bits (the
// word has `bits` spare bits by construction); only keys are loaded.  MIX is
// the plan's key mixing as a compile-time choice (no branch per element).
template <bool MIX>
__device__ __forceinline__ uint64_t mixKey(const KeyMix &m, uint64_t k) {
  if constexpr (MIX)
    return KeyMix{1u, m.bits}.apply(k);
  else
    return k;
}
template <bool MIX, typename In = ulonglong2>
struct NetKeyPol : KeyLoad<In> {
  using InT = In;
  using LoadT = uint64_t;
  using StageT = uint64_t;
  using OutT = uint64_t;
  static constexpr bool kDigArray = false;
  uint64_t mask;
  uint32_t bits;
  KeyMix mix;
  __device__ __forceinline__ uint32_t digit(const LoadT &k) const { return (uint32_t)(mixKey<MIX>(mix, k) & mask); }
  __device__ __forceinline__ StageT stage(const LoadT &k, uint32_t d) const {
    return (mixKey<MIX>(mix, k) >> bits) | ((uint64_t)d << (64 - bits));
  }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &v) const { return (uint32_t)(v >> (64 - bits)); }
  __device__ __forceinline__ OutT out(const StageT &v) const { return v & (~0ull >> bits); }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
// Count-only projection: a counting join never reads a rid, so the network
// pass keeps only the key fragment above the network digit (4 bytes instead
// of the 8-byte CompressedTuple; the reference compares key bits only,
// tasks/BuildProbe.cpp:101-102, and reports only the count, :115).  The
// digit rides in the staged word's top bits (fragBits + bits <= 32, checked
// by the launcher).
//
// FILT (partition-group passes, kernels.h netScatterFragRange): only digits
// [dLo, dLo + range) are written, renumbered 0..range-1; every other tuple
// gets the sentinel digit `range`, is ranked and staged behind the kept ones
// and never stored (scatterTile: FilterOf).
template <bool FILT>
__device__ __forceinline__ uint32_t rangeDigit(uint32_t d, uint32_t dLo, uint32_t range) {
  if constexpr (FILT) {
    d -= dLo;  // wraps below dLo
    return d < range ? d : range;
  } else {
    return d;
  }
}
template <bool MIX, bool FILT = false, typename In = ulonglong2>
struct NetFragPolT : KeyLoad<In> {
  using InT = In;
  using LoadT = uint64_t;
  using StageT = uint32_t;
  using OutT = uint32_t;
  static constexpr bool kDigArray = false;
  static constexpr bool kEarly = true;  // earlyPrefetch
  static constexpr bool kFilter = FILT;
  uint64_t mask;
  uint32_t bits;
  KeyMix mix;
  uint32_t dLo = 0, range = 0;
  __device__ __forceinline__ uint32_t digit(const LoadT &k) const {
    return rangeDigit<FILT>((uint32_t)(mixKey<MIX>(mix, k) & mask), dLo, range);
  }
  __device__ __forceinline__ StageT stage(const LoadT &k, uint32_t d) const {
    return (uint32_t)(mixKey<MIX>(mix, k) >> bits) | (d << (32 - bits));
  }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &v) const { return v >> (32 - bits); }
  __device__ __forceinline__ OutT out(const StageT &v) const { return v & (0xFFFFFFFFu >> bits); }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
using NetFragPol = NetFragPolT<false>;  // ablation entry (no key mixing)
// Fragments of keys wider than 32 bits (fragWordFits: keyBits <= 32 + bits,
// e.g. 6B dense keys = 33 bits): the staged u32 word is the whole fragment
// and the digit goes to the tile's u16 digit array (no early prefetch).
template <bool MIX, bool FILT = false, typename In = ulonglong2>
struct NetFragDigPolT : KeyLoad<In> {
  using InT = In;
  using LoadT = uint64_t;
  using StageT = uint32_t;
  using OutT = uint32_t;
  static constexpr bool kDigArray = true;
  static constexpr bool kFilter = FILT;
  uint64_t mask;
  uint32_t bits;
  KeyMix mix;
  uint32_t dLo = 0, range = 0;
  __device__ __forceinline__ uint32_t digit(const LoadT &k) const {
    return rangeDigit<FILT>((uint32_t)(mixKey<MIX>(mix, k) & mask), dLo, range);
  }
  __device__ __forceinline__ StageT stage(const LoadT &k, uint32_t) const {
    return (uint32_t)(mixKey<MIX>(mix, k) >> bits);
  }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &) const { return 0; }  // digits: LDS array
  __device__ __forceinline__ OutT out(const StageT &v) const { return v; }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = v; }
};
struct NetWidePol : PlainLoad<ulonglong2> {  // 16 B tuple -> 16 B tuple (full-range keys)
  using InT = ulonglong2;
  using StageT = ulonglong2;
  using OutT = ulonglong2;
  static constexpr bool kDigArray = false;
  uint64_t mask;
  KeyMix mix;
  __device__ __forceinline__ uint32_t digit(const InT &x) const { return (uint32_t)(mix.apply(x.x) & mask); }
  __device__ __forceinline__ StageT stage(const InT &x, uint32_t) const {
    return make_ulonglong2(mix.apply(x.x), x.y);
  }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &v) const { return (uint32_t)(v.x & mask); }
  __device__ __forceinline__ OutT out(const StageT &v) const { return v; }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
struct LocalCompressedPol : PlainLoad<uint64_t> {  // 8 B -> 8 B, digit = (value >> shift) & mask
  using InT = uint64_t;
  using StageT = uint64_t;
  using OutT = uint64_t;
  static constexpr bool kDigArray = false;
  uint64_t mask;
  uint32_t shift;
  __device__ __forceinline__ uint32_t digit(const InT &x) const { return (uint32_t)((x >> shift) & mask); }
  __device__ __forceinline__ StageT stage(const InT &x, uint32_t) const { return x; }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &v) const { return digit(v); }
  __device__ __forceinline__ OutT out(const StageT &v) const { return v; }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
struct LocalWidePol : PlainLoad<ulonglong2> {  // 16 B -> 16 B, digit = (key >> shift) & mask
  using InT = ulonglong2;
  using StageT = ulonglong2;
  using OutT = ulonglong2;
  static constexpr bool kDigArray = false;
  uint64_t mask;
  uint32_t shift;
  __device__ __forceinline__ uint32_t digit(const InT &x) const { return (uint32_t)((x.x >> shift) & mask); }
  __device__ __forceinline__ StageT stage(const InT &x, uint32_t) const { return x; }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &v) const { return digit(v); }
  __device__ __forceinline__ OutT out(const StageT &v) const { return v; }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
// u32 key fragment -> u16 of the bits above the local digit (count-only
// two-level pass, JoinPlan::fragments): 2 bytes written per tuple.
struct LocalFragPol : PlainLoad<uint32_t> {
  using InT = uint32_t;
  using StageT = uint32_t;
  using OutT = uint16_t;
  static constexpr bool kDigArray = false;
  uint64_t mask;
  uint32_t shift;
  uint32_t fragShift;
  __device__ __forceinline__ uint32_t digit(const InT &x) const { return (uint32_t)((x >> shift) & mask); }
  __device__ __forceinline__ StageT stage(const InT &x, uint32_t) const { return x; }
  __device__ __forceinline__ uint32_t stagedDigit(const StageT &v) const { return digit(v); }
  __device__ __forceinline__ OutT out(const StageT &v) const { return (uint16_t)(v >> fragShift); }
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const { o[pos] = out(v); }
};
struct LocalSplitPol : LocalCompressedPol {  // 8 B -> u32 rid / key low word + u16 fragment (kernels.h, SplitLayout)
  using OutT = uint32_t;
  uint16_t *hi;
  uint32_t fragShift;
  uint32_t loShift = 0;
  __device__ __forceinline__ void store(OutT *o, uint64_t pos, const StageT &v) const {
    o[pos] = (uint32_t)(v >> loShift);
    hi[pos] = (uint16_t)(v >> fragShift);
  }
};

// Digit arrays in LDS are padded to at least 1024 entries (the widest
// workgroup): every thread of the claim loop then owns whole, existing
// entries, and the loop needs no per-thread bound check (see scatterTile).
HJ_HD uint32_t padDigits(uint32_t F) { return F > 1024u ? F : 1024u; }

// LDS per workgroup: cursor and wbase (FP x CurT), cnt and off (FP x u32)
// with FP = padDigits(F), scan scratch, the reordered tile (TILE x StageT)
// and, only for NetCompressedDigPol, the tile's digits (TILE x u16).
template <class Pol, typename CurT, int TILE>
struct ScatterLayout {
  static __host__ __device__ constexpr size_t valOffset(uint32_t F) {
    return ((size_t)padDigits(F) * (2 * sizeof(CurT) + 8) + 64 + 15) & ~size_t(15);
  }
  static __host__ __device__ constexpr size_t bytes(uint32_t F) {
    return valOffset(F) + (size_t)TILE * sizeof(typename Pol::StageT) + (Pol::kDigArray ? (size_t)TILE * 2 : 0);
  }
};

// Per-workgroup LDS carve of the scatter (see ScatterLayout).
template <class Pol, typename CurT, int TILE>
struct ScatterSmem {
  CurT *cursor, *wbase;
  uint32_t *cnt, *off, *wave;
  typename Pol::StageT *val;
  uint16_t *dig;
  __device__ __forceinline__ ScatterSmem(unsigned char *smem, uint32_t F) {
    const uint32_t FP = padDigits(F);
    cursor = reinterpret_cast<CurT *>(smem);
    wbase = cursor + FP;
    cnt = reinterpret_cast<uint32_t *>(wbase + FP);
    off = cnt + FP;
    wave = off + FP;
    val = reinterpret_cast<typename Pol::StageT *>(smem + ScatterLayout<Pol, CurT, TILE>::valOffset(F));
    dig = reinterpret_cast<uint16_t *>(val + TILE);
  }
};

// Where the branch-free scatter sends what must not land in the output:
// stores of lanes without an element (a range's tail tile) or past a bounded
// slice, and the claim atomics of padding digits (adding 0).  Writing these
// to scratch instead of branching around them keeps the tile loop free of
// divergent control flow: after a store or atomic under an exec mask the
// compiler's wait-count pass can no longer count the wave's memory operations
// and falls back to vmcnt(0) -- every load and store of the wave in flight
// must land -- and it serialises the write-out's LDS reads element by element.
static __device__ ulonglong2 g_scatterTrash[1024];

// Per-phase shader-clock breakdown of the claim scatter's tile loop, built
// only with -DHPCJOIN_SCATTER_PROF (HPCJOIN_EXTRA_HIPFLAGS at build time;
// tools/scatter_phases.py reads it through ops.scatter_profile()).  Wave 0
// of every workgroup stamps s_memtime at the phase boundaries; the sums of
// the per-phase deltas (scalar registers) are added to g_scatterProf once per
// range, by lane 0, with vector atomics.
//   0 rank (includes waiting for the tile's loads)  1 barrier A
//   2 claims + prefetch issue  3 scan  4 staging  5 write bases (claims land)
//   6 barrier B  7 write-out issue
static __device__ unsigned long long g_scatterProf[10];
// acc += this file's counters (kernels::scatterProfile sums every scatter file).
static inline void scatterProfileAdd(unsigned long long acc[10], bool reset) {
  unsigned long long mine[10];
  HIP_CHECK(hipMemcpyFromSymbol(mine, HIP_SYMBOL(g_scatterProf), sizeof(mine)));
  for (int i = 0; i < 10; ++i) acc[i] += mine[i];
  if (reset) {
    const unsigned long long z[10] = {};
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_scatterProf), z, sizeof(z)));
  }
}
struct ScatterProf {
#ifdef HPCJOIN_SCATTER_PROF
  uint64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t last = 0, tiles = 0;
  __device__ __forceinline__ void start() { last = __builtin_readcyclecounter(); }
  __device__ __forceinline__ void mark(int i) {
    const uint64_t now = __builtin_readcyclecounter();
    acc[i] += now - last;
    last = now;
  }
  __device__ __forceinline__ void flush() {
    if (threadIdx.x != 0) return;
    for (int i = 0; i < 8; ++i) atomicAdd(&g_scatterProf[i], (unsigned long long)acc[i]);
    atomicAdd(&g_scatterProf[8], (unsigned long long)tiles);
    atomicAdd(&g_scatterProf[9], 1ull);
  }
#else
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void flush() {}
#endif
};

template <class P, class = void>
struct TwoArrayStore : std::false_type {};
template <class P>
struct TwoArrayStore<P, std::void_t<decltype(&P::hi)>> : std::true_type {};

// Stores x at out[pos] when ok, else into the trash line of thread t.
template <class Pol>
__device__ __forceinline__ void storeSel(const Pol &pol, typename Pol::OutT *out, uint64_t pos,
                                         const typename Pol::StageT &x, bool ok, uint32_t t) {
  using OutT = typename Pol::OutT;
  OutT *trash = reinterpret_cast<OutT *>(g_scatterTrash);
  if constexpr (TwoArrayStore<Pol>::value) {
    uint16_t *hi = ok ? pol.hi + pos : reinterpret_cast<uint16_t *>(g_scatterTrash + 512) + t;
    OutT *lo = ok ? out + pos : trash + t;
    *lo = (OutT)(x >> pol.loShift);
    *hi = (uint16_t)(x >> pol.fragShift);
  } else {
    OutT *p = ok ? out + pos : trash + t;
    *p = pol.out(x);
  }
}

template <class Pol, int NTH, int IPT, bool FULL>
__device__ __forceinline__ void loadTile(const typename Pol::InT *__restrict__ src, uint32_t count,
                                         typename Pol::LoadT (&v)[IPT]) {
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const uint32_t idx = i * NTH + threadIdx.x;
    if (FULL || idx < count) v[i] = Pol::load(src + idx);
  }
}

// Next tile into registers, branch-free: indices past the range end read its
// last element (loaded, never ranked), so every tile issues exactly IPT loads.
// im: slot map of the input (RoundMap; identity unless the local pass reads a
// round-interleaved network window).
template <class Pol, int NTH, int IPT>
__device__ __forceinline__ void prefetchTile(const typename Pol::InT *__restrict__ in, uint64_t nbase, uint64_t last,
                                             typename Pol::LoadT (&v)[IPT], const RoundMap &im = RoundMap()) {
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const uint64_t idx = nbase + (uint64_t)(i * NTH + threadIdx.x);
    v[i] = Pol::load(in + im(idx < last ? idx : last));
  }
}

// Early prefetch: when the staged word is no wider than the loaded one and
// carries its digit (no separate digit array), the rank phase turns every
// loaded element into its staged word right away, so the registers of the
// loaded tile are free again before the scan -- the next tile's loads are
// issued after the claims (so the claim atomics, issued first, can be waited
// for without waiting for the loads) and overlap the scan, the staging and
// the write-out instead of only the write-out.  Only where the tile's loads
// take at most 16 VGPRs per thread: with wider tiles the staged words, ranks
// and next tile no longer fit 128 VGPRs (1024-thread groups) and spill.  And
// only for policies that opt in (kEarly): measured on MI355X, same box, the
// count-only fragment scatter gains (1.90 -> 1.80 ms per call, 1B x 1B join
// 10.16 -> 9.62 ms) while the key-only scatter is unchanged (2.28 / 2.31) and
// the local split scatter loses (1.45 -> 1.54).
template <class P, class = void>
struct FilterOf : std::false_type {};
template <class P>
struct FilterOf<P, std::void_t<decltype(P::kFilter)>> : std::integral_constant<bool, P::kFilter> {};

template <class P, class = void>
struct EarlyOptIn : std::false_type {};
template <class P>
struct EarlyOptIn<P, std::void_t<decltype(P::kEarly)>> : std::integral_constant<bool, P::kEarly> {};
template <class Pol, int IPT>
constexpr bool earlyPrefetch() {
  return EarlyOptIn<Pol>::value && !Pol::kDigArray && sizeof(typename Pol::StageT) <= sizeof(typename Pol::LoadT) &&
         IPT * sizeof(typename Pol::LoadT) <= 64;
}

// One tile.  The next tile's loads ([nbase, nbase + TILE), clamped to nlast)
// are issued into v while this one is staged or written out: the caller's
// next tile of the same range, or the first tile of its next range.
// FULL tiles (every tile but a range's tail) have no divergent
// control flow at all, so hipcc keeps the IPT LDS atomics, loads and stores
// in flight with counted waits; the tail tile predicates its LDS work only.
// BOUNDED (claim mode with estimated slices): l.cursor[d] holds the end of the
// group's slice of digit d; claimed positions past it are not written (the
// caller detects the overflow from the final claim cursors and re-runs).
// MAXD = padDigits(F) / NTH claim entries per thread.
template <class Pol, typename CurT, int NTH, int IPT, int MODE, bool FULL, bool CLAIM, bool BOUNDED, int MAXD>
__device__ __forceinline__ void scatterTile(const typename Pol::InT *__restrict__ in, uint64_t base, uint64_t end,
                                            uint32_t count, uint32_t F, const ScatterSmem<Pol, CurT, NTH * IPT> &l,
                                            const Pol &pol, typename Pol::OutT *__restrict__ out,
                                            typename Pol::LoadT (&v)[IPT], CurT *__restrict__ gcur,
                                            ScatterProf &pf, uint64_t nbase, uint64_t nlast,
                                            const RoundMap &im = RoundMap(), const RoundMap &om = RoundMap()) {
  constexpr uint32_t TILE = NTH * IPT;
  pf.start();
  constexpr bool EARLY = earlyPrefetch<Pol, IPT>();
  const uint32_t t = threadIdx.x;
  // EARLY: sw = staged words, dr = ranks (then positions); else dr = digit << 16 | rank.
  uint32_t dr[IPT];
  typename Pol::StageT sw[EARLY ? IPT : 1];
  // FILT: tuples outside the pass's digit range (sentinel digit F) are neither
  // ranked nor staged -- a pass over a quarter of the digits does a quarter of
  // the LDS work; the scan's entry F then stays 0 and off[F] = kept.
  constexpr bool FILT = FilterOf<Pol>::value;
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const uint32_t idx = i * NTH + t;
    if (FULL || idx < count) {
      const uint32_t d = pol.digit(v[i]);
      const bool keep = !FILT || d < F;
      if constexpr (EARLY) {
        if (keep) dr[i] = atomicAdd(&l.cnt[d], 1u);
        sw[i] = pol.stage(v[i], d);
      } else {
        dr[i] = (d << 16) | (keep ? atomicAdd(&l.cnt[d], 1u) : 0u);
      }
    }
  }
  pf.mark(0);
  // Barriers of the tile loop order LDS only (ldsBarrier): the waves share
  // nothing through global memory here, and a full __syncthreads() would make
  // every wave wait for its prefetch of the next tile (vmcnt(0)) before the
  // write-out, so loads and stores of a workgroup would never overlap.
  ldsBarrier();  // A: counts final; previous tile's write-out done
  pf.mark(1);
  CurT claim[MAXD];
  if constexpr (CLAIM) {
    // One device atomic per digit claims this tile's run in the group's slice,
    // issued before the scan so its round trip overlaps the scan.  Waves whose
    // digits are all padding (d >= F: F < NTH) skip it on a scalar branch (no
    // exec mask); a wave straddling F (only F < 64) sends its padding lanes'
    // zero adds to the trash.
    CurT *trash = reinterpret_cast<CurT *>(g_scatterTrash);
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t & ~(uint32_t)(WAVE - 1)));
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
      const uint32_t d = t + k * NTH;
      if (wave0 + k * NTH < F) claim[k] = atomicAdd(d < F ? gcur + d : trash + t, (CurT)l.cnt[d]);
    }
  }
  if constexpr (EARLY) prefetchTile<Pol, NTH, IPT>(in, nbase, nlast, v, im);
  pf.mark(2);
  // FILT: entry F (never counted) is scanned too: off[F] = kept tuples, and
  // the write-out stops there.
  blockExclusiveScanLds<NTH, uint32_t, uint32_t, true>(l.cnt, l.off, (int)F + (FILT ? 1 : 0), l.wave);
  uint32_t kept = count;
  if constexpr (FILT) kept = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.off[F]);
  pf.mark(3);
  if constexpr (!CLAIM) {
    for (uint32_t d = t; d < F; d += NTH) {
      const CurT c = l.cursor[d];
      l.wbase[d] = c - (CurT)l.off[d];  // wraps; wbase + idx lands back in range
      l.cursor[d] = c + (CurT)l.cnt[d];
      l.cnt[d] = 0;
    }
  }
  // Staging: every position first, then every write (one batch of LDS reads
  // and one of writes; interleaved, each write waited for its own read).
  if constexpr (EARLY) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint32_t idx = i * NTH + t;
      if ((FULL || idx < count) && (!FILT || pol.stagedDigit(sw[i]) < F)) dr[i] += l.off[pol.stagedDigit(sw[i])];
    }
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint32_t idx = i * NTH + t;
      if ((FULL || idx < count) && (!FILT || pol.stagedDigit(sw[i]) < F)) l.val[dr[i]] = sw[i];
    }
  } else {
    uint32_t pos[IPT];
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint32_t idx = i * NTH + t;
      if (FULL || idx < count) pos[i] = l.off[dr[i] >> 16] + (dr[i] & 0xFFFFu);
    }
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint32_t idx = i * NTH + t;
      if ((FULL || idx < count) && (!FILT || (dr[i] >> 16) < F)) {
        const uint32_t d = dr[i] >> 16;
        l.val[pos[i]] = pol.stage(v[i], d);
        if constexpr (Pol::kDigArray) l.dig[pos[i]] = (uint16_t)d;
      }
    }
    // Prefetch the next tile while this one is streamed out.
    prefetchTile<Pol, NTH, IPT>(in, nbase, nlast, v, im);
  }
  pf.mark(4);
  if constexpr (CLAIM) {
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {  // padding entries get garbage bases nobody reads
      const uint32_t d = t + k * NTH;
      l.wbase[d] = claim[k] - (CurT)l.off[d];
      l.cnt[d] = 0;
    }
  }
  pf.mark(5);
  ldsBarrier();  // B: staged tile and write bases visible
  pf.mark(6);
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const uint32_t idx = i * NTH + t;
    if constexpr (FILT) {  // whole waves past the kept tuples skip on a scalar branch
      if ((uint32_t)i * NTH + (t & ~(uint32_t)(WAVE - 1)) >= kept) continue;
    }
    const bool have = FILT ? idx < kept : (FULL || idx < count);
    const uint32_t at = have ? idx : 0;  // the tail tile's element 0 exists
    const typename Pol::StageT x = l.val[at];
    uint32_t d;
    if constexpr (Pol::kDigArray)
      d = l.dig[at];
    else
      d = pol.stagedDigit(x);
    if constexpr (MODE == 0) {
      const CurT pos = (CurT)(l.wbase[d] + (CurT)idx);
      bool ok = have;
      if constexpr (BOUNDED) ok = ok && pos < l.cursor[d];
      storeSel(pol, out, om((uint64_t)pos), x, ok, t);
    } else if constexpr (MODE == 1) {
      if (have) out[base + idx] = pol.out(x);
      asm volatile("" ::"v"(l.wbase[d]));
    } else {
      const auto y = pol.out(x);
      asm volatile("" ::"v"(y), "v"(l.wbase[d]));
    }
  }
  pf.mark(7);
#ifdef HPCJOIN_SCATTER_PROF
  ++pf.tiles;
#endif
}

// Scatter [begin, end) of `in` into `out` at the cursors held in LDS
// (initialised by the caller, advanced here).  Per tile:
//   rank (LDS atomics) | A | claim + scan + per-digit write base | stage into
//   LDS, prefetch next tile into registers | B | stream the reordered tile out.
// MODE (ablation only): 0 = real scatter, 1 = coalesced write-out, 2 = none.
template <class Pol, typename CurT, int NTH, int IPT, int MODE, bool CLAIM = false, bool BOUNDED = false,
          int MAXD = 1>
__device__ __forceinline__ void scatterRange(const typename Pol::InT *__restrict__ in, uint64_t begin, uint64_t end,
                                             uint32_t F, unsigned char *smem, const Pol &pol,
                                             typename Pol::OutT *__restrict__ out, CurT *gcur = nullptr,
                                             const RoundMap &im = RoundMap(), const RoundMap &om = RoundMap()) {
  constexpr uint32_t TILE = NTH * IPT;
  const ScatterSmem<Pol, CurT, TILE> l(smem, F);
  typename Pol::LoadT v[IPT];
  ScatterProf pf;
  if (begin < end) prefetchTile<Pol, NTH, IPT>(in, begin, end - 1, v, im);
  for (uint64_t base = begin; base < end; base += TILE) {
    if (base + TILE <= end)
      scatterTile<Pol, CurT, NTH, IPT, MODE, true, CLAIM, BOUNDED, MAXD>(in, base, end, TILE, F, l, pol, out, v,
                                                                         gcur, pf, base + TILE, end - 1, im, om);
    else
      scatterTile<Pol, CurT, NTH, IPT, MODE, false, CLAIM, BOUNDED, MAXD>(in, base, end, (uint32_t)(end - base), F, l,
                                                                          pol, out, v, gcur, pf, base + TILE, end - 1,
                                                                          im, om);
  }
  pf.flush();
  __syncthreads();
}

// Occupancy target per geometry: 256-thread groups aim at 3 per CU (LDS-bound),
// 512 at 2, 1024 at 1 (second launch-bounds argument = waves per SIMD).
template <int NTH>
struct ScatterOcc {
  static constexpr int value = NTH == 256 ? 3 : (NTH == 512 ? 4 : 4);
};

// Claim-mode network scatter: cursors come from the group slices (gcur is
// [NGROUPS][F] for this chunk), so no per-workgroup cursor array is loaded.
// MAXD = padDigits(F) / NTH (withMaxd).  Here rather than in
// net_partition.hip because the ablation matrix launches it as well.
template <class Pol, typename CurT, int NTH, int IPT, int MODE, bool BOUNDED, int MAXD>
__global__ __launch_bounds__(NTH, ScatterOcc<NTH>::value) void netScatterClaimKernel(
    const typename Pol::InT *__restrict__ in, uint64_t n, uint32_t tpb, uint32_t F, Pol pol, uint32_t blockBegin,
    CurT *__restrict__ gcur, typename Pol::OutT *out, const CurT *__restrict__ gend = nullptr,
    const uint32_t *__restrict__ roundMeta = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t blk = blockBegin + blockIdx.x;
  RoundMap om;  // output slot map, decided by the layout kernel (RoundMap)
  if (roundMeta) {
    om.lp = roundMeta[0];
    om.lv = roundMeta[1];
    om.lns = roundMeta[2];
  }
  const uint32_t FP = padDigits(F);
  CurT *sliceEnd = reinterpret_cast<CurT *>(smem);  // the per-workgroup cursor array is unused in claim mode
  uint32_t *cnt = reinterpret_cast<uint32_t *>(reinterpret_cast<CurT *>(smem) + 2 * FP);
  const size_t grp = (size_t)(blockIdx.x % NGROUPS) * F;
  for (uint32_t d = threadIdx.x; d < FP; d += NTH) {
    cnt[d] = 0;
    if constexpr (BOUNDED)
      if (d < F) sliceEnd[d] = gend[grp + d];
  }
  __syncthreads();
  const uint64_t begin = (uint64_t)blk * tpb * PART_TILE;
  const uint64_t end = min(n, begin + (uint64_t)tpb * PART_TILE);
  scatterRange<Pol, CurT, NTH, IPT, MODE, true, BOUNDED, MAXD>(in, begin, end, F, smem, pol, out, gcur + grp,
                                                               RoundMap(), om);
}

// Calls fn(std::integral_constant<int, MAXD>) with MAXD = padDigits(F) / NTH:
// one of two values per workgroup width (F <= 1024 or F = 2048).
template <int NTH, class Fn>
static void withMaxd(uint32_t F, Fn &&fn) {
  constexpr int LO = 1024 / NTH, HI = (1 << MAX_PART_BITS) / NTH;
  static_assert(HI == 2 * LO, "withMaxd: two digit-array sizes");
  if (padDigits(F) / NTH == (uint32_t)LO)
    fn(std::integral_constant<int, LO>());
  else
    fn(std::integral_constant<int, HI>());
}

// The one production geometry of the claim-mode scatter, both passes
// (tools/microbench.py ablation on MI355X: 1024 threads x 8 tuples per LDS
// tile = 8192-tuple tiles, one workgroup per CU).
constexpr int CL_NTH = 1024;
constexpr int CL_IPT = 8;

// ------------------------------------------------ packed fragment scatter
// The count-only fragment scatter of the headline plan, writing the packed
// window of kernels.h (PK_*): three 20-bit fragments per 8-byte word, and
// nothing but whole, aligned 64-byte chunks of 24 fragments.  A digit's run in
// one 8192-tuple tile (8 fragments at 1024 digits) is far short of a chunk, so
// the workgroup carries every digit's partial tail (< 24 fragments) in LDS
// from tile to tile and flushes (carry + run) / 24 chunks per tile; what is
// left of the run becomes the new carry.  At the end of its range the
// workgroup writes every non-empty carry as one last, partial chunk.
//
// Same tile pipeline as scatterTile (rank by LDS atomics, ldsBarrier, claims
// issued before the scan, next tile prefetched into registers, trash stores
// instead of divergent global stores, one claim atomic per (XCD group, digit)
// and tile -- adding 0 when no chunk fills -- bounded slices), with 1024
// threads = at most 1024 digits: thread t owns digit t (its carry length lives
// in a register).
//   rank | A | move the previous tile's tail into the carry, claim 8 k words |
//   scan of (run length, k) in one packed word, chunk -> digit map | prefetch,
//   staging | B | write-out: 8 lanes per chunk, lane j packs fragments 3j..3j+2
//   of "carry, then the staged run" and stores one word.
// The carry is updated one tile late (after the next tile's barrier A): the
// write-out still reads the old carry, and this way no third barrier is needed.
// LDS (1024 digits, 64-bit cursors): counters and per-digit records 24 KiB,
// chunk map 2.6 KiB, staged tile 32 KiB, carry 96 KiB (fragment-major:
// carry[s][digit], conflict-free for the owner threads) = 154.7 KiB.
constexpr uint32_t PK_DIGITS = 1024;  // digits per workgroup (= CL_NTH)
// Chunks one tile can flush: (23 carried per digit + the tile) / 24, padded.
constexpr uint32_t PK_MAP = ((PK_CHUNK_FRAGS - 1) * PK_DIGITS + CL_NTH * CL_IPT) / PK_CHUNK_FRAGS + 22;
static_assert(PK_MAP % 8 == 0, "packed scatter: the chunk map keeps the LDS carve 16-byte aligned");

template <typename CurT>
constexpr size_t packedScatterLds() {
  return (size_t)PK_DIGITS * (8 + 2 * sizeof(CurT)) + PK_MAP * 2 + 64 + (size_t)CL_NTH * CL_IPT * 4 +
         (size_t)PK_CHUNK_FRAGS * PK_DIGITS * 4;
}

template <bool MIX, typename CurT, typename InT = ulonglong2>
__global__ __launch_bounds__(CL_NTH, ScatterOcc<CL_NTH>::value) void netScatterFragPackedKernel(
    const InT *__restrict__ in, uint64_t n, uint32_t tpb, uint32_t F, uint32_t bits, KeyMix mix,
    CurT *__restrict__ gcur, unsigned long long *out, const CurT *__restrict__ gend,
    const uint32_t *__restrict__ roundMeta, unsigned long long *__restrict__ wideFlag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Pol = NetFragPolT<MIX, false, InT>;  // the loads of the u32 fragment scatter (keys only, non-temporal)
  constexpr uint32_t D = PK_DIGITS, NTH = CL_NTH, IPT = CL_IPT, TILE = NTH * IPT;
  constexpr uint32_t FB = PK_FRAG_BITS, FMASK = (1u << FB) - 1, CF = PK_CHUNK_FRAGS, CW = PK_CHUNK_WORDS;
  static_assert(D == NTH, "packed scatter: one thread per digit");
  uint32_t *cnt = reinterpret_cast<uint32_t *>(smem);  // tile rank counters
  uint32_t *info = cnt + D;                            // run start (14 bits) | first chunk << 14 | carry length << 25
  CurT *wbq = reinterpret_cast<CurT *>(info + D);      // claimed position of the digit's chunk 0 minus 8 * first chunk
  CurT *send = wbq + D;                                // slice ends
  uint16_t *cmap = reinterpret_cast<uint16_t *>(send + D);  // digit of every chunk the tile flushes
  uint32_t *wave = reinterpret_cast<uint32_t *>(cmap + PK_MAP);
  uint32_t *val = wave + 16;                           // the staged tile: fragment | digit << 20
  uint32_t *carry = val + TILE;                        // carry[s * D + digit], s < 24
  const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wid = t / WAVE;
  RoundMap om;  // output slot map, decided by the layout kernel (RoundMap)
  if (roundMeta) {
    om.lp = roundMeta[0];
    om.lv = roundMeta[1];
    om.lns = roundMeta[2];
  }
  const size_t grp = (size_t)(blockIdx.x % NGROUPS) * F;
  gcur += grp;
  cnt[t] = 0;
  send[t] = t < F ? gend[grp + t] : (CurT)0;
  __syncthreads();
  const uint64_t begin = (uint64_t)blockIdx.x * tpb * PART_TILE;
  const uint64_t end = min(n, begin + (uint64_t)tpb * PART_TILE);
  const uint32_t mask = F - 1;
  uint32_t c = 0;                            // fragments of digit t in the carry
  // The pending carry update, carry[to + j] = val[from + j] for j < count, in
  // one register: from | to << 16 | count << 24.
  uint32_t mv = 0;
  uint32_t tooWide = 0;
  typename Pol::LoadT v[IPT];
  ScatterProf pf;
  auto moveTail = [&]() {
    const uint32_t from = mv & 0xFFFFu, to = (mv >> 16) & 0xFFu, count = mv >> 24;
#pragma unroll 1
    for (uint32_t j = 0; j < count; ++j) carry[(to + j) * D + t] = val[from + j];
  };
  // Next tile into registers, as prefetchTile (indices past the range end read
  // its last element), from a thread index the compiler cannot hoist out of
  // the tile loop: the eight loop-invariant addresses it would otherwise keep
  // (16 VGPRs) pushed the prefetched tile itself into scratch.
  auto prefetch = [&](uint64_t nbase, uint32_t tt) {
    const uint64_t last = end - 1;
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint64_t idx = nbase + (uint64_t)(i * NTH + tt);
      v[i] = Pol::load(in + (idx < last ? idx : last));
    }
  };
  auto tile = [&](auto fullTile, uint64_t base, uint32_t count) {
    constexpr bool FULL = decltype(fullTile)::value;
    pf.start();
    uint32_t tt = t;
    asm volatile("" : "+v"(tt));  // opaque per tile (see prefetch)
    uint32_t r[IPT], sw[IPT];
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint32_t idx = i * NTH + t;
      if (FULL || idx < count) {
        const uint64_t k = mixKey<MIX>(mix, v[i]);
        const uint32_t d = (uint32_t)k & mask;
        const uint64_t f = k >> bits;
        // A fragment above 20 bits is not truncated into one that could match:
        // it is stored saturated and the join's fallback flag is raised.
        const bool wide = (f >> FB) != 0;
        tooWide |= wide ? 1u : 0u;
        r[i] = atomicAdd(&cnt[d], 1u);
        sw[i] = (wide ? FMASK : (uint32_t)f) | (d << FB);
      }
    }
    pf.mark(0);
    ldsBarrier();  // A: counts final; previous tile's write-out done
    pf.mark(1);
    moveTail();  // the previous tile's tail joins the carry (its staged run is still in val)
    const uint32_t nn = cnt[t];
    cnt[t] = 0;
    const uint32_t tot = c + nn, k = tot / CF;
    // One device atomic per digit claims the chunks this tile flushes (0 words
    // when none fills; padding digits add 0 to the trash).
    CurT *const claimAt = tt < F ? gcur + tt : reinterpret_cast<CurT *>(g_scatterTrash) + tt;
    const CurT claim = atomicAdd(claimAt, (CurT)(k * CW));
    pf.mark(2);
    // One scan for both run starts (low half) and first chunks (high half).
    const uint32_t packed = nn | (k << 16);
    const uint32_t incl = waveInclusiveScan<uint32_t>(packed);
    if (lane == WAVE - 1) wave[wid] = incl;
    ldsBarrier();
    uint32_t prefix = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NTH / WAVE; ++w) {
      const uint32_t x = wave[w];
      if (w < (int)wid) prefix += x;
      total += x;
    }
    const uint32_t excl = prefix + incl - packed;
    const uint32_t n0 = excl & 0xFFFFu, k0 = excl >> 16;
    info[t] = n0 | (k0 << 14) | (c << 25);
#pragma unroll 1
    for (uint32_t j = 0; j < k; ++j) cmap[k0 + j] = (uint16_t)t;
    wbq[t] = claim - (CurT)(k0 * CW);
    // The tail that stays: elements [max(24 k, c), tot) of "carry, then run".
    const uint32_t lo = max(k * CF, c);
    mv = (n0 + lo - c) | ((lo - k * CF) << 16) | ((tot - lo) << 24);
    c = tot - k * CF;
    ldsBarrier();  // run starts visible
    // The next tile's loads overlap the staging and the write-out.  (Issued
    // before the scan, as scatterTile's early prefetch does, they do not fit
    // 128 VGPRs next to the scan: half of the loaded tile went to scratch.)
    prefetch(base + TILE, tt);
    pf.mark(3);
    const uint32_t chunks = (uint32_t)__builtin_amdgcn_readfirstlane((int)(total >> 16));
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint32_t idx = i * NTH + t;
      if (FULL || idx < count) r[i] += info[sw[i] >> FB] & 0x3FFFu;
    }
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const uint32_t idx = i * NTH + t;
      if (FULL || idx < count) val[r[i]] = sw[i];
    }
    pf.mark(4);
    ldsBarrier();  // B: staged tile, chunk map and write bases visible
    pf.mark(6);
    // Write-out: chunk q of the tile by lanes 8 q' .. 8 q' + 7 (a wave stores
    // eight whole chunks per instruction); lanes past the last chunk rebuild
    // chunk 0 and store it to the trash.
    const uint32_t w8 = t & (CW - 1);
    for (uint32_t q0 = 0; q0 < chunks; q0 += NTH / CW) {
      const uint32_t q = q0 + t / CW;
      const bool have = q < chunks;
      const uint32_t qq = have ? q : 0;
      const uint32_t d = cmap[qq];
      const uint32_t inf = info[d];
      const uint32_t dn0 = inf & 0x3FFFu, dk0 = (inf >> 14) & 0x7FFu, dc = inf >> 25;
      const uint32_t s0 = ((qq - dk0) * CW + w8) * PK_WORD_FRAGS;
      unsigned long long word = (unsigned long long)PK_WORD_FRAGS << 60;
#pragma unroll
      for (uint32_t e = 0; e < PK_WORD_FRAGS; ++e) {
        const uint32_t s = s0 + e;
        // One LDS read: the carry sits TILE words behind the staged tile.
        const uint32_t f = val[s < dc ? TILE + s * D + d : dn0 + (s - dc)];
        word |= (unsigned long long)(f & FMASK) << (FB * e);
      }
      const CurT pos = wbq[d] + (CurT)(qq * CW + w8);
      const bool ok = have && (pos | (CurT)(CW - 1)) < send[d];  // the whole chunk ends inside the slice
      unsigned long long *p =
          ok ? out + om((uint64_t)pos) : reinterpret_cast<unsigned long long *>(g_scatterTrash) + tt;
      *p = word;
    }
    pf.mark(7);
#ifdef HPCJOIN_SCATTER_PROF
    ++pf.tiles;
#endif
  };
  if (begin < end) prefetch(begin, t);
  for (uint64_t base = begin; base < end; base += TILE) {
    if (base + TILE <= end)
      tile(std::true_type(), base, TILE);
    else
      tile(std::false_type(), base, (uint32_t)(end - base));
  }
  pf.flush();
  __syncthreads();  // the last write-out has read the carry
  moveTail();
  // The tails: one last chunk per digit with a carry, counts per word.
  if (c > 0) {  // only digits < F ever hold fragments
    uint32_t te = t;
    asm volatile("" : "+v"(te));  // recomputed here: kept from the kernel's start it cost a spill across the loop
    const CurT pos = atomicAdd(gcur + te, (CurT)CW);
    if (pos + (CurT)CW <= send[t]) {
#pragma unroll
      for (uint32_t w = 0; w < CW; ++w) {
        const uint32_t have = c > PK_WORD_FRAGS * w ? min(c - PK_WORD_FRAGS * w, PK_WORD_FRAGS) : 0u;
        unsigned long long word = (unsigned long long)have << 60;
#pragma unroll
        for (uint32_t e = 0; e < PK_WORD_FRAGS; ++e)
          if (e < have) word |= (unsigned long long)(carry[(PK_WORD_FRAGS * w + e) * D + t] & FMASK) << (FB * e);
        out[om((uint64_t)pos + w)] = word;
      }
    }
  }
  if (__ballot(tooWide != 0) != 0 && lane == 0) atomicAdd(wideFlag, 1ull);
}

}  // namespace kernels
}  // namespace hpcjoin
