#include "HostOps.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <unordered_set>

#include "../utils/Debug.h"

namespace hpcjoin {
namespace host {

using kernels::KeyDistribution;

// ------------------------------------------------------------------ datagen
static double zeta(uint64_t n, double theta) {
  // Exact for small n, Euler-Maclaurin tail beyond 2^20 terms.
  const uint64_t m = std::min<uint64_t>(n, 1u << 20);
  double s = 0;
  for (uint64_t i = 1; i <= m; ++i) s += std::pow((double)i, -theta);
  if (n > m) {
    const double a = (double)m, b = (double)n;
    // integral_a^b x^-t dx + (f(b) - f(a))/2 - (f'(b) - f'(a))/12
    s += (std::pow(b, 1 - theta) - std::pow(a, 1 - theta)) / (1 - theta);
    s += (std::pow(b, -theta) - std::pow(a, -theta)) / 2;
    s += (-theta * std::pow(b, -theta - 1) + theta * std::pow(a, -theta - 1)) / 12;
  }
  return s;
}

kernels::ZipfParams makeZipf(uint64_t n, double theta) {
  JOIN_ASSERT(n >= 2, "Zipf", "domain must be >= 2");
  // Gray et al.'s closed-form inverse is the continuous approximation of
  // sum_{i<=r} i^-theta, valid on both sides of 1 (alpha = 1/(1-theta) < 0
  // above it): ranks 0 and 1 are exact, the rest within ~1% of the mass
  // (tests/test_package.py checks theta 0.99 and 1.1).  theta = 1 has no alpha.
  JOIN_ASSERT(theta > 0 && theta <= 4 && std::fabs(theta - 1.0) >= 1e-3, "Zipf",
              "theta must be in (0,4] and not 1, got %f", theta);
  kernels::ZipfParams z;
  z.n = n;
  z.theta = theta;
  z.alpha = 1.0 / (1.0 - theta);
  z.zetan = zeta(n, theta);
  const double zeta2 = 1.0 + std::pow(2.0, -theta);
  z.eta = (1.0 - std::pow(2.0 / (double)n, 1.0 - theta)) / (1.0 - zeta2 / z.zetan);
  z.half_pow_theta = std::pow(0.5, theta);
  return z;
}

static inline uint64_t zipfRank(const kernels::ZipfParams &z, double u) {
  const double uz = u * z.zetan;
  if (uz < 1.0) return 0;
  if (uz < 1.0 + z.half_pow_theta) return 1;
  uint64_t r = (uint64_t)((double)z.n * std::pow(z.eta * u - z.eta + 1.0, z.alpha));
  return r >= z.n ? z.n - 1 : r;
}

void generate(data::Tuple *out, uint64_t n, const kernels::GenParams &p) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t gi = p.globalOffset + i;
    uint64_t k;
    switch (p.dist) {
      case KeyDistribution::Unique: k = p.keyOffset + p.perm(gi); break;
      case KeyDistribution::Dense: k = p.keyOffset + gi; break;
      case KeyDistribution::Modulo: k = p.keyOffset + p.perm(gi % p.modulo); break;
      case KeyDistribution::Uniform:
        k = p.keyOffset + (uint64_t)(kernels::uniform01(p.seed, gi) * (double)p.domain) % p.domain;
        break;
      default: k = p.keyOffset + p.perm(zipfRank(p.zipf, kernels::uniform01(p.seed, gi))); break;
    }
    if (p.tpchSparse) k = kernels::tpchSparseKey(k);
    out[i].key = p.sparse64 ? kernels::sparseKey(k) : k;
    out[i].rid = p.ridOffset + i;
  }
}

// ------------------------------------------------------------ pass 1 (host)
void netHistogram(const data::Tuple *in, uint64_t n, uint32_t bits, const kernels::PartitionGeometry &g,
                  uint32_t *blockHist, kernels::KeyMix mix) {
  const uint32_t F = 1u << bits;
  const uint64_t mask = F - 1;
  std::memset(blockHist, 0, sizeof(uint32_t) * F * g.blocks);
  for (uint32_t b = 0; b < g.blocks; ++b) {
    const uint64_t begin = (uint64_t)b * g.tuplesPerBlock(), end = std::min(n, begin + g.tuplesPerBlock());
    for (uint64_t i = begin; i < end; ++i) blockHist[(mix.apply(in[i].key) & mask) * g.blocks + b]++;
  }
}

void digitTotals(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t bpc, uint32_t chunks,
                 uint64_t *totals) {
  for (uint32_t c = 0; c < chunks; ++c)
    for (uint32_t d = 0; d < F; ++d) {
      uint64_t s = 0;
      for (uint32_t b = c * bpc; b < std::min(blocks, (c + 1) * bpc); ++b) s += blockHist[(uint64_t)d * blocks + b];
      totals[(uint64_t)c * F + d] = s;
    }
}

void netCursors(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t bpc, const uint64_t *base,
                uint64_t *cursors) {
  const uint32_t chunks = (blocks + bpc - 1) / bpc;
  for (uint32_t d = 0; d < F; ++d)
    for (uint32_t c = 0; c < chunks; ++c) {
      uint64_t run = base[(uint64_t)c * F + d];
      for (uint32_t b = c * bpc; b < std::min(blocks, (c + 1) * bpc); ++b) {
        cursors[(uint64_t)d * blocks + b] = run;
        run += blockHist[(uint64_t)d * blocks + b];
      }
    }
}

void netScatter(const data::Tuple *in, uint64_t n, uint32_t bits, uint32_t keyShift,
                const kernels::PartitionGeometry &g, uint32_t blockBegin, uint32_t blockEnd, const uint64_t *cursors,
                void *out, bool wide, kernels::KeyMix mix, bool withRids) {
  const uint32_t F = 1u << bits;
  const uint64_t ridMask = withRids ? ~0ull : 0ull;
  const uint64_t mask = F - 1;
  std::vector<uint64_t> cur(F);
  for (uint32_t b = blockBegin; b < blockEnd; ++b) {
    for (uint32_t d = 0; d < F; ++d) cur[d] = cursors[(uint64_t)d * g.blocks + b];
    const uint64_t begin = (uint64_t)b * g.tuplesPerBlock(), end = std::min(n, begin + g.tuplesPerBlock());
    for (uint64_t i = begin; i < end; ++i) {
      const uint64_t key = mix.apply(in[i].key);
      const uint64_t d = key & mask;
      if (wide)
        static_cast<data::Tuple *>(out)[cur[d]++] = data::Tuple{key, in[i].rid};
      else
        static_cast<uint64_t *>(out)[cur[d]++] = (in[i].rid & ridMask) | ((key >> bits) << keyShift);
    }
  }
}

// ------------------------------------------------------------ pass 2 (host)
static inline uint64_t word(const void *in, bool wide, uint64_t i) {
  return wide ? static_cast<const data::Tuple *>(in)[i].key : static_cast<const uint64_t *>(in)[i];
}

void localHistogram(const void *in, bool wide, const kernels::LocalItem *items, uint32_t nItems, uint32_t shift,
                    uint32_t bits, uint32_t *itemHist) {
  const uint32_t F = 1u << bits;
  const uint64_t mask = F - 1;
  std::memset(itemHist, 0, sizeof(uint32_t) * (uint64_t)F * nItems);
  for (uint32_t it = 0; it < nItems; ++it)
    for (uint64_t i = items[it].begin; i < items[it].begin + items[it].len; ++i)
      itemHist[(uint64_t)it * F + ((word(in, wide, i) >> shift) & mask)]++;
}

void localCursors(const uint32_t *itemHist, const uint32_t *lpItemBegin, uint32_t owned, uint32_t bits,
                  const uint64_t *lpBase, uint64_t *itemCursors, uint64_t *partBegin) {
  const uint32_t F = 1u << bits;
  for (uint32_t lp = 0; lp < owned; ++lp) {
    uint64_t run = lpBase[lp];
    for (uint32_t q = 0; q < F; ++q) {
      partBegin[(uint64_t)lp * F + q] = run;
      for (uint32_t it = lpItemBegin[lp]; it < lpItemBegin[lp + 1]; ++it) {
        itemCursors[(uint64_t)it * F + q] = run;
        run += itemHist[(uint64_t)it * F + q];
      }
    }
  }
  if (owned) partBegin[(uint64_t)owned * F] = lpBase[owned];
}

void localScatter(const void *in, bool wide, const kernels::LocalItem *items, uint32_t nItems, uint32_t shift,
                  uint32_t bits, const uint64_t *itemCursors, void *out) {
  const uint32_t F = 1u << bits;
  const uint64_t mask = F - 1;
  std::vector<uint64_t> cur(F);
  for (uint32_t it = 0; it < nItems; ++it) {
    for (uint32_t q = 0; q < F; ++q) cur[q] = itemCursors[(uint64_t)it * F + q];
    for (uint64_t i = items[it].begin; i < items[it].begin + items[it].len; ++i) {
      const uint64_t q = (word(in, wide, i) >> shift) & mask;
      if (wide)
        static_cast<data::Tuple *>(out)[cur[q]++] = static_cast<const data::Tuple *>(in)[i];
      else
        static_cast<uint64_t *>(out)[cur[q]++] = static_cast<const uint64_t *>(in)[i];
    }
  }
}

// --------------------------------------------------------------- build/probe
static inline uint64_t nextPow2(uint64_t x) {  // 64-bit (reference NEXT_POW_2 was 32-bit only)
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

uint64_t buildProbe(const kernels::BPArgs &a) {
  uint64_t matches = 0;
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  std::vector<uint64_t> bucket, next;
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t rb = a.partR[p], re = a.partREnd ? a.partREnd[p] : a.partR[p + 1], sb = a.partS[p],
                   se = a.partSEnd ? a.partSEnd[p] : a.partS[p + 1];
    const uint64_t nr = re - rb;
    if (nr == 0 || se == sb) continue;
    const uint64_t N = nextPow2(nr);
    bucket.assign(N, 0);
    next.assign(nr, 0);
    if (!a.wide) {
      const uint64_t *R = static_cast<const uint64_t *>(a.R) + rb;
      const uint64_t *S = static_cast<const uint64_t *>(a.S);
      const uint64_t mask = (N - 1) << a.fragShift;
      for (uint64_t t = 0; t < nr; ++t) {
        const uint64_t idx = (a.fragShift >= 64) ? 0 : ((R[t] & mask) >> a.fragShift);
        next[t] = bucket[idx];
        bucket[idx] = t + 1;
      }
      for (uint64_t s = sb; s < se; ++s) {
        const uint64_t v = S[s];
        const uint64_t idx = (a.fragShift >= 64) ? 0 : ((v & mask) >> a.fragShift);
        for (uint64_t hit = bucket[idx]; hit > 0; hit = next[hit - 1]) {
          if ((R[hit - 1] >> a.keyShift) == (v >> a.keyShift)) {
            ++matches;
            if (a.materialize) {
              const unsigned long long pos = (*a.outCursor)++;
              if (pos < a.outCapacity) a.outPairs[pos] = make_ulonglong2(R[hit - 1] & ridMask, v & ridMask);
            }
          }
        }
      }
    } else {
      const data::Tuple *R = static_cast<const data::Tuple *>(a.R) + rb;
      const data::Tuple *S = static_cast<const data::Tuple *>(a.S);
      for (uint64_t t = 0; t < nr; ++t) {
        const uint64_t idx = kernels::mix64(R[t].key) & (N - 1);
        next[t] = bucket[idx];
        bucket[idx] = t + 1;
      }
      for (uint64_t s = sb; s < se; ++s) {
        const uint64_t idx = kernels::mix64(S[s].key) & (N - 1);
        for (uint64_t hit = bucket[idx]; hit > 0; hit = next[hit - 1])
          if (R[hit - 1].key == S[s].key) {
            ++matches;
            if (a.materialize) {
              const unsigned long long pos = (*a.outCursor)++;
              if (pos < a.outCapacity) a.outPairs[pos] = make_ulonglong2(R[hit - 1].rid, S[s].rid);
            }
          }
      }
    }
  }
  return matches;
}

void buildProbeMark(const kernels::BPArgs &a, uint64_t *marks) {
  std::unordered_set<uint64_t> keys;
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t rb = a.partR[p], re = a.partREnd ? a.partREnd[p] : a.partR[p + 1], sb = a.partS[p],
                   se = a.partSEnd ? a.partSEnd[p] : a.partS[p + 1];
    if (re == rb || se == sb) continue;
    keys.clear();
    keys.reserve(2 * (re - rb));
    if (!a.wide) {
      const uint64_t *R = static_cast<const uint64_t *>(a.R), *S = static_cast<const uint64_t *>(a.S);
      for (uint64_t t = rb; t < re; ++t) keys.insert(a.keyShift >= 64 ? 0 : R[t] >> a.keyShift);
      for (uint64_t s = sb; s < se; ++s)
        if (keys.count(a.keyShift >= 64 ? 0 : S[s] >> a.keyShift)) marks[s >> 6] |= 1ull << (s & 63);
    } else {
      const data::Tuple *R = static_cast<const data::Tuple *>(a.R), *S = static_cast<const data::Tuple *>(a.S);
      for (uint64_t t = rb; t < re; ++t) keys.insert(R[t].key);
      for (uint64_t s = sb; s < se; ++s)
        if (keys.count(S[s].key)) marks[s >> 6] |= 1ull << (s & 63);
    }
  }
}

uint64_t markCompact(const kernels::BPArgs &a, const uint64_t *marks, bool anti, uint64_t *out,
                     uint64_t outCapacity) {
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  uint64_t n = 0;
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t sb = a.partS[p], se = a.partSEnd ? a.partSEnd[p] : a.partS[p + 1];
    for (uint64_t s = sb; s < se; ++s) {
      const bool marked = (marks[s >> 6] >> (s & 63)) & 1;
      if (marked == anti) continue;
      if (out && n < outCapacity)
        out[n] = a.wide ? static_cast<const data::Tuple *>(a.S)[s].rid : (static_cast<const uint64_t *>(a.S)[s] & ridMask);
      ++n;
    }
  }
  return n;
}

uint64_t buildProbeOuter(const kernels::BPArgs &a, uint64_t *marksR, uint64_t *marksS) {
  uint64_t pairs = 0;
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  std::vector<uint64_t> bucket, next;
  auto key = [&](const void *base, uint64_t i) -> uint64_t {
    if (a.wide) return static_cast<const data::Tuple *>(base)[i].key;
    return a.keyShift >= 64 ? 0ull : static_cast<const uint64_t *>(base)[i] >> a.keyShift;
  };
  auto rid = [&](const void *base, uint64_t i) -> uint64_t {
    return a.wide ? static_cast<const data::Tuple *>(base)[i].rid : (static_cast<const uint64_t *>(base)[i] & ridMask);
  };
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t rb = a.partR[p], re = a.partREnd ? a.partREnd[p] : a.partR[p + 1], sb = a.partS[p],
                   se = a.partSEnd ? a.partSEnd[p] : a.partS[p + 1];
    const uint64_t nr = re - rb;
    if (nr == 0 || se == sb) continue;  // one-sided partitions: nothing is marked
    const uint64_t N = nextPow2(nr);
    bucket.assign(N, 0);
    next.assign(nr, 0);
    for (uint64_t t = 0; t < nr; ++t) {
      const uint64_t idx = kernels::mix64(key(a.R, rb + t)) & (N - 1);
      next[t] = bucket[idx];
      bucket[idx] = t + 1;
    }
    for (uint64_t s = sb; s < se; ++s) {
      const uint64_t k = key(a.S, s);
      bool any = false;
      for (uint64_t hit = bucket[kernels::mix64(k) & (N - 1)]; hit > 0; hit = next[hit - 1]) {
        const uint64_t r = rb + hit - 1;
        if (key(a.R, r) != k) continue;
        any = true;
        ++pairs;
        if (marksR) marksR[r >> 6] |= 1ull << (r & 63);
        if (a.materialize) {
          const unsigned long long pos = (*a.outCursor)++;
          if (pos < a.outCapacity) a.outPairs[pos] = make_ulonglong2(rid(a.R, r), rid(a.S, s));
        }
      }
      if (any && marksS) marksS[s >> 6] |= 1ull << (s & 63);
    }
  }
  return pairs;
}

uint64_t markCompactPairs(const kernels::BPArgs &a, const uint64_t *marks, bool innerSide, ulonglong2 *out,
                          uint64_t *cursor, uint64_t outCapacity) {
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  const void *base = innerSide ? a.R : a.S;
  const uint64_t *pb = innerSide ? a.partR : a.partS, *pe = innerSide ? a.partREnd : a.partSEnd;
  uint64_t n = 0;
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t b = pb[p], e = pe ? pe[p] : pb[p + 1];
    for (uint64_t i = b; i < e; ++i) {
      if ((marks[i >> 6] >> (i & 63)) & 1) continue;
      const uint64_t rid =
          a.wide ? static_cast<const data::Tuple *>(base)[i].rid : (static_cast<const uint64_t *>(base)[i] & ridMask);
      const uint64_t at = (*cursor)++;
      if (out && at < outCapacity)
        out[at] = innerSide ? make_ulonglong2(rid, kernels::NULL_RID) : make_ulonglong2(kernels::NULL_RID, rid);
      ++n;
    }
  }
  return n;
}

uint64_t markCompactRows(const kernels::BPArgs &a, const uint64_t *marks, bool anti, kernels::KindRowShape shape,
                         const uint64_t *rows, uint64_t rowOffset, uint64_t *out, uint64_t *cursor,
                         uint64_t outCapacity) {
  using kernels::KindRowShape;
  using kernels::NULL_RID;
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  const bool innerSide = shape == KindRowShape::InnerPad;
  const void *base = innerSide ? a.R : a.S;
  const uint64_t *pb = innerSide ? a.partR : a.partS, *pe = innerSide ? a.partREnd : a.partSEnd;
  const uint32_t W = kernels::kindRowWords(shape);
  uint64_t n = 0;
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t b = pb[p], e = pe ? pe[p] : pb[p + 1];
    for (uint64_t i = b; i < e; ++i) {
      const bool marked = (marks[i >> 6] >> (i & 63)) & 1;
      if (marked == anti) continue;
      const uint64_t rid =
          a.wide ? static_cast<const data::Tuple *>(base)[i].rid : (static_cast<const uint64_t *>(base)[i] & ridMask);
      const uint64_t at = (*cursor)++;
      ++n;
      if (!out || at >= outCapacity) continue;
      uint64_t *o = out + at * W;
      const uint64_t *row = rows + (rid - rowOffset) * kernels::ROW_WORDS;
      if (shape == KindRowShape::Rid) {
        o[0] = rid;
        std::copy(row, row + kernels::ROW_WORDS, o + 1);
      } else {
        o[0] = innerSide ? rid : NULL_RID;
        o[1] = innerSide ? NULL_RID : rid;
        std::copy(row, row + kernels::ROW_WORDS, o + (innerSide ? 2 : 6));
        std::fill(o + (innerSide ? 6 : 2), o + (innerSide ? 10 : 6), (uint64_t)NULL_RID);
      }
    }
  }
  return n;
}

void ridRows(const uint64_t *rids, uint64_t n, const uint64_t *rows, uint64_t rowOffset, uint64_t *out) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t *row = rows + (rids[i] - rowOffset) * kernels::ROW_WORDS;
    out[i * kernels::RID_ROW_WORDS] = rids[i];
    std::copy(row, row + kernels::ROW_WORDS, out + i * kernels::RID_ROW_WORDS + 1);
  }
}

void pairRows(const ulonglong2 *pairs, uint64_t n, const uint64_t *rowsA, uint64_t offA, const uint64_t *rowsB,
              uint64_t offB, uint64_t *out) {
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t *o = out + i * kernels::PAIR_ROW_WORDS;
    o[0] = pairs[i].x;
    o[1] = pairs[i].y;
    const uint64_t rid[2] = {pairs[i].x, pairs[i].y}, off[2] = {offA, offB};
    const uint64_t *cols[2] = {rowsA, rowsB};
    for (int s = 0; s < 2; ++s) {
      uint64_t *dst = o + 2 + s * kernels::ROW_WORDS;
      if (rid[s] == kernels::NULL_RID) {
        std::fill(dst, dst + kernels::ROW_WORDS, (uint64_t)kernels::NULL_RID);
      } else {
        const uint64_t *row = cols[s] + (rid[s] - off[s]) * kernels::ROW_WORDS;
        std::copy(row, row + kernels::ROW_WORDS, dst);
      }
    }
  }
}

// One partition's set bitmap over the whole planned range (the device kernels
// split 21-bit ranges over two workgroups; the host needs no pieces).
namespace {
template <typename E, typename Emit>
BitmapSemiResult bitmapSemi(const uint32_t *r, const uint64_t *rBegin, const E *s, const uint64_t *sBegin,
                            uint32_t partitions, uint32_t keyShift, uint32_t bits, Emit &&emit) {
  BitmapSemiResult o;
  const uint64_t range = (uint64_t)kernels::bitmapWords(std::min(bits, kernels::BITMAP_MAX_BITS)) * 32
                         << (bits > kernels::BITMAP_MAX_BITS ? bits - kernels::BITMAP_MAX_BITS : 0);  // as the kernels
  std::vector<uint64_t> bm((size_t)((range + 63) / 64));
  for (uint32_t p = 0; p < partitions; ++p) {
    std::fill(bm.begin(), bm.end(), 0);
    for (uint64_t i = rBegin[p]; i < rBegin[p + 1]; ++i) {
      const uint64_t f = r[i];
      if (f >= range)
        o.flags |= kernels::BM_FLAG_DUP;  // outside the planned range: the plan does not hold
      else
        bm[f >> 6] |= 1ull << (f & 63);
    }
    for (uint64_t i = sBegin[p]; i < sBegin[p + 1]; ++i) {
      const uint64_t f = (uint64_t)s[i] >> keyShift;
      const bool hit = f < range && ((bm[f >> 6] >> (f & 63)) & 1ull);
      ++(hit ? o.hits : o.misses);
      emit(o, s[i], hit);
    }
  }
  return o;
}
}  // namespace

BitmapSemiResult bitmapSemiCount(const uint32_t *r, const uint64_t *rBegin, const uint32_t *s, const uint64_t *sBegin,
                                 uint32_t partitions, uint32_t bits) {
  return bitmapSemi(r, rBegin, s, sBegin, partitions, 0, bits, [](BitmapSemiResult &, uint32_t, bool) {});
}

BitmapSemiResult bitmapSemiRids(const uint32_t *r, const uint64_t *rBegin, const uint64_t *s, const uint64_t *sBegin,
                                uint32_t partitions, uint32_t keyShift, uint32_t bits, bool anti, uint64_t *out) {
  const uint64_t ridMask = (1ull << keyShift) - 1;
  return bitmapSemi(r, rBegin, s, sBegin, partitions, keyShift, bits, [&](BitmapSemiResult &o, uint64_t w, bool hit) {
    if (hit != anti) out[o.written++] = w & ridMask;
  });
}

uint64_t buildProbeGroup(const kernels::BPArgs &a, const kernels::GroupColumns &cols, uint32_t *accCount,
                         uint64_t *accAgg, uint64_t accSlots) {
  uint64_t pairs = 0;
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  for (uint32_t c = 0; c < cols.n; ++c)
    std::fill(accAgg + c * accSlots, accAgg + (c + 1) * accSlots,
              (uint64_t)kernels::groupAggIdentity(cols.agg[c], cols.dtype[c]));
  // Column c's value of a row, widened to the accumulator's word: int32 sign-extended, float32 as binary64 bits.
  auto load = [&](uint32_t c, uint64_t row) -> uint64_t {
    const uint64_t idx = row * cols.stride[c];
    switch (cols.dtype[c]) {
      case kernels::GROUP_I32: return (uint64_t)(int64_t) static_cast<const int32_t *>(cols.col[c])[idx];
      case kernels::GROUP_F32: {
        const double d = (double)static_cast<const float *>(cols.col[c])[idx];
        uint64_t bits;
        std::memcpy(&bits, &d, 8);
        return bits;
      }
      default: return static_cast<const uint64_t *>(cols.col[c])[idx];
    }
  };
  std::vector<uint64_t> bucket, next, rep;
  auto key = [&](const void *base, uint64_t i) -> uint64_t {
    if (a.wide) return static_cast<const data::Tuple *>(base)[i].key;
    return a.keyShift >= 64 ? 0ull : static_cast<const uint64_t *>(base)[i] >> a.keyShift;
  };
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t rb = a.partR[p], re = a.partREnd ? a.partREnd[p] : a.partR[p + 1], sb = a.partS[p],
                   se = a.partSEnd ? a.partSEnd[p] : a.partS[p + 1];
    const uint64_t nr = re - rb;
    if (nr == 0 || se == sb) continue;  // one-sided partitions: count 0, every aggregate its identity
    const uint64_t N = nextPow2(nr);
    bucket.assign(N, 0);
    next.assign(nr, 0);
    rep.assign(nr, 0);  // the first inner tuple of each key aggregates for its copies
    for (uint64_t t = 0; t < nr; ++t) {
      const uint64_t k = key(a.R, rb + t), idx = kernels::mix64(k) & (N - 1);
      rep[t] = t;
      for (uint64_t hit = bucket[idx]; hit > 0; hit = next[hit - 1])
        if (key(a.R, rb + hit - 1) == k) {
          rep[t] = rep[hit - 1];
          break;
        }
      next[t] = bucket[idx];
      bucket[idx] = t + 1;
    }
    for (uint64_t s = sb; s < se; ++s) {
      const uint64_t k = key(a.S, s);
      for (uint64_t hit = bucket[kernels::mix64(k) & (N - 1)]; hit > 0; hit = next[hit - 1]) {
        if (key(a.R, rb + hit - 1) != k) continue;
        const uint64_t r = rb + rep[hit - 1];
        ++accCount[r];
        const uint64_t rid =
            a.wide ? static_cast<const data::Tuple *>(a.S)[s].rid : (static_cast<const uint64_t *>(a.S)[s] & ridMask);
        for (uint32_t c = 0; c < cols.n; ++c) {
          const uint64_t v = load(c, rid - cols.offset);
          uint64_t &acc = accAgg[c * accSlots + r];
          if (kernels::groupDtypeIsFloat(cols.dtype[c])) {  // binary64 on the bits, in sequential order
            double x, y;
            std::memcpy(&x, &acc, 8);
            std::memcpy(&y, &v, 8);
            x = cols.agg[c] == kernels::GROUP_MIN ? std::fmin(x, y) : cols.agg[c] == kernels::GROUP_MAX ? std::fmax(x, y) : x + y;
            std::memcpy(&acc, &x, 8);
          } else if (cols.agg[c] == kernels::GROUP_MIN)
            acc = (uint64_t)std::min((int64_t)acc, (int64_t)v);
          else if (cols.agg[c] == kernels::GROUP_MAX)
            acc = (uint64_t)std::max((int64_t)acc, (int64_t)v);
          else
            acc += v;
        }
        break;
      }
    }
    for (uint64_t t = 0; t < nr; ++t) {  // copies take their key's totals; every tuple adds its count to the pairs
      if (rep[t] != t) {
        accCount[rb + t] = accCount[rb + rep[t]];
        for (uint32_t c = 0; c < cols.n; ++c) accAgg[c * accSlots + rb + t] = accAgg[c * accSlots + rb + rep[t]];
      }
      pairs += accCount[rb + t];
    }
  }
  return pairs;
}

uint64_t groupEmit(const kernels::BPArgs &a, const uint32_t *accCount, const uint64_t *accAgg, uint64_t accSlots,
                   uint32_t columns, uint64_t *out, uint64_t outCapacity, uint64_t *rows) {
  const uint64_t ridMask = a.keyShift >= 64 ? ~0ull : ((1ull << a.keyShift) - 1);
  const uint64_t W = 2 + columns;
  uint64_t n = 0, zeros = 0;
  for (uint32_t p = 0; p < a.P; ++p) {
    const uint64_t b = a.partR[p], e = a.partREnd ? a.partREnd[p] : a.partR[p + 1];
    for (uint64_t i = b; i < e; ++i) {
      zeros += accCount[i] == 0;
      if (out && n < outCapacity) {
        out[n * W] = a.wide ? static_cast<const data::Tuple *>(a.R)[i].rid : (static_cast<const uint64_t *>(a.R)[i] & ridMask);
        out[n * W + 1] = accCount[i];
        for (uint32_t c = 0; c < columns; ++c) out[n * W + 2 + c] = accAgg[c * accSlots + i];
      }
      ++n;
    }
  }
  if (rows) *rows = n;
  return zeros;
}

uint64_t npjJoin(const data::Tuple *R, uint64_t nR, const data::Tuple *S, uint64_t nS) {
  std::unordered_map<uint64_t, uint64_t> counts;
  counts.reserve(nR * 2);
  for (uint64_t i = 0; i < nR; ++i) counts[R[i].key]++;
  uint64_t m = 0;
  for (uint64_t i = 0; i < nS; ++i) {
    auto it = counts.find(S[i].key);
    if (it != counts.end()) m += it->second;
  }
  return m;
}

std::vector<std::pair<uint64_t, uint64_t>> npjPairs(const data::Tuple *R, uint64_t nR, const data::Tuple *S,
                                                    uint64_t nS) {
  std::unordered_map<uint64_t, std::vector<uint64_t>> rids;
  rids.reserve(nR * 2);
  for (uint64_t i = 0; i < nR; ++i) rids[R[i].key].push_back(R[i].rid);
  std::vector<std::pair<uint64_t, uint64_t>> out;
  for (uint64_t i = 0; i < nS; ++i) {
    auto it = rids.find(S[i].key);
    if (it == rids.end()) continue;
    for (uint64_t r : it->second) out.emplace_back(r, S[i].rid);
  }
  return out;
}

// Wire codec twins: a plain bit-stream writer/reader over each segment's
// groups of 64 (independent of the device's per-lane word assembly).
void wirePack(const uint64_t *raw, uint64_t *wire, const kernels::WireSeg *segs, uint32_t nSegs,
              const kernels::WireCodec &c) {
  const uint64_t wmask = c.w >= 64 ? ~0ull : ((1ull << c.w) - 1);
  for (uint32_t s = 0; s < nSegs; ++s) {
    const kernels::WireSeg &sg = segs[s];
    uint64_t *out = wire + sg.wire;
    std::fill(out, out + c.words(sg.n), 0ull);
    for (uint64_t t = 0; t < sg.n; ++t) {
      const uint64_t e = c.encode(raw[sg.raw + t], sg.base) & wmask;
      const uint64_t bit = (t / 64) * 64 * c.w + (t % 64) * c.w;
      const uint64_t j = bit / 64, o = bit % 64;
      out[j] |= e << o;
      if (o + c.w > 64) out[j + 1] |= e >> (64 - o);
    }
  }
}

void wireUnpack(const uint64_t *wire, uint64_t *raw, const kernels::WireSeg *segs, uint32_t nSegs,
                const kernels::WireCodec &c) {
  const uint64_t wmask = c.w >= 64 ? ~0ull : ((1ull << c.w) - 1);
  for (uint32_t s = 0; s < nSegs; ++s) {
    const kernels::WireSeg &sg = segs[s];
    const uint64_t *in = wire + sg.wire;
    for (uint64_t t = 0; t < sg.n; ++t) {
      const uint64_t bit = (t / 64) * 64 * c.w + (t % 64) * c.w;
      const uint64_t j = bit / 64, o = bit % 64;
      uint64_t e = in[j] >> o;
      if (o + c.w > 64) e |= in[j + 1] << (64 - o);
      raw[sg.raw + t] = c.decode(e & wmask, sg.base);
    }
  }
}

}  // namespace host
}  // namespace hpcjoin
