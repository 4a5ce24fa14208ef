// Unit geometry, selection and rid access of the mark/compact kernels
// (semi_join.hip: markCount / markPlace; kind_rows.hip: markPlaceRows).
// Device-side, header-only.
#pragma once

#include "kernels.h"
#include "device_common.h"

namespace hpcjoin {
namespace kernels {

enum MarkLayout : int { MK_COMPRESSED = 0, MK_SPLIT = 1, MK_WIDE = 2 };

static inline int markLayout(const BPArgs &a) { return a.wide ? MK_WIDE : a.split ? MK_SPLIT : MK_COMPRESSED; }

// Positions [ub, ue) of unit u (ue > ub: units are emitted for non-empty runs only).
__device__ __forceinline__ void unitRange(const BPArgs &a, const MarkUnit u, uint64_t &ub, uint64_t &ue) {
  ub = a.partS[u.part] + (uint64_t)u.chunk * a.sChunk;
  ue = min(a.partSEnd[u.part], ub + a.sChunk);
}

// Selected positions of mark word w within [ub, ue): marked (semi) or unmarked (anti).
__device__ __forceinline__ unsigned long long unitSelect(const unsigned long long *__restrict__ marks, uint64_t w,
                                                         uint64_t ub, uint64_t ue, bool anti) {
  unsigned long long valid = ~0ull;
  if (w == (ub >> 6)) valid &= ~0ull << (ub & 63);
  if (w == ((ue - 1) >> 6)) valid &= ~0ull >> (63 - ((ue - 1) & 63));
  const unsigned long long m = marks[w];
  return (anti ? ~m : m) & valid;
}

template <int LAYOUT>
__device__ __forceinline__ unsigned long long markRid(const BPArgs &a, uint64_t pos, uint64_t ridMask) {
  if constexpr (LAYOUT == MK_SPLIT)
    return reinterpret_cast<const uint32_t *>(a.S)[pos];
  else if constexpr (LAYOUT == MK_COMPRESSED)
    return reinterpret_cast<const unsigned long long *>(a.S)[pos] & ridMask;
  else
    return reinterpret_cast<const unsigned long long *>(a.S)[2 * pos + 1];
}

}  // namespace kernels
}  // namespace hpcjoin
