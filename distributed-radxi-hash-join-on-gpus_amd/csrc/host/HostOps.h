// Single-thread host implementations of every device kernel, with the SAME
// data layouts (digit-major block histograms, per-block cursors, per-item
// local cursors, partition begin arrays).  They are the reference CPU path
// of BASELINE config 1 (plumbing, no GPU), and the oracle the GPU kernels are
// tested against.  Build/probe uses the reference's bucket-chained table
// (/root/reference/tasks/BuildProbe.cpp:47-121) rather than the GPU's LDS
// open addressing, so the two paths are independent implementations.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "../kernels/kernels.h"

namespace hpcjoin {
namespace host {

kernels::ZipfParams makeZipf(uint64_t n, double theta);

void generate(data::Tuple *out, uint64_t n, const kernels::GenParams &p);

void netHistogram(const data::Tuple *in, uint64_t n, uint32_t bits, const kernels::PartitionGeometry &g,
                  uint32_t *blockHist, kernels::KeyMix mix = kernels::KeyMix());
void digitTotals(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t blocksPerChunk, uint32_t chunks,
                 uint64_t *totals);
void netCursors(const uint32_t *blockHist, uint32_t F, uint32_t blocks, uint32_t blocksPerChunk,
                const uint64_t *base, uint64_t *cursors);
void netScatter(const data::Tuple *in, uint64_t n, uint32_t bits, uint32_t keyShift,
                const kernels::PartitionGeometry &g, uint32_t blockBegin, uint32_t blockEnd, const uint64_t *cursors,
                void *out, bool wide, kernels::KeyMix mix = kernels::KeyMix(), bool withRids = true);

void localHistogram(const void *in, bool wide, const kernels::LocalItem *items, uint32_t nItems, uint32_t shift,
                    uint32_t bits, uint32_t *itemHist);
void localCursors(const uint32_t *itemHist, const uint32_t *lpItemBegin, uint32_t owned, uint32_t bits,
                  const uint64_t *lpBase, uint64_t *itemCursors, uint64_t *partBegin);
void localScatter(const void *in, bool wide, const kernels::LocalItem *items, uint32_t nItems, uint32_t shift,
                  uint32_t bits, const uint64_t *itemCursors, void *out);

// Bucket-chained build/probe per final partition; returns matches and (when
// a.materialize) writes pairs through a.outPairs / a.outCursor (host memory).
uint64_t buildProbe(const kernels::BPArgs &a);
// Semi / anti joins (twins of kernels/semi_join.hip).  The host walks whole
// partitions: buildProbeMark sets bit s of marks for every outer position s
// whose key occurs on the inner side of its partition; markCompact counts the
// marked (anti: unmarked) positions of the partitions' valid ranges and, with
// out != null, appends their rids (at most outCapacity are written).
void buildProbeMark(const kernels::BPArgs &a, uint64_t *marks);
uint64_t markCompact(const kernels::BPArgs &a, const uint64_t *marks, bool anti, uint64_t *out, uint64_t outCapacity);
// Outer joins (twins of kernels/outer_join.hip).  buildProbeOuter walks whole
// partitions with the bucket-chained table: returns the pairs, written (when
// a.materialize) through a.outPairs / a.outCursor as buildProbe does, and sets
// bit r of marksR / bit s of marksS (each optional, zeroed by the caller) for
// every inner / outer position with a partner.  markCompactPairs appends one
// row {rid, NULL_RID} (innerSide: the partitions of a.R) or {NULL_RID, rid}
// (those of a.S) per unmarked position from out[*cursor] (out may be null;
// rows at or beyond outCapacity are counted, not stored) and returns their
// number.
uint64_t buildProbeOuter(const kernels::BPArgs &a, uint64_t *marksR, uint64_t *marksS);
uint64_t markCompactPairs(const kernels::BPArgs &a, const uint64_t *marks, bool innerSide, ulonglong2 *out,
                          uint64_t *cursor, uint64_t outCapacity);

// Payload rows of semi, anti and outer joins (twins of kernels/kind_rows.hip;
// row shapes: kernels::KindRowShape).  markCompactRows appends one row per
// marked (anti: unmarked) position of the partitions of a.S (InnerPad: of a.R)
// from out row *cursor, as markCompactPairs does; ridRows writes
// out[i] = {rids[i], rows[rids[i] - rowOffset]}; pairRows writes the 10-word
// row of every pair, a NULL_RID side as five NULL_RID words (no row is read
// for it).
uint64_t markCompactRows(const kernels::BPArgs &a, const uint64_t *marks, bool anti, kernels::KindRowShape shape,
                         const uint64_t *rows, uint64_t rowOffset, uint64_t *out, uint64_t *cursor,
                         uint64_t outCapacity);
void ridRows(const uint64_t *rids, uint64_t n, const uint64_t *rows, uint64_t rowOffset, uint64_t *out);
void pairRows(const ulonglong2 *pairs, uint64_t n, const uint64_t *rowsA, uint64_t offA, const uint64_t *rowsB,
              uint64_t offB, uint64_t *out);

// Set-semantics bitmap join (twins of kernels::bitmapSemiCount / bitmapSemiRids)
// over exactly partitioned sides: partition p holds elements [begin[p],
// begin[p + 1]).  Inner: u32 fragments; outer: u32 fragments (count) or 8-byte
// words fragment << keyShift | rid (rids: the rid of every hit, anti: miss, is
// appended to out, which holds one slot per outer element).  Returns the
// BM_FLAG_* raised (an inner fragment >= 2^bits: BM_FLAG_DUP; repeats are no
// error); outer fragments beyond the range are misses.
struct BitmapSemiResult {
  uint64_t hits = 0, misses = 0, written = 0;
  uint32_t flags = 0;
};
BitmapSemiResult bitmapSemiCount(const uint32_t *r, const uint64_t *rBegin, const uint32_t *s, const uint64_t *sBegin,
                                 uint32_t partitions, uint32_t bits);
BitmapSemiResult bitmapSemiRids(const uint32_t *r, const uint64_t *rBegin, const uint64_t *s, const uint64_t *sBegin,
                                uint32_t partitions, uint32_t keyShift, uint32_t bits, bool anti, uint64_t *out);
// Group joins (twins of kernels::bpGroup / groupEmit).  buildProbeGroup walks
// whole partitions: accCount[r] of every position r of the partitioned inner
// buffer (zeroed by the caller) becomes the number of outer tuples with r's
// key, and accAgg[c * accSlots + r] (column-major; set here to every column's
// identity first; untouched when cols.n == 0) the aggregate of column c over
// them; returns the pairs (the sum of the counts).  Typed columns (cols.dtype)
// are widened as the kernel does -- int32 sign-extended, float32 to binary64 --
// and float columns aggregate as binary64 in sequential order.
// groupEmit writes one row (rid, count, agg_0, ..., agg_{columns-1}) per inner
// position of every partition (out may be null; rows at or beyond outCapacity
// are counted, not stored), stores their number in *rows and returns the
// groups with count 0.
uint64_t buildProbeGroup(const kernels::BPArgs &a, const kernels::GroupColumns &cols, uint32_t *accCount,
                         uint64_t *accAgg, uint64_t accSlots);
uint64_t groupEmit(const kernels::BPArgs &a, const uint32_t *accCount, const uint64_t *accAgg, uint64_t accSlots,
                   uint32_t columns, uint64_t *out, uint64_t outCapacity, uint64_t *rows);

// Wire codec (kernels.h, WireCodec) over host segment lists.
void wirePack(const uint64_t *raw, uint64_t *wire, const kernels::WireSeg *segs, uint32_t nSegs,
              const kernels::WireCodec &c);
void wireUnpack(const uint64_t *wire, uint64_t *raw, const kernels::WireSeg *segs, uint32_t nSegs,
                const kernels::WireCodec &c);

uint64_t npjJoin(const data::Tuple *R, uint64_t nR, const data::Tuple *S, uint64_t nS);
// (inner rid, outer rid) of every match, outer order, inner copies in input order.
std::vector<std::pair<uint64_t, uint64_t>> npjPairs(const data::Tuple *R, uint64_t nR, const data::Tuple *S,
                                                    uint64_t nS);

}  // namespace host
}  // namespace hpcjoin
