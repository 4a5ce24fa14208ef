// Build/probe phase.  Reference: /root/reference/tasks/BuildProbe.cpp:47-121
// (host bucket chaining per partition pair) and the GPU offload of
// tasks/gpu/GPUWrapper.cu + operators/gpu/eth.cu (whose result was never
// read back).  Device flow, all stream-ordered:
//   plan counts -> wave64 scan (item count stays on the device) -> emit items
//   -> persistent LDS build/probe kernel -> one 64-bit atomic per workgroup.
// Semi / anti joins (JoinPlan::kind): the same item list -> bpMark (hit masks
// into a bit array over the outer positions) -> markCount over outer units
// -> (materialize) scan -> markPlace writes the outer rids.
// Outer joins: the same item list -> bpOuterCount (per-item pair counts and
// the hit marks of the preserved sides) -> markCount(anti) over the units of
// each preserved side -> (materialize) scans -> the inner join's place pass
// -> markPlacePairs appends the NULL-padded rows (kernels/outer_join.hip).
// Group joins: the same item list -> groupAggInit (the accumulators'
// identities) -> bpGroup (per-slot counters and aggregates in LDS, applied to
// accumulators over the inner positions) -> the inner side's units ->
// (materialize) lengths, scan -> groupEmit writes the rows and counts the
// empty groups (kernels/group_join.hip).
// With a row sink (HashJoin::setKindRowSink, device, N = 1) the place pass of
// those kinds writes payload rows instead: markPlaceRows in place of markPlace
// / markPlacePairs, and for outer kinds over the split layout the inner join's
// fused row kernels for the matched pairs (kernels/kind_rows.hip).
// The host reads the counters once, after the join's single final sync.
#pragma once

#include <vector>

#include "../core/ExecContext.h"
#include "../data/CompressedTuple.h"
#include "../data/Window.h"
#include "../kernels/kernels.h"
#include "Task.h"

namespace hpcjoin {
namespace tasks {

class BuildProbe : public Task {
 public:
  // Reference-compatible: one (inner, outer) partition pair in host memory,
  // reference bit layout (compare value >> 32, hash bits from 37).
  BuildProbe(uint64_t innerPartitionSize, data::CompressedTuple *innerPartition, uint64_t outerPartitionSize,
             data::CompressedTuple *outerPartition);
  BuildProbe(data::Window *innerWindow, data::Window *outerWindow, core::ExecContext *ctx, const core::JoinPlan &plan,
             uint64_t outputCapacity);
  ~BuildProbe();

  void execute();
  task_type_t getType() { return TASK_BUILD_PROBE; }

  // After the caller synchronised the streams: pull the counters; returns
  // true if the work-item list or the output buffer overflowed and
  // execute() must run again (it then sizes both exactly).
  bool collect();

 private:
  void readBackCounters();

 public:
  uint64_t getMatches() const { return matches; }
  uint64_t getOutputCount() const { return outputCount; }
  uint32_t getWorkItems() const { return workItems; }
  // Outer kinds: getMatches() = pairs + unmatched tuples of the preserved sides.
  uint64_t getMatchedPairs() const { return matchedPairs; }
  uint64_t getUnmatchedInner() const { return unmatchedInner; }
  uint64_t getUnmatchedOuter() const { return unmatchedOuter; }
  const ulonglong2 *getOutput() const { return outPairs; }
  // kind != Inner, materialize: getOutputCount() outer rids (null otherwise).
  const uint64_t *getOutputRids() const { return outRids; }
  // kind Group, materialize: getOutputCount() rows (rid, count, agg_0, ...) of
  // 2 + C words for C aggregated columns (null otherwise).
  const uint64_t *getOutputGroups() const { return outGroups; }
  // kind Group: aggregate cols.n outer value columns per group (kernels::GroupColumns; the columns cover this
  // rank's outer rids; null = counts only).  The rows are then (rid, count, agg_0, ...): 2 + cols.n words.
  void setGroupColumns(const kernels::GroupColumns *cols) { groupColumns = cols; }
  bool outputOverflowed() const { return overflowOut; }
  // Fused row output (device, split layout): the materialize pass writes whole
  // rows to the sink.  A sink overflow is reported, not re-run (the caller
  // owns the buffer).  Semi / anti and outer kinds (device): the place pass
  // writes their payload rows to the sink (kernels::markPlaceRows) and no rid
  // or pair list is kept.
  void setRowSink(const kernels::RowSink *s) { sink = s; }
  // Pairs go to this pinned host buffer (JoinConfig::outputHost, outputCapacity
  // pairs); an overflow is reported, not re-run.
  void setHostOutput(void *host) { hostOut = static_cast<ulonglong2 *>(host); }
  // The quotient table chained copies of a key (repeated inner keys), or a
  // span filled its overflow table and this task re-ran on counted tables.
  bool sawDuplicateChains() const { return duplicateChains; }
  bool rowsFused() const { return fused; }

 protected:
  uint64_t innerPartitionSize;
  data::CompressedTuple *innerPartition;
  uint64_t outerPartitionSize;
  data::CompressedTuple *outerPartition;

 private:
  void configure();
  void executeMarks();
  void executeOuter();
  void executeGroup();
  core::ExecContext *ctx = nullptr;
  core::JoinPlan plan;
  data::Window *windows[2] = {nullptr, nullptr};
  kernels::BPArgs args;
  uint32_t capacity = 0;
  uint64_t outputCapacity = 0;
  // [0] matches [1] out cursor [2] item count (u32) [3] materialize: count-pass
  // matches / key spans: quotient-table side-list overflow flag
  // semi / anti: [0] qualifying outer tuples [1] rids placed [2] item count (u32) [3] outer unit count (u32)
  // outer kinds: [0] pairs [1] pairs by the item-count scan [2] item count (u32) [3] place-pass matches (unused)
  // [4] unmatched inner [5] unmatched outer [6] inner / outer unit counts (u32 each) [7] spare
  // group: [0] pairs [1] rows by the unit scan [2] item count (u32) [4] empty groups [6] inner unit count (u32)
  unsigned long long *counters = nullptr;
  unsigned long long *countersBack = nullptr;  // pinned copy, enqueued at the end of execute()
  ulonglong2 *outPairs = nullptr;
  uint64_t *outRids = nullptr;               // semi / anti: outer rid list (workspace)
  uint64_t *outGroups = nullptr;             // group: rows (workspace)
  const kernels::GroupColumns *groupColumns = nullptr;  // group: aggregated value columns (null = counts only)
  uint32_t unitCapacity = 0;                 // semi / anti / outer kinds: upper bound of the outer units
  uint32_t unitCapacityR = 0;                // outer kinds preserving R: upper bound of the inner units
  uint64_t matchedPairs = 0, unmatchedInner = 0, unmatchedOuter = 0;  // outer kinds (matches = their sum)
  std::vector<uint64_t> refBounds;  // reference ctor: partition begin arrays
  uint64_t matches = 0, outputCount = 0;
  uint32_t workItems = 0;
  bool reference = false, overflowOut = false, fused = false;
  bool duplicateChains = false;   // copies of a key chained in the quotient table
  bool countedAll = false;        // a quotient span overflowed: this task counts every partition on counted tables
  bool deduped = false;           // heavy inner partitions compacted in place (kernels::bpKeyDedup)
  uint32_t *dedupCounts = nullptr;
  uint64_t *dedupLen = nullptr;
  const kernels::RowSink *sink = nullptr;
  ulonglong2 *hostOut = nullptr;
  uint64_t hostCursor = 0;
};

}  // namespace tasks
}  // namespace hpcjoin
