#include "BuildProbe.h"

#include <algorithm>
#include <cstring>

#include "../host/HostOps.h"
#include "../memory/Arena.h"
#include "../performance/Clock.h"
#include "../performance/Measurements.h"
#include "../performance/Timeline.h"
#include "../operators/HashJoin.h"
#include "../utils/Hip.h"

namespace hpcjoin {
namespace tasks {

// Device counter block, read back once per execute() (BuildProbe.h, counters).
static constexpr uint32_t kCounters = 8;

BuildProbe::BuildProbe(uint64_t innerPartitionSize, data::CompressedTuple *innerPartition,
                       uint64_t outerPartitionSize, data::CompressedTuple *outerPartition)
    : innerPartitionSize(innerPartitionSize), innerPartition(innerPartition), outerPartitionSize(outerPartitionSize),
      outerPartition(outerPartition), reference(true) {
  refBounds = {0, innerPartitionSize, 0, outerPartitionSize};
  args.R = innerPartition;
  args.S = outerPartition;
  args.partR = &refBounds[0];
  args.partS = &refBounds[2];
  args.P = 1;
  args.keyShift = core::Configuration::NETWORK_PARTITIONING_FANOUT + core::Configuration::PAYLOAD_BITS;  // 32
  args.fragShift = args.keyShift + core::Configuration::LOCAL_PARTITIONING_FANOUT;                      // 37
}

BuildProbe::BuildProbe(data::Window *innerWindow, data::Window *outerWindow, core::ExecContext *ctx,
                       const core::JoinPlan &plan, uint64_t outputCapacity)
    : innerPartitionSize(innerWindow->computeLocalWindowSize()), innerPartition(nullptr),
      outerPartitionSize(outerWindow->computeLocalWindowSize()), outerPartition(nullptr), ctx(ctx), plan(plan),
      outputCapacity(outputCapacity) {
  windows[0] = innerWindow;
  windows[1] = outerWindow;
}

BuildProbe::~BuildProbe() {}

void BuildProbe::configure() {
  data::Window *wi = windows[0], *wo = windows[1];
  const uint32_t owned = (uint32_t)wi->getPlan().owned.size();
  args = kernels::BPArgs();
  args.R = wi->getPartitionedData();
  args.S = wo->getPartitionedData();
  args.partR = wi->getPartitionBegin();
  args.partS = wo->getPartitionBegin();
  args.partREnd = wi->getPartitionEnd();
  args.partSEnd = wo->getPartitionEnd();
  args.P = owned << wi->getLocalBits();
  args.rChunk = plan.rChunk;
  args.sChunk = plan.sChunk;
  args.fragShift = plan.wide ? 64 : plan.keyShift + wi->getLocalBits();
  args.keyShift = plan.keyShift;
  if (!plan.wide && !plan.keyOnly && plan.directCount) {  // fragments are < 2^fragBits (direct-addressed counting when small)
    const uint32_t passBits = plan.networkBits + wi->getLocalBits();
    args.fragBits = plan.keyBits > passBits ? std::min<uint32_t>(32, plan.keyBits - passBits) : 1;
  }
  args.wide = plan.wide;
  args.keyOnly = plan.keyOnly;
  args.materialize = plan.materialize;
  args.keyCount = plan.variants.keyCount >= 8 && countedAll ? 9 : plan.variants.keyCount;
  if (plan.keyOnly) {
    const uint32_t passBits = plan.networkBits + wi->getLocalBits();
    args.keyFragBits = plan.keyBits > passBits ? plan.keyBits - passBits : 1;
  }
  args.rowsLds = plan.variants.rowsLds;
  if (wi->getPartitionedHi()) {
    JOIN_ASSERT(wo->getPartitionedHi(), "BuildProbe", "one side split, the other not");
    args.split = 1;
    args.Rhi = wi->getPartitionedHi();
    args.Shi = wo->getPartitionedHi();
  }
  // Direct-addressed counting: duplicate-heavy inner partitions (Zipf) need
  // no inner chunking into rChunk-sized tables -- each work item counts up to
  // 2^18 inner tuples into its count table and probes its outer chunk, so a
  // hot partition costs (inner / 2^18) passes over its outer side instead of
  // (inner / rChunk).
  // (Semi / anti joins build key sets in LDS: rChunk stays the table's size.)
  // (Outer joins build key multisets in LDS as well.)
  if (ctx && ctx->onDevice() && plan.kind == core::JoinKind::Inner && kernels::bpDirectSplit(args))
    args.rChunk = std::max<uint32_t>(args.rChunk, kernels::BP_DIRECT_R_CHUNK);
  if (capacity == 0)
    capacity = (uint32_t)std::min<uint64_t>(
        0xFFFFFFF0ull, 2ull * args.P + outerPartitionSize / args.sChunk + innerPartitionSize / args.rChunk + 1024);
}

// Semi / anti join: mark, then compact (kernels/semi_join.hip).  The marks are
// zeroed here, so every re-run (item-list overflow in collect(), the exact
// redo after a sampled local pass overflowed) starts from clean marks.
// The rid list is bounded by the outer tuples of this rank's window: it
// cannot overflow, so there is no output re-run.
// With a row sink on a device join the place pass writes the payload rows
// {rid, outer row} to the sink (kernels::markPlaceRows) and no rid list is kept.
void BuildProbe::executeMarks() {
  const bool dev = ctx->onDevice();
  const bool anti = plan.kind == core::JoinKind::Anti;
  memory::Arena &ws = ctx->workspace();
  performance::Timeline &tl = ctx->timeline();
  const double wb = (double)innerPartitionSize, wp = (double)outerPartitionSize;
  performance::Measurements::add("BPBUILDELEM", wb, "tuples");
  performance::Measurements::add("BPPROBEELEM", wp, "tuples");
  args.materialize = false;  // no pairs; plan.materialize asks for the rid list
  const uint64_t words = kernels::markWords(windows[1]->getPartitionedCapacity());
  auto *marks = ws.getArray<unsigned long long>(words);
  ctx->zero(marks, words * 8);
  fused = plan.materialize && sink && dev;
  outputCapacity = fused ? sink->capacity : outerPartitionSize;
  outRids = nullptr;
  if (plan.materialize && !fused) outRids = ws.getArray<uint64_t>(outputCapacity + 1);
  if (!dev) {
    tl.begin("BPTASKTIME");
    tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp);
    host::buildProbeMark(args, reinterpret_cast<uint64_t *>(marks));
    matches = host::markCompact(args, reinterpret_cast<const uint64_t *>(marks), anti, outRids, outputCapacity);
    tl.end("BPKERNEL");
    tl.end("BPTASKTIME");
    outputCount = plan.materialize ? matches : 0;
    workItems = args.P;
    return;
  }
  tl.begin("BPTASKTIME", ctx->stream());
  const uint64_t tAlloc = performance::nowUs();
  const uint32_t P1 = std::max<uint32_t>(args.P, 1);
  // Outer units of the compaction: uargs.sChunk positions of one partition each (kernels::MARK_UNIT).
  kernels::BPArgs uargs = args;
  uargs.sChunk = std::min<uint32_t>(args.sChunk, kernels::MARK_UNIT);
  // sum over partitions of ceil(ns / unit) <= P + total / unit: never overflows
  // (even: the u32 unit counts are then zeroed as whole words by the engine's own kernel)
  unitCapacity =
      (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, ((uint64_t)args.P + outerPartitionSize / uargs.sChunk + 2) & ~1ull);
  counters = ws.getArray<unsigned long long>(kCounters);
  ctx->zero(counters, kCounters * sizeof(unsigned long long));
  args.result = uargs.result = counters;
  args.outCursor = uargs.outCursor = counters + 1;
  uint32_t *nItems = reinterpret_cast<uint32_t *>(counters + 2);
  uint32_t *nUnits = reinterpret_cast<uint32_t *>(counters + 3);
  uint32_t *counts = ws.getArray<uint32_t>(P1);
  uint32_t *offsets = ws.getArray<uint32_t>(P1);
  void *scanWs = ws.get(kernels::scanWorkspaceBytes(std::max<uint64_t>(args.P, unitCapacity)));
  kernels::BPItem *items = ws.getArray<kernels::BPItem>(capacity);
  auto *units = ws.getArray<kernels::MarkUnit>(unitCapacity);
  uint32_t *unitCounts = ws.getArray<uint32_t>(unitCapacity);
  unsigned long long *unitOffsets = plan.materialize ? ws.getArray<unsigned long long>(unitCapacity) : nullptr;
  performance::Measurements::add("BPMEMALLOC", (double)(performance::nowUs() - tAlloc), "us");
  performance::Measurements::add("BPMEMSIZE",
                                 (double)(2ull * P1 * 4 + kernels::scanWorkspaceBytes(args.P) +
                                          (uint64_t)capacity * sizeof(kernels::BPItem) + words * 8 +
                                          (uint64_t)unitCapacity * (sizeof(kernels::MarkUnit) + 12) +
                                          kernels::bpMarkLdsBytes(args)),
                                 "bytes");
  hipStream_t s = ctx->stream();
  kernels::bpPlanCounts(args, counts, s);
  kernels::scanExclusiveU32(counts, offsets, args.P, nItems, scanWs, s);
  kernels::bpEmit(args, counts, offsets, items, capacity, s);
  tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp, s);
  kernels::bpMark(args, items, nItems, capacity, marks, s);
  // Outer units (counts / offsets are free again: bpEmit has consumed them in stream order).
  kernels::markPlanUnits(uargs, counts, s);
  kernels::scanExclusiveU32(counts, offsets, args.P, nUnits, scanWs, s);
  kernels::markEmitUnits(uargs, counts, offsets, units, unitCapacity, s);
  ctx->zero(unitCounts, (uint64_t)unitCapacity * sizeof(uint32_t));
  kernels::markCount(uargs, units, nUnits, unitCapacity, marks, anti, unitCounts, s);  // -> counters[0]
  if (plan.materialize) {
    kernels::scanExclusiveU32to64(unitCounts, unitOffsets, unitCapacity, args.outCursor, scanWs, s);
    if (fused)
      kernels::markPlaceRows(uargs, units, nUnits, unitCapacity, marks, anti, unitOffsets, nullptr, nullptr,
                             kernels::KindRowShape::Rid, sink->rowsB, sink->offB, sink->out, outputCapacity, s);
    else
      kernels::markPlace(uargs, units, nUnits, unitCapacity, marks, anti, unitOffsets,
                         reinterpret_cast<unsigned long long *>(outRids), outputCapacity, s);
  }
  hipEvent_t done = tl.mark(s);
  tl.endAt("BPKERNEL", done);
  tl.endAt("BPTASKTIME", done);
  readBackCounters();
}

// Left / right / full outer join (kernels/outer_join.hip): the two-pass pair
// materialization with bpOuterCount as its count pass (per-item pair counts
// and the hit marks of the preserved sides from one read of the keys), the
// unchanged place pass, and per preserved side the unit compaction of the
// unmarked tuples into NULL-padded rows behind the pairs.  Marks, item counts
// and unit counts are zeroed here, so every re-run (item-list or output
// overflow in collect(), the exact redo after a sampled local pass
// overflowed) starts from clean marks.
// With a row sink on a device join over the split layout the place pass writes
// whole rows to the sink: the matched pairs' rows through the inner join's
// fused row kernels, the NULL-padded rows behind them by
// kernels::markPlaceRows, from the same bases as the pairs.  The sink is the
// caller's: an overflow is reported, not re-run.
void BuildProbe::executeOuter() {
  const bool dev = ctx->onDevice();
  const bool keepR = core::preservesInner(plan.kind), keepS = core::preservesOuter(plan.kind);
  memory::Arena &ws = ctx->workspace();
  performance::Timeline &tl = ctx->timeline();
  const double wb = (double)innerPartitionSize, wp = (double)outerPartitionSize;
  performance::Measurements::add("BPBUILDELEM", wb, "tuples");
  performance::Measurements::add("BPPROBEELEM", wp, "tuples");
  const uint64_t wordsR = keepR ? kernels::markWords(windows[0]->getPartitionedCapacity()) : 0;
  const uint64_t wordsS = keepS ? kernels::markWords(windows[1]->getPartitionedCapacity()) : 0;
  auto *marksR = keepR ? ws.getArray<unsigned long long>(wordsR) : nullptr;
  auto *marksS = keepS ? ws.getArray<unsigned long long>(wordsS) : nullptr;
  if (keepR) ctx->zero(marksR, wordsR * 8);
  if (keepS) ctx->zero(marksS, wordsS * 8);
  outPairs = nullptr;
  args.materialize = plan.materialize;
  fused = plan.materialize && sink && dev && args.split && !args.wide;
  if (fused) {
    outputCapacity = sink->capacity;
    args.outRows = reinterpret_cast<ulonglong2 *>(sink->out);
    args.rowsA = reinterpret_cast<const ulonglong2 *>(sink->rowsA);
    args.rowsB = reinterpret_cast<const ulonglong2 *>(sink->rowsB);
    args.offA = sink->offA;
    args.offB = sink->offB;
    args.outCapacity = outputCapacity;
  } else if (plan.materialize) {
    // The unmatched rows alone never overflow the default; the pairs can (repeated keys): collect() grows it.
    if (outputCapacity == 0) outputCapacity = outerPartitionSize + 1024 + (keepR ? innerPartitionSize : 0);
    outPairs = static_cast<ulonglong2 *>(ws.get(outputCapacity * sizeof(ulonglong2)));
    args.outPairs = outPairs;
    args.outCapacity = outputCapacity;
  }
  if (!dev) {
    tl.begin("BPTASKTIME");
    tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp);
    for (;;) {
      hostCursor = 0;
      args.outCursor = reinterpret_cast<unsigned long long *>(&hostCursor);
      matchedPairs = host::buildProbeOuter(args, reinterpret_cast<uint64_t *>(marksR), reinterpret_cast<uint64_t *>(marksS));
      if (!plan.materialize) hostCursor = matchedPairs;
      unmatchedInner = keepR ? host::markCompactPairs(args, reinterpret_cast<const uint64_t *>(marksR), true, outPairs,
                                                      &hostCursor, outputCapacity)
                             : 0;
      unmatchedOuter = keepS ? host::markCompactPairs(args, reinterpret_cast<const uint64_t *>(marksS), false, outPairs,
                                                      &hostCursor, outputCapacity)
                             : 0;
      if (!plan.materialize || hostCursor <= outputCapacity) break;
      // more pairs than the default capacity (repeated keys): once more, exactly sized, from clean marks
      outputCapacity = hostCursor;
      outPairs = static_cast<ulonglong2 *>(ws.get(outputCapacity * sizeof(ulonglong2)));
      args.outPairs = outPairs;
      args.outCapacity = outputCapacity;
      if (keepR) ctx->zero(marksR, wordsR * 8);
      if (keepS) ctx->zero(marksS, wordsS * 8);
    }
    tl.end("BPKERNEL");
    tl.end("BPTASKTIME");
    matches = matchedPairs + unmatchedInner + unmatchedOuter;
    outputCount = plan.materialize ? hostCursor : 0;
    workItems = args.P;
    return;
  }
  tl.begin("BPTASKTIME", ctx->stream());
  const uint64_t tAlloc = performance::nowUs();
  const uint32_t P1 = std::max<uint32_t>(args.P, 1);
  // Units of the compaction, per preserved side: runs of one partition's
  // positions (kernels::MARK_UNIT); the inner side through swapped arguments.
  const kernels::BPArgs rargs0 = kernels::outerSwapSides(args, kernels::MARK_UNIT);
  kernels::BPArgs sargs0 = args;
  sargs0.sChunk = std::min<uint32_t>(args.sChunk, kernels::MARK_UNIT);
  // sum over partitions of ceil(n / unit) <= P + total / unit: never overflows (even: zeroed as whole words)
  auto unitBound = [&](uint64_t n, uint32_t unit) {
    return (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, ((uint64_t)args.P + n / unit + 2) & ~1ull);
  };
  unitCapacityR = keepR ? unitBound(innerPartitionSize, rargs0.sChunk) : 0;
  unitCapacity = keepS ? unitBound(outerPartitionSize, sargs0.sChunk) : 0;
  const uint32_t itemWords = (capacity + 1) & ~1u;  // u32 item counts, zeroed as whole words
  counters = ws.getArray<unsigned long long>(kCounters);
  ctx->zero(counters, kCounters * sizeof(unsigned long long));
  args.result = counters;         // [0] pairs (count pass)
  args.outCursor = counters + 1;  // [1] pairs (scan total of the item counts)
  uint32_t *nItems = reinterpret_cast<uint32_t *>(counters + 2);
  uint32_t *nUnitsR = reinterpret_cast<uint32_t *>(counters + 6), *nUnitsS = nUnitsR + 1;
  uint32_t *counts = ws.getArray<uint32_t>(P1);
  uint32_t *offsets = ws.getArray<uint32_t>(P1);
  const uint64_t scanN = std::max<uint64_t>(std::max<uint64_t>(args.P, capacity), std::max(unitCapacityR, unitCapacity));
  void *scanWs = ws.get(kernels::scanWorkspaceBytes(scanN));
  kernels::BPItem *items = ws.getArray<kernels::BPItem>(capacity);
  uint32_t *itemCounts = ws.getArray<uint32_t>(itemWords);
  unsigned long long *itemOffsets = plan.materialize ? ws.getArray<unsigned long long>(capacity) : nullptr;
  struct Side {
    kernels::BPArgs a;
    uint32_t cap = 0, *nUnits = nullptr, *unitCounts = nullptr;
    kernels::MarkUnit *units = nullptr;
    unsigned long long *unitOffsets = nullptr, *marks = nullptr;
  } side[2];
  side[0].a = rargs0;
  side[0].cap = unitCapacityR;
  side[0].nUnits = nUnitsR;
  side[0].marks = marksR;
  side[1].a = sargs0;
  side[1].cap = unitCapacity;
  side[1].nUnits = nUnitsS;
  side[1].marks = marksS;
  uint64_t unitBytes = 0;
  for (int r = 0; r < 2; ++r) {
    Side &sd = side[r];
    if (!sd.cap) continue;
    sd.units = ws.getArray<kernels::MarkUnit>(sd.cap);
    sd.unitCounts = ws.getArray<uint32_t>(sd.cap);
    if (plan.materialize) sd.unitOffsets = ws.getArray<unsigned long long>(sd.cap);
    sd.a.result = counters + 4 + r;  // [4] unmatched inner, [5] unmatched outer
    unitBytes += (uint64_t)sd.cap * (sizeof(kernels::MarkUnit) + 12);
  }
  performance::Measurements::add("BPMEMALLOC", (double)(performance::nowUs() - tAlloc), "us");
  performance::Measurements::add("BPMEMSIZE",
                                 (double)(2ull * P1 * 4 + kernels::scanWorkspaceBytes(scanN) +
                                          (uint64_t)capacity * (sizeof(kernels::BPItem) + 12) + (wordsR + wordsS) * 8 +
                                          unitBytes + kernels::bpOuterLdsBytes(args)),
                                 "bytes");
  hipStream_t s = ctx->stream();
  kernels::bpPlanCounts(args, counts, s);
  kernels::scanExclusiveU32(counts, offsets, args.P, nItems, scanWs, s);
  kernels::bpEmit(args, counts, offsets, items, capacity, s);
  ctx->zero(itemCounts, (uint64_t)itemWords * sizeof(uint32_t));
  for (const Side &sd : side)
    if (sd.cap) ctx->zero(sd.unitCounts, (uint64_t)sd.cap * sizeof(uint32_t));
  tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp, s);
  kernels::BPArgs countArgs = args;
  countArgs.materialize = false;
  countArgs.itemCounts = itemCounts;
  kernels::bpOuterCount(countArgs, items, nItems, capacity, marksR, marksS, s);  // -> counters[0], marks
  // Unit lists (counts / offsets are free again: bpEmit has consumed them in stream order), unmatched counts.
  for (const Side &sd : side) {
    if (!sd.cap) continue;
    kernels::markPlanUnits(sd.a, counts, s);
    kernels::scanExclusiveU32(counts, offsets, args.P, sd.nUnits, scanWs, s);
    kernels::markEmitUnits(sd.a, counts, offsets, sd.units, sd.cap, s);
    kernels::markCount(sd.a, sd.units, sd.nUnits, sd.cap, sd.marks, true, sd.unitCounts, s);  // -> counters[4 + side]
  }
  if (plan.materialize) {
    kernels::scanExclusiveU32to64(itemCounts, itemOffsets, capacity, args.outCursor, scanWs, s);
    for (const Side &sd : side)
      if (sd.cap) kernels::scanExclusiveU32to64(sd.unitCounts, sd.unitOffsets, sd.cap, nullptr, scanWs, s);
    args.itemOffsets = itemOffsets;
    args.result = counters + 3;  // the count pass already counted
    kernels::buildProbe(args, items, nItems, capacity, s);  // the inner join's place pass, unchanged
    // Unmatched rows behind the pairs: inner side from [1], outer side from [1] + [4] ([4] = 0 unless R is preserved).
    if (keepR && fused)
      kernels::markPlaceRows(side[0].a, side[0].units, nUnitsR, side[0].cap, marksR, true, side[0].unitOffsets,
                             counters + 1, nullptr, kernels::KindRowShape::InnerPad, sink->rowsA, sink->offA, sink->out,
                             outputCapacity, s);
    else if (keepR)
      kernels::markPlacePairs(side[0].a, side[0].units, nUnitsR, side[0].cap, marksR, side[0].unitOffsets, counters + 1,
                              nullptr, true, outPairs, outputCapacity, s);
    if (keepS && fused)
      kernels::markPlaceRows(side[1].a, side[1].units, nUnitsS, side[1].cap, marksS, true, side[1].unitOffsets,
                             counters + 1, counters + 4, kernels::KindRowShape::OuterPad, sink->rowsB, sink->offB,
                             sink->out, outputCapacity, s);
    else if (keepS)
      kernels::markPlacePairs(side[1].a, side[1].units, nUnitsS, side[1].cap, marksS, side[1].unitOffsets, counters + 1,
                              counters + 4, false, outPairs, outputCapacity, s);
  }
  hipEvent_t done = tl.mark(s);
  tl.endAt("BPKERNEL", done);
  tl.endAt("BPTASKTIME", done);
  readBackCounters();
}

// Group join (kernels/group_join.hip): no pair is written and nothing can
// overflow but the item list -- the rows are this rank's inner tuples.  The
// accumulators (u32 counts and, column-major, C u64 aggregates per position of
// the partitioned inner buffer; groupColumns carries each column's aggregate
// and element type to the kernels and the host twin) and the unit counts are
// reset here, so every re-run (item-list overflow in collect(), the exact redo
// after a sampled local pass overflowed, a second run()) starts clean: the
// counts are zeroed, the aggregates get their identities (kernels::groupAggInit;
// the host twin writes them itself).  The accumulators come from the Arena
// (hipMalloc, coarse-grained), where the hardware float atomics of typed
// columns are valid.
void BuildProbe::executeGroup() {
  const bool dev = ctx->onDevice();
  const kernels::GroupColumns cols = groupColumns ? *groupColumns : kernels::GroupColumns();
  const uint32_t C = cols.n;
  const uint64_t W = 2 + C;
  memory::Arena &ws = ctx->workspace();
  performance::Timeline &tl = ctx->timeline();
  const double wb = (double)innerPartitionSize, wp = (double)outerPartitionSize;
  performance::Measurements::add("BPBUILDELEM", wb, "tuples");
  performance::Measurements::add("BPPROBEELEM", wp, "tuples");
  args.materialize = false;  // no pairs; plan.materialize asks for the rows
  const uint64_t slots = (windows[0]->getPartitionedCapacity() + 2) & ~1ull;  // (u32 counts zeroed as whole words)
  uint32_t *accCount = ws.getArray<uint32_t>(slots);
  auto *accAgg = C ? ws.getArray<unsigned long long>(slots * C) : nullptr;
  ctx->zero(accCount, slots * sizeof(uint32_t));
  if (dev) kernels::groupAggInit(cols, accAgg, slots, ctx->stream());
  outputCapacity = innerPartitionSize;  // one row per inner tuple: cannot overflow
  outGroups = plan.materialize ? ws.getArray<uint64_t>(std::max<uint64_t>(1, outputCapacity * W)) : nullptr;
  if (!dev) {
    tl.begin("BPTASKTIME");
    tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp);
    uint64_t rows = 0;
    matchedPairs = host::buildProbeGroup(args, cols, accCount, reinterpret_cast<uint64_t *>(accAgg), slots);
    unmatchedInner = host::groupEmit(args, accCount, reinterpret_cast<const uint64_t *>(accAgg), slots, C, outGroups,
                                     outputCapacity, &rows);
    tl.end("BPKERNEL");
    tl.end("BPTASKTIME");
    unmatchedOuter = 0;
    matches = rows;
    outputCount = plan.materialize ? rows : 0;
    workItems = args.P;
    return;
  }
  tl.begin("BPTASKTIME", ctx->stream());
  const uint64_t tAlloc = performance::nowUs();
  const uint32_t P1 = std::max<uint32_t>(args.P, 1);
  // Units of the inner side (also of partitions without outer tuples, which get no work item).
  kernels::BPArgs uargs = kernels::outerSwapSides(args, kernels::MARK_UNIT);
  unitCapacityR = (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull,
                                               ((uint64_t)args.P + innerPartitionSize / uargs.sChunk + 2) & ~1ull);
  counters = ws.getArray<unsigned long long>(kCounters);
  ctx->zero(counters, kCounters * sizeof(unsigned long long));
  args.result = counters;       // [0] pairs
  uargs.result = counters + 4;  // [4] empty groups
  uint32_t *nItems = reinterpret_cast<uint32_t *>(counters + 2);
  uint32_t *nUnits = reinterpret_cast<uint32_t *>(counters + 6);
  uint32_t *counts = ws.getArray<uint32_t>(P1);
  uint32_t *offsets = ws.getArray<uint32_t>(P1);
  void *scanWs = ws.get(kernels::scanWorkspaceBytes(std::max<uint64_t>(args.P, unitCapacityR)));
  kernels::BPItem *items = ws.getArray<kernels::BPItem>(capacity);
  auto *units = ws.getArray<kernels::MarkUnit>(unitCapacityR);
  uint32_t *unitCounts = plan.materialize ? ws.getArray<uint32_t>(unitCapacityR) : nullptr;
  unsigned long long *unitOffsets = plan.materialize ? ws.getArray<unsigned long long>(unitCapacityR) : nullptr;
  performance::Measurements::add("BPMEMALLOC", (double)(performance::nowUs() - tAlloc), "us");
  performance::Measurements::add("BPMEMSIZE",
                                 (double)(2ull * P1 * 4 + kernels::scanWorkspaceBytes(std::max<uint64_t>(args.P, unitCapacityR)) +
                                          (uint64_t)capacity * sizeof(kernels::BPItem) + slots * (4 + 8ull * C) +
                                          (uint64_t)unitCapacityR * (sizeof(kernels::MarkUnit) + 12) +
                                          kernels::bpGroupLdsBytes(args, C)),
                                 "bytes");
  hipStream_t s = ctx->stream();
  kernels::bpPlanCounts(args, counts, s);
  kernels::scanExclusiveU32(counts, offsets, args.P, nItems, scanWs, s);
  kernels::bpEmit(args, counts, offsets, items, capacity, s);
  if (unitCounts) ctx->zero(unitCounts, (uint64_t)unitCapacityR * sizeof(uint32_t));
  tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp, s);
  kernels::bpGroup(args, items, nItems, capacity, cols, accCount, accAgg, slots, s);  // -> counters[0], accumulators
  // Inner units (counts / offsets are free again: bpEmit has consumed them in stream order).
  kernels::markPlanUnits(uargs, counts, s);
  kernels::scanExclusiveU32(counts, offsets, args.P, nUnits, scanWs, s);
  kernels::markEmitUnits(uargs, counts, offsets, units, unitCapacityR, s);
  if (plan.materialize) {
    kernels::groupUnitLengths(uargs, units, nUnits, unitCapacityR, unitCounts, s);
    kernels::scanExclusiveU32to64(unitCounts, unitOffsets, unitCapacityR, counters + 1, scanWs, s);  // -> [1] rows
  }
  kernels::groupEmit(uargs, units, nUnits, unitCapacityR, accCount, accAgg, slots, C, unitOffsets,
                     reinterpret_cast<unsigned long long *>(outGroups), outputCapacity, s);  // -> counters[4], rows
  hipEvent_t done = tl.mark(s);
  tl.endAt("BPKERNEL", done);
  tl.endAt("BPTASKTIME", done);
  readBackCounters();
}

void BuildProbe::execute() {
  if (reference) {
    args.result = nullptr;
    matches = host::buildProbe(args);
    operators::HashJoin::RESULT_COUNTER += matches;
    return;
  }
  configure();
  if (plan.kind == core::JoinKind::Group) {
    executeGroup();
    return;
  }
  if (core::isOuterKind(plan.kind)) {
    executeOuter();
    return;
  }
  if (plan.kind != core::JoinKind::Inner) {
    executeMarks();
    return;
  }
  const bool dev = ctx->onDevice();
  memory::Arena &ws = ctx->workspace();
  fused = plan.materialize && sink && dev && args.split;
  if (fused) {
    outputCapacity = sink->capacity;
    outPairs = nullptr;
    args.outRows = reinterpret_cast<ulonglong2 *>(sink->out);
    args.rowsA = reinterpret_cast<const ulonglong2 *>(sink->rowsA);
    args.rowsB = reinterpret_cast<const ulonglong2 *>(sink->rowsB);
    args.offA = sink->offA;
    args.offB = sink->offB;
    args.outCapacity = outputCapacity;
  } else if (plan.materialize && hostOut) {
    outPairs = hostOut;  // pinned host memory, written by the place kernel over the host link
    args.outPairs = outPairs;
    args.outCapacity = outputCapacity;
  } else if (plan.materialize) {
    if (outputCapacity == 0) outputCapacity = outerPartitionSize + 1024;
    outPairs = static_cast<ulonglong2 *>(ws.get(outputCapacity * sizeof(ulonglong2)));
    args.outPairs = outPairs;
    args.outCapacity = outputCapacity;
  }
  performance::Timeline &tl = ctx->timeline();
  // The build and the probe of one LDS table run in one kernel (one work
  // item = build + probe): its time is charged to BPBUILD / BPPROBE in
  // proportion to the tuples each reads.
  const double wb = (double)innerPartitionSize, wp = (double)outerPartitionSize;
  performance::Measurements::add("BPBUILDELEM", wb, "tuples");
  performance::Measurements::add("BPPROBEELEM", wp, "tuples");
  if (!dev) {
    args.outCursor = reinterpret_cast<unsigned long long *>(&hostCursor);
    tl.begin("BPTASKTIME");
    tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp);
    for (;;) {
      hostCursor = 0;
      matches = host::buildProbe(args);
      if (!plan.materialize || hostOut || hostCursor <= outputCapacity) break;
      // more pairs than the default capacity (repeated keys): once more, exactly sized, as the device path's
      // collect() does -- the stores past the capacity were dropped, and getOutput() would be read beyond it.
      // (The undersized buffer stays in the arena until the next reset: host twin, one extra build/probe.)
      // hostOut is the caller's buffer and cannot grow: pairs past its capacity stay dropped, outputCount
      // keeps the true total and collect() reports it as outputOverflow, as on the device.
      outputCapacity = hostCursor;
      outPairs = static_cast<ulonglong2 *>(ws.get(outputCapacity * sizeof(ulonglong2)));
      args.outPairs = outPairs;
      args.outCapacity = outputCapacity;
    }
    tl.end("BPKERNEL");
    tl.end("BPTASKTIME");
    outputCount = hostCursor;
    workItems = args.P;
    return;
  }
  tl.begin("BPTASKTIME", ctx->stream());
  const uint64_t tAlloc = performance::nowUs();
  counters = ws.getArray<unsigned long long>(kCounters);
  ctx->zero(counters, kCounters * sizeof(unsigned long long));
  args.result = counters;
  args.outCursor = counters + 1;
  uint32_t *nItems = reinterpret_cast<uint32_t *>(counters + 2);
  uint32_t *counts = ws.getArray<uint32_t>(std::max<uint32_t>(args.P, 1));
  uint32_t *offsets = ws.getArray<uint32_t>(std::max<uint32_t>(args.P, 1));
  void *scanWs = ws.get(kernels::scanWorkspaceBytes(args.P));
  kernels::BPItem *items = ws.getArray<kernels::BPItem>(capacity);
  performance::Measurements::add("BPMEMALLOC", (double)(performance::nowUs() - tAlloc), "us");
  performance::Measurements::add("BPMEMSIZE",
                                 (double)(2ull * std::max<uint32_t>(args.P, 1) * 4 + kernels::scanWorkspaceBytes(args.P) +
                                          (uint64_t)capacity * sizeof(kernels::BPItem) + kernels::bpLdsBytes(args)),
                                 "bytes");
  // Key-only counting on the quotient table: partitions of repeated keys go
  // to the counted-table kernel instead of the span work queue.  Fragments
  // of 45-48 bits (inputs below ~500M tuples) do not fit the quotient table:
  // every partition is counted there.
  const bool keySpans = args.keyOnly;
  const bool counted = keySpans && args.keyCount >= 8 && kernels::bpKeyCountedFits(args);
  const bool quotient = counted && kernels::bpKeyQuotientFits(args);
  // keyCount 9 (repeated inner keys): partitions of more than one inner chunk
  // are first compacted to (distinct word, count) (kernels::bpKeyDedup), once
  // per join -- not with per-chunk rebuilds of a pipelined outer side, which
  // re-read the inner words.
  // (Leaving partitions of at most one inner chunk on the quotient table
  // instead -- heavy ones compacted and counted -- was exact but took 119 ms
  // of build/probe for Zipf-both sparse 1e9 x 4e9 instead of 13.8: keys with
  // hundreds of copies in light partitions walk the overflow table.)
  const bool dedup = counted && args.keyCount == 9 && args.split && !plan.pipelineOuter;
  if (counted) {
    args.heavySpans = ws.getArray<kernels::BPSpan>(capacity);
    args.heavyCapacity = capacity;
    // keyCount 9 (repeated keys seen): every partition on counted tables.
    args.heavyMin = (args.keyCount == 9 || !quotient) ? 0 : args.rChunk;
    args.heavyCount = nItems + 1;  // high half of counters[2]: read back with the rest
  }
  if (dedup) {
    if (!dedupCounts) {  // kept for the join: a re-run only re-emits the compacted spans
      dedupCounts = ws.getArray<uint32_t>(std::max<uint64_t>(windows[0]->getPartitionedCapacity(), 1));
      dedupLen = ws.getArray<uint64_t>((uint64_t)std::max<uint32_t>(args.P, 1) * kernels::BP_DEDUP_SEGS);
    }
    args.dedupParts = ws.getArray<uint32_t>(std::max<uint32_t>(args.P, 1));
    args.dedupCount = reinterpret_cast<uint32_t *>(counters + 1);  // the pair cursor is unused by a count
    args.dedupBig = ws.getArray<uint32_t>(std::max<uint32_t>(args.P, 1));
    args.dedupBigCount = reinterpret_cast<uint32_t *>(counters + 1) + 1;  // (zeroed with the counters)
    args.dedupCounts = dedupCounts;
    args.dedupLen = dedupLen;
  }
  kernels::bpPlanCounts(args, counts, ctx->stream());
  kernels::scanExclusiveU32(counts, offsets, args.P, nItems, scanWs, ctx->stream());
  if (keySpans) {
    // Key-only counting: resolved spans through a device work queue.
    auto *spans = ws.getArray<kernels::BPSpan>(capacity);
    uint32_t *queue = ws.getArray<uint32_t>(1);
    kernels::bpEmitSpans(args, counts, offsets, spans, capacity, ctx->stream());
    args.sideOverflow = counters + 3;  // quotient table flags (kernels.h, BPArgs::sideOverflow)
    tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp, ctx->stream());
    if (dedup) {
      kernels::bpKeyDedup(args, args.P, deduped, ctx->stream());
      if (!deduped) kernels::bpKeyDedupMerge(args, args.P, ctx->stream());
      deduped = true;
    }
    if (!counted || args.heavyMin != 0)  // otherwise every span is on the heavy list
      kernels::buildProbeKeySpans(args, spans, nItems, capacity, queue, ctx->stream());
    if (counted) kernels::bpKeyCountedSpans(args, queue, ctx->stream());  // (the queue word is re-zeroed)
    hipEvent_t done = tl.mark(ctx->stream());
    tl.endAt("BPKERNEL", done);
    tl.endAt("BPTASKTIME", done);
    readBackCounters();
    return;
  }
  kernels::bpEmit(args, counts, offsets, items, capacity, ctx->stream());
  if (!plan.materialize) {
    tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp, ctx->stream());
    kernels::buildProbe(args, items, nItems, capacity, ctx->stream());
    hipEvent_t done = tl.mark(ctx->stream());  // one event ends both spans
    tl.endAt("BPKERNEL", done);
    tl.endAt("BPTASKTIME", done);
    readBackCounters();
    return;
  }
  // Two-pass exact materialization: count per item -> 64-bit offsets -> place.
  // (A single pass with one device atomic per wave and batch on a shared
  // output cursor measured 65 ms instead of 29 for the SF100 row output: 4.7M
  // atomics on one address serialize.)
  uint32_t *itemCounts = ws.getArray<uint32_t>(capacity);
  unsigned long long *itemOffsets = ws.getArray<unsigned long long>(capacity);
  void *scanWs64 = ws.get(kernels::scanWorkspaceBytes(capacity));
  ctx->zero(itemCounts, (size_t)capacity * sizeof(uint32_t));
  kernels::BPArgs countArgs = args;
  countArgs.materialize = false;
  countArgs.itemCounts = itemCounts;
  tl.beginSplit("BPKERNEL", "BPBUILD", wb, "BPPROBE", wp, ctx->stream());
  kernels::buildProbe(countArgs, items, nItems, capacity, ctx->stream());  // -> counters[0] = matches
  kernels::scanExclusiveU32to64(itemCounts, itemOffsets, capacity, args.outCursor, scanWs64, ctx->stream());
  args.itemOffsets = itemOffsets;
  args.result = counters + 3;  // the count pass already counted
  kernels::buildProbe(args, items, nItems, capacity, ctx->stream());
  hipEvent_t done = tl.mark(ctx->stream());
  tl.endAt("BPKERNEL", done);
  tl.endAt("BPTASKTIME", done);
  readBackCounters();
}

// Enqueued behind the build/probe, so the join's final synchronisation also
// completes the read-back (no separate blocking copy afterwards).
void BuildProbe::readBackCounters() {
  countersBack = ctx->staging().getArray<unsigned long long>(kCounters);
  ctx->readBack(countersBack, counters, kCounters * sizeof(unsigned long long));
}

bool BuildProbe::collect() {
  if (reference || !ctx->onDevice()) {
    overflowOut = plan.materialize && outputCount > outputCapacity;
    return false;
  }
  unsigned long long h[kCounters];
  HIP_CHECK(hipStreamSynchronize(ctx->stream()));  // no-op after the caller's sync
  std::memcpy(h, countersBack, sizeof(h));
  matches = h[0];
  outputCount = h[1];
  if (plan.kind == core::JoinKind::Group) {
    // [0] pairs [1] rows by the unit scan [2] item count (u32) [4] empty groups [6] inner unit count (u32)
    uint32_t nItems, nUnits;
    std::memcpy(&nItems, &h[2], sizeof(nItems));
    std::memcpy(&nUnits, &h[6], sizeof(nUnits));
    workItems = nItems;
    matchedPairs = h[0];
    unmatchedInner = h[4];
    unmatchedOuter = 0;
    matches = innerPartitionSize;  // one row per inner tuple of this rank's partitions
    outputCount = plan.materialize ? matches : 0;
    JOIN_ASSERT(nUnits <= unitCapacityR, "BuildProbe", "%u inner units, bound %u", nUnits, unitCapacityR);
    if (nItems > capacity) {  // the only re-run: the rows cannot overflow
      capacity = nItems;
      return true;
    }
    JOIN_ASSERT(!plan.materialize || h[1] == matches, "BuildProbe", "group join: the units hold %lu rows, the window %lu",
                (unsigned long)h[1], (unsigned long)matches);
    return false;
  }
  if (core::isOuterKind(plan.kind)) {
    // [0] pairs [1] pairs by the scan [2] item count (u32) [4] unmatched inner [5] unmatched outer
    // [6] inner / outer unit counts (u32 each)
    uint32_t nItems, nUnits[2];
    std::memcpy(&nItems, &h[2], sizeof(nItems));
    std::memcpy(nUnits, &h[6], sizeof(nUnits));
    workItems = nItems;
    matchedPairs = h[0];
    unmatchedInner = h[4];
    unmatchedOuter = h[5];
    matches = matchedPairs + unmatchedInner + unmatchedOuter;
    // The true row total, also when stores were clipped at the capacity.
    outputCount = plan.materialize ? matches : 0;
    JOIN_ASSERT(nUnits[0] <= unitCapacityR && nUnits[1] <= unitCapacity, "BuildProbe",
                "%u inner / %u outer units, bounds %u / %u", nUnits[0], nUnits[1], unitCapacityR, unitCapacity);
    bool again = false;
    if (nItems > capacity) {
      capacity = nItems;
      again = true;
    } else {
      JOIN_ASSERT(!plan.materialize || h[1] == h[0], "BuildProbe", "outer join: item counts sum to %lu pairs, counted %lu",
                  (unsigned long)h[1], (unsigned long)h[0]);
    }
    if (plan.materialize && outputCount > outputCapacity) {
      if (fused) {
        overflowOut = true;  // the buffer is the caller's: it re-runs with a larger one
      } else {
        outputCapacity = outputCount;
        again = true;
      }
    }
    return again;
  }
  if (plan.kind != core::JoinKind::Inner) {  // [2] item count, [3] unit count (u32 each); the rid list cannot overflow
    uint32_t nItems, nUnits;
    std::memcpy(&nItems, &h[2], sizeof(nItems));
    std::memcpy(&nUnits, &h[3], sizeof(nUnits));
    workItems = nItems;
    JOIN_ASSERT(nUnits <= unitCapacity, "BuildProbe", "%u outer units, bound %u", nUnits, unitCapacity);
    JOIN_ASSERT(!plan.materialize || outputCount == matches, "BuildProbe",
                "semi/anti join placed %lu rids but counted %lu", (unsigned long)outputCount, (unsigned long)matches);
    if (fused && outputCount > outputCapacity) overflowOut = true;  // a sink smaller than the outer side
    if (nItems > capacity) {
      capacity = nItems;
      return true;
    }
    return false;
  }
  uint32_t items, heavy;
  std::memcpy(&items, &h[2], sizeof(items));
  std::memcpy(&heavy, reinterpret_cast<const char *>(&h[2]) + sizeof(items), sizeof(heavy));
  workItems = items + heavy;
  bool again = false;
  if (h[3] & 2) duplicateChains = true;  // exact count; later joins use counted tables throughout
  if (args.sideOverflow && (h[3] & 8)) {  // a quotient span's overflow table filled: count void, counted tables
    countedAll = duplicateChains = true;
    again = true;
  }
  if (items > capacity || heavy > capacity) {
    capacity = std::max(items, heavy);
    again = true;
  }
  if (plan.materialize && outputCount > outputCapacity) {
    if (fused || hostOut) {
      overflowOut = true;  // the buffer is the caller's: it re-runs with a larger one
    } else {
      outputCapacity = outputCount;
      again = true;
    }
  }
  return again;
}

}  // namespace tasks
}  // namespace hpcjoin
