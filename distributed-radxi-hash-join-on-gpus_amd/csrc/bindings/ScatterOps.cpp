// Kernel-level entry points of every production scatter policy (ops submodule):
// the sampled network pass and the local pass with their real layouts, on
// sentinel-filled outputs, so tests can pin each kernel by what it writes.
//
// Nothing here lays anything out: every step is the kernels:: call that
// tasks/SampledNetworkPartitioning.cpp (sidePlan / sample / layoutSide /
// scatterSide), tasks/BitmapJoin.cpp (range passes) and
// tasks/LocalPartitioning.cpp (partitionImpl) make, in their order.
#include "ScatterOps.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "../kernels/kernels.h"
#include "../utils/Debug.h"
#include "../utils/Hip.h"

namespace py = pybind11;
using namespace hpcjoin;

namespace {

using kernels::CLAIM_GROUPS;

// Every output element is pre-filled with this word (its low 32 / 16 bits for
// narrower columns).  The top bit is set: no compressed, key-only or
// digit-on-top fragment word can equal it.
constexpr uint64_t SENTINEL = 0xA5A5A5A5A5A5A5A5ull;

template <typename T>
T *ptr(const at::Tensor &t) {
  return reinterpret_cast<T *>(t.data_ptr());
}

at::TensorOptions on(const at::Tensor &t, at::ScalarType st) {
  return at::TensorOptions().dtype(st).device(t.device());
}

at::Tensor sentinelFilled(std::vector<int64_t> shape, const at::Tensor &like, at::ScalarType st) {
  at::Tensor t = at::empty(shape, on(like, st));
  if (st == at::kLong)
    t.fill_((int64_t)SENTINEL);
  else if (st == at::kInt)
    t.fill_((int64_t)(int32_t)(uint32_t)SENTINEL);
  else
    t.fill_((int64_t)(int16_t)(uint16_t)SENTINEL);
  return t;
}

// Claim cursors ([m] u32 or u64 on the device) as int64 on the host.
at::Tensor cursorsToHost(const at::Tensor &c, bool narrow) {
  at::Tensor h = c.cpu().to(at::kLong);
  return narrow ? h.bitwise_and((int64_t)0xFFFFFFFFll) : h;
}

// gend -= shrink on every slice of at least shrink + 16 slots (the bounded
// protocol's overflow path: the allocation stays, the slice end moves).
void shrinkSlices(const at::Tensor &gstart, at::Tensor gend, int64_t shrink) {
  HIP_CHECK(hipDeviceSynchronize());
  at::Tensor cap = gend - gstart;  // wraps like the cursors do
  gend.copy_(at::where(cap >= shrink + 16, gend - shrink, gend));
  HIP_CHECK(hipDeviceSynchronize());
}

py::dict opNetScatterSlices(const at::Tensor &tuples, int64_t bits, const std::string &format, int64_t keyShift,
                            int64_t keyBits, int64_t mixBits, int64_t narrowArg, int64_t maxBlocks,
                            int64_t sampleStride, int64_t roundLpArg, int64_t dLo, int64_t range, int64_t shrink,
                            int64_t guard, bool unbounded) {
  // [n, 2] (key, rid) tuples, or a 1-D key column for the formats that write no rid.
  const bool column = tuples.dim() == 1;
  const bool compressed = format == "compressed", keyOnly = format == "key_only", frag = format == "frag",
             wide = format == "wide", packed = format == "frag_packed";
  TORCH_CHECK(compressed || keyOnly || frag || wide || packed, "net_scatter_slices: format ", format);
  TORCH_CHECK(!column || !(compressed || wide), "net_scatter_slices: format ", format,
              " carries a rid, which a 1-D key column does not have; key columns take frag, frag_packed and key_only");
  TORCH_CHECK(tuples.is_cuda() && (column || (tuples.dim() == 2 && tuples.size(1) == 2)) &&
                  tuples.scalar_type() == at::kLong && tuples.is_contiguous(),
              "net_scatter_slices: tuples must be a contiguous device int64 tensor of shape [n, 2] (key, rid), or [n] "
              "(a key column)");
  // Packed fragment words (kernels.h, PK_*): the window and the slice tables count u64 words.
  TORCH_CHECK(!packed || (bits <= kernels::PK_MAX_PART_BITS && !unbounded && shrink % kernels::PK_CHUNK_WORDS == 0 &&
                          (roundLpArg == 0 || roundLpArg >= 3)),
              "net_scatter_slices: frag_packed takes at most ", kernels::PK_MAX_PART_BITS,
              " bits, bounded slices, shrink in whole chunks and round pieces of whole chunks");
  TORCH_CHECK(bits >= 1 && bits <= kernels::MAX_PART_BITS, "net_scatter_slices: bits=", bits);
  TORCH_CHECK(range == 0 || frag, "net_scatter_slices: range passes scatter fragments");
  TORCH_CHECK(roundLpArg == 0 || (!wide && range == 0), "net_scatter_slices: round slices need a whole-range, ",
              "non-wide pass");
  TORCH_CHECK(shrink >= 0 && guard >= 0 && maxBlocks >= 1 && sampleStride >= 1 && mixBits >= 0 && mixBits <= 64,
              "net_scatter_slices: negative option");
  // The exact multi-rank pass (tasks/NetworkPartitioning.cpp) scatters without slice ends.
  TORCH_CHECK(!unbounded || (sampleStride == 1 && shrink == 0 && range == 0),
              "net_scatter_slices: only exact, whole slices may be scattered unbounded");
  HIP_CHECK(hipSetDevice(tuples.get_device()));
  const hipStream_t st = nullptr;
  const uint64_t n = tuples.size(0);
  const uint32_t F = 1u << bits, G = CLAIM_GROUPS;
  const uint32_t Fp = range ? (uint32_t)range : F;  // slices per group
  const kernels::KeyMix mix{mixBits ? 1u : 0u, mixBits ? (uint32_t)mixBits : 64u};
  const kernels::KeySource in = column ? kernels::KeySource::column(ptr<const uint64_t>(tuples))
                                       : kernels::KeySource(ptr<const data::Tuple>(tuples));

  // sidePlan(): geometry, stride, scale, window capacity.
  const auto geom = kernels::partitionGeometry(n, (uint32_t)maxBlocks);
  const uint32_t stride = kernels::sampleStrideFor(geom, n, F, (uint32_t)sampleStride);
  const kernels::SampleScale sc = kernels::sampleScale(geom, n, stride, stride == 1);
  const uint32_t roundLp = kernels::roundLpFor((uint32_t)roundLpArg, frag ? 4 : 8);
  const uint32_t tailWords = packed ? kernels::packedTailWords(geom) : 0;
  const uint64_t capacity = packed ? kernels::sampledPackedWindowCapacity(sc, F, roundLp, tailWords)
                                   : kernels::sampledWindowCapacity(sc, F, roundLp);

  // sample(): sampled totals, or the exact histogram.
  at::Tensor totals = at::zeros({(int64_t)G * F}, on(tuples, at::kLong));
  if (stride > 1) {
    kernels::netSampledTotals(in, n, (uint32_t)bits, geom, ptr<uint64_t>(totals), st, mix, stride);
  } else {
    at::Tensor blockHist = at::empty({(int64_t)F * geom.blocks}, on(tuples, at::kInt));
    kernels::netHistogram(in, n, (uint32_t)bits, geom, ptr<uint32_t>(blockHist), st, mix, 1);
    kernels::netGroupTotals(ptr<uint32_t>(blockHist), F, geom.blocks, ptr<uint64_t>(totals), st);
    HIP_CHECK(hipDeviceSynchronize());  // blockHist is released below
  }

  // layoutSide(): cursor width, window, [G][F'] starts / cursors / ends + round map.
  const bool narrow = narrowArg < 0 ? kernels::cursorsNarrow(capacity + n) : narrowArg != 0;
  TORCH_CHECK(!narrow || kernels::cursorsNarrow(capacity + n), "net_scatter_slices: 32-bit cursors wrap at ",
              capacity + n, " positions");
  const int64_t slots = (int64_t)(capacity + (uint64_t)guard);
  at::Tensor window = wide   ? sentinelFilled({slots, 2}, tuples, at::kLong)
                      : frag ? sentinelFilled({slots}, tuples, at::kInt)
                             : sentinelFilled({slots}, tuples, at::kLong);
  const int64_t m = (int64_t)G * Fp;
  const size_t cb = narrow ? 4 : 8, per = (size_t)m * cb;
  at::Tensor cursors = at::zeros({(int64_t)((3 * per + 16 + 7) / 8)}, on(tuples, at::kLong));
  at::Tensor cview = narrow ? cursors.view(at::kInt) : cursors;
  at::Tensor gstartT = cview.slice(0, 0, m), gcurT = cview.slice(0, m, 2 * m), gendT = cview.slice(0, 2 * m, 3 * m);
  uint8_t *base = ptr<uint8_t>(cursors);
  uint32_t *roundMeta = reinterpret_cast<uint32_t *>(base + 3 * per);  // zeroed: linear slices
  at::Tensor capacityUsed = at::zeros({1}, on(tuples, at::kLong));
  kernels::LayoutInput lin{ptr<uint64_t>(totals), sc, base, base + per, base + 2 * per,
                           ptr<unsigned long long>(capacityUsed)};
  lin.packed = packed;
  lin.packedTail = tailWords;
  if (roundLp) {
    uint32_t lns = 0;
    while ((1u << lns) < G * F) ++lns;
    const uint64_t limit = narrow ? (1ull << 32) : (1ull << 62);
    uint32_t maxLv = 0;
    while (maxLv < 40 && ((uint64_t)G * F << (maxLv + 1)) + n < limit) ++maxLv;
    lin.roundMeta = roundMeta;
    lin.roundLp = roundLp;
    lin.roundMaxLv = maxLv;
    lin.roundCapacity = capacity;
  }
  kernels::netSampledLayout(&lin, 1, F, narrow, st, (uint32_t)dLo, (uint32_t)range);
  if (shrink) shrinkSlices(gstartT, gendT, shrink);

  // What finishSide() checks after the scatter, checked before it: no slice
  // reaches past the window, whatever the layout decided.
  HIP_CHECK(hipDeviceSynchronize());
  at::Tensor gstartH = cursorsToHost(gstartT, narrow), gendH = cursorsToHost(gendT, narrow);
  at::Tensor metaH = cursors.view(at::kInt).slice(0, (int64_t)(3 * per / 4), (int64_t)(3 * per / 4) + 4).cpu();
  kernels::RoundMap rm;
  rm.lp = (uint32_t)metaH[0].item<int32_t>();
  rm.lv = (uint32_t)metaH[1].item<int32_t>();
  rm.lns = (uint32_t)metaH[2].item<int32_t>();
  const uint64_t used = (uint64_t)capacityUsed.cpu()[0].item<int64_t>();
  {
    const int64_t *gs = gstartH.data_ptr<int64_t>(), *ge = gendH.data_ptr<int64_t>();
    uint64_t maxEnd = 0, maxCap = 0;
    for (int64_t i = 0; i < m; ++i) {
      TORCH_CHECK(ge[i] >= gs[i], "net_scatter_slices: slice ", i, " ends before it starts");
      maxEnd = std::max<uint64_t>(maxEnd, (uint64_t)ge[i]);
      maxCap = std::max<uint64_t>(maxCap, (uint64_t)(ge[i] - gs[i]));
    }
    if (rm.on()) {
      TORCH_CHECK(rm.lv >= rm.lp && maxCap <= (1ull << rm.lv) && (1ull << rm.lns) == (uint64_t)m,
                  "net_scatter_slices: round map lp=", rm.lp, " lv=", rm.lv, " lns=", rm.lns, " for slices of ", maxCap);
      maxEnd = kernels::roundSlots(maxCap, rm.lp, rm.lns);
    }
    TORCH_CHECK(maxEnd <= capacity && used <= capacity, "net_scatter_slices: slices end at ", maxEnd, " (", used,
                " used), the window holds ", capacity);
  }

  // scatterSide().
  const int nm = narrow ? 1 : 0;
  void *gcur = base + per;
  const void *gend = unbounded ? nullptr : base + 2 * per;
  at::Tensor wideFlag = at::zeros({1}, on(tuples, at::kLong));
  if (packed)
    kernels::netScatterFragPacked(in, n, (uint32_t)bits, geom, gcur, ptr<uint64_t>(window), st, mix, gend, narrow,
                                  roundMeta, ptr<unsigned long long>(wideFlag));
  else if (frag && range)
    kernels::netScatterFragRange(in, n, (uint32_t)bits, geom, gcur, ptr<uint32_t>(window), st, (uint32_t)keyBits, mix,
                                 gend, narrow, (uint32_t)dLo, (uint32_t)range);
  else if (frag)
    kernels::netScatterFrag(in, n, (uint32_t)bits, geom, 0, geom.blocks, gcur, ptr<uint32_t>(window), st,
                            (uint32_t)keyBits, mix, gend, nm, roundMeta);
  else if (wide)
    kernels::netScatterWide(ptr<const data::Tuple>(tuples), n, (uint32_t)bits, geom, 0, geom.blocks, gcur,
                            ptr<data::Tuple>(window), st, mix, gend, nm);
  else
    kernels::netScatter(in, n, (uint32_t)bits, keyOnly ? 0u : (uint32_t)keyShift, geom, 0, geom.blocks, gcur,
                        ptr<uint64_t>(window), st, (uint32_t)keyBits, mix, gend, nm, !keyOnly, roundMeta);
  HIP_CHECK(hipDeviceSynchronize());

  py::dict d;
  d["window"] = window;
  d["gstart"] = gstartH.view({(int64_t)G, (int64_t)Fp});
  d["gcur"] = cursorsToHost(gcurT, narrow).view({(int64_t)G, (int64_t)Fp});
  d["gend"] = gendH.view({(int64_t)G, (int64_t)Fp});
  d["round_map"] = py::make_tuple(rm.lp, rm.lv, rm.lns);
  d["capacity_used"] = used;
  d["capacity"] = capacity;
  d["blocks"] = geom.blocks;
  d["tiles_per_block"] = geom.tilesPerBlock;
  d["sample_stride"] = stride;
  d["narrow"] = narrow;
  if (packed) d["wide_flag"] = (uint64_t)wideFlag.cpu()[0].item<int64_t>();  // waves that met a fragment above 20 bits
  return d;
}

py::dict opLocalScatterSlices(const at::Tensor &window, const at::Tensor &runsIn, int64_t ownedArg, int64_t shift,
                              int64_t bits, const std::string &mode, std::tuple<int64_t, int64_t, int64_t> roundMap,
                              int64_t fragShift, int64_t loShift, int64_t narrowArg, int64_t sampleStride,
                              int64_t shrink, int64_t guard) {
  const bool compressed = mode == "compressed", wide = mode == "wide", splitMode = mode == "split",
             frag = mode == "frag";
  TORCH_CHECK(compressed || wide || splitMode || frag, "local_scatter_slices: mode ", mode);
  TORCH_CHECK(window.is_cuda() && window.is_contiguous(), "local_scatter_slices: the window is a contiguous device tensor");
  if (wide) {
    TORCH_CHECK(window.dim() == 2 && window.size(1) == 2 && window.scalar_type() == at::kLong,
                "local_scatter_slices: wide windows are int64 [m, 2]");
  } else {
    TORCH_CHECK(window.dim() == 1 && window.scalar_type() == (frag ? at::kInt : at::kLong),
                "local_scatter_slices: ", mode, " windows are 1-D ", frag ? "int32" : "int64");
  }
  TORCH_CHECK(bits >= 0 && bits <= kernels::MAX_PART_BITS && shift >= 0 && shift < 64 && ownedArg >= 0,
              "local_scatter_slices: shift / bits / owned");
  TORCH_CHECK(shrink >= 0 && guard >= 0 && sampleStride >= 1, "local_scatter_slices: negative option");
  at::Tensor runs = runsIn.cpu().to(at::kLong).contiguous();
  TORCH_CHECK(runs.dim() == 2 && runs.size(1) == 3, "local_scatter_slices: runs are [r, 3] (lp, begin, len)");
  HIP_CHECK(hipSetDevice(window.get_device()));
  const hipStream_t st = nullptr;
  kernels::RoundMap rm;
  rm.lp = (uint32_t)std::get<0>(roundMap);
  rm.lv = (uint32_t)std::get<1>(roundMap);
  rm.lns = (uint32_t)std::get<2>(roundMap);
  const uint32_t owned = (uint32_t)ownedArg, F = 1u << bits;
  const uint64_t windowSlots = (uint64_t)window.size(0);

  // partitionImpl(): the lp-sorted items of at most LOCAL_ITEM_MAX tuples.
  std::vector<kernels::LocalItem> items;
  std::vector<uint32_t> lb(owned + 1, 0);
  std::vector<uint64_t> lpBase(owned + 1, 0);
  const int64_t *r = runs.data_ptr<int64_t>();
  int64_t seg = 0;
  const int64_t nRuns = runs.size(0);
  for (uint32_t lp = 0; lp < owned; ++lp) {
    lb[lp] = (uint32_t)items.size();
    uint64_t size = 0;
    for (; seg < nRuns && r[3 * seg] == (int64_t)lp; ++seg) {
      const uint64_t begin = (uint64_t)r[3 * seg + 1], len = (uint64_t)r[3 * seg + 2];
      TORCH_CHECK(r[3 * seg + 1] >= 0 && r[3 * seg + 2] >= 0, "local_scatter_slices: negative run");
      if (!len) continue;
      const uint64_t lastL = begin + len - 1;
      TORCH_CHECK(!rm.on() || (begin >> rm.lv) == (lastL >> rm.lv), "local_scatter_slices: run ", seg,
                  " leaves its round-map slice");
      TORCH_CHECK(rm(lastL) < windowSlots, "local_scatter_slices: run ", seg, " ends at slot ", rm(lastL), " of ",
                  windowSlots);
      for (uint64_t off = 0; off < len; off += kernels::LOCAL_ITEM_MAX)
        items.push_back(kernels::LocalItem{begin + off, (uint32_t)std::min<uint64_t>(kernels::LOCAL_ITEM_MAX, len - off),
                                           lp, 0, 0});
      size += len;
    }
    lpBase[lp + 1] = lpBase[lp] + size;
  }
  TORCH_CHECK(seg == nRuns, "local_scatter_slices: runs must be sorted by lp < owned");
  lb[owned] = (uint32_t)items.size();
  const uint32_t nItems = (uint32_t)items.size();
  const uint64_t recvTotal = lpBase[owned];

  kernels::SplitLayout split;
  split.on = !wide && (splitMode || frag) ? 1u : 0u;
  split.fragShift = (uint32_t)fragShift;
  split.loShift = (uint32_t)loShift;
  const uint32_t align = split.on ? 64 : 16;
  const at::ScalarType mainType = frag ? at::kShort : split.on ? at::kInt : at::kLong;
  auto column = [&](uint64_t slots, at::ScalarType t) {
    if (wide) return sentinelFilled({(int64_t)slots, 2}, window, t);
    return sentinelFilled({(int64_t)slots}, window, t);
  };
  auto toDevice = [&](const void *src, size_t bytes) {
    at::Tensor t = at::empty({(int64_t)(bytes + 7) / 8 + 1}, on(window, at::kLong));
    if (bytes) HIP_CHECK(hipMemcpy(t.data_ptr(), src, bytes, hipMemcpyHostToDevice));
    return t;
  };
  at::Tensor itemHist = at::zeros({std::max<int64_t>(1, (int64_t)nItems * F)}, on(window, at::kInt));
  const uint64_t P = (uint64_t)owned * F;
  py::dict d;

  if (sampleStride > 1) {
    for (auto &x : items) x.stream = x.lp;
    const uint32_t S = (uint32_t)sampleStride;
    const uint64_t cap = kernels::localSampledCapacityBound(recvTotal, P, S, align);
    const uint64_t slots = std::max<uint64_t>(cap, 1) + (uint64_t)guard;
    at::Tensor out = column(slots, mainType), hi;
    if (frag)
      split.hi = ptr<uint16_t>(out);
    else if (split.on) {
      hi = column(slots, at::kShort);
      split.hi = ptr<uint16_t>(hi);
    }
    const int64_t Pn = (int64_t)std::max<uint64_t>(P, 1);
    at::Tensor caps = at::zeros({Pn}, on(window, at::kInt));
    at::Tensor starts = at::zeros({Pn}, on(window, at::kLong));
    at::Tensor scanWs = at::empty({(int64_t)kernels::scanWorkspaceBytes(Pn) / 8 + 1}, on(window, at::kLong));
    at::Tensor gcur = at::zeros({Pn}, on(window, at::kLong));
    at::Tensor gend = at::zeros({Pn}, on(window, at::kLong));
    at::Tensor pbeg = at::zeros({Pn}, on(window, at::kLong));
    at::Tensor flag = at::zeros({1}, on(window, at::kInt));
    at::Tensor dItems = toDevice(items.data(), (size_t)nItems * sizeof(kernels::LocalItem));
    at::Tensor dLb = toDevice(lb.data(), (owned + 1) * 4ull);
    const auto *di = ptr<const kernels::LocalItem>(dItems);
    kernels::localHistogram(window.data_ptr(), wide, di, nItems, (uint32_t)shift, (uint32_t)bits,
                            ptr<uint32_t>(itemHist), st, S, frag, rm);
    kernels::localSampledLayout(ptr<uint32_t>(itemHist), ptr<uint32_t>(dLb), di, owned, (uint32_t)bits, S,
                                ptr<uint32_t>(caps), ptr<unsigned long long>(starts), scanWs.data_ptr(),
                                ptr<unsigned long long>(gcur), ptr<unsigned long long>(gend), ptr<uint64_t>(pbeg), cap,
                                st, align);
    if (shrink) shrinkSlices(pbeg, gend, shrink);
    kernels::localScatter(window.data_ptr(), wide, di, nItems, (uint32_t)shift, (uint32_t)bits, gcur.data_ptr(), false,
                          out.data_ptr(), st, gend.data_ptr(), split, frag, rm);
    HIP_CHECK(hipDeviceSynchronize());
    at::Tensor claimed = gcur.clone();  // before the clamp
    kernels::claimOverflow(ptr<unsigned long long>(gcur), ptr<unsigned long long>(gend), P, ptr<unsigned int>(flag), st);
    HIP_CHECK(hipDeviceSynchronize());
    at::Tensor pb = pbeg.cpu().slice(0, 0, (int64_t)P);
    d["out"] = out;
    d["hi"] = hi.defined() ? py::cast(hi) : py::none();
    d["part_begin"] = pb;
    d["part_end"] = gcur.cpu().slice(0, 0, (int64_t)P);
    d["slot_end"] = gend.cpu().slice(0, 0, (int64_t)P);
    d["demand"] = claimed.cpu().slice(0, 0, (int64_t)P) - pb;
    d["overflow"] = flag.cpu()[0].item<int32_t>() != 0;
    d["capacity"] = cap;
    d["items"] = nItems;
    return d;
  }

  const uint64_t slots = std::max<uint64_t>(recvTotal, 1) + (uint64_t)guard;
  at::Tensor out = column(slots, mainType), hi;
  if (frag)
    split.hi = ptr<uint16_t>(out);
  else if (split.on) {
    hi = column(slots, at::kShort);
    split.hi = ptr<uint16_t>(hi);
  }
  at::Tensor partBegin = at::zeros({(int64_t)P + 1}, on(window, at::kLong));
  const uint32_t streams = kernels::assignLocalStreams(items.data(), nItems);
  const bool narrow = narrowArg < 0 ? kernels::cursorsNarrow(recvTotal) : narrowArg != 0;
  TORCH_CHECK(!narrow || kernels::cursorsNarrow(recvTotal), "local_scatter_slices: 32-bit cursors wrap");
  at::Tensor gcur = at::zeros({std::max<int64_t>(1, (int64_t)streams * F)}, on(window, at::kLong));
  at::Tensor dItems = toDevice(items.data(), (size_t)nItems * sizeof(kernels::LocalItem));
  at::Tensor dLb = toDevice(lb.data(), (owned + 1) * 4ull);
  at::Tensor dBase = toDevice(lpBase.data(), (owned + 1) * 8ull);
  const auto *di = ptr<const kernels::LocalItem>(dItems);
  kernels::localHistogram(window.data_ptr(), wide, di, nItems, (uint32_t)shift, (uint32_t)bits, ptr<uint32_t>(itemHist),
                          st, 1, frag, rm);
  kernels::localCursors(ptr<uint32_t>(itemHist), ptr<uint32_t>(dLb), owned, (uint32_t)bits, ptr<uint64_t>(dBase), di,
                        gcur.data_ptr(), narrow, ptr<uint64_t>(partBegin), st);
  kernels::localScatter(window.data_ptr(), wide, di, nItems, (uint32_t)shift, (uint32_t)bits, gcur.data_ptr(), narrow,
                        out.data_ptr(), st, nullptr, split, frag, rm);
  HIP_CHECK(hipDeviceSynchronize());
  at::Tensor pb = partBegin.cpu();
  d["out"] = out;
  d["hi"] = hi.defined() ? py::cast(hi) : py::none();
  d["part_begin"] = pb;
  d["part_end"] = pb.slice(0, 1);
  d["slot_end"] = pb.slice(0, 1);
  d["demand"] = pb.slice(0, 1) - pb.slice(0, 0, (int64_t)P);
  d["overflow"] = false;
  d["capacity"] = std::max<uint64_t>(recvTotal, 1);
  d["items"] = nItems;
  return d;
}

at::Tensor opKeyMix(const at::Tensor &keys, int64_t bits) {
  TORCH_CHECK(!keys.is_cuda() && keys.scalar_type() == at::kLong, "key_mix: a host int64 tensor");
  TORCH_CHECK(bits >= 1 && bits <= 64, "key_mix: bits=", bits);
  at::Tensor in = keys.contiguous(), out = at::empty_like(in);
  const kernels::KeyMix mix{1u, (uint32_t)bits};
  const uint64_t *k = ptr<const uint64_t>(in);
  uint64_t *o = ptr<uint64_t>(out);
  for (int64_t i = 0; i < in.numel(); ++i) o[i] = mix.apply(k[i]);
  return out;
}

// Host twins of the packed fragment word (kernels.h, PK_*; kernels::packFragments).
at::Tensor opPackFragments(const at::Tensor &frags, const at::Tensor &counts) {
  TORCH_CHECK(!frags.is_cuda() && frags.scalar_type() == at::kLong && frags.dim() == 2 &&
                  frags.size(1) == kernels::PK_WORD_FRAGS && !counts.is_cuda() && counts.scalar_type() == at::kLong &&
                  counts.dim() == 1 && counts.size(0) == frags.size(0),
              "pack_fragments: host int64 fragments [m, 3] and counts [m]");
  at::Tensor f = frags.contiguous(), c = counts.contiguous(), out = at::empty({f.size(0)}, f.options());
  const int64_t *pf = f.data_ptr<int64_t>(), *pc = c.data_ptr<int64_t>();
  uint64_t *po = ptr<uint64_t>(out);
  for (int64_t i = 0; i < f.size(0); ++i) {
    TORCH_CHECK(pc[i] >= 0 && pc[i] <= (int64_t)kernels::PK_WORD_FRAGS, "pack_fragments: count ", pc[i]);
    for (int e = 0; e < 3; ++e)
      TORCH_CHECK(pf[3 * i + e] >= 0 && pf[3 * i + e] < (int64_t)1 << kernels::PK_FRAG_BITS,
                  "pack_fragments: fragment ", pf[3 * i + e], " does not fit ", kernels::PK_FRAG_BITS, " bits");
    po[i] = kernels::packFragments((uint32_t)pf[3 * i], (uint32_t)pf[3 * i + 1], (uint32_t)pf[3 * i + 2],
                                   (uint32_t)pc[i]);
  }
  return out;
}

py::tuple opUnpackFragments(const at::Tensor &words) {
  TORCH_CHECK(!words.is_cuda() && words.scalar_type() == at::kLong && words.dim() == 1,
              "unpack_fragments: a host int64 tensor of words");
  at::Tensor w = words.contiguous();
  at::Tensor frags = at::empty({w.size(0), (int64_t)kernels::PK_WORD_FRAGS}, w.options());
  at::Tensor counts = at::empty({w.size(0)}, w.options());
  const uint64_t *pw = ptr<const uint64_t>(w);
  int64_t *pf = frags.data_ptr<int64_t>(), *pc = counts.data_ptr<int64_t>();
  const uint64_t m = (1ull << kernels::PK_FRAG_BITS) - 1;
  for (int64_t i = 0; i < w.size(0); ++i) {
    for (uint32_t e = 0; e < kernels::PK_WORD_FRAGS; ++e)
      pf[3 * i + e] = (int64_t)((pw[i] >> (kernels::PK_FRAG_BITS * e)) & m);
    pc[i] = (int64_t)(pw[i] >> 60);
  }
  return py::make_tuple(frags, counts);
}

}  // namespace

void bindScatterOps(py::module_ &ops) {
  ops.def("pack_fragments", &opPackFragments, py::arg("frags"), py::arg("counts"),
          "Packed fragment words (three 20-bit fragments, count in bits 60-63) from [m, 3] fragments and [m] counts");
  ops.def("unpack_fragments", &opUnpackFragments, py::arg("words"), "(fragments [m, 3], counts [m]) of packed words");
  ops.def("net_scatter_slices", &opNetScatterSlices, py::arg("tuples"), py::arg("bits"), py::arg("format"),
          py::arg("key_shift") = 32, py::arg("key_bits") = 64, py::arg("mix_bits") = 0, py::arg("narrow") = -1,
          py::arg("max_blocks") = 2048, py::arg("sample_stride") = 1, py::arg("round_lp") = 0, py::arg("d_lo") = 0,
          py::arg("range") = 0, py::arg("shrink") = 0, py::arg("guard") = 0, py::arg("unbounded") = false,
          "The sampled network pass of one relation (layout + bounded claim scatter) into a sentinel-filled window; "
          "format = compressed | key_only | frag | wide | frag_packed (window and slice tables in packed u64 words); "
          "tuples may be a 1-D key column for the formats without a rid (key_only, frag, frag_packed)");
  ops.def("local_scatter_slices", &opLocalScatterSlices, py::arg("window"), py::arg("runs"), py::arg("owned"),
          py::arg("shift"), py::arg("bits"), py::arg("mode"), py::arg("round_map") = std::make_tuple(0, 0, 0),
          py::arg("frag_shift") = 32, py::arg("lo_shift") = 0, py::arg("narrow") = -1, py::arg("sample_stride") = 1,
          py::arg("shrink") = 0, py::arg("guard") = 0,
          "The local pass over runs (lp, begin, len) of logical window positions into sentinel-filled columns; "
          "mode = compressed | wide | split | frag");
  ops.def("key_mix", &opKeyMix, py::arg("keys"), py::arg("bits"), "KeyMix{1, bits}.apply, element-wise (host)");
  ops.def("scatter_sentinel", []() { return (int64_t)SENTINEL; });
  ops.def("local_item_max", []() { return kernels::LOCAL_ITEM_MAX; });
}
