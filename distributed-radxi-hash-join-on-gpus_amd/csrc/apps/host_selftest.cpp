// Host-path self test for sanitizer builds (SURVEY §5 "race detection /
// sanitizers": the reference has none and its kernels race).  GPU sanitizers
// are not available on the MI355X pool, so the host runtime -- tasks,
// histograms, offsets, windows, the in-process communicator's threads, late
// materialization and failure propagation -- is exercised here under
// AddressSanitizer + UBSan and, in a second build, ThreadSanitizer
// (tools/sanitize_host.sh, tests/test_sanitizers.py).
//
//   host_selftest [--ranks N] [--size G]
// Exit code 0 iff every join matches its oracle.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../comm/InProcessCommunicator.h"
#include "../core/ExecContext.h"
#include "../data/Relation.h"
#include "../kernels/kernels.h"
#include "../operators/HashJoin.h"
#include "../operators/LateMaterialization.h"
#include "../utils/Fault.h"

using namespace hpcjoin;

namespace {

struct Case {
  const char *name;
  kernels::KeyDistribution outer;
  bool wide, materialize, tpch;
  core::KeyHashing hashing;
  bool wire = false;  // bit-packed exchange (host twin of kernels/wire.hip)
  // semi / anti: outer rids, outer kinds: NULL-padded rows, each checked against a set oracle
  core::JoinKind kind = core::JoinKind::Inner;
  // semi / anti on the set-semantics bitmap plan (JoinConfig::semiBitmap): one rank, the plan must be taken
  bool semiBitmap = false;
  // kind Group: sum an outer value column per group (HashJoin::joinGroup with one int64 SUM column; one rank), else counts only
  bool groupValues = false;
  // kind Group: sum, min and max of three strided outer columns per group (HashJoin::joinGroup; one rank)
  bool groupAgg = false;
  // kind Group: typed columns -- float64 sum, float32 min (stride 2), int32 max (stride 3) per group
  bool groupTyped = false;
};

// The value of outer tuple `rid` in the group-join cases: spread over the int64 range, so the sums wrap.
uint64_t groupValue(uint64_t rid) { return kernels::mix64(rid + 77) * 0x9E3779B97F4A7C15ull; }
// The typed columns of outer tuple `rid`: multiples of 1/8 below 2^27 (every partial sum is exact in binary64,
// whatever the order), float32 values exact in their type, and int32 values over the whole range.
double groupF64(uint64_t rid) { return (double)((int64_t)(groupValue(rid) >> 33) - (int64_t(1) << 30)) / 8.0; }
float groupF32(uint64_t rid) { return (float)((int64_t)(groupValue(rid + 5) >> 43) - (int64_t(1) << 20)) / 8.0f; }
int32_t groupI32(uint64_t rid) { return (int32_t)(uint32_t)(groupValue(rid + 9) >> 32); }
uint64_t bitsOf(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

bool runCase(const Case &c, uint32_t ranks, uint64_t G) {
  if (c.semiBitmap || c.groupValues || c.groupAgg || c.groupTyped) ranks = 1;
  auto group = std::make_shared<comm::InProcessGroup>(ranks);
  std::vector<std::string> errors(ranks);
  std::vector<uint64_t> matches(ranks, 0), pairs(ranks, 0);
  std::vector<std::vector<uint64_t>> rids(ranks);
  std::vector<std::vector<std::pair<uint64_t, uint64_t>>> rows(ranks);
  const bool inner = c.kind == core::JoinKind::Inner, outerKind = core::isOuterKind(c.kind);
  const bool groupKind = c.kind == core::JoinKind::Group;
  std::vector<std::vector<uint64_t>> groups(ranks);  // group rows, 2 or 3 words each
  data::GenSpec is, os;
  is.seed = 11;
  is.tpchSparse = c.tpch;
  os.seed = 12;
  os.distribution = c.outer;
  os.domain = c.outer == kernels::KeyDistribution::Unique ? 0 : G;
  os.tpchSparse = c.tpch;
  if (!inner) {  // repeated inner keys, and half of the outer key domain without a partner
    is.distribution = kernels::KeyDistribution::Uniform;
    is.domain = G / 4;
    os.domain = 2 * G;
  }
  const uint64_t GS = c.outer == kernels::KeyDistribution::Unique ? G : 3 * G;
  auto rankMain = [&](uint32_t r) {
    try {
      comm::InProcessCommunicator comm(group, r);
      core::ExecContext ctx(Location::Host, -1, &comm);
      data::Relation R(data::Relation::localSizeFor(G, r, ranks), G, Location::Host, 0);
      data::Relation S(data::Relation::localSizeFor(GS, r, ranks), GS, Location::Host, 0);
      R.generate(is, data::Relation::localOffsetFor(G, r, ranks));
      S.generate(os, data::Relation::localOffsetFor(GS, r, ranks));
      core::JoinConfig cfg;
      cfg.format = c.wide ? core::TupleFormat::Wide : core::TupleFormat::Compressed;
      cfg.materialize = c.materialize;
      cfg.kind = c.kind;
      cfg.keyHashing = c.hashing;
      cfg.chunks = 2;
      cfg.wireCodec = c.wire ? core::WireCodecMode::On : core::WireCodecMode::Off;
      cfg.semiBitmap = c.semiBitmap;
      if (c.groupAgg || c.groupTyped) cfg.groupColumns = 3;
      operators::HashJoin j(&R, &S, &ctx, cfg);
      if (c.semiBitmap && !(j.getPlan().bitmapJoin && j.getPlan().bitmapSet))
        throw std::runtime_error("the set bitmap plan was not taken");
      std::vector<uint64_t> values;
      if (c.groupValues) {  // strided column: word 1 of 3-word rows, rids from 0 (one rank)
        values.assign(3 * GS, 0);
        for (uint64_t i = 0; i < GS; ++i) values[3 * i + 1] = groupValue(i);
      }
      kernels::GroupColumns cols;
      if (c.groupValues) {
        cols.n = 1;
        cols.col[0] = values.data() + 1;
        cols.stride[0] = 3;
      }
      if (c.groupAgg) {  // words 0, 1, 2 of 3-word rows: sum of the first, min of the second, max of the third
        values.assign(3 * GS, 0);
        for (uint64_t i = 0; i < 3 * GS; ++i) values[i] = groupValue(i);
        cols.n = 3;
        for (uint32_t k = 0; k < 3; ++k) {
          cols.col[k] = reinterpret_cast<const unsigned long long *>(values.data()) + k;
          cols.stride[k] = 3;
        }
        cols.agg[0] = kernels::GROUP_SUM;
        cols.agg[1] = kernels::GROUP_MIN;
        cols.agg[2] = kernels::GROUP_MAX;
      }
      std::vector<double> f64;
      std::vector<float> f32;
      std::vector<int32_t> i32;
      if (c.groupTyped) {  // one tensor per type; the 4-byte columns are strided views (element strides 2 and 3)
        f64.resize(GS);
        f32.assign(2 * GS, 0.0f);
        i32.assign(3 * GS, 0);
        for (uint64_t i = 0; i < GS; ++i) {
          f64[i] = groupF64(i);
          f32[2 * i + 1] = groupF32(i);
          i32[3 * i + 2] = groupI32(i);
        }
        cols.n = 3;
        cols.col[0] = f64.data();
        cols.col[1] = f32.data() + 1;
        cols.col[2] = i32.data() + 2;
        cols.stride[1] = 2;
        cols.stride[2] = 3;
        cols.dtype[0] = kernels::GROUP_F64;
        cols.dtype[1] = kernels::GROUP_F32;
        cols.dtype[2] = kernels::GROUP_I32;
        cols.agg[0] = kernels::GROUP_SUM;
        cols.agg[1] = kernels::GROUP_MIN;
        cols.agg[2] = kernels::GROUP_MAX;
      }
      operators::JoinResult res = cols.n ? j.joinGroup(cols, 0, GS, "joinGroup") : j.run();
      if (groupKind) {
        const uint64_t W = c.groupAgg || c.groupTyped ? 5 : c.groupValues ? 3 : 2;
        if (res.localMatches != res.outputGroups || res.unmatchedOuter != 0 || res.outputPairs != 0 ||
            res.outputRids != 0 || (res.groupColumns == 1) != c.groupValues || res.groupColumns != W - 2 || !j.getOutputGroups())
          throw std::runtime_error("group join: the result fields do not add up");
        groups[r].assign(j.getOutputGroups(), j.getOutputGroups() + res.outputGroups * W);
        uint64_t pairsSum = 0, zeros = 0;
        for (uint64_t i = 0; i < res.outputGroups; ++i) {
          pairsSum += groups[r][i * W + 1];
          zeros += groups[r][i * W + 1] == 0;
        }
        if (pairsSum != res.matchedPairs || zeros != res.unmatchedInner)
          throw std::runtime_error("group join: matchedPairs / unmatchedInner differ from the rows");
      }
      if (c.semiBitmap && !(res.bitmapJoin && res.localFallbacks == 0 && res.outputPairs == 0 &&
                            res.outputRids == (c.materialize ? res.localMatches : 0)))
        throw std::runtime_error("set bitmap plan: the result fields do not add up");
      matches[r] = res.globalMatches;
      pairs[r] = res.outputPairs;
      if (groupKind) {
      } else if (outerKind) {
        if (res.localMatches != res.matchedPairs + res.unmatchedInner + res.unmatchedOuter ||
            res.outputPairs != (c.materialize ? res.localMatches : 0) || res.outputRids != 0)
          throw std::runtime_error("outer join: the result fields do not add up");
        for (uint64_t i = 0; i < res.outputPairs; ++i) rows[r].emplace_back(j.getOutput()[i].x, j.getOutput()[i].y);
      } else if (!inner && c.materialize) {
        rids[r].assign(j.getOutputRids(), j.getOutputRids() + res.outputRids);
      }
      if (inner && c.materialize) {  // fetch 32-byte payload rows of both sides from their owners
        const uint64_t oR = data::Relation::localOffsetFor(G, r, ranks), oS = data::Relation::localOffsetFor(GS, r, ranks);
        std::vector<uint64_t> rowsR(R.getLocalSize() * kernels::ROW_WORDS), rowsS(S.getLocalSize() * kernels::ROW_WORDS);
        for (uint64_t i = 0; i < R.getLocalSize(); ++i)
          for (uint32_t w = 0; w < kernels::ROW_WORDS; ++w) rowsR[i * kernels::ROW_WORDS + w] = kernels::payloadWord(1, oR + i, w);
        for (uint64_t i = 0; i < S.getLocalSize(); ++i)
          for (uint32_t w = 0; w < kernels::ROW_WORDS; ++w) rowsS[i * kernels::ROW_WORDS + w] = kernels::payloadWord(2, oS + i, w);
        operators::PayloadColumn a{rowsR.data(), R.getLocalSize(), oR, G}, b{rowsS.data(), S.getLocalSize(), oS, GS};
        operators::LateMaterialization lm(&ctx, a, b);
        std::vector<uint64_t> out(res.outputPairs * operators::LateMaterialization::OUT_WORDS + 1);
        lm.materialize(j.getOutput(), res.outputPairs, out.data());
        for (uint64_t i = 0; i < res.outputPairs; ++i) {
          const uint64_t *row = &out[i * operators::LateMaterialization::OUT_WORDS];
          for (uint32_t w = 0; w < kernels::ROW_WORDS; ++w)
            if (row[2 + w] != kernels::payloadWord(1, row[0], w) || row[6 + w] != kernels::payloadWord(2, row[1], w))
              throw std::runtime_error("payload row does not belong to its rid");
        }
      }
    } catch (const std::exception &e) {
      errors[r] = e.what();
    }
  };
  std::vector<std::thread> ts;
  for (uint32_t r = 0; r < ranks; ++r) ts.emplace_back(rankMain, r);
  for (auto &t : ts) t.join();
  uint64_t expected = data::Relation::expectedMatches(is, G, os, GS);
  std::unordered_set<uint64_t> expectedRids;
  std::set<std::pair<uint64_t, uint64_t>> expectedRows;
  if (outerKind) {  // the inner join's pairs and one NULL-padded row per unmatched tuple of a preserved side
    data::Relation R(G, G, Location::Host, 0), S(GS, GS, Location::Host, 0);
    R.generate(is, 0);
    S.generate(os, 0);
    std::unordered_map<uint64_t, std::vector<uint64_t>> byKey;
    std::unordered_set<uint64_t> probed;
    for (uint64_t i = 0; i < G; ++i) byKey[R.getData()[i].key].push_back(R.getData()[i].rid);
    for (uint64_t i = 0; i < GS; ++i) {
      auto it = byKey.find(S.getData()[i].key);
      if (it == byKey.end()) {
        if (core::preservesOuter(c.kind)) expectedRows.emplace(kernels::NULL_RID, S.getData()[i].rid);
        continue;
      }
      probed.insert(it->first);
      for (uint64_t rid : it->second) expectedRows.emplace(rid, S.getData()[i].rid);
    }
    if (core::preservesInner(c.kind))
      for (const auto &kv : byKey)
        if (!probed.count(kv.first))
          for (uint64_t rid : kv.second) expectedRows.emplace(rid, kernels::NULL_RID);
    expected = expectedRows.size();
  } else if (groupKind) {  // per inner tuple the count (and wrapping sum) of the outer tuples with its key
    expected = G;
  } else if (!inner) {  // the outer tuples whose key is (semi) / is not (anti) among the inner keys
    data::Relation R(G, G, Location::Host, 0), S(GS, GS, Location::Host, 0);
    R.generate(is, 0);
    S.generate(os, 0);
    std::unordered_set<uint64_t> keys;
    for (uint64_t i = 0; i < G; ++i) keys.insert(R.getData()[i].key);
    for (uint64_t i = 0; i < GS; ++i)
      if ((keys.count(S.getData()[i].key) != 0) == (c.kind == core::JoinKind::Semi)) expectedRids.insert(S.getData()[i].rid);
    expected = expectedRids.size();
  }
  bool ok = true;
  for (uint32_t r = 0; r < ranks; ++r) {
    if (!errors[r].empty()) {
      std::printf("[%s] rank %u failed: %s\n", c.name, r, errors[r].c_str());
      ok = false;
    } else if (matches[r] != expected) {
      std::printf("[%s] rank %u: %lu matches, expected %lu\n", c.name, r, (unsigned long)matches[r],
                  (unsigned long)expected);
      ok = false;
    }
  }
  if (ok && c.materialize && outerKind) {  // the ranks' rows together: the oracle set, no row twice
    std::set<std::pair<uint64_t, uint64_t>> seen;
    for (const auto &v : rows)
      for (const auto &x : v)
        if (!expectedRows.count(x) || !seen.insert(x).second) ok = false;
    if (seen.size() != expected) ok = false;
    if (!ok) std::printf("[%s] rows differ from the oracle (%lu distinct, expected %lu)\n", c.name,
                         (unsigned long)seen.size(), (unsigned long)expected);
  }
  if (ok && groupKind) {  // the ranks' rows together: every inner rid once, with the oracle's count and sum
    data::Relation R(G, G, Location::Host, 0), S(GS, GS, Location::Host, 0);
    R.generate(is, 0);
    S.generate(os, 0);
    std::unordered_map<uint64_t, std::pair<uint64_t, uint64_t>> byKey;  // outer key -> (count, sum)
    struct Agg {
      uint64_t sum = 0;
      int64_t min = INT64_MAX, max = INT64_MIN;
    };
    std::unordered_map<uint64_t, Agg> aggByKey;  // groupAgg: outer key -> (sum of word 0, min of word 1, max of word 2)
    struct Typed {
      double sum = 0.0, min = HUGE_VAL;
      int64_t max = INT64_MIN;
    };
    std::unordered_map<uint64_t, Typed> typedByKey;  // groupTyped: outer key -> (float64 sum, float32 min, int32 max)
    for (uint64_t i = 0; i < GS; ++i) {
      auto &e = byKey[S.getData()[i].key];
      ++e.first;
      e.second += groupValue(S.getData()[i].rid);
      if (c.groupAgg) {
        Agg &g = aggByKey[S.getData()[i].key];
        const uint64_t rid = S.getData()[i].rid;
        g.sum += groupValue(3 * rid);
        g.min = std::min(g.min, (int64_t)groupValue(3 * rid + 1));
        g.max = std::max(g.max, (int64_t)groupValue(3 * rid + 2));
      }
      if (c.groupTyped) {
        Typed &g = typedByKey[S.getData()[i].key];
        const uint64_t rid = S.getData()[i].rid;
        g.sum += groupF64(rid);
        g.min = std::min(g.min, (double)groupF32(rid));
        g.max = std::max(g.max, (int64_t)groupI32(rid));
      }
    }
    std::unordered_map<uint64_t, uint64_t> keyOf;  // inner rid -> key
    for (uint64_t i = 0; i < G; ++i) keyOf[R.getData()[i].rid] = R.getData()[i].key;
    const uint64_t W = c.groupAgg || c.groupTyped ? 5 : c.groupValues ? 3 : 2;
    std::unordered_set<uint64_t> seen;
    uint64_t repeated = 0, empty = 0;
    for (const auto &v : groups)
      for (uint64_t i = 0; i + W <= v.size(); i += W) {
        auto k = keyOf.find(v[i]);
        if (k == keyOf.end() || !seen.insert(v[i]).second) {
          ok = false;
          continue;
        }
        auto e = byKey.find(k->second);
        const uint64_t cnt = e == byKey.end() ? 0 : e->second.first, sum = e == byKey.end() ? 0 : e->second.second;
        if (v[i + 1] != cnt || (c.groupValues && v[i + 2] != sum)) ok = false;
        if (c.groupAgg) {  // an empty group carries the identities
          const Agg g = e == byKey.end() ? Agg() : aggByKey[k->second];
          if (v[i + 2] != g.sum || (int64_t)v[i + 3] != g.min || (int64_t)v[i + 4] != g.max) ok = false;
        }
        if (c.groupTyped) {  // bit for bit: +0.0 and +inf in the float words of an empty group, INT64_MIN in the int32's
          const Typed g = e == byKey.end() ? Typed() : typedByKey[k->second];
          if (v[i + 2] != bitsOf(g.sum) || v[i + 3] != bitsOf(g.min) || (int64_t)v[i + 4] != g.max) ok = false;
        }
        empty += cnt == 0;
      }
    if (seen.size() != G) ok = false;
    std::unordered_map<uint64_t, uint64_t> copies;
    for (uint64_t i = 0; i < G; ++i) ++copies[R.getData()[i].key];
    for (const auto &kc : copies) repeated += kc.second > 1 ? kc.second : 0;
    if (repeated * 5 < G || empty == 0) ok = false;  // the case must have repeated inner keys and empty groups
    if (!ok) std::printf("[%s] group rows differ from the oracle (%lu distinct rids, expected %lu)\n", c.name,
                         (unsigned long)seen.size(), (unsigned long)G);
  }
  if (ok && c.materialize && !inner && !outerKind && !groupKind) {  // the ranks' rid lists together: the oracle set, no rid twice
    std::unordered_set<uint64_t> seen;
    for (const auto &v : rids)
      for (uint64_t x : v)
        if (!expectedRids.count(x) || !seen.insert(x).second) ok = false;
    if (seen.size() != expected) ok = false;
    if (!ok) std::printf("[%s] rid lists differ from the oracle (%lu distinct, expected %lu)\n", c.name,
                         (unsigned long)seen.size(), (unsigned long)expected);
  }
  if (ok && c.materialize && inner) {
    uint64_t total = 0;
    for (uint64_t p : pairs) total += p;
    if (total != expected) {
      std::printf("[%s] %lu pairs, expected %lu\n", c.name, (unsigned long)total, (unsigned long)expected);
      ok = false;
    }
  }
  std::printf("[%s] ranks=%u %s\n", c.name, ranks, ok ? "OK" : "FAIL");
  return ok;
}

// A rank failing mid-join must make every peer fail (not hang), under the sanitizers too.
bool runFaultCase(uint32_t ranks, uint64_t G) {
  auto group = std::make_shared<comm::InProcessGroup>(ranks);
  std::vector<int> failed(ranks, 0);
  auto rankMain = [&](uint32_t r) {
    try {
      utils::armFault("network", 1);
      comm::InProcessCommunicator comm(group, r);
      core::ExecContext ctx(Location::Host, -1, &comm);
      data::Relation R(data::Relation::localSizeFor(G, r, ranks), G, Location::Host, 0);
      data::Relation S(data::Relation::localSizeFor(G, r, ranks), G, Location::Host, 0);
      R.generate(data::GenSpec(), data::Relation::localOffsetFor(G, r, ranks));
      S.generate(data::GenSpec(), data::Relation::localOffsetFor(G, r, ranks));
      operators::HashJoin j(&R, &S, &ctx, core::JoinConfig());
      j.run();
    } catch (const std::exception &) {
      failed[r] = 1;
    }
    utils::armFault("", -1);
  };
  std::vector<std::thread> ts;
  for (uint32_t r = 0; r < ranks; ++r) ts.emplace_back(rankMain, r);
  for (auto &t : ts) t.join();
  bool ok = true;
  for (int f : failed) ok = ok && f;
  std::printf("[fault] ranks=%u %s\n", ranks, ok ? "OK" : "FAIL");
  return ok;
}

// Key-column relations on the host path: every rank holds a slice of two key
// columns (rids = global positions) and the materializing join of the
// expansions must give the pairs of the tuple relations built from the same
// keys and rids.  The expansion is allocated, filled and freed under the
// sanitizers.
bool runKeyColumnCase(uint32_t ranks, uint64_t G) {
  std::vector<uint64_t> keys[2];
  for (int s = 0; s < 2; ++s) {
    keys[s].resize(G);
    for (uint64_t i = 0; i < G; ++i) keys[s][i] = kernels::mix64(i * 2 + s + 7) % (G / 2 + 1);
  }
  auto group = std::make_shared<comm::InProcessGroup>(ranks);
  std::vector<std::vector<std::pair<uint64_t, uint64_t>>> got(2 * ranks);
  std::vector<int> failed(ranks, 0);
  auto rankMain = [&](uint32_t r) {
    try {
      comm::InProcessCommunicator comm(group, r);
      core::ExecContext ctx(Location::Host, -1, &comm);
      core::JoinConfig cfg;
      cfg.materialize = true;
      cfg.outputCapacity = 8 * G;  // keys repeat on both sides: about two pairs per outer tuple, on whichever rank
      const uint64_t off = data::Relation::localOffsetFor(G, r, ranks), n = data::Relation::localSizeFor(G, r, ranks);
      for (int columns = 1; columns >= 0; --columns) {
        std::unique_ptr<data::Relation> rel[2];
        for (int s = 0; s < 2; ++s) {
          if (columns) {
            rel[s].reset(new data::Relation(keys[s].data() + off, n, G, Location::Host, 0, off));
          } else {
            rel[s].reset(new data::Relation(n, G, Location::Host, 0));
            for (uint64_t i = 0; i < n; ++i) rel[s]->getData()[i] = data::Tuple{keys[s][off + i], off + i};
          }
        }
        operators::HashJoin j(rel[0].get(), rel[1].get(), &ctx, cfg);
        const operators::JoinResult res = j.run();
        const auto want = columns ? operators::JoinResult::Expanded : operators::JoinResult::Tuples;
        if (res.keyColumns[0] != want || res.keyColumns[1] != want || rel[0]->expanded() != (columns == 1) ||
            res.outputOverflow)
          failed[r] = 1;
        const ulonglong2 *out = j.getOutput();
        for (uint64_t i = 0; i < res.outputPairs; ++i) got[2 * r + columns].emplace_back(out[i].x, out[i].y);
      }
    } catch (const std::exception &e) {
      std::printf("[key_columns] rank %u: %s\n", r, e.what());
      failed[r] = 1;
    }
  };
  std::vector<std::thread> ts;
  for (uint32_t r = 0; r < ranks; ++r) ts.emplace_back(rankMain, r);
  for (auto &t : ts) t.join();
  bool ok = true;
  std::vector<std::pair<uint64_t, uint64_t>> all[2];
  for (uint32_t r = 0; r < ranks; ++r) {
    ok = ok && !failed[r];
    for (int c = 0; c < 2; ++c) all[c].insert(all[c].end(), got[2 * r + c].begin(), got[2 * r + c].end());
  }
  for (auto &a : all) std::sort(a.begin(), a.end());
  uint64_t expected = 0;
  {
    std::unordered_map<uint64_t, uint64_t> copies;
    for (uint64_t k : keys[0]) ++copies[k];
    for (uint64_t k : keys[1]) {
      auto it = copies.find(k);
      if (it != copies.end()) expected += it->second;
    }
  }
  ok = ok && all[0] == all[1] && all[1].size() == expected;
  for (const auto &p : all[1]) ok = ok && p.first < G && p.second < G && keys[0][p.first] == keys[1][p.second];
  std::printf("[key_columns] ranks=%u pairs=%lu expected=%lu %s\n", ranks, (unsigned long)all[1].size(),
              (unsigned long)expected, ok ? "OK" : "FAIL");
  return ok;
}

}  // namespace

int main(int argc, char **argv) {
  uint32_t ranks = 3;
  uint64_t G = 50000;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--ranks") && i + 1 < argc) ranks = (uint32_t)std::stoul(argv[++i]);
    else if (!std::strcmp(argv[i], "--size") && i + 1 < argc) G = std::stoull(argv[++i]);
  }
  utils::setCommTimeoutMs(60000);
  const Case cases[] = {
      {"unique", kernels::KeyDistribution::Unique, false, false, false, core::KeyHashing::Auto},
      {"zipf", kernels::KeyDistribution::Zipf, false, false, false, core::KeyHashing::Auto},
      {"wide_materialize", kernels::KeyDistribution::Uniform, true, true, false, core::KeyHashing::Auto},
      {"tpch_materialize", kernels::KeyDistribution::Modulo, false, true, true, core::KeyHashing::Auto},
      {"mix_on_wide", kernels::KeyDistribution::Modulo, true, false, false, core::KeyHashing::On},
      {"wire_zipf", kernels::KeyDistribution::Zipf, false, false, false, core::KeyHashing::Auto, true},
      {"wire_tpch_materialize", kernels::KeyDistribution::Modulo, false, true, true, core::KeyHashing::Auto, true},
      {"semi_zipf_materialize", kernels::KeyDistribution::Zipf, false, true, false, core::KeyHashing::Auto, true,
       core::JoinKind::Semi},
      {"anti_wide_materialize", kernels::KeyDistribution::Uniform, true, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::Anti},
      {"left_zipf_materialize", kernels::KeyDistribution::Zipf, false, true, false, core::KeyHashing::Auto, true,
       core::JoinKind::LeftOuter},
      {"right_wide_materialize", kernels::KeyDistribution::Uniform, true, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::RightOuter},
      {"full_uniform_materialize", kernels::KeyDistribution::Uniform, false, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::FullOuter},
      {"group_zipf_count", kernels::KeyDistribution::Zipf, false, true, false, core::KeyHashing::Auto, true,
       core::JoinKind::Group},
      {"group_uniform_sum", kernels::KeyDistribution::Uniform, false, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::Group, false, true},
      {"group_wide_sum", kernels::KeyDistribution::Zipf, true, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::Group, false, true},
      {"group_zipf_sum_min_max", kernels::KeyDistribution::Zipf, false, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::Group, false, false, true},
      {"group_zipf_typed_f64_f32_i32", kernels::KeyDistribution::Zipf, false, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::Group, false, false, false, true},
      {"semi_bitmap_zipf_rids", kernels::KeyDistribution::Zipf, false, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::Semi, true},
      {"semi_bitmap_uniform_count", kernels::KeyDistribution::Uniform, false, false, false, core::KeyHashing::Auto,
       false, core::JoinKind::Semi, true},
      {"anti_bitmap_uniform_rids", kernels::KeyDistribution::Uniform, false, true, false, core::KeyHashing::Auto, false,
       core::JoinKind::Anti, true},
      {"anti_bitmap_zipf_count", kernels::KeyDistribution::Zipf, false, false, false, core::KeyHashing::Auto, false,
       core::JoinKind::Anti, true},
  };
  bool ok = true;
  for (const Case &c : cases) ok = runCase(c, ranks, G) && ok;
  ok = runKeyColumnCase(ranks, G) && ok;
  ok = runFaultCase(ranks, G) && ok;
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
