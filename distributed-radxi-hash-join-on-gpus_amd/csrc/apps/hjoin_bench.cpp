// Standalone driver: the analog of the reference's `program`
// (/root/reference/main.cpp:28-149) without MPI or Python.
//
//   hjoin_bench [--inner N] [--outer N] [--dist unique|modulo|uniform|zipf]
//               [--theta T] [--device D] [--host] [--iters K] [--warmup W]
//               [--rank R --world W --id-file PATH]   (one process per GPU; rank 0
//                                                      writes the ncclUniqueId to PATH)
//               [--chunks C] [--net-bits B] [--local-bits B] [--materialize] [--wide]
//               [--round-robin] [--perf-dir DIR] [--kind inner|semi|anti|left|right|full|group]
//               [--inner-domain D] [--outer-domain D] [--outer-key-offset K] [--semi-bitmap]
//               [--packed-fragments auto|on|off]
// --semi-bitmap: JoinConfig::semiBitmap (--kind semi|anti on one rank: the
// set-semantics bitmap plan; the [INFO] plan line then says bitmapSet).
// --kind semi|anti: `matches` is the number of outer tuples with / without an
// inner partner; --kind left|right|full: the number of result rows (the inner
// join's pairs plus the unmatched tuples of the preserved sides); --kind group:
// `matches` is `matched_pairs`, the sum of the per-inner-tuple counts (the
// inner join's count), printed with `groups` (result rows: the inner tuples)
// and `empty_groups` (rows with count 0).  `correct`
// is checked against a host oracle computed here when that is cheap (one
// rank, at most 64M tuples in all), else omitted.
// --inner-domain D: inner keys UNIFORM over D keys (repeated and missing
// keys); --outer-domain / --outer-key-offset: the outer keys' domain and its
// first key (outer keys without a partner).  With any of them the oracle of
// every kind is the host one.
// Default workload per rank: 20M x 20M unique keys, as in main.cpp:70-71.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../comm/RcclCommunicator.h"
#include "../comm/World.h"
#include "../core/ExecContext.h"
#include "../data/Relation.h"
#include "../operators/HashJoin.h"
#include "../performance/Measurements.h"
#include "../utils/Hip.h"

using namespace hpcjoin;

int main(int argc, char **argv) {
  uint32_t rank = 0, world = 1;
  int device = -1;
  std::string idFile = "/tmp/hjoin_bench.id", dist = "unique", perfDir;
  uint64_t inner = 0, outer = 0;
  double theta = 0.75;
  int iters = 5, warmup = 1;
  bool host = false;
  uint64_t innerDomain = 0, outerDomain = 0, outerKeyOffset = 0;
  core::JoinConfig cfg;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> std::string { return i + 1 < argc ? argv[++i] : ""; };
    if (a == "--inner") inner = std::stoull(next());
    else if (a == "--outer") outer = std::stoull(next());
    else if (a == "--dist") dist = next();
    else if (a == "--theta") theta = std::stod(next());
    else if (a == "--device") device = std::stoi(next());
    else if (a == "--host") host = true;
    else if (a == "--iters") iters = std::stoi(next());
    else if (a == "--warmup") warmup = std::stoi(next());
    else if (a == "--rank") rank = std::stoul(next());
    else if (a == "--world") world = std::stoul(next());
    else if (a == "--id-file") idFile = next();
    else if (a == "--chunks") cfg.chunks = std::stoul(next());
    else if (a == "--net-bits") cfg.networkBits = std::stoul(next());
    else if (a == "--local-bits") cfg.localBits = std::stoul(next());
    else if (a == "--materialize") cfg.materialize = true;
    else if (a == "--wide") cfg.format = core::TupleFormat::Wide;
    else if (a == "--round-robin") cfg.assignment = core::AssignmentPolicy::RoundRobin;
    else if (a == "--two-level-only") cfg.bitmapJoin = false;  // no single-level bitmap join (N == 1)
    else if (a == "--semi-bitmap") cfg.semiBitmap = true;  // --kind semi|anti at N == 1: the set bitmap plan
    else if (a == "--packed-fragments") {  // JoinConfig::packedFragments: the [INFO] plan line then says packed
      const std::string k = next();
      if (k == "auto") cfg.packedFragments = core::PlanChoice::Auto;
      else if (k == "on") cfg.packedFragments = core::PlanChoice::On;
      else if (k == "off") cfg.packedFragments = core::PlanChoice::Off;
      else {
        std::fprintf(stderr, "unknown --packed-fragments %s (auto|on|off)\n", k.c_str());
        return 2;
      }
    }
    else if (a == "--perf-dir") perfDir = next();
    else if (a == "--inner-domain") innerDomain = std::stoull(next());
    else if (a == "--outer-domain") outerDomain = std::stoull(next());
    else if (a == "--outer-key-offset") outerKeyOffset = std::stoull(next());
    else if (a == "--kind") {
      const std::string k = next();
      if (k == "inner") cfg.kind = core::JoinKind::Inner;
      else if (k == "semi") cfg.kind = core::JoinKind::Semi;
      else if (k == "anti") cfg.kind = core::JoinKind::Anti;
      else if (k == "left") cfg.kind = core::JoinKind::LeftOuter;
      else if (k == "right") cfg.kind = core::JoinKind::RightOuter;
      else if (k == "full") cfg.kind = core::JoinKind::FullOuter;
      else if (k == "group") cfg.kind = core::JoinKind::Group;
      else {
        std::fprintf(stderr, "unknown --kind %s (inner|semi|anti|left|right|full|group)\n", k.c_str());
        return 2;
      }
    }
    else {
      std::fprintf(stderr, "unknown argument %s\n", a.c_str());
      return 2;
    }
  }
  if (!inner) inner = (uint64_t)world * 20000000ull;
  if (!outer) outer = inner;
  if (device < 0) device = (int)rank;

  std::unique_ptr<comm::Communicator> comm;
  if (world == 1 || host) {
    comm.reset(new comm::LocalCommunicator());
    world = 1;
    rank = 0;
  } else {
    std::vector<uint8_t> id;
    if (rank == 0) {
      id = comm::RcclCommunicator::uniqueId();
      std::string tmp = idFile + ".tmp";
      std::ofstream(tmp, std::ios::binary).write(reinterpret_cast<const char *>(id.data()), id.size());
      std::rename(tmp.c_str(), idFile.c_str());
    } else {
      for (int t = 0; t < 600; ++t) {
        std::ifstream f(idFile, std::ios::binary);
        id.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        if (id.size() == comm::RcclCommunicator::UNIQUE_ID_BYTES) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
      }
    }
    comm.reset(new comm::RcclCommunicator(id, rank, world, device));
  }
  comm::setWorld(comm.get());
  const Location loc = host ? Location::Host : Location::Device;

  performance::Measurements::init(rank, world, "experiment", perfDir);
  performance::Measurements::writeMetaData("GISZ", inner);
  performance::Measurements::writeMetaData("GOSZ", outer);

  data::GenSpec is, os;
  is.seed = 1234;
  os.seed = 4321;
  if (dist == "unique") {
  } else if (dist == "modulo") {
    os.distribution = kernels::KeyDistribution::Modulo;
    os.domain = inner;
  } else if (dist == "uniform") {
    os.distribution = kernels::KeyDistribution::Uniform;
    os.domain = inner;
  } else if (dist == "zipf") {
    os.distribution = kernels::KeyDistribution::Zipf;
    os.domain = inner;
    os.zipfTheta = theta;
  } else {
    std::fprintf(stderr, "unknown --dist %s\n", dist.c_str());
    return 2;
  }
  if (innerDomain) {
    is.distribution = kernels::KeyDistribution::Uniform;
    is.domain = innerDomain;
  }
  if (outerDomain) {
    if (dist == "unique") {
      std::fprintf(stderr, "--outer-domain needs --dist modulo|uniform|zipf\n");
      return 2;
    }
    os.domain = outerDomain;
  }
  os.keyOffset = outerKeyOffset;
  const bool customKeys = innerDomain || outerDomain || outerKeyOffset;
  const uint64_t li = data::Relation::localSizeFor(inner, rank, world);
  const uint64_t lo = data::Relation::localSizeFor(outer, rank, world);
  performance::Measurements::writeMetaData("LISZ", li);
  performance::Measurements::writeMetaData("LOSZ", lo);
  data::Relation R(li, inner, loc, device), S(lo, outer, loc, device);
  R.generate(is, data::Relation::localOffsetFor(inner, rank, world));
  S.generate(os, data::Relation::localOffsetFor(outer, rank, world));
  uint64_t expected = data::Relation::expectedMatches(is, inner, os, outer);
  if (cfg.kind != core::JoinKind::Inner || customKeys) {
    // Host oracle from the same generator specs: the outer tuples whose key is
    // (semi) / is not (anti) among the inner keys; outer kinds: the inner
    // join's matches plus the unmatched tuples of the preserved sides.
    expected = UINT64_MAX;
    if (world == 1 && inner + outer <= (64ull << 20)) {
      data::Relation Rh(inner, inner, Location::Host, 0), Sh(outer, outer, Location::Host, 0);
      Rh.generate(is, 0);
      Sh.generate(os, 0);
      std::unordered_map<uint64_t, uint64_t> copies;  // inner key -> copies
      copies.reserve(2 * inner);
      for (uint64_t i = 0; i < inner; ++i) ++copies[Rh.getData()[i].key];
      std::unordered_set<uint64_t> probed;  // inner keys some outer tuple has
      uint64_t semi = 0, pairs = 0, unmatchedInner = 0;
      for (uint64_t i = 0; i < outer; ++i) {
        auto it = copies.find(Sh.getData()[i].key);
        if (it == copies.end()) continue;
        ++semi;
        pairs += it->second;
        probed.insert(it->first);
      }
      for (const auto &kc : copies)
        if (!probed.count(kc.first)) unmatchedInner += kc.second;
      switch (cfg.kind) {
        case core::JoinKind::Inner:
        case core::JoinKind::Group: expected = pairs; break;  // group: the counts add up to the pairs
        case core::JoinKind::Semi: expected = semi; break;
        case core::JoinKind::Anti: expected = outer - semi; break;
        default:
          expected = pairs + (core::preservesInner(cfg.kind) ? unmatchedInner : 0) +
                     (core::preservesOuter(cfg.kind) ? outer - semi : 0);
      }
    }
  }

  core::ExecContext ctx(loc, device, comm.get());
  operators::HashJoin join(&R, &S, &ctx, cfg);
  if (rank == 0) std::printf("[INFO] %s\n", join.getPlan().describe().c_str());
  for (int w = 0; w < warmup; ++w) join.run();
  ctx.resetScratch();  // grow the arena to the warmup peak before timing
  std::vector<double> times;
  uint64_t matches = 0, groupTotals[3] = {0, 0, 0};  // group: matched pairs, groups, empty groups (all ranks)
  for (int it = 0; it < iters; ++it) {
    comm->barrier();
    operators::JoinResult r = join.run();
    std::vector<uint64_t> mine{(uint64_t)(r.joinMs * 1000.0)}, all(world);
    comm->allGatherHost(mine.data(), all.data(), 1);
    times.push_back(*std::max_element(all.begin(), all.end()) / 1000.0);
    matches = r.globalMatches;
    if (cfg.kind == core::JoinKind::Group) {
      groupTotals[0] = r.matchedPairs;
      groupTotals[1] = r.localMatches;
      groupTotals[2] = r.unmatchedInner;
      comm->allReduceSumHost(groupTotals, 3);
      matches = groupTotals[0];
    }
  }
  performance::Measurements::printMeasurements(comm.get());
  performance::Measurements::storeAllMeasurements();
  std::sort(times.begin(), times.end());
  const double med = times.empty() ? 0 : times[times.size() / 2];
  if (rank == 0) {
    std::printf("{\"metric\": \"join_throughput\", \"value\": %.4f, \"unit\": \"billion tuples/s\", \"n_gpus\": %u, "
                "\"ms_per_join\": %.3f, \"matches\": %lu",
                med > 0 ? (inner + outer) / (med * 1e6) : 0.0, world, med, (unsigned long)matches);
    if (cfg.kind != core::JoinKind::Inner) std::printf(", \"kind\": \"%s\"", core::joinKindName(cfg.kind));
    if (cfg.kind == core::JoinKind::Group)
      std::printf(", \"matched_pairs\": %lu, \"groups\": %lu, \"empty_groups\": %lu", (unsigned long)groupTotals[0],
                  (unsigned long)groupTotals[1], (unsigned long)groupTotals[2]);
    if (cfg.kind == core::JoinKind::Inner || expected != UINT64_MAX)  // semi / anti without an oracle: omitted
      std::printf(", \"expected\": %s%lu, \"correct\": %s", expected == UINT64_MAX ? "-" : "",
                  (unsigned long)(expected == UINT64_MAX ? 0 : expected),
                  (expected == UINT64_MAX || expected == matches) ? "true" : "false");
    std::printf("}\n");
  }
  return (expected == UINT64_MAX || expected == matches) ? 0 : 1;
}
