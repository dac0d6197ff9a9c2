// The routing header (zk-paillier_amd/csrc/route_plan.hpp) as a program of its own: the full decision for every RangeProofNi prove and verify
// call of 1 ... 400 proofs under one 2048-bit key, error factor 128, as csrc/zkp_api.hip and csrc/zkp_api_proofs.inc ask for it — which engine,
// cut or not, and on the engine that runs each part the base-n plan, the pair ladder and the second stream.  tests/test_cpp_route_plan.py
// builds it under the sanitizers and compares what it prints with tests/routing_model.py and with the pinned table tests/golden/route_plan.json.
//
//   test_route_plan            error factor 128, every config, 1 ... 400 proofs (the table of tests/golden/route_plan.json)
//   test_route_plan <EF>       another error factor (1 ... 256), the three chips only, every batch from 1 to the first one whose items
//                              (2 EF per proof) exceed 48 per SIMD — beyond that no rule looks at the size any more.  "prove" is then the
//                              Enc launch of zkp_range_generate_encrypted_pairs_batch: zkp_range_ni_prove_batch always writes 128 rows, and
//                              only a call of 128 rows per proof asks range_split (csrc/zkp_api_proofs.inc)
//
//   config <name>                                  the knobs of the ctx (throughput build, 36 limbs per lane)
//   prove|verify <B> <decision>                    one line per call
//   takes <w> <B> <asked> <placed>                 B < cus: "takes the hashes" as range_verify_impl asks it | hash blocks of the launch's own plan
//   pass 2                                         everything once more, computed in the opposite order
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../zk-paillier_amd/csrc/route_plan.hpp"

using namespace zkp;

static const int N_BITS = 2048, DEFAULT_EF = 128;
static int EF = DEFAULT_EF, MAX_B = 400;      // MAX_B == 0: up to the first batch beyond 48 items per SIMD (max_batch)
static bool CHIPS_ONLY = false;
static const int OCCUPANCY = 2;      // resident workgroups per compute unit of the base-n kernels: an input of the plan (the library asks the runtime)

struct Config { std::string name; RouteKnobs k; };

static RouteKnobs base_knobs(int cus) {
  RouteKnobs k;
  k.w = 36; k.eng_w[0] = 9; k.eng_w[1] = 18; k.cus = cus;
  return k;
}
// the twin ctx of a secondary engine: the same switches (zkp_diag_set_* pass them on, the presets come from the same environment), no engines of its own
static RouteKnobs engine_knobs(RouteKnobs k, int w) {
  k.w = w; k.eng_w[0] = k.eng_w[1] = 0; k.geometry = 0;
  return k;
}
// the second latency-engine ctx of a cut call (range_split_ctx)
static RouteKnobs tail_knobs(RouteKnobs k) {
  k = engine_knobs(k, 9);
  if (!k.r2l_lanes) k.r2l_lanes = 12;
  k.fuse_hash_on = 0;
  return k;
}

static std::vector<Config> configs() {
  std::vector<Config> v;
  for (int cus : {256, 64, 304}) v.push_back({"cus" + std::to_string(cus), base_knobs(cus)});
  auto variant = [&](const char* name, auto set) { RouteKnobs k = base_knobs(256); set(k); v.push_back({name, k}); };
  if (CHIPS_ONLY) return v;
  variant("grid_expected0", [](RouteKnobs& k) { k.grid_expected = 0; });
  variant("split0", [](RouteKnobs& k) { k.split_calls = 0; });
  variant("fuse_hash0", [](RouteKnobs& k) { k.fuse_hash_on = 0; });
  variant("r2l0", [](RouteKnobs& k) { k.r2l = 0; });
  variant("r2l2", [](RouteKnobs& k) { k.r2l = 2; });
  variant("r2l_lanes8", [](RouteKnobs& k) { k.r2l_lanes = 8; });
  variant("r2l_lanes12", [](RouteKnobs& k) { k.r2l_lanes = 12; });
  variant("r2l_lanes36", [](RouteKnobs& k) { k.r2l_lanes = 36; });
  variant("form_n2", [](RouteKnobs& k) { k.enc_form = ZKP_ENC_FORM_N2; });
  variant("form_shared", [](RouteKnobs& k) { k.enc_form = ZKP_ENC_FORM_SHARED; });
  variant("form_always", [](RouteKnobs& k) { k.enc_form = ZKP_ENC_FORM_ALWAYS; });
  variant("no_lat", [](RouteKnobs& k) { k.eng_w[0] = 0; });
  variant("no_mid", [](RouteKnobs& k) { k.eng_w[1] = 0; });
  variant("no_engines", [](RouteKnobs& k) { k.eng_w[0] = k.eng_w[1] = 0; });
  return v;
}

// the shape launch_basen builds from the EncArgs of a RangeProofNi prove (mode 0) or verify (mode 1) launch of `batch` proofs on build k.w
static BasenShape launch_shape(const RouteKnobs& k, bool verify, uint64_t batch, bool hashes_offered) {
  const int lanes_n2 = 144 / k.w;      // group_for_bits(2 * 2048)
  BasenShape s;
  s.lanes = lanes_n2 / 2; s.n_bits = N_BITS; s.mode = verify ? 1 : 0; s.count = 2 * batch * EF; s.listed = verify;
  s.has_sched = !pair_ladder(k, lanes_n2, s.count);
  s.hashes_offered = hashes_offered; s.hashes = hashes_offered ? batch : 0;
  s.groups_per_block = 256 / s.lanes; s.per_cu = OCCUPANCY;
  return s;
}
static bool takes_hashes(const RouteKnobs& k, uint64_t batch) {      // as basen_r2l_takes_hashes asks
  return basen_plan(k, verify_shape(k, 144 / k.w / 2, 0, N_BITS, 2 * batch * EF, true, batch)).hash_blocks != 0;
}

// one part of a call, on the engine whose knobs are k
static std::string part(const RouteKnobs& k, bool verify, uint64_t batch) {
  const int lanes_n2 = 144 / k.w;
  const uint64_t count = 2 * batch * EF;
  bool two = false, fuse = false;
  if (verify) {
    const uint64_t gpb = 256 / lanes_n2;
    two = two_streams(k, (count + gpb - 1) / gpb, -1);
    fuse = two && k.fuse_hash_on && batch < (uint64_t)k.cus && takes_hashes(k, batch);
  }
  const BasenPlan p = basen_plan(k, launch_shape(k, verify, batch, fuse));
  char buf[256];
  std::snprintf(buf, sizeof buf, "w=%d pair=%d form=%d r2l=%d lanes=%d blocks=%u wgs=%llu hash=%d two=%d side=%d", k.w, (int)pair_ladder(k, lanes_n2, count), (int)p.take,
                (int)p.r2l, p.r2l_lanes, p.blocks, (unsigned long long)p.enc_wgs, p.hash_blocks, (int)two, (int)(two && !fuse));
  return buf;
}
static const char* engine_name(int e) { return e < 0 ? "own" : e == 0 ? "lat" : "mid"; }

static int max_batch(const RouteKnobs& k) {
  if (MAX_B) return MAX_B;
  return (int)(48 * simds(k) / (2 * (uint64_t)EF)) + 1;
}

static std::string decide(const RouteKnobs& k, bool verify, uint64_t batch) {
  const uint64_t rows = 2 * (uint64_t)EF;
  // (a prove of another row count is the interactive generate_encrypted_pairs: routed by its items, never cut)
  const RangeSplit sp = (verify || EF == DEFAULT_EF) ? range_split(k, batch, rows, N_BITS, 0, verify) : RangeSplit();
  auto on = [&](int e) { return e < 0 ? k : engine_knobs(k, k.eng_w[e]); };
  if (sp.head)
    return "cut head=" + std::to_string(sp.head) + "@" + engine_name(sp.head_engine) + " [" + part(on(sp.head_engine), verify, sp.head) + "] tail=" +
           std::to_string(batch - sp.head) + " [" + part(tail_knobs(k), verify, batch - sp.head) + "]";
  const int e = route_engine(k, batch * rows, 2 * N_BITS, true, verify);
  return std::string("whole @") + engine_name(e) + " [" + part(on(e), verify, batch) + "]";
}

// every line of the output, computed config by config and line by line in the order asked for, stored in its place
static std::vector<std::string> run(bool backwards) {
  struct Job { int kind, w, B; };      // kind 0 / 1: a prove / verify call; 2: "takes" on build w
  const std::vector<Config> cfg = configs();
  std::vector<std::vector<std::string>> blocks(cfg.size());
  for (size_t ci = 0; ci < cfg.size(); ci++) {
    const Config& c = cfg[backwards ? cfg.size() - 1 - ci : ci];
    std::vector<Job> jobs;
    const int last = max_batch(c.k);
    for (int kind = 0; kind < 2; kind++) for (int B = 1; B <= last; B++) jobs.push_back({kind, 36, B});
    for (int w : {36, 18, 9}) for (int B = 1; B < c.k.cus && B <= last; B++) jobs.push_back({2, w, B});
    std::vector<std::string>& lines = blocks[backwards ? cfg.size() - 1 - ci : ci];
    lines.assign(jobs.size() + 1, "");
    lines[0] = "config " + c.name;
    for (size_t ji = 0; ji < jobs.size(); ji++) {
      const size_t at = backwards ? jobs.size() - 1 - ji : ji;
      const Job& j = jobs[at];
      if (j.kind < 2) lines[at + 1] = std::string(j.kind ? "verify " : "prove ") + std::to_string(j.B) + " " + decide(c.k, j.kind != 0, (uint64_t)j.B);
      else {
        const RouteKnobs k = j.w == 36 ? c.k : engine_knobs(c.k, j.w);
        lines[at + 1] = "takes " + std::to_string(j.w) + " " + std::to_string(j.B) + " " + std::to_string((int)takes_hashes(k, (uint64_t)j.B)) + " " +
                        std::to_string(basen_plan(k, launch_shape(k, true, (uint64_t)j.B, true)).hash_blocks);
      }
    }
  }
  std::vector<std::string> out;
  for (const auto& b : blocks) out.insert(out.end(), b.begin(), b.end());
  return out;
}

int main(int argc, char** argv) {
  if (argc > 1) {
    EF = std::atoi(argv[1]);
    if (EF < 1 || EF > 256) { std::fprintf(stderr, "usage: test_route_plan [error factor 1 ... 256]\n"); return 2; }
    MAX_B = 0;
    CHIPS_ONLY = true;
  }
  for (const std::string& l : run(false)) std::puts(l.c_str());
  std::puts("pass 2");
  for (const std::string& l : run(true)) std::puts(l.c_str());
  return 0;
}
