// route_plan.hpp — every decision of the host layer that is a function of sizes and switches: which engine takes a call, whether a
// RangeProofNi call is cut in two, which Paillier launches take the base-n form and on which ladder, grid sizes, where the transcript
// hashes of a verify ride, the second stream.  Pure functions over small structs: no HIP header, no ctx, no state — zkp_api.hip and
// zkp_api_proofs.inc ask them and do the allocating and launching; tests/cpp/test_route_plan.cpp prints them for every batch size on a CPU.
// A proof-count window is changed HERE, in one place: the predicates below are what the rules share.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/zkp_hip_diag.h"

#ifndef ZKP_R2L5_ITEMS_PER_CU
#define ZKP_R2L5_ITEMS_PER_CU 1ull      /* launches of up to this many Enc per compute unit take five wavefronts per Enc (k_enc_basen_r2l5): one proof 13.3 / 9.3 -> 10.2 / 6.0 ms;
                                           two proofs (two workgroups per CU) 13.8 / 9.6 against 13.9 / 9.7 on one wavefront per Enc, but the verify time is bimodal there (9.6 or 12.4 ms:
                                           a transcript-hash wavefront that shares its SIMD with three others); three: 17.7 / 13.4 against 13.9 / 9.9 (profiles/r05/r2l5/) */
#endif

namespace zkp {

// The switches of a ctx ($ZKP_* presets at zkp_ctx_create, zkp_diag_set_* / zkp_ctx_set_geometry afterwards) and the engines it can hand
// calls to.  `w` is a run-time field so that one host program can ask what each of the three builds would do.
struct RouteKnobs {
  int w = 0;                           // limbs per lane of the build that decides (36: throughput engine, 18: mid, 9: latency)
  int eng_w[2] = {0, 0};               // limbs per lane of the secondary engines of this ctx ([0] latency, [1] mid; 0: absent — always inside a secondary engine)
  int cus = 0;
  int geometry = 0;                    // 0 = automatic, else the limbs per lane every call must run on
  int enc_form = ZKP_ENC_FORM_AUTO;    // which Paillier launches take the base-n form (zkp_diag_set_enc_form; $ZKP_BASEN is read ONCE, at zkp_ctx_create)
  int r2l = 1;                         // the one-Enc-per-wavefront ladder of the latency engine (kernels_basen_r2l.hpp): 0 = never, 1 = the library's rule (launches of up to
                                       // two wavefronts per SIMD), 2 = whenever it can run (tests); $ZKP_R2L at ctx create
  int r2l_lanes = 0;                   // ... its lane geometry: 0 = the library's rule (five wavefronts of 36 lanes x 2 limbs per Enc while every Enc finds a CU's worth of
                                       // SIMDs, else one wavefront of five groups of 12 lanes x 6 limbs); 36 / 12 / 8 (x 9 limbs) pin one ($ZKP_R2L_LANES at ctx create, zkp_diag_set_r2l_lanes)
  int grid_expected = 1;               // the base-n launch of a verify sized by the items expected, not by the bound (basen_plan); $ZKP_GRID_EXPECTED=0 at zkp_ctx_create: A/B runs
  int split_calls = 1;                 // range_split; $ZKP_SPLIT=0 at zkp_ctx_create / zkp_diag_set_split turn it off
  int fuse_hash_on = 1;                // the transcript hashes of a verify of a few proofs as workgroups of its Enc launch; $ZKP_FUSE_HASH=0 at zkp_ctx_create keeps them in a launch of their own
};

// the items a verify's work list is expected to hold when the launch is sized for `bound` (2 per row: an Open row has two Enc checks, a Mask
// row one, the challenge bits are fair): three quarters, + 3 % (5 proofs: 960 + 40 of 1280; the spread of 5 proofs is 13).
// A PERFORMANCE assumption only: the prover chooses the response kinds, and the kind-derived list of the two-stream shape holds up to the
// whole bound — crafted all-Open proofs, about 1.33x the items planned here.  Every launch sized by it claims until the list is empty, so
// such a verify is slower, its verdicts the same (tests/test_gpu_verify_crafted.py).
inline uint64_t expected_items(uint64_t bound) { return (3 * bound + 3) / 4 + bound / 32; }
inline uint64_t simds(const RouteKnobs& k) { return 4 * (uint64_t)k.cus; }
// what a launch over at most `items` is judged by: the items expected when they are the bound of a verify's work list
inline uint64_t judged_items(const RouteKnobs& k, uint64_t items, bool listed) { return (listed && k.grid_expected) ? expected_items(items) : items; }
// which of the secondary engines has this many limbs per lane (-1: none)
inline int engine_with(const RouteKnobs& k, int limbs_per_lane) {
  for (int e = 0; e < 2; e++) if (limbs_per_lane && k.eng_w[e] == limbs_per_lane) return e;
  return -1;
}

// ---- the windows that more than one rule compares (Enc under ONE 2048-bit key; `items` = Enc of the call, 256 per proof at 128 rows) ----
// one wavefront per SIMD of the mid engine, 16 Enc each (k_enc_basen<4>): 64 proofs — a verify by the items EXPECTED, its grid is sized by
// them too, so that 65 ... 81 proofs verify in one round there (37.4 ms) instead of as two concurrent calls (46.3; tools/dev/two_streams_sweep.py
// with the engine pinned, profiles/r06/expected_items/)
inline bool mid_one_round(const RouteKnobs& k, uint64_t items, bool listed) { return items <= 16 * simds(k) || (listed && k.grid_expected && expected_items(items) <= 16 * simds(k)); }
// one wavefront per SIMD of the latency engine's k_enc_basen<8>, 8 Enc each: 32 proofs; a verify by the items expected
inline bool lat_basen_one_round(const RouteKnobs& k, uint64_t items, bool listed) { return items <= 8 * simds(k) || (listed && k.grid_expected && expected_items(items) <= 8 * simds(k)); }
// the latency engine stays ahead of the throughput engine up to three wavefronts per SIMD at 8 Enc each: 96 proofs
inline bool lat_three_rounds(const RouteKnobs& k, uint64_t items) { return items <= 3 * simds(k) * 8; }
// one wavefront per SIMD of the throughput engine's k_enc_basen<2>, 32 Enc each: 128 proofs
inline bool own_basen_one_round(const RouteKnobs& k, uint64_t items) { return items <= 32 * simds(k); }
// every wavefront of the n^2-sized kernel (64 / lanes_n2 items each) finds a SIMD of its own: 16 proofs on the latency engine's window ladder
inline bool n2_one_round(const RouteKnobs& k, uint64_t items, int lanes_n2) { return items <= simds(k) * (uint64_t)(64 / lanes_n2); }
// up to two wavefronts per SIMD at ONE Enc per wavefront: 8 proofs — what the library's rule gives the r2l ladder
inline bool r2l_two_per_simd(const RouteKnobs& k, uint64_t items) { return items <= 2 * simds(k); }

// ---- which engine ------------------------------------------------------------------------------------------------------------------------
// Does this call (items independent modexp chains under mod_bits-bit moduli) go to a secondary engine?  -1: no, else the engine's index.
// one_key_paillier: the items are Paillier Enc under ONE 2048-bit key — the latency engine then runs them in base-n form, 8 Enc per wavefront
// (k_enc_basen<8>), and stays ahead of the throughput engine up to three wavefronts per SIMD.  Measured round 5 (tools/dev/size_sweep.py,
// profiles/r05/size_sweep.jsonl, prove / verify ms): 48 proofs 43.9 / 43.5 against 49.3 / 44.2 on the n^2-sized throughput kernels, 64 proofs
// 45.1 / 44.3 against 51.0 / 44.3, 96 proofs 60.7 / 59.7 against 64.9 / 61.6 on the throughput engine's base-n kernels, 128 proofs 76.7 / 74.5
// against 66.7 / 61.7: the hand-over is at 96 proofs.
// With the mid engine loaded (18 limbs per lane: 16 Enc per wavefront in base-n form, k_enc_basen<4>) the one-key Paillier calls are cut
// three ways (same sweep, profiles/r05/size_sweep_w18.jsonl): up to 40 proofs the latency engine (32 proofs 33.1 / 29.5 ms against 40.0 / 38.3),
// from there to 64 proofs — one wavefront per SIMD at 16 Enc each — the mid engine (64 proofs 41.4 / 38.5 against 45.9 / 44.4), the latency
// engine again up to 96 (80 proofs 61.1 / 59.7 against 65.2 / 63.9), the throughput engine beyond — except 129 ... 192 proofs, where two mid
// wavefronts per SIMD beat its second round of 32-Enc claims (160 proofs 90.7 / 67.7 against 111.7 / 66.1, 192: 93.2 / 89.8 against 113.6 / 111.2).
// `listed`: the items are the bound of a verify's work list (2 per row; about three quarters exist): see mid_one_round.
inline int route_engine(const RouteKnobs& k, uint64_t items, uint32_t mod_bits, bool one_key_paillier, bool listed) {
  if (!k.eng_w[0] && !k.eng_w[1]) return -1;
  if (k.geometry == k.w || items == 0) return -1;
  if (k.geometry) return engine_with(k, k.geometry);              // pinned to a secondary engine
  if (one_key_paillier && mod_bits == 4096 && k.enc_form != ZKP_ENC_FORM_N2) {
    const int lat9 = engine_with(k, 9), mid18 = engine_with(k, 18);
    if (mid18 >= 0 && ((items > 10 * simds(k) && mid_one_round(k, items, listed)) || (!own_basen_one_round(k, items) && items <= 48 * simds(k)))) return mid18;
    if (lat9 >= 0 && lat_three_rounds(k, items)) return lat9;
    if (lat9 >= 0) return -1;
  }
  if (!k.eng_w[0]) return -1;
  // automatic: the latency engine wins while its launch stays within a few wavefronts per SIMD — measured on MI355X
  // (tools/dev/sweep.py, both engines pinned): RangeProofNi n = 2048 (16 lanes per integer) 48 proofs = 3 waves per SIMD:
  // 56 ms against 62 ms, 64 proofs: 70 against 63; NiCorrectKeyProof (2048-bit moduli, 8 lanes) 4096 keys = 5.5 per SIMD:
  // 62 against 70 ms, 8192 keys: 101 against 96; CompositeDLogProof 16384 proofs = 4 per SIMD: 11 against 18 ms
  const uint64_t limbs = mod_bits <= 2048 ? 72 : mod_bits <= 4096 ? 144 : 288;
  const uint64_t lanes = limbs / (uint64_t)k.eng_w[0];
  // (round 3, both engines with squarings where their product allows: RangeProofNi n = 2048 32 proofs 40.7 / 37.5 ms against 49.2 / 44.4,
  // 48 proofs 55.3 / 54.9 against 49.5 / 44.2 -> 2.5 waves per SIMD; NiCorrectKeyProof 4096 keys 56.9 against 59.0 ms, 8192 keys 90 against 81)
  const uint64_t half_waves_per_simd = mod_bits <= 2048 ? 12 : 5;
  return 2 * items <= (half_waves_per_simd * simds(k) * 64) / lanes ? 0 : -1;
}

// ---- a RangeProofNi call under one 2048-bit key as TWO concurrent calls --------------------------------------------------------------
// The mid engine serves 64 proofs with ONE wavefront per SIMD (16 Enc each: 41 / 39 ms); the 65th proof gives a SIMD its second wavefront
// and the call 60 ms on whichever engine runs it.  The chip is not full at that point — a lone wavefront leaves a third of its SIMD's
// issue slots unused — so the call is cut at proof 64: the head runs on the mid engine on the ctx's stream, the tail (1 ... 32 proofs) on a
// SECOND ctx of the latency engine with a stream of its own, issued from a helper thread (a host-pointer call blocks its thread).  Measured
// (tools/dev/split_probe.py, one board each): 72 proofs 58.2 / 57.1 -> 53.2 / 41.4 ms prove / verify, 80 proofs 58.6 / 58.0 -> 49.1 / 43.7,
// 96 proofs 59.5 / 58.6 -> 53.4 / 52.9; beyond 96 proofs two wavefronts per SIMD of one engine are the better deal.  Proofs are
// independent: the bytes are those of one call (tests/test_gpu_routing.py).
struct RangeSplit { uint64_t head = 0; int head_engine = 1; };      // head == 0: the call is not cut; head_engine -1 = the throughput engine itself
inline RangeSplit range_split(const RouteKnobs& k, uint64_t batch, uint64_t rows_per_proof, uint32_t n_bits, uint64_t n_stride, bool listed) {
  const RangeSplit none;
  if (!k.split_calls || k.geometry || k.enc_form != ZKP_ENC_FORM_AUTO || n_stride || n_bits != 2048 || rows_per_proof == 0) return none;
  if (engine_with(k, 9) != 0 || engine_with(k, 18) != 1) return none;
  const uint64_t items = batch * rows_per_proof;
  RangeSplit r;
  // (a verify whose EXPECTED items fit one wavefront per SIMD of the mid engine is not cut: route_engine sends the whole call there)
  if (items > 16 * simds(k) && mid_one_round(k, items, listed)) return none;
  if (!mid_one_round(k, items, false) && lat_three_rounds(k, items)) {
    // head: one wavefront per SIMD of the mid engine at most (16 Enc each); tail: at least one wavefront per SIMD of the latency engine's
    // window ladder (4 Enc each: 16 proofs) — a tail of a few proofs would run on the one-Enc-per-wavefront ladder, whose 60-lane wavefronts
    // are the worse neighbours (72 proofs as 64 + 8: 53.0 / 41.4 ms, 80 as 64 + 16: 48.9 / 43.3)
    const uint64_t full = 16 * simds(k) / rows_per_proof, least_tail = 4 * simds(k) / rows_per_proof;
    r.head = batch - full >= least_tail ? full : (batch > least_tail ? batch - least_tail : 0);
    r.head_engine = 1;
  } else if (!lat_basen_one_round(k, items, listed) && items <= 9 * simds(k)) {
    // 33 ... 36 proofs: the latency engine's k_enc_basen<8> holds 32 proofs at one wavefront of 8 Enc per SIMD (27.8 ms); the 33rd gave a
    // quarter of the units a second workgroup and the call 39.8 ms.  The rest — 1 ... 4 proofs: one wavefront per SIMD — runs beside the 32 on
    // the one-Enc-per-wavefront ladder of a second ctx instead: prove 32.6 ... 33.6 ms (a tail of 5 ... 8 proofs: 39.1 — no better than one call;
    // a verify of that size fits the one round by its expected items and is not cut).  tools/dev/size_sweep.py, profiles/r06/expected_items/
    r.head = 8 * simds(k) / rows_per_proof;
    r.head_engine = 0;
  } else if (!listed && !own_basen_one_round(k, items) && items <= 40 * simds(k)) {
    // 129 ... 160 proofs, PROVE: the throughput engine holds 128 proofs at one wavefront of 32 Enc per SIMD (60 ms); the 129th gave some SIMDs a
    // second one and the call 87 ms on whichever engine ran it.  The head — 128 proofs — stays on this ctx, the rest (up to 32 proofs: one
    // round of the latency engine's k_enc_basen<8>) runs beside it.
    // Measured (tools/dev/size_sweep.py, profiles/r06/expected_items/): 129 proofs 86.6 -> 64.8 ms, 132: 70.0, 144: 70.4, 160: 77.3 (one call: 87.4 ... 87.8).
    // A tail of 7 or 8 proofs — 1792 ... 2048 single-wavefront workgroups of the r2l ladder, 12 KB of LDS each — does not fit beside the head's
    // 78 KB per unit and waits for it (115 ms): such a call is cut one proof beyond that, where the tail is the window ladder's.
    r.head = 32 * simds(k) / rows_per_proof;
    const uint64_t tail_items = (batch - r.head) * rows_per_proof;
    if (tail_items > 3 * simds(k) / 2 && r2l_two_per_simd(k, tail_items)) r.head = batch - (2 * simds(k) / rows_per_proof + 1);
    r.head_engine = -1;
  } else if (!n2_one_round(k, items, 144 / 9) && items <= 5 * simds(k)) {
    // 17 ... 20 proofs: the window ladder's full round (16 proofs) on the latency engine, the rest beside it on the one-Enc-per-wavefront ladder
    r.head = 4 * simds(k) / rows_per_proof;
    r.head_engine = 0;
  }
  return (r.head > 0 && r.head < batch) ? r : none;
}

// ---- the pair ladder ---------------------------------------------------------------------------------------------------------------------
// may `items` exponentiations take the pair ladder (two groups of `lanes` lanes each)?  Latency engine only (the pair kernels are
// instantiated there), and only while the launch with twice the lanes still leaves every SIMD at most one wavefront (tools/dev/pair_sweep.py
// on MI355X, RangeProofNi n = 2048: 8 proofs 24.0 / 22.2 ms either way; 12 proofs 27.2 / 22.8 ms on the window ladder, 34.6 / 29.2 ms on
// pairs that share SIMDs two by two).
inline bool pair_ladder(const RouteKnobs& k, int lanes, uint64_t items) {
  if (k.enc_form == ZKP_ENC_FORM_ALWAYS) return false;      // (tests that pin the base-n kernels of the latency engine on small batches: they need the window script)
  return k.w <= 9 && 2 * lanes <= 64 && items * 2 * (uint64_t)lanes <= simds(k) * 64;
}

// ---- the base-n launch of an Enc call ----------------------------------------------------------------------------------------------------
struct BasenShape {
  int lanes = 0;                 // per n-sized integer: 72 / 144 limbs over w limbs per lane
  bool per_key = false;          // one key per proof (n_stride != 0), else one for the call
  bool key_stride_fits = true;   // ... and the keys lie n_bits / 32 words apart
  int n_bits = 0;
  int mode = 0;                  // EncArgs::mode: 0 = Enc, 1 = a verify's work list, 2 = Enc and compare
  uint64_t count = 0;            // items; an upper bound when
  bool listed = false;           // ... it is the bound of a verify's work list (EncArgs::count_ptr)
  bool has_sched = false;        // a sliding-window script of n exists (a shared key whose launch does not take the pair ladder)
  bool operands_fit = true;      // mode 0: m and r are no wider than n
  bool hashes_offered = false;   // the call's transcript hashes may ride in this launch (range_verify_impl) ...
  uint64_t hashes = 0;           // ... this many, one workgroup each
  int groups_per_block = 0;      // BnLds<lanes>::GROUPS_PER_BLOCK
  int per_cu = 1;                // resident workgroups per compute unit of k_enc_basen<lanes> / k_enc_basen_keys<lanes> (the occupancy query)
};
constexpr int HASH_WAVE_BLOCKS = 64;   // kernels_proofs.hpp HW_BLOCKS: the wave hash at its full LDS footprint
struct BasenPlan {
  bool take = false;             // the launch takes the base-n form (false: nothing is launched, the n^2-sized kernel does the work)
  bool r2l = false;              // ... on the one-Enc-per-wavefront ladder of the latency engine,
  int r2l_lanes = 0;             // ... its lane geometry: 36 (k_enc_basen_r2l5) / 12 / 8
  unsigned blocks = 0;           // workgroups of k_enc_basen / k_enc_basen_keys
  uint64_t enc_wgs = 0;          // r2l: the Enc workgroups, behind
  int hash_blocks = 0;           // ... one workgroup per transcript hash: 0 = the hashes are not aboard, else blocks per batch of the wave hash (HASH_WAVE_BLOCKS or 16)
};
// Does a launch of the one-wavefront-per-Enc ladder over at most `count` items (`listed`: a verify's work list, of which about three quarters
// exist) fit one wavefront per SIMD together with `hashes` transcript-hash wavefronts?
inline bool r2l_one_per_simd(const RouteKnobs& k, uint64_t count, bool listed, uint64_t hashes) {
  return hashes < simds(k) && judged_items(k, count, listed) + hashes <= simds(k);
}
// Which Paillier launches take the base-n form is a property of the ctx (include/zkp_hip_diag.h: zkp_diag_set_enc_form):
//   AUTO   the library's own rule — every launch that fills the chip, under one key or under per-proof keys
//   N2     none: every launch stays on the n^2-sized kernels (A/B runs, the parity tests that pin the two forms against each other)
//   SHARED as AUTO, but launches under per-proof keys stay on the n^2-sized kernels
//   ALWAYS also the launches too small to gain from it (the parity tests of the small shapes)
inline BasenPlan basen_plan(const RouteKnobs& k, const BasenShape& s) {
  BasenPlan p;
  const uint64_t cus = (uint64_t)k.cus;
  const int lanes_n2 = 2 * s.lanes;
  if (k.enc_form == ZKP_ENC_FORM_N2 || (s.per_key && k.enc_form == ZKP_ENC_FORM_SHARED) || s.n_bits != (s.lanes == 72 / k.w ? 2048 : 4096)) return p;
  // The latency engine's smallest calls — up to two wavefronts per SIMD at ONE Enc per wavefront: 8 proofs at n = 2048 — take the five-group
  // right-to-left ladder (kernels_basen_r2l.hpp): half the chain of the pair ladder that served them (the launch behind this one, which then
  // finds nothing to claim).
  // (a verify's work list: judged by the items expected — 9 and 10 proofs, 2304 / 2560 by the bound, still fit two wavefronts per SIMD: 14.5 ms
  //  there against 19.2 on the window ladder)
  const bool sized_by_expected = s.listed && s.mode == 1 && k.grid_expected;
  const uint64_t r2l_items = sized_by_expected ? std::min<uint64_t>(s.count, expected_items(s.count)) : s.count;
  p.r2l = k.w == 9 && s.lanes == 8 && !s.per_key && k.r2l && s.n_bits == 2048 && (k.r2l == 2 || (k.enc_form != ZKP_ENC_FORM_ALWAYS && r2l_two_per_simd(k, r2l_items)));
  if (!s.per_key && !s.has_sched && !p.r2l) return p;          // (a shared key whose launch takes the pair ladder of the latency engine)
  if (s.per_key && !s.key_stride_fits) return p;
  if (s.mode == 0 && !s.operands_fit) return p;
  // A launch whose n^2-sized wavefronts (64 / lanes_n2 items each) all find a SIMD of their own is a single chain per wavefront either way,
  // and the base-n chain is the longer one (27.4 M against 22.3 M VALU instructions per claim, for twice the items): measured at
  // n = 2048, 64 proofs: prove 51 -> 64 ms, verify 45 -> 61 ms; from 96 proofs on: 88 -> 65 ms (profiles/r04/basen/midsize_sweep.jsonl)
  if (k.enc_form != ZKP_ENC_FORM_ALWAYS && !p.r2l && n2_one_round(k, s.count, lanes_n2)) return p;
  p.take = true;
  const uint64_t gpb = (uint64_t)s.groups_per_block;
  uint64_t grid = std::min<uint64_t>((s.count + gpb - 1) / gpb, (uint64_t)s.per_cu * cus);
  // A verify's work list holds 128 + the Open rows of every proof — about three quarters — of the 2 Enc per row the launch is
  // sized for.  A workgroup claims until nothing is left, so the grid only has to hold the items EXPECTED: when those need fewer workgroups
  // per compute unit than the bound, the launch stops there (40 proofs on the latency engine: 320 workgroups of 32 Enc for 7680 items gave
  // a quarter of the units a second workgroup, and three calls of six took 27 ... 37 ms instead of 26; 65 ... 81 proofs on the mid engine:
  // one round, 37.3 ms — profiles/r06/expected_items/).  expected_items: 3 % above the mean.
  if (sized_by_expected) {
    const uint64_t need_e = (expected_items(s.count) + gpb - 1) / gpb;
    grid = std::min<uint64_t>(grid, (need_e + cus - 1) / cus * cus);
  }
  p.blocks = (unsigned)std::max<uint64_t>(1, grid);
  if (!p.r2l) return p;
  const uint64_t hashes = s.hashes_offered ? s.hashes : 0;
  // five wavefronts per Enc (36 lanes x 2 limbs each, k_enc_basen_r2l5) while the launch leaves a CU to every Enc: one proof;
  // one wavefront of five groups of 12 lanes x 6 limbs beyond; 8 lanes x 9 limbs only when pinned (A/B runs)
  p.r2l_lanes = k.r2l_lanes ? k.r2l_lanes : (s.count <= ZKP_R2L5_ITEMS_PER_CU * cus ? 36 : 12);
  if (p.r2l_lanes == 36) {
    // (with the call's transcript hashes aboard: one workgroup each in front of the Enc workgroups, the launch as a whole within one workgroup per
    //  compute unit — an Enc workgroup claims items until none is left, so fewer of them than items is only a longer loop for some)
    p.enc_wgs = std::max<uint64_t>(1, std::min<uint64_t>(s.count, simds(k)));
    if (s.hashes_offered && hashes < cus) {
      p.hash_blocks = HASH_WAVE_BLOCKS;
      p.enc_wgs = std::max<uint64_t>(1, std::min<uint64_t>(p.enc_wgs, cus - hashes));
    }
    return p;
  }
  // one wavefront per Enc: the call's transcript hashes aboard — at 64 blocks per batch while the launch as a whole stays within one
  // wavefront per SIMD (2 - 5 proofs), at 16 (6.6 KB of LDS on every workgroup) beyond (6 - 8 proofs: two wavefronts per SIMD)
  // (a verify's work list holds 128 + the Open rows of every proof — about 192 — of the 256 Enc per proof the launch is sized for: while the
  //  items EXPECTED fit one wavefront per SIMD the grid stops there — five proofs: 960 of 1280 — and a wavefront claims until none is left)
  p.enc_wgs = std::max<uint64_t>(1, std::min<uint64_t>(s.count, r2l_items < s.count ? std::max<uint64_t>(r2l_items, 2 * simds(k)) : 8 * simds(k)));
  if (r2l_one_per_simd(k, s.count, s.listed, hashes)) {
    p.enc_wgs = std::max<uint64_t>(1, std::min<uint64_t>(p.enc_wgs, simds(k) - hashes));
    if (s.hashes_offered) p.hash_blocks = HASH_WAVE_BLOCKS;
  } else if (s.hashes_offered && hashes < simds(k) && r2l_two_per_simd(k, r2l_items)) {
    // two wavefronts per SIMD: the hashes among them (the first workgroups) instead of beside them — with the small LDS footprint
    p.hash_blocks = 16;
    p.enc_wgs = std::max<uint64_t>(1, std::min<uint64_t>(p.enc_wgs, 2 * simds(k) - hashes));
  }
  return p;
}
// the shape of the Enc launch of a RangeProofNi verify (range_verify_impl: mode 1, the bound of its work list) with `hashes` transcript hashes offered
inline BasenShape verify_shape(const RouteKnobs& k, int lanes, uint64_t n_stride, uint32_t n_bits, uint64_t count, bool hashes_offered, uint64_t hashes) {
  BasenShape s;
  s.lanes = lanes; s.per_key = n_stride != 0; s.key_stride_fits = n_stride == n_bits / 32; s.n_bits = (int)n_bits; s.mode = 1; s.count = count; s.listed = true;
  s.has_sched = n_stride == 0 && !pair_ladder(k, 2 * lanes, count);
  s.hashes_offered = hashes_offered; s.hashes = hashes;
  s.groups_per_block = 256 / lanes;
  return s;
}

// ---- the second stream of a RangeProofNi verify --------------------------------------------------------------------------------------
// enc_blocks: workgroups the bound of the work list would fill on the n^2-sized kernel; forced: $ZKP_TWO_STREAMS (A/B switch: 1 = the two-stream
// shape for every batch size, 0 = never), -1 when it is not set.
// Round 6, throughput engine (tools/dev/two_streams_sweep.py, profiles/r06/two_streams_sweep_w36.txt): the second stream pays up to 192 proofs
// (-3 ... -4.5 %) and again from 1536 on (-1.6 %; 4096: -0.4 %: the hash of the whole batch, 10 - 18 ms, hides behind the Enc launch); in
// between — 224 ... 384 proofs, where the Enc launch needs every resident workgroup slot for its one round — the hash wavefronts hold
// registers the Enc workgroups are waiting for: +5 ... +35 %.  The other engines keep the rule their sweeps were made with.
// (latency engine: up to the 40 proofs the library sends it under one key — 16 proofs' worth of workgroups per compute unit and a half more;
//  the rule stopped at 32 until the end of round 6, and 33 - 40 proofs paid the hash in front of their Enc launch: 28.4 against 24.3 - 26.1 ms)
inline bool two_streams(const RouteKnobs& k, uint64_t enc_blocks, int forced) {
  if (forced >= 0) return forced == 1;
  const uint64_t cus = (uint64_t)k.cus;
  if (k.w == 36) return enc_blocks <= 3 * cus / 2 || enc_blocks >= 12 * cus;
  if (k.w == 9) return enc_blocks <= 5 * cus / 2;
  return enc_blocks <= 11 * cus / 4;      // (mid engine: up to the 81 ... 88 proofs whose expected items fit its one round)
}

}  // namespace zkp
