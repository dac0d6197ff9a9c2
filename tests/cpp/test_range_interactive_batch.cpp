// The batch forms of the interactive RangeProof (zk-paillier_amd/host/zkproofs.hpp): generate_encrypted_pairs_batch_seeded and
// generate_proof_batch_seeded from a ProverSeed, verifier_output_json_batch on the two received documents of every session — GPU verdicts
// for the sessions the device readers convert, the host parser + verifier_output for the ones they hand back, a panic for what is no document.
// Needs a gfx950 GPU.  Exit code 0 = all passed.
#include <cstdio>
#include <string>

#include "../../zk-paillier_amd/host/zkproofs.hpp"

using namespace zkproofs;

#define ASSERT(c) do { if (!(c)) throw Panic(std::string("assertion failed: ") + #c); } while (0)

static Keypair test_keypair() {   // range_proof_ni.rs:141-145
  return Keypair{
      BigInt::from_str_radix10("148677972634832330983979593310074301486537017973460461278300587514468301043894574906886127642530475786889672304776052879927627556769456140664043088700743909632312483413393134504352834240399191134336344285483935856491230340093391784574980688823380828143810804684752914935441384845195613674104960646037368551517"),
      BigInt::from_str_radix10("158741574437007245654463598139927898730476924736461654463975966787719309357536545869203069369466212089132653564188443272208127277664424448947476335413293018778018615899291704693105620242763173357203898195318179150836424196645745308205164116144020613415407736216097185962171301808761138424668335445923774195463")};
}

static const size_t EF = RangeProof::STATISTICAL_ERROR_FACTOR;

struct Sessions {
  std::vector<BigInt> ranges, xs, rs, ciphers;
  std::vector<ChallengeBits> challenges;
  std::vector<EncryptedPairs> pairs;
  std::vector<Proof> proofs;
  std::vector<std::string> pairs_docs, proof_docs;
};

// B sessions run through both seeded steps; session `dishonest` has x far outside its range
static Sessions run_sessions(const EncryptionKey& ek, int B, int dishonest, const RangeProof::ProverSeed& seed, uint64_t first_index) {
  Sessions s;
  for (int i = 0; i < B; i++) {
    BigInt range = BigInt::sample(256);
    BigInt r = BigInt::sample_below(ek.n);
    BigInt x = i == dishonest ? BigInt::sample_range(BigInt(100) * range, BigInt(10000) * range) : BigInt::sample_below(range.div_floor(BigInt(3)));
    s.ranges.push_back(range); s.xs.push_back(x); s.rs.push_back(r);
    s.ciphers.push_back(Paillier::encrypt_with_chosen_randomness(ek, x, r));
  }
  s.pairs = RangeProof::generate_encrypted_pairs_batch_seeded(ek, s.ranges, EF, seed, first_index);
  for (int i = 0; i < B; i++) s.challenges.push_back(RangeProof::verifier_commit(ek).e);
  s.proofs = RangeProof::generate_proof_batch_seeded(ek, s.xs, s.rs, s.challenges, s.ranges, EF, seed, first_index);
  for (int i = 0; i < B; i++) {
    s.pairs_docs.push_back(serde_json::to_string(s.pairs[i], ek));
    s.proof_docs.push_back(serde_json::to_string(s.proofs[i], ek));
  }
  return s;
}

static std::string replaced(std::string s, const std::string& from, const std::string& to) {
  const size_t at = s.find(from);
  ASSERT(at != std::string::npos);
  return s.replace(at, from.size(), to);
}

static bool same(const Result& a, const Result& b) { return a.would_panic() == b.would_panic() && (a.would_panic() || a.is_ok() == b.is_ok()); }

static void seeded_steps_make_sessions_the_verifier_accepts() {
  auto [ek, dk] = test_keypair().keys();
  const RangeProof::ProverSeed seed = RangeProof::ProverSeed::fresh();
  Sessions s = run_sessions(ek, 5, 3, seed, 7);
  ASSERT(s.pairs.size() == 5 && s.proofs.size() == 5);
  for (int i = 0; i < 5; i++) {
    ASSERT(s.pairs[i].c1.size() == EF && s.pairs[i].c2.size() == EF && s.proofs[i].responses.size() == EF);
    ASSERT(RangeProof::verifier_output(ek, s.challenges[i], s.pairs[i], s.proofs[i], s.ranges[i], s.ciphers[i], EF).is_ok() == (i != 3));
  }
  // the commitments are a function of (seed, index, key, range): the same call again gives the same pairs, a chunk at its own index its
  // slice of them, another index or another seed other pairs
  auto again = RangeProof::generate_encrypted_pairs_batch_seeded(ek, s.ranges, EF, seed, 7);
  for (int i = 0; i < 5; i++) ASSERT(again[i].c1 == s.pairs[i].c1 && again[i].c2 == s.pairs[i].c2);
  auto tail = RangeProof::generate_encrypted_pairs_batch_seeded(ek, {s.ranges[3], s.ranges[4]}, EF, seed, 10);
  ASSERT(tail[0].c1 == s.pairs[3].c1 && tail[1].c2 == s.pairs[4].c2);
  auto moved = RangeProof::generate_encrypted_pairs_batch_seeded(ek, s.ranges, EF, seed, 8);
  ASSERT(!(moved[0].c1[0] == s.pairs[0].c1[0]));
  auto other = RangeProof::generate_encrypted_pairs_batch_seeded(ek, s.ranges, EF, RangeProof::ProverSeed::fresh(), 7);
  ASSERT(!(other[0].c1[0] == s.pairs[0].c1[0]));
  ASSERT(!(s.pairs[0].c1[0] == s.pairs[0].c1[1]) && !(s.pairs[0].c1[0] == s.pairs[1].c1[0]));
  // a challenge too short for the error factor: generate_proof panics, in the batch as for one session
  auto short_challenges = s.challenges;
  short_challenges[1].bytes.pop_back();
  bool panicked = false;
  try { (void)RangeProof::generate_proof_batch_seeded(ek, s.xs, s.rs, short_challenges, s.ranges, EF, seed, 7); } catch (const Panic&) { panicked = true; }
  ASSERT(panicked);
  ASSERT(RangeProof::generate_encrypted_pairs_batch_seeded(ek, {}, EF, seed).empty());
}

static void documents_get_the_verdicts_of_their_sessions() {
  auto [ek, dk] = test_keypair().keys();
  Sessions s = run_sessions(ek, 5, 3, RangeProof::ProverSeed::fresh(), 0);
  auto r = RangeProof::verifier_output_json_batch(ek, s.challenges, s.pairs_docs, s.proof_docs, s.ranges, s.ciphers, EF);
  ASSERT(r.size() == 5);
  for (int i = 0; i < 5; i++) ASSERT(r[i].is_ok() == (i != 3));
  // one digit of each commitment of row 0 (an Open row checks both, a Mask row the one its j names), a flipped challenge bit, a short
  // challenge: only those sessions' results change
  auto pd = s.pairs_docs;
  for (const char* field : {"\"c1\":[\"", "\"c2\":[\""}) {
    const size_t at = pd[1].find(field) + 20;
    pd[1][at] = pd[1][at] == '4' ? '6' : '4';
  }
  auto ch = s.challenges;
  ch[2].bytes[0] ^= 0x80;
  ch[4].bytes.pop_back();
  r = RangeProof::verifier_output_json_batch(ek, ch, pd, s.proof_docs, s.ranges, s.ciphers, EF);
  ASSERT(r[0].is_ok() && r[1].is_err() && r[2].is_err() && r[3].is_err() && r[4].would_panic());
  ASSERT(RangeProof::verifier_output_json_batch(ek, {}, {}, {}, {}, {}, EF).empty());
}

static void sessions_the_device_readers_hand_back() {
  auto [ek, dk] = test_keypair().keys();
  Sessions s = run_sessions(ek, 6, -1, RangeProof::ProverSeed::fresh(), 0);
  auto pd = s.pairs_docs, fd = s.proof_docs;
  auto ch = s.challenges;
  pd[1] = replaced(pd[1], "\"c2\":", " \"c2\" : ");                       // white space: the host tokeniser reads it, the GPU verifies it
  fd[2] = replaced(fd[2], "\"masked_r\":\"", "\"masked_r\":\"-");         // a negative response: a valid Proof, verified on the host path
  pd[3] = pd[3].substr(0, pd[3].size() / 2);                              // no document
  fd[4] = "[]";                                                           // a Proof of no rows: the reference indexes past its end
  ch[5].bytes.resize(33, 0);                                              // more challenge bytes than the ABI carries: the general path
  auto r = RangeProof::verifier_output_json_batch(ek, ch, pd, fd, s.ranges, s.ciphers, EF);
  ASSERT(r.size() == 6);
  ASSERT(r[0].is_ok() && r[1].is_ok());
  auto single = [&](int b) -> Result {
    try { return RangeProof::verifier_output(ek, ch[b], serde_json::encrypted_pairs_from_str_host(pd[b]), serde_json::proof_from_str_host(fd[b]), s.ranges[b], s.ciphers[b], EF); }
    catch (const Panic& p) { return Result::panicked(p.what()); }
  };
  ASSERT(same(r[2], single(2)));
  ASSERT(r[3].would_panic());
  ASSERT(r[4].would_panic() && same(r[4], single(4)));
  ASSERT(r[5].is_ok() && same(r[5], single(5)));
  // a statement the layout cannot carry keeps its session from the call, the others stay in it
  auto ranges = s.ranges;
  ranges[0] = BigInt::pow2(2048 + 5);
  auto w = RangeProof::verifier_output_json_batch(ek, s.challenges, s.pairs_docs, s.proof_docs, ranges, s.ciphers, EF);
  Result want = [&]() -> Result {
    try { return RangeProof::verifier_output(ek, s.challenges[0], s.pairs[0], s.proofs[0], ranges[0], s.ciphers[0], EF); } catch (const Panic& p) { return Result::panicked(p.what()); }
  }();
  ASSERT(same(w[0], want));
  for (int i = 1; i < 6; i++) ASSERT(w[i].is_ok());
}

int main() {
  struct T { const char* name; void (*fn)(); } tests[] = {
      {"seeded_steps_make_sessions_the_verifier_accepts", seeded_steps_make_sessions_the_verifier_accepts},
      {"documents_get_the_verdicts_of_their_sessions", documents_get_the_verdicts_of_their_sessions},
      {"sessions_the_device_readers_hand_back", sessions_the_device_readers_hand_back},
  };
  int failed = 0;
  for (auto& t : tests) {
    try { t.fn(); std::printf("PASS %s\n", t.name); }
    catch (const std::exception& e) { std::printf("FAIL %s: %s\n", t.name, e.what()); failed++; }
  }
  return failed ? 1 : 0;
}
