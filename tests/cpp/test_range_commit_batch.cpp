// The batch forms of the verifier's commitment of the interactive RangeProof (zk-paillier_amd/host/zkproofs.hpp): verifier_commit_batch_seeded and
// verifier_reveal_batch_seeded from a VerifierSeed, verify_commit_batch — against the single-session verifier_commit / verify_commit arithmetic
// on the same (r, e), with the sessions the fixed layout cannot carry taking the single-session host path.
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

static bool same(const Result& a, const Result& b) {
  return a.would_panic() == b.would_panic() && a.is_unsupported() == b.is_unsupported() && (a.would_panic() || a.is_unsupported() || a.is_ok() == b.is_ok());
}

static Result single(const EncryptionKey& ek, const Commitment& c, const ChallengeRandomness& r, const ChallengeBits& e) {
  try { return RangeProof::verify_commit(ek, c, r, e); }
  catch (const Panic& p) { return Result::panicked(p.what()); }
  catch (const std::exception& x) { return Result::unsupported(x.what()); }
}

struct Opened { std::vector<Commitment> coms; std::vector<ChallengeRandomness> rs; std::vector<ChallengeBits> es; };

static Opened commit_and_reveal(const std::vector<EncryptionKey>& keys, const RangeProof::VerifierSeed& seed, uint64_t first, size_t sessions) {
  Opened o;
  o.coms = RangeProof::verifier_commit_batch_seeded(keys, seed, first, sessions);
  for (auto& re : RangeProof::verifier_reveal_batch_seeded(keys, seed, first, sessions)) { o.rs.push_back(re.first); o.es.push_back(re.second); }
  return o;
}

static void a_batch_of_sessions_equals_the_single_session_functions() {
  auto [ek, dk] = test_keypair().keys();
  const std::vector<EncryptionKey> keys{ek};
  const RangeProof::VerifierSeed seed = RangeProof::VerifierSeed::fresh();
  const Opened o = commit_and_reveal(keys, seed, 5, 6);
  ASSERT(o.coms.size() == 6 && o.rs.size() == 6 && o.es.size() == 6);
  for (int b = 0; b < 6; b++) {
    ASSERT(o.es[b].bytes.size() == RangeProof::STATISTICAL_ERROR_FACTOR / 8 && o.rs[b].r < ek.n && !o.rs[b].r.is_zero());
    // what the single-session verifier_commit computes from this (r, e)
    ASSERT(o.coms[b].com == RangeProof::get_paillier_commitment(ek, RangeProof::compute_digest(o.es[b].bytes), o.rs[b].r));
    ASSERT(RangeProof::verify_commit(ek, o.coms[b], o.rs[b], o.es[b]).is_ok());
  }
  auto v = RangeProof::verify_commit_batch(keys, o.coms, o.rs, o.es);
  ASSERT(v.size() == 6);
  for (int b = 0; b < 6; b++) ASSERT(v[b].is_ok());
  // a function of (seed, index, key): the same call again, a chunk at its own index, another index, another seed
  const Opened again = commit_and_reveal(keys, seed, 5, 6);
  for (int b = 0; b < 6; b++) ASSERT(again.coms[b].com == o.coms[b].com && again.rs[b].r == o.rs[b].r && again.es[b].bytes == o.es[b].bytes);
  const Opened tail = commit_and_reveal(keys, seed, 8, 3);
  for (int b = 0; b < 3; b++) ASSERT(tail.coms[b].com == o.coms[3 + b].com && tail.rs[b].r == o.rs[3 + b].r && tail.es[b].bytes == o.es[3 + b].bytes);
  const Opened moved = commit_and_reveal(keys, seed, 6, 1);
  ASSERT(moved.coms[0].com == o.coms[1].com && !(moved.coms[0].com == o.coms[0].com));
  const Opened other = commit_and_reveal(keys, RangeProof::VerifierSeed::fresh(), 5, 1);
  ASSERT(!(other.coms[0].com == o.coms[0].com) && !(other.rs[0].r == o.rs[0].r));
  // a commitment of the single-session verifier_commit is accepted by the batch form
  auto vc = RangeProof::verifier_commit(ek);
  ASSERT(RangeProof::verify_commit_batch(keys, {vc.com}, {vc.r}, {vc.e})[0].is_ok());
  ASSERT(RangeProof::verifier_commit_batch_seeded({}, seed).empty() && RangeProof::verify_commit_batch(keys, {}, {}, {}).empty());
}

static void tampered_sessions_and_sessions_the_layout_cannot_carry() {
  auto [ek, dk] = test_keypair().keys();
  const std::vector<EncryptionKey> keys{ek};
  const Opened o = commit_and_reveal(keys, RangeProof::VerifierSeed::fresh(), 0, 8);
  Opened t = o;
  t.coms[1].com = o.coms[1].com + BigInt(1);                                  // another commitment
  t.rs[2].r = o.rs[2].r + BigInt::pow2(2048 + 5);                            // an over-wide r, not congruent to r: the host path rejects it
  t.es[3].bytes.resize(33, 0);                                               // 33 bytes of e: the host path hashes all of them
  t.coms[4].com = -o.coms[4].com;                                            // a negative commitment
  t.es[5].bytes[0] ^= 1;                                                     // another challenge
  t.rs[6].r = o.rs[6].r + ek.n * BigInt::pow2(2048);                         // an over-wide r congruent to r mod n: the reference accepts it
  auto v = RangeProof::verify_commit_batch(keys, t.coms, t.rs, t.es);
  ASSERT(v.size() == 8);
  for (int b = 0; b < 8; b++) ASSERT(same(v[b], single(ek, t.coms[b], t.rs[b], t.es[b])));
  ASSERT(v[0].is_ok() && v[1].is_err() && v[2].is_err() && v[3].is_err() && v[4].is_err() && v[5].is_err() && v[6].is_ok() && v[7].is_ok());
  // a session that really committed to 33 bytes is accepted, through the host path
  ChallengeBits e33;
  e33.bytes.assign(33, 0x5a);
  Commitment c33{RangeProof::get_paillier_commitment(ek, RangeProof::compute_digest(e33.bytes), o.rs[0].r)};
  auto w = RangeProof::verify_commit_batch(keys, {o.coms[0], c33}, {o.rs[0], o.rs[0]}, {o.es[0], e33});
  ASSERT(w[0].is_ok() && w[1].is_ok());
  // a key outside the domain takes the single-session path too; the seeded calls refuse it
  EncryptionKey even{ek.n - BigInt(1), (ek.n - BigInt(1)) * (ek.n - BigInt(1))};
  auto u = RangeProof::verify_commit_batch({ek, even}, {o.coms[0], o.coms[1]}, {o.rs[0], o.rs[1]}, {o.es[0], o.es[1]});
  ASSERT(u[0].is_ok() && same(u[1], single(even, o.coms[1], o.rs[1], o.es[1])) && !u[1].is_ok());
  EncryptionKey tiny{BigInt::pow2(199) + BigInt(1), (BigInt::pow2(199) + BigInt(1)) * (BigInt::pow2(199) + BigInt(1))};
  bool refused = false;
  try { (void)RangeProof::verifier_commit_batch_seeded({tiny}, RangeProof::VerifierSeed::fresh(), 0, 2); } catch (const std::invalid_argument&) { refused = true; }
  ASSERT(refused);
}

static void one_key_per_session() {
  auto [ek, dk] = test_keypair().keys();
  const BigInt n2 = ek.n + BigInt(2);                                        // (Enc and the sampler read a key as an odd number)
  const EncryptionKey ek2{n2, n2 * n2};
  const std::vector<EncryptionKey> keys{ek, ek2, ek};
  const RangeProof::VerifierSeed seed = RangeProof::VerifierSeed::fresh();
  const Opened o = commit_and_reveal(keys, seed, 1, 0);
  ASSERT(o.coms.size() == 3);
  for (int b = 0; b < 3; b++) {
    ASSERT(o.coms[b].com == RangeProof::get_paillier_commitment(keys[b], RangeProof::compute_digest(o.es[b].bytes), o.rs[b].r));
    ASSERT(o.rs[b].r < keys[b].n);
  }
  auto v = RangeProof::verify_commit_batch(keys, o.coms, o.rs, o.es);
  ASSERT(v[0].is_ok() && v[1].is_ok() && v[2].is_ok());
  // session 1's opening under session 0's key
  auto x = RangeProof::verify_commit_batch({ek, ek, ek}, o.coms, o.rs, o.es);
  ASSERT(x[0].is_ok() && x[1].is_err() && x[2].is_ok());
  // e does not depend on the key, r does
  const Opened shared = commit_and_reveal({ek}, seed, 1, 3);
  ASSERT(shared.es[1].bytes == o.es[1].bytes && shared.coms[0].com == o.coms[0].com && !(shared.coms[1].com == o.coms[1].com));
}

int main() {
  struct T { const char* name; void (*fn)(); } tests[] = {
      {"a_batch_of_sessions_equals_the_single_session_functions", a_batch_of_sessions_equals_the_single_session_functions},
      {"tampered_sessions_and_sessions_the_layout_cannot_carry", tampered_sessions_and_sessions_the_layout_cannot_carry},
      {"one_key_per_session", one_key_per_session},
  };
  int failed = 0;
  for (auto& t : tests) {
    try { t.fn(); std::printf("PASS %s\n", t.name); }
    catch (const std::exception& e) { std::printf("FAIL %s: %s\n", t.name, e.what()); failed++; }
  }
  return failed ? 1 : 0;
}
