// The batched interactive CorrectKey of zk-paillier_amd/host/zkproofs.hpp on zkp_correct_key_challenge_seeded_batch,
// zkp_correct_key_prove_batch and zkp_correct_key_verify_seeded_batch: prove_batch over three keys — the fixture key of the reference's
// tests, the same key with its factors swapped, a 1024-bit key of two smaller primes — equals three prove() calls; the seeded challenge,
// prove_batch and verify_batch_seeded round trip accepts, and rejects a touched proof and another seed; a ragged session takes the
// single-session path and gives the same ProveResult.  Needs a gfx950 GPU.  Exit code 0 = all passed.
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

// two 127-bit primes (2^127 - 1 and 2^127 - 25, the largest prime below it): a key of the 1024-bit kernel width
static DecryptionKey small_key() {
  return DecryptionKey{BigInt::from_str_radix10("170141183460469231731687303715884105727"), BigInt::from_str_radix10("170141183460469231731687303715884105703")};
}

static bool same(const CorrectKey::ProveResult& a, const CorrectKey::ProveResult& b) {
  return a.ok == b.ok && (a.ok ? a.proof.s_digest == b.proof.s_digest : a.err == b.err);
}

struct Sessions {
  DecryptionKey dk, swapped, small;
  std::vector<EncryptionKey> eks;
  std::vector<const DecryptionKey*> dks;
  Sessions() {
    auto [ek, d] = test_keypair().keys();
    dk = d; swapped = DecryptionKey{d.q, d.p}; small = small_key();
    const BigInt ns = small.p * small.q;
    eks = {ek, EncryptionKey{ns, ns * ns}, ek};
    dks = {&dk, &small, &swapped};
  }
};

static void prove_batch_equals_single_proves() {
  const Sessions s;
  const CorrectKey::VerifierSeed seed = CorrectKey::VerifierSeed::fresh();
  std::vector<Challenge> ch = CorrectKey::challenge_batch_seeded(s.eks, seed, 7);
  ASSERT(ch.size() == 3 && ch[0].sn.size() == CorrectKey::STATISTICAL_ERROR_FACTOR);
  ch[2].e = ch[2].e + BigInt::one();                              // a wrong challenge: EWasntComputedCorrectly, on both paths
  const std::vector<CorrectKey::ProveResult> got = CorrectKey::prove_batch(s.dks, ch);
  ASSERT(got.size() == 3);
  for (size_t k = 0; k < 3; k++) ASSERT(same(got[k], CorrectKey::prove(*s.dks[k], ch[k])));
  ASSERT(got[0].is_ok() && got[1].is_ok() && got[2].is_err() && got[2].err == CorrectKeyProveError::EWasntComputedCorrectly);
  ASSERT(CorrectKey::prove_batch({}, {}).empty());
}

static void seeded_round_trip_accepts() {
  const Sessions s;
  const CorrectKey::VerifierSeed seed = CorrectKey::VerifierSeed::fresh(), other = CorrectKey::VerifierSeed::fresh();
  std::vector<VerificationAid> aids;
  const std::vector<Challenge> ch = CorrectKey::challenge_batch_seeded(s.eks, seed, 1000, aids);
  const std::vector<Challenge> again = CorrectKey::challenge_batch_seeded(s.eks, seed, 1000);
  ASSERT(aids.size() == 3 && again.size() == 3);
  for (size_t k = 0; k < 3; k++) ASSERT(again[k].e == ch[k].e && again[k].sn == ch[k].sn && again[k].z == ch[k].z);
  const std::vector<CorrectKey::ProveResult> res = CorrectKey::prove_batch(s.dks, ch);
  std::vector<CorrectKeyProof> proofs;
  for (size_t k = 0; k < 3; k++) {
    ASSERT(res[k].is_ok());
    ASSERT(CorrectKey::verify(res[k].unwrap(), aids[k]).is_ok());  // the stored aid and the regenerated one agree
    proofs.push_back(res[k].unwrap());
  }
  std::vector<Result> v = CorrectKey::verify_batch_seeded(s.eks, seed, 1000, proofs);
  ASSERT(v.size() == 3 && v[0].is_ok() && v[1].is_ok() && v[2].is_ok());
  proofs[1].s_digest = proofs[1].s_digest + BigInt::one();
  v = CorrectKey::verify_batch_seeded(s.eks, seed, 1000, proofs);
  ASSERT(v[0].is_ok() && !v[1].is_ok() && v[2].is_ok());
  v = CorrectKey::verify_batch_seeded(s.eks, other, 1000, proofs);
  ASSERT(!v[0].is_ok() && !v[1].is_ok() && !v[2].is_ok());
  v = CorrectKey::verify_batch_seeded(s.eks, seed, 1001, proofs);
  ASSERT(!v[0].is_ok() && !v[2].is_ok());
}

static void ragged_session_takes_the_fallback() {
  const Sessions s;
  const CorrectKey::VerifierSeed seed = CorrectKey::VerifierSeed::fresh();
  std::vector<Challenge> ch = CorrectKey::challenge_batch_seeded(s.eks, seed, 0, nullptr, 4);
  ch[1].sn.pop_back(); ch[1].z.pop_back();                        // a number of rounds of its own
  ch[2].z.pop_back();                                             // |sn| != |z|: the reference zips, the single-session path does what it does
  const std::vector<CorrectKey::ProveResult> got = CorrectKey::prove_batch(s.dks, ch);
  ASSERT(got[0].is_ok());
  ASSERT(same(got[1], CorrectKey::prove(*s.dks[1], ch[1])));
  bool threw = false;
  CorrectKey::ProveResult one{false, CorrectKeyProof{}, CorrectKeyProveError::SniNotCoprimeWithN};
  try { one = CorrectKey::prove(*s.dks[2], ch[2]); } catch (const std::exception&) { threw = true; }
  if (!threw) ASSERT(same(got[2], one));
  std::vector<Challenge> wide = CorrectKey::challenge_batch_seeded(s.eks, seed, 0, nullptr, 2);
  wide[0].e = wide[0].e + BigInt::pow2(256);                       // e >= 2^256: no 8-word value
  const std::vector<CorrectKey::ProveResult> w = CorrectKey::prove_batch(s.dks, wide);
  ASSERT(w[0].is_err() && same(w[0], CorrectKey::prove(*s.dks[0], wide[0])) && w[1].is_ok() && w[2].is_ok());
}

int main() {
  int failures = 0;
  struct { const char* name; void (*f)(); } tests[] = {{"prove_batch_equals_single_proves", prove_batch_equals_single_proves},
                                                       {"seeded_round_trip_accepts", seeded_round_trip_accepts},
                                                       {"ragged_session_takes_the_fallback", ragged_session_takes_the_fallback}};
  for (auto& t : tests) {
    try { t.f(); std::printf("PASS %s\n", t.name); }
    catch (const Panic& e) { std::printf("FAIL %s  [panic: %s]\n", t.name, e.what()); failures++; }
    catch (const std::exception& e) { std::printf("FAIL %s  [%s]\n", t.name, e.what()); failures++; }
  }
  return failures ? 1 : 0;
}
