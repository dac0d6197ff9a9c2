// prove_batch_seeded of VerlinProof and MulProof (zk-paillier_amd/host/zkproofs.hpp): the nonces — r_a and r_d redrawn until they are
// coprime to n — are expanded on the GPU from a seed the host layer draws itself; the proofs must verify like those of prove.
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

static void seeded_coprime_round_trips() {
  auto [ek, dk] = test_keypair().keys();
  const size_t B = 5;

  // VerlinProof (verlin_proof.rs:181-262); the statement of proof 3 is about 2 x (:226-236)
  std::vector<VerlinWitness> vw;
  std::vector<VerlinStatement> vs;
  for (size_t i = 0; i < B; i++) {
    BigInt x = BigInt::sample_below(ek.n), xp = BigInt::sample_below(ek.n), xpp = BigInt::sample_below(ek.n), r_x = sample_paillier_random(ek.n);
    BigInt c = Paillier::encrypt_with_chosen_randomness(ek, x, BigInt::sample_below(ek.n));
    BigInt cp = Paillier::encrypt_with_chosen_randomness(ek, xp, BigInt::sample_below(ek.n));
    vs.push_back({ek, c, cp, gen_phi(ek, c, cp, i == 3 ? x * BigInt(2) : x, xp, xpp, r_x)});
    vw.push_back({x, xp, xpp, r_x});
  }
  auto vp = VerlinProof::prove_batch_seeded(vw, vs);
  ASSERT(vp.size() == B);
  for (size_t i = 0; i < B; i++) ASSERT(vp[i].verify(vs[i]).is_ok() == (i != 3));
  // a fresh seed per call, a stream per proof
  auto vp2 = VerlinProof::prove_batch_seeded(vw, vs);
  ASSERT(!(vp2[0].phi_a == vp[0].phi_a) && !(vp[0].r_z == vp[1].r_z));

  // MulProof (multiplication_proof.rs:172-290); proof 1 is about c = a b + 1
  std::vector<MulWitness> mw;
  std::vector<MulStatement> ms;
  for (size_t i = 0; i < B; i++) {
    BigInt a = BigInt::sample_below(ek.n), b = BigInt::sample_below(ek.n);
    BigInt c = (a * b) % ek.n;
    if (i == 1) c = c + BigInt::one();
    BigInt r_a = sample_paillier_random(ek.n), r_b = sample_paillier_random(ek.n), r_c = sample_paillier_random(ek.n);
    ms.push_back({ek, Paillier::encrypt_with_chosen_randomness(ek, a, r_a), Paillier::encrypt_with_chosen_randomness(ek, b, r_b),
                  Paillier::encrypt_with_chosen_randomness(ek, c, r_c)});
    mw.push_back({a, b, c, r_a, r_b, r_c});
  }
  auto mp = MulProof::prove_batch_seeded(mw, ms);
  ASSERT(mp.size() == B);
  for (size_t i = 0; i < B; i++) ASSERT(mp[i].verify(ms[i]).is_ok() == (i != 1));
  auto mp2 = MulProof::prove_batch_seeded(mw, ms);
  ASSERT(!(mp2[0].e_d == mp[0].e_d) && !(mp[0].e_d == mp[2].e_d));

  // one witness per statement
  bool refused = false;
  mw.pop_back();
  try { (void)MulProof::prove_batch_seeded(mw, ms); } catch (const std::invalid_argument&) { refused = true; }
  ASSERT(refused);
}

int main() {
  int failures = 0;
  try { seeded_coprime_round_trips(); std::printf("PASS seeded_coprime_round_trips\n"); }
  catch (const Panic& e) { std::printf("FAIL seeded_coprime_round_trips  [panic: %s]\n", e.what()); failures++; }
  catch (const std::exception& e) { std::printf("FAIL seeded_coprime_round_trips  [%s]\n", e.what()); failures++; }
  return failures ? 1 : 0;
}
