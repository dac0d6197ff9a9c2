// RangeProofNi::prove_batch_seeded (zk-paillier_amd/host/zkproofs.hpp): the witness is expanded on the GPU from a seed the host layer
// draws itself; the proofs must verify like those of prove_batch.  Needs a gfx950 GPU.  Exit code 0 = all passed.
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

static void seeded_batch_round_trip() {
  auto [ek, dk] = test_keypair().keys();
  std::vector<RangeProofNi::Statement> st;
  for (int i = 0; i < 6; i++) {
    BigInt range = BigInt::sample(256);
    BigInt r = BigInt::sample_below(ek.n);
    BigInt x = i == 4 ? BigInt::sample_range(BigInt(100) * range, BigInt(10000) * range) : BigInt::sample_below(range.div_floor(BigInt(3)));
    st.push_back({range, Paillier::encrypt_with_chosen_randomness(ek, x, r), x, r});
  }
  auto proofs = RangeProofNi::prove_batch_seeded(ek, st);
  ASSERT(proofs.size() == 6);
  std::vector<const RangeProofNi*> ptr;
  for (auto& p : proofs) ptr.push_back(&p);
  auto res = RangeProofNi::verify_batch(ek, ptr);
  for (int i = 0; i < 6; i++) ASSERT(res[i].is_ok() == (i != 4));
  // a fresh seed per call: the same statements again give other commitments
  auto again = RangeProofNi::prove_batch_seeded(ek, st);
  ASSERT(!(again[0].encrypted_pairs.c1[0] == proofs[0].encrypted_pairs.c1[0]));
  // every row's witness differs from every other row's (one stream per row, not one per proof)
  ASSERT(!(proofs[0].encrypted_pairs.c1[0] == proofs[0].encrypted_pairs.c1[1]));
  ASSERT(!(proofs[0].encrypted_pairs.c1[0] == proofs[1].encrypted_pairs.c1[0]));
}

int main() {
  int failures = 0;
  try { seeded_batch_round_trip(); std::printf("PASS seeded_batch_round_trip\n"); }
  catch (const Panic& e) { std::printf("FAIL seeded_batch_round_trip  [panic: %s]\n", e.what()); failures++; }
  return failures ? 1 : 0;
}
