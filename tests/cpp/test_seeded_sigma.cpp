// prove_batch_seeded of ZeroProof, CiphertextProof, CorrectMessageProof and CompositeDLogProof (zk-paillier_amd/host/zkproofs.hpp): the nonces
// are expanded on the GPU from a seed the host layer draws itself; the proofs must verify like those of prove.  Needs a gfx950 GPU.
// Exit code 0 = all passed.
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

static void seeded_sigma_round_trips() {
  auto [ek, dk] = test_keypair().keys();
  const size_t B = 5;

  // ZeroProof (zero_enc_proof.rs:112-131); proof 3 is about a ciphertext of 1
  std::vector<ZeroWitness> zw;
  std::vector<ZeroStatement> zs;
  for (size_t i = 0; i < B; i++) {
    BigInt r = BigInt::sample_below(ek.n);
    zw.push_back({r});
    zs.push_back({ek, Paillier::encrypt_with_chosen_randomness(ek, i == 3 ? BigInt(1) : BigInt(0), r)});
  }
  auto zp = ZeroProof::prove_batch_seeded(zw, zs);
  ASSERT(zp.size() == B);
  for (size_t i = 0; i < B; i++) ASSERT(zp[i].verify(zs[i]).is_ok() == (i != 3));
  // a fresh seed per call, a stream per proof
  auto zp2 = ZeroProof::prove_batch_seeded(zw, zs);
  ASSERT(!(zp2[0].a == zp[0].a) && !(zp[0].a == zp[1].a));

  // CiphertextProof (correct_ciphertext.rs:113-134); the witness of proof 1 has another r
  std::vector<CiphertextWitness> cw;
  std::vector<CiphertextStatement> cs;
  for (size_t i = 0; i < B; i++) {
    BigInt x = BigInt::sample_below(ek.n), r = BigInt::sample_below(ek.n);
    cs.push_back({ek, Paillier::encrypt_with_chosen_randomness(ek, x, r)});
    cw.push_back({x, i == 1 ? r + BigInt(1) : r});
  }
  auto cp = CiphertextProof::prove_batch_seeded(cw, cs);
  ASSERT(cp.size() == B);
  for (size_t i = 0; i < B; i++) ASSERT(cp[i].verify(cs[i]).is_ok() == (i != 1));
  ASSERT(!(cp[0].c_prime == cp[2].c_prime));

  // CorrectMessageProof (correct_message.rs:169-181): four valid messages, the encrypted one at position i % 4
  std::vector<std::vector<BigInt>> valid;
  std::vector<BigInt> msg;
  for (size_t i = 0; i < B; i++) {
    valid.push_back({BigInt(10 * i + 1), BigInt(10 * i + 2), BigInt(10 * i + 3), BigInt(10 * i + 4)});
    msg.push_back(valid[i][i % 4]);
  }
  auto mp = CorrectMessageProof::prove_batch_seeded(ek, valid, msg);
  ASSERT(mp.size() == B);
  for (size_t i = 0; i < B; i++) { ASSERT(mp[i].verify().is_ok()); ASSERT(mp[i].e_vec.size() == 4); }
  ASSERT(!(mp[0].ciphertext == mp[1].ciphertext) && !(mp[0].z_vec[1] == mp[0].z_vec[2]));
  // a message that is not in its list: the reference's prove panics (:184-200)
  msg[2] = BigInt(999);
  bool panicked = false;
  try { (void)CorrectMessageProof::prove_batch_seeded(ek, valid, msg); } catch (const Panic&) { panicked = true; }
  ASSERT(panicked);

  // CompositeDLogProof (wi_dlog_proof.rs:117-141): ni = g^-s mod N; proof 4 is about ni = g^s (:145-168)
  const BigInt N = ek.n;
  std::vector<DLogStatement> ds;
  std::vector<BigInt> secrets;
  for (size_t i = 0; i < B; i++) {
    BigInt g = BigInt::sample_below(N), s = BigInt::sample(256);
    BigInt gs = mod_pow(g, s, N);
    ds.push_back({N, g, i == 4 ? gs : BigInt::mod_inv(gs, N)});
    secrets.push_back(s);
  }
  auto dp = CompositeDLogProof::prove_batch_seeded(ds, secrets);
  ASSERT(dp.size() == B);
  for (size_t i = 0; i < B; i++) ASSERT(dp[i].verify(ds[i]).is_ok() == (i != 4));
  ASSERT(!(dp[0].x == dp[1].x));
}

int main() {
  int failures = 0;
  try { seeded_sigma_round_trips(); std::printf("PASS seeded_sigma_round_trips\n"); }
  catch (const Panic& e) { std::printf("FAIL seeded_sigma_round_trips  [panic: %s]\n", e.what()); failures++; }
  catch (const std::exception& e) { std::printf("FAIL seeded_sigma_round_trips  [%s]\n", e.what()); failures++; }
  return failures ? 1 : 0;
}
