// Paillier::open / decrypt / verify_opening and their batch forms (zk-paillier_amd/host/zkproofs.hpp) on zkp_paillier_open_batch:
// the reference's own test of verify_opening (correct_opening.rs:48-56) — encrypt 10 under the fixture key, open with the decryption key,
// verify the opening —, decrypt_batch of 17 ciphertexts, ciphertexts the fixed layout cannot carry, and the Panic of a one-item open on c = 0.
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

static void correct_opening() {   // correct_opening.rs:48-56
  auto [ek, dk] = test_keypair().keys();
  const BigInt m(10), r0 = BigInt::sample_below(ek.n);
  const BigInt c = Paillier::encrypt_with_chosen_randomness(ek, m, r0);
  auto [m2, r] = Paillier::open(dk, c);
  ASSERT(m2 == m && r == r0);
  ASSERT(Paillier::verify_opening(ek, m2, r, c));
  ASSERT(!Paillier::verify_opening(ek, m2 + BigInt::one(), r, c));
  ASSERT(Paillier::decrypt(dk, c) == m);
}

static void batches() {
  auto [ek, dk] = test_keypair().keys();
  std::vector<BigInt> ms, rs, cs;
  for (int i = 0; i < 17; i++) {
    ms.push_back(i == 0 ? BigInt::zero() : i == 1 ? ek.n - BigInt::one() : BigInt::sample_below(ek.n));
    rs.push_back(i == 2 ? BigInt::one() : BigInt::sample_below(ek.n));
    cs.push_back(Paillier::encrypt_with_chosen_randomness(ek, ms[i], rs[i]));
  }
  auto dec = Paillier::decrypt_batch(dk, cs);
  ASSERT(dec.size() == 17);
  for (int i = 0; i < 17; i++) ASSERT(!dec[i].malformed && dec[i].m == ms[i] && dec[i].r.is_zero());
  // a batch form returns MALFORMED as a status and keeps the neighbours; what the layout cannot carry is reduced modulo n^2 on the host
  std::vector<BigInt> odd = {cs[3], BigInt::zero(), cs[4] - ek.nn, cs[5] + ek.nn * BigInt::pow2(4096), dk.p * BigInt(7), cs[6]};
  auto op = Paillier::open_batch(dk, odd);
  ASSERT(!op[0].malformed && op[0].m == ms[3] && op[0].r == rs[3]);
  ASSERT(op[1].malformed && op[1].m.is_zero() && op[1].r.is_zero());
  ASSERT(!op[2].malformed && op[2].m == ms[4] && op[2].r == rs[4]);
  ASSERT(!op[3].malformed && op[3].m == ms[5] && op[3].r == rs[5]);
  ASSERT(op[4].malformed);
  ASSERT(!op[5].malformed && op[5].m == ms[6] && op[5].r == rs[6]);
  ASSERT(Paillier::open_batch(dk, {}).empty());
  // keys outside the domain: p = q; a factor that is not positive
  ASSERT(Paillier::decrypt_batch(DecryptionKey{dk.p, dk.p}, {cs[0]})[0].malformed);
  ASSERT(Paillier::decrypt_batch(DecryptionKey{-dk.p, dk.q}, {cs[0], cs[1]})[1].malformed);
}

static void one_item_forms_panic() {
  auto [ek, dk] = test_keypair().keys();
  (void)ek;
  bool open_panicked = false, decrypt_panicked = false;
  try { (void)Paillier::open(dk, BigInt::zero()); } catch (const Panic&) { open_panicked = true; }
  try { (void)Paillier::decrypt(dk, dk.q); } catch (const Panic&) { decrypt_panicked = true; }
  ASSERT(open_panicked && decrypt_panicked);
}

int main() {
  int failures = 0;
  struct { const char* name; void (*f)(); } tests[] = {{"correct_opening", correct_opening}, {"batches", batches}, {"one_item_forms_panic", one_item_forms_panic}};
  for (auto& t : tests) {
    try { t.f(); std::printf("PASS %s\n", t.name); }
    catch (const Panic& e) { std::printf("FAIL %s  [panic: %s]\n", t.name, e.what()); failures++; }
    catch (const std::exception& e) { std::printf("FAIL %s  [%s]\n", t.name, e.what()); failures++; }
  }
  return failures ? 1 : 0;
}
