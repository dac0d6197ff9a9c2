// DLogStatement::generate_batch_seeded, wi_dlog_proof::legendre_symbol and wi_dlog_proof::jacobi_symbol (zk-paillier_amd/host/zkproofs.hpp):
// the reference's tests test_correct_dlog_proof and test_bad_dlog_proof (wi_dlog_proof.rs:117-168) on statements set up on the GPU without
// the factors of N, and the two symbols against each other with the factors at hand.
// Needs a gfx950 GPU.  Exit code 0 = all passed.
#include <cstdio>
#include <string>

#include "../../zk-paillier_amd/host/zkproofs.hpp"

using namespace zkproofs;
using wi_dlog_proof::jacobi_symbol;

#define ASSERT(c) do { if (!(c)) throw Panic(std::string("assertion failed: ") + #c); } while (0)

static Keypair test_keypair() {   // range_proof_ni.rs:141-145
  return Keypair{
      BigInt::from_str_radix10("148677972634832330983979593310074301486537017973460461278300587514468301043894574906886127642530475786889672304776052879927627556769456140664043088700743909632312483413393134504352834240399191134336344285483935856491230340093391784574980688823380828143810804684752914935441384845195613674104960646037368551517"),
      BigInt::from_str_radix10("158741574437007245654463598139927898730476924736461654463975966787719309357536545869203069369466212089132653564188443272208127277664424448947476335413293018778018615899291704693105620242763173357203898195318179150836424196645745308205164116144020613415407736216097185962171301808761138424668335445923774195463")};
}

static void dlog_setup_round_trips() {
  auto [ek, dk] = test_keypair().keys();
  const BigInt one = BigInt::one();
  const size_t B = 5;
  const std::vector<BigInt> N(B, ek.n);
  auto [st, secrets] = DLogStatement::generate_batch_seeded(N);
  ASSERT(st.size() == B && secrets.size() == B);
  for (size_t b = 0; b < B; b++) {
    ASSERT(st[b].N == ek.n && one < st[b].g && st[b].g < ek.n - one && secrets[b] < BigInt::pow2(256));
    // "Jacobi symbol should be -1" (:123), by the reference's own route with p and q, and by ours without them
    ASSERT(wi_dlog_proof::legendre_symbol(st[b].g, dk.p) * wi_dlog_proof::legendre_symbol(st[b].g, dk.q) == -1);
    ASSERT(jacobi_symbol(st[b].g, ek.n) == -1);
    ASSERT(st[b].ni == mod_pow(BigInt::mod_inv(st[b].g, ek.n), secrets[b], ek.n));          // :131-132
  }
  // a stream per statement, a fresh seed per call
  ASSERT(!(st[0].g == st[1].g) && !(secrets[0] == secrets[1]));
  auto again = DLogStatement::generate_batch_seeded(N);
  ASSERT(!(again.first[0].g == st[0].g) && !(again.second[0] == secrets[0]));
  // test_correct_dlog_proof
  auto proofs = CompositeDLogProof::prove_batch_seeded(st, secrets);
  for (size_t b = 0; b < B; b++) ASSERT(proofs[b].verify(st[b]).is_ok());
  // test_bad_dlog_proof: "+secret" instead of "-secret" (:158-159)
  std::vector<DLogStatement> bad = st;
  for (size_t b = 0; b < B; b++) bad[b].ni = mod_pow(st[b].g, secrets[b], ek.n);
  auto bad_proofs = CompositeDLogProof::prove_batch_seeded(bad, secrets);
  for (size_t b = 0; b < B; b++) ASSERT(bad_proofs[b].verify(bad[b]).is_err());

  // the symbols: multiplicative over N = p q; 0 where a shares a factor with N, where the reference's product is never 0
  for (int k = 0; k < 6; k++) {
    const BigInt a = BigInt::sample_below(ek.n);
    ASSERT(jacobi_symbol(a, ek.n) == wi_dlog_proof::legendre_symbol(a, dk.p) * wi_dlog_proof::legendre_symbol(a, dk.q));
    ASSERT(jacobi_symbol(a + ek.n, ek.n) == jacobi_symbol(a, ek.n));
  }
  ASSERT(jacobi_symbol(dk.p * BigInt(3), ek.n) == 0 && wi_dlog_proof::legendre_symbol(dk.p * BigInt(3), dk.p) == -1);
  ASSERT(jacobi_symbol(BigInt(2), BigInt(15)) == 1 && wi_dlog_proof::legendre_symbol(BigInt(2), BigInt(15)) == -1 && jacobi_symbol(BigInt(7), one) == 1);
  ASSERT(wi_dlog_proof::legendre_symbol(BigInt(4), BigInt(7)) == 1 && wi_dlog_proof::legendre_symbol(BigInt(3), BigInt(7)) == -1);
  bool panicked = false, domain = false;
  try { (void)wi_dlog_proof::legendre_symbol(BigInt(3), dk.p + one); } catch (const Panic&) { panicked = true; }      // an even p: mod_inv(2, p).unwrap()
  try { (void)jacobi_symbol(BigInt(3), ek.n + one); } catch (const std::domain_error&) { domain = true; }
  ASSERT(panicked && domain);

  // a square modulus has no h1 of symbol -1; an even one is outside the domain; one per statement, another width; nothing for nothing
  bool no_h1 = false, even = false, refused = false;
  try { (void)DLogStatement::generate_batch_seeded({ek.n, dk.p * dk.p}); } catch (const Panic&) { no_h1 = true; }
  try { (void)DLogStatement::generate_batch_seeded({ek.n + one}); } catch (const Panic&) { even = true; }
  try { (void)DLogStatement::generate_batch_seeded({ek.n, -ek.n}); } catch (const std::invalid_argument&) { refused = true; }
  ASSERT(no_h1 && even && refused);
  auto mixed = DLogStatement::generate_batch_seeded({dk.p, ek.n});          // a 1024-bit modulus in a 2048-bit batch
  ASSERT(jacobi_symbol(mixed.first[0].g, dk.p) == -1 && mixed.first[0].g < dk.p && jacobi_symbol(mixed.first[1].g, ek.n) == -1);
  ASSERT(DLogStatement::generate_batch_seeded({}).first.empty());
}

int main() {
  int failures = 0;
  try { dlog_setup_round_trips(); std::printf("PASS dlog_setup_round_trips\n"); }
  catch (const Panic& e) { std::printf("FAIL dlog_setup_round_trips  [panic: %s]\n", e.what()); failures++; }
  catch (const std::exception& e) { std::printf("FAIL dlog_setup_round_trips  [%s]\n", e.what()); failures++; }
  return failures ? 1 : 0;
}
