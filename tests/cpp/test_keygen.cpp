// Paillier::keypair_batch_seeded, keypair_with_modulus_size, keypair and is_probable_prime_batch (zk-paillier_amd/host/zkproofs.hpp) on
// zkp_paillier_keygen_seeded_batch and zkp_probable_prime_batch: the batch equals the C call's bytes and its chunks; a key fresh from the
// operating system's seed proves correct (NiCorrectKeyProof::proof -> verify, correct_key_ni.rs:127-137) and decrypts what was encrypted
// under it; the prime test says what it must on a handful of known values.  Needs a gfx950 GPU.  Exit code 0 = all passed.
#include <cstdio>
#include <string>

#include "../../zk-paillier_amd/host/zkproofs.hpp"

using namespace zkproofs;

#define ASSERT(c) do { if (!(c)) throw Panic(std::string("assertion failed: ") + #c); } while (0)

static void batch_equals_the_c_call() {
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(7 * i + 3);
  const uint32_t n_bits = 1024, hw = n_bits / 64, kw = n_bits / 32;
  const size_t B = 5;
  const uint64_t first = 77;
  Engine& e = Engine::instance();
  std::vector<uint32_t> p(B * hw), q(B * hw), n(B * kw);
  std::vector<uint8_t> st(B, 9);
  e.check(zkp_paillier_keygen_seeded_batch(e.ctx(), n_bits, B, 5, seed, first, p.data(), q.data(), n.data(), st.data(), 0), "zkp_paillier_keygen_seeded_batch");
  const std::vector<Keypair> keys = Paillier::keypair_batch_seeded(n_bits, B, seed, first);
  ASSERT(keys.size() == B);
  for (size_t b = 0; b < B; b++) {
    ASSERT(st[b] == 0);
    ASSERT(keys[b].p == BigInt::from_limbs(&p[b * hw], hw) && keys[b].q == BigInt::from_limbs(&q[b * hw], hw));
    ASSERT(keys[b].p * keys[b].q == BigInt::from_limbs(&n[b * kw], kw));
    ASSERT(keys[b].p.bit_length() == n_bits / 2 && keys[b].q.bit_length() == n_bits / 2 && !(keys[b].p == keys[b].q));
  }
  const std::vector<Keypair> tail = Paillier::keypair_batch_seeded(n_bits, 2, seed, first + 3);      // a chunk is the same keys
  ASSERT(tail[0].p == keys[3].p && tail[0].q == keys[3].q && tail[1].p == keys[4].p && tail[1].q == keys[4].q);
  ASSERT(Paillier::keypair_batch_seeded(n_bits, 0, seed).empty());
  bool refused = false;
  try { (void)Paillier::keypair_batch_seeded(1536, 1, seed); } catch (const std::exception&) { refused = true; }
  ASSERT(refused);
}

static void fresh_key_proves_correct_and_decrypts() {
  const Keypair kp = Paillier::keypair();
  auto [ek, dk] = kp.keys();
  ASSERT(ek.n.bit_length() == 2048 || ek.n.bit_length() == 2047);
  const Keypair other = Paillier::keypair_with_modulus_size(1024);
  ASSERT(!(other.p == kp.p) && other.p.bit_length() == 512 && other.q.bit_length() == 512);
  const NiCorrectKeyProof proof = NiCorrectKeyProof::proof(dk);
  ASSERT(proof.verify(ek).is_ok());
  ASSERT(!proof.verify(other.keys().first).is_ok());
  const BigInt m = BigInt::from_str_radix10("123456789012345678901234567890123456789");
  const BigInt r = BigInt::sample_below(ek.n);
  const BigInt c = Paillier::encrypt_with_chosen_randomness(ek, m, r);
  ASSERT(Paillier::decrypt(dk, c) == m);
  const auto opened = Paillier::open(dk, c);
  ASSERT(opened.first == m && opened.second == r);
}

static void prime_test_on_known_values() {
  const Keypair kp = Paillier::keypair_with_modulus_size(1024);
  uint8_t seed[32] = {1, 2, 3};
  const std::vector<BigInt> v = {BigInt(0), BigInt(1), BigInt(2), BigInt(6367), BigInt(6369), BigInt::from_str_radix10("170141183460469231731687303715884105727"),
                                 BigInt::from_str_radix10("170141183460469231731687303715884105725"), kp.p, kp.q, kp.p * kp.q, -kp.p};
  const bool want[] = {false, false, true, true, false, true, false, true, true, false, false};
  for (uint32_t rounds : {0u, 5u}) {
    const std::vector<bool> got = is_probable_prime_batch(v, rounds, rounds ? seed : nullptr);
    ASSERT(got.size() == v.size());
    for (size_t i = 0; i < v.size(); i++) ASSERT(got[i] == want[i]);
  }
  ASSERT(is_probable_prime_batch({}).empty());
}

int main() {
  int failures = 0;
  struct { const char* name; void (*f)(); } tests[] = {{"batch_equals_the_c_call", batch_equals_the_c_call},
                                                       {"fresh_key_proves_correct_and_decrypts", fresh_key_proves_correct_and_decrypts},
                                                       {"prime_test_on_known_values", prime_test_on_known_values}};
  for (auto& t : tests) {
    try { t.f(); std::printf("PASS %s\n", t.name); }
    catch (const Panic& e) { std::printf("FAIL %s  [panic: %s]\n", t.name, e.what()); failures++; }
    catch (const std::exception& e) { std::printf("FAIL %s  [%s]\n", t.name, e.what()); failures++; }
  }
  return failures ? 1 : 0;
}
