// NiCorrectKeyProof::proof_batch (zk-paillier_amd/host/zkproofs.hpp) on zkp_correct_key_ni_prove_batch: over three keys — the fixture key
// of the reference's tests, the same key with its factors swapped, a 1024-bit key of two smaller primes — it equals three proof() calls
// element by element, each result verifies (correct_key_ni.rs:127-137), under the reference's salt and under another one; a malformed key
// panics with its index.  Needs a gfx950 GPU.  Exit code 0 = all passed.
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

static void batch_equals_single_proofs() {
  auto [ek, dk] = test_keypair().keys();
  const DecryptionKey swapped{dk.q, dk.p}, small = small_key();
  const EncryptionKey ek_small{small.p * small.q, (small.p * small.q) * (small.p * small.q)};
  const std::vector<const DecryptionKey*> keys = {&dk, &small, &swapped};
  const EncryptionKey* eks[3] = {&ek, &ek_small, &ek};
  const uint8_t other_salt[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  for (int round = 0; round < 2; round++) {
    const uint8_t* salt = round ? other_salt : SALT_STRING;
    const size_t salt_len = round ? 8 : 4;
    const std::vector<NiCorrectKeyProof> got = NiCorrectKeyProof::proof_batch(keys, salt, salt_len);
    ASSERT(got.size() == 3);
    for (size_t k = 0; k < 3; k++) {
      const NiCorrectKeyProof one = NiCorrectKeyProof::proof(*keys[k], salt, salt_len);
      ASSERT(got[k].sigma_vec.size() == NiCorrectKeyProof::M2 && one.sigma_vec.size() == NiCorrectKeyProof::M2);
      for (size_t i = 0; i < NiCorrectKeyProof::M2; i++) ASSERT(got[k].sigma_vec[i] == one.sigma_vec[i]);
      ASSERT(got[k].verify(*eks[k], salt, salt_len).is_ok());
    }
    ASSERT(!got[0].verify(ek_small, salt, salt_len).is_ok());
  }
  ASSERT(NiCorrectKeyProof::proof_batch({}).empty());
}

static void malformed_key_panics_with_its_index() {
  auto [ek, dk] = test_keypair().keys();
  (void)ek;
  const DecryptionKey same{dk.p, dk.p}, even{dk.p + BigInt::one(), dk.q}, negative{-dk.p, dk.q};
  const DecryptionKey* bad[3] = {&same, &even, &negative};
  for (const DecryptionKey* b : bad) {
    std::string what;
    try { (void)NiCorrectKeyProof::proof_batch({&dk, &dk, b, &dk}); } catch (const Panic& e) { what = e.what(); }
    ASSERT(what.find("key 2 ") != std::string::npos);
  }
}

int main() {
  int failures = 0;
  struct { const char* name; void (*f)(); } tests[] = {{"batch_equals_single_proofs", batch_equals_single_proofs},
                                                       {"malformed_key_panics_with_its_index", malformed_key_panics_with_its_index}};
  for (auto& t : tests) {
    try { t.f(); std::printf("PASS %s\n", t.name); }
    catch (const Panic& e) { std::printf("FAIL %s  [panic: %s]\n", t.name, e.what()); failures++; }
    catch (const std::exception& e) { std::printf("FAIL %s  [%s]\n", t.name, e.what()); failures++; }
  }
  return failures ? 1 : 0;
}
