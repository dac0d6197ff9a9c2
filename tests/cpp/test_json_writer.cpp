// serde_json::to_string_batch and to_string(const RangeProofNi&) (zk-paillier_amd/host/zkproofs.hpp): whole batches of documents written
// on the GPU must equal the loop over the per-document writers, and the whole-document writer must round-trip through
// range_proof_ni_from_str.  Needs a gfx950 GPU.  Exit code 0 = all passed.
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

static std::vector<RangeProofNi> some_proofs(const EncryptionKey& ek, int count) {
  std::vector<RangeProofNi::Statement> st;
  for (int i = 0; i < count; i++) {
    BigInt range = BigInt::sample(256);
    BigInt r = BigInt::sample_below(ek.n);
    BigInt x = BigInt::sample_below(range.div_floor(BigInt(3)));
    st.push_back({range, Paillier::encrypt_with_chosen_randomness(ek, x, r), x, r});
  }
  return RangeProofNi::prove_batch_seeded(ek, st);
}

static void batch_equals_the_loop() {
  auto [ek, dk] = test_keypair().keys();
  auto proofs = some_proofs(ek, 5);
  std::vector<EncryptedPairs> pairs; std::vector<Proof> prs;
  for (auto& p : proofs) { pairs.push_back(p.encrypted_pairs); prs.push_back(p.proof); }
  auto a = serde_json::to_string_batch(pairs, ek);
  auto b = serde_json::to_string_batch(prs, ek);
  ASSERT(a.size() == 5 && b.size() == 5);
  for (size_t i = 0; i < 5; i++) {
    ASSERT(a[i] == serde_json::to_string(pairs[i], ek));
    ASSERT(b[i] == serde_json::to_string(prs[i], ek));
  }
  std::vector<NiCorrectKeyProof> cks;
  for (int i = 0; i < 3; i++) {
    NiCorrectKeyProof ck;
    for (int k = 0; k < ZKP_CORRECT_KEY_M2; k++) ck.sigma_vec.push_back(k == i ? BigInt(0) : BigInt::sample_below(ek.n));
    cks.push_back(ck);
  }
  auto c = serde_json::to_string_batch(cks, ek);
  for (size_t i = 0; i < 3; i++) ASSERT(c[i] == serde_json::to_string(cks[i], ek));
  ASSERT(serde_json::to_string_batch(std::vector<Proof>{}, ek).empty());
}

static void whole_documents_round_trip() {
  auto [ek, dk] = test_keypair().keys();
  auto proofs = some_proofs(ek, 3);
  using serde_json::BigintText;
  for (BigintText kf : {BigintText::Dec, BigintText::Hex, BigintText::Bytes})
    for (BigintText bf : {BigintText::Dec, BigintText::Hex, BigintText::Bytes}) {
      auto docs = serde_json::to_string_batch(proofs, kf, bf);
      ASSERT(docs.size() == 3 && docs[1] == serde_json::to_string(proofs[1], kf, bf));
      for (size_t i = 0; i < 3; i++) {
        RangeProofNi q = serde_json::range_proof_ni_from_str(docs[i], kf, bf);
        ASSERT(q.ek.n == proofs[i].ek.n && q.range == proofs[i].range && q.ciphertext == proofs[i].ciphertext && q.error_factor == proofs[i].error_factor);
        ASSERT(serde_json::to_string(q.encrypted_pairs, ek) == serde_json::to_string(proofs[i].encrypted_pairs, ek));
        ASSERT(serde_json::to_string(q.proof, ek) == serde_json::to_string(proofs[i].proof, ek));
        ASSERT(q.verify(ek, proofs[i].ciphertext).is_ok());
      }
    }
}

int main() {
  int failures = 0;
  struct { const char* name; void (*fn)(); } tests[] = {{"batch_equals_the_loop", batch_equals_the_loop}, {"whole_documents_round_trip", whole_documents_round_trip}};
  for (auto& t : tests) {
    try { t.fn(); std::printf("PASS %s\n", t.name); }
    catch (const Panic& e) { std::printf("FAIL %s  [panic: %s]\n", t.name, e.what()); failures++; }
    catch (const std::exception& e) { std::printf("FAIL %s  [%s]\n", t.name, e.what()); failures++; }
  }
  return failures ? 1 : 0;
}
