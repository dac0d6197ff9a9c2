// RangeProofNi::verify_json_batch (zk-paillier_amd/host/zkproofs.hpp): documents in, one Result per document — GPU verdicts for the
// documents the device reader converts, the host parser + verify_batch for the ones it hands back, a panic for what is no document.
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

static std::vector<std::string> some_documents(const EncryptionKey& ek, int count, bool honest = true) {
  std::vector<RangeProofNi::Statement> st;
  for (int i = 0; i < count; i++) {
    BigInt range = BigInt::sample(256);
    BigInt r = BigInt::sample_below(ek.n);
    BigInt x = honest ? BigInt::sample_below(range.div_floor(BigInt(3))) : range * BigInt(1000);
    st.push_back({range, Paillier::encrypt_with_chosen_randomness(ek, x, r), x, r});
  }
  return serde_json::to_string_batch(RangeProofNi::prove_batch_seeded(ek, st));
}

static std::string replaced(std::string s, const std::string& from, const std::string& to) {
  const size_t at = s.find(from);
  ASSERT(at != std::string::npos);
  return s.replace(at, from.size(), to);
}

static void documents_get_the_verdicts_of_their_proofs() {
  auto [ek, dk] = test_keypair().keys();
  auto docs = some_documents(ek, 4);
  docs.push_back(some_documents(ek, 1, false)[0]);
  for (const EncryptionKey* key : {(const EncryptionKey*)nullptr, (const EncryptionKey*)&ek}) {
    auto r = RangeProofNi::verify_json_batch(docs, 0, key);
    ASSERT(r.size() == 5);
    for (int i = 0; i < 4; i++) ASSERT(r[i].is_ok());
    ASSERT(r[4].is_err());
  }
  // one digit of one commitment: only that document's verdict changes
  auto tampered = docs;
  const size_t at = tampered[1].find("\"c1\":[\"") + 20;
  tampered[1][at] = tampered[1][at] == '4' ? '6' : '4';
  auto r = RangeProofNi::verify_json_batch(tampered, 0, &ek);
  ASSERT(r[0].is_ok() && r[1].is_err() && r[2].is_ok() && r[3].is_ok() && r[4].is_err());
  ASSERT(RangeProofNi::verify_json_batch({}, 0, &ek).empty());
}

static void documents_the_device_reader_hands_back() {
  auto [ek, dk] = test_keypair().keys();
  auto docs = some_documents(ek, 3);
  std::vector<std::string> v = {
      docs[0],
      replaced(docs[1], "\"range\":", " \"range\" : "),              // white space: the host tokeniser reads it, the GPU verifies it
      replaced(docs[2], "\"masked_r\":\"", "\"masked_r\":\"-"),       // a negative response: a valid RangeProofNi, verified on the host path
      docs[0].substr(0, docs[0].size() - 1),                          // no document
      std::string(),
      replaced(docs[1], "\"error_factor\":128", "\"error_factor\":40"),
  };
  auto r = RangeProofNi::verify_json_batch(v);
  ASSERT(r.size() == v.size());
  ASSERT(r[0].is_ok() && r[1].is_ok());
  RangeProofNi neg = serde_json::range_proof_ni_from_str(v[2]);
  Result want = RangeProofNi::verify_batch(neg.ek, {&neg})[0];
  ASSERT(r[2].would_panic() == want.would_panic() && (want.would_panic() || r[2].is_ok() == want.is_ok()));
  ASSERT(r[3].would_panic() && r[4].would_panic());
  RangeProofNi other = serde_json::range_proof_ni_from_str(v[5]);
  Result want5 = RangeProofNi::verify_batch(other.ek, {&other})[0];
  ASSERT(r[5].would_panic() == want5.would_panic() && (want5.would_panic() || r[5].is_ok() == want5.is_ok()));
  // under another verifier's key every document is verify's assert_eq!(ek)
  EncryptionKey wrong = ek;
  wrong.n = ek.n + BigInt(2); wrong.nn = wrong.n * wrong.n;
  auto w = RangeProofNi::verify_json_batch({docs[0], v[1]}, 0, &wrong);
  ASSERT(w[0].would_panic() && w[1].would_panic());
}

int main() {
  struct T { const char* name; void (*fn)(); } tests[] = {
      {"documents_get_the_verdicts_of_their_proofs", documents_get_the_verdicts_of_their_proofs},
      {"documents_the_device_reader_hands_back", documents_the_device_reader_hands_back},
  };
  int failed = 0;
  for (auto& t : tests) {
    try { t.fn(); std::printf("PASS %s\n", t.name); }
    catch (const std::exception& e) { std::printf("FAIL %s: %s\n", t.name, e.what()); failed++; }
  }
  return failed ? 1 : 0;
}
