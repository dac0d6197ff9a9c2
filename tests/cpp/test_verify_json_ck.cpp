// NiCorrectKeyProof::verify_json_batch (zk-paillier_amd/host/zkproofs.hpp): (key, document) pairs in, one Result per pair — GPU verdicts
// for the documents the device reader converts, the host parser + verify_batch for the ones it hands back, a panic for what is no
// document.  Every Result must be verify_batch's on the parsed proof.  Needs a gfx950 GPU.  Exit code 0 = all passed.
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

static std::string replaced(std::string s, const std::string& from, const std::string& to) {
  const size_t at = s.find(from);
  ASSERT(at != std::string::npos);
  return s.replace(at, from.size(), to);
}

// the document of any roots, signed and of any size (serde_json::to_string goes through the fixed-width writer)
static std::string document(const NiCorrectKeyProof& p) {
  std::string s = "{\"sigma_vec\":[";
  for (size_t i = 0; i < p.sigma_vec.size(); i++) s += std::string(i ? "," : "") + "\"" + p.sigma_vec[i].to_str_radix10() + "\"";
  return s + "]}";
}

static bool same(const Result& a, const Result& b) { return a.would_panic() == b.would_panic() && (a.would_panic() || a.is_ok() == b.is_ok()); }

// what the reference computes: from_str, then verify
static Result parsed_verdict(const EncryptionKey& ek, const std::string& doc) {
  NiCorrectKeyProof p = serde_json::correct_key_from_str_host(doc);
  return NiCorrectKeyProof::verify_batch({{&ek, &p}})[0];
}

static void documents_get_the_verdicts_of_their_proofs() {
  auto [ek, dk] = test_keypair().keys();
  const NiCorrectKeyProof proof = NiCorrectKeyProof::proof(dk);
  const std::string honest = serde_json::to_string(proof, ek);
  ASSERT(honest == document(proof));
  std::string tampered = honest;
  const size_t at = tampered.find("\",\"") + 10;                       // a digit of the second root
  tampered[at] = tampered[at] == '4' ? '6' : '4';
  std::string pretty = replaced(honest, "{\"sigma_vec\":[", "{ \"sigma_vec\" : [\n ");
  NiCorrectKeyProof wide = proof;
  wide.sigma_vec[3] = wide.sigma_vec[3] + ek.n * ek.n;                  // the same residue in more digits than the field has: the host path
  const std::string over_wide = document(wide);
  NiCorrectKeyProof neg = proof;
  neg.sigma_vec[0] = neg.sigma_vec[0] - ek.n;                           // a negative root of the same residue
  const std::string negative = document(neg);
  std::vector<std::pair<const EncryptionKey*, std::string>> items = {{&ek, honest}, {&ek, tampered}, {&ek, pretty}, {&ek, over_wide}, {&ek, negative}, {&ek, honest}};
  auto r = NiCorrectKeyProof::verify_json_batch(items);
  ASSERT(r.size() == items.size());
  ASSERT(r[0].is_ok() && r[1].is_err() && r[2].is_ok() && r[3].is_ok() && r[4].is_ok() && r[5].is_ok());
  for (size_t k = 0; k < items.size(); k++) ASSERT(same(r[k], parsed_verdict(ek, items[k].second)));
  ASSERT(NiCorrectKeyProof::verify_json_batch({}).empty());
}

static void documents_that_are_no_proofs_and_other_keys() {
  auto [ek, dk] = test_keypair().keys();
  const std::string honest = serde_json::to_string(NiCorrectKeyProof::proof(dk), ek);
  EncryptionKey other = ek;
  other.n = ek.n + BigInt(2); other.nn = other.n * other.n;
  EncryptionKey even = ek;
  even.n = ek.n + BigInt(1); even.nn = even.n * even.n;
  const std::string ten = honest.substr(0, honest.rfind(",\"")) + "]}";      // ten roots: a valid NiCorrectKeyProof whose verify panics
  std::vector<std::pair<const EncryptionKey*, std::string>> items = {{&ek, honest}, {&ek, "[]"}, {&ek, honest.substr(0, honest.size() - 1)}, {&ek, std::string()},
                                                                     {&other, honest}, {&even, honest}, {&ek, ten}};
  auto r = NiCorrectKeyProof::verify_json_batch(items);
  ASSERT(r[0].is_ok());
  ASSERT(r[1].would_panic() && r[2].would_panic() && r[3].would_panic());
  ASSERT(r[4].is_err() && r[5].is_err());
  for (size_t k : {size_t(0), size_t(4), size_t(5), size_t(6)}) ASSERT(same(r[k], parsed_verdict(*items[k].first, items[k].second)));
  ASSERT(r[6].would_panic());
}

int main() {
  struct T { const char* name; void (*fn)(); } tests[] = {
      {"documents_get_the_verdicts_of_their_proofs", documents_get_the_verdicts_of_their_proofs},
      {"documents_that_are_no_proofs_and_other_keys", documents_that_are_no_proofs_and_other_keys},
  };
  int failed = 0;
  for (auto& t : tests) {
    try { t.fn(); std::printf("PASS %s\n", t.name); }
    catch (const std::exception& e) { std::printf("FAIL %s: %s\n", t.name, e.what()); failed++; }
  }
  return failed ? 1 : 0;
}
