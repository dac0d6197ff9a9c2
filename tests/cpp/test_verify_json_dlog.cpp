// CompositeDLogProof::verify_json_batch (zk-paillier_amd/host/zkproofs.hpp): (statement, proof) document pairs in, one Result per pair — GPU
// verdicts for the pairs the device reader converts and finds inside the limb kernels' domain, the host parser + verify() for the ones it
// hands back, a panic for what is no document or fails one of verify's assertions.  Every Result must be what from_str + verify gives for the
// pair alone.  Needs a gfx950 GPU.  Exit code 0 = all passed.
#include <cstdio>
#include <string>

#include "../../zk-paillier_amd/host/zkproofs.hpp"

using namespace zkproofs;
using serde_json::BigintText;

#define ASSERT(c) do { if (!(c)) throw Panic(std::string("assertion failed: ") + #c); } while (0)

static Keypair test_keypair() {   // range_proof_ni.rs:141-145
  return Keypair{
      BigInt::from_str_radix10("148677972634832330983979593310074301486537017973460461278300587514468301043894574906886127642530475786889672304776052879927627556769456140664043088700743909632312483413393134504352834240399191134336344285483935856491230340093391784574980688823380828143810804684752914935441384845195613674104960646037368551517"),
      BigInt::from_str_radix10("158741574437007245654463598139927898730476924736461654463975966787719309357536545869203069369466212089132653564188443272208127277664424448947476335413293018778018615899291704693105620242763173357203898195318179150836424196645745308205164116144020613415407736216097185962171301808761138424668335445923774195463")};
}

// 0 = Ok, 1 = Err, 2 = panic, 3 = unsupported
static int outcome(const Result& r) { return r.would_panic() ? 2 : r.is_unsupported() ? 3 : r.is_ok() ? 0 : 1; }

// what the reference computes for one pair: from_str of both, then verify
static int parsed_outcome(const std::string& st, const std::string& pf, BigintText form) {
  DLogStatement s; CompositeDLogProof p;
  try { s = serde_json::dlog_statement_from_str(st, form); p = serde_json::dlog_proof_from_str(pf, form); } catch (const std::exception&) { return 2; }
  try { return outcome(p.verify(s)); } catch (const Panic&) { return 2; }
}

// wi_dlog_proof.rs:46-65 on the host, for a statement whose g the limb prover does not take (g >= N): mod_pow reduces its base, the hash does not
static CompositeDLogProof prove_on_host(const DLogStatement& st, const BigInt& secret) {
  const BigInt r = BigInt::sample_below(BigInt::pow2(512));
  const BigInt x = mod_pow(st.g.modulus(st.N), r, st.N);
  const BigInt e = detail::compute_digest({&x, &st.g, &st.N, &st.ni});
  return CompositeDLogProof{x, r + e * secret};
}

static void one_pair_of_every_class(BigintText form) {
  auto [ek, dk] = test_keypair().keys();
  const BigInt N = ek.n, one = BigInt::one();
  const BigInt g = BigInt::sample_range(one, N.div_floor(BigInt(4)));                  // (g + N still fits the 2048-bit layout)
  const BigInt secret = BigInt::sample_below(BigInt::pow2(256));
  const BigInt ni = mod_pow(BigInt::mod_inv(g, N), secret, N);
  const DLogStatement st{N, g, ni};
  const CompositeDLogProof pf = CompositeDLogProof::prove(st, secret);
  struct Pair { const char* name; DLogStatement s; CompositeDLogProof p; int want; };
  std::vector<Pair> pairs;
  pairs.push_back({"honest", st, pf, 0});
  pairs.push_back({"tampered x", st, {pf.x + one, pf.y}, 1});
  pairs.push_back({"tampered y", st, {pf.x, pf.y + one}, 1});
  { DLogStatement s{N, g, mod_pow(g, secret, N)}; pairs.push_back({"+secret (:145-168)", s, CompositeDLogProof::prove(s, secret), 1}); }
  { DLogStatement s{N, g, BigInt::sample_range(one, N - one)}; pairs.push_back({"random ni (:172-196)", s, CompositeDLogProof::prove(s, secret), 1}); }
  pairs.push_back({"N <= 2^128", {BigInt::pow2(128) - BigInt(159), BigInt(5), BigInt(7)}, {BigInt(3), BigInt(4)}, 2});
  pairs.push_back({"gcd(g, N) != 1", {N, dk.p, ni}, pf, 2});
  pairs.push_back({"gcd(ni, N) != 1", {N, g, dk.q * BigInt(3)}, pf, 2});
  pairs.push_back({"even N", {N + one, g, ni}, pf, 3});
  pairs.push_back({"g = N", {N, N, ni}, pf, 2});
  pairs.push_back({"ni = N + 1", {N, g, N + one}, pf, 1});
  pairs.push_back({"x = N", st, {N, pf.y}, 1});
  pairs.push_back({"x = 2^2048 - 1", st, {BigInt::pow2(2048) - one, pf.y}, 1});
  pairs.push_back({"over-wide y", st, {pf.x, pf.y + BigInt::pow2(800)}, 1});
  { DLogStatement s{N, g + N, ni}; pairs.push_back({"g + N, proved for it: the reference accepts", s, prove_on_host(s, secret), 0}); }
  pairs.push_back({"g + N, proved for g: another hash", {N, g + N, ni}, pf, 1});
  pairs.push_back({"honest again", st, pf, 0});
  std::vector<std::string> sd, pd;
  for (const Pair& q : pairs) { sd.push_back(serde_json::to_string(q.s, form)); pd.push_back(serde_json::to_string(q.p, form)); }
  // around them: a pretty-printed pair, and documents that are no values of their types
  const size_t n_pairs = pairs.size();
  std::vector<int> want;
  for (const Pair& q : pairs) want.push_back(q.want);
  std::string pretty = sd[0];
  pretty.replace(pretty.find("\"g\""), 3, " \"g\" ");
  sd.push_back(pretty); pd.push_back(pd[0]); want.push_back(0);
  sd.push_back(sd[0].substr(0, sd[0].size() - 1)); pd.push_back(pd[0]); want.push_back(2);
  sd.push_back(sd[0]); pd.push_back("[]"); want.push_back(2);
  sd.push_back(std::string()); pd.push_back(pd[0]); want.push_back(2);
  const auto r = CompositeDLogProof::verify_json_batch(sd, pd, (uint32_t)form);
  ASSERT(r.size() == sd.size());
  for (size_t k = 0; k < r.size(); k++) {
    const int got = outcome(r[k]), alone = parsed_outcome(sd[k], pd[k], form);
    if (got != want[k] || got != alone) {
      std::printf("  pair %zu (%s): batch %d, alone %d, expected %d\n", k, k < n_pairs ? pairs[k].name : "document", got, alone, want[k]);
      ASSERT(got == want[k] && got == alone);
    }
  }
  // the documents are what the reference writes, and from_str reads them back
  ASSERT(serde_json::dlog_statement_from_str(sd[0], form).g == g && serde_json::dlog_proof_from_str(pd[0], form).y == pf.y);
  ASSERT(CompositeDLogProof::verify_json_batch({}, {}, (uint32_t)form).empty());
}

static void decimal_documents() { one_pair_of_every_class(BigintText::Dec); }
static void hex_documents() { one_pair_of_every_class(BigintText::Hex); }
static void byte_array_documents() { one_pair_of_every_class(BigintText::Bytes); }
static void text_forms() {
  const CompositeDLogProof p{BigInt(1234), BigInt(0)};
  ASSERT(serde_json::to_string(p) == "{\"x\":\"1234\",\"y\":\"0\"}");
  ASSERT(serde_json::to_string(p, BigintText::Hex) == "{\"x\":\"04d2\",\"y\":\"00\"}");
  ASSERT(serde_json::to_string(DLogStatement{BigInt(1234), BigInt(5), BigInt(0)}, BigintText::Bytes) == "{\"N\":[4,210],\"g\":[5],\"ni\":[0]}");
}

int main() {
  struct T { const char* name; void (*fn)(); } tests[] = {
      {"text_forms", text_forms},
      {"decimal_documents", decimal_documents},
      {"hex_documents", hex_documents},
      {"byte_array_documents", byte_array_documents},
  };
  int failed = 0;
  for (auto& t : tests) {
    try { t.fn(); std::printf("PASS %s\n", t.name); }
    catch (const std::exception& e) { std::printf("FAIL %s: %s\n", t.name, e.what()); failed++; }
  }
  return failed ? 1 : 0;
}
