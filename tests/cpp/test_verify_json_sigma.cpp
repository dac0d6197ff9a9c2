// ZeroProof / CiphertextProof / VerlinProof / MulProof::verify_json_batch (zk-paillier_amd/host/zkproofs.hpp): (statement, proof) document pairs
// in, one Result per pair — the GPU's verdict for the pairs the device reader converts and finds inside the limb kernels' domain, a panic for
// what is no document, Result::unsupported for a pair outside the domain.  Honest and tampered pairs must get what from_str + verify gives
// for the pair alone.  Needs a gfx950 GPU.  Exit code 0 = all passed.
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
template <class Proof, class Statement> static int parsed_outcome(const std::string& st, const std::string& pf, BigintText kf, BigintText bf) {
  Statement s; Proof p;
  try { s = serde_json::sigma_from_str<Statement>(st, kf, bf); p = serde_json::sigma_from_str<Proof>(pf, kf, bf); } catch (const std::exception&) { return 2; }
  try { return outcome(p.verify(s)); } catch (const Panic&) { return 2; }
}

struct Doc { std::string name, st, pf; int want; bool alone; };      // alone: the single verify() is defined for the pair and must agree

// pairs: honest / tampered (name, statement, proof, expected outcome); outside: pairs outside the domain (unsupported)
template <class Proof, class Statement>
static void run(std::vector<Doc> docs, BigintText kf, BigintText bf) {
  // around them: a pretty-printed statement, and documents that are no values of their types
  std::string pretty = docs[0].st;
  pretty.replace(pretty.find("\"ek\""), 4, " \"ek\" ");
  docs.push_back({"pretty statement", pretty, docs[0].pf, 0, true});
  docs.push_back({"truncated statement", docs[0].st.substr(0, docs[0].st.size() - 1), docs[0].pf, 2, true});
  docs.push_back({"array for a proof", docs[0].st, "[]", 2, true});
  docs.push_back({"empty statement", std::string(), docs[0].pf, 2, true});
  docs.push_back({"key without n", "{\"ek\":{}" + docs[0].st.substr(docs[0].st.find("},") + 1), docs[0].pf, 2, true});
  docs.push_back({"honest again", docs[0].st, docs[0].pf, 0, true});
  std::vector<std::string> sd, pd;
  for (const Doc& d : docs) { sd.push_back(d.st); pd.push_back(d.pf); }
  const auto r = Proof::verify_json_batch(sd, pd, ZKP_BIGINT_FORMS((uint32_t)kf, (uint32_t)bf));
  ASSERT(r.size() == docs.size());
  for (size_t k = 0; k < r.size(); k++) {
    const int got = outcome(r[k]), alone = docs[k].alone ? parsed_outcome<Proof, Statement>(sd[k], pd[k], kf, bf) : got;
    if (got != docs[k].want || got != alone) {
      std::printf("  pair %zu (%s): batch %d, alone %d, expected %d\n", k, docs[k].name.c_str(), got, alone, docs[k].want);
      ASSERT(got == docs[k].want && got == alone);
    }
    if (got == 3) {                                      // looking at it names the reason
      std::string why;
      try { (void)r[k].is_ok(); } catch (const Unsupported& u) { why = u.what(); }
      ASSERT(why.find("outside the domain") != std::string::npos);
    }
  }
  ASSERT(Proof::verify_json_batch({}, {}, 0).empty());
}

template <class T> static std::string text(const T& v, BigintText kf, BigintText bf) { return serde_json::to_string(v, kf, bf); }

static void zero_and_ciphertext(BigintText kf, BigintText bf) {
  auto [ek, dk] = test_keypair().keys();
  const BigInt one = BigInt::one();
  EncryptionKey even = ek; even.n = ek.n + one; even.nn = even.n * even.n;
  {
    const BigInt r = BigInt::sample_below(ek.n);
    const ZeroStatement st{ek, Paillier::encrypt_with_chosen_randomness(ek, BigInt::zero(), r)};
    const ZeroProof pf = ZeroProof::prove(ZeroWitness{r}, st);
    const ZeroStatement st1{ek, Paillier::encrypt_with_chosen_randomness(ek, one, r)};          // test_one_proof, zero_enc_proof.rs:134-155
    auto S = [&](const ZeroStatement& s) { return text(s, kf, bf); };
    auto Q = [&](const ZeroProof& p) { return text(p, kf, bf); };
    // a byte array is the magnitude (curv's to_bytes): the document of -z is the document of z, and the pair is the honest one
    const bool sign = bf != BigintText::Bytes;
    // batches through the GPU writer equal the single documents
    ASSERT(serde_json::to_string_batch(std::vector<ZeroStatement>{st, st1}, kf, bf) == (std::vector<std::string>{S(st), S(st1)}));
    ASSERT(serde_json::to_string_batch(std::vector<ZeroProof>{pf, pf}, kf, bf) == (std::vector<std::string>{Q(pf), Q(pf)}));
    ASSERT(serde_json::sigma_from_str<ZeroProof>(Q(pf), kf, bf).z == pf.z && serde_json::sigma_from_str<ZeroStatement>(S(st), kf, bf).ek.nn == ek.nn);
    run<ZeroProof, ZeroStatement>({{"honest", S(st), Q(pf), 0, true},
                                   {"tampered z", S(st), Q({pf.z + one, pf.a}), 1, true},
                                   {"encrypts one", S(st1), Q(ZeroProof::prove(ZeroWitness{r}, st1)), 1, true},
                                   {"even key", S({even, st.c}), Q(pf), 3, false},
                                   {"c = n^2", S({ek, ek.nn}), Q(pf), 3, false},
                                   {"a = n^2 + a", S(st), Q({pf.z, pf.a + ek.nn}), 3, false},
                                   {"negative z", S(st), Q({BigInt::zero() - pf.z, pf.a}), sign ? 3 : 0, !sign},
                                   {"z of 4097 bits", S(st), Q({BigInt::pow2(4096), pf.a}), 3, false}}, kf, bf);
  }
  {
    const BigInt x = BigInt::sample_below(ek.n), r = BigInt::sample_below(ek.n);
    const CiphertextStatement st{ek, Paillier::encrypt_with_chosen_randomness(ek, x, r)};
    const CiphertextProof pf = CiphertextProof::prove(CiphertextWitness{x, r}, st);
    auto S = [&](const CiphertextStatement& s) { return text(s, kf, bf); };
    auto Q = [&](const CiphertextProof& p) { return text(p, kf, bf); };
    ASSERT(serde_json::to_string_batch(std::vector<CiphertextProof>{pf}, kf, bf) == (std::vector<std::string>{Q(pf)}));
    run<CiphertextProof, CiphertextStatement>({{"honest", S(st), Q(pf), 0, true},
                                               {"tampered z1", S(st), Q({pf.z1 + one, pf.z2, pf.c_prime}), 1, true},
                                               {"wrong witness", S(st), Q(CiphertextProof::prove(CiphertextWitness{x, r + one}, st)), 1, true},
                                               {"z2 = n^2", S(st), Q({pf.z1, ek.nn, pf.c_prime}), 3, false},
                                               {"z1 wider than its array", S(st), Q({BigInt::pow2(2048 + 512), pf.z2, pf.c_prime}), 3, false},
                                               {"key 1", S({EncryptionKey{one, one}, BigInt::zero()}), Q({one, BigInt::zero(), BigInt::zero()}), 3, false}}, kf, bf);
  }
}

static void verlin_and_mul(BigintText kf, BigintText bf) {
  auto [ek, dk] = test_keypair().keys();
  const BigInt one = BigInt::one();
  {
    const BigInt x = BigInt::sample_below(ek.n), xp = BigInt::sample_below(ek.n), xpp = BigInt::sample_below(ek.n), r_x = sample_paillier_random(ek.n);
    const BigInt c = Paillier::encrypt_with_chosen_randomness(ek, x, BigInt::sample_below(ek.n));
    const BigInt cp = Paillier::encrypt_with_chosen_randomness(ek, xp, BigInt::sample_below(ek.n));
    const VerlinStatement st{ek, c, cp, gen_phi(ek, c, cp, x, xp, xpp, r_x)};
    const VerlinStatement bad{ek, c, cp, gen_phi(ek, c, cp, x * BigInt(2), xp, xpp, r_x)};            // verlin_proof.rs:226-236
    const VerlinWitness w{x, xp, xpp, r_x};
    const VerlinProof pf = VerlinProof::prove(w, st);
    auto S = [&](const VerlinStatement& s) { return text(s, kf, bf); };
    auto Q = [&](const VerlinProof& p) { return text(p, kf, bf); };
    ASSERT(serde_json::to_string_batch(std::vector<VerlinStatement>{st, bad}, kf, bf) == (std::vector<std::string>{S(st), S(bad)}));
    ASSERT(serde_json::to_string_batch(std::vector<VerlinProof>{pf}, kf, bf) == (std::vector<std::string>{Q(pf)}));
    run<VerlinProof, VerlinStatement>({{"honest", S(st), Q(pf), 0, true},
                                       {"tampered z_prime", S(st), Q({pf.phi_a, pf.z, pf.z_prime + one, pf.z_double_prime, pf.r_z}), 1, true},
                                       {"x doubled in phi_x", S(bad), Q(VerlinProof::prove(w, bad)), 1, true},
                                       {"phi_x = n^2", S({ek, c, cp, ek.nn}), Q(pf), 3, false},
                                       {"r_z + n^2", S(st), Q({pf.phi_a, pf.z, pf.z_prime, pf.z_double_prime, pf.r_z + ek.nn}), 3, false}}, kf, bf);
  }
  {
    const BigInt a = BigInt::sample_below(ek.n), b = BigInt::sample_below(ek.n), c = (a * b) % ek.n;
    const BigInt r_a = sample_paillier_random(ek.n), r_b = sample_paillier_random(ek.n), r_c = sample_paillier_random(ek.n);
    auto enc = [&](const BigInt& m, const BigInt& r) { return Paillier::encrypt_with_chosen_randomness(ek, m, r); };
    const MulStatement st{ek, enc(a, r_a), enc(b, r_b), enc(c, r_c)};
    const MulStatement bad{ek, st.e_a, st.e_b, enc(c + one, r_c)};                                    // multiplication_proof.rs:232-290
    const MulProof pf = MulProof::prove(MulWitness{a, b, c, r_a, r_b, r_c}, st);
    auto S = [&](const MulStatement& s) { return text(s, kf, bf); };
    auto Q = [&](const MulProof& p) { return text(p, kf, bf); };
    ASSERT(serde_json::to_string_batch(std::vector<MulProof>{pf, pf, pf}, kf, bf) == (std::vector<std::string>{Q(pf), Q(pf), Q(pf)}));
    run<MulProof, MulStatement>({{"honest", S(st), Q(pf), 0, true},
                                 {"tampered f", S(st), Q({pf.f + one, pf.z1, pf.z2, pf.e_d, pf.e_db}), 1, true},
                                 {"c = a b + 1", S(bad), Q(MulProof::prove(MulWitness{a, b, c + one, r_a, r_b, r_c}, bad)), 1, true},
                                 {"no inverse (:135)", S(st), Q({pf.f, pf.z1, pf.z2, pf.e_d, dk.p * BigInt(7)}), 2, true},
                                 {"f = n", S(st), Q({ek.n, pf.z1, pf.z2, pf.e_d, pf.e_db}), 3, false},
                                 {"e_d = n^2", S(st), Q({pf.f, pf.z1, pf.z2, ek.nn, pf.e_db}), 3, false}}, kf, bf);
  }
}

static void text_forms() {
  const EncryptionKey ek{BigInt(1234), BigInt(1234) * BigInt(1234)};
  ASSERT(serde_json::to_string(ZeroStatement{ek, BigInt(5)}) == "{\"ek\":{\"n\":\"1234\"},\"c\":\"5\"}");
  ASSERT(serde_json::to_string(CiphertextStatement{ek, BigInt(5)}, BigintText::Hex, BigintText::Dec) == "{\"ek\":{\"n\":\"04d2\"},\"c\":\"5\"}");
  ASSERT(serde_json::to_string(ZeroProof{BigInt(1234), BigInt(5)}, BigintText::Bytes, BigintText::Bytes) == "{\"z\":[4,210],\"a\":[5]}");
  ASSERT(serde_json::to_string(VerlinProof{BigInt(1), BigInt(2), BigInt(3), BigInt(4), BigInt(5)}) ==
         "{\"phi_a\":\"1\",\"z\":\"2\",\"z_prime\":\"3\",\"z_double_prime\":\"4\",\"r_z\":\"5\"}");
  ASSERT(serde_json::to_string(MulStatement{ek, BigInt(2), BigInt(3), BigInt(4)}) == "{\"ek\":{\"n\":\"1234\"},\"e_a\":\"2\",\"e_b\":\"3\",\"e_c\":\"4\"}");
  ASSERT(serde_json::to_string(MulProof{BigInt(1), BigInt(2), BigInt(3), BigInt(4), BigInt(5)}) == "{\"f\":\"1\",\"z1\":\"2\",\"z2\":\"3\",\"e_d\":\"4\",\"e_db\":\"5\"}");
  ASSERT(serde_json::to_string(CiphertextProof{BigInt(1), BigInt(2), BigInt(3)}) == "{\"z1\":\"1\",\"z2\":\"2\",\"c_prime\":\"3\"}");
}

static void zero_and_ciphertext_decimal() { zero_and_ciphertext(BigintText::Dec, BigintText::Dec); }
static void zero_and_ciphertext_hex_key_byte_arrays() { zero_and_ciphertext(BigintText::Hex, BigintText::Bytes); }
static void verlin_and_mul_decimal() { verlin_and_mul(BigintText::Dec, BigintText::Dec); }
static void verlin_and_mul_hex() { verlin_and_mul(BigintText::Hex, BigintText::Hex); }

int main() {
  struct T { const char* name; void (*fn)(); } tests[] = {
      {"text_forms", text_forms},
      {"zero_and_ciphertext_decimal", zero_and_ciphertext_decimal},
      {"zero_and_ciphertext_hex_key_byte_arrays", zero_and_ciphertext_hex_key_byte_arrays},
      {"verlin_and_mul_decimal", verlin_and_mul_decimal},
      {"verlin_and_mul_hex", verlin_and_mul_hex},
  };
  int failed = 0;
  for (auto& t : tests) {
    try { t.fn(); std::printf("PASS %s\n", t.name); }
    catch (const std::exception& e) { std::printf("FAIL %s: %s\n", t.name, e.what()); failed++; }
  }
  return failed ? 1 : 0;
}
