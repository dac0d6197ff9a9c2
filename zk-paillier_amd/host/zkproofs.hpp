// zkproofs.hpp — C++ host mirror of the reference's proof API for the hot path, on top of the C
// ABI of include/zkp_hip.h.  (The reference is Rust; there is no Rust toolchain in this image, so
// the host side above the C ABI is C++ — same type and method names, argument meaning and error
// behaviour as the reference, so that tests read like the reference's own tests.)
//
//   reference                                                      here
//   zkproofs::RangeProofNi::{prove,verify,verify_self}              RangeProofNi::{prove,verify,verify_self}   (+ *_batch)
//   zkproofs::{MulProof, CorrectMessageProof}::{prove,verify}, BigInt::mod_inv    MulProof, CorrectMessageProof, mod_inv_batch
//   zkproofs::RangeProof::{verifier_commit,verify_commit,generate_encrypted_pairs,generate_proof,verifier_output}   RangeProof::*
//     src/zkproofs/range_proof_ni.rs:36-128
//   zkproofs::NiCorrectKeyProof::{proof,verify}                     NiCorrectKeyProof::{proof,verify}   (+ proof_batch, verify_batch)
//     src/zkproofs/correct_key_ni.rs:36-100
//   zkproofs::{CompositeDLogProof,DLogStatement}::{prove,verify}    same (+ DLogStatement::generate_batch_seeded)
//     src/zkproofs/wi_dlog_proof.rs:33-91
//   zkproofs::wi_dlog_proof::legendre_symbol (:94-107)              wi_dlog_proof::legendre_symbol, wi_dlog_proof::jacobi_symbol
//   zkproofs::{CorrectKey,Challenge,VerificationAid,CorrectKeyProof} same (interactive, correct_key.rs:28-183)
//   zkproofs::{VerlinProof,VerlinStatement,VerlinWitness}, gen_phi   same (verlin_proof.rs:35-165)
//   zkproofs::{ZeroProof,ZeroStatement,ZeroWitness}                 same (zero_enc_proof.rs:26-95)
//   zkproofs::{CiphertextProof,CiphertextStatement,CiphertextWitness} same (correct_ciphertext.rs:23-98)
//   paillier::{Keypair,EncryptionKey,DecryptionKey,Paillier}        same names, only what the path needs
//   zkproofs::IncorrectProof (errors.rs:5-13)                       Result<> with is_ok()/is_err()/expect()
//
// Rust panics (assert_eq!, index out of bounds, .expect on Err) become C++ exceptions (Panic).
// Every modular exponentiation runs on the GPU; this layer only samples, hashes small transcripts
// (NiCorrectKeyProof::proof's MGF), converts BigInt <-> limbs and flattens proofs into batches (the layouts: range_batch.hpp; their
// memory: staging.hpp).
#pragma once
#include <sys/mman.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/zkp_hip.h"
#include "bigint.hpp"
#include "range_batch.hpp"
#include "staging.hpp"

namespace zkproofs {

struct Panic : std::runtime_error { using std::runtime_error::runtime_error; };
struct IncorrectProof {};   // src/zkproofs/errors.rs:5-13

// Result<(), IncorrectProof>.  A batch call returns one Result per proof; a proof on which the reference would have
// PANICKED (index out of bounds, assert) carries that panic and throws it when it is looked at, so that one crafted proof
// cannot take the verdicts of the others with it.
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };
class Result {
  enum State { Ok, Err, Panicked, Unsupp } st_;
  std::string what_;
  void look() const { if (st_ == Panicked) throw Panic(what_); if (st_ == Unsupp) throw Unsupported(what_); }
 public:
  explicit Result(bool ok) : st_(ok ? Ok : Err) {}
  static Result panicked(const std::string& what) { Result r(false); r.st_ = Panicked; r.what_ = what; return r; }
  // the ONLY outcome that is not the reference's: a statement this fixed-width engine cannot carry at all (a key that is not a
  // positive odd integer of at most 4096 bits).  Every other input — any size, either sign — gets the reference's verdict or panic.
  static Result unsupported(const std::string& what) { Result r(false); r.st_ = Unsupp; r.what_ = what; return r; }
  bool would_panic() const { return st_ == Panicked; }
  bool is_unsupported() const { return st_ == Unsupp; }
  bool is_ok() const { look(); return st_ == Ok; }
  bool is_err() const { look(); return st_ == Err; }
  void expect(const char* msg) const { look(); if (st_ != Ok) throw Panic(std::string(msg) + ": IncorrectProof"); }
};

// ------------------------------------------------------------------ engine (one ctx per device)
class Engine {
  zkp_ctx* ctx_ = nullptr;
 public:
  explicit Engine(int device = 0) {
    if (zkp_ctx_create(device, &ctx_) != ZKP_OK) throw std::runtime_error("zkp_ctx_create failed: no gfx950 GPU (there is no CPU fallback)");
  }
  ~Engine() { if (ctx_) zkp_ctx_destroy(ctx_); }
  Engine(const Engine&) = delete;
  zkp_ctx* ctx() const { return ctx_; }
  void check(int32_t st, const char* what) const {
    if (st != ZKP_OK) throw std::runtime_error(std::string(what) + " failed (status " + std::to_string(st) + "): " + zkp_last_error_string(ctx_));
  }
  static Engine& instance() { static Engine e(0); return e; }
};

// ------------------------------------------------------------------ host-side parallelism and timing of the batch calls
// The reference spreads a proof's rows over a rayon pool (range_proof.rs:136-187); here the per-proof HOST work of a batch call —
// sampling 4 x 128 values, BigInt <-> limb conversion, rebuilding the proof objects — runs on a few threads (ZKP_HOST_THREADS,
// default min(16, hardware threads)) around the one GPU call.  last_host_timing(): where the time of the most recent
// RangeProofNi::{prove,verify}_batch went (bench.py's host_api leg prints it next to the GPU step).
struct HostTiming { double sample_flatten_ms = 0, gpu_ms = 0, rebuild_ms = 0, general_ms = 0; size_t proofs = 0, general_proofs = 0; unsigned threads = 1; };
inline HostTiming& last_host_timing() { static HostTiming t; return t; }
inline unsigned host_threads() {
  static const unsigned n = [] {
    const char* e = std::getenv("ZKP_HOST_THREADS");
    unsigned v = e ? (unsigned)std::atoi(e) : std::min(16u, std::thread::hardware_concurrency());
    return std::max(1u, std::min(v, 64u));
  }();
  return n;
}
template <class F> inline void parallel_for(size_t count, F body, unsigned max_threads = ~0u) {
  const size_t T = std::min<size_t>(std::min(host_threads(), max_threads), count);
  if (T <= 1) { for (size_t i = 0; i < count; i++) body(i); return; }
  std::exception_ptr first;
  std::mutex mu;
  std::vector<std::thread> th;
  for (size_t t = 0; t < T; t++)
    th.emplace_back([&, t] {
      try { for (size_t i = count * t / T; i < count * (t + 1) / T; i++) body(i); }
      catch (...) { std::lock_guard<std::mutex> g(mu); if (!first) first = std::current_exception(); }
    });
  for (auto& x : th) x.join();
  if (first) std::rethrow_exception(first);
}
// (RawBuf, StagingPool: host/staging.hpp)
struct StopWatch {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double lap() { const auto t1 = std::chrono::steady_clock::now(); const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count(); t0 = t1; return ms; }
};

// kernel width (bits) for an n of the given size
inline uint32_t width_for(const BigInt& n) {
  const size_t b = n.bit_length();
  if (b <= 1024) return 1024;
  if (b <= 2048) return 2048;
  if (b <= 4096) return 4096;
  throw std::length_error("modulus wider than 4096 bits");
}

// ------------------------------------------------------------------ Paillier key types
struct EncryptionKey {
  BigInt n, nn;
  friend bool operator==(const EncryptionKey& a, const EncryptionKey& b) { return a.n == b.n && a.nn == b.nn; }
};
struct DecryptionKey { BigInt p, q; };
struct Keypair {
  BigInt p, q;
  // [upstream paillier::Keypair::keys]: ek = {n, nn = n^2}, dk = {p, q}
  std::pair<EncryptionKey, DecryptionKey> keys() const { BigInt n = p * q; return {EncryptionKey{n, n * n}, DecryptionKey{p, q}}; }
};

struct Paillier {
  // [upstream kzen-paillier EncryptWithChosenRandomness] on ANY integers m, r (a received proof may hold negative or over-wide
  // fields), exactly as the reference's operators give it:
  //     rn = mod_pow(r, n, nn) in [0, nn);   gm = (m n + 1) % nn  (truncated: negative for m < 0);   c = gm rn % nn
  // With E = Enc(m mod n, r mod n) — floored residues, the canonical operands the kernels take — that is  c = E  for m >= 0 and
  // c = E - nn (or 0 when E = 0) for m < 0: (m n + 1) % nn = -(nn - G) with G = 1 + (m mod n) n, hence c = -((nn - G) rn mod nn).
  // ONE zkp_paillier_enc_batch for the whole list.
  static std::vector<BigInt> encrypt_with_chosen_randomness_batch(const EncryptionKey& ek, const std::vector<std::pair<const BigInt*, const BigInt*>>& mr) {
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t cnt = mr.size();
    std::vector<uint32_t> n(kw), mm(cnt * kw), rr(cnt * kw), c(cnt * 2 * kw);
    ek.n.to_limbs(n.data(), kw);
    for (size_t i = 0; i < cnt; i++) {
      const BigInt &m = *mr[i].first, &r = *mr[i].second;
      (m.fits_limbs(kw) && m < ek.n ? m : m.modulus(ek.n)).to_limbs(&mm[i * kw], kw);
      (r.fits_limbs(kw) && r < ek.n ? r : r.modulus(ek.n)).to_limbs(&rr[i * kw], kw);
    }
    if (cnt) e.check(zkp_paillier_enc_batch(e.ctx(), nb, cnt, n.data(), 0, mm.data(), rr.data(), c.data(), 0), "zkp_paillier_enc_batch");
    std::vector<BigInt> out;
    out.reserve(cnt);
    for (size_t i = 0; i < cnt; i++) {
      BigInt E = BigInt::from_limbs(&c[i * 2 * kw], 2 * kw);
      out.push_back(mr[i].first->is_negative() && !E.is_zero() ? E - ek.nn : E);
    }
    return out;
  }
  static BigInt encrypt_with_chosen_randomness(const EncryptionKey& ek, const BigInt& m, const BigInt& r) {
    return encrypt_with_chosen_randomness_batch(ek, {{&m, &r}})[0];
  }

  // [upstream kzen-paillier Decrypt / Open] with the factors, by the CRT formulas of zkp_paillier_open_batch (include/zkp_hip.h): ONE GPU call
  // for the whole list.  `malformed` is that call's ZKP_VERDICT_MALFORMED — a key with gcd(n, phi(n)) != 1 or an even or trivial factor, a
  // ciphertext that shares a factor with n — where the reference returns a number that means nothing; m and r are zero then.
  // What the fixed layout cannot carry: a ciphertext that is negative or not below 2^(2 n_bits) is REDUCED on the host to its floored residue
  // modulo n^2, as encrypt_with_chosen_randomness_batch reduces its operands (m and r depend on c mod n^2 only); a key wider than 4096 bits
  // throws std::length_error, as it does there; a factor that is not positive makes every item malformed.
  struct Opened { BigInt m, r; bool malformed = false; };
  static std::vector<Opened> open_batch(const DecryptionKey& dk, const std::vector<BigInt>& cs) { return open_impl(dk, cs, true); }
  static std::vector<Opened> decrypt_batch(const DecryptionKey& dk, const std::vector<BigInt>& cs) { return open_impl(dk, cs, false); }   // (r stays zero)
  static BigInt decrypt(const DecryptionKey& dk, const BigInt& c) {
    Opened o = decrypt_batch(dk, {c})[0];
    if (o.malformed) throw Panic("Paillier::decrypt: the key or the ciphertext is outside the domain (ZKP_VERDICT_MALFORMED)");
    return o.m;
  }
  static std::pair<BigInt, BigInt> open(const DecryptionKey& dk, const BigInt& c) {
    Opened o = open_batch(dk, {c})[0];
    if (o.malformed) throw Panic("Paillier::open: the key or the ciphertext is outside the domain (ZKP_VERDICT_MALFORMED)");
    return {o.m, o.r};
  }
  // [upstream kzen-paillier KeyGeneration] by the published rule of zkp_paillier_keygen_seeded_batch (include/zkp_hip.h): key b comes from
  // (seed, first_index + b), its primes are found on the GPU, ONE call for the whole list.  n_bits in {1024, 2048, 4096}; `seed` is 32
  // bytes and worth every key made from it: one (seed, index) pair serves one key, and the caller wipes the seed.  A key the call reports
  // ZKP_VERDICT_MALFORMED (a search that used up its attempts, p == q) throws Panic.  The limb copies of the factors are wiped.
  static std::vector<Keypair> keypair_batch_seeded(uint32_t n_bits, size_t count, const uint8_t* seed, uint64_t first_index = 0, uint32_t rounds = 5) {
    Engine& e = Engine::instance();
    const size_t hw = n_bits / 64;
    std::vector<uint32_t> p(count * hw), q(count * hw);
    std::vector<uint8_t> st(count);
    const int32_t rc = zkp_paillier_keygen_seeded_batch(e.ctx(), n_bits, count, rounds, seed, first_index, p.data(), q.data(), nullptr, st.data(), 0);
    std::vector<Keypair> out;
    if (rc == ZKP_OK) {
      out.reserve(count);
      for (size_t b = 0; b < count; b++) out.push_back(Keypair{BigInt::from_limbs(&p[b * hw], hw), BigInt::from_limbs(&q[b * hw], hw)});
    }
    detail::ChaChaRng::wipe(p.data(), p.size() * 4);
    detail::ChaChaRng::wipe(q.data(), q.size() * 4);
    e.check(rc, "zkp_paillier_keygen_seeded_batch");
    for (size_t b = 0; b < count; b++)
      if (st[b] != 0) throw Panic("Paillier::keypair_batch_seeded: key " + std::to_string(b) + " is malformed (ZKP_VERDICT_MALFORMED)");
    return out;
  }
  // [upstream Paillier::keypair_with_modulus_size / Paillier::keypair (2048)]: a seed fresh from the operating system, one key, the seed wiped
  static Keypair keypair_with_modulus_size(uint32_t n_bits) {
    struct Seed {
      uint8_t bytes[32];
      Seed() { detail::ChaChaRng::os_random(bytes, sizeof bytes); }
      ~Seed() { detail::ChaChaRng::wipe(bytes, sizeof bytes); }
    } seed;
    return keypair_batch_seeded(n_bits, 1, seed.bytes)[0];
  }
  static Keypair keypair() { return keypair_with_modulus_size(2048); }

  // CorrectOpening::verify_opening (correct_opening.rs:17-30): `encrypt_with_chosen_randomness(ek, m, r) == c`
  static bool verify_opening(const EncryptionKey& ek, const BigInt& m, const BigInt& r, const BigInt& c) {
    return encrypt_with_chosen_randomness(ek, m, r) == c;
  }

 private:
  static std::vector<Opened> open_impl(const DecryptionKey& dk, const std::vector<BigInt>& cs, bool with_r) {
    const size_t cnt = cs.size();
    std::vector<Opened> out(cnt);
    if (dk.p.is_negative() || dk.q.is_negative() || dk.p.is_zero() || dk.q.is_zero()) { for (Opened& o : out) o.malformed = true; return out; }
    const BigInt n = dk.p * dk.q, nn = n * n;
    uint32_t nb = width_for(n);
    while (nb < 4096 && std::max(dk.p.bit_length(), dk.q.bit_length()) > nb / 2) nb *= 2;       // (an unbalanced key: both factors in hw words)
    if (std::max(dk.p.bit_length(), dk.q.bit_length()) > nb / 2) throw std::length_error("factor wider than 2048 bits");
    const uint32_t kw = nb / 32, hw = nb / 64;
    if (cnt == 0) return out;
    Engine& e = Engine::instance();
    std::vector<uint32_t> p(hw), q(hw), c(cnt * 2 * kw), m(cnt * kw), r(with_r ? cnt * kw : 0);
    std::vector<uint8_t> st(cnt);
    dk.p.to_limbs(p.data(), hw); dk.q.to_limbs(q.data(), hw);
    for (size_t i = 0; i < cnt; i++) (!cs[i].is_negative() && cs[i].fits_limbs(2 * kw) ? cs[i] : cs[i].modulus(nn)).to_limbs(&c[i * 2 * kw], 2 * kw);
    const int32_t rc = zkp_paillier_open_batch(e.ctx(), nb, cnt, p.data(), q.data(), 0, c.data(), m.data(), with_r ? r.data() : nullptr, st.data(), 0);
    volatile uint32_t* wp = p.data(); volatile uint32_t* wq = q.data();
    for (uint32_t w = 0; w < hw; w++) { wp[w] = 0; wq[w] = 0; }                                 // the factors' limb copies
    e.check(rc, "zkp_paillier_open_batch");
    for (size_t i = 0; i < cnt; i++) {
      out[i].malformed = st[i] != 0;
      out[i].m = BigInt::from_limbs(&m[i * kw], kw);
      if (with_r) out[i].r = BigInt::from_limbs(&r[i * kw], kw);
    }
    return out;
  }
};

inline BigInt mod_pow(const BigInt& base, const BigInt& exp, const BigInt& modulus) {
  Engine& e = Engine::instance();
  const size_t b = modulus.bit_length();
  const uint32_t mb = b <= 2048 ? 2048 : b <= 4096 ? 4096 : 8192, L = mb / 32;
  if (exp.bit_length() > mb) throw std::length_error("exponent wider than the modulus width");
  std::vector<uint32_t> bb(L), ee(L), mm(L), out(L);
  base.modulus(modulus).to_limbs(bb.data(), L); exp.to_limbs(ee.data(), L); modulus.to_limbs(mm.data(), L);   // mpz_powm: a negative base gives the residue in [0, m)
  e.check(zkp_modexp_batch(e.ctx(), mb, mb, 1, bb.data(), ee.data(), L, mm.data(), L, out.data(), 0), "zkp_modexp_batch");
  return BigInt::from_limbs(out.data(), L);
}

// is_probable_prime of zkp_probable_prime_batch (include/zkp_hip.h) for a list of non-negative integers of at most 2048 bits: trial division by
// the odd primes below 6370, the strong test to base 2 and `rounds` (<= 64) strong tests to bases drawn from (seed, first_index + i); seed
// (32 bytes) may be null when rounds == 0.  ONE GPU call at the narrowest width that carries every value.  A negative value is not prime.
inline std::vector<bool> is_probable_prime_batch(const std::vector<BigInt>& values, uint32_t rounds = 0, const uint8_t* seed = nullptr, uint64_t first_index = 0) {
  Engine& e = Engine::instance();
  const size_t cnt = values.size();
  size_t widest = 0;
  for (const BigInt& v : values) if (!v.is_negative()) widest = std::max(widest, v.bit_length());
  if (widest > 2048) throw std::length_error("is_probable_prime_batch: value wider than 2048 bits");
  const uint32_t bits = widest <= 512 ? 512 : widest <= 1024 ? 1024 : 2048, pw = bits / 32;
  std::vector<uint32_t> w(cnt * pw);               // (zero: a negative value is tested as 0)
  std::vector<uint8_t> verdict(cnt);
  for (size_t i = 0; i < cnt; i++) if (!values[i].is_negative()) values[i].to_limbs(&w[i * pw], pw);
  const int32_t rc = cnt ? zkp_probable_prime_batch(e.ctx(), bits, cnt, w.data(), rounds, seed, first_index, verdict.data(), 0) : ZKP_OK;
  detail::ChaChaRng::wipe(w.data(), w.size() * 4);
  e.check(rc, "zkp_probable_prime_batch");
  std::vector<bool> out(cnt);
  for (size_t i = 0; i < cnt; i++) out[i] = verdict[i] == 1;
  return out;
}

// batched BigInt::mod_pow over one modulus: out[i] = bases[i]^exps[i or 0] mod modulus (ONE zkp_modexp_batch)
inline std::vector<BigInt> mod_pow_batch(const std::vector<BigInt>& bases, const std::vector<BigInt>& exps, const BigInt& modulus) {
  Engine& e = Engine::instance();
  const size_t b = modulus.bit_length(), cnt = bases.size();
  const uint32_t mb = b <= 2048 ? 2048 : b <= 4096 ? 4096 : 8192, L = mb / 32;
  const bool shared = exps.size() == 1;
  if (!shared && exps.size() != cnt) throw std::invalid_argument("mod_pow_batch: exps must have 1 or bases.size() entries");
  std::vector<uint32_t> bb(cnt * L), ee(exps.size() * L), mm(L), out(cnt * L);
  for (size_t i = 0; i < cnt; i++) bases[i].modulus(modulus).to_limbs(&bb[i * L], L);
  for (size_t i = 0; i < exps.size(); i++) exps[i].to_limbs(&ee[i * L], L);
  modulus.to_limbs(mm.data(), L);
  if (cnt) e.check(zkp_modexp_batch(e.ctx(), mb, mb, cnt, bb.data(), ee.data(), shared ? 0 : L, mm.data(), 0, out.data(), 0), "zkp_modexp_batch");
  std::vector<BigInt> r;
  for (size_t i = 0; i < cnt; i++) r.push_back(BigInt::from_limbs(&out[i * L], L));
  return r;
}

// ------------------------------------------------------------------ host SHA-256 (NiCorrectKeyProof::proof's MGF; the challenge of a RangeProofNi whose transcript holds over-wide values)
namespace detail {
struct Sha256 {
  uint32_t h[8]; uint8_t buf[64]; uint64_t len = 0; size_t fill = 0;
  static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  Sha256() { static const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19}; std::memcpy(h, iv, 32); }
  void block(const uint8_t* p) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10));
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  void update(const uint8_t* p, size_t n) {
    len += n;
    while (n) { size_t k = std::min(n, 64 - fill); std::memcpy(buf + fill, p, k); fill += k; p += k; n -= k; if (fill == 64) { block(buf); fill = 0; } }
  }
  void update(const BigInt& v) { auto b = v.to_bytes(); update(b.data(), b.size()); }
  BigInt finish() {
    uint64_t bits = len * 8; uint8_t pad = 0x80; update(&pad, 1); pad = 0;
    while (fill != 56) update(&pad, 1);
    uint8_t lb[8]; for (int i = 0; i < 8; i++) lb[i] = (uint8_t)(bits >> (56 - 8 * i));
    update(lb, 8);
    uint8_t out[32]; for (int i = 0; i < 8; i++) { out[4 * i] = h[i] >> 24; out[4 * i + 1] = h[i] >> 16; out[4 * i + 2] = h[i] >> 8; out[4 * i + 3] = h[i]; }
    return BigInt::from_bytes(out, 32);
  }
};
// src/zkproofs/utils.rs:9-22
inline BigInt compute_digest(std::initializer_list<const BigInt*> items) { Sha256 s; for (auto* v : items) s.update(*v); return s.finish(); }
}  // namespace detail

// ------------------------------------------------------------------ RangeProofNi
// (Response, EncryptedPairs, Proof and the batch layout they are flattened into: host/range_batch.hpp)
class RangeProofNi {
 public:
  static constexpr size_t SECURITY_PARAMETER = ZKP_SECURITY_PARAMETER;   // range_proof_ni.rs:23
  EncryptionKey ek;
  BigInt range, ciphertext;
  EncryptedPairs encrypted_pairs;
  Proof proof;
  size_t error_factor = SECURITY_PARAMETER;

  struct Statement { BigInt range, ciphertext, secret_x, secret_r; };

  // range_proof_ni.rs:47-82 for many provers sharing one key; randomness sampled as range_proof.rs:133-159.
  // ONE GPU call per batch.  (Rounds 3 - 4 ran a pipeline of 4 chunks to hide the rebuild of the proof objects behind the next chunk's
  // call — and paid a launch tail and a copy per chunk for it: 2022 ms of GPU calls against 1794 ms for one call at B = 4096, measured
  // on one box; measured again before the chunked path was removed: profiles/host_layer/ab.jsonl.)  What made the rebuild expensive was
  // never the copying of 0.8 GB of limbs but the first touch of the heap they go to (3 million small allocations, a quarter of a million
  // page faults): so the proof objects are ALLOCATED AND TOUCHED WHILE THE GPU WORKS (`prealloc`: every BigInt of every proof at its full
  // capacity, on a few helper threads under the blocking call), and after the call the rebuild only copies limbs into memory that is
  // already there, on all threads.
  //
  // The staging of a finished LARGE call (2.2 GB at B = 4096) goes back to the pool / the OS on a thread of its own: unmapping it is tens
  // of milliseconds that the caller need not wait for.  Small calls (nothing pooled: a single proof is a batch of one) free theirs inline
  // — no thread per call.  Secret blocks are wiped by the CALLER before this (RangeWitness::wipe_secrets), never only in the background:
  // a process that exits right after the call must not leave witnesses behind.
  template <class Staging> static void release_later(std::unique_ptr<Staging> held, bool large) {
    if (!large) return;                                                                                       // (freed here, by `held` going out of scope)
    try { std::thread([h = std::move(held)]() mutable { h.reset(); }).detach(); } catch (...) {}              // (no thread: freed here as well)
  }
  static std::vector<RangeProofNi> prove_batch(const EncryptionKey& ek, const std::vector<Statement>& st) { return prove_batch_impl(ek, st, false); }
  // The same from what the reference's prove takes — statement and secret, nothing else: a fresh 32-byte seed from the operating system per
  // call, expanded into (w1, w2, r1, r2) ON THE GPU (zkp_range_ni_prove_seeded_batch; the stream is defined in include/zkp_hip.h).  No
  // witness is sampled, flattened, uploaded or kept on the host: HostTiming.sample_flatten_ms covers the flattening of the statements only.
  static std::vector<RangeProofNi> prove_batch_seeded(const EncryptionKey& ek, const std::vector<Statement>& st) { return prove_batch_impl(ek, st, true); }
  struct SeedGuard {      // the seed is worth the whole witness: wiped on every path out of the call
    uint8_t bytes[32];
    explicit SeedGuard(bool draw) { if (draw) detail::ChaChaRng::os_random(bytes, sizeof bytes); else std::memset(bytes, 0, sizeof bytes); }
    ~SeedGuard() { detail::ChaChaRng::wipe(bytes, sizeof bytes); }
  };
  static std::vector<RangeProofNi> prove_batch_impl(const EncryptionKey& ek, const std::vector<Statement>& st, bool seeded) {
    Engine& e = Engine::instance();
    SeedGuard seed(seeded);
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t B = st.size(), EF = SECURITY_PARAMETER;
    RawBuf<uint32_t> n(kw);
    ek.n.to_limbs(n.data(), kw);
    HostTiming& tm = last_host_timing();
    tm = HostTiming(); tm.proofs = B; tm.threads = host_threads();
    std::vector<RangeProofNi> out(B);
    struct Staging {
      RangeSlab proofs; RangeWitness witness;
      Staging(size_t B, size_t EF, size_t kw, bool nonces) : proofs(B, EF, kw, RangeSlab::ALL), witness(B, EF, kw, true, nonces) {}
    };
    StopWatch sw;
    std::unique_ptr<Staging> sg(new Staging(B, EF, kw, !seeded));
    RangeSlab& s = sg->proofs;
    RangeWitness& w = sg->witness;
    std::vector<uint8_t> status(B);

    // stage A: sample (range_proof.rs:133-159) and flatten the statements
    parallel_for(B, [&](size_t b) {
      s.put_statement(b, st[b].range, st[b].ciphertext);
      w.put_secret(b, st[b].secret_x, st[b].secret_r);
      if (seeded) return;
      const BigInt third = st[b].range.div_floor(BigInt(3)), two_thirds = BigInt(2) * third;   // range_proof.rs:133-134
      for (size_t i = 0; i < EF; i++) {
        BigInt a = BigInt::sample_range(third, two_thirds), cc = a - third;                     // :136-141
        if (BigInt::coin()) std::swap(a, cc);                                                    // :144-149
        const BigInt r1 = BigInt::sample_below(ek.n), r2 = BigInt::sample_below(ek.n);          // :151-159
        w.put_nonces(b * EF + i, a, cc, r1, r2);
      }
    });
    tm.sample_flatten_ms = sw.lap();
    // stage C1, under the GPU call: the proof objects at their final shape — every BigInt allocated at full capacity and zero-filled (the
    // first touch of its pages).  Which rows will be Open and which Mask is not known yet: every row gets the four fields of an Open
    // response; RangeSlab::read_response moves two of them over for a Mask row and lets the other two go.
    // (more than a few threads only contend for the address space: measured round 4, 16 threads 674 ms against one 377 ms)
    auto prealloc = [&] {
      parallel_for(B, [&](size_t b) {
        RangeProofNi& o = out[b];
        o.ek = ek; o.range = st[b].range; o.ciphertext = st[b].ciphertext; o.error_factor = EF;
        o.encrypted_pairs.c1.resize(EF); o.encrypted_pairs.c2.resize(EF); o.proof.responses.resize(EF);
        for (size_t i = 0; i < EF; i++) {
          o.encrypted_pairs.c1[i].l.resize(2 * kw); o.encrypted_pairs.c2[i].l.resize(2 * kw);
          Response& rs = o.proof.responses[i];
          rs.w1.l.resize(kw); rs.r1.l.resize(kw); rs.w2.l.resize(kw); rs.r2.l.resize(kw);
        }
      }, std::max(1u, std::min(4u, host_threads() / 2)));
    };
    std::exception_ptr helper_error;
    std::thread helper([&] { try { prealloc(); } catch (...) { helper_error = std::current_exception(); } });
    // stage B: the 256 Enc per proof, challenges and responses on the GPU (blocking: host buffers)
    StopWatch g;
    try {
      zkp_range_ni_proofs p = s.abi(nb, n.data(), 0);
      if (seeded) e.check(zkp_range_ni_prove_seeded_batch(e.ctx(), &p, w.x(), w.r(), seed.bytes, 0, nullptr, nullptr, status.data(), 0), "zkp_range_ni_prove_seeded_batch");
      else {
        zkp_range_ni_witness wt = w.abi();
        e.check(zkp_range_ni_prove_batch(e.ctx(), &p, &wt, nullptr, nullptr, status.data(), 0), "zkp_range_ni_prove_batch");
      }
    } catch (...) { helper.join(); throw; }
    tm.gpu_ms = g.lap();
    helper.join();
    if (helper_error) std::rethrow_exception(helper_error);
    // stage C2, after the call: limbs into the memory that is already there (no allocation, no page fault: a copy at memory bandwidth)
    sw.lap();
    parallel_for(B, [&](size_t b) {
      if (status[b] != 0) throw Panic("RangeProofNi::prove: malformed (the reference would panic)");
      RangeProofNi& o = out[b];
      for (size_t i = 0; i < EF; i++) {             // row by row, in the order prealloc laid the heap out
        s.read_pair(b * EF + i, o.encrypted_pairs.c1[i], o.encrypted_pairs.c2[i]);
        s.read_response(b * EF + i, o.proof.responses[i]);
      }
    });
    tm.rebuild_ms = sw.lap();
    w.wipe_secrets();                                   // witnesses and nonces: gone before this call returns
    const bool large = s.large();
    release_later(std::move(sg), large);
    return out;
  }
  static RangeProofNi prove(const EncryptionKey& ek, const BigInt& range, const BigInt& ciphertext, const BigInt& secret_x, const BigInt& secret_r) {
    return prove_batch(ek, {Statement{range, ciphertext, secret_x, secret_r}})[0];
  }

  // verify_self for many proofs sharing one key (range_proof_ni.rs:109-128).  Every field of a received proof is prover-chosen: any
  // size, either sign (curv::BigInt over GMP; the decimal serde takes a leading '-').  The fixed-width ABI carries kw / 2kw limbs of
  // non-negative values.  So each proof is classified on the host:
  //   * CANONICAL (range_layout_carries: every field non-negative and within its width, exactly error_factor rows stored): flattened
  //     into the SoA batch, ONE zkp_range_ni_verify_batch for all of them;
  //   * anything else goes through verify_general below: the reference's row logic verbatim on signed host integers, its modular
  //     exponentiations — the Enc of every row that needs one — still batched on the GPU.  Such a proof gets exactly the verdict,
  //     or the panic, the reference reaches for it (tests/golden/signed_cases.json);
  //   * the one thing that has no answer here is a KEY the engine cannot carry (not a positive odd integer of <= 4096 bits):
  //     Result::unsupported.
  static std::vector<Result> verify_batch(const EncryptionKey& ek, const std::vector<const RangeProofNi*>& proofs) {
    const size_t B = proofs.size();
    if (B == 0) return {};
    if (ek.n.is_negative() || !ek.n.is_odd() || ek.n.bit_length() > 4096 || ek.n.bit_length() < 2)
      return std::vector<Result>(B, Result::unsupported("RangeProofNi::verify: the key is not a positive odd integer of at most 4096 bits"));
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    // The batch-wide row count of the single-call path is the one MOST proofs carry (prove always writes SECURITY_PARAMETER, so that is
    // what wins in practice; ties go to it) — not that of proofs[0]: one odd proof at the head of a batch must not push the honest ones
    // off the fast path.  Proofs with another error_factor are verified correctly, by verify_general.
    size_t EF = SECURITY_PARAMETER;
    {
      std::map<size_t, size_t> votes;
      for (const RangeProofNi* p : proofs) votes[p->error_factor]++;
      size_t best = votes.count(EF) ? votes[EF] : 0;
      for (const auto& kv : votes) if (kv.second > best && kv.first > 0 && kv.first <= 4096) { best = kv.second; EF = kv.first; }
    }
    std::vector<size_t> fast, general;
    HostTiming& tm = last_host_timing();
    tm = HostTiming(); tm.proofs = B; tm.threads = host_threads();
    StopWatch sw;
    std::vector<char> canon(B);
    parallel_for(B, [&](size_t b) {
      const RangeProofNi& p = *proofs[b];
      canon[b] = p.error_factor == EF && range_layout_carries(kw, EF, p.range, p.ciphertext, p.encrypted_pairs, p.proof, true);
    });
    for (size_t b = 0; b < B; b++) (canon[b] ? fast : general).push_back(b);
    tm.general_proofs = general.size();
    std::vector<Result> out(B, Result(false));
    if (!fast.empty()) {
      // ONE GPU call.  What a pipeline of chunks could hide is small — flattening 0.78 GB of received proofs takes 13 ms on 16 threads now
      // that the staging memory is huge-page backed (95 ms in round 4: first-touch faults) — and every extra launch has a tail of its
      // own.  B = 4096, one box, round 5: one call 3025 verifies/s, a quarter + the rest 2940, 2 / 4 equal chunks 2938 / 2650.
      const size_t F = fast.size();
      RawBuf<uint32_t> n(kw);
      ek.n.to_limbs(n.data(), kw);
      std::unique_ptr<RangeSlab> s(new RangeSlab(F, EF, kw, RangeSlab::ALL));
      std::vector<uint8_t> verdict(F);
      parallel_for(F, [&](size_t k) {
        const RangeProofNi& p = *proofs[fast[k]];
        s->put_statement(k, p.range, p.ciphertext); s->put_pairs(k, p.encrypted_pairs); s->put_proof(k, p.proof);
      });
      tm.sample_flatten_ms = sw.lap();
      zkp_range_ni_proofs p = s->abi(nb, n.data(), 0);
      e.check(zkp_range_ni_verify_batch(e.ctx(), &p, verdict.data(), 0), "zkp_range_ni_verify_batch");
      tm.gpu_ms = sw.lap();
      for (size_t k = 0; k < F; k++)
        out[fast[k]] = verdict[k] == ZKP_VERDICT_MALFORMED ? Result::panicked("RangeProofNi::verify: malformed proof (the reference would panic)") : Result(verdict[k] == ZKP_VERDICT_ACCEPT);
      const bool large = s->large();
      release_later(std::move(s), large);
    }
    if (!general.empty()) {
      std::vector<const RangeProofNi*> g;
      for (size_t b : general) g.push_back(proofs[b]);
      sw.lap();
      std::vector<Result> r = verify_general(ek, g);
      for (size_t k = 0; k < general.size(); k++) out[general[k]] = r[k];
      tm.general_ms = sw.lap();
    }
    return out;
  }

  // range_proof_ni.rs:109-128 -> range_proof.rs:254-355 on signed integers of any size (see verify_batch).  Operators as the
  // reference's BigInt has them: `%` truncated (:325,327), div_floor floored (:264), comparisons signed (:300-305,338), equality
  // exact (:293-298,335), to_bytes = magnitude in compute_digest (utils.rs:15-18, over EVERY stored c1 / c2).  Panics of the
  // reference — bits_of_e[i], responses[i], c1[i] / c2[i] past the end (:272-274,293,296,325,327) — are found per row, in the arm
  // that indexes, and win over any `false`.  All Enc of all these proofs: one batch on the GPU.
  // challenges: the verifier's own challenge bytes per proof (interactive RangeProof::verifier_output); null = Fiat-Shamir (above).
  static std::vector<Result> verify_general(const EncryptionKey& ek, const std::vector<const RangeProofNi*>& proofs,
                                            const std::vector<std::vector<uint8_t>>* challenges = nullptr) {
    struct Row { uint8_t what = 0; size_t enc0 = 0; BigInt expect0, expect1; bool flag = true; };   // what: 0 false, 1 open, 2 mask
    using EncList = std::vector<std::pair<const BigInt*, const BigInt*>>;
    struct Plan { std::vector<Row> rows; bool panic = false; EncList encs; size_t base = 0; };     // (enc0 of a row: relative to the plan's own list until the merge below)
    std::vector<Plan> plans(proofs.size());
    // one plan per proof, on the host threads: a transcript hash, a BigInt product and a Knuth division per Mask row — for a batch that an
    // adversarial sender pushed here that is the bulk of the host time
    parallel_for(proofs.size(), [&](size_t b) {
      const RangeProofNi& p = *proofs[b];
      Plan& pl = plans[b];
      EncList& encs = pl.encs;
      std::vector<uint8_t> ebytes;
      if (challenges) ebytes = (*challenges)[b];
      else {
        detail::Sha256 sh;
        sh.update(ek.n);
        for (const BigInt& v : p.encrypted_pairs.c1) sh.update(v);
        for (const BigInt& v : p.encrypted_pairs.c2) sh.update(v);
        ebytes = sh.finish().to_bytes();                               // leading zero bytes of the digest are dropped
      }
      const BigInt third = p.range.div_floor(BigInt(3)), two_thirds = BigInt(2) * third;      // :264-265
      for (size_t i = 0; i < p.error_factor && !pl.panic; i++) {
        if (i >= 8 * ebytes.size() || i >= p.proof.responses.size()) { pl.panic = true; break; }
        const bool ei = (ebytes[i / 8] >> (7 - i % 8)) & 1;
        const Response& rs = p.proof.responses[i];
        Row row;
        if (!ei && rs.kind == Response::Open) {                                              // :277-313
          if (i >= p.encrypted_pairs.c1.size() || i >= p.encrypted_pairs.c2.size()) { pl.panic = true; break; }
          row.what = 1; row.enc0 = encs.size();
          encs.push_back({&rs.w1, &rs.r1}); encs.push_back({&rs.w2, &rs.r2});
          row.expect0 = p.encrypted_pairs.c1[i]; row.expect1 = p.encrypted_pairs.c2[i];
          row.flag = (rs.w2 < third && rs.w1 > third && rs.w1 < two_thirds) || (rs.w1 < third && rs.w2 > third && rs.w2 < two_thirds);   // :300-305
        } else if (ei && rs.kind == Response::Mask) {                                         // :315-343
          const std::vector<BigInt>& cj = rs.j == 1 ? p.encrypted_pairs.c1 : p.encrypted_pairs.c2;   // any j != 1 selects c2, :324-328
          if (i >= cj.size()) { pl.panic = true; break; }
          row.what = 2; row.enc0 = encs.size();
          encs.push_back({&rs.masked_x, &rs.masked_r});
          row.expect0 = (cj[i] * p.ciphertext) % ek.nn;                                       // truncated, sign of the product
          row.flag = !(rs.masked_x < third || rs.masked_x > two_thirds);                      // :338
        }
        pl.rows.push_back(std::move(row));
      }
    });
    EncList encs;
    for (Plan& pl : plans) {
      pl.base = encs.size();
      if (pl.panic) continue;                                        // (a proof that panics needs no Enc: the panic wins over any `false`)
      encs.insert(encs.end(), pl.encs.begin(), pl.encs.end());
    }
    const std::vector<BigInt> E = Paillier::encrypt_with_chosen_randomness_batch(ek, encs);
    std::vector<Result> out;
    for (const Plan& pl : plans) {
      if (pl.panic) { out.push_back(Result::panicked("index out of bounds: the len is less than error_factor")); continue; }
      bool all = true;
      for (const Row& r : pl.rows) {
        bool res = r.what != 0 && r.flag;
        if (r.what == 1) res = res && E[pl.base + r.enc0] == r.expect0 && E[pl.base + r.enc0 + 1] == r.expect1;
        if (r.what == 2) res = res && E[pl.base + r.enc0] == r.expect0;
        all = all && res;
      }
      out.emplace_back(all);
    }
    return out;
  }

  // range_proof_ni.rs:84-107
  Result verify(const EncryptionKey& ek_, const BigInt& ciphertext_) const {
    if (!(ek_ == ek)) throw Panic("assertion failed: `(left == right)` ek");                  // :86
    if (ciphertext_ != ciphertext) throw Panic("assertion failed: `(left == right)` ciphertext");   // :88
    Result r = verify_batch(ek, {this})[0];
    (void)r.is_ok();                          // a single proof panics right here, as the reference does
    return r;
  }
  Result verify_self() const { Result r = verify_batch(ek, {this})[0]; (void)r.is_ok(); return r; }   // :109-128

  // serde_json::from_str + verify (ek given) / verify_self (ek == nullptr) for whole batches of documents, one Result per document:
  // zkp_range_ni_verify_json_batch tokenises, converts and verifies on the GPU; a document it hands back (ZKP_DOC_HOST_PATH: a valid
  // RangeProofNi the fixed layout cannot carry) is parsed here and goes through verify_batch; a document that is no RangeProofNi, or —
  // with ek — one made under another key, is the panic `from_str(..).unwrap()` / verify's assert_eq! is in the reference.
  // forms = ZKP_BIGINT_FORMS(key form, bare form).  Defined behind serde_json, at the end of this header.
  static std::vector<Result> verify_json_batch(const std::vector<std::string>& docs, uint32_t forms = 0, const EncryptionKey* ek = nullptr);
};


// ------------------------------------------------------------------ interactive RangeProof (src/zkproofs/range_proof.rs:83-355)
struct DataRandomnessPairs { std::vector<BigInt> w1, w2, r1, r2; };   // range_proof.rs:41-47
struct ChallengeBits { std::vector<uint8_t> bytes; };                 // :49-50
struct Commitment { BigInt com; };                                    // :83
struct ChallengeRandomness { BigInt r; };                             // :100

struct RangeProof {
  static constexpr size_t STATISTICAL_ERROR_FACTOR = 40;   // range_proof.rs:30

  // :359-369
  static BigInt compute_digest(const std::vector<uint8_t>& bytes) { detail::Sha256 s; s.update(bytes.data(), bytes.size()); return s.finish(); }
  static BigInt get_paillier_commitment(const EncryptionKey& ek, const BigInt& x, const BigInt& r) { return Paillier::encrypt_with_chosen_randomness(ek, x, r); }

  struct VerifierCommit { Commitment com; ChallengeRandomness r; ChallengeBits e; };
  // :118-126 — e = STATISTICAL_ERROR_FACTOR random bits, com = Enc(SHA256(e), r)
  static VerifierCommit verifier_commit(const EncryptionKey& ek) {
    ChallengeBits e;
    e.bytes.resize(STATISTICAL_ERROR_FACTOR / 8);
    for (auto& b : e.bytes) b = (uint8_t)detail::ChaChaRng::local().next();
    BigInt r = BigInt::sample_below(ek.n);
    return {Commitment{get_paillier_commitment(ek, compute_digest(e.bytes), r)}, ChallengeRandomness{r}, e};
  }
  // :195-208
  static Result verify_commit(const EncryptionKey& ek, const Commitment& com, const ChallengeRandomness& r, const ChallengeBits& e) {
    return Result(com.com == get_paillier_commitment(ek, compute_digest(e.bytes), r.r));
  }

  // :128-193 — the 2 * error_factor encryptions are one launch
  static std::pair<EncryptedPairs, DataRandomnessPairs> generate_encrypted_pairs(const EncryptionKey& ek, const BigInt& range, size_t error_factor) {
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t EF = error_factor;
    DataRandomnessPairs d;
    const BigInt third = range.div_floor(BigInt(3)), two_thirds = BigInt(2) * third;   // :133-134
    for (size_t i = 0; i < EF; i++) {
      BigInt a = BigInt::sample_range(third, two_thirds), c = a - third;                // :136-141
      if (BigInt::coin()) std::swap(a, c);                                               // :144-149
      d.w1.push_back(a); d.w2.push_back(c);
      d.r1.push_back(BigInt::sample_below(ek.n)); d.r2.push_back(BigInt::sample_below(ek.n));   // :151-159
    }
    std::vector<uint32_t> n(kw);
    ek.n.to_limbs(n.data(), kw);
    RangeSlab s(1, EF, kw, RangeSlab::PAIRS);
    RangeWitness wt(1, EF, kw, false, true);
    for (size_t i = 0; i < EF; i++) wt.put_nonces(i, d.w1[i], d.w2[i], d.r1[i], d.r2[i]);
    const zkp_range_ni_proofs p = s.abi(nb, n.data(), 0);
    const zkp_range_ni_witness w = wt.abi();
    e.check(zkp_range_generate_encrypted_pairs_batch(e.ctx(), &p, &w, 0), "zkp_range_generate_encrypted_pairs_batch");
    EncryptedPairs ep;
    s.read_pairs(0, ep);
    return {ep, d};
  }

  static void pack_challenge(const ChallengeBits& e, uint8_t (&eb)[32], uint8_t& elen) {
    if (e.bytes.size() > 32) throw std::invalid_argument("ChallengeBits: the fixed-layout ABI carries at most 256 challenge bits");
    std::memset(eb, 0, 32);
    std::memcpy(eb, e.bytes.data(), e.bytes.size());
    elen = (uint8_t)e.bytes.size();
  }

  // :210-252
  static Proof generate_proof(const EncryptionKey& ek, const BigInt& secret_x, const BigInt& secret_r, const ChallengeBits& ch, const BigInt& range,
                              const DataRandomnessPairs& d, size_t error_factor) {
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t EF = error_factor;
    if (d.w1.size() < EF || d.w2.size() < EF || d.r1.size() < EF || d.r2.size() < EF) throw Panic("index out of bounds");   // data.w1[i]
    std::vector<uint32_t> n(kw);
    ek.n.to_limbs(n.data(), kw);
    RangeSlab s(1, EF, kw, RangeSlab::STATEMENT | RangeSlab::RESPONSES);
    RangeWitness wt(1, EF, kw, true, true);
    s.put_statement(0, range, BigInt());             // (no prover function reads the ciphertext)
    wt.put_secret(0, secret_x, secret_r);
    for (size_t i = 0; i < EF; i++) wt.put_nonces(i, d.w1[i], d.w2[i], d.r1[i], d.r2[i]);
    uint8_t eb[32], elen, status = 0;
    pack_challenge(ch, eb, elen);
    const zkp_range_ni_proofs p = s.abi(nb, n.data(), 0);
    const zkp_range_ni_witness w = wt.abi();
    e.check(zkp_range_generate_proof_batch(e.ctx(), &p, &w, eb, &elen, &status, 0), "zkp_range_generate_proof_batch");
    if (status != 0) throw Panic("RangeProof::generate_proof: malformed (the reference would panic: bits_of_e[i])");
    Proof out;
    s.read_proof(0, out);
    return out;
  }

  // :254-355
  static Result verifier_output(const EncryptionKey& ek, const ChallengeBits& ch, const EncryptedPairs& ep, const Proof& proof, const BigInt& range,
                                const BigInt& cipher_x, size_t error_factor) {
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t EF = error_factor;
    // values the fixed-width call cannot carry (negative, over-wide), short vectors, a challenge of more than 32 bytes: the reference's
    // row logic on signed host integers with the verifier's own challenge (RangeProofNi::verify_general), Enc still on the GPU
    const bool canonical = ch.bytes.size() <= 32 && range_layout_carries(kw, EF, range, cipher_x, ep, proof, false);
    if (!canonical) {
      RangeProofNi tmp;
      tmp.ek = ek; tmp.range = range; tmp.ciphertext = cipher_x; tmp.encrypted_pairs = ep; tmp.proof = proof; tmp.error_factor = EF;
      const std::vector<std::vector<uint8_t>> chal{ch.bytes};
      Result r = RangeProofNi::verify_general(ek, {&tmp}, &chal)[0];
      (void)r.is_ok();                          // a panic of the reference is thrown here
      return r;
    }
    std::vector<uint32_t> n(kw);
    ek.n.to_limbs(n.data(), kw);
    RangeSlab s(1, EF, kw, RangeSlab::ALL);
    s.put_statement(0, range, cipher_x); s.put_pairs(0, ep); s.put_proof(0, proof);
    uint8_t eb[32], elen, verdict = 0;
    pack_challenge(ch, eb, elen);
    const zkp_range_ni_proofs p = s.abi(nb, n.data(), 0);
    e.check(zkp_range_verifier_output_batch(e.ctx(), &p, eb, &elen, &verdict, 0), "zkp_range_verifier_output_batch");
    if (verdict == ZKP_VERDICT_MALFORMED) throw Panic("RangeProof::verifier_output: malformed proof (the reference would panic)");
    return Result(verdict == ZKP_VERDICT_ACCEPT);
  }

  // ---- whole batches of sessions under one key, one GPU call per step.  The prover keeps a ProverSeed between message 1 and message 3 instead
  // of DataRandomnessPairs: both steps expand the witness of session b from (seed, first_index + b) ON THE GPU (the stream is defined in
  // include/zkp_hip.h), where it is wiped before the call returns.  A (seed, index) commits to ONE statement and answers ONE challenge: a second
  // challenge over the same commitments opens some row both ways and gives x away.
  struct ProverSeed {
    uint8_t bytes[32];
    ProverSeed() { std::memset(bytes, 0, sizeof bytes); }
    static ProverSeed fresh() { ProverSeed s; detail::ChaChaRng::os_random(s.bytes, sizeof s.bytes); return s; }     // (the source of prove_batch_seeded)
    ~ProverSeed() { detail::ChaChaRng::wipe(bytes, sizeof bytes); }
  };
  // :128-193 for B sessions: EncryptedPairs only — there is no DataRandomnessPairs to hand back
  static std::vector<EncryptedPairs> generate_encrypted_pairs_batch_seeded(const EncryptionKey& ek, const std::vector<BigInt>& ranges, size_t error_factor,
                                                                           const ProverSeed& seed, uint64_t first_index = 0) {
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t B = ranges.size(), EF = error_factor;
    std::vector<EncryptedPairs> out(B);
    if (B == 0) return out;
    std::vector<uint32_t> n(kw);
    ek.n.to_limbs(n.data(), kw);
    RangeSlab s(B, EF, kw, RangeSlab::STATEMENT | RangeSlab::PAIRS);
    parallel_for(B, [&](size_t b) { s.put_statement(b, ranges[b], BigInt()); });      // (no prover function reads the ciphertext)
    std::vector<uint8_t> status(B, 0);
    const zkp_range_ni_proofs p = s.abi(nb, n.data(), 0);
    e.check(zkp_range_generate_encrypted_pairs_seeded_batch(e.ctx(), &p, seed.bytes, first_index, status.data(), 0), "zkp_range_generate_encrypted_pairs_seeded_batch");
    statuses_ok(status, "RangeProof::generate_encrypted_pairs: malformed (an empty interval to sample from: the reference would panic)");
    parallel_for(B, [&](size_t b) { s.read_pairs(b, out[b]); });
    return out;
  }
  // :210-252 for B sessions, with the seed and first_index of their generate_encrypted_pairs_batch_seeded
  static std::vector<Proof> generate_proof_batch_seeded(const EncryptionKey& ek, const std::vector<BigInt>& xs, const std::vector<BigInt>& rs,
                                                        const std::vector<ChallengeBits>& challenges, const std::vector<BigInt>& ranges, size_t error_factor,
                                                        const ProverSeed& seed, uint64_t first_index = 0) {
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t B = ranges.size(), EF = error_factor;
    if (xs.size() != B || rs.size() != B || challenges.size() != B) throw std::invalid_argument("RangeProof::generate_proof_batch_seeded: one secret and one challenge per session");
    std::vector<Proof> out(B);
    if (B == 0) return out;
    std::vector<uint32_t> n(kw);
    ek.n.to_limbs(n.data(), kw);
    RangeSlab s(B, EF, kw, RangeSlab::STATEMENT | RangeSlab::RESPONSES);
    RangeWitness wt(B, EF, kw, true, false);
    std::vector<uint8_t> eb(B * 32), elen(B), status(B, 0);
    for (size_t b = 0; b < B; b++) {
      s.put_statement(b, ranges[b], BigInt());
      wt.put_secret(b, xs[b], rs[b]);
      uint8_t one[32];
      pack_challenge(challenges[b], one, elen[b]);
      std::memcpy(&eb[b * 32], one, 32);
    }
    const zkp_range_ni_proofs p = s.abi(nb, n.data(), 0);
    const int32_t st = zkp_range_generate_proof_seeded_batch(e.ctx(), &p, wt.x(), wt.r(), seed.bytes, first_index, eb.data(), elen.data(), status.data(), 0);
    wt.wipe_secrets();                                  // x and r: gone before this call returns, whatever it returns
    e.check(st, "zkp_range_generate_proof_seeded_batch");
    statuses_ok(status, "RangeProof::generate_proof: malformed (the reference would panic: bits_of_e[i])");
    parallel_for(B, [&](size_t b) { s.read_proof(b, out[b]); });
    return out;
  }
  // ---- the verifier's commitment to its challenge for whole batches of sessions, one GPU call per step.  The verifier keeps a VerifierSeed
  // between its messages instead of (r, e) per session: the commit call expands (seed, first_index + b) ON THE GPU into r and e, hashes e and
  // encrypts, and nothing but com leaves the device; the reveal call regenerates the same (r, e) for the decommit message and for
  // verifier_output.  A (seed, index) belongs to ONE session; reveal only after the prover's encrypted pairs have arrived.
  // keys: one key for all `sessions` sessions, or one key per session (sessions = 0: keys.size()), all of one kernel width.  A key of this
  // step is an odd integer of 257 .. 4096 bits (the digest must be a canonical plaintext): anything else is std::invalid_argument.
  struct VerifierSeed {
    uint8_t bytes[32];
    VerifierSeed() { std::memset(bytes, 0, sizeof bytes); }
    static VerifierSeed fresh() { VerifierSeed s; detail::ChaChaRng::os_random(s.bytes, sizeof s.bytes); return s; }
    ~VerifierSeed() { detail::ChaChaRng::wipe(bytes, sizeof bytes); }
  };
  // :118-126 for B sessions: the commitments only
  static std::vector<Commitment> verifier_commit_batch_seeded(const std::vector<EncryptionKey>& keys, const VerifierSeed& seed, uint64_t first_index = 0,
                                                              size_t sessions = 0, size_t e_len = STATISTICAL_ERROR_FACTOR / 8) {
    Engine& e = Engine::instance();
    const CommitKeys k = commit_keys(keys, sessions, "RangeProof::verifier_commit_batch_seeded");
    std::vector<Commitment> out(k.B);
    if (k.B == 0) return out;
    std::vector<uint32_t> com(k.B * 2 * k.kw);
    std::vector<uint8_t> status(k.B, 0);
    e.check(zkp_range_verifier_commit_seeded_batch(e.ctx(), k.nb, k.B, k.n.data(), k.stride, (uint32_t)e_len, seed.bytes, first_index, com.data(), status.data(), 0),
            "zkp_range_verifier_commit_seeded_batch");
    statuses_ok(status, "RangeProof::verifier_commit: no r below n in 128 attempts");
    for (size_t b = 0; b < k.B; b++) out[b].com = BigInt::from_limbs(&com[b * 2 * k.kw], 2 * k.kw);
    return out;
  }
  // the (r, e) of those commitments, from the same (keys, seed, first_index, sessions, e_len)
  static std::vector<std::pair<ChallengeRandomness, ChallengeBits>> verifier_reveal_batch_seeded(const std::vector<EncryptionKey>& keys, const VerifierSeed& seed,
                                                                                                 uint64_t first_index = 0, size_t sessions = 0,
                                                                                                 size_t e_len = STATISTICAL_ERROR_FACTOR / 8) {
    Engine& e = Engine::instance();
    const CommitKeys k = commit_keys(keys, sessions, "RangeProof::verifier_reveal_batch_seeded");
    std::vector<std::pair<ChallengeRandomness, ChallengeBits>> out(k.B);
    if (k.B == 0) return out;
    std::vector<uint32_t> r(k.B * k.kw);
    std::vector<uint8_t> eb(k.B * 32), status(k.B, 0);
    const int32_t st = zkp_range_verifier_reveal_seeded_batch(e.ctx(), k.nb, k.B, k.n.data(), k.stride, (uint32_t)e_len, seed.bytes, first_index, r.data(), eb.data(),
                                                              status.data(), 0);
    if (st == ZKP_OK)
      for (size_t b = 0; b < k.B; b++) {
        out[b].first.r = BigInt::from_limbs(&r[b * k.kw], k.kw);
        out[b].second.bytes.assign(&eb[b * 32], &eb[b * 32] + e_len);
      }
    detail::ChaChaRng::wipe(r.data(), r.size() * 4);
    detail::ChaChaRng::wipe(eb.data(), eb.size());
    e.check(st, "zkp_range_verifier_reveal_seeded_batch");
    statuses_ok(status, "RangeProof::verifier_commit: no r below n in 128 attempts");
    return out;
  }
  // :195-208 for B sessions, one Result per session: one zkp_range_verify_commit_batch per kernel width.  A session the fixed layout cannot
  // carry — a negative or over-wide r or com, an e of more than 32 bytes, a key outside the domain above — goes through verify_commit, the
  // single-session host path, and is merged in (a key that path cannot carry either is Result::unsupported).
  static std::vector<Result> verify_commit_batch(const std::vector<EncryptionKey>& keys, const std::vector<Commitment>& coms, const std::vector<ChallengeRandomness>& rs,
                                                 const std::vector<ChallengeBits>& es) {
    Engine& e = Engine::instance();
    const size_t B = coms.size();
    if (rs.size() != B || es.size() != B || (B && keys.size() != 1 && keys.size() != B))
      throw std::invalid_argument("RangeProof::verify_commit_batch: one commitment, one r and one e per session, one key or one key per session");
    std::vector<Result> out(B, Result(false));
    auto key_of = [&](size_t b) -> const EncryptionKey& { return keys.size() == 1 ? keys[0] : keys[b]; };
    std::vector<uint8_t> carried(B, 0);
    for (size_t b = 0; b < B; b++) {
      const BigInt& n = key_of(b).n;
      if (commit_key_ok(n)) {
        const uint32_t kw = width_for(n) / 32;
        carried[b] = !coms[b].com.is_negative() && coms[b].com.fits_limbs(2 * kw) && !rs[b].r.is_negative() && rs[b].r.fits_limbs(kw) && es[b].bytes.size() <= 32;
      }
      if (carried[b]) continue;
      try { out[b] = verify_commit(key_of(b), coms[b], rs[b], es[b]); }
      catch (const Panic& p) { out[b] = Result::panicked(p.what()); }
      catch (const std::exception& x) { out[b] = Result::unsupported(x.what()); }
    }
    for (uint32_t nb : {1024u, 2048u, 4096u}) {
      const uint32_t kw = nb / 32;
      std::vector<size_t> idx;
      for (size_t b = 0; b < B; b++) if (carried[b] && width_for(key_of(b).n) == nb) idx.push_back(b);
      if (idx.empty()) continue;
      const bool shared = keys.size() == 1;
      const size_t cnt = idx.size();
      std::vector<uint32_t> n((shared ? 1 : cnt) * kw), com(cnt * 2 * kw), r(cnt * kw);
      std::vector<uint8_t> eb(cnt * 32, 0), elen(cnt), v(cnt, 9);
      if (shared) keys[0].n.to_limbs(n.data(), kw);
      for (size_t q = 0; q < cnt; q++) {
        const size_t b = idx[q];
        if (!shared) keys[b].n.to_limbs(&n[q * kw], kw);
        coms[b].com.to_limbs(&com[q * 2 * kw], 2 * kw);
        rs[b].r.to_limbs(&r[q * kw], kw);
        std::memcpy(&eb[q * 32], es[b].bytes.data(), es[b].bytes.size());
        elen[q] = (uint8_t)es[b].bytes.size();
      }
      e.check(zkp_range_verify_commit_batch(e.ctx(), nb, cnt, n.data(), shared ? 0 : kw, com.data(), r.data(), eb.data(), elen.data(), v.data(), 0),
              "zkp_range_verify_commit_batch");
      for (size_t q = 0; q < cnt; q++)
        out[idx[q]] = v[q] == ZKP_VERDICT_MALFORMED ? Result::panicked("RangeProof::verify_commit: malformed session") : Result(v[q] == ZKP_VERDICT_ACCEPT);
    }
    return out;
  }

  // :254-355 for B sessions on the two received documents of each: zkp_range_verifier_output_json_batch tokenises, converts and verifies on the
  // GPU.  A session it hands back (ZKP_DOC_HOST_PATH: valid documents the fixed layout cannot carry), one whose statement the layout cannot
  // carry and one whose challenge has more than 32 bytes are parsed here and go through verifier_output, which handles signed and over-wide
  // values; a document that is no EncryptedPairs / Proof is the panic `from_str(..).unwrap()` is in the reference.  A panic of the reference
  // is a Result that throws when looked at.  Defined behind serde_json, at the end of this header.
  static std::vector<Result> verifier_output_json_batch(const EncryptionKey& ek, const std::vector<ChallengeBits>& challenges, const std::vector<std::string>& pairs_docs,
                                                        const std::vector<std::string>& proof_docs, const std::vector<BigInt>& ranges, const std::vector<BigInt>& cipher_xs,
                                                        size_t error_factor);

 private:
  static void statuses_ok(const std::vector<uint8_t>& status, const char* what) { for (uint8_t s : status) if (s != 0) throw Panic(what); }
  // the key domain of the commitment calls (include/zkp_hip.h): odd, more than 256 bits — and no wider than the widest kernel
  static bool commit_key_ok(const BigInt& n) { return !n.is_negative() && n.is_odd() && n.bit_length() > 256 && n.bit_length() <= 4096; }
  // the keys of a seeded commitment call as limbs: one key for B sessions (stride 0) or B keys of one width
  struct CommitKeys { uint32_t nb = 0, kw = 0; size_t B = 0; uint64_t stride = 0; std::vector<uint32_t> n; };
  static CommitKeys commit_keys(const std::vector<EncryptionKey>& keys, size_t sessions, const char* who) {
    CommitKeys k;
    k.B = sessions ? sessions : keys.size();
    if (k.B == 0) return k;
    if (keys.size() != 1 && keys.size() != k.B) throw std::invalid_argument(std::string(who) + ": one key, or one key per session");
    for (const EncryptionKey& ek : keys)
      if (!commit_key_ok(ek.n)) throw std::invalid_argument(std::string(who) + ": a key of this step is an odd integer of 257 .. 4096 bits");
    k.nb = width_for(keys[0].n); k.kw = k.nb / 32; k.stride = keys.size() == 1 ? 0 : k.kw;
    k.n.resize(keys.size() * k.kw);
    for (size_t i = 0; i < keys.size(); i++) {
      if (width_for(keys[i].n) != k.nb) throw std::invalid_argument(std::string(who) + ": the keys of one call are of one kernel width (1024, 2048 or 4096 bits)");
      keys[i].n.to_limbs(&k.n[i * k.kw], k.kw);
    }
    return k;
  }
};

// ------------------------------------------------------------------ NiCorrectKeyProof
static const uint8_t SALT_STRING[4] = {75, 90, 101, 110};   // correct_key_ni.rs:28

class NiCorrectKeyProof {
 public:
  static constexpr size_t M2 = ZKP_CORRECT_KEY_M2, DIGEST_SIZE = 256;   // correct_key_ni.rs:29-30
  std::vector<BigInt> sigma_vec;

  // correct_key_ni.rs:105-117
  static BigInt mask_generation(size_t out_length, const BigInt& seed) {
    const size_t msklen = out_length / DIGEST_SIZE + 1;
    BigInt acc;
    for (size_t j = 0; j < msklen; j++) { BigInt jj(j); acc = acc + detail::compute_digest({&seed, &jj}).shl(j * DIGEST_SIZE); }
    return acc;
  }
  // correct_key_ni.rs:42-71 — prover side (needs the secret key).  The n-th roots are
  // rho^(n^-1 mod phi) mod n ([upstream] extract_nroot), computed by ONE batched GPU modexp.
  static NiCorrectKeyProof proof(const DecryptionKey& dk, const uint8_t* salt = SALT_STRING, size_t salt_len = 4) {
    Engine& e = Engine::instance();
    const BigInt n = dk.p * dk.q;
    const BigInt phi = (dk.p - BigInt::one()) * (dk.q - BigInt::one());
    const BigInt d = BigInt::mod_inv(n, phi);
    const BigInt salt_bn = [&] { BigInt s = BigInt::from_bytes(salt, salt_len); return detail::compute_digest({&s}); }();
    const uint32_t nb = n.bit_length() <= 2048 ? 2048 : 4096, kw = nb / 32;   // modexp kernel widths
    std::vector<uint32_t> base(M2 * kw), ex(kw), mod(kw), out(M2 * kw);
    for (size_t i = 0; i < M2; i++) {
      BigInt ii(i);
      BigInt seed = detail::compute_digest({&n, &salt_bn, &ii});
      (mask_generation(n.bit_length(), seed) % n).to_limbs(&base[i * kw], kw);
    }
    d.to_limbs(ex.data(), kw); n.to_limbs(mod.data(), kw);
    e.check(zkp_modexp_batch(e.ctx(), nb, nb, M2, base.data(), ex.data(), 0, mod.data(), 0, out.data(), 0), "zkp_modexp_batch");
    NiCorrectKeyProof p;
    for (size_t i = 0; i < M2; i++) p.sigma_vec.push_back(BigInt::from_limbs(&out[i * kw], kw));
    return p;
  }
  // The same for many keys in ONE zkp_correct_key_ni_prove_batch per kernel width (the widths are grouped as verify_batch groups them; a key
  // whose factors do not both fit half its width takes the next one): n, rho and the n-th roots — by upstream's extract_nroot, CRT under p
  // and q — are computed on the GPU, n^-1 mod phi is never formed, and the staging that carries p and q is wiped on release.  A key the call
  // marks ZKP_VERDICT_MALFORMED (an even or trivial factor, gcd(n, phi(n)) != 1), or a factor that is not positive, is a Panic naming the
  // key's index, as `mod_inv(..).unwrap()` is in the reference; a factor wider than 2048 bits throws std::length_error.
  static std::vector<NiCorrectKeyProof> proof_batch(const std::vector<const DecryptionKey*>& keys, const uint8_t* salt = SALT_STRING, size_t salt_len = 4) {
    Engine& e = Engine::instance();
    std::vector<NiCorrectKeyProof> out(keys.size());
    std::vector<uint32_t> width(keys.size());
    for (size_t k = 0; k < keys.size(); k++) {
      const DecryptionKey& dk = *keys[k];
      if (dk.p.is_negative() || dk.q.is_negative() || dk.p.is_zero() || dk.q.is_zero()) throw Panic("NiCorrectKeyProof::proof_batch: key " + std::to_string(k) + " is outside the domain (a factor is not positive)");
      const size_t fb = std::max(dk.p.bit_length(), dk.q.bit_length());
      if (fb > 2048) throw std::length_error("NiCorrectKeyProof::proof_batch: key " + std::to_string(k) + ": factor wider than 2048 bits");
      uint32_t nb = width_for(dk.p * dk.q);
      while (fb > nb / 2) nb *= 2;
      width[k] = nb;
    }
    for (uint32_t nb : {1024u, 2048u, 4096u}) {
      const uint32_t kw = nb / 32, hw = nb / 64;
      std::vector<size_t> idx;
      for (size_t k = 0; k < keys.size(); k++) if (width[k] == nb) idx.push_back(k);
      if (idx.empty()) continue;
      RawBuf<uint32_t> p(idx.size() * hw, true), q(idx.size() * hw, true);                       // (secret: wiped on release)
      std::vector<uint32_t> sg(idx.size() * M2 * kw);
      std::vector<uint8_t> st(idx.size(), 9);
      for (size_t j = 0; j < idx.size(); j++) { keys[idx[j]]->p.to_limbs(&p[j * hw], hw); keys[idx[j]]->q.to_limbs(&q[j * hw], hw); }
      const int32_t rc = zkp_correct_key_ni_prove_batch(e.ctx(), nb, idx.size(), p.data(), q.data(), salt, (uint32_t)salt_len, nullptr, sg.data(), st.data(), 0);
      p.wipe_now(); q.wipe_now();
      e.check(rc, "zkp_correct_key_ni_prove_batch");
      for (size_t j = 0; j < idx.size(); j++) {
        if (st[j] != 0) throw Panic("NiCorrectKeyProof::proof_batch: key " + std::to_string(idx[j]) + " is outside the domain (ZKP_VERDICT_MALFORMED)");
        for (size_t i = 0; i < M2; i++) out[idx[j]].sigma_vec.push_back(BigInt::from_limbs(&sg[(j * M2 + i) * kw], kw));
      }
    }
    return out;
  }
  // correct_key_ni.rs:73-100 for many (key, proof) pairs in ONE zkp_correct_key_ni_verify_batch (keys of one kernel width per call; the
  // widths are grouped here).  sigma_i is prover-chosen: any size, either sign — the reference only uses it as mod_pow(sigma_i, n, n),
  // which depends on sigma_i mod n (floored: mpz_powm), so a non-canonical root is reduced on the host and gets the reference's verdict;
  // a zero key and fewer than 11 roots are the reference's panics (:82-85, :92), checked in its order; an even key then fails the primorial gcd test whatever the roots are (Err); a key
  // the engine cannot carry (not positive, or wider than 4096 bits) is Result::unsupported.
  static std::vector<Result> verify_batch(const std::vector<std::pair<const EncryptionKey*, const NiCorrectKeyProof*>>& items, const uint8_t* salt = SALT_STRING,
                                          size_t salt_len = 4) {
    Engine& e = Engine::instance();
    std::vector<Result> out(items.size(), Result(false));
    for (uint32_t nb : {1024u, 2048u, 4096u}) {
      const uint32_t kw = nb / 32;
      std::vector<size_t> idx;
      for (size_t k = 0; k < items.size(); k++) {
        const BigInt& n = items[k].first->n;
        // in the reference's order: rho_i = mask_generation(..) % n panics on n = 0 (:82-85); sigma_vec[i] for i < 11 panics on a short vector
        // (:90-93) — both BEFORE anything is compared; only then does an even key fail the primorial gcd test whatever the roots are (:87-88,95)
        if (n.is_zero()) { out[k] = Result::panicked("attempt to calculate the remainder with a divisor of zero"); continue; }
        if (items[k].second->sigma_vec.size() < M2) { out[k] = Result::panicked("index out of bounds: sigma_vec"); continue; }
        if (!n.is_negative() && !n.is_odd()) continue;                    // an even key: Err(IncorrectProof); `out` holds that already
        const bool supported = !n.is_negative() && n.is_odd() && n.bit_length() >= 2 && n.bit_length() <= 4096;
        if (!supported) { if (nb == 1024) out[k] = Result::unsupported("NiCorrectKeyProof::verify: the key is not a positive integer of at most 4096 bits"); continue; }
        if (width_for(n) != nb) continue;
        idx.push_back(k);
      }
      if (idx.empty()) continue;
      std::vector<uint32_t> n(idx.size() * kw), sg(idx.size() * M2 * kw);
      std::vector<uint8_t> v(idx.size(), 9);
      for (size_t q = 0; q < idx.size(); q++) {
        const EncryptionKey& ek = *items[idx[q]].first;
        ek.n.to_limbs(&n[q * kw], kw);
        for (size_t i = 0; i < M2; i++) {
          const BigInt& s = items[idx[q]].second->sigma_vec[i];
          (s.fits_limbs(kw) ? s : s.modulus(ek.n)).to_limbs(&sg[(q * M2 + i) * kw], kw);
        }
      }
      e.check(zkp_correct_key_ni_verify_batch(e.ctx(), nb, idx.size(), n.data(), sg.data(), salt, (uint32_t)salt_len, v.data(), 0), "zkp_correct_key_ni_verify_batch");
      for (size_t q = 0; q < idx.size(); q++) out[idx[q]] = Result(v[q] == ZKP_VERDICT_ACCEPT);
    }
    return out;
  }
  Result verify(const EncryptionKey& ek, const uint8_t* salt = SALT_STRING, size_t salt_len = 4) const {
    Result r = verify_batch({{&ek, this}}, salt, salt_len)[0];
    (void)r.is_ok();                          // a single proof panics right here, as the reference does
    return r;
  }
  // serde_json::from_str + verify for whole batches of (key, document) pairs, one Result per pair: zkp_correct_key_ni_verify_json_batch
  // tokenises, converts and verifies on the GPU (one call per key width).  A document it does not convert is parsed here: one that is no
  // NiCorrectKeyProof is the panic `from_str(..).unwrap()` is in the reference; every other one (ZKP_DOC_HOST_PATH: a root the fixed
  // layout cannot carry; a sigma_vec of another length), and every document under a key the engine does not take, goes through
  // verify_batch.  Defined behind serde_json, at the end of this header.
  static std::vector<Result> verify_json_batch(const std::vector<std::pair<const EncryptionKey*, std::string>>& items, const uint8_t* salt = SALT_STRING,
                                               size_t salt_len = 4);
};

// ------------------------------------------------------------------ interactive CorrectKey (src/zkproofs/correct_key.rs:28-183)
// the same 2048-bit modexp shape x40, composed on the host from batched GPU calls.
struct Challenge { std::vector<BigInt> sn; BigInt e; std::vector<BigInt> z; };   // :29-39
struct VerificationAid { BigInt s_digest; };                                       // :41-45
struct CorrectKeyProof { BigInt s_digest; };                                       // :47-51
enum class CorrectKeyProveError { SniNotCoprimeWithN, ZiNotCoprimeWithN, RniNotCoprimeWithN, EWasntComputedCorrectly };   // :174-183

struct CorrectKey {
  static constexpr size_t STATISTICAL_ERROR_FACTOR = 40;   // :26
  static BigInt digest_chain(const BigInt* first, const std::vector<BigInt>& a, const std::vector<BigInt>* b = nullptr) {
    detail::Sha256 s;
    if (first) s.update(*first);
    for (auto& v : a) s.update(v);
    if (b) for (auto& v : *b) s.update(v);
    return s.finish();
  }
  // :64-102
  static std::pair<Challenge, VerificationAid> challenge(const EncryptionKey& ek) {
    std::vector<BigInt> s, r;
    for (size_t i = 0; i < STATISTICAL_ERROR_FACTOR; i++) { s.push_back(BigInt::sample_below(ek.n)); r.push_back(BigInt::sample_below(ek.n)); }
    return challenge_with(ek, s, r);
  }
  // the same with the values the reference samples (:67-70, :80-83) supplied by the caller (parity tests)
  static std::pair<Challenge, VerificationAid> challenge_with(const EncryptionKey& ek, const std::vector<BigInt>& s, const std::vector<BigInt>& r) {
    if (s.size() != r.size()) throw std::invalid_argument("CorrectKey::challenge_with: |s| != |r|");
    const size_t K = s.size();
    std::vector<BigInt> both = s; both.insert(both.end(), r.begin(), r.end());
    std::vector<BigInt> pw = mod_pow_batch(both, {ek.n}, ek.n);                               // sn, rn  (:73-76, :86-89)
    std::vector<BigInt> sn(pw.begin(), pw.begin() + K), rn(pw.begin() + K, pw.end());
    BigInt e = digest_chain(&ek.n, sn, &rn);                                                  // :91
    std::vector<BigInt> se = mod_pow_batch(s, {e}, ek.n);                                     // s_i^e  (:96)
    std::vector<BigInt> z;
    for (size_t i = 0; i < K; i++) z.push_back((r[i] * se[i]) % ek.n);
    return {Challenge{sn, e, z}, VerificationAid{digest_chain(nullptr, s)}};                  // :100-102
  }
  // :104-162 — returns the proof or the error
  struct ProveResult {
    bool ok; CorrectKeyProof proof; CorrectKeyProveError err;
    bool is_ok() const { return ok; }
    bool is_err() const { return !ok; }
    const CorrectKeyProof& unwrap() const { if (!ok) throw Panic("called `Result::unwrap()` on an `Err` value"); return proof; }
  };
  static ProveResult prove(const DecryptionKey& dk, const Challenge& ch) {
    const BigInt dk_n = dk.q * dk.p, one = BigInt::one();
    auto fail = [](CorrectKeyProveError e) { return ProveResult{false, CorrectKeyProof{}, e}; };
    for (auto& v : ch.sn) if (BigInt::gcd(dk_n, v) != one) return fail(CorrectKeyProveError::SniNotCoprimeWithN);   // :110-116
    for (auto& v : ch.z) if (BigInt::gcd(dk_n, v) != one) return fail(CorrectKeyProveError::ZiNotCoprimeWithN);     // :119-125
    const BigInt phi = (dk.q - one) * (dk.p - one);
    const BigInt phimine = phi - (ch.e % phi);                                                                       // :130
    std::vector<BigInt> zn = mod_pow_batch(ch.z, {dk_n}, dk_n), snphi = mod_pow_batch(ch.sn, {phimine}, dk_n);       // :135-137
    std::vector<BigInt> rn;
    for (size_t i = 0; i < ch.z.size(); i++) rn.push_back((zn[i] * snphi[i]) % dk_n);
    for (auto& v : rn) if (BigInt::gcd(dk_n, v) != one) return fail(CorrectKeyProveError::RniNotCoprimeWithN);       // :143-148
    if (ch.e != digest_chain(&dk_n, ch.sn, &rn)) return fail(CorrectKeyProveError::EWasntComputedCorrectly);         // :151-156
    // s_digest = H(extract_nroot(dk, sn_i)...): sn_i^(n^-1 mod phi) mod n  ([upstream] extract_nroot)              // :159
    std::vector<BigInt> roots = mod_pow_batch(ch.sn, {BigInt::mod_inv(dk_n, phi)}, dk_n);
    return ProveResult{true, CorrectKeyProof{digest_chain(nullptr, roots)}, CorrectKeyProveError::EWasntComputedCorrectly};
  }
  // :164-171
  static Result verify(const CorrectKeyProof& proof, const VerificationAid& va) { return Result(proof.s_digest == va.s_digest); }

  // ---- whole batches of sessions, one GPU call per step and kernel width (include/zkp_hip.h: zkp_correct_key_challenge_seeded_batch,
  // zkp_correct_key_prove_batch, zkp_correct_key_verify_seeded_batch).  The verifier keeps a VerifierSeed between its messages instead of
  // an aid per session: session b of a call is (seed, first_index + b), its s and r are expanded ON THE GPU, and verify_batch_seeded
  // regenerates s there.  s and its digest are the verifier's secret until the proof has arrived; a (seed, index) belongs to ONE session.
  struct VerifierSeed {
    uint8_t bytes[32];
    VerifierSeed() { std::memset(bytes, 0, sizeof bytes); }
    static VerifierSeed fresh() { VerifierSeed s; detail::ChaChaRng::os_random(s.bytes, sizeof s.bytes); return s; }
    ~VerifierSeed() { detail::ChaChaRng::wipe(bytes, sizeof bytes); }
  };
  // calls f(lo, hi, nb) for every run [lo, hi) of consecutive keys of one kernel width (a batch of one width: one run, one GPU call)
  template <class F> static void width_runs(const std::vector<EncryptionKey>& keys, const char* who, F&& f) {
    for (const EncryptionKey& k : keys)
      if (k.n.is_negative() || k.n.is_zero() || k.n.bit_length() > 4096) throw std::invalid_argument(std::string(who) + ": a key is a positive integer of at most 4096 bits");
    for (size_t lo = 0; lo < keys.size();) {
      const uint32_t nb = width_for(keys[lo].n);
      size_t hi = lo + 1;
      while (hi < keys.size() && width_for(keys[hi].n) == nb) hi++;
      f(lo, hi, nb);
      lo = hi;
    }
  }
  // :64-102 for one session per key; aids (nullable) receives the VerificationAids.  A key the call marks ZKP_VERDICT_MALFORMED (even, or no
  // s below n in 128 attempts) is a Panic naming the session.
  static std::vector<Challenge> challenge_batch_seeded(const std::vector<EncryptionKey>& keys, const VerifierSeed& seed, uint64_t first_index,
                                                       std::vector<VerificationAid>* aids, size_t K = STATISTICAL_ERROR_FACTOR) {
    Engine& e = Engine::instance();
    std::vector<Challenge> out(keys.size());
    if (aids) aids->assign(keys.size(), VerificationAid{});
    width_runs(keys, "CorrectKey::challenge_batch_seeded", [&](size_t lo, size_t hi, uint32_t nb) {
      const size_t B = hi - lo, kw = nb / 32;
      std::vector<uint32_t> n(B * kw), sn(B * K * kw), z(B * K * kw), ee(B * 8);
      RawBuf<uint32_t> sd(aids ? B * 8 : 0, true);                                            // (secret until the proof has arrived: wiped on release)
      std::vector<uint8_t> st(B, 9);
      for (size_t b = 0; b < B; b++) keys[lo + b].n.to_limbs(&n[b * kw], kw);
      e.check(zkp_correct_key_challenge_seeded_batch(e.ctx(), nb, B, (uint32_t)K, n.data(), kw, seed.bytes, first_index + lo, sn.data(), ee.data(), z.data(),
                                                     aids ? sd.data() : nullptr, st.data(), 0), "zkp_correct_key_challenge_seeded_batch");
      for (size_t b = 0; b < B; b++) {
        if (st[b] != 0) throw Panic("CorrectKey::challenge_batch_seeded: session " + std::to_string(lo + b) + ": the key is outside the domain (ZKP_VERDICT_MALFORMED)");
        Challenge& c = out[lo + b];
        for (size_t i = 0; i < K; i++) { c.sn.push_back(BigInt::from_limbs(&sn[(b * K + i) * kw], kw)); c.z.push_back(BigInt::from_limbs(&z[(b * K + i) * kw], kw)); }
        c.e = BigInt::from_limbs(&ee[b * 8], 8);
        if (aids) (*aids)[lo + b].s_digest = BigInt::from_limbs(&sd[b * 8], 8);
      }
    });
    return out;
  }
  static std::vector<Challenge> challenge_batch_seeded(const std::vector<EncryptionKey>& keys, const VerifierSeed& seed, uint64_t first_index = 0) {
    return challenge_batch_seeded(keys, seed, first_index, nullptr);
  }
  static std::vector<Challenge> challenge_batch_seeded(const std::vector<EncryptionKey>& keys, const VerifierSeed& seed, uint64_t first_index,
                                                       std::vector<VerificationAid>& aids) {
    return challenge_batch_seeded(keys, seed, first_index, &aids);
  }
  // :164-171 against the s of (seed, first_index + b), regenerated and hashed on the GPU: one Result per session.  A digest that is no
  // 256-bit number equals no digest (Err); a session whose seeded challenge panics, panics here.
  static std::vector<Result> verify_batch_seeded(const std::vector<EncryptionKey>& keys, const VerifierSeed& seed, uint64_t first_index,
                                                 const std::vector<CorrectKeyProof>& proofs, size_t K = STATISTICAL_ERROR_FACTOR) {
    Engine& e = Engine::instance();
    if (proofs.size() != keys.size()) throw std::invalid_argument("CorrectKey::verify_batch_seeded: one proof per key");
    std::vector<Result> out(keys.size(), Result(false));
    width_runs(keys, "CorrectKey::verify_batch_seeded", [&](size_t lo, size_t hi, uint32_t nb) {
      const size_t B = hi - lo, kw = nb / 32;
      std::vector<uint32_t> n(B * kw), pd(B * 8, 0);
      std::vector<uint8_t> v(B, 9), fits(B, 0);
      for (size_t b = 0; b < B; b++) {
        keys[lo + b].n.to_limbs(&n[b * kw], kw);
        const BigInt& d = proofs[lo + b].s_digest;
        if ((fits[b] = !d.is_negative() && d.fits_limbs(8))) d.to_limbs(&pd[b * 8], 8);
      }
      e.check(zkp_correct_key_verify_seeded_batch(e.ctx(), nb, B, (uint32_t)K, n.data(), kw, seed.bytes, first_index + lo, pd.data(), v.data(), 0),
              "zkp_correct_key_verify_seeded_batch");
      for (size_t b = 0; b < B; b++)
        out[lo + b] = v[b] == ZKP_VERDICT_MALFORMED ? Result::panicked("CorrectKey::challenge: the key is outside the domain") : Result(fits[b] && v[b] == ZKP_VERDICT_ACCEPT);
    });
    return out;
  }
  // :104-162 for one (key, challenge) pair per session in ONE zkp_correct_key_prove_batch per kernel width (grouped as
  // NiCorrectKeyProof::proof_batch groups them): n, the residues, rn and the n-th roots — CRT under p and q — are computed on the GPU; phi,
  // phi - e mod phi and n^-1 mod phi are never formed, and the staging that carries p and q is wiped on release.  A session the call's shape
  // cannot hold — |sn| != |z|, a number of rounds other than the batch's (that of its first session), e negative or >= 2^256, a value
  // negative or wider than the key's width, a factor that is not positive or wider than 2048 bits — and a key the call reports as outside
  // its domain goes through prove(), the single-session path, unchanged.
  static std::vector<ProveResult> prove_batch(const std::vector<const DecryptionKey*>& keys, const std::vector<Challenge>& challenges) {
    Engine& e = Engine::instance();
    if (keys.size() != challenges.size()) throw std::invalid_argument("CorrectKey::prove_batch: one challenge per key");
    const size_t N = keys.size();
    std::vector<ProveResult> out(N, ProveResult{false, CorrectKeyProof{}, CorrectKeyProveError::EWasntComputedCorrectly});
    const size_t K = N ? challenges[0].sn.size() : 0;
    std::vector<uint32_t> width(N, 0);                                                        // 0: the single-session path
    for (size_t k = 0; k < N; k++) {
      const DecryptionKey& dk = *keys[k];
      const Challenge& c = challenges[k];
      if (K < 1 || K > 256 || c.sn.size() != K || c.z.size() != K || c.e.is_negative() || !c.e.fits_limbs(8)) continue;
      if (dk.p.is_negative() || dk.q.is_negative() || dk.p.is_zero() || dk.q.is_zero() || std::max(dk.p.bit_length(), dk.q.bit_length()) > 2048) continue;
      uint32_t nb = width_for(dk.p * dk.q);
      while (std::max(dk.p.bit_length(), dk.q.bit_length()) > nb / 2) nb *= 2;
      bool fits = true;
      for (size_t i = 0; i < K; i++) fits = fits && !c.sn[i].is_negative() && c.sn[i].fits_limbs(nb / 32) && !c.z[i].is_negative() && c.z[i].fits_limbs(nb / 32);
      if (fits) width[k] = nb;
    }
    for (uint32_t nb : {1024u, 2048u, 4096u}) {
      const uint32_t kw = nb / 32, hw = nb / 64;
      std::vector<size_t> idx;
      for (size_t k = 0; k < N; k++) if (width[k] == nb) idx.push_back(k);
      if (idx.empty()) continue;
      const size_t B = idx.size();
      RawBuf<uint32_t> p(B * hw, true), q(B * hw, true);                                      // (secret: wiped on release)
      std::vector<uint32_t> sn(B * K * kw), z(B * K * kw), ee(B * 8), sd(B * 8);
      std::vector<uint8_t> err(B, 9);
      for (size_t j = 0; j < B; j++) {
        const Challenge& c = challenges[idx[j]];
        keys[idx[j]]->p.to_limbs(&p[j * hw], hw); keys[idx[j]]->q.to_limbs(&q[j * hw], hw);
        for (size_t i = 0; i < K; i++) { c.sn[i].to_limbs(&sn[(j * K + i) * kw], kw); c.z[i].to_limbs(&z[(j * K + i) * kw], kw); }
        c.e.to_limbs(&ee[j * 8], 8);
      }
      const int32_t rc = zkp_correct_key_prove_batch(e.ctx(), nb, B, (uint32_t)K, p.data(), q.data(), sn.data(), ee.data(), z.data(), sd.data(), err.data(), 0);
      p.wipe_now(); q.wipe_now();
      e.check(rc, "zkp_correct_key_prove_batch");
      for (size_t j = 0; j < B; j++) {
        if (err[j] == ZKP_CK_PROVE_BAD_KEY) width[idx[j]] = 0;
        else if (err[j] == ZKP_CK_PROVE_OK) out[idx[j]] = ProveResult{true, CorrectKeyProof{BigInt::from_limbs(&sd[j * 8], 8)}, CorrectKeyProveError::EWasntComputedCorrectly};
        else out[idx[j]].err = (CorrectKeyProveError)(err[j] - 1);
      }
    }
    for (size_t k = 0; k < N; k++) if (width[k] == 0) out[k] = prove(*keys[k], challenges[k]);
    return out;
  }
};

// ------------------------------------------------------------------ seeded proving of the sigma proofs (zkp_*_prove_seeded_batch)
// What the prove_batch_seeded functions below share: one fresh 32-byte seed from the operating system per call (RangeProofNi::SeedGuard wipes
// it on every path out), expanded into the proofs' nonces ON THE GPU — the stream is defined in include/zkp_hip.h.  No nonce is sampled,
// flattened or kept on the host; the buffers that carry the caller's secrets to the GPU are wiped when they are released.
namespace detail {
// the keys of a batch as one array: [1][kw] with stride 0 when every statement names the same n, else [B][kw]; every key takes one kernel width
struct BatchKeys {
  uint32_t nb = 0, kw = 0;
  uint64_t stride = 0;
  std::vector<uint32_t> n;
  template <class It, class GetN> BatchKeys(It first, It last, GetN get) {
    bool shared = true;
    for (It it = first; it != last; ++it) {
      const uint32_t w = width_for(get(*it));
      if (nb && w != nb) throw std::invalid_argument("prove_batch_seeded: the keys of one batch must share a kernel width");
      nb = w;
      shared = shared && get(*it) == get(*first);
    }
    kw = nb / 32;
    const size_t rows = shared ? 1 : (size_t)(last - first);
    stride = shared ? 0 : kw;
    n.resize(rows * kw);
    for (size_t i = 0; i < rows; i++) get(first[i]).to_limbs(&n[i * kw], kw);
  }
};
inline void seeded_status_ok(const std::vector<uint8_t>& status, const char* what) {
  for (uint8_t s : status) if (s != 0) throw Panic(what);
}
}  // namespace detail

// ------------------------------------------------------------------ CompositeDLogProof
struct DLogStatement {                        // wi_dlog_proof.rs:38-43
  BigInt N, g, ni;
  // What the reference's tests do before CompositeDLogProof::prove (wi_dlog_proof.rs:117-141, "per definition 3 in the paper"), for a whole
  // batch of moduli and without their factors: g = h1 with Jacobi symbol (h1 / N) == -1, secret < 2^256, ni = (h1^-1)^secret mod N — from
  // one fresh OS seed expanded ON THE GPU (zkp_dlog_statement_setup_seeded_batch; the seed is worth the secrets and is wiped on every path
  // out, the secrets travel in a column that is wiped on release).  -> (statements, secrets), one each per modulus.
  // Panic where a modulus has no such h1: N zero or even, or a square (the reference's loop would not end).
  static std::pair<std::vector<DLogStatement>, std::vector<BigInt>> generate_batch_seeded(const std::vector<BigInt>& N);
};

class CompositeDLogProof {
 public:
  static constexpr uint32_t Y_BITS = 768;     // y = r + e*s < 2^513 for honest provers
  BigInt x, y;
  // wi_dlog_proof.rs:46-65
  static CompositeDLogProof prove(const DLogStatement& st, const BigInt& secret);
  // prove for a whole batch from what the reference's prove takes: the 512-bit nonces come from one OS seed, expanded on the GPU
  static std::vector<CompositeDLogProof> prove_batch_seeded(const std::vector<DLogStatement>& st, const std::vector<BigInt>& secrets);
  static std::vector<CompositeDLogProof> prove_impl(const DLogStatement* st, const BigInt* secrets, size_t B, bool seeded);
  // base^exp mod N for a non-negative exponent of ANY length (a prover-chosen y is not bounded): exponents wider than the modulus
  // width go through the GPU in chunks, acc = acc^(2^c) * base^chunk, most significant chunk first
  static BigInt mod_pow_wide(const BigInt& base, const BigInt& exp, const BigInt& N) {
    const size_t mb = N.bit_length() <= 2048 ? 2048 : N.bit_length() <= 4096 ? 4096 : 8192, chunk = mb - 32;
    if (exp.bit_length() <= mb) return mod_pow(base, exp, N);
    BigInt acc = BigInt::one();
    for (size_t hi = (exp.bit_length() + chunk - 1) / chunk; hi-- > 0;) {
      BigInt part;
      for (size_t b = 0; b < chunk; b++) if (exp.bit(hi * chunk + b)) part = part + BigInt::pow2(b);
      acc = (mod_pow(acc, BigInt::pow2(chunk), N) * mod_pow(base, part, N)).modulus(N);
    }
    return acc;
  }
  // wi_dlog_proof.rs:67-91.  Honest shapes (x, g, ni < N, 0 <= y < 2^768) go to zkp_dlog_verify_batch.  Anything else a received proof
  // or statement may hold — an over-wide y (y = r + e s is not bounded by the reference), g / ni / x that are negative or >= N — is
  // evaluated as the reference does it: the pre-checks and the hash (over the RAW values' magnitudes) on the host, the two
  // exponentiations on the GPU (mod_pow reduces its base into [0, N), as mpz_powm does), mod_mul and the compare on the host.
  // Not carried: a modulus the engine cannot take (even, or wider than 4096 bits) and a NEGATIVE y ([upstream] mod_pow with a negative
  // exponent: inverse or panic, not recalled with confidence): Result::unsupported.
  Result verify(const DLogStatement& st) const {
    Engine& e = Engine::instance();
    if (st.N.is_negative() || st.N <= BigInt::pow2(128)) throw Panic("assertion failed: statement.N > BigInt::from(2).pow(K as u32)");   // :69
    if (!st.N.is_odd() || st.N.bit_length() > 4096) return Result::unsupported("CompositeDLogProof::verify: the modulus is even or wider than 4096 bits");
    const uint32_t nb = width_for(st.N), kw = nb / 32;
    const bool canonical = !st.g.is_negative() && st.g < st.N && !st.ni.is_negative() && st.ni < st.N && x.fits_limbs(kw) && y.fits_limbs(Y_BITS / 32);
    if (!canonical) {
      if (y.is_negative()) return Result::unsupported("CompositeDLogProof::verify: negative response y");
      if (BigInt::gcd(st.g, st.N) != BigInt::one() || BigInt::gcd(st.ni, st.N) != BigInt::one())
        throw Panic("assertion failed: `(left == right)` gcd(g, N) / gcd(ni, N)");                                      // :72-73
      const BigInt ee = detail::compute_digest({&x, &st.g, &st.N, &st.ni});                                               // :75-80
      const BigInt ni_e = mod_pow(st.ni, ee, st.N), g_y = mod_pow_wide(st.g, y, st.N);                                    // :81-82
      return Result(x == (g_y * ni_e).modulus(st.N));                                                                     // :83-90
    }
    Columns in(1, {{kw, false}, {kw, false}, {kw, false}, {kw, false}, {Y_BITS / 32, false}});
    in.put_row(0, {&st.N, &st.g, &st.ni, &x, &y});
    uint8_t v = 9;
    e.check(zkp_dlog_verify_batch(e.ctx(), nb, Y_BITS, 1, in[0], in[1], in[2], in[3], in[4], &v, 0), "zkp_dlog_verify_batch");
    if (v == ZKP_VERDICT_MALFORMED) throw Panic("assertion failed in CompositeDLogProof::verify (N > 2^128, gcd(g,N) = gcd(ni,N) = 1)");   // :69,72,73
    return Result(v == ZKP_VERDICT_ACCEPT);
  }
  // serde_json::from_str of both documents + verify for whole batches, one Result per (statement, proof) pair: zkp_dlog_verify_json_batch
  // scans, converts, range-checks and verifies on the GPU.  A pair it hands back (ZKP_DOC_HOST_PATH: a field the fixed layout cannot
  // carry, an even N, g / ni / x >= N) is parsed here and goes through verify() above, so the caller gets the reference's answer for it;
  // a document that is no value of its type is the panic `from_str(..).unwrap()` is in the reference, and so are verify's assertions.
  // bare_form: ZKP_BIGINT_DEC / _HEX / _BYTES, the text form of every integer of the batch.
  static std::vector<Result> verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t bare_form = ZKP_BIGINT_DEC);
};

// ------------------------------------------------------------------ ZeroProof (src/zkproofs/zero_enc_proof.rs:26-95)
struct ZeroWitness { BigInt r; };
struct ZeroStatement { EncryptionKey ek; BigInt c; };
class ZeroProof {
 public:
  BigInt z, a;
  static ZeroProof prove(const ZeroWitness& w, const ZeroStatement& st);   // :44-64
  // prove for a whole batch from what the reference's prove takes: every r' comes from one OS seed, expanded on the GPU
  static std::vector<ZeroProof> prove_batch_seeded(const std::vector<ZeroWitness>& w, const std::vector<ZeroStatement>& st);
  static std::vector<ZeroProof> prove_impl(const ZeroWitness* w, const ZeroStatement* st, size_t B, bool seeded);
  Result verify(const ZeroStatement& st) const;   // :66-94
  // serde_json::from_str of both documents + verify for whole batches, one Result per (statement, proof) pair: zkp_sigma_verify_json_batch reads,
  // checks and verifies on the GPU.  forms = ZKP_BIGINT_FORMS(key_form, bare_form).  A document that is no value of its type is the panic of
  // `from_str(..).unwrap()`; a pair the limb kernels are not specified for (ZKP_DOC_HOST_PATH) is Result::unsupported naming the reason.
  static std::vector<Result> verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms = 0);
};

// ------------------------------------------------------------------ CiphertextProof (src/zkproofs/correct_ciphertext.rs:23-98)
struct CiphertextWitness { BigInt x, r; };
struct CiphertextStatement { EncryptionKey ek; BigInt c; };
class CiphertextProof {
 public:
  BigInt z1, z2, c_prime;
  static CiphertextProof prove(const CiphertextWitness& w, const CiphertextStatement& st);   // :42-64
  // prove for a whole batch from what the reference's prove takes: every (x', r') comes from one OS seed, expanded on the GPU
  static std::vector<CiphertextProof> prove_batch_seeded(const std::vector<CiphertextWitness>& w, const std::vector<CiphertextStatement>& st);
  static std::vector<CiphertextProof> prove_impl(const CiphertextWitness* w, const CiphertextStatement* st, size_t B, bool seeded);
  Result verify(const CiphertextStatement& st) const;   // :66-97
  // serde_json::from_str of both documents + verify for whole batches, one Result per (statement, proof) pair: zkp_sigma_verify_json_batch reads,
  // checks and verifies on the GPU.  forms = ZKP_BIGINT_FORMS(key_form, bare_form).  A document that is no value of its type is the panic of
  // `from_str(..).unwrap()`; a pair the limb kernels are not specified for (ZKP_DOC_HOST_PATH) is Result::unsupported naming the reason.
  static std::vector<Result> verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms = 0);
};

// ------------------------------------------------------------------ VerlinProof (src/zkproofs/verlin_proof.rs:35-165)
struct VerlinWitness { BigInt x, x_prime, x_double_prime, r_x; };
struct VerlinStatement { EncryptionKey ek; BigInt c, c_prime, phi_x; };

// gen_phi (verlin_proof.rs:138-165) = c^y * c'^y' * Enc(y'', r_y) mod n^2, from three batched GPU calls
inline BigInt gen_phi(const EncryptionKey& ek, const BigInt& c, const BigInt& c_prime, const BigInt& y, const BigInt& y_prime,
                      const BigInt& y_double_prime, const BigInt& r_y) {
  std::vector<BigInt> p = mod_pow_batch({c, c_prime}, {y, y_prime}, ek.nn);
  BigInt e3 = Paillier::encrypt_with_chosen_randomness(ek, y_double_prime % ek.n, r_y);   // (1 + m n) mod n^2 depends on m mod n only; r_y < n for honest callers
  return ((p[0] * p[1]) % ek.nn) * e3 % ek.nn;
}

class VerlinProof {
 public:
  BigInt phi_a, z, z_prime, z_double_prime, r_z;
  static VerlinProof prove(const VerlinWitness& w, const VerlinStatement& st);   // :60-99
  // prove for a whole batch from what the reference's prove takes: every (a, a', a'', r_a) comes from one OS seed, expanded on the GPU — r_a
  // redrawn there until gcd(r_a, n) == 1 (:64-67; the rule is sample_coprime_below of include/zkp_hip.h)
  static std::vector<VerlinProof> prove_batch_seeded(const std::vector<VerlinWitness>& w, const std::vector<VerlinStatement>& st);
  static std::vector<VerlinProof> prove_impl(const VerlinWitness* w, const VerlinStatement* st, size_t B, bool seeded);
  Result verify(const VerlinStatement& st) const;   // :101-135
  // serde_json::from_str of both documents + verify for whole batches, one Result per (statement, proof) pair: zkp_sigma_verify_json_batch reads,
  // checks and verifies on the GPU.  forms = ZKP_BIGINT_FORMS(key_form, bare_form).  A document that is no value of its type is the panic of
  // `from_str(..).unwrap()`; a pair the limb kernels are not specified for (ZKP_DOC_HOST_PATH) is Result::unsupported naming the reason.
  static std::vector<Result> verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms = 0);
};

// ------------------------------------------------------------------ BigInt::mod_inv (batched on the GPU)
// None (std::nullopt-like: empty vector entry flagged) when no inverse exists; throws std::domain_error outside the ABI's domain
struct ModInvResult { bool some; BigInt value; };
inline std::vector<ModInvResult> mod_inv_batch(const std::vector<BigInt>& a, const BigInt& modulus) {
  Engine& e = Engine::instance();
  uint32_t mb = width_for(modulus); if (mb < 2048) mb = 2048;
  const size_t L = mb / 32, cnt = a.size();
  std::vector<uint32_t> av(cnt * L), mv(L), out(cnt * L);
  std::vector<uint8_t> stv(cnt);
  modulus.to_limbs(mv.data(), L);
  for (size_t i = 0; i < cnt; i++) (a[i] % modulus).to_limbs(&av[i * L], L);
  if (cnt) e.check(zkp_modinv_batch(e.ctx(), mb, cnt, av.data(), mv.data(), 0, out.data(), stv.data(), 0), "zkp_modinv_batch");
  std::vector<ModInvResult> r;
  for (size_t i = 0; i < cnt; i++) {
    if (stv[i] == ZKP_INV_DOMAIN) throw std::domain_error("mod_inv: even or trivial modulus");
    r.push_back({stv[i] == ZKP_INV_OK, BigInt::from_limbs(&out[i * L], L)});
  }
  return r;
}

// ------------------------------------------------------------------ MulProof (src/zkproofs/multiplication_proof.rs)
struct MulWitness { BigInt a, b, c, r_a, r_b, r_c; };          // :42-50
struct MulStatement { EncryptionKey ek; BigInt e_a, e_b, e_c; };   // :52-58
inline BigInt sample_paillier_random(const BigInt& modulo) {    // :148-154
  BigInt r = BigInt::sample_below(modulo);
  while (BigInt::gcd(r, modulo) != BigInt::one()) r = BigInt::sample_below(modulo);
  return r;
}
class MulProof {
 public:
  BigInt f, z1, z2, e_d, e_db;
  static MulProof prove(const MulWitness& w, const MulStatement& st);   // :60-104
  // prove for a whole batch from what the reference's prove takes: every (d, r_d) comes from one OS seed, expanded on the GPU — r_d
  // redrawn there until gcd(r_d, n) == 1 (sample_paillier_random, :148-154; the rule is sample_coprime_below of include/zkp_hip.h)
  static std::vector<MulProof> prove_batch_seeded(const std::vector<MulWitness>& w, const std::vector<MulStatement>& st);
  static std::vector<MulProof> prove_impl(const MulWitness* w, const MulStatement* st, size_t B, bool seeded);
  Result verify(const MulStatement& st) const;   // :106-146
  // serde_json::from_str of both documents + verify for whole batches, one Result per (statement, proof) pair: zkp_sigma_verify_json_batch reads,
  // checks and verifies on the GPU.  forms = ZKP_BIGINT_FORMS(key_form, bare_form).  A document that is no value of its type is the panic of
  // `from_str(..).unwrap()`; a pair the limb kernels are not specified for (ZKP_DOC_HOST_PATH) is Result::unsupported naming the reason.
  static std::vector<Result> verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms = 0);
};

// ------------------------------------------------------------------ CorrectMessageProof (src/zkproofs/correct_message.rs)
class CorrectMessageProof {
 public:
  std::vector<BigInt> e_vec, z_vec, a_vec;
  BigInt ciphertext;
  std::vector<BigInt> valid_messages;
  EncryptionKey ek;
  static constexpr size_t B = 256;   // :19
  static CorrectMessageProof prove(const EncryptionKey& ek, const std::vector<BigInt>& valid_messages, const BigInt& message_to_encrypt) {   // :35-123
    return prove_impl(ek, &valid_messages, &message_to_encrypt, 1, false)[0];
  }
  // prove for a whole batch under one key from what the reference's prove takes: r, w and the simulated (e_j, z_j) of every proof come from
  // one OS seed, expanded on the GPU.  Every proof of the batch has the same number of valid messages.
  static std::vector<CorrectMessageProof> prove_batch_seeded(const EncryptionKey& ek, const std::vector<std::vector<BigInt>>& valid_messages,
                                                             const std::vector<BigInt>& messages_to_encrypt) {
    if (valid_messages.size() != messages_to_encrypt.size()) throw std::invalid_argument("CorrectMessageProof::prove_batch_seeded: one message per list");
    if (valid_messages.empty()) return {};
    for (auto& v : valid_messages) if (v.size() != valid_messages[0].size()) throw std::invalid_argument("CorrectMessageProof::prove_batch_seeded: lists of one length per batch");
    return prove_impl(ek, valid_messages.data(), messages_to_encrypt.data(), valid_messages.size(), true);
  }
  // Bn proofs of K valid messages each.  Columns: the key; per proof the message (secret) and the ciphertext; per (proof, message) the
  // valid message and the proof's (e, z, a).
  static std::vector<CorrectMessageProof> prove_impl(const EncryptionKey& ek, const std::vector<BigInt>* valid_messages, const BigInt* messages, size_t Bn, bool seeded) {
    const size_t K = valid_messages[0].size();
    if (K == 0) throw Panic("attempt to subtract with overflow (num_of_message - 1, correct_message.rs:58)");
    Engine& e = Engine::instance();
    RangeProofNi::SeedGuard seed(seeded);
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    Columns key(1, {{kw, false}}), msg(Bn, {{kw, true}}), valid(Bn * K, {{kw, false}}), ct(Bn, {{2 * kw, false}}), rows(Bn * K, {{8, false}, {kw, false}, {2 * kw, false}});
    key.put(0, 0, ek.n);
    for (size_t b = 0; b < Bn; b++) {
      msg.put(b, 0, messages[b]);
      for (size_t i = 0; i < K; i++) valid.put(b * K + i, 0, valid_messages[b][i]);
    }
    std::vector<uint8_t> status(Bn, 9);
    if (seeded)
      e.check(zkp_correct_message_prove_seeded_batch(e.ctx(), nb, Bn, (uint32_t)K, key[0], 0, valid[0], msg[0], seed.bytes, 0, ct[0], rows[0], rows[1], rows[2], status.data(), 0),
              "zkp_correct_message_prove_seeded_batch");
    else {
      Columns nonce(Bn, {{kw, true}, {kw, true}}), sim(Bn * (K - 1) + 1, {{8, true}, {kw, true}});      // (one spare row: K = 1 simulates nothing)
      for (size_t f = 0; f < 2; f++) for (size_t b = 0; b < Bn; b++) nonce.put(b, f, BigInt::sample_below(ek.n));   // r, w: :43, :65
      for (size_t j = 0; j < Bn * (K - 1); j++) { sim.put(j, 0, BigInt::sample(B)); sim.put(j, 1, BigInt::sample_below(ek.n)); }      // the simulated (e_j, z_j), :59-64
      sim.put(Bn * (K - 1), 0, BigInt()); sim.put(Bn * (K - 1), 1, BigInt());
      e.check(zkp_correct_message_prove_batch(e.ctx(), nb, Bn, (uint32_t)K, key[0], 0, valid[0], msg[0], nonce[0], sim[0], sim[1], nonce[1], ct[0], rows[0], rows[1], rows[2],
                                              status.data(), 0), "zkp_correct_message_prove_batch");
    }
    detail::seeded_status_ok(status, "index out of bounds (correct_message.rs:72: no valid message equals the encrypted one)");
    std::vector<CorrectMessageProof> out(Bn);
    for (size_t b = 0; b < Bn; b++) {
      CorrectMessageProof& p = out[b];
      p.ciphertext = ct.get(b, 0); p.valid_messages = valid_messages[b]; p.ek = ek;
      for (size_t i = 0; i < K; i++) { p.e_vec.push_back(rows.get(b * K + i, 0)); p.z_vec.push_back(rows.get(b * K + i, 1)); p.a_vec.push_back(rows.get(b * K + i, 2)); }
    }
    return out;
  }
  Result verify() const {                                                 // :124-162
    Engine& e = Engine::instance();
    const uint32_t nb = width_for(ek.n), kw = nb / 32;
    const size_t K = valid_messages.size();
    if (e_vec.size() < K || z_vec.size() < K || a_vec.size() < K) throw Panic("index out of bounds");
    Columns head(1, {{kw, false}, {2 * kw, false}}), rows(K, {{kw, false}, {8, false}, {kw, false}, {2 * kw, false}});
    head.put_row(0, {&ek.n, &ciphertext});
    for (size_t i = 0; i < K; i++) rows.put_row(i, {&valid_messages[i], &e_vec[i], &z_vec[i], &a_vec[i]});
    uint8_t v = 9;
    e.check(zkp_correct_message_verify_batch(e.ctx(), nb, 1, (uint32_t)K, head[0], 0, rows[0], head[1], rows[1], rows[2], rows[3], &v, 0), "zkp_correct_message_verify_batch");
    if (v == ZKP_VERDICT_MALFORMED) throw Panic("assertion failed: `(left == right)` chal / ei_sum (correct_message.rs:132)");
    return Result(v == ZKP_VERDICT_ACCEPT);
  }
};

// ------------------------------------------------------------------ the sigma proofs: one field table per type
// ZeroProof, CiphertextProof, VerlinProof, MulProof, their statements and their witnesses (zero_enc_proof.rs:26-41, correct_ciphertext.rs:22-39,
// verlin_proof.rs:34-57, multiplication_proof.rs:32-57), every field with its width in the batch layout, in declaration order.  The tables
// flatten a batch into Columns for the C ABI and read one back (prove, prove_batch_seeded, verify below), and they are the serde defaults of
// the derives for the documents (serde_json::to_string, sigma_from_str, to_string_batch, verify_json_batch): a statement's key is the
// object "ek" with the field "n" in the key form; every other field is a bare BigInt.  A witness has no document form; its columns are secret.
namespace detail {
enum class SigmaWidth { N, NN, Z };          // kw | 2 kw | kw + ZKP_Z1_EXTRA_LIMBS words in the batch layout
struct SigmaField { const char* name; BigInt* v; SigmaWidth w; bool key; };
template <class T> struct SigmaDoc;
#define ZKP_SIGMA_DOC(T, KIND, SECRET, ...)                                                                     \
  template <> struct SigmaDoc<T> {                                                                              \
    static constexpr uint32_t kind = KIND;                                                                      \
    static constexpr bool secret = SECRET;                                                                      \
    static constexpr const char* type = #T;                                                                     \
    static std::vector<SigmaField> fields(T& d) { return __VA_ARGS__; }                                         \
  };
ZKP_SIGMA_DOC(ZeroStatement, ZKP_JSON_DOC_ZERO_STATEMENT, false, {{"ek", &d.ek.n, SigmaWidth::N, true}, {"c", &d.c, SigmaWidth::NN, false}})
ZKP_SIGMA_DOC(ZeroProof, ZKP_JSON_DOC_ZERO_PROOF, false, {{"z", &d.z, SigmaWidth::NN, false}, {"a", &d.a, SigmaWidth::NN, false}})
ZKP_SIGMA_DOC(CiphertextStatement, ZKP_JSON_DOC_CIPHERTEXT_STATEMENT, false, {{"ek", &d.ek.n, SigmaWidth::N, true}, {"c", &d.c, SigmaWidth::NN, false}})
ZKP_SIGMA_DOC(CiphertextProof, ZKP_JSON_DOC_CIPHERTEXT_PROOF, false,
              {{"z1", &d.z1, SigmaWidth::Z, false}, {"z2", &d.z2, SigmaWidth::NN, false}, {"c_prime", &d.c_prime, SigmaWidth::NN, false}})
ZKP_SIGMA_DOC(VerlinStatement, ZKP_JSON_DOC_VERLIN_STATEMENT, false,
              {{"ek", &d.ek.n, SigmaWidth::N, true}, {"c", &d.c, SigmaWidth::NN, false}, {"c_prime", &d.c_prime, SigmaWidth::NN, false}, {"phi_x", &d.phi_x, SigmaWidth::NN, false}})
ZKP_SIGMA_DOC(VerlinProof, ZKP_JSON_DOC_VERLIN_PROOF, false,
              {{"phi_a", &d.phi_a, SigmaWidth::NN, false}, {"z", &d.z, SigmaWidth::Z, false}, {"z_prime", &d.z_prime, SigmaWidth::Z, false},
               {"z_double_prime", &d.z_double_prime, SigmaWidth::Z, false}, {"r_z", &d.r_z, SigmaWidth::NN, false}})
ZKP_SIGMA_DOC(MulStatement, ZKP_JSON_DOC_MUL_STATEMENT, false,
              {{"ek", &d.ek.n, SigmaWidth::N, true}, {"e_a", &d.e_a, SigmaWidth::NN, false}, {"e_b", &d.e_b, SigmaWidth::NN, false}, {"e_c", &d.e_c, SigmaWidth::NN, false}})
ZKP_SIGMA_DOC(MulProof, ZKP_JSON_DOC_MUL_PROOF, false,
              {{"f", &d.f, SigmaWidth::N, false}, {"z1", &d.z1, SigmaWidth::NN, false}, {"z2", &d.z2, SigmaWidth::NN, false}, {"e_d", &d.e_d, SigmaWidth::NN, false},
               {"e_db", &d.e_db, SigmaWidth::NN, false}})
// the witnesses as the prove entry points take them (MulWitness::c is not an input of the proof: multiplication_proof.rs:60-104 never reads it)
ZKP_SIGMA_DOC(ZeroWitness, 0, true, {{"r", &d.r, SigmaWidth::N, false}})
ZKP_SIGMA_DOC(CiphertextWitness, 0, true, {{"x", &d.x, SigmaWidth::N, false}, {"r", &d.r, SigmaWidth::N, false}})
ZKP_SIGMA_DOC(VerlinWitness, 0, true,
              {{"x", &d.x, SigmaWidth::N, false}, {"x_prime", &d.x_prime, SigmaWidth::N, false}, {"x_double_prime", &d.x_double_prime, SigmaWidth::N, false},
               {"r_x", &d.r_x, SigmaWidth::N, false}})
ZKP_SIGMA_DOC(MulWitness, 0, true,
              {{"a", &d.a, SigmaWidth::N, false}, {"b", &d.b, SigmaWidth::N, false}, {"r_a", &d.r_a, SigmaWidth::N, false}, {"r_b", &d.r_b, SigmaWidth::N, false},
               {"r_c", &d.r_c, SigmaWidth::N, false}})
#undef ZKP_SIGMA_DOC
inline size_t sigma_words(SigmaWidth w, uint32_t kw) { return w == SigmaWidth::N ? kw : w == SigmaWidth::NN ? 2 * kw : kw + ZKP_Z1_EXTRA_LIMBS; }

// The columns of B values of T at kw limbs: one per field of the table — without the key unless with_key (the prove and verify entry
// points take the keys as an array of their own, BatchKeys; a document writer takes it as field 0).
template <class T> std::vector<Column> sigma_layout(uint32_t kw, bool with_key = false) {
  T proto;
  std::vector<Column> cols;
  for (const SigmaField& f : SigmaDoc<T>::fields(proto)) if (with_key || !f.key) cols.push_back({sigma_words(f.w, kw), SigmaDoc<T>::secret});
  return cols;
}
template <class T> Columns sigma_flatten(const T* v, size_t B, uint32_t kw, bool with_key = false) {
  Columns c(B, sigma_layout<T>(kw, with_key));
  for (size_t b = 0; b < B; b++) {
    size_t k = 0;
    for (const SigmaField& f : SigmaDoc<T>::fields(const_cast<T&>(v[b]))) if (with_key || !f.key) c.put(b, k++, *f.v);
  }
  return c;
}
template <class T> std::vector<T> sigma_read(const Columns& c) {
  std::vector<T> out(c.B);
  for (size_t b = 0; b < c.B; b++) {
    size_t k = 0;
    for (const SigmaField& f : SigmaDoc<T>::fields(out[b])) *f.v = c.get(b, k++);
  }
  return out;
}
// B nonces per column, each sample(b) — secret columns, wiped on release
template <class F> void sample_column(Columns& c, size_t f, F sample) { for (size_t b = 0; b < c.B; b++) c.put(b, f, sample(b)); }
struct KeyOfStatement { template <class S> const BigInt& operator()(const S& s) const { return s.ek.n; } };
}  // namespace detail

// prove, prove_batch_seeded and verify of every class are the same three steps: the columns from the tables, the ONE call, the result
// columns back.  prove is the batch of one with nonces sampled here (into secret columns); prove_batch_seeded hands a seed over instead.

// ---- ZeroProof (zero_enc_proof.rs:44-94)
inline std::vector<ZeroProof> ZeroProof::prove_impl(const ZeroWitness* w, const ZeroStatement* st, size_t B, bool seeded) {
  if (B == 0) return {};
  Engine& e = Engine::instance();
  RangeProofNi::SeedGuard seed(seeded);
  const detail::BatchKeys keys(st, st + B, detail::KeyOfStatement());
  const uint32_t nb = keys.nb, kw = keys.kw;
  std::vector<ZeroWitness> reduced(B);
  for (size_t b = 0; b < B; b++) reduced[b].r = w[b].r % st[b].ek.nn;
  Columns S = detail::sigma_flatten(st, B, kw), W = detail::sigma_flatten(reduced.data(), B, kw), P(B, detail::sigma_layout<ZeroProof>(kw));
  std::vector<uint8_t> status(B, seeded ? 9 : 0);
  if (seeded)
    e.check(zkp_zero_proof_prove_seeded_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], W[0], seed.bytes, 0, P[0], P[1], status.data(), 0), "zkp_zero_proof_prove_seeded_batch");
  else {
    Columns nonce(B, {{kw, true}});
    detail::sample_column(nonce, 0, [&](size_t b) { return BigInt::sample_below(st[b].ek.n); });                // r', :45
    e.check(zkp_zero_proof_prove_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], W[0], nonce[0], P[0], P[1], 0), "zkp_zero_proof_prove_batch");
  }
  detail::seeded_status_ok(status, "BigInt::sample_below(0) (zero_enc_proof.rs:45)");
  return detail::sigma_read<ZeroProof>(P);
}
inline ZeroProof ZeroProof::prove(const ZeroWitness& w, const ZeroStatement& st) { return prove_impl(&w, &st, 1, false)[0]; }
inline std::vector<ZeroProof> ZeroProof::prove_batch_seeded(const std::vector<ZeroWitness>& w, const std::vector<ZeroStatement>& st) {
  if (w.size() != st.size()) throw std::invalid_argument("ZeroProof::prove_batch_seeded: one witness per statement");
  return prove_impl(w.data(), st.data(), st.size(), true);
}
inline Result ZeroProof::verify(const ZeroStatement& st) const {
  Engine& e = Engine::instance();
  const detail::BatchKeys keys(&st, &st + 1, detail::KeyOfStatement());
  Columns S = detail::sigma_flatten(&st, 1, keys.kw), P = detail::sigma_flatten(this, 1, keys.kw);
  uint8_t v = 9;
  e.check(zkp_zero_proof_verify_batch(e.ctx(), keys.nb, 1, keys.n.data(), 0, S[0], P[0], P[1], &v, 0), "zkp_zero_proof_verify_batch");
  return Result(v == ZKP_VERDICT_ACCEPT);
}

// ---- CiphertextProof (correct_ciphertext.rs:42-97)
inline std::vector<CiphertextProof> CiphertextProof::prove_impl(const CiphertextWitness* w, const CiphertextStatement* st, size_t B, bool seeded) {
  if (B == 0) return {};
  Engine& e = Engine::instance();
  RangeProofNi::SeedGuard seed(seeded);
  const detail::BatchKeys keys(st, st + B, detail::KeyOfStatement());
  const uint32_t nb = keys.nb, kw = keys.kw;
  Columns S = detail::sigma_flatten(st, B, kw), W = detail::sigma_flatten(w, B, kw), P(B, detail::sigma_layout<CiphertextProof>(kw));
  std::vector<uint8_t> status(B, seeded ? 9 : 0);
  if (seeded)
    e.check(zkp_ciphertext_proof_prove_seeded_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], W[0], W[1], seed.bytes, 0, P[0], P[1], P[2], status.data(), 0),
            "zkp_ciphertext_proof_prove_seeded_batch");
  else {
    Columns nonce(B, {{kw, true}, {kw, true}});
    for (size_t f = 0; f < 2; f++) detail::sample_column(nonce, f, [&](size_t b) { return BigInt::sample_below(st[b].ek.n); });   // x', r', :43-44
    e.check(zkp_ciphertext_proof_prove_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], W[0], W[1], nonce[0], nonce[1], P[0], P[1], P[2], 0),
            "zkp_ciphertext_proof_prove_batch");
  }
  detail::seeded_status_ok(status, "BigInt::sample_below(0) (correct_ciphertext.rs:43)");
  return detail::sigma_read<CiphertextProof>(P);
}
inline CiphertextProof CiphertextProof::prove(const CiphertextWitness& w, const CiphertextStatement& st) { return prove_impl(&w, &st, 1, false)[0]; }
inline std::vector<CiphertextProof> CiphertextProof::prove_batch_seeded(const std::vector<CiphertextWitness>& w, const std::vector<CiphertextStatement>& st) {
  if (w.size() != st.size()) throw std::invalid_argument("CiphertextProof::prove_batch_seeded: one witness per statement");
  return prove_impl(w.data(), st.data(), st.size(), true);
}
inline Result CiphertextProof::verify(const CiphertextStatement& st) const {
  Engine& e = Engine::instance();
  const detail::BatchKeys keys(&st, &st + 1, detail::KeyOfStatement());
  Columns S = detail::sigma_flatten(&st, 1, keys.kw), P = detail::sigma_flatten(this, 1, keys.kw);
  uint8_t v = 9;
  e.check(zkp_ciphertext_proof_verify_batch(e.ctx(), keys.nb, 1, keys.n.data(), 0, S[0], P[0], P[1], P[2], &v, 0), "zkp_ciphertext_proof_verify_batch");
  return Result(v == ZKP_VERDICT_ACCEPT);
}

// ---- VerlinProof (verlin_proof.rs:60-135)
inline std::vector<VerlinProof> VerlinProof::prove_impl(const VerlinWitness* w, const VerlinStatement* st, size_t B, bool seeded) {
  if (B == 0) return {};
  Engine& e = Engine::instance();
  RangeProofNi::SeedGuard seed(seeded);
  const detail::BatchKeys keys(st, st + B, detail::KeyOfStatement());
  const uint32_t nb = keys.nb, kw = keys.kw;
  Columns S = detail::sigma_flatten(st, B, kw), W = detail::sigma_flatten(w, B, kw), P(B, detail::sigma_layout<VerlinProof>(kw));
  std::vector<uint8_t> status(B, seeded ? 9 : 0);
  if (seeded)
    e.check(zkp_verlin_proof_prove_seeded_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], S[1], S[2], W[0], W[1], W[2], W[3], seed.bytes, 0, P[0], P[1], P[2], P[3], P[4],
                                                status.data(), 0), "zkp_verlin_proof_prove_seeded_batch");
  else {
    Columns nonce(B, {{kw, true}, {kw, true}, {kw, true}, {kw, true}});
    for (size_t f = 0; f < 3; f++) detail::sample_column(nonce, f, [&](size_t b) { return BigInt::sample_below(st[b].ek.n); });   // a, a', a'', :61-63
    detail::sample_column(nonce, 3, [&](size_t b) { return sample_paillier_random(st[b].ek.n); });                                // r_a coprime to n, :64-67
    e.check(zkp_verlin_proof_prove_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], S[1], S[2], W[0], W[1], W[2], W[3], nonce[0], nonce[1], nonce[2], nonce[3],
                                         P[0], P[1], P[2], P[3], P[4], 0), "zkp_verlin_proof_prove_batch");
  }
  detail::seeded_status_ok(status, "BigInt::sample_below(0), or no r_a coprime to n (verlin_proof.rs:61-67)");
  return detail::sigma_read<VerlinProof>(P);
}
inline VerlinProof VerlinProof::prove(const VerlinWitness& w, const VerlinStatement& st) { return prove_impl(&w, &st, 1, false)[0]; }
inline std::vector<VerlinProof> VerlinProof::prove_batch_seeded(const std::vector<VerlinWitness>& w, const std::vector<VerlinStatement>& st) {
  if (w.size() != st.size()) throw std::invalid_argument("VerlinProof::prove_batch_seeded: one witness per statement");
  return prove_impl(w.data(), st.data(), st.size(), true);
}
inline Result VerlinProof::verify(const VerlinStatement& st) const {
  Engine& e = Engine::instance();
  const detail::BatchKeys keys(&st, &st + 1, detail::KeyOfStatement());
  Columns S = detail::sigma_flatten(&st, 1, keys.kw), P = detail::sigma_flatten(this, 1, keys.kw);
  uint8_t v = 9;
  e.check(zkp_verlin_proof_verify_batch(e.ctx(), keys.nb, 1, keys.n.data(), 0, S[0], S[1], S[2], P[0], P[1], P[2], P[3], P[4], &v, 0), "zkp_verlin_proof_verify_batch");
  return Result(v == ZKP_VERDICT_ACCEPT);
}

// ---- MulProof (multiplication_proof.rs:60-146)
inline std::vector<MulProof> MulProof::prove_impl(const MulWitness* w, const MulStatement* st, size_t B, bool seeded) {
  if (B == 0) return {};
  Engine& e = Engine::instance();
  RangeProofNi::SeedGuard seed(seeded);
  const detail::BatchKeys keys(st, st + B, detail::KeyOfStatement());
  const uint32_t nb = keys.nb, kw = keys.kw;
  Columns S = detail::sigma_flatten(st, B, kw), W = detail::sigma_flatten(w, B, kw), P(B, detail::sigma_layout<MulProof>(kw));
  std::vector<uint8_t> status(B, 9);
  if (seeded)
    e.check(zkp_mul_proof_prove_seeded_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], S[1], S[2], W[0], W[1], W[2], W[3], W[4], seed.bytes, 0, P[0], P[1], P[2], P[3], P[4],
                                             status.data(), 0), "zkp_mul_proof_prove_seeded_batch");
  else {
    Columns nonce(B, {{kw, true}, {kw, true}});
    detail::sample_column(nonce, 0, [&](size_t b) { return BigInt::sample_below(st[b].ek.n); });          // d, :61
    detail::sample_column(nonce, 1, [&](size_t b) { return sample_paillier_random(st[b].ek.n); });        // r_d, :62
    e.check(zkp_mul_proof_prove_batch(e.ctx(), nb, B, keys.n.data(), keys.stride, S[0], S[1], S[2], W[0], W[1], W[2], W[3], W[4], nonce[0], nonce[1], P[0], P[1], P[2], P[3], P[4],
                                      status.data(), 0), "zkp_mul_proof_prove_batch");
  }
  detail::seeded_status_ok(status, seeded ? "called `Option::unwrap()` on a `None` value (mod_inv, multiplication_proof.rs:95), or no r_d coprime to n (:148-154)"
                                          : "called `Option::unwrap()` on a `None` value (mod_inv, multiplication_proof.rs:95)");
  return detail::sigma_read<MulProof>(P);
}
inline MulProof MulProof::prove(const MulWitness& w, const MulStatement& st) { return prove_impl(&w, &st, 1, false)[0]; }
inline std::vector<MulProof> MulProof::prove_batch_seeded(const std::vector<MulWitness>& w, const std::vector<MulStatement>& st) {
  if (w.size() != st.size()) throw std::invalid_argument("MulProof::prove_batch_seeded: one witness per statement");
  return prove_impl(w.data(), st.data(), st.size(), true);
}
inline Result MulProof::verify(const MulStatement& st) const {
  Engine& e = Engine::instance();
  const detail::BatchKeys keys(&st, &st + 1, detail::KeyOfStatement());
  Columns S = detail::sigma_flatten(&st, 1, keys.kw), P = detail::sigma_flatten(this, 1, keys.kw);
  uint8_t v = 9;
  e.check(zkp_mul_proof_verify_batch(e.ctx(), keys.nb, 1, keys.n.data(), 0, S[0], S[1], S[2], P[0], P[1], P[2], P[3], P[4], &v, 0), "zkp_mul_proof_verify_batch");
  if (v == ZKP_VERDICT_MALFORMED) throw Panic("called `Option::unwrap()` on a `None` value (mod_inv, multiplication_proof.rs:135)");
  return Result(v == ZKP_VERDICT_ACCEPT);
}

// ---- CompositeDLogProof (wi_dlog_proof.rs:46-65): explicit widths — N, g, ni, x at kw limbs, the secret at 8, the nonce at 16, y at Y_BITS / 32
inline std::vector<CompositeDLogProof> CompositeDLogProof::prove_impl(const DLogStatement* st, const BigInt* secrets, size_t B, bool seeded) {
  if (B == 0) return {};
  Engine& e = Engine::instance();
  RangeProofNi::SeedGuard seed(seeded);
  const detail::BatchKeys keys(st, st + B, [](const DLogStatement& q) -> const BigInt& { return q.N; });
  const uint32_t nb = keys.nb, kw = keys.kw;
  Columns in(B, {{kw, false}, {kw, false}, {kw, false}, {8, true}}), out(B, {{kw, false}, {Y_BITS / 32, false}});
  for (size_t b = 0; b < B; b++) in.put_row(b, {&st[b].N, &st[b].g, &st[b].ni, &secrets[b]});
  if (seeded)
    e.check(zkp_dlog_prove_seeded_batch(e.ctx(), nb, Y_BITS, B, in[0], in[1], in[2], in[3], seed.bytes, 0, out[0], out[1], nullptr, 0), "zkp_dlog_prove_seeded_batch");
  else {
    Columns nonce(B, {{16, true}});
    detail::sample_column(nonce, 0, [](size_t) { return BigInt::sample_below(BigInt::pow2(512)); });     // K + K' + SAMPLE_S = 512, :53-54
    e.check(zkp_dlog_prove_batch(e.ctx(), nb, Y_BITS, B, in[0], in[1], in[2], in[3], nonce[0], out[0], out[1], 0), "zkp_dlog_prove_batch");
  }
  std::vector<CompositeDLogProof> proofs;
  for (size_t b = 0; b < B; b++) proofs.push_back(CompositeDLogProof{out.get(b, 0), out.get(b, 1)});
  return proofs;
}
inline CompositeDLogProof CompositeDLogProof::prove(const DLogStatement& st, const BigInt& secret) { return prove_impl(&st, &secret, 1, false)[0]; }
inline std::vector<CompositeDLogProof> CompositeDLogProof::prove_batch_seeded(const std::vector<DLogStatement>& st, const std::vector<BigInt>& secrets) {
  if (st.size() != secrets.size()) throw std::invalid_argument("CompositeDLogProof::prove_batch_seeded: one secret per statement");
  return prove_impl(st.data(), secrets.data(), st.size(), true);
}

// ---- DLogStatement::generate_batch_seeded, legendre_symbol, jacobi_symbol
inline std::pair<std::vector<DLogStatement>, std::vector<BigInt>> DLogStatement::generate_batch_seeded(const std::vector<BigInt>& N) {
  std::pair<std::vector<DLogStatement>, std::vector<BigInt>> r;
  if (N.empty()) return r;
  DLogSetupBatch q(N);                  // (refuses what the layout cannot carry before the engine or a seed exists)
  Engine& e = Engine::instance();
  RangeProofNi::SeedGuard seed(true);
  e.check(zkp_dlog_statement_setup_seeded_batch(e.ctx(), q.n_bits, q.B, q.N(), seed.bytes, 0, q.g(), q.ni(), q.secret(), q.status.data(), 0),
          "zkp_dlog_statement_setup_seeded_batch");
  if (q.first_failed() != q.B) throw Panic("DLogStatement::generate_batch_seeded: no h1 with Jacobi symbol -1 (N zero, even or a square), statement " + std::to_string(q.first_failed()));
  for (size_t b = 0; b < q.B; b++) {
    r.first.push_back(DLogStatement{N[b], q.out.get(b, 0), q.out.get(b, 1)});
    r.second.push_back(q.out.get(b, 2));
  }
  return r;
}

// The reference's `zkproofs::wi_dlog_proof::legendre_symbol` (wi_dlog_proof.rs:94-107) under its module's name — a namespace of its own, so
// that programs which define a helper of that name next to `using namespace zkproofs` keep compiling — and the Jacobi symbol beside it.
namespace wi_dlog_proof {
// 1 if a^((p - 1) / 2) == 1 mod p, else -1: Euler's criterion, also for a == 0 mod p and for a composite p (both -1), as in the reference.
// Panic where it panics (`mod_inv(2, p).unwrap()` for an even p); std::domain_error for p < 3 or wider than 8192 bits.
inline int legendre_symbol(const BigInt& a, const BigInt& p) {
  if (p.is_negative() || p < BigInt(3) || p.bit_length() > 8192) throw std::domain_error("legendre_symbol: p < 3 or wider than 8192 bits");
  if (!p.is_odd()) throw Panic("called `Option::unwrap()` on a `None` value (mod_inv(2, p), wi_dlog_proof.rs:98)");
  Engine& e = Engine::instance();
  const uint32_t mb = p.bit_length() <= 2048 ? 2048 : p.bit_length() <= 4096 ? 4096 : 8192, L = mb / 32;
  std::vector<uint32_t> av(L), pv(L);
  a.modulus(p).to_limbs(av.data(), L);         // (mod_pow reduces its base, as mpz_powm does)
  p.to_limbs(pv.data(), L);
  int32_t sym = 0;
  uint8_t st = 9;
  e.check(zkp_legendre_batch(e.ctx(), mb, 1, av.data(), pv.data(), 0, &sym, &st, 0), "zkp_legendre_batch");
  if (st != 0) throw std::domain_error("legendre_symbol: outside the domain");
  return sym;
}
// (a / n), the Jacobi symbol: -1, 0 or 1, for an odd n > 0 of at most 8192 bits and any integer a; std::domain_error otherwise
inline int jacobi_symbol(const BigInt& a, const BigInt& n) {
  if (n.is_negative() || n.is_zero() || !n.is_odd() || n.bit_length() > 8192) throw std::domain_error("jacobi_symbol: n is not a positive odd integer of at most 8192 bits");
  Engine& e = Engine::instance();
  const uint32_t mb = n.bit_length() <= 1024 ? 1024 : n.bit_length() <= 2048 ? 2048 : n.bit_length() <= 4096 ? 4096 : 8192, L = mb / 32;
  std::vector<uint32_t> av(L), nv(L);
  a.modulus(n).to_limbs(av.data(), L);         // ((a / n) depends on a mod n only)
  n.to_limbs(nv.data(), L);
  int32_t sym = 0;
  uint8_t st = 9;
  e.check(zkp_jacobi_batch(e.ctx(), mb, 1, av.data(), nv.data(), 0, &sym, &st, 0), "zkp_jacobi_batch");
  if (st != 0) throw std::domain_error("jacobi_symbol: outside the domain");
  return sym;
}
}  // namespace wi_dlog_proof

// ------------------------------------------------------------------ wire format (src/serialize.rs + the serde derives)
// Writers produce what serde_json::to_string produces for the reference's types; readers go through the batched
// ingestion entry points of the C ABI (decimal strings are converted on the GPU).
namespace serde_json {
// BigInt::to_str_radix(10) for many values at once (zkp_limbs_to_decimal_batch)
inline std::vector<std::string> to_decimal(const std::vector<BigInt>& v, uint32_t words) {
  Engine& e = Engine::instance();
  const size_t cnt = v.size();
  const uint32_t pitch = zkp_decimal_pitch(words);
  std::vector<uint32_t> src(cnt * words), len(cnt);
  std::vector<char> txt(cnt * (size_t)pitch);
  for (size_t i = 0; i < cnt; i++) v[i].to_limbs(&src[i * words], words);
  if (cnt) e.check(zkp_limbs_to_decimal_batch(e.ctx(), src.data(), words, words, cnt, txt.data(), pitch, len.data(), 0), "zkp_limbs_to_decimal_batch");
  std::vector<std::string> out;
  for (size_t i = 0; i < cnt; i++) out.emplace_back(&txt[i * (size_t)pitch + pitch - len[i]], len[i]);
  return out;
}
inline std::string vecbigint(const std::vector<std::string>& d, size_t lo, size_t n) {   // serialize.rs:33-46
  std::string s = "[";
  for (size_t i = 0; i < n; i++) { if (i) s += ","; s += "\"" + d[lo + i] + "\""; }
  return s + "]";
}
inline std::string to_string(const EncryptedPairs& p, const EncryptionKey& ek) {          // range_proof.rs:32-39
  const uint32_t w = 2 * width_for(ek.n) / 32;
  std::vector<BigInt> all(p.c1); all.insert(all.end(), p.c2.begin(), p.c2.end());
  auto d = to_decimal(all, w);
  return "{\"c1\":" + vecbigint(d, 0, p.c1.size()) + ",\"c2\":" + vecbigint(d, p.c1.size(), p.c2.size()) + "}";
}
inline std::string to_string(const Proof& p, const EncryptionKey& ek) {                   // range_proof.rs:53-81
  const uint32_t w = width_for(ek.n) / 32;
  std::vector<BigInt> all;
  for (const Response& r : p.responses) {
    if (r.kind == Response::Open) { all.push_back(r.w1); all.push_back(r.r1); all.push_back(r.w2); all.push_back(r.r2); }
    else { all.push_back(r.masked_x); all.push_back(r.masked_r); }
  }
  auto d = to_decimal(all, w);
  std::string s = "[";
  size_t k = 0;
  for (size_t i = 0; i < p.responses.size(); i++) {
    const Response& r = p.responses[i];
    if (i) s += ",";
    if (r.kind == Response::Open) { s += "{\"Open\":{\"w1\":\"" + d[k] + "\",\"r1\":\"" + d[k + 1] + "\",\"w2\":\"" + d[k + 2] + "\",\"r2\":\"" + d[k + 3] + "\"}}"; k += 4; }
    else { s += "{\"Mask\":{\"j\":" + std::to_string((unsigned)r.j) + ",\"masked_x\":\"" + d[k] + "\",\"masked_r\":\"" + d[k + 1] + "\"}}"; k += 2; }
  }
  return s + "]";
}
inline std::string to_string(const NiCorrectKeyProof& p, const EncryptionKey& ek) {       // correct_key_ni.rs:35-39
  auto d = to_decimal(p.sigma_vec, width_for(ek.n) / 32);
  return "{\"sigma_vec\":" + vecbigint(d, 0, d.size()) + "}";
}

// serde_json::from_str for many documents of one shape; an Err (or a value the fixed-width ABI cannot carry) throws
inline std::vector<std::pair<EncryptedPairs, Proof>> range_from_str(const EncryptionKey& ek, size_t error_factor, const std::vector<std::string>& pairs_docs,
                                                                    const std::vector<std::string>& proof_docs) {
  Engine& e = Engine::instance();
  const uint32_t nb = width_for(ek.n), kw = nb / 32;
  const size_t B = pairs_docs.size(), EF = error_factor;
  if (proof_docs.size() != B) throw std::invalid_argument("range_from_str: one EncryptedPairs and one Proof document per proof");
  RangeSlab s(B, EF, kw, RangeSlab::PAIRS | RangeSlab::RESPONSES);
  std::vector<uint8_t> st1(B), st2(B);
  const zkp_range_ni_proofs p = s.abi(nb, nullptr, 0);
  auto run = [&](const std::vector<std::string>& docs, bool proofs, std::vector<uint8_t>& st) {
    std::string text; std::vector<uint64_t> off, len;
    for (auto& d : docs) { off.push_back(text.size()); len.push_back(d.size()); text += d; }
    if (proofs) e.check(zkp_json_range_proof_batch(e.ctx(), text.data(), off.data(), len.data(), &p, st.data(), 0), "zkp_json_range_proof_batch");
    else e.check(zkp_json_encrypted_pairs_batch(e.ctx(), text.data(), off.data(), len.data(), &p, st.data(), 0), "zkp_json_encrypted_pairs_batch");
  };
  run(pairs_docs, false, st1); run(proof_docs, true, st2);
  std::vector<std::pair<EncryptedPairs, Proof>> out(B);
  for (size_t b = 0; b < B; b++) {
    if (st1[b] || st2[b]) throw std::runtime_error("serde_json: document " + std::to_string(b) + " is not a valid EncryptedPairs / Proof of this width");
    s.read_pairs(b, out[b].first); s.read_proof(b, out[b].second);
  }
  return out;
}
inline NiCorrectKeyProof correct_key_from_str_host(const std::string& doc);
inline NiCorrectKeyProof correct_key_from_str(const EncryptionKey& ek, const std::string& doc) {
  Engine& e = Engine::instance();
  const uint32_t nb = width_for(ek.n), kw = nb / 32;
  std::vector<uint32_t> sig(NiCorrectKeyProof::M2 * kw);
  uint64_t off = 0, len = doc.size();
  uint8_t st = 9;
  e.check(zkp_json_correct_key_proof_batch(e.ctx(), doc.data(), &off, &len, nb, 1, sig.data(), &st, 0), "zkp_json_correct_key_proof_batch");
  if (st == ZKP_DOC_HOST_PATH) return correct_key_from_str_host(doc);     // a negative or over-wide root: a valid NiCorrectKeyProof, parsed here
  if (st) throw std::runtime_error("serde_json: not a NiCorrectKeyProof of this width");
  NiCorrectKeyProof p;
  for (size_t i = 0; i < NiCorrectKeyProof::M2; i++) p.sigma_vec.push_back(BigInt::from_limbs(&sig[i * kw], kw));
  return p;
}

// ---- serde_json::from_str::<RangeProofNi> on the HOST, for the documents the GPU reader hands back (status ZKP_DOC_HOST_PATH: a
// well-formed document holding a number the fixed-width ABI cannot carry — negative or over-wide — or another row count).  Numbers
// become signed BigInts of any size, so RangeProofNi::verify_batch gives such a proof the reference's verdict (verify_general).
// encrypted_pairs / proof: decimal strings (serialize.rs:1-78, mpz_set_str: a leading '-' is a sign).  ek.n and the bare BigInts
// range / ciphertext are un-annotated in the reference (range_proof_ni.rs:38-40): their text forms are the caller's to name,
// separately (kzen-paillier's EncryptionKey and curv's BigInt need not agree), as for zkp_json_range_proof_ni_batch.
enum class BigintText { Dec = ZKP_BIGINT_DEC, Hex = ZKP_BIGINT_HEX, Bytes = ZKP_BIGINT_BYTES };
// ---- whole batches: zkp_json_write_*_batch converts, sizes and assembles the documents on the GPU; one call per batch, the text comes
// back finished.  (RangeProofNi::prove_batch / prove_batch_seeded hand their result over as host BigInts — this layer keeps no
// device-resident batch —, so these overloads stage the limbs in again; a caller that holds the SoA batch on the device uses the C ABI
// entry points with ZKP_F_DEVICE_PTRS and moves no limb at all.)
namespace detail_json {
// the ONE sizing protocol of the writers: call(text or null, capacity, offsets[B + 1]) -> status — the sizing call, one allocation, the
// writing call, the text cut at the offsets
template <class F> std::vector<std::string> write_documents(size_t B, F call, const char* what) {
  Engine& e = Engine::instance();
  std::vector<uint64_t> off(B + 1, 0);
  e.check(call((char*)nullptr, (uint64_t)0, off.data()), what);
  std::string text((size_t)off[B], '\0');
  if (!text.empty()) e.check(call(&text[0], (uint64_t)text.size(), off.data()), what);
  std::vector<std::string> out(B);
  for (size_t b = 0; b < B; b++) out[b] = text.substr((size_t)off[b], (size_t)(off[b + 1] - off[b]));
  return out;
}
inline void same_rows(size_t have, size_t EF) { if (have != EF) throw std::invalid_argument("to_string_batch: every document of a batch has the same number of rows"); }
}  // namespace detail_json

inline std::vector<std::string> to_string_batch(const std::vector<EncryptedPairs>& v, const EncryptionKey& ek) {
  if (v.empty()) return {};
  Engine& e = Engine::instance();
  const uint32_t nb = width_for(ek.n);
  RangeSlab s(v.size(), v[0].c1.size(), nb / 32, RangeSlab::PAIRS);
  for (size_t b = 0; b < v.size(); b++) { detail_json::same_rows(v[b].c1.size(), s.EF); detail_json::same_rows(v[b].c2.size(), s.EF); s.put_pairs(b, v[b]); }
  const zkp_range_ni_proofs p = s.abi(nb, nullptr, 0);
  return detail_json::write_documents(v.size(), [&](char* t, uint64_t cap, uint64_t* off) { return zkp_json_write_encrypted_pairs_batch(e.ctx(), &p, t, cap, off, nullptr, 0); },
                                      "zkp_json_write_encrypted_pairs_batch");
}
inline std::vector<std::string> to_string_batch(const std::vector<Proof>& v, const EncryptionKey& ek) {
  if (v.empty()) return {};
  Engine& e = Engine::instance();
  const uint32_t nb = width_for(ek.n);
  RangeSlab s(v.size(), v[0].responses.size(), nb / 32, RangeSlab::RESPONSES);
  for (size_t b = 0; b < v.size(); b++) { detail_json::same_rows(v[b].responses.size(), s.EF); s.put_proof(b, v[b]); }
  const zkp_range_ni_proofs p = s.abi(nb, nullptr, 0);
  return detail_json::write_documents(v.size(), [&](char* t, uint64_t cap, uint64_t* off) { return zkp_json_write_range_proof_batch(e.ctx(), &p, t, cap, off, nullptr, 0); },
                                      "zkp_json_write_range_proof_batch");
}
inline std::vector<std::string> to_string_batch(const std::vector<NiCorrectKeyProof>& v, const EncryptionKey& ek) {
  if (v.empty()) return {};
  Engine& e = Engine::instance();
  const uint32_t nb = width_for(ek.n), kw = nb / 32;
  std::vector<uint32_t> sigma(v.size() * ZKP_CORRECT_KEY_M2 * kw);
  for (size_t b = 0; b < v.size(); b++) {
    if (v[b].sigma_vec.size() != ZKP_CORRECT_KEY_M2) throw std::invalid_argument("to_string_batch: a NiCorrectKeyProof has 11 values");
    for (size_t i = 0; i < ZKP_CORRECT_KEY_M2; i++) v[b].sigma_vec[i].to_limbs(&sigma[(b * ZKP_CORRECT_KEY_M2 + i) * kw], kw);
  }
  return detail_json::write_documents(v.size(), [&](char* t, uint64_t cap, uint64_t* off) { return zkp_json_write_correct_key_proof_batch(e.ctx(), nb, v.size(), sigma.data(), t, cap, off, nullptr, 0); },
                                      "zkp_json_write_correct_key_proof_batch");
}
inline std::vector<std::string> to_string_batch(const std::vector<RangeProofNi>& v, BigintText key_form = BigintText::Dec, BigintText bigint_form = BigintText::Dec) {
  if (v.empty()) return {};
  Engine& e = Engine::instance();
  const uint32_t nb = width_for(v[0].ek.n), kw = nb / 32;
  RangeSlab s(v.size(), v[0].error_factor, kw, RangeSlab::ALL);
  std::vector<uint32_t> n(v.size() * kw);
  for (size_t b = 0; b < v.size(); b++) {
    if (width_for(v[b].ek.n) != nb || v[b].error_factor != s.EF) throw std::invalid_argument("to_string_batch: one key width and one error_factor per batch");
    detail_json::same_rows(v[b].encrypted_pairs.c1.size(), s.EF); detail_json::same_rows(v[b].encrypted_pairs.c2.size(), s.EF); detail_json::same_rows(v[b].proof.responses.size(), s.EF);
    v[b].ek.n.to_limbs(&n[b * kw], kw);
    s.put_statement(b, v[b].range, v[b].ciphertext); s.put_pairs(b, v[b].encrypted_pairs); s.put_proof(b, v[b].proof);
  }
  const zkp_range_ni_proofs p = s.abi(nb, n.data(), kw);
  const uint32_t forms = ZKP_BIGINT_FORMS((uint32_t)key_form, (uint32_t)bigint_form);
  return detail_json::write_documents(v.size(), [&](char* t, uint64_t cap, uint64_t* off) { return zkp_json_write_range_proof_ni_batch(e.ctx(), &p, forms, t, cap, off, nullptr, 0); },
                                      "zkp_json_write_range_proof_ni_batch");
}
// the whole document (range_proof_ni.rs:36-44), the inverse of range_proof_ni_from_str
inline std::string to_string(const RangeProofNi& p, BigintText key_form = BigintText::Dec, BigintText bigint_form = BigintText::Dec) {
  return to_string_batch(std::vector<RangeProofNi>{p}, key_form, bigint_form)[0];
}

namespace detail_json {
struct Cur {
  const std::string& t; size_t p = 0;
  [[noreturn]] void fail(const char* what) const { throw std::runtime_error(std::string("serde_json: ") + what + " at byte " + std::to_string(p)); }
  void ws() { while (p < t.size() && (t[p] == ' ' || t[p] == '\n' || t[p] == '\r' || t[p] == '\t')) p++; }
  bool eat(char c) { ws(); if (p < t.size() && t[p] == c) { p++; return true; } return false; }
  void expect(char c) { if (!eat(c)) fail("unexpected token"); }
  std::string str() {
    expect('"');
    std::string out;
    while (p < t.size() && t[p] != '"') {
      if (t[p] == '\\') {
        if (++p >= t.size()) fail("bad escape");
        const char c = t[p++];
        if (c == 'u') {
          if (p + 4 > t.size()) fail("bad \\u escape");
          const unsigned v = (unsigned)std::stoul(t.substr(p, 4), nullptr, 16); p += 4;
          if (v > 0x7f) fail("non-ASCII escape in a number or field name");
          out.push_back((char)v);
        } else out.push_back(c == 'n' ? '\n' : c == 't' ? '\t' : c == 'r' ? '\r' : c == 'b' ? '\b' : c == 'f' ? '\f' : c);
      } else out.push_back(t[p++]);
    }
    if (p >= t.size()) fail("unterminated string");
    p++;
    return out;
  }
  uint64_t uint() {
    ws();
    if (p >= t.size() || t[p] < '0' || t[p] > '9') fail("expected an unsigned integer");
    uint64_t v = 0;
    while (p < t.size() && t[p] >= '0' && t[p] <= '9') { if (v > (~0ull - 9) / 10) fail("integer overflow"); v = v * 10 + (uint64_t)(t[p++] - '0'); }
    if (p < t.size() && (t[p] == '.' || t[p] == 'e' || t[p] == 'E')) fail("expected an integer");
    return v;
  }
  void skip() {
    ws();
    if (p >= t.size()) fail("unexpected end");
    if (t[p] == '"') { (void)str(); return; }
    if (t[p] == '{' || t[p] == '[') {
      const char close = t[p] == '{' ? '}' : ']';
      p++;
      if (eat(close)) return;
      do { if (close == '}') { (void)str(); expect(':'); } skip(); } while (eat(','));
      expect(close); return;
    }
    while (p < t.size() && t[p] != ',' && t[p] != '}' && t[p] != ']' && t[p] != ' ' && t[p] != '\n') p++;
  }
  template <class F> void object(F&& field) {      // field(name) consumes the value and returns true, or returns false (unknown: skipped)
    expect('{');
    if (eat('}')) return;
    do { const std::string nm = str(); expect(':'); if (!field(nm)) skip(); } while (eat(','));
    expect('}');
  }
  BigInt dec() { const std::string s = str(); try { return BigInt::from_str_radix10(s); } catch (const std::invalid_argument&) { fail("not a decimal integer"); } }
  BigInt bigint(BigintText form) {
    if (form == BigintText::Dec) return dec();
    if (form == BigintText::Bytes) {
      std::vector<uint8_t> b;
      expect('[');
      if (!eat(']')) { do { const uint64_t v = uint(); if (v > 255) fail("byte out of range"); b.push_back((uint8_t)v); } while (eat(',')); expect(']'); }
      return BigInt::from_bytes(b);
    }
    std::string h = str();
    const bool minus = !h.empty() && h[0] == '-';
    if (minus) h.erase(0, 1);
    if (h.empty()) fail("empty hex integer");
    BigInt r;
    r.l.assign((h.size() + 7) / 8, 0);
    for (size_t i = 0; i < h.size(); i++) {
      const char c = h[h.size() - 1 - i];
      const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
      if (v < 0) fail("not a hex integer");
      r.l[i / 8] |= (uint32_t)v << (4 * (i % 8));
    }
    r.trim();
    r.neg = minus && !r.is_zero();
    return r;
  }
};
}  // namespace detail_json

// {"sigma_vec":["..", ..]} (correct_key_ni.rs:35-39) with signed roots of any size and any count
inline NiCorrectKeyProof correct_key_from_str_host(const std::string& doc) {
  detail_json::Cur j{doc};
  NiCorrectKeyProof out;
  bool seen = false;
  j.object([&](const std::string& nm) {
    if (nm != "sigma_vec") return false;
    if (seen) j.fail("duplicate field");
    seen = true;
    j.expect('[');
    if (!j.eat(']')) { do out.sigma_vec.push_back(j.dec()); while (j.eat(',')); j.expect(']'); }
    return true;
  });
  if (!seen) j.fail("missing field `sigma_vec`");
  j.ws();
  if (j.p != doc.size()) j.fail("trailing characters");
  return out;
}

// CompositeDLogProof {"x":X,"y":X} and DLogStatement {"N":X,"g":X,"ni":X} (wi_dlog_proof.rs:32-43): un-annotated BigInts of any size and sign, on
// the host (whole batches: zkp_json_write_dlog_*_batch / zkp_json_dlog_*_batch of the C ABI, CompositeDLogProof::verify_json_batch)
inline std::string bigint_text(const BigInt& v, BigintText form) {
  if (form == BigintText::Dec) return "\"" + v.to_str_radix10() + "\"";
  const std::vector<uint8_t> b = v.to_bytes();
  std::string s = form == BigintText::Hex ? (v.is_negative() ? "\"-" : "\"") : "[";
  for (size_t i = 0; i < b.size(); i++) {
    if (form == BigintText::Hex) { static const char* d = "0123456789abcdef"; s.push_back(d[b[i] >> 4]); s.push_back(d[b[i] & 15]); }
    else s += (i ? "," : "") + std::to_string((unsigned)b[i]);
  }
  return s + (form == BigintText::Hex ? "\"" : "]");
}
inline std::string to_string(const CompositeDLogProof& p, BigintText form = BigintText::Dec) { return "{\"x\":" + bigint_text(p.x, form) + ",\"y\":" + bigint_text(p.y, form) + "}"; }
inline std::string to_string(const DLogStatement& s, BigintText form = BigintText::Dec) {
  return "{\"N\":" + bigint_text(s.N, form) + ",\"g\":" + bigint_text(s.g, form) + ",\"ni\":" + bigint_text(s.ni, form) + "}";
}
namespace detail_json {
inline void bigint_fields(const std::string& doc, BigintText form, const std::vector<std::pair<const char*, BigInt*>>& fields) {
  Cur j{doc};
  unsigned seen = 0;
  j.object([&](const std::string& nm) {
    for (size_t f = 0; f < fields.size(); f++) {
      if (nm != fields[f].first) continue;
      if (seen & (1u << f)) j.fail("duplicate field");
      seen |= 1u << f;
      *fields[f].second = j.bigint(form);
      return true;
    }
    return false;
  });
  if (seen != (1u << fields.size()) - 1) j.fail("missing field");
  j.ws();
  if (j.p != doc.size()) j.fail("trailing characters");
}
}  // namespace detail_json
inline CompositeDLogProof dlog_proof_from_str(const std::string& doc, BigintText form = BigintText::Dec) {
  CompositeDLogProof p;
  detail_json::bigint_fields(doc, form, {{"x", &p.x}, {"y", &p.y}});
  return p;
}
inline DLogStatement dlog_statement_from_str(const std::string& doc, BigintText form = BigintText::Dec) {
  DLogStatement s;
  detail_json::bigint_fields(doc, form, {{"N", &s.N}, {"g", &s.g}, {"ni", &s.ni}});
  return s;
}

// the documents of the sigma proofs and their statements: driven by the tables of zkproofs::detail (SigmaDoc, above)
namespace detail_json {
// MinimalEncryptionKey -> EncryptionKey { n, nn = n * n } for the types that carry a key [upstream kzen-paillier]
template <class T> auto set_nn(T& d, int) -> decltype(d.ek.nn, void()) { d.ek.nn = d.ek.n * d.ek.n; }
template <class T> void set_nn(T&, long) {}
}  // namespace detail_json

template <class T, class D = detail::SigmaDoc<T>> std::string to_string(const T& doc, BigintText key_form = BigintText::Dec, BigintText bare_form = BigintText::Dec) {
  std::string s = "{";
  bool after_key = false;
  for (const detail::SigmaField& f : D::fields(const_cast<T&>(doc))) {
    if (s.size() > 1) s += after_key ? "}," : ",";
    s += std::string("\"") + f.name + "\":" + (f.key ? "{\"n\":" : "") + bigint_text(*f.v, f.key ? key_form : bare_form);
    after_key = f.key;
  }
  return s + (after_key ? "}}" : "}");
}
// serde_json::from_str::<T>: throws (std::runtime_error) where serde reports an error
template <class T, class D = detail::SigmaDoc<T>> T sigma_from_str(const std::string& doc, BigintText key_form = BigintText::Dec, BigintText bare_form = BigintText::Dec) {
  T out;
  const std::vector<detail::SigmaField> fields = D::fields(out);
  detail_json::Cur j{doc};
  unsigned seen = 0;
  j.object([&](const std::string& nm) {
    for (size_t f = 0; f < fields.size(); f++) {
      if (nm != fields[f].name) continue;
      if (seen & (1u << f)) j.fail("duplicate field");
      seen |= 1u << f;
      if (!fields[f].key) { *fields[f].v = j.bigint(bare_form); return true; }
      bool has_n = false;
      j.object([&](const std::string& k) { if (k != "n") return false; if (has_n) j.fail("duplicate field"); has_n = true; *fields[f].v = j.bigint(key_form); return true; });
      if (!has_n) j.fail("missing field `n`");
      return true;
    }
    return false;
  });
  if (seen != (1u << fields.size()) - 1) j.fail((std::string("missing field of ") + D::type).c_str());
  j.ws();
  if (j.p != doc.size()) j.fail("trailing characters");
  detail_json::set_nn(out, 0);
  return out;
}
// whole batches through zkp_json_write_sigma_batch: one key width per batch — the smallest in which every value fits its array
template <class T, class D = detail::SigmaDoc<T>>
std::vector<std::string> to_string_batch(const std::vector<T>& v, BigintText key_form = BigintText::Dec, BigintText bare_form = BigintText::Dec) {
  static_assert(!D::secret, "a witness has no document form");
  const size_t B = v.size();
  if (B == 0) return {};
  uint32_t nb = 0;
  for (uint32_t cand : {1024u, 2048u, 4096u}) {
    bool fits = true;
    for (const T& d : v) for (const detail::SigmaField& f : D::fields(const_cast<T&>(d))) fits = fits && f.v->fits_limbs(detail::sigma_words(f.w, cand / 32));
    if (fits) { nb = cand; break; }
  }
  if (!nb) throw std::invalid_argument(std::string("to_string_batch: a ") + D::type + " with a negative value or one wider than the 4096-bit layout");
  Columns c = detail::sigma_flatten(v.data(), B, nb / 32, true);
  const zkp_sigma_fields in{c[0], c[1], c[2], c[3], c[4]};
  const uint32_t forms = ZKP_BIGINT_FORMS((uint32_t)key_form, (uint32_t)bare_form);
  Engine& e = Engine::instance();
  return detail_json::write_documents(B, [&](char* t, uint64_t cap, uint64_t* off) { return zkp_json_write_sigma_batch(e.ctx(), D::kind, nb, B, &in, forms, t, cap, off, nullptr, 0); },
                                      "zkp_json_write_sigma_batch");
}

namespace detail_json {
// EncryptedPairs {"c1":[..],"c2":[..]} and Proof [{"Open":{..}} | {"Mask":{..}}, ..] (range_proof.rs:32-81) at the cursor: signed integers of any
// size, any number of rows
inline void read_encrypted_pairs(Cur& j, EncryptedPairs& ep) {
  auto vec = [&](std::vector<BigInt>& v) { j.expect('['); if (!j.eat(']')) { do v.push_back(j.dec()); while (j.eat(',')); j.expect(']'); } };
  unsigned s2 = 0;
  j.object([&](const std::string& f) {
    if (f == "c1") { if (s2 & 1) j.fail("duplicate field"); s2 |= 1; vec(ep.c1); return true; }
    if (f == "c2") { if (s2 & 2) j.fail("duplicate field"); s2 |= 2; vec(ep.c2); return true; }
    return false;
  });
  if (s2 != 3) j.fail("missing field of EncryptedPairs");
}
inline void read_proof(Cur& j, Proof& proof) {
  j.expect('[');
  if (j.eat(']')) return;
  do {
    Response rs;
    int variants = 0;
    j.object([&](const std::string& var) {
      if (++variants > 1) j.fail("expected a single-variant enum map");
      unsigned s3 = 0;
      if (var == "Open") {
        rs.kind = Response::Open;
        j.object([&](const std::string& f) {
          BigInt* dst = f == "w1" ? &rs.w1 : f == "r1" ? &rs.r1 : f == "w2" ? &rs.w2 : f == "r2" ? &rs.r2 : nullptr;
          if (!dst) return false;
          const unsigned bit = f == "w1" ? 1 : f == "r1" ? 2 : f == "w2" ? 4 : 8;
          if (s3 & bit) j.fail("duplicate field");
          s3 |= bit;
          *dst = j.dec();
          return true;
        });
        if (s3 != 15) j.fail("missing field of Response::Open");
      } else if (var == "Mask") {
        rs.kind = Response::Mask;
        j.object([&](const std::string& f) {
          if (f == "j") { if (s3 & 1) j.fail("duplicate field"); s3 |= 1; const uint64_t v = j.uint(); if (v > 255) j.fail("j is a u8"); rs.j = (uint8_t)v; return true; }
          if (f == "masked_x") { if (s3 & 2) j.fail("duplicate field"); s3 |= 2; rs.masked_x = j.dec(); return true; }
          if (f == "masked_r") { if (s3 & 4) j.fail("duplicate field"); s3 |= 4; rs.masked_r = j.dec(); return true; }
          return false;
        });
        if (s3 != 7) j.fail("missing field of Response::Mask");
      } else j.fail("unknown variant of Response");
      return true;
    });
    if (variants != 1) j.fail("expected a single-variant enum map");
    proof.responses.push_back(std::move(rs));
  } while (j.eat(','));
  j.expect(']');
}
}  // namespace detail_json

// serde_json::from_str::<EncryptedPairs> / ::<Proof> on the HOST, for the documents of an interactive session the GPU readers hand back
inline EncryptedPairs encrypted_pairs_from_str_host(const std::string& doc) {
  detail_json::Cur j{doc};
  EncryptedPairs out;
  detail_json::read_encrypted_pairs(j, out);
  j.ws();
  if (j.p != doc.size()) j.fail("trailing characters");
  return out;
}
inline Proof proof_from_str_host(const std::string& doc) {
  detail_json::Cur j{doc};
  Proof out;
  detail_json::read_proof(j, out);
  j.ws();
  if (j.p != doc.size()) j.fail("trailing characters");
  return out;
}

inline RangeProofNi range_proof_ni_from_str(const std::string& doc, BigintText key_form = BigintText::Dec, BigintText bigint_form = BigintText::Dec) {
  detail_json::Cur j{doc};
  RangeProofNi out;
  unsigned seen = 0;
  auto once = [&](unsigned bit) { if (seen & bit) j.fail("duplicate field"); seen |= bit; };
  j.object([&](const std::string& nm) {
    if (nm == "ek") {
      once(1);
      bool has_n = false;
      j.object([&](const std::string& f) { if (f != "n") return false; if (has_n) j.fail("duplicate field"); has_n = true; out.ek.n = j.bigint(key_form); return true; });
      if (!has_n) j.fail("missing field `n`");
      out.ek.nn = out.ek.n * out.ek.n;       // MinimalEncryptionKey -> EncryptionKey { n, nn = n * n } [upstream kzen-paillier]
    } else if (nm == "range") { once(2); out.range = j.bigint(bigint_form); }
    else if (nm == "ciphertext") { once(4); out.ciphertext = j.bigint(bigint_form); }
    else if (nm == "encrypted_pairs") { once(8); detail_json::read_encrypted_pairs(j, out.encrypted_pairs); }
    else if (nm == "proof") { once(16); detail_json::read_proof(j, out.proof); }
    else if (nm == "error_factor") { once(32); out.error_factor = (size_t)j.uint(); }
    else return false;
    return true;
  });
  if (seen != 63u) j.fail("missing field of RangeProofNi");
  j.ws();
  if (j.p != doc.size()) j.fail("trailing characters");
  return out;
}
}  // namespace serde_json

inline std::vector<Result> RangeProofNi::verify_json_batch(const std::vector<std::string>& docs, uint32_t forms, const EncryptionKey* ek) {
  const size_t B = docs.size();
  if (B == 0) return {};
  const auto kf = (serde_json::BigintText)((forms >> 4) & 15u), bf = (serde_json::BigintText)(forms & 15u);
  auto parse = [&](const std::string& doc, RangeProofNi* out) -> std::string {
    try { *out = serde_json::range_proof_ni_from_str(doc, kf, bf); return std::string(); } catch (const std::exception& e) { return e.what(); }
  };
  auto carried = [](const BigInt& n) { return !n.is_negative() && n.is_odd() && n.bit_length() <= 4096 && n.bit_length() >= 2; };
  if (ek && !carried(ek->n)) return std::vector<Result>(B, Result::unsupported("RangeProofNi::verify: the key is not a positive odd integer of at most 4096 bits"));
  // one key width per call: the verifier's, else that of the first document that parses and has a key the engine carries
  uint32_t nb = ek ? width_for(ek->n) : 0;
  for (size_t b = 0; b < B && nb == 0; b++) { RangeProofNi q; if (parse(docs[b], &q).empty() && carried(q.ek.n)) nb = width_for(q.ek.n); }
  std::vector<Result> out(B, Result(false));
  std::vector<uint8_t> status(B, ZKP_DOC_HOST_PATH), verdict(B, ZKP_VERDICT_REJECT);
  if (nb) {
    const uint32_t kw = nb / 32;
    std::string text;
    std::vector<uint64_t> off(B), len(B);
    for (size_t b = 0; b < B; b++) { off[b] = text.size(); len[b] = docs[b].size(); text += docs[b]; }
    std::vector<uint32_t> n(kw);
    if (ek) ek->n.to_limbs(n.data(), kw);
    Engine& e = Engine::instance();
    if (zkp_range_ni_verify_json_batch(e.ctx(), text.data(), off.data(), len.data(), B, nb, SECURITY_PARAMETER, forms, ek ? n.data() : nullptr, status.data(),
                                       verdict.data(), 0) != ZKP_OK)
      throw std::runtime_error(std::string("zkp_range_ni_verify_json_batch: ") + zkp_last_error_string(e.ctx()));
  }
  for (size_t b = 0; b < B; b++) {
    if (status[b] == ZKP_DOC_OK) { out[b] = Result(verdict[b] == ZKP_VERDICT_ACCEPT); continue; }
    RangeProofNi q;
    const std::string err = parse(docs[b], &q);
    if (!err.empty()) { out[b] = Result::panicked("called `Result::unwrap()` on an `Err` value: " + err); continue; }
    if (ek && !(q.ek == *ek)) { out[b] = Result::panicked("assertion failed: `(left == right)` ek"); continue; }
    out[b] = verify_batch(q.ek, {&q})[0];       // ZKP_DOC_HOST_PATH (or a key of another width): the host path for integers of any size and sign
  }
  return out;
}

inline std::vector<Result> RangeProof::verifier_output_json_batch(const EncryptionKey& ek, const std::vector<ChallengeBits>& challenges, const std::vector<std::string>& pairs_docs,
                                                                  const std::vector<std::string>& proof_docs, const std::vector<BigInt>& ranges,
                                                                  const std::vector<BigInt>& cipher_xs, size_t error_factor) {
  const size_t B = pairs_docs.size(), EF = error_factor;
  if (proof_docs.size() != B || challenges.size() != B || ranges.size() != B || cipher_xs.size() != B)
    throw std::invalid_argument("RangeProof::verifier_output_json_batch: one challenge, two documents and one statement per session");
  if (B == 0) return {};
  const bool key_carried = !ek.n.is_negative() && ek.n.is_odd() && ek.n.bit_length() <= 4096 && ek.n.bit_length() >= 2;
  if (!key_carried) return std::vector<Result>(B, Result::unsupported("RangeProof::verifier_output: the key is not a positive odd integer of at most 4096 bits"));
  const uint32_t nb = width_for(ek.n), kw = nb / 32;
  // the sessions the one call takes: a challenge the ABI carries and a statement within the widths; at least one row, at most 256
  std::vector<size_t> idx;
  if (EF >= 1 && EF <= 256)
    for (size_t b = 0; b < B; b++)
      if (challenges[b].bytes.size() <= 32 && ranges[b].fits_limbs(kw) && cipher_xs[b].fits_limbs(2 * kw)) idx.push_back(b);
  std::vector<uint8_t> status(B, ZKP_DOC_HOST_PATH), verdict(B, ZKP_VERDICT_REJECT);
  if (!idx.empty()) {
    const size_t G = idx.size();
    std::string text;
    std::vector<uint64_t> ao(G), al(G), po(G), pl(G);
    for (size_t q = 0; q < G; q++) { ao[q] = text.size(); al[q] = pairs_docs[idx[q]].size(); text += pairs_docs[idx[q]]; }
    for (size_t q = 0; q < G; q++) { po[q] = text.size(); pl[q] = proof_docs[idx[q]].size(); text += proof_docs[idx[q]]; }
    std::vector<uint32_t> n(kw);
    ek.n.to_limbs(n.data(), kw);
    RangeSlab s(G, EF, kw, RangeSlab::STATEMENT);
    std::vector<uint8_t> eb(G * 32), elen(G), st(G, ZKP_DOC_HOST_PATH), v(G, ZKP_VERDICT_REJECT);
    for (size_t q = 0; q < G; q++) {
      s.put_statement(q, ranges[idx[q]], cipher_xs[idx[q]]);
      uint8_t one[32];
      pack_challenge(challenges[idx[q]], one, elen[q]);
      std::memcpy(&eb[q * 32], one, 32);
    }
    const zkp_range_ni_proofs p = s.abi(nb, n.data(), 0);
    Engine& e = Engine::instance();
    e.check(zkp_range_verifier_output_json_batch(e.ctx(), text.data(), ao.data(), al.data(), po.data(), pl.data(), G, nb, (uint32_t)EF, p.n, 0, p.range, p.ciphertext, eb.data(),
                                                 elen.data(), st.data(), v.data(), 0), "zkp_range_verifier_output_json_batch");
    for (size_t q = 0; q < G; q++) { status[idx[q]] = st[q]; verdict[idx[q]] = v[q]; }
  }
  std::vector<Result> out(B, Result(false));
  for (size_t b = 0; b < B; b++) {
    if (status[b] == ZKP_DOC_OK) {
      out[b] = verdict[b] == ZKP_VERDICT_MALFORMED ? Result::panicked("RangeProof::verifier_output: malformed proof (the reference would panic)") : Result(verdict[b] == ZKP_VERDICT_ACCEPT);
      continue;
    }
    EncryptedPairs ep; Proof pr;
    try { ep = serde_json::encrypted_pairs_from_str_host(pairs_docs[b]); pr = serde_json::proof_from_str_host(proof_docs[b]); }
    catch (const std::exception& err) { out[b] = Result::panicked(std::string("called `Result::unwrap()` on an `Err` value: ") + err.what()); continue; }
    // ZKP_DOC_HOST_PATH, or a session kept from the call: the single-session path for integers of any size and sign
    try { out[b] = verifier_output(ek, challenges[b], ep, pr, ranges[b], cipher_xs[b], EF); }
    catch (const Panic& panic) { out[b] = Result::panicked(panic.what()); }
  }
  return out;
}

inline std::vector<Result> CompositeDLogProof::verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t bare_form) {
  const size_t B = statements.size();
  if (proofs.size() != B) throw std::invalid_argument("CompositeDLogProof::verify_json_batch: one proof per statement");
  if (bare_form > ZKP_BIGINT_BYTES) throw std::invalid_argument("CompositeDLogProof::verify_json_batch: unknown text form");
  const auto form = (serde_json::BigintText)bare_form;
  std::vector<Result> out(B, Result(false));
  std::vector<uint8_t> status(B, ZKP_DOC_HOST_PATH), verdict(B, ZKP_VERDICT_REJECT);
  // one modulus width per call: that of the first statement that parses and has a modulus the engine carries
  uint32_t nb = 0;
  for (size_t b = 0; b < B && nb == 0; b++) {
    try {
      const DLogStatement s = serde_json::dlog_statement_from_str(statements[b], form);
      if (!s.N.is_negative() && s.N.is_odd() && s.N.bit_length() >= 2 && s.N.bit_length() <= 4096) nb = width_for(s.N);
    } catch (const std::exception&) {}
  }
  if (nb) {
    std::string text;
    std::vector<uint64_t> so(B), sl(B), po(B), pl(B);
    for (size_t b = 0; b < B; b++) { so[b] = text.size(); sl[b] = statements[b].size(); text += statements[b]; }
    for (size_t b = 0; b < B; b++) { po[b] = text.size(); pl[b] = proofs[b].size(); text += proofs[b]; }
    Engine& e = Engine::instance();
    if (zkp_dlog_verify_json_batch(e.ctx(), text.data(), so.data(), sl.data(), po.data(), pl.data(), B, nb, Y_BITS, bare_form, status.data(), verdict.data(), 0) != ZKP_OK)
      throw std::runtime_error(std::string("zkp_dlog_verify_json_batch: ") + zkp_last_error_string(e.ctx()));
  }
  for (size_t b = 0; b < B; b++) {
    if (status[b] == ZKP_DOC_OK && verdict[b] != ZKP_VERDICT_MALFORMED) { out[b] = Result(verdict[b] == ZKP_VERDICT_ACCEPT); continue; }
    try {
      DLogStatement s; CompositeDLogProof p;
      try { s = serde_json::dlog_statement_from_str(statements[b], form); p = serde_json::dlog_proof_from_str(proofs[b], form); }
      catch (const std::exception& err) { out[b] = Result::panicked(std::string("called `Result::unwrap()` on an `Err` value: ") + err.what()); continue; }
      out[b] = p.verify(s);         // (a MALFORMED verdict as well: verify() names the assertion that failed)
    } catch (const Panic& panic) { out[b] = Result::panicked(panic.what()); }
  }
  return out;
}

inline std::vector<Result> NiCorrectKeyProof::verify_json_batch(const std::vector<std::pair<const EncryptionKey*, std::string>>& items, const uint8_t* salt,
                                                                size_t salt_len) {
  const size_t B = items.size();
  std::vector<Result> out(B, Result(false));
  std::vector<uint8_t> status(B, ZKP_DOC_HOST_PATH), verdict(B, ZKP_VERDICT_REJECT);
  auto carried = [](const BigInt& n) { return !n.is_negative() && n.is_odd() && n.bit_length() >= 2 && n.bit_length() <= 4096; };
  Engine& e = Engine::instance();
  for (uint32_t nb : {1024u, 2048u, 4096u}) {
    const uint32_t kw = nb / 32;
    std::vector<size_t> idx;
    for (size_t k = 0; k < B; k++) if (carried(items[k].first->n) && width_for(items[k].first->n) == nb) idx.push_back(k);
    if (idx.empty()) continue;
    std::string text;
    std::vector<uint64_t> off(idx.size()), len(idx.size());
    std::vector<uint32_t> n(idx.size() * kw);
    std::vector<uint8_t> st(idx.size(), ZKP_DOC_HOST_PATH), v(idx.size(), ZKP_VERDICT_REJECT);
    for (size_t q = 0; q < idx.size(); q++) {
      const std::string& doc = items[idx[q]].second;
      off[q] = text.size(); len[q] = doc.size(); text += doc;
      items[idx[q]].first->n.to_limbs(&n[q * kw], kw);
    }
    if (zkp_correct_key_ni_verify_json_batch(e.ctx(), text.data(), off.data(), len.data(), idx.size(), nb, n.data(), salt, (uint32_t)salt_len, st.data(), v.data(), 0) != ZKP_OK)
      throw std::runtime_error(std::string("zkp_correct_key_ni_verify_json_batch: ") + zkp_last_error_string(e.ctx()));
    for (size_t q = 0; q < idx.size(); q++) { status[idx[q]] = st[q]; verdict[idx[q]] = v[q]; }
  }
  for (size_t k = 0; k < B; k++) {
    if (status[k] == ZKP_DOC_OK) { out[k] = Result(verdict[k] == ZKP_VERDICT_ACCEPT); continue; }
    NiCorrectKeyProof q;
    try { q = serde_json::correct_key_from_str_host(items[k].second); }
    catch (const std::exception& err) { out[k] = Result::panicked(std::string("called `Result::unwrap()` on an `Err` value: ") + err.what()); continue; }
    out[k] = verify_batch({{items[k].first, &q}}, salt, salt_len)[0];
  }
  return out;
}

// The four sigma proofs on documents.  Why a pair the GPU handed back (ZKP_DOC_HOST_PATH) is unsupported: the host mirror has no evaluator for
// these types outside the limb kernels' domain — a negative or over-wide value, an even or trivial key, a residue not reduced mod n^2 (f: mod n).
namespace detail_json_sigma {
template <class Proof, class Statement>
std::vector<Result> verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms) {
  using PD = detail::SigmaDoc<Proof>;
  using SD = detail::SigmaDoc<Statement>;
  using detail::SigmaWidth;
  const std::string name = std::string(PD::type) + "::verify_json_batch";
  const size_t B = statements.size();
  if (proofs.size() != B) throw std::invalid_argument(name + ": one proof per statement");
  const uint32_t kf = (forms >> 4) & 15u, bf = forms & 15u;
  if ((forms >> 8) || kf > ZKP_BIGINT_BYTES || bf > ZKP_BIGINT_BYTES) throw std::invalid_argument(name + ": unknown text form");
  const auto key_form = (serde_json::BigintText)kf, bare_form = (serde_json::BigintText)bf;
  auto carried = [](const BigInt& n) { return !n.is_negative() && n.is_odd() && n.bit_length() >= 2 && n.bit_length() <= 4096; };
  std::vector<Result> out(B, Result(false));
  std::vector<uint8_t> status(B, ZKP_DOC_HOST_PATH), verdict(B, ZKP_VERDICT_REJECT);
  // one key width per call: that of the first statement that parses and has a key the engine carries
  uint32_t nb = 0;
  for (size_t b = 0; b < B && nb == 0; b++) {
    try { const Statement s = serde_json::sigma_from_str<Statement>(statements[b], key_form, bare_form); if (carried(s.ek.n)) nb = width_for(s.ek.n); } catch (const std::exception&) {}
  }
  if (nb) {
    std::string text;
    std::vector<uint64_t> so(B), sl(B), po(B), pl(B);
    for (size_t b = 0; b < B; b++) { so[b] = text.size(); sl[b] = statements[b].size(); text += statements[b]; }
    for (size_t b = 0; b < B; b++) { po[b] = text.size(); pl[b] = proofs[b].size(); text += proofs[b]; }
    Engine& e = Engine::instance();
    if (zkp_sigma_verify_json_batch(e.ctx(), PD::kind, text.data(), so.data(), sl.data(), po.data(), pl.data(), B, nb, forms, status.data(), verdict.data(), 0) != ZKP_OK)
      throw std::runtime_error(std::string("zkp_sigma_verify_json_batch: ") + zkp_last_error_string(e.ctx()));
  }
  for (size_t b = 0; b < B; b++) {
    if (status[b] == ZKP_DOC_OK) {
      out[b] = verdict[b] == ZKP_VERDICT_MALFORMED ? Result::panicked("called `Option::unwrap()` on a `None` value (mod_inv, multiplication_proof.rs:135)")
                                                   : Result(verdict[b] == ZKP_VERDICT_ACCEPT);
      continue;
    }
    Statement s; Proof p;
    try { s = serde_json::sigma_from_str<Statement>(statements[b], key_form, bare_form); p = serde_json::sigma_from_str<Proof>(proofs[b], key_form, bare_form); }
    catch (const std::exception& err) { out[b] = Result::panicked(std::string("called `Result::unwrap()` on an `Err` value: ") + err.what()); continue; }
    std::string why;
    if (!carried(s.ek.n)) why = "the key is not a positive odd integer of 2 to 4096 bits";
    else {
      const BigInt nn = s.ek.n * s.ek.n;
      const uint32_t kw = width_for(s.ek.n) / 32;
      auto look = [&](const std::vector<detail::SigmaField>& fields) {
        for (const auto& f : fields) {
          if (f.key || !why.empty()) continue;
          if (f.v->is_negative()) why = std::string(f.name) + " is negative";
          else if (f.w == SigmaWidth::Z && f.v->bit_length() > 32 * detail::sigma_words(f.w, kw)) why = std::string(f.name) + " is wider than n by more than 512 bits";
          else if (f.w == SigmaWidth::NN && !(*f.v < nn)) why = std::string(f.name) + " is not below n^2";
          else if (f.w == SigmaWidth::N && !(*f.v < s.ek.n)) why = std::string(f.name) + " is not below n";
        }
      };
      look(SD::fields(s)); look(PD::fields(p));
    }
    if (!why.empty()) { out[b] = Result::unsupported(std::string(PD::type) + "::verify: " + why + ": outside the domain of the GPU kernels, and the host mirror has no evaluator for it"); continue; }
    // inside the domain under a key of another width than the batch's: the single-proof path
    try { out[b] = p.verify(s); } catch (const Panic& panic) { out[b] = Result::panicked(panic.what()); }
  }
  return out;
}
}  // namespace detail_json_sigma
inline std::vector<Result> ZeroProof::verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms) {
  return detail_json_sigma::verify_json_batch<ZeroProof, ZeroStatement>(statements, proofs, forms);
}
inline std::vector<Result> CiphertextProof::verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms) {
  return detail_json_sigma::verify_json_batch<CiphertextProof, CiphertextStatement>(statements, proofs, forms);
}
inline std::vector<Result> VerlinProof::verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms) {
  return detail_json_sigma::verify_json_batch<VerlinProof, VerlinStatement>(statements, proofs, forms);
}
inline std::vector<Result> MulProof::verify_json_batch(const std::vector<std::string>& statements, const std::vector<std::string>& proofs, uint32_t forms) {
  return detail_json_sigma::verify_json_batch<MulProof, MulStatement>(statements, proofs, forms);
}

}  // namespace zkproofs
