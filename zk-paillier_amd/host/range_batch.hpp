// range_batch.hpp — the batches of the host API (host/zkproofs.hpp) in host memory: no Engine, no GPU call.
//
//   Response, EncryptedPairs, Proof   the reference's range-proof types (src/zkproofs/range_proof.rs:32-81)
//   RangeSlab       the structure-of-arrays batch of include/zkp_hip.h (zkp_range_ni_proofs) for `rows` proofs of EF rows at kw limbs: owns the
//                   arrays, writes and reads a statement / a pair / a Response of row t, and hands the ABI struct out (abi(): the ONE place
//                   under host/ that names the struct's fields)
//   RangeWitness    its secret counterpart (zkp_range_ni_witness)
//   range_layout_carries   "the fixed-width layout at (kw, EF) carries this proof": every value non-negative and within its width
//   Columns         B rows of a few fixed-width fields, one array per field (the sigma proofs, CompositeDLogProof)
//   DLogSetupBatch  the moduli of DLogStatement::generate_batch_seeded in, (g, ni, secret, status) out
//
// All of it is RawBuf staging (host/staging.hpp): NOT zero-initialised, pooled and huge-page backed when large.  So every writer here
// writes every word of the row it is given — a Mask response zero-fills w2 / r2 and an Open one stores j = 0 —, and whatever is read is
// something a writer or the GPU call wrote.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <vector>

#include "../../include/zkp_hip.h"
#include "bigint.hpp"
#include "staging.hpp"

namespace zkproofs {

struct Response {           // src/zkproofs/range_proof.rs:53-78
  enum Kind { Open, Mask } kind = Open;
  BigInt w1, r1, w2, r2;    // Open
  uint8_t j = 0;            // Mask
  BigInt masked_x, masked_r;
};
struct EncryptedPairs { std::vector<BigInt> c1, c2; };   // range_proof.rs:32-39
struct Proof { std::vector<Response> responses; };       // range_proof.rs:80-81

// limbs into a BigInt whose storage is already there (capacity >= n: no allocation, a copy at memory bandwidth); allocates otherwise
inline void take_limbs(BigInt& dst, const uint32_t* p, size_t n) {
  while (n && p[n - 1] == 0) n--;
  dst.l.assign(p, p + n);
  dst.neg = false;
}

class RangeSlab {
 public:
  enum Groups : unsigned { STATEMENT = 1, PAIRS = 2, RESPONSES = 4, ALL = 7 };   // range, ciphertext | c1, c2 | resp_*
  const size_t rows, EF, kw;
  const unsigned groups;
  RangeSlab(size_t rows_, size_t EF_, size_t kw_, unsigned groups_)
      : rows(rows_), EF(EF_), kw(kw_), groups(groups_), range_(words(STATEMENT, 1)), ct_(words(STATEMENT, 2)), c1_(words(PAIRS, 2 * EF)), c2_(words(PAIRS, 2 * EF)),
        w1_(words(RESPONSES, EF)), r1_(words(RESPONSES, EF)), w2_(words(RESPONSES, EF)), r2_(words(RESPONSES, EF)), kind_(words(RESPONSES, EF) / kw),
        j_(words(RESPONSES, EF) / kw) {}
  bool large() const { return c1_.pooled() || w1_.pooled(); }
  // the batch as the C ABI takes it: the first `batch` proofs (default: all), absent groups null
  zkp_range_ni_proofs abi(uint32_t n_bits, const uint32_t* n, uint64_t n_stride) { return abi(n_bits, n, n_stride, rows); }
  zkp_range_ni_proofs abi(uint32_t n_bits, const uint32_t* n, uint64_t n_stride, size_t batch) {
    zkp_range_ni_proofs p{};
    p.n_bits = n_bits; p.error_factor = (uint32_t)EF; p.batch = batch; p.n_stride = n_stride; p.n = n;
    if (groups & STATEMENT) { p.range = range_.data(); p.ciphertext = ct_.data(); }
    if (groups & PAIRS) { p.c1 = c1_.data(); p.c2 = c2_.data(); }
    if (groups & RESPONSES) {
      p.resp_kind = kind_.data(); p.resp_j = j_.data();
      p.resp_w1 = w1_.data(); p.resp_r1 = r1_.data(); p.resp_w2 = w2_.data(); p.resp_r2 = r2_.data();
    }
    return p;
  }
  // proof b's statement; row t = b * EF + i of the pairs and of the responses.  to_limbs throws (std::length_error) on a value the
  // layout cannot carry: callers that receive proofs ask range_layout_carries first.
  void put_statement(size_t b, const BigInt& range, const BigInt& ciphertext) { range.to_limbs(&range_[b * kw], kw); ciphertext.to_limbs(&ct_[b * 2 * kw], 2 * kw); }
  void put_pair(size_t t, const BigInt& c1, const BigInt& c2) { c1.to_limbs(&c1_[t * 2 * kw], 2 * kw); c2.to_limbs(&c2_[t * 2 * kw], 2 * kw); }
  void put_response(size_t t, const Response& rs) {
    const bool open = rs.kind == Response::Open;
    kind_[t] = open ? ZKP_RESP_OPEN : ZKP_RESP_MASK;
    j_[t] = open ? 0 : rs.j;
    (open ? rs.w1 : rs.masked_x).to_limbs(&w1_[t * kw], kw); (open ? rs.r1 : rs.masked_r).to_limbs(&r1_[t * kw], kw);
    if (open) { rs.w2.to_limbs(&w2_[t * kw], kw); rs.r2.to_limbs(&r2_[t * kw], kw); }
    else { std::fill(&w2_[t * kw], &w2_[t * kw] + kw, 0u); std::fill(&r2_[t * kw], &r2_[t * kw] + kw, 0u); }
  }
  void read_pair(size_t t, BigInt& c1, BigInt& c2) const { take_limbs(c1, &c1_[t * 2 * kw], 2 * kw); take_limbs(c2, &c2_[t * 2 * kw], 2 * kw); }
  // into a Response that may hold storage already (RangeProofNi::prove_batch sizes w1, r1, w2, r2 under the GPU call): allocation-free
  // then.  A Mask row moves w1 / r1 over into masked_x / masked_r; w2 / r2 are emptied but KEEP their storage (a free() here goes to the
  // allocating thread's arena, and 16 threads queue for its lock).
  void read_response(size_t t, Response& rs) const {
    take_limbs(rs.w1, &w1_[t * kw], kw); take_limbs(rs.r1, &r1_[t * kw], kw);
    if (kind_[t] == ZKP_RESP_OPEN) {
      rs.kind = Response::Open; rs.j = 0;
      take_limbs(rs.w2, &w2_[t * kw], kw); take_limbs(rs.r2, &r2_[t * kw], kw);
      rs.masked_x.l.clear(); rs.masked_r.l.clear();
    } else {
      rs.kind = Response::Mask; rs.j = j_[t];
      rs.masked_x = std::move(rs.w1); rs.masked_r = std::move(rs.r1);
      rs.w1.l.clear(); rs.r1.l.clear(); rs.w2.l.clear(); rs.r2.l.clear();
    }
  }
  Response response(size_t t) const { Response rs; read_response(t, rs); return rs; }
  // the EF rows of proof b
  void put_pairs(size_t b, const EncryptedPairs& ep) { for (size_t i = 0; i < EF; i++) put_pair(b * EF + i, ep.c1[i], ep.c2[i]); }
  void put_proof(size_t b, const Proof& pr) { for (size_t i = 0; i < EF; i++) put_response(b * EF + i, pr.responses[i]); }
  void read_pairs(size_t b, EncryptedPairs& ep) const {
    ep.c1.resize(EF); ep.c2.resize(EF);
    for (size_t i = 0; i < EF; i++) read_pair(b * EF + i, ep.c1[i], ep.c2[i]);
  }
  void read_proof(size_t b, Proof& pr) const {
    pr.responses.resize(EF);
    for (size_t i = 0; i < EF; i++) read_response(b * EF + i, pr.responses[i]);
  }

 private:
  size_t words(unsigned group, size_t per_proof) const { return groups & group ? rows * per_proof * kw : 0; }
  RawBuf<uint32_t> range_, ct_, c1_, c2_, w1_, r1_, w2_, r2_;
  RawBuf<uint8_t> kind_, j_;
};

// secret_x, secret_r per proof and the (w1, w2, r1, r2) of every row: wiped on release, or by wipe_secrets() where the owner decides
// (on the calling thread, before the blocks go to a background release).  secrets = false: no x / r (generate_encrypted_pairs);
// nonces = false: no w* / r1 / r2 (seeded proving: the GPU expands them itself).
class RangeWitness {
 public:
  const size_t kw, EF;
  RangeWitness(size_t rows, size_t EF_, size_t kw_, bool secrets, bool nonces)
      : kw(kw_), EF(EF_), secrets_(secrets), nonces_(nonces), x_(secrets ? rows * kw_ : 0, true), r_(secrets ? rows * kw_ : 0, true), w1_(nonces ? rows * EF_ * kw_ : 0, true),
        w2_(nonces ? rows * EF_ * kw_ : 0, true), r1_(nonces ? rows * EF_ * kw_ : 0, true), r2_(nonces ? rows * EF_ * kw_ : 0, true) {}
  const uint32_t* x() { return secrets_ ? x_.data() : nullptr; }
  const uint32_t* r() { return secrets_ ? r_.data() : nullptr; }
  zkp_range_ni_witness abi() {
    if (!nonces_) return zkp_range_ni_witness{x(), r(), nullptr, nullptr, nullptr, nullptr};
    return zkp_range_ni_witness{x(), r(), w1_.data(), w2_.data(), r1_.data(), r2_.data()};
  }
  void put_secret(size_t b, const BigInt& x, const BigInt& r) { x.to_limbs(&x_[b * kw], kw); r.to_limbs(&r_[b * kw], kw); }
  void put_nonces(size_t t, const BigInt& w1, const BigInt& w2, const BigInt& r1, const BigInt& r2) {
    w1.to_limbs(&w1_[t * kw], kw); w2.to_limbs(&w2_[t * kw], kw); r1.to_limbs(&r1_[t * kw], kw); r2.to_limbs(&r2_[t * kw], kw);
  }
  void wipe_secrets() { for (RawBuf<uint32_t>* b : {&x_, &r_, &w1_, &w2_, &r1_, &r2_}) b->wipe_now(); }

 private:
  const bool secrets_, nonces_;
  RawBuf<uint32_t> x_, r_, w1_, w2_, r1_, r2_;
};

// The layout at (kw, EF) carries (range, ciphertext, pairs, proof): every value non-negative and within its width, and EF rows stored —
// exactly EF (a RangeProofNi: its own error_factor counts) or at least EF (the interactive verifier reads the first EF).
inline bool range_layout_carries(size_t kw, size_t EF, const BigInt& range, const BigInt& ciphertext, const EncryptedPairs& ep, const Proof& pr, bool exact_rows) {
  for (size_t have : {pr.responses.size(), ep.c1.size(), ep.c2.size()}) if (exact_rows ? have != EF : have < EF) return false;
  if (!range.fits_limbs(kw) || !ciphertext.fits_limbs(2 * kw)) return false;
  for (size_t i = 0; i < EF; i++) {
    const Response& rs = pr.responses[i];
    if (!ep.c1[i].fits_limbs(2 * kw) || !ep.c2[i].fits_limbs(2 * kw)) return false;
    if (rs.kind == Response::Open ? !(rs.w1.fits_limbs(kw) && rs.r1.fits_limbs(kw) && rs.w2.fits_limbs(kw) && rs.r2.fits_limbs(kw))
                                  : !(rs.masked_x.fits_limbs(kw) && rs.masked_r.fits_limbs(kw))) return false;
  }
  return true;
}

// B rows of fixed-width fields, one [B][words] array per field; a secret field (a witness, a nonce) lives in a block that is wiped on
// release.  An output column is written by the GPU call before get() reads it.
struct Column { size_t words; bool secret; };
class Columns {
 public:
  const size_t B;
  Columns(size_t B_, const std::vector<Column>& cols) : B(B_), cols_(cols) {
    for (const Column& c : cols_) buf_.emplace_back(new RawBuf<uint32_t>(B * c.words, c.secret));
  }
  Columns(size_t B_, std::initializer_list<Column> cols) : Columns(B_, std::vector<Column>(cols)) {}
  size_t fields() const { return cols_.size(); }
  size_t words(size_t f) const { return cols_[f].words; }
  uint32_t* operator[](size_t f) { return f < buf_.size() ? buf_[f]->data() : nullptr; }      // (past the last field: null, an unused slot of an ABI struct)
  void put(size_t b, size_t f, const BigInt& v) { v.to_limbs(buf_[f]->data() + b * cols_[f].words, cols_[f].words); }
  void put_row(size_t b, std::initializer_list<const BigInt*> row) { size_t f = 0; for (const BigInt* v : row) put(b, f++, *v); }
  BigInt get(size_t b, size_t f) const { return BigInt::from_limbs(buf_[f]->data() + b * cols_[f].words, cols_[f].words); }
  void wipe_secrets() { for (auto& b : buf_) b->wipe_now(); }

 private:
  std::vector<Column> cols_;
  std::vector<std::unique_ptr<RawBuf<uint32_t>>> buf_;
};

// The batch of zkp_dlog_statement_setup_seeded_batch: the moduli N in; g = h1, ni = h2, the secrets (a secret column, wiped on release) and
// one status byte per statement out.  The moduli of one batch share a kernel width (1024, 2048 or 4096 bits: the narrowest that takes the
// widest of them); a negative modulus or one wider than 4096 bits has no row in this layout and is refused before anything is flattened.
struct DLogSetupBatch {
  static uint32_t width(const std::vector<BigInt>& N) {
    size_t bits = 0;
    for (const BigInt& n : N) {
      if (n.is_negative()) throw std::invalid_argument("DLogStatement::generate_batch_seeded: a negative modulus");
      bits = std::max(bits, n.bit_length());
    }
    if (bits > 4096) throw std::invalid_argument("DLogStatement::generate_batch_seeded: a modulus wider than 4096 bits");
    return bits <= 1024 ? 1024 : bits <= 2048 ? 2048 : 4096;
  }
  const size_t B;
  const uint32_t n_bits, kw;
  Columns in, out;
  std::vector<uint8_t> status;
  explicit DLogSetupBatch(const std::vector<BigInt>& N)
      : B(N.size()), n_bits(width(N)), kw(n_bits / 32), in(B, {{kw, false}}), out(B, {{kw, false}, {kw, false}, {8, true}}), status(B, 9) {
    for (size_t b = 0; b < B; b++) in.put(b, 0, N[b]);
  }
  uint32_t* N() { return in[0]; }
  uint32_t* g() { return out[0]; }
  uint32_t* ni() { return out[1]; }
  uint32_t* secret() { return out[2]; }
  // the first statement without a value (N zero or even, or no h1 of symbol -1 in 128 attempts: a square), B if every one has its own
  size_t first_failed() const { size_t b = 0; while (b < B && status[b] == 0) b++; return b; }
};

}  // namespace zkproofs
