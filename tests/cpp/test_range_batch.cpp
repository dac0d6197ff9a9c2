// host/range_batch.hpp on its own (no GPU, no library): the range-proof slab, its witness counterpart, the carry predicate and the
// column type, at the smallest shape that can go wrong — kw = 32 limbs, EF = 3 rows, two proofs.  tests/test_cpp_range_batch.py builds
// and runs it under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>

#include "../../zk-paillier_amd/host/range_batch.hpp"
using namespace zkproofs;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static const size_t KW = 32, EF = 3, ROWS = 2;

static BigInt max_value(size_t words) { return BigInt::pow2(32 * words) - BigInt::one(); }
static Response open(const BigInt& w1, const BigInt& r1, const BigInt& w2, const BigInt& r2) { Response r; r.kind = Response::Open; r.w1 = w1; r.r1 = r1; r.w2 = w2; r.r2 = r2; return r; }
static Response mask(uint8_t j, const BigInt& x, const BigInt& r) { Response m; m.kind = Response::Mask; m.j = j; m.masked_x = x; m.masked_r = r; return m; }
static bool same(const Response& a, const Response& b) {
  return a.kind == b.kind && a.j == b.j && a.w1 == b.w1 && a.r1 == b.r1 && a.w2 == b.w2 && a.r2 == b.r2 && a.masked_x == b.masked_x && a.masked_r == b.masked_r;
}
static bool all_zero(const uint32_t* p, size_t n) { for (size_t i = 0; i < n; i++) if (p[i]) return false; return true; }

// the six rows every check uses: Open, Mask j = 1, Mask j = 2 | all zero, all 2^(32 kw) - 1 (Open), all 2^(32 kw) - 1 (Mask)
static std::vector<Response> rows() {
  const BigInt top = max_value(KW);
  return {open(BigInt(5), BigInt::pow2(1000), BigInt::pow2(33) + BigInt(7), BigInt(1)), mask(1, BigInt::pow2(700), BigInt(9)), mask(2, BigInt(3), BigInt::pow2(1023)),
          open(BigInt(), BigInt(), BigInt(), BigInt()), open(top, top, top, top), mask(1, top, top)};
}
static void paint(zkp_range_ni_proofs p, uint8_t byte) {      // every array of a full slab, as stale memory would leave it
  std::memset((void*)p.range, byte, ROWS * KW * 4); std::memset((void*)p.ciphertext, byte, ROWS * 2 * KW * 4);
  std::memset(p.c1, byte, ROWS * EF * 2 * KW * 4); std::memset(p.c2, byte, ROWS * EF * 2 * KW * 4);
  for (uint32_t* a : {p.resp_w1, p.resp_r1, p.resp_w2, p.resp_r2}) std::memset(a, byte, ROWS * EF * KW * 4);
  std::memset(p.resp_kind, byte, ROWS * EF); std::memset(p.resp_j, byte, ROWS * EF);
}

static void test_response_round_trip() {
  const std::vector<Response> want = rows();
  RangeSlab s(ROWS, EF, KW, RangeSlab::ALL);
  paint(s.abi(1024, nullptr, 0), 0xFF);
  for (size_t t = 0; t < want.size(); t++) s.put_response(t, want[t]);
  for (size_t t = 0; t < want.size(); t++) CHECK(same(s.response(t), want[t]));
  // the variant that reads into storage that is already there: the same values, and no BigInt changes its block
  for (size_t t = 0; t < want.size(); t++) {
    Response rs;
    for (BigInt* v : {&rs.w1, &rs.r1, &rs.w2, &rs.r2}) v->l.resize(KW);
    const uint32_t *w1 = rs.w1.l.data(), *r1 = rs.r1.l.data(), *w2 = rs.w2.l.data(), *r2 = rs.r2.l.data();
    s.read_response(t, rs);
    CHECK(same(rs, want[t]));
    if (want[t].kind == Response::Open) CHECK(rs.w1.l.data() == w1 && rs.r1.l.data() == r1 && rs.w2.l.data() == w2 && rs.r2.l.data() == r2);
    else CHECK(rs.masked_x.l.data() == w1 && rs.masked_r.l.data() == r1 && rs.w2.l.capacity() >= KW && rs.r2.l.capacity() >= KW);
  }
  // a Response object used twice: nothing of the first row is left in the second
  Response reused;
  s.read_response(1, reused); s.read_response(0, reused); CHECK(same(reused, want[0]));
  s.read_response(0, reused); s.read_response(2, reused); CHECK(same(reused, want[2]));
  // whole proofs
  Proof p0, p1;
  s.read_proof(0, p0); s.read_proof(1, p1);
  CHECK(p0.responses.size() == EF && p1.responses.size() == EF);
  for (size_t i = 0; i < EF; i++) CHECK(same(p0.responses[i], want[i]) && same(p1.responses[i], want[EF + i]));
  RangeSlab s2(ROWS, EF, KW, RangeSlab::RESPONSES);
  s2.put_proof(0, p0); s2.put_proof(1, p1);
  for (size_t t = 0; t < want.size(); t++) CHECK(same(s2.response(t), want[t]));
}

static void test_stale_memory() {
  RangeSlab s(ROWS, EF, KW, RangeSlab::ALL);
  const zkp_range_ni_proofs p = s.abi(1024, nullptr, 0);
  paint(p, 0xFF);
  const std::vector<Response> want = rows();
  for (size_t t = 0; t < want.size(); t++) s.put_response(t, want[t]);
  for (size_t t = 0; t < want.size(); t++) {
    if (want[t].kind == Response::Mask) {
      CHECK(p.resp_kind[t] == ZKP_RESP_MASK && p.resp_j[t] == want[t].j);
      CHECK(all_zero(p.resp_w2 + t * KW, KW) && all_zero(p.resp_r2 + t * KW, KW));
    } else CHECK(p.resp_kind[t] == ZKP_RESP_OPEN && p.resp_j[t] == 0);
  }
  CHECK(all_zero(p.resp_w1 + 3 * KW, KW) && all_zero(p.resp_r1 + 3 * KW, KW) && all_zero(p.resp_w2 + 3 * KW, KW) && all_zero(p.resp_r2 + 3 * KW, KW));   // the all-zero row
  // statement and pairs: every word of the row written as well
  s.put_statement(1, BigInt(1), BigInt(2)); s.put_pair(4, BigInt(3), BigInt());
  CHECK(p.range[KW] == 1 && all_zero(p.range + KW + 1, KW - 1) && p.ciphertext[2 * KW] == 2 && all_zero(p.ciphertext + 2 * KW + 1, 2 * KW - 1));
  CHECK(p.c1[4 * 2 * KW] == 3 && all_zero(p.c1 + 4 * 2 * KW + 1, 2 * KW - 1) && all_zero(p.c2 + 4 * 2 * KW, 2 * KW));
}

static void test_predicate() {
  const std::vector<Response> r = rows();
  const BigInt range = max_value(KW), ct = max_value(2 * KW);
  EncryptedPairs ep;
  for (size_t i = 0; i < EF; i++) { ep.c1.push_back(i ? max_value(2 * KW) : BigInt()); ep.c2.push_back(BigInt::pow2(64 * KW - 1)); }
  const Proof a{{r[0], r[1], r[2]}}, b{{r[3], r[4], r[5]}};
  for (const Proof* pr : {&a, &b}) for (bool exact : {true, false}) CHECK(range_layout_carries(KW, EF, range, ct, ep, *pr, exact));
  auto carries = [&](const BigInt& rg, const BigInt& c, const EncryptedPairs& e, const Proof& pr, bool exact) { return range_layout_carries(KW, EF, rg, c, e, pr, exact); };
  // a negative field, each alone
  CHECK(!carries(-BigInt(1), ct, ep, a, true) && !carries(range, -BigInt(1), ep, a, true));
  for (size_t i = 0; i < EF; i++)
    for (int f = 0; f < 6; f++) {
      Proof bad = a;
      Response& rs = bad.responses[i];
      BigInt* field[6] = {&rs.w1, &rs.r1, &rs.w2, &rs.r2, &rs.masked_x, &rs.masked_r};
      const bool read = rs.kind == Response::Open ? f < 4 : f >= 4;          // the fields of the OTHER variant are not part of the proof
      for (const BigInt& v : {-BigInt(1), BigInt::pow2(32 * KW)}) {          // negative | 32 kw + 1 bits
        const BigInt keep = *field[f];
        *field[f] = v;
        CHECK(carries(range, ct, ep, bad, true) == !read && carries(range, ct, ep, bad, false) == !read);
        *field[f] = keep;
      }
    }
  CHECK(!carries(BigInt::pow2(32 * KW), ct, ep, a, true) && !carries(range, BigInt::pow2(64 * KW), ep, a, true));
  // a pair of 64 kw + 1 bits, a negative pair
  for (size_t i = 0; i < EF; i++)
    for (const BigInt& v : {BigInt::pow2(64 * KW), -BigInt(1)}) {
      EncryptedPairs e1 = ep, e2 = ep;
      e1.c1[i] = v; e2.c2[i] = v;
      CHECK(!carries(range, ct, e1, a, true) && !carries(range, ct, e2, a, true) && !carries(range, ct, e1, a, false) && !carries(range, ct, e2, a, false));
    }
  // row counts: exactly EF for a RangeProofNi, at least EF for the interactive verifier
  Proof longer = a, shorter = a;
  longer.responses.push_back(r[0]); shorter.responses.pop_back();
  CHECK(!carries(range, ct, ep, longer, true) && carries(range, ct, ep, longer, false));
  CHECK(!carries(range, ct, ep, shorter, true) && !carries(range, ct, ep, shorter, false));
  EncryptedPairs more = ep, fewer1 = ep, fewer2 = ep;
  more.c1.push_back(BigInt()); fewer1.c1.pop_back(); fewer2.c2.pop_back();
  CHECK(!carries(range, ct, more, a, true) && carries(range, ct, more, a, false));
  CHECK(!carries(range, ct, fewer1, a, true) && !carries(range, ct, fewer1, a, false) && !carries(range, ct, fewer2, a, true) && !carries(range, ct, fewer2, a, false));
  // what lies past row EF is not looked at
  longer.responses[EF].w1 = -BigInt(1);
  CHECK(carries(range, ct, ep, longer, false));
}

static void test_abi_struct() {
  uint32_t n[KW] = {7};
  RangeSlab s(ROWS, EF, KW, RangeSlab::ALL);
  const zkp_range_ni_proofs p = s.abi(1024, n, KW);
  CHECK(p.n_bits == 1024 && p.error_factor == EF && p.batch == ROWS && p.n_stride == KW && p.n == n);
  const zkp_range_ni_proofs head = s.abi(1024, n, 0, 1);
  CHECK(head.batch == 1 && head.n_stride == 0 && head.c1 == p.c1 && head.resp_kind == p.resp_kind);
  // every pointer lands on the array the writers fill: one distinct value per array, in the last row
  const size_t t = ROWS * EF - 1;
  s.put_statement(ROWS - 1, BigInt(11), BigInt(12)); s.put_pair(t, BigInt(13), BigInt(14));
  s.put_response(t, open(BigInt(15), BigInt(16), BigInt(17), BigInt(18)));
  CHECK(p.range[(ROWS - 1) * KW] == 11 && p.ciphertext[(ROWS - 1) * 2 * KW] == 12 && p.c1[t * 2 * KW] == 13 && p.c2[t * 2 * KW] == 14);
  CHECK(p.resp_w1[t * KW] == 15 && p.resp_r1[t * KW] == 16 && p.resp_w2[t * KW] == 17 && p.resp_r2[t * KW] == 18 && p.resp_kind[t] == ZKP_RESP_OPEN && p.resp_j[t] == 0);
  s.put_response(t, mask(2, BigInt(19), BigInt(20)));
  CHECK(p.resp_w1[t * KW] == 19 && p.resp_r1[t * KW] == 20 && p.resp_kind[t] == ZKP_RESP_MASK && p.resp_j[t] == 2);
  BigInt c1, c2;
  s.read_pair(t, c1, c2);
  CHECK(c1 == BigInt(13) && c2 == BigInt(14));
  EncryptedPairs ep;
  s.read_pairs(ROWS - 1, ep);
  CHECK(ep.c1.size() == EF && ep.c2.size() == EF && ep.c1[EF - 1] == BigInt(13) && ep.c2[EF - 1] == BigInt(14));
  // absent groups are null
  RangeSlab pairs(ROWS, EF, KW, RangeSlab::PAIRS), resp(ROWS, EF, KW, RangeSlab::RESPONSES), head_only(ROWS, EF, KW, RangeSlab::STATEMENT | RangeSlab::RESPONSES);
  const zkp_range_ni_proofs a = pairs.abi(2048, nullptr, 0), b = resp.abi(2048, nullptr, 0), c = head_only.abi(2048, nullptr, 0);
  CHECK(a.n == nullptr && a.n_bits == 2048 && a.c1 && a.c2 && !a.range && !a.ciphertext && !a.resp_kind && !a.resp_j && !a.resp_w1 && !a.resp_r1 && !a.resp_w2 && !a.resp_r2);
  CHECK(!b.c1 && !b.c2 && !b.range && !b.ciphertext && b.resp_kind && b.resp_j && b.resp_w1 && b.resp_r1 && b.resp_w2 && b.resp_r2);
  CHECK(c.range && c.ciphertext && !c.c1 && !c.c2 && c.resp_w1);
  CHECK(!s.large() && !pairs.large());
  // the witness: what is absent is null, what is there is wiped by wipe_secrets
  RangeWitness full(ROWS, EF, KW, true, true), seeded(ROWS, EF, KW, true, false), pairs_only(1, EF, KW, false, true);
  const zkp_range_ni_witness wf = full.abi(), ws = seeded.abi(), wp = pairs_only.abi();
  CHECK(wf.x && wf.r && wf.w1 && wf.w2 && wf.r1 && wf.r2 && wf.x == full.x() && wf.r == full.r());
  CHECK(ws.x && ws.r && !ws.w1 && !ws.w2 && !ws.r1 && !ws.r2);
  CHECK(!wp.x && !wp.r && wp.w1 && wp.w2 && wp.r1 && wp.r2);
  const BigInt top = max_value(KW);
  for (size_t bb = 0; bb < ROWS; bb++) full.put_secret(bb, top, top);
  for (size_t tt = 0; tt < ROWS * EF; tt++) full.put_nonces(tt, top, BigInt(1), BigInt(2), top);
  CHECK(wf.x[ROWS * KW - 1] == ~0u && wf.w1[ROWS * EF * KW - 1] == ~0u && wf.w2[(ROWS * EF - 1) * KW] == 1 && wf.r1[(ROWS * EF - 1) * KW] == 2 && wf.r2[ROWS * EF * KW - 1] == ~0u);
  full.wipe_secrets();
  CHECK(all_zero(wf.x, ROWS * KW) && all_zero(wf.r, ROWS * KW));
  for (const uint32_t* a4 : {wf.w1, wf.w2, wf.r1, wf.r2}) CHECK(all_zero(a4, ROWS * EF * KW));
}

static void test_columns() {
  const uint32_t kw = KW;
  const size_t N = kw, NN = 2 * kw, Z = kw + ZKP_Z1_EXTRA_LIMBS;
  Columns c(2, {{N, false}, {NN, false}, {Z, false}, {8, true}, {16, true}, {768 / 32, false}});
  CHECK(c.B == 2 && c.fields() == 6 && c.words(2) == Z && c.words(3) == 8 && c[6] == nullptr && c[5] != nullptr);
  const size_t widths[6] = {N, NN, Z, 8, 16, 768 / 32};
  std::vector<BigInt> row0, row1;
  for (size_t f = 0; f < 6; f++) { row0.push_back(max_value(widths[f])); row1.push_back(BigInt(f)); }      // the widest value of each field | 0 ... 5
  for (size_t f = 0; f < 6; f++) std::memset(c[f], 0xFF, 2 * widths[f] * 4);
  c.put_row(0, {&row0[0], &row0[1], &row0[2], &row0[3], &row0[4], &row0[5]});
  for (size_t f = 0; f < 6; f++) c.put(1, f, row1[f]);
  for (size_t f = 0; f < 6; f++) {
    CHECK(c.get(0, f) == row0[f] && c.get(1, f) == row1[f]);
    CHECK(c[f][widths[f] - 1] == ~0u && c[f][widths[f]] == f && all_zero(c[f] + widths[f] + 1, widths[f] - 1));       // [B][words], every word written
  }
  bool threw = false;
  try { c.put(0, 3, BigInt::pow2(256)); } catch (const std::length_error&) { threw = true; }      // one bit too wide for its column
  CHECK(threw);
  threw = false;
  try { c.put(0, 0, -BigInt(1)); } catch (const std::length_error&) { threw = true; }
  CHECK(threw);
  c.wipe_secrets();
  CHECK(all_zero(c[3], 2 * 8) && all_zero(c[4], 2 * 16) && c.get(0, 3) == BigInt() && c.get(1, 4) == BigInt());
  CHECK(c.get(0, 0) == row0[0] && c.get(1, 5) == row1[5]);                 // what is not secret is left alone
}

int main() {
  test_response_round_trip();
  test_stale_memory();
  test_predicate();
  test_abi_struct();
  test_columns();
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("range_batch ok\n");
  return 0;
}
