// The plain-C++ half of DLogStatement::generate_batch_seeded (zk-paillier_amd/host/range_batch.hpp: DLogSetupBatch): the argument checks
// and the flattening of the moduli into the [B][kw] array of zkp_dlog_statement_setup_seeded_batch, the columns the call writes, and the
// wipe of the secret column — as a program of its own under the address and undefined-behaviour sanitizers.  No GPU, no library.
#include <cstdio>
#include <cstring>

#include "../../zk-paillier_amd/host/range_batch.hpp"
using namespace zkproofs;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool all_zero(const uint32_t* p, size_t n) { for (size_t i = 0; i < n; i++) if (p[i]) return false; return true; }
template <class F> static bool refuses(F f) { try { f(); } catch (const std::invalid_argument&) { return true; } return false; }

static void test_width() {
  const BigInt one = BigInt::one();
  CHECK(DLogSetupBatch::width({BigInt(15)}) == 1024 && DLogSetupBatch::width({BigInt()}) == 1024);
  CHECK(DLogSetupBatch::width({BigInt::pow2(1024) - one}) == 1024 && DLogSetupBatch::width({BigInt::pow2(1024)}) == 2048);
  CHECK(DLogSetupBatch::width({BigInt::pow2(2048) - one}) == 2048 && DLogSetupBatch::width({BigInt::pow2(2048) + one}) == 4096);
  CHECK(DLogSetupBatch::width({BigInt::pow2(4096) - one}) == 4096);
  // the widest modulus of a batch decides for all of it
  CHECK(DLogSetupBatch::width({BigInt(15), BigInt::pow2(3000) + one, BigInt::pow2(1500) + one}) == 4096);
  CHECK(refuses([&] { (void)DLogSetupBatch::width({BigInt(15), BigInt::pow2(4096)}); }));
  CHECK(refuses([&] { (void)DLogSetupBatch::width({-BigInt(15)}); }));
  CHECK(refuses([&] { DLogSetupBatch q({BigInt(7), -BigInt::pow2(100)}); }));
}

static void test_flatten_and_read_back() {
  const std::vector<BigInt> N{BigInt::pow2(1023) + BigInt(0x1235), BigInt(15), BigInt(), BigInt::pow2(1024) - BigInt::one()};
  DLogSetupBatch q(N);
  CHECK(q.B == 4 && q.n_bits == 1024 && q.kw == 32 && q.status.size() == 4);
  CHECK(q.N() == q.in[0] && q.g() == q.out[0] && q.ni() == q.out[1] && q.secret() == q.out[2] && q.in.words(0) == 32 && q.out.words(2) == 8);
  // every word of every row is written, whatever the staging block held: short moduli are zero-extended
  for (size_t b = 0; b < 4; b++) CHECK(BigInt::from_limbs(q.N() + b * 32, 32) == N[b]);
  CHECK(q.N()[0] == 0x1235 && q.N()[31] == 0x80000000u && q.N()[32] == 15 && all_zero(q.N() + 33, 31) && all_zero(q.N() + 64, 32));
  for (size_t w = 0; w < 32; w++) CHECK(q.N()[96 + w] == 0xffffffffu);
  // the status starts as "not written" and the first failing statement is the one reported
  CHECK(q.first_failed() == 0);
  std::memset(q.status.data(), 0, 4);
  CHECK(q.first_failed() == 4);
  q.status[2] = ZKP_VERDICT_MALFORMED;
  q.status[3] = ZKP_VERDICT_MALFORMED;
  CHECK(q.first_failed() == 2);
  // what the call writes is what is read back; the secret column alone is wiped
  for (size_t i = 0; i < 4 * 32; i++) { q.g()[i] = (uint32_t)(i + 1); q.ni()[i] = (uint32_t)(0x9000 + i); }
  for (size_t i = 0; i < 4 * 8; i++) q.secret()[i] = (uint32_t)(0x5000 + i);
  CHECK(q.out.get(1, 0) == BigInt::from_limbs(q.g() + 32, 32) && q.out.get(3, 1) == BigInt::from_limbs(q.ni() + 96, 32));
  CHECK(q.out.get(2, 2) == BigInt::from_limbs(q.secret() + 16, 8) && q.out.get(2, 2).bit_length() <= 256 && !q.out.get(2, 2).is_zero());
  q.out.wipe_secrets();
  CHECK(all_zero(q.secret(), 4 * 8) && q.out.get(2, 2).is_zero() && q.g()[5] == 6 && q.ni()[7] == 0x9007);
}

static void test_wider_batches_and_the_empty_one() {
  DLogSetupBatch q({BigInt(15), BigInt::pow2(2047) + BigInt::one()});
  CHECK(q.n_bits == 2048 && q.kw == 64 && q.N()[0] == 15 && all_zero(q.N() + 1, 63) && q.N()[64] == 1 && q.N()[127] == 0x80000000u);
  DLogSetupBatch w({BigInt::pow2(4095) + BigInt::one()});
  CHECK(w.n_bits == 4096 && w.kw == 128 && w.N()[127] == 0x80000000u && w.out.words(0) == 128 && w.out.words(1) == 128);
  DLogSetupBatch none(std::vector<BigInt>{});
  CHECK(none.B == 0 && none.first_failed() == 0 && none.n_bits == 1024);
}

int main() {
  test_width();
  test_flatten_and_read_back();
  test_wider_batches_and_the_empty_one();
  if (failures) return 1;
  std::printf("dlog_setup_host ok\n");
  return 0;
}
