// kernels_coprime.hpp — the nonce VerlinProof::prove and MulProof::prove redraw until it is coprime to n (verlin_proof.rs:64-67: r_a;
// multiplication_proof.rs:62, 148-154: r_d), expanded on the device from the 32-byte seed (include/zkp_hip.h:
// zkp_nonce_sample_coprime_batch; the rule is in DESIGN.md section 4, tests/seeded_coprime_model.py restates it).
//
// sample_coprime_below(n): attempt t is the candidate sample_below(n) would look at in attempt t (kernels_sample.hpp: the nw first words
// of blocks [t nb, (t + 1) nb), the top limb masked); it is taken when it is < n AND gcd(candidate, n) == 1.  One counter for both sorts
// of rejection, so the test is part of the draw and cannot be a pass over finished draws: k_nonce_sample's lanes-per-value geometry has
// no GCD, and the word-batched GCD (kernels_gcd.hpp) is one lane per value.  Hence k_modinv's shape: one lane per value, both operands in
// thread-interleaved LDS (word w of this lane at p[w * S]), the ChaCha state of an attempt in this lane's registers as in k_nonce_raw.
// The loop has no cross-lane operation: lanes that are done idle until the slowest of their wavefront is.  Every loop is bounded
// (max_attempts; wb_gcd's rounds by the operand length).
#pragma once
#include "kernels_gcd.hpp"
#include "kernels_sample.hpp"

namespace zkp {

struct NonceCoprimeArgs {
  const uint32_t* key;        // the seed as 8 little-endian words (device memory)
  const uint32_t* n; uint64_t n_stride;
  const uint32_t* meta;       // [B] bit_length(n)                 (written by k_nonce_prep)
  uint32_t* out;              // [B][kw]
  uint8_t* status;            // [B] 0 | ZKP_VERDICT_MALFORMED     (k_nonce_prep wrote it; this kernel only ever raises it)
  uint64_t first_index, batch;
  uint32_t kw, kind, field, max_attempts;
};
constexpr size_t coprime_lds_words_per_lane(uint32_t kw) { return 2 * (size_t)kw; }

// What is left of the secret in LDS when a lane ends: nothing.  An accepted candidate went to its output row BEFORE the GCD, which
// consumes its operands — after wb_gcd a == 0 and b == gcd == 1.  A lane that ends without a value (a zero or even n, max_attempts
// rejections) may leave its last rejected candidate behind; no nonce is made of it, and k_nonce_fixup zeroes the row it was stored to.
__global__ void __launch_bounds__(64) k_nonce_coprime(NonceCoprimeArgs a) {
  extern __shared__ __align__(16) uint32_t cop_lds[];
  const int S = (int)blockDim.x, kw = (int)a.kw;
  const uint64_t b = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (b >= a.batch) return;
  const uint32_t bits = a.meta[b];
  if (bits == 0) return;                                         // n == 0: k_nonce_prep has set the status
  const uint32_t* n = a.n + b * a.n_stride;
  if (!(n[0] & 1u)) { a.status[b] = 2; return; }                 // an even n is outside the domain of wb_gcd (b odd) and of the limb kernels
  uint32_t* pa = cop_lds + threadIdx.x;                          // the candidate, then the GCD's a
  uint32_t* pb = pa + (size_t)kw * S;                            // n, then the GCD's b
  uint32_t* out = a.out + b * a.kw;
  const uint32_t nw = (bits + 31) / 32, nb = (nw + 15) / 16;     // (16 nb <= kw: kw is a multiple of 16)
  const uint32_t topmask = (bits & 31u) ? (1u << (bits & 31u)) - 1u : 0xffffffffu;
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; i++) key[i] = a.key[i];
  const uint64_t index = a.first_index + b;
  const uint32_t n0 = (uint32_t)index, n1 = (uint32_t)(index >> 32), n2 = nonce_word15(a.kind, 0u, a.field);

  bool ok = false;
  for (uint32_t t = 0; t < a.max_attempts && !ok; t++) {
    for (uint32_t k = 0; k < nb; k++) {
      uint32_t v[16];
      chacha20_block(key, t * nb + k, n0, n1, n2, v);
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint32_t wi = 16 * k + i;
        pa[wi * S] = wi >= nw ? 0u : wi == nw - 1 ? v[i] & topmask : v[i];
      }
    }
    for (int w = 16 * (int)nb; w < kw; w++) pa[w * S] = 0u;
    int c = 0;
    for (int w = (int)nw - 1; w >= 0 && c == 0; w--) {
      const uint32_t x = pa[w * S], y = n[w];
      if (x != y) c = x < y ? -1 : 1;
    }
    if (c >= 0) continue;                                        // not below n
    for (int w = 0; w < kw; w++) { out[w] = pa[w * S]; pb[w * S] = n[w]; }
    const int lb = wb_gcd<false>(pa, pb, nullptr, nullptr, nullptr, 0u, kw, S);
    ok = pb[0] == 1u;
    for (int w = 1; w < lb; w++) ok = ok && pb[w * S] == 0u;     // (candidate 0: gcd == n, taken for n == 1 alone)
  }
  if (!ok) a.status[b] = 2;                                      // every nonce of the proof is zeroed by k_nonce_fixup
}

}  // namespace zkp
