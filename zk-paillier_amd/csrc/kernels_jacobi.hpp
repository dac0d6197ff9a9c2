// kernels_jacobi.hpp — the Jacobi symbol (a / n) for odd n, one pair of big integers per lane, and what is built on it: the reference's
// legendre_symbol (wi_dlog_proof.rs:94-107) and the set-up of a DLogStatement "per definition 3 in the paper" (wi_dlog_proof.rs:117-141:
// h1 drawn until its symbol is -1, secret < 2^256, h2 = (h1^-1)^secret mod N).
//
// Algorithm: the binary algorithm for the symbol is the binary GCD with a sign — while a != 0: an even a is halved, and (2 / b) = -1 for
// b = 3, 5 mod 8 flips the sign; an odd a < b is swapped with b, and reciprocity flips the sign when a = b = 3 mod 4; then a <- a - b.  At
// a == 0 the symbol is the sign if b == 1 and 0 otherwise.  wb_jacobi runs it in the form of wb_gcd (kernels_gcd.hpp): up to JAC_K = 28
// steps on 64-bit approximations (xa, xb) — the low 30 bits of (a, b) glued to their 34 bits below the common bit length n — recorded in
// a 2x2 matrix that one pass applies to the full operands, (a, b) <- ((f0 a + g0 b) >> sh, (f1 a + g1 b) >> sh), sh = steps taken.
//
// wb_gcd tolerates two things a symbol cannot; here both are excluded, so every step is a step of the exact algorithm:
//  (i) Low bits.  xa = a and xb = b mod 2^30 at the start, and the matrix relation 2^i xa_i = f0 xa + g0 xb (the same for xb_i) holds
//      for the approximations and the operands alike, so after i steps xa_i = a_i and xb_i = b_i mod 2^(30 - i).  A step reads the
//      parity of a_i, a_i mod 4 and b_i mod 8: three bits, exact while 30 - i >= 3.  Hence JAC_K = 28 and not 30.
//  (ii) Signs.  With s = n - 34, a~ = xa 2^(s - 30) differs from a by less than 2^s (the bits between the two glued parts), and so does
//      b~ from b.  Rows of the matrix keep |f| + |g| <= 2^i, so a_i - a~_i = (f0 (a - a~) + g0 (b - b~)) / 2^i is below 2^s in
//      magnitude at EVERY step, and the same for b_i: the error does not grow.  In units of xa that is 2^30 each.  So an odd step's
//      comparison is decided by the approximations whenever |xa_i - xb_i| >= 2^31 (Lehmer's condition), and a step is taken only then:
//      no operand ever comes out negative, and reciprocity is only applied to the positive values it holds for.  Where the condition
//      fails the round ends early with the steps it has (sh = i); where it fails at the round's first step (operands that agree in their
//      top 33 bits or so, a == b included) that ONE step is decided by an exact top-down comparison of the full operands and ends the
//      round.  With n <= 64 the approximations are the operands and every comparison is exact.
// Every loop is bounded by the operand length: a step removes at least one bit from len(a) + len(b) (a halving from a; an odd step
// replaces the larger operand by less than half of it), a round takes at least one step, so there are at most 64 kw rounds — typically
// 64 kw / 28 / 1.4, as Lehmer's condition fails with probability about 2^-32 per odd step on operands nobody chose.
// tools/wbjacobi_model.py is the word-for-word Python model of wb_jacobi (integer ranges asserted); tests/jacobi_model.py is the symbol
// from its definition, which both are held to.
//
// Data layout: as kernels_gcd.hpp — operands in thread-interleaved LDS (word w of this lane at p[w * S]), chunks of GCD_CH words.
#pragma once
#include "kernels_coprime.hpp"

namespace zkp {

constexpr int JAC_K = 28;                      // steps per round at most: 30 exact low bits, 3 of them read by the last step
constexpr uint64_t JAC_MARGIN = 1ull << 31;    // |xa - xb| from which the approximations decide the comparison

// (a / b) for an odd b; a any value.  a, b: kw words each in LDS, consumed.  Returns -1, 0 or 1.
__device__ __forceinline__ int wb_jacobi(uint32_t* a, uint32_t* b, int kw, int S) {
  int na = kw, nb = kw;
  uint32_t t = 0;                                                 // bit 0: the sign so far
  for (int round = 0; round < 64 * kw; round++) {
    while (na > 0 && a[(na - 1) * S] == 0) na--;
    if (na == 0) break;
    while (nb > 1 && b[(nb - 1) * S] == 0) nb--;
    const int la = 32 * na - __builtin_clz(a[(na - 1) * S]);
    const int lb = 32 * nb - __builtin_clz(b[(nb - 1) * S]);
    const int n = la > lb ? la : lb;
    const bool exact = n <= 64;
    uint64_t xa, xb;
    if (exact) {
      xa = (uint64_t)a[0] | ((uint64_t)(kw > 1 ? a[S] : 0u) << 32);
      xb = (uint64_t)b[0] | ((uint64_t)(kw > 1 ? b[S] : 0u) << 32);
    } else {
      xa = (gcd_top34(a, S, kw, n - 34) << GCD_K) | (a[0] & GCD_MK);
      xb = (gcd_top34(b, S, kw, n - 34) << GCD_K) | (b[0] & GCD_MK);
    }
    const int nw0 = na > nb ? na : nb;
    // ---- up to JAC_K steps on the approximations, each one only while it is a step of the exact algorithm
    int32_t f0 = 1, g0 = 0, f1 = 0, g1 = 1;
    int sh = 0;
    for (int i = 0; i < JAC_K; i++) {
      const bool odd = (xa & 1) != 0;
      bool sw = odd && xa < xb, last = false;
      if (odd && !exact && (sw ? xb - xa : xa - xb) < JAC_MARGIN) {
        if (i > 0) break;                                         // undecided: the round ends with the steps it has
        int c = 0;                                                // the round's first step: decided on the full operands
        for (int w = nw0 - 1; w >= 0 && c == 0; w--) {
          const uint32_t x = a[w * S], y = b[w * S];
          if (x != y) c = x < y ? -1 : 1;
        }
        sw = c < 0;
        last = true;                                              // (xa - xb may have the wrong sign now: no further step on it)
      }
      t ^= (uint32_t)sw & (uint32_t)(xa >> 1) & (uint32_t)(xb >> 1);                  // reciprocity: a = b = 3 mod 4
      const uint64_t ta = sw ? xb : xa, tb = sw ? xa : xb;
      const int32_t tf0 = sw ? f1 : f0, tg0 = sw ? g1 : g0, tf1 = sw ? f0 : f1, tg1 = sw ? g0 : g1;
      t ^= (uint32_t)(tb >> 1) ^ (uint32_t)(tb >> 2);                                 // the halving: (2 / b) = -1 for b = 3, 5 mod 8
      xa = (odd ? ta - tb : ta) >> 1;
      xb = tb;
      f0 = odd ? tf0 - tf1 : tf0;
      g0 = odd ? tg0 - tg1 : tg0;
      f1 = tf1 * 2;
      g1 = tg1 * 2;
      sh = i + 1;
      if (last) break;
    }
    // ---- (a, b) <- ((f0 a + g0 b) >> sh, (f1 a + g1 b) >> sh) in one pass, 1 <= sh <= 28; |f| + |g| <= 2^28 keeps every sum inside int64.
    // Both results are the non-negative operands of the exact algorithm: nothing to negate.
    const int nw = (nw0 + GCD_CH - 1) / GCD_CH * GCD_CH;          // (words above a live count are zero: a chunk may run past it)
    int64_t accA = 0, accB = 0;
    uint32_t pA = 0, pB = 0;
    for (int w0 = 0; w0 < nw; w0 += GCD_CH) {
      uint32_t A[GCD_CH], Bv[GCD_CH], Ta[GCD_CH], Tb[GCD_CH];
#pragma unroll
      for (int k = 0; k < GCD_CH; k++) { A[k] = a[(w0 + k) * S]; Bv[k] = b[(w0 + k) * S]; }
#pragma unroll
      for (int k = 0; k < GCD_CH; k++) {
        const int64_t aw = (int64_t)(uint64_t)A[k], bw = (int64_t)(uint64_t)Bv[k];
        accA += (int64_t)f0 * aw + (int64_t)g0 * bw;
        accB += (int64_t)f1 * aw + (int64_t)g1 * bw;
        Ta[k] = (uint32_t)accA; accA >>= 32;
        Tb[k] = (uint32_t)accB; accB >>= 32;
      }
#pragma unroll
      for (int k = 0; k < GCD_CH; k++) {
        if (w0 + k > 0) {
          a[(w0 + k - 1) * S] = ((k ? Ta[k - 1] : pA) >> sh) | (Ta[k] << (32 - sh));
          b[(w0 + k - 1) * S] = ((k ? Tb[k - 1] : pB) >> sh) | (Tb[k] << (32 - sh));
        }
      }
      pA = Ta[GCD_CH - 1]; pB = Tb[GCD_CH - 1];
    }
    a[(nw - 1) * S] = (pA >> sh) | ((uint32_t)accA << (32 - sh));
    b[(nw - 1) * S] = (pB >> sh) | ((uint32_t)accB << (32 - sh));
    na = nb = nw;                                                 // either result may be as long as the longer input
  }
  while (nb > 1 && b[(nb - 1) * S] == 0) nb--;
  const bool one = nb == 1 && b[0] == 1u && na == 0;
  return one ? ((t & 1u) ? -1 : 1) : 0;
}

// ---- zkp_jacobi_batch: symbol[i] = (a[i] / n[i]); an even n (zero included) is outside the domain: symbol 0, status 2
struct JacobiArgs {
  const uint32_t* a;
  const uint32_t* n; uint64_t n_stride;
  int32_t* symbol;
  uint8_t* status;            // nullable
  uint64_t count; int kw;
};
constexpr size_t jacobi_lds_words_per_lane(uint32_t kw) { return 2 * (size_t)kw; }

__global__ void __launch_bounds__(64) k_jacobi(JacobiArgs q) {
  extern __shared__ __align__(16) uint32_t jac_lds[];
  const int S = (int)blockDim.x, kw = q.kw;
  const uint64_t item = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (item >= q.count) return;
  const uint32_t* A = q.a + item * (uint64_t)kw;
  const uint32_t* N = q.n + item * q.n_stride;
  const bool domain = (N[0] & 1u) != 0;
  int sym = 0;
  if (domain) {
    uint32_t* pa = jac_lds + threadIdx.x;
    uint32_t* pb = pa + (size_t)kw * S;
    for (int w = 0; w < kw; w++) { pa[w * S] = A[w]; pb[w * S] = N[w]; }
    sym = wb_jacobi(pa, pb, kw, S);
  }
  q.symbol[item] = sym;
  if (q.status) q.status[item] = domain ? 0 : 2;
}

// ---- zkp_legendre_batch: the two kernels around the modexp launch.  Domain (that of zkp_modinv_batch): p odd, p >= 3, a < p.
struct LegendreArgs {
  const uint32_t* a;
  const uint32_t* p; uint64_t p_stride;
  uint32_t* base;             // [count][kw]   a, or 0 outside the domain
  uint32_t* exp;              // [count][kw]   (p - 1) >> 1, or 0 outside the domain
  const uint32_t* ls;         // [count][kw]   base^exp mod p (k_legendre_finish)
  int32_t* symbol;
  uint8_t* status;            // [count]
  uint64_t count; int kw;
};

__global__ void __launch_bounds__(256) k_legendre_prep(LegendreArgs q) {
  const uint64_t item = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= q.count) return;
  const int kw = q.kw;
  const uint32_t* A = q.a + item * (uint64_t)kw;
  const uint32_t* P = q.p + item * q.p_stride;
  int cmp = 0;
  bool p_small = P[0] < 3;
  for (int w = kw - 1; w >= 0; w--) {
    const uint32_t aw = A[w], pw = P[w];
    if (cmp == 0 && aw != pw) cmp = aw > pw ? 1 : -1;
    if (w > 0) p_small = p_small && pw == 0;
  }
  const bool ok = (P[0] & 1u) && !p_small && cmp < 0;
  uint32_t* base = q.base + item * (uint64_t)kw;
  uint32_t* e = q.exp + item * (uint64_t)kw;
  for (int w = 0; w < kw; w++) {
    base[w] = ok ? A[w] : 0u;
    const uint32_t lo = w == 0 ? P[0] - 1u : P[w];                // (p odd: p - 1 clears bit 0, no borrow)
    const uint32_t hi = w + 1 < kw ? P[w + 1] : 0u;
    e[w] = ok ? (lo >> 1) | (hi << 31) : 0u;
  }
  q.status[item] = ok ? 0 : 2;
}

__global__ void __launch_bounds__(256) k_legendre_finish(LegendreArgs q) {
  const uint64_t item = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= q.count) return;
  const uint32_t* ls = q.ls + item * (uint64_t)q.kw;
  bool one = ls[0] == 1u;
  for (int w = 1; w < q.kw; w++) one = one && ls[w] == 0u;
  q.symbol[item] = q.status[item] ? 0 : one ? 1 : -1;             // `if ls == BigInt::one() { 1 } else { -1 }` (:102-106)
}

// ---- the seeded set-up of a DLogStatement: stream kind 8 of the nonce construction (include/zkp_hip.h, DESIGN.md section 4;
// tests/seeded_dlog_setup_model.py restates it).  field 0: h1 = sample_jacobi_minus_below(N) — attempt t is the candidate v that
// sample_below(N) would look at in attempt t, taken when v + 1 < N (the reference's sample_range(1, N - 1) draws below N - 1) AND
// (v / N) == -1; one counter for both sorts of rejection, so wb_jacobi sits in the draw: k_nonce_coprime's shape.  field 1: secret = words
// 0 .. 7 of block 0.  A statement without a value (N zero or even, max_attempts rejections — certain for a square N) is MALFORMED and
// this kernel leaves its h1 and secret rows zero.  h1 is public; the secret goes straight to its row and never to LDS.
struct NonceJacobiArgs {
  const uint32_t* key;        // the seed as 8 little-endian words (device memory)
  const uint32_t* n;          // [B][kw]
  uint32_t* out;              // [B][kw]  h1
  uint32_t* secret;           // [B][8]
  uint8_t* status;            // [B] 0 | ZKP_VERDICT_MALFORMED, written for every statement
  uint64_t first_index, batch;
  uint32_t kw, kind, max_attempts;
};

__global__ void __launch_bounds__(64) k_nonce_jacobi(NonceJacobiArgs a) {
  extern __shared__ __align__(16) uint32_t jac_lds[];
  const int S = (int)blockDim.x, kw = (int)a.kw;
  const uint64_t b = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (b >= a.batch) return;
  const uint32_t* n = a.n + b * a.kw;
  uint32_t* out = a.out + b * a.kw;
  uint32_t* sec = a.secret + b * 8;
  uint32_t bits = 0;
  for (int i = kw - 1; i >= 0 && !bits; i--) {
    const uint32_t nv = n[i];
    if (nv) bits = 32u * (uint32_t)i + 32u - (uint32_t)__builtin_clz(nv);
  }
  bool ok = false;
  if (bits != 0 && (n[0] & 1u)) {
    uint32_t* pa = jac_lds + threadIdx.x;                        // the candidate, then wb_jacobi's a
    uint32_t* pb = pa + (size_t)kw * S;                          // N, then wb_jacobi's b
    const uint32_t nw = (bits + 31) / 32, nb = (nw + 15) / 16;   // (16 nb <= kw: kw is a multiple of 16)
    const uint32_t topmask = (bits & 31u) ? (1u << (bits & 31u)) - 1u : 0xffffffffu;
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = a.key[i];
    const uint64_t index = a.first_index + b;
    const uint32_t n0 = (uint32_t)index, n1 = (uint32_t)(index >> 32), n2 = nonce_word15(a.kind, 0u, 0u);
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
      int c = 0;                                                 // candidate + 1 < N ?
      for (int w = (int)nw - 1; w >= 1 && c == 0; w--) {
        const uint32_t x = pa[w * S], y = n[w];
        if (x != y) c = x < y ? -1 : 1;
      }
      if (c == 0) c = pa[0] < n[0] - 1u ? -1 : 1;                // equal above word 0: x + 1 < y, y odd
      if (c >= 0) continue;
      for (int w = 0; w < kw; w++) { out[w] = pa[w * S]; pb[w * S] = n[w]; }
      ok = wb_jacobi(pa, pb, kw, S) == -1;
    }
    if (ok) {
      uint32_t v[16];
      chacha20_block(key, 0u, n0, n1, nonce_word15(a.kind, 0u, 1u), v);
#pragma unroll
      for (int i = 0; i < 8; i++) sec[i] = v[i];
    }
  }
  if (!ok) {
    for (int w = 0; w < kw; w++) out[w] = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) sec[i] = 0u;
  }
  a.status[b] = ok ? 0 : 2;
}

// a MALFORMED statement's h2 is zero as well (its modexp ran on a zero base, or under a modulus k_setup refused and stored nothing)
__global__ void __launch_bounds__(256) k_dlog_setup_finish(const uint8_t* __restrict__ status, uint32_t* __restrict__ ni, uint32_t kw, uint64_t batch) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= batch * kw) return;
  if (status[gid / kw]) ni[gid] = 0u;
}

}  // namespace zkp
