// kernels_paillier_dec.hpp — the arithmetic around the ladder in Paillier decryption and opening with the factors (zkp_paillier_open_batch):
//   x_p = (c mod p^2)^(p-1) mod p^2, L_p = (x_p - 1) / p, m_p = L_p h_p mod p, m = m_p + p ((m_q - m_p) pinv mod q)      (and q alike)
//   r_p = (c mod p)^(d_p) mod p,                            r = r_p + p ((r_q - r_p) pinv mod q)
// with h_p = (p - (q mod p))^-1 mod p, pinv = p^-1 mod q, d_p = q^-1 mod (p - 1).  The exponentiations run on the modexp ladder; the kernels
// here prepare a key (k_pdec_key_a, k_modinv, k_pdec_key_b), split a ciphertext into the ladder's rows (k_pdec_split) and recombine what the
// ladder returns (k_pdec_finish).  tests/paillier_dec_model.py states the values; tools/paillier_dec_model.py is the word-for-word model of
// pd_mod, pd_divexact and the even-modulus inverse, with the integer ranges asserted.
//
// Three routines carry everything:
//  * pd_mod — x mod m for an x of any length: Knuth's algorithm D on 32-bit digits.  The divisor is normalised (top bit set), a quotient
//    digit is estimated from the top two digits of the running remainder over the top digit of m, corrected against the second digit of m
//    (then it is at most one too large), and one multiply-subtract over m's digits with an add-back on borrow settles it.
//  * pd_divexact — x / d for an odd d, quotient below 2^(32 nq): digit i of the quotient is x_i d^-1 mod 2^32 (the Hensel inverse of d taken
//    one word at a time: the same value as the low-half product with d^-1 mod 2^(32 nq)), and x <- x - q_i d 2^(32 i).  The division was
//    exact iff every word of x is zero afterwards: with nx >= nq + nd both x and Q d are below 2^(32 nx), so they are equal when they agree
//    modulo it.  That comparison is the domain test of an item: x_p = 1 mod p.
//  * the inverse modulo the EVEN p - 1: with M = p - 1 and y = M^-1 mod q (odd modulus: k_modinv), M y = 1 + t q, so t = (M y - 1) / q is an
//    exact division, and -t q = 1 mod M: d_p = M - t (0 < t < M, as 0 < y < q).
// h_q needs no inverse of its own: (q - (p mod q))^-1 = -(p^-1) = q - pinv mod q.
// The split and finish kernels of kernels_ck_prove.hpp and kernels_ck_inter.hpp compute other rows with the same pieces: the ladder-row
// writers (pd_row_null, pd_row_put, pd_exp_put), pd_load_pair, and the recombination pd_crt over its LDS carve PdCrtLds.
//
// Data layout: as kernels_gcd.hpp — one value per lane, operands in thread-interleaved LDS (word w of this lane at x[w * S]).  Trip counts
// depend on the operands' lengths only, but nothing here is claimed to run in constant time (the quotient correction and the add-back are
// data-dependent branches).
#pragma once
#include "kernels_inv.hpp"

namespace zkp {

// The inner loops run in chunks of PD_CH words, as kernels_gcd.hpp's do: the LDS reads of a chunk are issued before its first store, so a
// lane waits for the LDS once per chunk and not once per word.  The values are those of the word-by-word loops of the model.
constexpr int PD_CH = 8;

__device__ __forceinline__ uint32_t pd_inv32(uint32_t d0) {        // d0^-1 mod 2^32 for an odd d0
  uint32_t v = d0;
#pragma unroll
  for (int it = 0; it < 5; it++) v *= 2u - d0 * v;
  return v;
}

// out[0 .. na + nb) = a * b.  a: LDS (stride S), b: any memory (stride bs); out does not alias either.
__device__ __forceinline__ void pd_mul(uint32_t* out, const uint32_t* a, int na, const uint32_t* b, int bs, int nb, int S) {
  for (int w = 0; w < na + nb; w++) out[w * S] = 0u;
  for (int i = 0; i < nb; i++) {
    const uint64_t bi = b[i * bs];
    uint64_t carry = 0;
    int j0 = 0;
    for (; j0 + PD_CH <= na; j0 += PD_CH) {
      uint32_t A[PD_CH], O[PD_CH];
#pragma unroll
      for (int k = 0; k < PD_CH; k++) { A[k] = a[(j0 + k) * S]; O[k] = out[(i + j0 + k) * S]; }
#pragma unroll
      for (int k = 0; k < PD_CH; k++) {
        const uint64_t t = bi * A[k] + O[k] + carry;                // <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        O[k] = (uint32_t)t;
        carry = t >> 32;
      }
#pragma unroll
      for (int k = 0; k < PD_CH; k++) out[(i + j0 + k) * S] = O[k];
    }
    for (int j = j0; j < na; j++) {                                 // (a length that is no multiple of the chunk)
      const uint64_t t = bi * a[j * S] + out[(i + j) * S] + carry;
      out[(i + j) * S] = (uint32_t)t;
      carry = t >> 32;
    }
    out[(i + na) * S] = (uint32_t)carry;
  }
}

// x <- x mod m in place.  x: nx + 1 words of LDS, the value in words 0 .. nx - 1 (word nx is scratch); m: nmf words of any memory
// (stride ms), m != 0, nx >= nmf; mn: nmf words of LDS (the normalised divisor).  Afterwards words 0 .. nx of x hold the remainder.
__device__ __forceinline__ void pd_mod(uint32_t* x, int nx, const uint32_t* m, int ms, int nmf, uint32_t* mn, int S) {
  int nm = nmf;
  while (nm > 1 && m[(nm - 1) * ms] == 0u) nm--;
  const int s = __builtin_clz(m[(nm - 1) * ms]);
  for (int w = nm - 1; w >= 0; w--) {
    const uint32_t hi = m[w * ms], lo = w ? m[(w - 1) * ms] : 0u;
    mn[w * S] = s ? (hi << s) | (lo >> (32 - s)) : hi;
  }
  x[nx * S] = s ? x[(nx - 1) * S] >> (32 - s) : 0u;
  for (int w = nx - 1; w >= 0; w--) {
    const uint32_t hi = x[w * S], lo = w ? x[(w - 1) * S] : 0u;
    x[w * S] = s ? (hi << s) | (lo >> (32 - s)) : hi;
  }
  const uint64_t v1 = mn[(nm - 1) * S], v2 = nm > 1 ? mn[(nm - 2) * S] : 0u;
  for (int j = nx - nm; j >= 0; j--) {
    // the running remainder x[j .. j + nm] is below mn 2^32: its top digit is at most v1, the estimate at most 2^32 + 1
    const uint64_t num = ((uint64_t)x[(j + nm) * S] << 32) | x[(j + nm - 1) * S];
    uint64_t qh = num / v1, rh = num % v1;
    const uint64_t x2 = j + nm >= 2 ? x[(j + nm - 2) * S] : 0u;
    while ((qh >> 32) != 0 || qh * v2 > ((rh << 32) | x2)) {
      qh--; rh += v1;
      if (rh >> 32) break;
    }
    uint64_t carry = 0;
    uint32_t borrow = 0;
    int i0 = 0;
    for (; i0 + PD_CH <= nm; i0 += PD_CH) {
      uint32_t X[PD_CH], V[PD_CH];
#pragma unroll
      for (int k = 0; k < PD_CH; k++) { X[k] = x[(j + i0 + k) * S]; V[k] = mn[(i0 + k) * S]; }
#pragma unroll
      for (int k = 0; k < PD_CH; k++) {
        const uint64_t p = qh * V[k] + carry;
        carry = p >> 32;
        const uint64_t t = (uint64_t)X[k] - (uint32_t)p - borrow;
        X[k] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
      }
#pragma unroll
      for (int k = 0; k < PD_CH; k++) x[(j + i0 + k) * S] = X[k];
    }
    for (int i = i0; i < nm; i++) {                                 // (a divisor whose length is no multiple of the chunk)
      const uint64_t p = qh * mn[i * S] + carry;
      carry = p >> 32;
      const uint64_t t = (uint64_t)x[(j + i) * S] - (uint32_t)p - borrow;
      x[(j + i) * S] = (uint32_t)t;
      borrow = (uint32_t)(t >> 63);
    }
    const uint64_t t = (uint64_t)x[(j + nm) * S] - carry - borrow;
    x[(j + nm) * S] = (uint32_t)t;
    if (t >> 63) {                                                 // the estimate was one too large: add the divisor back
      uint32_t c = 0;
      for (int i = 0; i < nm; i++) {
        const uint64_t u = (uint64_t)x[(j + i) * S] + mn[i * S] + c;
        x[(j + i) * S] = (uint32_t)u;
        c = (uint32_t)(u >> 32);
      }
      x[(j + nm) * S] += c;
    }
  }
  for (int w = 0; w < nm; w++) {
    const uint32_t lo = x[w * S], hi = w + 1 < nm ? x[(w + 1) * S] : 0u;
    x[w * S] = s ? (lo >> s) | (hi << (32 - s)) : lo;
  }
  for (int w = nm; w <= nx; w++) x[w * S] = 0u;
}

// q[0 .. nq) = x / d for an odd d of nd words (any memory, stride ds), x: nx words of LDS, nx >= nq + nd, consumed.  True iff d divides x
// and the quotient is below 2^(32 nq).
__device__ __forceinline__ bool pd_divexact(uint32_t* x, int nx, const uint32_t* d, int ds, int nd, uint32_t* q, int nq, int S) {
  const uint32_t dinv = pd_inv32(d[0]);
  for (int i = 0; i < nq; i++) {
    const uint32_t qi = x[i * S] * dinv;
    q[i * S] = qi;
    uint64_t carry = 0;
    uint32_t borrow = 0;
    int k0 = 0;
    for (; k0 + PD_CH <= nd; k0 += PD_CH) {                        // (i + nd < nx)
      uint32_t X[PD_CH], D[PD_CH];
#pragma unroll
      for (int k = 0; k < PD_CH; k++) { X[k] = x[(i + k0 + k) * S]; D[k] = d[(k0 + k) * ds]; }
#pragma unroll
      for (int k = 0; k < PD_CH; k++) {
        const uint64_t p = (uint64_t)qi * D[k] + carry;
        carry = p >> 32;
        const uint64_t t = (uint64_t)X[k] - (uint32_t)p - borrow;
        X[k] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
      }
#pragma unroll
      for (int k = 0; k < PD_CH; k++) x[(i + k0 + k) * S] = X[k];
    }
    for (int k = k0; k < nd; k++) {
      const uint64_t p = (uint64_t)qi * d[k * ds] + carry;
      carry = p >> 32;
      const uint64_t t = (uint64_t)x[(i + k) * S] - (uint32_t)p - borrow;
      x[(i + k) * S] = (uint32_t)t;
      borrow = (uint32_t)(t >> 63);
    }
    for (int w = i + nd; w < nx && (carry | borrow) != 0; w++) {
      const uint64_t t = (uint64_t)x[w * S] - carry - borrow;
      x[w * S] = (uint32_t)t;
      borrow = (uint32_t)(t >> 63);
      carry = 0;
    }
  }
  bool zero = true;
  for (int w = 0; w < nx; w++) zero = zero && x[w * S] == 0u;
  return zero;
}

__device__ __forceinline__ bool pd_odd_ge3(const uint32_t* v, int n) {
  bool big = v[0] >= 3u;
  for (int w = 1; w < n; w++) big = big || v[w] != 0u;
  return (v[0] & 1u) && big;
}

// ---- what the split and finish kernels of the calls that hold p and q share (kernels_ck_prove.hpp, kernels_ck_inter.hpp)
// The ladder's row of an item under a bad key: base and exponent zero under the modulus 3 (the ladder refuses a modulus below 2 bits or an
// even one for the whole call).  m, b: rw words, e: hw words.
__device__ __forceinline__ void pd_row_null(uint32_t* m, uint32_t* b, uint32_t* e, int rw, int hw) {
  for (int w = 0; w < rw; w++) { m[w] = w == 0 ? 3u : 0u; b[w] = 0u; }
  for (int w = 0; w < hw; w++) e[w] = 0u;
}
// m <- the factor F, b <- the reduced base x (LDS): nf words each, zero-padded to the row width rw
__device__ __forceinline__ void pd_row_put(uint32_t* m, uint32_t* b, int rw, const uint32_t* F, int nf, const uint32_t* x, int S) {
  for (int w = 0; w < rw; w++) { m[w] = w < nf ? F[w] : 0u; b[w] = w < nf ? x[w * S] : 0u; }
}
__device__ __forceinline__ void pd_exp_put(uint32_t* e, const uint32_t* src, int hw) {
  for (int w = 0; w < hw; w++) e[w] = src[w];
}
// vp, vq <- the first hw words of the p-side row at `rows` and of the q-side row behind it
__device__ __forceinline__ void pd_load_pair(uint32_t* vp, uint32_t* vq, const uint32_t* rows, int rw, int hw, int S) {
  for (int w = 0; w < hw; w++) vp[w * S] = rows[w];
  for (int w = 0; w < hw; w++) vq[w * S] = rows[rw + w];
}

// The recombination's LDS of one lane, thread-interleaved: x (2 hw + 1 words), then mn, d, vp, vq (hw words each).
struct PdCrtLds {
  uint32_t* x; uint32_t* mn; uint32_t* d; uint32_t* vp; uint32_t* vq;
  __device__ __forceinline__ PdCrtLds(uint32_t* lds, int hw, int S)
      : x(lds + threadIdx.x), mn(x + (size_t)(2 * hw + 1) * S), d(mn + (size_t)hw * S), vp(d + (size_t)hw * S), vq(vp + (size_t)hw * S) {}
};
constexpr size_t pd_crt_lds_words_per_lane(int hw) { return 6 * (size_t)hw + 1; }

// out[0 .. 2 hw) = vp + P ((vq - vp) pinv mod Q), or zeros.  l.vp < P and l.vq < Q are kept.
__device__ __forceinline__ void pd_crt(uint32_t* out, bool ok, const PdCrtLds& l, const uint32_t* P, const uint32_t* Q, const uint32_t* pinv, int hw, int S) {
  uint32_t* const x = l.x; uint32_t* const mn = l.mn; uint32_t* const d = l.d;
  const uint32_t* const vp = l.vp; const uint32_t* const vq = l.vq;
  for (int w = 0; w < hw; w++) x[w * S] = vp[w * S];
  pd_mod(x, hw, Q, 1, hw, mn, S);                              // vp mod q   (p > q: vp may exceed q)
  uint32_t borrow = 0;
  for (int w = 0; w < hw; w++) {
    const uint64_t t = (uint64_t)vq[w * S] - x[w * S] - borrow;
    d[w * S] = (uint32_t)t;
    borrow = (uint32_t)(t >> 63);
  }
  if (borrow) {                                                // negative: + q
    uint32_t c = 0;
    for (int w = 0; w < hw; w++) {
      const uint64_t t = (uint64_t)d[w * S] + Q[w] + c;
      d[w * S] = (uint32_t)t;
      c = (uint32_t)(t >> 32);
    }
  }
  pd_mul(x, d, hw, pinv, 1, hw, S);
  pd_mod(x, 2 * hw, Q, 1, hw, mn, S);
  for (int w = 0; w < hw; w++) d[w * S] = x[w * S];
  pd_mul(x, d, hw, P, 1, hw, S);                               // p u <= p (q - 1), + vp < n: no carry out of 2 hw words
  uint32_t c = 0;
  for (int w = 0; w < 2 * hw; w++) {
    const uint64_t t = (uint64_t)x[w * S] + (w < hw ? vp[w * S] : 0u) + c;
    out[w] = ok ? (uint32_t)t : 0u;
    c = (uint32_t)(t >> 32);
  }
}

// ---- key preparation, one key per lane.  Part a writes the four rows of the inverse kernel:
//   0: (q mod p)^-1 mod p = -h_p      1: (p mod q)^-1 mod q = pinv = -h_q      2: ((p - 1) mod q)^-1 mod q      3: ((q - 1) mod p)^-1 mod p
// A key with an even p or q, or one below 3, gets zero rows (outside k_modinv's domain: status, no work) and key status 2.
struct PdecKeyArgs {
  const uint32_t* p; const uint32_t* q; uint64_t key_stride;   // [nkeys][hw]
  uint32_t* inv_a; uint32_t* inv_m;                            // [4 nkeys][hw]   operands and moduli of the inverse kernel
  const uint32_t* inv; const uint8_t* inv_status;              // [4 nkeys][hw], [4 nkeys]   its results (part b)
  uint32_t* hp; uint32_t* hq; uint32_t* dp; uint32_t* dq;      // [nkeys][hw]   (pinv is row 1 of inv); hp, hq nullable
  uint8_t* kst;                                                // [nkeys] 0 | 2
  uint64_t nkeys; int hw;
};
constexpr size_t pdec_key_lds_words_per_lane(int hw) { return 4 * (size_t)hw + 1; }

__global__ void __launch_bounds__(64) k_pdec_key_a(PdecKeyArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw;
  const uint64_t key = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (key >= a.nkeys) return;
  const uint32_t* P = a.p + key * a.key_stride;
  const uint32_t* Q = a.q + key * a.key_stride;
  uint32_t* x = pd_lds + threadIdx.x;                          // hw + 1 words
  uint32_t* mn = x + (size_t)(hw + 1) * S;                     // hw words
  const bool ok = pd_odd_ge3(P, hw) && pd_odd_ge3(Q, hw);
  a.kst[key] = ok ? 0 : 2;
  for (int row = 0; row < 4; row++) {
    const uint32_t* src = (row == 0 || row == 3) ? Q : P;      // rows 0 and 3 reduce q (- 1) modulo p; rows 1 and 2, p (- 1) modulo q
    const uint32_t* mod = (row == 0 || row == 3) ? P : Q;
    uint32_t* oa = a.inv_a + (key * 4 + row) * (uint64_t)hw;
    uint32_t* om = a.inv_m + (key * 4 + row) * (uint64_t)hw;
    if (!ok) {
      for (int w = 0; w < hw; w++) { oa[w] = 0u; om[w] = 0u; }
      continue;
    }
    for (int w = 0; w < hw; w++) x[w * S] = src[w];
    if (row >= 2) x[0] -= 1u;                                  // (odd: no borrow)
    pd_mod(x, hw, mod, 1, hw, mn, S);
    for (int w = 0; w < hw; w++) { oa[w] = x[w * S]; om[w] = mod[w]; }
  }
}

// Part b: the constants from the four inverses; a key one of whose inverses does not exist (gcd(n, phi(n)) != 1) is status 2, constants zero.
__global__ void __launch_bounds__(64) k_pdec_key_b(PdecKeyArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw;
  const uint64_t key = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (key >= a.nkeys) return;
  const uint32_t* P = a.p + key * a.key_stride;
  const uint32_t* Q = a.q + key * a.key_stride;
  bool ok = a.kst[key] == 0;
  for (int row = 0; row < 4; row++) ok = ok && a.inv_status[key * 4 + row] == ZKP_INV_OK;
  uint32_t* hp = a.hp ? a.hp + key * (uint64_t)hw : nullptr;  // (hp, hq null: a caller that takes roots only, kernels_ck_prove.hpp)
  uint32_t* hq = a.hq ? a.hq + key * (uint64_t)hw : nullptr;
  uint32_t* dp = a.dp + key * (uint64_t)hw;
  uint32_t* dq = a.dq + key * (uint64_t)hw;
  a.kst[key] = ok ? 0 : 2;
  if (!ok) {
    for (int w = 0; w < hw; w++) { if (hp) hp[w] = 0u; if (hq) hq[w] = 0u; dp[w] = 0u; dq[w] = 0u; }
    return;
  }
  uint32_t* x = pd_lds + threadIdx.x;                          // 2 hw words: M y, then the exact division's running value
  uint32_t* mm = x + (size_t)(2 * hw) * S;                     // hw words: M = p - 1 | q - 1
  uint32_t* t = mm + (size_t)hw * S;                           // hw words: the quotient
  for (int side = 0; side < 2; side++) {
    const uint32_t* F = side ? Q : P;                          // this side's factor, and the other one
    const uint32_t* O = side ? P : Q;
    const uint32_t* u = a.inv + (key * 4 + side) * (uint64_t)hw;          // (O mod F)^-1 mod F
    const uint32_t* y = a.inv + (key * 4 + 2 + side) * (uint64_t)hw;      // (F - 1)^-1 mod O
    uint32_t* h = side ? hq : hp;
    uint32_t* d = side ? dq : dp;
    uint32_t borrow = 0;
    for (int w = 0; h && w < hw; w++) {                        // h = F - u   (0 < u < F)
      const uint64_t v = (uint64_t)F[w] - u[w] - borrow;
      h[w] = (uint32_t)v;
      borrow = (uint32_t)(v >> 63);
    }
    for (int w = 0; w < hw; w++) mm[w * S] = w == 0 ? F[0] - 1u : F[w];
    pd_mul(x, mm, hw, y, 1, hw, S);
    for (int w = 0; w < 2 * hw; w++) { if (x[w * S]-- != 0u) break; }     // M y - 1   (M y >= 2)
    (void)pd_divexact(x, 2 * hw, O, 1, hw, t, hw, S);
    borrow = 0;
    for (int w = 0; w < hw; w++) {                             // d = M - t   (0 < t < M)
      const uint64_t v = (uint64_t)mm[w * S] - t[w * S] - borrow;
      d[w] = (uint32_t)v;
      borrow = (uint32_t)(v >> 63);
    }
  }
}

// ---- split, one ciphertext per pair of lanes (one lane per factor): the ladder's rows.  Rows 2 i and 2 i + 1 are item i under p^2 and q^2; with roots, rows
// 2 count + 2 i and 2 count + 2 i + 1 are item i under p and q, zero-padded to the same row width.  An item under a bad key gets base and
// exponent zero under the modulus 3 (the ladder refuses a modulus below 2 bits or an even one for the whole call).
struct PdecSplitArgs {
  const uint32_t* c;                                           // [count][2 kw]
  const uint32_t* p; const uint32_t* q; uint64_t key_stride;
  const uint32_t* p2; const uint32_t* q2;                      // [nkeys][kw]
  const uint32_t* dp; const uint32_t* dq;                      // [nkeys][hw]
  const uint8_t* kst;
  uint32_t* mods; uint32_t* base;                              // [rows][rw]
  uint32_t* exp;                                               // [rows][hw]
  uint64_t count; int hw, rw, roots;
};
constexpr size_t pdec_split_lds_words_per_lane(int hw) { return 6 * (size_t)hw + 1; }

__global__ void __launch_bounds__(64) k_pdec_split(PdecSplitArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw, kw = 2 * a.hw, rw = a.rw;
  const uint64_t gid = (uint64_t)blockIdx.x * S + threadIdx.x, item = gid >> 1;
  if (item >= a.count) return;
  const uint64_t key = a.key_stride ? item : 0;
  const bool bad = a.kst[key] != 0;
  uint32_t* x = pd_lds + threadIdx.x;                          // 2 kw + 1 words
  uint32_t* mn = x + (size_t)(2 * kw + 1) * S;                 // kw words
  const uint32_t* C = a.c + item * 2 * (uint64_t)kw;
  const int side = (int)(gid & 1);                             // two lanes per item: the reductions under p^2 and q^2 share nothing
  const uint32_t* F = (side ? a.q : a.p) + key * a.key_stride;
  const uint32_t* F2 = (side ? a.q2 : a.p2) + key * (uint64_t)kw;
  const uint32_t* D = (side ? a.dq : a.dp) + key * (uint64_t)hw;
  const uint64_t r0 = 2 * item + side, r1 = 2 * a.count + 2 * item + side;
  uint32_t* m0 = a.mods + r0 * rw; uint32_t* b0 = a.base + r0 * rw; uint32_t* e0 = a.exp + r0 * hw;
  if (bad) pd_row_null(m0, b0, e0, rw, hw);
  else {
    for (int w = 0; w < 2 * kw; w++) x[w * S] = C[w];
    pd_mod(x, 2 * kw, F2, 1, kw, mn, S);
    pd_row_put(m0, b0, rw, F2, kw, x, S);
    for (int w = 0; w < hw; w++) e0[w] = w == 0 ? F[0] - 1u : F[w];
  }
  if (!a.roots) return;
  uint32_t* m1 = a.mods + r1 * rw; uint32_t* b1 = a.base + r1 * rw; uint32_t* e1 = a.exp + r1 * hw;
  if (bad) pd_row_null(m1, b1, e1, rw, hw);
  else {
    pd_mod(x, kw, F, 1, hw, mn, S);                            // (c mod p^2) mod p
    pd_row_put(m1, b1, rw, F, hw, x, S);
    pd_exp_put(e1, D, hw);
  }
}

// ---- finish, one item per lane: L and its domain test, the products by h_p and h_q, both recombinations, the status.
struct PdecFinishArgs {
  const uint32_t* rows;                                        // [rows][rw]   what the ladder returned
  const uint32_t* p; const uint32_t* q; uint64_t key_stride;
  const uint32_t* hp; const uint32_t* hq; const uint32_t* pinv; uint64_t pinv_stride;
  const uint8_t* kst;
  uint32_t* out_m; uint32_t* out_r;                            // [count][kw]; out_r nullable
  uint8_t* status;                                             // [count]
  uint64_t count; int hw, rw;
};

__global__ void __launch_bounds__(64) k_pdec_finish(PdecFinishArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw, kw = 2 * a.hw, rw = a.rw;
  const uint64_t item = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (item >= a.count) return;
  const uint64_t key = a.key_stride ? item : 0;
  uint32_t* om = a.out_m + item * (uint64_t)kw;
  uint32_t* orr = a.out_r ? a.out_r + item * (uint64_t)kw : nullptr;
  if (a.kst[key] != 0) {
    for (int w = 0; w < kw; w++) { om[w] = 0u; if (orr) orr[w] = 0u; }
    a.status[item] = 2;
    return;
  }
  const uint32_t* P = a.p + key * a.key_stride;
  const uint32_t* Q = a.q + key * a.key_stride;
  const uint32_t* pinv = a.pinv + key * a.pinv_stride;
  const PdCrtLds l(pd_lds, hw, S);                             // d: L, then the recombination's difference; vp, vq: m_p | r_p, m_q | r_q
  uint32_t* const x = l.x; uint32_t* const d = l.d;
  bool ok = true;
  for (int side = 0; side < 2; side++) {
    const uint32_t* F = side ? Q : P;
    const uint32_t* h = (side ? a.hq : a.hp) + key * (uint64_t)hw;
    const uint32_t* X = a.rows + (2 * item + side) * (uint64_t)rw;
    bool zero = true;
    for (int w = 0; w < kw; w++) { const uint32_t v = X[w]; x[w * S] = v; zero = zero && v == 0u; }
    for (int w = 0; w < kw; w++) { if (x[w * S]-- != 0u) break; }                   // x_p - 1 (x_p == 0: the test below fails it)
    const bool exact = pd_divexact(x, kw, F, 1, hw, d, hw, S);
    ok = ok && exact && !zero;
    pd_mul(x, d, hw, h, 1, hw, S);
    pd_mod(x, kw, F, 1, hw, l.mn, S);
    uint32_t* v = side ? l.vq : l.vp;
    for (int w = 0; w < hw; w++) v[w * S] = x[w * S];
  }
  pd_crt(om, ok, l, P, Q, pinv, hw, S);
  if (orr) {
    pd_load_pair(l.vp, l.vq, a.rows + (2 * a.count + 2 * item) * (uint64_t)rw, rw, hw, S);
    pd_crt(orr, ok, l, P, Q, pinv, hw, S);
  }
  a.status[item] = ok ? 0 : 2;
}

}  // namespace zkp
