// kernels_ck_prove.hpp — the arithmetic around the ladder in NiCorrectKeyProof::proof for whole batches of keys (zkp_correct_key_ni_prove_batch;
// correct_key_ni.rs:42-71 with upstream's extract_nroot): for key b = (p, q) and root i < 11, item j = 11 b + i,
//   n = p q      rho_i = mask_generation(bit_length(n), H(n, H(salt), i))      (k_ck_hash / k_ck_hash_wave, kernels_proofs.hpp)
//   s_p = (rho_i mod p)^(d_p) mod p,  s_q alike      sigma_i = s_p + p ((s_q - s_p) pinv mod q)
// with d_p = q^-1 mod (p - 1), pinv = p^-1 mod q from the key kernels of kernels_paillier_dec.hpp (k_pdec_key_a, k_modinv, k_pdec_key_b).
// The hash kernels leave the mask unreduced (kw + 8 words); p and q divide n, so reducing the mask modulo p and q is reducing rho mod n.
// The kernels here: the product (k_ck_prove_n), the ladder's 22 rows per key (k_ck_prove_split) and the recombination (k_ck_prove_finish).
// tests/ck_prove_model.py states the values.
//
// Data layout: as kernels_paillier_dec.hpp — one value per lane, operands in thread-interleaved LDS.  Items are consecutive lanes and a key
// owns 11 of them, so a block of 16 lanes spans two keys (or three): every pointer that depends on the key is taken per lane from item / 11.
#pragma once
#include "kernels_paillier_dec.hpp"

namespace zkp {

// n = p q as kw = 2 hw words (one thread per key; schoolbook, as k_square_words)
__global__ void __launch_bounds__(64) k_ck_prove_n(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q, int hw, uint64_t nkeys, uint32_t* __restrict__ out) {
  const uint64_t key = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= nkeys) return;
  const uint32_t* P = p + key * (uint64_t)hw;
  const uint32_t* Q = q + key * (uint64_t)hw;
  uint32_t* o = out + key * 2 * (uint64_t)hw;
  for (int w = 0; w < 2 * hw; w++) o[w] = 0;
  for (int i = 0; i < hw; i++) {
    uint64_t carry = 0;
    const uint64_t pi = P[i];
    for (int j = 0; j < hw; j++) {
      const uint64_t t = pi * Q[j] + o[i + j] + carry;
      o[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    o[i + hw] = (uint32_t)carry;
  }
}

// ---- split, one root per pair of lanes (one lane per factor): rows 2 j and 2 j + 1 of the ladder are item j under p and q, zero-padded to
// the row width.  A root of a bad key gets the null row (pd_row_null).
struct CkProveSplitArgs {
  const uint32_t* mgf;                                         // [items][kw + 8]   what the hash kernels wrote
  const uint32_t* p; const uint32_t* q;                        // [nkeys][hw]
  const uint32_t* dp; const uint32_t* dq;                      // [nkeys][hw]
  const uint8_t* kst;                                          // [nkeys]
  uint32_t* mods; uint32_t* base;                              // [2 items][rw]
  uint32_t* exp;                                               // [2 items][hw]
  uint64_t items; int hw, rw;
};
constexpr size_t ck_prove_split_lds_words_per_lane(int hw) { return 3 * (size_t)hw + 9; }

__global__ void __launch_bounds__(64) k_ck_prove_split(CkProveSplitArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw, mw = 2 * a.hw + 8, rw = a.rw;
  const uint64_t gid = (uint64_t)blockIdx.x * S + threadIdx.x, item = gid >> 1;
  if (item >= a.items) return;
  const uint64_t key = item / ZKP_CORRECT_KEY_M2;
  const int side = (int)(gid & 1);
  uint32_t* x = pd_lds + threadIdx.x;                          // kw + 8 + 1 words
  uint32_t* mn = x + (size_t)(mw + 1) * S;                     // hw words
  const uint32_t* F = (side ? a.q : a.p) + key * (uint64_t)hw;
  const uint32_t* D = (side ? a.dq : a.dp) + key * (uint64_t)hw;
  uint32_t* m = a.mods + gid * (uint64_t)rw; uint32_t* b = a.base + gid * (uint64_t)rw; uint32_t* e = a.exp + gid * (uint64_t)hw;
  if (a.kst[key] != 0) { pd_row_null(m, b, e, rw, hw); return; }
  const uint32_t* R = a.mgf + item * (uint64_t)mw;
  for (int w = 0; w < mw; w++) x[w * S] = R[w];
  pd_mod(x, mw, F, 1, hw, mn, S);
  pd_row_put(m, b, rw, F, hw, x, S);
  pd_exp_put(e, D, hw);
}

// ---- finish, one root per lane: the recombination (pd_crt); the lane of a key's root 0 writes the key's status and zeroes the n of a bad key.
struct CkProveFinishArgs {
  const uint32_t* rows;                                        // [2 items][rw]   what the ladder returned
  const uint32_t* p; const uint32_t* q;                        // [nkeys][hw]
  const uint32_t* pinv; uint64_t pinv_stride;
  const uint8_t* kst;
  uint32_t* out_n;                                             // [nkeys][kw]   (holds p q on entry)
  uint32_t* out_sigma;                                         // [items][kw]
  uint8_t* status;                                             // [nkeys]
  uint64_t items; int hw, rw;
};

__global__ void __launch_bounds__(64) k_ck_prove_finish(CkProveFinishArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw, kw = 2 * a.hw, rw = a.rw;
  const uint64_t item = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (item >= a.items) return;
  const uint64_t key = item / ZKP_CORRECT_KEY_M2;
  const bool first = item % ZKP_CORRECT_KEY_M2 == 0;
  uint32_t* os = a.out_sigma + item * (uint64_t)kw;
  if (a.kst[key] != 0) {
    for (int w = 0; w < kw; w++) os[w] = 0u;
    if (first) {
      uint32_t* on = a.out_n + key * (uint64_t)kw;
      for (int w = 0; w < kw; w++) on[w] = 0u;
      a.status[key] = 2;
    }
    return;
  }
  if (first) a.status[key] = 0;
  const uint32_t* P = a.p + key * (uint64_t)hw;
  const uint32_t* Q = a.q + key * (uint64_t)hw;
  const uint32_t* pinv = a.pinv + key * a.pinv_stride;
  const PdCrtLds l(pd_lds, hw, S);                             // vp, vq: s_p, s_q
  pd_load_pair(l.vp, l.vq, a.rows + 2 * item * (uint64_t)rw, rw, hw, S);
  pd_crt(os, true, l, P, Q, pinv, hw, S);
}

}  // namespace zkp
