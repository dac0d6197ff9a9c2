// kernels_ck_inter.hpp — the arithmetic around the ladder in the interactive CorrectKey for whole batches of sessions (correct_key.rs:64-171;
// zkp_correct_key_challenge_batch, its seeded form, zkp_correct_key_prove_batch, zkp_correct_key_verify_seeded_batch).  A session b has K
// rounds; item j = K b + i is round i of session b.
//   challenge: sn_i = s_i^n mod n, rn_i = r_i^n mod n, e = H(n, sn.., rn..), z_i = r_i s_i^e mod n, s_digest = H(s..).  The kernels here
//     reduce s and r under n (k_cki_chal_reduce), lay out the ladder's per-row moduli (k_cki_chal_rows) and settle status and outputs
//     (k_cki_chal_status, k_cki_chal_finish); the ladder, the product and the hashes are the existing launches.
//   prove, for key b = (p, q), n = p q, without phi, phi - e mod phi or n^-1 mod phi:
//     rn_i mod p = (z_i mod p)^(n mod (p-1)) (sn_i mod p)^((p-1) - e mod (p-1)) mod p      (q alike)      rn_i = CRT(rn_p, rn_q)
//     root_i     = CRT((sn_i mod p)^(d_p) mod p, (sn_i mod q)^(d_q) mod q)                 d_p = q^-1 mod (p-1)   (upstream's extract_nroot)
//     six half-width rows per round (k_cki_prove_split), the recombinations (k_cki_prove_finish), gcd(n, .) over sn, z and rn
//     (k_cki_prove_gcd) and the reference's checks in its order, one lane per session (k_cki_prove_merge).
//   verify from the seed: the verdict from the regenerated digest (k_cki_verdict).
// tests/ck_inter_model.py states the values.
//
// Data layout: as kernels_ck_prove.hpp — one value per lane, 16-lane blocks, operands in thread-interleaved LDS.  Items are consecutive lanes
// and a session owns K of them, so a block spans sessions whenever K is no multiple of 16: every pointer that depends on the key is taken
// per lane from item / K.
#pragma once
#include "kernels_ck_prove.hpp"

namespace zkp {

// an n the challenge accepts: odd and at least 3 (the ladder's domain)
__device__ __forceinline__ bool cki_n_ok(const uint32_t* n, int kw) { return pd_odd_ge3(n, kw); }

// ---- challenge.  status[b] = (the sampler's status of a seeded call) | MALFORMED for an n outside the domain; one thread per session
__global__ void __launch_bounds__(256) k_cki_chal_status(const uint32_t* __restrict__ n, uint64_t n_stride, int kw, uint64_t batch, int seeded,
                                                         uint8_t* __restrict__ status) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const uint8_t pre = seeded ? status[b] : (uint8_t)0;
  status[b] = (pre || !cki_n_ok(n + b * n_stride, kw)) ? (uint8_t)ZKP_VERDICT_MALFORMED : (uint8_t)0;
}

// The ladder's moduli, which are its n_bits-bit exponents too: one row for a shared n, else row r of 2 K B is the n of session (r mod K B) / K.
// An n outside the domain travels as 3 (the ladder refuses an even modulus for the whole call); its sessions' bases are zero.
__global__ void __launch_bounds__(256) k_cki_chal_rows(const uint32_t* __restrict__ n, uint64_t n_stride, int kw, uint64_t items, uint32_t K,
                                                       uint64_t nrows, uint32_t* __restrict__ out) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= nrows * (uint64_t)kw) return;
  const uint64_t row = gid / (uint64_t)kw;
  const int w = (int)(gid % (uint64_t)kw);
  const uint32_t* N = n + ((row % items) / K) * n_stride;
  out[gid] = cki_n_ok(N, kw) ? N[w] : (w == 0 ? 3u : 0u);
}

// base[v] = value v mod n for the 2 K B values s (v < K B) and r, one per lane; zero in a MALFORMED session.  mod_pow reduces its base.
struct CkiChalReduceArgs {
  const uint32_t* s; const uint32_t* r;                        // [items][kw], any values
  const uint32_t* n; uint64_t n_stride;
  const uint8_t* status;                                       // [batch]
  uint32_t* base;                                              // [2 items][kw]
  uint64_t items; uint32_t K; int kw;
};
constexpr size_t cki_chal_reduce_lds_words_per_lane(int kw) { return 2 * (size_t)kw + 1; }

__global__ void __launch_bounds__(64) k_cki_chal_reduce(CkiChalReduceArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, kw = a.kw;
  const uint64_t v = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (v >= 2 * a.items) return;
  const uint64_t item = v < a.items ? v : v - a.items, key = item / a.K;
  const uint32_t* X = (v < a.items ? a.s : a.r) + item * (uint64_t)kw;
  uint32_t* o = a.base + v * (uint64_t)kw;
  if (a.status[key] != 0) {
    for (int w = 0; w < kw; w++) o[w] = 0u;
    return;
  }
  uint32_t* x = pd_lds + threadIdx.x;                          // kw + 1 words
  uint32_t* mn = x + (size_t)(kw + 1) * S;                     // kw words
  for (int w = 0; w < kw; w++) x[w * S] = X[w];
  pd_mod(x, kw, a.n + key * a.n_stride, 1, kw, mn, S);
  for (int w = 0; w < kw; w++) o[w] = x[w * S];
}

// out_sn <- the ladder's sn; a MALFORMED session's sn, z, e and s_digest become zero.  One thread per word of an item; the threads of a
// session's item 0 take its e and s_digest.
struct CkiChalFinishArgs {
  const uint32_t* sn; const uint8_t* status;
  uint32_t* out_sn; uint32_t* out_z;                           // [items][kw]
  uint32_t* out_e; uint32_t* out_s_digest;                     // [batch][8]; out_s_digest nullable
  uint64_t items; uint32_t K; int kw;
};
__global__ void __launch_bounds__(256) k_cki_chal_finish(CkiChalFinishArgs a) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= a.items * (uint64_t)a.kw) return;
  const uint64_t item = gid / (uint64_t)a.kw, key = item / a.K;
  const int w = (int)(gid % (uint64_t)a.kw);
  const bool bad = a.status[key] != 0;
  a.out_sn[gid] = bad ? 0u : a.sn[gid];
  if (!bad) return;
  a.out_z[gid] = 0u;
  if (item % a.K == 0 && w < 8) {
    a.out_e[key * 8 + w] = 0u;
    if (a.out_s_digest) a.out_s_digest[key * 8 + w] = 0u;
  }
}

// ---- verify from the seed: ACCEPT iff the regenerated digest equals the proof's; MALFORMED where the seeded challenge is
__global__ void __launch_bounds__(256) k_cki_verdict(const uint32_t* __restrict__ digest, const uint32_t* __restrict__ proof, const uint8_t* __restrict__ status,
                                                     uint64_t batch, uint8_t* __restrict__ verdict) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  bool same = true;
  for (int w = 0; w < 8; w++) same = same && digest[b * 8 + w] == proof[b * 8 + w];
  verdict[b] = status[b] != 0 ? ZKP_VERDICT_MALFORMED : same ? ZKP_VERDICT_ACCEPT : ZKP_VERDICT_REJECT;
}

// ---- prove: split, one round per pair of lanes (one lane per factor F).  Rows 6 j + 2 t + side of the ladder, zero-padded to the row width:
//   t = 0: (z mod F)^(n mod (F-1))      t = 1: (sn mod F)^((F-1) - e mod (F-1))      t = 2: (sn mod F)^(d_F)
// n mod (F-1) and e mod (F-1) are real reductions: no primality or size test is made on F.  A round of a bad key gets three null rows
// (pd_row_null).
constexpr int CKI_ROWS = 6;                                    // half-width rows per round
struct CkiProveSplitArgs {
  const uint32_t* sn; const uint32_t* z;                       // [items][kw], any values
  const uint32_t* e;                                           // [nkeys][8]
  const uint32_t* n;                                           // [nkeys][kw]   p q
  const uint32_t* p; const uint32_t* q;                        // [nkeys][hw]
  const uint32_t* dp; const uint32_t* dq;                      // [nkeys][hw]
  const uint8_t* kst;                                          // [nkeys]
  uint32_t* mods; uint32_t* base;                              // [6 items][rw]
  uint32_t* exp;                                               // [6 items][hw]
  uint64_t items; uint32_t K; int hw, rw;
};
constexpr size_t cki_prove_split_lds_words_per_lane(int hw) { return 4 * (size_t)hw + 1; }

__global__ void __launch_bounds__(64) k_cki_prove_split(CkiProveSplitArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw, kw = 2 * a.hw, rw = a.rw;
  const uint64_t gid = (uint64_t)blockIdx.x * S + threadIdx.x, item = gid >> 1;
  if (item >= a.items) return;
  const uint64_t key = item / a.K;
  const int side = (int)(gid & 1);
  const uint64_t r0 = CKI_ROWS * item + side;
  if (a.kst[key] != 0) {
    for (int t = 0; t < 3; t++) pd_row_null(a.mods + (r0 + 2 * t) * (uint64_t)rw, a.base + (r0 + 2 * t) * (uint64_t)rw, a.exp + (r0 + 2 * t) * (uint64_t)hw, rw, hw);
    return;
  }
  uint32_t* x = pd_lds + threadIdx.x;                          // kw + 1 words
  uint32_t* mn = x + (size_t)(kw + 1) * S;                     // hw words
  uint32_t* f1 = mn + (size_t)hw * S;                          // hw words: F - 1
  const uint32_t* F = (side ? a.q : a.p) + key * (uint64_t)hw;
  const uint32_t* D = (side ? a.dq : a.dp) + key * (uint64_t)hw;
  for (int w = 0; w < hw; w++) f1[w * S] = w == 0 ? F[0] - 1u : F[w];     // (odd: no borrow)
  for (int t = 0; t < 3; t++) {
    const uint64_t row = r0 + 2 * t;
    uint32_t* m = a.mods + row * (uint64_t)rw; uint32_t* b = a.base + row * (uint64_t)rw; uint32_t* e = a.exp + row * (uint64_t)hw;
    // the base: z or sn under F
    const uint32_t* V = (t == 0 ? a.z : a.sn) + item * (uint64_t)kw;
    for (int w = 0; w < kw; w++) x[w * S] = V[w];
    pd_mod(x, kw, F, 1, hw, mn, S);
    pd_row_put(m, b, rw, F, hw, x, S);
    // the exponent
    if (t == 0) {
      const uint32_t* N = a.n + key * (uint64_t)kw;
      for (int w = 0; w < kw; w++) x[w * S] = N[w];
      pd_mod(x, kw, f1, S, hw, mn, S);
      for (int w = 0; w < hw; w++) e[w] = x[w * S];
    } else if (t == 1) {
      const uint32_t* E = a.e + key * 8;
      for (int w = 0; w < hw; w++) x[w * S] = w < 8 ? E[w] : 0u;
      pd_mod(x, hw, f1, S, hw, mn, S);
      uint32_t borrow = 0;
      for (int w = 0; w < hw; w++) {                           // (F - 1) - (e mod (F - 1)), in (0, F - 1]
        const uint64_t d = (uint64_t)f1[w * S] - x[w * S] - borrow;
        e[w] = (uint32_t)d;
        borrow = (uint32_t)(d >> 63);
      }
    } else pd_exp_put(e, D, hw);
  }
}

// ---- finish, one round per lane: rn = CRT of the two products, root = CRT of the two root rows.  A round of a bad key gets zeros.
struct CkiProveFinishArgs {
  const uint32_t* rows;                                        // [6 items][rw]   what the ladder returned
  const uint32_t* p; const uint32_t* q;                        // [nkeys][hw]
  const uint32_t* pinv; uint64_t pinv_stride;
  const uint8_t* kst;
  uint32_t* rn; uint32_t* root;                                // [items][kw]
  uint64_t items; uint32_t K; int hw, rw;
};

__global__ void __launch_bounds__(64) k_cki_prove_finish(CkiProveFinishArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, hw = a.hw, kw = 2 * a.hw, rw = a.rw;
  const uint64_t item = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (item >= a.items) return;
  const uint64_t key = item / a.K;
  uint32_t* orn = a.rn + item * (uint64_t)kw;
  uint32_t* ort = a.root + item * (uint64_t)kw;
  if (a.kst[key] != 0) {
    for (int w = 0; w < kw; w++) { orn[w] = 0u; ort[w] = 0u; }
    return;
  }
  const uint32_t* P = a.p + key * (uint64_t)hw;
  const uint32_t* Q = a.q + key * (uint64_t)hw;
  const uint32_t* pinv = a.pinv + key * a.pinv_stride;
  const uint32_t* R = a.rows + CKI_ROWS * item * (uint64_t)rw;
  const PdCrtLds l(pd_lds, hw, S);
  for (int side = 0; side < 2; side++) {                       // the product of rows t = 0 and t = 1 under this side's factor
    uint32_t* v = side ? l.vq : l.vp;
    for (int w = 0; w < hw; w++) v[w * S] = R[(uint64_t)side * rw + w];
    pd_mul(l.x, v, hw, R + (uint64_t)(2 + side) * rw, 1, hw, S);
    pd_mod(l.x, kw, side ? Q : P, 1, hw, l.mn, S);
    for (int w = 0; w < hw; w++) v[w * S] = l.x[w * S];
  }
  pd_crt(orn, true, l, P, Q, pinv, hw, S);
  pd_load_pair(l.vp, l.vq, R + 4 * (uint64_t)rw, rw, hw, S);
  pd_crt(ort, true, l, P, Q, pinv, hw, S);
}

// ---- gcd(n, v) != 1 for the 3 K B values sn (class 0), z (class 1) and rn (class 2), one per lane: share[class * items + item].
constexpr size_t cki_prove_gcd_lds_words_per_lane(int kw) { return 2 * (size_t)kw; }

__global__ void __launch_bounds__(64) k_cki_prove_gcd(const uint32_t* __restrict__ sn, const uint32_t* __restrict__ z, const uint32_t* __restrict__ rn,
                                                      const uint32_t* __restrict__ n, const uint8_t* __restrict__ kst, uint64_t items, uint32_t K, int kw,
                                                      uint8_t* __restrict__ share) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x;
  const uint64_t v = (uint64_t)blockIdx.x * S + threadIdx.x;
  if (v >= 3 * items) return;
  const uint64_t cls = v / items, item = v - cls * items, key = item / K;
  if (kst[key] != 0) { share[v] = 0; return; }                 // (n = 0 is no modulus; the merge reports the key)
  const uint32_t* X = (cls == 0 ? sn : cls == 1 ? z : rn) + item * (uint64_t)kw;
  uint32_t* ga = pd_lds + threadIdx.x;
  uint32_t* gb = ga + (size_t)kw * S;
  share[v] = wb_coprime_to_odd(X, n + key * (uint64_t)kw, kw, ga, gb, S) ? 0 : 1;
}

// ---- merge, one lane per session: the reference's checks in its order (correct_key.rs:109-156), after the key's own
struct CkiProveMergeArgs {
  const uint8_t* share;                                        // [3][items]
  const uint8_t* kst;
  const uint32_t* e; const uint32_t* e_check;                  // [nkeys][8]: the caller's, H(n, sn.., rn..)
  uint32_t* s_digest;                                          // [nkeys][8]: H(roots) on entry
  uint8_t* error;                                              // [nkeys], nullable
  uint64_t nkeys; uint32_t K;
};
__global__ void __launch_bounds__(256) k_cki_prove_merge(CkiProveMergeArgs a) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nkeys) return;
  const uint64_t items = a.nkeys * a.K;
  uint8_t code = 0;
  if (a.kst[b] != 0) code = ZKP_CK_PROVE_BAD_KEY;
  for (uint32_t cls = 0; cls < 3 && !code; cls++)
    for (uint32_t i = 0; i < a.K; i++) if (a.share[cls * items + b * a.K + i]) code = (uint8_t)(ZKP_CK_PROVE_SN_NOT_COPRIME + cls);
  if (!code) for (int w = 0; w < 8; w++) if (a.e[b * 8 + w] != a.e_check[b * 8 + w]) code = ZKP_CK_PROVE_E_MISMATCH;
  if (code) for (int w = 0; w < 8; w++) a.s_digest[b * 8 + w] = 0u;
  if (a.error) a.error[b] = code;
}

}  // namespace zkp
