// kernels_prime.hpp — the arithmetic around the ladder in the probable-prime test, the next-prime search and seeded Paillier key generation
// (zkp_probable_prime_batch, zkp_next_prime_batch, zkp_paillier_keygen_seeded_batch; the rule is stated in include/zkp_hip.h and restated
// by tests/prime_model.py).  A SLOT is one search: one w, one start, or one factor of one key.  Its window is c_j = c_0 + 2 j, j < 512
// (one candidate for the test), and its state is the survivor map of the window plus a few words:
//   k_prime_window   a slot that needs a window: the start from the keystream (keygen), the residues of c_0 modulo every table prime and
//                    from them the survivor map; the rules for values below 6370^2 are decided here, such values never reach the ladder
//   k_prime_rows     C ladder rows per unresolved slot: the next C survivors under base 2; for a slot whose candidate passed base 2, its
//                    random bases first and the following survivors behind them — modulus c_j, exponent d = (c_j - 1) >> s
//   (SecretLadder's kernels: y = base^d mod c_j)
//   k_prime_tail     one row per lane: y == 1, y == c_j - 1, or up to s - 1 squarings (pd_mul, pd_mod) looking for c_j - 1
//   k_prime_pick     per slot, what the verdicts of its rows mean: dead candidates leave the map, the first base-2 pass becomes the
//                    candidate, a candidate that passed every base resolves the slot, an empty map ends the window
//   k_prime_compact  the unresolved slots of the next round and their number — the one word the host reads per round
// C is a tuning quantity that the host chooses per round: a slot's result is a function of its window and its bases alone.  Nothing here is claimed to run in constant
// time: the number of rounds, rows and squarings depends on the candidates.
#pragma once
#include "chacha_dev.hpp"
#include "kernels_sample.hpp"
#include "kernels_ck_prove.hpp"

namespace zkp {

constexpr uint32_t PRIME_TABLE_BOUND = 6370;                   // the bound of the NiCorrectKeyProof verifier's primorial test
constexpr uint32_t PRIME_EXACT_BELOW = PRIME_TABLE_BOUND * PRIME_TABLE_BOUND;   // a composite below it has a factor in the table
constexpr int PRIME_WINDOW = 512, PRIME_MAP_WORDS = PRIME_WINDOW / 32;
constexpr uint32_t PRIME_MAX_ATTEMPTS = 128, PRIME_MAX_ROUNDS = 64;
constexpr uint32_t PRIME_NO_J = 0xffffffffu;

// all odd primes below PRIME_TABLE_BOUND, by a sieve at compile time: ONE initialiser for the device table and for the host copy that
// zkp_diag_prime_table reports
struct PrimeTable { uint16_t p[1024]; uint32_t count; };
constexpr PrimeTable make_prime_table() {
  PrimeTable t{};
  bool composite[PRIME_TABLE_BOUND] = {};
  for (uint32_t i = 2; i < PRIME_TABLE_BOUND; i++) {
    if (composite[i]) continue;
    if (i != 2) t.p[t.count++] = (uint16_t)i;
    for (uint32_t k = i * i; k < PRIME_TABLE_BOUND; k += i) composite[k] = true;
  }
  return t;
}
constexpr PrimeTable PRIME_TABLE_HOST = make_prime_table();
static __device__ const PrimeTable PRIME_TABLE_DEV = make_prime_table();

enum PrimeMode : int { PRIME_MODE_TEST = 0, PRIME_MODE_NEXT = 1, PRIME_MODE_KEYGEN = 2 };
enum PrimeState : uint32_t { PRIME_ST_NEW = 0, PRIME_ST_SEARCH = 1, PRIME_ST_CONFIRM = 2, PRIME_ST_DONE = 3 };

struct PrimeArgs {
  const uint32_t* key;                                         // the seed as 8 words (null: rounds == 0 and no keygen)
  uint64_t first_index, slot0;                                 // slot0: the call-wide number of this slab's slot 0
  int mode, pw, rounds, C;
  uint32_t nslots;
  const uint32_t* in;                                          // [nslots][pw]   w / start of this slab (test, next)
  uint32_t* start;                                             // [nslots][pw]   c_0 of the current window
  uint32_t* map;                                               // [nslots][16]   bit j: c_j is alive
  uint32_t* state; uint32_t* attempt; uint32_t* cand; uint32_t* next_r;         // [nslots]
  uint32_t* found_j;                                           // [nslots]   j of the prime of a DONE slot, PRIME_NO_J: none
  uint32_t* mods; uint32_t* base; uint32_t* exp;               // [rows][64], [rows][64], [rows][pw]
  const uint32_t* lad;                                         // [rows][64]   what the ladder returned
  uint32_t* row_j;                                             // [rows]   the candidate of a row, PRIME_NO_J: a filler row
  uint8_t* row_ok;                                             // [rows]
  const uint32_t* active; uint32_t nactive;                    // the unresolved slots of this round
  uint32_t* next_active; uint32_t* next_count;
  uint32_t nrows;                                              // rows of the ladder launch (>= nactive C)
};
constexpr int PRIME_ROW_WORDS = 64;                            // the ladder's row at mod_bits = 2048

__device__ __forceinline__ uint64_t prime_item(const PrimeArgs& a, uint32_t slot) {
  const uint64_t g = a.slot0 + slot;
  return a.mode == PRIME_MODE_KEYGEN ? g >> 1 : g;
}
__device__ __forceinline__ uint32_t prime_side(const PrimeArgs& a, uint32_t slot) { return a.mode == PRIME_MODE_KEYGEN ? (uint32_t)((a.slot0 + slot) & 1) : 0u; }

__global__ void __launch_bounds__(256) k_prime_init(PrimeArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nslots) return;
  a.state[i] = PRIME_ST_NEW; a.attempt[i] = 0; a.cand[i] = 0; a.next_r[i] = 0; a.found_j[i] = PRIME_NO_J;
  a.next_active[i] = i;
  if (i == 0) *a.next_count = a.nslots;
}

// ---- window: one block of 64 lanes per unresolved slot; (slot, prime) spread over the lanes.  Horner over 16-bit half-limbs: a residue is
// below 2^13, so (r << 16 | half) stays below 2^29.
__global__ void __launch_bounds__(64) k_prime_window(PrimeArgs a) {
  __shared__ uint32_t sw[PRIME_ROW_WORDS];
  __shared__ uint32_t smap[PRIME_MAP_WORDS];
  __shared__ uint32_t sflag[2];                                // [1]: 1 = the window held nothing, go round again with the next attempt
  const uint32_t slot = a.active[blockIdx.x];
  if (a.state[slot] != PRIME_ST_NEW) return;
  const int pw = a.pw, lane = (int)threadIdx.x;
  const int window = a.mode == PRIME_MODE_TEST ? 1 : PRIME_WINDOW;
  const uint64_t index = a.first_index + prime_item(a, slot);
  const uint32_t side = prime_side(a, slot);
  uint32_t attempt = a.attempt[slot];
  for (;;) {
    if (a.mode == PRIME_MODE_KEYGEN) {
      const int nb = (pw + 15) / 16;
      if (lane < nb) {
        uint32_t key[8], v[16];
        for (int i = 0; i < 8; i++) key[i] = a.key[i];
        chacha20_block(key, attempt * (uint32_t)nb + (uint32_t)lane, (uint32_t)index, (uint32_t)(index >> 32), nonce_word15(ZKP_SEEDED_KIND_KEYGEN, 0u, side), v);
        for (int i = 0; i < 16; i++) if (lane * 16 + i < pw) sw[lane * 16 + i] = v[i];
      }
      __syncthreads();
      if (lane == 0) { sw[0] |= 1u; sw[pw - 1] |= 0x80000000u; }
    } else {
      for (int w = lane; w < pw; w += 64) sw[w] = a.in[(uint64_t)slot * pw + w];
      __syncthreads();
      if (lane == 0 && a.mode == PRIME_MODE_NEXT) sw[0] |= 1u;
    }
    if (lane < PRIME_MAP_WORDS) smap[lane] = window == 1 ? (lane == 0 ? 1u : 0u) : 0xffffffffu;
    __syncthreads();
    bool hi_zero = true;
    for (int w = 1; w < pw; w++) hi_zero = hi_zero && sw[w] == 0u;
    const uint32_t w0 = sw[0];
    const bool even = (w0 & 1u) == 0u;                         // (the test alone: its c_0 is w itself)
    const bool small = hi_zero && w0 < PRIME_EXACT_BELOW;
    if (lane == 0 && window > 1) {                             // candidates at or beyond 2^bits leave the window: 2^bits - 1 - c_0 = 2 (j_max)
      bool room = false;
      for (int w = 1; w < pw; w++) room = room || sw[w] != 0xffffffffu;
      const uint32_t jmax = ~w0 >> 1;
      if (!room && jmax < (uint32_t)(window - 1))
        for (int j = (int)jmax + 1; j < window; j++) smap[j >> 5] &= ~(1u << (j & 31));
    }
    __syncthreads();
    if (!even) {
      for (uint32_t pi = (uint32_t)lane; pi < PRIME_TABLE_DEV.count; pi += 64) {
        const uint32_t l = PRIME_TABLE_DEV.p[pi];
        uint32_t r = 0;
        for (int w = pw - 1; w >= 0; w--) {
          const uint32_t v = sw[w];
          r = ((r << 16) | (v >> 16)) % l;
          r = ((r << 16) | (v & 0xffffu)) % l;
        }
        // c_j = c_0 + 2 j is divisible by l  <=>  j = (l - r) 2^-1 mod l, 2^-1 = (l + 1) / 2
        const uint32_t j0 = r == 0 ? 0u : ((l - r) * ((l + 1) >> 1)) % l;
        for (uint32_t j = j0; j < (uint32_t)window; j += l) {
          if (small && w0 + 2 * j == l) continue;              // c_j IS the table prime
          atomicAnd(&smap[j >> 5], ~(1u << (j & 31)));
        }
      }
    }
    __syncthreads();
    if (lane == 0) {
      sflag[1] = 0;
      uint32_t st = PRIME_ST_SEARCH, found = PRIME_NO_J;
      if (even) {                                              // w even: prime iff w == 2
        st = PRIME_ST_DONE;
        if (hi_zero && w0 == 2u) found = 0;
      } else {
        if (small && w0 == 1u) smap[0] &= ~1u;                 // 1 is no prime
        int first = -1;
        for (int k = 0; k < PRIME_MAP_WORDS && first < 0; k++) if (smap[k]) first = k * 32 + __builtin_ctz(smap[k]);
        if (first < 0) {                                       // nothing survived: the window is used up
          if (a.mode == PRIME_MODE_KEYGEN && attempt + 1 < PRIME_MAX_ATTEMPTS) { st = PRIME_ST_NEW; sflag[1] = 1; }
          else st = PRIME_ST_DONE;
        } else if (small && w0 + 2 * (uint32_t)first < PRIME_EXACT_BELOW) {       // a survivor below 6370^2 is prime, exactly
          st = PRIME_ST_DONE; found = (uint32_t)first;
        }
      }
      a.state[slot] = st; a.attempt[slot] = attempt + sflag[1]; a.found_j[slot] = found;
    }
    __syncthreads();
    if (!sflag[1]) break;
    attempt++;
    __syncthreads();
  }
  for (int w = lane; w < pw; w += 64) a.start[(uint64_t)slot * pw + w] = sw[w];
  if (lane < PRIME_MAP_WORDS) a.map[(uint64_t)slot * PRIME_MAP_WORDS + lane] = smap[lane];
}

// ---- rows: one thread per (unresolved slot, row).
// base a_r = 2 + (the first ceil((L - 2) / 32) keystream words of (index, slot r, field), masked to L - 2 bits), L = bit_length(c_j)
__device__ __forceinline__ void prime_base(const PrimeArgs& a, uint64_t index, uint32_t r, uint32_t field, int L, uint32_t* out) {
  const int vb = L - 2, nw = (vb + 31) / 32;
  uint32_t key[8], v[16];
  for (int i = 0; i < 8; i++) key[i] = a.key[i];
  uint32_t carry = 2;
  for (int w = 0; w < PRIME_ROW_WORDS; w++) {
    uint32_t x = 0;
    if (w < nw) {
      if ((w & 15) == 0) chacha20_block(key, (uint32_t)(w >> 4), (uint32_t)index, (uint32_t)(index >> 32), nonce_word15(ZKP_SEEDED_KIND_KEYGEN, r, field), v);
      x = v[w & 15];
      if (w == nw - 1 && (vb & 31)) x &= (1u << (vb & 31)) - 1u;
    }
    const uint64_t t = (uint64_t)x + carry;
    out[w] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
}

__global__ void __launch_bounds__(64) k_prime_rows(PrimeArgs a) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.nrows) return;
  const int pw = a.pw;
  uint32_t* M = a.mods + (uint64_t)row * PRIME_ROW_WORDS;
  uint32_t* B = a.base + (uint64_t)row * PRIME_ROW_WORDS;
  uint32_t* E = a.exp + (uint64_t)row * pw;
  const uint32_t ai = row / (uint32_t)a.C, k = row % (uint32_t)a.C;
  uint32_t j = PRIME_NO_J, r = 0, slot = 0;
  if (ai < a.nactive) {
    slot = a.active[ai];
    const uint32_t st = a.state[slot];
    // a slot in search: the k-th survivor in order of j.  A slot whose candidate is under its random bases: `cnt` rows for the bases, and
    // behind them the search goes on speculatively — the survivors after the candidate under base 2, used only if the candidate falls
    uint32_t cnt = 0;
    if (st == PRIME_ST_CONFIRM) {
      cnt = min((uint32_t)a.rounds + 1u - a.next_r[slot], (uint32_t)a.C);
      if (k < cnt) { j = a.cand[slot]; r = a.next_r[slot] + k; }
    }
    if ((st == PRIME_ST_SEARCH || st == PRIME_ST_CONFIRM) && k >= cnt) {
      const uint32_t* map = a.map + (uint64_t)slot * PRIME_MAP_WORDS;
      uint32_t skip = k - cnt;
      for (int w = 0; w < PRIME_MAP_WORDS && j == PRIME_NO_J; w++) {
        uint32_t bits = map[w];
        const uint32_t n = (uint32_t)__builtin_popcount(bits);
        if (skip >= n) { skip -= n; continue; }
        for (; skip; skip--) bits &= bits - 1u;
        j = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(bits);
      }
    }
  }
  a.row_j[row] = j;
  if (j == PRIME_NO_J) {                                       // a filler row: 0^0 under the modulus 3, as k_pdec_split's rows of a bad key
    for (int w = 0; w < PRIME_ROW_WORDS; w++) { M[w] = w == 0 ? 3u : 0u; B[w] = 0u; }
    for (int w = 0; w < pw; w++) E[w] = 0u;
    return;
  }
  const uint32_t* S0 = a.start + (uint64_t)slot * pw;
  uint32_t carry = 2 * j;
  int top = 0;
  for (int w = 0; w < PRIME_ROW_WORDS; w++) {                  // c_j = c_0 + 2 j   (below 2^bits: the window's limit)
    const uint64_t t = (uint64_t)(w < pw ? S0[w] : 0u) + carry;
    M[w] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
    if ((uint32_t)t) top = w;
  }
  // d = (c_j - 1) >> s
  int s = 0;
  for (int w = 0; w < pw; w++) {
    const uint32_t v = w == 0 ? M[0] & ~1u : M[w];
    if (v) { s = w * 32 + __builtin_ctz(v); break; }
  }
  const int sw_ = s >> 5, sb = s & 31;
  for (int w = 0; w < pw; w++) {
    const int lo_i = w + sw_, hi_i = w + sw_ + 1;
    const uint32_t lo = lo_i < pw ? (lo_i == 0 ? M[0] & ~1u : M[lo_i]) : 0u;
    const uint32_t hi = hi_i < pw ? M[hi_i] : 0u;
    E[w] = sb ? (lo >> sb) | (hi << (32 - sb)) : lo;
  }
  if (r == 0) {
    for (int w = 0; w < PRIME_ROW_WORDS; w++) B[w] = w == 0 ? 2u : 0u;
  } else {
    const int L = top * 32 + 32 - __builtin_clz(M[top]);
    prime_base(a, a.first_index + prime_item(a, slot), r, 2u + prime_side(a, slot), L, B);
  }
}

// ---- tail, one row per lane: the strong test's verdict from y = base^d mod c_j
constexpr size_t prime_tail_lds_words_per_lane(int pw) { return 4 * (size_t)pw + 1; }

__global__ void __launch_bounds__(64) k_prime_tail(PrimeArgs a) {
  extern __shared__ __align__(16) uint32_t pd_lds[];
  const int S = (int)blockDim.x, pw = a.pw;
  const uint32_t row = blockIdx.x * S + threadIdx.x;
  if (row >= a.nrows) return;
  if (a.row_j[row] == PRIME_NO_J) { a.row_ok[row] = 0; return; }
  const uint32_t* M = a.mods + (uint64_t)row * PRIME_ROW_WORDS;
  const uint32_t* Y = a.lad + (uint64_t)row * PRIME_ROW_WORDS;
  uint32_t* x = pd_lds + threadIdx.x;                          // 2 pw + 1 words
  uint32_t* y = x + (size_t)(2 * pw + 1) * S;                  // pw words
  uint32_t* mn = y + (size_t)pw * S;                           // pw words
  int s = 0;
  for (int w = 0; w < pw; w++) {
    const uint32_t v = w == 0 ? M[0] & ~1u : M[w];
    if (v) { s = w * 32 + __builtin_ctz(v); break; }
  }
  for (int w = 0; w < pw; w++) y[w * S] = Y[w];
  bool ok = false;
  for (int it = 0;; it++) {
    bool one = true, minus = true;                             // y == 1, y == c_j - 1
    for (int w = 0; w < pw; w++) {
      const uint32_t v = y[w * S];
      one = one && v == (w == 0 ? 1u : 0u);
      minus = minus && v == (w == 0 ? M[0] & ~1u : M[w]);
    }
    if (minus || (one && it == 0)) { ok = true; break; }
    if (one || it + 1 >= s) break;                             // 1 without -1 before it, or s - 1 squarings made: composite
    pd_mul(x, y, pw, y, S, pw, S);
    pd_mod(x, 2 * pw, M, 1, pw, mn, S);
    for (int w = 0; w < pw; w++) y[w * S] = x[w * S];
  }
  a.row_ok[row] = ok ? 1 : 0;
}

// ---- pick, one thread per unresolved slot
__global__ void __launch_bounds__(64) k_prime_pick(PrimeArgs a) {
  const uint32_t ai = blockIdx.x * blockDim.x + threadIdx.x;
  if (ai >= a.nactive) return;
  const uint32_t slot = a.active[ai];
  uint32_t* map = a.map + (uint64_t)slot * PRIME_MAP_WORDS;
  const uint32_t row0 = ai * (uint32_t)a.C;
  uint32_t st = a.state[slot];
  int k0 = 0;                                                  // the first row of the slot that is a search row
  if (st == PRIME_ST_CONFIRM) {
    const uint32_t cnt = min((uint32_t)a.rounds + 1u - a.next_r[slot], (uint32_t)a.C);
    bool all = true;
    for (uint32_t k = 0; k < cnt; k++) all = all && a.row_ok[row0 + k] != 0;
    if (!all) { st = PRIME_ST_SEARCH; k0 = (int)cnt; }         // composite: the search goes on behind it, with the rows that ran ahead
    else {
      const uint32_t nr = a.next_r[slot] + cnt;
      a.next_r[slot] = nr;
      if (nr > (uint32_t)a.rounds) { st = PRIME_ST_DONE; a.found_j[slot] = a.cand[slot]; }
    }
  }
  if (st == PRIME_ST_SEARCH) {
    for (int k = k0; k < a.C; k++) {
      const uint32_t j = a.row_j[row0 + k];
      if (j == PRIME_NO_J) break;
      map[j >> 5] &= ~(1u << (j & 31));                        // tested: dead, or the candidate
      if (!a.row_ok[row0 + k]) continue;
      if (a.rounds == 0) { st = PRIME_ST_DONE; a.found_j[slot] = j; }
      else { st = PRIME_ST_CONFIRM; a.cand[slot] = j; a.next_r[slot] = 1; }
      break;                                                   // (later rows of this chunk come again if the candidate falls)
    }
  }
  if (st == PRIME_ST_SEARCH) {
    bool any = false;
    for (int w = 0; w < PRIME_MAP_WORDS; w++) any = any || map[w] != 0u;
    if (!any) {                                                // the window is used up
      const uint32_t t = a.attempt[slot] + 1;
      if (a.mode == PRIME_MODE_KEYGEN && t < PRIME_MAX_ATTEMPTS) { st = PRIME_ST_NEW; a.attempt[slot] = t; }
      else st = PRIME_ST_DONE;
    }
  }
  a.state[slot] = st;
}

__global__ void __launch_bounds__(256) k_prime_compact(PrimeArgs a) {
  const uint32_t ai = blockIdx.x * blockDim.x + threadIdx.x;
  if (ai >= a.nactive) return;
  const uint32_t slot = a.active[ai];
  if (a.state[slot] != PRIME_ST_DONE) a.next_active[atomicAdd(a.next_count, 1u)] = slot;
}

// ---- results.  value = c_0 + 2 j of a slot that found one
__device__ __forceinline__ void prime_value(const PrimeArgs& a, uint32_t slot, bool found, uint32_t* out) {
  const uint32_t* S0 = a.start + (uint64_t)slot * a.pw;
  uint32_t carry = found ? 2 * a.found_j[slot] : 0u;
  for (int w = 0; w < a.pw; w++) {
    const uint64_t t = (uint64_t)S0[w] + carry;
    out[w] = found ? (uint32_t)t : 0u;
    carry = (uint32_t)(t >> 32);
  }
}

// test and next: out_* point at this slab's first slot; every one of them nullable
__global__ void __launch_bounds__(256) k_prime_out(PrimeArgs a, uint8_t* verdict, uint32_t* out_prime, uint32_t* out_offset, uint8_t* out_status) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= a.nslots) return;
  const bool found = a.found_j[slot] != PRIME_NO_J;
  if (verdict) verdict[slot] = found ? 1 : 0;
  if (out_prime) prime_value(a, slot, found, out_prime + (uint64_t)slot * a.pw);
  if (out_offset) out_offset[slot] = found ? a.found_j[slot] : 0u;
  if (out_status) out_status[slot] = found ? 0 : 2;
}

// keygen: slots 2 b and 2 b + 1 are p and q of key b; a key one of whose searches found nothing, or with p == q, is zero and status 2
__global__ void __launch_bounds__(256) k_prime_out_key(PrimeArgs a, uint32_t* out_p, uint32_t* out_q, uint8_t* out_status) {
  const uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
  if (2 * key >= a.nslots) return;
  const uint32_t sp = 2 * key, sq = 2 * key + 1;
  uint32_t* P = out_p + (uint64_t)key * a.pw;
  uint32_t* Q = out_q + (uint64_t)key * a.pw;
  bool ok = a.found_j[sp] != PRIME_NO_J && a.found_j[sq] != PRIME_NO_J;
  prime_value(a, sp, ok, P);
  prime_value(a, sq, ok, Q);
  if (ok) {
    bool same = true;
    for (int w = 0; w < a.pw; w++) same = same && P[w] == Q[w];
    if (same) { ok = false; for (int w = 0; w < a.pw; w++) { P[w] = 0u; Q[w] = 0u; } }
  }
  out_status[key] = ok ? 0 : 2;
}

}  // namespace zkp
