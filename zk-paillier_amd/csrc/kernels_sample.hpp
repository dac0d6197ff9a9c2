// kernels_sample.hpp — the witness of RangeProofNi::prove expanded on the device from a 32-byte seed (include/zkp_hip.h:
// zkp_range_sample_witness_batch; the stream is defined in DESIGN.md section 4 and restated by tests/seeded_model.py), and below it the
// nonces of the sigma proofs and of CompositeDLogProof (zkp_nonce_sample_batch, tests/seeded_nonce_model.py), and the two operands of the verifier's
// commitment of the interactive RangeProof (zkp_range_verifier_commit_seeded_batch, tests/seeded_commit_model.py).
//
// Per row the reference draws w1, w2, a coin, r1 and r2 (range_proof.rs:133-159).  Here every (proof, row, field) has a ChaCha20
// stream of its own — key = the seed, nonce = (index lo, index hi, row << 2 | field) — and sample_below(u) reads WHOLE blocks per
// attempt, so lanes compute blocks and attempts independently of one another.
//
// Geometry: a group of G = kw / 16 lanes per (proof, row, field); lane l of a group holds words [16 l, 16 l + 16) of the kw-word value,
// i.e. the keystream block with counter attempt * nb + l.  Consecutive lanes hold consecutive 64-byte pieces of a row, so a group's
// stores cover the row without gaps.  The comparison `< u` is decided by the most significant lane that differs (two ballots); the
// carry of third + s crosses the lanes of a group the same way.  Every loop is bounded (max_attempts).
// Tasks are numbered field-major, so the lanes of a wavefront nearly always work on one field.
#pragma once
#include "chacha_dev.hpp"
#include "sha256_dev.hpp"

namespace zkp {

struct RangeSampleArgs {
  const uint32_t* key;        // the seed as 8 little-endian words (device memory)
  const uint32_t* n; uint64_t n_stride;
  const uint32_t* range;      // [B][kw]
  uint32_t* third;            // [B][kw]  floor(range / 3)         (written by k_range_sample_prep)
  uint32_t* meta;             // [B][2]   bit_length(third), bit_length(n)
  uint32_t* w1; uint32_t* w2; uint32_t* r1; uint32_t* r2;   // [B][EF][kw], 16-byte aligned
  uint8_t* status;            // [B] 0 | ZKP_VERDICT_MALFORMED
  uint64_t first_index, batch;
  uint32_t kw, ef, max_attempts;
};

// one thread per proof: third = floor(range / 3), the bit lengths of both bounds, status = MALFORMED for an empty interval
// (third == 0, i.e. range < 3 — or n == 0)
__global__ void __launch_bounds__(256) k_range_sample_prep(RangeSampleArgs a) {
  const uint64_t b = blockIdx.x * 256ull + threadIdx.x;
  if (b >= a.batch) return;
  const uint32_t* q = a.range + b * a.kw;
  const uint32_t* n = a.n + b * a.n_stride;
  uint32_t* t = a.third + b * a.kw;
  uint32_t rem = 0, tbits = 0, nbits = 0;
  for (int i = (int)a.kw - 1; i >= 0; i--) {
    const uint64_t cur = ((uint64_t)rem << 32) | q[i];
    const uint32_t d = (uint32_t)(cur / 3);
    rem = (uint32_t)(cur - 3ull * d);
    t[i] = d;
    if (d && !tbits) tbits = 32u * (uint32_t)i + 32u - (uint32_t)__clz((int)d);
    const uint32_t nv = n[i];
    if (nv && !nbits) nbits = 32u * (uint32_t)i + 32u - (uint32_t)__clz((int)nv);
  }
  a.meta[2 * b] = tbits;
  a.meta[2 * b + 1] = nbits;
  a.status[b] = (tbits == 0 || nbits == 0) ? 2 : 0;
}

template <int G>
__global__ void __launch_bounds__(256) k_range_sample(RangeSampleArgs a) {
  static_assert(G == 2 || G == 4 || G == 8, "kw = 32, 64 or 128 words");
  constexpr uint64_t GM = (1ull << G) - 1;
  const uint64_t gid = blockIdx.x * 256ull + threadIdx.x;
  const uint64_t task = gid / G, rows = a.batch * a.ef;
  const uint32_t l = (uint32_t)(gid % G);
  if (task >= 3 * rows) return;                                  // (whole groups leave together: 256 and 64 are multiples of G)
  const uint32_t f = (uint32_t)(task / rows);                    // 0 = w, 1 = r1, 2 = r2
  const uint64_t br = task - (uint64_t)f * rows, b = br / a.ef;
  const uint32_t row = (uint32_t)(br - b * a.ef);
  const uint32_t tbits = a.meta[2 * b], nbits = a.meta[2 * b + 1];
  if (tbits == 0 || nbits == 0) return;                          // an empty interval: k_range_sample_fixup zeroes the proof's rows
  const uint32_t g0 = (threadIdx.x & 63u) - l;                   // the group's first bit in a ballot
  const uint32_t bits = f ? nbits : tbits, nw = (bits + 31) / 32, nb = (nw + 15) / 16;
  const uint32_t topmask = (bits & 31u) ? (1u << (bits & 31u)) - 1u : 0xffffffffu;
  const uint32_t* u = f ? a.n + b * a.n_stride : a.third + b * a.kw;
  uint32_t uw[16], key[8], v[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { const uint32_t wi = 16 * l + i; uw[i] = wi < nw ? u[wi] : 0u; v[i] = 0u; }
#pragma unroll
  for (int i = 0; i < 8; i++) key[i] = a.key[i];
  const uint64_t index = a.first_index + b;
  const uint32_t n0 = (uint32_t)index, n1 = (uint32_t)(index >> 32), n2 = (row << 2) | f;

  bool active = true, ok = false;
  for (uint32_t t = 0; t < a.max_attempts; t++) {
    int c = 0;
    if (active) {
      if (l < nb) {
        chacha20_block(key, t * nb + l, n0, n1, n2, v);
#pragma unroll
        for (int i = 0; i < 16; i++) { const uint32_t wi = 16 * l + i; if (wi >= nw) v[i] = 0u; else if (wi == nw - 1) v[i] &= topmask; }
      }
#pragma unroll
      for (int i = 15; i >= 0; i--) if (c == 0 && v[i] != uw[i]) c = v[i] < uw[i] ? -1 : 1;
    }
    const uint64_t ne = __ballot(active && c != 0), lt = __ballot(active && c < 0);
    if (active) {
      const uint32_t m = (uint32_t)((ne >> g0) & GM);
      if (m) ok = ((lt >> (g0 + (31u - (uint32_t)__clz((int)m)))) & 1ull) != 0;      // the most significant lane that differs decides
      if (ok) active = false;
    }
    if (__ballot(active) == 0) break;
  }
  if (!ok) {                     // max_attempts rejections in a row (probability <= 2^-max_attempts): the whole proof is zeroed by k_range_sample_fixup
    if (l == 0) a.status[b] = 2;
    return;
  }
  const uint64_t off = br * a.kw + 16 * l;
  if (f) {
    uint4* o = (uint4*)((f == 1 ? a.r1 : a.r2) + off);
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    return;
  }
  // field 0: a = third + s with s = v < third; the carry crosses the lanes of the group (generate / propagate masks, one addition)
  uint32_t sum[16], carry = 0;
  bool all_ones = true;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint64_t x = (uint64_t)v[i] + uw[i] + carry;
    sum[i] = (uint32_t)x; carry = (uint32_t)(x >> 32);
    all_ones = all_ones && sum[i] == 0xffffffffu;
  }
  const uint64_t gen = (__ballot(carry != 0) >> g0) & GM, prop = (__ballot(all_ones) >> g0) & GM;
  uint32_t cin = (uint32_t)(((((gen << 1) + prop) ^ prop) >> l) & 1ull);
#pragma unroll
  for (int i = 0; i < 16; i++) { sum[i] += cin; cin = (cin && sum[i] == 0u) ? 1u : 0u; }
  uint32_t cs[16];
  chacha20_block(key, 0u, n0, n1, (row << 2) | 3u, cs);
  const bool coin = (cs[0] & 1u) != 0;                           // (w1, w2) = (a, a - third), swapped when the coin is 1
  uint4* o1 = (uint4*)(a.w1 + off);
  uint4* o2 = (uint4*)(a.w2 + off);
  uint32_t first[16], second[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { first[i] = coin ? v[i] : sum[i]; second[i] = coin ? sum[i] : v[i]; }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    o1[i] = make_uint4(first[4 * i], first[4 * i + 1], first[4 * i + 2], first[4 * i + 3]);
    o2[i] = make_uint4(second[4 * i], second[4 * i + 1], second[4 * i + 2], second[4 * i + 3]);
  }
}

// 16 words per thread: the four rows of every (proof, row) whose proof is MALFORMED become zero
template <int G>
__global__ void __launch_bounds__(256) k_range_sample_fixup(RangeSampleArgs a) {
  const uint64_t gid = blockIdx.x * 256ull + threadIdx.x, br = gid / G;
  if (br >= a.batch * a.ef || a.status[br / a.ef] == 0) return;
  const uint64_t off = br * a.kw + 16 * (gid % G);
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  uint32_t* const arrays[4] = {a.w1, a.w2, a.r1, a.r2};
  for (int k = 0; k < 4; k++)
    for (int i = 0; i < 4; i++) ((uint4*)(arrays[k] + off))[i] = z;
}

// ---- the nonces of ZeroProof, CiphertextProof, CorrectMessageProof and CompositeDLogProof (include/zkp_hip.h: zkp_nonce_sample_batch) ----
// The same construction on streams of their own: state word 15 = 0x80000000 | kind << 20 | slot << 4 | field (bit 31 keeps them apart from
// every range stream, whose word 15 is below 1024).  A proof has up to three sample_below(n) fields — slot 0, or slots 1 .. K - 1 of a
// CorrectMessageProof — and at most one field that is the first 8 or 16 words of block 0 as they come (e_sim, the DLog r).
struct NonceSampleArgs {
  const uint32_t* key;        // the seed as 8 little-endian words (device memory)
  const uint32_t* n; uint64_t n_stride;      // (null for a kind without sample_below fields)
  uint32_t* meta;             // [B] bit_length(n)                 (written by k_nonce_prep)
  uint32_t* below[3];         // the sample_below fields: [B][below_per][kw], 16-byte aligned
  uint32_t* raw;              // the power-of-two field: [B][raw_per][raw_words], 16-byte aligned
  uint8_t* status;            // [B] 0 | ZKP_VERDICT_MALFORMED
  uint64_t first_index, batch;
  uint32_t kw, kind, max_attempts;
  uint32_t nbelow, below_field[3], below_per[3], below_slot0[3];
  uint32_t raw_field, raw_per, raw_slot0, raw_words;      // raw_words = 0: the kind has no such field
};

__device__ __forceinline__ uint32_t nonce_word15(uint32_t kind, uint32_t slot, uint32_t field) { return 0x80000000u | (kind << 20) | (slot << 4) | field; }

// one thread per proof: the bit length of n, status = MALFORMED for n == 0
__global__ void __launch_bounds__(256) k_nonce_prep(NonceSampleArgs a) {
  const uint64_t b = blockIdx.x * 256ull + threadIdx.x;
  if (b >= a.batch) return;
  uint32_t nbits = 1;
  if (a.n) {
    const uint32_t* n = a.n + b * a.n_stride;
    nbits = 0;
    for (int i = (int)a.kw - 1; i >= 0 && !nbits; i--) {
      const uint32_t nv = n[i];
      if (nv) nbits = 32u * (uint32_t)i + 32u - (uint32_t)__clz((int)nv);
    }
  }
  a.meta[b] = nbits;
  a.status[b] = nbits == 0 ? 2 : 0;
}

// G lanes per (proof, slot, sample_below field), numbered field-major; the attempt loop is k_range_sample's
template <int G>
__global__ void __launch_bounds__(256) k_nonce_sample(NonceSampleArgs a) {
  static_assert(G == 2 || G == 4 || G == 8, "kw = 32, 64 or 128 words");
  constexpr uint64_t GM = (1ull << G) - 1;
  const uint64_t gid = blockIdx.x * 256ull + threadIdx.x;
  uint64_t task = gid / G;
  const uint32_t l = (uint32_t)(gid % G);
  uint32_t field = 0, per = 1, slot0 = 0;
  uint32_t* out = nullptr;
  bool found = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (!found && (uint32_t)k < a.nbelow) {
      const uint64_t count = a.batch * a.below_per[k];
      if (task < count) { found = true; field = a.below_field[k]; per = a.below_per[k]; slot0 = a.below_slot0[k]; out = a.below[k]; }
      else task -= count;
    }
  }
  if (!found) return;                                            // (whole groups leave together: 256 and 64 are multiples of G)
  const uint64_t b = task / per;
  const uint32_t slot = slot0 + (uint32_t)(task - b * per);
  const uint32_t bits = a.meta[b];
  if (bits == 0) return;                                         // n == 0: k_nonce_fixup zeroes the proof's nonces
  const uint32_t g0 = (threadIdx.x & 63u) - l;                   // the group's first bit in a ballot
  const uint32_t nw = (bits + 31) / 32, nb = (nw + 15) / 16;
  const uint32_t topmask = (bits & 31u) ? (1u << (bits & 31u)) - 1u : 0xffffffffu;
  const uint32_t* u = a.n + b * a.n_stride;
  uint32_t uw[16], key[8], v[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { const uint32_t wi = 16 * l + i; uw[i] = wi < nw ? u[wi] : 0u; v[i] = 0u; }
#pragma unroll
  for (int i = 0; i < 8; i++) key[i] = a.key[i];
  const uint64_t index = a.first_index + b;
  const uint32_t n0 = (uint32_t)index, n1 = (uint32_t)(index >> 32), n2 = nonce_word15(a.kind, slot, field);

  bool active = true, ok = false;
  for (uint32_t t = 0; t < a.max_attempts; t++) {
    int c = 0;
    if (active) {
      if (l < nb) {
        chacha20_block(key, t * nb + l, n0, n1, n2, v);
#pragma unroll
        for (int i = 0; i < 16; i++) { const uint32_t wi = 16 * l + i; if (wi >= nw) v[i] = 0u; else if (wi == nw - 1) v[i] &= topmask; }
      }
#pragma unroll
      for (int i = 15; i >= 0; i--) if (c == 0 && v[i] != uw[i]) c = v[i] < uw[i] ? -1 : 1;
    }
    const uint64_t ne = __ballot(active && c != 0), lt = __ballot(active && c < 0);
    if (active) {
      const uint32_t m = (uint32_t)((ne >> g0) & GM);
      if (m) ok = ((lt >> (g0 + (31u - (uint32_t)__clz((int)m)))) & 1ull) != 0;      // the most significant lane that differs decides
      if (ok) active = false;
    }
    if (__ballot(active) == 0) break;
  }
  if (!ok) {                     // max_attempts rejections in a row: every nonce of the proof is zeroed by k_nonce_fixup
    if (l == 0) a.status[b] = 2;
    return;
  }
  uint4* o = (uint4*)(out + task * a.kw + 16 * l);
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

// one lane per (proof, slot) of the power-of-two field: words [0, raw_words) of block 0, no comparison
__global__ void __launch_bounds__(256) k_nonce_raw(NonceSampleArgs a) {
  const uint64_t task = blockIdx.x * 256ull + threadIdx.x;
  if (task >= a.batch * a.raw_per) return;
  const uint64_t b = task / a.raw_per;
  const uint32_t slot = a.raw_slot0 + (uint32_t)(task - b * a.raw_per);
  uint32_t key[8], v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) key[i] = a.key[i];
  const uint64_t index = a.first_index + b;
  chacha20_block(key, 0u, (uint32_t)index, (uint32_t)(index >> 32), nonce_word15(a.kind, slot, a.raw_field), v);
  uint4* o = (uint4*)(a.raw + task * a.raw_words);
#pragma unroll
  for (int i = 0; i < 4; i++) if (4u * (uint32_t)i < a.raw_words) o[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

// four words per thread: every nonce of a MALFORMED proof becomes zero
__global__ void __launch_bounds__(256) k_nonce_fixup(NonceSampleArgs a) {
  const uint64_t gid = blockIdx.x * 256ull + threadIdx.x;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint32_t* out = k < 3 ? a.below[k] : a.raw;
    const bool present = k < 3 ? (uint32_t)k < a.nbelow : a.raw_words != 0;
    const uint64_t quads = k < 3 ? (uint64_t)a.below_per[k] * a.kw / 4 : (uint64_t)a.raw_per * a.raw_words / 4;      // per proof
    if (present && quads && gid < a.batch * quads && a.status[gid / quads]) ((uint4*)out)[gid] = z;
  }
}

// ---- the verifier's commitment of the interactive RangeProof (include/zkp_hip.h: zkp_range_verifier_commit_seeded_batch and its two
// neighbours; tests/seeded_commit_model.py) ----
// RangeProof::verifier_commit (range_proof.rs:118-126) sends com = Enc(ek_v, from(SHA256(e)), r); verify_commit (:195-208) recomputes it.
// This kernel makes the two operands of that ONE Enc per session; the Enc itself is the existing launch.  G lanes per session:
//   seeded (key != null): r = sample_below(n) on stream (kind 7, slot 0, field 0) — the attempt loop is k_nonce_sample's —, e = the first
//     e_len bytes of block 0 of field 1; e_in / e_len_in are not read;
//   given  (key == null): e = the caller's e_in[b][0 .. e_len_in[b]); r is the caller's and is not touched.
//   m (nullable) = the 32 digest bytes of SHA256(e) read big-endian, as kw little-endian limbs: one block, since e_len <= 32.
// A session whose key is outside the domain (even — zero included —, or of at most 256 bits: m < 2^256 must be a canonical plaintext), whose
// e_len_in is above 32 or whose 128 attempts were all rejected is MALFORMED: r and e are zero; m is zero too, except after 128 rejections
// (the key is good there: m is the hash of the zero bytes).
struct RangeCommitArgs {
  const uint32_t* key;        // the seed as 8 little-endian words (device memory), or null: e is given
  const uint32_t* n; uint64_t n_stride;
  const uint8_t* e_in;        // [B][32] left aligned   (given)
  const uint8_t* e_len_in;    // [B]                    (given)
  uint32_t* r;                // [B][kw], 16-byte aligned   (seeded)
  uint32_t* m;                // [B][kw], 16-byte aligned; nullable
  uint8_t* e_out;             // [B][32]: e left aligned, zero behind it; nullable   (seeded)
  uint8_t* status;            // [B] 0 | ZKP_VERDICT_MALFORMED
  uint64_t first_index, batch;
  uint32_t kw, e_len, kind, max_attempts;
};

template <int G>
__global__ void __launch_bounds__(256) k_range_commit(RangeCommitArgs a) {
  static_assert(G == 2 || G == 4 || G == 8, "kw = 32, 64 or 128 words");
  constexpr uint64_t GM = (1ull << G) - 1;
  const uint64_t gid = blockIdx.x * 256ull + threadIdx.x, b = gid / G;
  const uint32_t l = (uint32_t)(gid % G);
  if (b >= a.batch) return;                                      // (whole groups leave together: 256 and 64 are multiples of G)
  const bool seeded = a.key != nullptr;
  const uint32_t* u = a.n + b * a.n_stride;
  uint32_t bits = 0;                                             // every lane of the group reads the same words
  for (int i = (int)a.kw - 1; i >= 0 && !bits; i--) {
    const uint32_t nv = u[i];
    if (nv) bits = 32u * (uint32_t)i + 32u - (uint32_t)__clz((int)nv);
  }
  const bool key_ok = bits > 256u && (u[0] & 1u) != 0;
  const uint32_t elen = seeded ? a.e_len : a.e_len_in[b];
  const uint32_t g0 = (threadIdx.x & 63u) - l;                   // the group's first bit in a ballot
  const uint64_t index = a.first_index + b;
  const uint32_t n0 = (uint32_t)index, n1 = (uint32_t)(index >> 32);
  uint32_t key[8], v[16];
#pragma unroll
  for (int i = 0; i < 16; i++) v[i] = 0u;
  bool ok = key_ok && elen <= 32u;
  if (seeded) {
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = a.key[i];
    bool active = ok;
    ok = false;
    if (active) {                                                // (a group is in or out as a whole)
      const uint32_t nw = (bits + 31) / 32, nb = (nw + 15) / 16;
      const uint32_t topmask = (bits & 31u) ? (1u << (bits & 31u)) - 1u : 0xffffffffu;
      const uint32_t n2 = nonce_word15(a.kind, 0u, 0u);
      uint32_t uw[16];
#pragma unroll
      for (int i = 0; i < 16; i++) { const uint32_t wi = 16 * l + i; uw[i] = wi < nw ? u[wi] : 0u; }
      for (uint32_t t = 0; t < a.max_attempts; t++) {
        int c = 0;
        if (active) {
          if (l < nb) {
            chacha20_block(key, t * nb + l, n0, n1, n2, v);
#pragma unroll
            for (int i = 0; i < 16; i++) { const uint32_t wi = 16 * l + i; if (wi >= nw) v[i] = 0u; else if (wi == nw - 1) v[i] &= topmask; }
          }
#pragma unroll
          for (int i = 15; i >= 0; i--) if (c == 0 && v[i] != uw[i]) c = v[i] < uw[i] ? -1 : 1;
        }
        const uint64_t ne = __ballot(active && c != 0), lt = __ballot(active && c < 0);
        if (active) {
          const uint32_t mm = (uint32_t)((ne >> g0) & GM);
          if (mm) ok = ((lt >> (g0 + (31u - (uint32_t)__clz((int)mm)))) & 1ull) != 0;     // the most significant lane that differs decides
          if (ok) active = false;
        }
        if (__ballot(active) == 0) break;
      }
    }
    uint4* o = (uint4*)(a.r + b * a.kw + 16 * l);
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = ok ? make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]) : make_uint4(0u, 0u, 0u, 0u);
  }
  uint4* om = a.m ? (uint4*)(a.m + b * a.kw + 16 * l) : nullptr;
  if (l != 0) {                                                  // m < 2^256: the words of lane 0
    if (om) for (int i = 0; i < 4; i++) om[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  a.status[b] = ok ? 0 : 2;
  // e as 8 little-endian words (byte k = bits 8 (k % 4) .. of word k / 4), zero from byte elen on
  uint32_t e[9];
#pragma unroll
  for (int j = 0; j < 9; j++) e[j] = 0u;
  if (ok && seeded) {
    uint32_t ks[16];
    chacha20_block(key, 0u, n0, n1, nonce_word15(a.kind, 0u, 1u), ks);
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = ks[j];
  } else if (ok) {
    const uint8_t* src = a.e_in + b * 32;
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = (uint32_t)src[4 * j] | ((uint32_t)src[4 * j + 1] << 8) | ((uint32_t)src[4 * j + 2] << 16) | ((uint32_t)src[4 * j + 3] << 24);
  }
  const uint32_t len = elen <= 32u ? elen : 0u;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t have = len > 4u * j ? len - 4u * j : 0u;      // bytes of word j that belong to e
    if (have < 4u) e[j] &= (1u << (8u * have)) - 1u;
  }
  if (a.e_out) {
    uint8_t* dst = a.e_out + b * 32;
#pragma unroll
    for (int j = 0; j < 8; j++) { dst[4 * j] = (uint8_t)e[j]; dst[4 * j + 1] = (uint8_t)(e[j] >> 8); dst[4 * j + 2] = (uint8_t)(e[j] >> 16); dst[4 * j + 3] = (uint8_t)(e[j] >> 24); }
  }
  if (!om) return;
  uint32_t h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = 0u;
  if (key_ok && elen <= 32u) {                                   // one padded block: e, 80, zeros, the bit count
#pragma unroll
    for (int j = 0; j < 9; j++) if (len / 4u == (uint32_t)j) e[j] |= 0x80u << (8u * (len & 3u));
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = j < 9 ? __builtin_bswap32(e[j]) : 0u;
    w[15] = 8u * len;
    Sha256 sh;
    sh.init(nullptr, 0);
    sh.compress_words(w);
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = sh.h[i];
  }
  om[0] = make_uint4(h[7], h[6], h[5], h[4]);
  om[1] = make_uint4(h[3], h[2], h[1], h[0]);
  om[2] = make_uint4(0u, 0u, 0u, 0u);
  om[3] = make_uint4(0u, 0u, 0u, 0u);
}

// verdict[b] = MALFORMED where the session was (zkp_range_verify_commit_batch: the Enc launch wrote 0 / 1 for every session)
__global__ void __launch_bounds__(256) k_range_commit_verdict(uint8_t* verdict, const uint8_t* status, uint64_t count) {
  const uint64_t b = blockIdx.x * 256ull + threadIdx.x;
  if (b < count && status[b]) verdict[b] = 2;
}

// non-zero words of a device region (zkp_diag_witness_residue)
__global__ void __launch_bounds__(256) k_count_nonzero(const uint32_t* p, uint64_t words, unsigned long long* out) {
  unsigned long long mine = 0;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256ull) mine += p[i] != 0u;
  if (mine) atomicAdd(out, mine);
}

// status[b] |= extra[b]
__global__ void __launch_bounds__(256) k_or_bytes(uint8_t* status, const uint8_t* extra, uint64_t count) {
  const uint64_t b = blockIdx.x * 256ull + threadIdx.x;
  if (b < count && extra[b]) status[b] |= extra[b];
}

}  // namespace zkp
