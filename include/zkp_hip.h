/*
 * zkp_hip.h — C ABI of libzkp_hip.so: MI355X (gfx950) batched Paillier ZK-proof engine.
 *
 * This is the drop-in boundary for the hot path of ZenGo-X/zk-paillier.  The reference has
 * no FFI of its own: its proof modules (L3) call the big-integer layer (L1: curv::BigInt
 * over GMP, kzen-paillier) through ordinary Rust calls.  Every entry point below replaces
 * one of those L3->L1 call shapes, batched; the reference call site each one replaces is
 * cited as file:line relative to the reference tree.  The Rust-side binding a maintainer
 * would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Big integers are fixed-width little-endian arrays of 32-bit limbs (limb 0 = least
 *    significant), zero padded.  kw = n_bits/32 limbs for values of the size of n
 *    (n, r, m, w, x, sigma, masked_r ...); 2*kw limbs for values mod n^2 (ciphertexts).
 *    n_bits / mod_bits is the kernel width: 2048, 4096 or 8192 bits for moduli
 *    (n^2 of a 2048-bit n is a 4096-bit modulus).  Moduli must be odd.
 *  - Batches are structure-of-arrays, element i at ptr + i*stride (stride in limbs).  A
 *    modulus/key stride of 0 means one shared modulus/key for the whole batch.
 *  - All pointers of one call live in the same memory space: host memory by default,
 *    device (HBM) memory of the context's GPU when ZKP_F_DEVICE_PTRS is set.  The caller
 *    owns every buffer; the library keeps no pointer after a call returns.
 *  - Every function returns a zkp_status.  Proof rejection is DATA (verdict byte 0), never
 *    an error code (mirrors Result<(), IncorrectProof>, src/zkproofs/errors.rs:5-13).
 *    Nothing aborts or throws across this boundary.
 *  - One ctx = one GPU + one HIP stream.  Calls on one ctx are serialised by the caller;
 *    different ctxs are independent (one per GPU / per rank) and may be driven from different
 *    host threads at the same time (zkp_multi_* does exactly that).
 *  - There is NO CPU fallback: if no gfx950 device is present zkp_ctx_create fails with
 *    ZKP_EDEVICE.
 */
#ifndef ZKP_HIP_H
#define ZKP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ZKP_OK = 0,
  ZKP_EINVAL = 1,        /* bad width / null pointer / count overflow */
  ZKP_ENONCANONICAL = 2, /* even modulus (Montgomery needs odd) */
  ZKP_EDEVICE = 3,       /* HIP error; text via zkp_last_error_string */
  ZKP_ENOMEM = 4
} zkp_status;

enum { ZKP_F_DEVICE_PTRS = 1u };

/* verdict bytes written by the *_verify_batch entry points */
enum {
  ZKP_VERDICT_REJECT = 0,    /* Err(IncorrectProof) */
  ZKP_VERDICT_ACCEPT = 1,    /* Ok(()) */
  ZKP_VERDICT_MALFORMED = 2  /* the reference would panic (index out of bounds / assert) */
};

/* response kinds (src/zkproofs/range_proof.rs:53-78, enum Response) */
enum { ZKP_RESP_OPEN = 0, ZKP_RESP_MASK = 1 };

#define ZKP_SECURITY_PARAMETER 128 /* src/zkproofs/range_proof_ni.rs:23 */
#define ZKP_CORRECT_KEY_M2 11      /* src/zkproofs/correct_key_ni.rs:29 */

typedef struct zkp_ctx zkp_ctx;

int32_t zkp_ctx_create(int32_t device_id, zkp_ctx** out_ctx);
/* The same, launching on a stream the caller owns (a hipStream_t, e.g. the framework's current stream); the ctx never
 * destroys it. */
int32_t zkp_ctx_create_on_stream(int32_t device_id, void* hip_stream, zkp_ctx** out_ctx);
int32_t zkp_ctx_destroy(zkp_ctx* ctx);
const char* zkp_backend_name(void);               /* "hip-gfx950" */
int32_t zkp_build_limbs_per_lane(void);           /* compile-time W of the throughput kernels (36): G = 144/W lanes per 4096-bit integer */

/* Two kernel geometries serve one ctx.  The throughput engine (libzkp_hip.so itself: W = 36 limbs per lane, 4 lanes per
 * 4096-bit integer) is the one the batch metric is quoted on.  A modular exponentiation is a chain of ~2400 dependent
 * products, so ONE proof (the reference's own bench, benches/all.rs:55-71) takes as long as ~30 of them there; the latency
 * engine (libzkp_hip_lat.so next to this library, the same sources built with W = 9: 16 lanes per integer) halves that time
 * and is chosen automatically while a call's work fits 3-5 wavefronts per SIMD of it.  Results are bit-identical.
 * zkp_ctx_set_geometry: limbs_per_lane 0 = automatic (default), 36 / 9 = always that engine (ZKP_EINVAL when it is not
 * loaded).  zkp_ctx_last_geometry: limbs per lane of the engine the most recent batch call ran on.
 * zkp_ctx_latency_limbs_per_lane: W of the loaded latency engine, 0 when there is none (small calls then run on the
 * throughput engine: slower, never wrong). */
int32_t zkp_ctx_set_geometry(zkp_ctx* ctx, int32_t limbs_per_lane);
int32_t zkp_ctx_last_geometry(zkp_ctx* ctx);
int32_t zkp_ctx_latency_limbs_per_lane(zkp_ctx* ctx);
const char* zkp_last_error_string(zkp_ctx* ctx);  /* valid until the next call on ctx */
void* zkp_ctx_stream(zkp_ctx* ctx);               /* the hipStream_t every call is ordered on (a small verify call forks part of
                                                     its work to an internal second stream and joins it back before it returns) */
int32_t zkp_ctx_synchronize(zkp_ctx* ctx);
/* Host-pointer calls stage their buffers through device blocks the ctx keeps between calls (no hipMalloc / hipFree per
 * call once warm).  This frees the cached blocks (zkp_ctx_destroy does so too). */
int32_t zkp_ctx_release_staging(zkp_ctx* ctx);

/* Kernel timing of the dominant (modexp) kernels, measured with HIP events on the ctx
 * stream.  zkp_timing_reset clears the accumulators and arms event recording;
 * zkp_timing_get synchronises and returns total milliseconds, launch count and the
 * number of modular exponentiations those launches performed. */
int32_t zkp_timing_reset(zkp_ctx* ctx, int32_t enable);
int32_t zkp_timing_get(zkp_ctx* ctx, double* out_ms, uint64_t* out_launches, uint64_t* out_modexps);
/* (Profiler calibration aids are NOT part of this boundary: include/zkp_hip_diag.h.) */

/* ------------------------------------------------------------------ L1 primitives
 * out[i] = base[i]^exp[i] mod mod[i].
 * Replaces BigInt::mod_pow (src/zkproofs/correct_key_ni.rs:92; wi_dlog_proof.rs:55,81,82).
 * mod_bits in {2048,4096,8192}; exp_bits a multiple of 32, 32..mod_bits.
 * base/out: mod_bits/32 limbs each; exp: exp_bits/32 limbs; *_stride in limbs, 0 = shared. */
int32_t zkp_modexp_batch(zkp_ctx* ctx, uint32_t mod_bits, uint32_t exp_bits, uint64_t count,
                         const uint32_t* base, const uint32_t* exp, uint64_t exp_stride,
                         const uint32_t* mod, uint64_t mod_stride, uint32_t* out, uint32_t flags);

/* out[i] = a[i]*b[i] mod mod[i].  Replaces BigInt::mod_mul (wi_dlog_proof.rs:83) and the
 * `x * y % m` forms at range_proof.rs:239,245,325,327. */
int32_t zkp_modmul_batch(zkp_ctx* ctx, uint32_t mod_bits, uint64_t count, const uint32_t* a,
                         const uint32_t* b, const uint32_t* mod, uint64_t mod_stride,
                         uint32_t* out, uint32_t flags);

/* c[i] = (1 + m[i]*n[i]) * r[i]^n[i] mod n[i]^2.
 * Replaces Paillier::encrypt_with_chosen_randomness (kzen-paillier 0.4.3; call sites
 * src/zkproofs/range_proof.rs:165-169,179-183,280-291,330-334,361).
 * n, m, r: n_bits/32 limbs; out_c: 2*n_bits/32 limbs.  n_bits in {1024,2048,4096}. */
int32_t zkp_paillier_enc_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t count, const uint32_t* n,
                               uint64_t n_stride, const uint32_t* m, const uint32_t* r,
                               uint32_t* out_c, uint32_t flags);

/* ok[i] = (Enc(m[i], r[i]) == expected[i])                       when mulc_a == mulc_b == NULL
 * ok[i] = (Enc(m[i], r[i]) == mulc_a[i] * mulc_b[i] mod n[i]^2)   when expected == NULL
 * Replaces CorrectOpening::verify_opening (src/zkproofs/correct_opening.rs:17-30) and the verifier's two equality
 * shapes: `expected_c1i != encrypted_pairs.c1[i]` (range_proof.rs:280-298: the stored value is compared as it is, so
 * an expected[i] >= n^2 never matches) and `c_j[i] * cipher_x % nn` vs Enc(masked_x, masked_r) (range_proof.rs:324-337:
 * the product is reduced, factors of any size up to 2*n_bits bits).  Exactly one of (expected) / (mulc_a, mulc_b)
 * is given.  expected, mulc_a, mulc_b: [count][2kw]; out_ok: [count] bytes 0 / 1.  An even n gives ok = 0. */
int32_t zkp_paillier_enc_check_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t count, const uint32_t* n,
                                     uint64_t n_stride, const uint32_t* m, const uint32_t* r,
                                     const uint32_t* mulc_a, const uint32_t* mulc_b, const uint32_t* expected,
                                     uint8_t* out_ok, uint32_t flags);

/* ------------------------------------------------------------------ RangeProofNi
 * Batch of B non-interactive range proofs, structure-of-arrays
 * (src/zkproofs/range_proof_ni.rs:36-44 RangeProofNi; range_proof.rs:32-81 EncryptedPairs,
 * Response, Proof).  EF = error_factor rows per proof. */
typedef struct {
  uint32_t n_bits;        /* width of n: 1024, 2048 or 4096 */
  uint32_t error_factor;  /* rows per proof; prove always writes ZKP_SECURITY_PARAMETER */
  uint64_t batch;         /* B */
  uint64_t n_stride;      /* kw, or 0 = every proof uses n[0] */
  const uint32_t* n;      /* [B or 1][kw]          ek.n                        */
  const uint32_t* range;  /* [B][kw]               q                           */
  const uint32_t* ciphertext; /* [B][2kw]          c = Enc(x, r)               */
  uint32_t* c1;           /* [B][EF][2kw]          encrypted_pairs.c1          */
  uint32_t* c2;           /* [B][EF][2kw]          encrypted_pairs.c2          */
  uint8_t* resp_kind;     /* [B][EF]               ZKP_RESP_OPEN | ZKP_RESP_MASK */
  uint8_t* resp_j;        /* [B][EF]               Mask.j (0 for Open)         */
  uint32_t* resp_w1;      /* [B][EF][kw]           Open.w1 | Mask.masked_x     */
  uint32_t* resp_r1;      /* [B][EF][kw]           Open.r1 | Mask.masked_r     */
  uint32_t* resp_w2;      /* [B][EF][kw]           Open.w2 | 0                 */
  uint32_t* resp_r2;      /* [B][EF][kw]           Open.r2 | 0                 */
} zkp_range_ni_proofs;

/* Secret prover inputs.  The reference draws (w1,w2,r1,r2) from the OS RNG inside
 * generate_encrypted_pairs (range_proof.rs:136-159); the boundary takes them as inputs
 * (already coin-flip swapped) so that proving is reproducible. */
typedef struct {
  const uint32_t* x;   /* [B][kw]      secret_x */
  const uint32_t* r;   /* [B][kw]      secret_r */
  const uint32_t* w1;  /* [B][EF][kw]  */
  const uint32_t* w2;  /* [B][EF][kw]  */
  const uint32_t* r1;  /* [B][EF][kw]  */
  const uint32_t* r2;  /* [B][EF][kw]  */
} zkp_range_ni_witness;

/* RangeProofNi::prove (src/zkproofs/range_proof_ni.rs:47-82) for B proofs:
 * generate_encrypted_pairs (range_proof.rs:161-187) -> Fiat-Shamir challenge
 * (range_proof_ni.rs:58-61, utils.rs:9-22) -> generate_proof (range_proof.rs:210-252).
 * Writes c1,c2,resp_* of `p`; out_e [B][32] receives the challenge bytes left-aligned,
 * out_e_len [B] their count (leading zero digest bytes are dropped, N2); either may be null.
 * out_status [B] (nullable): 0 ok, ZKP_VERDICT_MALFORMED if the reference would panic. */
int32_t zkp_range_ni_prove_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p,
                                 const zkp_range_ni_witness* w, uint8_t* out_e,
                                 uint8_t* out_e_len, uint8_t* out_status, uint32_t flags);

/* ---- seeded proving: RangeProofNi::prove with what the reference's prove takes.
 * The reference draws w1, w2, a coin, r1 and r2 per row itself (range_proof.rs:133-159).  Here a 32-byte seed is expanded ON THE DEVICE
 * into that witness, by a published, deterministic function of (seed, proof index, row) — DESIGN.md section 4 has the definition,
 * tests/seeded_model.py restates it — so sharded or chunked calls are identical to one call and the result can be checked bit for bit:
 *   ChaCha20 block function of RFC 8439 (20 rounds, 32-bit block counter in state word 12); key = seed as 8 little-endian words;
 *   nonce words (state 13, 14, 15) = (index & 0xffffffff, index >> 32, row << 2 | field), index = first_index + b for proof b of the
 *   call, row < error_factor <= 256, field 0 = w, 1 = r1, 2 = r2, 3 = coin.
 *   sample_below(u) for a field: bits = bit_length(u), nw = ceil(bits / 32), nb = ceil(nw / 16); attempt t = 0, 1, ... takes the first nw
 *   keystream words of blocks [t nb, (t + 1) nb) as limbs 0 .. nw - 1, clears the bits of the top limb above `bits`, and is accepted when
 *   the value is < u.  At most 128 attempts (each accepts with probability >= 1/2).
 *   Per row: third = floor(range / 3); a = third + sample_below(third) (field 0); coin = bit 0 of word 0 of block 0 of field 3;
 *   (w1, w2) = (a, a - third), swapped when coin = 1; r1 = sample_below(n) (field 1); r2 = sample_below(n) (field 2).
 * OUR rule for an empty interval — third == 0 (range < 3), likewise n == 0 — and for 128 rejected attempts in a row: that proof's witness is
 * all zero and its status is ZKP_VERDICT_MALFORMED; the other proofs of the batch are unaffected.  (The reference reaches curv's
 * BigInt::sample_below(0) there; what that does is recalled as a panic, not pinned by any vector of this repository.)
 *
 * SECURITY CONTRACT.  The seed is worth the whole witness: whoever learns it learns x from any Mask response.  A (seed, index) pair must
 * never be used for two different statements: under one key the commitments (c1, c2), and hence the challenge, repeat only if the
 * statement does, and two Mask responses over the same w give away x - x'.  Callers draw a fresh seed per call from the operating system
 * and wipe it afterwards.  `seed` is always a HOST pointer, also under ZKP_F_DEVICE_PTRS. */

/* the witness of rows [0, p->error_factor) of proofs first_index .. first_index + p->batch - 1, expanded from seed[32]; reads p->n, p->range.
 * Device-pointer calls: the four output arrays are 16-byte aligned. */
int32_t zkp_range_sample_witness_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, const uint8_t* seed, uint64_t first_index,
                                       uint32_t* out_w1, uint32_t* out_w2, uint32_t* out_r1, uint32_t* out_r2,   /* [B][EF][kw] */
                                       uint8_t* out_status /* [B], nullable */, uint32_t flags);
/* zkp_range_ni_prove_batch with that witness (ZKP_SECURITY_PARAMETER rows), which never leaves the device and is zeroed there — as are the
 * staged copies of x and r of a host-pointer call — before the call's blocks are given back, on error returns too.  out_status: the status
 * of zkp_range_ni_prove_batch, with the sampler's MALFORMED cases OR-ed in. */
int32_t zkp_range_ni_prove_seeded_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, const uint32_t* x, const uint32_t* r,
                                        const uint8_t* seed, uint64_t first_index,
                                        uint8_t* out_e, uint8_t* out_e_len, uint8_t* out_status, uint32_t flags);

/* RangeProofNi::verify_self / verify (range_proof_ni.rs:84-128 -> range_proof.rs:254-355).
 * out_verdict [B]: ZKP_VERDICT_*.  (verify()'s two assert_eq! on ek and ciphertext are the
 * host layer's job: here the statement is whatever `p` holds.) */
int32_t zkp_range_ni_verify_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p,
                                  uint8_t* out_verdict, uint32_t flags);

/* The three functions of the interactive RangeProof, usable on their own with any error_factor <= 256 and a
 * challenge supplied by the caller (the verifier's random bits of RangeProof::verifier_commit, range_proof.rs:118-126;
 * benches/all.rs:10-53 runs them with STATISTICAL_ERROR_FACTOR = 40).  e: [B][32] challenge bytes left aligned,
 * e_len: [B] byte counts (bit i of a challenge is bit 7-(i%8) of byte i/8, range_proof.rs:221,267).
 *   generate_encrypted_pairs (range_proof.rs:128-193): c1 = Enc(w1, r1), c2 = Enc(w2, r2), EF = p->error_factor rows
 *   generate_proof           (range_proof.rs:210-252): resp_* from the witness and e
 *   verifier_output          (range_proof.rs:254-355): verdicts from (c1, c2, resp_*, e) */
int32_t zkp_range_generate_encrypted_pairs_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w,
                                                 uint32_t flags);
/* The Fiat-Shamir challenge alone (utils::compute_digest, src/zkproofs/utils.rs:9-22, with the glue of
 * range_proof_ni.rs:58-61 / 89-92 / 110-113): out_e[b] = to_bytes(from_bytes(SHA256(to_bytes(n) || to_bytes(c1[0..EF)) ||
 * to_bytes(c2[0..EF))))), left aligned in 32 bytes, out_e_len[b] its length (leading zero bytes of the digest are dropped, a
 * zero digest is the one byte 00).  Reads p->n, p->c1, p->c2 only. */
int32_t zkp_range_challenge_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, uint8_t* out_e, uint8_t* out_e_len, uint32_t flags);
int32_t zkp_range_generate_proof_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w,
                                       const uint8_t* e, const uint8_t* e_len, uint8_t* out_status, uint32_t flags);
int32_t zkp_range_verifier_output_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, const uint8_t* e, const uint8_t* e_len,
                                        uint8_t* out_verdict, uint32_t flags);
/* The two prover steps from a seed: zkp_range_generate_encrypted_pairs_batch and zkp_range_generate_proof_batch with the witness of
 * zkp_range_sample_witness_batch at p->error_factor rows (1 .. 256; the stream above is unchanged, a row does not depend on the row count).
 * Step 1 reads p->n, p->range and writes p->c1, p->c2 only; step 2 reads p->n, p->range, x, r, e, e_len and writes p->resp_* only.  Step 2
 * regenerates exactly the witness step 1 committed to from the same (seed, first_index): the prover keeps 32 bytes between the two
 * messages, not 4 * EF * kw limbs per session.  The witness never leaves the device and is zeroed there — as are the staged seed and the
 * staged copies of x and r of a host-pointer call — before the call's blocks are given back, on error returns too.
 * out_status [B] (nullable): step 1, the sampler's ZKP_VERDICT_MALFORMED cases (range < 3, n == 0, 128 rejected attempts: that session's
 * witness is all zero, and its c1 / c2 rows are what the unseeded call writes for a zero witness); step 2, those OR-ed with the status of
 * zkp_range_generate_proof_batch (a challenge shorter than ceil(EF / 8) bytes is ZKP_VERDICT_MALFORMED).  `seed` is always a HOST pointer.
 * SECURITY CONTRACT, extended.  Besides "never one (seed, index) for two statements": a (seed, index) answers ONE challenge only.  Two
 * different challenges over the same commitments open some row both as Open (w1, w2) and as Mask (x + w), which reveals x.  The same holds
 * for a prover who keeps the witness itself; it is stated here because a seed makes answering again easy. */
int32_t zkp_range_generate_encrypted_pairs_seeded_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, const uint8_t* seed,
                                                        uint64_t first_index, uint8_t* out_status, uint32_t flags);
int32_t zkp_range_generate_proof_seeded_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, const uint32_t* x, const uint32_t* r,
                                              const uint8_t* seed, uint64_t first_index, const uint8_t* e, const uint8_t* e_len,
                                              uint8_t* out_status, uint32_t flags);
/* The verifier's commitment to its challenge, for whole batches of sessions: RangeProof::verifier_commit (range_proof.rs:118-126) draws the
 * challenge bits e and a randomness r and sends com = Enc(ek_v, m, r) with m = from_bytes(SHA256(e)); RangeProof::verify_commit
 * (range_proof.rs:195-208) is the prover's check of the revealed (r, e) against com before it trusts the challenge it answered.
 *   m: the 32 digest bytes read big-endian (result_bigint()).  It does not pass through to_bytes: a digest with leading zero bytes is simply
 *   a smaller integer.
 * The stream of (r, e), by the construction of zkp_nonce_sample_batch below (state word 15 = 0x80000000 | kind << 20 | slot << 4 | field) with
 * a kind of its own, ZKP_SEEDED_KIND_RANGE_COMMIT, slot 0 (tests/seeded_commit_model.py restates it):
 *   field 0 = r = sample_below(n), the rule above word for word, at most 128 attempts;
 *   field 1 = e = the first e_len bytes of keystream block 0: byte k is bits 8 (k % 4) .. 8 (k % 4) + 7 of word k / 4.  No rejection.
 *   e_len is 1 .. 32 in the seeded calls (5 = the reference's STATISTICAL_ERROR_FACTOR / 8); anything else is ZKP_EINVAL, no byte touched.
 * zkp_range_verifier_commit_seeded_batch expands (seed, first_index + b) on the device, hashes e into m and writes out_com[b] = Enc(m, r)
 * under n (n_stride 0: one key for the batch, or n_bits/32: one per session).  It writes out_com (and out_status) only; r, e and m never
 * leave the device.  zkp_range_verifier_reveal_seeded_batch regenerates exactly the (r, e) that call committed to, from the same
 * (n, e_len, seed, first_index), for the decommit message and for the verifier's own zkp_range_verifier_output_batch /
 * zkp_range_verifier_output_json_batch: out_r [B][kw], out_e [B][32] left aligned — all 32 bytes of a row are written, zero past e_len.
 * The verifier keeps 32 bytes between its messages.  In both calls the staged seed and every device copy of r, e and m (the staged copies
 * of out_r / out_e of a host-pointer call included) are zeroed on the device before the call's blocks are given back, on error returns too.
 * zkp_range_verify_commit_batch: out_verdict[b] = ZKP_VERDICT_ACCEPT iff com[b] == Enc(from_bytes(SHA256(e[b][0 .. e_len[b]))), r[b]) under
 * n, ZKP_VERDICT_REJECT otherwise.  The stored com is compared as it is, so a com >= n^2 never matches (the `expected` shape of
 * zkp_paillier_enc_check_batch, whose launch this is); e_len[b] is 0 .. 32, and zero bytes hash the empty string, as the reference would.
 * KEY DOMAIN.  That of zkp_paillier_enc_batch — n odd — and, OUR rule, bit_length(n) > 256: m < 2^256 must be a canonical plaintext, and a
 * Paillier key below 257 bits is no key.  A key outside the domain does not fail the call: the three calls return what the Enc call under
 * that key returns (ZKP_OK; zkp_paillier_enc_batch writes zeros under an even n), and the session is ZKP_VERDICT_MALFORMED — in out_status
 * of the seeded calls, with r, e and com all zero, and in out_verdict of zkp_range_verify_commit_batch, as is a session whose e_len[b] is
 * above 32.  The sampler's failures (n == 0, 128 rejected attempts) are ZKP_VERDICT_MALFORMED for that session too: its r and e are zero in
 * both seeded calls, its com is what a zero (r, e) gives, zero; the other sessions are unaffected.
 * `seed` is always a HOST pointer; ZKP_F_DEVICE_PTRS applies to the limb, byte and verdict arrays (a device out_r is 16-byte aligned).
 * n_bits in {1024, 2048, 4096}, batch 0 .. 2^24, out_status [B] nullable.
 * SECURITY CONTRACT.  A (seed, index) pair belongs to ONE session: the same pair under another key or in another session repeats (r, e).
 * The commitment hides e only while r is secret, and the seed is worth both.  Reveal AFTER the prover's encrypted pairs have arrived,
 * never before: a prover who knows e before it commits can answer without knowing x.  Draw the seed from the operating system, wipe it
 * after the reveal. */
#define ZKP_SEEDED_KIND_RANGE_COMMIT 7u
int32_t zkp_range_verifier_commit_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                               uint32_t e_len, const uint8_t* seed, uint64_t first_index,
                                               uint32_t* out_com /* [B][2kw] */, uint8_t* out_status /* [B], nullable */, uint32_t flags);
int32_t zkp_range_verifier_reveal_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                               uint32_t e_len, const uint8_t* seed, uint64_t first_index, uint32_t* out_r /* [B][kw] */,
                                               uint8_t* out_e /* [B][32] */, uint8_t* out_status /* [B], nullable */, uint32_t flags);
int32_t zkp_range_verify_commit_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                      const uint32_t* com /* [B][2kw] */, const uint32_t* r /* [B][kw] */, const uint8_t* e /* [B][32] */,
                                      const uint8_t* e_len /* [B] */, uint8_t* out_verdict /* [B] ZKP_VERDICT_* */, uint32_t flags);

/* ------------------------------------------------------------------ NiCorrectKeyProof
 * NiCorrectKeyProof::verify (src/zkproofs/correct_key_ni.rs:73-100) for B (key, proof)
 * pairs: rho_i from the SHA-256 MGF (:77-86,105-117), sigma_i^n mod n (:90-93),
 * gcd(primorial(6370), n) == 1 (:87-88).  n: [B][kw]; sigma: [B][11][kw]. */
int32_t zkp_correct_key_ni_verify_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch,
                                        const uint32_t* n, const uint32_t* sigma,
                                        const uint8_t* salt, uint32_t salt_len,
                                        uint8_t* out_verdict, uint32_t flags);

/* ------------------------------------------------------------------ CompositeDLogProof
 * src/zkproofs/wi_dlog_proof.rs:46-91.  N,g,ni,x: [B][kw]; y/r: [B][y_bits/32] (y_bits a
 * multiple of 32, >= 544 for honest proofs: y = r + e*s < 2^513); secret s: [B][8].
 * prove takes the 512-bit nonce r as an input (reference: BigInt::sample_below(2^512)). */
int32_t zkp_dlog_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint32_t y_bits, uint64_t batch,
                             const uint32_t* N, const uint32_t* g, const uint32_t* ni,
                             const uint32_t* secret, const uint32_t* r, uint32_t* out_x,
                             uint32_t* out_y, uint32_t flags);
int32_t zkp_dlog_verify_batch(zkp_ctx* ctx, uint32_t n_bits, uint32_t y_bits, uint64_t batch,
                              const uint32_t* N, const uint32_t* g, const uint32_t* ni,
                              const uint32_t* x, const uint32_t* y, uint8_t* out_verdict,
                              uint32_t flags);

/* ------------------------------------------------------------------ ZeroProof / CiphertextProof
 * (single-shot sigma proofs composed from the same kernels.)
 * ZeroProof (src/zkproofs/zero_enc_proof.rs:26-95): c = r^n mod n^2 encrypts zero.
 *   prove : a = Enc(0, r'), e = H(n || c || a), z = r' * r^e mod n^2           (:44-64)
 *   verify: Enc(0, z) == c^e * a mod n^2                                        (:66-94)
 * n: [B or 1][kw]; c, z, a: [B][2kw]; r, r_prime: [B][kw] (r' is sampled by the caller:
 * BigInt::sample_below(n), :45). */
int32_t zkp_zero_proof_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                   const uint32_t* c, const uint32_t* r, const uint32_t* r_prime, uint32_t* out_z,
                                   uint32_t* out_a, uint32_t flags);
int32_t zkp_zero_proof_verify_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                    const uint32_t* c, const uint32_t* z, const uint32_t* a, uint8_t* out_verdict,
                                    uint32_t flags);

/* CiphertextProof (src/zkproofs/correct_ciphertext.rs:23-98): knowledge of (x, r) with c = Enc(x, r).
 *   prove : c' = Enc(x', r'), e = H(n || c || c'), z1 = x' + x*e (over Z), z2 = r' * r^e mod n^2   (:42-64)
 *   verify: Enc(z1, z2) == c^e * c' mod n^2                                                          (:66-97)
 * x, r, x_prime, r_prime: [B][kw]; z1: [B][kw + ZKP_Z1_EXTRA_LIMBS] (x' + x*e < 2^(n_bits+257));
 * c, z2, c_prime: [B][2kw]. */
#define ZKP_Z1_EXTRA_LIMBS 16
int32_t zkp_ciphertext_proof_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                         const uint32_t* c, const uint32_t* x, const uint32_t* r, const uint32_t* x_prime,
                                         const uint32_t* r_prime, uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_c_prime,
                                         uint32_t flags);
int32_t zkp_ciphertext_proof_verify_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                          const uint32_t* c, const uint32_t* z1, const uint32_t* z2, const uint32_t* c_prime,
                                          uint8_t* out_verdict, uint32_t flags);

/* VerlinProof (src/zkproofs/verlin_proof.rs:35-165): phi_x = c^x * c'^x' * Enc(x'', r_x).
 *   gen_phi(c, c', y, y', y'', r_y) = c^y * c'^y' * Enc(y'', r_y) mod n^2                         (:138-165)
 *   prove : phi_a = gen_phi(c, c', a, a', a'', r_a); e = H(n || c || c' || phi_x || phi_a);
 *           z = x e + a, z' = x' e + a', z'' = x'' e + a'' (over Z); r_z = r_x^e * r_a mod n^2     (:60-99)
 *   verify: gen_phi(c, c', z, z', z'', r_z) == phi_x^e * phi_a mod n^2                             (:101-135)
 * c, c_prime, phi_x, phi_a, r_z: [B][2kw]; witness x, x_prime, x_double_prime, r_x and the nonces a, a_prime,
 * a_double_prime, r_a (sampled by the caller, :61-67): [B][kw]; z, z_prime, z_double_prime: [B][kw + ZKP_Z1_EXTRA_LIMBS]. */
int32_t zkp_verlin_proof_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                     const uint32_t* c, const uint32_t* c_prime, const uint32_t* phi_x,
                                     const uint32_t* x, const uint32_t* x_prime, const uint32_t* x_double_prime, const uint32_t* r_x,
                                     const uint32_t* a, const uint32_t* a_prime, const uint32_t* a_double_prime, const uint32_t* r_a,
                                     uint32_t* out_phi_a, uint32_t* out_z, uint32_t* out_z_prime, uint32_t* out_z_double_prime,
                                     uint32_t* out_r_z, uint32_t flags);
int32_t zkp_verlin_proof_verify_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                      const uint32_t* c, const uint32_t* c_prime, const uint32_t* phi_x, const uint32_t* phi_a,
                                      const uint32_t* z, const uint32_t* z_prime, const uint32_t* z_double_prime, const uint32_t* r_z,
                                      uint8_t* out_verdict, uint32_t flags);

/* ------------------------------------------------------------------ modular inverse (L1)
 * out[i] = a[i]^-1 mod M[i]: curv BigInt::mod_inv (GMP mpz_invert) as used by multiplication_proof.rs:95,133 and
 * correct_message.rs:53,76,141.  mod_bits in {2048, 4096, 8192}; a, M, out: mod_bits/32 words per element.
 * out_status[i]: 0 = out[i] holds the inverse, 1 = no inverse exists (mod_inv returns None; out[i] = 0),
 * 2 = outside the domain of this entry point (a >= M, M even or M < 3; out[i] = 0). */
#define ZKP_INV_OK 0
#define ZKP_INV_NONE 1
#define ZKP_INV_DOMAIN 2
int32_t zkp_modinv_batch(zkp_ctx* ctx, uint32_t mod_bits, uint64_t count, const uint32_t* a, const uint32_t* modulus, uint64_t mod_stride,
                         uint32_t* out, uint8_t* out_status, uint32_t flags);

/* ------------------------------------------------------------------ MulProof
 * multiplication_proof.rs:60-146.  kw = n_bits/32.  Statement: e_a, e_b, e_c [B][2kw].  Witness: a, b [B][kw] (c is not read
 * by the prover), r_a, r_b, r_c [B][kw].  Nonces the reference samples (:61-62), supplied by the caller: d, r_d [B][kw].
 * Proof: f [B][kw], z1, z2, e_d, e_db [B][2kw].
 * prove: out_status[b] = 0, or ZKP_VERDICT_MALFORMED where `mod_inv(..).unwrap()` (:95) panics in the reference.
 * verify: verdict bytes as above; MALFORMED where :133 panics. */
int32_t zkp_mul_proof_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a,
                                  const uint32_t* e_b, const uint32_t* e_c, const uint32_t* a, const uint32_t* b, const uint32_t* r_a,
                                  const uint32_t* r_b, const uint32_t* r_c, const uint32_t* d, const uint32_t* r_d, uint32_t* out_f,
                                  uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_e_d, uint32_t* out_e_db, uint8_t* out_status, uint32_t flags);
int32_t zkp_mul_proof_verify_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a,
                                   const uint32_t* e_b, const uint32_t* e_c, const uint32_t* f, const uint32_t* z1, const uint32_t* z2,
                                   const uint32_t* e_d, const uint32_t* e_db, uint8_t* out_verdict, uint32_t flags);

/* ------------------------------------------------------------------ CorrectMessageProof
 * correct_message.rs:35-162: ring proof that a ciphertext encrypts one of K valid messages (K = num_messages >= 1, the same for
 * every proof of the batch).  valid_messages [B][K][kw]; message [B][kw].  Values the reference samples, supplied by the caller:
 * r (:43), w (:65) [B][kw]; e_sim [B][K-1][8] (:59-61, 256-bit); z_sim [B][K-1][kw] (:62-64).
 * Proof: ciphertext [B][2kw], e_vec [B][K][8], z_vec [B][K][kw], a_vec [B][K][2kw].
 * prove: out_status[b] = MALFORMED where the reference panics (no valid message equals `message`: index out of bounds :74).
 * verify: MALFORMED where `assert_eq!(chal, ei_sum)` (:132) panics; REJECT / ACCEPT from :144-161. */
int32_t zkp_correct_message_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t num_messages, const uint32_t* n,
                                        uint64_t n_stride, const uint32_t* valid_messages, const uint32_t* message, const uint32_t* r,
                                        const uint32_t* e_sim, const uint32_t* z_sim, const uint32_t* w, uint32_t* out_ciphertext,
                                        uint32_t* out_e_vec, uint32_t* out_z_vec, uint32_t* out_a_vec, uint8_t* out_status, uint32_t flags);
int32_t zkp_correct_message_verify_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t num_messages, const uint32_t* n,
                                         uint64_t n_stride, const uint32_t* valid_messages, const uint32_t* ciphertext, const uint32_t* e_vec,
                                         const uint32_t* z_vec, const uint32_t* a_vec, uint8_t* out_verdict, uint32_t flags);

/* ------------------------------------------------------------------ seeded proving: ZeroProof, CiphertextProof, CorrectMessageProof, CompositeDLogProof
 * The four proves above take the nonces the reference draws itself (zero_enc_proof.rs:45, correct_ciphertext.rs:43-44,
 * correct_message.rs:42, 59-66, wi_dlog_proof.rs:53-54) as inputs.  The calls below take what the reference's prove takes: a 32-byte seed is
 * expanded ON THE DEVICE into those nonces, by the construction of the RangeProofNi stream above on streams of its own (DESIGN.md section 4
 * has the definition, tests/seeded_nonce_model.py restates it):
 *   ChaCha20 block function of RFC 8439 (20 rounds, 32-bit block counter in state word 12); key = seed as 8 little-endian words;
 *   state words 13, 14 = (index & 0xffffffff, index >> 32), index = first_index + b for proof b of the call;
 *   state word 15 = 0x80000000 | kind << 20 | slot << 4 | field, slot < 65536, field < 16.  Bit 31 separates these streams from every
 *   RangeProofNi stream, whose word 15 is row << 2 | field < 1024.
 *   sample_below(n) is the rule of the range sampler, word for word: bits = bit_length(n), nw = ceil(bits / 32), nb = ceil(nw / 16);
 *   attempt t takes the first nw keystream words of blocks [t nb, (t + 1) nb) as limbs 0 .. nw - 1, clears the bits of the top limb above
 *   `bits`, and is accepted when the value is < n; at most 128 attempts.
 *     kind                 slot                   field  value      draw
 *     1 Zero               0                      0      r_prime    sample_below(n)
 *     2 Ciphertext         0                      0      x_prime    sample_below(n)
 *     2 Ciphertext         0                      1      r_prime    sample_below(n)
 *     3 CorrectMessage     0                      0      r          sample_below(n)
 *     3 CorrectMessage     0                      1      w          sample_below(n)
 *     3 CorrectMessage     j + 1, j < K - 1       2      e_sim[j]   words 0 .. 7 of block 0, no rejection (BigInt::sample(256))
 *     3 CorrectMessage     j + 1, j < K - 1       3      z_sim[j]   sample_below(n)
 *     4 DLog               0                      0      r          words 0 .. 15 of block 0: uniform on [0, 2^512), as sample_below(2^512) is
 * OUR rule for n == 0 and for 128 rejected attempts in a row is the range sampler's: all of that proof's nonces are zero and its status
 * is ZKP_VERDICT_MALFORMED; its outputs are what the nonce-input call writes for zero nonces; the other proofs of the batch are unaffected.
 * VerlinProof and MulProof redraw a nonce until it is coprime to n (verlin_proof.rs:64-67, multiplication_proof.rs:148-154): a GCD loop and
 * not a plain draw.  Their seeded proves, kinds 5 and 6 of the same construction, follow below this section's entry points.
 *
 * SECURITY CONTRACT.  The seed is worth every nonce of the call: whoever learns it learns the witness from any response (r from
 * z = r' r^e, x from z1 = x' + x e, the DLog secret from y = r + e s).  A (seed, index) pair must never be used for two different
 * statements: two responses over one r_prime under two challenges give away r.  Callers draw a fresh seed per call from the operating
 * system and wipe it afterwards.  `seed` is always a HOST pointer, also under ZKP_F_DEVICE_PTRS.  A caller who splits a batch passes
 * first_index + lo for the part that starts at proof lo: split calls equal one call. */
#define ZKP_SEEDED_KIND_ZERO 1u
#define ZKP_SEEDED_KIND_CIPHERTEXT 2u
#define ZKP_SEEDED_KIND_CORRECT_MESSAGE 3u
#define ZKP_SEEDED_KIND_DLOG 4u

/* The nonces of proofs first_index .. first_index + batch - 1 of one kind, by field id: out_field is an array of four pointers (read, not
 * written), out_field[f] is null where the kind has no field f
 * (and may be null where it has no slots: e_sim, z_sim at num_messages == 1).  Shapes: [B][kw] for the slot-0 fields, [B][K-1][8] for
 * e_sim, [B][K-1][kw] for z_sim, [B][16] for the DLog r.  num_messages = K is read for CorrectMessage only (1 <= K <= 65536); n and n_stride
 * are not read for DLog.  out_status [B], nullable.  Device-pointer calls: the output arrays are 16-byte aligned. */
int32_t zkp_nonce_sample_batch(zkp_ctx* ctx, uint32_t proof_kind, uint32_t n_bits, uint64_t batch, uint32_t num_messages, const uint32_t* n,
                               uint64_t n_stride, const uint8_t* seed, uint64_t first_index, uint32_t** out_field /* [4], by field id */,
                               uint8_t* out_status, uint32_t flags);

/* The nonce-input proves with their nonce pointers replaced by (seed, first_index): the nonces are sampled into blocks of the context,
 * the nonce-input call runs on them unchanged, and they are zeroed on the device — as are the seed and the staged copies of r / x / message /
 * secret of a host-pointer call — before the call's blocks are given back, on error returns too.  out_status [B], nullable for Zero,
 * Ciphertext and DLog: the sampler's status (for CorrectMessage: the prove's status with the sampler's OR-ed in).  A seeded CorrectMessage
 * call accepts the num_messages zkp_correct_message_prove_batch accepts; beyond 65536 the stream itself has no slots. */
int32_t zkp_zero_proof_prove_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                          const uint32_t* c, const uint32_t* r, const uint8_t* seed, uint64_t first_index, uint32_t* out_z,
                                          uint32_t* out_a, uint8_t* out_status, uint32_t flags);
int32_t zkp_ciphertext_proof_prove_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                                const uint32_t* c, const uint32_t* x, const uint32_t* r, const uint8_t* seed,
                                                uint64_t first_index, uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_c_prime,
                                                uint8_t* out_status, uint32_t flags);
int32_t zkp_correct_message_prove_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t num_messages, const uint32_t* n,
                                               uint64_t n_stride, const uint32_t* valid_messages, const uint32_t* message, const uint8_t* seed,
                                               uint64_t first_index, uint32_t* out_ciphertext, uint32_t* out_e_vec, uint32_t* out_z_vec,
                                               uint32_t* out_a_vec, uint8_t* out_status, uint32_t flags);
int32_t zkp_dlog_prove_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* N, const uint32_t* g,
                                    const uint32_t* ni, const uint32_t* secret, const uint8_t* seed, uint64_t first_index, uint32_t* out_x,
                                    uint32_t* out_y, uint8_t* out_status, uint32_t flags);

/* ------------------------------------------------------------------ seeded proving: VerlinProof, MulProof (nonces coprime to n)
 * VerlinProof::prove redraws r_a until gcd(r_a, n) == 1 (verlin_proof.rs:61-67), MulProof::prove does the same for r_d
 * (multiplication_proof.rs:61-62, sample_paillier_random :148-154).  The construction is that of the nonce streams above, unchanged: the
 * ChaCha20 block function of RFC 8439, key = the seed as 8 little-endian words, state words 13, 14 = (index & 0xffffffff, index >> 32),
 * state word 15 = 0x80000000 | kind << 20 | slot << 4 | field, with two more kinds:
 *     kind                 slot                   field  value            draw
 *     5 Verlin             0                      0      a                sample_below(n)
 *     5 Verlin             0                      1      a_prime          sample_below(n)
 *     5 Verlin             0                      2      a_double_prime   sample_below(n)
 *     5 Verlin             0                      3      r_a              sample_coprime_below(n)
 *     6 Mul                0                      0      d                sample_below(n)
 *     6 Mul                0                      1      r_d              sample_coprime_below(n)
 * sample_coprime_below(n): attempts t = 0, 1, ... produce exactly the candidates of sample_below(n) — the nw first words of blocks
 * [t nb, (t + 1) nb), the top limb masked to bit_length(n); candidate t is accepted when it is < n AND gcd(candidate, n) == 1; at most 128
 * attempts in all, rejections of both sorts share the one counter t.  Candidate 0 is rejected by the gcd test unless n == 1.
 * OUR rule for n == 0, for an even n (outside the limb kernels' domain, as it is for the sigma documents) and for 128 rejected attempts in a
 * row in any field of the proof: every nonce of that proof is zero and its status is ZKP_VERDICT_MALFORMED; its outputs are what the
 * nonce-input call writes for zero nonces; the other proofs of the batch are unaffected.  Chunked calls with first_index + lo equal one call.
 * The SECURITY CONTRACT above holds word for word: `seed` is always a HOST pointer, fresh per call, never reused for another statement. */
#define ZKP_SEEDED_KIND_VERLIN 5u
#define ZKP_SEEDED_KIND_MUL 6u

/* The nonces of proofs first_index .. first_index + batch - 1 of kind 5 or 6 (every other kind: ZKP_EINVAL — zkp_nonce_sample_batch keeps
 * kinds 1 .. 4), by field id: out_field is an array of four pointers (read, not written), each [B][kw]; entries 2 and 3 are not read
 * for Mul.  out_status [B], nullable.  Device-pointer calls: the output arrays are 16-byte aligned. */
int32_t zkp_nonce_sample_coprime_batch(zkp_ctx* ctx, uint32_t proof_kind, uint32_t n_bits, uint64_t batch, const uint32_t* n,
                                       uint64_t n_stride, const uint8_t* seed, uint64_t first_index, uint32_t** out_field /* [4], by field id */,
                                       uint8_t* out_status, uint32_t flags);

/* zkp_verlin_proof_prove_batch and zkp_mul_proof_prove_batch with their nonce pointers replaced by (seed, first_index): the nonces are
 * sampled into blocks of the context, the nonce-input call runs on them unchanged, and they are zeroed on the device — as are the seed
 * and the staged copies of the witness of a host-pointer call — before the call's blocks are given back, on error returns too.
 * Verlin: out_status [B], nullable, is the sampler's status.  Mul: out_status [B] is the prove's status with the sampler's OR-ed in. */
int32_t zkp_verlin_proof_prove_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                            const uint32_t* c, const uint32_t* c_prime, const uint32_t* phi_x, const uint32_t* x,
                                            const uint32_t* x_prime, const uint32_t* x_double_prime, const uint32_t* r_x, const uint8_t* seed,
                                            uint64_t first_index, uint32_t* out_phi_a, uint32_t* out_z, uint32_t* out_z_prime,
                                            uint32_t* out_z_double_prime, uint32_t* out_r_z, uint8_t* out_status, uint32_t flags);
int32_t zkp_mul_proof_prove_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                         const uint32_t* e_a, const uint32_t* e_b, const uint32_t* e_c, const uint32_t* a, const uint32_t* b,
                                         const uint32_t* r_a, const uint32_t* r_b, const uint32_t* r_c, const uint8_t* seed,
                                         uint64_t first_index, uint32_t* out_f, uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_e_d,
                                         uint32_t* out_e_db, uint8_t* out_status, uint32_t flags);

/* ------------------------------------------------------------------ Jacobi symbol, legendre_symbol, DLogStatement set-up
 * zkp_jacobi_batch: out_symbol[i] = (a[i] / n[i]), the Jacobi symbol, -1 | 0 | 1 (an int32_t: the i32 the reference's legendre_symbol returns), for odd n.  It needs neither the factors of n nor an
 * exponentiation: a binary-GCD-shaped loop, one pair per lane (csrc/kernels_jacobi.hpp states why every step is exact).
 * mod_bits in {1024, 2048, 4096, 8192}; a, n: mod_bits/32 words per element; n_stride = 0 (one n for the call) or mod_bits/32.  a is any
 * value: zero and a >= n are in the domain.  n == 1 gives 1.  out_status[i] (nullable): 0, or 2 where n is even or zero (outside the
 * domain, as zkp_modinv_batch reports its own; the symbol is 0).
 *
 * zkp_legendre_batch: the reference's `pub fn legendre_symbol(a, p)` (wi_dlog_proof.rs:94-107), word for word:
 * ls = a^((p - 1) * 2^-1 mod p) mod p; out_symbol[i] = 1 if ls == 1, else -1.  It is Euler's criterion and not the Jacobi symbol:
 * a == 0 mod p and a composite p give -1 as they do there.  mod_bits in {2048, 4096, 8192} (what zkp_modexp_batch takes: a 1024-bit
 * prime travels zero-padded in a 2048-bit row); p_stride = 0 or mod_bits/32.  out_status[i] (nullable): 0, or ZKP_VERDICT_MALFORMED (2)
 * where the reference panics (p even: `mod_inv(2, p).unwrap()`), and 2 also for p < 3 and a >= p (OUR domain rule, that of
 * zkp_modinv_batch); the symbol of such an item is 0. */
int32_t zkp_jacobi_batch(zkp_ctx* ctx, uint32_t mod_bits, uint64_t count, const uint32_t* a, const uint32_t* n, uint64_t n_stride,
                         int32_t* out_symbol, uint8_t* out_status, uint32_t flags);
int32_t zkp_legendre_batch(zkp_ctx* ctx, uint32_t mod_bits, uint64_t count, const uint32_t* a, const uint32_t* p, uint64_t p_stride,
                           int32_t* out_symbol, uint8_t* out_status, uint32_t flags);

/* The set-up of a DLogStatement "per definition 3 in the paper", as the reference's own tests do it before CompositeDLogProof::prove
 * (wi_dlog_proof.rs:117-141): h1 drawn until its symbol is -1, secret < 2^256, h2 = (h1^-1)^secret mod N — the ring-Pedersen parameters
 * N~, h1, h2 of the threshold-ECDSA protocols.  From a 32-byte seed, by the construction of the nonce streams above, unchanged, with one
 * more kind:
 *     kind                 slot                   field  value      draw
 *     8 DLogSetup          0                      0      h1         sample_jacobi_minus_below(N)
 *     8 DLogSetup          0                      1      secret     words 0 .. 7 of block 0: uniform on [0, 2^256), as sample_below(2^256) is
 * sample_jacobi_minus_below(N): attempts t = 0, 1, ... produce exactly the candidates of sample_below(N) — the same blocks, the same
 * top-limb mask; candidate v is accepted when v + 1 < N (the reference's sample_range(1, N - 1) draws below N - 1; v = 0 and v = 1 fall to
 * the symbol test) AND the Jacobi symbol (v / N) == -1; at most 128 attempts, rejections of both sorts share the one counter t.
 * Where this is STRICTER than the reference: it tests legendre(h1, p) * legendre(h1, q) with its legendre_symbol, which is -1 for
 * h1 == 0 mod p, so it can accept an h1 that shares a factor with N — and then panics in mod_inv.  The Jacobi symbol is 0 there and the
 * candidate is redrawn: every h1 made here is invertible.  p and q are not needed.
 * out_g = h1, out_ni = h2 [B][kw], out_secret [B][8], kw = n_bits/32; n_bits is what zkp_dlog_prove_batch accepts.  N zero, N even and 128
 * rejections in a row (CERTAIN for a square N, whose symbols are all 0 or 1) make that statement ZKP_VERDICT_MALFORMED in out_status
 * [B] (nullable): its g, ni and secret are zero; the other statements are unaffected.  Chunked calls with first_index + lo equal one call.
 * The staged seed, the device copies of secret and h1^-1 and the staged out_secret of a host-pointer call are zeroed on the device before
 * the call's blocks are given back, on error returns too.
 * SECURITY CONTRACT, extended.  The seed is worth the secret: whoever learns it computes the discrete logarithm this statement exists to
 * hide.  One (seed, index) pair serves ONE statement.  `seed` is always a HOST pointer, fresh from the operating system, wiped by the
 * caller afterwards.  A seed used here must not also be handed to zkp_dlog_prove_seeded_batch: the streams of kind 8 and kind 4 are
 * disjoint by construction (state word 15), but one seed for the secret and for the nonce that masks it makes either leak fatal to
 * both. */
#define ZKP_SEEDED_KIND_DLOG_SETUP 8u
int32_t zkp_dlog_statement_setup_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* N, const uint8_t* seed,
                                              uint64_t first_index, uint32_t* out_g, uint32_t* out_ni, uint32_t* out_secret,
                                              uint8_t* out_status, uint32_t flags);

/* ------------------------------------------------------------------ Paillier decrypt and open with the factors (CRT)
 * zkp_paillier_open_batch: for a key (p, q), n = p q, and a ciphertext c — ANY value below 2^(2 n_bits), c >= n^2 included —
 *     x_p = (c mod p^2)^(p-1) mod p^2     L_p = (x_p - 1) / p     m_p = L_p h_p mod p      m = m_p + p ((m_q - m_p) pinv mod q)
 *     r_p = (c mod p)^(d_p) mod p                                                          r = r_p + p ((r_q - r_p) pinv mod q)
 * (q alike) with the per-key constants h_p = (p - (q mod p))^-1 mod p, pinv = p^-1 mod q, d_p = q^-1 mod (p - 1).  out_m is what
 * Paillier::decrypt returns and (out_m, out_r) what Paillier::open returns (the call `correct_opening.rs:48-56` makes before
 * verify_opening; the n-th root `extract_nroot` takes, correct_key_ni.rs:68): for c = Enc(m0, r0) with r0 coprime to n they are m0 and r0.
 * n_bits in {1024, 2048, 4096}; p, q: hw = n_bits/64 words each, key_stride = 0 (one key for the call) or hw (one key per item);
 * c [count][2 kw], out_m, out_r [count][kw], kw = n_bits/32, count <= 2^24.  out_r == NULL: decrypt only, the two root exponentiations are not run.
 * The exponentiations are zkp_modexp_batch's ladder at mod_bits = max(n_bits, 2048) with n_bits/2-bit exponents — 2 rows per item, 4
 * with out_r — and a call goes, whole, to the engine that call would go to for the same (rows, mod_bits); the rest is
 * csrc/kernels_paillier_dec.hpp.
 * DOMAIN (rules of THIS library; the reference has no error here and returns a number that means nothing).  out_status[i] (nullable) is
 * 0, or ZKP_VERDICT_MALFORMED (2) — then out_m and out_r of item i are zero, and the other items are unaffected.  A KEY is bad when p or
 * q is even or below 3, or when one of the inverses above does not exist: gcd(p, q), gcd(q, p - 1) or gcd(p, q - 1) != 1, together
 * gcd(n, phi(n)) != 1.  No primality test is made: the formulas are applied to the key the caller gave.  An ITEM is bad when its key is,
 * or when x_p != 1 mod p or x_q != 1 mod q — for prime factors: c shares a factor with n, c = 0 included.
 * SECURITY CONTRACT.  For the length of the call, p and q, the constants derived from them, the exponents p - 1, q - 1, d_p, d_q, the
 * residues and ladder results, the ladder's per-row constants (which hold the moduli p^2, q^2, p, q) and window tables, and the recovered
 * m and r of a host-pointer call live in device blocks of the context that runs the call.  Every one of those
 * blocks is zeroed on the stream before the call's blocks are given back, on error returns too; zkp_diag_witness_residue then reads 0.
 * With ZKP_F_DEVICE_PTRS p, q, out_m and out_r are the caller's to wipe.  The secret exponents go through the ladder that every other
 * exponentiation of this library uses (NiCorrectKeyProof's n^-1 mod phi among them); nothing is claimed about its timing behaviour, nor
 * about that of the division and reduction kernels around it. */
int32_t zkp_paillier_open_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t count, const uint32_t* p, const uint32_t* q, uint64_t key_stride,
                                const uint32_t* c, uint32_t* out_m, uint32_t* out_r /* nullable: decrypt only */,
                                uint8_t* out_status /* nullable */, uint32_t flags);

/* ------------------------------------------------------------------ NiCorrectKeyProof::proof for whole batches of keys (CRT n-th roots)
 * zkp_correct_key_ni_prove_batch: for key b = (p, q) (correct_key_ni.rs:42-71; one key per proof — a proof is about its key)
 *     n = p q      rho_i = mask_generation(bit_length(n), H(n, H(salt), i)) mod n,  i = 0..10      sigma_i = rho_i^(n^-1 mod phi(n)) mod n
 * with sigma_i computed as upstream's extract_nroot does:
 *     s_p = (rho_i mod p)^(d_p) mod p,  s_q alike      sigma_i = s_p + p ((s_q - s_p) pinv mod q)
 * d_p = q^-1 mod (p - 1) (= n^-1 mod (p - 1)), d_q = p^-1 mod (q - 1), pinv = p^-1 mod q.  bit_length(n) is the key's own, not n_bits.
 * n_bits in {1024, 2048, 4096}; p, q [batch][hw], hw = n_bits/64; salt: HOST bytes in both memory modes, as in verify; out_n [batch][kw]
 * (nullable), out_sigma [batch][11][kw], kw = n_bits/32; batch <= 2^24, batch == 0 is ZKP_OK.  ZKP_EINVAL: a null ctx, p, q or out_sigma,
 * another n_bits, salt_len without salt, a flag bit other than ZKP_F_DEVICE_PTRS.  (out_n, out_sigma) are what
 * zkp_correct_key_ni_verify_batch and zkp_json_write_correct_key_proof_batch take.
 * The exponentiations are zkp_modexp_batch's ladder at mod_bits = 2048 (= max(n_bits/2, 2048): the narrowest group) with n_bits/2-bit
 * exponents, 22 rows per key, and a call goes, whole, to the engine that call would go to for the same (rows, mod_bits); rho comes from
 * the verifier's hash kernels over the device-resident n; the rest is csrc/kernels_ck_prove.hpp and the key kernels of
 * csrc/kernels_paillier_dec.hpp.
 * DOMAIN (rules of THIS library, those of zkp_paillier_open_batch; the reference's `mod_inv(..).unwrap()` panics on such a key).
 * out_status[b] (nullable) is 0, or ZKP_VERDICT_MALFORMED (2) — then out_sigma[b] and out_n[b] are zero, and the other keys are
 * unaffected.  A key is bad when p or q is even or below 3, or when gcd(p, q), gcd(q, p - 1) or gcd(p, q - 1) != 1.  No primality test is
 * made: the formulas are applied to the key the caller gave, and for prime p and q their value is rho_i^(n^-1 mod phi(n)) mod n.  There is
 * no per-root status: a rho_i that shares a factor with n has the value the formulas give (for prime factors still rho_i^d mod n).
 * SECURITY CONTRACT.  For the length of the call, p and q, the constants derived from them (d_p, d_q, pinv), the residues rho mod p and
 * rho mod q and the ladder's results, the ladder's per-row constants (which hold the moduli p, q) and window tables live in device blocks
 * of the context that runs the call.  Every one of those blocks is zeroed on the stream before the call's blocks are given back, on error
 * returns too; zkp_diag_witness_residue then reads 0.  rho, n and sigma are public.  With ZKP_F_DEVICE_PTRS the caller's p and q are the
 * caller's to wipe.  The secret exponents go through the ladder that every other exponentiation of this library uses; nothing is claimed
 * about its timing behaviour, nor about that of the division and reduction kernels around it. */
int32_t zkp_correct_key_ni_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* p, const uint32_t* q,
                                       const uint8_t* salt, uint32_t salt_len, uint32_t* out_n /* nullable */, uint32_t* out_sigma,
                                       uint8_t* out_status /* nullable */, uint32_t flags);

/* ------------------------------------------------------------------ interactive CorrectKey for whole batches of sessions
 * CorrectKey::challenge / prove / verify (src/zkproofs/correct_key.rs:64-171).  A session has K rounds (`rounds`, 1 .. 256; the reference's
 * STATISTICAL_ERROR_FACTOR is ZKP_CORRECT_KEY_ROUNDS), the same for every session of a call.  kw = n_bits/32, hw = n_bits/64, n_bits in
 * {1024, 2048, 4096}; batch * K <= 2^24, batch == 0 is ZKP_OK.  Digests (e, s_digest) are 8 little-endian words: the number
 * compute_digest returns (utils.rs:9-22).  ZKP_EINVAL, no byte touched: a null ctx, another n_bits, K outside 1 .. 256, batch * K above
 * 2^24, an n_stride other than 0 or kw, a null required pointer, a flag bit other than ZKP_F_DEVICE_PTRS.
 *
 * zkp_correct_key_challenge_batch (correct_key.rs:64-102 with the s_i, r_i the reference draws at :67-70, :80-83 as inputs): for session b
 * under n (n_stride 0: one key for the batch, or kw: one per session) and round i
 *     sn_i = s_i^n mod n     rn_i = r_i^n mod n     e = compute_digest(n, sn.., rn..)     z_i = r_i s_i^e mod n     s_digest = compute_digest(s..)
 * s, r [B][K][kw] are taken as given, any kw-word value (mod_pow reduces its base; s_digest hashes s as given).  out_sn, out_z [B][K][kw],
 * out_e [B][8]: the Challenge; out_s_digest [B][8] (nullable): the VerificationAid.  The exponentiations are zkp_modexp_batch's ladder at
 * mod_bits = max(n_bits, 2048): 2 K B rows with the n_bits-bit exponent n and K B rows with the 256-bit exponent e, under one shared
 * modulus (n_stride 0) or per-row moduli; the call goes, whole, to the engine zkp_modexp_batch would choose for the larger launch.
 * DOMAIN (rule of THIS library).  out_status[b] (nullable) is 0, or ZKP_VERDICT_MALFORMED (2) for an n that is even (zero included) or 1:
 * every output of that session is zero, the other sessions are unaffected.
 *
 * zkp_correct_key_challenge_seeded_batch: what the reference's challenge takes.  s and r are expanded ON THE DEVICE from a 32-byte seed by
 * the construction of the nonce streams above, unchanged (state words 13, 14 = index = first_index + b; word 15 = 0x80000000 | kind << 20 |
 * slot << 4 | field), with one more kind (tests/ck_inter_model.py restates it):
 *     kind                 slot                   field  value      draw
 *     10 CorrectKey        i, i < K               0      s_i        sample_below(n)
 *     10 CorrectKey        i, i < K               1      r_i        sample_below(n)
 * sample_below is the rule above word for word, at most 128 attempts; a round does not depend on K.  A sampler failure (n == 0, 128
 * rejected attempts) makes the session ZKP_VERDICT_MALFORMED with zero outputs, as a key outside the domain does.  A call split with
 * first_index + lo equals the one call.  zkp_nonce_sample_batch does not serve this kind.
 *
 * zkp_correct_key_verify_seeded_batch (correct_key.rs:164-171 without a stored aid): regenerates s of (seed, first_index + b) under n,
 * hashes it and compares with proof_s_digest[b].  out_verdict[b]: ZKP_VERDICT_ACCEPT, ZKP_VERDICT_REJECT, or ZKP_VERDICT_MALFORMED where
 * the seeded challenge is.  The sampler and the hash only: no ladder, the call runs on the context that receives it.  The aid never leaves
 * the device: the verifier keeps 32 bytes between its messages.
 *
 * SECURITY CONTRACT of the three.  s and s_digest are the verifier's secret until the proof has arrived: a prover who learns either answers
 * without the key.  The seed is worth both.  A (seed, index) pair belongs to ONE session: under another key it repeats s and r.  Draw the
 * seed from the operating system and wipe it after the verify.  `seed` is a HOST pointer in both memory modes.  The staged seed, every
 * device copy of s and r (those reduced under n included), s^e, the regenerated digest and the staged out_s_digest of a host-pointer call
 * are zeroed on the stream before the call's blocks are given back, on error returns too; zkp_diag_witness_residue then reads 0.  With
 * ZKP_F_DEVICE_PTRS the caller's s, r and out_s_digest are the caller's to wipe.
 *
 * zkp_correct_key_prove_batch (correct_key.rs:104-162): for key b = (p, q) [B][hw] and the challenge (sn [B][K][kw], e [B][8], z [B][K][kw])
 *     n = p q
 *     rn_i mod p = (z_i mod p)^(n mod (p-1)) (sn_i mod p)^((p-1) - e mod (p-1)) mod p     (q alike)      rn_i = CRT(rn_p, rn_q)
 *     root_i     = CRT((sn_i mod p)^(d_p) mod p, (sn_i mod q)^(d_q) mod q)                d_p = q^-1 mod (p-1)   (upstream's extract_nroot)
 *     out_s_digest[b] = compute_digest(root..)
 * six rows per round of zkp_modexp_batch's ladder at mod_bits = 2048 (= max(n_bits/2, 2048)) with n_bits/2-bit exponents, and the call
 * goes, whole, to the engine that call would go to for the same (6 K B rows, mod_bits).  phi, phi - e mod phi and n^-1 mod phi are never
 * formed; the rest is csrc/kernels_ck_inter.hpp and the key kernels of csrc/kernels_paillier_dec.hpp.  sn and z are any kw-word values.
 * out_error[b] (nullable): 0, or the reference's first error in its order — the variants of CorrectKeyProveError in declaration order,
 * ZKP_CK_PROVE_* 1 .. 4 — or ZKP_CK_PROVE_BAD_KEY (5, rule of THIS library: the key domain of zkp_paillier_open_batch, tested first).  On
 * any non-zero code out_s_digest[b] is zero; the other sessions are unaffected.  No primality test is made: for prime p and q the values are
 * the reference's, for other factors they are what the formulas above give.
 * SECURITY CONTRACT: that of zkp_correct_key_ni_prove_batch.  In addition the residues of sn and z, the three exponent pairs, the ladder's
 * rows, constants records and window tables and the roots are registered secret and zeroed before the call's blocks are given back, on
 * error returns too.  n, rn, the error codes and the digest are public. */
#define ZKP_CORRECT_KEY_ROUNDS 40 /* src/zkproofs/correct_key.rs:26 */
#define ZKP_SEEDED_KIND_CORRECT_KEY 10u
#define ZKP_CK_PROVE_OK 0
#define ZKP_CK_PROVE_SN_NOT_COPRIME 1 /* SniNotCoprimeWithN */
#define ZKP_CK_PROVE_Z_NOT_COPRIME 2  /* ZiNotCoprimeWithN */
#define ZKP_CK_PROVE_RN_NOT_COPRIME 3 /* RniNotCoprimeWithN */
#define ZKP_CK_PROVE_E_MISMATCH 4     /* EWasntComputedCorrectly */
#define ZKP_CK_PROVE_BAD_KEY 5
int32_t zkp_correct_key_challenge_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t rounds, const uint32_t* n, uint64_t n_stride,
                                        const uint32_t* s, const uint32_t* r, uint32_t* out_sn, uint32_t* out_e, uint32_t* out_z,
                                        uint32_t* out_s_digest /* nullable */, uint8_t* out_status /* nullable */, uint32_t flags);
int32_t zkp_correct_key_challenge_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t rounds, const uint32_t* n,
                                               uint64_t n_stride, const uint8_t* seed, uint64_t first_index, uint32_t* out_sn, uint32_t* out_e,
                                               uint32_t* out_z, uint32_t* out_s_digest /* nullable */, uint8_t* out_status /* nullable */,
                                               uint32_t flags);
int32_t zkp_correct_key_prove_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t rounds, const uint32_t* p, const uint32_t* q,
                                    const uint32_t* sn, const uint32_t* e, const uint32_t* z, uint32_t* out_s_digest,
                                    uint8_t* out_error /* nullable */, uint32_t flags);
int32_t zkp_correct_key_verify_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t rounds, const uint32_t* n,
                                            uint64_t n_stride, const uint8_t* seed, uint64_t first_index, const uint32_t* proof_s_digest,
                                            uint8_t* out_verdict, uint32_t flags);

/* ------------------------------------------------------------------ probable primes, next prime, seeded Paillier key generation
 * Three layers of one piece of code (csrc/kernels_prime.hpp).  bits in {512, 1024, 2048} is the width of a value, pw = bits/32 words; these
 * are the factor widths of n_bits in {1024, 2048, 4096}.  The rule below is THIS library's published rule (tests/prime_model.py restates
 * it); it is not a claim of parity with upstream's keygen, whose shape it keeps: draw, set the low and the top bit, walk +2 through trial
 * division and strong tests, redraw.
 *   T: all odd primes below 6370 (the bound of the NiCorrectKeyProof verifier's primorial test).
 *   sprp(w, a), w odd > 3, 2 <= a <= w - 2: w - 1 = 2^s d with d odd, y = a^d mod w; passes iff y == 1, or y == w - 1, or
 *     y^(2^j) == w - 1 for some 1 <= j <= s - 1.
 *   Bases: base 0 is 2.  For round r = 1 .. rounds and L = bit_length(w), a_r = 2 + v, v = the first ceil((L - 2) / 32) keystream words from
 *     block 0 on of the stream below, as limbs, masked to L - 2 bits: a_r in [2, 2^(L-2) + 1], a subset of [2, w - 2].  The bases depend on
 *     (seed, index, field, r) and on L only: all candidates of one window share them.
 *   Stream: the nonce-stream construction above, unchanged (state words 13, 14 = index = first_index + i; word 15 = 0x80000000 |
 *     kind << 20 | slot << 4 | field), with one more kind:
 *       kind        slot              field   value
 *       9 Keygen    0                 0 / 1   start of attempt t for p / q: the first pw words of blocks [t nb, (t + 1) nb), nb = ceil(pw / 16),
 *                                             then bit 0 and bit bits - 1 set
 *       9 Keygen    r (1 .. rounds)   2 / 3   base a_r for p / q          (zkp_probable_prime_batch and zkp_next_prime_batch: field 2)
 *   is_probable_prime(w), any w < 2^bits, in this order: w < 2 -> 0; w == 2 -> 1; w even -> 0; for each l in T: w == l -> 1, l | w -> 0;
 *     w < 6370^2 -> 1 (exact: a composite below that has a factor in T); otherwise 1 iff sprp(w, 2) and sprp(w, a_r) for every r <= rounds.
 *     0 <= rounds <= 64; rounds == 0 is the base-2 test alone.
 *   next_prime(start): c_j = (start | 1) + 2 j, j = 0 .. 511; the first c_j < 2^bits, in order of j, with is_probable_prime(c_j) == 1, else none.
 *   Key b: for p (field 0) and q (field 1), attempts t = 0, 1, .., at most 128, take next_prime(start_t) with that factor's bases; the first
 *     attempt that finds one ends the search.  n = p q has n_bits or n_bits - 1 bits.  ZKP_VERDICT_MALFORMED (2) with zero p, q, n when
 *     either search used up its attempts or p == q; the other keys are unaffected.  With equal-width primes gcd(n, phi(n)) = 1 follows
 *     from p != q: a key made here is in the domain of zkp_paillier_open_batch.  No safe primes, no congruence conditions.
 * zkp_probable_prime_batch: out_verdict[i] = is_probable_prime(w[i]), w [count][pw].
 * zkp_next_prime_batch: out_prime [count][pw], out_offset [count] (j; nullable), out_status [count] (nullable; 0, or 2: none in the window,
 *   then out_prime and out_offset of the item are zero).
 * zkp_paillier_keygen_seeded_batch: out_p, out_q [batch][hw], hw = n_bits/64; out_n [batch][kw] (nullable), kw = n_bits/32; out_status
 *   [batch] (nullable).
 * `seed` (32 bytes) is a HOST pointer in both memory modes; it may be null only when rounds == 0, in the first two calls.
 * ZKP_F_DEVICE_PTRS is the only flag.  count, batch <= 2^20; 0 is ZKP_OK.  ZKP_EINVAL: a null ctx, a null required pointer, another width,
 * rounds > 64, an unknown flag; nothing is launched then.  A call split with first_index + lo equals the one call.
 * The exponentiations are zkp_modexp_batch's ladder at mod_bits = 2048 (narrower candidates travel zero-padded) with bits-bit exponents.
 * The calls run on the engine of the context that receives them, as zkp_dlog_statement_setup_seeded_batch does.
 * SECURITY CONTRACT, in the words of the two calls above: the seed is worth the key.  Every block of the context that held a start, a
 * candidate, a residue or a survivor map, a ladder row, the ladder's constants records and window tables (they hold the candidates as
 * moduli), a base, or the staged w / start / out_p / out_q / out_prime of a host-pointer call is registered secret with the call's stage
 * and zeroed on the stream before the call's blocks are given back, on error returns too; zkp_diag_witness_residue then reads 0.  With
 * ZKP_F_DEVICE_PTRS the caller's arrays are the caller's to wipe.  Nothing is claimed about timing: the number of attempts, of ladder rows
 * and of squarings depends on the secret, as upstream's loop count does. */
#define ZKP_SEEDED_KIND_KEYGEN 9u
int32_t zkp_probable_prime_batch(zkp_ctx* ctx, uint32_t bits, uint64_t count, const uint32_t* w, uint32_t rounds, const uint8_t* seed,
                                 uint64_t first_index, uint8_t* out_verdict, uint32_t flags);
int32_t zkp_next_prime_batch(zkp_ctx* ctx, uint32_t bits, uint64_t count, const uint32_t* start, uint32_t rounds, const uint8_t* seed,
                             uint64_t first_index, uint32_t* out_prime, uint32_t* out_offset /* nullable */,
                             uint8_t* out_status /* nullable */, uint32_t flags);
int32_t zkp_paillier_keygen_seeded_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, uint32_t rounds, const uint8_t* seed,
                                         uint64_t first_index, uint32_t* out_p, uint32_t* out_q, uint32_t* out_n /* nullable */,
                                         uint8_t* out_status /* nullable */, uint32_t flags);

/* ------------------------------------------------------------------ wire format
 * The reference serialises big integers as DECIMAL strings (src/serialize.rs:1-31 `bigint`, :33-78 `vecbigint`:
 * BigInt::to_str_radix(10) / from_str_radix(s, 10) = GMP mpz_get_str / mpz_set_str).  The two L1 entry points below
 * convert between that text and the fixed-width limb arrays of this ABI on the GPU, one number per lane.
 *
 * zkp_decimal_to_limbs_batch: item i is text[text_off .. text_off+len), converted into dst[dst_off .. dst_off+words)
 * (little-endian words, zero extended).  Accepted exactly as mpz_set_str(s, 10): optional leading '-', white space
 * anywhere.  out_status[i]: ZKP_DEC_OK; ZKP_DEC_INVALID (mpz_set_str fails: serde error / `unwrap()` panic at
 * serialize.rs:66); ZKP_DEC_NEGATIVE, ZKP_DEC_OVERFLOW (a valid BigInt this fixed-width ABI cannot carry: the caller
 * keeps that proof on its CPU path).  dst words of a failed item are zero.  words <= 528. */
typedef struct zkp_dec_item { uint64_t text_off; uint64_t dst_off; uint32_t len; uint32_t words; } zkp_dec_item;
#define ZKP_DEC_OK 0
#define ZKP_DEC_INVALID 1
#define ZKP_DEC_NEGATIVE 2
#define ZKP_DEC_OVERFLOW 3
int32_t zkp_decimal_to_limbs_batch(zkp_ctx* ctx, const char* text, uint64_t text_len, const zkp_dec_item* items, uint64_t count,
                                   uint32_t* dst, uint64_t dst_words, uint8_t* out_status, uint32_t flags);
/* zkp_limbs_to_decimal_batch: src[i*src_stride .. +words) -> the decimal string of item i, right aligned in row i of
 * out_text (rows of `pitch` bytes, pitch >= zkp_decimal_pitch(words)): the string is out_text + i*pitch + pitch - out_len[i],
 * out_len[i] bytes, no terminator, no leading zeros, "0" for zero. */
uint32_t zkp_decimal_pitch(uint32_t words);
int32_t zkp_limbs_to_decimal_batch(zkp_ctx* ctx, const uint32_t* src, uint64_t src_stride, uint32_t words, uint64_t count,
                                   char* out_text, uint32_t pitch, uint32_t* out_len, uint32_t flags);

/* serde_json documents of the reference's proof types -> the SoA batch (one document per proof, documents back to back or
 * anywhere in `text`; doc_off/doc_len [B]).  Field layout = serde defaults for the derives at range_proof.rs:32-81
 * (EncryptedPairs {"c1":[..],"c2":[..]}, Proof = [{"Open":{"w1","r1","w2","r2"}} | {"Mask":{"j","masked_x","masked_r"}} ..])
 * and correct_key_ni.rs:35-39 ({"sigma_vec":[..]}).  The reader is as tolerant as serde_json with the derived Deserialize impls: white
 * space between tokens (to_string_pretty), object fields in any order, unknown fields skipped, string escapes decoded; duplicate
 * or missing fields, a Response with more than one variant key and values of the wrong JSON type are errors, as they are for serde.
 * With flags == 0 the tokenising runs on the host (threads); with ZKP_F_DEVICE_PTRS on the device (see below
 * zkp_json_correct_key_proof_batch).  Every number is converted on the GPU into p->c1/c2 (pairs) or p->resp_*
 * (proof); p->error_factor rows are expected.  out_status[b]:
 *   ZKP_DOC_OK        converted;
 *   ZKP_DOC_INVALID   document b is not a value of the expected type (serde_json::from_str is Err in Rust);
 *   ZKP_DOC_HOST_PATH a well-formed document that this fixed layout cannot carry: a negative or over-wide integer (see ZKP_DEC_*), or
 *                     another number of rows.  It IS a valid value of the reference's type and has a verdict there: the caller parses
 *                     it itself (host/zkproofs.hpp: serde_json::range_proof_ni_from_str; bindings/rust: serde) and verifies it through
 *                     the host path that handles signed integers of any size (RangeProofNi::verify_batch).  Its rows here are zero.
 * ZKP_F_DEVICE_PTRS applies to the p-> arrays and out_status; text and offsets are host memory. */
#define ZKP_DOC_OK 0
#define ZKP_DOC_INVALID 2      /* == ZKP_VERDICT_MALFORMED */
#define ZKP_DOC_HOST_PATH 3
int32_t zkp_json_encrypted_pairs_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                       const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags);
int32_t zkp_json_range_proof_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                   const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags);
/* Whole RangeProofNi documents (range_proof_ni.rs:36-44): {"ek":{"n":..},"range":..,"ciphertext":..,"encrypted_pairs":{..},"proof":[..],
 * "error_factor":N} -> every field of the batch.  encrypted_pairs / proof as above.  ek, range and ciphertext are UN-annotated
 * in the reference: ek is kzen-paillier's EncryptionKey, range / ciphertext are bare curv BigInts; their text forms are fixed by crates
 * outside the tree and need not agree with each other, so `bigint_forms` names BOTH: ZKP_BIGINT_FORMS(key_form, bare_form) (a sample
 * written by a Rust build decides, tools/reference_vectors "serde" section).  A string that is not an integer of the named form is
 * ZKP_DOC_INVALID — an all-digit decimal read as hex would silently be another number, which is why the two forms are separate.
 * error_factor other than p->error_factor: ZKP_DOC_HOST_PATH.
 * p->n_stride = n_bits/32: one key per proof, p->n receives the documents' keys (verify_self, range_proof_ni.rs:109-128).
 * p->n_stride = 0: p->n is the VERIFIER's key, an input that is never written; a document under another key is ZKP_DOC_INVALID
 * (RangeProofNi::verify asserts equality, :86), so no received document can change the key the others are verified under.
 * Writes p->range and p->ciphertext (inputs of the other entry points, hence const in the struct).
 * flags 0: host arrays, tokenised on the host as described above.
 * ZKP_F_DEVICE_PTRS: the p-> arrays and out_status are device memory (with n_stride == 0 the verifier's key p->n as well); text and
 * offsets stay host memory.  The text is uploaded once and tokenised ON THE DEVICE (csrc/kernels_serde_scan.hpp): a document that is byte
 * for byte what serde_json::to_string writes — compact, fields in declaration order, no escapes — is read there; any other document goes
 * through the host tokeniser and is merged into the same arrays.  Arrays and statuses are those of the flags-0 call, byte for byte. */
#define ZKP_BIGINT_DEC 0u     /* "1234": decimal string (serialize::bigint, serialize.rs:8-33) */
#define ZKP_BIGINT_HEX 1u     /* "04d2": hex string of the big-endian magnitude */
#define ZKP_BIGINT_BYTES 2u   /* [4,210]: array of big-endian byte values */
#define ZKP_BIGINT_FORMS(key_form, bare_form) (((key_form) << 4) | (bare_form))
int32_t zkp_json_range_proof_ni_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t bigint_forms,
                                      const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags);
/* RangeProofNi::verify / verify_self on documents: text in, one status byte and one verdict byte per document out.
 * = zkp_json_range_proof_ni_batch (device route) into arrays the call owns, then zkp_range_ni_verify_batch on them; no limb leaves the device.
 * text, doc_off, doc_len and verifier_n are host memory; ZKP_F_DEVICE_PTRS applies to out_status and out_verdict only.
 * verifier_n [n_bits/32]: RangeProofNi::verify under that key (a document under another key: ZKP_DOC_INVALID); NULL: verify_self, every
 * document under its own key.  out_status[b]: ZKP_DOC_*, exactly what zkp_json_range_proof_ni_batch gives for the document in that key
 * mode.  out_verdict[b]: what zkp_range_ni_verify_batch gives for the converted document where the status is ZKP_DOC_OK, and
 * ZKP_VERDICT_REJECT everywhere else, so a caller who ignores the status never accepts an unread proof (ZKP_DOC_HOST_PATH documents do
 * have a verdict in the reference: the caller's host path, see above).
 * The WHOLE batch is verified and the verdicts of unconverted documents are MASKED AFTERWARDS: such a document leaves zero rows (and, with
 * verify_self, a zero key), which costs its share of the launch, changes no other document's verdict and never fails the call. */
int32_t zkp_range_ni_verify_json_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                       uint64_t batch, uint32_t n_bits, uint32_t error_factor, uint32_t bigint_forms,
                                       const uint32_t* verifier_n /* [kw], NULL = verify_self: each document's own key */,
                                       uint8_t* out_status /* [B] ZKP_DOC_* */, uint8_t* out_verdict /* [B] ZKP_VERDICT_* */,
                                       uint32_t flags);
/* RangeProof::verifier_output (range_proof.rs:254-355) on the two received documents of an interactive session: EncryptedPairs b and Proof b
 * are two spans of the same `text` (host memory, uploaded once, like the four offset arrays); one status byte and one verdict byte per
 * session come out.  = zkp_json_encrypted_pairs_batch and zkp_json_range_proof_batch (device route) into arrays the call owns, then
 * zkp_range_verifier_output_batch on them; no limb travels to the host.  The statement (n, n_stride, range, ciphertext: n_stride 0 or
 * n_bits/32) and the verifier's own challenge (e [B][32] left aligned, e_len [B]) are limbs and bytes; ZKP_F_DEVICE_PTRS applies to them and
 * to out_status and out_verdict.  out_status[b]: the worse of the two documents' reader statuses (ZKP_DOC_INVALID beats ZKP_DOC_HOST_PATH
 * beats ZKP_DOC_OK; a document with another number of rows than error_factor is ZKP_DOC_HOST_PATH).  out_verdict[b]: what
 * zkp_range_verifier_output_batch gives where the status is ZKP_DOC_OK (ZKP_VERDICT_MALFORMED for a challenge shorter than
 * ceil(error_factor / 8) bytes included), ZKP_VERDICT_REJECT everywhere else.  The whole batch is launched and the verdicts of unread
 * sessions are masked afterwards: such a session costs its share of the launch, changes no other verdict and never fails the call.
 * n_bits in {1024, 2048, 4096}, error_factor 1 .. 256, batch 0 .. 2^24. */
int32_t zkp_range_verifier_output_json_batch(zkp_ctx* ctx, const char* text, const uint64_t* pairs_off, const uint64_t* pairs_len,
                                             const uint64_t* proof_off, const uint64_t* proof_len, uint64_t batch, uint32_t n_bits,
                                             uint32_t error_factor, const uint32_t* n, uint64_t n_stride, const uint32_t* range,
                                             const uint32_t* ciphertext, const uint8_t* e, const uint8_t* e_len,
                                             uint8_t* out_status /* [B] ZKP_DOC_* */, uint8_t* out_verdict /* [B] ZKP_VERDICT_* */, uint32_t flags);
/* {"sigma_vec":["..", x11]} -> sigma [B][11][n_bits/32].  A sigma_vec of another length is ZKP_DOC_INVALID; an over-wide or negative
 * entry is ZKP_DOC_HOST_PATH (that entry is zero, the others are converted). */
int32_t zkp_json_correct_key_proof_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits,
                                         uint64_t batch, uint32_t* out_sigma, uint8_t* out_status, uint32_t flags);
/* The three readers above with ZKP_F_DEVICE_PTRS (outputs in device memory) take the route of zkp_json_range_proof_ni_batch: the text is
 * uploaded once and tokenised ON THE DEVICE (csrc/kernels_serde_scan.hpp).  A document that is byte for byte what serde_json::to_string
 * writes — {"c1":["D",..EF],"c2":["D",..EF]} / [ROW,..EF] / {"sigma_vec":["D",..11]}, compact, fields in declaration order, no escapes,
 * every D of at most zkp_decimal_pitch(words) - 1 digits — is read there; any other document goes through the host tokeniser, as a
 * sub-batch of the flags-0 call, and is merged into the same arrays.  Arrays and statuses are those of the flags-0 call, byte for byte.
 *
 * NiCorrectKeyProof::verify (correct_key_ni.rs:73-100) on documents: text in, one status byte and one verdict byte per document out.
 * = zkp_json_correct_key_proof_batch (device route) into a sigma block the call owns, then zkp_correct_key_ni_verify_batch on it; no limb
 * travels to the host.  text, doc_off, doc_len and salt are host memory; ZKP_F_DEVICE_PTRS applies to n, out_status and out_verdict.
 * n [B][n_bits/32]: one key per document, as limbs.  out_status[b]: exactly what zkp_json_correct_key_proof_batch gives for document b.
 * out_verdict[b]: what zkp_correct_key_ni_verify_batch gives for the converted proof where the status is ZKP_DOC_OK, ZKP_VERDICT_REJECT
 * everywhere else.  The WHOLE batch is verified and the verdicts of unread documents are masked afterwards: such a document costs its
 * share of the launch, changes no other verdict and never fails the call.  n_bits in {1024, 2048, 4096}, batch 0 .. 2^24. */
int32_t zkp_correct_key_ni_verify_json_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                             uint64_t batch, uint32_t n_bits, const uint32_t* n /* [B][n_bits/32], one key per document */,
                                             const uint8_t* salt, uint32_t salt_len,
                                             uint8_t* out_status /* [B] ZKP_DOC_* */, uint8_t* out_verdict /* [B] ZKP_VERDICT_* */, uint32_t flags);

/* The SoA batch -> serde_json documents: the mirror images of the four readers.  The text is byte for byte what serde_json::to_string
 * gives for the reference's derives: compact, fields in declaration order, every annotated BigInt a decimal string as mpz_get_str writes
 * it (no leading zeros, "0" for zero), `j` and `error_factor` bare numbers; ek.n, range and ciphertext in the forms `bigint_forms`
 * names, exactly as the reader understands them (hex: lower case, two characters per byte of the big-endian magnitude, "00" for zero).
 * Radix conversion, sizing and assembly all run on the GPU; only finished text leaves it.
 *   Documents lie back to back in out_text, no separator, no terminator: document b is [out_doc_off[b], out_doc_off[b + 1]);
 *   out_doc_off has batch + 1 entries (4096 proofs under a 2048-bit key are more than 2^31 bytes: everything here is 64 bits wide).
 *   out_text == NULL: the sizing call — only the exact offsets are computed.  text_cap < out_doc_off[batch]: ZKP_EINVAL, the offsets
 *   are written, the error string names both numbers, no byte of out_text is touched.  zkp_json_doc_bound (a pure host function, no
 *   device needed): an upper bound of one document's length, so that batch * bound can be allocated once and the sizing call skipped;
 *   0 for arguments no writer accepts.  doc_kind: ZKP_JSON_DOC_*; error_factor is ignored for a NiCorrectKeyProof and the two
 *   DLog kinds, bigint_forms for everything but a RangeProofNi and the two DLog kinds (whose bare form it is).
 *   out_status [batch] (nullable): ZKP_DOC_OK, or ZKP_DOC_INVALID where a row of proof b has a resp_kind that is neither ZKP_RESP_OPEN nor
 *   ZKP_RESP_MASK: no Response has that variant, the document is empty (out_doc_off[b + 1] == out_doc_off[b]), the others are unaffected.
 *   resp_j is written as the byte it is.  Reads c1, c2 (pairs); resp_* (proof); every field (RangeProofNi: n_stride == 0 writes the
 *   shared key into every document).  n_bits in {1024, 2048, 4096}, error_factor 1 .. 256, batch 0 .. 2^24.
 *   ZKP_F_DEVICE_PTRS applies to the p-> arrays, sigma and out_status — a batch is consumed as zkp_range_ni_prove_batch /
 *   zkp_range_ni_prove_seeded_batch left it, no limb travels to the host; out_text and out_doc_off are host memory. */
#define ZKP_JSON_DOC_ENCRYPTED_PAIRS 0u
#define ZKP_JSON_DOC_RANGE_PROOF 1u
#define ZKP_JSON_DOC_RANGE_PROOF_NI 2u
#define ZKP_JSON_DOC_CORRECT_KEY_PROOF 3u
/* (4 is no kind, and stays none: zkp_json_doc_bound answers 0 for it, as callers written against the first four kinds expect) */
#define ZKP_JSON_DOC_DLOG_PROOF 5u         /* bigint_forms = the bare form alone; error_factor is ignored; the bound is taken at y_bits == n_bits, */
#define ZKP_JSON_DOC_DLOG_STATEMENT 6u     /* the widest y the entry points accept, so it holds for every y_bits */
/* (7 is no kind either.)  The sigma-proof kinds, see "ZeroProof, CiphertextProof, VerlinProof and MulProof as documents" below: bigint_forms
 * names both forms, error_factor is ignored. */
#define ZKP_JSON_DOC_ZERO_STATEMENT 8u
#define ZKP_JSON_DOC_ZERO_PROOF 9u
#define ZKP_JSON_DOC_CIPHERTEXT_STATEMENT 10u
#define ZKP_JSON_DOC_CIPHERTEXT_PROOF 11u
#define ZKP_JSON_DOC_VERLIN_STATEMENT 12u
#define ZKP_JSON_DOC_VERLIN_PROOF 13u
#define ZKP_JSON_DOC_MUL_STATEMENT 14u
#define ZKP_JSON_DOC_MUL_PROOF 15u
uint64_t zkp_json_doc_bound(uint32_t doc_kind, uint32_t n_bits, uint32_t error_factor, uint32_t bigint_forms);
int32_t zkp_json_write_encrypted_pairs_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, char* out_text, uint64_t text_cap, uint64_t* out_doc_off,
                                             uint8_t* out_status, uint32_t flags);
int32_t zkp_json_write_range_proof_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, char* out_text, uint64_t text_cap, uint64_t* out_doc_off,
                                         uint8_t* out_status, uint32_t flags);
int32_t zkp_json_write_range_proof_ni_batch(zkp_ctx* ctx, const zkp_range_ni_proofs* p, uint32_t bigint_forms, char* out_text, uint64_t text_cap,
                                            uint64_t* out_doc_off, uint8_t* out_status, uint32_t flags);
int32_t zkp_json_write_correct_key_proof_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* sigma, char* out_text, uint64_t text_cap,
                                               uint64_t* out_doc_off, uint8_t* out_status, uint32_t flags);

/* ------------------------------------------------------------------ CompositeDLogProof and DLogStatement as documents
 * wi_dlog_proof.rs:32-43, field order of the derives:
 *   CompositeDLogProof   {"x":X,"y":X}            x [B][kw], y [B][y_bits/32]
 *   DLogStatement        {"N":X,"g":X,"ni":X}     N, g, ni [B][kw]
 * kw = n_bits/32; n_bits in {1024, 2048, 4096}; y_bits a multiple of 32, 544 .. n_bits (as for zkp_dlog_verify_batch); batch 0 .. 2^24.
 * Every X is an un-annotated curv BigInt; bare_form (ZKP_BIGINT_DEC / _HEX / _BYTES) names its text form and means exactly what it means
 * for `range` and `ciphertext` of a RangeProofNi document.
 *
 * Readers.  out_status[b]: ZKP_DOC_OK; ZKP_DOC_INVALID (not a value of the type: a missing or duplicate field, a wrong JSON type, a string
 * that is not an integer of the named form; every field of the document is zero); ZKP_DOC_HOST_PATH (a valid value the fixed layout
 * cannot carry: a negative field, or one wider than its array; THAT field is zero, the others are converted).
 * flags 0: host arrays, tokenised on the host by the tolerant tokeniser of the readers above (white space, any field order, unknown
 * fields skipped, escapes in field names decoded).  ZKP_F_DEVICE_PTRS: outputs and status in device memory, text and offsets host memory;
 * the text is uploaded once; a document that is byte for byte canonical — compact, fields in declaration order, X = "D" with at most
 * zkp_decimal_pitch(words) - 1 digits | lower-case even-length hex of at most 8 * words characters | [U,..] of at most 4 * words byte
 * values — is read on the device, any other falls back to the flags-0 path as a sub-batch and is merged in.  Arrays and statuses equal
 * the flags-0 call's, byte for byte. */
int32_t zkp_json_dlog_statement_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits,
                                      uint64_t batch, uint32_t bare_form, uint32_t* out_N, uint32_t* out_g, uint32_t* out_ni,
                                      uint8_t* out_status, uint32_t flags);
int32_t zkp_json_dlog_proof_batch(zkp_ctx* ctx, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits,
                                  uint32_t y_bits, uint64_t batch, uint32_t bare_form, uint32_t* out_x, uint32_t* out_y,
                                  uint8_t* out_status, uint32_t flags);
/* Writers: the contract of the four writers above (sizing call with out_text == NULL, batch + 1 offsets of 64 bits, ZKP_EINVAL with no
 * byte touched when text_cap is short, out_status nullable and always ZKP_DOC_OK here).  ZKP_F_DEVICE_PTRS applies to the limb arrays
 * and out_status, so the output of zkp_dlog_prove_batch is serialised where it lies.  The text is what the readers call canonical:
 * decimal without leading zeros, hex with two characters per byte of the magnitude ("00" for zero), byte arrays without a leading zero
 * byte ([0] for zero). */
int32_t zkp_json_write_dlog_statement_batch(zkp_ctx* ctx, uint32_t n_bits, uint64_t batch, const uint32_t* N, const uint32_t* g,
                                            const uint32_t* ni, uint32_t bare_form, char* out_text, uint64_t text_cap,
                                            uint64_t* out_doc_off, uint8_t* out_status, uint32_t flags);
int32_t zkp_json_write_dlog_proof_batch(zkp_ctx* ctx, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* x,
                                        const uint32_t* y, uint32_t bare_form, char* out_text, uint64_t text_cap, uint64_t* out_doc_off,
                                        uint8_t* out_status, uint32_t flags);
/* CompositeDLogProof::verify (wi_dlog_proof.rs:67-91) on documents: statement b and proof b are two spans of the same `text` (host memory,
 * uploaded once); one status byte and one verdict byte per pair come out; ZKP_F_DEVICE_PTRS applies to out_status and out_verdict only.
 * = both readers (device route) into arrays the call owns, a domain check on the device, zkp_dlog_verify_batch on those arrays.
 * out_status[b] starts as the worse of the two documents' statuses (ZKP_DOC_INVALID beats ZKP_DOC_HOST_PATH beats ZKP_DOC_OK).  A pair
 * still OK becomes ZKP_DOC_HOST_PATH when N is even or zero, or one of g, ni, x is >= N: such a pair has a verdict in the reference
 * (mod_pow reduces its base, x >= N never equals the product, an even N is legal), which the limb kernels cannot give; the caller's
 * host path does (host/zkproofs.hpp: CompositeDLogProof::verify).  This is STRICTER than zkp_dlog_verify_batch, which assumes
 * x, g, ni < N unchecked and reports an even N as ZKP_VERDICT_MALFORMED (its documented deviation): here no such pair reaches it.
 * out_verdict[b]: what zkp_dlog_verify_batch gives where the status is ZKP_DOC_OK (ZKP_VERDICT_MALFORMED for the reference's three
 * assertions included), ZKP_VERDICT_REJECT everywhere else.  The whole batch is launched and the verdicts of unread pairs are masked
 * afterwards: such a pair is five zero rows, costs its share of the launch, changes no other verdict and never fails the call. */
int32_t zkp_dlog_verify_json_batch(zkp_ctx* ctx, const char* text, const uint64_t* st_off, const uint64_t* st_len, const uint64_t* pf_off,
                                   const uint64_t* pf_len, uint64_t batch, uint32_t n_bits, uint32_t y_bits, uint32_t bare_form,
                                   uint8_t* out_status /* [B] ZKP_DOC_* */, uint8_t* out_verdict /* [B] ZKP_VERDICT_* */, uint32_t flags);

/* ------------------------------------------------------------------ ZeroProof, CiphertextProof, VerlinProof and MulProof as documents
 * zero_enc_proof.rs:26-41, correct_ciphertext.rs:22-39, verlin_proof.rs:34-57, multiplication_proof.rs:32-57: the serde defaults of the
 * derives, fields in declaration order.  K = ek.n in the key form, every X an un-annotated curv BigInt in the bare form, both named by
 * bigint_forms = ZKP_BIGINT_FORMS(key_form, bare_form) exactly as for a RangeProofNi document.  kw = n_bits/32, zw = kw + ZKP_Z1_EXTRA_LIMBS.
 *   ZKP_JSON_DOC_ZERO_STATEMENT        {"ek":{"n":K},"c":X}                                      n [kw], c [2kw]
 *   ZKP_JSON_DOC_ZERO_PROOF            {"z":X,"a":X}                                             z, a [2kw]
 *   ZKP_JSON_DOC_CIPHERTEXT_STATEMENT  {"ek":{"n":K},"c":X}                                      n [kw], c [2kw]
 *   ZKP_JSON_DOC_CIPHERTEXT_PROOF      {"z1":X,"z2":X,"c_prime":X}                               z1 [zw], z2, c_prime [2kw]
 *   ZKP_JSON_DOC_VERLIN_STATEMENT      {"ek":{"n":K},"c":X,"c_prime":X,"phi_x":X}                n [kw], c, c_prime, phi_x [2kw]
 *   ZKP_JSON_DOC_VERLIN_PROOF          {"phi_a":X,"z":X,"z_prime":X,"z_double_prime":X,"r_z":X}  phi_a, r_z [2kw]; z, z_prime, z_double_prime [zw]
 *   ZKP_JSON_DOC_MUL_STATEMENT         {"ek":{"n":K},"e_a":X,"e_b":X,"e_c":X}                    n [kw], e_a, e_b, e_c [2kw]
 *   ZKP_JSON_DOC_MUL_PROOF             {"f":X,"z1":X,"z2":X,"e_d":X,"e_db":X}                    f [kw]; z1, z2, e_d, e_db [2kw]
 * zkp_sigma_fields: the arrays of one kind, [B][words] each, in the order of the table (a statement's f0 is the key); unused entries NULL.
 * Its layout is that of `uint32_t* f[5]`, five pointers back to back, and may be filled as such; the members are spelled out one by one
 * because the generated Rust bindings and their check carry scalar members only.
 *
 * zkp_json_sigma_batch, the reader: the contract of zkp_json_dlog_*_batch.  out_status[b]: ZKP_DOC_OK; ZKP_DOC_INVALID (a missing or duplicate
 * field, "ek" without "n", a wrong JSON type, a string that is no integer of the named form; every field of the document is zero);
 * ZKP_DOC_HOST_PATH (a negative field, or one wider than its array; THAT field is zero, the others are converted).  flags 0: host arrays, the
 * tolerant host tokeniser (white space, any field order, unknown fields skipped — inside "ek" too —, escapes in names decoded).
 * ZKP_F_DEVICE_PTRS: outputs and status in device memory; the text is uploaded once; a byte-for-byte canonical document is scanned on the
 * device, any other falls back to the flags-0 path as a sub-batch and is merged in.  Arrays and statuses equal the flags-0 call's.
 * zkp_json_write_sigma_batch, the writer: the contract of the writers above (sizing call with out_text == NULL, batch + 1 offsets of 64 bits,
 * ZKP_EINVAL with no byte touched when text_cap is short, canonical text as the reader defines it); ZKP_F_DEVICE_PTRS applies to the limb
 * arrays and out_status, so the output of a zkp_*_prove_batch call is serialised where it lies.
 * n_bits in {1024, 2048, 4096}, batch 0 .. 2^24; zkp_json_doc_bound answers for the eight kinds. */
typedef struct zkp_sigma_fields { uint32_t* f0; uint32_t* f1; uint32_t* f2; uint32_t* f3; uint32_t* f4; } zkp_sigma_fields;
int32_t zkp_json_sigma_batch(zkp_ctx* ctx, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits,
                             uint64_t batch, uint32_t bigint_forms, const zkp_sigma_fields* out, uint8_t* out_status, uint32_t flags);
int32_t zkp_json_write_sigma_batch(zkp_ctx* ctx, uint32_t doc_kind, uint32_t n_bits, uint64_t batch, const zkp_sigma_fields* in,
                                   uint32_t bigint_forms, char* out_text, uint64_t text_cap, uint64_t* out_doc_off, uint8_t* out_status,
                                   uint32_t flags);
/* The four verifies on documents.  proof_kind: one of the four ZKP_JSON_DOC_*_PROOF kinds; statement b is of the kind in front of it.
 * Statement b and proof b are two spans of the same `text` (host memory, uploaded once); one status byte and one verdict byte per pair come
 * out; ZKP_F_DEVICE_PTRS applies to out_status and out_verdict only.  = both readers (device route) into arrays the call owns, a domain
 * check on the device, the type's zkp_*_verify_batch on those arrays with one key per pair, taken from its statement; no limb travels to
 * the host.  out_status[b] starts as the worse of the two documents' statuses (ZKP_DOC_INVALID beats ZKP_DOC_HOST_PATH beats ZKP_DOC_OK).
 * A pair still OK becomes ZKP_DOC_HOST_PATH when its key is even or below 2, when one of its 2kw-wide fields is >= n^2, or when MulProof.f
 * is >= n.  Every honest value is inside this domain; outside it the reference still has a verdict (mod_pow, % and Paillier::add reduce,
 * the challenge hashes the raw value) that the limb kernels were never specified to give, and reducing first would change the hash.
 * out_verdict[b]: what the type's verify gives where the status is ZKP_DOC_OK (ZKP_VERDICT_MALFORMED where multiplication_proof.rs:133
 * panics included), ZKP_VERDICT_REJECT everywhere else.  The whole batch is launched and the verdicts of unread pairs are masked
 * afterwards: such a pair is zero rows, costs its share of the launch, changes no other verdict and never fails the call. */
int32_t zkp_sigma_verify_json_batch(zkp_ctx* ctx, uint32_t proof_kind, const char* text, const uint64_t* st_off, const uint64_t* st_len,
                                    const uint64_t* pf_off, const uint64_t* pf_len, uint64_t batch, uint32_t n_bits, uint32_t bigint_forms,
                                    uint8_t* out_status /* [B] ZKP_DOC_* */, uint8_t* out_verdict /* [B] ZKP_VERDICT_* */, uint32_t flags);

/* ------------------------------------------------------------------ several GPUs behind one caller
 * The reference spreads a proof's rows over a rayon pool (src/zkproofs/range_proof.rs:161-187,270-348); here a batch
 * is cut into contiguous blocks of PROOF indices, one block per device context, one host thread per context
 * (the only threads this library starts).  The caller hands over HOST pointers: every block reads its slice of the caller's
 * arrays and its output slab lands in the caller's output arrays — by per-GPU D2H, or, with ZKP_GATHER_RCCL, after an RCCL
 * all-gather that also leaves the whole result device-resident on every GPU (below).  (One PROCESS per GPU — torch.distributed
 * ranks — is zk-paillier_amd/shard.py + bench.py.)  device_ids may repeat in ZKP_GATHER_HOST mode: two contexts on one GPU are
 * two independent streams.  Results are identical to one call of the single-context entry point on the whole batch. */
typedef struct zkp_multi zkp_multi;
int32_t zkp_multi_create(const int32_t* device_ids, uint32_t n_devices, zkp_multi** out);
int32_t zkp_multi_destroy(zkp_multi* m);
uint32_t zkp_multi_size(zkp_multi* m);
zkp_ctx* zkp_multi_ctx(zkp_multi* m, uint32_t i);            /* context i (owned by m), e.g. for zkp_timing_* */
const char* zkp_multi_last_error_string(zkp_multi* m);
/* the most recent batch call, per device context i: the block [lo, hi) of items it was given and the wall time of its share
 * (staging, launches and the D2H of its output slab), in milliseconds */
int32_t zkp_multi_last_timing(zkp_multi* m, uint32_t i, double* out_ms, uint64_t* out_lo, uint64_t* out_hi);
/* ... and its two phases on device context i's own stream (HIP events), in milliseconds: the compute of its block (staging of its inputs
 * included) and, in the gathering modes below, the all-gather behind it — which ends when the slowest peer has delivered, so it holds the
 * wait for stragglers as well as the exchange.  ZKP_GATHER_HOST: compute = the wall time of the context's blocking call, gather = 0. */
int32_t zkp_multi_last_phases(zkp_multi* m, uint32_t i, double* out_compute_ms, double* out_gather_ms);
/* Where the outputs of the batch calls below are reassembled.
 *   ZKP_GATHER_HOST (default): every context copies its output slab into the caller's host arrays (one D2H per GPU, no collective).
 *   ZKP_GATHER_RCCL: every context works on device-resident copies of its block and writes its slab into its segment of a buffer
 *     holding the WHOLE batch; one grouped ncclAllGather per output (RCCL over xGMI, on the contexts' streams) then leaves the whole
 *     gathered output in the memory of EVERY GPU, and the caller's host arrays are filled from one GPU's copy — same bytes as
 *     ZKP_GATHER_HOST.  Gathered: the verdict bytes of the verify calls; status bytes, c1 and c2 of a prove call.  The first switch
 *     to ZKP_GATHER_RCCL creates one communicator per context (ncclCommInitAll): ZKP_EDEVICE with RCCL's text
 *     (zkp_multi_last_error_string) if that fails, e.g. for a device listed twice.
 * zkp_multi_gathered: the device-resident result of the most recent ZKP_GATHER_RCCL call on device context `device_index`:
 *   which = 0 verdict / status bytes, 1 c1, 2 c2.  Blocks of unequal size are padded to the largest: block i (the items
 *   zkp_multi_last_timing reports for context i) starts at i * *out_block_stride_bytes; *out_bytes = n_contexts * stride.  The pointer
 *   stays valid until the next batch call or zkp_multi_destroy; work that consumes it is ordered on zkp_ctx_stream(zkp_multi_ctx(m, i)). */
#define ZKP_GATHER_HOST 0u
#define ZKP_GATHER_RCCL 1u
#define ZKP_GATHER_COPY 2u   /* the device-resident gather of ZKP_GATHER_RCCL by device-to-device copies instead of the collective: for device
                                lists RCCL has no communicator for (a GPU listed several times); same layout, same zkp_multi_gathered */
int32_t zkp_multi_set_gather(zkp_multi* m, uint32_t mode);
int32_t zkp_multi_gathered(zkp_multi* m, uint32_t device_index, uint32_t which, void** out_device_ptr, uint64_t* out_block_stride_bytes,
                           uint64_t* out_bytes);
int32_t zkp_multi_range_ni_prove_batch(zkp_multi* m, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w,
                                       uint8_t* out_e, uint8_t* out_e_len, uint8_t* out_status);
/* zkp_range_ni_prove_seeded_batch over the contexts: block i passes first_index + lo_i, so the result is byte-identical to one
 * single-context call.  ZKP_GATHER_HOST only (ZKP_EINVAL in the device-resident gathering modes). */
int32_t zkp_multi_range_ni_prove_seeded_batch(zkp_multi* m, const zkp_range_ni_proofs* p, const uint32_t* x, const uint32_t* r,
                                              const uint8_t* seed, uint64_t first_index,
                                              uint8_t* out_e, uint8_t* out_e_len, uint8_t* out_status);
int32_t zkp_multi_range_ni_verify_batch(zkp_multi* m, const zkp_range_ni_proofs* p, uint8_t* out_verdict);
int32_t zkp_multi_correct_key_ni_verify_batch(zkp_multi* m, uint32_t n_bits, uint64_t batch, const uint32_t* n,
                                              const uint32_t* sigma, const uint8_t* salt, uint32_t salt_len,
                                              uint8_t* out_verdict);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_HIP_H */
