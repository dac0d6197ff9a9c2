// zkp_api_ck_inter.inc — host side of the interactive CorrectKey for whole batches of sessions (kernels_ck_inter.hpp); included by zkp_api.hip
// behind zkp_api_ck_prove.inc.  The challenge runs the ladder zkp_modexp_batch uses (run_setup, modexp_core) under the verifier's n, the
// existing product (modmul_ctx) and hash_list; its seeded form puts the sampler (nonce_sample_run) in front.  The prove runs the shared
// pieces of zkp_api_paillier_dec.inc — crt_keys_prepare, ladder_rows_take, SecretLadder — over six half-width rows per round.  The challenge
// and the prove go to one engine whole (ZKP_ROUTE_WHOLE, by the larger launch).

static bool cki_args_ok(uint32_t n_bits, uint64_t batch, uint32_t K, uint32_t flags) {
  return key_bits_ok(n_bits) && K >= 1 && K <= 256 && batch <= (1ull << 24) && batch * K <= (1ull << 24) && !(flags & ~(uint32_t)ZKP_F_DEVICE_PTRS);
}

// The stream of kind ZKP_SEEDED_KIND_CORRECT_KEY: slot i < K, field 0 = s_i, field 1 = r_i (r null: s alone, the verifier's second message).
// Every pointer is device memory; status is written for every session.
static int32_t cki_sample(zkp_ctx* c, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* key, uint64_t first_index,
                          uint32_t* s_out, uint32_t* r_out, uint8_t* status) {
  NonceSampleArgs a{};
  a.key = key; a.n = n; a.n_stride = n_stride; a.status = status;
  a.first_index = first_index; a.batch = B; a.kw = n_bits / 32; a.kind = ZKP_SEEDED_KIND_CORRECT_KEY;
  uint32_t* const fields[2] = {s_out, r_out};
  for (uint32_t f = 0; f < 2; f++)
    if (fields[f]) { a.below[a.nbelow] = fields[f]; a.below_field[a.nbelow] = f; a.below_per[a.nbelow] = K; a.below_slot0[a.nbelow] = 0; a.nbelow++; }
  return nonce_sample_run(c, a, ND_NONE);
}

// The challenge on device memory.  status holds the sampler's verdicts on entry when `seeded`.  Blocks of `s`: base (s and r under n) and s^e
// are registered secret; the rows of n, sn, rn and the repeated e are public.
template <int G>
static int32_t cki_challenge_impl(zkp_ctx* c, Stage& s, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* ds,
                                  const uint32_t* dr, uint32_t* out_sn, uint32_t* out_e, uint32_t* out_z, uint32_t* out_sd, uint8_t* status, bool seeded) {
  const uint32_t kw = n_bits / 32;
  const uint64_t items = B * K, nrows = n_stride ? 2 * items : 1;
  const bool per_row = n_stride != 0;
  uint32_t *base = s.secret_scratch<uint32_t>(2 * items * kw), *se = s.secret_scratch<uint32_t>(items * kw);
  uint32_t *nrow = s.scratch<uint32_t>(nrows * kw), *pw = s.scratch<uint32_t>(2 * items * kw), *erow = s.scratch<uint32_t>(items * 8);
  if (s.st) return s.st;
  const int lanes = 16;
  hipLaunchKernelGGL(k_cki_chal_status, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, n, n_stride, (int)kw, B, seeded ? 1 : 0, status);
  hipLaunchKernelGGL(k_cki_chal_rows, dim3((unsigned)((nrows * kw + 255) / 256)), dim3(256), 0, c->stream, n, n_stride, (int)kw, items, K, nrows, nrow);
  CkiChalReduceArgs ra{ds, dr, n, n_stride, status, base, items, K, (int)kw};
  hipLaunchKernelGGL(k_cki_chal_reduce, dim3((unsigned)((2 * items + lanes - 1) / lanes)), dim3(lanes), lanes * cki_chal_reduce_lds_words_per_lane((int)kw) * 4, c->stream, ra);
  HIPCHK(c, hipGetLastError());
  int32_t st;
  if ((st = run_setup<G>(c, nrow, per_row ? kw : 0, (int)kw, 0, nrows, c->consts))) return st;
  // sn | rn: 2 K B rows with the n_bits-bit exponent n
  if ((st = modexp_core<G>(c, c->consts, n_bits, 2 * items, base, nrow, per_row ? kw : 0, per_row, pw, (int)kw))) return st;
  if ((st = hash_list(c, B, {{n, n_stride, 0, kw, 1}, {pw, (uint64_t)K * kw, kw, kw, K}, {pw + items * kw, (uint64_t)K * kw, kw, kw, K}}, out_e))) return st;
  if ((st = launch_rows(c, k_repeat_rows, items * 8, (const uint32_t*)out_e, (uint64_t)8, 8u, K, items, erow))) return st;
  // s^e: K B rows with a 256-bit exponent, under the records of the first K B rows
  if ((st = modexp_core<G>(c, c->consts, 256, items, base, erow, 8, per_row, se, (int)kw))) return st;
  if ((st = modmul_ctx<G>(c, c->consts, per_row, items, base + items * kw, 0, se, 0, out_z, (int)kw))) return st;
  if (out_sd && (st = hash_list(c, B, {{ds, (uint64_t)K * kw, kw, kw, K}}, out_sd))) return st;
  CkiChalFinishArgs fa{pw, status, out_sn, out_z, out_e, out_sd, items, K, (int)kw};
  return launch_rows(c, k_cki_chal_finish, items * kw, fa);
}

// both challenge calls: seed null = the caller's s and r
static int32_t cki_challenge(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* sv,
                             const uint32_t* rv, const uint8_t* seed, uint64_t first_index, uint32_t* out_sn, uint32_t* out_e, uint32_t* out_z,
                             uint32_t* out_sd, uint8_t* out_status, uint32_t flags) {
  const uint32_t kw = n_bits / 32;
  const uint64_t items = batch * K;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  uint32_t* dsn = s.out(out_sn, items * kw);
  uint32_t* de = s.out(out_e, batch * 8);
  uint32_t* dz = s.out(out_z, items * kw);
  uint32_t* dsd = s.out(out_sd, batch * 8);
  uint8_t* dst = s.out(out_status, batch);
  if (!s.dev) s.secret(dsd, batch * 8 * 4);                  // (host arrays: the staged copy is wiped behind the D2H)
  if (!dst) dst = s.scratch<uint8_t>(batch);
  const uint32_t *dsv = nullptr, *drv = nullptr;
  int32_t st = s.st;
  if (seed) {
    const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
    s.secret(key, 32);
    uint32_t* f[2] = {s.secret_scratch<uint32_t>(items * kw), s.secret_scratch<uint32_t>(items * kw)};
    if (!(st = s.st)) st = cki_sample(c, n_bits, batch, K, dn, n_stride, key, first_index, f[0], f[1], dst);
    dsv = f[0]; drv = f[1];
  } else {
    dsv = s.in(sv, items * kw); drv = s.in(rv, items * kw);
    if (!s.dev) { s.secret(dsv, items * kw * 4); s.secret(drv, items * kw * 4); }
    st = s.st;
  }
  if (!st) st = with_group<GA, GB>(group_for_bits(n_bits < 2048 ? 2048 : n_bits), [&](auto G) {
    return cki_challenge_impl<G()>(c, s, n_bits, batch, K, dn, n_stride, dsv, drv, dsn, de, dz, dsd, dst, seed != nullptr);
  });
  return s.finish(st);
}

extern "C" int32_t zkp_correct_key_challenge_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                                   const uint32_t* sv, const uint32_t* rv, uint32_t* out_sn, uint32_t* out_e, uint32_t* out_z,
                                                   uint32_t* out_s_digest, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!cki_args_ok(n_bits, batch, K, flags) || (n_stride != 0 && n_stride != n_bits / 32) || (batch && (!n || !sv || !rv || !out_sn || !out_e || !out_z))) {
    c->err = "zkp_correct_key_challenge_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  ZKP_ROUTE_WHOLE(c, 2 * (uint64_t)K * batch, n_bits < 2048 ? 2048 : n_bits, zkp_correct_key_challenge_batch,       // (the larger launch)
                  n_bits, batch, K, n, n_stride, sv, rv, out_sn, out_e, out_z, out_s_digest, out_status, flags)
  HIPCHK(c, hipSetDevice(c->device));
  return cki_challenge(c, n_bits, batch, K, n, n_stride, sv, rv, nullptr, 0, out_sn, out_e, out_z, out_s_digest, out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_correct_key_challenge_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                                          const uint8_t* seed, uint64_t first_index, uint32_t* out_sn, uint32_t* out_e, uint32_t* out_z,
                                                          uint32_t* out_s_digest, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!cki_args_ok(n_bits, batch, K, flags) || (n_stride != 0 && n_stride != n_bits / 32) || (batch && (!n || !seed || !out_sn || !out_e || !out_z))) {
    c->err = "zkp_correct_key_challenge_seeded_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  ZKP_ROUTE_WHOLE(c, 2 * (uint64_t)K * batch, n_bits < 2048 ? 2048 : n_bits, zkp_correct_key_challenge_seeded_batch,
                  n_bits, batch, K, n, n_stride, seed, first_index, out_sn, out_e, out_z, out_s_digest, out_status, flags)
  HIPCHK(c, hipSetDevice(c->device));
  return cki_challenge(c, n_bits, batch, K, n, n_stride, nullptr, nullptr, seed, first_index, out_sn, out_e, out_z,
                       out_s_digest, out_status, flags);
} ZKP_CATCH(c)

// the verifier's second message: s alone from (seed, first_index + b), its digest, the comparison.  No ladder: the call runs on the ctx that
// receives it; s and its digest never leave the device.
extern "C" int32_t zkp_correct_key_verify_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                                       const uint8_t* seed, uint64_t first_index, const uint32_t* proof_s_digest, uint8_t* out_verdict,
                                                       uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!cki_args_ok(n_bits, batch, K, flags) || (n_stride != 0 && n_stride != n_bits / 32) || (batch && (!n || !seed || !proof_s_digest || !out_verdict))) {
    c->err = "zkp_correct_key_verify_seeded_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t kw = n_bits / 32;
  const uint64_t items = batch * K;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t* dpd = s.in(proof_s_digest, batch * 8);
  uint8_t* dv = s.out(out_verdict, batch);
  const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(key, 32);
  uint32_t *dsv = s.secret_scratch<uint32_t>(items * kw), *dig = s.secret_scratch<uint32_t>(batch * 8);
  uint8_t* dst = s.scratch<uint8_t>(batch);
  int32_t st;
  if ((st = s.st) || (st = cki_sample(c, n_bits, batch, K, dn, n_stride, key, first_index, dsv, nullptr, dst))) return st;
  hipLaunchKernelGGL(k_cki_chal_status, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, c->stream, dn, n_stride, (int)kw, batch, 1, dst);
  if ((st = hash_list(c, batch, {{dsv, (uint64_t)K * kw, kw, kw, K}}, dig))) return st;
  hipLaunchKernelGGL(k_cki_verdict, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t*)dig, dpd, (const uint8_t*)dst, batch, dv);
  HIPCHK(c, hipGetLastError());
  return s.finish();
} ZKP_CATCH(c)

extern "C" int32_t zkp_correct_key_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* p, const uint32_t* q, const uint32_t* sn,
                                               const uint32_t* e, const uint32_t* z, uint32_t* out_s_digest, uint8_t* out_error, uint32_t flags) try {
  constexpr uint32_t MOD_BITS = 2048;                        // the ladder's row, as zkp_correct_key_ni_prove_batch: max(n_bits / 2, 2048)
  if (!c) return ZKP_EINVAL;
  if (!cki_args_ok(n_bits, batch, K, flags) || (batch && (!p || !q || !sn || !e || !z || !out_s_digest))) {
    c->err = "zkp_correct_key_prove_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  const uint64_t items = batch * K, rows = CKI_ROWS * items;
  ZKP_ROUTE_WHOLE(c, rows, MOD_BITS, zkp_correct_key_prove_batch, n_bits, batch, K, p, q, sn, e, z, out_s_digest, out_error, flags)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t hw = n_bits / 64, rw = MOD_BITS / 32;
  const uint32_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dp = s.in(p, batch * hw);
  const uint32_t* dq = s.in(q, batch * hw);
  const uint32_t* dsn = s.in(sn, items * kw);
  const uint32_t* de = s.in(e, batch * 8);
  const uint32_t* dz = s.in(z, items * kw);
  uint32_t* dsd = s.out(out_s_digest, batch * 8);
  uint8_t* derr = s.out(out_error, batch);
  if (!s.dev) { s.secret(dp, batch * hw * 4); s.secret(dq, batch * hw * 4); }
  const LadderRows r = ladder_rows_take(s, rows, rw, hw);    // the bases are the residues of sn and z under p and q
  uint32_t* root = s.secret_scratch<uint32_t>(items * kw);
  // public: n, rn, the digest of (n, sn, rn), the coprimality flags
  uint32_t *dn = s.scratch<uint32_t>(batch * kw), *rn = s.scratch<uint32_t>(items * kw), *echk = s.scratch<uint32_t>(batch * 8);
  uint8_t* share = s.scratch<uint8_t>(3 * items);
  if (s.st) return s.st;
  const int lanes = 16;
  hipLaunchKernelGGL(k_ck_prove_n, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, c->stream, dp, dq, (int)hw, batch, dn);
  HIPCHK(c, hipGetLastError());
  CrtKeys k;
  int32_t st;
  if ((st = crt_keys_prepare(c, s, dp, dq, hw, batch, hw, false, &k))) return st;
  CkiProveSplitArgs sa{dsn, dz, de, dn, dp, dq, k.dp, k.dq, k.kst, r.mods, r.base, r.exps, items, K, (int)hw, (int)rw};
  if ((st = launch_lanes(c, k_cki_prove_split, 2 * items, cki_prove_split_lds_words_per_lane((int)hw), sa))) return st;
  SecretLadder<GA> ladder{c};
  if ((st = ladder.take(s, rows)) || (st = ladder.run(n_bits / 2, rows, r.mods, r.base, r.exps, hw, r.lad))) return st;
  CkiProveFinishArgs fa{r.lad, dp, dq, k.pinv, k.pinv_stride, k.kst, rn, root, items, K, (int)hw, (int)rw};
  hipLaunchKernelGGL(k_cki_prove_finish, dim3((unsigned)((items + lanes - 1) / lanes)), dim3(lanes), lanes * pd_crt_lds_words_per_lane((int)hw) * 4, c->stream, fa);
  hipLaunchKernelGGL(k_cki_prove_gcd, dim3((unsigned)((3 * items + lanes - 1) / lanes)), dim3(lanes), lanes * cki_prove_gcd_lds_words_per_lane((int)kw) * 4, c->stream,
                     dsn, dz, (const uint32_t*)rn, (const uint32_t*)dn, k.kst, items, K, (int)kw, share);
  HIPCHK(c, hipGetLastError());
  if ((st = hash_list(c, batch, {{dn, kw, 0, kw, 1}, {dsn, (uint64_t)K * kw, kw, kw, K}, {rn, (uint64_t)K * kw, kw, kw, K}}, echk))) return st;
  if ((st = hash_list(c, batch, {{root, (uint64_t)K * kw, kw, kw, K}}, dsd))) return st;
  CkiProveMergeArgs ma{share, k.kst, de, echk, dsd, derr, batch, K};
  if ((st = launch_rows(c, k_cki_prove_merge, batch, ma))) return st;
  return s.finish();
} ZKP_CATCH(c)
