// zkp_api_ck_prove.inc — host side of zkp_correct_key_ni_prove_batch (kernels_ck_prove.hpp); included by zkp_api.hip behind
// zkp_api_paillier_dec.inc, whose key preparation and ladder (pdec_ladder: constants records and window tables in blocks of the call,
// registered secret) it runs.  n = p q, the hash kernels of the verifier over the device-resident n, the split into 22 half-width rows per
// key, the ladder, the recombination, all on the ctx stream.  A call that zkp_modexp_batch would hand to a secondary engine for the same
// (rows, mod_bits) goes there WHOLE, as zkp_paillier_open_batch does: one ctx's Stage owns — and wipes — every secret block.

extern "C" int32_t zkp_correct_key_ni_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* p, const uint32_t* q, const uint8_t* salt,
                                                  uint32_t salt_len, uint32_t* out_n, uint32_t* out_sigma, uint8_t* out_status, uint32_t flags) try {
  constexpr uint32_t MOD_BITS = 2048;                        // the ladder's row: max(n_bits / 2, 2048), and 2048 bits is the narrowest group
#ifndef ZKP_SECONDARY_ENGINE
  if (c && batch <= (1ull << 24) && route_latency(c, 2 * ZKP_CORRECT_KEY_M2 * batch, MOD_BITS)) {      // (zkp_modexp_batch's rule for the ladder's rows)
    c->wiped_on = c->lat_ctx == c->eng_ctx[1] ? 1 : 0;
    return lat_forward_plain(c, c->lat->p_zkp_correct_key_ni_prove_batch(c->lat_ctx, n_bits, batch, p, q, salt, salt_len, out_n, out_sigma, out_status, flags));
  }
#endif
  if (!c) return ZKP_EINVAL;
  if (!key_bits_ok(n_bits) || batch > (1ull << 24) || (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || (salt_len && !salt) || (batch && (!p || !q || !out_sigma))) {
    c->err = "zkp_correct_key_ni_prove_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t hw = n_bits / 64, kw = n_bits / 32, rw = MOD_BITS / 32, mw = kw + 8;
  const uint64_t items = batch * ZKP_CORRECT_KEY_M2, rows = 2 * items;
  Stage s(c, flags);
  const uint32_t* dp = s.in(p, batch * hw);
  const uint32_t* dq = s.in(q, batch * hw);
  uint32_t* dn = s.out(out_n, batch * kw);
  uint32_t* dsg = s.out(out_sigma, items * kw);
  uint8_t* dst = s.out(out_status, batch);
  const uint8_t* dsalt = salt_len ? s.host_in(salt, salt_len) : nullptr;     // (a short host byte string in both memory modes)
  if (!s.dev) { s.secret(dp, batch * hw * 4); s.secret(dq, batch * hw * 4); }
  // everything derived from p and q: the inverse kernel's rows, the constants, the ladder's moduli, bases, exponents and results
  auto tmp = [&](size_t words) { uint32_t* b = s.st ? nullptr : (uint32_t*)s.take(words * 4); s.secret(b, words * 4); return b; };
  uint32_t *inv_a = tmp(4 * batch * hw), *inv_m = tmp(4 * batch * hw), *inv = tmp(4 * batch * hw), *dpe = tmp(batch * hw), *dqe = tmp(batch * hw);
  uint32_t *mods = tmp(rows * rw), *base = tmp(rows * rw), *lad = tmp(rows * rw), *exps = tmp(rows * hw);
  // public: n (when the caller does not ask for it), the masks, the hash kernels' primorial verdict (not tested by the prover: no primes given)
  if (!s.st && !dn) dn = (uint32_t*)s.take(batch * kw * 4);
  uint32_t* mgf = s.st ? nullptr : (uint32_t*)s.take(items * mw * 4);
  uint8_t* hash_verdict = s.st ? nullptr : (uint8_t*)s.take(batch);
  uint8_t* inv_st = s.st ? nullptr : (uint8_t*)s.take(4 * batch);
  uint8_t* kst = s.st ? nullptr : (uint8_t*)s.take(batch);
  if (!s.st && !dst) dst = (uint8_t*)s.take(batch);
  int32_t st = s.st;
  const int lanes = 16;                                      // as zkp_paillier_open_batch: one value per lane, small blocks keep divergence local
  const unsigned key_blocks = (unsigned)((batch + lanes - 1) / lanes);
  PdecKeyArgs ka{dp, dq, hw, inv_a, inv_m, inv, inv_st, nullptr, nullptr, dpe, dqe, kst, batch, (int)hw};
  if (!st) {
    hipLaunchKernelGGL(k_ck_prove_n, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, c->stream, dp, dq, (int)hw, batch, dn);
    CkHashArgs h{dn, (uint32_t)kw, batch, dsalt, salt_len, mgf, hash_verdict, nullptr, 0};
    if (batch <= 4ull * (uint64_t)c->route.cus) hipLaunchKernelGGL(k_ck_hash_wave, dim3((unsigned)batch), dim3(64), 0, c->stream, h);     // (ck_verify_impl's rule)
    else hipLaunchKernelGGL(k_ck_hash, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, c->stream, h);
    hipLaunchKernelGGL(k_pdec_key_a, dim3(key_blocks), dim3(lanes), lanes * pdec_key_lds_words_per_lane((int)hw) * 4, c->stream, ka);
    if (hipGetLastError() != hipSuccess) { c->err = "zkp_correct_key_ni_prove_batch: key preparation launch"; st = ZKP_EDEVICE; }
  }
  if (!st) st = launch_modinv(c, 4 * batch, (int)hw, inv_a, hw, inv_m, hw, inv, hw, inv_st);
  if (!st) {
    hipLaunchKernelGGL(k_pdec_key_b, dim3(key_blocks), dim3(lanes), lanes * pdec_key_lds_words_per_lane((int)hw) * 4, c->stream, ka);
    CkProveSplitArgs sa{mgf, dp, dq, dpe, dqe, kst, mods, base, exps, items, (int)hw, (int)rw};
    hipLaunchKernelGGL(k_ck_prove_split, dim3((unsigned)((rows + lanes - 1) / lanes)), dim3(lanes), lanes * ck_prove_split_lds_words_per_lane((int)hw) * 4, c->stream, sa);
    if (hipGetLastError() != hipSuccess || hipMemsetAsync(lad, 0, rows * rw * 4, c->stream) != hipSuccess) { c->err = "zkp_correct_key_ni_prove_batch: split launch"; st = ZKP_EDEVICE; }
  }
  if (!st) st = pdec_ladder<GA>(c, s, n_bits / 2, rows, mods, base, exps, hw, lad);
  if (!st) {
    CkProveFinishArgs fa{lad, dp, dq, inv + hw, 4 * hw, kst, dn, dsg, dst, items, (int)hw, (int)rw};
    hipLaunchKernelGGL(k_ck_prove_finish, dim3((unsigned)((items + lanes - 1) / lanes)), dim3(lanes), lanes * ck_prove_finish_lds_words_per_lane((int)hw) * 4, c->stream, fa);
    if (hipGetLastError() != hipSuccess) { c->err = "k_ck_prove_finish launch"; st = ZKP_EDEVICE; }
  }
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)
