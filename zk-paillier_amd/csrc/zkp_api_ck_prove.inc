// zkp_api_ck_prove.inc — host side of zkp_correct_key_ni_prove_batch (kernels_ck_prove.hpp); included by zkp_api.hip behind
// zkp_api_paillier_dec.inc, whose shared pieces it runs: crt_keys_prepare, ladder_rows_take, SecretLadder.  n = p q, the hash kernels of the
// verifier over the device-resident n, the split into 22 half-width rows per key, the ladder, the recombination, all on the ctx stream.

extern "C" int32_t zkp_correct_key_ni_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* p, const uint32_t* q, const uint8_t* salt,
                                                  uint32_t salt_len, uint32_t* out_n, uint32_t* out_sigma, uint8_t* out_status, uint32_t flags) try {
  constexpr uint32_t MOD_BITS = 2048;                        // the ladder's row: max(n_bits / 2, 2048), and 2048 bits is the narrowest group
  if (!c) return ZKP_EINVAL;
  if (!key_bits_ok(n_bits) || batch > (1ull << 24) || (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || (salt_len && !salt) || (batch && (!p || !q || !out_sigma))) {
    c->err = "zkp_correct_key_ni_prove_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  const uint64_t items = batch * ZKP_CORRECT_KEY_M2, rows = 2 * items;
  ZKP_ROUTE_WHOLE(c, rows, MOD_BITS, zkp_correct_key_ni_prove_batch, n_bits, batch, p, q, salt, salt_len, out_n, out_sigma, out_status, flags)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t hw = n_bits / 64, kw = n_bits / 32, rw = MOD_BITS / 32, mw = kw + 8;
  Stage s(c, flags);
  const uint32_t* dp = s.in(p, batch * hw);
  const uint32_t* dq = s.in(q, batch * hw);
  uint32_t* dn = s.out(out_n, batch * kw);
  uint32_t* dsg = s.out(out_sigma, items * kw);
  uint8_t* dst = s.out(out_status, batch);
  const uint8_t* dsalt = salt_len ? s.host_in(salt, salt_len) : nullptr;     // (a short host byte string in both memory modes)
  if (!s.dev) { s.secret(dp, batch * hw * 4); s.secret(dq, batch * hw * 4); }
  const LadderRows r = ladder_rows_take(s, rows, rw, hw);
  // public: n (when the caller does not ask for it), the masks, the hash kernels' primorial verdict (not tested by the prover: no primes given)
  if (!dn) dn = s.scratch<uint32_t>(batch * kw);
  uint32_t* mgf = s.scratch<uint32_t>(items * mw);
  uint8_t* hash_verdict = s.scratch<uint8_t>(batch);
  if (!dst) dst = s.scratch<uint8_t>(batch);
  if (s.st) return s.st;
  hipLaunchKernelGGL(k_ck_prove_n, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, c->stream, dp, dq, (int)hw, batch, dn);
  CkHashArgs h{dn, (uint32_t)kw, batch, dsalt, salt_len, mgf, hash_verdict, nullptr, 0};
  if (batch <= 4ull * (uint64_t)c->route.cus) hipLaunchKernelGGL(k_ck_hash_wave, dim3((unsigned)batch), dim3(64), 0, c->stream, h);     // (ck_verify_impl's rule)
  else hipLaunchKernelGGL(k_ck_hash, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, c->stream, h);
  HIPCHK(c, hipGetLastError());
  CrtKeys k;
  int32_t st;
  if ((st = crt_keys_prepare(c, s, dp, dq, hw, batch, hw, false, &k))) return st;
  CkProveSplitArgs sa{mgf, dp, dq, k.dp, k.dq, k.kst, r.mods, r.base, r.exps, items, (int)hw, (int)rw};
  if ((st = launch_lanes(c, k_ck_prove_split, rows, ck_prove_split_lds_words_per_lane((int)hw), sa))) return st;
  SecretLadder<GA> ladder{c};
  if ((st = ladder.take(s, rows)) || (st = ladder.run(n_bits / 2, rows, r.mods, r.base, r.exps, hw, r.lad))) return st;
  CkProveFinishArgs fa{r.lad, dp, dq, k.pinv, k.pinv_stride, k.kst, dn, dsg, dst, items, (int)hw, (int)rw};
  if ((st = launch_lanes(c, k_ck_prove_finish, items, pd_crt_lds_words_per_lane((int)hw), fa))) return st;
  return s.finish();
} ZKP_CATCH(c)
