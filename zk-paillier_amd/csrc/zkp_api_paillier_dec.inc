// zkp_api_paillier_dec.inc — host side of zkp_paillier_open_batch (kernels_paillier_dec.hpp); included by zkp_api.hip.  Key preparation
// (k_pdec_key_a, launch_modinv, k_pdec_key_b), the split, the ladder (run_setup under per-item moduli, modexp_core) and the finish, all on
// the ctx stream.  A call that zkp_modexp_batch would hand to a secondary engine for the same (rows, mod_bits) goes there WHOLE, so every
// block that holds a secret belongs to the ONE ctx that runs the call and is wiped by that ctx's Stage.

// The ladder's moduli are p^2, q^2, p and q: k_setup stores them, R^2 mod p and the rest of the Montgomery record in the constants buffer,
// and the ladder fills the window tables with powers of c mod p^2 (gcd(c - (c mod p^2), n) = p).  Every other caller of run_setup passes
// public moduli and uses the ctx's own persistent buffers; here both are blocks of this call's Stage, registered secret, that stand in for
// c->consts and c->table for the length of the ladder.  The ctx's own buffers — the cached record of a key among them — are untouched.
struct PdecBorrowedBufs {
  zkp_ctx* c; DevBuf consts, table;
  PdecBorrowedBufs(zkp_ctx* c_, void* cp, size_t cbytes, void* tp, size_t tbytes) : c(c_) {
    consts.p = cp; consts.cap = cbytes; table.p = tp; table.cap = tbytes;
    std::swap(c->consts, consts); std::swap(c->table, table);
  }
  PdecBorrowedBufs(const PdecBorrowedBufs&) = delete;
  PdecBorrowedBufs& operator=(const PdecBorrowedBufs&) = delete;
  ~PdecBorrowedBufs() { std::swap(c->consts, consts); std::swap(c->table, table); }
};

template <int G>
static int32_t pdec_ladder(zkp_ctx* c, Stage& s, uint32_t exp_bits, uint64_t rows, const uint32_t* mods, const uint32_t* base, const uint32_t* exps,
                           uint64_t exp_stride, uint32_t* out) {
  using CL = ConstLayout<G>;
  using LL = LdsLayout<G>;
  unsigned blocks = 0;
  const size_t cbytes = rows * CL::WORDS * sizeof(uint32_t), tbytes = table_bytes<G>(c, k_modexp<G, false>, rows, &blocks);   // (what run_setup and modexp_core ask ensure() for)
  void* cp = s.take(cbytes);
  void* tp = s.st ? nullptr : s.take(tbytes);
  if (s.st) return s.st;
  s.secret(cp, cbytes); s.secret(tp, tbytes);
  PdecBorrowedBufs borrowed(c, cp, cbytes, tp, tbytes);
  int32_t st;
  if ((st = run_setup<G>(c, mods, LL::NW, LL::NW, 0, rows, c->consts))) return st;
  return modexp_core<G>(c, exp_bits, rows, base, exps, exp_stride, true, out, LL::NW);
}

extern "C" int32_t zkp_paillier_open_batch(zkp_ctx* c, uint32_t n_bits, uint64_t count, const uint32_t* p, const uint32_t* q, uint64_t key_stride,
                                           const uint32_t* ct, uint32_t* out_m, uint32_t* out_r, uint8_t* out_status, uint32_t flags) try {
#ifndef ZKP_SECONDARY_ENGINE
  if (c && route_latency(c, (out_r ? 4 : 2) * count, n_bits < 2048 ? 2048 : n_bits)) {       // (zkp_modexp_batch's rule for the ladder's rows)
    c->wiped_on = c->lat_ctx == c->eng_ctx[1] ? 1 : 0;
    return lat_forward_plain(c, c->lat->p_zkp_paillier_open_batch(c->lat_ctx, n_bits, count, p, q, key_stride, ct, out_m, out_r, out_status, flags));
  }
#endif
  if (!c) return ZKP_EINVAL;
  const size_t hw = n_bits / 64, kw = n_bits / 32;
  if (!key_bits_ok(n_bits) || (key_stride != 0 && key_stride != hw) || count > (1ull << 24) || (count && (!p || !q || !ct || !out_m))) {
    c->err = "zkp_paillier_open_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (count == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t mod_bits = n_bits < 2048 ? 2048 : n_bits;   // the ladder's row: a modulus of n_bits (p^2, q^2), zero-padded at n_bits == 1024
  const size_t rw = mod_bits / 32;
  const uint64_t nkeys = key_stride ? count : 1, rows = (out_r ? 4 : 2) * count;
  Stage s(c, flags);
  const uint32_t* dp = s.in(p, nkeys * hw);
  const uint32_t* dq = s.in(q, nkeys * hw);
  const uint32_t* dc = s.in(ct, count * 2 * kw);
  uint32_t* dm = s.out(out_m, count * kw);
  uint32_t* dr = s.out(out_r, count * kw);
  uint8_t* dst = s.out(out_status, count);
  if (!s.dev) {                                              // (host arrays: the staged copies are wiped behind the D2H)
    s.secret(dp, nkeys * hw * 4); s.secret(dq, nkeys * hw * 4); s.secret(dm, count * kw * 4); s.secret(dr, count * kw * 4);
  }
  // everything derived from p and q: the inverse kernel's rows, the constants, the ladder's moduli, bases, exponents and results
  auto tmp = [&](size_t words) { uint32_t* b = s.st ? nullptr : (uint32_t*)s.take(words * 4); s.secret(b, words * 4); return b; };
  uint32_t *inv_a = tmp(4 * nkeys * hw), *inv_m = tmp(4 * nkeys * hw), *inv = tmp(4 * nkeys * hw);
  uint32_t *p2 = tmp(nkeys * kw), *q2 = tmp(nkeys * kw), *hp = tmp(nkeys * hw), *hq = tmp(nkeys * hw), *dpe = tmp(nkeys * hw), *dqe = tmp(nkeys * hw);
  uint32_t *mods = tmp(rows * rw), *base = tmp(rows * rw), *lad = tmp(rows * rw), *exps = tmp(rows * hw);
  uint8_t* inv_st = s.st ? nullptr : (uint8_t*)s.take(4 * nkeys);
  uint8_t* kst = s.st ? nullptr : (uint8_t*)s.take(nkeys);
  if (!s.st && !dst) dst = (uint8_t*)s.take(count);
  int32_t st = s.st;
  const int lanes = 16;                                      // as launch_modinv: one value per lane, small blocks keep divergence local
  const unsigned key_blocks = (unsigned)((nkeys + lanes - 1) / lanes), item_blocks = (unsigned)((count + lanes - 1) / lanes);
  PdecKeyArgs ka{dp, dq, key_stride, inv_a, inv_m, inv, inv_st, hp, hq, dpe, dqe, kst, nkeys, (int)hw};
  if (!st) {
    hipLaunchKernelGGL(k_square_words, dim3((unsigned)((nkeys + 63) / 64)), dim3(64), 0, c->stream, dp, key_stride, (int)hw, nkeys, p2);
    hipLaunchKernelGGL(k_square_words, dim3((unsigned)((nkeys + 63) / 64)), dim3(64), 0, c->stream, dq, key_stride, (int)hw, nkeys, q2);
    hipLaunchKernelGGL(k_pdec_key_a, dim3(key_blocks), dim3(lanes), lanes * pdec_key_lds_words_per_lane((int)hw) * 4, c->stream, ka);
    HIPCHK(c, hipGetLastError());
    st = launch_modinv(c, 4 * nkeys, (int)hw, inv_a, hw, inv_m, hw, inv, hw, inv_st);
  }
  if (!st) {
    hipLaunchKernelGGL(k_pdec_key_b, dim3(key_blocks), dim3(lanes), lanes * pdec_key_lds_words_per_lane((int)hw) * 4, c->stream, ka);
    PdecSplitArgs sa{dc, dp, dq, key_stride, p2, q2, dpe, dqe, kst, mods, base, exps, count, (int)hw, (int)rw, out_r ? 1 : 0};
    hipLaunchKernelGGL(k_pdec_split, dim3((unsigned)((2 * count + lanes - 1) / lanes)), dim3(lanes), lanes * pdec_split_lds_words_per_lane((int)hw) * 4, c->stream, sa);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(lad, 0, rows * rw * 4, c->stream));
    st = with_group<GA, GB>(group_for_bits(mod_bits), [&](auto G) { return pdec_ladder<G()>(c, s, n_bits / 2, rows, mods, base, exps, hw, lad); });
  }
  if (!st) {
    PdecFinishArgs fa{lad, dp, dq, key_stride, hp, hq, inv + hw, 4 * hw, kst, dm, dr, dst, count, (int)hw, (int)rw};
    hipLaunchKernelGGL(k_pdec_finish, dim3(item_blocks), dim3(lanes), lanes * pdec_finish_lds_words_per_lane((int)hw) * 4, c->stream, fa);
    if (hipGetLastError() != hipSuccess) { c->err = "k_pdec_finish launch"; st = ZKP_EDEVICE; }
  }
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)
