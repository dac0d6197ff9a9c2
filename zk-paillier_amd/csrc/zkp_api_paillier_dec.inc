// zkp_api_paillier_dec.inc — what the calls that hold p and q share (SecretLadder, crt_keys_prepare, ladder_rows_take) and the host side of
// zkp_paillier_open_batch (kernels_paillier_dec.hpp); included by zkp_api.hip.  The open: key preparation, the split, the ladder and the
// finish, all on the ctx stream.  Such a call goes to ONE engine whole (ZKP_ROUTE_WHOLE), and every block derived from p or q is taken with
// Stage::secret_scratch: the Stage of the ctx that runs the call wipes it on every path out.

// The ladder under secret moduli.  Here they are p^2, q^2, p and q (or prime candidates): k_setup stores them, R^2 mod p and the rest of the
// Montgomery record in the constants buffer, and the ladder fills the window tables with powers of c mod p^2 (gcd(c - (c mod p^2), n) = p).
// Every other caller of run_setup passes public moduli and uses the ctx's own persistent buffers; here both are blocks of the call's Stage,
// registered secret: the constants block is what run_setup and modexp_core are given, the table block stands in for c->table for the length
// of a run.  The ctx's own buffers — the cached record of a key among them — are untouched.  take() sizes the two blocks for the most rows
// any run of the call has (both sizes grow with the rows).
template <int G>
struct SecretLadder {
  zkp_ctx* c; void* cp = nullptr; void* tp = nullptr; size_t cbytes = 0, tbytes = 0;
  int32_t take(Stage& s, uint64_t max_rows) {
    unsigned blocks = 0;
    cbytes = max_rows * ConstLayout<G>::WORDS * sizeof(uint32_t);          // (what run_setup and modexp_core ask ensure() for)
    tbytes = table_bytes<G>(c, k_modexp<G, false>, max_rows, &blocks);
    cp = s.secret_scratch<char>(cbytes);
    tp = s.secret_scratch<char>(tbytes);
    return s.st;
  }
  int32_t run(uint32_t exp_bits, uint64_t rows, const uint32_t* mods, const uint32_t* base, const uint32_t* exps, uint64_t exp_stride, uint32_t* out) {
    // (the constants are an argument of both launchers; the window tables are the ctx's, so that block is swapped in)
    struct Borrowed {
      zkp_ctx* c; DevBuf table;
      Borrowed(zkp_ctx* c_, void* tp, size_t tbytes) : c(c_) { table.p = tp; table.cap = tbytes; std::swap(c->table, table); }
      Borrowed(const Borrowed&) = delete;
      Borrowed& operator=(const Borrowed&) = delete;
      ~Borrowed() { std::swap(c->table, table); }
    } borrowed(c, tp, tbytes);
    DevBuf consts;
    consts.p = cp; consts.cap = cbytes;
    using LL = LdsLayout<G>;
    int32_t st;
    if ((st = run_setup<G>(c, mods, LL::NW, LL::NW, 0, rows, consts))) return st;
    return modexp_core<G>(c, consts, exp_bits, rows, base, exps, exp_stride, true, out, LL::NW);
  }
};

// The CRT constants of nkeys keys (p, q) on the device: rows 4 k .. 4 k + 3 of inv are key k's four inverses (k_pdec_key_a), pinv = p^-1 mod q
// is row 1 of them; d_p = q^-1 mod (p - 1), d_q alike; h_p, h_q (the open's L-multipliers) when asked for; kst 0 | 2 per key.
struct CrtKeys {
  const uint32_t* inv; const uint32_t* pinv; uint64_t pinv_stride;
  const uint32_t* dp; const uint32_t* dq; const uint32_t* hp; const uint32_t* hq;
  const uint8_t* kst;
};
// Takes the blocks — all secret but the two status arrays — and enqueues k_pdec_key_a, the inverse kernel over its 4 nkeys rows and k_pdec_key_b.
static int32_t crt_keys_prepare(zkp_ctx* c, Stage& s, const uint32_t* dp, const uint32_t* dq, uint64_t key_stride, uint64_t nkeys, size_t hw, bool want_h,
                                CrtKeys* out) {
  uint32_t *inv_a = s.secret_scratch<uint32_t>(4 * nkeys * hw), *inv_m = s.secret_scratch<uint32_t>(4 * nkeys * hw), *inv = s.secret_scratch<uint32_t>(4 * nkeys * hw);
  uint32_t *hp = want_h ? s.secret_scratch<uint32_t>(nkeys * hw) : nullptr, *hq = want_h ? s.secret_scratch<uint32_t>(nkeys * hw) : nullptr;
  uint32_t *dpe = s.secret_scratch<uint32_t>(nkeys * hw), *dqe = s.secret_scratch<uint32_t>(nkeys * hw);
  uint8_t *inv_st = s.scratch<uint8_t>(4 * nkeys), *kst = s.scratch<uint8_t>(nkeys);
  if (s.st) return s.st;
  PdecKeyArgs ka{dp, dq, key_stride, inv_a, inv_m, inv, inv_st, hp, hq, dpe, dqe, kst, nkeys, (int)hw};
  int32_t st;
  if ((st = launch_lanes(c, k_pdec_key_a, nkeys, pdec_key_lds_words_per_lane((int)hw), ka))) return st;
  if ((st = launch_modinv(c, 4 * nkeys, (int)hw, inv_a, hw, inv_m, hw, inv, hw, inv_st))) return st;
  if ((st = launch_lanes(c, k_pdec_key_b, nkeys, pdec_key_lds_words_per_lane((int)hw), ka))) return st;
  *out = CrtKeys{inv, inv + hw, 4 * hw, dpe, dqe, hp, hq, kst};
  return ZKP_OK;
}

// The ladder's rows of a call: moduli, bases and results of rw words, exponents of hw words — all secret.  A row narrower than rw is
// zero-padded: the split kernels pad what they write, the results start out zero.
struct LadderRows { uint32_t* mods; uint32_t* base; uint32_t* lad; uint32_t* exps; };
static LadderRows ladder_rows_take(Stage& s, uint64_t rows, size_t rw, size_t hw) {
  LadderRows r{s.secret_scratch<uint32_t>(rows * rw), s.secret_scratch<uint32_t>(rows * rw), s.secret_scratch<uint32_t>(rows * rw), s.secret_scratch<uint32_t>(rows * hw)};
  if (!s.st && hipMemsetAsync(r.lad, 0, rows * rw * 4, s.c->stream) != hipSuccess) { s.st = ZKP_EDEVICE; s.c->err = "ladder rows: zero-fill"; }
  return r;
}

extern "C" int32_t zkp_paillier_open_batch(zkp_ctx* c, uint32_t n_bits, uint64_t count, const uint32_t* p, const uint32_t* q, uint64_t key_stride,
                                           const uint32_t* ct, uint32_t* out_m, uint32_t* out_r, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  const size_t hw = n_bits / 64, kw = n_bits / 32;
  if (!key_bits_ok(n_bits) || (key_stride != 0 && key_stride != hw) || count > (1ull << 24) || (count && (!p || !q || !ct || !out_m))) {
    c->err = "zkp_paillier_open_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (count == 0) return ZKP_OK;
  const uint32_t mod_bits = n_bits < 2048 ? 2048 : n_bits;   // the ladder's row: a modulus of n_bits (p^2, q^2), zero-padded at n_bits == 1024
  const uint64_t nkeys = key_stride ? count : 1, rows = (out_r ? 4 : 2) * count;
  ZKP_ROUTE_WHOLE(c, rows, mod_bits, zkp_paillier_open_batch, n_bits, count, p, q, key_stride, ct, out_m, out_r, out_status, flags)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t rw = mod_bits / 32;
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
  uint32_t *p2 = s.secret_scratch<uint32_t>(nkeys * kw), *q2 = s.secret_scratch<uint32_t>(nkeys * kw);
  const LadderRows r = ladder_rows_take(s, rows, rw, hw);
  if (!dst) dst = s.scratch<uint8_t>(count);
  if (s.st) return s.st;
  hipLaunchKernelGGL(k_square_words, dim3((unsigned)((nkeys + 63) / 64)), dim3(64), 0, c->stream, dp, key_stride, (int)hw, nkeys, p2);
  hipLaunchKernelGGL(k_square_words, dim3((unsigned)((nkeys + 63) / 64)), dim3(64), 0, c->stream, dq, key_stride, (int)hw, nkeys, q2);
  HIPCHK(c, hipGetLastError());
  CrtKeys k;
  int32_t st;
  if ((st = crt_keys_prepare(c, s, dp, dq, key_stride, nkeys, hw, true, &k))) return st;
  PdecSplitArgs sa{dc, dp, dq, key_stride, p2, q2, k.dp, k.dq, k.kst, r.mods, r.base, r.exps, count, (int)hw, (int)rw, out_r ? 1 : 0};
  if ((st = launch_lanes(c, k_pdec_split, 2 * count, pdec_split_lds_words_per_lane((int)hw), sa))) return st;
  st = with_group<GA, GB>(group_for_bits(mod_bits), [&](auto G) {
    SecretLadder<G()> ladder{c};
    const int32_t e = ladder.take(s, rows);
    return e ? e : ladder.run(n_bits / 2, rows, r.mods, r.base, r.exps, hw, r.lad);
  });
  if (st) return st;
  PdecFinishArgs fa{r.lad, dp, dq, key_stride, k.hp, k.hq, k.pinv, k.pinv_stride, k.kst, dm, dr, dst, count, (int)hw, (int)rw};
  if ((st = launch_lanes(c, k_pdec_finish, count, pd_crt_lds_words_per_lane((int)hw), fa))) return st;
  return s.finish();
} ZKP_CATCH(c)
