// zkp_api_mul.inc — host side of zkp_modinv_batch, MulProof and CorrectMessageProof (SURVEY §8(f) rank 4);
// included by zkp_api.hip.  Compositions of k_enc / k_modexp / k_modmul with the kernels of kernels_inv.hpp.

static int32_t launch_modinv(zkp_ctx* c, uint64_t count, int kw, const uint32_t* a, uint64_t a_stride, const uint32_t* mod, uint64_t mod_stride,
                             uint32_t* out, uint64_t out_stride, uint8_t* status) {
  // The kernel is latency bound (dependent LDS / carry chains, data-dependent branches): small blocks of `lanes` items
  // (five operand arrays per lane in LDS) let several wavefronts share a CU and keep divergence local.
  int lanes = 16;
  while (lanes * modinv_lds_words_per_lane(kw) * 4 > 96 * 1024) lanes >>= 1;
  const size_t lds = lanes * modinv_lds_words_per_lane(kw) * 4;
  ModinvArgs args{a, a_stride, mod, mod_stride, out, out_stride, status, count, kw};
  hipLaunchKernelGGL(k_modinv, dim3((unsigned)((count + lanes - 1) / lanes)), dim3(lanes), lds, c->stream, args);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

extern "C" int32_t zkp_modinv_batch(zkp_ctx* c, uint32_t mod_bits, uint64_t count, const uint32_t* a, const uint32_t* modulus, uint64_t mod_stride,
                                    uint32_t* out, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (count == 0) return ZKP_OK;
  const uint64_t kw = mod_bits / 32;
  if (!a || !modulus || !out || !out_status || (mod_bits != 2048 && mod_bits != 4096 && mod_bits != 8192) || (mod_stride != 0 && mod_stride != kw) ||
      count > (1ull << 31)) { c->err = "zkp_modinv_batch: invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  const uint32_t* da = s.in(a, count * kw);
  const uint32_t* dm = s.in(modulus, mod_stride ? count * kw : kw);
  uint32_t* dout = s.out(out, count * kw);
  uint8_t* dst = s.out(out_status, count);
  int32_t st = s.st;
  if (!st) st = launch_modinv(c, count, (int)kw, da, kw, dm, mod_stride, dout, kw, dst);
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)

// n^2 as 32-bit words for the inverse kernel (ctx scratch S_MP_NN): [keys][2kw]
static int32_t square_words(zkp_ctx* c, const uint32_t* n, uint64_t n_stride, int kw, uint64_t nkeys, const uint32_t** out) {
  int32_t st;
  if ((st = ensure(c, c->scratch[S_MP_NN], nkeys * 2 * kw * 4))) return st;
  hipLaunchKernelGGL(k_square_words, dim3((unsigned)((nkeys + 63) / 64)), dim3(64), 0, c->stream, n, n_stride, kw, nkeys, (uint32_t*)c->scratch[S_MP_NN].p);
  HIPCHK(c, hipGetLastError());
  *out = (const uint32_t*)c->scratch[S_MP_NN].p;
  return ZKP_OK;
}

static int32_t hash_list(zkp_ctx* c, uint64_t batch, std::initializer_list<HashOp> ops, uint32_t* e) {
  HashListArgs h{};
  for (const HashOp& o : ops) h.op[h.nops++] = o;
  h.batch = batch; h.e = e;
  hipLaunchKernelGGL(k_hash_list, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, c->stream, h);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

struct MulBufs { uint32_t* t[10]; uint8_t* invst; uint32_t* e; };
static int32_t mul_bufs(zkp_ctx* c, uint64_t batch, uint32_t kw, MulBufs* b) {
  int32_t st;
  for (int k = 0; k < 10; k++) { if ((st = ensure(c, c->scratch[S_MP_T0 + k], batch * 2 * kw * 4))) return st; b->t[k] = (uint32_t*)c->scratch[S_MP_T0 + k].p; }
  if ((st = ensure(c, c->scratch[S_MP_INVST], batch))) return st;
  if ((st = ensure(c, c->scratch[S_E], batch * 32))) return st;
  b->invst = (uint8_t*)c->scratch[S_MP_INVST].p; b->e = (uint32_t*)c->scratch[S_E].p;
  return ZKP_OK;
}

// multiplication_proof.rs:60-104
template <int G>
static int32_t mul_prove_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a, const uint32_t* e_b,
                              const uint32_t* e_c, const uint32_t* a, const uint32_t* b, const uint32_t* r_a, const uint32_t* r_b, const uint32_t* r_c,
                              const uint32_t* d, const uint32_t* r_d, uint32_t* f, uint32_t* z1, uint32_t* z2, uint32_t* e_d, uint32_t* e_db, uint8_t* status) {
  using CL = ConstLayout<G>;
  constexpr int GN = N_GROUP<G>;
  const uint32_t kw = n_bits / 32;
  const uint64_t nkeys = n_stride ? B : 1;
  const bool per = n_stride != 0;
  int32_t st;
  MulBufs q;
  if ((st = mul_bufs(c, B, kw, &q))) return st;
  if ((st = run_setup<G>(c, n, n_stride, (int)kw, 1, nkeys, c->consts))) return st;       // modulus n^2
  if ((st = run_setup<GN>(c, n, n_stride, (int)kw, 0, nkeys, c->consts2))) return st;     // modulus n
  const uint32_t* nn = nullptr;
  if ((st = square_words(c, n, n_stride, (int)kw, nkeys, &nn))) return st;
  uint32_t *rdb = q.t[0], *db = q.t[1], *t2 = q.t[2], *t3 = q.t[3], *t4 = q.t[4], *t5 = q.t[5], *ea = q.t[6], *dred = q.t[7];
  if ((st = enc_launch<G>(c, n_bits, B, n, n_stride, d, (int)kw, r_d, (int)kw, e_d))) return st;                       // e_d = Enc(d, r_d) :63-68
  if ((st = modmul_ctx<G>(c, c->consts, per, B, r_d, (int)kw, r_b, (int)kw, rdb, (int)(2 * kw)))) return st;          // r_db = r_d * r_b :69 (< n^2: exact)
  if ((st = modmul_ctx<G>(c, c->consts, per, B, d, (int)kw, b, (int)kw, db, (int)(2 * kw)))) return st;               // db = d * b :70
  if ((st = enc_launch<G>(c, n_bits, B, n, n_stride, db, (int)(2 * kw), rdb, (int)(2 * kw), e_db))) return st;         // e_db :71-76
  if ((st = hash_list(c, B, {{n, n_stride, 0, kw, 1}, {e_a, 2 * kw, 0, 2 * kw, 1}, {e_b, 2 * kw, 0, 2 * kw, 1}, {e_c, 2 * kw, 0, 2 * kw, 1},
                             {e_d, 2 * kw, 0, 2 * kw, 1}, {e_db, 2 * kw, 0, 2 * kw, 1}}, q.e))) return st;              // e :77-84
  if ((st = modmul_ctx<GN>(c, c->consts2, per, B, q.e, 8, a, (int)kw, ea, (int)kw))) return st;                       // e*a mod n :87
  if ((st = modmul_ctx<GN>(c, c->consts2, per, B, d, (int)kw, nullptr, (int)kw, dred, (int)kw))) return st;                 // d mod n
  hipLaunchKernelGGL(k_modadd, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, ea, dred, n, n_stride, (int)kw, B, f);   // f :88
  HIPCHK(c, hipGetLastError());
  // r_a^e (:89), r_c^e (:92) and r_b^f (:91) are independent of each other: one launch, their chains side by side
  if ((st = modexp_multi<G>(c, B, per, {{256, r_a, q.e, 8, t2, (int)kw, (int)(2 * kw)}, {256, r_c, q.e, 8, t3, (int)kw, (int)(2 * kw)},
                                        {n_bits, r_b, f, kw, t5, (int)kw, (int)(2 * kw)}}))) return st;
  if ((st = modmul_ctx<G>(c, c->consts, per, B, t2, (int)(2 * kw), r_d, (int)kw, z1, (int)(2 * kw)))) return st;      // z1 :90
  if ((st = modmul_ctx<G>(c, c->consts, per, B, rdb, (int)(2 * kw), t3, (int)(2 * kw), t3, (int)(2 * kw)))) return st; // r_db * r_c^e :93
  if ((st = launch_modinv(c, B, (int)(2 * kw), t3, 2 * kw, nn, per ? 2 * kw : 0, t4, 2 * kw, q.invst))) return st;    // mod_inv :95
  if ((st = modmul_ctx<G>(c, c->consts, per, B, t5, (int)(2 * kw), t4, (int)(2 * kw), z2, (int)(2 * kw)))) return st; // z2 :96
  MulFinishArgs fa{q.invst, (const uint32_t*)c->consts.p, per ? (uint64_t)CL::WORDS : 0, CL::OFF_ST, (int)kw, B, f, z1, z2, status};
  hipLaunchKernelGGL(k_mul_finish, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, fa);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

// multiplication_proof.rs:106-146
template <int G>
static int32_t mul_verify_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a, const uint32_t* e_b,
                               const uint32_t* e_c, const uint32_t* f, const uint32_t* z1, const uint32_t* z2, const uint32_t* e_d, const uint32_t* e_db,
                               uint8_t* verdict) {
  using CL = ConstLayout<G>;
  const uint32_t kw = n_bits / 32;
  const uint64_t nkeys = n_stride ? B : 1;
  const bool per = n_stride != 0;
  int32_t st;
  MulBufs q;
  if ((st = mul_bufs(c, B, kw, &q))) return st;
  if ((st = run_setup<G>(c, n, n_stride, (int)kw, 1, nkeys, c->consts))) return st;
  const uint32_t* nn = nullptr;
  if ((st = square_words(c, n, n_stride, (int)kw, nkeys, &nn))) return st;
  uint32_t *c1 = q.t[0], *c2 = q.t[1], *l1 = q.t[2], *t3 = q.t[3], *t4 = q.t[4], *l2 = q.t[5];
  if ((st = hash_list(c, B, {{n, n_stride, 0, kw, 1}, {e_a, 2 * kw, 0, 2 * kw, 1}, {e_b, 2 * kw, 0, 2 * kw, 1}, {e_c, 2 * kw, 0, 2 * kw, 1},
                             {e_d, 2 * kw, 0, 2 * kw, 1}, {e_db, 2 * kw, 0, 2 * kw, 1}}, q.e))) return st;              // e :107-114
  if ((st = enc_launch<G>(c, n_bits, B, n, n_stride, f, (int)kw, z1, (int)(2 * kw), c1))) return st;                   // Enc(f, z1) :116-122
  if ((st = enc_launch<G>(c, n_bits, B, n, n_stride, nullptr, -1, z2, (int)(2 * kw), c2))) return st;                  // Enc(0, z2) :123-129
  // e_a^e (:131), e_c^e (:133) and e_b^f (:136): one launch
  if ((st = modexp_multi<G>(c, B, per, {{256, e_a, q.e, 8, l1, (int)(2 * kw), 0}, {256, e_c, q.e, 8, t3, (int)(2 * kw), 0},
                                        {n_bits, e_b, f, kw, l2, (int)(2 * kw), 0}}))) return st;
  if ((st = modmul_ctx<G>(c, c->consts, per, B, l1, (int)(2 * kw), e_d, (int)(2 * kw), l1, (int)(2 * kw)))) return st; // * e_d :132
  if ((st = modmul_ctx<G>(c, c->consts, per, B, e_db, (int)(2 * kw), t3, (int)(2 * kw), t3, (int)(2 * kw)))) return st; // e_db * e_c^e :134
  if ((st = launch_modinv(c, B, (int)(2 * kw), t3, 2 * kw, nn, per ? 2 * kw : 0, t4, 2 * kw, q.invst))) return st;    // mod_inv :135
  if ((st = modmul_ctx<G>(c, c->consts, per, B, l2, (int)(2 * kw), t4, (int)(2 * kw), l2, (int)(2 * kw)))) return st; // :137
  MulVerdictArgs va{l1, c1, l2, c2, q.invst, (const uint32_t*)c->consts.p, per ? (uint64_t)CL::WORDS : 0, CL::OFF_ST, 2 * kw, B, verdict};
  hipLaunchKernelGGL(k_mul_verdict, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, va);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

extern "C" int32_t zkp_mul_proof_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a,
                                             const uint32_t* e_b, const uint32_t* e_c, const uint32_t* a, const uint32_t* b, const uint32_t* r_a,
                                             const uint32_t* r_b, const uint32_t* r_c, const uint32_t* d, const uint32_t* r_d, uint32_t* out_f,
                                             uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_e_d, uint32_t* out_e_db, uint8_t* out_status, uint32_t flags) try {
  ZKP_ROUTE(c, 3 * batch, 2 * n_bits, zkp_mul_proof_prove_batch, n_bits, batch, n, n_stride, e_a, e_b, e_c, a, b, r_a, r_b, r_c, d, r_d, out_f, out_z1, out_z2, out_e_d, out_e_db, out_status, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !e_a || !e_b || !e_c || !a || !b || !r_a || !r_b || !r_c || !d || !r_d || !out_f || !out_z1 || !out_z2 ||
      !out_e_d || !out_e_db || !out_status) { c->err = "zkp_mul_proof_prove_batch: invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dea = s.in(e_a, batch * 2 * kw), *deb = s.in(e_b, batch * 2 * kw), *dec = s.in(e_c, batch * 2 * kw);
  const uint32_t *da = s.in(a, batch * kw), *db = s.in(b, batch * kw), *dra = s.in(r_a, batch * kw), *drb = s.in(r_b, batch * kw), *drc = s.in(r_c, batch * kw);
  const uint32_t *dd = s.in(d, batch * kw), *drd = s.in(r_d, batch * kw);
  uint32_t* df = s.out(out_f, batch * kw);
  uint32_t *dz1 = s.out(out_z1, batch * 2 * kw), *dz2 = s.out(out_z2, batch * 2 * kw), *ded = s.out(out_e_d, batch * 2 * kw), *dedb = s.out(out_e_db, batch * 2 * kw);
  uint8_t* dst = s.out(out_status, batch);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return mul_prove_impl<G()>(c, n_bits, batch, dn, n_stride, dea, deb, dec, da, db, dra, drb, drc, dd, drd, df, dz1, dz2, ded, dedb, dst); });
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)

extern "C" int32_t zkp_mul_proof_verify_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a,
                                              const uint32_t* e_b, const uint32_t* e_c, const uint32_t* f, const uint32_t* z1, const uint32_t* z2,
                                              const uint32_t* e_d, const uint32_t* e_db, uint8_t* out_verdict, uint32_t flags) try {
  ZKP_ROUTE(c, 3 * batch, 2 * n_bits, zkp_mul_proof_verify_batch, n_bits, batch, n, n_stride, e_a, e_b, e_c, f, z1, z2, e_d, e_db, out_verdict, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !e_a || !e_b || !e_c || !f || !z1 || !z2 || !e_d || !e_db || !out_verdict) {
    c->err = "zkp_mul_proof_verify_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dea = s.in(e_a, batch * 2 * kw), *deb = s.in(e_b, batch * 2 * kw), *dec = s.in(e_c, batch * 2 * kw);
  const uint32_t* df = s.in(f, batch * kw);
  const uint32_t *dz1 = s.in(z1, batch * 2 * kw), *dz2 = s.in(z2, batch * 2 * kw), *ded = s.in(e_d, batch * 2 * kw), *dedb = s.in(e_db, batch * 2 * kw);
  uint8_t* dv = s.out(out_verdict, batch);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return mul_verify_impl<G()>(c, n_bits, batch, dn, n_stride, dea, deb, dec, df, dz1, dz2, ded, dedb, dv); });
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)

// ---- CorrectMessageProof (correct_message.rs:35-162) ------------------------------------------------------
struct CmCommon {
  uint64_t R;                 // rows = B * K
  const uint32_t* nr;         // modulus source per row: n (shared) or the replicated [R][kw]
  uint64_t nr_stride;         // 0 (shared) or kw
  const uint32_t* nn;         // n^2 words for the inverse kernel
  bool per;
  uint32_t* u;                // u_i = ciphertext * gm_i^-1 mod n^2   [R][2kw]
  uint8_t* inv1;              // status of the gm inverses [R]
  MulBufs q;
};

// everything both sides need: per-row keys, n^2 contexts, u_i (:50-56 / :136-144)
template <int G>
static int32_t cm_common(zkp_ctx* c, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* valid,
                         const uint32_t* ciphertext, CmCommon* o) {
  const uint32_t kw = n_bits / 32;
  const uint64_t R = B * K;
  int32_t st;
  o->R = R; o->per = n_stride != 0;
  if ((st = mul_bufs(c, R, kw, &o->q))) return st;
  for (int k : {S_CM_T0 + 0, S_CM_T0 + 1, S_CM_T0 + 2}) if ((st = ensure(c, c->scratch[k], R * 2 * kw * 4))) return st;
  if ((st = ensure(c, c->scratch[S_CM_FLAGS], 4 * R + 64))) return st;
  uint32_t* n_rows = (uint32_t*)c->scratch[S_CM_T0].p;         // [R][kw] (always built: it is also the factor n of gm = m*n + 1)
  uint32_t* ct_rows = (uint32_t*)c->scratch[S_CM_T0 + 1].p;    // [R][2kw]
  o->u = (uint32_t*)c->scratch[S_CM_T0 + 2].p;
  o->inv1 = (uint8_t*)c->scratch[S_CM_FLAGS].p;
  hipLaunchKernelGGL(k_repeat_rows, dim3((unsigned)((R * kw + 255) / 256)), dim3(256), 0, c->stream, n, n_stride, kw, K, R, n_rows);
  hipLaunchKernelGGL(k_repeat_rows, dim3((unsigned)((R * 2 * kw + 255) / 256)), dim3(256), 0, c->stream, ciphertext, (uint64_t)(2 * kw), 2 * kw, K, R, ct_rows);
  HIPCHK(c, hipGetLastError());
  o->nr = o->per ? n_rows : n; o->nr_stride = o->per ? kw : 0;
  if ((st = run_setup<G>(c, o->nr, o->nr_stride, (int)kw, 1, o->per ? R : 1, c->consts))) return st;
  if ((st = square_words(c, o->nr, o->nr_stride, (int)kw, o->per ? R : 1, &o->nn))) return st;
  uint32_t *gm = o->q.t[0], *gi = o->q.t[1];
  if ((st = modmul_ctx<G>(c, c->consts, o->per, R, valid, (int)kw, n_rows, (int)kw, gm, (int)(2 * kw)))) return st;       // m*n mod n^2
  hipLaunchKernelGGL(k_add_one, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, c->stream, gm, 2 * kw, R);                // + 1
  HIPCHK(c, hipGetLastError());
  if ((st = launch_modinv(c, R, (int)(2 * kw), gm, 2 * kw, o->nn, o->per ? 2 * kw : 0, gi, 2 * kw, o->inv1))) return st;   // mod_inv :53 / :141
  return modmul_ctx<G>(c, c->consts, o->per, R, ct_rows, (int)(2 * kw), gi, (int)(2 * kw), o->u, (int)(2 * kw));           // u_i
}

template <int G>
static int32_t cm_prove_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* valid,
                             const uint32_t* message, const uint32_t* r, const uint32_t* e_sim, const uint32_t* z_sim, const uint32_t* w, uint32_t* ct,
                             uint32_t* e_vec, uint32_t* z_vec, uint32_t* a_vec, uint8_t* status) {
  using CL = ConstLayout<G>;
  constexpr int GN = N_GROUP<G>;
  const uint32_t kw = n_bits / 32;
  const uint64_t R = B * K;
  int32_t st;
  // ciphertext = Enc(message, r) :44-49 (per-proof key context; cm_common then switches c->consts to the row view)
  if ((st = run_setup<G>(c, n, n_stride, (int)kw, 1, n_stride ? B : 1, c->consts))) return st;
  if ((st = enc_launch<G>(c, n_bits, B, n, n_stride, message, (int)kw, r, (int)kw, ct))) return st;
  CmCommon o;
  if ((st = cm_common<G>(c, n_bits, B, K, n, n_stride, valid, ct, &o))) return st;
  for (int k : {S_CM_T0 + 3, S_CM_T0 + 4, S_CM_T0 + 5, S_CM_T0 + 6}) if ((st = ensure(c, c->scratch[k], R * 2 * kw * 4 + 64))) return st;
  if ((st = ensure(c, c->scratch[S_CM_SUM], B * 64 + R * 8 + 64))) return st;
  uint32_t* row_sim = (uint32_t*)c->scratch[S_CM_T0 + 3].p;                 // [R]
  uint8_t* panic = (uint8_t*)(row_sim + R);                                 // [B]
  uint32_t* base = (uint32_t*)c->scratch[S_CM_T0 + 4].p;                    // [R][kw]
  uint32_t* expw = (uint32_t*)c->scratch[S_CM_T0 + 5].p;                    // [R][8]
  uint32_t* zi = (uint32_t*)c->scratch[S_CM_T0 + 6].p;                      // [B][kw] | r^ei [B][kw]
  uint32_t* rpow = zi + B * kw;
  uint32_t* ei = (uint32_t*)c->scratch[S_CM_SUM].p;                         // [B][8]
  uint8_t* inv2 = (uint8_t*)(ei + B * 8);                                   // [R]
  CmPlanArgs pa{valid, message, kw, K, B, row_sim, panic};
  hipLaunchKernelGGL(k_cm_plan, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, pa);
  CmGatherArgs ga{row_sim, panic, w, z_sim, e_sim, kw, K, R, base, expw};
  hipLaunchKernelGGL(k_cm_gather, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, c->stream, ga);
  HIPCHK(c, hipGetLastError());
  uint32_t *P = o.q.t[2], *Q = o.q.t[3], *Qi = o.q.t[4];
  // P = base^n : w^n (:70) or z_j^n (:72)
  if ((st = modexp_core<G>(c, n_bits, R, base, o.nr, o.nr_stride, o.per, P, (int)kw, (int)(2 * kw)))) return st;
  if ((st = modexp_core<G>(c, 256, R, o.u, expw, 8, o.per, Q, (int)(2 * kw)))) return st;                                 // u_i^e_j :73 (1 on real rows)
  if ((st = launch_modinv(c, R, (int)(2 * kw), Q, 2 * kw, o.nn, o.per ? 2 * kw : 0, Qi, 2 * kw, inv2))) return st;        // mod_inv :74
  if ((st = modmul_ctx<G>(c, c->consts, o.per, R, P, (int)(2 * kw), Qi, (int)(2 * kw), a_vec, (int)(2 * kw)))) return st; // a_i :76
  if ((st = hash_list(c, B, {{a_vec, (uint64_t)K * 2 * kw, 2 * kw, 2 * kw, K}}, o.q.e))) return st;                      // chal :83 (256 bits: the modulus :88 is a no-op)
  hipLaunchKernelGGL(k_cm_ei, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t*)o.q.e, e_sim, K, B, ei);   // :90-93
  HIPCHK(c, hipGetLastError());
  if ((st = run_setup<GN>(c, n, n_stride, (int)kw, 0, n_stride ? B : 1, c->consts2))) return st;                         // modulus n
  {
    // r^ei mod n (:94) on the modulus-n context: swap it in for modexp_core, which reads c->consts
    std::swap(c->consts, c->consts2);
    st = modexp_core<GN>(c, 256, B, r, ei, 8, n_stride != 0, rpow, (int)kw);
    std::swap(c->consts, c->consts2);
    if (st) return st;
  }
  if ((st = modmul_ctx<GN>(c, c->consts2, n_stride != 0, B, w, (int)kw, rpow, (int)kw, zi, (int)kw))) return st;         // zi = w * r^ei mod n :95
  CmScatterArgs sa{row_sim, panic, o.inv1, inv2, (const uint32_t*)c->consts.p, o.per ? (uint64_t)CL::WORDS : 0, CL::OFF_ST, ei, zi, e_sim, z_sim, kw, K, B,
                   e_vec, z_vec, a_vec, status};
  hipLaunchKernelGGL(k_cm_scatter, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, sa);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

template <int G>
static int32_t cm_verify_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* valid,
                              const uint32_t* ct, const uint32_t* e_vec, const uint32_t* z_vec, const uint32_t* a_vec, uint8_t* verdict) {
  using CL = ConstLayout<G>;
  const uint32_t kw = n_bits / 32;
  const uint64_t R = B * K;
  int32_t st;
  CmCommon o;
  if ((st = cm_common<G>(c, n_bits, B, K, n, n_stride, valid, ct, &o))) return st;
  uint32_t *zn = o.q.t[2], *ue = o.q.t[3];
  if ((st = hash_list(c, B, {{a_vec, (uint64_t)K * 2 * kw, 2 * kw, 2 * kw, K}}, o.q.e))) return st;                      // chal :128
  if ((st = modexp_core<G>(c, n_bits, R, z_vec, o.nr, o.nr_stride, o.per, zn, (int)kw, (int)(2 * kw)))) return st;       // z_i^n :146
  if ((st = modexp_core<G>(c, 256, R, o.u, e_vec, 8, o.per, ue, (int)(2 * kw)))) return st;                              // u_i^e_i :147
  if ((st = modmul_ctx<G>(c, c->consts, o.per, R, ue, (int)(2 * kw), a_vec, (int)(2 * kw), ue, (int)(2 * kw)))) return st; // * a_i :148
  CmVerdictArgs va{o.q.e, e_vec, ue, zn, o.inv1, (const uint32_t*)c->consts.p, o.per ? (uint64_t)CL::WORDS : 0, CL::OFF_ST, kw, K, B, verdict};
  hipLaunchKernelGGL(k_cm_verdict, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, va);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

static bool cm_args_ok(uint32_t n_bits, uint64_t batch, uint32_t K, uint64_t n_stride) {
  return sigma_args_ok(n_bits, batch, n_stride) && K >= 1 && K <= 4096 && batch * K <= (1ull << 24);
}

extern "C" int32_t zkp_correct_message_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                                   const uint32_t* valid_messages, const uint32_t* message, const uint32_t* r, const uint32_t* e_sim,
                                                   const uint32_t* z_sim, const uint32_t* w, uint32_t* out_ciphertext, uint32_t* out_e_vec,
                                                   uint32_t* out_z_vec, uint32_t* out_a_vec, uint8_t* out_status, uint32_t flags) try {
  ZKP_ROUTE(c, batch * K, 2 * n_bits, zkp_correct_message_prove_batch, n_bits, batch, K, n, n_stride, valid_messages, message, r, e_sim, z_sim, w, out_ciphertext, out_e_vec, out_z_vec, out_a_vec, out_status, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!cm_args_ok(n_bits, batch, K, n_stride) || !n || !valid_messages || !message || !r || !w || (K > 1 && (!e_sim || !z_sim)) || !out_ciphertext || !out_e_vec ||
      !out_z_vec || !out_a_vec || !out_status) { c->err = "zkp_correct_message_prove_batch: invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32, R = batch * K, RS = batch * (K - 1);
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dv = s.in(valid_messages, R * kw), *dm = s.in(message, batch * kw), *dr = s.in(r, batch * kw), *dw = s.in(w, batch * kw);
  const uint32_t *des = RS ? s.in(e_sim, RS * 8) : nullptr, *dzs = RS ? s.in(z_sim, RS * kw) : nullptr;
  uint32_t *dct = s.out(out_ciphertext, batch * 2 * kw), *dev = s.out(out_e_vec, R * 8), *dzv = s.out(out_z_vec, R * kw), *dav = s.out(out_a_vec, R * 2 * kw);
  uint8_t* dst = s.out(out_status, batch);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return cm_prove_impl<G()>(c, n_bits, batch, K, dn, n_stride, dv, dm, dr, des, dzs, dw, dct, dev, dzv, dav, dst); });
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)

extern "C" int32_t zkp_correct_message_verify_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                                    const uint32_t* valid_messages, const uint32_t* ciphertext, const uint32_t* e_vec, const uint32_t* z_vec,
                                                    const uint32_t* a_vec, uint8_t* out_verdict, uint32_t flags) try {
  ZKP_ROUTE(c, batch * K, 2 * n_bits, zkp_correct_message_verify_batch, n_bits, batch, K, n, n_stride, valid_messages, ciphertext, e_vec, z_vec, a_vec, out_verdict, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!cm_args_ok(n_bits, batch, K, n_stride) || !n || !valid_messages || !ciphertext || !e_vec || !z_vec || !a_vec || !out_verdict) {
    c->err = "zkp_correct_message_verify_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32, R = batch * K;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dv = s.in(valid_messages, R * kw), *dct = s.in(ciphertext, batch * 2 * kw), *dev = s.in(e_vec, R * 8), *dzv = s.in(z_vec, R * kw),
                 *dav = s.in(a_vec, R * 2 * kw);
  uint8_t* dvd = s.out(out_verdict, batch);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return cm_verify_impl<G()>(c, n_bits, batch, K, dn, n_stride, dv, dct, dev, dzv, dav, dvd); });
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)
