// zkp_api_mul.inc — host side of zkp_modinv_batch, MulProof and CorrectMessageProof (SURVEY §8(f) rank 4);
// included by zkp_api.hip.  Compositions of k_enc / k_modexp / k_modmul with the kernels of kernels_inv.hpp.

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
  return s.finish(st);
} ZKP_CATCH(c)

struct MulBufs { uint32_t* t[10]; uint8_t* invst; uint32_t* e; };
template <int G> static MulBufs mul_bufs(Compose<G>& m) {
  MulBufs b;
  for (int k = 0; k < 10; k++) b.t[k] = m.buf(S_MP_T0 + k, m.batch * 2 * m.kw);
  b.invst = m.template buf<uint8_t>(S_MP_INVST, m.batch);
  b.e = m.buf(S_E, m.batch * 8);
  return b;
}

// multiplication_proof.rs:60-104
template <int G>
static int32_t mul_prove_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a, const uint32_t* e_b,
                              const uint32_t* e_c, const uint32_t* a, const uint32_t* b, const uint32_t* r_a, const uint32_t* r_b, const uint32_t* r_c,
                              const uint32_t* d, const uint32_t* r_d, uint32_t* f, uint32_t* z1, uint32_t* z2, uint32_t* e_d, uint32_t* e_db, uint8_t* status) {
  using CL = ConstLayout<G>;
  const uint32_t kw = n_bits / 32;
  const int w1 = (int)kw, w2 = (int)(2 * kw);
  Compose<G> m(c, B, n_stride != 0, kw);
  const MulBufs q = mul_bufs(m);
  m.M.setup(n, n_stride, 1);                                      // modulus n^2
  m.n.setup(n, n_stride, 0);                                      // modulus n
  m.square_words(n, n_stride, m.per ? B : 1);
  uint32_t *rdb = q.t[0], *db = q.t[1], *t2 = q.t[2], *t3 = q.t[3], *t4 = q.t[4], *t5 = q.t[5], *ea = q.t[6], *dred = q.t[7];
  m.enc(n, n_stride, d, w1, r_d, w1, e_d);                        // e_d = Enc(d, r_d) :63-68
  m.M.mul(r_d, w1, r_b, w1, rdb, w2);                             // r_db = r_d * r_b :69 (< n^2: exact)
  m.M.mul(d, w1, b, w1, db, w2);                                  // db = d * b :70
  m.enc(n, n_stride, db, w2, rdb, w2, e_db);                      // e_db :71-76
  m.hash({{n, n_stride, 0, kw, 1}, {e_a, 2 * kw, 0, 2 * kw, 1}, {e_b, 2 * kw, 0, 2 * kw, 1}, {e_c, 2 * kw, 0, 2 * kw, 1}, {e_d, 2 * kw, 0, 2 * kw, 1},
          {e_db, 2 * kw, 0, 2 * kw, 1}}, q.e);                    // e :77-84
  m.n.mul(q.e, 8, a, w1, ea, w1);                                 // e*a mod n :87
  m.n.mul(d, w1, nullptr, w1, dred, w1);                          // d mod n
  m.rows(k_modadd, B, ea, dred, n, n_stride, w1, B, f);           // f :88
  // r_a^e (:89), r_c^e (:92) and r_b^f (:91) are independent of each other: one launch, their chains side by side
  m.M.pow_multi({{256, r_a, q.e, 8, t2, w1, w2}, {256, r_c, q.e, 8, t3, w1, w2}, {n_bits, r_b, f, kw, t5, w1, w2}});
  m.M.mul(t2, w2, r_d, w1, z1, w2);                               // z1 :90
  m.M.mul(rdb, w2, t3, w2, t3, w2);                               // r_db * r_c^e :93
  m.inv(t3, t4, q.invst);                                         // mod_inv :95
  m.M.mul(t5, w2, t4, w2, z2, w2);                                // z2 :96
  m.rows(k_mul_finish, B, MulFinishArgs{q.invst, m.M.cst(), m.M.cst_stride(), CL::OFF_ST, w1, B, f, z1, z2, status});
  return m.st;
}

// multiplication_proof.rs:106-146
template <int G>
static int32_t mul_verify_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a, const uint32_t* e_b,
                               const uint32_t* e_c, const uint32_t* f, const uint32_t* z1, const uint32_t* z2, const uint32_t* e_d, const uint32_t* e_db,
                               uint8_t* verdict) {
  using CL = ConstLayout<G>;
  const uint32_t kw = n_bits / 32;
  const int w1 = (int)kw, w2 = (int)(2 * kw);
  Compose<G> m(c, B, n_stride != 0, kw);
  const MulBufs q = mul_bufs(m);
  m.M.setup(n, n_stride, 1);
  m.square_words(n, n_stride, m.per ? B : 1);
  uint32_t *c1 = q.t[0], *c2 = q.t[1], *l1 = q.t[2], *t3 = q.t[3], *t4 = q.t[4], *l2 = q.t[5];
  m.hash({{n, n_stride, 0, kw, 1}, {e_a, 2 * kw, 0, 2 * kw, 1}, {e_b, 2 * kw, 0, 2 * kw, 1}, {e_c, 2 * kw, 0, 2 * kw, 1}, {e_d, 2 * kw, 0, 2 * kw, 1},
          {e_db, 2 * kw, 0, 2 * kw, 1}}, q.e);                    // e :107-114
  m.enc(n, n_stride, f, w1, z1, w2, c1);                          // Enc(f, z1) :116-122
  m.enc(n, n_stride, nullptr, -1, z2, w2, c2);                    // Enc(0, z2) :123-129
  // e_a^e (:131), e_c^e (:133) and e_b^f (:136): one launch
  m.M.pow_multi({{256, e_a, q.e, 8, l1, w2, 0}, {256, e_c, q.e, 8, t3, w2, 0}, {n_bits, e_b, f, kw, l2, w2, 0}});
  m.M.mul(l1, w2, e_d, w2, l1, w2);                               // * e_d :132
  m.M.mul(e_db, w2, t3, w2, t3, w2);                              // e_db * e_c^e :134
  m.inv(t3, t4, q.invst);                                         // mod_inv :135
  m.M.mul(l2, w2, t4, w2, l2, w2);                                // :137
  m.rows(k_mul_verdict, B, MulVerdictArgs{l1, c1, l2, c2, q.invst, m.M.cst(), m.M.cst_stride(), CL::OFF_ST, 2 * kw, B, verdict});
  return m.st;
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
  return s.finish(st);
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
  return s.finish(st);
} ZKP_CATCH(c)

// ---- CorrectMessageProof (correct_message.rs:35-162) ------------------------------------------------------
struct CmCommon {
  const uint32_t* nr;         // modulus source per row: n (shared) or the replicated [R][kw]
  uint64_t nr_stride;         // 0 (shared) or kw
  uint32_t* u;                // u_i = ciphertext * gm_i^-1 mod n^2   [R][2kw]
  uint8_t* inv1;              // status of the gm inverses [R]
  MulBufs q;
};

// everything both sides need: per-row keys, n^2 contexts, u_i (:50-56 / :136-144).  `m` composes over the R = B * K rows.
template <int G>
static CmCommon cm_common(Compose<G>& m, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* valid, const uint32_t* ciphertext) {
  const uint32_t kw = m.kw;
  const uint64_t R = m.batch;
  const int w1 = (int)kw, w2 = (int)(2 * kw);
  CmCommon o;
  o.q = mul_bufs(m);
  uint32_t* n_rows = m.buf(S_CM_T0, R * 2 * kw);              // [R][kw] (always built: it is also the factor n of gm = m*n + 1)
  uint32_t* ct_rows = m.buf(S_CM_T0 + 1, R * 2 * kw);         // [R][2kw]
  o.u = m.buf(S_CM_T0 + 2, R * 2 * kw);
  o.inv1 = m.template buf<uint8_t>(S_CM_FLAGS, 4 * R + 64);
  m.rows(k_repeat_rows, R * kw, n, n_stride, kw, K, R, n_rows);
  m.rows(k_repeat_rows, R * 2 * kw, ciphertext, (uint64_t)(2 * kw), 2 * kw, K, R, ct_rows);
  o.nr = m.per ? n_rows : n; o.nr_stride = m.per ? kw : 0;
  m.M.setup(o.nr, o.nr_stride, 1);
  m.square_words(o.nr, o.nr_stride, m.per ? R : 1);
  uint32_t *gm = o.q.t[0], *gi = o.q.t[1];
  m.M.mul(valid, w1, n_rows, w1, gm, w2);                     // m*n mod n^2
  m.rows(k_add_one, R, gm, 2 * kw, R);                        // + 1
  m.inv(gm, gi, o.inv1);                                      // mod_inv :53 / :141
  m.M.mul(ct_rows, w2, gi, w2, o.u, w2);                      // u_i
  return o;
}

template <int G>
static int32_t cm_prove_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* valid,
                             const uint32_t* message, const uint32_t* r, const uint32_t* e_sim, const uint32_t* z_sim, const uint32_t* w, uint32_t* ct,
                             uint32_t* e_vec, uint32_t* z_vec, uint32_t* a_vec, uint8_t* status) {
  using CL = ConstLayout<G>;
  const uint32_t kw = n_bits / 32;
  const uint64_t R = B * K;
  const int w1 = (int)kw, w2 = (int)(2 * kw);
  Compose<G> m(c, R, n_stride != 0, kw);
  // ciphertext = Enc(message, r) :44-49 (per-proof key context; cm_common then switches M to the row view)
  m.M.setup(n, n_stride, 1, m.per ? B : 1);
  m.enc(n, n_stride, message, w1, r, w1, ct, B);
  const CmCommon o = cm_common(m, K, n, n_stride, valid, ct);
  uint32_t* row_sim = m.buf(S_CM_T0 + 3, R * 2 * kw + 16);                  // [R]
  uint32_t* base = m.buf(S_CM_T0 + 4, R * 2 * kw + 16);                     // [R][kw]
  uint32_t* expw = m.buf(S_CM_T0 + 5, R * 2 * kw + 16);                     // [R][8]
  uint32_t* zi = m.buf(S_CM_T0 + 6, R * 2 * kw + 16);                       // [B][kw] | r^ei [B][kw]
  uint32_t* ei = (uint32_t*)m.template buf<uint8_t>(S_CM_SUM, B * 64 + R * 8 + 64);      // [B][8]
  if (m.st) return m.st;
  uint8_t* panic = (uint8_t*)(row_sim + R);                                 // [B]
  uint32_t* rpow = zi + B * kw;
  uint8_t* inv2 = (uint8_t*)(ei + B * 8);                                   // [R]
  m.rows(k_cm_plan, B, CmPlanArgs{valid, message, kw, K, B, row_sim, panic});
  m.rows(k_cm_gather, R, CmGatherArgs{row_sim, panic, w, z_sim, e_sim, kw, K, R, base, expw});
  uint32_t *P = o.q.t[2], *Q = o.q.t[3], *Qi = o.q.t[4];
  m.M.pow(n_bits, base, o.nr, o.nr_stride, P, w1, w2);                      // P = base^n : w^n (:70) or z_j^n (:72)
  m.M.pow(256, o.u, expw, 8, Q, w2);                                        // u_i^e_j :73 (1 on real rows)
  m.inv(Q, Qi, inv2);                                                       // mod_inv :74
  m.M.mul(P, w2, Qi, w2, a_vec, w2);                                        // a_i :76
  m.hash({{a_vec, (uint64_t)K * 2 * kw, 2 * kw, 2 * kw, K}}, o.q.e, B);     // chal :83 (256 bits: the modulus :88 is a no-op)
  m.rows(k_cm_ei, B, (const uint32_t*)o.q.e, e_sim, K, B, ei);              // :90-93
  m.n.setup(n, n_stride, 0, m.per ? B : 1);                                 // modulus n
  m.n.pow(256, r, ei, 8, rpow, w1, 0, B);                                   // r^ei mod n :94
  m.n.mul(w, w1, rpow, w1, zi, w1, B);                                      // zi = w * r^ei mod n :95
  m.rows(k_cm_scatter, B, CmScatterArgs{row_sim, panic, o.inv1, inv2, m.M.cst(), m.M.cst_stride(), CL::OFF_ST, ei, zi, e_sim, z_sim, kw, K, B, e_vec, z_vec,
                                        a_vec, status});
  return m.st;
}

template <int G>
static int32_t cm_verify_impl(zkp_ctx* c, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride, const uint32_t* valid,
                              const uint32_t* ct, const uint32_t* e_vec, const uint32_t* z_vec, const uint32_t* a_vec, uint8_t* verdict) {
  using CL = ConstLayout<G>;
  const uint32_t kw = n_bits / 32;
  const int w1 = (int)kw, w2 = (int)(2 * kw);
  Compose<G> m(c, B * K, n_stride != 0, kw);
  const CmCommon o = cm_common(m, K, n, n_stride, valid, ct);
  uint32_t *zn = o.q.t[2], *ue = o.q.t[3];
  m.hash({{a_vec, (uint64_t)K * 2 * kw, 2 * kw, 2 * kw, K}}, o.q.e, B);     // chal :128
  m.M.pow(n_bits, z_vec, o.nr, o.nr_stride, zn, w1, w2);                    // z_i^n :146
  m.M.pow(256, o.u, e_vec, 8, ue, w2);                                      // u_i^e_i :147
  m.M.mul(ue, w2, a_vec, w2, ue, w2);                                       // * a_i :148
  m.rows(k_cm_verdict, B, CmVerdictArgs{o.q.e, e_vec, ue, zn, o.inv1, m.M.cst(), m.M.cst_stride(), CL::OFF_ST, kw, K, B, verdict});
  return m.st;
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
  return s.finish(st);
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
  return s.finish(st);
} ZKP_CATCH(c)
