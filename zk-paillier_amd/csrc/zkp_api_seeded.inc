// zkp_api_seeded.inc — seeded proving for ZeroProof, CiphertextProof, CorrectMessageProof, CompositeDLogProof, VerlinProof and MulProof: the
// nonces the reference's prove draws itself are expanded on the device from a 32-byte seed (kernels_sample.hpp: k_nonce_sample; the two proofs
// whose prove redraws a nonce until it is coprime to n — verlin_proof.rs:64-67, multiplication_proof.rs:148-154 — kernels_coprime.hpp:
// k_nonce_coprime; the stream is defined in include/zkp_hip.h and DESIGN.md section 4), the nonce-input entry point runs on them as the
// device-pointer call it already knows, and Stage::secret wipes them — with the staged copies of the caller's secrets — on every path out.

// The nonce fields of every kind, in the order of out_field[]: how a field is drawn, its rows per proof (1, or one per simulated message:
// K - 1), the slot of its first row and the words of a row (0: kw).  At most three BELOW fields and one RAW or COPRIME field per kind.
enum NonceDraw : uint8_t { ND_NONE = 0, ND_BELOW /* sample_below(n) */, ND_RAW /* a power of two: the block's first words */, ND_COPRIME /* below n and coprime to it */ };
struct NonceField { NonceDraw draw; bool per_sim; uint8_t slot0, words; };
static constexpr NonceField NONCE_FIELDS[ZKP_SEEDED_KIND_MUL + 1][4] = {
  {},
  /* ZERO */            {{ND_BELOW, false, 0, 0}},
  /* CIPHERTEXT */      {{ND_BELOW, false, 0, 0}, {ND_BELOW, false, 0, 0}},
  /* CORRECT_MESSAGE */ {{ND_BELOW, false, 0, 0}, {ND_BELOW, false, 0, 0}, {ND_RAW, true, 1, 8}, {ND_BELOW, true, 1, 0}},
  /* DLOG */            {{ND_RAW, false, 0, 16}},
  /* VERLIN */          {{ND_BELOW, false, 0, 0}, {ND_BELOW, false, 0, 0}, {ND_BELOW, false, 0, 0}, {ND_COPRIME, false, 0, 0}},
  /* MUL */             {{ND_BELOW, false, 0, 0}, {ND_COPRIME, false, 0, 0}},
};
static bool nonce_kind_ok(uint32_t kind) { return kind >= ZKP_SEEDED_KIND_ZERO && kind <= ZKP_SEEDED_KIND_MUL; }
// does the kind have a coprime field (the kinds of zkp_nonce_sample_coprime_batch)?
static bool nonce_kind_coprime(uint32_t kind) {
  for (const NonceField& d : NONCE_FIELDS[kind]) if (d.draw == ND_COPRIME) return true;
  return false;
}
static uint32_t nonce_field_rows(const NonceField& d, uint32_t K) { return d.draw == ND_NONE ? 0 : d.per_sim ? K - 1 : 1; }
// the words of one proof's rows of field f, 0 where the kind has no such field
static size_t nonce_field_words(uint32_t kind, uint32_t f, uint32_t kw, uint32_t K) {
  const NonceField& d = NONCE_FIELDS[kind][f];
  return (size_t)nonce_field_rows(d, K) * (d.words ? d.words : kw);
}

// The sampler's launches over filled args (everything but meta and max_attempts): k_nonce_prep, the BELOW draws, the kind's RAW or COPRIME
// field (`fourth`; k_nonce_prep and k_nonce_sample do not read it, k_nonce_fixup zeroes it by (raw_per, raw_words): a COPRIME field is handed
// to it as one row of kw words per proof) and the fixup.  Every pointer is device memory; status is written for every proof.
static int32_t nonce_sample_run(zkp_ctx* c, NonceSampleArgs& a, NonceDraw fourth) {
  int32_t st;
  if ((st = ensure(c, c->scratch[S_SAMPLE_META], a.batch * 8))) return st;
  a.meta = (uint32_t*)c->scratch[S_SAMPLE_META].p; a.max_attempts = RANGE_SAMPLE_MAX_ATTEMPTS;
  const uint64_t B = a.batch;
  const uint32_t kw = a.kw;
  if ((st = launch_rows(c, k_nonce_prep, B, a))) return st;
  const uint64_t G = kw / 16;
  uint64_t tasks = 0, fix = 0;
  for (uint32_t k = 0; k < a.nbelow; k++) { tasks += B * a.below_per[k]; fix = std::max<uint64_t>(fix, B * a.below_per[k] * kw / 4); }
  if (tasks) {
    switch (G) {
      case 2: st = launch_rows(c, k_nonce_sample<2>, tasks * G, a); break;
      case 4: st = launch_rows(c, k_nonce_sample<4>, tasks * G, a); break;
      default: st = launch_rows(c, k_nonce_sample<8>, tasks * G, a); break;
    }
    if (st) return st;
  }
  const uint64_t rows = B * a.raw_per;
  if (fourth == ND_RAW && rows && (st = launch_rows(c, k_nonce_raw, rows, a))) return st;
  if (fourth == ND_COPRIME) {
    NonceCoprimeArgs q{a.key, a.n, a.n_stride, a.meta, a.raw, a.status, a.first_index, B, kw, a.kind, a.raw_field, RANGE_SAMPLE_MAX_ATTEMPTS};
    if ((st = launch_lanes(c, k_nonce_coprime, B, coprime_lds_words_per_lane(kw), q))) return st;
  }
  fix = std::max<uint64_t>(fix, rows * a.raw_words / 4);
  if (a.n && fix) return launch_rows(c, k_nonce_fixup, fix, a);      // (a kind without a bound has no MALFORMED case)
  return ZKP_OK;
}

// the kinds of NONCE_FIELDS: out[f] is the array of field f (null where the kind has none, or no slots)
static int32_t nonce_sample_launch(zkp_ctx* c, uint32_t kind, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                   const uint32_t* key, uint64_t first_index, uint32_t* const out[4], uint8_t* status) {
  const uint32_t kw = n_bits / 32;
  NonceSampleArgs a{};
  a.key = key; a.n = kind == ZKP_SEEDED_KIND_DLOG ? nullptr : n; a.n_stride = n_stride; a.status = status;
  a.first_index = first_index; a.batch = B; a.kw = kw; a.kind = kind;
  NonceDraw fourth = ND_NONE;
  for (uint32_t f = 0; f < 4; f++) {
    const NonceField& d = NONCE_FIELDS[kind][f];
    if (d.draw == ND_BELOW) {
      a.below[a.nbelow] = out[f]; a.below_field[a.nbelow] = f; a.below_per[a.nbelow] = nonce_field_rows(d, K); a.below_slot0[a.nbelow] = d.slot0; a.nbelow++;
    } else if (d.draw != ND_NONE) {
      a.raw = out[f]; a.raw_field = f; a.raw_per = nonce_field_rows(d, K); a.raw_slot0 = d.slot0; a.raw_words = d.words ? d.words : kw;
      fourth = d.draw;
    }
  }
  return nonce_sample_run(c, a, fourth);
}

static bool nonce_args_ok(uint32_t kind, uint32_t n_bits, uint64_t batch, uint32_t K, uint64_t n_stride) {
  if (!nonce_kind_ok(kind) || !sigma_args_ok(n_bits, batch, n_stride)) return false;
  return kind != ZKP_SEEDED_KIND_CORRECT_MESSAGE || (K >= 1 && K <= 65536 && batch * K <= (1ull << 24));
}

// zkp_nonce_sample_batch (the kinds without a coprime field) and zkp_nonce_sample_coprime_batch (those with one)
static int32_t nonce_sample_entry(zkp_ctx* c, const char* name, bool coprime, uint32_t proof_kind, uint32_t n_bits, uint64_t batch, uint32_t num_messages,
                                  const uint32_t* n, uint64_t n_stride, const uint8_t* seed, uint64_t first_index, uint32_t** out_field, uint8_t* out_status,
                                  uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  bool ok = nonce_args_ok(proof_kind, n_bits, batch, num_messages, n_stride) && nonce_kind_coprime(proof_kind) == coprime && seed && out_field &&
            (n || proof_kind == ZKP_SEEDED_KIND_DLOG);
  const uint32_t kw = n_bits / 32, K = proof_kind == ZKP_SEEDED_KIND_CORRECT_MESSAGE ? num_messages : 1;
  uintptr_t align = 0;
  for (uint32_t f = 0; ok && f < 4; f++)
    if (nonce_field_words(proof_kind, f, kw, K)) { ok = out_field[f] != nullptr; align |= (uintptr_t)out_field[f]; }
  if (!ok) { c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL; }
  if ((flags & ZKP_F_DEVICE_PTRS) && (align & 15u)) { c->err = std::string(name) + ": device output arrays must be 16-byte aligned"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  const uint32_t* dn = proof_kind == ZKP_SEEDED_KIND_DLOG ? nullptr : s.in(n, n_stride ? batch * kw : kw);
  const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(key, 32);
  uint32_t* out[4] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t f = 0; f < 4; f++)
    if (const size_t words = batch * nonce_field_words(proof_kind, f, kw, K)) {
      out[f] = s.out(out_field[f], words);
      if (!s.dev) s.secret(out[f], words * 4);      // (host arrays: the staged copies are wiped behind the D2H)
    }
  uint8_t* ds = s.out(out_status, batch);
  int32_t st = s.st;
  if (!st && !ds) { st = ensure(c, c->scratch[S_SAMPLE_STATUS], batch); ds = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p; }
  if (!st) st = nonce_sample_launch(c, proof_kind, n_bits, batch, K, dn, n_stride, key, first_index, out, ds);
  return s.finish(st);
}

extern "C" int32_t zkp_nonce_sample_batch(zkp_ctx* c, uint32_t proof_kind, uint32_t n_bits, uint64_t batch, uint32_t num_messages, const uint32_t* n,
                                          uint64_t n_stride, const uint8_t* seed, uint64_t first_index, uint32_t** out_field,
                                          uint8_t* out_status, uint32_t flags) try {
  return nonce_sample_entry(c, "zkp_nonce_sample_batch", false, proof_kind, n_bits, batch, num_messages, n, n_stride, seed, first_index, out_field, out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_nonce_sample_coprime_batch(zkp_ctx* c, uint32_t proof_kind, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                                  const uint8_t* seed, uint64_t first_index, uint32_t** out_field, uint8_t* out_status,
                                                  uint32_t flags) try {
  return nonce_sample_entry(c, "zkp_nonce_sample_coprime_batch", true, proof_kind, n_bits, batch, 1, n, n_stride, seed, first_index, out_field, out_status, flags);
} ZKP_CATCH(c)

// What the six seeded proves share: the seed and the nonce blocks of a call, all of them secret.  The sampler's status goes to the ctx's
// own array: Zero, Ciphertext, DLog and Verlin copy it out (their nonce-input calls have no status), CorrectMessage and Mul OR it into the prove's
// (seeded_status, zkp_api_proofs.inc).
struct SeededNonces {
  const uint32_t* key = nullptr;
  uint32_t* f[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* status = nullptr;
  int32_t st = ZKP_OK;
  SeededNonces(zkp_ctx* c, Stage& s, uint32_t kind, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* dn, uint64_t n_stride, const uint8_t* seed,
               uint64_t first_index) {
    key = (const uint32_t*)s.host_in(seed, 32);
    s.secret(key, 32);
    for (uint32_t k = 0; k < 4; k++)
      if (const size_t words = B * nonce_field_words(kind, k, n_bits / 32, K)) f[k] = s.secret_scratch<uint32_t>(words);
    if ((st = s.st)) return;
    if ((st = ensure(c, c->scratch[S_SAMPLE_STATUS], B))) return;
    status = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p;
    st = nonce_sample_launch(c, kind, n_bits, B, K, dn, n_stride, key, first_index, f, status);
  }
};

static int32_t sigma_prove_seeded(zkp_ctx* c, const char* name, bool with_x, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                  const uint32_t* cc, const uint32_t* x, const uint32_t* r, const uint8_t* seed, uint64_t first_index, uint32_t* out_z1,
                                  uint32_t* out_z, uint32_t* out_commit, uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !seed) { c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t* dc = s.in(cc, batch * 2 * kw);
  const uint32_t* dr = s.in(r, batch * kw);
  const uint32_t* dx = with_x ? s.in(x, batch * kw) : nullptr;
  if (!s.dev) { s.secret(dr, batch * kw * 4); s.secret(dx, batch * kw * 4); }
  uint32_t* dz1 = with_x ? s.out(out_z1, batch * (kw + ZKP_Z1_EXTRA_LIMBS)) : nullptr;
  uint32_t* dz = s.out(out_z, batch * 2 * kw);
  uint32_t* dcm = s.out(out_commit, batch * 2 * kw);
  uint8_t* ds = s.out(out_status, batch);
  SeededNonces q(c, s, with_x ? ZKP_SEEDED_KIND_CIPHERTEXT : ZKP_SEEDED_KIND_ZERO, n_bits, batch, 1, dn, n_stride, seed, first_index);
  int32_t st = q.st;      // (a null c, x, r or output is refused by the nonce-input call: ZKP_EINVAL, after the sampler ran)
  if (!st) st = with_x ? zkp_ciphertext_proof_prove_batch(c, n_bits, batch, dn, n_stride, dc, dx, dr, q.f[0], q.f[1], dz1, dz, dcm, ZKP_F_DEVICE_PTRS)
                       : zkp_zero_proof_prove_batch(c, n_bits, batch, dn, n_stride, dc, dr, q.f[0], dz, dcm, ZKP_F_DEVICE_PTRS);
  if (!st) st = seeded_status(c, ds, q.status, batch, false);
  return s.finish(st);
}

extern "C" int32_t zkp_zero_proof_prove_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                                     const uint32_t* r, const uint8_t* seed, uint64_t first_index, uint32_t* out_z, uint32_t* out_a,
                                                     uint8_t* out_status, uint32_t flags) try {
  return sigma_prove_seeded(c, "zkp_zero_proof_prove_seeded_batch", false, n_bits, batch, n, n_stride, cc, nullptr, r, seed, first_index, nullptr, out_z, out_a,
                            out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_ciphertext_proof_prove_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                                           const uint32_t* cc, const uint32_t* x, const uint32_t* r, const uint8_t* seed, uint64_t first_index,
                                                           uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_c_prime, uint8_t* out_status, uint32_t flags) try {
  return sigma_prove_seeded(c, "zkp_ciphertext_proof_prove_seeded_batch", true, n_bits, batch, n, n_stride, cc, x, r, seed, first_index, out_z1, out_z2,
                            out_c_prime, out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_correct_message_prove_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                                          const uint32_t* valid_messages, const uint32_t* message, const uint8_t* seed, uint64_t first_index,
                                                          uint32_t* out_ciphertext, uint32_t* out_e_vec, uint32_t* out_z_vec, uint32_t* out_a_vec,
                                                          uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  // (K <= 65536 is the stream's bound — slot < 65536; the prove's own, smaller one is checked here too, so that nothing is launched for a K it refuses)
  if (!nonce_args_ok(ZKP_SEEDED_KIND_CORRECT_MESSAGE, n_bits, batch, K, n_stride) || !cm_args_ok(n_bits, batch, K, n_stride) || !n || !seed) {
    c->err = "zkp_correct_message_prove_seeded_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32, R = batch * K;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dv = s.in(valid_messages, R * kw), *dm = s.in(message, batch * kw);
  if (!s.dev) s.secret(dm, batch * kw * 4);
  uint32_t *dct = s.out(out_ciphertext, batch * 2 * kw), *dev = s.out(out_e_vec, R * 8), *dzv = s.out(out_z_vec, R * kw), *dav = s.out(out_a_vec, R * 2 * kw);
  uint8_t* ds = s.out(out_status, batch);
  SeededNonces q(c, s, ZKP_SEEDED_KIND_CORRECT_MESSAGE, n_bits, batch, K, dn, n_stride, seed, first_index);
  int32_t st = q.st;      // (a null list, message or output is refused by the nonce-input call: ZKP_EINVAL, after the sampler ran)
  if (!st) st = zkp_correct_message_prove_batch(c, n_bits, batch, K, dn, n_stride, dv, dm, q.f[0], q.f[2], q.f[3], q.f[1], dct, dev, dzv, dav, ds, ZKP_F_DEVICE_PTRS);
  if (!st) st = seeded_status(c, ds, q.status, batch, true);
  return s.finish(st);
} ZKP_CATCH(c)

extern "C" int32_t zkp_dlog_prove_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* N, const uint32_t* g,
                                               const uint32_t* ni, const uint32_t* secret, const uint8_t* seed, uint64_t first_index, uint32_t* out_x,
                                               uint32_t* out_y, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!dlog_args_ok(n_bits, y_bits, batch) || !seed) { c->err = "zkp_dlog_prove_seeded_batch: invalid argument"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t *dN = s.in(N, batch * kw), *dg = s.in(g, batch * kw), *dni = s.in(ni, batch * kw), *dsec = s.in(secret, batch * 8);
  if (!s.dev) s.secret(dsec, batch * 8 * 4);
  uint32_t* dx = s.out(out_x, batch * kw);
  uint32_t* dy = s.out(out_y, batch * (y_bits / 32));
  uint8_t* ds = s.out(out_status, batch);
  SeededNonces q(c, s, ZKP_SEEDED_KIND_DLOG, n_bits, batch, 1, nullptr, 0, seed, first_index);
  int32_t st = q.st;      // (a null statement, secret or output is refused by the nonce-input call: ZKP_EINVAL, after the sampler ran)
  if (!st) st = zkp_dlog_prove_batch(c, n_bits, y_bits, batch, dN, dg, dni, dsec, q.f[0], dx, dy, ZKP_F_DEVICE_PTRS);
  if (!st) st = seeded_status(c, ds, q.status, batch, false);
  return s.finish(st);
} ZKP_CATCH(c)

extern "C" int32_t zkp_verlin_proof_prove_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                                       const uint32_t* c_prime, const uint32_t* phi_x, const uint32_t* x, const uint32_t* x_prime,
                                                       const uint32_t* x_double_prime, const uint32_t* r_x, const uint8_t* seed, uint64_t first_index,
                                                       uint32_t* out_phi_a, uint32_t* out_z, uint32_t* out_z_prime, uint32_t* out_z_double_prime,
                                                       uint32_t* out_r_z, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !seed) { c->err = "zkp_verlin_proof_prove_seeded_batch: invalid argument"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32, zw = kw + ZKP_Z1_EXTRA_LIMBS;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dc = s.in(cc, batch * 2 * kw), *dcp = s.in(c_prime, batch * 2 * kw), *dphx = s.in(phi_x, batch * 2 * kw);
  const uint32_t *dx = s.in(x, batch * kw), *dxp = s.in(x_prime, batch * kw), *dxpp = s.in(x_double_prime, batch * kw), *drx = s.in(r_x, batch * kw);
  if (!s.dev) for (const uint32_t* p : {dx, dxp, dxpp, drx}) s.secret(p, batch * kw * 4);
  uint32_t* dpa = s.out(out_phi_a, batch * 2 * kw);
  uint32_t *dz = s.out(out_z, batch * zw), *dzp = s.out(out_z_prime, batch * zw), *dzpp = s.out(out_z_double_prime, batch * zw);
  uint32_t* drz = s.out(out_r_z, batch * 2 * kw);
  uint8_t* ds = s.out(out_status, batch);
  SeededNonces q(c, s, ZKP_SEEDED_KIND_VERLIN, n_bits, batch, 1, dn, n_stride, seed, first_index);
  int32_t st = q.st;      // (a null statement, witness or output is refused by the nonce-input call: ZKP_EINVAL, after the sampler ran)
  if (!st) st = zkp_verlin_proof_prove_batch(c, n_bits, batch, dn, n_stride, dc, dcp, dphx, dx, dxp, dxpp, drx, q.f[0], q.f[1], q.f[2], q.f[3], dpa, dz, dzp,
                                             dzpp, drz, ZKP_F_DEVICE_PTRS);
  if (!st) st = seeded_status(c, ds, q.status, batch, false);
  return s.finish(st);
} ZKP_CATCH(c)

extern "C" int32_t zkp_mul_proof_prove_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* e_a,
                                                    const uint32_t* e_b, const uint32_t* e_c, const uint32_t* a, const uint32_t* b, const uint32_t* r_a,
                                                    const uint32_t* r_b, const uint32_t* r_c, const uint8_t* seed, uint64_t first_index, uint32_t* out_f,
                                                    uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_e_d, uint32_t* out_e_db, uint8_t* out_status,
                                                    uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !seed) { c->err = "zkp_mul_proof_prove_seeded_batch: invalid argument"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dea = s.in(e_a, batch * 2 * kw), *deb = s.in(e_b, batch * 2 * kw), *dec = s.in(e_c, batch * 2 * kw);
  const uint32_t *da = s.in(a, batch * kw), *db = s.in(b, batch * kw), *dra = s.in(r_a, batch * kw), *drb = s.in(r_b, batch * kw), *drc = s.in(r_c, batch * kw);
  if (!s.dev) for (const uint32_t* p : {da, db, dra, drb, drc}) s.secret(p, batch * kw * 4);
  uint32_t* df = s.out(out_f, batch * kw);
  uint32_t *dz1 = s.out(out_z1, batch * 2 * kw), *dz2 = s.out(out_z2, batch * 2 * kw), *ded = s.out(out_e_d, batch * 2 * kw), *dedb = s.out(out_e_db, batch * 2 * kw);
  uint8_t* ds = s.out(out_status, batch);
  SeededNonces q(c, s, ZKP_SEEDED_KIND_MUL, n_bits, batch, 1, dn, n_stride, seed, first_index);
  int32_t st = q.st;      // (a null statement, witness or output is refused by the nonce-input call: ZKP_EINVAL, after the sampler ran)
  if (!st) st = zkp_mul_proof_prove_batch(c, n_bits, batch, dn, n_stride, dea, deb, dec, da, db, dra, drb, drc, q.f[0], q.f[1], df, dz1, dz2, ded, dedb, ds,
                                          ZKP_F_DEVICE_PTRS);
  if (!st) st = seeded_status(c, ds, q.status, batch, true);
  return s.finish(st);
} ZKP_CATCH(c)

// ---- the verifier's commitment of the interactive RangeProof: RangeProof::verifier_commit from a seed, the (r, e) it committed to for the
// decommit message, and RangeProof::verify_commit (range_proof.rs:118-126, 195-208).  k_range_commit makes the two operands of the one Enc
// of every session, and the Enc runs as the device-pointer call it already is: zkp_paillier_enc_batch (store) or
// zkp_paillier_enc_check_batch (compare with `expected`), with their routing, key cache and kernels.
static int32_t range_commit_launch(zkp_ctx* c, uint32_t n_bits, const RangeCommitArgs& a) {
  const uint64_t rows = a.batch * (n_bits / 512);
  switch (n_bits / 512) {
    case 2: return launch_rows(c, k_range_commit<2>, rows, a);
    case 4: return launch_rows(c, k_range_commit<4>, rows, a);
    default: return launch_rows(c, k_range_commit<8>, rows, a);
  }
}

// commit (out_com) or reveal (out_r, out_e): the same stream, so the same (r, e).  `s` wipes the seed and every copy of r, e and m on every
// path out; in the commit call none of them is ever outside the blocks it wipes.
static int32_t range_commit_seeded(zkp_ctx* c, const char* name, bool reveal, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                   uint32_t e_len, const uint8_t* seed, uint64_t first_index, uint32_t* out_com, uint32_t* out_r, uint8_t* out_e,
                                   uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !seed || e_len < 1 || e_len > 32 || (batch && (reveal ? !out_r || !out_e : !out_com))) {
    c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL;
  }
  if (reveal && (flags & ZKP_F_DEVICE_PTRS) && ((uintptr_t)out_r & 15u)) { c->err = std::string(name) + ": device output arrays must be 16-byte aligned"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  RangeCommitArgs a{};
  a.n = s.in(n, n_stride ? batch * kw : kw); a.n_stride = n_stride;
  a.key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(a.key, 32);
  uint32_t* dcom = nullptr;
  if (reveal) {
    a.r = s.out(out_r, batch * kw); a.e_out = s.out(out_e, batch * 32);
    if (!s.dev) { s.secret(a.r, batch * kw * 4); s.secret(a.e_out, batch * 32); }      // (host arrays: the staged copies are wiped behind the D2H)
  } else {
    dcom = s.out(out_com, batch * 2 * kw);
    a.r = s.secret_scratch<uint32_t>(batch * kw); a.m = s.secret_scratch<uint32_t>(batch * kw);
  }
  a.status = s.out(out_status, batch);
  a.first_index = first_index; a.batch = batch; a.kw = (uint32_t)kw; a.e_len = e_len; a.kind = ZKP_SEEDED_KIND_RANGE_COMMIT; a.max_attempts = RANGE_SAMPLE_MAX_ATTEMPTS;
  int32_t st = s.st;
  if (!st && !a.status) { st = ensure(c, c->scratch[S_SAMPLE_STATUS], batch); a.status = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p; }
  if (!st) st = range_commit_launch(c, n_bits, a);
  if (!st && !reveal) st = zkp_paillier_enc_batch(c, n_bits, batch, a.n, n_stride, a.m, a.r, dcom, ZKP_F_DEVICE_PTRS);
  return s.finish(st);
}

extern "C" int32_t zkp_range_verifier_commit_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, uint32_t e_len,
                                                          const uint8_t* seed, uint64_t first_index, uint32_t* out_com, uint8_t* out_status,
                                                          uint32_t flags) try {
  return range_commit_seeded(c, "zkp_range_verifier_commit_seeded_batch", false, n_bits, batch, n, n_stride, e_len, seed, first_index, out_com, nullptr, nullptr,
                             out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_range_verifier_reveal_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, uint32_t e_len,
                                                          const uint8_t* seed, uint64_t first_index, uint32_t* out_r, uint8_t* out_e, uint8_t* out_status,
                                                          uint32_t flags) try {
  return range_commit_seeded(c, "zkp_range_verifier_reveal_seeded_batch", true, n_bits, batch, n, n_stride, e_len, seed, first_index, nullptr, out_r, out_e,
                             out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_range_verify_commit_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* com,
                                                 const uint32_t* r, const uint8_t* e, const uint8_t* e_len, uint8_t* out_verdict, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || (batch && (!com || !r || !e || !e_len || !out_verdict))) { c->err = "zkp_range_verify_commit_batch: invalid argument"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  RangeCommitArgs a{};
  a.n = s.in(n, n_stride ? batch * kw : kw); a.n_stride = n_stride;
  const uint32_t* dcom = s.in(com, batch * 2 * kw);
  const uint32_t* dr = s.in(r, batch * kw);
  a.e_in = s.in(e, batch * 32); a.e_len_in = s.in(e_len, batch);
  uint8_t* dv = s.out(out_verdict, batch);
  a.m = s.scratch<uint32_t>(batch * kw);           // (r and e are public by now: nothing to wipe)
  a.batch = batch; a.kw = (uint32_t)kw;
  int32_t st = s.st;
  if (!st) st = ensure(c, c->scratch[S_SAMPLE_STATUS], batch);
  a.status = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p;
  if (!st) st = range_commit_launch(c, n_bits, a);
  if (!st) st = zkp_paillier_enc_check_batch(c, n_bits, batch, a.n, n_stride, a.m, dr, nullptr, nullptr, dcom, dv, ZKP_F_DEVICE_PTRS);
  if (!st) st = launch_rows(c, k_range_commit_verdict, batch, dv, (const uint8_t*)a.status, batch);
  return s.finish(st);
} ZKP_CATCH(c)
