// zkp_api_seeded_coprime.inc — seeded proving for VerlinProof and MulProof: the two proofs whose prove redraws a nonce until it is coprime
// to n (verlin_proof.rs:64-67, multiplication_proof.rs:148-154).  The plain sample_below fields of a proof are drawn by k_nonce_prep /
// k_nonce_sample / k_nonce_fixup as they are (kernels_sample.hpp, kinds 5 and 6), the coprime field by k_nonce_coprime
// (kernels_coprime.hpp); the call path is zkp_api_seeded.inc's: the nonce-input entry point runs on the sampled blocks as the
// device-pointer call it already knows, and Stage::secret wipes them, the seed and the staged secrets on every path out.

static bool coprime_kind_ok(uint32_t kind) { return kind == ZKP_SEEDED_KIND_VERLIN || kind == ZKP_SEEDED_KIND_MUL; }
// fields 0 .. count - 2 are sample_below(n), field count - 1 is sample_coprime_below(n); each [B][kw]
static uint32_t coprime_field_count(uint32_t kind) { return kind == ZKP_SEEDED_KIND_VERLIN ? 4 : 2; }

// every pointer is device memory; out[f] is the array of field f; status is written for every proof
static int32_t nonce_coprime_launch(zkp_ctx* c, uint32_t kind, uint32_t n_bits, uint64_t B, const uint32_t* n, uint64_t n_stride, const uint32_t* key,
                                    uint64_t first_index, uint32_t* const out[4], uint8_t* status) {
  int32_t st;
  if ((st = ensure(c, c->scratch[S_SAMPLE_META], B * 8))) return st;
  const uint32_t nf = coprime_field_count(kind), kw = n_bits / 32;
  NonceSampleArgs a{};
  a.key = key; a.n = n; a.n_stride = n_stride;
  a.meta = (uint32_t*)c->scratch[S_SAMPLE_META].p; a.status = status;
  a.first_index = first_index; a.batch = B; a.kw = kw; a.kind = kind; a.max_attempts = RANGE_SAMPLE_MAX_ATTEMPTS;
  for (uint32_t f = 0; f + 1 < nf; f++) { a.below[f] = out[f]; a.below_field[f] = f; a.below_per[f] = 1; a.below_slot0[f] = 0; a.nbelow++; }
  hipLaunchKernelGGL(k_nonce_prep, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  const uint64_t G = kw / 16;
  const dim3 grid((unsigned)((B * a.nbelow * G + 255) / 256));
  switch (G) {
    case 2: hipLaunchKernelGGL(k_nonce_sample<2>, grid, dim3(256), 0, c->stream, a); break;
    case 4: hipLaunchKernelGGL(k_nonce_sample<4>, grid, dim3(256), 0, c->stream, a); break;
    default: hipLaunchKernelGGL(k_nonce_sample<8>, grid, dim3(256), 0, c->stream, a); break;
  }
  HIPCHK(c, hipGetLastError());
  // As launch_modinv: latency-bound work with data-dependent trip counts, so small blocks — divergence stays among 16 lanes, several
  // wavefronts share a compute unit, and two operands per lane are 16 KB of LDS per block at kw = 128.
  const int lanes = 16;
  NonceCoprimeArgs q{key, n, n_stride, a.meta, out[nf - 1], status, first_index, B, kw, kind, nf - 1, RANGE_SAMPLE_MAX_ATTEMPTS};
  hipLaunchKernelGGL(k_nonce_coprime, dim3((unsigned)((B + lanes - 1) / lanes)), dim3(lanes), lanes * coprime_lds_words_per_lane(kw) * 4, c->stream, q);
  HIPCHK(c, hipGetLastError());
  // k_nonce_fixup zeroes its fourth array by (raw_per, raw_words): the coprime field is handed to it as one row of kw words per proof
  a.raw = out[nf - 1]; a.raw_field = nf - 1; a.raw_per = 1; a.raw_slot0 = 0; a.raw_words = kw;
  hipLaunchKernelGGL(k_nonce_fixup, dim3((unsigned)((B * kw / 4 + 255) / 256)), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

extern "C" int32_t zkp_nonce_sample_coprime_batch(zkp_ctx* c, uint32_t proof_kind, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride,
                                                  const uint8_t* seed, uint64_t first_index, uint32_t** out_field, uint8_t* out_status,
                                                  uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  bool ok = coprime_kind_ok(proof_kind) && sigma_args_ok(n_bits, batch, n_stride) && n && seed && out_field;
  const uint32_t kw = n_bits / 32, nf = ok ? coprime_field_count(proof_kind) : 0;
  uintptr_t align = 0;
  for (uint32_t f = 0; ok && f < nf; f++) { ok = out_field[f] != nullptr; align |= (uintptr_t)out_field[f]; }
  if (!ok) { c->err = "zkp_nonce_sample_coprime_batch: invalid argument"; return ZKP_EINVAL; }
  if ((flags & ZKP_F_DEVICE_PTRS) && (align & 15u)) { c->err = "zkp_nonce_sample_coprime_batch: device output arrays must be 16-byte aligned"; return ZKP_EINVAL; }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(key, 32);
  uint32_t* out[4] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t f = 0; f < nf; f++) {
    out[f] = s.out(out_field[f], batch * kw);
    if (!s.dev) s.secret(out[f], batch * kw * 4);      // (host arrays: the staged copies are wiped behind the D2H)
  }
  uint8_t* ds = s.out(out_status, batch);
  int32_t st = s.st;
  if (!st && !ds) { st = ensure(c, c->scratch[S_SAMPLE_STATUS], batch); ds = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p; }
  if (!st) st = nonce_coprime_launch(c, proof_kind, n_bits, batch, dn, n_stride, key, first_index, out, ds);
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)

// The seed and the nonce blocks of a call, all of them secret; the sampler's status goes to the ctx's own array (SeededNonces' twin).
struct CoprimeNonces {
  const uint32_t* key = nullptr;
  uint32_t* f[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* status = nullptr;
  int32_t st = ZKP_OK;
  CoprimeNonces(zkp_ctx* c, Stage& s, uint32_t kind, uint32_t n_bits, uint64_t B, const uint32_t* dn, uint64_t n_stride, const uint8_t* seed,
                uint64_t first_index) {
    key = (const uint32_t*)s.host_in(seed, 32);
    s.secret(key, 32);
    const size_t bytes = B * (n_bits / 32) * 4;
    for (uint32_t k = 0; k < coprime_field_count(kind) && !s.st; k++) { f[k] = (uint32_t*)s.take(bytes); s.secret(f[k], bytes); }
    if ((st = s.st)) return;
    if ((st = ensure(c, c->scratch[S_SAMPLE_STATUS], B))) return;
    status = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p;
    st = nonce_coprime_launch(c, kind, n_bits, B, dn, n_stride, key, first_index, f, status);
  }
};

// out_status (device, nullable) = / |= the sampler's status
static int32_t coprime_status(zkp_ctx* c, uint8_t* ds, const CoprimeNonces& q, uint64_t B, bool merge) {
  if (!ds) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (!merge) HIPCHK(c, hipMemsetAsync(ds, 0, B, c->stream));
  hipLaunchKernelGGL(k_or_bytes, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, ds, (const uint8_t*)q.status, B);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

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
  CoprimeNonces q(c, s, ZKP_SEEDED_KIND_VERLIN, n_bits, batch, dn, n_stride, seed, first_index);
  int32_t st = q.st;      // (a null statement, witness or output is refused by the nonce-input call: ZKP_EINVAL, after the sampler ran)
  if (!st) st = zkp_verlin_proof_prove_batch(c, n_bits, batch, dn, n_stride, dc, dcp, dphx, dx, dxp, dxpp, drx, q.f[0], q.f[1], q.f[2], q.f[3], dpa, dz, dzp,
                                             dzpp, drz, ZKP_F_DEVICE_PTRS);
  if (!st) st = coprime_status(c, ds, q, batch, false);
  const int32_t fin = s.finish();
  return st ? st : fin;
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
  CoprimeNonces q(c, s, ZKP_SEEDED_KIND_MUL, n_bits, batch, dn, n_stride, seed, first_index);
  int32_t st = q.st;      // (a null statement, witness or output is refused by the nonce-input call: ZKP_EINVAL, after the sampler ran)
  if (!st) st = zkp_mul_proof_prove_batch(c, n_bits, batch, dn, n_stride, dea, deb, dec, da, db, dra, drb, drc, q.f[0], q.f[1], df, dz1, dz2, ded, dedb, ds,
                                          ZKP_F_DEVICE_PTRS);
  if (!st) st = coprime_status(c, ds, q, batch, true);
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)
