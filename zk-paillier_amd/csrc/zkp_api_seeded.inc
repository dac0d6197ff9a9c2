// zkp_api_seeded.inc — seeded proving for ZeroProof, CiphertextProof, CorrectMessageProof and CompositeDLogProof: the nonces the reference's
// prove draws itself are expanded on the device from a 32-byte seed (kernels_sample.hpp: k_nonce_sample; the stream is defined in
// include/zkp_hip.h and DESIGN.md section 4), the nonce-input entry point runs on them as the device-pointer call it already knows, and
// Stage::secret wipes them — with the staged copies of the caller's secrets — on every path out.

static bool nonce_kind_ok(uint32_t kind) { return kind >= ZKP_SEEDED_KIND_ZERO && kind <= ZKP_SEEDED_KIND_DLOG; }

// every pointer is device memory; out[f] is the array of field f (null where the kind has none, or no slots); status is written for every proof
static int32_t nonce_sample_launch(zkp_ctx* c, uint32_t kind, uint32_t n_bits, uint64_t B, uint32_t K, const uint32_t* n, uint64_t n_stride,
                                   const uint32_t* key, uint64_t first_index, uint32_t* const out[4], uint8_t* status) {
  int32_t st;
  if ((st = ensure(c, c->scratch[S_SAMPLE_META], B * 8))) return st;
  NonceSampleArgs a{};
  a.key = key; a.n = kind == ZKP_SEEDED_KIND_DLOG ? nullptr : n; a.n_stride = n_stride;
  a.meta = (uint32_t*)c->scratch[S_SAMPLE_META].p; a.status = status;
  a.first_index = first_index; a.batch = B; a.kw = n_bits / 32; a.kind = kind; a.max_attempts = RANGE_SAMPLE_MAX_ATTEMPTS;
  auto below = [&](uint32_t field, uint32_t per, uint32_t slot0) {
    a.below[a.nbelow] = out[field]; a.below_field[a.nbelow] = field; a.below_per[a.nbelow] = per; a.below_slot0[a.nbelow] = slot0; a.nbelow++;
  };
  switch (kind) {
    case ZKP_SEEDED_KIND_ZERO: below(0, 1, 0); break;
    case ZKP_SEEDED_KIND_CIPHERTEXT: below(0, 1, 0); below(1, 1, 0); break;
    case ZKP_SEEDED_KIND_CORRECT_MESSAGE:
      below(0, 1, 0); below(1, 1, 0); below(3, K - 1, 1);
      a.raw = out[2]; a.raw_field = 2; a.raw_per = K - 1; a.raw_slot0 = 1; a.raw_words = 8;
      break;
    default: a.raw = out[0]; a.raw_field = 0; a.raw_per = 1; a.raw_slot0 = 0; a.raw_words = 16; break;
  }
  hipLaunchKernelGGL(k_nonce_prep, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  const uint64_t G = a.kw / 16;
  uint64_t tasks = 0, fix = 0;
  for (uint32_t k = 0; k < a.nbelow; k++) { tasks += B * a.below_per[k]; fix = std::max<uint64_t>(fix, B * a.below_per[k] * a.kw / 4); }
  if (tasks) {
    const dim3 grid((unsigned)((tasks * G + 255) / 256));
    switch (G) {
      case 2: hipLaunchKernelGGL(k_nonce_sample<2>, grid, dim3(256), 0, c->stream, a); break;
      case 4: hipLaunchKernelGGL(k_nonce_sample<4>, grid, dim3(256), 0, c->stream, a); break;
      default: hipLaunchKernelGGL(k_nonce_sample<8>, grid, dim3(256), 0, c->stream, a); break;
    }
    HIPCHK(c, hipGetLastError());
  }
  if (const uint64_t raw = B * a.raw_per; raw && a.raw_words) {
    hipLaunchKernelGGL(k_nonce_raw, dim3((unsigned)((raw + 255) / 256)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    fix = std::max<uint64_t>(fix, raw * a.raw_words / 4);
  }
  if (a.n && fix) {                      // (a kind without a bound has no MALFORMED case)
    hipLaunchKernelGGL(k_nonce_fixup, dim3((unsigned)((fix + 255) / 256)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
  }
  return ZKP_OK;
}

// the words of one proof's rows of field f, 0 where the kind has no such field
static size_t nonce_field_words(uint32_t kind, uint32_t f, uint32_t kw, uint32_t K) {
  switch (kind) {
    case ZKP_SEEDED_KIND_ZERO: return f == 0 ? kw : 0;
    case ZKP_SEEDED_KIND_CIPHERTEXT: return f <= 1 ? kw : 0;
    case ZKP_SEEDED_KIND_CORRECT_MESSAGE: return f <= 1 ? kw : f == 2 ? (size_t)(K - 1) * 8 : (size_t)(K - 1) * kw;
    default: return f == 0 ? 16 : 0;
  }
}

static bool nonce_args_ok(uint32_t kind, uint32_t n_bits, uint64_t batch, uint32_t K, uint64_t n_stride) {
  if (!nonce_kind_ok(kind) || !sigma_args_ok(n_bits, batch, n_stride)) return false;
  return kind != ZKP_SEEDED_KIND_CORRECT_MESSAGE || (K >= 1 && K <= 65536 && batch * K <= (1ull << 24));
}

extern "C" int32_t zkp_nonce_sample_batch(zkp_ctx* c, uint32_t proof_kind, uint32_t n_bits, uint64_t batch, uint32_t num_messages, const uint32_t* n,
                                          uint64_t n_stride, const uint8_t* seed, uint64_t first_index, uint32_t** out_field,
                                          uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  bool ok = nonce_args_ok(proof_kind, n_bits, batch, num_messages, n_stride) && seed && out_field && (n || proof_kind == ZKP_SEEDED_KIND_DLOG);
  const uint32_t kw = n_bits / 32, K = proof_kind == ZKP_SEEDED_KIND_CORRECT_MESSAGE ? num_messages : 1;
  uintptr_t align = 0;
  for (uint32_t f = 0; ok && f < 4; f++)
    if (nonce_field_words(proof_kind, f, kw, K)) { ok = out_field[f] != nullptr; align |= (uintptr_t)out_field[f]; }
  if (!ok) { c->err = "zkp_nonce_sample_batch: invalid argument"; return ZKP_EINVAL; }
  if ((flags & ZKP_F_DEVICE_PTRS) && (align & 15u)) { c->err = "zkp_nonce_sample_batch: device output arrays must be 16-byte aligned"; return ZKP_EINVAL; }
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
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)

// What the four seeded proves share: the seed and the nonce blocks of a call, all of them secret.  The sampler's status goes to the ctx's
// own array: Zero, Ciphertext and DLog copy it out (their nonce-input calls have no status), CorrectMessage ORs it into the prove's.
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
      if (const size_t bytes = B * nonce_field_words(kind, k, n_bits / 32, K) * 4; bytes && !s.st) { f[k] = (uint32_t*)s.take(bytes); s.secret(f[k], bytes); }
    if ((st = s.st)) return;
    if ((st = ensure(c, c->scratch[S_SAMPLE_STATUS], B))) return;
    status = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p;
    st = nonce_sample_launch(c, kind, n_bits, B, K, dn, n_stride, key, first_index, f, status);
  }
};

// out_status (device, nullable) = / |= the sampler's status
static int32_t seeded_status(zkp_ctx* c, uint8_t* ds, const SeededNonces& q, uint64_t B, bool merge) {
  if (!ds) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (!merge) HIPCHK(c, hipMemsetAsync(ds, 0, B, c->stream));
  hipLaunchKernelGGL(k_or_bytes, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, ds, (const uint8_t*)q.status, B);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

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
  if (!st) st = seeded_status(c, ds, q, batch, false);
  const int32_t fin = s.finish();
  return st ? st : fin;
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
  if (!st) st = seeded_status(c, ds, q, batch, true);
  const int32_t fin = s.finish();
  return st ? st : fin;
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
  if (!st) st = seeded_status(c, ds, q, batch, false);
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)
