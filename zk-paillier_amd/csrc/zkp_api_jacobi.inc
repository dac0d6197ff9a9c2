// zkp_api_jacobi.inc — host side of zkp_jacobi_batch, zkp_legendre_batch and zkp_dlog_statement_setup_seeded_batch (kernels_jacobi.hpp);
// included by zkp_api.hip.  The Jacobi kernel is the new arithmetic; the rest composes launch_modinv and the modexp ladder.

static int32_t launch_jacobi(zkp_ctx* c, uint64_t count, uint32_t kw, const uint32_t* a, const uint32_t* n, uint64_t n_stride, int32_t* symbol, uint8_t* status) {
  return launch_lanes(c, k_jacobi, count, jacobi_lds_words_per_lane(kw), JacobiArgs{a, n, n_stride, symbol, status, count, (int)kw});
}

extern "C" int32_t zkp_jacobi_batch(zkp_ctx* c, uint32_t mod_bits, uint64_t count, const uint32_t* a, const uint32_t* n, uint64_t n_stride,
                                    int32_t* out_symbol, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  const uint64_t kw = mod_bits / 32;
  if ((mod_bits != 1024 && mod_bits != 2048 && mod_bits != 4096 && mod_bits != 8192) || (n_stride != 0 && n_stride != kw) || count > (1ull << 31) ||
      (count && (!a || !n || !out_symbol))) { c->err = "zkp_jacobi_batch: invalid argument"; return ZKP_EINVAL; }
  if (count == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  const uint32_t* da = s.in(a, count * kw);
  const uint32_t* dn = s.in(n, n_stride ? count * kw : kw);
  int32_t* dsym = s.out(out_symbol, count);
  uint8_t* dst = s.out(out_status, count);
  int32_t st = s.st;
  if (!st) st = launch_jacobi(c, count, (uint32_t)kw, da, dn, n_stride, dsym, dst);
  return s.finish(st);
} ZKP_CATCH(c)

// legendre_symbol (wi_dlog_proof.rs:94-107): ls = a^((p - 1) / 2) mod p on the modexp ladder, between the kernel that writes the exponent
// and the one that compares ls with 1
template <int G>
static int32_t legendre_impl(zkp_ctx* c, uint32_t mod_bits, uint64_t count, const LegendreArgs& q, uint32_t* ls) {
  Compose<G> m(c, count, q.p_stride != 0, LdsLayout<G>::NW);
  m.M.setup(q.p, q.p_stride, 0);
  m.M.pow(mod_bits, q.base, q.exp, (uint64_t)q.kw, ls, LdsLayout<G>::NW);
  return m.st;
}

extern "C" int32_t zkp_legendre_batch(zkp_ctx* c, uint32_t mod_bits, uint64_t count, const uint32_t* a, const uint32_t* p, uint64_t p_stride,
                                      int32_t* out_symbol, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  const uint64_t kw = mod_bits / 32;
  if ((mod_bits != 2048 && mod_bits != 4096 && mod_bits != 8192) || (p_stride != 0 && p_stride != kw) || count > (1ull << 31) ||
      (count && (!a || !p || !out_symbol))) { c->err = "zkp_legendre_batch: invalid argument"; return ZKP_EINVAL; }
  if (count == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  LegendreArgs q{};
  q.a = s.in(a, count * kw);
  q.p = s.in(p, p_stride ? count * kw : kw); q.p_stride = p_stride;
  q.symbol = s.out(out_symbol, count);
  q.status = s.out(out_status, count);
  q.count = count; q.kw = (int)kw;
  int32_t st = s.st;
  uint32_t* ls = nullptr;
  if (!st) {
    q.base = (uint32_t*)s.take(count * kw * 4); q.exp = (uint32_t*)s.take(count * kw * 4); ls = (uint32_t*)s.take(count * kw * 4);
    if (!q.status) q.status = (uint8_t*)s.take(count);
    st = s.st;
  }
  if (!st) {
    // (an item outside the domain: base and exponent zero; under an even p the ladder stores nothing, so ls starts as zero)
    HIPCHK(c, hipMemsetAsync(ls, 0, count * kw * 4, c->stream));
    if ((st = launch_rows(c, k_legendre_prep, count, q))) return st;
    st = with_group<GA, GB, GC>(group_for_bits(mod_bits), [&](auto G) { return legendre_impl<G()>(c, mod_bits, count, q, ls); });
  }
  if (!st) {
    q.ls = ls;
    st = launch_rows(c, k_legendre_finish, count, q);
  }
  return s.finish(st);
} ZKP_CATCH(c)

// ni = (h1^-1)^secret mod N under per-statement moduli (an even N: k_setup refuses it and the ladder stores nothing)
template <int G>
static int32_t dlog_setup_impl(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* N, const uint32_t* h1inv, const uint32_t* secret, uint32_t* ni) {
  const uint32_t kw = n_bits / 32;
  Compose<G> m(c, batch, true, kw);
  m.M.setup(N, kw, 0);
  m.M.pow(256, h1inv, secret, 8, ni, (int)kw);
  return m.st;
}

extern "C" int32_t zkp_dlog_statement_setup_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* N, const uint8_t* seed,
                                                         uint64_t first_index, uint32_t* out_g, uint32_t* out_ni, uint32_t* out_secret,
                                                         uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!key_bits_ok(n_bits) || batch > (1ull << 24) || !seed || (batch && (!N || !out_g || !out_ni || !out_secret))) {
    c->err = "zkp_dlog_statement_setup_seeded_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dN = s.in(N, batch * kw);
  const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(key, 32);
  uint32_t *dg = s.out(out_g, batch * kw), *dni = s.out(out_ni, batch * kw), *dsec = s.out(out_secret, batch * 8);
  if (!s.dev) s.secret(dsec, batch * 8 * 4);        // (host arrays: the staged copy is wiped behind the D2H)
  uint8_t* ds = s.out(out_status, batch);
  uint32_t* h1inv = s.secret_scratch<uint32_t>(batch * kw);       // h2 = (h1^-1)^secret: whoever has h1^-1 and h2 is one discrete logarithm from the secret — wiped with it
  uint8_t* invst = s.scratch<uint8_t>(batch);
  if (!ds) ds = s.scratch<uint8_t>(batch);
  int32_t st = s.st;
  if (!st) {
    HIPCHK(c, hipMemsetAsync(dni, 0, batch * kw * 4, c->stream));
    NonceJacobiArgs q{key, dN, dg, dsec, ds, first_index, batch, (uint32_t)kw, ZKP_SEEDED_KIND_DLOG_SETUP, RANGE_SAMPLE_MAX_ATTEMPTS};
    st = launch_lanes(c, k_nonce_jacobi, batch, jacobi_lds_words_per_lane((uint32_t)kw), q);
    // (h1 / N) == -1 implies gcd(h1, N) == 1: every statement that has an h1 has its inverse; the zero h1 of a MALFORMED one gets zero
    if (!st) st = launch_modinv(c, batch, (int)kw, dg, kw, dN, kw, h1inv, kw, invst);
  }
  if (!st) st = with_group<GA, GB>(group_for_bits(n_bits), [&](auto G) { return dlog_setup_impl<G()>(c, n_bits, batch, dN, h1inv, dsec, dni); });
  if (!st) st = launch_rows(c, k_dlog_setup_finish, batch * kw, (const uint8_t*)ds, dni, (uint32_t)kw, (uint64_t)batch);
  return s.finish(st);
} ZKP_CATCH(c)
