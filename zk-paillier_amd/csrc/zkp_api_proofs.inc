// zkp_api_proofs.inc — proof-level entry points of the C ABI (included by zkp_api.hip).

// which arrays of the struct a call dereferences
enum : unsigned { RA_RANGE = 1, RA_CIPHERTEXT = 2, RA_PAIRS = 4, RA_RESP = 8 };
static bool range_args_ok(const zkp_range_ni_proofs* p, unsigned need = RA_RANGE | RA_CIPHERTEXT | RA_PAIRS | RA_RESP) {
  if (!p) return false;
  if (!key_bits_ok(p->n_bits)) return false;
  if (p->batch > (1ull << 24) || p->error_factor > 256) return false;   // challenge has at most 256 bits
  if (p->n_stride != 0 && p->n_stride != p->n_bits / 32) return false;
  if (p->batch == 0) return true;
  if (!p->n || ((need & RA_RANGE) && !p->range) || ((need & RA_CIPHERTEXT) && !p->ciphertext)) return false;
  if (p->error_factor && (need & RA_PAIRS) && (!p->c1 || !p->c2)) return false;
  if (p->error_factor && (need & RA_RESP) && (!p->resp_kind || !p->resp_j || !p->resp_w1 || !p->resp_r1 || !p->resp_w2 || !p->resp_r2)) return false;
  return true;
}

// proofs [lo, lo + count) of `p` at EF rows per proof, and their witness: a batch is structure-of-arrays, so a slice of it is one too
static zkp_range_ni_proofs range_slice(const zkp_range_ni_proofs& p, size_t EF, uint64_t lo, uint64_t count) {
  const size_t kw = p.n_bits / 32;
  zkp_range_ni_proofs q = p;
  q.batch = count;
  if (q.n) q.n += lo * p.n_stride;
  if (q.range) q.range += lo * kw;
  if (q.ciphertext) q.ciphertext += lo * 2 * kw;
  for (uint32_t** a : {&q.c1, &q.c2}) if (*a) *a += lo * EF * 2 * kw;
  for (uint8_t** a : {&q.resp_kind, &q.resp_j}) if (*a) *a += lo * EF;
  for (uint32_t** a : {&q.resp_w1, &q.resp_r1, &q.resp_w2, &q.resp_r2}) if (*a) *a += lo * EF * kw;
  return q;
}
static zkp_range_ni_witness range_witness_slice(const zkp_range_ni_witness& w, size_t kw, size_t EF, uint64_t lo) {
  zkp_range_ni_witness q = w;
  for (const uint32_t** a : {&q.x, &q.r}) if (*a) *a += lo * kw;
  for (const uint32_t** a : {&q.w1, &q.w2, &q.r1, &q.r2}) if (*a) *a += lo * EF * kw;
  return q;
}

template <int G>
static int32_t range_hash(zkp_ctx* c, const zkp_range_ni_proofs& p, uint8_t* e, uint8_t* elen, uint8_t* verdict, uint8_t ok_value,
                          const uint8_t* e_in = nullptr, const uint8_t* e_len_in = nullptr, hipStream_t stream = nullptr, RangeHashArgs* args_only = nullptr) {
  const uint32_t kw = p.n_bits / 32;
  int32_t st;
  if ((st = ensure(c, c->scratch[S_T1], p.batch * kw * 4))) return st;
  if ((st = ensure(c, c->scratch[S_T2], p.batch * kw * 4))) return st;
  RangeHashArgs a{p.n, p.n_stride, p.c1, p.c2, p.range, kw, p.error_factor, p.batch, e, elen,
                  (uint32_t*)c->scratch[S_T1].p, (uint32_t*)c->scratch[S_T2].p, verdict, ok_value, e_in, e_len_in};
  if (args_only) { *args_only = a; return ZKP_OK; }          // (the caller launches it: the hashes travel with its Enc launch)
  if (!e_in && p.batch <= 4ull * (uint64_t)c->route.cus) {
    // a few proofs: one wavefront per proof, the message schedule spread over its lanes (kernels_proofs.hpp: WaveSha)
    hipLaunchKernelGGL(k_range_hash_wave, dim3((unsigned)p.batch), dim3(64), hw_lds_words((int)kw) * sizeof(uint32_t), stream ? stream : c->stream, a);
  } else {
    const size_t hash_lds_bytes = (16 * HASH_PROOFS + HASH_PROOFS * (2 * kw + 1)) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_range_hash, dim3((unsigned)((p.batch + HASH_PROOFS - 1) / HASH_PROOFS)), dim3(HASH_PROOFS), hash_lds_bytes, stream ? stream : c->stream, a);
  }
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

// phases: 1 = generate_encrypted_pairs, 2 = challenge + generate_proof; e_in != nullptr: challenge supplied by the caller
template <int G>
static int32_t range_prove_impl(zkp_ctx* c, const zkp_range_ni_proofs& p, const zkp_range_ni_witness& w, uint8_t* e, uint8_t* elen, uint8_t* status,
                                uint32_t EF = ZKP_SECURITY_PARAMETER, int phases = 3, const uint8_t* e_in = nullptr, const uint8_t* e_len_in = nullptr) {
  using CL = ConstLayout<G>;
  constexpr int GN = N_GROUP<G>;
  const uint32_t kw = p.n_bits / 32;
  const uint64_t nkeys = p.n_stride ? p.batch : 1;
  int32_t st;
  const uint64_t items = p.batch * EF;
  if (items == 0) return ZKP_OK;
  if (phases & 1) {
  if ((st = run_setup<G>(c, p.n, p.n_stride, (int)kw, 1, nkeys, c->consts))) return st;      // modulus n^2
  // generate_encrypted_pairs (range_proof.rs:161-187): c1 = Enc(w1, r1), c2 = Enc(w2, r2)
  unsigned blocks = 0;
  if ((st = table_for<G>(c, k_enc<G, true>, 2 * items, &blocks))) return st;
  const uint8_t* sched = nullptr;
  if (p.n_stride == 0 && !pair_ladder(c->route, G, 2 * items) && (st = build_schedule(c, p.n, p.n_bits, &sched))) return st;   // (the pair ladder reads n itself)
  {
    // ONE launch over the 2 * B * EF encryptions of both halves: a group takes ~0.1 s per Enc, so every launch
    // ramps up and drains with idle lanes; one ramp instead of two (measured +1.2 % proofs/s)
    EncArgs a{};
    a.sched = sched;
    a.n = p.n; a.n_stride = p.n_stride; a.consts = (const uint32_t*)c->consts.p; a.const_stride = p.n_stride ? (uint64_t)CL::WORDS : 0;
    a.table = (uint32_t*)c->table.p; a.count = 2 * items; a.half = items; a.n_bits = (int)p.n_bits; a.mode = 0;
    a.m = w.w1; a.r = w.r1; a.out = p.c1; a.m2 = w.w2; a.r2 = w.r2; a.out2 = p.c2; a.items_per_key = EF;
    if ((st = fresh_work_counter(c, &a.work_counter))) return st;
    TimedRegion tr(c, 2 * items);
    launch_k_enc<G>(c, blocks, a);
  }
  HIPCHK(c, hipGetLastError());
  }
  if (!(phases & 2)) return ZKP_OK;
  if ((st = run_setup<GN>(c, p.n, p.n_stride, (int)kw, 0, nkeys, c->consts2))) return st;    // modulus n
  zkp_range_ni_proofs pp = p;
  pp.error_factor = EF;
  if ((st = range_hash<G>(c, pp, e, elen, status, 0, e_in, e_len_in))) return st;
  // generate_proof (range_proof.rs:210-252)
  ResponseArgs r{};
  r.consts = (const uint32_t*)c->consts2.p; r.const_stride = p.n_stride ? (uint64_t)ConstLayout<GN>::WORDS : 0;
  r.x = w.x; r.r = w.r; r.w1 = w.w1; r.w2 = w.w2; r.r1 = w.r1; r.r2 = w.r2;
  r.e = e; r.third = (const uint32_t*)c->scratch[S_T1].p; r.two_thirds = (const uint32_t*)c->scratch[S_T2].p;
  r.resp_kind = p.resp_kind; r.resp_j = p.resp_j; r.resp_w1 = p.resp_w1; r.resp_r1 = p.resp_r1; r.resp_w2 = p.resp_w2; r.resp_r2 = p.resp_r2;
  r.status = status; r.kw = kw; r.ef = EF; r.batch = p.batch;
  using LN = LdsLayoutFull<GN>;
  const unsigned rblocks = (unsigned)((items + LN::GROUPS_PER_BLOCK - 1) / LN::GROUPS_PER_BLOCK);
  hipLaunchKernelGGL(k_range_responses<GN>, dim3(rblocks), dim3(LN::THREADS), LN::BYTES_PER_BLOCK, c->stream, r);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

// phases 1 = generate_encrypted_pairs, 2 = generate_proof, 3 = RangeProofNi::prove
static int32_t range_prove_entry(zkp_ctx* c, const char* name, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w, uint32_t ef, int phases,
                                 const uint8_t* e_in, const uint8_t* e_len_in, uint8_t* out_e, uint8_t* out_e_len, uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  // generate_encrypted_pairs reads (n, w1, w2, r1, r2) and writes (c1, c2); generate_proof reads (n, range, x, r, w*, r*, e)
  // and writes resp_*; the ciphertext is not read by any prover function (the reference only clones it into the proof)
  const unsigned need = ((phases & 1) ? RA_PAIRS : 0) | ((phases & 2) ? RA_RANGE | RA_RESP : 0);
  if (!range_args_ok(p, need) || !w || (p->batch && ef && (!w->w1 || !w->w2 || !w->r1 || !w->r2 || ((phases & 2) && (!w->x || !w->r)))) ||
      (e_in && !e_len_in)) {
    c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL;
  }
  if (p->batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = p->n_bits / 32, B = p->batch, EF = ef, rows = B * EF;
  Stage s(c, flags);
  const std::vector<size_t> blocks = (s.dev || !(phases & 1)) ? std::vector<size_t>() : host_blocks(c, B, EF, false);
  c->last_host_blocks = blocks.empty() ? 1 : (int)blocks.size() - 1;
  if (!blocks.empty()) {
    // host arrays, a large batch: block k + 1 is copied in and block k - 1 copied out while the kernels of block k run (Piped, zkp_api.hip)
    Piped pp(c, s);
    zkp_range_ni_proofs d = *p;
    d.n = p->n_stride ? pp.in(p->n, kw, B) : s.in(p->n, kw);
    if (phases & 2) d.range = pp.in(p->range, kw, B);
    d.c1 = pp.out(p->c1, EF * 2 * kw, B); d.c2 = pp.out(p->c2, EF * 2 * kw, B);
    if (phases & 2) {
      d.resp_kind = pp.out(p->resp_kind, EF, B); d.resp_j = pp.out(p->resp_j, EF, B);
      d.resp_w1 = pp.out(p->resp_w1, EF * kw, B); d.resp_r1 = pp.out(p->resp_r1, EF * kw, B);
      d.resp_w2 = pp.out(p->resp_w2, EF * kw, B); d.resp_r2 = pp.out(p->resp_r2, EF * kw, B);
    }
    zkp_range_ni_witness dw = *w;
    if (phases & 2) { dw.x = pp.in(w->x, kw, B); dw.r = pp.in(w->r, kw, B); }
    dw.w1 = pp.in(w->w1, EF * kw, B); dw.w2 = pp.in(w->w2, EF * kw, B); dw.r1 = pp.in(w->r1, EF * kw, B); dw.r2 = pp.in(w->r2, EF * kw, B);
    uint8_t* de = pp.out(out_e, 32, B);
    uint8_t* dl = pp.out(out_e_len, 1, B);
    uint8_t* ds = pp.out(out_status, 1, B);
    const uint8_t* dei = pp.in(e_in, 32, B);
    const uint8_t* deli = pp.in(e_len_in, 1, B);
    int32_t st = s.st;
    if (!st && !de) { st = ensure(c, c->scratch[S_E], B * 32); de = (uint8_t*)c->scratch[S_E].p; }
    if (!st && !dl) { st = ensure(c, c->scratch[S_ELEN], B); dl = (uint8_t*)c->scratch[S_ELEN].p; }
    if (!st && !ds) { st = ensure(c, c->scratch[S_STATUS], B); ds = (uint8_t*)c->scratch[S_STATUS].p; }
    const size_t nb = blocks.size() - 1;
    if (!st) st = pp.streams(nb);
    if (!st) st = pp.h2d(blocks[0], blocks[1], c->ev_pipe[0]);
    for (size_t k = 0; k < nb && !st; k++) {
      const size_t lo = blocks[k], hi = blocks[k + 1];
      // (arrays the phases do not read are the caller's own pointers here: sliced like the rest, and as little dereferenced)
      const zkp_range_ni_proofs q = range_slice(d, EF, lo, hi - lo);
      const zkp_range_ni_witness qw = range_witness_slice(dw, kw, EF, lo);
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_pipe[2 * k], 0));
      const uint8_t* qe = dei ? dei + lo * 32 : nullptr;
      const uint8_t* ql = deli ? deli + lo : nullptr;
      st = with_group<GA, GB, GC>(group_for_bits(2 * p->n_bits), [&](auto G) { return range_prove_impl<G()>(c, q, qw, de + lo * 32, dl + lo, ds + lo, ef, phases, qe, ql); });
      if (st) break;
      HIPCHK(c, hipEventRecord(c->ev_pipe[2 * k + 1], c->stream));
      if (k + 1 < nb) st = pp.h2d(blocks[k + 1], blocks[k + 2], c->ev_pipe[2 * k + 2]);     // (under the kernels of block k)
    }
    for (size_t k = 0; k < nb && !st; k++) st = pp.d2h(blocks[k], blocks[k + 1], c->ev_pipe[2 * k + 1]);
    const int32_t fc = pp.finish();
    return s.finish(st ? st : fc);
  }
  zkp_range_ni_proofs d = *p;
  d.n = s.in(p->n, p->n_stride ? B * kw : kw);
  if (phases & 2) d.range = s.in(p->range, B * kw);
  // phase 1 writes c1/c2; phase 2 with a supplied challenge never touches them (no hashing), so they are not staged
  if (phases & 1) { d.c1 = s.out(p->c1, rows * 2 * kw); d.c2 = s.out(p->c2, rows * 2 * kw); }
  if (phases & 2) {                // phase 1 alone leaves the caller's response arrays untouched
    d.resp_kind = s.out(p->resp_kind, rows); d.resp_j = s.out(p->resp_j, rows);
    d.resp_w1 = s.out(p->resp_w1, rows * kw); d.resp_r1 = s.out(p->resp_r1, rows * kw);
    d.resp_w2 = s.out(p->resp_w2, rows * kw); d.resp_r2 = s.out(p->resp_r2, rows * kw);
  }
  zkp_range_ni_witness dw = *w;
  if (phases & 2) { dw.x = s.in(w->x, B * kw); dw.r = s.in(w->r, B * kw); }
  dw.w1 = s.in(w->w1, rows * kw); dw.w2 = s.in(w->w2, rows * kw); dw.r1 = s.in(w->r1, rows * kw); dw.r2 = s.in(w->r2, rows * kw);
  uint8_t* de = s.out(out_e, B * 32);
  uint8_t* dl = s.out(out_e_len, B);
  uint8_t* ds = s.out(out_status, B);
  const uint8_t* dei = s.in(e_in, B * 32);
  const uint8_t* deli = s.in(e_len_in, B);
  int32_t st = s.st;
  if (!st && !de) { st = ensure(c, c->scratch[S_E], B * 32); de = (uint8_t*)c->scratch[S_E].p; }
  if (!st && !dl) { st = ensure(c, c->scratch[S_ELEN], B); dl = (uint8_t*)c->scratch[S_ELEN].p; }
  if (!st && !ds) { st = ensure(c, c->scratch[S_STATUS], B); ds = (uint8_t*)c->scratch[S_STATUS].p; }
  if (!st && ef == 0) HIPCHK(c, hipMemsetAsync(ds, 0, B, c->stream));   // no rows: nothing can go wrong
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * p->n_bits), [&](auto G) { return range_prove_impl<G()>(c, d, dw, de, dl, ds, ef, phases, dei, deli); });
  return s.finish(st);
}

// ---- a RangeProofNi call as TWO concurrent calls: where route_plan.hpp's range_split cuts it ------------------------------------------------
#ifndef ZKP_SECONDARY_ENGINE
static RangeSplit range_split_plan(zkp_ctx* c, const zkp_range_ni_proofs* p, uint64_t rows_per_proof, bool listed = false) {
  return (c && p) ? range_split(c->route, p->batch, rows_per_proof, p->n_bits, p->n_stride, listed) : RangeSplit();
}
static int32_t range_split_ctx(zkp_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->split_ctx) {
    if (!c->split_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->split_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : c->ev_split) if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int32_t st = c->eng[0]->p_zkp_ctx_create_on_stream(c->device, (void*)c->split_stream, &c->split_ctx);
    if (st) { c->split_ctx = nullptr; c->err = "the second latency-engine ctx of a split call could not be created"; return st; }
    if (c->timing) (void)c->eng[0]->p_zkp_timing_reset(c->split_ctx, 1);      // (created inside a timed region: it is timed from its first call)
  }
  (void)c->eng[0]->p_zkp_diag_set_enc_form(c->split_ctx, c->route.enc_form);
  (void)c->eng[0]->p_zkp_diag_set_r2l(c->split_ctx, c->route.r2l);
  (void)c->eng[0]->p_zkp_diag_set_r2l_lanes(c->split_ctx, c->route.r2l_lanes ? c->route.r2l_lanes : 12);      // (beside a head that fills every SIMD the tail keeps ONE wavefront per Enc: the sizes of range_split were measured that way)
  (void)c->eng[0]->p_zkp_diag_set_key_cache(c->split_ctx, c->key_cache);
  // (the tail runs BESIDE a head that fills the chip: the transcript hashes stay in a launch of their own there — aboard the tail's Enc launch their
  //  22.8 KB of LDS per workgroup no longer fit beside the head's workgroups: 20 proofs verified in 34.7 ms instead of 22.5)
  (void)c->eng[0]->p_zkp_diag_set_fuse_hash(c->split_ctx, 0);
  return ZKP_OK;
}
// the second ctx is there (or could be made); a failure is not an error of the call — it runs as ONE call, as before — so it leaves no message
static bool range_split_ready(zkp_ctx* c) {
  if (range_split_ctx(c) == ZKP_OK) return true;
  c->err.clear();
  return false;
}
// run `head_call` (mid engine, this thread, the ctx's stream) and `tail_call` (latency engine, helper thread, the split stream) side by side
template <class FH, class FT> static int32_t range_split_run(zkp_ctx* c, int head_engine, uint64_t tail_proofs, FH head_call, FT tail_call) {
  // what the caller enqueued on the ctx's stream (device-resident inputs) comes first on both streams
  HIPCHK(c, hipEventRecord(c->ev_split[0], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->split_stream, c->ev_split[0], 0));
  if (head_engine >= 0) { select_engine(c, head_engine); c->last_geometry = c->eng[head_engine]->limbs_per_lane; }
  else c->last_geometry = W;
  int32_t st_tail = ZKP_OK;
  std::string err_tail;
  std::exception_ptr thrown;
  std::thread helper([&] {
    try {
      (void)hipSetDevice(c->device);
      st_tail = tail_call(c->eng[0], c->split_ctx);
      if (st_tail) err_tail = c->eng[0]->p_zkp_last_error_string(c->split_ctx);
    } catch (...) { thrown = std::current_exception(); }
  });
  int32_t st_head = ZKP_OK;
  try { st_head = head_engine >= 0 ? head_call(c->eng[head_engine], c->eng_ctx[head_engine]) : head_call(nullptr, c); } catch (...) { helper.join(); throw; }
  helper.join();
  if (thrown) std::rethrow_exception(thrown);
  // ... and what follows on the ctx's stream waits for the tail
  HIPCHK(c, hipEventRecord(c->ev_split[1], c->split_stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_split[1], 0));
  c->last_split = (int)tail_proofs;
  if (st_head) { if (head_engine >= 0) c->err = c->eng[head_engine]->p_zkp_last_error_string(c->eng_ctx[head_engine]); return st_head; }
  if (st_tail) { c->err = err_tail; return st_tail; }
  return ZKP_OK;
}
#define ZKP_RANGE_SPLIT_RESET(c) if (c) (c)->last_split = 0;
#else
#define ZKP_RANGE_SPLIT_RESET(c)
#endif

extern "C" int32_t zkp_range_ni_prove_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w, uint8_t* out_e,
                                            uint8_t* out_e_len, uint8_t* out_status, uint32_t flags) try {
  ZKP_RANGE_SPLIT_RESET(c)
#ifndef ZKP_SECONDARY_ENGINE
  if (const RangeSplit sp = (p && w && p->error_factor == ZKP_SECURITY_PARAMETER && range_args_ok(p, RA_PAIRS | RA_RANGE | RA_RESP) && w->x && w->r && w->w1 && w->w2 && w->r1 && w->r2)
                                ? range_split_plan(c, p, 2 * ZKP_SECURITY_PARAMETER) : RangeSplit(); sp.head && range_split_ready(c)) {      // (no second ctx: one call, as before)
    const size_t kw = p->n_bits / 32, EF = ZKP_SECURITY_PARAMETER;
    const uint64_t head = sp.head, tail = p->batch - head;
    auto part = [&](const LatEngine* e, zkp_ctx* ec, uint64_t lo, uint64_t count) {
      const zkp_range_ni_proofs q = range_slice(*p, EF, lo, count);
      const zkp_range_ni_witness qw = range_witness_slice(*w, kw, EF, lo);
      uint8_t* qe = out_e ? out_e + lo * 32 : nullptr; uint8_t* ql = out_e_len ? out_e_len + lo : nullptr; uint8_t* qs = out_status ? out_status + lo : nullptr;
      if (!e) return range_prove_entry(ec, "zkp_range_ni_prove_batch", &q, &qw, ZKP_SECURITY_PARAMETER, 3, nullptr, nullptr, qe, ql, qs, flags);      // (the head on this very ctx)
      return e->p_zkp_range_ni_prove_batch(ec, &q, &qw, qe, ql, qs, flags);
    };
    return range_split_run(c, sp.head_engine, tail, [&](const LatEngine* e, zkp_ctx* ec) { return part(e, ec, 0, head); }, [&](const LatEngine* e, zkp_ctx* ec) { return part(e, ec, head, tail); });
  }
#endif
  ZKP_ROUTE_ENC(c, p ? p->batch * 2 * ZKP_SECURITY_PARAMETER : 0, p ? 2 * p->n_bits : 0, p && p->n_stride == 0, zkp_range_ni_prove_batch, p, w, out_e, out_e_len, out_status, flags)
  return range_prove_entry(c, "zkp_range_ni_prove_batch", p, w, ZKP_SECURITY_PARAMETER, 3, nullptr, nullptr, out_e, out_e_len, out_status, flags);
} ZKP_CATCH(c)
// ---- seeded proving: the witness expanded on the device (kernels_sample.hpp) -----------------------------------------------------------
enum { RANGE_SAMPLE_MAX_ATTEMPTS = 128 };

// every pointer is device memory; `d` supplies n_bits, batch, n, n_stride and range; status is written for every proof
static int32_t range_sample_launch(zkp_ctx* c, const zkp_range_ni_proofs& d, uint32_t ef, const uint32_t* key, uint64_t first_index,
                                   uint32_t* w1, uint32_t* w2, uint32_t* r1, uint32_t* r2, uint8_t* status) {
  const uint32_t kw = d.n_bits / 32;
  const uint64_t B = d.batch, rows = B * ef;
  int32_t st;
  if ((st = ensure(c, c->scratch[S_SAMPLE_THIRD], B * kw * 4))) return st;
  if ((st = ensure(c, c->scratch[S_SAMPLE_META], B * 8))) return st;
  RangeSampleArgs a{};
  a.key = key; a.n = d.n; a.n_stride = d.n_stride; a.range = d.range;
  a.third = (uint32_t*)c->scratch[S_SAMPLE_THIRD].p; a.meta = (uint32_t*)c->scratch[S_SAMPLE_META].p;
  a.w1 = w1; a.w2 = w2; a.r1 = r1; a.r2 = r2; a.status = status;
  a.first_index = first_index; a.batch = B; a.kw = kw; a.ef = ef; a.max_attempts = RANGE_SAMPLE_MAX_ATTEMPTS;
  if ((st = launch_rows(c, k_range_sample_prep, B, a))) return st;
  if (rows == 0) return ZKP_OK;
  const uint64_t G = kw / 16;
  const unsigned sample_blocks = (unsigned)((3 * rows * G + 255) / 256), fix_blocks = (unsigned)((rows * G + 255) / 256);
  switch (G) {
    case 2: hipLaunchKernelGGL(k_range_sample<2>, dim3(sample_blocks), dim3(256), 0, c->stream, a);
            hipLaunchKernelGGL(k_range_sample_fixup<2>, dim3(fix_blocks), dim3(256), 0, c->stream, a); break;
    case 4: hipLaunchKernelGGL(k_range_sample<4>, dim3(sample_blocks), dim3(256), 0, c->stream, a);
            hipLaunchKernelGGL(k_range_sample_fixup<4>, dim3(fix_blocks), dim3(256), 0, c->stream, a); break;
    default: hipLaunchKernelGGL(k_range_sample<8>, dim3(sample_blocks), dim3(256), 0, c->stream, a);
             hipLaunchKernelGGL(k_range_sample_fixup<8>, dim3(fix_blocks), dim3(256), 0, c->stream, a); break;
  }
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

// out_status (device, nullable) = / |= the status of the sampler that ran in front of the prove
static int32_t seeded_status(zkp_ctx* c, uint8_t* ds, const uint8_t* sampler_status, uint64_t B, bool merge) {
  if (!ds) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (!merge) HIPCHK(c, hipMemsetAsync(ds, 0, B, c->stream));
  return launch_rows(c, k_or_bytes, B, ds, sampler_status, B);
}

extern "C" int32_t zkp_range_sample_witness_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const uint8_t* seed, uint64_t first_index,
                                                  uint32_t* out_w1, uint32_t* out_w2, uint32_t* out_r1, uint32_t* out_r2, uint8_t* out_status,
                                                  uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!range_args_ok(p, RA_RANGE) || !seed || (p->batch && p->error_factor && (!out_w1 || !out_w2 || !out_r1 || !out_r2))) {
    c->err = "zkp_range_sample_witness_batch: invalid argument"; return ZKP_EINVAL;
  }
  if ((flags & ZKP_F_DEVICE_PTRS) && ((((uintptr_t)out_w1 | (uintptr_t)out_w2 | (uintptr_t)out_r1 | (uintptr_t)out_r2) & 15u) != 0)) {
    c->err = "zkp_range_sample_witness_batch: device output arrays must be 16-byte aligned"; return ZKP_EINVAL;
  }
  if (p->batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = p->n_bits / 32, B = p->batch, rows = B * p->error_factor;
  Stage s(c, flags);
  zkp_range_ni_proofs d = *p;
  d.n = s.in(p->n, p->n_stride ? B * kw : kw);
  d.range = s.in(p->range, B * kw);
  const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(key, 32);
  uint32_t* w[4] = {out_w1, out_w2, out_r1, out_r2};
  for (auto& q : w) { q = s.out(q, rows * kw); if (!s.dev) s.secret(q, rows * kw * 4); }      // (host arrays: the staged copies are wiped behind the D2H)
  uint8_t* ds = s.out(out_status, B);
  int32_t st = s.st;
  if (!st && !ds) { st = ensure(c, c->scratch[S_SAMPLE_STATUS], B); ds = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p; }
  if (!st) st = range_sample_launch(c, d, p->error_factor, key, first_index, w[0], w[1], w[2], w[3], ds);
  return s.finish(st);
} ZKP_CATCH(c)

extern "C" int32_t zkp_range_ni_prove_seeded_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const uint32_t* x, const uint32_t* r, const uint8_t* seed,
                                                   uint64_t first_index, uint8_t* out_e, uint8_t* out_e_len, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!range_args_ok(p, RA_PAIRS | RA_RANGE | RA_RESP) || !seed) { c->err = "zkp_range_ni_prove_seeded_batch: invalid argument"; return ZKP_EINVAL; }
  if (p->batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = p->n_bits / 32, B = p->batch, EF = ZKP_SECURITY_PARAMETER, rows = B * EF;
  // Everything is made device-resident HERE (a host-pointer call stages its statement, x, r and outputs in blocks of this ctx), the sampler
  // fills four more blocks, and zkp_range_ni_prove_batch runs as the device-pointer call it already knows: routing, split plans, the key
  // cache and the kernels are those of that entry point.  `s` wipes what is secret on every path out (Stage::secret).
  Stage s(c, flags);
  zkp_range_ni_proofs d = *p;
  d.n = s.in(p->n, p->n_stride ? B * kw : kw);
  d.range = s.in(p->range, B * kw);
  if (!s.dev) d.ciphertext = nullptr;                  // (no prover function reads it)
  d.c1 = s.out(p->c1, rows * 2 * kw); d.c2 = s.out(p->c2, rows * 2 * kw);
  d.resp_kind = s.out(p->resp_kind, rows); d.resp_j = s.out(p->resp_j, rows);
  d.resp_w1 = s.out(p->resp_w1, rows * kw); d.resp_r1 = s.out(p->resp_r1, rows * kw);
  d.resp_w2 = s.out(p->resp_w2, rows * kw); d.resp_r2 = s.out(p->resp_r2, rows * kw);
  const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(key, 32);
  zkp_range_ni_witness dw{};
  uint32_t* wit[4] = {nullptr, nullptr, nullptr, nullptr};
  for (auto& q : wit) q = s.secret_scratch<uint32_t>(rows * kw);
  dw.w1 = wit[0]; dw.w2 = wit[1]; dw.r1 = wit[2]; dw.r2 = wit[3];
  dw.x = s.in(x, B * kw); dw.r = s.in(r, B * kw);
  if (!s.dev) { s.secret(dw.x, B * kw * 4); s.secret(dw.r, B * kw * 4); }
  uint8_t* de = s.out(out_e, B * 32);
  uint8_t* dl = s.out(out_e_len, B);
  uint8_t* ds = s.out(out_status, B);
  int32_t st = s.st;
  if (!st) st = ensure(c, c->scratch[S_SAMPLE_STATUS], B);
  uint8_t* sampler_status = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p;
  if (!st) st = range_sample_launch(c, d, (uint32_t)EF, key, first_index, wit[0], wit[1], wit[2], wit[3], sampler_status);
  if (!st) st = zkp_range_ni_prove_batch(c, &d, &dw, de, dl, ds, ZKP_F_DEVICE_PTRS);      // (a null x or r is refused there: ZKP_EINVAL, after the sampler ran)
  if (!st) st = seeded_status(c, ds, sampler_status, B, true);
  return s.finish(st);
} ZKP_CATCH(c)

extern "C" int32_t zkp_diag_witness_residue(zkp_ctx* c, uint64_t* out_nonzero_words) try {
  if (!c || !out_nonzero_words) return ZKP_EINVAL;
  *out_nonzero_words = 0;
#ifndef ZKP_SECONDARY_ENGINE
  // the most recent call with secrets ran whole on a secondary engine's twin ctx: its blocks, its wipe, its answer
  if (c->wiped_on >= 0 && c->eng[c->wiped_on] && c->eng_ctx[c->wiped_on]) {
    const int32_t st = c->eng[c->wiped_on]->p_zkp_diag_witness_residue(c->eng_ctx[c->wiped_on], out_nonzero_words);
    if (st) { try { c->err = c->eng[c->wiped_on]->p_zkp_last_error_string(c->eng_ctx[c->wiped_on]); } catch (...) {} }
    return st;
  }
#endif
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->last_wiped.empty()) return ZKP_OK;
  int32_t st = ensure(c, c->scratch[S_RESIDUE], 8);
  if (st) return st;
  unsigned long long* count = (unsigned long long*)c->scratch[S_RESIDUE].p;
  HIPCHK(c, hipMemsetAsync(count, 0, 8, c->stream));
  for (auto& w : c->last_wiped) {
    bool cached = false;                                // only memory the ctx still owns is read
    for (auto& b : c->stage_free) cached = cached || ((char*)w.first >= (char*)b.p && (char*)w.first + w.second <= (char*)b.p + b.cap);
    if (!cached) { c->err = "zkp_diag_witness_residue: the blocks of the last seeded call have left the staging cache"; return ZKP_EINVAL; }
    const uint64_t words = w.second / 4;
    const unsigned blocks = (unsigned)std::min<uint64_t>((words + 255) / 256, 4096);
    hipLaunchKernelGGL(k_count_nonzero, dim3(blocks), dim3(256), 0, c->stream, (const uint32_t*)w.first, words, count);
    HIPCHK(c, hipGetLastError());
  }
  unsigned long long host = 0;
  HIPCHK(c, hipMemcpyAsync(&host, count, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out_nonzero_words = host;
  return ZKP_OK;
} ZKP_CATCH(c)

extern "C" int32_t zkp_range_generate_encrypted_pairs_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w, uint32_t flags) try {
  ZKP_ROUTE_ENC(c, p ? p->batch * 2 * p->error_factor : 0, p ? 2 * p->n_bits : 0, p && p->n_stride == 0, zkp_range_generate_encrypted_pairs_batch, p, w, flags)
  return range_prove_entry(c, "zkp_range_generate_encrypted_pairs_batch", p, w, p ? p->error_factor : 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_range_generate_proof_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w, const uint8_t* e,
                                                  const uint8_t* e_len, uint8_t* out_status, uint32_t flags) try {
  if (c && (!e || !e_len)) { c->err = "zkp_range_generate_proof_batch: the challenge is an input"; return ZKP_EINVAL; }
  return range_prove_entry(c, "zkp_range_generate_proof_batch", p, w, p ? p->error_factor : 0, 2, e, e_len, nullptr, nullptr, out_status, flags);
} ZKP_CATCH(c)

// The two prover steps of the interactive protocol from a seed: built as zkp_range_ni_prove_seeded_batch is.  Everything is made device-resident
// in a Stage, the sampler expands rows [0, p->error_factor) of the published stream, and the unseeded step runs as the device-pointer call it
// already knows (its routing, split plans, key cache and kernels).  step 1 writes c1 / c2 only; step 2 regenerates the SAME witness from the
// same (seed, first_index) and writes resp_* only.  `s` wipes the witness, the staged seed and the staged x and r on every path out.
static int32_t range_interactive_seeded(zkp_ctx* c, const char* name, int step, const zkp_range_ni_proofs* p, const uint32_t* x, const uint32_t* r,
                                        const uint8_t* seed, uint64_t first_index, const uint8_t* e, const uint8_t* e_len, uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (!range_args_ok(p, RA_RANGE | (step == 1 ? RA_PAIRS : RA_RESP)) || p->error_factor == 0 || !seed || (step == 2 && (!e || !e_len || (p->batch && (!x || !r))))) {
    c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL;
  }
  if (p->batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = p->n_bits / 32, B = p->batch, EF = p->error_factor, rows = B * EF;
  Stage s(c, flags);
  zkp_range_ni_proofs d = *p;
  d.n = s.in(p->n, p->n_stride ? B * kw : kw);
  d.range = s.in(p->range, B * kw);
  d.ciphertext = nullptr;                                // (no prover function reads it)
  d.c1 = d.c2 = nullptr; d.resp_kind = d.resp_j = nullptr; d.resp_w1 = d.resp_r1 = d.resp_w2 = d.resp_r2 = nullptr;
  if (step == 1) { d.c1 = s.out(p->c1, rows * 2 * kw); d.c2 = s.out(p->c2, rows * 2 * kw); }
  else {
    d.resp_kind = s.out(p->resp_kind, rows); d.resp_j = s.out(p->resp_j, rows);
    d.resp_w1 = s.out(p->resp_w1, rows * kw); d.resp_r1 = s.out(p->resp_r1, rows * kw);
    d.resp_w2 = s.out(p->resp_w2, rows * kw); d.resp_r2 = s.out(p->resp_r2, rows * kw);
  }
  const uint32_t* key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(key, 32);
  zkp_range_ni_witness dw{};
  uint32_t* wit[4] = {nullptr, nullptr, nullptr, nullptr};
  for (auto& q : wit) q = s.secret_scratch<uint32_t>(rows * kw);
  dw.w1 = wit[0]; dw.w2 = wit[1]; dw.r1 = wit[2]; dw.r2 = wit[3];
  const uint8_t *de = nullptr, *dl = nullptr;
  if (step == 2) {
    dw.x = s.in(x, B * kw); dw.r = s.in(r, B * kw);
    if (!s.dev) { s.secret(dw.x, B * kw * 4); s.secret(dw.r, B * kw * 4); }
    de = s.in(e, B * 32); dl = s.in(e_len, B);
  }
  uint8_t* ds = s.out(out_status, B);
  int32_t st = s.st;
  if (!st) st = ensure(c, c->scratch[S_SAMPLE_STATUS], B);
  uint8_t* sampler_status = (uint8_t*)c->scratch[S_SAMPLE_STATUS].p;
  if (!st) st = range_sample_launch(c, d, (uint32_t)EF, key, first_index, wit[0], wit[1], wit[2], wit[3], sampler_status);
  if (!st) st = step == 1 ? zkp_range_generate_encrypted_pairs_batch(c, &d, &dw, ZKP_F_DEVICE_PTRS)
                          : zkp_range_generate_proof_batch(c, &d, &dw, de, dl, ds, ZKP_F_DEVICE_PTRS);
  if (!st) st = seeded_status(c, ds, sampler_status, B, step == 2);      // (step 1 has no status of its own: the sampler's alone)
  return s.finish(st);
}
extern "C" int32_t zkp_range_generate_encrypted_pairs_seeded_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const uint8_t* seed, uint64_t first_index,
                                                                   uint8_t* out_status, uint32_t flags) try {
  return range_interactive_seeded(c, "zkp_range_generate_encrypted_pairs_seeded_batch", 1, p, nullptr, nullptr, seed, first_index, nullptr, nullptr, out_status, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_range_generate_proof_seeded_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const uint32_t* x, const uint32_t* r, const uint8_t* seed,
                                                         uint64_t first_index, const uint8_t* e, const uint8_t* e_len, uint8_t* out_status, uint32_t flags) try {
  return range_interactive_seeded(c, "zkp_range_generate_proof_seeded_batch", 2, p, x, r, seed, first_index, e, e_len, out_status, flags);
} ZKP_CATCH(c)

// utils::compute_digest + the Fiat-Shamir glue as an entry point of its own (SURVEY 8(a) row a3)
extern "C" int32_t zkp_range_challenge_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, uint8_t* out_e, uint8_t* out_e_len, uint32_t flags) try {
  ZKP_ROUTE(c, p ? p->batch * 2 * p->error_factor : 0, p ? 2 * p->n_bits : 0, zkp_range_challenge_batch, p, out_e, out_e_len, flags)
  if (!c) return ZKP_EINVAL;
  if (!range_args_ok(p, RA_PAIRS) || (p->batch && (!out_e || !out_e_len))) { c->err = "zkp_range_challenge_batch: invalid argument"; return ZKP_EINVAL; }
  if (p->batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = p->n_bits / 32, B = p->batch, rows = B * p->error_factor;
  Stage s(c, flags);
  zkp_range_ni_proofs d = *p;
  d.n = s.in(p->n, p->n_stride ? B * kw : kw);
  d.c1 = (uint32_t*)s.in((const uint32_t*)p->c1, rows * 2 * kw); d.c2 = (uint32_t*)s.in((const uint32_t*)p->c2, rows * 2 * kw);
  d.range = nullptr;
  uint8_t* de = s.out(out_e, B * 32);
  uint8_t* dl = s.out(out_e_len, B);
  int32_t st = s.st;
  if (!st) st = ensure(c, c->scratch[S_STATUS], B);
  if (!st) st = range_hash<GA>(c, d, de, dl, (uint8_t*)c->scratch[S_STATUS].p, 0);
  return s.finish(st);
} ZKP_CATCH(c)

// Names a verify's transcript hashes to the Enc launch for the length of it (c->fuse_hash points at a local of range_verify_impl): cleared
// however the scope is left, so that no later call finds it dangling.  fuse_hash_taken outlives a normal exit (the caller and
// zkp_diag_last_fused_hash read it); an exception out of the launch clears it too.
struct FuseHashScope {
  zkp_ctx* c;
  int unwinding;
  FuseHashScope(zkp_ctx* c_, const RangeHashArgs* h) : c(c_), unwinding(std::uncaught_exceptions()) { c->fuse_hash = h; c->fuse_hash_taken = false; }
  ~FuseHashScope() {
    c->fuse_hash = nullptr;
    if (std::uncaught_exceptions() > unwinding) c->fuse_hash_taken = false;
  }
  FuseHashScope(const FuseHashScope&) = delete;
  FuseHashScope& operator=(const FuseHashScope&) = delete;
};

template <int G>
static int32_t range_verify_impl(zkp_ctx* c, const zkp_range_ni_proofs& p, uint8_t* verdict, const uint8_t* e_in = nullptr,
                                 const uint8_t* e_len_in = nullptr) {
  using CL = ConstLayout<G>;
  const uint32_t kw = p.n_bits / 32, EF = p.error_factor;
  const uint64_t nkeys = p.n_stride ? p.batch : 1, rows = p.batch * EF;
  int32_t st;
  if ((st = run_setup<G>(c, p.n, p.n_stride, (int)kw, 1, nkeys, c->consts))) return st;
  if ((st = ensure(c, c->scratch[S_E], p.batch * 32))) return st;
  if ((st = ensure(c, c->scratch[S_ELEN], p.batch))) return st;
  // A call of a few proofs leaves most of the GPU idle, and its transcript hash (one lane per proof, ~10 ms whatever the
  // batch) is a third of its latency: the hash and the row predicates go to a second stream while the Enc checks of the
  // kind-derived work list run here (k_verify_plan / k_verdict_merge, kernels_proofs.hpp).  Large batches keep one stream:
  // there k_enc owns every register file and the hash would only delay the groups it displaces (measured, DESIGN.md §8).
  const uint64_t enc_blocks = (2 * rows + LdsLayout<G>::GROUPS_PER_BLOCK - 1) / LdsLayout<G>::GROUPS_PER_BLOCK;
  const char* two_env = std::getenv("ZKP_TWO_STREAMS");    // A/B switch, read on every call: 1 = the two-stream shape for every batch size, 0 = never
  const bool two = rows != 0 && !e_in && two_streams(c->route, enc_blocks, two_env ? (two_env[0] == '1' ? 1 : 0) : -1);
  // One proof on the latency engine (k_enc_basen_r2l5: a workgroup of five wavefronts per Enc, one per compute unit): the hash wavefront travels
  // WITH the Enc launch, as a workgroup of it — a unit to itself — instead of beside it on the second stream, where it shared a SIMD with two
  // role wavefronts one call in four (verify 6.2 or 8.0 ms: profiles/r06/one_proof/).  The row predicates and the merge follow on this stream.
  // The same for 2 - 4 proofs (k_enc_basen_r2l, one wavefront per Enc and at most one per SIMD: 10.0 or 12.5 ms).
  const bool fuse = two && c->route.fuse_hash_on && p.batch < (uint64_t)c->route.cus && basen_r2l_takes_hashes<G>(c, p.n_stride, p.n_bits, 2 * rows, p.batch);
  hipStream_t hs = c->stream;
  uint8_t* enc_verdict = verdict;
  if (two) {
    if ((st = ensure(c, c->scratch[S_ENCV], p.batch))) return st;
    enc_verdict = (uint8_t*)c->scratch[S_ENCV].p;
    HIPCHK(c, hipMemsetAsync(enc_verdict, ZKP_VERDICT_ACCEPT, p.batch, c->stream));
  }
  if (two && !fuse) {
    if ((st = side_stream(c))) return st;
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));          // inputs staged, constants set up
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    c->side_busy = true;                                       // until the join below is enqueued (Stage waits on an early return)
    hs = c->side;
  }
  RangeHashArgs fused_hash{};
  if ((st = range_hash<G>(c, p, (uint8_t*)c->scratch[S_E].p, (uint8_t*)c->scratch[S_ELEN].p, verdict, ZKP_VERDICT_ACCEPT, e_in, e_len_in, hs, fuse ? &fused_hash : nullptr))) return st;
  if (rows == 0) return ZKP_OK;   // error_factor 0: all() over nothing accepts (range_proof.rs:350)
  if ((st = ensure(c, c->scratch[S_IPROOF], 2 * rows * 4))) return st;
  if ((st = ensure(c, c->scratch[S_IROW], 2 * rows * 4))) return st;
  if ((st = ensure(c, c->scratch[S_COUNTER], 16))) return st;
  HIPCHK(c, hipMemsetAsync(c->scratch[S_COUNTER].p, 0, 16, c->stream));
  VerifyPlanArgs v{(const uint8_t*)c->scratch[S_E].p, p.resp_kind, p.resp_w1, p.resp_w2, (const uint32_t*)c->scratch[S_T1].p,
                   (const uint32_t*)c->scratch[S_T2].p, kw, EF, p.batch, verdict, (uint32_t*)c->scratch[S_IPROOF].p,
                   (uint32_t*)c->scratch[S_IROW].p, (unsigned long long*)c->scratch[S_COUNTER].p};
  const dim3 plan_grid((unsigned)((rows + 255) / 256));
  VerifyPlanArgs pred = v; pred.item_proof = nullptr; pred.item_row = nullptr; pred.counter = nullptr;
  if (two) {
    if (!fuse) {
      hipLaunchKernelGGL(k_verify_plan, plan_grid, dim3(256), 0, c->side, pred);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->ev_join, c->side));
    }
    VerifyPlanArgs list = v; list.e = nullptr; list.verdict = nullptr;
    hipLaunchKernelGGL(k_verify_plan, plan_grid, dim3(256), 0, c->stream, list);
  } else {
    hipLaunchKernelGGL(k_verify_plan, plan_grid, dim3(256), 0, c->stream, v);
  }
  HIPCHK(c, hipGetLastError());
  unsigned blocks = 0;
  if ((st = table_for<G>(c, k_enc<G, true>, 2 * rows, &blocks))) return st;
  EncArgs a{};
  a.n = p.n; a.n_stride = p.n_stride; a.consts = (const uint32_t*)c->consts.p; a.const_stride = p.n_stride ? (uint64_t)CL::WORDS : 0;
  a.table = (uint32_t*)c->table.p; a.count = 2 * rows /* upper bound; the kernel reads count_ptr */; a.n_bits = (int)p.n_bits; a.mode = 1;
  a.item_proof = (const uint32_t*)c->scratch[S_IPROOF].p; a.item_row = (const uint32_t*)c->scratch[S_IROW].p;
  a.resp_w1 = p.resp_w1; a.resp_r1 = p.resp_r1; a.resp_w2 = p.resp_w2; a.resp_r2 = p.resp_r2; a.resp_kind = p.resp_kind; a.resp_j = p.resp_j;
  a.c1 = p.c1; a.c2 = p.c2; a.cipher_x = p.ciphertext; a.verdict = enc_verdict;
  a.count_ptr = (const unsigned long long*)c->scratch[S_COUNTER].p; a.ef = EF;
  if (p.n_stride == 0 && !pair_ladder(c->route, G, a.count) && (st = build_schedule(c, p.n, p.n_bits, &a.sched))) return st;
  if ((st = fresh_work_counter(c, &a.work_counter))) return st;
  {
    TimedRegion tr(c, 0);
    FuseHashScope fh(c, fuse ? &fused_hash : nullptr);
    launch_k_enc<G>(c, blocks, a);
  }
  HIPCHK(c, hipGetLastError());
  if (fuse) {
    if (!c->fuse_hash_taken) {      // (the launch went another way after all: the hashes in a launch of their own, behind it)
      hipLaunchKernelGGL(k_range_hash_wave, dim3((unsigned)p.batch), dim3(64), hw_lds_words((int)kw) * sizeof(uint32_t), c->stream, fused_hash);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_verify_plan, plan_grid, dim3(256), 0, c->stream, pred);
    HIPCHK(c, hipGetLastError());
  }
  if (two) {
    if (!fuse) {
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
      c->side_busy = false;
    }
    VerdictMergeArgs m{verdict, enc_verdict, (const uint8_t*)c->scratch[S_E].p, p.resp_kind, EF, p.batch};
    hipLaunchKernelGGL(k_verdict_merge, dim3((unsigned)((p.batch + 255) / 256)), dim3(256), 0, c->stream, m);
    HIPCHK(c, hipGetLastError());
  }
  if (c->timing && c->pinned_counts && c->pinned_used < zkp_ctx::PINNED_SLOTS)
    HIPCHK(c, hipMemcpyAsync(&c->pinned_counts[c->pinned_used++], c->scratch[S_COUNTER].p, 8, hipMemcpyDeviceToHost, c->stream));
  return ZKP_OK;
}

static int32_t range_verify_entry(zkp_ctx* c, const zkp_range_ni_proofs* p, const uint8_t* e_in, const uint8_t* e_len_in, uint8_t* out_verdict, uint32_t flags);
extern "C" int32_t zkp_range_ni_verify_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, uint8_t* out_verdict, uint32_t flags) try {
  ZKP_RANGE_SPLIT_RESET(c)
#ifndef ZKP_SECONDARY_ENGINE
  if (const RangeSplit sp = (p && out_verdict && range_args_ok(p)) ? range_split_plan(c, p, 2 * (uint64_t)p->error_factor, true) : RangeSplit(); sp.head && range_split_ready(c)) {
    const uint64_t head = sp.head, tail = p->batch - head;
    auto part = [&](const LatEngine* e, zkp_ctx* ec, uint64_t lo, uint64_t count) {
      const zkp_range_ni_proofs q = range_slice(*p, p->error_factor, lo, count);
      return e->p_zkp_range_ni_verify_batch(ec, &q, out_verdict + lo, flags);
    };
    return range_split_run(c, sp.head_engine, tail, [&](const LatEngine* e, zkp_ctx* ec) { return part(e, ec, 0, head); }, [&](const LatEngine* e, zkp_ctx* ec) { return part(e, ec, head, tail); });
  }
#endif
  ZKP_ROUTE_VERIFY(c, p ? p->batch * 2 * p->error_factor : 0, p ? 2 * p->n_bits : 0, p && p->n_stride == 0, zkp_range_ni_verify_batch, p, out_verdict, flags)
  return range_verify_entry(c, p, nullptr, nullptr, out_verdict, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_range_verifier_output_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, const uint8_t* e, const uint8_t* e_len, uint8_t* out_verdict,
                                                   uint32_t flags) try {
  ZKP_ROUTE_ENC(c, p ? p->batch * 2 * p->error_factor : 0, p ? 2 * p->n_bits : 0, p && p->n_stride == 0, zkp_range_verifier_output_batch, p, e, e_len, out_verdict, flags)
  if (c && (!e || !e_len)) { c->err = "zkp_range_verifier_output_batch: the challenge is an input"; return ZKP_EINVAL; }
  return range_verify_entry(c, p, e, e_len, out_verdict, flags);
} ZKP_CATCH(c)
static int32_t range_verify_entry(zkp_ctx* c, const zkp_range_ni_proofs* p, const uint8_t* e_in, const uint8_t* e_len_in, uint8_t* out_verdict, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (!range_args_ok(p) || (p->batch && !out_verdict)) { c->err = "zkp_range_ni_verify_batch: invalid argument"; return ZKP_EINVAL; }
  if (p->batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = p->n_bits / 32, B = p->batch, rows = B * p->error_factor;
  Stage s(c, flags);
  const std::vector<size_t> blocks = s.dev ? std::vector<size_t>() : host_blocks(c, B, p->error_factor, true);
  c->last_host_blocks = blocks.empty() ? 1 : (int)blocks.size() - 1;
  if (!blocks.empty()) {
    // host arrays, a large batch: a pipeline of proof blocks — block k + 1 is copied in while the kernels of block k run (Piped, zkp_api.hip)
    const size_t EF = p->error_factor;
    Piped pp(c, s);
    zkp_range_ni_proofs d = *p;
    d.n = p->n_stride ? pp.in(p->n, kw, B) : s.in(p->n, kw);
    d.range = pp.in(p->range, kw, B);
    d.ciphertext = pp.in(p->ciphertext, 2 * kw, B);
    d.c1 = (uint32_t*)pp.in((const uint32_t*)p->c1, EF * 2 * kw, B); d.c2 = (uint32_t*)pp.in((const uint32_t*)p->c2, EF * 2 * kw, B);
    d.resp_kind = (uint8_t*)pp.in((const uint8_t*)p->resp_kind, EF, B); d.resp_j = (uint8_t*)pp.in((const uint8_t*)p->resp_j, EF, B);
    d.resp_w1 = (uint32_t*)pp.in((const uint32_t*)p->resp_w1, EF * kw, B); d.resp_r1 = (uint32_t*)pp.in((const uint32_t*)p->resp_r1, EF * kw, B);
    d.resp_w2 = (uint32_t*)pp.in((const uint32_t*)p->resp_w2, EF * kw, B); d.resp_r2 = (uint32_t*)pp.in((const uint32_t*)p->resp_r2, EF * kw, B);
    uint8_t* dv = pp.out(out_verdict, 1, B);
    const uint8_t* dei = pp.in(e_in, 32, B);
    const uint8_t* deli = pp.in(e_len_in, 1, B);
    int32_t st = s.st;
    const size_t nb = blocks.size() - 1;
    if (!st) st = pp.streams(nb);
    if (!st) st = pp.h2d(blocks[0], blocks[1], c->ev_pipe[0]);
    for (size_t k = 0; k < nb && !st; k++) {
      const size_t lo = blocks[k], hi = blocks[k + 1];
      const zkp_range_ni_proofs q = range_slice(d, EF, lo, hi - lo);
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_pipe[2 * k], 0));
      st = with_group<GA, GB, GC>(group_for_bits(2 * p->n_bits), [&](auto G) { return range_verify_impl<G()>(c, q, dv + lo, dei ? dei + lo * 32 : nullptr, deli ? deli + lo : nullptr); });
      if (st) break;
      HIPCHK(c, hipEventRecord(c->ev_pipe[2 * k + 1], c->stream));
      if (k + 1 < nb) st = pp.h2d(blocks[k + 1], blocks[k + 2], c->ev_pipe[2 * k + 2]);     // (under the kernels of block k)
    }
    for (size_t k = 0; k < nb && !st; k++) st = pp.d2h(blocks[k], blocks[k + 1], c->ev_pipe[2 * k + 1]);
    const int32_t fc = pp.finish();
    return s.finish(st ? st : fc);
  }
  zkp_range_ni_proofs d = *p;
  d.n = s.in(p->n, p->n_stride ? B * kw : kw);
  d.range = s.in(p->range, B * kw);
  d.ciphertext = s.in(p->ciphertext, B * 2 * kw);
  d.c1 = (uint32_t*)s.in((const uint32_t*)p->c1, rows * 2 * kw); d.c2 = (uint32_t*)s.in((const uint32_t*)p->c2, rows * 2 * kw);
  d.resp_kind = (uint8_t*)s.in((const uint8_t*)p->resp_kind, rows); d.resp_j = (uint8_t*)s.in((const uint8_t*)p->resp_j, rows);
  d.resp_w1 = (uint32_t*)s.in((const uint32_t*)p->resp_w1, rows * kw); d.resp_r1 = (uint32_t*)s.in((const uint32_t*)p->resp_r1, rows * kw);
  d.resp_w2 = (uint32_t*)s.in((const uint32_t*)p->resp_w2, rows * kw); d.resp_r2 = (uint32_t*)s.in((const uint32_t*)p->resp_r2, rows * kw);
  uint8_t* dv = s.out(out_verdict, B);
  const uint8_t* dei = s.in(e_in, B * 32);
  const uint8_t* deli = s.in(e_len_in, B);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * p->n_bits), [&](auto G) { return range_verify_impl<G()>(c, d, dv, dei, deli); });
  return s.finish(st);
}

// ---- NiCorrectKeyProof ------------------------------------------------------------------------
static int32_t upload_primes(zkp_ctx* c, uint32_t* count) {
  std::vector<uint32_t> pr;
  for (uint32_t v = 2; v < 6370; v++) {   // alpha = 6370, correct_key_ni.rs:24-26
    bool prime = true;
    for (uint32_t d = 2; d * d <= v; d++) if (v % d == 0) { prime = false; break; }
    if (prime) pr.push_back(v);
  }
  *count = (uint32_t)pr.size();
  if (c->scratch[S_PRIMES].p) return ZKP_OK;
  int32_t st = ensure(c, c->scratch[S_PRIMES], pr.size() * 4);
  if (st) return st;
  HIPCHK(c, hipMemcpy(c->scratch[S_PRIMES].p, pr.data(), pr.size() * 4, hipMemcpyHostToDevice));
  return ZKP_OK;
}

template <int G>
static int32_t ck_verify_impl(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, const uint32_t* sigma, const uint8_t* salt,
                              uint32_t salt_len, uint8_t* verdict) {
  using LL = LdsLayout<G>;
  const uint32_t kw = n_bits / 32;
  int32_t st;
  uint32_t nprimes = 0;
  if ((st = upload_primes(c, &nprimes))) return st;
  if ((st = run_setup<G>(c, n, kw, (int)kw, 0, batch, c->consts))) return st;
  if ((st = ensure(c, c->scratch[S_MGF], batch * ZKP_CORRECT_KEY_M2 * (kw + 8) * 4))) return st;
  CkHashArgs h{n, kw, batch, salt, salt_len, (uint32_t*)c->scratch[S_MGF].p, verdict, (const uint32_t*)c->scratch[S_PRIMES].p, nprimes};
  if (batch <= 4ull * (uint64_t)c->route.cus) hipLaunchKernelGGL(k_ck_hash_wave, dim3((unsigned)batch), dim3(64), 0, c->stream, h);      // a few keys: one wavefront each
  else hipLaunchKernelGGL(k_ck_hash, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, c->stream, h);
  HIPCHK(c, hipGetLastError());
  const uint64_t items = batch * ZKP_CORRECT_KEY_M2;
  unsigned blocks = 0;
  if ((st = table_for<G>(c, k_ck_check<G, false>, items, &blocks))) return st;
  unsigned long long* wc = nullptr;
  if ((st = fresh_work_counter(c, &wc))) return st;
  CkCheckArgs a{n, sigma, (const uint32_t*)c->scratch[S_MGF].p, (const uint32_t*)c->consts.p, (uint32_t*)c->table.p, verdict, items, (int)n_bits, wc};
  {
    TimedRegion tr(c, items);
    bool launched = false;
    if constexpr (PAIR_LADDER_BUILD && 2 * G <= 64) {
      if (pair_ladder(c->route, G, items)) {                     // a few keys on the latency engine: right-to-left ladder on pairs of groups
        const unsigned pair_blocks = (unsigned)std::max<uint64_t>(1, (items + LL::GROUPS_PER_BLOCK / 2 - 1) / (LL::GROUPS_PER_BLOCK / 2));
        hipLaunchKernelGGL((k_ck_check<G, true>), dim3(pair_blocks), dim3(256), LL::BYTES_PER_BLOCK, c->stream, a);
        launched = true;
      }
    }
    if (!launched) hipLaunchKernelGGL((k_ck_check<G, false>), dim3(blocks), dim3(256), LL::BYTES_PER_BLOCK, c->stream, a);
  }
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

extern "C" int32_t zkp_correct_key_ni_verify_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, const uint32_t* sigma,
                                                   const uint8_t* salt, uint32_t salt_len, uint8_t* out_verdict, uint32_t flags) try {
  ZKP_ROUTE(c, batch * ZKP_CORRECT_KEY_M2, n_bits, zkp_correct_key_ni_verify_batch, n_bits, batch, n, sigma, salt, salt_len, out_verdict, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!n || !sigma || !out_verdict || (salt_len && !salt) || !key_bits_ok(n_bits) || batch > (1ull << 26)) { c->err = "zkp_correct_key_ni_verify_batch: invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, batch * kw);
  const uint32_t* dsg = s.in(sigma, batch * ZKP_CORRECT_KEY_M2 * kw);
  uint8_t* dv = s.out(out_verdict, batch);
  // the salt is a short host byte string in both memory modes
  const uint8_t* dsalt = salt_len ? s.host_in(salt, salt_len) : nullptr;
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB>(group_for_bits(n_bits), [&](auto G) { return ck_verify_impl<G()>(c, n_bits, batch, dn, dsg, dsalt, salt_len, dv); });
  if (!st && (flags & ZKP_F_DEVICE_PTRS)) { if (hipStreamSynchronize(c->stream) != hipSuccess) { st = ZKP_EDEVICE; c->err = "sync"; } }   // salt staging is freed below
  return s.finish(st);
} ZKP_CATCH(c)

// ---- CompositeDLogProof ------------------------------------------------------------------------
static bool dlog_args_ok(uint32_t n_bits, uint32_t y_bits, uint64_t batch) {
  return key_bits_ok(n_bits) && y_bits >= 544 && y_bits % 32 == 0 && y_bits <= n_bits && batch <= (1ull << 24);
}

template <int G>
static int32_t dlog_prove_impl(zkp_ctx* c, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* N, const uint32_t* g, const uint32_t* ni,
                               const uint32_t* secret, const uint32_t* r, uint32_t* x, uint32_t* y) {
  const uint32_t kw = n_bits / 32;
  Compose<G> m(c, batch, true, kw);
  m.M.setup(N, kw, 0);
  m.M.pow(512, g, r, 16, x, (int)kw);                                 // x = g^r mod N, r < 2^512 (wi_dlog_proof.rs:53-55)
  uint32_t* e = m.buf(S_DLOG_E, batch * 8);
  if (m.st) return m.st;
  DlogHashArgs h{N, g, ni, x, kw, batch, e, nullptr, secret, r, y, y_bits / 32, 3};
  hipLaunchKernelGGL(k_dlog_hash, dim3((unsigned)((batch + DLOG_THREADS - 1) / DLOG_THREADS)), dim3(DLOG_THREADS), 16 * DLOG_THREADS * 4, c->stream, h);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

extern "C" int32_t zkp_dlog_prove_batch(zkp_ctx* c, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* N, const uint32_t* g,
                                        const uint32_t* ni, const uint32_t* secret, const uint32_t* r, uint32_t* out_x, uint32_t* out_y, uint32_t flags) try {
  ZKP_ROUTE(c, batch, n_bits, zkp_dlog_prove_batch, n_bits, y_bits, batch, N, g, ni, secret, r, out_x, out_y, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!dlog_args_ok(n_bits, y_bits, batch) || !N || !g || !ni || !secret || !r || !out_x || !out_y) { c->err = "zkp_dlog_prove_batch: invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t *dN = s.in(N, batch * kw), *dg = s.in(g, batch * kw), *dni = s.in(ni, batch * kw), *dsec = s.in(secret, batch * 8), *dr = s.in(r, batch * 16);
  uint32_t* dx = s.out(out_x, batch * kw);
  uint32_t* dy = s.out(out_y, batch * (y_bits / 32));
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB>(group_for_bits(n_bits), [&](auto G) { return dlog_prove_impl<G()>(c, n_bits, y_bits, batch, dN, dg, dni, dsec, dr, dx, dy); });
  return s.finish(st);
} ZKP_CATCH(c)

template <int G>
static int32_t dlog_verify_impl(zkp_ctx* c, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* N, const uint32_t* g, const uint32_t* ni,
                                const uint32_t* x, const uint32_t* y, uint8_t* verdict) {
  using CL = ConstLayout<G>;
  const uint32_t kw = n_bits / 32;
  Compose<G> m(c, batch, true, kw);
  m.M.setup(N, kw, 0);
  uint32_t* e = m.buf(S_DLOG_E, batch * 8);
  uint32_t *t1 = m.buf(S_TMP1, batch * kw), *t2 = m.buf(S_TMP2, batch * kw), *t3 = m.buf(S_TMP3, batch * kw);
  if (m.st) return m.st;
  HIPCHK(c, hipMemsetAsync(c->scratch[S_TMP3].p, 0, batch * kw * 4, c->stream));
  // A call that leaves room on the GPU runs the verifier's pre-checks (N > 2^128 and the two GCDs: ~1 ms on one lane per
  // proof, needed only by the final compare) on the second stream, next to the exponentiations; the challenge stays here.
  const bool two = batch <= 16ull * (uint64_t)c->route.cus;      // (64 wavefronts of pre-checks at most)
  DlogHashArgs h{N, g, ni, x, kw, batch, e, verdict, nullptr, nullptr, nullptr, 0, two ? 1u : 3u};
  const dim3 hash_grid((unsigned)((batch + DLOG_THREADS - 1) / DLOG_THREADS));
  const size_t hash_lds = (16 + 2 * kw) * DLOG_THREADS * 4;
  if (two) {
    int32_t st;
    if ((st = side_stream(c))) return st;
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));            // inputs staged
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    c->side_busy = true;
    DlogHashArgs pre = h; pre.parts = 2;
    hipLaunchKernelGGL(k_dlog_hash, hash_grid, dim3(DLOG_THREADS), hash_lds, c->side, pre);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_join, c->side));
  }
  hipLaunchKernelGGL(k_dlog_hash, hash_grid, dim3(DLOG_THREADS), hash_lds, c->stream, h);
  HIPCHK(c, hipGetLastError());
  m.M.pow_multi({{256, ni, e, 8, t1, (int)kw, 0}, {y_bits, g, y, y_bits / 32, t2, (int)kw, 0}});      // ni^e (:81) and g^y (:82) side by side in one launch
  m.M.mul(t1, 0, t2, 0, t3, (int)kw);                                                                 // mod_mul :83
  if (m.st) return m.st;
  if (two) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0)); c->side_busy = false; }
  m.rows(k_dlog_compare, batch, DlogCmpArgs{x, t3, m.M.cst(), (uint64_t)CL::WORDS, CL::OFF_ST, kw, batch, verdict});
  return m.st;
}

extern "C" int32_t zkp_dlog_verify_batch(zkp_ctx* c, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* N, const uint32_t* g,
                                         const uint32_t* ni, const uint32_t* x, const uint32_t* y, uint8_t* out_verdict, uint32_t flags) try {
  ZKP_ROUTE(c, 2 * batch, n_bits, zkp_dlog_verify_batch, n_bits, y_bits, batch, N, g, ni, x, y, out_verdict, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!dlog_args_ok(n_bits, y_bits, batch) || !N || !g || !ni || !x || !y || !out_verdict) { c->err = "zkp_dlog_verify_batch: invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t *dN = s.in(N, batch * kw), *dg = s.in(g, batch * kw), *dni = s.in(ni, batch * kw), *dx = s.in(x, batch * kw), *dy = s.in(y, batch * (y_bits / 32));
  uint8_t* dv = s.out(out_verdict, batch);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB>(group_for_bits(n_bits), [&](auto G) { return dlog_verify_impl<G()>(c, n_bits, y_bits, batch, dN, dg, dni, dx, dy, dv); });
  return s.finish(st);
} ZKP_CATCH(c)

// ---- ZeroProof / CiphertextProof (SURVEY §8(f) rank 1): compositions of the same kernels ---------------
static bool sigma_args_ok(uint32_t n_bits, uint64_t batch, uint64_t n_stride) {
  return key_bits_ok(n_bits) && batch <= (1ull << 24) && (n_stride == 0 || n_stride == n_bits / 32);
}

// commit: out_commit = Enc(m', r');  e = H(n, c, commit);  [z1 = x' + x e];  z = r' * r^e mod n^2
template <int G>
static int32_t sigma_prove_impl(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                const uint32_t* x, const uint32_t* r, const uint32_t* x_prime, const uint32_t* r_prime, uint32_t* out_z1,
                                uint32_t* out_z, uint32_t* out_commit) {
  const uint32_t kw = n_bits / 32;
  const int w1 = (int)kw, w2 = (int)(2 * kw);
  Compose<G> m(c, batch, n_stride != 0, kw);
  m.M.setup(n, n_stride, 1);
  m.enc(n, n_stride, x_prime, x_prime ? 0 : -1, r_prime, 0, out_commit);
  uint32_t *e = m.buf(S_E, batch * 8), *t1 = m.buf(S_TMP1, batch * 2 * kw);
  m.rows(k_sigma_hash, batch, SigmaHashArgs{n, n_stride, cc, out_commit, kw, batch, e, x, x_prime, out_z1, kw + ZKP_Z1_EXTRA_LIMBS});
  m.M.pow(256, r, e, 8, t1, w1, w2);               // r^e mod nn
  m.M.mul(r_prime, w1, t1, w2, out_z, w2);
  return m.st;
}

// Enc(z1, z) == c^e * commit mod n^2
template <int G>
static int32_t sigma_verify_impl(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                 const uint32_t* z1, const uint32_t* z, const uint32_t* commit, uint8_t* verdict) {
  const uint32_t kw = n_bits / 32;
  const int w2 = (int)(2 * kw);
  Compose<G> m(c, batch, n_stride != 0, kw);
  m.M.setup(n, n_stride, 1);
  uint32_t* e = m.buf(S_E, batch * 8);
  uint32_t *t1 = m.buf(S_TMP1, batch * 2 * kw), *t2 = m.buf(S_TMP2, batch * 2 * kw), *t3 = m.buf(S_TMP3, batch * 2 * kw);
  if (m.st) return m.st;
  HIPCHK(c, hipMemsetAsync(t3, 0, batch * 2 * kw * 4, c->stream));
  m.rows(k_sigma_hash, batch, SigmaHashArgs{n, n_stride, cc, commit, kw, batch, e, nullptr, nullptr, nullptr, 0});
  m.enc(n, n_stride, z1, z1 ? (int)(kw + ZKP_Z1_EXTRA_LIMBS) : -1, z, w2, t1);      // c_z
  m.M.pow(256, cc, e, 8, t2, w2);                                                   // c^e  (Paillier::mul)
  m.M.mul(t2, 0, commit, 0, t3, w2);                                                // Paillier::add
  m.compare(t1, t3, 2 * kw, verdict);
  return m.st;
}

static int32_t sigma_prove_entry(zkp_ctx* c, const char* name, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                 const uint32_t* x, const uint32_t* r, const uint32_t* x_prime, const uint32_t* r_prime, uint32_t* out_z1, uint32_t* out_z,
                                 uint32_t* out_commit, bool with_x, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !cc || !r || !r_prime || !out_z || !out_commit || (with_x && (!x || !x_prime || !out_z1))) {
    c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t* dc = s.in(cc, batch * 2 * kw);
  const uint32_t* dr = s.in(r, batch * kw);
  const uint32_t* drp = s.in(r_prime, batch * kw);
  const uint32_t* dx = with_x ? s.in(x, batch * kw) : nullptr;
  const uint32_t* dxp = with_x ? s.in(x_prime, batch * kw) : nullptr;
  uint32_t* dz1 = with_x ? s.out(out_z1, batch * (kw + ZKP_Z1_EXTRA_LIMBS)) : nullptr;
  uint32_t* dz = s.out(out_z, batch * 2 * kw);
  uint32_t* dcm = s.out(out_commit, batch * 2 * kw);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return sigma_prove_impl<G()>(c, n_bits, batch, dn, n_stride, dc, dx, dr, dxp, drp, dz1, dz, dcm); });
  return s.finish(st);
}

static int32_t sigma_verify_entry(zkp_ctx* c, const char* name, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                  const uint32_t* z1, const uint32_t* z, const uint32_t* commit, uint8_t* verdict, bool with_z1, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !cc || !z || !commit || !verdict || (with_z1 && !z1)) { c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t* dc = s.in(cc, batch * 2 * kw);
  const uint32_t* dz1 = with_z1 ? s.in(z1, batch * (kw + ZKP_Z1_EXTRA_LIMBS)) : nullptr;
  const uint32_t* dz = s.in(z, batch * 2 * kw);
  const uint32_t* dcm = s.in(commit, batch * 2 * kw);
  uint8_t* dv = s.out(verdict, batch);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return sigma_verify_impl<G()>(c, n_bits, batch, dn, n_stride, dc, dz1, dz, dcm, dv); });
  return s.finish(st);
}

extern "C" int32_t zkp_zero_proof_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                              const uint32_t* r, const uint32_t* r_prime, uint32_t* out_z, uint32_t* out_a, uint32_t flags) try {
  ZKP_ROUTE(c, 2 * batch, 2 * n_bits, zkp_zero_proof_prove_batch, n_bits, batch, n, n_stride, cc, r, r_prime, out_z, out_a, flags)
  return sigma_prove_entry(c, "zkp_zero_proof_prove_batch", n_bits, batch, n, n_stride, cc, nullptr, r, nullptr, r_prime, nullptr, out_z, out_a, false, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_zero_proof_verify_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                               const uint32_t* z, const uint32_t* a, uint8_t* out_verdict, uint32_t flags) try {
  ZKP_ROUTE(c, 2 * batch, 2 * n_bits, zkp_zero_proof_verify_batch, n_bits, batch, n, n_stride, cc, z, a, out_verdict, flags)
  return sigma_verify_entry(c, "zkp_zero_proof_verify_batch", n_bits, batch, n, n_stride, cc, nullptr, z, a, out_verdict, false, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_ciphertext_proof_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                                    const uint32_t* x, const uint32_t* r, const uint32_t* x_prime, const uint32_t* r_prime,
                                                    uint32_t* out_z1, uint32_t* out_z2, uint32_t* out_c_prime, uint32_t flags) try {
  ZKP_ROUTE(c, 2 * batch, 2 * n_bits, zkp_ciphertext_proof_prove_batch, n_bits, batch, n, n_stride, cc, x, r, x_prime, r_prime, out_z1, out_z2, out_c_prime, flags)
  return sigma_prove_entry(c, "zkp_ciphertext_proof_prove_batch", n_bits, batch, n, n_stride, cc, x, r, x_prime, r_prime, out_z1, out_z2, out_c_prime, true, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_ciphertext_proof_verify_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                                     const uint32_t* z1, const uint32_t* z2, const uint32_t* c_prime, uint8_t* out_verdict, uint32_t flags) try {
  ZKP_ROUTE(c, 2 * batch, 2 * n_bits, zkp_ciphertext_proof_verify_batch, n_bits, batch, n, n_stride, cc, z1, z2, c_prime, out_verdict, flags)
  return sigma_verify_entry(c, "zkp_ciphertext_proof_verify_batch", n_bits, batch, n, n_stride, cc, z1, z2, c_prime, out_verdict, true, flags);
} ZKP_CATCH(c)

// ---- VerlinProof (verlin_proof.rs:35-165): the same kernels once more ------------------------------------
// out = c^y * c'^y' * Enc(y'', r_y) mod n^2   (gen_phi, verlin_proof.rs:138-165).  Uses scratch T1..T3.
template <int G>
static void verlin_gen_phi(Compose<G>& m, const uint32_t* n, uint64_t n_stride, const uint32_t* cc, const uint32_t* ccp, const uint32_t* y, const uint32_t* yp,
                           const uint32_t* ypp, int y_words, const uint32_t* ry, int ry_words, uint32_t* out) {
  const int w2 = (int)(2 * m.kw);
  uint32_t *t1 = m.buf(S_TMP1, m.batch * w2), *t2 = m.buf(S_TMP2, m.batch * w2), *t3 = m.buf(S_TMP3, m.batch * w2);
  // Paillier::mul(c, y) and Paillier::mul(c', y'): one launch
  m.M.pow_multi({{(uint32_t)y_words * 32, cc, y, (uint64_t)y_words, t1, w2, 0}, {(uint32_t)y_words * 32, ccp, yp, (uint64_t)y_words, t2, w2, 0}});
  m.enc(n, n_stride, ypp, y_words, ry, ry_words, t3);      // Enc(y'', r_y)
  m.M.mul(t1, 0, t2, 0, t1, w2);                           // Paillier::add
  m.M.mul(t1, 0, t3, 0, out, w2);
}

template <int G>
static int32_t verlin_impl(zkp_ctx* c, bool prove, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc, const uint32_t* ccp,
                           const uint32_t* phi_x, const uint32_t* const x[3], const uint32_t* r_x, const uint32_t* const a[3], const uint32_t* r_a,
                           uint32_t* phi_a, uint32_t* const z[3], uint32_t* r_z, uint8_t* verdict) {
  const uint32_t kw = n_bits / 32, zw = kw + ZKP_Z1_EXTRA_LIMBS;
  const int w1 = (int)kw, w2 = (int)(2 * kw);
  Compose<G> m(c, batch, n_stride != 0, kw);
  m.M.setup(n, n_stride, 1);
  uint32_t* e = m.buf(S_E, batch * 8);
  for (int k : {S_TMP1, S_TMP2, S_TMP3}) (void)m.buf(k, batch * 2 * kw);
  uint32_t *t4 = m.buf(S_TMP4, batch * 2 * kw), *t5 = m.buf(S_TMP5, batch * 2 * kw);
  if (prove) {
    verlin_gen_phi(m, n, n_stride, cc, ccp, a[0], a[1], a[2], w1, r_a, w1, phi_a);
    m.rows(k_verlin_hash, batch, VerlinHashArgs{n, n_stride, {cc, ccp, phi_x, phi_a}, kw, batch, e, {x[0], x[1], x[2]}, {a[0], a[1], a[2]}, {z[0], z[1], z[2]}, zw});
    m.M.pow(256, r_x, e, 8, t4, w1, w2);                   // r_x^e mod nn (:88)
    m.M.mul(t4, w2, r_a, w1, r_z, w2);
    return m.st;
  }
  m.rows(k_verlin_hash, batch, VerlinHashArgs{n, n_stride, {cc, ccp, phi_x, phi_a}, kw, batch, e, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, 0});
  verlin_gen_phi(m, n, n_stride, cc, ccp, z[0], z[1], z[2], (int)zw, r_z, w2, t4);      // phi_z
  m.M.pow(256, phi_x, e, 8, t5, w2);                                                    // phi_x^e
  m.M.mul(t5, 0, phi_a, 0, t5, w2);                                                     // * phi_a
  m.compare(t4, t5, 2 * kw, verdict);
  return m.st;
}

extern "C" int32_t zkp_verlin_proof_prove_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                                const uint32_t* c_prime, const uint32_t* phi_x, const uint32_t* x, const uint32_t* x_prime,
                                                const uint32_t* x_double_prime, const uint32_t* r_x, const uint32_t* a, const uint32_t* a_prime,
                                                const uint32_t* a_double_prime, const uint32_t* r_a, uint32_t* out_phi_a, uint32_t* out_z,
                                                uint32_t* out_z_prime, uint32_t* out_z_double_prime, uint32_t* out_r_z, uint32_t flags) try {
  ZKP_ROUTE(c, 4 * batch, 2 * n_bits, zkp_verlin_proof_prove_batch, n_bits, batch, n, n_stride, cc, c_prime, phi_x, x, x_prime, x_double_prime, r_x, a, a_prime, a_double_prime, r_a, out_phi_a, out_z, out_z_prime, out_z_double_prime, out_r_z, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !cc || !c_prime || !phi_x || !x || !x_prime || !x_double_prime || !r_x || !a || !a_prime ||
      !a_double_prime || !r_a || !out_phi_a || !out_z || !out_z_prime || !out_z_double_prime || !out_r_z) { c->err = "zkp_verlin_proof_prove_batch: invalid argument"; return ZKP_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32, zw = kw + ZKP_Z1_EXTRA_LIMBS;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dc = s.in(cc, batch * 2 * kw), *dcp = s.in(c_prime, batch * 2 * kw), *dphx = s.in(phi_x, batch * 2 * kw);
  const uint32_t* dx[3] = {s.in(x, batch * kw), s.in(x_prime, batch * kw), s.in(x_double_prime, batch * kw)};
  const uint32_t* da[3] = {s.in(a, batch * kw), s.in(a_prime, batch * kw), s.in(a_double_prime, batch * kw)};
  const uint32_t *drx = s.in(r_x, batch * kw), *dra = s.in(r_a, batch * kw);
  uint32_t* dpa = s.out(out_phi_a, batch * 2 * kw);
  uint32_t* dz[3] = {s.out(out_z, batch * zw), s.out(out_z_prime, batch * zw), s.out(out_z_double_prime, batch * zw)};
  uint32_t* drz = s.out(out_r_z, batch * 2 * kw);
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return verlin_impl<G()>(c, true, n_bits, batch, dn, n_stride, dc, dcp, dphx, dx, drx, da, dra, dpa, dz, drz, nullptr); });
  return s.finish(st);
} ZKP_CATCH(c)

extern "C" int32_t zkp_verlin_proof_verify_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* n, uint64_t n_stride, const uint32_t* cc,
                                                 const uint32_t* c_prime, const uint32_t* phi_x, const uint32_t* phi_a, const uint32_t* z,
                                                 const uint32_t* z_prime, const uint32_t* z_double_prime, const uint32_t* r_z, uint8_t* out_verdict,
                                                 uint32_t flags) try {
  ZKP_ROUTE(c, 4 * batch, 2 * n_bits, zkp_verlin_proof_verify_batch, n_bits, batch, n, n_stride, cc, c_prime, phi_x, phi_a, z, z_prime, z_double_prime, r_z, out_verdict, flags)
  if (!c) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!sigma_args_ok(n_bits, batch, n_stride) || !n || !cc || !c_prime || !phi_x || !phi_a || !z || !z_prime || !z_double_prime || !r_z || !out_verdict) {
    c->err = "zkp_verlin_proof_verify_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t kw = n_bits / 32, zw = kw + ZKP_Z1_EXTRA_LIMBS;
  Stage s(c, flags);
  const uint32_t* dn = s.in(n, n_stride ? batch * kw : kw);
  const uint32_t *dc = s.in(cc, batch * 2 * kw), *dcp = s.in(c_prime, batch * 2 * kw), *dphx = s.in(phi_x, batch * 2 * kw), *dpa = s.in(phi_a, batch * 2 * kw);
  uint32_t* dz[3] = {(uint32_t*)s.in(z, batch * zw), (uint32_t*)s.in(z_prime, batch * zw), (uint32_t*)s.in(z_double_prime, batch * zw)};
  const uint32_t* drz = s.in(r_z, batch * 2 * kw);
  uint8_t* dv = s.out(out_verdict, batch);
  const uint32_t* none[3] = {nullptr, nullptr, nullptr};
  int32_t st = s.st;
  if (!st) st = with_group<GA, GB, GC>(group_for_bits(2 * n_bits), [&](auto G) { return verlin_impl<G()>(c, false, n_bits, batch, dn, n_stride, dc, dcp, dphx, none, nullptr, none, nullptr, (uint32_t*)dpa, dz, (uint32_t*)drz, dv); });
  return s.finish(st);
} ZKP_CATCH(c)
