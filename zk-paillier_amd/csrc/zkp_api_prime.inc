// zkp_api_prime.inc — host side of zkp_probable_prime_batch, zkp_next_prime_batch and zkp_paillier_keygen_seeded_batch (kernels_prime.hpp);
// included by zkp_api.hip behind zkp_api_ck_prove.inc.  The three calls are ONE search (prime_search) over slots: a loop of rounds
// "rows -> ladder -> tail -> pick -> window -> compact" for the still-unresolved slots, on the ctx stream, in which the host reads one word
// per round: the number of slots left.  The ladder is a SecretLadder (zkp_api_paillier_dec.inc): its constants records and window tables hold
// the candidates, so they are secret blocks of the call's Stage — taken ONCE per call, sized for the first round, and run every round.  The
// calls run on the engine of the ctx that receives them.

// Rows per slot and round: C = PRIME_TARGET_ROWS / (slots left), at least PRIME_C and at most PRIME_C_MAX.  A ladder launch of a few rows
// takes as long as one of tens of thousands (it is one chain of products per row), so while many slots are left the rows are kept few —
// every row behind a slot's prime is wasted — and as the slots run out each of them looks further ahead.  tools/dev/keygen_ab.py measures
// the choices; no result depends on them.
constexpr int PRIME_C = 4, PRIME_C_MAX = 64;
constexpr uint64_t PRIME_TARGET_ROWS = 32768;
constexpr uint64_t PRIME_SLAB_SLOTS = 8192;                  // slots in flight: 32 768 ladder rows, about 50 MB of the call's blocks

struct PrimeCall {
  int mode; uint32_t bits, rounds; uint64_t nslots, first_index;
  const uint32_t* in;                                        // [nslots][pw] device (test, next)
  const uint32_t* key;                                       // device seed words, or null
  uint8_t* verdict; uint32_t* out_prime; uint32_t* out_offset; uint8_t* out_status;     // test / next (device, nullable)
  uint32_t* out_p; uint32_t* out_q; uint8_t* key_status;     // keygen (device)
};

static int32_t prime_search(zkp_ctx* c, Stage& s, const PrimeCall& q) {
  static_assert(LdsLayout<GA>::NW == PRIME_ROW_WORDS, "the ladder's row at mod_bits = 2048");
  const int pw = (int)(q.bits / 32);
  const uint64_t cmin = q.mode == PRIME_MODE_TEST ? 1 : c->prime_chunk ? c->prime_chunk : PRIME_C;     // the test's window is one candidate
  const uint64_t target = c->prime_target ? c->prime_target : PRIME_TARGET_ROWS;
  c->prime_rows = 0; c->prime_rounds = 0;
  const uint64_t slab = std::min<uint64_t>(q.nslots, PRIME_SLAB_SLOTS);
  // rows of a round: left * clamp(target / left, cmin, PRIME_C_MAX) <= max(left * cmin, target); two rows at least: a one-row launch
  // would tag the borrowed constants as ONE key's record
  const uint64_t max_rows = std::max<uint64_t>(2, std::max(slab * cmin, target));
  PrimeArgs a{};
  a.key = q.key; a.first_index = q.first_index; a.mode = q.mode; a.pw = pw; a.rounds = (int)q.rounds;
  a.start = s.secret_scratch<uint32_t>(slab * pw); a.map = s.secret_scratch<uint32_t>(slab * PRIME_MAP_WORDS);
  for (uint32_t** per_slot : {&a.state, &a.attempt, &a.cand, &a.next_r, &a.found_j}) *per_slot = s.secret_scratch<uint32_t>(slab);
  a.mods = s.secret_scratch<uint32_t>(max_rows * PRIME_ROW_WORDS); a.base = s.secret_scratch<uint32_t>(max_rows * PRIME_ROW_WORDS);
  a.exp = s.secret_scratch<uint32_t>(max_rows * pw);
  uint32_t* lad = s.secret_scratch<uint32_t>(max_rows * PRIME_ROW_WORDS);
  a.lad = lad;
  a.row_j = s.secret_scratch<uint32_t>(max_rows); a.row_ok = (uint8_t*)s.secret_scratch<uint32_t>((max_rows + 3) / 4);
  uint32_t* list[2] = {s.secret_scratch<uint32_t>(slab), s.secret_scratch<uint32_t>(slab)};
  uint32_t* counter = s.secret_scratch<uint32_t>(1);
  SecretLadder<GA> ladder{c};
  if (ladder.take(s, max_rows)) return s.st;
  // the tail: one value per lane in LDS, (4 pw + 1) words each — 64 lanes would be 65.8 KB at pw = 64, 16 lanes are 16.4 KB and leave room
  // for several blocks per compute unit (the block size of the key kernels; 32 lanes were not measured)
  const int lanes = 16;
  for (uint64_t lo = 0; lo < q.nslots; lo += slab) {
    const uint32_t ns = (uint32_t)std::min<uint64_t>(slab, q.nslots - lo);
    a.slot0 = lo; a.nslots = ns; a.in = q.in ? q.in + lo * pw : nullptr;
    a.next_active = list[0]; a.next_count = counter;
    hipLaunchKernelGGL(k_prime_init, dim3((ns + 255) / 256), dim3(256), 0, c->stream, a);
    int cur = 0;
    uint32_t left = ns;
    bool first = true;
    while (left) {
      a.active = list[cur]; a.nactive = left; a.next_active = list[cur ^ 1];
      if (!first) {
        a.C = (int)std::min<uint64_t>(PRIME_C_MAX, std::max<uint64_t>(cmin, target / left));
        a.nrows = (uint32_t)std::max<uint64_t>(2, (uint64_t)left * a.C);
        hipLaunchKernelGGL(k_prime_rows, dim3((a.nrows + 63) / 64), dim3(64), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        int32_t st = ladder.run(q.bits, a.nrows, a.mods, a.base, a.exp, (uint64_t)pw, lad);
        c->prime_rows += a.nrows; c->prime_rounds++;
        if (st) return st;
        hipLaunchKernelGGL(k_prime_tail, dim3((a.nrows + lanes - 1) / lanes), dim3(lanes), lanes * prime_tail_lds_words_per_lane(pw) * 4, c->stream, a);
        hipLaunchKernelGGL(k_prime_pick, dim3((left + 63) / 64), dim3(64), 0, c->stream, a);
      }
      first = false;
      HIPCHK(c, hipMemsetAsync(counter, 0, 4, c->stream));
      hipLaunchKernelGGL(k_prime_window, dim3(left), dim3(64), 0, c->stream, a);
      hipLaunchKernelGGL(k_prime_compact, dim3((left + 255) / 256), dim3(256), 0, c->stream, a);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(&left, counter, 4, hipMemcpyDeviceToHost, c->stream));       // the one word of the round
      HIPCHK(c, hipStreamSynchronize(c->stream));
      cur ^= 1;
    }
    if (q.mode == PRIME_MODE_KEYGEN) {
      const uint64_t k0 = lo / 2;
      hipLaunchKernelGGL(k_prime_out_key, dim3((ns / 2 + 255) / 256), dim3(256), 0, c->stream, a, q.out_p + k0 * pw, q.out_q + k0 * pw, q.key_status + k0);
    } else {
      hipLaunchKernelGGL(k_prime_out, dim3((ns + 255) / 256), dim3(256), 0, c->stream, a, q.verdict ? q.verdict + lo : nullptr,
                         q.out_prime ? q.out_prime + lo * pw : nullptr, q.out_offset ? q.out_offset + lo : nullptr, q.out_status ? q.out_status + lo : nullptr);
    }
    HIPCHK(c, hipGetLastError());
  }
  return ZKP_OK;
}

static bool prime_bits_ok(uint32_t bits) { return bits == 512 || bits == 1024 || bits == 2048; }

// test (out_prime == nullptr, `out` is the verdict) and next
static int32_t prime_entry(zkp_ctx* c, const char* what, int mode, uint32_t bits, uint64_t count, const uint32_t* in, uint32_t rounds, const uint8_t* seed,
                           uint64_t first_index, uint8_t* out_verdict, uint32_t* out_prime, uint32_t* out_offset, uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (!prime_bits_ok(bits) || count > (1ull << 20) || rounds > PRIME_MAX_ROUNDS || (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || (rounds && !seed) ||
      (count && (!in || (mode == PRIME_MODE_TEST ? !out_verdict : !out_prime)))) {
    c->err = std::string(what) + ": invalid argument"; return ZKP_EINVAL;
  }
  if (count == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t pw = bits / 32;
  Stage s(c, flags);
  PrimeCall q{};
  q.mode = mode; q.bits = bits; q.rounds = rounds; q.nslots = count; q.first_index = first_index;
  q.in = s.in(in, count * pw);
  q.key = rounds ? (const uint32_t*)s.host_in(seed, 32) : nullptr;
  s.secret(q.key, 32);
  q.verdict = s.out(out_verdict, count);
  q.out_prime = s.out(out_prime, count * pw);
  q.out_offset = s.out(out_offset, count);
  q.out_status = s.out(out_status, count);
  if (!s.dev && !s.st) { s.secret(q.in, count * pw * 4); s.secret(q.out_prime, count * pw * 4); }       // (after a failed take, in() and out() hand back the HOST pointer)
  int32_t st;
  if ((st = s.st) || (st = prime_search(c, s, q))) return st;       // a call that failed copies nothing back: the caller's arrays stay as they were
  return s.finish();
}

extern "C" int32_t zkp_probable_prime_batch(zkp_ctx* c, uint32_t bits, uint64_t count, const uint32_t* w, uint32_t rounds, const uint8_t* seed,
                                            uint64_t first_index, uint8_t* out_verdict, uint32_t flags) try {
  return prime_entry(c, "zkp_probable_prime_batch", PRIME_MODE_TEST, bits, count, w, rounds, seed, first_index, out_verdict, nullptr, nullptr, nullptr, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_next_prime_batch(zkp_ctx* c, uint32_t bits, uint64_t count, const uint32_t* start, uint32_t rounds, const uint8_t* seed,
                                        uint64_t first_index, uint32_t* out_prime, uint32_t* out_offset, uint8_t* out_status, uint32_t flags) try {
  return prime_entry(c, "zkp_next_prime_batch", PRIME_MODE_NEXT, bits, count, start, rounds, seed, first_index, nullptr, out_prime, out_offset, out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_paillier_keygen_seeded_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, uint32_t rounds, const uint8_t* seed, uint64_t first_index,
                                                    uint32_t* out_p, uint32_t* out_q, uint32_t* out_n, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!key_bits_ok(n_bits) || batch > (1ull << 20) || rounds > PRIME_MAX_ROUNDS || (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !seed || (batch && (!out_p || !out_q))) {
    c->err = "zkp_paillier_keygen_seeded_batch: invalid argument"; return ZKP_EINVAL;
  }
  if (batch == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t hw = n_bits / 64, kw = n_bits / 32;
  Stage s(c, flags);
  PrimeCall q{};
  q.mode = PRIME_MODE_KEYGEN; q.bits = n_bits / 2; q.rounds = rounds; q.nslots = 2 * batch; q.first_index = first_index;
  q.key = (const uint32_t*)s.host_in(seed, 32);
  s.secret(q.key, 32);
  q.out_p = s.out(out_p, batch * hw);
  q.out_q = s.out(out_q, batch * hw);
  uint32_t* dn = s.out(out_n, batch * kw);
  q.key_status = s.out(out_status, batch);
  if (!s.dev && !s.st) { s.secret(q.out_p, batch * hw * 4); s.secret(q.out_q, batch * hw * 4); }
  if (!q.key_status) q.key_status = s.scratch<uint8_t>(batch);
  int32_t st;
  if ((st = s.st) || (st = prime_search(c, s, q))) return st;       // a call that failed copies nothing back: the caller's arrays stay as they were
  if (dn) {                                                  // n = p q (zero for a malformed key, whose p and q are zero)
    hipLaunchKernelGGL(k_ck_prove_n, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, c->stream, q.out_p, q.out_q, (int)hw, batch, dn);
    HIPCHK(c, hipGetLastError());
  }
  return s.finish();
} ZKP_CATCH(c)

// measurement only (tools/dev/keygen_ab.py): chunk > 0 sets the least rows per slot and round for this ctx, target_rows > 0 the rows a round
// aims at (1: a fixed chunk); 0 restores the built-in value, < 0 leaves it.  out_rows / out_rounds (nullable): ladder rows and rounds of
// the most recent search.  A result never depends on either.
extern "C" int32_t zkp_diag_prime_search(zkp_ctx* c, int32_t chunk, int64_t target_rows, uint64_t* out_rows, uint64_t* out_rounds) {
  if (!c || chunk > PRIME_C_MAX || target_rows > (1 << 20)) return ZKP_EINVAL;
  if (chunk >= 0) c->prime_chunk = chunk;
  if (target_rows >= 0) c->prime_target = (uint64_t)target_rows;
  if (out_rows) *out_rows = c->prime_rows;
  if (out_rounds) *out_rounds = c->prime_rounds;
  return ZKP_OK;
}

extern "C" int32_t zkp_diag_prime_table(uint32_t* out_count, uint32_t* out_last) {
  if (!out_count || !out_last) return ZKP_EINVAL;
  *out_count = PRIME_TABLE_HOST.count;
  *out_last = PRIME_TABLE_HOST.p[PRIME_TABLE_HOST.count - 1];
  return ZKP_OK;
}
