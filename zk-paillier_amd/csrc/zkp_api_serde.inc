// zkp_api_serde.inc — wire-format ingestion (SURVEY §8(f) rank 3); included by zkp_api.hip.
// Host: tokenise serde_json documents of the reference's proof types (threads, one document at a time) into lists of
// (text offset, length, destination) per big integer.  GPU: k_dec2bin converts every decimal string straight into the
// SoA limb arrays of the batch.

#include "json_host.hpp"

namespace {
// bigint_forms = ZKP_BIGINT_FORMS(key, bare): the text form of ek.n, the text form of every other un-annotated integer, and whether both are forms
struct BigintForms { uint32_t key, bare; bool ok; };
BigintForms decode_forms(uint32_t forms) {
  const uint32_t key = (forms >> 4) & 15u, bare = forms & 15u;
  return {key, bare, !(forms >> 8) && key <= ZKP_BIGINT_BYTES && bare <= ZKP_BIGINT_BYTES};
}

// The end of a call: the first error goes into the stage (nothing is copied back after one), the outputs are delivered and the blocks returned;
// sync: the stream is idle when the call returns, in device-pointer mode too (host vectors of the call were read by copies on it)
int32_t call_end(zkp_ctx* c, Stage& s, int32_t st, bool sync = false) {
  if (st && !s.st) s.st = st;
  const int32_t fin = s.finish();
  if (sync && hipStreamSynchronize(c->stream) != hipSuccess && !st) { st = ZKP_EDEVICE; c->err = "stream sync"; }
  return st ? st : fin;
}
}  // namespace

extern "C" uint32_t zkp_decimal_pitch(uint32_t words) { return (uint32_t)((uint64_t)words * 32 * 30103 / 100000 + 2); }

static int32_t launch_dec2bin(zkp_ctx* c, const char* dtext, const zkp_dec_item* ditems, uint64_t count, uint32_t* dst, uint8_t* dstatus, uint32_t max_words) {
  if (count == 0) return ZKP_OK;
  const size_t lds = (size_t)max_words * SERDE_LANES * 4;
  hipLaunchKernelGGL(k_dec2bin, dim3((unsigned)((count + SERDE_LANES - 1) / SERDE_LANES)), dim3(SERDE_LANES), lds, c->stream, dtext, ditems, count, dst, dstatus,
                     (int)max_words);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

extern "C" int32_t zkp_decimal_to_limbs_batch(zkp_ctx* c, const char* text, uint64_t text_len, const zkp_dec_item* items, uint64_t count, uint32_t* dst,
                                              uint64_t dst_words, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (count == 0) return ZKP_OK;
  if (!text || !items || !dst || !out_status) { c->err = "zkp_decimal_to_limbs_batch: invalid argument"; return ZKP_EINVAL; }
  const bool dev = (flags & ZKP_F_DEVICE_PTRS) != 0;
  uint32_t max_words = 0;
  if (!dev) {
    for (uint64_t i = 0; i < count; i++) {
      const zkp_dec_item& it = items[i];
      if (it.words == 0 || it.words > 512 || it.text_off + it.len > text_len || it.dst_off + it.words > dst_words) { c->err = "zkp_decimal_to_limbs_batch: item out of range"; return ZKP_EINVAL; }
      max_words = std::max(max_words, it.words);
    }
  } else {
    max_words = 512;    // device-resident item list: not inspected here
  }
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  const char* dt = s.in(text, text_len);
  const zkp_dec_item* di = s.in(items, count);
  uint32_t* dd = s.out(dst, dst_words, true);
  uint8_t* ds = s.out(out_status, count);
  int32_t st = s.st;
  if (!st) st = launch_dec2bin(c, dt, di, count, dd, ds, max_words);
  return call_end(c, s, st);
} ZKP_CATCH(c)

extern "C" int32_t zkp_limbs_to_decimal_batch(zkp_ctx* c, const uint32_t* src, uint64_t src_stride, uint32_t words, uint64_t count, char* out_text,
                                              uint32_t pitch, uint32_t* out_len, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (count == 0) return ZKP_OK;
  if (!src || !out_text || !out_len || words == 0 || words > 512 || src_stride < words || pitch < zkp_decimal_pitch(words)) {
    c->err = "zkp_limbs_to_decimal_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  const uint32_t* dsrc = s.in(src, count * src_stride);
  char* dt = s.out(out_text, count * (uint64_t)pitch);
  uint32_t* dl = s.out(out_len, count);
  int32_t st = s.st;
  if (!st) {
    hipLaunchKernelGGL(k_bin2dec, dim3((unsigned)((count + SERDE_LANES - 1) / SERDE_LANES)), dim3(SERDE_LANES), (size_t)words * SERDE_LANES * 4, c->stream, dsrc,
                       src_stride, (int)words, count, dt, pitch, dl);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_bin2dec launch"; }
  }
  return call_end(c, s, st);
} ZKP_CATCH(c)

namespace {
template <class T> void clear_failed_docs(zkp_ctx* c, const uint8_t* dstat, T* dst, uint64_t units_per_doc, uint64_t docs) {
  const uint64_t total = docs * units_per_doc;
  if (total) hipLaunchKernelGGL(k_clear_failed_docs<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, dstat, dst, units_per_doc, docs);
}

// The documents' text as the flags-0 readers upload it: byte `a` of the caller's text is d[a - lo].  The decoded copies of strings that had
// escapes (one buffer per parser thread) follow the span on the device: thread k's buffer starts at text offset extra_base[k].
struct HostText { char* d; uint64_t lo; uint64_t extra_base[READER_THREADS]; };

// convert target array q's item lists (one per thread) on the GPU and fold the item statuses into the documents'
int32_t convert_lists(zkp_ctx* c, Stage& s, const HostText& ht, const std::vector<ReaderThread>& threads, int q, uint32_t* dst, uint32_t max_words, uint8_t* d_doc_status) {
  size_t total = 0;
  for (auto& t : threads) total += t.L[q].items.size();
  if (total == 0) return ZKP_OK;
  std::vector<zkp_dec_item> items; items.reserve(total);
  std::vector<uint32_t> doc; doc.reserve(total);
  for (size_t k = 0; k < threads.size(); k++) {
    for (auto it : threads[k].L[q].items) {
      if (it.text_off & EXTRA_FLAG) it.text_off = ht.extra_base[k] + (it.text_off & ~EXTRA_FLAG);
      it.text_off -= ht.lo;
      items.push_back(it);
    }
    doc.insert(doc.end(), threads[k].L[q].doc.begin(), threads[k].L[q].doc.end());
  }
  const zkp_dec_item* di = s.host_in(items.data(), total);
  const uint32_t* dd = s.host_in(doc.data(), total);
  uint8_t* item_status = (uint8_t*)s.take(total);
  if (s.st) return s.st;
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the host vectors go out of scope
  int32_t st = launch_dec2bin(c, ht.d, di, total, dst, item_status, max_words);
  if (st) return st;
  for (int pass = 0; pass < 2; pass++)
    hipLaunchKernelGGL(k_mark_docs, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)item_status, dd, total, d_doc_status, pass);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

// The flags-0 reader of the annotated types, on host pointers: tok(b, thread, kinds, js) tokenises document b (json_host.hpp) and returns its
// status; every number it lists is converted on the GPU into tgt[q] ([B][per_doc] numbers of `words` limbs, q < ntgt), the item statuses are
// folded into the documents', and (clear) whatever was converted of a document that is not ZKP_DOC_OK is zero again.  resp_kind, resp_j: the
// [B][per_doc] row variants of a Proof, or null.  Every device block is the stage's: whatever ends the call returns them to the ctx.
template <class Tok>
int32_t json_read_host(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, int ntgt, uint32_t* const* tgt, uint32_t words, uint64_t per_doc,
                       uint8_t* resp_kind, uint8_t* resp_j, bool clear, uint8_t* out_status, Tok tok) {
  const uint64_t rows = B * per_doc;
  std::vector<uint8_t> status(B, 0), kinds(resp_kind ? rows : 0, 0), js(resp_kind ? rows : 0, 0);
  std::vector<ReaderThread> threads(READER_THREADS);
  for_docs(B, [&](uint64_t b, unsigned k) { status[b] = tok(b, threads[k], kinds.data(), js.data()); });
  Stage s(c, 0);
  uint8_t* dstat = s.out(out_status, B);
  uint32_t* dt[4] = {};
  for (int q = 0; q < ntgt; q++) dt[q] = s.out(tgt[q], rows * words);       // (zeroed: a document that lists no number for a row leaves it so)
  uint8_t* dkind = s.out(resp_kind, rows);
  uint8_t* dj = s.out(resp_j, rows);
  HostText ht{};
  uint64_t hi = 0, extra_total = 0;
  ht.lo = ~0ull;
  for (uint64_t b = 0; b < B; b++) { ht.lo = std::min(ht.lo, doc_off[b]); hi = std::max(hi, doc_off[b] + doc_len[b]); }
  for (unsigned k = 0; k < READER_THREADS; k++) { ht.extra_base[k] = hi + extra_total; extra_total += threads[k].extra.size(); }
  ht.d = (char*)s.take(std::max<uint64_t>(hi - ht.lo + extra_total, 16));
  int32_t st = s.st;
  auto h2d = [&](void* dst, const void* src, uint64_t bytes) {
    if (!st && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { st = ZKP_EDEVICE; c->err = "H2D copy"; }
  };
  h2d(ht.d, text + ht.lo, hi - ht.lo);
  for (unsigned k = 0; k < READER_THREADS; k++) h2d(ht.d + (ht.extra_base[k] - ht.lo), threads[k].extra.data(), threads[k].extra.size());
  h2d(dstat, status.data(), B);
  if (resp_kind) { h2d(dkind, kinds.data(), rows); h2d(dj, js.data(), rows); }
  for (int q = 0; q < ntgt && !st; q++) st = convert_lists(c, s, ht, threads, q, dt[q], words, dstat);
  if (!st && clear) {
    for (int q = 0; q < ntgt; q++) clear_failed_docs(c, dstat, dt[q], per_doc * words, B);
    if (resp_kind) { clear_failed_docs(c, dstat, dkind, per_doc, B); clear_failed_docs(c, dstat, dj, per_doc, B); }
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_clear_failed_docs"; }
  }
  return call_end(c, s, st, true);
}
}  // namespace

// With ZKP_F_DEVICE_PTRS every reader goes through the device scanner (json_scan, further down): the text is uploaded once and tokenised
// there, and only the documents it leaves come back to the reader's flags-0 path, as a sub-batch.
namespace {
int32_t json_scan_entry(zkp_ctx* c, const char* name, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t forms,
                        const zkp_range_ni_proofs& d, uint32_t* const* head_dst, uint8_t* out_status, uint32_t y_bits = 0);
}  // namespace

// kind: 0 = EncryptedPairs -> c1, c2; 1 = Proof -> resp_*
static int32_t json_range_entry(zkp_ctx* c, const char* name, int kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (!p || p->batch == 0) return ZKP_OK;
  const uint64_t B = p->batch, EF = p->error_factor;
  const uint32_t kw = p->n_bits / 32;
  if (!text || !doc_off || !doc_len || !out_status || !key_bits_ok(p->n_bits) || EF == 0 || EF > 256 || B > (1ull << 24) ||
      (kind == 0 && (!p->c1 || !p->c2)) || (kind == 1 && (!p->resp_kind || !p->resp_j || !p->resp_w1 || !p->resp_r1 || !p->resp_w2 || !p->resp_r2))) {
    c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (flags & ZKP_F_DEVICE_PTRS) return json_scan_entry(c, name, kind == 0 ? W_DOC_PAIRS : W_DOC_PROOF, text, doc_off, doc_len, 0, *p, nullptr, out_status);
  uint32_t* const pairs[2] = {p->c1, p->c2};
  uint32_t* const resp[4] = {p->resp_w1, p->resp_r1, p->resp_w2, p->resp_r2};
  auto tok = [&](uint64_t b, ReaderThread& T, uint8_t* kinds, uint8_t* js) { return json_range_doc(kind, text, doc_off[b], doc_len[b], b, EF, kw, T, kinds, js); };
  return kind == 0 ? json_read_host(c, text, doc_off, doc_len, B, 2, pairs, 2 * kw, EF, nullptr, nullptr, true, out_status, tok)
                   : json_read_host(c, text, doc_off, doc_len, B, 4, resp, kw, EF, p->resp_kind, p->resp_j, true, out_status, tok);
}

extern "C" int32_t zkp_json_encrypted_pairs_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                                  const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags) try {
  return json_range_entry(c, "zkp_json_encrypted_pairs_batch", 0, text, doc_off, doc_len, p, out_status, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_json_range_proof_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                              const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags) try {
  return json_range_entry(c, "zkp_json_range_proof_batch", 1, text, doc_off, doc_len, p, out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_json_correct_key_proof_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits,
                                                    uint64_t B, uint32_t* out_sigma, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  if (!text || !doc_off || !doc_len || !out_sigma || !out_status || !key_bits_ok(n_bits) || B > (1ull << 24)) {
    c->err = "zkp_json_correct_key_proof_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (flags & ZKP_F_DEVICE_PTRS) {
    zkp_range_ni_proofs d{};
    d.n_bits = n_bits; d.batch = B; d.resp_w1 = out_sigma;
    return json_scan_entry(c, "zkp_json_correct_key_proof_batch", W_DOC_CK, text, doc_off, doc_len, 0, d, nullptr, out_status);
  }
  // Two things set this reader apart from the range kinds, and both stay: the sigma rows of a document that fails are NOT cleared (clear = false:
  // an over-wide entry is zero, the others stay converted), and the status of a malformed document is written as ZKP_VERDICT_MALFORMED.
  static_assert(ZKP_VERDICT_MALFORMED == ZKP_DOC_INVALID, "the tokeniser's ZKP_DOC_INVALID is the byte this reader documents as ZKP_VERDICT_MALFORMED");
  const uint32_t kw = n_bits / 32;
  uint32_t* const sigma[1] = {out_sigma};
  return json_read_host(c, text, doc_off, doc_len, B, 1, sigma, kw, ZKP_CORRECT_KEY_M2, nullptr, nullptr, false, out_status,
                        [&](uint64_t b, ReaderThread& T, uint8_t*, uint8_t*) { return json_sigma_vec_doc(text, doc_off[b], doc_len[b], b, kw, T); });
} ZKP_CATCH(c)

// ---- the same documents through the device scanner (kernels_serde_scan.hpp): the text is uploaded once and tokenised there; what the
// scanner does not take byte for byte goes through the host reader above, unchanged, and is merged into the same device arrays.
namespace {
int32_t scan_event(zkp_ctx* c, int k) {
  if (!c->ev_scan[k]) HIPCHK(c, hipEventCreate(&c->ev_scan[k]));
  HIPCHK(c, hipEventRecord(c->ev_scan[k], c->stream));
  c->scan_phases = k + 1;
  return ZKP_OK;
}
template <class T> int32_t scan_merge(zkp_ctx* c, Stage& s, const std::vector<T>& host, T* dst, uint64_t units_per_doc, const uint32_t* didx, uint64_t docs) {
  const T* src = s.host_in(host.data(), host.size());
  if (s.st) return s.st;
  const uint64_t total = docs * units_per_doc;
  return launch_rows(c, k_scan_merge<T>, total, src, dst, units_per_doc, didx, docs);
}

// the text of a call as the scanner reads it, uploaded by the caller: byte `a` of the caller's text is d[a - lo], and 16 bytes '0' follow the span
struct ScanText { char* d; uint64_t lo, span; };
void scan_span(const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint64_t* lo, uint64_t* hi) {
  for (uint64_t b = 0; b < B; b++) if (doc_len[b]) { *lo = std::min(*lo, doc_off[b]); *hi = std::max(*hi, doc_off[b] + doc_len[b]); }
}
// The start of every call that scans: the counters of zkp_diag_last_json_scan start over, event 0, and the span of the call's one or two lists
// of documents (off2 / len2 nullable) goes to the device
int32_t scan_begin(zkp_ctx* c, Stage& s, const char* text, const uint64_t* off1, const uint64_t* len1, const uint64_t* off2, const uint64_t* len2, uint64_t B, ScanText* o) {
  c->scan_fast = c->scan_fallback = 0; c->scan_phases = 0;
  if (const int32_t st = scan_event(c, 0)) return st;
  uint64_t lo = ~0ull, hi = 0;
  scan_span(off1, len1, B, &lo, &hi);
  if (off2) scan_span(off2, len2, B, &lo, &hi);
  if (hi == 0) lo = 0;
  o->lo = lo; o->span = hi - lo;
  o->d = (char*)s.take(o->span + 16);
  if (s.st) return s.st;
  if (o->span) HIPCHK(c, hipMemcpyAsync(o->d, text + lo, o->span, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(o->d + o->span, '0', 16, c->stream));
  return ZKP_OK;
}

// One batch of documents of one kind (W_DOC_*) into device memory, from text the caller has uploaded (scan_begin).  Every kind takes d.n_bits and
// d.batch; its destinations are
//   RangeProofNi        every array of d; d.n is the verifier's key when d.n_stride == 0 (an input), else it receives the documents' keys
//   EncryptedPairs      d.c1, d.c2                      Proof   d.resp_*
//   NiCorrectKeyProof   d.resp_w1: sigma [B][11][kw] (the writer's W_ARR_W1)
//   a heads-only kind   head_dst[i]: head i of w_doc_spec(doc_kind), one number per document (CompositeDLogProof.y: y_bits / 32 words)
// forms is ZKP_BIGINT_FORMS(key, bare) (the DLog kinds have no key: the bare form alone).
// Statuses and arrays are what the kind's reader gives with flags == 0 on host arrays, byte for byte:
//   - a scanned document has no malformed number and no sign, so the only status left is k_dec2bin's overflow (ZKP_DOC_HOST_PATH);
//   - RangeProofNi: the head is converted and marked first, then compared with the verifier's key (ZKP_DOC_INVALID, as the host reader
//     decides before it looks at the rows), then the rows: k_mark_docs only ever turns ZKP_DOC_OK into ZKP_DOC_HOST_PATH;
//   - what was converted of a document that ends up unconverted is cleared where the host reader clears it: everywhere but in sigma and in
//     the heads-only kinds, where an over-wide field is zero and the others stay converted.
// marks: the call scans once, and events 1 and 2 of zkp_diag_last_json_scan_ms lie around the scan kernel (the caller records 0 and 3).
int32_t json_scan(zkp_ctx* c, Stage& s, const char* name, uint32_t doc_kind, const ScanText& up, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                  uint32_t forms, const zkp_range_ni_proofs& d, uint32_t* const* head_dst, uint8_t* dstat, uint32_t y_bits, bool marks) {
  const bool ni = doc_kind == W_DOC_NI, ck = doc_kind == W_DOC_CK, has_pairs = ni || doc_kind == W_DOC_PAIRS, has_rows = ni || doc_kind == W_DOC_PROOF;
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const bool dl = spec.heads_only, heads = spec.n_heads != 0;
  const uint64_t B = d.batch, EF = ck ? ZKP_CORRECT_KEY_M2 : dl ? 0 : d.error_factor, rows = B * EF;
  const uint32_t kw = d.n_bits / 32, yw = y_bits / 32;
  const uint32_t key_form = decode_forms(forms).key, bare_form = decode_forms(forms).bare;
  const bool per_key = !ni || d.n_stride != 0;      // head 0 is one number per document and a destination (not the batch's one key)
  int32_t st = ZKP_OK;
  const uint64_t lo = up.lo, span = up.span;
  ScanJob J{};
  char* dtext = up.d;
  J.doc_off = s.host_in(doc_off, B); J.doc_len = s.host_in(doc_len, B);
  J.text = dtext; J.lo = lo; J.B = B; J.zero_at = span;
  J.max_len = zkp_json_doc_bound(doc_kind, d.n_bits, d.error_factor, forms);
  J.doc_kind = doc_kind; J.ef = (uint32_t)EF; J.kw = kw; J.key_form = key_form; J.bare_form = bare_form;
  J.dig_n = zkp_decimal_pitch(kw) - 1; J.dig_c = zkp_decimal_pitch(2 * kw) - 1;      // (max_digits below)
  // the heads: the table's rows with this batch's widths, forms and destinations (a RangeProofNi under the verifier's key reads its own into a block)
  uint32_t* const ni_dst[3] = {!ni ? nullptr : per_key ? const_cast<uint32_t*>(d.n) : (uint32_t*)s.take(B * kw * 4), const_cast<uint32_t*>(d.range),
                               const_cast<uint32_t*>(d.ciphertext)};
  if (ni) head_dst = ni_dst;
  J.n_heads = spec.n_heads; J.heads_only = spec.heads_only;
  struct Target { int arr; uint32_t* dst; uint32_t words; };      // arr < W_ARR_C1: head `arr`, one number per document; else EF
  std::vector<Target> targets;
  for (uint32_t i = 0; i < spec.n_heads; i++) {
    ScanHead& h = J.head[i];
    w_head_lit(h, spec.h[i]);
    h.words = w_head_words(spec.h[i], kw, yw); h.dig = zkp_decimal_pitch(h.words) - 1;
    h.form = spec.h[i].key ? key_form : bare_form; h.dst = head_dst[i];
    targets.push_back({(int)i, h.dst, h.words});
  }
  if (has_rows) { J.kind = d.resp_kind; J.j = d.resp_j; }
  if (has_pairs) targets.insert(targets.end(), {{W_ARR_C1, d.c1, 2 * kw}, {W_ARR_C2, d.c2, 2 * kw}});
  if (has_rows) targets.insert(targets.end(), {{W_ARR_W1, d.resp_w1, kw}, {W_ARR_R1, d.resp_r1, kw}, {W_ARR_W2, d.resp_w2, kw}, {W_ARR_R2, d.resp_r2, kw}});
  if (ck) targets.push_back({W_ARR_W1, d.resp_w1, kw});
  for (const Target& t : targets) {
    const bool head = t.arr < W_ARR_C1;
    if (head && J.head[t.arr].form != ZKP_BIGINT_DEC) continue;
    J.items[t.arr] = (zkp_dec_item*)s.take((head ? B : rows) * sizeof(zkp_dec_item));
  }
  J.row_doc = (uint32_t*)s.take(rows * 4);
  if (heads) J.head_doc = (uint32_t*)s.take(B * 4);
  J.fast = (uint8_t*)s.take(B); J.status = dstat;
  uint8_t* item_status = (uint8_t*)s.take(std::max<uint64_t>(rows, B));
  if (s.st) return s.st;
  for (const Target& t : targets) HIPCHK(c, hipMemsetAsync(t.dst, 0, (t.arr < W_ARR_C1 ? B : rows) * t.words * 4, c->stream));
  if (has_rows) {
    HIPCHK(c, hipMemsetAsync(d.resp_kind, 0, rows, c->stream));
    HIPCHK(c, hipMemsetAsync(d.resp_j, 0, rows, c->stream));
  }
  if (marks && (st = scan_event(c, 1))) return st;
  hipLaunchKernelGGL(k_json_scan, dim3((unsigned)B), dim3(64), 0, c->stream, J);
  HIPCHK(c, hipGetLastError());
  if (marks && (st = scan_event(c, 2))) return st;
  auto convert = [&](const Target& t) -> int32_t {
    if (!J.items[t.arr]) return ZKP_OK;                      // a head integer in hex / byte-array form: the scanner wrote its limbs
    const bool head = t.arr < W_ARR_C1;
    const uint64_t count = head ? B : rows;
    const int32_t e = launch_dec2bin(c, dtext, J.items[t.arr], count, t.dst, item_status, t.words);
    if (e) return e;
    return launch_rows(c, k_mark_docs, count, item_status, head ? J.head_doc : J.row_doc, count, dstat, 0);
  };
  for (const Target& t : targets) if (t.arr < W_ARR_C1 && !st) st = convert(t);
  if (st) return st;
  if (ni && !per_key) {
    hipLaunchKernelGGL(k_scan_key_check, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, (const uint32_t*)J.head[0].dst, d.n, kw, B, (const uint8_t*)J.fast, dstat);
    HIPCHK(c, hipGetLastError());
  }
  for (const Target& t : targets) if (t.arr >= W_ARR_C1 && !st) st = convert(t);
  if (st) return st;
  if (!ck && !dl) {
    for (const Target& t : targets) {
      if (t.arr == W_ARR_N && !per_key) continue;
      clear_failed_docs(c, dstat, t.dst, (t.arr < W_ARR_C1 ? 1 : EF) * t.words, B);
    }
    if (has_rows) { clear_failed_docs(c, dstat, d.resp_kind, EF, B); clear_failed_docs(c, dstat, d.resp_j, EF, B); }
    HIPCHK(c, hipGetLastError());
  }
  // the documents the scanner left: the host reader, on host arrays of their own, merged into the batch
  std::vector<uint8_t> fast(B);
  HIPCHK(c, hipMemcpyAsync(fast.data(), J.fast, B, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<uint32_t> idx;
  for (uint64_t b = 0; b < B; b++) if (!fast[b]) idx.push_back((uint32_t)b);
  c->scan_fast += B - idx.size(); c->scan_fallback += idx.size();
  if (!idx.empty()) {
    const uint64_t nf = idx.size();
    std::vector<uint64_t> foff(nf), flen(nf);
    for (uint64_t i = 0; i < nf; i++) { foff[i] = doc_off[idx[i]]; flen[i] = doc_len[idx[i]]; }
    std::vector<std::vector<uint32_t>> h(W_ARRS);
    for (const Target& t : targets) h[t.arr].resize(t.arr == W_ARR_N && !per_key ? kw : nf * (t.arr < W_ARR_C1 ? 1 : EF) * t.words);
    std::vector<uint8_t> hkind(has_rows ? nf * EF : 0), hj(has_rows ? nf * EF : 0), hst(nf, 0);
    if (ni && !per_key) { HIPCHK(c, hipMemcpyAsync(h[W_ARR_N].data(), d.n, (size_t)kw * 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    zkp_range_ni_proofs hp = d;
    hp.batch = nf; hp.n = h[W_ARR_N].data(); hp.range = h[W_ARR_RANGE].data(); hp.ciphertext = h[W_ARR_CT].data(); hp.c1 = h[W_ARR_C1].data(); hp.c2 = h[W_ARR_C2].data();
    hp.resp_kind = hkind.data(); hp.resp_j = hj.data();
    hp.resp_w1 = h[W_ARR_W1].data(); hp.resp_r1 = h[W_ARR_R1].data(); hp.resp_w2 = h[W_ARR_W2].data(); hp.resp_r2 = h[W_ARR_R2].data();
    uint32_t* hdl[W_MAX_HEADS];
    for (int i = 0; i < W_MAX_HEADS; i++) hdl[i] = h[i].data();
    st = dl              ? json_heads_host(text, foff.data(), flen.data(), nf, doc_kind, key_form, bare_form, kw, yw, hdl, hst.data())
         : ni            ? zkp_json_range_proof_ni_batch(c, text, foff.data(), flen.data(), forms, &hp, hst.data(), 0)
         : ck            ? zkp_json_correct_key_proof_batch(c, text, foff.data(), flen.data(), d.n_bits, nf, h[W_ARR_W1].data(), hst.data(), 0)
         : has_pairs     ? zkp_json_encrypted_pairs_batch(c, text, foff.data(), flen.data(), &hp, hst.data(), 0)
                         : zkp_json_range_proof_batch(c, text, foff.data(), flen.data(), &hp, hst.data(), 0);
    if (st) { c->err = std::string(name) + ": host reader: " + c->err; return st; }
    const uint32_t* didx = s.host_in(idx.data(), nf);
    if (s.st) return s.st;
    for (const Target& t : targets) {
      if (t.arr == W_ARR_N && !per_key) continue;
      if (!st) st = scan_merge(c, s, h[t.arr], t.dst, (t.arr < W_ARR_C1 ? 1 : EF) * t.words, didx, nf);
    }
    if (has_rows) {
      if (!st) st = scan_merge(c, s, hkind, d.resp_kind, EF, didx, nf);
      if (!st) st = scan_merge(c, s, hj, d.resp_j, EF, didx, nf);
    }
    if (!st) st = scan_merge(c, s, hst, dstat, 1, didx, nf);
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // the host vectors go out of scope
  }
  return ZKP_OK;
}
// a call that scans ONE list of documents; the phases of zkp_diag_last_json_scan_ms: upload | scan | convert and merge | (a verify: the rest)
int32_t scan_one(zkp_ctx* c, Stage& s, const char* name, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t forms,
                 const zkp_range_ni_proofs& d, uint32_t* const* head_dst, uint8_t* dstat, uint32_t y_bits = 0) {
  ScanText up{};
  int32_t st = scan_begin(c, s, text, doc_off, doc_len, nullptr, nullptr, d.batch, &up);
  if (!st) st = json_scan(c, s, name, doc_kind, up, text, doc_off, doc_len, forms, d, head_dst, dstat, y_bits, true);
  return st ? st : scan_event(c, 3);
}
// The prelude of a verify of (statement, proof) pairs: two lists of documents in one text, uploaded once; the statements are scanned into st_dst
// with their statuses in dstat, the proofs into pf_dst with theirs in dstat2.  The phases: upload | statements read | proofs read | (the rest)
int32_t scan_pairs(zkp_ctx* c, Stage& s, const char* name, const char* text, uint32_t st_kind, const uint64_t* st_off, const uint64_t* st_len, uint32_t* const* st_dst,
                   uint8_t* dstat, uint32_t pf_kind, const uint64_t* pf_off, const uint64_t* pf_len, uint32_t* const* pf_dst, uint8_t* dstat2, uint64_t B, uint32_t n_bits,
                   uint32_t y_bits, uint32_t forms) {
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.batch = B;
  ScanText up{};
  int32_t st = scan_begin(c, s, text, st_off, st_len, pf_off, pf_len, B, &up);
  if (!st) st = scan_event(c, 1);
  if (!st) st = json_scan(c, s, name, st_kind, up, text, st_off, st_len, forms, d, st_dst, dstat, y_bits, false);
  if (!st) st = scan_event(c, 2);
  if (!st) st = json_scan(c, s, name, pf_kind, up, text, pf_off, pf_len, forms, d, pf_dst, dstat2, y_bits, false);
  return st ? st : scan_event(c, 3);
}
// The end of every verify on documents: the verdicts of the documents that were not converted are masked, event 4, the call's end
int32_t verify_end(zkp_ctx* c, Stage& s, int32_t st, const uint8_t* dstat, uint8_t* dv, uint64_t B) {
  if (!st) {
    hipLaunchKernelGGL(k_scan_mask_verdicts, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, dstat, dv, B);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_scan_mask_verdicts launch"; }
  }
  if (!st) st = scan_event(c, 4);
  return call_end(c, s, st, true);
}
int32_t json_scan_entry(zkp_ctx* c, const char* name, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t forms,
                        const zkp_range_ni_proofs& d, uint32_t* const* head_dst, uint8_t* out_status, uint32_t y_bits) {
  Stage s(c, ZKP_F_DEVICE_PTRS);
  return call_end(c, s, scan_one(c, s, name, doc_kind, text, doc_off, doc_len, forms, d, head_dst, out_status, y_bits), true);
}
bool json_ni_common_args_ok(const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t n_bits, uint32_t ef, uint32_t forms) {
  return text && doc_off && doc_len && B <= (1ull << 24) && key_bits_ok(n_bits) && ef != 0 && ef <= 256 && decode_forms(forms).ok;
}
}  // namespace

extern "C" int32_t zkp_diag_last_json_scan(zkp_ctx* c, uint64_t* fast_docs, uint64_t* fallback_docs) {
  if (!c || !fast_docs || !fallback_docs) return ZKP_EINVAL;
  *fast_docs = c->scan_fast; *fallback_docs = c->scan_fallback;
  return ZKP_OK;
}
extern "C" int32_t zkp_diag_last_json_scan_ms(zkp_ctx* c, double* out_ms) try {
  if (!c || !out_ms) return ZKP_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 4; k++) {
    float ms = 0;
    if (k + 1 < c->scan_phases) HIPCHK(c, hipEventElapsedTime(&ms, c->ev_scan[k], c->ev_scan[k + 1]));
    out_ms[k] = ms;
  }
  return ZKP_OK;
} ZKP_CATCH(c)

extern "C" int32_t zkp_range_ni_verify_json_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t n_bits,
                                                  uint32_t error_factor, uint32_t bigint_forms, const uint32_t* verifier_n, uint8_t* out_status,
                                                  uint8_t* out_verdict, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  if ((flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !out_status || !out_verdict || !json_ni_common_args_ok(text, doc_off, doc_len, B, n_bits, error_factor, bigint_forms)) {
    c->err = "zkp_range_ni_verify_json_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t kw = n_bits / 32, rows = B * error_factor;
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint8_t* dv = s.out(out_verdict, B);
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.error_factor = error_factor; d.batch = B; d.n_stride = verifier_n ? 0 : kw;
  d.n = verifier_n ? s.host_in(verifier_n, kw) : (const uint32_t*)s.take(B * kw * 4);
  d.range = (const uint32_t*)s.take(B * kw * 4); d.ciphertext = (const uint32_t*)s.take(B * 2 * kw * 4);
  d.c1 = (uint32_t*)s.take(rows * 2 * kw * 4); d.c2 = (uint32_t*)s.take(rows * 2 * kw * 4);
  d.resp_kind = (uint8_t*)s.take(rows); d.resp_j = (uint8_t*)s.take(rows);
  d.resp_w1 = (uint32_t*)s.take(rows * kw * 4); d.resp_r1 = (uint32_t*)s.take(rows * kw * 4);
  d.resp_w2 = (uint32_t*)s.take(rows * kw * 4); d.resp_r2 = (uint32_t*)s.take(rows * kw * 4);
  int32_t st = s.st;
  if (!st) st = scan_one(c, s, "zkp_range_ni_verify_json_batch", W_DOC_NI, text, doc_off, doc_len, bigint_forms, d, nullptr, dstat);
  // The whole batch is verified and the verdicts of the documents that were not converted are masked afterwards: their rows are zero, and
  // with verify_self so is their key, which the verify kernels answer with a verdict of that proof alone (never an error of the call).
  if (!st) st = zkp_range_ni_verify_batch(c, &d, dv, ZKP_F_DEVICE_PTRS);
  return verify_end(c, s, st, dstat, dv, B);
} ZKP_CATCH(c)

// RangeProof::verifier_output (range_proof.rs:254-355) on the two received documents of a session: EncryptedPairs b and Proof b are two spans of
// one text, uploaded once and read by the device route of the two readers into arrays the call owns; the statement and the verifier's own
// challenge come in as limbs and bytes.  The status of a session is the worse of its two documents'; zkp_range_verifier_output_batch runs on the
// whole batch — an unread document is zero rows under the caller's key, answered with a verdict of that session alone — and the verdicts of
// unread sessions are masked afterwards.  The events of zkp_diag_last_json_scan_ms are: upload | pairs read | proofs read | verify.
extern "C" int32_t zkp_range_verifier_output_json_batch(zkp_ctx* c, const char* text, const uint64_t* pairs_off, const uint64_t* pairs_len, const uint64_t* proof_off,
                                                        const uint64_t* proof_len, uint64_t B, uint32_t n_bits, uint32_t error_factor, const uint32_t* n, uint64_t n_stride,
                                                        const uint32_t* range, const uint32_t* ciphertext, const uint8_t* e, const uint8_t* e_len, uint8_t* out_status,
                                                        uint8_t* out_verdict, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  if ((flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !text || !pairs_off || !pairs_len || !proof_off || !proof_len || !n || !range || !ciphertext || !e || !e_len || !out_status ||
      !out_verdict || !key_bits_ok(n_bits) || error_factor == 0 || error_factor > 256 || B > (1ull << 24) || (n_stride != 0 && n_stride != n_bits / 32)) {
    c->err = "zkp_range_verifier_output_json_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const char* name = "zkp_range_verifier_output_json_batch";
  const uint64_t kw = n_bits / 32, rows = B * error_factor;
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint8_t* dv = s.out(out_verdict, B);
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.error_factor = error_factor; d.batch = B; d.n_stride = n_stride;
  d.n = s.in(n, n_stride ? B * kw : kw); d.range = s.in(range, B * kw); d.ciphertext = s.in(ciphertext, B * 2 * kw);
  const uint8_t* de = s.in(e, B * 32);
  const uint8_t* dl = s.in(e_len, B);
  d.c1 = (uint32_t*)s.take(rows * 2 * kw * 4); d.c2 = (uint32_t*)s.take(rows * 2 * kw * 4);
  d.resp_kind = (uint8_t*)s.take(rows); d.resp_j = (uint8_t*)s.take(rows);
  d.resp_w1 = (uint32_t*)s.take(rows * kw * 4); d.resp_r1 = (uint32_t*)s.take(rows * kw * 4);
  d.resp_w2 = (uint32_t*)s.take(rows * kw * 4); d.resp_r2 = (uint32_t*)s.take(rows * kw * 4);
  uint8_t* dstat2 = (uint8_t*)s.take(B);
  ScanText up{};
  int32_t st = s.st;
  if (!st) st = scan_begin(c, s, text, pairs_off, pairs_len, proof_off, proof_len, B, &up);
  if (!st) st = scan_event(c, 1);
  if (!st) st = json_scan(c, s, name, W_DOC_PAIRS, up, text, pairs_off, pairs_len, 0, d, nullptr, dstat, 0, false);
  if (!st) st = scan_event(c, 2);
  if (!st) st = json_scan(c, s, name, W_DOC_PROOF, up, text, proof_off, proof_len, 0, d, nullptr, dstat2, 0, false);
  if (!st) st = scan_event(c, 3);
  if (!st) {
    hipLaunchKernelGGL(k_scan_worse_status, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, dstat, (const uint8_t*)dstat2, B);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_scan_worse_status launch"; }
  }
  if (!st) st = zkp_range_verifier_output_batch(c, &d, de, dl, dv, ZKP_F_DEVICE_PTRS);
  return verify_end(c, s, st, dstat, dv, B);
} ZKP_CATCH(c)

// NiCorrectKeyProof::verify on documents: the same three steps with sigma in a block the call owns.  An unread document leaves zero (or, where
// one number overflowed, partly converted) sigma rows: k_ck_check answers them with a verdict of that proof alone, masked afterwards.
extern "C" int32_t zkp_correct_key_ni_verify_json_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t n_bits,
                                                        const uint32_t* n, const uint8_t* salt, uint32_t salt_len, uint8_t* out_status, uint8_t* out_verdict,
                                                        uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  if ((flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !text || !doc_off || !doc_len || !n || !out_status || !out_verdict || (salt_len && !salt) ||
      !key_bits_ok(n_bits) || B > (1ull << 24)) {
    c->err = "zkp_correct_key_ni_verify_json_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t kw = n_bits / 32;
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint8_t* dv = s.out(out_verdict, B);
  const uint32_t* dn = s.in(n, B * kw);
  uint32_t* dsig = (uint32_t*)s.take(B * ZKP_CORRECT_KEY_M2 * kw * 4);
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.batch = B; d.resp_w1 = dsig;
  int32_t st = s.st;
  if (!st) st = scan_one(c, s, "zkp_correct_key_ni_verify_json_batch", W_DOC_CK, text, doc_off, doc_len, 0, d, nullptr, dstat);
  if (!st) st = zkp_correct_key_ni_verify_batch(c, n_bits, B, dn, dsig, salt, salt_len, dv, ZKP_F_DEVICE_PTRS);
  return verify_end(c, s, st, dstat, dv, B);
} ZKP_CATCH(c)

// ---- whole RangeProofNi documents (range_proof_ni.rs:36-44): {"ek":..,"range":..,"ciphertext":..,"encrypted_pairs":..,"proof":..,"error_factor":..}
// encrypted_pairs / proof are the annotated types above (serialize::{vecbigint,bigint}: decimal strings, serialize.rs:1-78) and go
// through the same GPU conversion; ek, range and ciphertext are UN-annotated (EncryptionKey of kzen-paillier, bare curv BigInt):
// their text form is fixed by crates that are not in the tree, so the caller names it — the sample a Rust build writes
// (tools/reference_vectors: "serde" section) decides which one is real:
//   ZKP_BIGINT_DEC   "1234"            decimal string (what serialize::bigint writes)
//   ZKP_BIGINT_HEX   "04d2"            hex string of the big-endian magnitude (either case, odd length allowed)
//   ZKP_BIGINT_BYTES [4,210]           array of big-endian byte values (serde_json's rendering of serialize_bytes)
// EncryptionKey: an object with a field "n" in that form (other fields, e.g. "nn", are skipped).  This is the host-pointer reader (flags 0);
// with ZKP_F_DEVICE_PTRS the documents go through the device scanner first (json_scan below) and only its fall-backs come here.
extern "C" int32_t zkp_json_range_proof_ni_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t bigint_forms,
                                                 const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!p || p->batch == 0) return ZKP_OK;
  if (flags == ZKP_F_DEVICE_PTRS) {
    // the batch and the statuses in device memory (with one shared key the verifier's key too): the device scanner's route
    if (!out_status || !p->n || !p->range || !p->ciphertext || !p->c1 || !p->c2 || !p->resp_kind || !p->resp_j || !p->resp_w1 || !p->resp_r1 || !p->resp_w2 ||
        !p->resp_r2 || (p->n_stride != 0 && p->n_stride != p->n_bits / 32) || !json_ni_common_args_ok(text, doc_off, doc_len, p->batch, p->n_bits, p->error_factor, bigint_forms)) {
      c->err = "zkp_json_range_proof_ni_batch: invalid argument"; return ZKP_EINVAL;
    }
    HIPCHK(c, hipSetDevice(c->device));
    return json_scan_entry(c, "zkp_json_range_proof_ni_batch", W_DOC_NI, text, doc_off, doc_len, bigint_forms, *p, nullptr, out_status);
  }
  const uint64_t B = p->batch;
  const uint32_t kw = p->n_bits / 32;
  const BigintForms forms = decode_forms(bigint_forms);
  if (flags != 0 || !text || !doc_off || !doc_len || !out_status || !p->n || !p->range || !p->ciphertext || !forms.ok || (p->n_stride != 0 && p->n_stride != kw) ||
      !key_bits_ok(p->n_bits)) {
    c->err = "zkp_json_range_proof_ni_batch: invalid argument"; return ZKP_EINVAL;
  }
  // (range and ciphertext — and n with one key per proof — are inputs of every other entry point, hence const in the struct; here
  // they are what is produced.  With ONE shared key (n_stride == 0) p->n is the VERIFIER's key: an input, never written)
  uint32_t* const out_range = const_cast<uint32_t*>(p->range);
  uint32_t* const out_ct = const_cast<uint32_t*>(p->ciphertext);
  std::vector<uint8_t> top(B, 0);
  std::vector<uint64_t> ep_off(B), ep_len(B), pr_off(B), pr_len(B);
  std::vector<uint32_t> keys((size_t)B * kw, 0);
  for_docs(B, [&](uint64_t b, unsigned) {
    NiSpans sp;
    top[b] = json_range_ni_top(text, doc_off[b], doc_len[b], forms.key, forms.bare, kw, p->error_factor, &keys[b * kw], out_range + b * kw, out_ct + b * 2 * kw, &sp);
    ep_off[b] = sp.ep_off; ep_len[b] = sp.ep_len; pr_off[b] = sp.pr_off; pr_len[b] = sp.pr_len;
  });
  if (p->n_stride) {
    // one key per proof: the documents' keys are the output (verify_self semantics, range_proof_ni.rs:109-128)
    uint32_t* const out_n = const_cast<uint32_t*>(p->n);
    for (uint64_t b = 0; b < B; b++) {
      if (top[b]) memset(out_n + b * kw, 0, (size_t)kw * 4);
      else memcpy(out_n + b * kw, &keys[b * kw], (size_t)kw * 4);
    }
  } else {
    // RangeProofNi::verify(ek, ..) asserts that the proof was made under the verifier's key (range_proof_ni.rs:86): a document
    // under another key is a panic there, ZKP_DOC_INVALID here — and no document can change the key the batch is verified under
    for (uint64_t b = 0; b < B; b++)
      if (!top[b] && memcmp(&keys[b * kw], p->n, (size_t)kw * 4) != 0) {
        top[b] = ZKP_DOC_INVALID;
        memset(out_range + b * kw, 0, (size_t)kw * 4); memset(out_ct + b * 2 * kw, 0, (size_t)kw * 8); ep_off[b] = pr_off[b] = doc_off[b]; ep_len[b] = pr_len[b] = 0;
      }
  }
  std::vector<uint8_t> s1(B, 0), s2(B, 0);
  int32_t st = json_range_entry(c, "zkp_json_range_proof_ni_batch", 0, text, ep_off.data(), ep_len.data(), p, s1.data(), 0);
  if (!st) st = json_range_entry(c, "zkp_json_range_proof_ni_batch", 1, text, pr_off.data(), pr_len.data(), p, s2.data(), 0);
  for (uint64_t b = 0; b < B; b++) {
    // (the sub-documents of a document that already failed were replaced by empty spans, which read as invalid: the top status stands)
    const uint8_t a = top[b] ? top[b] : (s1[b] == ZKP_DOC_INVALID || s2[b] == ZKP_DOC_INVALID) ? (uint8_t)ZKP_DOC_INVALID : (s1[b] || s2[b]) ? (uint8_t)ZKP_DOC_HOST_PATH : (uint8_t)ZKP_DOC_OK;
    out_status[b] = a;
    if (a != ZKP_DOC_OK && !st) {      // every row of a document that is not converted as a whole is zero
      const uint64_t EF = p->error_factor;
      memset(out_range + b * kw, 0, (size_t)kw * 4); memset(out_ct + b * 2 * kw, 0, (size_t)kw * 8);
      if (p->n_stride) memset(const_cast<uint32_t*>(p->n) + b * kw, 0, (size_t)kw * 4);
      memset(p->c1 + b * EF * 2 * kw, 0, EF * 2 * kw * 4); memset(p->c2 + b * EF * 2 * kw, 0, EF * 2 * kw * 4);
      memset(p->resp_kind + b * EF, 0, EF); memset(p->resp_j + b * EF, 0, EF);
      for (uint32_t* arr : {p->resp_w1, p->resp_r1, p->resp_w2, p->resp_r2}) memset(arr + b * EF * kw, 0, EF * kw * 4);
    }
  }
  return st;
} ZKP_CATCH(c)

// ---- the writers: the SoA batch -> serde_json documents, back to back in host memory (kernels_serde_write.hpp has the three phases).
// Not modexp work: like the readers they run on this library whatever engine the ctx routes its proof calls to (no ZKP_ROUTE).
namespace {
// decimal digits of the largest value of `words` limbs (zkp_decimal_pitch is that plus one)
uint64_t max_digits(uint32_t words) { return (uint64_t)zkp_decimal_pitch(words) - 1; }
uint64_t max_form_len(uint32_t words, uint32_t form) {       // the body of an un-annotated BigInt, quotes / brackets excluded
  const uint64_t nb = 4ull * words;
  return form == ZKP_BIGINT_DEC ? max_digits(words) : form == ZKP_BIGINT_HEX ? 2 * nb : 4 * nb - 1;
}
uint64_t uint_digits(uint64_t v) { uint64_t d = 1; while (v >= 10) { v /= 10; d++; } return d; }
constexpr uint64_t cstrlen(const char* s) { return *s ? 1 + cstrlen(s + 1) : 0; }
}  // namespace

extern "C" uint64_t zkp_json_doc_bound(uint32_t doc_kind, uint32_t n_bits, uint32_t error_factor, uint32_t bigint_forms) {
  const BigintForms forms = decode_forms(bigint_forms);
  const uint32_t key_form = forms.key, bare_form = forms.bare;
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const bool dl = spec.heads_only;
  if (!key_bits_ok(n_bits) || (doc_kind > ZKP_JSON_DOC_CORRECT_KEY_PROOF && !dl) || !forms.ok || (doc_kind != ZKP_JSON_DOC_CORRECT_KEY_PROOF && !dl && error_factor == 0))
    return 0;
  const uint32_t kw = n_bits / 32;
  if (dl) {
    // a heads-only kind: the table's literals, every number at its widest between its quotes or brackets, `}` (a CompositeDLogProof's y at
    // y_bits == n_bits)
    uint64_t bound = 1;
    for (uint32_t i = 0; i < spec.n_heads; i++)
      bound += strlen(spec.h[i].lit) + 2 + max_form_len(w_head_words(spec.h[i], kw, kw), spec.h[i].key ? key_form : bare_form);
    return bound;
  }
  const uint64_t EF = error_factor, dn = max_digits(kw), dc = max_digits(2 * kw);
  if (doc_kind == ZKP_JSON_DOC_CORRECT_KEY_PROOF) return cstrlen("{\"sigma_vec\":[") + ZKP_CORRECT_KEY_M2 * (dn + 3) - 1 + cstrlen("]}");
  // {"c1":["..",".."],"c2":[..]}
  const uint64_t pairs = cstrlen("{\"c1\":[") + cstrlen("],\"c2\":[") + cstrlen("]}") + 2 * (EF * (dc + 3) - 1);
  // the longer of the two variants per row (Open for every width of this ABI; both are written down so that nothing depends on it)
  const uint64_t open = cstrlen("{\"Open\":{\"w1\":\"\",\"r1\":\"\",\"w2\":\"\",\"r2\":\"\"}}") + 4 * dn;
  const uint64_t mask = cstrlen("{\"Mask\":{\"j\":255,\"masked_x\":\"\",\"masked_r\":\"\"}}") + 2 * dn;
  const uint64_t proof = 2 + EF * (std::max(open, mask) + 1) - 1;
  if (doc_kind == ZKP_JSON_DOC_ENCRYPTED_PAIRS) return pairs;
  if (doc_kind == ZKP_JSON_DOC_RANGE_PROOF) return proof;
  return cstrlen("{\"ek\":{\"n\":},\"range\":,\"ciphertext\":,\"encrypted_pairs\":,\"proof\":,\"error_factor\":}") + 6 /* quotes or brackets */ +
         max_form_len(kw, key_form) + max_form_len(kw, bare_form) + max_form_len(2 * kw, bare_form) + pairs + proof + uint_digits(EF);
}

// the fields of a heads-only document (the two DLog kinds): field i is one number of words[i] limbs per document
struct WHeads { const uint32_t* a[W_MAX_HEADS]; uint32_t words[W_MAX_HEADS]; };
static int32_t json_write_impl(zkp_ctx* c, const char* name, uint32_t doc_kind, const zkp_range_ni_proofs* p, uint32_t n_bits, uint64_t B, uint64_t EF,
                               const uint32_t* sigma, uint32_t forms, char* out_text, uint64_t text_cap, uint64_t* out_doc_off, uint8_t* out_status, uint32_t flags,
                               const WHeads* hd = nullptr) {
  if (!c) return ZKP_EINVAL;
  const uint32_t key_form = decode_forms(forms).key, bare_form = decode_forms(forms).bare;
  const bool ck = doc_kind == W_DOC_CK, ni = doc_kind == W_DOC_NI, has_pairs = doc_kind == W_DOC_PAIRS || ni, has_proof = doc_kind == W_DOC_PROOF || ni;
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const bool dl = spec.heads_only;
  const uint32_t kw = n_bits / 32;
  bool bad = !out_doc_off || (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !key_bits_ok(n_bits) || B > (1ull << 24) || !decode_forms(forms).ok ||
             (!ck && !dl && !p) || (!ck && !dl && (EF == 0 || EF > 256));
  if (!bad && B) {
    if (dl) { bad = !hd; for (uint32_t i = 0; !bad && i < w_heads(doc_kind); i++) bad = !hd->a[i]; }
    else if (ck) bad = !sigma;
    else bad = (has_pairs && (!p->c1 || !p->c2)) || (has_proof && (!p->resp_kind || !p->resp_j || !p->resp_w1 || !p->resp_r1 || !p->resp_w2 || !p->resp_r2)) ||
               (ni && (!p->n || !p->range || !p->ciphertext || (p->n_stride != 0 && p->n_stride != kw)));
  }
  if (bad) { c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL; }
  out_doc_off[0] = 0;
  if (B == 0) return ZKP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Stage s(c, flags);
  WJob J{};
  J.B = B; J.ef = (uint32_t)EF; J.doc_kind = doc_kind; J.key_form = key_form; J.bare_form = bare_form;
  J.per_proof_keys = ni ? p->n_stride != 0 : 1;
  J.n_heads = spec.n_heads; J.heads_only = spec.heads_only;
  for (uint32_t i = 0; i < spec.n_heads; i++) { w_head_lit(J.head[i], spec.h[i]); J.head[i].key = spec.h[i].key; }
  J.slots = ck ? ZKP_CORRECT_KEY_M2 : (uint32_t)(spec.n_heads + (has_pairs ? 2 * EF : 0) + (has_proof ? 4 * EF : 0));
  struct Todo { int arr; uint64_t count; uint32_t form; };
  std::vector<Todo> todo;
  auto add = [&](int arr, const uint32_t* src, uint64_t count, uint32_t words, uint32_t form) {
    WArr& a = J.a[arr];
    a.words = words; a.G = (uint32_t)((max_digits(words) + 8) / 9);
    a.src = s.in(src, count * words);
    a.len = (uint32_t*)s.take(count * sizeof(uint32_t));
    a.groups = (uint32_t*)s.take(form == ZKP_BIGINT_DEC ? (count + 63) / 64 * 64 * a.G * sizeof(uint32_t) : count * sizeof(uint32_t));
    todo.push_back({arr, count, form});
  };
  const uint64_t rows = B * EF;
  if (ck) add(W_ARR_W1, sigma, B * ZKP_CORRECT_KEY_M2, kw, ZKP_BIGINT_DEC);
  if (dl) for (uint32_t i = 0; i < spec.n_heads; i++) add((int)i, hd->a[i], B, hd->words[i], spec.h[i].key ? key_form : bare_form);
  if (ni) {
    add(W_ARR_N, p->n, p->n_stride ? B : 1, kw, key_form);
    add(W_ARR_RANGE, p->range, B, kw, bare_form);
    add(W_ARR_CT, p->ciphertext, B, 2 * kw, bare_form);
  }
  if (has_pairs) { add(W_ARR_C1, p->c1, rows, 2 * kw, ZKP_BIGINT_DEC); add(W_ARR_C2, p->c2, rows, 2 * kw, ZKP_BIGINT_DEC); }
  if (has_proof) {
    add(W_ARR_W1, p->resp_w1, rows, kw, ZKP_BIGINT_DEC); add(W_ARR_R1, p->resp_r1, rows, kw, ZKP_BIGINT_DEC);
    add(W_ARR_W2, p->resp_w2, rows, kw, ZKP_BIGINT_DEC); add(W_ARR_R2, p->resp_r2, rows, kw, ZKP_BIGINT_DEC);
    J.kind = s.in((const uint8_t*)p->resp_kind, rows); J.j = s.in((const uint8_t*)p->resp_j, rows);
  }
  uint8_t* dstat = s.out(out_status, B);
  uint64_t* rel = (uint64_t*)s.take(B * J.slots * sizeof(uint64_t));
  uint64_t* doclen = (uint64_t*)s.take(B * sizeof(uint64_t));
  uint64_t* doff = (uint64_t*)s.take((B + 1) * sizeof(uint64_t));
  int32_t st = s.st;
  auto launched = [&](const char* what) { if (!st && hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = std::string(name) + ": " + what; } };
  if (!st) {
    // convert
    for (const Todo& t : todo) {
      const WArr& a = J.a[t.arr];
      if (t.form == ZKP_BIGINT_DEC)
        hipLaunchKernelGGL(k_w_convert, dim3((unsigned)((t.count + SERDE_LANES - 1) / SERDE_LANES)), dim3(SERDE_LANES), (size_t)a.words * SERDE_LANES * 4, c->stream, a.src,
                           (int)a.words, t.count, a.groups, a.G, a.len);
      else
        hipLaunchKernelGGL(k_w_formlen, dim3((unsigned)((t.count + 255) / 256)), dim3(256), 0, c->stream, a.src, (int)a.words, t.count, t.form, a.groups, a.len);
    }
    launched("convert");
    // size
    if (!st) {
      hipLaunchKernelGGL(k_w_doclen, dim3((unsigned)B), dim3(64), 0, c->stream, J, rel, doclen, dstat);
      hipLaunchKernelGGL(k_w_scan, dim3(1), dim3(1024), 0, c->stream, (const uint64_t*)doclen, B, doff);
      launched("size");
    }
    if (!st && (hipMemcpyAsync(out_doc_off, doff, (B + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess)) { st = ZKP_EDEVICE; c->err = std::string(name) + ": offsets D2H"; }
  }
  const uint64_t total = st ? 0 : out_doc_off[B];
  if (!st && out_text && text_cap < total) {
    st = ZKP_EINVAL;
    c->err = std::string(name) + ": text_cap " + std::to_string(text_cap) + " is less than the " + std::to_string(total) + " bytes of the documents";
    (void)s.finish();       // (the status bytes are still delivered)
    return ZKP_EINVAL;
  }
  if (!st && out_text && total) {
    // assemble, in runs of whole documents of at most `chunk` bytes: run k + 1 is assembled while run k travels to the host.  Every byte
    // is placed by its absolute offset, so the text does not depend on where the runs are cut.
    uint64_t chunk = 256ull << 20;
    if (const char* e = std::getenv("ZKP_JSON_WRITE_CHUNK")) { const unsigned long long v = std::strtoull(e, nullptr, 10); if (v) chunk = v; }
    uint64_t longest = 0;
    for (uint64_t b = 0; b < B; b++) longest = std::max(longest, out_doc_off[b + 1] - out_doc_off[b]);
    chunk = std::min(std::max(chunk, longest), total);
    Piped pipe(c, s);
    st = pipe.streams(2);
    char* buf[2] = {nullptr, nullptr};
    if (!st) { buf[0] = (char*)s.take(chunk + 8); buf[1] = chunk < total ? (char*)s.take(chunk + 8) : buf[0]; st = s.st; }
    uint64_t lo = 0;
    for (int k = 0; !st && lo < B; k++) {
      uint64_t hi = lo + 1;
      while (hi < B && out_doc_off[hi + 1] - out_doc_off[lo] <= chunk) hi++;
      const uint64_t a0 = out_doc_off[lo], a1 = out_doc_off[hi], base = a0 & ~3ull;
      hipEvent_t assembled = c->ev_pipe[k & 1], copied = c->ev_pipe[2 + (k & 1)];
      if (a1 > a0) {
        if (k >= 2 && hipStreamWaitEvent(c->stream, copied, 0) != hipSuccess) { st = ZKP_EDEVICE; c->err = "stream wait"; break; }
        const uint64_t n_slots = (hi - lo) * J.slots;
        hipLaunchKernelGGL(k_w_assemble, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, c->stream, J, (const uint64_t*)rel, (const uint64_t*)doff, lo * J.slots, n_slots,
                           buf[k & 1], base);
        launched("assemble");
        if (!st && (hipEventRecord(assembled, c->stream) != hipSuccess || hipStreamWaitEvent(c->copy, assembled, 0) != hipSuccess ||
                    hipMemcpyAsync(out_text + a0, buf[k & 1] + (a0 - base), a1 - a0, hipMemcpyDeviceToHost, c->copy) != hipSuccess ||
                    hipEventRecord(copied, c->copy) != hipSuccess)) { st = ZKP_EDEVICE; c->err = std::string(name) + ": text D2H"; }
        c->copy_busy = true;
      }
      lo = hi;
    }
    const int32_t pf = pipe.finish();
    if (!st) st = pf;
  }
  return call_end(c, s, st, true);
}

extern "C" int32_t zkp_json_write_encrypted_pairs_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, char* out_text, uint64_t text_cap, uint64_t* out_doc_off,
                                                        uint8_t* out_status, uint32_t flags) try {
  return json_write_impl(c, "zkp_json_write_encrypted_pairs_batch", W_DOC_PAIRS, p, p ? p->n_bits : 0, p ? p->batch : 0, p ? p->error_factor : 0, nullptr, 0,
                         out_text, text_cap, out_doc_off, out_status, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_json_write_range_proof_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, char* out_text, uint64_t text_cap, uint64_t* out_doc_off,
                                                    uint8_t* out_status, uint32_t flags) try {
  return json_write_impl(c, "zkp_json_write_range_proof_batch", W_DOC_PROOF, p, p ? p->n_bits : 0, p ? p->batch : 0, p ? p->error_factor : 0, nullptr, 0,
                         out_text, text_cap, out_doc_off, out_status, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_json_write_range_proof_ni_batch(zkp_ctx* c, const zkp_range_ni_proofs* p, uint32_t bigint_forms, char* out_text, uint64_t text_cap,
                                                       uint64_t* out_doc_off, uint8_t* out_status, uint32_t flags) try {
  return json_write_impl(c, "zkp_json_write_range_proof_ni_batch", W_DOC_NI, p, p ? p->n_bits : 0, p ? p->batch : 0, p ? p->error_factor : 0, nullptr, bigint_forms,
                         out_text, text_cap, out_doc_off, out_status, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_json_write_correct_key_proof_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* sigma, char* out_text, uint64_t text_cap,
                                                          uint64_t* out_doc_off, uint8_t* out_status, uint32_t flags) try {
  return json_write_impl(c, "zkp_json_write_correct_key_proof_batch", W_DOC_CK, nullptr, n_bits, batch, 0, sigma, 0, out_text, text_cap, out_doc_off, out_status, flags);
} ZKP_CATCH(c)

// ---- CompositeDLogProof and DLogStatement (wi_dlog_proof.rs:32-43): {"x":X,"y":X} and {"N":X,"g":X,"ni":X}, every X an un-annotated curv BigInt
// in the one form the caller names.
namespace {
int32_t json_dlog_entry(zkp_ctx* c, const char* name, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits,
                        uint32_t y_bits, uint64_t B, uint32_t bare_form, uint32_t* const* out, uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  bool bad = (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !text || !doc_off || !doc_len || !out_status || bare_form > ZKP_BIGINT_BYTES || !dlog_args_ok(n_bits, y_bits, B);
  for (unsigned f = 0; f < w_heads(doc_kind); f++) bad = bad || !out[f];
  if (bad) { c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL; }
  const uint32_t kw = n_bits / 32;
  if (!(flags & ZKP_F_DEVICE_PTRS)) return json_heads_host(text, doc_off, doc_len, B, doc_kind, 0, bare_form, kw, y_bits / 32, out, out_status);
  HIPCHK(c, hipSetDevice(c->device));
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.batch = B;
  return json_scan_entry(c, name, doc_kind, text, doc_off, doc_len, bare_form, d, out, out_status, y_bits);
}
}  // namespace

extern "C" int32_t zkp_json_dlog_statement_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits, uint64_t B,
                                                 uint32_t bare_form, uint32_t* out_N, uint32_t* out_g, uint32_t* out_ni, uint8_t* out_status, uint32_t flags) try {
  uint32_t* const out[3] = {out_N, out_g, out_ni};
  return json_dlog_entry(c, "zkp_json_dlog_statement_batch", W_DOC_DLOG_STATEMENT, text, doc_off, doc_len, n_bits, n_bits, B, bare_form, out, out_status, flags);
} ZKP_CATCH(c)
extern "C" int32_t zkp_json_dlog_proof_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits, uint32_t y_bits,
                                             uint64_t B, uint32_t bare_form, uint32_t* out_x, uint32_t* out_y, uint8_t* out_status, uint32_t flags) try {
  uint32_t* const out[3] = {out_x, out_y, nullptr};
  return json_dlog_entry(c, "zkp_json_dlog_proof_batch", W_DOC_DLOG_PROOF, text, doc_off, doc_len, n_bits, y_bits, B, bare_form, out, out_status, flags);
} ZKP_CATCH(c)

extern "C" int32_t zkp_json_write_dlog_statement_batch(zkp_ctx* c, uint32_t n_bits, uint64_t batch, const uint32_t* N, const uint32_t* g, const uint32_t* ni,
                                                       uint32_t bare_form, char* out_text, uint64_t text_cap, uint64_t* out_doc_off, uint8_t* out_status,
                                                       uint32_t flags) try {
  const uint32_t kw = n_bits / 32;
  const WHeads hd{{N, g, ni}, {kw, kw, kw}};
  if (c && bare_form > ZKP_BIGINT_BYTES) { c->err = "zkp_json_write_dlog_statement_batch: invalid argument"; return ZKP_EINVAL; }
  return json_write_impl(c, "zkp_json_write_dlog_statement_batch", W_DOC_DLOG_STATEMENT, nullptr, n_bits, batch, 0, nullptr, bare_form, out_text, text_cap, out_doc_off,
                         out_status, flags, &hd);
} ZKP_CATCH(c)
extern "C" int32_t zkp_json_write_dlog_proof_batch(zkp_ctx* c, uint32_t n_bits, uint32_t y_bits, uint64_t batch, const uint32_t* x, const uint32_t* y,
                                                   uint32_t bare_form, char* out_text, uint64_t text_cap, uint64_t* out_doc_off, uint8_t* out_status,
                                                   uint32_t flags) try {
  const WHeads hd{{x, y, nullptr}, {n_bits / 32, y_bits / 32, 0}};
  if (c && (bare_form > ZKP_BIGINT_BYTES || !dlog_args_ok(n_bits, y_bits, batch))) { c->err = "zkp_json_write_dlog_proof_batch: invalid argument"; return ZKP_EINVAL; }
  return json_write_impl(c, "zkp_json_write_dlog_proof_batch", W_DOC_DLOG_PROOF, nullptr, n_bits, batch, 0, nullptr, bare_form, out_text, text_cap, out_doc_off, out_status,
                         flags, &hd);
} ZKP_CATCH(c)

// CompositeDLogProof::verify (wi_dlog_proof.rs:67-91) on documents: statement b and proof b are two spans of one text, uploaded once.  Both are read
// by the device route into arrays the call owns; k_dlog_domain_check folds the two statuses and keeps every pair the limb kernels are not defined for
// (N even or zero, g / ni / x >= N) away from them; then zkp_dlog_verify_batch on the whole batch, the verdicts of unread pairs masked afterwards.
// An unread pair is five zero rows.  N = 0: k_setup marks the modulus (status 2, before any loop that depends on its value; every later loop runs
// over the fixed limb count or the exponent's bits), so k_modexp / k_modmul compute on zeros and store nothing, k_dlog_hash answers MALFORMED from
// the `N > 2^128` test without entering the GCD, and k_dlog_compare leaves that verdict alone: no placeholder modulus is needed.
// The events of zkp_diag_last_json_scan_ms are: upload | statements read | proofs read | domain check and verify.
extern "C" int32_t zkp_dlog_verify_json_batch(zkp_ctx* c, const char* text, const uint64_t* st_off, const uint64_t* st_len, const uint64_t* pf_off,
                                              const uint64_t* pf_len, uint64_t B, uint32_t n_bits, uint32_t y_bits, uint32_t bare_form, uint8_t* out_status,
                                              uint8_t* out_verdict, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  if ((flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !text || !st_off || !st_len || !pf_off || !pf_len || !out_status || !out_verdict || bare_form > ZKP_BIGINT_BYTES ||
      !dlog_args_ok(n_bits, y_bits, B)) {
    c->err = "zkp_dlog_verify_json_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t kw = n_bits / 32, yw = y_bits / 32;
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint8_t* dv = s.out(out_verdict, B);
  uint32_t* arr[4];
  for (auto& a : arr) a = (uint32_t*)s.take(B * kw * 4);
  uint32_t* dy = (uint32_t*)s.take(B * yw * 4);
  uint8_t* dstat2 = (uint8_t*)s.take(B);
  uint32_t* const pf[2] = {arr[3], dy};      // (arr[0 .. 2]: N, g, ni)
  int32_t st = s.st;
  if (!st) st = scan_pairs(c, s, "zkp_dlog_verify_json_batch", text, W_DOC_DLOG_STATEMENT, st_off, st_len, arr, dstat, W_DOC_DLOG_PROOF, pf_off, pf_len, pf, dstat2, B, n_bits,
                           y_bits, bare_form);
  if (!st) {
    hipLaunchKernelGGL(k_dlog_domain_check, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, arr[0], arr[1], arr[2], arr[3], dy, (uint32_t)kw, (uint32_t)yw, B,
                       (const uint8_t*)dstat2, dstat);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_dlog_domain_check launch"; }
  }
  if (!st) st = zkp_dlog_verify_batch(c, n_bits, y_bits, B, arr[0], arr[1], arr[2], arr[3], dy, dv, ZKP_F_DEVICE_PTRS);
  return verify_end(c, s, st, dstat, dv, B);
} ZKP_CATCH(c)

// ---- ZeroProof, CiphertextProof, VerlinProof, MulProof and their statements (zero_enc_proof.rs:26-41, correct_ciphertext.rs:22-39,
// verlin_proof.rs:34-57, multiplication_proof.rs:32-57): heads-only documents of up to five integers, the rows of w_doc_spec().
namespace {
static_assert(sizeof(zkp_sigma_fields) == 5 * sizeof(uint32_t*), "zkp_sigma_fields is five pointers back to back");
struct SigmaFieldList {
  uint32_t* f[W_MAX_HEADS] = {};
  explicit SigmaFieldList(const zkp_sigma_fields* p) { if (p) { f[0] = p->f0; f[1] = p->f1; f[2] = p->f2; f[3] = p->f3; f[4] = p->f4; } }
};
bool sigma_json_args_ok(uint32_t doc_kind, uint32_t n_bits, uint64_t B, uint32_t forms) {
  return w_sigma_kind(doc_kind) && key_bits_ok(n_bits) && B <= (1ull << 24) && decode_forms(forms).ok;
}
}  // namespace

extern "C" int32_t zkp_json_sigma_batch(zkp_ctx* c, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t n_bits, uint64_t B,
                                        uint32_t bigint_forms, const zkp_sigma_fields* out, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  bool bad = (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !text || !doc_off || !doc_len || !out || !out_status || !sigma_json_args_ok(doc_kind, n_bits, B, bigint_forms);
  const SigmaFieldList o(out);
  for (unsigned f = 0; !bad && f < w_heads(doc_kind); f++) bad = !o.f[f];
  if (bad) { c->err = "zkp_json_sigma_batch: invalid argument"; return ZKP_EINVAL; }
  const uint32_t kw = n_bits / 32;
  if (!(flags & ZKP_F_DEVICE_PTRS)) return json_heads_host(text, doc_off, doc_len, B, doc_kind, decode_forms(bigint_forms).key, decode_forms(bigint_forms).bare, kw, 0, o.f, out_status);
  HIPCHK(c, hipSetDevice(c->device));
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.batch = B;
  return json_scan_entry(c, "zkp_json_sigma_batch", doc_kind, text, doc_off, doc_len, bigint_forms, d, o.f, out_status);
} ZKP_CATCH(c)

extern "C" int32_t zkp_json_write_sigma_batch(zkp_ctx* c, uint32_t doc_kind, uint32_t n_bits, uint64_t batch, const zkp_sigma_fields* in, uint32_t bigint_forms, char* out_text,
                                              uint64_t text_cap, uint64_t* out_doc_off, uint8_t* out_status, uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (!w_sigma_kind(doc_kind) || (batch && !in)) { c->err = "zkp_json_write_sigma_batch: invalid argument"; return ZKP_EINVAL; }
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const SigmaFieldList f(in);
  WHeads hd{};
  for (uint32_t i = 0; i < spec.n_heads; i++) { hd.a[i] = f.f[i]; hd.words[i] = w_head_words(spec.h[i], n_bits / 32, 0); }
  return json_write_impl(c, "zkp_json_write_sigma_batch", doc_kind, nullptr, n_bits, batch, 0, nullptr, bigint_forms, out_text, text_cap, out_doc_off, out_status, flags, &hd);
} ZKP_CATCH(c)

// The four verifies on documents: statement b and proof b are two spans of one text, uploaded once.  Both are read by the device route into arrays the
// call owns; n^2 is squared on the device and k_sigma_domain_check folds the two statuses and keeps every pair outside the limb kernels' domain (key
// even or trivial, a 2 kw field >= n^2, MulProof.f >= n) away from them; then the type's zkp_*_verify_batch on the whole batch with one key per pair
// — it routes itself by its own work measure, on the same stream — and the verdicts of unread pairs masked afterwards.  An unread pair is zero rows
// under the key 0, which k_setup marks before any arithmetic: nothing is stored for it and the compare kernels answer MALFORMED.
// The events of zkp_diag_last_json_scan_ms are: upload | statements read | proofs read | domain check and verify.
extern "C" int32_t zkp_sigma_verify_json_batch(zkp_ctx* c, uint32_t proof_kind, const char* text, const uint64_t* st_off, const uint64_t* st_len, const uint64_t* pf_off,
                                               const uint64_t* pf_len, uint64_t B, uint32_t n_bits, uint32_t bigint_forms, uint8_t* out_status, uint8_t* out_verdict,
                                               uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  const bool is_proof = proof_kind == W_DOC_ZERO_PROOF || proof_kind == W_DOC_CT_PROOF || proof_kind == W_DOC_VERLIN_PROOF || proof_kind == W_DOC_MUL_PROOF;
  if ((flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !is_proof || !text || !st_off || !st_len || !pf_off || !pf_len || !out_status || !out_verdict ||
      !sigma_json_args_ok(proof_kind, n_bits, B, bigint_forms)) {
    c->err = "zkp_sigma_verify_json_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t st_kind = proof_kind - 1;
  const WDocSpec &ss = w_doc_spec(st_kind), &ps = w_doc_spec(proof_kind);
  const uint64_t kw = n_bits / 32;
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint8_t* dv = s.out(out_verdict, B);
  // S[i]: field i of the statement (S[0] the key), P[i]: field i of the proof
  uint32_t *S[W_MAX_HEADS] = {}, *P[W_MAX_HEADS] = {};
  SigmaDomainArgs dom{};
  auto own = [&](const WDocSpec& spec, uint32_t** arr) {
    for (uint32_t i = 0; i < spec.n_heads; i++) {
      const uint32_t w = w_head_words(spec.h[i], (uint32_t)kw, 0);
      arr[i] = (uint32_t*)s.take(B * w * 4);
      dom.arr[dom.n_arr] = arr[i]; dom.words[dom.n_arr] = w;
      dom.rule[dom.n_arr] = spec.h[i].key ? SIGMA_ANY : spec.h[i].width == W_WID_NN ? SIGMA_LT_NN : spec.h[i].width == W_WID_N ? SIGMA_LT_N : SIGMA_ANY;
      dom.n_arr++;
    }
  };
  static_assert(2 * W_MAX_HEADS - 2 <= SIGMA_MAX_ARR, "a statement (key and three fields) and a proof of five fields");
  own(ss, S); own(ps, P);
  uint32_t* nn = (uint32_t*)s.take(B * 2 * kw * 4);
  uint8_t* dstat2 = (uint8_t*)s.take(B);
  int32_t st = s.st;
  if (!st) st = scan_pairs(c, s, "zkp_sigma_verify_json_batch", text, st_kind, st_off, st_len, S, dstat, proof_kind, pf_off, pf_len, P, dstat2, B, n_bits, 0, bigint_forms);
  if (!st) {
    hipLaunchKernelGGL(k_square_words, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, c->stream, (const uint32_t*)S[0], kw, (int)kw, B, nn);
    dom.kw = (uint32_t)kw; dom.nn = nn; dom.B = B; dom.proof_status = dstat2; dom.status = dstat;
    hipLaunchKernelGGL(k_sigma_domain_check, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, dom);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_sigma_domain_check launch"; }
  }
  const uint32_t F = ZKP_F_DEVICE_PTRS;
  if (!st) {
    switch (proof_kind) {
      case W_DOC_ZERO_PROOF: st = zkp_zero_proof_verify_batch(c, n_bits, B, S[0], kw, S[1], P[0], P[1], dv, F); break;
      case W_DOC_CT_PROOF: st = zkp_ciphertext_proof_verify_batch(c, n_bits, B, S[0], kw, S[1], P[0], P[1], P[2], dv, F); break;
      case W_DOC_VERLIN_PROOF: st = zkp_verlin_proof_verify_batch(c, n_bits, B, S[0], kw, S[1], S[2], S[3], P[0], P[1], P[2], P[3], P[4], dv, F); break;
      default: st = zkp_mul_proof_verify_batch(c, n_bits, B, S[0], kw, S[1], S[2], S[3], P[0], P[1], P[2], P[3], P[4], dv, F); break;
    }
  }
  return verify_end(c, s, st, dstat, dv, B);
} ZKP_CATCH(c)
