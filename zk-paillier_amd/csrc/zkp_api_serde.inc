// zkp_api_serde.inc — wire-format ingestion (SURVEY §8(f) rank 3); included by zkp_api.hip.
// Host: tokenise serde_json documents of the reference's proof types (threads, one document at a time) into lists of
// (text offset, length, destination) per big integer.  GPU: k_dec2bin converts every decimal string straight into the
// SoA limb arrays of the batch.

#include <thread>

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
  const int32_t fin = s.finish();
  return st ? st : fin;
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
  const int32_t fin = s.finish();
  return st ? st : fin;
} ZKP_CATCH(c)

// ---- a JSON reader for the three document shapes, as tolerant as serde_json + the derived Deserialize impls are:
// object fields in any order, unknown fields skipped (whatever their value), white space anywhere, strings with escapes
// (\uXXXX included: serde_json hands the decoded text to the bigint visitors, serialize.rs:24-27,62-66); duplicate or
// missing fields, more than one variant key in a Response, and wrong value types are errors, as they are for serde.
namespace {
constexpr uint64_t EXTRA_FLAG = 1ull << 63;     // text_off of a string that had escapes: offset into the thread's decoded-copy buffer

struct JCur {
  const char* t; uint64_t p, end; bool ok = true;
  std::string* extra = nullptr;                 // decoded copies of value strings that contain escapes (per thread)
  void ws() { while (p < end && (t[p] == ' ' || t[p] == '\n' || t[p] == '\t' || t[p] == '\r')) p++; }
  bool eat(char ch) { ws(); if (p < end && t[p] == ch) { p++; return true; } return false; }
  bool expect(char ch) { if (!eat(ch)) ok = false; return ok; }
  // raw string token: content span and whether it holds a backslash
  bool raw_str(uint64_t* off, uint32_t* len, bool* esc) {
    ws();
    if (p >= end || t[p] != '"') return ok = false;
    const uint64_t b = ++p;
    *esc = false;
    while (p < end && t[p] != '"') {
      if ((unsigned char)t[p] < 0x20) return ok = false;           // control characters must be escaped
      if (t[p] == '\\') { *esc = true; p++; if (p >= end) return ok = false; }
      p++;
    }
    if (p >= end) return ok = false;
    *off = b; *len = (uint32_t)(p - b); p++;
    return true;
  }
  static int hexv(char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; }
  bool decode(uint64_t off, uint32_t len, std::string* out) {
    for (uint64_t i = off; i < off + len; i++) {
      if (t[i] != '\\') { out->push_back(t[i]); continue; }
      const char e = t[++i];
      switch (e) {
        case '"': out->push_back('"'); break;   case '\\': out->push_back('\\'); break;   case '/': out->push_back('/'); break;
        case 'b': out->push_back('\b'); break;  case 'f': out->push_back('\f'); break;    case 'n': out->push_back('\n'); break;
        case 'r': out->push_back('\r'); break;  case 't': out->push_back('\t'); break;
        case 'u': {
          if (i + 4 >= off + len) return ok = false;
          int v = 0;
          for (int k = 1; k <= 4; k++) { const int h = hexv(t[i + k]); if (h < 0) return ok = false; v = v * 16 + h; }
          i += 4;
          if (v >= 0xD800 && v <= 0xDFFF) return ok = false;        // surrogates: never part of a number or a field name here
          if (v < 0x80) out->push_back((char)v);
          else if (v < 0x800) { out->push_back((char)(0xC0 | (v >> 6))); out->push_back((char)(0x80 | (v & 63))); }
          else { out->push_back((char)(0xE0 | (v >> 12))); out->push_back((char)(0x80 | ((v >> 6) & 63))); out->push_back((char)(0x80 | (v & 63))); }
          break;
        }
        default: return ok = false;
      }
    }
    return true;
  }
  // a string VALUE to be converted on the GPU: (text offset, length); strings with escapes are decoded into *extra
  bool str(uint64_t* off, uint32_t* len) {
    uint64_t o; uint32_t l; bool esc;
    if (!raw_str(&o, &l, &esc)) return false;
    if (!esc) { *off = o; *len = l; return true; }
    const size_t at = extra->size();
    if (!decode(o, l, extra)) return false;
    *off = EXTRA_FLAG | at; *len = (uint32_t)(extra->size() - at);
    return true;
  }
  bool name(std::string* out) {                  // a field name, decoded
    uint64_t o; uint32_t l; bool esc;
    out->clear();
    if (!raw_str(&o, &l, &esc)) return false;
    if (esc) return decode(o, l, out);
    out->assign(t + o, l);
    return true;
  }
  bool uint(uint64_t* v) {
    ws();
    if (p >= end || t[p] < '0' || t[p] > '9') return ok = false;
    if (t[p] == '0' && p + 1 < end && t[p + 1] >= '0' && t[p + 1] <= '9') return ok = false;    // JSON has no leading zeros
    uint64_t x = 0; int nd = 0;
    while (p < end && t[p] >= '0' && t[p] <= '9') { x = x * 10 + (uint64_t)(t[p] - '0'); p++; if (++nd > 18) return ok = false; }
    if (p < end && (t[p] == '.' || t[p] == 'e' || t[p] == 'E')) return ok = false;                // not an integer
    *v = x;
    return true;
  }
  // any JSON value, skipped (the value of an unknown field)
  bool skip_value(int depth = 0) {
    if (depth > 64) return ok = false;
    ws();
    if (p >= end) return ok = false;
    const char ch = t[p];
    if (ch == '"') { uint64_t o; uint32_t l; bool e; return raw_str(&o, &l, &e); }
    if (ch == '{' || ch == '[') {
      const char close = ch == '{' ? '}' : ']';
      p++;
      if (eat(close)) return true;
      do {
        if (ch == '{') { uint64_t o; uint32_t l; bool e; if (!raw_str(&o, &l, &e) || !expect(':')) return false; }
        if (!skip_value(depth + 1)) return false;
      } while (eat(','));
      return expect(close);
    }
    auto lit = [&](const char* w) { const size_t n = strlen(w); if (p + n <= end && memcmp(t + p, w, n) == 0) { p += n; return true; } return false; };
    if (lit("true") || lit("false") || lit("null")) return true;
    if (ch == '-' || (ch >= '0' && ch <= '9')) {
      if (ch == '-') p++;
      const uint64_t b0 = p;
      while (p < end && ((t[p] >= '0' && t[p] <= '9') || t[p] == '.' || t[p] == 'e' || t[p] == 'E' || t[p] == '+' || t[p] == '-')) p++;
      return p > b0 ? true : (ok = false);
    }
    return ok = false;
  }
  // {"name": value, ...}: f(name) consumes the value and returns true, or returns false for a field it does not know (skipped)
  template <class F> bool object(F f) {
    if (!expect('{')) return false;
    if (eat('}')) return ok;
    std::string nm;
    do {
      if (!name(&nm) || !expect(':')) return false;
      if (!f(nm)) { if (!ok || !skip_value()) return ok = false; }
    } while (ok && eat(','));
    return expect('}');
  }
  bool done() { ws(); return ok && p == end; }
};

struct ItemList { std::vector<zkp_dec_item> items; std::vector<uint32_t> doc; };

// per-thread document loop
template <class F> void for_docs(uint64_t B, F f) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::max(1u, std::min(nt, 16u));
  if (B < 64) nt = 1;
  std::vector<std::thread> th;
  for (unsigned k = 0; k < nt; k++) th.emplace_back([=]() { for (uint64_t b = B * k / nt; b < B * (k + 1) / nt; b++) f(b, k); });
  for (auto& t : th) t.join();
}

// upload the text span covered by the documents; returns device pointer biased so that absolute offsets work
// The decoded copies of strings that had escapes (one buffer per parser thread) follow the span on the device: thread k's
// buffer starts at text offset extra_base[k].
struct TextSpan { char* d = nullptr; uint64_t lo = 0, hi = 0; std::vector<uint64_t> extra_base; };
int32_t upload_text(zkp_ctx* c, const char* text, const uint64_t* off, const uint64_t* len, uint64_t B, const std::vector<std::string>& extras, TextSpan* o) {
  uint64_t lo = ~0ull, hi = 0;
  for (uint64_t b = 0; b < B; b++) { lo = std::min(lo, off[b]); hi = std::max(hi, off[b] + len[b]); }
  o->lo = lo; o->hi = hi;
  uint64_t extra_total = 0;
  for (auto& e : extras) { o->extra_base.push_back(hi + extra_total); extra_total += e.size(); }
  HIPCHK(c, hipMalloc((void**)&o->d, std::max<uint64_t>(hi - lo + extra_total, 16)));
  HIPCHK(c, hipMemcpyAsync(o->d, text + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
  for (size_t k = 0; k < extras.size(); k++)
    if (!extras[k].empty()) HIPCHK(c, hipMemcpyAsync(o->d + (o->extra_base[k] - lo), extras[k].data(), extras[k].size(), hipMemcpyHostToDevice, c->stream));
  return ZKP_OK;
}

// pass 0: a number the fixed width cannot carry (negative, too wide) sends its document to the caller's host path; pass 1 (a later
// launch on the same stream, so it always wins): a string that is no integer at all is a serde error
__global__ void k_mark_docs(const uint8_t* __restrict__ item_status, const uint32_t* __restrict__ item_doc, uint64_t count, uint8_t* __restrict__ doc_status, int pass) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const uint8_t st = item_status[i];
  if (pass == 0 && (st == ZKP_DEC_NEGATIVE || st == ZKP_DEC_OVERFLOW) && doc_status[item_doc[i]] == ZKP_DOC_OK) doc_status[item_doc[i]] = ZKP_DOC_HOST_PATH;
  if (pass == 1 && st == ZKP_DEC_INVALID) doc_status[item_doc[i]] = ZKP_DOC_INVALID;
}

// "Its rows here are zero": whatever was converted of a document that ends up ZKP_DOC_INVALID or ZKP_DOC_HOST_PATH is cleared again, so
// that a caller who ignores the status never verifies a half-read proof
template <class T> __global__ void k_clear_failed_docs(const uint8_t* __restrict__ doc_status, T* __restrict__ dst, uint64_t units_per_doc, uint64_t docs) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < docs * units_per_doc && doc_status[i / units_per_doc] != ZKP_DOC_OK) dst[i] = 0;
}
template <class T> static void clear_failed_docs(zkp_ctx* c, const uint8_t* dstat, T* dst, uint64_t units_per_doc, uint64_t docs) {
  const uint64_t total = docs * units_per_doc;
  if (total) hipLaunchKernelGGL(k_clear_failed_docs<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, dstat, dst, units_per_doc, docs);
}

// convert one target array's item lists (one per thread) on the GPU and fold the item statuses into the documents'
int32_t convert_lists(zkp_ctx* c, const TextSpan& ts, std::vector<ItemList>& lists, uint32_t* dst, uint32_t max_words, uint8_t* d_doc_status,
                      std::vector<void*>& to_free) {
  size_t total = 0;
  for (auto& l : lists) total += l.items.size();
  if (total == 0) return ZKP_OK;
  std::vector<zkp_dec_item> items; items.reserve(total);
  std::vector<uint32_t> doc; doc.reserve(total);
  for (size_t k = 0; k < lists.size(); k++) {
    for (auto it : lists[k].items) {
      if (it.text_off & EXTRA_FLAG) it.text_off = ts.extra_base[k] + (it.text_off & ~EXTRA_FLAG);
      it.text_off -= ts.lo;
      items.push_back(it);
    }
    doc.insert(doc.end(), lists[k].doc.begin(), lists[k].doc.end());
  }
  zkp_dec_item* di = nullptr; uint32_t* dd = nullptr; uint8_t* dst_status = nullptr;
  HIPCHK(c, hipMalloc((void**)&di, total * sizeof(zkp_dec_item))); to_free.push_back(di);
  HIPCHK(c, hipMalloc((void**)&dd, total * 4)); to_free.push_back(dd);
  HIPCHK(c, hipMalloc((void**)&dst_status, total)); to_free.push_back(dst_status);
  HIPCHK(c, hipMemcpyAsync(di, items.data(), total * sizeof(zkp_dec_item), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dd, doc.data(), total * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the host vectors go out of scope
  int32_t st = launch_dec2bin(c, ts.d, di, total, dst, dst_status, max_words);
  if (st) return st;
  for (int pass = 0; pass < 2; pass++)
    hipLaunchKernelGGL(k_mark_docs, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, dst_status, dd, total, d_doc_status, pass);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}
}  // namespace

// With ZKP_F_DEVICE_PTRS every reader goes through the device scanner (json_scan, further down): the text is uploaded once and tokenised
// there, and only the documents it leaves come back to the reader's flags-0 path, as a sub-batch.
namespace {
// the text of a call that scans twice (zkp_dlog_verify_json_batch), uploaded by the caller: byte `a` of the caller's text is d[a - lo], and
// 16 bytes '0' follow the span
struct ScanText { char* d; uint64_t lo, span; };
int32_t json_scan(zkp_ctx* c, Stage& s, const char* name, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t forms,
                  const zkp_range_ni_proofs& d, uint32_t* sigma, uint8_t* dstat, uint32_t y_bits = 0, const ScanText* pre = nullptr, uint32_t* const* head_dst = nullptr);
int32_t json_scan_entry(zkp_ctx* c, const char* name, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t forms,
                        const zkp_range_ni_proofs& d, uint32_t* sigma, uint8_t* out_status, uint32_t y_bits = 0, uint32_t* const* head_dst = nullptr) {
  Stage s(c, ZKP_F_DEVICE_PTRS);
  int32_t st = json_scan(c, s, name, doc_kind, text, doc_off, doc_len, forms, d, sigma, out_status, y_bits, nullptr, head_dst);
  if (st && !s.st) s.st = st;
  const int32_t fin = s.finish();
  if (hipStreamSynchronize(c->stream) != hipSuccess && !st) { st = ZKP_EDEVICE; c->err = "stream sync"; }
  return st ? st : fin;
}
}  // namespace

// kind: 0 = EncryptedPairs -> c1, c2; 1 = Proof -> resp_*
static int32_t json_range_entry(zkp_ctx* c, const char* name, int kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len,
                                const zkp_range_ni_proofs* p, uint8_t* out_status, uint32_t flags) {
  if (!c) return ZKP_EINVAL;
  if (!p || p->batch == 0) return ZKP_OK;
  const uint64_t B = p->batch, EF = p->error_factor;
  const uint32_t kw = p->n_bits / 32;
  if (!text || !doc_off || !doc_len || !out_status || (p->n_bits != 1024 && p->n_bits != 2048 && p->n_bits != 4096) || EF == 0 || EF > 256 || B > (1ull << 24) ||
      (kind == 0 && (!p->c1 || !p->c2)) || (kind == 1 && (!p->resp_kind || !p->resp_j || !p->resp_w1 || !p->resp_r1 || !p->resp_w2 || !p->resp_r2))) {
    c->err = std::string(name) + ": invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (flags & ZKP_F_DEVICE_PTRS) return json_scan_entry(c, name, kind == 0 ? W_DOC_PAIRS : W_DOC_PROOF, text, doc_off, doc_len, 0, *p, nullptr, out_status);
  const uint64_t rows = B * EF;
  std::vector<uint8_t> status(B, 0), kinds, js;
  if (kind == 1) { kinds.assign(rows, 0); js.assign(rows, 0); }
  const unsigned NT = 16;
  std::vector<ItemList> L[4];
  for (auto& l : L) l.resize(NT);
  std::vector<std::string> extras(NT);
  for_docs(B, [&](uint64_t b, unsigned k) {
    JCur j{text, doc_off[b], doc_off[b] + doc_len[b]};
    j.extra = &extras[k];
    const size_t extra_mark = extras[k].size();
    bool other_count = false;       // a well-formed document with another number of rows: a valid value of the reference's type, outside this batch layout
    auto push = [&](int which, uint64_t row, uint32_t words) {
      uint64_t o; uint32_t l;
      if (!j.str(&o, &l)) return;
      L[which][k].items.push_back({o, row * words, l, words});
      L[which][k].doc.push_back((uint32_t)b);
    };
    const size_t mark[4] = {L[0][k].items.size(), L[1][k].items.size(), L[2][k].items.size(), L[3][k].items.size()};
    auto skip_str = [&]() { uint64_t o; uint32_t l; bool e; j.raw_str(&o, &l, &e); };
    if (kind == 0) {
      // {"c1":[...],"c2":[...]}  (range_proof.rs:32-39), fields in any order
      bool seen[2] = {false, false};
      j.object([&](const std::string& nm) {
        const int which = nm == "c1" ? 0 : nm == "c2" ? 1 : -1;
        if (which < 0) return false;
        if (seen[which]) { j.ok = false; return true; }                    // duplicate field
        seen[which] = true;
        j.expect('[');
        uint64_t cnt = 0;
        if (j.ok && !j.eat(']')) {
          do { if (cnt < EF) push(which, b * EF + cnt, 2 * kw); else skip_str(); cnt++; } while (j.ok && j.eat(','));
          j.expect(']');
        }
        if (cnt != EF) other_count = true;
        return true;
      });
      if (!seen[0] || !seen[1]) j.ok = false;                               // missing field
    } else {
      // [{"Open":{"w1":..,"r1":..,"w2":..,"r2":..}},{"Mask":{"j":1,"masked_x":..,"masked_r":..}},...]  (range_proof.rs:53-81):
      // externally tagged enum = an object with exactly one key, the variant name
      j.expect('[');
      uint64_t cnt = 0;
      if (j.ok && !j.eat(']')) {
        do {
          const uint64_t row = b * EF + (cnt < EF ? cnt : EF - 1);
          int variants = 0;
          j.object([&](const std::string& vn) {
            if (++variants > 1) { j.ok = false; return true; }
            if (vn == "Open") {
              static const char* names[4] = {"w1", "r1", "w2", "r2"};
              unsigned seen = 0;
              j.object([&](const std::string& nm) {
                int f = -1;
                for (int q = 0; q < 4; q++) if (nm == names[q]) f = q;
                if (f < 0) return false;
                if (seen & (1u << f)) { j.ok = false; return true; }
                seen |= 1u << f;
                if (cnt < EF) push(f, row, kw); else skip_str();
                return true;
              });
              if (seen != 15u) j.ok = false;
              if (cnt < EF) { kinds[row] = ZKP_RESP_OPEN; js[row] = 0; }
            } else if (vn == "Mask") {
              uint64_t jv = 0;
              unsigned seen = 0;
              j.object([&](const std::string& nm) {
                const int f = nm == "j" ? 0 : nm == "masked_x" ? 1 : nm == "masked_r" ? 2 : -1;
                if (f < 0) return false;
                if (seen & (1u << f)) { j.ok = false; return true; }
                seen |= 1u << f;
                if (f == 0) { j.uint(&jv); if (jv > 255) j.ok = false; }
                else if (cnt < EF) push(f - 1, row, kw);
                else skip_str();
                return true;
              });
              if (seen != 7u) j.ok = false;
              if (cnt < EF) { kinds[row] = ZKP_RESP_MASK; js[row] = (uint8_t)jv; }
            } else {
              j.ok = false;                                                 // unknown variant
            }
            return true;
          });
          if (variants != 1) j.ok = false;
          cnt++;
        } while (j.ok && j.eat(','));
        j.expect(']');
      }
      if (cnt != EF) other_count = true;
    }
    if (!j.done() || other_count) {
      status[b] = !j.done() ? ZKP_DOC_INVALID : ZKP_DOC_HOST_PATH;
      for (int q = 0; q < 4; q++) { L[q][k].items.resize(mark[q]); L[q][k].doc.resize(mark[q]); }   // nothing of a malformed document is converted
      extras[k].resize(extra_mark);
      if (kind == 1) for (uint64_t i = 0; i < EF; i++) { kinds[b * EF + i] = 0; js[b * EF + i] = 0; }
    }
  });
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint32_t* tgt[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t *dkind = nullptr, *dj = nullptr;
  if (kind == 0) { tgt[0] = s.out(p->c1, rows * 2 * kw); tgt[1] = s.out(p->c2, rows * 2 * kw); }
  else {
    tgt[0] = s.out(p->resp_w1, rows * kw); tgt[1] = s.out(p->resp_r1, rows * kw); tgt[2] = s.out(p->resp_w2, rows * kw); tgt[3] = s.out(p->resp_r2, rows * kw);
    dkind = s.out(p->resp_kind, rows); dj = s.out(p->resp_j, rows);
  }
  int32_t st = s.st;
  TextSpan ts;
  std::vector<void*> to_free;
  if (!st) st = upload_text(c, text, doc_off, doc_len, B, extras, &ts);
  if (!st) {
    const uint32_t words = kind == 0 ? 2 * kw : kw;
    const int ntgt = kind == 0 ? 2 : 4;
    for (int q = 0; q < ntgt && !st; q++) if (hipMemsetAsync(tgt[q], 0, rows * words * 4, c->stream) != hipSuccess) { st = ZKP_EDEVICE; c->err = "memset"; }
    if (!st && hipMemcpyAsync(dstat, status.data(), B, hipMemcpyHostToDevice, c->stream) != hipSuccess) { st = ZKP_EDEVICE; c->err = "H2D status"; }
    if (!st && kind == 1) {
      if (hipMemcpyAsync(dkind, kinds.data(), rows, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
          hipMemcpyAsync(dj, js.data(), rows, hipMemcpyHostToDevice, c->stream) != hipSuccess) { st = ZKP_EDEVICE; c->err = "H2D kinds"; }
    }
    for (int q = 0; q < ntgt && !st; q++) st = convert_lists(c, ts, L[q], tgt[q], words, dstat, to_free);
    if (!st) {
      for (int q = 0; q < ntgt; q++) clear_failed_docs(c, dstat, tgt[q], EF * words, B);
      if (kind == 1) { clear_failed_docs(c, dstat, dkind, EF, B); clear_failed_docs(c, dstat, dj, EF, B); }
      if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_clear_failed_docs"; }
    }
  }
  const int32_t fin = s.finish();
  (void)hipStreamSynchronize(c->stream);
  if (ts.d) (void)hipFree(ts.d);
  for (void* q : to_free) (void)hipFree(q);
  return st ? st : fin;
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
  if (!text || !doc_off || !doc_len || !out_sigma || !out_status || (n_bits != 1024 && n_bits != 2048 && n_bits != 4096) || B > (1ull << 24)) {
    c->err = "zkp_json_correct_key_proof_batch: invalid argument"; return ZKP_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (flags & ZKP_F_DEVICE_PTRS) {
    zkp_range_ni_proofs d{};
    d.n_bits = n_bits; d.batch = B;
    return json_scan_entry(c, "zkp_json_correct_key_proof_batch", W_DOC_CK, text, doc_off, doc_len, 0, d, out_sigma, out_status);
  }
  const uint32_t kw = n_bits / 32;
  const uint64_t M2 = ZKP_CORRECT_KEY_M2;
  std::vector<uint8_t> status(B, 0);
  const unsigned NT = 16;
  std::vector<ItemList> L(NT);
  std::vector<std::string> extras(NT);
  for_docs(B, [&](uint64_t b, unsigned k) {
    JCur j{text, doc_off[b], doc_off[b] + doc_len[b]};
    const size_t mark = L[k].items.size();
    // {"sigma_vec":[...]}  (correct_key_ni.rs:35-39); a vector of another length is a valid NiCorrectKeyProof whose verify() panics
    // or ignores the tail (sigma_vec[i], :90): outside the fixed layout -> malformed here
    j.extra = &extras[k];
    const size_t extra_mark = extras[k].size();
    bool seen = false;
    uint64_t cnt = 0;
    j.object([&](const std::string& nm) {
      if (nm != "sigma_vec") return false;
      if (seen) { j.ok = false; return true; }
      seen = true;
      j.expect('[');
      if (j.ok && !j.eat(']')) {
        do {
          uint64_t o; uint32_t l;
          if (j.str(&o, &l) && cnt < M2) { L[k].items.push_back({o, (b * M2 + cnt) * kw, l, kw}); L[k].doc.push_back((uint32_t)b); }
          cnt++;
        } while (j.ok && j.eat(','));
        j.expect(']');
      }
      return true;
    });
    if (!seen || cnt != M2) j.ok = false;
    if (!j.ok) extras[k].resize(extra_mark);
    if (!j.done()) { status[b] = ZKP_VERDICT_MALFORMED; L[k].items.resize(mark); L[k].doc.resize(mark); }
  });
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint32_t* dsig = s.out(out_sigma, B * M2 * kw);
  int32_t st = s.st;
  TextSpan ts;
  std::vector<void*> to_free;
  if (!st) st = upload_text(c, text, doc_off, doc_len, B, extras, &ts);
  if (!st) {
    if (hipMemsetAsync(dsig, 0, B * M2 * kw * 4, c->stream) != hipSuccess || hipMemcpyAsync(dstat, status.data(), B, hipMemcpyHostToDevice, c->stream) != hipSuccess) { st = ZKP_EDEVICE; c->err = "H2D"; }
    if (!st) st = convert_lists(c, ts, L, dsig, kw, dstat, to_free);
  }
  const int32_t fin = s.finish();
  (void)hipStreamSynchronize(c->stream);
  if (ts.d) (void)hipFree(ts.d);
  for (void* q : to_free) (void)hipFree(q);
  return st ? st : fin;
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
namespace {
// -> 0 converted; ZKP_DOC_HOST_PATH: an integer this width cannot carry (negative or too wide; the token is consumed, dst is zero);
// ZKP_DOC_INVALID: not an integer of this text form (j.ok = false)
int parse_bigint_value(JCur& j, uint32_t enc, uint32_t* dst, uint32_t words) {
  memset(dst, 0, (size_t)words * 4);
  auto invalid = [&]() { j.ok = false; return (int)ZKP_DOC_INVALID; };
  auto unrepresentable = [&]() { memset(dst, 0, (size_t)words * 4); return (int)ZKP_DOC_HOST_PATH; };
  if (enc == ZKP_BIGINT_BYTES) {
    std::vector<uint8_t> bytes;
    if (!j.expect('[')) return invalid();
    if (!j.eat(']')) {
      do { uint64_t v; if (!j.uint(&v) || v > 255) return invalid(); bytes.push_back((uint8_t)v); } while (j.eat(','));
      if (!j.expect(']')) return invalid();
    }
    size_t lead = 0;
    while (lead < bytes.size() && bytes[lead] == 0) lead++;
    if (bytes.size() - lead > (size_t)words * 4) return unrepresentable();
    for (size_t i = lead; i < bytes.size(); i++) { const size_t pos = bytes.size() - 1 - i; dst[pos / 4] |= (uint32_t)bytes[i] << (8 * (pos % 4)); }
    return 0;
  }
  uint64_t off; uint32_t len; bool esc;
  if (!j.raw_str(&off, &len, &esc) || esc || len == 0) return invalid();
  const char* t = j.t + off;
  const bool minus = t[0] == '-';
  if (minus) { t++; len--; if (len == 0) return invalid(); }
  bool nonzero = false, too_wide = false;
  if (enc == ZKP_BIGINT_HEX) {
    uint32_t lead = 0;
    while (lead + 1 < len && t[lead] == '0') lead++;
    for (uint32_t i = lead; i < len; i++) {
      const int h = JCur::hexv(t[i]);
      if (h < 0) return invalid();
      nonzero |= h != 0;
      const uint32_t pos = len - 1 - i;
      if (pos / 8 >= words) { too_wide |= h != 0; continue; }
      dst[pos / 8] |= (uint32_t)h << (4 * (pos % 8));
    }
  } else {
    // decimal: 9 digits at a time, x = x * 10^9 + chunk (BigInt::from_str_radix accepts leading zeros)
    uint32_t used = 0;
    for (uint32_t i = 0; i < len;) {
      const uint32_t take = std::min<uint32_t>(9, len - i);
      uint64_t chunk = 0, mul = 1;
      for (uint32_t k = 0; k < take; k++) { const char ch = t[i + k]; if (ch < '0' || ch > '9') return invalid(); chunk = chunk * 10 + (uint64_t)(ch - '0'); mul *= 10; }
      nonzero |= chunk != 0;
      if (!too_wide) {
        uint64_t carry = chunk;
        for (uint32_t w = 0; w < used; w++) { const uint64_t v = (uint64_t)dst[w] * mul + carry; dst[w] = (uint32_t)v; carry = v >> 32; }
        while (carry) { if (used == words) { too_wide = true; break; } dst[used++] = (uint32_t)carry; carry >>= 32; }
      }
      i += take;
    }
  }
  if (too_wide || (minus && nonzero)) return unrepresentable();
  return 0;
}
}  // namespace

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
  hipLaunchKernelGGL(k_scan_merge<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, src, dst, units_per_doc, didx, docs);
  HIPCHK(c, hipGetLastError());
  return ZKP_OK;
}

// One batch of documents of one kind (W_DOC_*) into device memory.  d: the arrays of the kind (RangeProofNi: every one; EncryptedPairs: c1, c2;
// Proof: resp_*; NiCorrectKeyProof: none of them — `sigma` [B][11][kw] instead, with d.n_bits and d.batch); d.n is the verifier's key when
// d.n_stride == 0 (an input), else it receives the documents' keys.
// Statuses and arrays are what the kind's reader gives with flags == 0 on host arrays, byte for byte:
//   - a scanned document has no malformed number and no sign, so the only status left is k_dec2bin's overflow (ZKP_DOC_HOST_PATH);
//   - RangeProofNi: the head is converted and marked first, then compared with the verifier's key (ZKP_DOC_INVALID, as the host reader
//     decides before it looks at the rows), then the rows: k_mark_docs only ever turns ZKP_DOC_OK into ZKP_DOC_HOST_PATH;
//   - what was converted of a document that ends up unconverted is cleared where the host reader clears it: everywhere but in sigma.
int32_t json_heads_host(const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t doc_kind, uint32_t key_form, uint32_t bare_form, uint32_t kw,
                        uint32_t yw, uint32_t* const* out, uint8_t* out_status);
void scan_span(const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint64_t* lo, uint64_t* hi) {
  for (uint64_t b = 0; b < B; b++) if (doc_len[b]) { *lo = std::min(*lo, doc_off[b]); *hi = std::max(*hi, doc_off[b] + doc_len[b]); }
}
int32_t scan_upload(zkp_ctx* c, Stage& s, const char* text, uint64_t lo, uint64_t hi, ScanText* o) {
  if (hi == 0) lo = 0;
  o->lo = lo; o->span = hi - lo;
  o->d = (char*)s.take(o->span + 16);
  if (s.st) return s.st;
  if (o->span) HIPCHK(c, hipMemcpyAsync(o->d, text + lo, o->span, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(o->d + o->span, '0', 16, c->stream));
  return ZKP_OK;
}
// The heads-only kinds: head_dst[i] is the destination of head i of w_doc_spec(doc_kind) (the two DLog kinds may name N, g, ni / x, y as d.n, d.range,
// d.ciphertext instead; y: y_bits / 32 words), d.n_stride = kw, forms is ZKP_BIGINT_FORMS(key, bare) (the DLog kinds have no key: the bare form
// alone), and nothing is cleared afterwards: as with sigma, an over-wide field is zero and the others stay converted.
// pre: the text is already on the device (the caller also keeps the diagnostics: events and counters of BOTH scans of its call).
int32_t json_scan(zkp_ctx* c, Stage& s, const char* name, uint32_t doc_kind, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint32_t forms,
                  const zkp_range_ni_proofs& d, uint32_t* sigma, uint8_t* dstat, uint32_t y_bits, const ScanText* pre, uint32_t* const* head_dst) {
  const bool ni = doc_kind == W_DOC_NI, ck = doc_kind == W_DOC_CK, has_pairs = ni || doc_kind == W_DOC_PAIRS, has_rows = ni || doc_kind == W_DOC_PROOF;
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const bool dl = spec.heads_only, heads = spec.n_heads != 0;
  const uint64_t B = d.batch, EF = ck ? ZKP_CORRECT_KEY_M2 : dl ? 0 : d.error_factor, rows = B * EF;
  const uint32_t kw = d.n_bits / 32, yw = y_bits / 32;
  const uint32_t key_form = (forms >> 4) & 15u, bare_form = forms & 15u;
  const bool per_key = d.n_stride != 0;
  int32_t st = ZKP_OK;
  ScanText up{};
  if (pre) up = *pre;
  else {
    c->scan_fast = c->scan_fallback = 0; c->scan_phases = 0;
    if ((st = scan_event(c, 0))) return st;
    uint64_t lo = ~0ull, hi = 0;
    scan_span(doc_off, doc_len, B, &lo, &hi);
    if ((st = scan_upload(c, s, text, lo, hi, &up))) return st;
  }
  const uint64_t lo = up.lo, span = up.span;
  ScanJob J{};
  char* dtext = up.d;
  J.doc_off = s.host_in(doc_off, B); J.doc_len = s.host_in(doc_len, B);
  J.text = dtext; J.lo = lo; J.B = B; J.zero_at = span;
  J.max_len = zkp_json_doc_bound(doc_kind, d.n_bits, d.error_factor, forms);
  J.doc_kind = doc_kind; J.ef = (uint32_t)EF; J.kw = kw; J.key_form = key_form; J.bare_form = bare_form;
  J.dig_n = zkp_decimal_pitch(kw) - 1; J.dig_c = zkp_decimal_pitch(2 * kw) - 1;      // (max_digits below)
  // the heads: the table's rows with this batch's widths, forms and destinations
  uint32_t* const legacy_dst[3] = {heads ? (per_key ? const_cast<uint32_t*>(d.n) : (uint32_t*)s.take(B * kw * 4)) : nullptr, const_cast<uint32_t*>(d.range),
                                   const_cast<uint32_t*>(d.ciphertext)};
  if (!head_dst) head_dst = legacy_dst;
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
  if (ck) targets.push_back({W_ARR_W1, sigma, kw});
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
  if (!pre && (st = scan_event(c, 1))) return st;
  hipLaunchKernelGGL(k_json_scan, dim3((unsigned)B), dim3(64), 0, c->stream, J);
  HIPCHK(c, hipGetLastError());
  if (!pre && (st = scan_event(c, 2))) return st;
  auto convert = [&](const Target& t) -> int32_t {
    if (!J.items[t.arr]) return ZKP_OK;                      // a head integer in hex / byte-array form: the scanner wrote its limbs
    const bool head = t.arr < W_ARR_C1;
    const uint64_t count = head ? B : rows;
    const int32_t e = launch_dec2bin(c, dtext, J.items[t.arr], count, t.dst, item_status, t.words);
    if (e) return e;
    hipLaunchKernelGGL(k_mark_docs, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, item_status, head ? J.head_doc : J.row_doc, count, dstat, 0);
    HIPCHK(c, hipGetLastError());
    return ZKP_OK;
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
  return pre ? ZKP_OK : scan_event(c, 3);
}
bool json_ni_common_args_ok(const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t n_bits, uint32_t ef, uint32_t forms) {
  return text && doc_off && doc_len && B <= (1ull << 24) && (n_bits == 1024 || n_bits == 2048 || n_bits == 4096) && ef != 0 && ef <= 256 && !(forms >> 8) &&
         ((forms >> 4) & 15u) <= ZKP_BIGINT_BYTES && (forms & 15u) <= ZKP_BIGINT_BYTES;
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
  if (!st) st = json_scan(c, s, "zkp_range_ni_verify_json_batch", W_DOC_NI, text, doc_off, doc_len, bigint_forms, d, nullptr, dstat);
  // The whole batch is verified and the verdicts of the documents that were not converted are masked afterwards: their rows are zero, and
  // with verify_self so is their key, which the verify kernels answer with a verdict of that proof alone (never an error of the call).
  if (!st) st = zkp_range_ni_verify_batch(c, &d, dv, ZKP_F_DEVICE_PTRS);
  if (!st) {
    hipLaunchKernelGGL(k_scan_mask_verdicts, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)dstat, dv, B);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_scan_mask_verdicts launch"; }
  }
  if (!st) st = scan_event(c, 4);
  if (st && !s.st) s.st = st;
  const int32_t fin = s.finish();
  if (hipStreamSynchronize(c->stream) != hipSuccess && !st) { st = ZKP_EDEVICE; c->err = "stream sync"; }
  return st ? st : fin;
} ZKP_CATCH(c)

// NiCorrectKeyProof::verify on documents: the same three steps with sigma in a block the call owns.  An unread document leaves zero (or, where
// one number overflowed, partly converted) sigma rows: k_ck_check answers them with a verdict of that proof alone, masked afterwards.
extern "C" int32_t zkp_correct_key_ni_verify_json_batch(zkp_ctx* c, const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t n_bits,
                                                        const uint32_t* n, const uint8_t* salt, uint32_t salt_len, uint8_t* out_status, uint8_t* out_verdict,
                                                        uint32_t flags) try {
  if (!c) return ZKP_EINVAL;
  if (B == 0) return ZKP_OK;
  if ((flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || !text || !doc_off || !doc_len || !n || !out_status || !out_verdict || (salt_len && !salt) ||
      (n_bits != 1024 && n_bits != 2048 && n_bits != 4096) || B > (1ull << 24)) {
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
  d.n_bits = n_bits; d.batch = B;
  int32_t st = s.st;
  if (!st) st = json_scan(c, s, "zkp_correct_key_ni_verify_json_batch", W_DOC_CK, text, doc_off, doc_len, 0, d, dsig, dstat);
  if (!st) st = zkp_correct_key_ni_verify_batch(c, n_bits, B, dn, dsig, salt, salt_len, dv, ZKP_F_DEVICE_PTRS);
  if (!st) {
    hipLaunchKernelGGL(k_scan_mask_verdicts, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)dstat, dv, B);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_scan_mask_verdicts launch"; }
  }
  if (!st) st = scan_event(c, 4);
  if (st && !s.st) s.st = st;
  const int32_t fin = s.finish();
  if (hipStreamSynchronize(c->stream) != hipSuccess && !st) { st = ZKP_EDEVICE; c->err = "stream sync"; }
  return st ? st : fin;
} ZKP_CATCH(c)

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
  const uint32_t key_form = (bigint_forms >> 4) & 15u, bare_form = bigint_forms & 15u;
  if (flags != 0 || !text || !doc_off || !doc_len || !out_status || !p->n || !p->range || !p->ciphertext || key_form > ZKP_BIGINT_BYTES || bare_form > ZKP_BIGINT_BYTES ||
      (bigint_forms >> 8) || (p->n_stride != 0 && p->n_stride != kw) || (p->n_bits != 1024 && p->n_bits != 2048 && p->n_bits != 4096)) {
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
    JCur j{text, doc_off[b], doc_off[b] + doc_len[b]};
    std::string none;
    j.extra = &none;
    unsigned seen = 0;
    bool host = false;
    ep_off[b] = pr_off[b] = doc_off[b]; ep_len[b] = pr_len[b] = 0;
    auto once = [&](unsigned bit) { if (seen & bit) { j.ok = false; return false; } seen |= bit; return true; };
    j.object([&](const std::string& nm) {
      if (nm == "ek") {
        if (!once(1)) return true;
        bool has_n = false;
        j.object([&](const std::string& f) {
          if (f != "n") return false;
          if (has_n) { j.ok = false; return true; }
          has_n = true;
          host |= parse_bigint_value(j, key_form, &keys[b * kw], kw) == ZKP_DOC_HOST_PATH;
          return true;
        });
        if (!has_n) j.ok = false;
      } else if (nm == "range") { if (once(2)) host |= parse_bigint_value(j, bare_form, out_range + b * kw, kw) == ZKP_DOC_HOST_PATH; }
      else if (nm == "ciphertext") { if (once(4)) host |= parse_bigint_value(j, bare_form, out_ct + b * 2 * kw, 2 * kw) == ZKP_DOC_HOST_PATH; }
      else if (nm == "encrypted_pairs") { if (once(8)) { j.ws(); ep_off[b] = j.p; j.skip_value(); ep_len[b] = j.p - ep_off[b]; } }
      else if (nm == "proof") { if (once(16)) { j.ws(); pr_off[b] = j.p; j.skip_value(); pr_len[b] = j.p - pr_off[b]; } }
      else if (nm == "error_factor") { uint64_t ef = 0; if (once(32)) { j.uint(&ef); if (ef != p->error_factor) host = true; } }   // any usize is a valid RangeProofNi
      else return false;
      return true;
    });
    if (seen != 63u) j.ok = false;
    top[b] = !j.done() ? ZKP_DOC_INVALID : host ? ZKP_DOC_HOST_PATH : ZKP_DOC_OK;
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
    for (uint64_t b = 0; b < B; b++) if (!top[b] && memcmp(&keys[b * kw], p->n, (size_t)kw * 4) != 0) top[b] = ZKP_DOC_INVALID;
  }
  for (uint64_t b = 0; b < B; b++)
    if (top[b]) { memset(out_range + b * kw, 0, (size_t)kw * 4); memset(out_ct + b * 2 * kw, 0, (size_t)kw * 8); ep_off[b] = pr_off[b] = doc_off[b]; ep_len[b] = pr_len[b] = 0; }
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
  const uint32_t key_form = (bigint_forms >> 4) & 15u, bare_form = bigint_forms & 15u;
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const bool dl = spec.heads_only;
  if ((n_bits != 1024 && n_bits != 2048 && n_bits != 4096) || (doc_kind > ZKP_JSON_DOC_CORRECT_KEY_PROOF && !dl) || (bigint_forms >> 8) ||
      key_form > ZKP_BIGINT_BYTES || bare_form > ZKP_BIGINT_BYTES || (doc_kind != ZKP_JSON_DOC_CORRECT_KEY_PROOF && !dl && error_factor == 0))
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
  const uint32_t key_form = (forms >> 4) & 15u, bare_form = forms & 15u;
  const bool ck = doc_kind == W_DOC_CK, ni = doc_kind == W_DOC_NI, has_pairs = doc_kind == W_DOC_PAIRS || ni, has_proof = doc_kind == W_DOC_PROOF || ni;
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const bool dl = spec.heads_only;
  const uint32_t kw = n_bits / 32;
  bool bad = !out_doc_off || (flags & ~(uint32_t)ZKP_F_DEVICE_PTRS) || (n_bits != 1024 && n_bits != 2048 && n_bits != 4096) || B > (1ull << 24) ||
             (forms >> 8) || key_form > ZKP_BIGINT_BYTES || bare_form > ZKP_BIGINT_BYTES || (!ck && !dl && !p) || (!ck && !dl && (EF == 0 || EF > 256));
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
    const int32_t fin = s.finish();       // (the status bytes are still delivered; finish() returns the sticky status)
    (void)fin;
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
  if (st && !s.st) s.st = st;
  const int32_t fin = s.finish();
  if (hipStreamSynchronize(c->stream) != hipSuccess && !st) { st = ZKP_EDEVICE; c->err = "stream sync"; }
  return st ? st : fin;
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
// The flags-0 reader of every heads-only kind: the tolerant tokeniser, every number converted on the host (parse_bigint_value, as for the head
// of a RangeProofNi document).  The fields are the rows of w_doc_spec(doc_kind); a key row is the object "ek" with a field "n" (its other
// fields are skipped, as for a RangeProofNi).  out[i]: [B][words of field i].  An invalid document leaves zero rows; an over-wide or negative
// field is zero, the others converted.
int32_t json_heads_host(const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t doc_kind, uint32_t key_form, uint32_t bare_form, uint32_t kw,
                        uint32_t yw, uint32_t* const* out, uint8_t* out_status) {
  const WDocSpec& spec = w_doc_spec(doc_kind);
  const unsigned nf = spec.n_heads;
  uint32_t words[W_MAX_HEADS] = {};
  for (unsigned f = 0; f < nf; f++) words[f] = w_head_words(spec.h[f], kw, yw);
  for (unsigned f = 0; f < nf; f++) memset(out[f], 0, (size_t)B * words[f] * 4);
  for_docs(B, [&](uint64_t b, unsigned) {
    JCur j{text, doc_off[b], doc_off[b] + doc_len[b]};
    unsigned seen = 0;
    bool host = false;
    j.object([&](const std::string& nm) {
      int f = -1;
      for (unsigned q = 0; q < nf; q++) if (nm == spec.h[q].name) f = (int)q;
      if (f < 0) return false;
      if (seen & (1u << f)) { j.ok = false; return true; }                      // duplicate field
      seen |= 1u << f;
      if (!spec.h[f].key) { host |= parse_bigint_value(j, bare_form, out[f] + b * words[f], words[f]) == ZKP_DOC_HOST_PATH; return true; }
      bool has_n = false;
      j.object([&](const std::string& k) {
        if (k != "n") return false;
        if (has_n) { j.ok = false; return true; }
        has_n = true;
        host |= parse_bigint_value(j, key_form, out[f] + b * words[f], words[f]) == ZKP_DOC_HOST_PATH;
        return true;
      });
      if (!has_n) j.ok = false;
      return true;
    });
    if (seen != (1u << nf) - 1) j.ok = false;                                   // missing field
    const uint8_t st = !j.done() ? ZKP_DOC_INVALID : host ? ZKP_DOC_HOST_PATH : ZKP_DOC_OK;
    out_status[b] = st;
    if (st == ZKP_DOC_INVALID) for (unsigned f = 0; f < nf; f++) memset(out[f] + b * words[f], 0, (size_t)words[f] * 4);
  });
  return ZKP_OK;
}

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
  d.n_bits = n_bits; d.batch = B; d.n_stride = kw;
  d.n = out[0]; d.range = out[1]; d.ciphertext = out[2];
  return json_scan_entry(c, name, doc_kind, text, doc_off, doc_len, bare_form, d, nullptr, out_status, y_bits);
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
  const char* name = "zkp_dlog_verify_json_batch";
  Stage s(c, flags);
  uint8_t* dstat = s.out(out_status, B);
  uint8_t* dv = s.out(out_verdict, B);
  uint32_t* arr[4];
  for (auto& a : arr) a = (uint32_t*)s.take(B * kw * 4);
  uint32_t* dy = (uint32_t*)s.take(B * yw * 4);
  uint8_t* dstat2 = (uint8_t*)s.take(B);
  int32_t st = s.st;
  c->scan_fast = c->scan_fallback = 0; c->scan_phases = 0;
  if (!st) st = scan_event(c, 0);
  ScanText up{};
  if (!st) {
    uint64_t lo = ~0ull, hi = 0;
    scan_span(st_off, st_len, B, &lo, &hi);
    scan_span(pf_off, pf_len, B, &lo, &hi);
    st = scan_upload(c, s, text, lo, hi, &up);
  }
  if (!st) st = scan_event(c, 1);
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.batch = B; d.n_stride = kw;
  d.n = arr[0]; d.range = arr[1]; d.ciphertext = arr[2];
  if (!st) st = json_scan(c, s, name, W_DOC_DLOG_STATEMENT, text, st_off, st_len, bare_form, d, nullptr, dstat, y_bits, &up);
  if (!st) st = scan_event(c, 2);
  d.n = arr[3]; d.range = dy; d.ciphertext = nullptr;
  if (!st) st = json_scan(c, s, name, W_DOC_DLOG_PROOF, text, pf_off, pf_len, bare_form, d, nullptr, dstat2, y_bits, &up);
  if (!st) st = scan_event(c, 3);
  if (!st) {
    hipLaunchKernelGGL(k_dlog_domain_check, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, arr[0], arr[1], arr[2], arr[3], dy, (uint32_t)kw, (uint32_t)yw, B,
                       (const uint8_t*)dstat2, dstat);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_dlog_domain_check launch"; }
  }
  if (!st) st = zkp_dlog_verify_batch(c, n_bits, y_bits, B, arr[0], arr[1], arr[2], arr[3], dy, dv, ZKP_F_DEVICE_PTRS);
  if (!st) {
    hipLaunchKernelGGL(k_scan_mask_verdicts, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)dstat, dv, B);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_scan_mask_verdicts launch"; }
  }
  if (!st) st = scan_event(c, 4);
  if (st && !s.st) s.st = st;
  const int32_t fin = s.finish();
  if (hipStreamSynchronize(c->stream) != hipSuccess && !st) { st = ZKP_EDEVICE; c->err = "stream sync"; }
  return st ? st : fin;
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
  return w_sigma_kind(doc_kind) && (n_bits == 1024 || n_bits == 2048 || n_bits == 4096) && B <= (1ull << 24) && !(forms >> 8) && ((forms >> 4) & 15u) <= ZKP_BIGINT_BYTES &&
         (forms & 15u) <= ZKP_BIGINT_BYTES;
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
  if (!(flags & ZKP_F_DEVICE_PTRS)) return json_heads_host(text, doc_off, doc_len, B, doc_kind, (bigint_forms >> 4) & 15u, bigint_forms & 15u, kw, 0, o.f, out_status);
  HIPCHK(c, hipSetDevice(c->device));
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.batch = B; d.n_stride = kw;
  return json_scan_entry(c, "zkp_json_sigma_batch", doc_kind, text, doc_off, doc_len, bigint_forms, d, nullptr, out_status, 0, o.f);
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
  const char* name = "zkp_sigma_verify_json_batch";
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
  c->scan_fast = c->scan_fallback = 0; c->scan_phases = 0;
  if (!st) st = scan_event(c, 0);
  ScanText up{};
  if (!st) {
    uint64_t lo = ~0ull, hi = 0;
    scan_span(st_off, st_len, B, &lo, &hi);
    scan_span(pf_off, pf_len, B, &lo, &hi);
    st = scan_upload(c, s, text, lo, hi, &up);
  }
  if (!st) st = scan_event(c, 1);
  zkp_range_ni_proofs d{};
  d.n_bits = n_bits; d.batch = B; d.n_stride = kw;
  if (!st) st = json_scan(c, s, name, st_kind, text, st_off, st_len, bigint_forms, d, nullptr, dstat, 0, &up, S);
  if (!st) st = scan_event(c, 2);
  if (!st) st = json_scan(c, s, name, proof_kind, text, pf_off, pf_len, bigint_forms, d, nullptr, dstat2, 0, &up, P);
  if (!st) st = scan_event(c, 3);
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
  if (!st) {
    hipLaunchKernelGGL(k_scan_mask_verdicts, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)dstat, dv, B);
    if (hipGetLastError() != hipSuccess) { st = ZKP_EDEVICE; c->err = "k_scan_mask_verdicts launch"; }
  }
  if (!st) st = scan_event(c, 4);
  if (st && !s.st) s.st = st;
  const int32_t fin = s.finish();
  if (hipStreamSynchronize(c->stream) != hipSuccess && !st) { st = ZKP_EDEVICE; c->err = "stream sync"; }
  return st ? st : fin;
} ZKP_CATCH(c)
