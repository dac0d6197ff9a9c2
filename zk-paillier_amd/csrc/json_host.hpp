// json_host.hpp — the host tokeniser of the wire-format readers (zkp_api_serde.inc): everything that reads a document's bytes on the CPU.
// Plain C++ (no HIP, no ctx) that parses untrusted text: tests/cpp/test_json_host.cpp runs it alone under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zkp_hip.h"
#include "serde_docs.hpp"

namespace zkp {
namespace {      // (internal linkage: a library that includes this header exports nothing of it)

// ---- a JSON reader for the document shapes, as tolerant as serde_json + the derived Deserialize impls are:
// object fields in any order, unknown fields skipped (whatever their value), white space anywhere, strings with escapes
// (\uXXXX included: serde_json hands the decoded text to the bigint visitors, serialize.rs:24-27,62-66); duplicate or
// missing fields, more than one variant key in a Response, and wrong value types are errors, as they are for serde.
constexpr uint64_t EXTRA_FLAG = 1ull << 63;     // text_off of a string that had escapes: offset into the thread's decoded-copy buffer

struct JCur {
  const char* t; uint64_t p, end; bool ok = true;
  std::string* extra = nullptr;                 // decoded copies of value strings that contain escapes (per thread)
  void ws() { while (p < end && (t[p] == ' ' || t[p] == '\n' || t[p] == '\t' || t[p] == '\r')) p++; }
  bool eat(char ch) { ws(); if (p < end && t[p] == ch) { p++; return true; } return false; }
  bool expect(char ch) { if (!eat(ch)) ok = false; return ok; }
  // raw string token: content span and whether it holds a backslash (a backslash is never the last byte of the span)
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
  void skip_str() { uint64_t o; uint32_t l; bool e; raw_str(&o, &l, &e); }
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
  // a field that may be there once: the bit of `*seen` it owns
  bool once(unsigned* seen, unsigned bit) { if (*seen & bit) return ok = false; *seen |= bit; return true; }
  bool done() { ws(); return ok && p == end; }
};

struct ItemList { std::vector<zkp_dec_item> items; std::vector<uint32_t> doc; };
// what one parser thread collects: an item list per target array of the call (up to four) and the decoded copies of its escaped strings
struct ReaderThread { ItemList L[4]; std::string extra; };
constexpr unsigned READER_THREADS = 16;

// per-thread document loop: f(document, thread)
template <class F> void for_docs(uint64_t B, F f) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::max(1u, std::min(nt, READER_THREADS));
  if (B < 64) nt = 1;
  std::vector<std::thread> th;
  for (unsigned k = 0; k < nt; k++) th.emplace_back([=]() { for (uint64_t b = B * k / nt; b < B * (k + 1) / nt; b++) f(b, k); });
  for (auto& t : th) t.join();
}

// ---- the un-annotated integers (ek.n, range, ciphertext, every field of a heads-only kind): converted here, in the text form the caller names.
// -> 0 converted; ZKP_DOC_HOST_PATH: an integer this width cannot carry (negative or too wide; the token is consumed, dst is zero);
// ZKP_DOC_INVALID: not an integer of this text form (j.ok = false)
inline int parse_bigint_value(JCur& j, uint32_t enc, uint32_t* dst, uint32_t words) {
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

// EncryptionKey: an object with exactly one field "n", an integer in the key form (other fields, e.g. "nn", are skipped).
// -> whether the key is an integer this width cannot carry; a key that is none at all clears j.ok
inline bool parse_key_object(JCur& j, uint32_t key_form, uint32_t* dst, uint32_t words) {
  bool has_n = false, host = false;
  j.object([&](const std::string& f) {
    if (f != "n") return false;
    if (has_n) { j.ok = false; return true; }
    has_n = true;
    host = parse_bigint_value(j, key_form, dst, words) == ZKP_DOC_HOST_PATH;
    return true;
  });
  if (!has_n) j.ok = false;
  return host;
}

// The flags-0 reader of every heads-only kind: the tolerant tokeniser, every number converted on the host (parse_bigint_value, as for the head
// of a RangeProofNi document).  The fields are the rows of w_doc_spec(doc_kind); a key row is the object "ek" (parse_key_object).
// out[i]: [B][words of field i].  An invalid document leaves zero rows; an over-wide or negative field is zero, the others converted.
inline int32_t json_heads_host(const char* text, const uint64_t* doc_off, const uint64_t* doc_len, uint64_t B, uint32_t doc_kind, uint32_t key_form, uint32_t bare_form,
                               uint32_t kw, uint32_t yw, uint32_t* const* out, uint8_t* out_status) {
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
      if (!j.once(&seen, 1u << f)) return true;                                 // duplicate field
      uint32_t* dst = out[f] + b * words[f];
      host |= spec.h[f].key ? parse_key_object(j, key_form, dst, words[f]) : parse_bigint_value(j, bare_form, dst, words[f]) == ZKP_DOC_HOST_PATH;
      return true;
    });
    if (seen != (1u << nf) - 1) j.ok = false;                                   // missing field
    const uint8_t st = !j.done() ? ZKP_DOC_INVALID : host ? ZKP_DOC_HOST_PATH : ZKP_DOC_OK;
    out_status[b] = st;
    if (st == ZKP_DOC_INVALID) for (unsigned f = 0; f < nf; f++) memset(out[f] + b * words[f], 0, (size_t)words[f] * 4);
  });
  return ZKP_OK;
}

// ---- the three per-document tokenisers of the annotated types (serialize::{vecbigint,bigint}: decimal strings, converted on the GPU).  Each
// appends (text offset, length, destination) per number to the thread's lists and returns the document's status; of a document that is
// not ZKP_DOC_OK nothing stays appended: lists, decoded copies, kinds and js are as they were.

// Document b of a batch of EncryptedPairs (kind 0: c1, c2 into L[0], L[1], 2 kw words a number) or Proof (kind 1: w1 | masked_x, r1 | masked_r,
// w2, r2 into L[0..3], kw words; kinds / js [B][EF]: the rows' variants).  ZKP_DOC_HOST_PATH: a well-formed document with another number of rows,
// a valid value of the reference's type outside this batch layout.
inline uint8_t json_range_doc(int kind, const char* text, uint64_t off, uint64_t len, uint64_t b, uint64_t EF, uint32_t kw, ReaderThread& T, uint8_t* kinds, uint8_t* js) {
  JCur j{text, off, off + len};
  j.extra = &T.extra;
  const size_t extra_mark = T.extra.size();
  const size_t mark[4] = {T.L[0].items.size(), T.L[1].items.size(), T.L[2].items.size(), T.L[3].items.size()};
  bool other_count = false;
  auto push = [&](int which, uint64_t row, uint32_t words) {
    uint64_t o; uint32_t l;
    if (!j.str(&o, &l)) return;
    T.L[which].items.push_back({o, row * words, l, words});
    T.L[which].doc.push_back((uint32_t)b);
  };
  if (kind == 0) {
    // {"c1":[...],"c2":[...]}  (range_proof.rs:32-39), fields in any order
    unsigned seen = 0;
    j.object([&](const std::string& nm) {
      const int which = nm == "c1" ? 0 : nm == "c2" ? 1 : -1;
      if (which < 0) return false;
      if (!j.once(&seen, 1u << which)) return true;                        // duplicate field
      j.expect('[');
      uint64_t cnt = 0;
      if (j.ok && !j.eat(']')) {
        do { if (cnt < EF) push(which, b * EF + cnt, 2 * kw); else j.skip_str(); cnt++; } while (j.ok && j.eat(','));
        j.expect(']');
      }
      if (cnt != EF) other_count = true;
      return true;
    });
    if (seen != 3u) j.ok = false;                                           // missing field
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
          const bool open = vn == "Open";
          if (!open && vn != "Mask") { j.ok = false; return true; }          // unknown variant
          // the fields of the variant in the order of their lists L[0 .. 3]; Mask's j is a number, not a list
          static const char* const names[2][4] = {{"masked_x", "masked_r", "j", nullptr}, {"w1", "r1", "w2", "r2"}};
          uint64_t jv = 0;
          unsigned seen = 0;
          j.object([&](const std::string& nm) {
            int f = -1;
            for (int q = 0; q < 4; q++) if (names[open][q] && nm == names[open][q]) f = q;
            if (f < 0) return false;
            if (!j.once(&seen, 1u << f)) return true;
            if (!open && f == 2) { j.uint(&jv); if (jv > 255) j.ok = false; }
            else if (cnt < EF) push(f, row, kw);
            else j.skip_str();
            return true;
          });
          if (seen != (open ? 15u : 7u)) j.ok = false;
          if (cnt < EF) { kinds[row] = open ? ZKP_RESP_OPEN : ZKP_RESP_MASK; js[row] = (uint8_t)jv; }
          return true;
        });
        if (variants != 1) j.ok = false;
        cnt++;
      } while (j.ok && j.eat(','));
      j.expect(']');
    }
    if (cnt != EF) other_count = true;
  }
  if (j.done() && !other_count) return ZKP_DOC_OK;
  for (int q = 0; q < 4; q++) { T.L[q].items.resize(mark[q]); T.L[q].doc.resize(mark[q]); }   // nothing of a malformed document is converted
  T.extra.resize(extra_mark);
  if (kind == 1) for (uint64_t i = 0; i < EF; i++) { kinds[b * EF + i] = 0; js[b * EF + i] = 0; }
  return !j.done() ? ZKP_DOC_INVALID : ZKP_DOC_HOST_PATH;
}

// Document b of a batch of NiCorrectKeyProof: {"sigma_vec":[...]}  (correct_key_ni.rs:35-39) into L[0], kw words a number.  A vector of another
// length is a valid NiCorrectKeyProof whose verify() panics or ignores the tail (sigma_vec[i], :90): outside the fixed layout -> ZKP_DOC_INVALID
inline uint8_t json_sigma_vec_doc(const char* text, uint64_t off, uint64_t len, uint64_t b, uint32_t kw, ReaderThread& T) {
  const uint64_t M2 = ZKP_CORRECT_KEY_M2;
  JCur j{text, off, off + len};
  j.extra = &T.extra;
  ItemList& L = T.L[0];
  const size_t mark = L.items.size(), extra_mark = T.extra.size();
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
        if (j.str(&o, &l) && cnt < M2) { L.items.push_back({o, (b * M2 + cnt) * kw, l, kw}); L.doc.push_back((uint32_t)b); }
        cnt++;
      } while (j.ok && j.eat(','));
      j.expect(']');
    }
    return true;
  });
  if (!seen || cnt != M2) j.ok = false;
  if (j.done()) return ZKP_DOC_OK;
  L.items.resize(mark); L.doc.resize(mark);
  T.extra.resize(extra_mark);
  return ZKP_DOC_INVALID;
}

// The top level of a RangeProofNi document (range_proof_ni.rs:36-44): {"ek":..,"range":..,"ciphertext":..,"encrypted_pairs":..,"proof":..,
// "error_factor":..}.  ek, range and ciphertext are converted here (key [kw], range [kw], ct [2 kw]); encrypted_pairs and proof are located
// (NiSpans: their text, for json_range_doc; of a document that is not ZKP_DOC_OK two empty spans, which read as invalid, and zero range and ct).
// ZKP_DOC_HOST_PATH: a head integer the width cannot carry, or an error_factor other than the batch's (any usize is a valid RangeProofNi).
struct NiSpans { uint64_t ep_off, ep_len, pr_off, pr_len; };
inline uint8_t json_range_ni_top(const char* text, uint64_t off, uint64_t len, uint32_t key_form, uint32_t bare_form, uint32_t kw, uint64_t error_factor, uint32_t* key,
                                 uint32_t* range, uint32_t* ct, NiSpans* o) {
  JCur j{text, off, off + len};
  unsigned seen = 0;
  bool host = false;
  *o = {off, 0, off, 0};
  auto span = [&](uint64_t* s_off, uint64_t* s_len) { j.ws(); *s_off = j.p; j.skip_value(); *s_len = j.p - *s_off; };
  j.object([&](const std::string& nm) {
    if (nm == "ek") { if (j.once(&seen, 1)) host |= parse_key_object(j, key_form, key, kw); }
    else if (nm == "range") { if (j.once(&seen, 2)) host |= parse_bigint_value(j, bare_form, range, kw) == ZKP_DOC_HOST_PATH; }
    else if (nm == "ciphertext") { if (j.once(&seen, 4)) host |= parse_bigint_value(j, bare_form, ct, 2 * kw) == ZKP_DOC_HOST_PATH; }
    else if (nm == "encrypted_pairs") { if (j.once(&seen, 8)) span(&o->ep_off, &o->ep_len); }
    else if (nm == "proof") { if (j.once(&seen, 16)) span(&o->pr_off, &o->pr_len); }
    else if (nm == "error_factor") { uint64_t ef = 0; if (j.once(&seen, 32)) { j.uint(&ef); if (ef != error_factor) host = true; } }
    else return false;
    return true;
  });
  if (seen != 63u) j.ok = false;
  const uint8_t st = !j.done() ? ZKP_DOC_INVALID : host ? ZKP_DOC_HOST_PATH : ZKP_DOC_OK;
  if (st) { memset(range, 0, (size_t)kw * 4); memset(ct, 0, (size_t)kw * 8); *o = {off, 0, off, 0}; }
  return st;
}

}  // namespace
}  // namespace zkp
