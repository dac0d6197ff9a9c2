// The host tokeniser (csrc/json_host.hpp) on its own: no GPU, no library.  tests/test_cpp_json_host.py builds this file with the address and
// undefined-behaviour sanitizers and writes the cases; every document is copied into a heap block of exactly its length before it is read,
// so a read past a document's end is a sanitizer report.
//
// The case file: u32 count, then per case (little endian)
//   u32 mode (0 heads-only kind | 1 RangeProofNi through the three tokenisers | 2 every strict prefix of a canonical document)
//   u32 doc_kind, forms, n_bits, error_factor, y_bits, expected status
//   u32 fields, then per field u32 words and that many u32 limbs (mode 0: what the reader must leave)
//   u32 name length, name; u64 document length, document
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/zkp_hip.h"
#include "../../zk-paillier_amd/csrc/json_host.hpp"

using namespace zkp;

static int failures = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) { failures++; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

struct Case {
  uint32_t mode, doc_kind, forms, n_bits, ef, y_bits, status;
  std::vector<std::vector<uint32_t>> limbs;
  std::string name, doc;
};

struct Reader {
  FILE* f;
  void raw(void* p, size_t n) { if (n && std::fread(p, 1, n, f) != n) { std::printf("short case file\n"); std::exit(2); } }
  uint32_t u32() { uint32_t v; raw(&v, 4); return v; }
  uint64_t u64() { uint64_t v; raw(&v, 8); return v; }
  std::string bytes(size_t n) { std::string s(n, '\0'); raw(&s[0], n); return s; }
};

// the document in a block of exactly its length
static std::unique_ptr<char[]> exact(const std::string& doc, size_t len) {
  std::unique_ptr<char[]> p(new char[len]);
  if (len) std::memcpy(p.get(), doc.data(), len);
  return p;
}

static bool nothing_appended(const ReaderThread& T) {
  for (const ItemList& l : T.L) if (!l.items.empty() || !l.doc.empty()) return false;
  return T.extra.empty();
}

// a heads-only document of `len` bytes -> status; out: the fields
static uint8_t read_heads(const Case& c, size_t len, std::vector<std::vector<uint32_t>>* out) {
  const WDocSpec& spec = w_doc_spec(c.doc_kind);
  const uint32_t kw = c.n_bits / 32, yw = c.y_bits / 32;
  uint32_t* dst[W_MAX_HEADS] = {};
  out->assign(spec.n_heads, {});
  for (uint32_t i = 0; i < spec.n_heads; i++) { (*out)[i].assign(w_head_words(spec.h[i], kw, yw), 0xA5A5A5A5u); dst[i] = (*out)[i].data(); }
  const auto text = exact(c.doc, len);
  const uint64_t off = 0, dl = len;
  uint8_t st = 9;
  json_heads_host(text.get(), &off, &dl, 1, c.doc_kind, (c.forms >> 4) & 15u, c.forms & 15u, kw, yw, dst, &st);
  return st;
}

// a RangeProofNi document through the top-level tokeniser, then the pairs and the proof tokenisers on the spans it names: the status the
// flags-0 reader folds from the three (before any number of encrypted_pairs / proof is converted: that is the GPU's part)
static uint8_t read_range_ni(const Case& c, size_t len, bool* clean) {
  const uint32_t kw = c.n_bits / 32;
  const auto text = exact(c.doc, len);
  std::vector<uint32_t> key(kw), range(kw), ct(2 * kw);
  std::vector<uint8_t> kinds(c.ef, 7), js(c.ef, 7);
  NiSpans sp;
  const uint8_t top = json_range_ni_top(text.get(), 0, len, (c.forms >> 4) & 15u, c.forms & 15u, kw, c.ef, key.data(), range.data(), ct.data(), &sp);
  ReaderThread T1, T2;
  const uint8_t s1 = json_range_doc(0, text.get(), sp.ep_off, sp.ep_len, 0, c.ef, kw, T1, nullptr, nullptr);
  const uint8_t s2 = json_range_doc(1, text.get(), sp.pr_off, sp.pr_len, 0, c.ef, kw, T2, kinds.data(), js.data());
  *clean = true;
  if (s1 != ZKP_DOC_OK) *clean = *clean && nothing_appended(T1);
  else *clean = *clean && T1.L[0].items.size() == c.ef && T1.L[1].items.size() == c.ef;
  if (s2 != ZKP_DOC_OK) { *clean = *clean && nothing_appended(T2); for (uint32_t i = 0; i < c.ef; i++) *clean = *clean && kinds[i] == 0 && js[i] == 0; }
  if (top != ZKP_DOC_OK) *clean = *clean && sp.ep_len == 0 && sp.pr_len == 0;
  return top ? top : (s1 == ZKP_DOC_INVALID || s2 == ZKP_DOC_INVALID) ? (uint8_t)ZKP_DOC_INVALID : (s1 || s2) ? (uint8_t)ZKP_DOC_HOST_PATH : (uint8_t)ZKP_DOC_OK;
}

// any kind through its own tokeniser -> status; *clean: nothing of the document stays appended or converted
static uint8_t read_any(const Case& c, size_t len, bool* clean) {
  const uint32_t kw = c.n_bits / 32;
  if (c.doc_kind == ZKP_JSON_DOC_RANGE_PROOF_NI) return read_range_ni(c, len, clean);
  if (w_doc_spec(c.doc_kind).heads_only) {
    std::vector<std::vector<uint32_t>> out;
    const uint8_t st = read_heads(c, len, &out);
    *clean = true;
    for (auto& f : out) for (uint32_t w : f) *clean = *clean && w == 0;
    return st;
  }
  const auto text = exact(c.doc, len);
  ReaderThread T;
  std::vector<uint8_t> kinds(c.ef, 7), js(c.ef, 7);
  const uint8_t st = c.doc_kind == ZKP_JSON_DOC_CORRECT_KEY_PROOF ? json_sigma_vec_doc(text.get(), 0, len, 0, kw, T)
                                                                  : json_range_doc((int)c.doc_kind, text.get(), 0, len, 0, c.ef, kw, T, kinds.data(), js.data());
  *clean = nothing_appended(T);
  return st;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: test_json_host CASES\n"); return 2; }
  Reader r{std::fopen(argv[1], "rb")};
  if (!r.f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  const uint32_t count = r.u32();
  size_t docs = 0, prefixes = 0;
  for (uint32_t k = 0; k < count; k++) {
    Case c;
    c.mode = r.u32(); c.doc_kind = r.u32(); c.forms = r.u32(); c.n_bits = r.u32(); c.ef = r.u32(); c.y_bits = r.u32(); c.status = r.u32();
    c.limbs.resize(r.u32());
    for (auto& f : c.limbs) { f.resize(r.u32()); r.raw(f.data(), f.size() * 4); }
    c.name = r.bytes(r.u32());
    c.doc = r.bytes(r.u64());
    const char* nm = c.name.c_str();
    if (c.mode == 0) {
      std::vector<std::vector<uint32_t>> out;
      const uint8_t st = read_heads(c, c.doc.size(), &out);
      CHECK(st == c.status, "%s: status %u, expected %u", nm, st, c.status);
      CHECK(out.size() == c.limbs.size(), "%s: %zu fields", nm, out.size());
      for (size_t f = 0; f < out.size() && f < c.limbs.size(); f++) CHECK(out[f] == c.limbs[f], "%s: field %zu", nm, f);
      docs++;
    } else if (c.mode == 1) {
      bool clean = false;
      const uint8_t st = read_range_ni(c, c.doc.size(), &clean);
      CHECK(st == c.status, "%s: status %u, expected %u", nm, st, c.status);
      CHECK(clean, "%s: a tokeniser left something of a document it did not take", nm);
      docs++;
    } else {
      bool clean = false;
      const uint8_t whole = read_any(c, c.doc.size(), &clean);
      CHECK(whole == ZKP_DOC_OK, "%s: the canonical document reads as %u", nm, whole);
      for (size_t len = 0; len < c.doc.size(); len++) {
        const uint8_t st = read_any(c, len, &clean);
        CHECK(st == ZKP_DOC_INVALID, "%s: prefix of %zu bytes reads as %u", nm, len, st);
        CHECK(clean, "%s: prefix of %zu bytes left something appended", nm, len);
        prefixes++;
      }
      docs++;
    }
  }
  std::fclose(r.f);
  std::printf("%zu documents, %zu prefixes, %d failures\n", docs, prefixes, failures);
  if (!failures) std::printf("json host ok\n");
  return failures ? 1 : 0;
}
