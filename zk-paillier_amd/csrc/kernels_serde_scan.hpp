// kernels_serde_scan.hpp — serde_json documents of the four proof types -> the item lists of k_dec2bin, found on the GPU: the inverse of
// the writer's grammar (w_slot() in kernels_serde_write.hpp).  One wavefront per document.
//
// CANONICAL is byte for byte what serde_json::to_string gives for the derives (and what the writer emits):
//   {"ek":{"n":X},"range":X,"ciphertext":X,"encrypted_pairs":{"c1":["D",..],"c2":["D",..]},"proof":[ROW,..],"error_factor":N}
//   ROW = {"Open":{"w1":"D","r1":"D","w2":"D","r2":"D"}} | {"Mask":{"j":U,"masked_x":"D","masked_r":"D"}}
//   D = one or more of 0-9 (leading zeros allowed), at most as many as the widest value of the field has; U = 0 .. 255 without leading
//   zeros; N = the batch's error_factor; X in the form the caller names: "D", a lower-case even-length hex string, or [U,U,..].
// The other three kinds are pieces of that grammar, scanned by the same phases started at another literal (ScanShape):
//   EncryptedPairs     {"c1":["D",..EF],"c2":["D",..EF]}
//   Proof              [ROW,..EF]
//   NiCorrectKeyProof  {"sigma_vec":["D",..11]}            one array instead of two
//   CompositeDLogProof {"x":X,"y":X}                       heads only: the head phase, then `}` and the document's end
//   DLogStatement      {"N":X,"g":X,"ni":X}
//   ZeroStatement .. MulProof                              heads only, up to five of three widths, a statement's first one behind `{"ek":{"n":`
// Which heads a kind has — literal, destination, limbs, digit bound, text form — is the table w_doc_spec() (serde_docs.hpp); the host
// copies the kind's rows into ScanJob::head, and the head phase below is a loop over them that knows no document kind.
// A document that differs in ONE byte from this is marked `fall back` and nothing else: the host tokeniser (json_host.hpp) reads it and
// decides its status.  So the scanner never has an opinion about a document it does not fully understand, and for one it understands the
// only thing left open is whether every number fits its field — k_dec2bin's overflow status, the host reader's ZKP_DOC_HOST_PATH.
//
// Phases inside the wavefront (every loop is bounded by the document's length, no byte outside [doc_off, doc_off + doc_len) is read):
//   head    (every kind with heads) the un-annotated integers: literal, value, literal ... — 64 bytes per step, the closing
//           quote / bracket found by ballot; every value is bounded by ITS field's width (ScanHead::words, dig)
//   mark    one pass over the rest, 64 bytes per step: a digit behind a quote opens a number, `{"O` / `{"M` opens a row; ballots and
//           popcounts number both (the slot of a number depends on the kinds of the rows before it) and count the non-digit bytes in
//           front of every number.  Positions go to LDS.
//   check   one lane per number / per row: the bytes between a number and the next one are exactly the literal the grammar puts there —
//           that fixes the number's length — and the count of non-digit bytes between the two starts is exactly that literal's, so every
//           byte of the number is a digit.  Literals, numbers and row openings tile the document: every byte has been compared.
//   emit    zkp_dec_item records at fixed positions (document b, row r -> item b * EF + r of the array's list, element i of sigma_vec ->
//           item b * 11 + i; an absent number — w2 / r2 of a Mask row, everything of a fall-back document — is the item "0" into its
//           own, already zero, destination)
#pragma once
#include "kernels_serde.hpp"
#include "kernels_serde_write.hpp"

namespace zkp {

constexpr int SCAN_MAX_EF = 256;
constexpr int SCAN_MAX_TOK = 6 * SCAN_MAX_EF;
constexpr int SCAN_MAX_BYTES = 1024;            // bytes of the widest head integer (ciphertext under a 4096-bit key; a DLog field has at most half)
static_assert(4 * W_MAX_HEAD_WORDS <= SCAN_MAX_BYTES, "a 2 kw head under a 4096-bit key (c, z2, e_db ..) must fit ScanLds::bytes in the byte-array form");

// one head of the job's kind: w_doc_spec()'s row with the widths and forms of this batch filled in
struct ScanHead {
  char lit[W_HEAD_LIT]; uint32_t lit_n;        // the literal in front of it, e.g. `{"ek":{"n":`, `},"c":`, `,"z_prime":`
  uint32_t words, dig, form;                  // limbs of its array element, most decimal digits of a value that wide, ZKP_BIGINT_*
  uint32_t* dst;                              // [B][words]
};

struct ScanJob {
  const char* text;            // the uploaded span: byte `a` of the caller's text is text[a - lo]
  uint64_t lo;
  const uint64_t* doc_off; const uint64_t* doc_len;
  uint64_t B;
  uint64_t zero_at;            // text[zero_at] == '0' (behind the span): the absent number
  uint64_t max_len;            // zkp_json_doc_bound: no canonical document is longer
  uint32_t doc_kind;           // W_DOC_*
  uint32_t ef, kw, key_form, bare_form;      // ef: entries per array and rows per document (NiCorrectKeyProof: the 11 of sigma_vec)
  uint32_t dig_n, dig_c;       // decimal digits of the widest kw- / 2kw-word value
  uint32_t n_heads, heads_only;              // heads_only: `}` and the document's end follow the last head
  ScanHead head[W_MAX_HEADS];
  uint8_t* kind; uint8_t* j;   // [B][EF], zero on entry
  zkp_dec_item* items[W_ARRS]; // head i: items[i] [B] (decimal form only, else null); W_ARR_C1 .. _R2: [B * EF]; sigma_vec is W_ARR_W1, as for the writer
  uint32_t* row_doc;           // [B * EF] item -> document, for k_mark_docs
  uint32_t* head_doc;          // [B] (kinds with heads only)
  uint8_t* fast;               // [B] 1 = scanned here, 0 = fall back
  uint8_t* status;             // [B] ZKP_DOC_OK | ZKP_DOC_INVALID (a fall-back document, until the host reader has spoken)
};

struct ScanLds {
  uint32_t tok_pos[SCAN_MAX_TOK + 1];   // start of number k, relative to the document
  uint32_t tok_nd[SCAN_MAX_TOK + 1];    // non-digit bytes of the marked region in front of it
  uint32_t row_pos[SCAN_MAX_EF];        // the `{` of row r
  uint32_t row_tok[SCAN_MAX_EF];        // numbers in front of row r
  uint8_t row_kind[SCAN_MAX_EF];
  uint8_t row_j[SCAN_MAX_EF];
  uint8_t bytes[SCAN_MAX_BYTES];        // a byte-array head integer, most significant byte first
  char tail[32];                        // `"}}],"error_factor":N}`
};

__device__ __forceinline__ bool sc_digit(uint32_t ch) { return ch - (uint32_t)'0' < 10u; }
__device__ __forceinline__ unsigned long long sc_below(int lane) { return lane ? ~0ull >> (64 - lane) : 0ull; }

// wave-uniform: is t[pos .. pos + n) == lit (n <= 64)?
__device__ __forceinline__ bool sc_lit(const char* t, uint32_t len, uint32_t pos, const char* lit, uint32_t n, int lane) {
  if ((uint64_t)pos + n > len) return false;
  const bool same = (uint32_t)lane >= n || t[pos + lane] == lit[lane];
  return __all(same);
}
// one lane: the same, any n
__device__ __forceinline__ bool sc_eq(const char* t, uint32_t pos, const char* lit, uint32_t n) {
  bool same = true;
  for (uint32_t i = 0; i < n; i++) same = same && t[pos + i] == lit[i];
  return same;
}

// One head integer at t[pos]: `"D"`, `"hex"` or `[U,..]`.  Returns false (wave-uniform) for anything the canonical grammar does not have;
// else pos is behind the value, a decimal value is an item, a hex / byte-array value is converted into dst[0 .. words) here.
__device__ inline bool sc_head_value(const char* t, uint32_t len, uint32_t& pos, uint32_t form, uint32_t words, uint32_t max_digits, uint32_t* dst,
                                     zkp_dec_item* item, uint64_t text_at, uint64_t dst_off, ScanLds& L, int lane) {
  const char open = form == W_FORM_BYTES ? '[' : '"', close = form == W_FORM_BYTES ? ']' : '"';
  if (pos >= len || t[pos] != open) return false;
  const uint32_t vs = pos + 1;
  const uint32_t max_chars = form == W_FORM_DEC ? max_digits : form == W_FORM_HEX ? 8 * words : 16 * words;   // (a byte value: at most "255,")
  uint32_t vlen = 0, commas = 0;
  bool found = false;
  for (uint32_t c0 = 0; c0 <= max_chars && !found; c0 += 64) {
    const uint32_t p = vs + c0 + lane;
    const uint32_t ch = p < len ? (uint8_t)t[p] : 0u;
    const bool is_close = ch == (uint8_t)close;
    bool good = sc_digit(ch);
    if (form == W_FORM_HEX) good = good || (ch >= 'a' && ch <= 'f');
    bool is_comma = false, is_first = false;
    uint32_t value = 0;
    if (form == W_FORM_BYTES && p < len) {
      is_comma = ch == ',';
      const uint32_t before = (uint8_t)t[p - 1];                 // (p - 1 >= pos: inside the document)
      if (is_comma) good = sc_digit(before) && p + 1 < len && sc_digit((uint8_t)t[p + 1]);
      else if (good && !sc_digit(before)) {
        // the first digit of a byte value: one to three digits, no leading zero, at most 255
        uint32_t nd = 1;
        value = ch - '0';
        while (nd < 4 && p + nd < len && sc_digit((uint8_t)t[p + nd])) { value = value * 10 + ((uint8_t)t[p + nd] - '0'); nd++; }
        good = nd <= 3 && value <= 255 && !(nd > 1 && ch == '0');
        is_first = good;
      }
    }
    const unsigned long long closes = __ballot(is_close), bad = __ballot(!good && !is_close), cm = __ballot(is_comma);
    const int first = closes ? __ffsll((long long)closes) - 1 : 64;
    const unsigned long long in_value = first == 64 ? ~0ull : sc_below(first);
    if (bad & in_value) return false;
    if (is_first && ((in_value >> lane) & 1ull)) {
      const uint32_t idx = commas + (uint32_t)__popcll(cm & sc_below(lane));
      if (idx < (uint32_t)SCAN_MAX_BYTES) L.bytes[idx] = (uint8_t)value;
    }
    commas += (uint32_t)__popcll(cm & in_value);
    if (first < 64) { found = true; vlen = c0 + (uint32_t)first; }
  }
  if (!found || vlen == 0 || vlen > max_chars) return false;
  if (form == W_FORM_HEX && (vlen & 1u)) return false;
  if (form == W_FORM_BYTES) {
    const uint32_t nb = commas + 1;
    if (!sc_digit((uint8_t)t[vs + vlen - 1]) || nb > 4 * words) return false;      // `[..,]`; more bytes than the field has: the host reader decides
    __syncthreads();
    for (uint32_t w = lane; w < words; w += 64) {
      uint32_t x = 0;
      for (uint32_t k = 0; k < 4; k++) { const uint32_t at = 4 * w + k; if (at < nb) x |= (uint32_t)L.bytes[nb - 1 - at] << (8 * k); }
      dst[w] = x;
    }
    __syncthreads();
  } else if (form == W_FORM_HEX) {
    for (uint32_t w = lane; w < words; w += 64) {
      uint32_t x = 0;
      for (uint32_t k = 0; k < 8; k++) {
        const uint32_t at = 8 * w + k;
        if (at < vlen) { const uint32_t ch = (uint8_t)t[vs + vlen - 1 - at]; x |= (ch <= '9' ? ch - '0' : ch - 'a' + 10) << (4 * k); }
      }
      dst[w] = x;
    }
  } else if (lane == 0) {
    *item = zkp_dec_item{text_at + vs, dst_off, vlen, words};
  }
  pos = vs + vlen + 1;
  return true;
}

// the literal behind number `f` of a row, and how many of its bytes are no digits
__device__ __forceinline__ const char* sc_after(bool mask, uint32_t f, uint32_t& n, uint32_t& nd) {
  if (mask) { n = 14; nd = 14; return "\",\"masked_r\":\""; }
  n = 8; nd = 7;
  return f == 0 ? "\",\"r1\":\"" : f == 1 ? "\",\"w2\":\"" : "\",\"r2\":\"";
}
// bytes of a row's opening up to its first number that are no digits: {"Open":{"w1":"  /  {"Mask":{"j":U,"masked_x":"
__device__ __forceinline__ uint32_t sc_open_nd(bool mask) { return mask ? 26u : 14u; }

// What the mark / check / emit phases need to know about a document kind: the arrays of strings in front of the rows, whether there are
// rows, the literal in front of the first number (or row) and the one between the last number and the end of the document.
struct ScanShape {
  uint32_t arrs;                 // 2: c1, c2; 1: sigma_vec; 0: a bare Proof
  uint32_t cnt;                  // entries per array
  uint32_t arr_words, arr_dig;   // limbs and most digits of an entry
  int arr_item;                  // W_ARR_* of the first array
  bool rows;
  const char* open; uint32_t open_n;
  const char* close; uint32_t close_n, close_nd;      // (nd: its bytes that are no digits)
};
__device__ __forceinline__ ScanShape sc_shape(const ScanJob& J, const ScanLds& L) {
  ScanShape S;
  const bool ck = J.doc_kind == W_DOC_CK;
  S.arrs = ck ? 1u : J.doc_kind == W_DOC_PROOF || J.heads_only ? 0u : 2u;
  S.cnt = J.ef;
  S.arr_words = ck ? J.kw : 2 * J.kw; S.arr_dig = ck ? J.dig_n : J.dig_c;
  S.arr_item = ck ? W_ARR_W1 : W_ARR_C1;
  S.rows = J.doc_kind == W_DOC_NI || J.doc_kind == W_DOC_PROOF;
  if (J.doc_kind == W_DOC_NI) {
    S.open = ",\"encrypted_pairs\":{\"c1\":[\""; S.open_n = 27;
    S.close = L.tail; S.close_n = 20 + (J.ef >= 100 ? 3 : J.ef >= 10 ? 2 : 1) + 1; S.close_nd = 21;
  } else if (J.doc_kind == W_DOC_PROOF) {
    S.open = "["; S.open_n = 1;
    S.close = "\"}}]"; S.close_n = 4; S.close_nd = 4;
  } else {
    S.open = ck ? "{\"sigma_vec\":[\"" : "{\"c1\":[\""; S.open_n = ck ? 15 : 8;
    S.close = "\"]}"; S.close_n = 3; S.close_nd = 3;
  }
  return S;
}
// the literal behind number k of the arrays (entry k % cnt of array k / cnt) and where it ends: the start of the next number, of row 0, or the
// document's end.  nd: bytes between the starts of this number and of the next one that are no digits; nd_at: that count at the anchor
__device__ __forceinline__ const char* sc_arr_after(const ScanShape& S, const ScanLds& L, uint32_t k, uint32_t len, uint32_t nd_total, uint32_t& n, uint32_t& nd,
                                                    uint32_t& anchor, uint32_t& nd_at) {
  const uint32_t which = k / S.cnt, i = k - which * S.cnt;
  if (k + 1 < S.arrs * S.cnt) {
    anchor = L.tok_pos[k + 1]; nd_at = L.tok_nd[k + 1];
    if (i + 1 < S.cnt) { n = 3; nd = 3; return "\",\""; }
    n = 10; nd = 9;
    return "\"],\"c2\":[\"";
  }
  if (S.rows) { n = 13; nd = 13 + sc_open_nd(L.row_kind[0] != 0); anchor = L.row_pos[0]; nd_at = L.tok_nd[k + 1]; return "\"]},\"proof\":["; }
  n = S.close_n; nd = S.close_nd; anchor = len; nd_at = nd_total;
  return S.close;
}
// the same for number f of the nf numbers of row r (number k of the document)
__device__ __forceinline__ const char* sc_row_after(const ScanShape& S, const ScanLds& L, uint32_t r, uint32_t f, uint32_t nf, bool mask, uint32_t k, uint32_t len,
                                                    uint32_t nd_total, uint32_t& n, uint32_t& nd, uint32_t& anchor, uint32_t& nd_at) {
  if (f + 1 < nf) { anchor = L.tok_pos[k + 1]; nd_at = L.tok_nd[k + 1]; return sc_after(mask, f, n, nd); }
  if (r + 1 < S.cnt) { n = 4; nd = 4 + sc_open_nd(L.row_kind[r + 1] != 0); anchor = L.row_pos[r + 1]; nd_at = L.tok_nd[k + 1]; return "\"}},"; }
  n = S.close_n; nd = S.close_nd; anchor = len; nd_at = nd_total;
  return S.close;
}

// -> wave-uniform: document [t, t + len) is canonical.  On true: L holds its numbers and rows, head_* its head (already converted unless decimal)
__device__ inline bool sc_scan_doc(const ScanJob& J, const ScanShape& S, uint64_t b, const char* t, uint32_t len, uint64_t text_at, ScanLds& L, uint32_t& ntok, int lane) {
  const uint32_t ef = J.ef, kw = J.kw;
  uint32_t pos = 0;
  for (uint32_t i = 0; i < J.n_heads; i++) {
    const ScanHead& h = J.head[i];
    if (!sc_lit(t, len, pos, h.lit, h.lit_n, lane)) return false;
    pos += h.lit_n;
    if (!sc_head_value(t, len, pos, h.form, h.words, h.dig, h.dst + b * h.words, J.items[i] ? J.items[i] + b : nullptr, text_at, b * h.words, L, lane)) return false;
  }
  if (J.heads_only) { ntok = 0; return sc_lit(t, len, pos, "}", 1, lane) && pos + 1 == len; }
  const uint32_t T = pos;
  if (!sc_lit(t, len, T, S.open, S.open_n, lane)) return false;

  // ---- mark
  const uint32_t na = S.arrs * S.cnt, want_rows = S.rows ? ef : 0u;
  const uint32_t min_toks = na + 2 * want_rows, max_toks = na + 4 * want_rows;
  uint32_t toks = 0, rows = 0, nd_base = 0, last62 = 0, last63 = 0;
  bool over = false;
  for (uint32_t p0 = T; p0 < len; p0 += 64) {
    const uint32_t p = p0 + lane;
    const bool in = p < len;
    const uint32_t ch = in ? (uint8_t)t[p] : 0u;
    uint32_t p1 = __shfl_up(ch, 1), p2 = __shfl_up(ch, 2);
    if (lane == 0) { p1 = last63; p2 = last62; } else if (lane == 1) p2 = last63;
    last62 = __shfl(ch, 62); last63 = __shfl(ch, 63);
    const bool dig = sc_digit(ch);
    const bool starts = dig && p1 == '"';
    const bool row = (ch == 'O' || ch == 'M') && p1 == '"' && p2 == '{';
    const unsigned long long m_start = __ballot(starts), m_row = __ballot(row), m_nd = __ballot(in && !dig);
    const unsigned long long lt = sc_below(lane);
    const uint32_t k = toks + (uint32_t)__popcll(m_start & lt), r = rows + (uint32_t)__popcll(m_row & lt);
    const uint32_t nd = nd_base + (uint32_t)__popcll(m_nd & lt);
    if (starts && k < (uint32_t)SCAN_MAX_TOK) { L.tok_pos[k] = p; L.tok_nd[k] = nd; }
    if (row && r < (uint32_t)SCAN_MAX_EF) { L.row_pos[r] = p - 2; L.row_tok[r] = k; L.row_kind[r] = ch == 'M'; }
    toks += (uint32_t)__popcll(m_start); rows += (uint32_t)__popcll(m_row); nd_base += (uint32_t)__popcll(m_nd);
    over = toks > max_toks || rows > want_rows;
    if (over) break;
  }
  if (over || rows != want_rows || toks < min_toks) return false;
  __syncthreads();
  ntok = toks;
  const uint32_t nd_total = nd_base;
  if ((na ? L.tok_pos[0] : L.row_pos[0]) != T + S.open_n) return false;

  // ---- check
  bool bad = false;
  // the arrays: number k = which * cnt + i
  for (uint32_t k = lane; k < na; k += 64) {
    uint32_t n, nd, anchor, nd_at;
    const char* lit = sc_arr_after(S, L, k, len, nd_total, n, nd, anchor, nd_at);
    const uint32_t s = L.tok_pos[k];
    const bool fits = anchor > s + n && anchor - s - n <= S.arr_dig;
    bad = bad || !fits || !sc_eq(t, anchor - n, lit, n) || nd_at - L.tok_nd[k] != nd;
  }
  // the rows
  for (uint32_t r = lane; r < want_rows; r += 64) {
    const bool mask = L.row_kind[r] != 0;
    const uint32_t R = L.row_pos[r], k0 = L.row_tok[r], nf = mask ? 2 : 4;
    const uint32_t expect_k0 = r == 0 ? na : L.row_tok[r - 1] + (L.row_kind[r - 1] ? 2u : 4u);
    if (k0 != expect_k0 || k0 + nf > toks || (r == ef - 1 && k0 + nf != toks)) { bad = true; continue; }
    const uint32_t s0 = L.tok_pos[k0];
    // the opening
    if (!mask) bad = bad || s0 != R + 15 || !sc_eq(t, R, "{\"Open\":{\"w1\":\"", 15);
    else {
      const uint32_t ulen = s0 - R - 26;            // (s0 > R + 2: the row was marked before its first number)
      if (s0 < R + 27 || ulen > 3 || !sc_eq(t, R, "{\"Mask\":{\"j\":", 13) || !sc_eq(t, R + 13 + ulen, ",\"masked_x\":\"", 13)) { bad = true; continue; }
      uint32_t v = 0;
      bool digits = true;
      for (uint32_t q = 0; q < ulen; q++) { const uint32_t ch = (uint8_t)t[R + 13 + q]; digits = digits && sc_digit(ch); v = v * 10 + (ch - '0'); }
      bad = bad || !digits || v > 255 || (ulen > 1 && t[R + 13] == '0');
      L.row_j[r] = (uint8_t)v;
    }
    for (uint32_t f = 0; f < nf; f++) {
      const uint32_t k = k0 + f, s = L.tok_pos[k];
      uint32_t n, nd, anchor, nd_at;
      const char* lit = sc_row_after(S, L, r, f, nf, mask, k, len, nd_total, n, nd, anchor, nd_at);
      const bool fits = anchor > s + n && anchor - s - n <= J.dig_n;
      bad = bad || !fits || !sc_eq(t, anchor - n, lit, n) || nd_at - L.tok_nd[k] != nd;
    }
  }
  return !__any(bad);
}

__global__ void __launch_bounds__(64) k_json_scan(ScanJob J) {
  __shared__ ScanLds L;
  const uint64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t ef = J.ef, kw = J.kw;
  const uint64_t len64 = J.doc_len[b], off = J.doc_off[b];
  const bool ni = J.doc_kind == W_DOC_NI;
  const uint32_t heads = J.n_heads;
  if (ni && lane == 0) {
    // `"}}],"error_factor":N}`
    const char* head = "\"}}],\"error_factor\":";
    int n = 0;
    for (; n < 20; n++) L.tail[n] = head[n];
    if (ef >= 100) L.tail[n++] = (char)('0' + ef / 100);
    if (ef >= 10) L.tail[n++] = (char)('0' + (ef / 10) % 10);
    L.tail[n++] = (char)('0' + ef % 10);
    L.tail[n++] = '}';
  }
  __syncthreads();
  const ScanShape S = sc_shape(J, L);
  bool ok = len64 != 0 && len64 <= J.max_len;
  const uint64_t text_at = ok ? off - J.lo : 0;
  const char* t = J.text + text_at;
  const uint32_t len = (uint32_t)len64;
  uint32_t ntok = 0;
  if (ok) ok = sc_scan_doc(J, S, b, t, len, text_at, L, ntok, lane);
  __syncthreads();

  // ---- emit
  if (lane == 0) {
    J.fast[b] = ok ? 1 : 0;
    J.status[b] = ok ? ZKP_DOC_OK : ZKP_DOC_INVALID;
    if (heads) J.head_doc[b] = (uint32_t)b;
    for (uint32_t i = 0; i < heads && !ok; i++)
      if (J.items[i]) J.items[i][b] = zkp_dec_item{J.zero_at, b * J.head[i].words, 1, J.head[i].words};
  }
  for (uint32_t k = lane; k < S.arrs * S.cnt; k += 64) {
    const uint32_t which = k / S.cnt, i = k - which * S.cnt;
    const uint64_t slot = b * S.cnt + i;
    if (which == 0) J.row_doc[slot] = (uint32_t)b;
    zkp_dec_item it{J.zero_at, slot * S.arr_words, 1, S.arr_words};
    if (ok) {
      uint32_t n, nd, anchor, nd_at;
      (void)sc_arr_after(S, L, k, len, 0, n, nd, anchor, nd_at);
      const uint32_t s = L.tok_pos[k];
      it.text_off = text_at + s; it.len = anchor - s - n;
    }
    J.items[S.arr_item + which][slot] = it;
  }
  for (uint32_t r = lane; S.rows && r < ef; r += 64) {
    const uint64_t slot = b * ef + r;
    J.row_doc[slot] = (uint32_t)b;
    const bool mask = ok && L.row_kind[r] != 0;
    const uint32_t nf = !ok ? 0 : mask ? 2 : 4;
    if (ok) { J.kind[slot] = mask ? ZKP_RESP_MASK : ZKP_RESP_OPEN; J.j[slot] = mask ? L.row_j[r] : 0; }
    for (uint32_t f = 0; f < 4; f++) {
      zkp_dec_item it{J.zero_at, slot * kw, 1, kw};
      if (f < nf) {
        const uint32_t k = L.row_tok[r] + f, s = L.tok_pos[k];
        uint32_t n, nd, anchor, nd_at;
        (void)sc_row_after(S, L, r, f, nf, mask, k, len, 0, n, nd, anchor, nd_at);
        it.text_off = text_at + s; it.len = anchor - s - n;
      }
      J.items[W_ARR_W1 + f][slot] = it;
    }
  }
}

// RangeProofNi::verify asserts that the proof was made under the verifier's key: a scanned document whose head converted (status still OK)
// under another key is ZKP_DOC_INVALID.  One wavefront per document.
__global__ void __launch_bounds__(256) k_scan_key_check(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ n, uint32_t kw, uint64_t B,
                                                        const uint8_t* __restrict__ fast, uint8_t* __restrict__ status) {
  const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  bool differs = false;
  for (uint32_t w = lane; w < kw; w += 64) differs = differs || keys[b * kw + w] != n[w];
  if (__any(differs) && lane == 0 && fast[b] && status[b] == ZKP_DOC_OK) status[b] = ZKP_DOC_INVALID;
}

// the documents the host reader took: unit u of its document i -> unit u of document idx[i] of the batch
template <class T> __global__ void __launch_bounds__(256) k_scan_merge(const T* __restrict__ src, T* __restrict__ dst, uint64_t units_per_doc,
                                                                        const uint32_t* __restrict__ idx, uint64_t docs) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= docs * units_per_doc) return;
  const uint64_t d = i / units_per_doc;
  dst[(uint64_t)idx[d] * units_per_doc + (i - d * units_per_doc)] = src[i];
}

// a caller who ignores the status never accepts an unread proof
__global__ void __launch_bounds__(256) k_scan_mask_verdicts(const uint8_t* __restrict__ status, uint8_t* __restrict__ verdict, uint64_t B) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < B && status[b] != ZKP_DOC_OK) verdict[b] = ZKP_VERDICT_REJECT;
}

// a session of two documents: its status is the worse of theirs (INVALID beats HOST_PATH beats OK)
__global__ void __launch_bounds__(256) k_scan_worse_status(uint8_t* __restrict__ status, const uint8_t* __restrict__ other, uint64_t B) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint8_t s1 = status[b], s2 = other[b];
  status[b] = (s1 == ZKP_DOC_INVALID || s2 == ZKP_DOC_INVALID) ? (uint8_t)ZKP_DOC_INVALID : (s1 != ZKP_DOC_OK || s2 != ZKP_DOC_OK) ? (uint8_t)ZKP_DOC_HOST_PATH : (uint8_t)ZKP_DOC_OK;
}

// ---- CompositeDLogProof::verify on documents: is pair b inside the domain of the limb kernels?
// wave-uniform: v < n, both kw words, most significant word first: the highest word in which they differ decides (found by ballot)
__device__ __forceinline__ bool sc_less(const uint32_t* __restrict__ v, const uint32_t* __restrict__ n, uint32_t kw, int lane) {
  for (int c0 = (int)((kw - 1) & ~63u); c0 >= 0; c0 -= 64) {
    const uint32_t w = (uint32_t)c0 + (uint32_t)lane;
    const uint32_t a = w < kw ? v[w] : 0u, m = w < kw ? n[w] : 0u;
    const unsigned long long differ = __ballot(a != m);
    if (differ) return __shfl((int)(a < m), 63 - __clzll((long long)differ)) != 0;
  }
  return false;
}
// The status of pair b starts as the worse of its two documents' (INVALID beats HOST_PATH beats OK).  A pair still OK whose N is even or zero,
// or with one of g, ni, x >= N, has a verdict in the reference (mod_pow reduces its base, an even N is legal there) that the Montgomery
// kernels cannot give: ZKP_DOC_HOST_PATH.  The five fields of every pair that is not OK are zeroed: N = 0 is answered by k_dlog_hash with
// MALFORMED before any arithmetic, and k_setup marks the modulus so that no ladder stores a result.  One wavefront per pair.
__global__ void __launch_bounds__(256) k_dlog_domain_check(uint32_t* __restrict__ N, uint32_t* __restrict__ g, uint32_t* __restrict__ ni, uint32_t* __restrict__ x,
                                                           uint32_t* __restrict__ y, uint32_t kw, uint32_t yw, uint64_t B, const uint8_t* __restrict__ proof_status,
                                                           uint8_t* __restrict__ status) {
  const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const uint8_t s1 = status[b], s2 = proof_status[b];
  uint8_t st = (s1 == ZKP_DOC_INVALID || s2 == ZKP_DOC_INVALID) ? (uint8_t)ZKP_DOC_INVALID : (s1 != ZKP_DOC_OK || s2 != ZKP_DOC_OK) ? (uint8_t)ZKP_DOC_HOST_PATH : (uint8_t)ZKP_DOC_OK;
  if (st == ZKP_DOC_OK) {
    const uint32_t* n = N + b * kw;
    const bool odd = (n[0] & 1u) != 0;
    const bool lg = sc_less(g + b * kw, n, kw, lane), lni = sc_less(ni + b * kw, n, kw, lane), lx = sc_less(x + b * kw, n, kw, lane);
    if (!(odd && lg && lni && lx)) st = ZKP_DOC_HOST_PATH;
  }
  if (lane == 0) status[b] = st;
  if (st == ZKP_DOC_OK) return;
  for (uint32_t w = lane; w < kw; w += 64) { N[b * kw + w] = 0; g[b * kw + w] = 0; ni[b * kw + w] = 0; x[b * kw + w] = 0; }
  for (uint32_t w = lane; w < yw; w += 64) y[b * yw + w] = 0;
}


// ---- ZeroProof / CiphertextProof / VerlinProof / MulProof::verify on documents: the same question for a (statement, proof) pair of those
// types.  Up to SIGMA_MAX_ARR arrays: arr[0] is the key n [B][kw], the others the fields of both documents; rule[i] says what field i must
// satisfy: SIGMA_LT_NN: < n^2 (nn [B][2 kw], squared on the device beforehand; words[i] == 2 kw), SIGMA_LT_N: < n (MulProof.f, words[i] == kw),
// SIGMA_ANY: nothing (the z fields are integers, not residues).  A pair still OK becomes ZKP_DOC_HOST_PATH when its key is even or trivial
// as k_setup defines it (no bits above the lowest), or a field breaks its rule: the reference reduces such a value (mod_pow, %,
// Paillier::add) and hashes it raw, the limb kernels were never specified for it.  Every row of a pair that is not OK is zeroed: the key 0
// is marked by k_setup (nothing is stored for it) and answered MALFORMED by the compare kernels, masked afterwards.  One wavefront per pair.
constexpr int SIGMA_MAX_ARR = 10;
enum { SIGMA_ANY = 0, SIGMA_LT_NN = 1, SIGMA_LT_N = 2 };
struct SigmaDomainArgs {
  uint32_t* arr[SIGMA_MAX_ARR]; uint32_t words[SIGMA_MAX_ARR]; uint32_t rule[SIGMA_MAX_ARR];
  uint32_t n_arr, kw;
  const uint32_t* nn;
  uint64_t B;
  const uint8_t* proof_status; uint8_t* status;
};
__global__ void __launch_bounds__(256) k_sigma_domain_check(SigmaDomainArgs a) {
  const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= a.B) return;
  const uint32_t kw = a.kw;
  const uint8_t s1 = a.status[b], s2 = a.proof_status[b];
  uint8_t st = (s1 == ZKP_DOC_INVALID || s2 == ZKP_DOC_INVALID) ? (uint8_t)ZKP_DOC_INVALID : (s1 != ZKP_DOC_OK || s2 != ZKP_DOC_OK) ? (uint8_t)ZKP_DOC_HOST_PATH : (uint8_t)ZKP_DOC_OK;
  if (st == ZKP_DOC_OK) {
    const uint32_t* n = a.arr[0] + b * kw;
    bool above = false;                                   // a bit above the lowest: n >= 2
    for (uint32_t w = lane; w < kw; w += 64) above = above || (w == 0 ? n[0] >> 1 : n[w]) != 0;
    bool inside = (n[0] & 1u) != 0 && __any(above);
    for (uint32_t i = 1; i < a.n_arr; i++) {
      if (a.rule[i] == SIGMA_LT_NN) inside = sc_less(a.arr[i] + b * 2 * kw, a.nn + b * 2 * kw, 2 * kw, lane) && inside;
      else if (a.rule[i] == SIGMA_LT_N) inside = sc_less(a.arr[i] + b * kw, n, kw, lane) && inside;
    }
    if (!inside) st = ZKP_DOC_HOST_PATH;
  }
  if (lane == 0) a.status[b] = st;
  if (st == ZKP_DOC_OK) return;
  for (uint32_t i = 0; i < a.n_arr; i++)
    for (uint32_t w = lane; w < a.words[i]; w += 64) a.arr[i][b * a.words[i] + w] = 0;
}

}  // namespace zkp
