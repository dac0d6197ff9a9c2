// kernels_serde_write.hpp — the SoA batch -> serde_json documents, written on the GPU (the mirror image of the readers in
// zkp_api_serde.inc).  A document is a row of SLOTS: a literal prefix, one number, a literal suffix — e.g. `","r1":"` <digits> `` or
// `,"` <digits> `"]}`.  Three phases:
//   convert   k_w_convert: limbs -> base-10^9 groups (k_bin2dec's short division in thread-interleaved LDS), one number per lane; a
//             group is ONE dword store and the 64 lanes of a pass write 64 consecutive dwords.  The exact digit count of every number
//             falls out.  (ek.n / range / ciphertext in a hex or byte-array form need no radix conversion: k_w_formlen sizes them.)
//   size      k_w_doclen: one wavefront per document adds up literal and digit counts of its slots (an exclusive scan: every slot gets
//             its own 64-bit start inside the document); k_w_scan: exclusive scan over the documents, 64 bits.
//   assemble  k_w_assemble: one wavefront per slot, lanes spread over OUTPUT bytes: lane t builds the four bytes of the t-th aligned
//             dword of the slot's span and stores it whole; only the ragged first / last dword of a span takes byte stores.
// Every offset and size is 64 bits wide: 4096 documents under a 2048-bit key are 2.3 GB of text.
#pragma once
#include "kernels_serde.hpp"
#include "serde_docs.hpp"

namespace zkp {

// a head as the writer's job carries it: the literal, and whether the number takes the key form
struct WHead { char lit[W_HEAD_LIT]; uint32_t lit_n, key; };
template <class H> inline void w_head_lit(H& dst, const WHeadSpec& h) {
  uint32_t n = 0;
  for (; h.lit[n]; n++) dst.lit[n] = h.lit[n];
  dst.lit_n = n;
}

// one SoA array of numbers: number i is src[i * words .. + words); its converted form is
//   decimal:        len[i] digits, group g (9 digits, least significant first) at groups[((i / 64) * G + g) * 64 + i % 64]
//   hex / bytes:    len[i] characters of text, groups[i] = bytes of the big-endian magnitude (at least one)
struct WArr { const uint32_t* src; uint32_t* groups; uint32_t* len; uint32_t words, G; };
struct WJob {
  WArr a[W_ARRS];
  const uint8_t* kind; const uint8_t* j;     // [B][EF]; null for documents without a Proof
  uint64_t B;
  uint32_t ef, doc_kind, key_form, bare_form, slots, per_proof_keys;     // per_proof_keys: head 0 is read per document, not once per batch
  uint32_t n_heads, heads_only;                                          // the kind's rows of w_doc_spec()
  WHead head[W_MAX_HEADS];
};

struct WSlot { int arr; uint32_t form; uint64_t idx; uint32_t pre_len, post_len; uint8_t pre_byte, post_byte; };

__device__ __forceinline__ void w_app(const char* s, int n, int& pos, int want, uint8_t& got) {
  const int k = want - pos;
  if (k >= 0 && k < n) got = (uint8_t)s[k];
  pos += n;
}
__device__ __forceinline__ void w_app_uint(uint32_t v, int& pos, int want, uint8_t& got) {      // v < 1000
  const int n = v >= 100 ? 3 : v >= 10 ? 2 : 1;
  const int k = want - pos;
  if (k >= 0 && k < n) { const uint32_t d = k == n - 1 ? v % 10 : k == n - 2 ? (v / 10) % 10 : v / 100; got = (uint8_t)('0' + d); }
  pos += n;
}
#define W_PRE(S) w_app(S, (int)sizeof(S) - 1, pre, want, o.pre_byte)
#define W_POST(S) w_app(S, (int)sizeof(S) - 1, post, want, o.post_byte)

// Slot s of document b: which number it carries and the literals around it.  `want`: the caller also gets byte `want` of the prefix and
// of the suffix (every lane of a wavefront asks for its own: 64 lanes hold the whole literal); -1: lengths only.
// The single statement of the documents' grammar: k_w_doclen and k_w_assemble both go through it.
__device__ inline WSlot w_slot(const WJob& J, uint64_t b, uint32_t s, int want) {
  WSlot o; o.arr = -1; o.form = W_FORM_DEC; o.idx = 0; o.pre_byte = o.post_byte = 0;
  int pre = 0, post = 0;
  const uint32_t ef = J.ef;
  const bool ni = J.doc_kind == W_DOC_NI;
  uint32_t t = s;
  if (J.doc_kind == W_DOC_CK) {
    o.arr = W_ARR_W1; o.idx = b * ZKP_CORRECT_KEY_M2 + s;
    if (s == 0) W_PRE("{\"sigma_vec\":[\""); else W_PRE(",\"");
    W_POST("\"");
    if (s == ZKP_CORRECT_KEY_M2 - 1) W_POST("]}");
  } else if (s < J.n_heads) {
    // a head: the table's literal, the number in its form; a heads-only document closes behind its last one
    const WHead& h = J.head[s];
    o.arr = (int)s; o.form = h.key ? J.key_form : J.bare_form;
    o.idx = s == 0 && !J.per_proof_keys ? 0 : b;
    w_app(h.lit, (int)h.lit_n, pre, want, o.pre_byte);
    if (o.form == W_FORM_BYTES) { W_PRE("["); W_POST("]"); } else { W_PRE("\""); W_POST("\""); }
    if (J.heads_only && s + 1 == J.slots) W_POST("}");
  } else {
    t -= J.n_heads;
    if (J.doc_kind != W_DOC_PROOF && t < 2 * ef) {
      const uint32_t which = t / ef, i = t - which * ef;
      o.arr = W_ARR_C1 + (int)which; o.idx = b * ef + i;
      if (i != 0) W_PRE(",\"");
      else if (which == 1) W_PRE(",\"c2\":[\"");
      else { if (ni) W_PRE(",\"encrypted_pairs\":"); W_PRE("{\"c1\":[\""); }
      W_POST("\"");
      if (i == ef - 1) { W_POST("]"); if (which == 1) W_POST("}"); }
    } else {
      if (J.doc_kind != W_DOC_PROOF) t -= 2 * ef;
      const uint32_t row = t / 4, f = t & 3;
      const uint64_t r = b * ef + row;
      const bool mask = J.kind[r] == ZKP_RESP_MASK;
      o.arr = W_ARR_W1 + (int)f; o.idx = r;
      if (mask && f >= 2) {
        o.form = W_FORM_NONE;                       // a Mask row has two numbers
      } else {
        if (f == 0) {
          if (row != 0) W_PRE(","); else { if (ni) W_PRE(",\"proof\":"); W_PRE("["); }
          if (mask) { W_PRE("{\"Mask\":{\"j\":"); w_app_uint(J.j[r], pre, want, o.pre_byte); W_PRE(",\"masked_x\":\""); }
          else W_PRE("{\"Open\":{\"w1\":\"");
        } else if (f == 1) { if (mask) W_PRE("\",\"masked_r\":\""); else W_PRE("\",\"r1\":\""); }
        else if (f == 2) W_PRE("\",\"w2\":\"");
        else W_PRE("\",\"r2\":\"");
        if (f == (mask ? 1u : 3u)) {
          W_POST("\"}}");
          if (row == ef - 1) {
            W_POST("]");
            if (ni) { W_POST(",\"error_factor\":"); w_app_uint(ef, post, want, o.post_byte); W_POST("}"); }
          }
        }
      }
    }
  }
  o.pre_len = (uint32_t)pre; o.post_len = (uint32_t)post;
  return o;
}
#undef W_PRE
#undef W_POST

// ---- convert: k_bin2dec's arithmetic, another output side
__global__ void __launch_bounds__(SERDE_LANES) k_w_convert(const uint32_t* __restrict__ src, int words, uint64_t count, uint32_t* __restrict__ groups, uint32_t G,
                                                           uint32_t* __restrict__ len) {
  extern __shared__ __align__(16) uint32_t acc[];
  const int lane = threadIdx.x;
  const uint64_t item0 = (uint64_t)blockIdx.x * SERDE_LANES;
  for (int j = 0; j < SERDE_LANES; j++) {                      // cooperative, coalesced read-in
    const uint64_t id = item0 + j;
    if (id >= count) break;
    for (int w = lane; w < words; w += SERDE_LANES) acc[w * SERDE_LANES + j] = src[id * (uint64_t)words + w];
  }
  __syncthreads();
  const uint64_t idx = item0 + lane;
  if (idx >= count) return;
  uint32_t* x = acc + lane;
  uint32_t* out = groups + (uint64_t)blockIdx.x * G * SERDE_LANES + lane;
  int n_live = words;
  while (n_live > 0 && x[(n_live - 1) * SERDE_LANES] == 0) n_live--;
  uint32_t g = 0, top = 0;
  if (n_live == 0) { out[0] = 0; g = 1; }
  while (n_live > 0) {
    uint64_t rem = 0;
    for (int w = n_live - 1; w >= 0; w--) {
      const uint64_t cur = (rem << 32) | x[w * SERDE_LANES];
      const uint64_t q = cur / 1000000000ull;
      rem = cur - q * 1000000000ull;
      x[w * SERDE_LANES] = (uint32_t)q;
    }
    while (n_live > 0 && x[(n_live - 1) * SERDE_LANES] == 0) n_live--;
    top = (uint32_t)rem;
    if (g < G) out[(uint64_t)g * SERDE_LANES] = top;           // (g < G always: G covers every value of this width)
    g++;
  }
  uint32_t d = 1;
  for (uint32_t p = 10; d < 9 && top >= p; p *= 10) d++;
  len[idx] = 9 * (g - 1) + d;
}

// ---- the text length of a number in hex (two characters per byte of the big-endian magnitude) or as an array of byte values
__device__ __forceinline__ uint32_t w_byte_digits(uint32_t v) { return v >= 100 ? 3 : v >= 10 ? 2 : 1; }
__global__ void __launch_bounds__(256) k_w_formlen(const uint32_t* __restrict__ src, int words, uint64_t count, uint32_t form, uint32_t* __restrict__ nbytes,
                                                   uint32_t* __restrict__ len) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const uint32_t* x = src + i * (uint64_t)words;
  int w = words - 1;
  while (w > 0 && x[w] == 0) w--;
  const uint32_t bits = x[w] ? 32u * (uint32_t)w + (32u - (uint32_t)__clz((int)x[w])) : 0u;
  const uint32_t nb = bits ? (bits + 7) / 8 : 1;
  uint32_t l = 2 * nb;
  if (form == W_FORM_BYTES) {
    l = nb - 1;                                               // commas
    for (uint32_t k = 0; k < nb; k++) l += w_byte_digits((x[k / 4] >> (8 * (k % 4))) & 255u);
  }
  nbytes[i] = nb; len[i] = l;
}

// ---- size
__global__ void __launch_bounds__(64) k_w_doclen(WJob J, uint64_t* __restrict__ rel, uint64_t* __restrict__ doclen, uint8_t* __restrict__ status) {
  const uint64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  int bad = 0;
  if (J.kind)
    for (uint32_t r = lane; r < J.ef; r += 64) { const uint8_t k = J.kind[b * J.ef + r]; bad |= (k != ZKP_RESP_OPEN && k != ZKP_RESP_MASK); }
  bad = __any(bad);
  uint64_t base = 0;
  for (uint32_t s0 = 0; s0 < J.slots; s0 += 64) {
    const uint32_t s = s0 + lane;
    uint32_t l = 0;
    if (s < J.slots && !bad) {
      const WSlot o = w_slot(J, b, s, -1);
      l = o.pre_len + o.post_len + (o.form != W_FORM_NONE ? J.a[o.arr].len[o.idx] : 0u);
    }
    uint32_t incl = l;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
    if (s < J.slots) rel[b * J.slots + s] = base + incl - l;
    base += __shfl(incl, 63);
  }
  if (lane == 0) { doclen[b] = base; if (status) status[b] = bad ? ZKP_DOC_INVALID : ZKP_DOC_OK; }
}

// off[0] = 0, off[b + 1] = off[b] + doclen[b]: one workgroup, every thread a contiguous run of documents
__global__ void __launch_bounds__(1024) k_w_scan(const uint64_t* __restrict__ doclen, uint64_t B, uint64_t* __restrict__ off) {
  __shared__ uint64_t part[1024];
  const uint64_t per = (B + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < B ? lo + per : B;
  uint64_t sum = 0;
  for (uint64_t i = lo; i < hi; i++) sum += doclen[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint64_t t = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += t;
    __syncthreads();
  }
  uint64_t run = part[threadIdx.x] - sum;
  if (threadIdx.x == 0) off[0] = 0;
  for (uint64_t i = lo; i < hi; i++) { run += doclen[i]; off[i + 1] = run; }
}

// ---- assemble: slots [slot_lo, slot_lo + n_slots) (global slot index = document * J.slots + slot); byte `a` of the batch's text lands in
// out[a - out_base], out_base a multiple of four and `out` dword aligned, so that alignment in the text is alignment in memory
__device__ __forceinline__ uint32_t w_dec_digit(uint32_t v, uint32_t k) {
  switch (k) {
    case 0: break;            case 1: v /= 10u; break;        case 2: v /= 100u; break;
    case 3: v /= 1000u; break; case 4: v /= 10000u; break;    case 5: v /= 100000u; break;
    case 6: v /= 1000000u; break; case 7: v /= 10000000u; break; default: v /= 100000000u; break;
  }
  return v % 10u;
}

__global__ void __launch_bounds__(256) k_w_assemble(WJob J, const uint64_t* __restrict__ rel, const uint64_t* __restrict__ off, uint64_t slot_lo, uint64_t n_slots,
                                                    char* __restrict__ out, uint64_t out_base) {
  __shared__ uint8_t lit[4][128];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t w = (uint64_t)blockIdx.x * 4 + wave;
  const bool live = w < n_slots;
  uint64_t A = 0;
  uint32_t body = 0;
  WSlot o; o.arr = -1; o.form = W_FORM_NONE; o.idx = 0; o.pre_len = o.post_len = 0;
  if (live) {
    const uint64_t gs = slot_lo + w, b = gs / J.slots;
    const uint32_t s = (uint32_t)(gs - b * J.slots);
    if (off[b + 1] != off[b]) {                                // an empty document: a Response kind no variant has
      o = w_slot(J, b, s, lane);
      A = off[b] + rel[gs];
      if (o.form != W_FORM_NONE) body = J.a[o.arr].len[o.idx];
      lit[wave][lane] = o.pre_byte; lit[wave][64 + lane] = o.post_byte;
    }
  }
  __syncthreads();
  const uint64_t end = A + o.pre_len + body + o.post_len;
  if (end == A) return;
  const WArr ar = J.a[o.arr];
  const uint32_t* grp = ar.groups + ((o.idx >> 6) * ar.G) * 64 + (o.idx & 63);
  const uint32_t* limbs = ar.src + o.idx * (uint64_t)ar.words;
  for (uint64_t d = (A & ~3ull) + 4u * (uint32_t)lane; d < end; d += 256) {
    uint32_t word = 0, mask = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t a = d + k;
      if (a < A || a >= end) continue;
      const uint32_t p = (uint32_t)(a - A);
      uint32_t ch;
      if (p < o.pre_len) ch = lit[wave][p];
      else if (p >= o.pre_len + body) ch = lit[wave][64 + p - o.pre_len - body];
      else if (o.form == W_FORM_DEC) {
        const uint32_t i = body - 1 - (p - o.pre_len), g = i / 9u;
        ch = '0' + w_dec_digit(grp[(uint64_t)g * 64], i - 9u * g);
      } else if (o.form == W_FORM_HEX) {
        const uint32_t i = body - 1 - (p - o.pre_len), nib = (limbs[i / 8] >> (4 * (i % 8))) & 15u;
        ch = nib < 10 ? '0' + nib : 'a' + (nib - 10);
      } else continue;                                         // byte values: below
      word |= ch << (8 * k); mask |= 1u << k;
    }
    char* dst = out + (d - out_base);
    if (mask == 15u) *reinterpret_cast<uint32_t*>(dst) = word;
    else
      for (int k = 0; k < 4; k++) if (mask >> k & 1u) dst[k] = (char)(word >> (8 * k));
  }
  if (o.form == W_FORM_BYTES) {
    // [4,210]: lanes over the bytes of the magnitude, most significant first; a wavefront scan places their one to three digits.
    // Three numbers of a document's ~770 take this path.
    const uint32_t nb = ar.groups[o.idx];
    uint64_t at = A + o.pre_len - out_base;
    for (uint32_t c0 = 0; c0 < nb; c0 += 64) {
      const uint32_t k = c0 + lane;
      uint32_t v = 0, l = 0;
      if (k < nb) { const uint32_t bp = nb - 1 - k; v = (limbs[bp / 4] >> (8 * (bp % 4))) & 255u; l = w_byte_digits(v) + (k + 1 < nb ? 1u : 0u); }
      uint32_t incl = l;
      for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t t = __shfl_up(incl, dd); if (lane >= dd) incl += t; }
      if (k < nb) {
        char* dst = out + at + (incl - l);
        const uint32_t nd = w_byte_digits(v);
        if (nd == 3) *dst++ = (char)('0' + v / 100);
        if (nd >= 2) *dst++ = (char)('0' + (v / 10) % 10);
        *dst++ = (char)('0' + v % 10);
        if (k + 1 < nb) *dst = ',';
      }
      at += __shfl(incl, 63);
    }
  }
}

}  // namespace zkp
