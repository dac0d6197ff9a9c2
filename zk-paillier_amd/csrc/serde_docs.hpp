// serde_docs.hpp — the table of document kinds: which un-annotated integers a serde_json document of each kind starts with or consists
// of.  Plain C++ (no HIP): the kernels (kernels_serde_write.hpp, kernels_serde_scan.hpp), the host tokeniser (json_host.hpp) and the C ABI
// (zkp_api_serde.inc) all read this one table.
#pragma once
#include <stdint.h>
#include "../../include/zkp_hip.h"

namespace zkp {

// ---- the heads: the un-annotated integers a document starts with (a RangeProofNi) or consists of (the DLog and sigma-proof kinds).
// ONE table states them for the scanner (kernels_serde_scan.hpp), the writer (w_slot below), the flags-0 reader and zkp_json_doc_bound:
// per document kind up to W_MAX_HEADS heads, each with the literal in front of it, its field name, its width and whether it is a Paillier
// key (`ek.n`, in the batch's key form) or a bare curv BigInt (the bare form).  The host copies a kind's rows into the job of a launch
// (ScanHead / WHead), so the kernels never test a document kind to find a literal.
constexpr int W_MAX_HEADS = 6;
constexpr int W_HEAD_LIT = 20;                        // bytes of the longest literal, `,"z_double_prime":` (18), and a spare dword
enum { W_ARR_N = 0, W_ARR_RANGE, W_ARR_CT, W_ARR_C1 = W_MAX_HEADS, W_ARR_C2, W_ARR_W1, W_ARR_R1, W_ARR_W2, W_ARR_R2, W_ARRS };   // head i is array i; NiCorrectKeyProof: sigma is W_ARR_W1
enum { W_DOC_PAIRS = 0, W_DOC_PROOF = 1, W_DOC_NI = 2, W_DOC_CK = 3, W_DOC_DLOG_PROOF = 5, W_DOC_DLOG_STATEMENT = 6,      // == ZKP_JSON_DOC_* (4 and 7 are no kinds)
       W_DOC_ZERO_STATEMENT = 8, W_DOC_ZERO_PROOF, W_DOC_CT_STATEMENT, W_DOC_CT_PROOF, W_DOC_VERLIN_STATEMENT, W_DOC_VERLIN_PROOF, W_DOC_MUL_STATEMENT,
       W_DOC_MUL_PROOF, W_DOCS };
enum { W_WID_N = 0, W_WID_NN, W_WID_Z, W_WID_Y };     // kw | 2 kw | kw + ZKP_Z1_EXTRA_LIMBS | y_bits / 32 (CompositeDLogProof.y)
struct WHeadSpec { const char* lit; const char* name; uint8_t width; bool key; };
struct WDocSpec { bool valid, heads_only; uint32_t n_heads; WHeadSpec h[W_MAX_HEADS]; };
// The widest head is a 2 kw field under a 4096-bit key: 256 limbs = 1024 bytes = SCAN_MAX_BYTES of the scanner's byte-array buffer, 2048 hex
// characters, 2467 digits (kernels_serde_scan.hpp asserts the first).
constexpr uint32_t W_MAX_HEAD_WORDS = 2 * 4096 / 32;
#define W_KEY {"{\"ek\":{\"n\":", "ek", W_WID_N, true}
#define W_NN(lit, name) {lit, name, W_WID_NN, false}
inline const WDocSpec& w_doc_spec(uint32_t doc_kind) {
  static const WDocSpec none{false, false, 0, {}};
  static const WDocSpec T[W_DOCS] = {
      {true, false, 0, {}}, {true, false, 0, {}},                                                                        // EncryptedPairs, Proof
      {true, false, 3, {W_KEY, {"},\"range\":", "range", W_WID_N, false}, W_NN(",\"ciphertext\":", "ciphertext")}},         // RangeProofNi: arrays and rows follow
      {true, false, 0, {}}, none,                                                                                        // NiCorrectKeyProof, 4
      {true, true, 2, {{"{\"x\":", "x", W_WID_N, false}, {",\"y\":", "y", W_WID_Y, false}}},                                  // CompositeDLogProof
      {true, true, 3, {{"{\"N\":", "N", W_WID_N, false}, {",\"g\":", "g", W_WID_N, false}, {",\"ni\":", "ni", W_WID_N, false}}},  // DLogStatement
      none,                                                                                                              // 7
      {true, true, 2, {W_KEY, W_NN("},\"c\":", "c")}},                                                                    // ZeroStatement
      {true, true, 2, {W_NN("{\"z\":", "z"), W_NN(",\"a\":", "a")}},                                                       // ZeroProof
      {true, true, 2, {W_KEY, W_NN("},\"c\":", "c")}},                                                                    // CiphertextStatement
      {true, true, 3, {{"{\"z1\":", "z1", W_WID_Z, false}, W_NN(",\"z2\":", "z2"), W_NN(",\"c_prime\":", "c_prime")}},        // CiphertextProof
      {true, true, 4, {W_KEY, W_NN("},\"c\":", "c"), W_NN(",\"c_prime\":", "c_prime"), W_NN(",\"phi_x\":", "phi_x")}},        // VerlinStatement
      {true, true, 5, {W_NN("{\"phi_a\":", "phi_a"), {",\"z\":", "z", W_WID_Z, false}, {",\"z_prime\":", "z_prime", W_WID_Z, false},
                       {",\"z_double_prime\":", "z_double_prime", W_WID_Z, false}, W_NN(",\"r_z\":", "r_z")}},                // VerlinProof
      {true, true, 4, {W_KEY, W_NN("},\"e_a\":", "e_a"), W_NN(",\"e_b\":", "e_b"), W_NN(",\"e_c\":", "e_c")}},                // MulStatement
      {true, true, 5, {{"{\"f\":", "f", W_WID_N, false}, W_NN(",\"z1\":", "z1"), W_NN(",\"z2\":", "z2"), W_NN(",\"e_d\":", "e_d"),
                       W_NN(",\"e_db\":", "e_db")}},                                                                     // MulProof
  };
  return doc_kind < W_DOCS ? T[doc_kind] : none;
}
#undef W_KEY
#undef W_NN
inline bool w_heads_only(uint32_t doc_kind) { return w_doc_spec(doc_kind).heads_only; }
inline uint32_t w_heads(uint32_t doc_kind) { return w_doc_spec(doc_kind).n_heads; }
inline bool w_sigma_kind(uint32_t doc_kind) { return doc_kind >= W_DOC_ZERO_STATEMENT && doc_kind < W_DOCS; }
inline uint32_t w_head_words(const WHeadSpec& h, uint32_t kw, uint32_t yw) {
  return h.width == W_WID_N ? kw : h.width == W_WID_NN ? 2 * kw : h.width == W_WID_Z ? kw + ZKP_Z1_EXTRA_LIMBS : yw;
}
enum { W_FORM_DEC = ZKP_BIGINT_DEC, W_FORM_HEX = ZKP_BIGINT_HEX, W_FORM_BYTES = ZKP_BIGINT_BYTES, W_FORM_NONE = 3 };

}  // namespace zkp
