"""ctypes binding of libzkp_hip.so (include/zkp_hip.h).

There is no CPU fallback: importing this module without the built library, or creating a
context without a gfx950 GPU, raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZKP_HIP_LIB") or os.path.join(_HERE, "libzkp_hip.so")   # (the override is for A/B measurements of kernel variants)

ZKP_OK, ZKP_EINVAL, ZKP_ENONCANONICAL, ZKP_EDEVICE, ZKP_ENOMEM = range(5)
ZKP_F_DEVICE_PTRS = 1
VERDICT_REJECT, VERDICT_ACCEPT, VERDICT_MALFORMED = 0, 1, 2
INV_OK, INV_NONE, INV_DOMAIN = 0, 1, 2
RESP_OPEN, RESP_MASK = 0, 1
SECURITY_PARAMETER = 128
CORRECT_KEY_M2 = 11

u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)


class RangeNiProofs(C.Structure):
    """zkp_range_ni_proofs"""
    _fields_ = [
        ("n_bits", C.c_uint32), ("error_factor", C.c_uint32), ("batch", C.c_uint64),
        ("n_stride", C.c_uint64), ("n", C.c_void_p), ("range", C.c_void_p),
        ("ciphertext", C.c_void_p), ("c1", C.c_void_p), ("c2", C.c_void_p),
        ("resp_kind", C.c_void_p), ("resp_j", C.c_void_p), ("resp_w1", C.c_void_p),
        ("resp_r1", C.c_void_p), ("resp_w2", C.c_void_p), ("resp_r2", C.c_void_p),
    ]


class RangeNiWitness(C.Structure):
    """zkp_range_ni_witness"""
    _fields_ = [("x", C.c_void_p), ("r", C.c_void_p), ("w1", C.c_void_p), ("w2", C.c_void_p),
                ("r1", C.c_void_p), ("r2", C.c_void_p)]


# include/zkp_hip_diag.h: measurement tooling, not the boundary
DIAG_EXPORTS = {
    "zkp_diag_table_traffic": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]),
    "zkp_diag_basen": (C.c_int32, [C.c_void_p, C.c_uint32] + [C.c_void_p, C.c_int32] + [C.c_void_p] * 5),
    "zkp_diag_basen_last": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
    "zkp_diag_basen_engine": (C.c_int32, []),
    "zkp_diag_set_enc_form": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_diag_enc_form": (C.c_int32, [C.c_void_p]),
    "zkp_diag_last_host_blocks": (C.c_int32, [C.c_void_p]),
    "zkp_diag_set_r2l": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_diag_r2l_last": (C.c_int32, [C.c_void_p]),
    "zkp_diag_set_r2l_lanes": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_diag_r2l_lanes_last": (C.c_int32, [C.c_void_p]),
    "zkp_diag_mid_limbs_per_lane": (C.c_int32, [C.c_void_p]),
    "zkp_diag_set_fuse_hash": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_diag_last_fused_hash": (C.c_int32, [C.c_void_p]),
    "zkp_diag_set_split": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_diag_last_split": (C.c_int32, [C.c_void_p]),
    "zkp_diag_set_key_cache": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_diag_key_cache_state": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32)]),
    "zkp_diag_witness_residue": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "zkp_diag_prime_table": (C.c_int32, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "zkp_diag_prime_search": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zkp_diag_last_json_scan": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zkp_diag_last_json_scan_ms": (C.c_int32, [C.c_void_p, C.POINTER(C.c_double)]),
}
ENC_FORM_AUTO, ENC_FORM_N2, ENC_FORM_SHARED, ENC_FORM_ALWAYS = 0, 1, 2, 3
ENC_FORMS = {"auto": ENC_FORM_AUTO, "n2": ENC_FORM_N2, "shared": ENC_FORM_SHARED, "basen": ENC_FORM_ALWAYS, "always": ENC_FORM_ALWAYS}

# include/zkp_hip.h: the boundary
EXPORTS = {
    # name: (restype, argtypes)
    "zkp_ctx_create": (C.c_int32, [C.c_int32, C.POINTER(C.c_void_p)]),
    "zkp_ctx_destroy": (C.c_int32, [C.c_void_p]),
    "zkp_backend_name": (C.c_char_p, []),
    "zkp_build_limbs_per_lane": (C.c_int32, []),
    "zkp_last_error_string": (C.c_char_p, [C.c_void_p]),
    "zkp_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "zkp_ctx_synchronize": (C.c_int32, [C.c_void_p]),
    "zkp_ctx_release_staging": (C.c_int32, [C.c_void_p]),
    "zkp_timing_reset": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_timing_get": (C.c_int32, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zkp_modexp_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    "zkp_modmul_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p, C.c_uint32]),
    "zkp_paillier_enc_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_paillier_enc_check_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_ni_prove_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.POINTER(RangeNiWitness),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_sample_witness_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_ni_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_ni_verify_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_uint32]),
    "zkp_range_generate_encrypted_pairs_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.POINTER(RangeNiWitness), C.c_uint32]),
    "zkp_range_challenge_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_generate_proof_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.POINTER(RangeNiWitness), C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_uint32]),
    "zkp_range_verifier_output_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_generate_encrypted_pairs_seeded_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    "zkp_range_generate_proof_seeded_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_verifier_output_json_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                                         C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_verifier_commit_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint64,
                                                           C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_verifier_reveal_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint64,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_range_verify_commit_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_uint32]),
    "zkp_modinv_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_mul_proof_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 16 + [C.c_uint32]),
    "zkp_mul_proof_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 9 + [C.c_uint32]),
    "zkp_correct_message_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 11 + [C.c_uint32]),
    "zkp_correct_message_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 6 + [C.c_uint32]),
    "zkp_decimal_to_limbs_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    "zkp_decimal_pitch": (C.c_uint32, [C.c_uint32]),
    "zkp_limbs_to_decimal_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "zkp_json_encrypted_pairs_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_uint32]),
    "zkp_json_range_proof_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_uint32]),
    "zkp_json_range_proof_ni_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RangeNiProofs), C.c_void_p, C.c_uint32]),
    "zkp_range_ni_verify_json_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_correct_key_proof_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_correct_key_ni_verify_json_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                         C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_doc_bound": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "zkp_json_write_encrypted_pairs_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_write_range_proof_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_write_range_proof_ni_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_write_correct_key_proof_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_dlog_statement_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_uint32]),
    "zkp_json_dlog_proof_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint32]),
    "zkp_json_write_dlog_statement_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                                        C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_write_dlog_proof_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                                    C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_dlog_verify_json_batch": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_json_sigma_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_uint32]),
    "zkp_json_write_sigma_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                               C.c_uint32]),
    "zkp_sigma_verify_json_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_correct_key_ni_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "zkp_dlog_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_dlog_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_zero_proof_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_zero_proof_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_uint32]),
    "zkp_ciphertext_proof_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_ciphertext_proof_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_nonce_sample_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64,
                                           C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32]),
    "zkp_zero_proof_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_ciphertext_proof_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_correct_message_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                           C.c_char_p, C.c_uint64] + [C.c_void_p] * 5 + [C.c_uint32]),
    "zkp_dlog_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p,
                                                C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_nonce_sample_coprime_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64,
                                                   C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32]),
    "zkp_verlin_proof_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 + [C.c_char_p, C.c_uint64] +
                                            [C.c_void_p] * 6 + [C.c_uint32]),
    "zkp_mul_proof_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 8 + [C.c_char_p, C.c_uint64] +
                                         [C.c_void_p] * 6 + [C.c_uint32]),
    "zkp_jacobi_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_legendre_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_dlog_statement_setup_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_paillier_open_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_uint32]),
    "zkp_correct_key_ni_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_correct_key_challenge_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 + [C.c_uint32]),
    "zkp_correct_key_challenge_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64] +
                                               [C.c_void_p] * 5 + [C.c_uint32]),
    "zkp_correct_key_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint32]),
    "zkp_correct_key_verify_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64,
                                                        C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_probable_prime_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    "zkp_next_prime_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint32]),
    "zkp_paillier_keygen_seeded_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_uint32]),
    "zkp_verlin_proof_prove_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 16 + [C.c_uint32]),
    "zkp_verlin_proof_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 9 + [C.c_uint32]),
    "zkp_multi_create": (C.c_int32, [C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_void_p)]),
    "zkp_multi_destroy": (C.c_int32, [C.c_void_p]),
    "zkp_multi_size": (C.c_uint32, [C.c_void_p]),
    "zkp_multi_ctx": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "zkp_multi_last_error_string": (C.c_char_p, [C.c_void_p]),
    "zkp_multi_last_timing": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zkp_multi_last_phases": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "zkp_ctx_create_on_stream": (C.c_int32, [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "zkp_ctx_set_geometry": (C.c_int32, [C.c_void_p, C.c_int32]),
    "zkp_ctx_last_geometry": (C.c_int32, [C.c_void_p]),
    "zkp_ctx_latency_limbs_per_lane": (C.c_int32, [C.c_void_p]),
    "zkp_multi_set_gather": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "zkp_multi_gathered": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zkp_multi_range_ni_prove_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.POINTER(RangeNiWitness), C.c_void_p, C.c_void_p, C.c_void_p]),
    "zkp_multi_range_ni_prove_seeded_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "zkp_multi_range_ni_verify_batch": (C.c_int32, [C.c_void_p, C.POINTER(RangeNiProofs), C.c_void_p]),
    "zkp_multi_correct_key_ni_verify_batch": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
}

Z1_EXTRA_LIMBS = 16
SEEDED_KIND_ZERO, SEEDED_KIND_CIPHERTEXT, SEEDED_KIND_CORRECT_MESSAGE, SEEDED_KIND_DLOG = 1, 2, 3, 4
SEEDED_KIND_VERLIN, SEEDED_KIND_MUL = 5, 6
SEEDED_KIND_RANGE_COMMIT = 7
SEEDED_KIND_DLOG_SETUP = 8
SEEDED_KIND_CORRECT_KEY = 10
CORRECT_KEY_ROUNDS = 40
CK_PROVE_BAD_KEY = 5          # out_error of correct_key_prove: 1 .. 4 are the reference's CorrectKeyProveError variants
_lib = None


def load():
    """dlopen libzkp_hip.so and attach signatures.  Raises if the library is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        # torch wheels bundle their own libamdhip64 under the same SONAME as /opt/rocm's: whichever is
        # loaded first serves the whole process, and torch refuses to find GPUs behind a foreign one.
        # So when torch is installed, let it load its runtime first (the C ABI itself does not need torch).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in list(EXPORTS.items()) + list(DIAG_EXPORTS.items()):
            fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class DecItem(C.Structure):
    """zkp_dec_item (include/zkp_hip.h)"""
    _fields_ = [("text_off", C.c_uint64), ("dst_off", C.c_uint64), ("len", C.c_uint32), ("words", C.c_uint32)]


DEC_OK, DEC_INVALID, DEC_NEGATIVE, DEC_OVERFLOW = 0, 1, 2, 3
BIGINT_DEC, BIGINT_HEX, BIGINT_BYTES = 0, 1, 2
DOC_OK, DOC_INVALID, DOC_HOST_PATH = 0, 2, 3
GATHER_HOST, GATHER_RCCL, GATHER_COPY = 0, 1, 2
JSON_DOC_ENCRYPTED_PAIRS, JSON_DOC_RANGE_PROOF, JSON_DOC_RANGE_PROOF_NI, JSON_DOC_CORRECT_KEY_PROOF = 0, 1, 2, 3
JSON_DOC_DLOG_PROOF, JSON_DOC_DLOG_STATEMENT = 5, 6
(JSON_DOC_ZERO_STATEMENT, JSON_DOC_ZERO_PROOF, JSON_DOC_CIPHERTEXT_STATEMENT, JSON_DOC_CIPHERTEXT_PROOF, JSON_DOC_VERLIN_STATEMENT, JSON_DOC_VERLIN_PROOF,
 JSON_DOC_MUL_STATEMENT, JSON_DOC_MUL_PROOF) = range(8, 16)
# fields per sigma-proof document kind, in declaration order (a statement's first one is the key)
SIGMA_FIELDS = {8: 2, 9: 2, 10: 2, 11: 3, 12: 4, 13: 5, 14: 4, 15: 5}


class SigmaFields(C.Structure):
    """zkp_sigma_fields"""
    _fields_ = [("f", C.c_void_p * 5)]


def json_doc_bound(doc_kind: int, n_bits: int, error_factor: int = SECURITY_PARAMETER, forms: int = 0) -> int:
    """zkp_json_doc_bound: an upper bound of one written document's length (a pure host function: no GPU, no context)"""
    return load().zkp_json_doc_bound(doc_kind, n_bits, error_factor, forms)


def bigint_forms(key_form: int, bare_form: int) -> int:
    """ZKP_BIGINT_FORMS: the text form of ek.n and of the bare BigInts (range, ciphertext), named separately"""
    return (key_form << 4) | bare_form


class ZkpError(RuntimeError):
    pass


def ptr(a):
    """numpy array / torch tensor / None -> void* address."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    if hasattr(a, "data_ptr"):   # torch tensor (host or device)
        assert a.is_contiguous()
        return a.data_ptr()
    raise TypeError(type(a))


def _seed(seed):
    """32 seed bytes, or None (the library refuses a null seed)"""
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes")
    return seed


class MultiContext:
    """zkp_multi: several device contexts behind one caller (host buffers only)."""

    def __init__(self, device_ids):
        self.lib = load()
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        h = C.c_void_p()
        st = self.lib.zkp_multi_create(ids, len(device_ids), C.byref(h))
        if st != ZKP_OK:
            raise ZkpError(f"zkp_multi_create({list(device_ids)}) failed with status {st} (no CPU fallback)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.zkp_multi_destroy(self.h)
            self.h = None

    __del__ = close

    def check(self, st):
        if st != ZKP_OK:
            msg = self.lib.zkp_multi_last_error_string(self.h)
            raise ZkpError(f"status {st}: {msg.decode() if msg else ''}")

    def size(self):
        return self.lib.zkp_multi_size(self.h)

    def last_timing(self):
        """[(ms, lo, hi)] per device context for the most recent batch call"""
        out = []
        for i in range(self.size()):
            ms, lo, hi = C.c_double(), C.c_uint64(), C.c_uint64()
            self.check(self.lib.zkp_multi_last_timing(self.h, i, C.byref(ms), C.byref(lo), C.byref(hi)))
            out.append((ms.value, lo.value, hi.value))
        return out

    def last_phases(self):
        """[(compute_ms, gather_ms)] per device context for the most recent batch call (HIP events on each context's stream)"""
        out = []
        for i in range(self.size()):
            cm, gm = C.c_double(), C.c_double()
            self.check(self.lib.zkp_multi_last_phases(self.h, i, C.byref(cm), C.byref(gm)))
            out.append((cm.value, gm.value))
        return out

    def set_gather(self, mode: int):
        """GATHER_HOST (per-GPU D2H) or GATHER_RCCL (one grouped ncclAllGather per output inside the library: the whole result
        device-resident on every GPU, host arrays filled from one copy)"""
        self.check(self.lib.zkp_multi_set_gather(self.h, mode))

    def gathered(self, device_index: int, which: int):
        """(device pointer, block stride in bytes, total bytes) of gathered output `which` (0 verdict/status, 1 c1, 2 c2)"""
        p, stride, total = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self.check(self.lib.zkp_multi_gathered(self.h, device_index, which, C.byref(p), C.byref(stride), C.byref(total)))
        return p.value, stride.value, total.value

    def range_ni_prove(self, proofs, wit, out_e=None, out_e_len=None, out_status=None):
        self.check(self.lib.zkp_multi_range_ni_prove_batch(self.h, C.byref(proofs), C.byref(wit), ptr(out_e), ptr(out_e_len), ptr(out_status)))

    def range_ni_prove_seeded(self, proofs, x, r, seed: bytes, first_index: int = 0, out_e=None, out_e_len=None, out_status=None):
        """zkp_multi_range_ni_prove_seeded_batch: the witness is expanded from the 32-byte seed on each context's GPU"""
        self.check(self.lib.zkp_multi_range_ni_prove_seeded_batch(self.h, C.byref(proofs), ptr(x), ptr(r), _seed(seed), first_index,
                                                                  ptr(out_e), ptr(out_e_len), ptr(out_status)))

    def range_ni_verify(self, proofs, out_verdict):
        self.check(self.lib.zkp_multi_range_ni_verify_batch(self.h, C.byref(proofs), ptr(out_verdict)))

    def correct_key_ni_verify(self, n_bits, batch, n, sigma, salt: bytes, out_verdict):
        self.check(self.lib.zkp_multi_correct_key_ni_verify_batch(self.h, n_bits, batch, ptr(n), ptr(sigma), salt, len(salt), ptr(out_verdict)))


class Context:
    """One GPU + one stream (zkp_ctx)."""

    def __init__(self, device_id: int = 0, stream=None):
        """stream: a hipStream_t (integer / pointer) the caller owns, e.g. torch.cuda.current_stream().cuda_stream; default: the
        ctx creates its own"""
        self.lib = load()
        h = C.c_void_p()
        if stream is None:
            st = self.lib.zkp_ctx_create(device_id, C.byref(h))
        else:
            st = self.lib.zkp_ctx_create_on_stream(device_id, C.c_void_p(stream), C.byref(h))
        if st != ZKP_OK:
            raise ZkpError(f"zkp_ctx_create(device {device_id}) failed with status {st} "
                           "(no gfx950 GPU / HIP runtime error; there is no CPU fallback)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.zkp_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def check(self, st):
        if st != ZKP_OK:
            msg = self.lib.zkp_last_error_string(self.h)
            raise ZkpError(f"status {st}: {msg.decode() if msg else ''}")

    def synchronize(self):
        self.check(self.lib.zkp_ctx_synchronize(self.h))

    def set_geometry(self, limbs_per_lane: int):
        """0 = automatic (small calls go to the latency engine), 36 / 9 = always that engine"""
        self.check(self.lib.zkp_ctx_set_geometry(self.h, limbs_per_lane))

    def last_geometry(self) -> int:
        """limbs per lane of the engine the most recent batch call ran on"""
        return self.lib.zkp_ctx_last_geometry(self.h)

    def latency_limbs_per_lane(self) -> int:
        """W of the loaded latency engine (libzkp_hip_lat.so); 0 when it is not there"""
        return self.lib.zkp_ctx_latency_limbs_per_lane(self.h)

    def stream(self):
        return self.lib.zkp_ctx_stream(self.h)

    def timing_reset(self, enable=True):
        self.check(self.lib.zkp_timing_reset(self.h, 1 if enable else 0))

    def timing_get(self):
        ms, launches, modexps = C.c_double(), C.c_uint64(), C.c_uint64()
        self.check(self.lib.zkp_timing_get(self.h, C.byref(ms), C.byref(launches), C.byref(modexps)))
        return ms.value, launches.value, modexps.value

    def diag_table_traffic(self, mode: int, passes: int) -> int:
        """a known amount of window-table traffic (reads: mode 0, writes: mode 1) for PMC calibration -> bytes moved"""
        n = C.c_uint64()
        self.check(self.lib.zkp_diag_table_traffic(self.h, mode, passes, C.byref(n)))
        return n.value

    def set_enc_form(self, form):
        """which Paillier launches run in base-n form (include/zkp_hip_diag.h): "auto" | "n2" | "shared" | "basen" (= always), or the number"""
        self.check(self.lib.zkp_diag_set_enc_form(self.h, ENC_FORMS[form] if isinstance(form, str) else int(form)))

    def set_r2l(self, mode: int):
        """the latency engine's one-Enc-per-wavefront ladder: 0 = never, 1 = the library's rule, 2 = whenever it can run"""
        self.check(self.lib.zkp_diag_set_r2l(self.h, mode))

    def mid_limbs_per_lane(self) -> int:
        """limbs per lane of the mid engine (libzkp_hip_mid.so), 0 when it is not loaded"""
        return self.lib.zkp_diag_mid_limbs_per_lane(self.h)

    def set_split(self, on: bool):
        """calls of 65 ... 96 proofs under one 2048-bit key as two concurrent calls on the mid and the latency engine (on by default)"""
        self.check(self.lib.zkp_diag_set_split(self.h, 1 if on else 0))

    def last_split(self) -> int:
        """proofs of the most recent RangeProofNi call that ran on the latency engine beside the mid engine (0: the call was not split)"""
        return self.lib.zkp_diag_last_split(self.h)

    def set_fuse_hash(self, on: bool):
        """the transcript hashes of a verify as workgroups of its Enc launch (include/zkp_hip_diag.h): taken whenever the call has the
        two-stream shape, fewer proofs than compute units, and its Enc launch on the latency engine's one-Enc-per-wavefront ladder, which
        takes the hashes (1 ... 10 proofs at 128 rows under one 2048-bit key); on by default"""
        self.check(self.lib.zkp_diag_set_fuse_hash(self.h, 1 if on else 0))

    def last_fused_hash(self) -> bool:
        """did the most recent verify call carry its transcript hashes inside its Enc launch (the rule of set_fuse_hash)?"""
        return self.lib.zkp_diag_last_fused_hash(self.h) == 1

    def set_key_cache(self, on: bool):
        """keep the constants of the one key of a shared-key call across calls (include/zkp_hip_diag.h); on by default"""
        self.check(self.lib.zkp_diag_set_key_cache(self.h, 1 if on else 0))

    def key_cache_state(self, which: int):
        """(valid, last set-up launch returned early, set-ups computed so far) of constants buffer `which` on the engine that ran last"""
        out = (C.c_uint32 * 3)()
        self.check(self.lib.zkp_diag_key_cache_state(self.h, which, out))
        return bool(out[0]), bool(out[1]), int(out[2])

    def r2l_last(self) -> bool:
        return self.lib.zkp_diag_r2l_last(self.h) == 1

    def set_r2l_lanes(self, lanes: int):
        """lane geometry of that ladder: 0 = the library's rule, 36 = five wavefronts per Enc (36 lanes x 2 limbs each), 12 / 8 = one wavefront"""
        self.check(self.lib.zkp_diag_set_r2l_lanes(self.h, lanes))

    def r2l_lanes_last(self) -> int:
        """geometry of the most recent launch of the ladder (0: the most recent Paillier launch was not one)"""
        return self.lib.zkp_diag_r2l_lanes_last(self.h)

    def last_host_blocks(self) -> int:
        """proof blocks of the most recent RangeProofNi prove / verify call on host arrays (1: not cut)"""
        return self.lib.zkp_diag_last_host_blocks(self.h)

    def enc_form(self) -> int:
        return self.lib.zkp_diag_enc_form(self.h)

    def diag_basen_last(self):
        """(lanes per n-sized integer of the most recent base-n launch or 0, whether its key qualified for the form)"""
        lanes, ok = C.c_int32(), C.c_uint32()
        self.check(self.lib.zkp_diag_basen_last(self.h, C.byref(lanes), C.byref(ok)))
        return lanes.value, bool(ok.value)

    def diag_basen(self, n_bits: int, n_words, op: int, xa=None, xb=None, ya=None, yb=None):
        """one base-n operation on raw 29-bit limbs (include/zkp_hip_diag.h) -> uint32 array of 4 L + 4 words"""
        import numpy as np
        L = 72 * (n_bits // 2048)
        z = np.zeros(L, np.uint32)
        arrs = [np.ascontiguousarray(z if v is None else v, dtype=np.uint32) for v in (xa, xb, ya, yb)]
        assert all(a.shape == (L,) for a in arrs)
        n_words = np.ascontiguousarray(n_words, dtype=np.uint32)
        out = np.zeros(4 * L + 4, np.uint32)
        self.check(self.lib.zkp_diag_basen(self.h, n_bits, n_words.ctypes.data, op, *[a.ctypes.data for a in arrs], out.ctypes.data))
        return out

    # ---- L1 primitives (buffers: numpy arrays = host pointers, torch cuda tensors = device pointers)
    @staticmethod
    def _flags(*arrs):
        dev = [hasattr(a, "is_cuda") and a.is_cuda for a in arrs if a is not None]
        if any(dev) and not all(dev):
            raise ValueError("all buffers of one call must live in the same memory space")
        return ZKP_F_DEVICE_PTRS if dev and dev[0] else 0

    def modexp(self, mod_bits, exp_bits, count, base, exp, exp_stride, mod, mod_stride, out):
        self.check(self.lib.zkp_modexp_batch(self.h, mod_bits, exp_bits, count, ptr(base), ptr(exp), exp_stride,
                                             ptr(mod), mod_stride, ptr(out), self._flags(base, exp, mod, out)))

    def modmul(self, mod_bits, count, a, b, mod, mod_stride, out):
        self.check(self.lib.zkp_modmul_batch(self.h, mod_bits, count, ptr(a), ptr(b), ptr(mod), mod_stride, ptr(out),
                                             self._flags(a, b, mod, out)))

    def paillier_enc(self, n_bits, count, n, n_stride, m, r, out_c):
        self.check(self.lib.zkp_paillier_enc_batch(self.h, n_bits, count, ptr(n), n_stride, ptr(m), ptr(r), ptr(out_c),
                                                   self._flags(n, m, r, out_c)))

    def paillier_enc_check(self, n_bits, count, n, n_stride, m, r, mulc_a, mulc_b, expected, out_ok):
        """out_ok[i] = Enc(m, r) == expected[i]  (or == mulc_a[i]*mulc_b[i] mod n^2 when expected is None)"""
        self.check(self.lib.zkp_paillier_enc_check_batch(self.h, n_bits, count, ptr(n), n_stride, ptr(m), ptr(r), ptr(mulc_a), ptr(mulc_b),
                                                         ptr(expected), ptr(out_ok), self._flags(n, m, r, mulc_a, mulc_b, expected, out_ok)))

    def release_staging(self):
        self.check(self.lib.zkp_ctx_release_staging(self.h))

    def range_ni_prove(self, proofs: RangeNiProofs, wit: RangeNiWitness, out_e, out_e_len, out_status, device: bool):
        self.check(self.lib.zkp_range_ni_prove_batch(self.h, C.byref(proofs), C.byref(wit), ptr(out_e), ptr(out_e_len),
                                                     ptr(out_status), ZKP_F_DEVICE_PTRS if device else 0))

    def range_sample_witness(self, proofs: RangeNiProofs, seed: bytes, first_index: int, out_w1, out_w2, out_r1, out_r2, out_status, device: bool):
        """zkp_range_sample_witness_batch: rows [0, proofs.error_factor) of the witness a seeded prove uses, expanded from the 32-byte seed
        (always host bytes) for proofs first_index .. first_index + batch - 1"""
        self.check(self.lib.zkp_range_sample_witness_batch(self.h, C.byref(proofs), _seed(seed), first_index, ptr(out_w1), ptr(out_w2), ptr(out_r1),
                                                           ptr(out_r2), ptr(out_status), ZKP_F_DEVICE_PTRS if device else 0))

    def range_ni_prove_seeded(self, proofs: RangeNiProofs, x, r, seed: bytes, first_index: int, out_e, out_e_len, out_status, device: bool):
        """zkp_range_ni_prove_seeded_batch: RangeProofNi::prove from (statement, x, r) and a fresh 32-byte seed; the witness never leaves the GPU"""
        self.check(self.lib.zkp_range_ni_prove_seeded_batch(self.h, C.byref(proofs), ptr(x), ptr(r), _seed(seed), first_index, ptr(out_e),
                                                            ptr(out_e_len), ptr(out_status), ZKP_F_DEVICE_PTRS if device else 0))

    def witness_residue(self) -> int:
        """non-zero words left in the device blocks that held the last seeded call's secrets (zkp_diag_witness_residue); 0 is the only good answer"""
        out = C.c_uint64()
        self.check(self.lib.zkp_diag_witness_residue(self.h, C.byref(out)))
        return out.value

    def range_ni_verify(self, proofs: RangeNiProofs, out_verdict, device: bool):
        self.check(self.lib.zkp_range_ni_verify_batch(self.h, C.byref(proofs), ptr(out_verdict),
                                                      ZKP_F_DEVICE_PTRS if device else 0))

    def correct_key_ni_verify(self, n_bits, batch, n, sigma, salt: bytes, out_verdict):
        sb = (C.c_uint8 * len(salt)).from_buffer_copy(salt) if salt else None
        self.check(self.lib.zkp_correct_key_ni_verify_batch(self.h, n_bits, batch, ptr(n), ptr(sigma),
                                                            C.cast(sb, C.c_void_p) if sb else None, len(salt),
                                                            ptr(out_verdict), self._flags(n, sigma, out_verdict)))

    def correct_key_ni_prove(self, n_bits, batch, p, q, salt: bytes, out_n, out_sigma, out_status=None):
        """zkp_correct_key_ni_prove_batch: one proof per key (p, q), the n-th roots by CRT on the GPU.  p, q: [batch][n_bits / 64];
        out_n (or None): [batch][n_bits / 32]; out_sigma: [batch][11][n_bits / 32]; out_status (or None): 2 where the key is outside
        the domain (its n and roots zero).  numpy arrays, or torch cuda tensors (all of them); the salt is host bytes in both modes."""
        self.check(self.lib.zkp_correct_key_ni_prove_batch(self.h, n_bits, batch, ptr(p), ptr(q), salt if salt else None, len(salt), ptr(out_n),
                                                           ptr(out_sigma), ptr(out_status), self._flags(p, q, out_n, out_sigma, out_status)))

    # ---- the interactive CorrectKey for whole batches of sessions: K rounds each; digests are [batch][8] little-endian words
    def correct_key_challenge(self, n_bits, batch, K, n, n_stride, s, r, out_sn, out_e, out_z, out_s_digest=None, out_status=None):
        """zkp_correct_key_challenge_batch: sn = s^n, e = H(n, sn, r^n), z = r s^e mod n, s_digest = H(s) from the caller's s, r [batch][K][kw];
        out_status (or None): 2 where n is even or 1 (that session's outputs zero)."""
        self.check(self.lib.zkp_correct_key_challenge_batch(self.h, n_bits, batch, K, ptr(n), n_stride, ptr(s), ptr(r), ptr(out_sn), ptr(out_e), ptr(out_z),
                                                            ptr(out_s_digest), ptr(out_status),
                                                            self._flags(n, s, r, out_sn, out_e, out_z, out_s_digest, out_status)))

    def correct_key_challenge_seeded(self, n_bits, batch, K, n, n_stride, seed: bytes, first_index: int, out_sn, out_e, out_z, out_s_digest=None,
                                     out_status=None):
        """zkp_correct_key_challenge_seeded_batch: the same with s, r expanded on the GPU from (seed, first_index + b); the seed is host bytes"""
        self.check(self.lib.zkp_correct_key_challenge_seeded_batch(self.h, n_bits, batch, K, ptr(n), n_stride, _seed(seed), first_index, ptr(out_sn),
                                                                   ptr(out_e), ptr(out_z), ptr(out_s_digest), ptr(out_status),
                                                                   self._flags(n, out_sn, out_e, out_z, out_s_digest, out_status)))

    def correct_key_prove(self, n_bits, batch, K, p, q, sn, e, z, out_s_digest, out_error=None):
        """zkp_correct_key_prove_batch: one answer per key (p, q) [batch][n_bits / 64]; out_error (or None): 0, the reference's error 1 .. 4,
        or 5 for a key outside the domain (the digest is zero then)."""
        self.check(self.lib.zkp_correct_key_prove_batch(self.h, n_bits, batch, K, ptr(p), ptr(q), ptr(sn), ptr(e), ptr(z), ptr(out_s_digest),
                                                        ptr(out_error), self._flags(p, q, sn, e, z, out_s_digest, out_error)))

    def correct_key_verify_seeded(self, n_bits, batch, K, n, n_stride, seed: bytes, first_index: int, proof_s_digest, out_verdict):
        """zkp_correct_key_verify_seeded_batch: the verdict from the s of (seed, first_index + b), regenerated and hashed on the GPU"""
        self.check(self.lib.zkp_correct_key_verify_seeded_batch(self.h, n_bits, batch, K, ptr(n), n_stride, _seed(seed), first_index, ptr(proof_s_digest),
                                                                ptr(out_verdict), self._flags(n, proof_s_digest, out_verdict)))

    def probable_prime(self, bits, count, w, rounds, seed, first_index, out_verdict):
        """zkp_probable_prime_batch: out_verdict[i] = is_probable_prime(w[i]) by the rule of include/zkp_hip.h (trial division by the odd
        primes below 6370, base 2, `rounds` seeded bases).  w: [count][bits / 32]; seed: 32 host bytes, or None when rounds == 0."""
        self.check(self.lib.zkp_probable_prime_batch(self.h, bits, count, ptr(w), rounds, _seed(seed), first_index, ptr(out_verdict),
                                                     self._flags(w, out_verdict)))

    def next_prime(self, bits, count, start, rounds, seed, first_index, out_prime, out_offset=None, out_status=None):
        """zkp_next_prime_batch: the first probable prime among (start | 1) + 2 j, j < 512, below 2^bits; out_offset (or None): j;
        out_status (or None): 2 where the window holds none (prime and offset zero)."""
        self.check(self.lib.zkp_next_prime_batch(self.h, bits, count, ptr(start), rounds, _seed(seed), first_index, ptr(out_prime), ptr(out_offset),
                                                 ptr(out_status), self._flags(start, out_prime, out_offset, out_status)))

    def paillier_keygen_seeded(self, n_bits, batch, rounds, seed, first_index, out_p, out_q, out_n=None, out_status=None):
        """zkp_paillier_keygen_seeded_batch: key b from (seed, first_index + b), primes found on the GPU.  out_p, out_q: [batch][n_bits / 64];
        out_n (or None): [batch][n_bits / 32]; out_status (or None): 2 for a malformed key (p, q, n zero).  The seed is worth the keys."""
        self.check(self.lib.zkp_paillier_keygen_seeded_batch(self.h, n_bits, batch, rounds, _seed(seed), first_index, ptr(out_p), ptr(out_q), ptr(out_n),
                                                             ptr(out_status), self._flags(out_p, out_q, out_n, out_status)))

    def dlog_prove(self, n_bits, y_bits, batch, N, g, ni, secret, r, out_x, out_y):
        self.check(self.lib.zkp_dlog_prove_batch(self.h, n_bits, y_bits, batch, ptr(N), ptr(g), ptr(ni), ptr(secret),
                                                 ptr(r), ptr(out_x), ptr(out_y), self._flags(N, g, ni, out_x)))

    def dlog_verify(self, n_bits, y_bits, batch, N, g, ni, x, y, out_verdict):
        self.check(self.lib.zkp_dlog_verify_batch(self.h, n_bits, y_bits, batch, ptr(N), ptr(g), ptr(ni), ptr(x),
                                                  ptr(y), ptr(out_verdict), self._flags(N, g, ni, x, y, out_verdict)))

    def zero_proof_prove(self, n_bits, batch, n, n_stride, c, r, r_prime, out_z, out_a):
        self.check(self.lib.zkp_zero_proof_prove_batch(self.h, n_bits, batch, ptr(n), n_stride, ptr(c), ptr(r), ptr(r_prime), ptr(out_z), ptr(out_a),
                                                       self._flags(n, c, r, r_prime, out_z, out_a)))

    def zero_proof_verify(self, n_bits, batch, n, n_stride, c, z, a, out_verdict):
        self.check(self.lib.zkp_zero_proof_verify_batch(self.h, n_bits, batch, ptr(n), n_stride, ptr(c), ptr(z), ptr(a), ptr(out_verdict),
                                                        self._flags(n, c, z, a, out_verdict)))

    def ciphertext_proof_prove(self, n_bits, batch, n, n_stride, c, x, r, x_prime, r_prime, out_z1, out_z2, out_c_prime):
        self.check(self.lib.zkp_ciphertext_proof_prove_batch(self.h, n_bits, batch, ptr(n), n_stride, ptr(c), ptr(x), ptr(r), ptr(x_prime), ptr(r_prime),
                                                             ptr(out_z1), ptr(out_z2), ptr(out_c_prime), self._flags(n, c, x, r, out_z1)))

    def ciphertext_proof_verify(self, n_bits, batch, n, n_stride, c, z1, z2, c_prime, out_verdict):
        self.check(self.lib.zkp_ciphertext_proof_verify_batch(self.h, n_bits, batch, ptr(n), n_stride, ptr(c), ptr(z1), ptr(z2), ptr(c_prime),
                                                              ptr(out_verdict), self._flags(n, c, z1, z2, c_prime, out_verdict)))

    # ---- seeded proving of the sigma proofs and CompositeDLogProof: the nonces are expanded from a 32-byte seed (always host bytes) on the GPU
    def nonce_sample(self, kind, n_bits, batch, K, n, n_stride, seed: bytes, first_index: int, out_fields, out_status):
        """zkp_nonce_sample_batch: out_fields = the four arrays by field id (None where the kind has none)"""
        arr = (C.c_void_p * 4)(*[ptr(a) for a in out_fields])
        self.check(self.lib.zkp_nonce_sample_batch(self.h, kind, n_bits, batch, K, ptr(n), n_stride, _seed(seed), first_index, arr, ptr(out_status),
                                                   self._flags(n, *out_fields, out_status)))

    def zero_proof_prove_seeded(self, n_bits, batch, n, n_stride, c, r, seed: bytes, first_index: int, out_z, out_a, out_status=None):
        self.check(self.lib.zkp_zero_proof_prove_seeded_batch(self.h, n_bits, batch, ptr(n), n_stride, ptr(c), ptr(r), _seed(seed), first_index, ptr(out_z),
                                                              ptr(out_a), ptr(out_status), self._flags(n, c, r, out_z, out_a, out_status)))

    def ciphertext_proof_prove_seeded(self, n_bits, batch, n, n_stride, c, x, r, seed: bytes, first_index: int, out_z1, out_z2, out_c_prime, out_status=None):
        self.check(self.lib.zkp_ciphertext_proof_prove_seeded_batch(self.h, n_bits, batch, ptr(n), n_stride, ptr(c), ptr(x), ptr(r), _seed(seed), first_index,
                                                                    ptr(out_z1), ptr(out_z2), ptr(out_c_prime), ptr(out_status),
                                                                    self._flags(n, c, x, r, out_z1, out_z2, out_c_prime, out_status)))

    def correct_message_prove_seeded(self, n_bits, batch, K, n, n_stride, valid, message, seed: bytes, first_index: int, out_ct, out_e_vec, out_z_vec,
                                     out_a_vec, out_status):
        arrs = (valid, message, out_ct, out_e_vec, out_z_vec, out_a_vec, out_status)
        self.check(self.lib.zkp_correct_message_prove_seeded_batch(self.h, n_bits, batch, K, ptr(n), n_stride, ptr(valid), ptr(message), _seed(seed), first_index,
                                                                   *[ptr(x) for x in arrs[2:]], self._flags(n, *arrs)))

    def dlog_prove_seeded(self, n_bits, y_bits, batch, N, g, ni, secret, seed: bytes, first_index: int, out_x, out_y, out_status=None):
        self.check(self.lib.zkp_dlog_prove_seeded_batch(self.h, n_bits, y_bits, batch, ptr(N), ptr(g), ptr(ni), ptr(secret), _seed(seed), first_index,
                                                        ptr(out_x), ptr(out_y), ptr(out_status), self._flags(N, g, ni, secret, out_x, out_y, out_status)))

    # ---- the Jacobi symbol, the reference's legendre_symbol, and the seeded set-up of a DLogStatement (h1 of symbol -1, secret, h2)
    def jacobi(self, mod_bits, count, a, n, n_stride, out_symbol, out_status=None):
        """zkp_jacobi_batch: out_symbol (int32) = (a / n) for odd n; out_status 2 where n is even or zero"""
        self.check(self.lib.zkp_jacobi_batch(self.h, mod_bits, count, ptr(a), ptr(n), n_stride, ptr(out_symbol), ptr(out_status),
                                             self._flags(a, n, out_symbol, out_status)))

    def legendre(self, mod_bits, count, a, p, p_stride, out_symbol, out_status=None):
        """zkp_legendre_batch: the reference's legendre_symbol (Euler's criterion: 1 iff a^((p-1)/2) == 1 mod p, else -1)"""
        self.check(self.lib.zkp_legendre_batch(self.h, mod_bits, count, ptr(a), ptr(p), p_stride, ptr(out_symbol), ptr(out_status),
                                               self._flags(a, p, out_symbol, out_status)))

    def dlog_statement_setup_seeded(self, n_bits, batch, N, seed: bytes, first_index: int, out_g, out_ni, out_secret, out_status=None):
        """zkp_dlog_statement_setup_seeded_batch: g = h1 with (h1 / N) == -1, secret < 2^256, ni = (h1^-1)^secret mod N"""
        self.check(self.lib.zkp_dlog_statement_setup_seeded_batch(self.h, n_bits, batch, ptr(N), _seed(seed), first_index, ptr(out_g), ptr(out_ni),
                                                                  ptr(out_secret), ptr(out_status), self._flags(N, out_g, out_ni, out_secret, out_status)))

    # ---- Paillier decrypt / open with the factors: CRT under p^2, q^2 (and p, q for the randomness)
    def paillier_open(self, n_bits, count, p, q, key_stride, c, out_m, out_r, out_status, device=False):
        """zkp_paillier_open_batch: out_m = Dec(c), out_r = the n-th root of c mod n (None: decrypt only); out_status 2 where the key or the
        ciphertext is outside the domain (outputs zero)"""
        self.check(self.lib.zkp_paillier_open_batch(self.h, n_bits, count, ptr(p), ptr(q), key_stride, ptr(c), ptr(out_m), ptr(out_r), ptr(out_status),
                                                    ZKP_F_DEVICE_PTRS if device else 0))

    # ---- seeded proving of VerlinProof and MulProof: r_a / r_d are redrawn on the GPU until they are coprime to n
    def nonce_sample_coprime(self, kind, n_bits, batch, n, n_stride, seed: bytes, first_index: int, out_fields, out_status):
        """zkp_nonce_sample_coprime_batch: out_fields = the four arrays by field id (None for fields 2 and 3 of Mul)"""
        arr = (C.c_void_p * 4)(*[ptr(a) for a in out_fields])
        self.check(self.lib.zkp_nonce_sample_coprime_batch(self.h, kind, n_bits, batch, ptr(n), n_stride, _seed(seed), first_index, arr, ptr(out_status),
                                                           self._flags(n, *out_fields, out_status)))

    def verlin_proof_prove_seeded(self, n_bits, batch, n, n_stride, c, c_prime, phi_x, witness, seed: bytes, first_index: int, outs, out_status=None):
        """witness = (x, x', x'', r_x); outs = (phi_a, z, z', z'', r_z)"""
        arrs = [c, c_prime, phi_x, *witness]
        self.check(self.lib.zkp_verlin_proof_prove_seeded_batch(self.h, n_bits, batch, ptr(n), n_stride, *[ptr(a) for a in arrs], _seed(seed), first_index,
                                                                *[ptr(a) for a in outs], ptr(out_status), self._flags(n, *arrs, *outs, out_status)))

    def mul_proof_prove_seeded(self, n_bits, batch, n, n_stride, e_a, e_b, e_c, a, b, r_a, r_b, r_c, seed: bytes, first_index: int, out_f, out_z1, out_z2,
                               out_e_d, out_e_db, out_status):
        ins, outs = (e_a, e_b, e_c, a, b, r_a, r_b, r_c), (out_f, out_z1, out_z2, out_e_d, out_e_db, out_status)
        self.check(self.lib.zkp_mul_proof_prove_seeded_batch(self.h, n_bits, batch, ptr(n), n_stride, *[ptr(x) for x in ins], _seed(seed), first_index,
                                                             *[ptr(x) for x in outs], self._flags(n, *ins, *outs)))

    def verlin_proof_prove(self, n_bits, batch, n, n_stride, c, c_prime, phi_x, witness, nonces, outs):
        """witness = (x, x', x'', r_x); nonces = (a, a', a'', r_a); outs = (phi_a, z, z', z'', r_z)"""
        arrs = [c, c_prime, phi_x, *witness, *nonces, *outs]
        self.check(self.lib.zkp_verlin_proof_prove_batch(self.h, n_bits, batch, ptr(n), n_stride, *[ptr(a) for a in arrs], self._flags(n, *arrs)))

    def verlin_proof_verify(self, n_bits, batch, n, n_stride, c, c_prime, phi_x, phi_a, z, zp, zpp, r_z, out_verdict):
        arrs = [c, c_prime, phi_x, phi_a, z, zp, zpp, r_z, out_verdict]
        self.check(self.lib.zkp_verlin_proof_verify_batch(self.h, n_bits, batch, ptr(n), n_stride, *[ptr(a) for a in arrs], self._flags(n, *arrs)))

    def range_challenge(self, proofs, out_e, out_e_len, device: bool):
        """the Fiat-Shamir challenge of (n, c1, c2) alone: out_e [B][32] left aligned, out_e_len [B]"""
        self.check(self.lib.zkp_range_challenge_batch(self.h, C.byref(proofs), ptr(out_e), ptr(out_e_len), ZKP_F_DEVICE_PTRS if device else 0))

    # ---- interactive RangeProof building blocks (challenge supplied by the caller)
    def range_generate_encrypted_pairs(self, proofs, wit, device: bool):
        self.check(self.lib.zkp_range_generate_encrypted_pairs_batch(self.h, C.byref(proofs), C.byref(wit), ZKP_F_DEVICE_PTRS if device else 0))

    def range_generate_proof(self, proofs, wit, e, e_len, out_status, device: bool):
        self.check(self.lib.zkp_range_generate_proof_batch(self.h, C.byref(proofs), C.byref(wit), ptr(e), ptr(e_len), ptr(out_status),
                                                           ZKP_F_DEVICE_PTRS if device else 0))

    def range_verifier_output(self, proofs, e, e_len, out_verdict, device: bool):
        self.check(self.lib.zkp_range_verifier_output_batch(self.h, C.byref(proofs), ptr(e), ptr(e_len), ptr(out_verdict),
                                                            ZKP_F_DEVICE_PTRS if device else 0))

    # ---- the two prover steps from a 32-byte seed (always host bytes): the witness is expanded on the GPU in both and never leaves it
    def range_generate_encrypted_pairs_seeded(self, proofs, seed: bytes, first_index: int = 0, out_status=None, device: bool = False):
        """zkp_range_generate_encrypted_pairs_seeded_batch: c1, c2 of `proofs` (proofs.error_factor rows) from (n, range) and the seed"""
        self.check(self.lib.zkp_range_generate_encrypted_pairs_seeded_batch(self.h, C.byref(proofs), _seed(seed), first_index, ptr(out_status),
                                                                            ZKP_F_DEVICE_PTRS if device else 0))

    def range_generate_proof_seeded(self, proofs, x, r, seed: bytes, first_index: int, e, e_len, out_status=None, device: bool = False):
        """zkp_range_generate_proof_seeded_batch: resp_* of `proofs` from (n, range, x, r), the verifier's challenge and the SAME
        (seed, first_index) that made the encrypted pairs.  One (seed, index) answers one challenge only."""
        self.check(self.lib.zkp_range_generate_proof_seeded_batch(self.h, C.byref(proofs), ptr(x), ptr(r), _seed(seed), first_index, ptr(e), ptr(e_len),
                                                                  ptr(out_status), ZKP_F_DEVICE_PTRS if device else 0))

    def range_verifier_output_json(self, pairs_docs, proof_docs, n_bits: int, ef: int, n, range, ciphertext, e, e_len, device: bool = False,
                                   out_status=None, out_verdict=None):
        """zkp_range_verifier_output_json_batch: EncryptedPairs document b and Proof document b (two lists) -> (status, verdict) bytes, one pair
        per session.  n: [n_bits / 32] or [1][n_bits / 32] (one key for the batch) or [B][n_bits / 32]; range [B][kw], ciphertext [B][2 kw],
        e [B][32], e_len [B].  device: those five and the two outputs are torch cuda tensors (the outputs are made here when not given)."""
        assert len(pairs_docs) == len(proof_docs)
        B = len(pairs_docs)
        buf, off, ln = self._json_docs(list(pairs_docs) + list(proof_docs))
        if out_status is None or out_verdict is None:
            if device:
                import torch
                out_status = torch.zeros(B, dtype=torch.uint8, device="cuda"); out_verdict = torch.zeros(B, dtype=torch.uint8, device="cuda")
            else:
                out_status = np.zeros(B, np.uint8); out_verdict = np.zeros(B, np.uint8)
        kw = n_bits // 32
        words = 0 if n is None else (n.numel() if hasattr(n, "numel") else n.size)
        n_stride = 0 if words <= kw else kw
        a_off, a_len, b_off, b_len = (np.ascontiguousarray(a) for a in (off[:B], ln[:B], off[B:], ln[B:]))
        self.check(self.lib.zkp_range_verifier_output_json_batch(self.h, C.cast(buf, C.c_void_p), ptr(a_off), ptr(a_len), ptr(b_off), ptr(b_len), B, n_bits, ef,
                                                                 ptr(n), n_stride, ptr(range), ptr(ciphertext), ptr(e), ptr(e_len), ptr(out_status),
                                                                 ptr(out_verdict), ZKP_F_DEVICE_PTRS if device else 0))
        return out_status, out_verdict

    # ---- the verifier's commitment to its challenge (RangeProof::verifier_commit / verify_commit) for whole batches of sessions
    def range_verifier_commit_seeded(self, n_bits, batch, n, n_stride, e_len: int, seed: bytes, first_index: int, out_com, out_status=None):
        """zkp_range_verifier_commit_seeded_batch: out_com[b] = Enc(SHA256(e), r) with (r, e) expanded from (seed, first_index + b) on the GPU;
        neither leaves it.  One (seed, index) belongs to one session."""
        self.check(self.lib.zkp_range_verifier_commit_seeded_batch(self.h, n_bits, batch, ptr(n), n_stride, e_len, _seed(seed), first_index, ptr(out_com),
                                                                   ptr(out_status), self._flags(n, out_com, out_status)))

    def range_verifier_reveal_seeded(self, n_bits, batch, n, n_stride, e_len: int, seed: bytes, first_index: int, out_r, out_e, out_status=None):
        """zkp_range_verifier_reveal_seeded_batch: the (r, e) the commit call committed to, from the SAME (n, e_len, seed, first_index):
        out_r [B][kw], out_e [B][32] left aligned.  Only after the prover's encrypted pairs have arrived."""
        self.check(self.lib.zkp_range_verifier_reveal_seeded_batch(self.h, n_bits, batch, ptr(n), n_stride, e_len, _seed(seed), first_index, ptr(out_r),
                                                                   ptr(out_e), ptr(out_status), self._flags(n, out_r, out_e, out_status)))

    def range_verify_commit(self, n_bits, batch, n, n_stride, com, r, e, e_len, out_verdict):
        """zkp_range_verify_commit_batch: out_verdict[b] = ACCEPT iff com[b] == Enc(SHA256(e[b][:e_len[b]]), r[b])"""
        self.check(self.lib.zkp_range_verify_commit_batch(self.h, n_bits, batch, ptr(n), n_stride, ptr(com), ptr(r), ptr(e), ptr(e_len), ptr(out_verdict),
                                                          self._flags(n, com, r, e, e_len, out_verdict)))

    # ---- mod_inv, MulProof
    def modinv(self, mod_bits, count, a, mod, mod_stride, out, out_status):
        self.check(self.lib.zkp_modinv_batch(self.h, mod_bits, count, ptr(a), ptr(mod), mod_stride, ptr(out), ptr(out_status),
                                             self._flags(a, mod, out, out_status)))

    def mul_proof_prove(self, n_bits, batch, n, n_stride, e_a, e_b, e_c, a, b, r_a, r_b, r_c, d, r_d, out_f, out_z1, out_z2, out_e_d, out_e_db, out_status):
        arrs = (e_a, e_b, e_c, a, b, r_a, r_b, r_c, d, r_d, out_f, out_z1, out_z2, out_e_d, out_e_db, out_status)
        self.check(self.lib.zkp_mul_proof_prove_batch(self.h, n_bits, batch, ptr(n), n_stride, *[ptr(x) for x in arrs], self._flags(n, *arrs)))

    def mul_proof_verify(self, n_bits, batch, n, n_stride, e_a, e_b, e_c, f, z1, z2, e_d, e_db, out_verdict):
        arrs = (e_a, e_b, e_c, f, z1, z2, e_d, e_db, out_verdict)
        self.check(self.lib.zkp_mul_proof_verify_batch(self.h, n_bits, batch, ptr(n), n_stride, *[ptr(x) for x in arrs], self._flags(n, *arrs)))

    # ---- CorrectMessageProof
    def correct_message_prove(self, n_bits, batch, K, n, n_stride, valid, message, r, e_sim, z_sim, w, out_ct, out_e_vec, out_z_vec, out_a_vec, out_status):
        arrs = (valid, message, r, e_sim if K > 1 else None, z_sim if K > 1 else None, w, out_ct, out_e_vec, out_z_vec, out_a_vec, out_status)
        self.check(self.lib.zkp_correct_message_prove_batch(self.h, n_bits, batch, K, ptr(n), n_stride, *[ptr(x) for x in arrs],
                                                            self._flags(n, *[x for x in arrs if x is not None])))

    def correct_message_verify(self, n_bits, batch, K, n, n_stride, valid, ct, e_vec, z_vec, a_vec, out_verdict):
        arrs = (valid, ct, e_vec, z_vec, a_vec, out_verdict)
        self.check(self.lib.zkp_correct_message_verify_batch(self.h, n_bits, batch, K, ptr(n), n_stride, *[ptr(x) for x in arrs], self._flags(n, *arrs)))

    # ---- wire format: decimal strings <-> limbs, serde_json documents -> SoA batch
    def decimal_to_limbs(self, text: bytes, items, dst, out_status):
        """items: ctypes array of DecItem (host); dst / out_status: numpy (host) arrays"""
        buf = (C.c_char * len(text)).from_buffer_copy(text)
        self.check(self.lib.zkp_decimal_to_limbs_batch(self.h, C.cast(buf, C.c_void_p), len(text), C.cast(items, C.c_void_p), len(items), ptr(dst),
                                                       dst.size, ptr(out_status), 0))

    def decimal_pitch(self, words):
        return self.lib.zkp_decimal_pitch(words)

    def limbs_to_decimal(self, src):
        """src: numpy [count][words] -> list of decimal strings (bytes)"""
        count, words = src.shape
        pitch = self.decimal_pitch(words)
        out = np.zeros((count, pitch), np.uint8); ln = np.zeros(count, np.uint32)
        self.check(self.lib.zkp_limbs_to_decimal_batch(self.h, ptr(src), words, words, count, ptr(out), pitch, ptr(ln), 0))
        return [bytes(out[i, pitch - ln[i]:]) for i in range(count)]

    def _json_docs(self, docs):
        text = b"".join(docs)
        off = np.zeros(len(docs), np.uint64); ln = np.array([len(d) for d in docs], np.uint64)
        off[1:] = np.cumsum(ln)[:-1]
        buf = (C.c_char * max(len(text), 1)).from_buffer_copy(text or b" ")
        return buf, off, ln

    def json_encrypted_pairs(self, docs, proofs, out_status, device: bool):
        buf, off, ln = self._json_docs(docs)
        self.check(self.lib.zkp_json_encrypted_pairs_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), C.byref(proofs), ptr(out_status),
                                                           ZKP_F_DEVICE_PTRS if device else 0))

    def json_range_proof(self, docs, proofs, out_status, device: bool):
        buf, off, ln = self._json_docs(docs)
        self.check(self.lib.zkp_json_range_proof_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), C.byref(proofs), ptr(out_status),
                                                       ZKP_F_DEVICE_PTRS if device else 0))

    def json_range_proof_ni(self, docs, forms: int, proofs, out_status, device: bool = False):
        """whole RangeProofNi documents -> every field of the batch; forms = bigint_forms(key_form, bare_form): BIGINT_DEC /
        BIGINT_HEX / BIGINT_BYTES for the un-annotated ek.n and, separately, for range / ciphertext.  With a shared key proofs.n is
        the verifier's key (an input).  device: the batch and out_status live in device memory and the documents are tokenised
        there (the documents themselves stay host text)."""
        buf, off, ln = self._json_docs(docs)
        self.check(self.lib.zkp_json_range_proof_ni_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), forms, C.byref(proofs), ptr(out_status),
                                                          ZKP_F_DEVICE_PTRS if device else 0))

    def range_ni_verify_json(self, docs, forms: int, n_bits: int, ef: int, verifier_n=None, device: bool = False, out_status=None, out_verdict=None):
        """zkp_range_ni_verify_json_batch: documents -> (status, verdict) bytes, one pair per document.  verifier_n: numpy [n_bits / 32]
        (RangeProofNi::verify under that key) or None (verify_self).  device: the two outputs are torch cuda tensors (made here
        when not given)."""
        buf, off, ln = self._json_docs(docs)
        B = len(docs)
        if out_status is None or out_verdict is None:
            if device:
                import torch
                out_status = torch.zeros(B, dtype=torch.uint8, device="cuda"); out_verdict = torch.zeros(B, dtype=torch.uint8, device="cuda")
            else:
                out_status = np.zeros(B, np.uint8); out_verdict = np.zeros(B, np.uint8)
        self.check(self.lib.zkp_range_ni_verify_json_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), B, n_bits, ef, forms, ptr(verifier_n),
                                                           ptr(out_status), ptr(out_verdict), ZKP_F_DEVICE_PTRS if device else 0))
        return out_status, out_verdict

    def last_json_scan(self):
        """(documents the device scanner took, documents it left to the host tokeniser) of the most recent scanning call"""
        fast, fb = C.c_uint64(), C.c_uint64()
        self.check(self.lib.zkp_diag_last_json_scan(self.h, C.byref(fast), C.byref(fb)))
        return fast.value, fb.value

    def last_json_scan_ms(self):
        """(upload, scan, convert + merge, verify) milliseconds of the most recent scanning call, between HIP events on the ctx stream"""
        out = (C.c_double * 4)()
        self.check(self.lib.zkp_diag_last_json_scan_ms(self.h, out))
        return tuple(out)

    def json_correct_key_proof(self, docs, n_bits, out_sigma, out_status):
        buf, off, ln = self._json_docs(docs)
        self.check(self.lib.zkp_json_correct_key_proof_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), n_bits, len(docs), ptr(out_sigma),
                                                             ptr(out_status), self._flags(out_sigma, out_status)))

    def correct_key_ni_verify_json(self, docs, n_bits: int, n, salt: bytes, device: bool = False, out_status=None, out_verdict=None):
        """zkp_correct_key_ni_verify_json_batch: NiCorrectKeyProof documents -> (status, verdict) bytes, one pair per document.
        n: [len(docs)][n_bits / 32], one key per document — numpy, or with device a torch cuda tensor like the two outputs (made here
        when not given)."""
        buf, off, ln = self._json_docs(docs)
        B = len(docs)
        if out_status is None or out_verdict is None:
            if device:
                import torch
                out_status = torch.zeros(B, dtype=torch.uint8, device="cuda"); out_verdict = torch.zeros(B, dtype=torch.uint8, device="cuda")
            else:
                out_status = np.zeros(B, np.uint8); out_verdict = np.zeros(B, np.uint8)
        sb = (C.c_uint8 * len(salt)).from_buffer_copy(salt) if salt else None
        self.check(self.lib.zkp_correct_key_ni_verify_json_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), B, n_bits, ptr(n),
                                                                 C.cast(sb, C.c_void_p) if sb else None, len(salt), ptr(out_status), ptr(out_verdict),
                                                                 ZKP_F_DEVICE_PTRS if device else 0))
        return out_status, out_verdict

    # ---- the writers: SoA batch -> serde_json documents (sizing call, one allocation, writing call)
    def _json_write(self, call, batch, out_status):
        """call(text pointer or None, capacity, offsets pointer) -> status.  Returns (text, offsets, status): text a numpy uint8 array
        holding the documents back to back, document b = text[offsets[b]:offsets[b + 1]]"""
        off = np.zeros(batch + 1, np.uint64)
        self.check(call(None, 0, ptr(off)))
        text = np.empty(int(off[batch]), np.uint8)
        if text.size:
            sized = off.copy()
            self.check(call(ptr(text), text.size, ptr(off)))
            assert np.array_equal(sized, off)
        return text, off, out_status

    def json_write_encrypted_pairs(self, proofs: RangeNiProofs, out_status=None, device: bool = False):
        fl = ZKP_F_DEVICE_PTRS if device else 0
        return self._json_write(lambda t, cap, off: self.lib.zkp_json_write_encrypted_pairs_batch(self.h, C.byref(proofs), t, cap, off, ptr(out_status), fl),
                                proofs.batch, out_status)

    def json_write_range_proof(self, proofs: RangeNiProofs, out_status=None, device: bool = False):
        fl = ZKP_F_DEVICE_PTRS if device else 0
        return self._json_write(lambda t, cap, off: self.lib.zkp_json_write_range_proof_batch(self.h, C.byref(proofs), t, cap, off, ptr(out_status), fl),
                                proofs.batch, out_status)

    def json_write_range_proof_ni(self, proofs: RangeNiProofs, forms: int = 0, out_status=None, device: bool = False):
        """whole RangeProofNi documents; forms = bigint_forms(key_form, bare_form), as for json_range_proof_ni"""
        fl = ZKP_F_DEVICE_PTRS if device else 0
        return self._json_write(lambda t, cap, off: self.lib.zkp_json_write_range_proof_ni_batch(self.h, C.byref(proofs), forms, t, cap, off, ptr(out_status), fl),
                                proofs.batch, out_status)

    def json_write_correct_key_proof(self, n_bits: int, batch: int, sigma, out_status=None):
        fl = self._flags(sigma, out_status)
        return self._json_write(lambda t, cap, off: self.lib.zkp_json_write_correct_key_proof_batch(self.h, n_bits, batch, ptr(sigma), t, cap, off, ptr(out_status), fl),
                                batch, out_status)

    # ---- CompositeDLogProof / DLogStatement documents: {"x":X,"y":X} and {"N":X,"g":X,"ni":X}, X in the one form `bare_form` names
    def json_dlog_statement(self, docs, n_bits: int, bare_form: int, out_N, out_g, out_ni, out_status):
        """numpy outputs: tokenised on the host; torch cuda tensors: scanned on the device (the documents stay host text)"""
        buf, off, ln = self._json_docs(docs)
        self.check(self.lib.zkp_json_dlog_statement_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), n_bits, len(docs), bare_form, ptr(out_N), ptr(out_g),
                                                          ptr(out_ni), ptr(out_status), self._flags(out_N, out_g, out_ni, out_status)))

    def json_dlog_proof(self, docs, n_bits: int, y_bits: int, bare_form: int, out_x, out_y, out_status):
        buf, off, ln = self._json_docs(docs)
        self.check(self.lib.zkp_json_dlog_proof_batch(self.h, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), n_bits, y_bits, len(docs), bare_form, ptr(out_x), ptr(out_y),
                                                      ptr(out_status), self._flags(out_x, out_y, out_status)))

    def json_write_dlog_statement(self, n_bits: int, batch: int, N, g, ni, bare_form: int = BIGINT_DEC, out_status=None):
        fl = self._flags(N, g, ni, out_status)
        return self._json_write(lambda t, cap, off: self.lib.zkp_json_write_dlog_statement_batch(self.h, n_bits, batch, ptr(N), ptr(g), ptr(ni), bare_form, t, cap, off,
                                                                                                 ptr(out_status), fl), batch, out_status)

    def json_write_dlog_proof(self, n_bits: int, y_bits: int, batch: int, x, y, bare_form: int = BIGINT_DEC, out_status=None):
        fl = self._flags(x, y, out_status)
        return self._json_write(lambda t, cap, off: self.lib.zkp_json_write_dlog_proof_batch(self.h, n_bits, y_bits, batch, ptr(x), ptr(y), bare_form, t, cap, off,
                                                                                             ptr(out_status), fl), batch, out_status)

    def dlog_verify_json(self, statements, proofs, n_bits: int, y_bits: int, bare_form: int = BIGINT_DEC, device: bool = False, out_status=None, out_verdict=None):
        """zkp_dlog_verify_json_batch: statement b and proof b (two lists of documents) -> (status, verdict) bytes, one pair per pair.
        device: the two outputs are torch cuda tensors (made here when not given)."""
        assert len(statements) == len(proofs)
        B = len(statements)
        buf, off, ln = self._json_docs(list(statements) + list(proofs))
        if out_status is None or out_verdict is None:
            if device:
                import torch
                out_status = torch.zeros(B, dtype=torch.uint8, device="cuda"); out_verdict = torch.zeros(B, dtype=torch.uint8, device="cuda")
            else:
                out_status = np.zeros(B, np.uint8); out_verdict = np.zeros(B, np.uint8)
        s_off, s_len, p_off, p_len = (np.ascontiguousarray(a) for a in (off[:B], ln[:B], off[B:], ln[B:]))
        self.check(self.lib.zkp_dlog_verify_json_batch(self.h, C.cast(buf, C.c_void_p), ptr(s_off), ptr(s_len), ptr(p_off), ptr(p_len), B, n_bits, y_bits, bare_form,
                                                       ptr(out_status), ptr(out_verdict), ZKP_F_DEVICE_PTRS if device else 0))
        return out_status, out_verdict

    # ---- ZeroProof / CiphertextProof / VerlinProof / MulProof documents and their statements (JSON_DOC_ZERO_STATEMENT .. JSON_DOC_MUL_PROOF)
    @staticmethod
    def _sigma_fields(kind, arrs):
        if kind not in SIGMA_FIELDS or len(arrs) != SIGMA_FIELDS[kind]:
            raise ValueError(f"document kind {kind} has {SIGMA_FIELDS.get(kind)} fields, {len(arrs)} given")
        f = SigmaFields()
        for i, a in enumerate(arrs):
            f.f[i] = ptr(a)
        return f

    def json_sigma(self, kind: int, docs, n_bits: int, forms: int, out_fields, out_status):
        """zkp_json_sigma_batch.  out_fields: one array per field of the kind, in declaration order, [len(docs)][words].  numpy outputs:
        tokenised on the host; torch cuda tensors: scanned on the device (the documents stay host text)"""
        buf, off, ln = self._json_docs(docs)
        f = self._sigma_fields(kind, out_fields)
        self.check(self.lib.zkp_json_sigma_batch(self.h, kind, C.cast(buf, C.c_void_p), ptr(off), ptr(ln), n_bits, len(docs), forms, C.byref(f), ptr(out_status),
                                                 self._flags(*out_fields, out_status)))

    def json_write_sigma(self, kind: int, n_bits: int, batch: int, fields, forms: int = 0, out_status=None):
        """zkp_json_write_sigma_batch -> (text, offsets, status) as the other writers; fields: numpy arrays or torch cuda tensors"""
        f = self._sigma_fields(kind, fields)
        fl = self._flags(*fields, out_status)
        return self._json_write(lambda t, cap, off: self.lib.zkp_json_write_sigma_batch(self.h, kind, n_bits, batch, C.byref(f), forms, t, cap, off, ptr(out_status), fl),
                                batch, out_status)

    def sigma_verify_json(self, kind: int, statements, proofs, n_bits: int, forms: int = 0, device: bool = False, out_status=None, out_verdict=None):
        """zkp_sigma_verify_json_batch: kind is the PROOF kind; statement b and proof b (two lists of documents) -> (status, verdict) bytes.
        device: the two outputs are torch cuda tensors (made here when not given)."""
        assert len(statements) == len(proofs)
        B = len(statements)
        buf, off, ln = self._json_docs(list(statements) + list(proofs))
        if out_status is None or out_verdict is None:
            if device:
                import torch
                out_status = torch.zeros(B, dtype=torch.uint8, device="cuda"); out_verdict = torch.zeros(B, dtype=torch.uint8, device="cuda")
            else:
                out_status = np.zeros(B, np.uint8); out_verdict = np.zeros(B, np.uint8)
        s_off, s_len, p_off, p_len = (np.ascontiguousarray(a) for a in (off[:B], ln[:B], off[B:], ln[B:]))
        self.check(self.lib.zkp_sigma_verify_json_batch(self.h, kind, C.cast(buf, C.c_void_p), ptr(s_off), ptr(s_len), ptr(p_off), ptr(p_len), B, n_bits, forms,
                                                        ptr(out_status), ptr(out_verdict), ZKP_F_DEVICE_PTRS if device else 0))
        return out_status, out_verdict
