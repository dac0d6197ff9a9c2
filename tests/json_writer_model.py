"""The documents the GPU writers (zkp_json_write_*_batch) must produce, byte for byte: what serde_json::to_string gives for the
reference's derives (range_proof.rs:32-81, range_proof_ni.rs:36-44, correct_key_ni.rs:35-39, serialize.rs), built from Python
integers with json.dumps(..., separators=(",", ":")).  Responses are the tuples of helpers.responses_from_batch:
("open", w1, r1, w2, r2) | ("mask", j, masked_x, masked_r)."""
import json
import sys

sys.set_int_max_str_digits(0)

BIGINT_DEC, BIGINT_HEX, BIGINT_BYTES = 0, 1, 2      # include/zkp_hip.h: ZKP_BIGINT_*
DOC_PAIRS, DOC_PROOF, DOC_NI, DOC_CK = 0, 1, 2, 3   # ZKP_JSON_DOC_*


def _dumps(v):
    return json.dumps(v, separators=(",", ":")).encode()


def enc_bigint(v, form):
    """an un-annotated BigInt in one of the three forms the reader understands"""
    if form == BIGINT_DEC:
        return str(v)
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return b.hex() if form == BIGINT_HEX else list(b)


def pairs_value(c1, c2):
    return {"c1": [str(v) for v in c1], "c2": [str(v) for v in c2]}


def proof_value(responses):
    rows = []
    for r in responses:
        if r[0] == "open":
            rows.append({"Open": {"w1": str(r[1]), "r1": str(r[2]), "w2": str(r[3]), "r2": str(r[4])}})
        else:
            rows.append({"Mask": {"j": int(r[1]), "masked_x": str(r[2]), "masked_r": str(r[3])}})
    return rows


def pairs_doc(c1, c2):
    return _dumps(pairs_value(c1, c2))


def proof_doc(responses):
    return _dumps(proof_value(responses))


def correct_key_doc(sigma):
    return _dumps({"sigma_vec": [str(v) for v in sigma]})


def range_ni_doc(n, rng, ciphertext, c1, c2, responses, error_factor, key_form=BIGINT_DEC, bare_form=BIGINT_DEC):
    return _dumps({"ek": {"n": enc_bigint(n, key_form)}, "range": enc_bigint(rng, bare_form), "ciphertext": enc_bigint(ciphertext, bare_form),
                   "encrypted_pairs": pairs_value(c1, c2), "proof": proof_value(responses), "error_factor": error_factor})


def forms(key_form, bare_form):
    return (key_form << 4) | bare_form


# ---- documents of a SoA batch (numpy arrays of little-endian 32-bit limbs), for comparing with the writers' text
def limbs_to_int(row):
    return int.from_bytes(row.astype("<u4").tobytes(), "little")


def batch_responses(pb, b):
    """like helpers.responses_from_batch, but j is whatever byte the batch holds"""
    out = []
    for i in range(pb.resp_kind.shape[1]):
        if pb.resp_kind[b, i] == 0:
            out.append(("open",) + tuple(limbs_to_int(getattr(pb, f)[b, i]) for f in ("resp_w1", "resp_r1", "resp_w2", "resp_r2")))
        else:
            out.append(("mask", int(pb.resp_j[b, i]), limbs_to_int(pb.resp_w1[b, i]), limbs_to_int(pb.resp_r1[b, i])))
    return out


def batch_doc(pb, b, kind, key_form=BIGINT_DEC, bare_form=BIGINT_DEC):
    """document b of a host RangeBatch"""
    ef = pb.resp_kind.shape[1]
    if kind in (DOC_PAIRS, DOC_NI):
        c1 = [limbs_to_int(x) for x in pb.c1[b]]; c2 = [limbs_to_int(x) for x in pb.c2[b]]
    if kind == DOC_PAIRS:
        return pairs_doc(c1, c2)
    resp = batch_responses(pb, b)
    if kind == DOC_PROOF:
        return proof_doc(resp)
    n = limbs_to_int(pb.n[0 if pb.n.shape[0] == 1 else b])
    return range_ni_doc(n, limbs_to_int(pb.range[b]), limbs_to_int(pb.ciphertext[b]), c1, c2, resp, ef, key_form, bare_form)


def worst_case_lengths(kind, n_bits, ef, key_form=BIGINT_DEC, bare_form=BIGINT_DEC):
    """lengths of the longest documents of a shape: all-ones limbs with every row Open, with every row Mask, and Mask rows with j = 255"""
    kw = n_bits // 32
    a, c = (1 << (32 * kw)) - 1, (1 << (64 * kw)) - 1
    if kind == DOC_CK:
        return [len(correct_key_doc([a] * 11))]
    if kind == DOC_PAIRS:
        return [len(pairs_doc([c] * ef, [c] * ef))]
    out = []
    for resp in ([("open", a, a, a, a)] * ef, [("mask", 1, a, a)] * ef, [("mask", 255, a, a)] * ef):
        out.append(len(proof_doc(resp)) if kind == DOC_PROOF else len(range_ni_doc(a, a, c, [c] * ef, [c] * ef, resp, ef, key_form, bare_form)))
    return out
