"""CPU tests of the JSON writers' contract: the Python model of the documents (tests/json_writer_model.py) against the byte-level
statement tests/test_wire_format.py already holds the reader to, and zkp_json_doc_bound — a pure host function of the library,
called here without a GPU — against the model's longest documents."""
import itertools

import pytest

import helpers as H
import json_writer_model as M
import test_wire_format as WF
from helpers import pm, zkp

FORMS = (zkp.BIGINT_DEC, zkp.BIGINT_HEX, zkp.BIGINT_BYTES)


def test_model_constants_are_the_headers():
    assert (M.BIGINT_DEC, M.BIGINT_HEX, M.BIGINT_BYTES) == FORMS
    assert (M.DOC_PAIRS, M.DOC_PROOF, M.DOC_NI, M.DOC_CK) == (zkp.JSON_DOC_ENCRYPTED_PAIRS, zkp.JSON_DOC_RANGE_PROOF, zkp.JSON_DOC_RANGE_PROOF_NI,
                                                             zkp.JSON_DOC_CORRECT_KEY_PROOF)
    assert M.forms(1, 2) == zkp.bigint_forms(1, 2)


@pytest.mark.parametrize("key_form,bare_form", list(itertools.product(FORMS, FORMS)))
def test_model_writes_the_document_the_reader_is_tested_with(key_form, bare_form):
    """a proof made by the Python model of the protocol, as a whole RangeProofNi document: same bytes as range_ni_document"""
    n_bits = 1024
    c = H.build_range_case(b"writer-model", [H.test_key(1024)[2]], n_bits, 1)[0]
    ct = pm.enc(c["n"], c["x"], c["r"])
    pr = pm.range_ni_prove(c["n"], c["range"], ct, c["x"], c["r"], c["w1"], c["w2"], c["r1"], c["r2"])
    pr["ciphertext"] = ct
    want = WF.range_ni_document(c, pr, bare_form, 128, key_enc=key_form)
    got = M.range_ni_doc(c["n"], c["range"], ct, pr["c1"], pr["c2"], pr["responses"], 128, key_form, bare_form)
    assert got == want
    assert M.pairs_doc(pr["c1"], pr["c2"]) == WF.pairs_json(pr["c1"], pr["c2"])
    assert M.proof_doc(pr["responses"]) == WF.proof_json(pr["responses"])
    for v in (0, 1, 255, 256, c["n"]):
        assert M.enc_bigint(v, bare_form) == WF._enc_bigint(v, bare_form)


@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_doc_bound_covers_the_longest_documents_and_is_tight(n_bits):
    """zkp_json_doc_bound >= every worst case of the model, and at most 1.1 x the largest of them (a cap against a lazy
    pitch-per-number bound; the all-Open document attains the bound up to the digits of j)"""
    lib = zkp.load()
    assert "zkp_json_doc_bound" in zkp.EXPORTS
    for ef in (1, 4, 40, 128, 256):
        for kind in (M.DOC_PAIRS, M.DOC_PROOF):
            worst = M.worst_case_lengths(kind, n_bits, ef)
            bound = lib.zkp_json_doc_bound(kind, n_bits, ef, 0)
            assert max(worst) <= bound <= 1.1 * max(worst), (kind, ef, worst, bound)
        for kf, bf in itertools.product(FORMS, FORMS):
            worst = M.worst_case_lengths(M.DOC_NI, n_bits, ef, kf, bf)
            bound = zkp.json_doc_bound(M.DOC_NI, n_bits, ef, zkp.bigint_forms(kf, bf))
            assert max(worst) <= bound <= 1.1 * max(worst), (ef, kf, bf, worst, bound)
    worst = M.worst_case_lengths(M.DOC_CK, n_bits, 0)
    bound = lib.zkp_json_doc_bound(M.DOC_CK, n_bits, 0, 0)
    assert max(worst) <= bound <= 1.1 * max(worst)


def test_doc_bound_refuses_what_no_writer_accepts():
    lib = zkp.load()
    assert lib.zkp_json_doc_bound(M.DOC_NI, 512, 128, 0) == 0
    assert lib.zkp_json_doc_bound(4, 2048, 128, 0) == 0
    assert lib.zkp_json_doc_bound(M.DOC_NI, 2048, 128, zkp.bigint_forms(3, 0)) == 0
    assert lib.zkp_json_doc_bound(M.DOC_PROOF, 2048, 0, 0) == 0


def test_python_binding_lists_the_writers():
    for name in ("zkp_json_doc_bound", "zkp_json_write_encrypted_pairs_batch", "zkp_json_write_range_proof_batch",
                 "zkp_json_write_range_proof_ni_batch", "zkp_json_write_correct_key_proof_batch"):
        assert name in zkp.EXPORTS
    for helper in ("json_write_encrypted_pairs", "json_write_range_proof", "json_write_range_proof_ni", "json_write_correct_key_proof"):
        assert hasattr(zkp.Context, helper)
