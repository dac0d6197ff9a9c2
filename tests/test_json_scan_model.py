"""CPU tests of the canonical grammar (tests/json_scan_model.py), the acceptance predicate of the device scanner: everything the writers'
model produces is canonical, compact json.dumps of the reader tests' generator is canonical, and every mutation that must send a
document to the host tokeniser is not."""
import itertools
import json

import pytest

import json_scan_cases as K
import json_scan_model as S
import json_writer_model as M
import test_wire_format as WF

FORMS = (S.BIGINT_DEC, S.BIGINT_HEX, S.BIGINT_BYTES)


@pytest.mark.parametrize("ef", [1, 2, 128, 256])
@pytest.mark.parametrize("kinds", ["open", "mask", "mixed"])
def test_writer_model_documents_are_canonical(ef, kinds):
    n_bits = 1024
    for kf, bf in itertools.product(FORMS, FORMS):
        case, pr = K.synthetic(b"model-%d" % ef, n_bits, ef, kinds=kinds)
        doc = M.range_ni_doc(case["n"], case["range"], pr["ciphertext"], pr["c1"], pr["c2"], pr["responses"], ef, kf, bf)
        assert S.is_canonical(doc, n_bits, ef, kf, bf), (kf, bf)
        # the form is part of the grammar: a hex or byte-array head is not a canonical decimal one (an all-digit hex string may be)
        if kf == S.BIGINT_BYTES:
            assert not S.is_canonical(doc, n_bits, ef, S.BIGINT_DEC, bf)


@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_edge_values_are_canonical(n_bits):
    kw = n_bits // 32
    for v in (0, 1, 255, 256, (1 << (32 * kw)) - 1):
        resp = [("open", v, v, v, v), ("mask", 255, v, v), ("mask", 0, v, v)]
        c = (1 << (64 * kw)) - 1 if v else 0
        for kf, bf in itertools.product(FORMS, FORMS):
            assert S.is_canonical(M.range_ni_doc(v, v, c, [c] * 3, [c] * 3, resp, 3, kf, bf), n_bits, 3, kf, bf)


@pytest.mark.parametrize("enc", FORMS)
def test_compact_dumps_of_the_reader_generator_is_canonical(enc):
    n_bits, ef = 1024, 4
    case, pr = K.synthetic(b"generator", n_bits, ef)
    doc = WF.range_ni_document(case, pr, enc, ef)
    assert doc == json.dumps(json.loads(doc), separators=(",", ":")).encode()
    assert S.is_canonical(doc, n_bits, ef, enc, enc)
    assert not S.is_canonical(WF.range_ni_document(case, pr, enc, ef, pretty=True), n_bits, ef, enc, enc)
    assert not S.is_canonical(WF.range_ni_document(case, pr, enc, ef, extra=True), n_bits, ef, enc, enc)


CANONICAL = {"canonical", "j 255", "j 0", "small numbers", "longest numbers", "all nines", "c1 one bit too wide", "longest head numbers", "hex leading zeros",
             "leading zero byte", "upper-case hex"}


@pytest.mark.parametrize("key_enc,enc", [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2)])
def test_mutations_are_not_canonical(key_enc, enc):
    n_bits, ef = 1024, 4
    vs = K.variants(b"mutations", n_bits, ef, key_enc, enc)
    names = [name for name, _ in vs]
    assert len(set(names)) == len(names)
    good = vs[0][1]
    for name, doc in vs:
        want = name in CANONICAL
        if name == "upper-case hex":
            want = doc == good            # (a value without a letter digit is unchanged)
        if name in ("hex leading zeros", "leading zero byte"):
            want = False                  # 1024-bit values fill the field: one more byte is one too many
        assert S.is_canonical(doc, n_bits, ef, key_enc, enc) == want, name
    # a document of the wrong row count is canonical for ITS count only
    fewer = dict(vs)["one row less"]
    assert not S.is_canonical(fewer, n_bits, ef - 1, key_enc, enc) and not S.is_canonical(fewer, n_bits, ef, key_enc, enc)


def test_single_byte_damage_is_never_canonical():
    """every literal byte matters: flipping any one byte of a small canonical document to a neighbour of the grammar's alphabet
    gives a document that is either not canonical or still a document of the grammar with another number in it"""
    n_bits, ef = 1024, 2
    case, pr = K.synthetic(b"damage", n_bits, ef)
    good = WF.range_ni_document(case, pr, S.BIGINT_DEC, ef)
    assert S.is_canonical(good, n_bits, ef)
    for i, ch in enumerate(good):
        for repl in (b" ", b"\\", b"-", b"x"):
            bad = good[:i] + repl + good[i + 1:]
            if bad == good:
                continue
            assert not S.is_canonical(bad, n_bits, ef), (i, repl)
        if not chr(ch).isdigit():
            assert not S.is_canonical(good[:i] + good[i + 1:], n_bits, ef), i
