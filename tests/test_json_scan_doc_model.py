"""tests/json_scan_doc_model.py — the statement of the grammars the device scanner takes for NiCorrectKeyProof, EncryptedPairs and Proof
documents — against the writer's model (tests/json_writer_model.py) and against Python's json + int: what the model takes, Python
reads as the same numbers; one changed byte either sends the document to the host tokeniser or changes one digit."""
import json

import pytest

import json_scan_doc_model as D
import json_writer_model as M

N_BITS, EF = 1024, 2
SUBSTITUTES = b'09",:[]{} -a'
DIGITS = b"0123456789"

SIGMAS = [0, 7, 10, 255, 1 << 40, 3, 99, 12345678901234567890, 5, 1, 42]
DOCS = [
    ("ck", D.DOC_CK, M.correct_key_doc(SIGMAS)),
    ("pairs", D.DOC_PAIRS, M.pairs_doc([0, 918], [77, 1 << 70])),
    ("proof-open-mask", D.DOC_PROOF, M.proof_doc([("open", 1, 20, 300, 0), ("mask", 25, 6, 78)])),
    ("proof-mask-open", D.DOC_PROOF, M.proof_doc([("mask", 1, 0, 9), ("open", 11, 2, 3, 4444)])),
    ("proof-mask-mask", D.DOC_PROOF, M.proof_doc([("mask", 0, 5, 6), ("mask", 255, 7, 8)])),
]
IDS = [d[0] for d in DOCS]


def python_parse(kind, doc):
    """-> (numbers in document order, rows) as serde would see them, or None where json / int / the shape refuse"""
    try:
        v = json.loads(doc)
        if kind == D.DOC_CK:
            return [int(s) for s in v["sigma_vec"]], []
        if kind == D.DOC_PAIRS:
            return [int(s) for s in v["c1"] + v["c2"]], []
        numbers, rows = [], []
        for row in v:
            (variant, body), = row.items()
            if variant == "Open":
                numbers += [int(body[f]) for f in ("w1", "r1", "w2", "r2")]
                rows.append((False, 0))
            else:
                numbers += [int(body[f]) for f in ("masked_x", "masked_r")]
                rows.append((True, body["j"]))
        return numbers, rows
    except (ValueError, KeyError, TypeError, AttributeError):
        return None


def model_values(kind, doc):
    spans = D.scan(kind, doc, N_BITS, EF)
    if spans is None:
        return None
    return [int(doc[p:p + n]) for p, n in spans], (D.rows(doc, N_BITS, EF) if kind == D.DOC_PROOF else [])


@pytest.mark.parametrize("name,kind,doc", DOCS, ids=IDS)
def test_the_model_takes_what_the_writer_writes(name, kind, doc):
    got = model_values(kind, doc)
    assert got is not None and got == python_parse(kind, doc)
    spans = D.scan(kind, doc, N_BITS, EF)
    assert all(doc[p - 1:p] == b'"' and doc[p + n:p + n + 1] == b'"' and doc[p:p + n].isdigit() for p, n in spans)
    assert len(spans) == {D.DOC_CK: 11, D.DOC_PAIRS: 2 * EF}.get(kind, len(spans))
    assert len(doc) <= D.doc_bound(kind, N_BITS, EF)


@pytest.mark.parametrize("name,kind,doc", DOCS, ids=IDS)
def test_one_substituted_byte_falls_back_or_changes_a_digit(name, kind, doc):
    taken = 0
    for at in range(len(doc)):
        for sub in SUBSTITUTES:
            if doc[at] == sub:
                continue
            changed = doc[:at] + bytes([sub]) + doc[at + 1:]
            got = model_values(kind, changed)
            if got is None:
                continue
            taken += 1
            assert doc[at] in DIGITS and sub in DIGITS, (at, chr(sub))
            assert got == python_parse(kind, changed), (at, chr(sub))
    assert taken > 0


@pytest.mark.parametrize("name,kind,doc", DOCS, ids=IDS)
def test_another_length_falls_back(name, kind, doc):
    assert D.scan(kind, doc[:-1], N_BITS, EF) is None
    for extra in SUBSTITUTES:
        assert D.scan(kind, doc + bytes([extra]), N_BITS, EF) is None
    assert D.scan(kind, b"", N_BITS, EF) is None


def test_a_number_fills_its_field_and_no_more():
    dn, dc = D.max_digits(N_BITS // 32), D.max_digits(N_BITS // 16)
    ck = M.correct_key_doc(SIGMAS).replace(b'"7"', b'"' + b"0" * (dn - 1) + b'7"')
    assert model_values(D.DOC_CK, ck) == (SIGMAS, [])
    assert D.scan(D.DOC_CK, M.correct_key_doc(SIGMAS).replace(b'"7"', b'"' + b"0" * dn + b'7"'), N_BITS) is None
    pairs = M.pairs_doc([0, 918], [77, 5]).replace(b'"918"', b'"' + b"0" * (dc - 3) + b'918"')
    assert model_values(D.DOC_PAIRS, pairs) == ([0, 918, 77, 5], [])
    assert D.scan(D.DOC_PAIRS, pairs.replace(b'"0"', b'"00"', 1).replace(b'0918"', b'00918"'), N_BITS, EF) is None
    # other counts
    assert D.scan(D.DOC_CK, M.correct_key_doc(SIGMAS[:10]), N_BITS) is None and D.scan(D.DOC_CK, M.correct_key_doc(SIGMAS + [1]), N_BITS) is None
    assert D.scan(D.DOC_PAIRS, M.pairs_doc([1, 2, 3], [4, 5, 6]), N_BITS, EF) is None
    assert D.scan(D.DOC_PROOF, M.proof_doc([("open", 1, 2, 3, 4)]), N_BITS, EF) is None and D.scan(D.DOC_PROOF, b"[]", N_BITS, EF) is None
