"""CPU tests of tests/json_sigma_model.py, the yardstick of the sigma-proof document tests: the canonical text is what json.dumps gives for the
obvious dict, write() and read() are inverse, doc_bound() covers the longest document, no one-byte change of a canonical document reads as
another value on the two routes, the documents of mutants() have their statuses, honest proofs made by the oracle are inside the domain rule,
and the new symbols and kinds are declared in the header and in the generated Rust bindings."""
import json
import os
import random
import re

import numpy as np
import pytest

import json_sigma_model as M
from helpers import L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {0x00: "dec", 0x11: "hex", 0x22: "bytes", 0x10: "hexkey-dec"}
KIND_IDS = [M.NAMES[k] for k in M.KINDS]


def values(words, rnd):
    wide = [(1 << (32 * w)) - 1 for w in words]
    lead = [rnd.getrandbits(32 * w - 8) | (1 << (32 * w - 9)) for w in words]
    rand = [rnd.getrandbits(32 * w - rnd.choice((0, 1, 7, 33))) for w in words]
    return [[0] * len(words), wide, lead, rand, [1] + wide[1:], wide[:-1] + [0]]


@pytest.mark.parametrize("forms", FORMS, ids=FORMS.values())
@pytest.mark.parametrize("kind", M.KINDS, ids=KIND_IDS)
def test_canonical_text_is_json_dumps_of_the_obvious_dict(kind, forms):
    for n_bits in (1024, 2048, 4096):
        words = M.field_words(kind, n_bits)
        for v in values(words, random.Random(n_bits + kind + forms)):
            doc = M.write(v, kind, forms)
            assert doc == json.dumps(M.as_dict(v, kind, forms), separators=(",", ":")).encode()
            assert M.canonical(doc, kind, forms, n_bits) and M.scan(doc, kind, forms, n_bits) == v
            assert M.read(doc, kind, forms, n_bits) == (M.DOC_OK, v)
            assert len(doc) <= M.doc_bound(kind, n_bits, forms)
        # the bound is reached by the all-ones document in hex, and is no more than a byte per byte value above it in the byte-array form
        ones = M.write([(1 << (32 * w)) - 1 for w in words], kind, forms)
        if forms == 0x11:
            assert len(ones) == M.doc_bound(kind, n_bits, forms)
        assert M.doc_bound(kind, n_bits, forms) - len(ones) <= len(words)          # (decimal: 2^k - 1 may have one digit less than the pitch allows)


def test_the_text_is_what_the_header_says():
    assert M.write([1234, 5], M.ZERO_STATEMENT, 0x00) == b'{"ek":{"n":"1234"},"c":"5"}'
    assert M.write([1234, 5], M.CIPHERTEXT_STATEMENT, 0x10) == b'{"ek":{"n":"04d2"},"c":"5"}'
    assert M.write([1234, 5], M.ZERO_PROOF, 0x22) == b'{"z":[4,210],"a":[5]}'
    assert M.write([1, 2, 3], M.CIPHERTEXT_PROOF, 0) == b'{"z1":"1","z2":"2","c_prime":"3"}'
    assert M.write([1, 2, 3, 4], M.VERLIN_STATEMENT, 0) == b'{"ek":{"n":"1"},"c":"2","c_prime":"3","phi_x":"4"}'
    assert M.write([1, 2, 3, 4, 5], M.VERLIN_PROOF, 0) == b'{"phi_a":"1","z":"2","z_prime":"3","z_double_prime":"4","r_z":"5"}'
    assert M.write([1, 2, 3, 4], M.MUL_STATEMENT, 0) == b'{"ek":{"n":"1"},"e_a":"2","e_b":"3","e_c":"4"}'
    assert M.write([1, 2, 3, 4, 5], M.MUL_PROOF, 0) == b'{"f":"1","z1":"2","z2":"3","e_d":"4","e_db":"5"}'
    assert M.doc_bound(4, 1024, 0) == M.doc_bound(7, 1024, 0) == M.doc_bound(16, 1024, 0) == M.doc_bound(8, 1536, 0) == M.doc_bound(8, 1024, 0x03) == 0


def agrees(m, kind, forms, n_bits):
    got = M.scan(m, kind, forms, n_bits)
    if got is None:
        return False
    st, ints = M.read(m, kind, forms, n_bits)
    fits = [x if x.bit_length() <= 32 * w else 0 for x, w in zip(got, M.field_words(kind, n_bits))]
    assert st == (M.DOC_OK if fits == got else M.DOC_HOST_PATH) and ints == fits, m
    return True


@pytest.mark.parametrize("forms", FORMS, ids=FORMS.values())
@pytest.mark.parametrize("kind", M.KINDS, ids=KIND_IDS)
def test_one_byte_mutations(kind, forms, monkeypatch):
    """a changed, dropped or doubled byte either makes the document non-canonical (the host tokeniser decides) or leaves a document that both
    routes read to the same integers"""
    monkeypatch.setattr(M, "field_words", lambda k, n_bits: tuple(2 if w != M.N else 1 for _, w in M.FIELDS[k]))     # short fields: every byte is tried
    rnd = random.Random(forms * 8 + kind)
    words = M.field_words(kind, 0)
    for v in ([rnd.getrandbits(32 * w) for w in words], [(1 << (32 * w)) - 1 for w in words]):
        doc = M.write(v, kind, forms)
        assert agrees(doc, kind, forms, 0)
        still = 0
        for at in range(len(doc)):
            for byte in set(b'019afF"\\,:[]{}- xn' + bytes([doc[at] ^ 1, doc[at] ^ 0x20, 0, 0x80])) - {doc[at]}:
                still += agrees(doc[:at] + bytes([byte]) + doc[at + 1:], kind, forms, 0)
            still += agrees(doc[:at] + doc[at + 1:], kind, forms, 0) + agrees(doc[:at] + doc[at:at + 1] + doc[at:], kind, forms, 0)
        assert still > 0


@pytest.mark.parametrize("forms", FORMS, ids=FORMS.values())
@pytest.mark.parametrize("kind", M.KINDS, ids=KIND_IDS)
def test_mutants_have_their_statuses(kind, forms):
    n_bits = 1024
    words = M.field_words(kind, n_bits)
    rnd = random.Random(7 * n_bits + kind + forms)
    ints = [rnd.getrandbits(32 * w - 3) | (1 << (32 * w - 4)) for w in words]
    ms = M.mutants(kind, forms, n_bits, ints)
    assert len({m[0] for m in ms}) == len(ms)
    for name, doc, want in ms:
        st, got = M.read(doc, kind, forms, n_bits)
        assert st == want, (name, doc, st)
        if st == M.DOC_INVALID:
            assert got == [0] * len(words) and not M.canonical(doc, kind, forms, n_bits), name
    by = {n: d for n, d, _ in ms}
    for n in ["canonical", "pretty", "reordered", "unknown field", "escaped key", "trailing space"] + (["key with other fields"] if M.is_statement(kind) else []):
        assert M.read(by[n], kind, forms, n_bits) == (M.DOC_OK, ints), n
    canon = {n for n, d, _ in ms if M.canonical(d, kind, forms, n_bits)}
    assert {"canonical", "zero", "last field fills its width"} <= canon
    assert not canon & {"pretty", "reordered", "unknown field", "escaped key", "trailing space", "truncated", "empty", "negative", "last field far too wide",
                        "upper-case hex", "odd-length hex", "no bytes", "byte 256", "padded past the field", "key with other fields", "key without n", "key not an object"}
    assert {M.DOC_OK, M.DOC_INVALID, M.DOC_HOST_PATH} == {m[2] for m in ms}


def test_the_domain_rule():
    n = 0xF123456789ABCDEF1
    for kind in M.PROOF_KINDS:
        st = [n] + [5] * (len(M.FIELDS[kind - 1]) - 1)
        pf = [7] * len(M.FIELDS[kind])
        assert M.in_domain(kind, st, pf)
        for bad_n in (0, 1, n - 1):
            assert not M.in_domain(kind, [bad_n] + st[1:], [0] * len(pf))
        for i, (_, w) in enumerate(M.FIELDS[kind - 1][1:], 1):
            assert w == M.NN and not M.in_domain(kind, st[:i] + [n * n] + st[i + 1:], pf) and M.in_domain(kind, st[:i] + [n * n - 1] + st[i + 1:], pf)
        for i, (name, w) in enumerate(M.FIELDS[kind]):
            edge = {M.NN: n * n, M.N: n, M.Z: None}[w]
            if edge is None:                                   # the z fields are integers, not residues: any value of the width
                assert M.in_domain(kind, st, pf[:i] + [1 << (32 * 48 - 1)] + pf[i + 1:])
            else:
                assert not M.in_domain(kind, st, pf[:i] + [edge] + pf[i + 1:]) and M.in_domain(kind, st, pf[:i] + [edge - 1] + pf[i + 1:]), name
    # the pair's status: the worse document first, then the domain
    doc = lambda v, k: M.write(v, k, 0)
    assert M.pair_status(M.ZERO_PROOF, doc([n, 5], M.ZERO_STATEMENT), doc([7, 7], M.ZERO_PROOF), 0, 1024) == (M.DOC_OK, [n, 5], [7, 7])
    assert M.pair_status(M.ZERO_PROOF, doc([n + 1, 5], M.ZERO_STATEMENT), doc([7, 7], M.ZERO_PROOF), 0, 1024)[0] == M.DOC_HOST_PATH
    assert M.pair_status(M.ZERO_PROOF, doc([n, 5], M.ZERO_STATEMENT), doc([7, 1 << 2048], M.ZERO_PROOF), 0, 1024)[0] == M.DOC_HOST_PATH
    assert M.pair_status(M.ZERO_PROOF, b"{}", doc([7, 1 << 2048], M.ZERO_PROOF), 0, 1024)[0] == M.DOC_INVALID


def test_honest_proofs_of_the_oracle_are_inside_the_domain():
    import sigma_json_cases as S
    for kind in M.PROOF_KINDS:
        cs = S.honest_pairs(kind, 6)
        for st, pf in zip(cs["st_ints"], cs["pf_ints"]):
            assert M.in_domain(kind, st, pf)
            for forms in FORMS:
                assert M.pair_status(kind, M.write(st, kind - 1, forms), M.write(pf, kind, forms), forms, 1024) == (M.DOC_OK, st, pf)
        assert list(S.oracle_verdicts(kind, cs["st_ints"], cs["pf_ints"], 1024)) == [1] * 6


def test_the_symbols_and_kinds_are_declared_for_c_and_rust():
    header = open(os.path.join(ROOT, "include", "zkp_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "zkp-hip-sys", "src", "lib.rs")).read()
    for sym in ("zkp_json_sigma_batch", "zkp_json_write_sigma_batch", "zkp_sigma_verify_json_batch"):
        assert re.search(r"\bint32_t %s\(zkp_ctx\* ctx, uint32_t (doc|proof)_kind," % sym, header), sym
        assert re.search(r"\bpub fn %s\(" % sym, rust), sym
    kinds = ["ZERO_STATEMENT", "ZERO_PROOF", "CIPHERTEXT_STATEMENT", "CIPHERTEXT_PROOF", "VERLIN_STATEMENT", "VERLIN_PROOF", "MUL_STATEMENT", "MUL_PROOF"]
    for value, name in enumerate(kinds, 8):
        assert re.search(r"#define ZKP_JSON_DOC_%s %du\b" % (name, value), header), name
        assert re.search(r"pub const ZKP_JSON_DOC_%s: u32 = %d;" % (name, value), rust), name
    assert "zkp_sigma_fields" in header and "zkp_sigma_fields" in rust
    assert getattr(M, kinds[0]) == 8 and M.MUL_PROOF == 15
