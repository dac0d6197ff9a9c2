"""CPU tests of tests/json_dlog_model.py, the yardstick of the DLog document tests: write() and read() are inverse, write() is canonical,
no one-byte change of a canonical document is still canonical AND another value, and the documents of mutants() have the statuses they
are listed with."""
import random

import pytest

import json_dlog_model as D

FORMS = {D.BIGINT_DEC: "dec", D.BIGINT_HEX: "hex", D.BIGINT_BYTES: "bytes"}
KINDS = {D.PROOF: "proof", D.STATEMENT: "statement"}
SHAPES = [(1024, 544), (2048, 768)]


def values(kind, words, rnd):
    """value tuples that exercise every field: zero, a leading 00 byte (the top byte of the width is zero), the widest value, random ones"""
    wide = [(1 << (32 * w)) - 1 for w in words]
    lead = [rnd.getrandbits(32 * w - 8) | (1 << (32 * w - 9)) for w in words]
    rand = [rnd.getrandbits(32 * w - rnd.choice((0, 1, 7, 33))) for w in words]
    return [[0] * len(words), wide, lead, rand, [1] + wide[1:], wide[:-1] + [0]]


@pytest.mark.parametrize("form", FORMS, ids=FORMS.values())
@pytest.mark.parametrize("kind", KINDS, ids=KINDS.values())
@pytest.mark.parametrize("n_bits,y_bits", SHAPES)
def test_write_is_canonical_and_read_inverts_it(n_bits, y_bits, kind, form):
    words = D.field_words(kind, n_bits, y_bits)
    rnd = random.Random(n_bits + kind + form)
    for v in values(kind, words, rnd):
        doc = D.write(v, kind, form)
        assert D.canonical(doc, kind, form, words), doc
        assert D.read(doc, kind, form, words) == (D.DOC_OK, v)
        # one bit more than the field carries: no longer canonical in hex / bytes, a HOST_PATH value in every form
        for i, w in enumerate(words):
            over = list(v); over[i] = 1 << (32 * w)
            d2 = D.write(over, kind, form)
            st, got = D.read(d2, kind, form, words)
            assert st == D.DOC_HOST_PATH and got == [0 if k == i else x for k, x in enumerate(v)]
            if form != D.BIGINT_DEC:
                assert not D.canonical(d2, kind, form, words)
    assert D.write([0] * len(words), kind, form) == {D.BIGINT_DEC: b'"0"', D.BIGINT_HEX: b'"00"', D.BIGINT_BYTES: b"[0]"}[form].join(
        [b"{" + b'"%s":' % D.FIELDS[kind][0].encode()] + [b',"%s":' % n.encode() for n in D.FIELDS[kind][1:]] + [b""]) + b"}"


def test_the_text_forms_are_what_the_header_says():
    assert D.write([1234, 5], D.PROOF, D.BIGINT_DEC) == b'{"x":"1234","y":"5"}'
    assert D.write([1234, 5], D.PROOF, D.BIGINT_HEX) == b'{"x":"04d2","y":"05"}'
    assert D.write([1234, 5, 0], D.STATEMENT, D.BIGINT_BYTES) == b'{"N":[4,210],"g":[5],"ni":[0]}'


def agrees(m, kind, form, words):
    """a document the scanner reads itself is read to the integers the tolerant reader gives (zero where the field overflows)"""
    got = D.scan(m, kind, form, words)
    if got is None:
        return False
    st, ints = D.read(m, kind, form, words)
    fits = [x if x.bit_length() <= 32 * w else 0 for x, w in zip(got, words)]
    assert st == (D.DOC_OK if fits == got else D.DOC_HOST_PATH) and ints == fits, m
    return True


@pytest.mark.parametrize("form", FORMS, ids=FORMS.values())
@pytest.mark.parametrize("kind", KINDS, ids=KINDS.values())
def test_one_byte_mutations(kind, form):
    """a changed, dropped or doubled byte either makes the document non-canonical (the host tokeniser decides) or leaves a document that both
    routes read to the same integers: the device scanner never reads a canonical-looking document as another value than the tolerant
    reader does"""
    words = (2, 1) if kind == D.PROOF else (2, 2, 2)          # short fields: every byte position of the document is tried
    rnd = random.Random(form * 8 + kind)
    for v in ([rnd.getrandbits(32 * w) for w in words], [0] * len(words), [(1 << (32 * w)) - 1 for w in words]):
        doc = D.write(v, kind, form)
        assert agrees(doc, kind, form, words)
        still = 0
        for at in range(len(doc)):
            for byte in set(b'0159afAF"\\,:[]{}- xgN' + bytes([doc[at] ^ 1, doc[at] ^ 0x20, 0, 0x80])) - {doc[at]}:
                still += agrees(doc[:at] + bytes([byte]) + doc[at + 1:], kind, form, words)
            still += agrees(doc[:at] + doc[at + 1:], kind, form, words) + agrees(doc[:at] + doc[at:at + 1] + doc[at:], kind, form, words)
        assert still > 0                                       # (a digit that became another digit)


@pytest.mark.parametrize("form", FORMS, ids=FORMS.values())
@pytest.mark.parametrize("kind", KINDS, ids=KINDS.values())
@pytest.mark.parametrize("n_bits,y_bits", SHAPES)
def test_mutants_have_their_statuses(n_bits, y_bits, kind, form):
    words = D.field_words(kind, n_bits, y_bits)
    rnd = random.Random(7 * n_bits + kind + form)
    ints = [rnd.getrandbits(32 * w - 3) | (1 << (32 * w - 4)) for w in words]
    ms = D.mutants(kind, form, words, ints)
    names = [m[0] for m in ms]
    assert len(set(names)) == len(names)
    for name, doc, want in ms:
        st, got = D.read(doc, kind, form, words)
        assert st == want, (name, doc, st)
        if st == D.DOC_INVALID:
            assert got == [0] * len(words) and not D.canonical(doc, kind, form, words), name
    by = {n: d for n, d, _ in ms}
    same = ["canonical", "pretty", "reordered", "unknown field", "escaped key", "trailing space"]
    same += {D.BIGINT_DEC: ["leading zeros", "padded to the field", "padded past the field"], D.BIGINT_HEX: ["upper-case hex", "odd-length hex", "hex leading zero byte"],
             D.BIGINT_BYTES: ["leading zero byte"]}[form]
    for n in same:
        assert D.read(by[n], kind, form, words) == (D.DOC_OK, ints), n
    canon = {n for n, d, _ in ms if D.canonical(d, kind, form, words)}
    assert {"canonical", "zero", "last field fills its width"} <= canon
    assert not canon & {"pretty", "reordered", "unknown field", "escaped key", "trailing space", "truncated", "empty", "sign", "last field far too wide", "upper-case hex",
                        "odd-length hex", "no bytes", "byte 256", "byte 01", "padded past the field"}
    # y of exactly y_bits bits is a value of the layout; one bit more is the caller's host path
    if kind == D.PROOF:
        assert D.read(by["last field fills its width"], kind, form, words) == (D.DOC_OK, [ints[0], (1 << y_bits) - 1])
        assert D.read(by["last field one bit too wide"], kind, form, words) == (D.DOC_HOST_PATH, [ints[0], 0])
