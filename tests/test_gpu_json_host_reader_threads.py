"""The flags-0 readers of EncryptedPairs, Proof and NiCorrectKeyProof documents past one parser thread.  The host tokeniser
(csrc/json_host.hpp: for_docs) uses one thread below 64 documents and up to sixteen from there on, each with a buffer of its own for the
decoded copies of strings that had escapes; the buffers follow the documents' text on the device, thread k's at its own base.  Every
other test with an escape in a number has fewer than 64 documents, so only thread 0's buffer is ever used there.

96 documents at 1024-bit keys, host pointers, flags 0.  In every third document one digit of one number is written as \\u003X, so every
thread's slice holds some; in two slices such a document is followed directly by a malformed one that has appended to the thread's buffer
before it fails (an escape, then the last byte cut), and the next escaped document of the slice takes the space it gave back.  Expected
limbs: int_to_limbs of the integers the documents were built from; expected statuses: from the construction.

These tests are about text: they run on a context of their own with the library's routing."""
import json
import random

import numpy as np
import pytest

from helpers import L, zkp

pytestmark = pytest.mark.gpu
N_BITS, KW, B, EF, M2 = 1024, 32, 96, 2, 11
MALFORMED = (7, 91)            # each directly behind an escaped document (6, 90), in the slices of two threads other than thread 0


@pytest.fixture(scope="module")
def tctx():
    c = zkp.Context(0)
    yield c
    c.close()


def dumps(o):
    return json.dumps(o, separators=(",", ":")).encode()


def escape_one_digit(doc, number, at):
    """`number` (an int that the document holds as a decimal string) with digit `at` written as \\u003X"""
    s = str(number)
    at %= len(s)
    esc = s[:at] + "\\u003" + s[at] + s[at + 1:]
    assert doc.count(b'"' + s.encode() + b'"') == 1
    return doc.replace(b'"' + s.encode() + b'"', b'"' + esc.encode() + b'"')


def finish(docs, numbers):
    """the escapes and the two malformed documents; -> (documents, statuses)"""
    status = [zkp.DOC_OK] * B
    for b in range(B):
        if b % 3 == 0 or b in MALFORMED:
            docs[b] = escape_one_digit(docs[b], numbers[b][b % len(numbers[b])], 5 * b)
        if b in MALFORMED:
            docs[b] = docs[b][:-1]
            status[b] = zkp.DOC_INVALID
    assert all(b - 1 not in MALFORMED and (b - 1) % 3 == 0 and (b + 2) % 3 == 0 for b in MALFORMED)
    return docs, status


def test_encrypted_pairs_from_every_parser_thread(tctx):
    rnd = random.Random(1)
    c1 = [[rnd.getrandbits(64 * KW) for _ in range(EF)] for _ in range(B)]
    c2 = [[rnd.getrandbits(64 * KW) for _ in range(EF)] for _ in range(B)]
    docs = [dumps({"c1": [str(v) for v in c1[b]], "c2": [str(v) for v in c2[b]]}) for b in range(B)]
    docs, status = finish(docs, [c1[b] + c2[b] for b in range(B)])
    pg = zkp.RangeBatch(N_BITS, B, EF, shared_key=True)
    pg.c1[:] = 0xA5A5A5A5; pg.c2[:] = 0xA5A5A5A5
    st = np.full(B, 9, np.uint8)
    tctx.json_encrypted_pairs(docs, pg.struct(), st, device=False)
    assert list(st) == status
    for b in MALFORMED:
        c1[b] = [0] * EF; c2[b] = [0] * EF
    assert np.array_equal(pg.c1, L.ints_to_limbs(c1, 2 * KW)) and np.array_equal(pg.c2, L.ints_to_limbs(c2, 2 * KW))


def test_proof_from_every_parser_thread(tctx):
    rnd = random.Random(2)
    top = 1 << (32 * KW)
    rows = [[("open", rnd.randrange(top), rnd.randrange(top), rnd.randrange(top), rnd.randrange(top)), ("mask", 1 + b % 2, rnd.randrange(top), rnd.randrange(top))]
            for b in range(B)]
    docs = [dumps([{"Open": dict(zip(("w1", "r1", "w2", "r2"), map(str, r[0][1:])))}, {"Mask": {"j": r[1][1], "masked_x": str(r[1][2]), "masked_r": str(r[1][3])}}])
            for r in rows]
    docs, status = finish(docs, [list(r[0][1:]) + list(r[1][2:]) for r in rows])
    pg = zkp.RangeBatch(N_BITS, B, EF, shared_key=True)
    for a in (pg.resp_w1, pg.resp_r1, pg.resp_w2, pg.resp_r2):
        a[:] = 0xA5A5A5A5
    pg.resp_kind[:] = 9; pg.resp_j[:] = 9
    st = np.full(B, 9, np.uint8)
    tctx.json_range_proof(docs, pg.struct(), st, device=False)
    assert list(st) == status
    ok = [s == zkp.DOC_OK for s in status]
    want = lambda f: L.ints_to_limbs([[f(r[0]), f(r[1])] if good else [0, 0] for r, good in zip(rows, ok)], KW)
    assert np.array_equal(pg.resp_w1, want(lambda r: r[1] if r[0] == "open" else r[2]))          # Open: w1, r1, w2, r2; Mask: masked_x, masked_r, 0, 0
    assert np.array_equal(pg.resp_r1, want(lambda r: r[2] if r[0] == "open" else r[3]))
    assert np.array_equal(pg.resp_w2, want(lambda r: r[3] if r[0] == "open" else 0))
    assert np.array_equal(pg.resp_r2, want(lambda r: r[4] if r[0] == "open" else 0))
    assert pg.resp_kind.tolist() == [[zkp.RESP_OPEN, zkp.RESP_MASK] if good else [0, 0] for good in ok]
    assert pg.resp_j.tolist() == [[0, r[1][1]] if good else [0, 0] for r, good in zip(rows, ok)]


def test_correct_key_proof_from_every_parser_thread(tctx):
    rnd = random.Random(3)
    sigma = [[rnd.getrandbits(32 * KW) for _ in range(M2)] for _ in range(B)]
    docs = [dumps({"sigma_vec": [str(v) for v in s]}) for s in sigma]
    docs, status = finish(docs, sigma)
    out = np.full((B, M2, KW), 0xA5A5A5A5, np.uint32)
    st = np.full(B, 9, np.uint8)
    tctx.json_correct_key_proof(docs, N_BITS, out, st)
    assert list(st) == status
    for b in MALFORMED:
        sigma[b] = [0] * M2
    assert np.array_equal(out, L.ints_to_limbs(sigma, KW))
