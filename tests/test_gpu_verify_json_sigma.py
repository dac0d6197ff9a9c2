"""GPU tests of zkp_sigma_verify_json_batch: ZeroProof, CiphertextProof, VerlinProof and MulProof::verify on (statement, proof) document
pairs.  Statuses are the model's (tests/json_sigma_model.py: the worse of the two documents, then the domain rule — an odd key of at least
two bits, every 2 kw field below n^2, MulProof.f below n, else ZKP_DOC_HOST_PATH), verdicts the oracle's on the parsed values of the pairs
that are OK and REJECT everywhere else."""
import functools

import numpy as np
import pytest

import json_sigma_model as M
import sigma_json_cases as S
from helpers import zkp

pytestmark = pytest.mark.gpu
OK, INVALID, HOST = zkp.DOC_OK, zkp.DOC_INVALID, zkp.DOC_HOST_PATH
ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED
N_BITS = 1024
KIND_IDS = [M.NAMES[k] for k in M.PROOF_KINDS]
# one text form per proof type in the large batch; every form in the small one
WIDE_FORMS = {M.ZERO_PROOF: 0x00, M.CIPHERTEXT_PROOF: 0x11, M.VERLIN_PROOF: 0x22, M.MUL_PROOF: 0x10}


@pytest.fixture(scope="module")
def sctx():
    c = zkp.Context(0)
    yield c
    c.close()


def expected(kind, statements, proofs, forms):
    """statuses from the model; verdicts from the oracle on the pairs that are OK, REJECT elsewhere"""
    got = [M.pair_status(kind, s, p, forms, N_BITS) for s, p in zip(statements, proofs)]
    status = [g[0] for g in got]
    ok = [b for b, st in enumerate(status) if st == OK]
    verdict = [REJECT] * len(got)
    if ok:
        for b, v in zip(ok, S.oracle_verdicts(kind, [got[b][1] for b in ok], [got[b][2] for b in ok], N_BITS)):
            verdict[b] = int(v)
    return status, verdict


def run(ctx, kind, statements, proofs, forms, device):
    st, v = ctx.sigma_verify_json(kind, statements, proofs, N_BITS, forms, device=device)
    if device:
        ctx.synchronize()
        st, v = st.cpu().numpy(), v.cpu().numpy()
    return [int(x) for x in st], [int(x) for x in v]


# ------------------------------------------------------------------ 1. a batch past one block
@pytest.mark.parametrize("kind", M.PROOF_KINDS, ids=KIND_IDS)
def test_batch_past_one_block(sctx, kind):
    """300 pairs under 300 distinct keys (k_sigma_hash and the compare kernels take 256 proofs per block), every tenth tampered in one field"""
    B, forms = 300, WIDE_FORMS[kind]
    cs = S.honest_pairs(kind, B, True)
    assert len({r[0] for r in cs["st_ints"]}) == B
    st_ints, pf_ints = [list(r) for r in cs["st_ints"]], [list(r) for r in cs["pf_ints"]]
    tampered = list(range(5, B, 10))
    for t, b in enumerate(tampered):
        # one field of the pair, the key excluded, statement and proof fields in turn: one bit, inside the field's residue range
        fields = [(st_ints[b], i) for i in range(1, len(st_ints[b]))] + [(pf_ints[b], i) for i in range(len(pf_ints[b]))]
        row, i = fields[t % len(fields)]
        row[i] ^= 1 << (3 + t % 64)
    statements = [M.write(r, kind - 1, forms) for r in st_ints]
    proofs = [M.write(r, kind, forms) for r in pf_ints]
    want_st, want_v = expected(kind, statements, proofs, forms)
    assert want_st == [OK] * B and [b for b, v in enumerate(want_v) if v != ACCEPT] == tampered
    got_st, got_v = run(sctx, kind, statements, proofs, forms, True)
    assert sctx.last_json_scan() == (2 * B, 0)
    assert got_st == want_st
    assert got_v == want_v, [b for b in range(B) if got_v[b] != want_v[b]]


# ------------------------------------------------------------------ 2. every class of status in one batch
@functools.lru_cache(maxsize=None)
def classes(kind):
    """-> [(name, statement ints or raw bytes, proof ints or raw bytes, status, verdict or None = the oracle's)]"""
    cs = S.honest_pairs(kind, 6)
    st, pf, pq = cs["st_ints"], cs["pf_ints"], cs["pq"]
    n = st[0][0]
    ws, wp = M.field_words(kind - 1, N_BITS), M.field_words(kind, N_BITS)
    sub = lambda row, i, v: row[:i] + [v] + row[i + 1:]
    out = [("honest %d" % t, st[t], pf[t], OK, ACCEPT) for t in range(6)]
    out += [("tampered proof", st[0], sub(pf[0], len(pf[0]) - 1, pf[0][-1] ^ 4), OK, REJECT),
            ("another statement under the same key", st[4], pf[0], OK, REJECT),
            ("invalid statement", b'{"ek":{"nn":"5"},"c":"7"}', pf[0], INVALID, REJECT),
            ("invalid proof", st[0], b"[]", INVALID, REJECT),
            ("both invalid", b"", b"{", INVALID, REJECT),
            ("wide proof field", st[0], sub(pf[0], 0, 1 << (32 * wp[0])), HOST, REJECT),
            ("wide statement field", sub(st[0], 1, 1 << (32 * ws[1])), pf[0], HOST, REJECT),
            ("wide key, invalid proof", sub(st[0], 0, 1 << (32 * ws[0])), b"7", INVALID, REJECT),
            ("even key", sub(st[0], 0, n + 1), pf[0], HOST, REJECT),
            ("key 1", sub(st[0], 0, 1), [0] * len(pf[0]), HOST, REJECT),
            ("key 0", sub(st[0], 0, 0), [0] * len(pf[0]), HOST, REJECT),
            ("statement field = n^2", sub(st[0], len(st[0]) - 1, n * n), pf[0], HOST, REJECT),
            ("statement field = n^2 - 1", sub(st[0], len(st[0]) - 1, n * n - 1), pf[0], OK, None)]
    for i, (name, w) in enumerate(M.FIELDS[kind]):
        if w == M.NN:
            out += [("%s = n^2" % name, st[0], sub(pf[0], i, n * n), HOST, REJECT), ("%s = n^2 - 1" % name, st[0], sub(pf[0], i, n * n - 1), OK, None)]
        elif w == M.N:
            out += [("%s = n" % name, st[0], sub(pf[0], i, n), HOST, REJECT), ("%s = n - 1" % name, st[0], sub(pf[0], i, n - 1), OK, None)]
        else:
            out += [("%s fills its array" % name, st[0], sub(pf[0], i, (1 << (32 * wp[i])) - 1), OK, None)]
    if kind == M.MUL_PROOF:
        # multiplication_proof.rs:135: e_db a multiple of p has no inverse mod n^2, mod_inv(..).unwrap() panics
        out += [("no inverse", st[0], sub(pf[0], 4, pq[0][0] * 12345), OK, MALFORMED)]
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", M.PROOF_KINDS, ids=KIND_IDS)
def test_every_class_of_status_in_one_batch(sctx, kind, device):
    cls = classes(kind)
    for forms in (0x00, 0x12, 0x21):
        doc = lambda v, k: v if isinstance(v, bytes) else M.write(v, k, forms)
        statements, proofs = [doc(c[1], kind - 1) for c in cls], [doc(c[2], kind) for c in cls]
        want_st, want_v = expected(kind, statements, proofs, forms)
        # the classes are what their names say, by the model and the oracle
        for c, s, v in zip(cls, want_st, want_v):
            assert s == c[3] and (c[4] is None or v == c[4]), (c[0], s, v)
        assert {OK, INVALID, HOST} == set(want_st) and all(v == REJECT for s, v in zip(want_st, want_v) if s != OK)
        got_st, got_v = run(sctx, kind, statements, proofs, forms, device)
        assert got_st == want_st, [(c[0], g, w) for c, g, w in zip(cls, got_st, want_st) if g != w]
        assert got_v == want_v, [(c[0], g, w) for c, g, w in zip(cls, got_v, want_v) if g != w]
        canonical = sum(M.canonical(s, kind - 1, forms, N_BITS) for s in statements) + sum(M.canonical(p, kind, forms, N_BITS) for p in proofs)
        assert sctx.last_json_scan() == (canonical, 2 * len(cls) - canonical)
    # the honest pairs alone: their verdicts are those they had among the others
    alone_st, alone_v = run(sctx, kind, statements[:6], proofs[:6], forms, device)
    assert alone_st == got_st[:6] == [OK] * 6 and alone_v == got_v[:6] == [ACCEPT] * 6
