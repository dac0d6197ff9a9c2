"""GPU tests of the verifier's commitment of the interactive RangeProof (include/zkp_hip.h: zkp_range_verifier_commit_seeded_batch,
zkp_range_verifier_reveal_seeded_batch, zkp_range_verify_commit_batch): commit and reveal bit for bit against tests/seeded_commit_model.py
with the oracle's Enc on the model's (m, r), what each call writes, the wipe, device pointers, chunk invariance, the verdicts of
verify_commit on revealed and tampered sessions, and the refusals.  No tolerance anywhere: every comparison is of bytes."""
import numpy as np
import pytest

import seeded_commit_cases as CC
import seeded_commit_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu

SEED = CC.SEED
ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED
_EXPECTED = {}


@pytest.fixture(scope="module")
def actx():
    """nothing pinned: the library's own routing, so that the session counts of the shapes reach the engines they name"""
    c = zkp.Context(0)
    yield c
    c.close()


def expected(name, oracle):
    """the model's sessions of a shape as arrays, computed once: (keys [1 or B][kw], n_stride, r [B][kw], e [B][32], com [B][2kw], m [B][kw])"""
    if name not in _EXPECTED:
        n_bits, _, shared, e_len, B, _ = CC.SHAPES[name]
        kw = n_bits // 32
        keys, ses = CC.model(name)
        assert not any(s["status"] for s in ses)
        n = CC.key_limbs(keys, n_bits)
        r = L.ints_to_limbs([s["r"] for s in ses], kw)
        m = L.ints_to_limbs([s["m"] for s in ses], kw)
        e, _ = CC.e_rows([s["e"] for s in ses])
        oracle.set_threads(min(16, oracle.max_threads()))
        com = oracle.paillier_enc(n_bits, n, 0 if shared else kw, m, r)
        for a in (n, r, m, e, com):
            a.setflags(write=False)
        _EXPECTED[name] = (n, 0 if shared else kw, r, e, com, m)
    return _EXPECTED[name]


def commit_and_reveal(c, name, oracle):
    """both seeded calls on host arrays against the model, with what each call writes and the residue after each"""
    n_bits, _, _, e_len, B, first = CC.SHAPES[name]
    kw = n_bits // 32
    n, stride, r, e, com, _ = expected(name, oracle)
    got_com, st = np.full((B, 2 * kw), 0xA5A5A5A5, np.uint32), np.full(B, 9, np.uint8)
    c.range_verifier_commit_seeded(n_bits, B, n, stride, e_len, SEED, first, got_com, st)
    assert c.witness_residue() == 0
    assert not st.any() and np.array_equal(got_com, com), name
    got_r, got_e, st2 = np.full((B, kw), 0xA5A5A5A5, np.uint32), np.full((B, 32), 0xEE, np.uint8), np.full(B, 9, np.uint8)
    c.range_verifier_reveal_seeded(n_bits, B, n, stride, e_len, SEED, first, got_r, got_e, st2)
    assert c.witness_residue() == 0
    assert not st2.any() and np.array_equal(got_r, r), name
    assert np.array_equal(got_e, e) and not got_e[:, e_len:].any(), "all 32 bytes of a row are written, zero past e_len"
    return got_com, got_r, got_e


# ---- 1. commit and reveal against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.SHAPES))
def test_commit_and_reveal_equal_the_model_under_the_librarys_own_routing(actx, oracle, name):
    commit_and_reveal(actx, name, oracle)
    if name == CC.ZERO_DIGEST_SHAPE:
        m = expected(name, oracle)[5]
        assert not m[CC.ZERO_DIGEST_SESSION][7] >> 24, "the digest of this session begins with a 00 byte"


@pytest.mark.parametrize("name", CC.PINNED_SHAPES)
def test_commit_and_reveal_equal_the_model_on_every_pinned_engine(ctx, oracle, name):
    commit_and_reveal(ctx, name, oracle)


def test_status_is_optional_and_an_empty_batch_is_fine(actx, oracle):
    name = "1024-narrow-perkey-e1-B4"
    n_bits, _, _, e_len, B, first = CC.SHAPES[name]
    n, stride, r, e, com, _ = expected(name, oracle)
    got = np.zeros_like(com)
    actx.range_verifier_commit_seeded(n_bits, B, n, stride, e_len, SEED, first, got)
    assert np.array_equal(got, com)
    actx.range_verifier_commit_seeded(n_bits, 0, n, stride, e_len, SEED, first, got)
    actx.range_verifier_reveal_seeded(n_bits, 0, n, stride, e_len, SEED, first, None, None)
    actx.range_verify_commit(n_bits, 0, n, stride, None, None, None, None, None)


# ---- 2. device pointers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2048-pow2-perkey-e5-B4", "1024-pow2-shared-e31-B70"])
def test_device_pointer_calls_equal_the_host_pointer_calls(actx, oracle, name):
    import torch
    n_bits, _, _, e_len, B, first = CC.SHAPES[name]
    kw = n_bits // 32
    n, stride, r, e, com, _ = expected(name, oracle)
    host = commit_and_reveal(actx, name, oracle)
    dev = lambda a: torch.from_numpy(np.array(a).view(np.int32 if a.dtype == np.uint32 else np.uint8)).cuda()
    dn = dev(n)
    dcom, dr = torch.full((B, 2 * kw), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), torch.full((B, kw), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    de = torch.full((B, 32), 0xEE, dtype=torch.uint8, device="cuda")
    d1, d2, dv = (torch.full((B,), 9, dtype=torch.uint8, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    actx.range_verifier_commit_seeded(n_bits, B, dn, stride, e_len, SEED, first, dcom, d1)
    assert actx.witness_residue() == 0
    actx.range_verifier_reveal_seeded(n_bits, B, dn, stride, e_len, SEED, first, dr, de, d2)
    assert actx.witness_residue() == 0
    elen = torch.full((B,), e_len, dtype=torch.uint8, device="cuda")
    actx.range_verify_commit(n_bits, B, dn, stride, dcom, dr, de, elen, dv)
    actx.synchronize()
    assert np.array_equal(dcom.cpu().numpy().view(np.uint32), host[0]) and np.array_equal(dr.cpu().numpy().view(np.uint32), host[1])
    assert np.array_equal(de.cpu().numpy(), host[2])
    assert not d1.cpu().numpy().any() and not d2.cpu().numpy().any() and (dv.cpu().numpy() == ACCEPT).all()


# ---- 3. chunk invariance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1024-narrow-perkey-e1-B4", "2048-full-shared-e5-B300"])
def test_a_call_split_at_three_equals_one_call(actx, oracle, name):
    n_bits, _, shared, e_len, B, first = CC.SHAPES[name]
    kw = n_bits // 32
    n, stride, r, e, com, _ = expected(name, oracle)
    got_com, got_r, got_e = np.zeros_like(com), np.zeros_like(r), np.full_like(e, 0xEE)
    s1, s2 = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
    for lo, hi in ((0, 3), (3, B)):
        nn = n if shared else n[lo:hi]
        actx.range_verifier_commit_seeded(n_bits, hi - lo, nn, stride, e_len, SEED, first + lo, got_com[lo:hi], s1[lo:hi])
        actx.range_verifier_reveal_seeded(n_bits, hi - lo, nn, stride, e_len, SEED, first + lo, got_r[lo:hi], got_e[lo:hi], s2[lo:hi])
    assert np.array_equal(got_com, com) and np.array_equal(got_r, r) and np.array_equal(got_e, e) and not s1.any() and not s2.any()


# ---- 4. verify_commit ------------------------------------------------------------------------------------------------------------------------
def verify_batch(name, oracle):
    """every revealed session of the shape, the tampered copies of sessions 0 and B - 1, and one session with e_len = 0 ->
    (n, n_stride, com, r, e, e_len, m of the model, expected verdicts, labels)"""
    n_bits, _, shared, e_len, B, _ = CC.SHAPES[name]
    kw = n_bits // 32
    keys, ses = CC.model(name)
    n, stride, r, e, com, _ = expected(name, oracle)
    coms = L.limbs_to_ints(com)
    rows = [(keys[0] if shared else keys[b], coms[b], s["r"], s["e"], ACCEPT, "revealed %d" % b) for b, s in enumerate(ses)]
    for b in sorted({0, B - 1}):
        nb = keys[0] if shared else keys[b]
        rows += [(nb, c2, r2, e2, REJECT, "%s of %d" % (what, b)) for what, c2, r2, e2 in CC.tampered(n_bits, nb, coms[b], ses[b]["r"], ses[b]["e"])]
    # e_len = 0: the commitment to the empty string under session 0's key and r, made by the oracle from the model's hash
    n0, r0 = rows[0][0], ses[0]["r"]
    m_empty = M.digest_int(b"")
    c_empty = L.limbs_to_int(oracle.paillier_enc(n_bits, L.ints_to_limbs([n0], kw), 0, L.ints_to_limbs([m_empty], kw), L.ints_to_limbs([r0], kw))[0])
    rows.append((n0, c_empty, r0, b"", ACCEPT, "e_len 0"))
    rows.append((n0, coms[0], r0, b"", REJECT, "e_len 0 against the commitment to e"))
    ev, elen = CC.e_rows([q[3] for q in rows])
    nv = n if shared else L.ints_to_limbs([q[0] for q in rows], kw)
    return (nv, stride, L.ints_to_limbs([q[1] for q in rows], 2 * kw), L.ints_to_limbs([q[2] for q in rows], kw), ev, elen,
            L.ints_to_limbs([M.digest_int(q[3]) for q in rows], kw), np.array([q[4] for q in rows], np.uint8), [q[5] for q in rows])


@pytest.mark.parametrize("name", CC.VERIFY_SHAPES)
def test_verify_commit_accepts_revealed_sessions_and_rejects_tampered_ones(actx, oracle, name):
    n_bits = CC.SHAPES[name][0]
    n, stride, com, r, e, elen, m, want, labels = verify_batch(name, oracle)
    count = len(want)
    assert {t for t in CC.TAMPERS if t != "com+nn" or CC.SHAPES[name][1] != "full"} <= {l.split(" of ")[0] for l in labels}
    v = np.full(count, 9, np.uint8)
    actx.range_verify_commit(n_bits, count, n, stride, com, r, e, elen, v)
    assert [labels[i] for i in range(count) if v[i] != want[i]] == [], list(v)
    ok = np.full(count, 9, np.uint8)
    actx.paillier_enc_check(n_bits, count, n, stride, m, r, None, None, com, ok)
    assert np.array_equal(v, ok), "the verdicts are those of zkp_paillier_enc_check_batch fed the model's m"


def test_verify_commit_on_a_pinned_engine(ctx, oracle):
    name = "1024-narrow-perkey-e1-B4"
    n, stride, com, r, e, elen, m, want, labels = verify_batch(name, oracle)
    v = np.full(len(want), 9, np.uint8)
    ctx.range_verify_commit(1024, len(want), n, stride, com, r, e, elen, v)
    assert [labels[i] for i in range(len(want)) if v[i] != want[i]] == [], list(v)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refused_lengths_touch_no_byte_and_leave_no_residue(actx, oracle):
    name = "1024-narrow-perkey-e1-B4"
    n_bits, _, _, e_len, B, first = CC.SHAPES[name]
    kw = n_bits // 32
    n, stride, r, e, com, _ = expected(name, oracle)
    commit_and_reveal(actx, name, oracle)               # (the blocks whose residue is counted below)
    got_com, got_r, got_e, st = np.full((B, 2 * kw), 7, np.uint32), np.full((B, kw), 7, np.uint32), np.full((B, 32), 7, np.uint8), np.full(B, 7, np.uint8)
    for bad in (0, 33):
        with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_verifier_commit_seeded_batch"):
            actx.range_verifier_commit_seeded(n_bits, B, n, stride, bad, SEED, first, got_com, st)
        with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_verifier_reveal_seeded_batch"):
            actx.range_verifier_reveal_seeded(n_bits, B, n, stride, bad, SEED, first, got_r, got_e, st)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_verifier_commit_seeded_batch"):
        actx.range_verifier_commit_seeded(n_bits, B, n, stride, e_len, None, first, got_com, st)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_verifier_commit_seeded_batch"):
        actx.range_verifier_commit_seeded(1536, B, n, stride, e_len, SEED, first, got_com, st)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_verify_commit_batch"):
        actx.range_verify_commit(n_bits, B, n, stride, com, r, e, None, st)
    assert (got_com == 7).all() and (got_r == 7).all() and (got_e == 7).all() and (st == 7).all()
    assert actx.witness_residue() == 0


def code_of(err):
    """the status code in a ZkpError's text: 'status N: ...'"""
    return int(str(err).split()[1].rstrip(":"))


def enc_call_code(c, n_bits, n_limbs):
    """the status code zkp_paillier_enc_batch returns under this key (0: the call succeeded)"""
    kw = n_bits // 32
    out = np.zeros((1, 2 * kw), np.uint32)
    try:
        c.paillier_enc(n_bits, 1, n_limbs, 0, L.ints_to_limbs([5], kw), L.ints_to_limbs([3], kw), out)
    except zkp.ZkpError as err:
        return code_of(err)
    return 0


def call_code(fn, *args):
    try:
        fn(*args)
    except zkp.ZkpError as err:
        return code_of(err)
    return 0


@pytest.mark.parametrize("what", ["even", "200-bit"])
def test_a_key_outside_the_domain_gives_the_enc_calls_code_and_malformed_sessions(actx, what):
    n_bits, kw, B = 1024, 32, 4
    even = CC.key(1024, "full") - 1
    code = enc_call_code(actx, n_bits, L.ints_to_limbs([even], kw))
    key = even if what == "even" else (1 << 199) + 1
    assert not M.key_in_domain(key)
    n = L.ints_to_limbs([key], kw)
    com, r, e, st = np.full((B, 2 * kw), 7, np.uint32), np.full((B, kw), 7, np.uint32), np.full((B, 32), 7, np.uint8), np.full(B, 7, np.uint8)
    assert call_code(actx.range_verifier_commit_seeded, n_bits, B, n, 0, 5, SEED, 0, com, st) == code
    assert actx.witness_residue() == 0
    if code == 0:
        assert (st == MALFORMED).all() and not com.any()
    st[:] = 7
    assert call_code(actx.range_verifier_reveal_seeded, n_bits, B, n, 0, 5, SEED, 0, r, e, st) == code
    assert actx.witness_residue() == 0
    if code == 0:
        assert (st == MALFORMED).all() and not r.any() and not e.any()
    v = np.full(B, 7, np.uint8)
    elen = np.full(B, 5, np.uint8)
    assert call_code(actx.range_verify_commit, n_bits, B, n, 0, np.zeros((B, 2 * kw), np.uint32), np.zeros((B, kw), np.uint32), np.zeros((B, 32), np.uint8), elen, v) == code
    if code == 0:
        assert (v == MALFORMED).all()


def test_a_zero_key_beside_good_ones_is_malformed_and_leaves_its_neighbours_alone(actx, oracle):
    name = "1024-narrow-perkey-e1-B4"
    n_bits, _, _, e_len, B, first = CC.SHAPES[name]
    kw = n_bits // 32
    n, stride, r, e, com, _ = expected(name, oracle)
    bad = n.copy()
    bad[2] = 0
    keys = L.limbs_to_ints(bad)
    ses = M.sessions(SEED, first, keys, B, e_len, with_com=False)
    assert [s["status"] for s in ses] == [0, 0, MALFORMED, 0]
    got_com, got_r, got_e = np.full_like(com, 7), np.full_like(r, 7), np.full_like(e, 7)
    s1, s2 = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
    actx.range_verifier_commit_seeded(n_bits, B, bad, stride, e_len, SEED, first, got_com, s1)
    actx.range_verifier_reveal_seeded(n_bits, B, bad, stride, e_len, SEED, first, got_r, got_e, s2)
    assert list(s1) == list(s2) == [0, 0, MALFORMED, 0]
    others = [0, 1, 3]
    assert np.array_equal(got_com[others], com[others]) and np.array_equal(got_r[others], r[others]) and np.array_equal(got_e[others], e[others])
    assert not got_com[2].any() and not got_r[2].any() and not got_e[2].any()
    # verify_commit: the session under the zero key is MALFORMED, a session whose e_len is above 32 too; the neighbours are accepted
    elen = np.full(B, e_len, np.uint8)
    elen[3] = 33
    v = np.full(B, 9, np.uint8)
    actx.range_verify_commit(n_bits, B, bad, stride, com, r, e, elen, v)
    assert list(v) == [ACCEPT, ACCEPT, MALFORMED, MALFORMED]
