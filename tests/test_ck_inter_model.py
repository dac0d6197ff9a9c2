"""CPU tests of the model of the interactive CorrectKey calls (tests/ck_inter_model.py) on the case list of tests/ck_inter_cases.py: the
challenge equals oracle/py_model.correct_key_challenge and the C oracle; for every prove session under prime factors the CRT form equals
pm.correct_key_prove and the C oracle in code and digest; the case list has the status / error pattern each batch is built for; the seeded
stream is the nonce streams' construction and a challenge made from it verifies."""
import numpy as np
import pytest

import ck_inter_cases as CC
import ck_inter_model as M
import seeded_nonce_model as N
from helpers import L
from oracle import py_model as pm

CHAL = CC.all_challenge_batches()
PROVE = CC.all_prove_batches()


def digest_words(v):
    return L.int_to_limbs(v, 8)


@pytest.mark.parametrize("name", [n for n, _ in CHAL])
def test_challenge_equals_reference_and_oracle(oracle, name):
    b = dict(CHAL)[name]
    kw, checked = b["n_bits"] // 32, 0
    for i, (s, r, want) in enumerate(zip(b["s"], b["r"], b["want"])):
        n = b["n"][0 if b["shared"] else i]
        if want[4]:
            assert not M.n_ok(n)
            continue
        assert want[:4] == pm.correct_key_challenge(n, s, r)
        sn, e, z, sd = oracle.correct_key_challenge(b["n_bits"], L.int_to_limbs(n, kw), L.ints_to_limbs(s, kw), L.ints_to_limbs(r, kw))
        assert (L.limbs_to_ints(sn), L.limbs_to_int(e), L.limbs_to_ints(z), L.limbs_to_int(sd)) == want[:4]
        checked += 1
    assert checked >= (3 if name == "domain" else len(b["s"]))


@pytest.mark.parametrize("name", [n for n, _ in PROVE])
def test_prove_equals_reference_and_oracle(oracle, name):
    b = dict(PROVE)[name]
    hw, kw, checked = b["n_bits"] // 64, b["n_bits"] // 32, 0
    for (p, q), prime, sn, e, z, (code, sd) in zip(b["keys"], b["prime"], b["sn"], b["e"], b["z"], b["want"]):
        if code == M.BAD_KEY or not prime:
            continue
        rcode, rsd = pm.correct_key_prove(p, q, sn, e, z)
        assert (code, sd) == (rcode, rsd or 0) and code in (0,) + tuple(pm.CK_ERRORS)
        ocode, osd = oracle.correct_key_prove(b["n_bits"], L.int_to_limbs(p, hw), L.int_to_limbs(q, hw), L.ints_to_limbs(sn, kw), digest_words(e), L.ints_to_limbs(z, kw))
        assert ocode == code and (code != 0 or L.limbs_to_int(osd) == sd)
        checked += 1
    assert checked >= len(b["keys"]) - 3


def test_case_list_conditions():
    b = CC.prove_1024()
    by_tag = {t: w[0] for t, w in zip(b["tag"], b["want"]) if not t.startswith("honest")}
    want = {"p | sn_0": 1, "q | z_{K-1}": 2, "both": 1, "e ^ 1": 4, "e = 0": 4, "(p + 1, q)": 5, "(p, p)": 5, "q = 0": 5, "e bit 255": 4, "sn + n, z + n": 4, "z + n": 0}
    assert all(by_tag[t] == want[t] for t in by_tag) and set(want) - set(by_tag) <= {"sn + n, z + n", "z + n"}
    codes = [w[0] for w in b["want"]]
    assert codes[0] == codes[-1] == 0 and all(codes[i - 1] == 0 == codes[i + 1] for i in range(1, len(codes) - 1) if codes[i])
    assert len({k for k, c in zip(b["keys"], codes) if c == 0}) == 2
    c = CC.chal_1024()
    assert 0 in c["s"][0] and c["n"][1] - 1 in c["s"][1] and any(v >= c["n"][2] for v in c["s"][2])
    assert [w[4] for w in CC.chal_domain()["want"]] == [0, 2, 0, 2, 0]
    assert [w[4] for w in CC.seeded_1024()["want"]] == [0, 0, 2, 0]


def test_wide_values_on_the_model():
    """z + n is the same session (z is reduced, not hashed); sn + n has the same residues but other bytes in the hash: code 4, in the
    reference and in the CRT form"""
    p, q = 1000003, 1000033
    n = p * q
    sn, e, z, _ = pm.correct_key_challenge(n, [5, 7, 11], [13, 17, 19])
    assert M.prove(p, q, sn, e, z) == pm.correct_key_prove(p, q, sn, e, z) and M.prove(p, q, sn, e, z)[0] == 0
    zw, snw = [z[0] + n] + z[1:], [sn[0] + n] + sn[1:]
    assert M.prove(p, q, sn, e, zw) == pm.correct_key_prove(p, q, sn, e, zw) == M.prove(p, q, sn, e, z)
    assert M.prove(p, q, snw, e, zw) == (4, 0) and pm.correct_key_prove(p, q, snw, e, zw) == (4, None)


def test_stream_is_the_nonce_construction():
    """kind 10 on the blocks of tests/seeded_nonce_model.py: word 15, the rule of sample_below, a round independent of K"""
    n = CC.H.test_key(1024, 0)[2]
    seed, index = CC.SEED, CC.FIRST_INDEX + 1
    blk = M.block(seed, 3, index, 2, 1)
    assert blk == N.block_words(list(N.R.SIGMA) + N.key_words(seed) + [3, index & M.M32, index >> 32, 0x80000000 | 10 << 20 | 2 << 4 | 1])
    s, r = M.nonces(seed, index, n, 3)
    assert all(0 <= v < n for v in s + r) and len(set(s + r)) == 6
    s5, r5 = M.nonces(seed, index, n, 5)
    assert s5[:3] == s and r5[:3] == r
    assert M.nonces(seed, index, 0, 3) is None
    # a small n exercises the rejection loop: attempts are blocks t nb .. of the same stream
    small = (1 << 40) + 1
    v = M.sample_below(seed, index, 0, 0, small)
    tries = [sum(w << (32 * i) for i, w in enumerate(M.block(seed, t, index, 0, 0)[:2])) & ((1 << 41) - 1) for t in range(N.MAX_ATTEMPTS)]
    assert v == next(t for t in tries if t < small)


def test_seeded_round_trip_on_the_model():
    b = CC.seeded_1024()
    p, q, n = CC.H.test_key(1024, 0)
    assert b["n"][0] == n
    sn, e, z, sd, st = b["want"][0]
    code, digest = M.prove(p, q, sn, e, z)
    assert st == 0 and code == 0 and digest == sd
    assert M.verify_seeded(n, CC.SEED, CC.FIRST_INDEX, 3, digest) == 1
    assert M.verify_seeded(n, CC.SEED, CC.FIRST_INDEX, 3, digest ^ 1) == 0
    assert M.verify_seeded(n, CC.OTHER_SEED, CC.FIRST_INDEX, 3, digest) == 0
    assert M.verify_seeded(0, CC.SEED, CC.FIRST_INDEX, 3, digest) == 2 and M.verify_seeded(n + 1, CC.SEED, CC.FIRST_INDEX, 3, digest) == 2
    assert np.array_equal(digest_words(digest), L.int_to_limbs(sd, 8))
