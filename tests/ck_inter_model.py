"""What the four calls of the interactive CorrectKey compute (include/zkp_hip.h: zkp_correct_key_challenge_batch, its seeded form,
zkp_correct_key_prove_batch, zkp_correct_key_verify_seeded_batch), on Python integers.

The stream is the construction of tests/seeded_nonce_model.py (its ChaCha block and the rule of its sample_below) under a kind of its own:
    kind 10, slot i < K, field 0: s_i = sample_below(n)        field 1: r_i = sample_below(n)
(seeded_nonce_model.sample_below itself asserts kind <= 4, as seeded_commit_model.py found for kind 7; the rule is restated here over its
block function.)  The challenge is the reference's formulas on the sampled values.  prove is DEFINED by the header's CRT identities — no
primality test is made — and oracle/py_model.correct_key_prove is the reference's statement: for prime p, q the two agree in code and digest
(tests/test_ck_inter_model.py asserts it for every such case)."""
from math import gcd

import ck_prove_model as CP
import seeded_nonce_model as N
from oracle import py_model as pm

KIND = 10
M32 = 0xFFFFFFFF
MALFORMED = 2
OK, SN_NOT_COPRIME, Z_NOT_COPRIME, RN_NOT_COPRIME, E_MISMATCH, BAD_KEY = 0, 1, 2, 3, 4, 5


def block(seed, counter, index, slot, field):
    assert 0 <= slot < 65536 and 0 <= field < 16
    w15 = 0x80000000 | (KIND << 20) | (slot << 4) | field
    return N.block_words(list(N.R.SIGMA) + N.key_words(seed) + [counter & M32, index & M32, (index >> 32) & M32, w15])


def sample_below(seed, index, slot, field, n):
    """the rule of seeded_nonce_model.sample_below -> value, or None after 128 rejected attempts"""
    bits = n.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    for t in range(N.MAX_ATTEMPTS):
        words = []
        for k in range(t * nb, (t + 1) * nb):
            words += block(seed, k, index, slot, field)
        v = sum(w << (32 * i) for i, w in enumerate(words[:nw])) & ((1 << bits) - 1)
        if v < n:
            return v
    return None


def n_ok(n):
    """the challenge's domain: n odd and at least 3"""
    return n >= 3 and n % 2 == 1


def nonces(seed, index, n, K):
    """-> (s, r), or None where the sampler fails (n == 0, 128 rejections)"""
    if n == 0:
        return None
    s = [sample_below(seed, index, i, 0, n) for i in range(K)]
    r = [sample_below(seed, index, i, 1, n) for i in range(K)]
    return None if None in s or None in r else (s, r)


def challenge(n, s, r):
    """-> (sn, e, z, s_digest, status); s, r any values"""
    K = len(s)
    if not n_ok(n):
        return [0] * K, 0, [0] * K, 0, MALFORMED
    return pm.correct_key_challenge(n, s, r) + (0,)


def challenge_seeded(n, seed, index, K):
    sr = nonces(seed, index, n, K)
    if sr is None:
        return [0] * K, 0, [0] * K, 0, MALFORMED
    return challenge(n, *sr)


def verify_seeded(n, seed, index, K, proof_digest):
    sr = nonces(seed, index, n, K)
    if sr is None or not n_ok(n):
        return MALFORMED
    return 1 if pm.compute_digest(sr[0]) == proof_digest else 0


def crt(p, q, vp, vq):
    return vp + p * ((vq - vp) * pow(p, -1, q) % q)


def prove(p, q, sn, e, z):
    """-> (code, s_digest): six half-width powers per round, no phi"""
    if CP.status(p, q):
        return BAD_KEY, 0
    n = p * q
    rn, roots = [], []
    for sni, zi in zip(sn, z):
        res = []
        for f, d in ((p, pow(q, -1, p - 1)), (q, pow(p, -1, q - 1))):
            a = pow(zi % f, n % (f - 1), f) * pow(sni % f, (f - 1) - e % (f - 1), f) % f
            res.append((a, pow(sni % f, d, f)))
        rn.append(crt(p, q, res[0][0], res[1][0]))
        roots.append(crt(p, q, res[0][1], res[1][1]))
    for code, vals in ((SN_NOT_COPRIME, sn), (Z_NOT_COPRIME, z), (RN_NOT_COPRIME, rn)):
        if any(gcd(n, v) != 1 for v in vals):
            return code, 0
    if e != pm.compute_digest([n] + list(sn) + rn):
        return E_MISMATCH, 0
    return OK, pm.compute_digest(roots)
