"""(statement, proof) pairs of ZeroProof, CiphertextProof, VerlinProof and MulProof as lists of integers in the field order of
tests/json_sigma_model.py, proved and judged by the C oracle: shared by the CPU model test, the GPU document tests and nothing else.
Everything is computed once per process and kept."""
import functools

import numpy as np

import helpers as H
import json_sigma_model as M
from helpers import pm, L
from small_proof_cases import Batch

N_BITS = 1024


@functools.lru_cache(maxsize=None)
def oracle():
    import oracle_lib
    return oracle_lib.Oracle()


@functools.lru_cache(maxsize=None)
def key_pool(count):
    """`count` DISTINCT 1024-bit keys (p, q, n) from few primes: n = p_i q_j over the primes of the suite's test keys"""
    side = 1
    while side * side < count:
        side += 1
    keys = [H.test_key(N_BITS, tag=t) for t in range(side)]
    pool = [(keys[i][0], keys[j][1], keys[i][0] * keys[j][1]) for i in range(side) for j in range(side)][:count]
    assert len({k[2] for k in pool}) == count and all(k[2].bit_length() > N_BITS - 2 for k in pool)
    return pool


def _rows(*arrs):
    return [list(r) for r in zip(*(L.limbs_to_ints(a) for a in arrs))]


@functools.lru_cache(maxsize=None)
def honest_pairs(kind, B, distinct=False):
    """-> dict(st_ints, pf_ints, pq): B honest pairs of `kind` (a PROOF kind) under per-pair keys, all distinct when asked"""
    o = oracle()
    bt = Batch(N_BITS, B, list(key_pool(B)) if distinct else [H.test_key(N_BITS, tag=t) for t in range(4)], False)
    d = pm.Drbg(b"sigma-json-%d-%d" % (kind, B))
    rnd = lambda: [d.below(n) for n in bt.ns]
    a = lambda v: L.ints_to_limbs(v, bt.kw)
    if kind == M.ZERO_PROOF:
        r, rp = rnd(), rnd()
        c = bt.enc(o, [0] * B, r)
        st, pf = (bt.n_full, c), o.zero_proof_prove(*bt.key(), c, a(r), a(rp))
    elif kind == M.CIPHERTEXT_PROOF:
        x, r, xp, rp = rnd(), rnd(), rnd(), rnd()
        c = bt.enc(o, x, r)
        st, pf = (bt.n_full, c), o.ciphertext_proof_prove(*bt.key(), c, a(x), a(r), a(xp), a(rp))
    elif kind == M.VERLIN_PROOF:
        wit, non = tuple(a(rnd()) for _ in range(4)), tuple(a(rnd()) for _ in range(4))
        c, cp = bt.enc(o, rnd(), rnd()), bt.enc(o, rnd(), rnd())
        phi_x = o.verlin_proof_prove(*bt.key(), c, cp, np.zeros_like(c), wit, wit)[0]          # gen_phi of the witness (verlin_proof.rs:138-165)
        st, pf = (bt.n_full, c, cp, phi_x), o.verlin_proof_prove(*bt.key(), c, cp, phi_x, wit, non)
    else:
        assert kind == M.MUL_PROOF
        v = {k: rnd() for k in ("a", "b", "r_a", "r_b", "r_c", "d", "r_d")}
        e = [bt.enc(o, v["a"], v["r_a"]), bt.enc(o, v["b"], v["r_b"]), bt.enc(o, [x * y % n for x, y, n in zip(v["a"], v["b"], bt.ns)], v["r_c"])]
        out = o.mul_proof_prove(*bt.key(), *e, *(a(v[k]) for k in ("a", "b", "r_a", "r_b", "r_c", "d", "r_d")))
        assert not out[5].any()
        st, pf = (bt.n_full, *e), out[:5]
    return dict(st_ints=_rows(*st), pf_ints=_rows(*pf), pq=bt.pq)


def oracle_verdicts(kind, st_ints, pf_ints, n_bits=N_BITS):
    """the oracle's verify on pairs given as integers (every one inside its array)"""
    o = oracle()
    kw = n_bits // 32
    cols = lambda rows, k: [L.ints_to_limbs([r[i] for r in rows], w) for i, w in enumerate(M.field_words(k, n_bits))]
    st, pf = cols(st_ints, kind - 1), cols(pf_ints, kind)
    verify = {M.ZERO_PROOF: o.zero_proof_verify, M.CIPHERTEXT_PROOF: o.ciphertext_proof_verify, M.VERLIN_PROOF: o.verlin_proof_verify, M.MUL_PROOF: o.mul_proof_verify}[kind]
    return verify(n_bits, st[0], kw, *st[1:], *pf)
