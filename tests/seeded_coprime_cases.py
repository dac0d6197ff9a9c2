"""The inputs of tests/test_gpu_seeded_coprime.py — a plain module, so that tests/test_seeded_coprime_model.py (CPU) can assert on the model
what the GPU cases rely on: that the bounds below really send the sampler through candidates that are not below n AND through candidates
that are below n but share a factor with it, and that no value comes near the cap of 128 attempts.

The sampler reads n only as a bound, so the "keys" of the sampler cases need not be Paillier keys; the prove-level cases use odd moduli
that are (honest keys, and 3 q with q prime: a third of all candidates below it are rejected by the gcd test, and the proofs still verify)."""
import functools
import hashlib
import math

import helpers as H
import seeded_coprime_model as M
from helpers import L, pm

SEED = hashlib.sha256(b"seeded-coprime-tests").digest()
BIG = (1 << 32) + 7
P_SMOOTH = math.prod(p for p in range(3, 60, 2) if all(p % q for q in range(3, p, 2)))      # the odd primes below 60


def SMOOTH(bits):
    """P c just above 2^(bits - 1), c odd: about 73 % of the candidates below it share a factor with it, about half of all are not below it"""
    c = -(-(1 << (bits - 1)) // P_SMOOTH)
    return P_SMOOTH * (c + 1 if c % 2 == 0 else c)


def HALF105(bits):
    """105 m, m the first odd integer above 2^(bits - 1) / 105"""
    m = (1 << (bits - 1)) // 105 + 1
    return 105 * (m + 1 if m % 2 == 0 else m)


def _bound(tag, bits):
    """an honest-looking odd bound of exactly `bits` bits"""
    return pm.Drbg(b"seeded-coprime-" + tag).bits(bits) | (1 << (bits - 1)) | 1


def sampler_cases():
    """name -> dict(kind, n_bits, n_list (one = shared), B, first_index, device)"""
    k1024 = H.test_key(1024)[2]
    fix = H.fixture_key()[2]
    even = _bound(b"even", 1024) - 1
    c = {
        # per-proof bounds in one block: a key, SMOOTH, 0 and an even number in the MIDDLE, 15, HALF105
        "verlin-1024-perkey-B6-host": dict(kind=M.KIND_VERLIN, n_bits=1024, n_list=[k1024, SMOOTH(1024), 0, even, 15, HALF105(1024)], first_index=BIG, device=False),
        # ... 3, 0, 1, and 1019 bits: a masked top limb
        "mul-1024-perkey-B5-device": dict(kind=M.KIND_MUL, n_bits=1024, n_list=[HALF105(1024), 3, 0, 1, SMOOTH(1019)], first_index=3, device=True),
        "verlin-2048-shared-B3-device": dict(kind=M.KIND_VERLIN, n_bits=2048, n_list=[fix], B=3, first_index=0, device=True),
        "mul-2048-shared-B4-host": dict(kind=M.KIND_MUL, n_bits=2048, n_list=[SMOOTH(2048)], B=4, first_index=BIG, device=False),
        # a 2048-bit-wide call: 15 (one word), an even number, 2043 bits
        "mul-2048-perkey-B4-device": dict(kind=M.KIND_MUL, n_bits=2048, n_list=[fix, 15, even, SMOOTH(2043)], first_index=BIG, device=True),
        "verlin-2048-perkey-B5-host": dict(kind=M.KIND_VERLIN, n_bits=2048, n_list=[HALF105(2048), 1, SMOOTH(2048), 3, fix], first_index=0, device=False),
        # kw = 128: 1 KB of LDS per lane
        "verlin-4096-perkey-B3-device": dict(kind=M.KIND_VERLIN, n_bits=4096, n_list=[SMOOTH(4096), _bound(b"k4096", 4096), HALF105(4096)], first_index=BIG, device=True),
        "mul-4096-shared-B3-host": dict(kind=M.KIND_MUL, n_bits=4096, n_list=[HALF105(4096)], B=3, first_index=0, device=False),
        "mul-4096-perkey-B3-host": dict(kind=M.KIND_MUL, n_bits=4096, n_list=[SMOOTH(4091), 15, _bound(b"m4096", 4096)], first_index=BIG, device=False),
        # more than one wavefront and more than one block; honest-looking odd bounds and SMOOTH alternate, so neighbouring lanes need
        # different numbers of attempts
        "verlin-1024-perkey-B130-host": dict(kind=M.KIND_VERLIN, n_bits=1024, n_list=[SMOOTH(1024) if b % 2 else _bound(b"big-%d" % b, 1024) for b in range(130)],
                                             first_index=BIG, device=False),
    }
    for v in c.values():
        v.setdefault("B", len(v["n_list"]))
    return c


@functools.lru_cache(maxsize=None)
def model_nonces(name):
    c = sampler_cases()[name]
    return M.nonces(c["kind"], SEED, c["first_index"], c["n_list"], c["B"])


def field_arrays(kind, nonces, kw):
    """the model's nonces of a batch -> the four arrays by field id (None where the kind has none): uint32 limbs [B][kw]"""
    names = M.FIELDS[kind]
    return [L.ints_to_limbs([d[names[f]] for d in nonces], kw) if f < len(names) else None for f in range(4)]


def gcd_candidates(name):
    """every candidate of a case's coprime field that reached the gcd test: (proof, n, candidate, accepted)"""
    c = sampler_cases()[name]
    field = len(M.FIELDS[c["kind"]]) - 1
    _, status, _, _ = model_nonces(name)
    out = []
    for b in range(c["B"]):
        n = c["n_list"][0] if len(c["n_list"]) == 1 else c["n_list"][b]
        if status[b]:
            continue
        for t in range(M.MAX_ATTEMPTS):
            v = M.candidate(SEED, c["first_index"] + b, c["kind"], field, n, t)
            if v < n:
                ok = math.gcd(v, n) == 1
                out.append((b, n, v, ok))
                if ok:
                    break
    return out


# ---- the prove-level cases ------------------------------------------------------------------------------------------------------------------
SHAPES = [(2048, 3, 0), (1024, 4, BIG)]
THREE_Q = (1024, 4, 7)          # n_bits, B, first_index: under it a proof with n = 3 q takes a gcd rejection, for r_a and for r_d
                                # (tests/test_seeded_coprime_model.py asserts it)


@functools.lru_cache(maxsize=None)
def three_q_modulus():
    """3 q of exactly 1024 bits, q a 1022-bit prime with its two top bits set"""
    d = pm.Drbg(b"seeded-coprime-3q")
    while True:
        q = d.bits(1022) | (3 << 1020) | 1
        if H.is_probable_prime(q):
            return 3 * q


def keys_for(n_bits, B, three_q=False):
    """the 2048-bit fixture key, shared; two 1024-bit keys, one per proof; or a 1024-bit key alternating with 3 q"""
    if three_q:
        return [three_q_modulus() if b % 2 else H.test_key(1024)[2] for b in range(B)], n_bits // 32
    if n_bits == 2048:
        return [H.fixture_key()[2]], 0
    return [H.test_key(1024, tag=b % 2)[2] for b in range(B)], n_bits // 32


def _unit(d, n):
    while True:
        r = d.below(n)
        if math.gcd(r, n) == 1:
            return r


@functools.lru_cache(maxsize=None)
def verlin_case(n_bits, B, first_index, three_q=False):
    """statement (c, c', phi_x = gen_phi of the witness), witness (x, x', x'', r_x) with r_x coprime to n, and the model's nonces"""
    keys, stride = keys_for(n_bits, B, three_q)
    kw = n_bits // 32
    d = pm.Drbg(b"seeded-verlin-%d-%d" % (n_bits, three_q))
    per = [keys[b % len(keys)] for b in range(B)]
    wit = [[d.below(n), d.below(n), d.below(n), _unit(d, n)] for n in per]
    c = [H.python_enc(n, d.below(n), _unit(d, n)) for n in per]
    cp = [H.python_enc(n, d.below(n), _unit(d, n)) for n in per]
    phi_x = [pm.gen_phi(n, c[b], cp[b], *wit[b]) for b, n in enumerate(per)]
    nonces, status, _, not_coprime = M.nonces(M.KIND_VERLIN, SEED, first_index, keys, B)
    assert not any(status)
    return dict(ns=per, n=L.ints_to_limbs(keys, kw), stride=stride, c=L.ints_to_limbs(c, 2 * kw), cp=L.ints_to_limbs(cp, 2 * kw), phi_x=L.ints_to_limbs(phi_x, 2 * kw),
                wit=tuple(L.ints_to_limbs([w[k] for w in wit], kw) for k in range(4)), nonce=tuple(field_arrays(M.KIND_VERLIN, nonces, kw)),
                ints=dict(c=c, cp=cp, phi_x=phi_x, wit=wit, nonces=nonces), not_coprime=not_coprime)


MUL_WIT = ("a", "b", "r_a", "r_b", "r_c")


@functools.lru_cache(maxsize=None)
def mul_case(n_bits, B, first_index, three_q=False):
    """statement (e_a, e_b, e_c = Enc(a b mod n, r_c)), witness (a, b, r_a, r_b, r_c) with the r coprime to n, and the model's nonces"""
    keys, stride = keys_for(n_bits, B, three_q)
    kw = n_bits // 32
    d = pm.Drbg(b"seeded-mul-%d-%d" % (n_bits, three_q))
    per = [keys[b % len(keys)] for b in range(B)]
    wit = [dict(a=d.below(n), b=d.below(n), r_a=_unit(d, n), r_b=_unit(d, n), r_c=_unit(d, n)) for n in per]
    e = [[H.python_enc(n, w["a"], w["r_a"]), H.python_enc(n, w["b"], w["r_b"]), H.python_enc(n, w["a"] * w["b"] % n, w["r_c"])] for n, w in zip(per, wit)]
    nonces, status, _, not_coprime = M.nonces(M.KIND_MUL, SEED, first_index, keys, B)
    assert not any(status)
    return dict(ns=per, n=L.ints_to_limbs(keys, kw), stride=stride, e=tuple(L.ints_to_limbs([x[k] for x in e], 2 * kw) for k in range(3)),
                wit=tuple(L.ints_to_limbs([w[k] for w in wit], kw) for k in MUL_WIT), nonce=tuple(field_arrays(M.KIND_MUL, nonces, kw)[:2]),
                ints=dict(e=e, wit=wit, nonces=nonces), not_coprime=not_coprime)
