"""The inputs of tests/test_gpu_dlog_setup.py — a plain module, so that tests/test_seeded_dlog_setup_model.py (CPU) can assert on the model
what the GPU cases rely on: that under the committed (seed, first_index, N) some statement is accepted at attempt 0, some candidate is
rejected at least three times in a row for its symbol, some is rejected as not below N - 1, and the square modulus runs out of attempts.

The set-up reads N as a bound and as the lower argument of a Jacobi symbol: it needs no factorisation, so the moduli need not be RSA
moduli.  They are odd numbers of full width, ABOVE(bits) just over a power of two (half of all candidates overshoot), the square of a
prime (every symbol is 0 or 1: 128 rejections), and an even number."""
import functools
import hashlib

import helpers as H
import seeded_dlog_setup_model as M
from helpers import L, pm

SEED = hashlib.sha256(b"seeded-dlog-setup-tests").digest()
PROVE_SEED = hashlib.sha256(b"seeded-dlog-setup-tests: the prover's nonces").digest()      # (never the set-up's seed: SECURITY CONTRACT)
BIG = (1 << 32) + 5
WIDTHS = (1024, 2048, 4096)
BATCHES = (1, 65, 130)
SQUARE_ROW, EVEN_ROW = 3, 5          # in batches of more than one statement


def honest(bits, tag):
    """an honest-looking odd modulus of exactly `bits` bits (the 2048-bit fixture key and generated 1024-bit keys where there are any)"""
    if bits == 2048 and tag % 3 == 0:
        return H.fixture_key()[2]
    if bits == 1024 and tag % 3 == 0:
        return H.test_key(1024, tag % 2)[2]
    return pm.Drbg(b"seeded-dlog-setup-%d-%d" % (bits, tag)).bits(bits) | (1 << (bits - 1)) | 1


def ABOVE(bits):
    """just above 2^(bits - 1): a candidate of `bits` bits is not below it with probability one half"""
    return (1 << (bits - 1)) + 0x1235


@functools.lru_cache(maxsize=None)
def square():
    p = H.test_key(1024)[0]
    return p * p


@functools.lru_cache(maxsize=None)
def moduli(n_bits, B):
    if B == 1:
        return (honest(n_bits, 0),)
    out = [ABOVE(n_bits) if b % 4 == 1 else honest(n_bits, b % 6) for b in range(B)]
    out[SQUARE_ROW] = square()
    out[EVEN_ROW] = honest(n_bits, 1) - 1
    return tuple(out)


def first_index(n_bits, B):
    return BIG if B == 65 else n_bits // 1024


@functools.lru_cache(maxsize=None)
def model(n_bits, B):
    """-> (statements, status, not_below, symbol) of the case, computed once"""
    return M.statements(SEED, first_index(n_bits, B), list(moduli(n_bits, B)))


def arrays(n_bits, B):
    """the model's statements as the arrays of the C ABI: N, g, ni [B][kw], secret [B][8], status [B]"""
    kw = n_bits // 32
    st, status, _, _ = model(n_bits, B)
    return (L.ints_to_limbs(list(moduli(n_bits, B)), kw), L.ints_to_limbs([s["g"] for s in st], kw), L.ints_to_limbs([s["ni"] for s in st], kw),
            L.ints_to_limbs([s["secret"] for s in st], 8), status)


# the reference's own tests (wi_dlog_proof.rs:117-141), end to end: set-up, prove, verify
E2E = (2048, 6)          # n_bits, B: honest moduli only — every statement has a value


@functools.lru_cache(maxsize=None)
def e2e_moduli():
    n_bits, B = E2E
    return tuple(honest(n_bits, b) for b in range(B))
