"""GPU parity: NiCorrectKeyProof::verify (correct_key_ni.rs:73-100) against the oracle."""
import functools
import importlib

import numpy as np
import pytest

import dlog_cases as D
import helpers as H
from helpers import pm, L, zkp

pytestmark = pytest.mark.gpu


def honest_keys(n_bits):
    if n_bits == 1024:
        return [H.test_key(n_bits, tag=t) for t in range(3)]
    if n_bits == 2048:
        return [H.fixture_key(), H.test_key(2048, 1)]
    # 4096 bits (another group size, twice the MGF bytes per rho_i, key windows over a 4096-bit exponent): the benchmark's key and the key
    # tests/test_gpu_fullsize.py generates, so that one run of the suite pays for it once
    synth = importlib.import_module("zk-paillier_amd.synth")
    return [synth.bench_key_4096(), H.test_key(4096, tag=3)]


# (the `ctx` fixture runs the test under five kernel families: what costs CPU time is computed once per process)
@functools.lru_cache(maxsize=None)
def small_factor_modulus(n_bits):
    """a modulus of n_bits bits with the factor 6361 (below the primorial's bound: gcd(n, primorial) != 1, correct_key_ni.rs:92-98)"""
    if n_bits < 4096:
        return 6361 * H.gen_prime(pm.Drbg(b"sf-%d" % n_bits), n_bits - 16)
    # no 4000-bit prime is generated: 6361 times three pooled 1024-bit primes (tests/dlog_cases.py) times a small key, top bit set
    for tag in range(40, 72):
        try:
            return D.pool_product(4096, 3, extra=6361 * H.test_key(1012, tag=tag)[2])[1]      # (exactly 4096 bits, or it raises)
        except AssertionError:
            continue
    raise AssertionError("no 4096-bit modulus with the factor 6361")


@functools.lru_cache(maxsize=None)
def short_key(n_bits, salt):
    """(n, sigma) of an honest proof under a key shorter than the ABI width: key_length drives the MGF length"""
    if n_bits < 4096:
        pk, qk, nk = H.test_key(n_bits - 64, tag=9)
        return nk, pm.correct_key_proof(pk, qk, salt)
    # three pooled primes, 3072 bits: sigma_i = rho_i^(n^-1 mod phi(n)) mod n with phi of the three factors
    fs, nk = D.pool_product(3072, 3)
    phi = (fs[0] - 1) * (fs[1] - 1) * (fs[2] - 1)
    d = pow(nk, -1, phi)
    return nk, [pow(rho, d, nk) for rho in pm.correct_key_rho(nk, salt)]


@pytest.mark.parametrize("n_bits,salt", [(1024, pm.SALT_STRING), (2048, bytes([90, 101, 110, 32, 71, 111, 32, 88])), (1024, b"\x00\x00ab"), (1024, b""), (4096, pm.SALT_STRING)])
def test_correct_key_verify(ctx, oracle, n_bits, salt):
    kw = n_bits // 32
    keys = honest_keys(n_bits)
    ns, sigmas = [], []
    for p, q, n in keys:
        nl, sg = oracle.correct_key_ni_prove(n_bits, L.int_to_limbs(p, kw // 2), L.int_to_limbs(q, kw // 2), salt)
        ns.append(nl); sigmas.append(sg)
    # tampered sigma, sigma + n (same residue: still accepted), sigma = 0 row, modulus with a small factor, short key
    ns.append(ns[0]); bad = sigmas[0].copy(); bad[7, 1] ^= 4; sigmas.append(bad)
    ns.append(ns[1]); plus = sigmas[1].copy()
    v = L.limbs_to_int(plus[2]) + keys[1][2]
    if v.bit_length() <= n_bits:
        plus[2] = L.int_to_limbs(v, kw)
    sigmas.append(plus)
    ns.append(ns[0]); z = sigmas[0].copy(); z[0] = 0; sigmas.append(z)
    n_small = small_factor_modulus(n_bits)
    ns.append(L.int_to_limbs(n_small, kw)); sigmas.append(L.ints_to_limbs(pm.correct_key_rho(n_small, salt), kw))
    nk, sigma_k = short_key(n_bits, salt)
    ns.append(L.int_to_limbs(nk, kw))
    sigmas.append(L.ints_to_limbs(sigma_k, kw))
    n_arr = np.stack(ns); s_arr = np.stack(sigmas)
    vo = oracle.correct_key_ni_verify(n_bits, n_arr, s_arr, salt)
    vg = np.full(len(ns), 7, np.uint8)
    ctx.correct_key_ni_verify(n_bits, len(ns), n_arr, s_arr, salt, vg)
    assert np.array_equal(vo, vg), (list(vo), list(vg))
    assert list(vo[:len(keys)]) == [zkp.VERDICT_ACCEPT] * len(keys)
    assert vo[len(keys)] == zkp.VERDICT_REJECT and vo[-1] == zkp.VERDICT_ACCEPT and vo[-2] == zkp.VERDICT_REJECT
