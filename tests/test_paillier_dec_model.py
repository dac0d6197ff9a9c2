"""CPU tests of zkp_paillier_open_batch's definitions and of the word-level routines of csrc/kernels_paillier_dec.hpp: the CRT formulas
(tests/paillier_dec_model.py) against the upstream shape and against what was encrypted, on the case list the GPU tests share; the word
model (tools/paillier_dec_model.py: Knuth's algorithm D, the digit-serial exact division, the inverse modulo the even p - 1) against
Python's integers, with its range assertions live; and the export of the new symbol."""
import functools
import importlib.util
import os
import random

import numpy as np
import pytest

import helpers as H
import paillier_dec_cases as PC
import paillier_dec_model as M
from helpers import zkp

# (tests/paillier_dec_model.py has the same module name: the word model is loaded by file)
_spec = importlib.util.spec_from_file_location("paillier_dec_word_model", os.path.join(H.ROOT, "tools", "paillier_dec_model.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)


_is_prime = functools.lru_cache(maxsize=None)(H.is_probable_prime)


def _key(b, i):
    return b["keys"][i if len(b["keys"]) > 1 else 0]


@pytest.mark.parametrize("name", [n for n, _ in PC.all_batches()])
def test_definitions_agree_with_the_upstream_shape_and_with_what_was_encrypted(name):
    b = dict(PC.all_batches())[name]
    good = [i for i, w in enumerate(b["want"]) if w[2] == 0 and all(_is_prime(f) for f in _key(b, i))]
    assert len(good) >= 6 and (name == "domain" or len(good) == len(b["c"]))
    for i in good:                                          # EVERY good item of the list (the per-key values of the upstream shape are kept)
        assert M.open_upstream(*_key(b, i), b["c"][i]) == b["want"][i][:2], b["tag"][i]
    if name == "per-item keys":
        assert len({_key(b, i) for i in good}) == 5
    for want, truth in zip(b["want"], b["truth"]):
        if truth is not None:
            assert want == (truth[0], truth[1], 0)


def test_case_list_holds_what_the_gpu_tests_rely_on():
    d = PC.domain()
    assert d["tag"].count("c=0") == 1 and sum(w[2] == 2 for w in d["want"]) >= 9 and sum(w[2] == 0 for w in d["want"]) >= 12
    for i, w in enumerate(d["want"]):                       # every bad item sits between good neighbours
        if w[2] == 2:
            assert d["want"][i - 1][2] == 0 and (i + 1 == len(d["want"]) or d["want"][i + 1][2] == 0)
    k = PC.per_item_keys()
    assert len(set(k["keys"])) == 5 and len(k["c"]) == 40
    for n_bits in (1024, 2048):
        assert len(PC.one_key(n_bits)["c"]) == 70 > 4 * 16
    w = PC.widened(PC.one_key(1024))
    assert all(c2 > c1 for c1, c2 in zip(PC.one_key(1024)["c"], w["c"]))


def test_key_constants_are_the_issue_s_identities():
    for bits in (1024, 2048):
        p, q, n = H.test_key(bits)
        hp, hq, pinv, dp, dq = M.key_constants(p, q)
        L = lambda u, f: (u - 1) // f
        assert hp == pow(L(pow(1 + n, p - 1, p * p), p), -1, p) and hq == pow(L(pow(1 + n, q - 1, q * q), q), -1, q)
        assert dp == pow(n, -1, p - 1) and dq == pow(n, -1, q - 1) and pinv * p % q == 1
        assert hq == q - pinv


# ---- the word model against Python's integers
def _mod_cases(rnd, nx, nm):
    """(x, m): random, and the shapes that drive algorithm D's estimate to its corrections and its add-back"""
    top = 1 << (32 * nm)
    out = []
    for _ in range(60):
        out.append((rnd.getrandbits(32 * nx), rnd.getrandbits(32 * nm) | 1))
    for _ in range(60):
        m = (1 << (32 * nm - 1)) | (rnd.getrandbits(32 * (nm - 1)) if nm > 1 else 0) | ((W.M32 << (32 * (nm - 2))) if nm > 1 else 0)
        m %= top
        k = rnd.getrandbits(32 * (nx - nm))
        out.append(((k * m + m - 1 - rnd.getrandbits(8)) % (1 << (32 * nx)), m))
        out.append(((m << (32 * (nx - nm))) - 1, m))
    out += [(0, 1), (top - 1, 1), ((1 << (32 * nx)) - 1, top - 1), ((1 << (32 * nx)) - 1, 3), (5, top - 1)]
    if nm > 2:
        out.append((rnd.getrandbits(32 * nx), rnd.getrandbits(32 * (nm - 2) - 5) | 1))      # a divisor two words and some bits short
    return [(x, m) for x, m in out if m]


@pytest.mark.parametrize("nx,nm", [(4, 2), (8, 4), (6, 3), (4, 4), (2, 1), (64, 32), (33, 32)])
def test_pd_mod_is_the_remainder(nx, nm):
    rnd = random.Random(nx * 100 + nm)
    stats = {}
    for x, m in _mod_cases(rnd, nx, nm):
        got = W.pd_mod(W.to_words(x, nx) + [0], nx, W.to_words(m, nm), stats)
        assert W.from_words(got) == x % m, (hex(x), hex(m))
    if nm >= 2 and nx > nm:
        assert stats["corrections"] > 0


def test_pd_mod_add_back_on_knuth_s_example():
    """the textbook operands whose quotient estimate survives the two-digit test and is still one too large (base 2^32): random operands
    reach that branch about once in 2^31 digits.  The case list's "add-back key" takes the GPU through it in the key preparation."""
    u, v = 0x7fffffff_80000000_00000000_00000000, 0x80000000_00000000_00000001
    stats = {}
    got = W.pd_mod(W.to_words(u, 4) + [0], 4, W.to_words(v, 3), stats)
    assert W.from_words(got) == u % v and stats["addbacks"] >= 1
    p, q = PC.ADD_BACK_KEY
    stats = {}
    assert W.from_words(W.pd_mod(W.to_words(q, 16) + [0], 16, W.to_words(p, 16), stats)) == q % p and stats["addbacks"] == 1


@pytest.mark.parametrize("nd", [1, 2, 16, 32])
def test_pd_divexact_divides_and_detects(nd):
    rnd = random.Random(nd)
    for _ in range(40):
        d = rnd.getrandbits(32 * nd) | 1
        q = rnd.getrandbits(32 * nd)
        got, exact = W.pd_divexact(W.to_words(q * d, 2 * nd), W.to_words(d, nd), nd)
        assert exact and W.from_words(got) == q
        off = q * d + rnd.randrange(1, d) if d > 1 else None
        if off is not None and off < 1 << (64 * nd):
            assert not W.pd_divexact(W.to_words(off, 2 * nd), W.to_words(d, nd), nd)[1]
    # x_p = 0: the kernel's x_p - 1 wraps to all ones, which no quotient below 2^(32 nd) reaches
    for d in (3, (1 << (32 * nd)) - 1, rnd.getrandbits(32 * nd) | 1):
        assert not W.pd_divexact([W.M32] * (2 * nd), W.to_words(d, nd), nd)[1]


def test_inverse_modulo_the_even_p_minus_1():
    for bits in (1024, 2048):
        p, q, n = H.test_key(bits)
        hw = bits // 64
        assert W.inv_even(p, pow(p - 1, -1, q), q, hw) == pow(q, -1, p - 1)
        assert W.inv_even(q, pow(q - 1, -1, p), p, hw) == pow(p, -1, q - 1)
    assert W.inv_even(7, pow(6, -1, 5), 5, 1) == pow(5, -1, 6) and W.inv_even(3, pow(2, -1, 5), 5, 1) == pow(5, -1, 2)


@pytest.mark.parametrize("name", ["one key 1024", "per-item keys", "domain"])
def test_word_model_of_the_whole_item_against_the_definitions(name):
    b = dict(PC.all_batches())[name]
    step = 1 if name == "domain" else 3
    for i in range(0, len(b["c"]), step):
        p, q = _key(b, i)
        assert W.open_words(p, q, b["c"][i], b["n_bits"] // 64) == b["want"][i], b["tag"][i]
    w = PC.widened(b) if name != "domain" else None
    if w:
        for i in range(0, len(w["c"]), 7):
            assert W.open_words(*_key(w, i), w["c"][i], w["n_bits"] // 64) == w["want"][i]


def test_new_entry_point_is_exported_and_refuses_a_null_ctx_without_a_gpu():
    """(the other argument checks need a context, which needs a GPU: tests/test_gpu_paillier_dec.py::test_bad_arguments)"""
    lib = zkp.load()
    assert hasattr(lib, "zkp_paillier_open_batch") and "zkp_paillier_open_batch" in zkp.EXPORTS
    assert callable(zkp.Context.paillier_open)
    a = np.zeros(64, np.uint32)
    assert lib.zkp_paillier_open_batch(None, 1024, 1, a.ctypes.data, a.ctypes.data, 0, a.ctypes.data, a.ctypes.data, None, None, 0) == zkp.capi.ZKP_EINVAL
    assert lib.zkp_paillier_open_batch(None, 1024, 0, None, None, 0, None, None, None, None, 0) == zkp.capi.ZKP_EINVAL
