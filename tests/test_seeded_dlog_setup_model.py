"""CPU tests of the seeded DLogStatement set-up: the Python restatement of the rule (tests/seeded_dlog_setup_model.py) against hand-built
candidates and against the samplers it extends, the statement that the GPU cases of tests/seeded_dlog_setup_cases.py contain every sort of
acceptance and rejection, the word model of the device's Jacobi loop on the very candidates the kernel will test, and the new entry points in
the built library."""
import os
import sys

import pytest

import helpers as H
import seeded_coprime_model as CM
import seeded_dlog_setup_cases as DC
import seeded_dlog_setup_model as M
from jacobi_model import jacobi

zkp = H.zkp
SEED = DC.SEED


def test_word_15_of_the_new_stream():
    assert M.word15(0) == 0x80800000 and M.word15(1) == 0x80800001
    # apart from every stream of kinds 1 .. 7 (slot < 65536, field < 16): kind 4 — the DLog prover's nonce — included
    assert M.word15(0) > 0x80000000 | (7 << 20) | (65535 << 4) | 15
    assert CM.word15(CM.KIND_MUL, 0, 1) < M.word15(0)
    with pytest.raises(AssertionError):
        M.word15(2)


@pytest.mark.parametrize("n", [15, DC.ABOVE(1024), DC.honest(2048, 0), DC.honest(4096, 2)])
def test_the_candidates_are_those_of_sample_below(n):
    """equal state words -> equal draws: the range model's sample_below with the word 15 of kind 8 swapped in sees the same candidates"""
    index = DC.BIG + 2
    w15 = M.word15(M.FIELD_H1)
    v, rejected = M.R.sample_below(SEED, index, w15 >> 2, w15 & 3, n)
    cands = [M.candidate(SEED, index, n, t) for t in range(rejected + 1)]
    assert cands[rejected] == v and all(c >= n for c in cands[:rejected])
    # and seeded_coprime_model.candidate's construction, block for block
    bits = n.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    words = sum((M.block(SEED, 3 * nb + k, index, M.FIELD_H1) for k in range(nb)), [])
    assert M.candidate(SEED, index, n, 3) == sum(x << (32 * i) for i, x in enumerate(words[:nw])) & ((1 << bits) - 1)


def test_attempt_order_and_the_shared_counter():
    for n in (15, 21, DC.ABOVE(1024), DC.honest(1024, 1)):
        for index in (0, DC.BIG + 1):
            v, not_below, symbol = M.sample_jacobi_minus_below(SEED, index, n)
            t = not_below + symbol
            cands = [M.candidate(SEED, index, n, k) for k in range(t + 1)]
            assert v == cands[t] and v + 1 < n and jacobi(v, n) == -1
            assert sum(1 for x in cands[:t] if x + 1 >= n) == not_below
            assert sum(1 for x in cands[:t] if x + 1 < n and jacobi(x, n) != -1) == symbol


def test_the_secret_is_block_0_of_field_1():
    x = M.secret(SEED, 7)
    assert x == sum(w << (32 * i) for i, w in enumerate(M.block(SEED, 0, 7, 1)[:8])) and x < 1 << 256
    assert x != M.secret(SEED, 8)


def test_failing_statements_leave_their_neighbours_alone():
    n = DC.honest(1024, 0)
    alone, st, _, _ = M.statements(SEED, 11, [n] * 5)
    mixed, status, _, symbol = M.statements(SEED, 11, [n, 0, n - 1, DC.square(), n])
    assert st == [0] * 5 and status == [0, M.MALFORMED, M.MALFORMED, M.MALFORMED, 0]
    assert mixed[0] == alone[0] and mixed[4] == alone[4] and mixed[1] == mixed[2] == mixed[3] == dict(g=0, ni=0, secret=0)
    assert symbol[3] >= 1
    assert M.statements(SEED, 12, [n] * 4)[0] == alone[1:]        # the index of statement b is first_index + b
    for s in alone:
        assert jacobi(s["g"], n) == -1 and s["ni"] * pow(s["g"], s["secret"], n) % n == 1


def test_a_square_modulus_runs_out_of_attempts():
    n = DC.square()
    v, not_below, symbol = M.sample_jacobi_minus_below(SEED, DC.BIG + DC.SQUARE_ROW, n)
    assert v is None and not_below + symbol == M.MAX_ATTEMPTS == 128 and symbol >= 60
    assert all(jacobi(M.candidate(SEED, DC.BIG + DC.SQUARE_ROW, n, t), n) in (0, 1) for t in range(8))


@pytest.mark.parametrize("n_bits", DC.WIDTHS)
def test_the_gpu_cases_contain_every_sort_of_acceptance_and_rejection(n_bits):
    seen0 = seen_symbol3 = seen_not_below = False
    for B in DC.BATCHES:
        ns = DC.moduli(n_bits, B)
        st, status, not_below, symbol = DC.model(n_bits, B)
        assert len(ns) == B and all(n.bit_length() <= n_bits for n in ns)
        want_bad = {DC.SQUARE_ROW, DC.EVEN_ROW} if B > 1 else set()
        assert {b for b in range(B) if status[b]} == want_bad
        for b in range(B):
            if status[b]:
                assert st[b] == dict(g=0, ni=0, secret=0)
                continue
            assert 1 < st[b]["g"] + 1 < ns[b] and jacobi(st[b]["g"], ns[b]) == -1 and not_below[b] + symbol[b] < 40
        ok = [b for b in range(B) if not status[b]]
        seen0 = seen0 or any(not_below[b] + symbol[b] == 0 for b in ok)
        seen_symbol3 = seen_symbol3 or any(symbol[b] >= 3 for b in ok)
        seen_not_below = seen_not_below or any(not_below[b] >= 1 and ns[b] == DC.ABOVE(n_bits) for b in ok)
        if B > 1:
            assert not_below[DC.SQUARE_ROW] + symbol[DC.SQUARE_ROW] == M.MAX_ATTEMPTS
            diff = sum(1 for b in range(B - 1) if not_below[b] + symbol[b] != not_below[b + 1] + symbol[b + 1])
            assert diff >= B // 3, "neighbouring lanes are to need different numbers of attempts"
    assert seen0 and seen_symbol3 and seen_not_below, (seen0, seen_symbol3, seen_not_below)


def test_the_word_model_of_the_device_loop_agrees_on_the_candidates_the_kernel_tests():
    """tools/wbjacobi_model.py is wb_jacobi word for word; k_nonce_jacobi calls it with (candidate, N) at the call's kernel width"""
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import wbjacobi_model as W
    for n_bits in (1024, 2048):
        ns = DC.moduli(n_bits, 65)
        first = DC.first_index(n_bits, 65)
        for b in (0, 1, 2, DC.SQUARE_ROW, 9):
            for t in range(4):
                v = M.candidate(SEED, first + b, ns[b], t)
                if v + 1 < ns[b]:
                    assert W.wbjacobi(v, ns[b], n_bits // 32) == jacobi(v, ns[b])


def test_the_models_statements_are_what_the_reference_sets_up():
    """wi_dlog_proof.rs:117-141 with p and q at hand: legendre(h1, p) legendre(h1, q) == -1 for the h1 made without them"""
    from jacobi_model import legendre_symbol
    p, q, n = H.fixture_key()
    st, status, _, _ = M.statements(SEED, 0, [n] * 8)
    assert not any(status)
    for s in st:
        assert legendre_symbol(s["g"], p) * legendre_symbol(s["g"], q) == -1
        assert s["ni"] == pow(pow(s["g"], -1, n), s["secret"], n) and s["secret"] < 1 << 256


def test_new_entry_points_are_exported_and_refuse_bad_arguments_without_a_gpu():
    lib = zkp.load()
    for name in ("zkp_jacobi_batch", "zkp_legendre_batch", "zkp_dlog_statement_setup_seeded_batch"):
        assert hasattr(lib, name) and name in zkp.EXPORTS, name
    for method in ("jacobi", "legendre", "dlog_statement_setup_seeded"):
        assert callable(getattr(zkp.Context, method))
    assert zkp.capi.SEEDED_KIND_DLOG_SETUP == M.KIND_DLOG_SETUP == 8
    E = zkp.capi.ZKP_EINVAL
    assert lib.zkp_jacobi_batch(None, 1024, 1, None, None, 0, None, None, 0) == E
    assert lib.zkp_legendre_batch(None, 2048, 1, None, None, 0, None, None, 0) == E
    assert lib.zkp_dlog_statement_setup_seeded_batch(None, 1024, 1, None, bytes(32), 0, None, None, None, None, 0) == E
