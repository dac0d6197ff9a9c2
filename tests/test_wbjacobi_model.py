"""tools/wbjacobi_model.py — the word-for-word model of csrc/kernels_jacobi.hpp: wb_jacobi, with its integer ranges and the exactness of
every step asserted inside — against tests/jacobi_model.py on the hazard classes of tests/jacobi_cases.py, which are the GPU's cases too."""
import os
import sys

import pytest

import helpers as H
import jacobi_cases as JC
from jacobi_model import jacobi

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import wbjacobi_model as W  # noqa: E402


def _classes(mod_bits):
    out = {}
    for (tag, a, n), want in zip(JC.cases(mod_bits), JC.expected_all(mod_bits)):
        out.setdefault(tag, []).append((a, n, want))
    return out


def test_every_hazard_class_is_present_at_every_width():
    for mod_bits in JC.WIDTHS:
        c = _classes(mod_bits)
        assert set(c) == {"mod8xmod4", "mod8xmod4-small", "special-a", "pow2", "shared-factor", "special-n", "far-apart", "close-pow2", "close-random", "fibonacci",
                          "mod8-late", "domain", "random"}
        assert {(n % 8, a % 4) for a, n, _ in c["mod8xmod4"]} == {(m, r) for m in (1, 3, 5, 7) for r in range(4)}
        assert all(w == (0, 0) for _, _, w in c["shared-factor"]) and all(w == (0, 2) for _, _, w in c["domain"])
        assert len(c["random"]) == JC.RANDOM_PAIRS
        syms = {w[0] for ws in c.values() for _, _, w in ws}
        assert syms == {-1, 0, 1}
        # close pairs: the operands agree in at least their top 64 bits
        for a, n, _ in c["close-pow2"] + c["close-random"]:
            bits = max(a.bit_length(), n.bit_length())
            assert a != n and (a >> (bits - 64)) - (n >> (bits - 64)) in (-1, 0, 1)


@pytest.mark.parametrize("mod_bits", JC.WIDTHS)
def test_word_model_against_the_definition(mod_bits):
    kw = mod_bits // 32
    exact_steps = early = 0
    for tag, ws in _classes(mod_bits).items():
        if tag == "domain":
            continue
        if tag == "random" and mod_bits > 1024:
            ws = ws[:40]                           # (the model takes 20 ms per pair at 4096 bits; the GPU runs them all)
        for a, n, want in ws:
            tr = []
            assert W.wbjacobi(a, n, kw, tr) == want[0], (tag, hex(a), hex(n))
            assert len(tr) <= 64 * kw // 28 + 8 or tag != "random"
            exact_steps += sum(r["exact_step"] for r in tr)
            early += sum(r["early"] for r in tr)
    # the close pairs really send the model through the step that an approximation cannot decide
    assert exact_steps >= 50, exact_steps
    print(mod_bits, "rounds decided on the full operands:", exact_steps, "rounds ended early:", early)


def test_the_committed_mod8_pairs_have_the_property_they_were_found_for():
    for a, n in JC.MOD8_LATE:
        tr = []
        assert W.wbjacobi(a, n, 32, tr) == jacobi(a, n)
        assert tr[0]["steps"] == W.K and tr[0]["i_mod8"] == W.K - 1
        assert sum(1 for r in tr if r["steps"] == W.K and r["i_mod8"] == W.K - 1) >= 0.6 * len(tr)


def test_a_sign_bit_on_the_gcd_rounds_would_be_wrong():
    """what the header of kernels_jacobi.hpp argues: K = 30 steps on 30 exact low bits read bits that are not the operand's — the model's
    own assertion of exact low bits fails for such a round"""
    saved = W.K
    W.K = 30
    try:
        with pytest.raises(AssertionError):
            for a, n in JC.MOD8_LATE:
                W.wbjacobi(a, n, 32)
    finally:
        W.K = saved
