"""CPU tests of the model of zkp_correct_key_ni_prove_batch (tests/ck_prove_model.py) on the case list of tests/ck_prove_cases.py: for every
good case key with prime factors the model equals the oracle's NiCorrectKeyProof::proof, the CRT formulas equal the plain power
rho^(n^-1 mod phi) and sigma^n = rho; the domain batch has the statuses the issue asks for; under the composite add-back key the formulas'
value is NOT the plain power (why the model is stated by the formulas)."""
import pytest

import ck_prove_cases as CC
import ck_prove_model as M
from helpers import L
from oracle import py_model as pm

BATCHES = CC.all_batches()


@pytest.mark.parametrize("name", [n for n, _ in BATCHES])
def test_model_equals_oracle_and_plain_power(oracle, name):
    b = dict(BATCHES)[name]
    hw, checked = b["n_bits"] // 64, 0
    for salt in CC.SALTS:
        for (p, q), prime, (n, sigma, st) in zip(b["keys"], b["prime"], b["want"][salt]):
            if st or not prime:
                continue
            rho = pm.correct_key_rho(n, salt)
            on, osig = oracle.correct_key_ni_prove(b["n_bits"], L.int_to_limbs(p, hw), L.int_to_limbs(q, hw), salt)
            assert L.limbs_to_int(on) == n == p * q and L.limbs_to_ints(osig) == sigma
            assert sigma == [M.plain(p, q, r) for r in rho]
            assert [pow(s, n, n) for s in sigma] == rho
            checked += 1
    assert checked >= (5 if name == "domain" else len(b["keys"])) * len(CC.SALTS)


def test_domain_statuses():
    b = CC.domain()
    st = {t: w[2] for t, w in zip(b["tag"], b["want"][CC.SALTS[0]])}
    assert [t for t, s in st.items() if s == 2] == ["even p", "p=1", "p=q", "q=0", "q | p-1"]
    assert sum(s == 0 for s in st.values()) >= 5
    for salt in CC.SALTS:
        assert all(w[0] == 0 and w[1] == [0] * 11 for w in b["want"][salt] if w[2] == 2)


def test_composite_factors_take_the_formulas_value():
    p, q = CC.PC.ADD_BACK_KEY
    assert M.status(p, q) == 0
    n, sigma, st = M.prove(p, q, CC.SALTS[0])
    rho = pm.correct_key_rho(n, CC.SALTS[0])
    assert st == 0 and n == p * q and sigma == [M.crt(p, q, r) for r in rho] and all(0 <= s < n for s in sigma)
    assert sigma != [M.plain(p, q, r) for r in rho]
