"""What zkp_correct_key_ni_prove_batch computes (include/zkp_hip.h), on Python integers: for a key (p, q) and a salt -> (n, [sigma_i], status).
rho is oracle/py_model.correct_key_rho (the hash helpers of the verify tests).  sigma is DEFINED by the header's CRT formulas — no primality
test is made, the formulas are applied to the key the caller gave — and `plain` is the reference's statement, rho^(n^-1 mod phi(n)) mod n:
for prime p and q the two are the same number, for every rho (tests/test_ck_prove_model.py asserts it for every such case key, against the
oracle too).  Under composite factors (the add-back key of tests/paillier_dec_cases.py) they differ, because the order of rho modulo p need
not divide p - 1, and the library's value is the formulas'."""
from math import gcd

from oracle import py_model as pm

M2 = 11


def status(p, q):
    """the domain rules of zkp_paillier_open_batch's keys"""
    if p < 3 or q < 3 or p % 2 == 0 or q % 2 == 0:
        return 2
    return 0 if gcd(p, q) == 1 and gcd(q, p - 1) == 1 and gcd(p, q - 1) == 1 else 2


def crt(p, q, rho):
    dp, dq, pinv = pow(q, -1, p - 1), pow(p, -1, q - 1), pow(p, -1, q)
    sp, sq = pow(rho % p, dp, p), pow(rho % q, dq, q)
    return sp + p * ((sq - sp) * pinv % q)


def plain(p, q, rho):
    n = p * q
    return pow(rho, pow(n, -1, (p - 1) * (q - 1)), n)


def prove(p, q, salt):
    if status(p, q):
        return 0, [0] * M2, 2
    n = p * q
    return n, [crt(p, q, rho) for rho in pm.correct_key_rho(n, salt)], 0
