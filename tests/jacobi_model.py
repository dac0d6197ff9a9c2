"""The Jacobi symbol from its definition, on Python ints: the textbook binary algorithm (halve an even a with the rule for (2 / n),
swap by quadratic reciprocity, reduce).  It has none of the structure of csrc/kernels_jacobi.hpp or tools/wbjacobi_model.py — no
approximations, no rounds, no matrix — and is the checker both are held to.  tests/test_jacobi_model.py pins it.

legendre_symbol is the reference's function (wi_dlog_proof.rs:94-107), word for word: Euler's criterion with the exponent
(p - 1) * 2^-1 mod p, 1 iff the power is 1 and -1 otherwise — so a = 0 mod p and a composite p give -1, not 0."""


def jacobi(a, n):
    """(a / n) for an odd n > 0 and any integer a >= 0"""
    assert n > 0 and n & 1 and a >= 0
    a %= n
    s = 1
    while a:
        while not a & 1:
            a >>= 1
            if n & 7 in (3, 5):
                s = -s
        a, n = n, a
        if a & 3 == 3 and n & 3 == 3:
            s = -s
        a %= n
    return s if n == 1 else 0


def legendre_symbol(a, p):
    """the reference's legendre_symbol(a, p); None where it panics (mod_inv(2, p) has no result: p even) or where p < 3"""
    if p < 3 or p % 2 == 0:
        return None
    e = ((p - 1) * pow(2, -1, p)) % p
    return 1 if pow(a, e, p) == 1 else -1
