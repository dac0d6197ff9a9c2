"""tests/jacobi_model.py — the checker of the Jacobi kernel and of its word model — pinned against what defines the symbol: Euler's criterion
for primes, multiplicativity over N = p q, and a brute-force table of quadratic residues for every odd n below 200."""
import random

import helpers as H
import jacobi_cases as JC
from jacobi_model import jacobi, legendre_symbol


def test_euler_criterion_for_the_fixture_primes():
    rnd = random.Random(11)
    for p in JC.fixture_primes():
        assert H.is_probable_prime(p)
        for a in [0, 1, 2, p - 1, p, p + 1] + [rnd.randrange(2 * p) for _ in range(60)]:
            e = pow(a, (p - 1) // 2, p)
            want = 0 if e == 0 else 1 if e == 1 else -1
            assert e in (0, 1, p - 1) and jacobi(a, p) == want, a
            # the reference's legendre_symbol: the same, except that a multiple of p gives -1
            assert legendre_symbol(a, p) == (want if want else -1), a


def test_multiplicative_over_pq():
    rnd = random.Random(12)
    p, q = JC.fixture_primes()
    n = p * q
    seen = set()
    for a in [0, 1, 2, p, q, 3 * p, n - 1, n + 1] + [rnd.randrange(n) for _ in range(60)]:
        assert jacobi(a, n) == jacobi(a, p) * jacobi(a, q), a
        seen.add(jacobi(a, n))
    assert seen == {-1, 0, 1}
    for a, b in [(rnd.randrange(n), rnd.randrange(n)) for _ in range(30)]:
        assert jacobi(a * b, n) == jacobi(a, n) * jacobi(b, n)


def _brute(a, n):
    """the symbol from the factorisation of n and the list of squares modulo each prime"""
    s, m, p = 1, n, 3
    while m > 1:
        while m % p == 0:
            m //= p
            r = a % p
            s *= 0 if r == 0 else 1 if r in {x * x % p for x in range(1, p)} else -1
        p += 2
    return s


def test_brute_force_table_below_200():
    for n in range(1, 200, 2):
        for a in range(0, 2 * n + 2):
            assert jacobi(a, n) == _brute(a, n), (a, n)


def test_legendre_symbol_where_the_reference_panics_or_differs():
    assert legendre_symbol(3, 10) is None and legendre_symbol(1, 2) is None and legendre_symbol(0, 1) is None
    assert legendre_symbol(0, 7) == -1 and jacobi(0, 7) == 0
    assert legendre_symbol(2, 15) == -1 and jacobi(2, 15) == 1        # a composite "p": Euler's criterion fails, the Jacobi symbol is defined
