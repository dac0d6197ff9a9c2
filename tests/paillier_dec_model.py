"""Paillier decrypt and open with the factors, from the definitions (include/zkp_hip.h: zkp_paillier_open_batch) in Python integers, and the
upstream shape — c^lambda mod n^2, floor-division L, mu, the root as (c mod n)^(n^-1 mod phi) mod n — that the definitions must agree with
on every item inside the domain.  Status 0 is good, 2 (ZKP_VERDICT_MALFORMED) is outside the domain: outputs zero."""
import functools
from math import gcd

MALFORMED = 2


def key_constants(p, q):
    """(h_p, h_q, pinv, d_p, d_q), or None for a key outside the domain"""
    if p < 3 or q < 3 or p % 2 == 0 or q % 2 == 0:
        return None
    if gcd(p, q) != 1 or gcd(q, p - 1) != 1 or gcd(p, q - 1) != 1:
        return None
    return (pow(p - q % p, -1, p), pow(q - p % q, -1, q), pow(p, -1, q), pow(q, -1, p - 1), pow(p, -1, q - 1))


def open(p, q, c):
    """(m, r, status) by the CRT formulas; c is any non-negative value"""
    k = key_constants(p, q)
    if k is None:
        return 0, 0, MALFORMED
    hp, hq, pinv, dp, dq = k
    xp, xq = pow(c % (p * p), p - 1, p * p), pow(c % (q * q), q - 1, q * q)
    if xp % p != 1 or xq % q != 1:
        return 0, 0, MALFORMED
    mp, mq = (xp - 1) // p * hp % p, (xq - 1) // q * hq % q
    m = mp + p * ((mq - mp) * pinv % q)
    rp, rq = pow(c % p, dp, p), pow(c % q, dq, q)
    r = rp + p * ((rq - rp) * pinv % q)
    return m, r, 0


@functools.lru_cache(maxsize=None)
def _upstream_key(p, q):
    """(lambda, mu, n^-1 mod phi): per key, as the upstream key set-up computes them once"""
    n, phi = p * q, (p - 1) * (q - 1)
    lam = phi // gcd(p - 1, q - 1)
    mu = pow((pow(1 + n, lam, n * n) - 1) // n, -1, n)
    return lam, mu, pow(n, -1, phi)


def open_upstream(p, q, c):
    """(m, r) as the textbook scheme computes them; meaningful for a valid key and a c coprime to n only"""
    n = p * q
    lam, mu, ninv = _upstream_key(p, q)
    m = (pow(c, lam, n * n) - 1) // n * mu % n
    r = pow(c % n, ninv, n)
    return m, r
