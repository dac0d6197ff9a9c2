"""Ciphertexts and keys that take zkp_paillier_open_batch through the rare branches of pd_mod (csrc/kernels_paillier_dec.hpp: Knuth's
algorithm D) at each of its call sites, built once and shared by tests/test_paillier_dec_branch_model.py (CPU) and
tests/test_gpu_paillier_dec_branches.py.  The batches have the layout of tests/paillier_dec_cases.py; every expected (m, r, status) is
tests/paillier_dec_model.py's (Python integers), and for encrypted items also what was encrypted.  The word model
(tools/paillier_dec_model.py) is used for one thing only: every crafted item carries its claims — (site, branch) pairs: the add-back positions
its builder certifies, and OTHER_BRANCHES below — and the CPU test holds the model's per-site records to them, so that a changed key or seed
cannot quietly lose a branch.  (The list of tests/paillier_dec_cases.py takes the add-back too, through r = n - 1, m = n - 1 and its add-back
key: always at position 0, the last step, never with an estimate of 2^32, never in vp mod q or in rows 1 and 2 of key preparation.)

One shape drives everything: an operand just BELOW a multiple of the divisor,  x = Qt F - delta  with Qt = 0 mod B^j (B = 2^32).
The true quotient is Qt - 1: digit j is one below Qt's and every digit under it is B - 1.  At step j the window is (digit of Qt) * F minus
something the estimate's three words cannot see when delta is small against (digit) * (F's words below the top two) * B^j: the estimate
passes the two-digit test one too large and the multiply-subtract borrows — the add-back.  From there on the running remainder is F - small,
its top word EQUALS the divisor's, and every lower digit starts from an estimate of 2^32 or 2^32 + 1: the `(qh >> 32) != 0` clause, and,
depending on the divisor's top words, the `rh >> 32` break (a top word v1 with a remainder word rh >= 2^32 - v1) or a second loop turn
(an estimate of 2^32 + 1: v2 >= v1 after normalisation).  A larger delta skips the add-back and keeps the rest.

How an item reaches a site:
 * split_sq (c mod F^2): c is free — for a key with prime factors every c coprime to n is a ciphertext.
 * split_root ((c mod F^2) mod F): the same shape below F^2.  The quotient is below F, so the positions end at nm - 1: the top steps
   (j >= nm) see a zero digit and a zero estimate — no add-back there, for any input.
 * finish_Lh (L h_F mod F): L = -m q mod p is the caller's through m.  L = floor((Qt F - 1) / h) puts L h within h below Qt F (j >= 1);
   for j = 0 the distance must be tiny: Qt = eps F^-1 mod h makes Qt F - eps an exact multiple of h.  The quotient is below h: positions
   end at nm - 1 here too.
 * crt_*_vp (vp mod q, p > q): vp = m mod p (r mod p) is the caller's.  With factors of one length there is one digit (m = q - 1 mod p);
   a key whose q is words shorter than p has more.
 * crt_*_prod (d pinv mod q): d = (v_q - v_p) mod q, chosen as L above, under either sign of v_q - v_p.
 * key_a (key preparation, rows 0 .. 3: q mod p, p mod q, (p - 1) mod q, (q - 1) mod p): the key itself, with composite factors for which
   every inverse exists (no primality test is made).  Rows 0 and 3 take the add-back together (q = Qt p - delta), rows 1 and 2 together
   (p = Qt q - delta); a row of each pair in one key is impossible: q >= p - delta and p >= q - delta' with both positive.

Gaps, with what was tried:
 * the add-back at the TOP step exists only where the operand can exceed the divisor times B^(nx - nm): split_sq (c < F^2: an estimate of 1
   for a digit of 0) and the crt_*_vp of a short q.  Elsewhere the quotient is below the divisor (split_root, finish_Lh, crt_*_prod: the
   highest position is nm - 1, taken) or has one digit (key rows 0 and 3, crt_*_vp under factors of one length).
 * a second loop turn needs a normalised divisor with v2 >= v1 (the estimate 2^32 + 1), which a key has or has not: p of K1, q^2 of K3 and
   q of B12 have it — split_sq_q, split_root_p, finish_Lh_p, crt_*_prod, key rows 1 and 2 at 1024 bits; finish_Lh_q, split_sq_q, split_root_q
   and crt_*_prod at 2048.  Neither short q has it, so crt_*_vp takes none; split_sq_p takes none either.
 * one-digit sites (crt_*_vp under K0 and K1r, key rows 0 and 3) have no digit under the add-back: no estimate of 2^32, no break there.
 * the `(qh >> 32) != 0` clause decides no value (UNOBSERVABLE), and rows 2 and 3 of the composite keys do not show (UNOBSERVABLE_ITEMS).

NOT reachable, and not searched for: the ck-prove split (mgf mod F), its pd_crt inputs (s_p = rho^dp mod p) and the strong test's squarings
(y^2 mod c) reduce hash outputs or powers, which nobody steers into a 2^-31 branch.  They run the same inlined routine — the reason to pin
it here."""
import functools
import importlib
import importlib.util
import itertools
import os
import random
from math import gcd

import helpers as H
import paillier_dec_cases as PC
import paillier_dec_model as M

# (tests/paillier_dec_model.py has the same module name: the word model is loaded by file)
_spec = importlib.util.spec_from_file_location("paillier_dec_word_model", os.path.join(H.ROOT, "tools", "paillier_dec_model.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

B = 1 << 32


def words(v):
    return (v.bit_length() + 31) // 32


def mod_stats(x, nx, F, fault=None):
    st = {}
    W.pd_mod(W.to_words(x, nx) + [0], nx, W.to_words(F, words(F)), st, fault)
    return st


def _unseen(F, j, digit):
    """the distance below (digit) F B^j that the estimate's three words cannot see (a quarter of it, to stay clear of the edge)"""
    nm, s = words(F), -F.bit_length() % 32
    low = (F << s) % (1 << (32 * max(nm - 2, 0)))
    return ((digit * low) << (32 * j)) >> (s + 2)


def below_multiple(rnd, F, nx, j, cap=None, high=False, seen=False):
    """x = Qt F - delta below cap (default B^nx), Qt = 0 mod B^j with a non-zero digit j; high: the largest such Qt.  delta is unseen by
    the estimate at step j: the add-back, certified by the word model.  seen: a small digit j and a delta that the two-digit test does
    see, yet below F's top word: no add-back at j (certified), the estimates of 2^32 under it."""
    cap = cap if cap is not None else 1 << (32 * nx)
    qt_max = (cap - 1) // F
    assert j >= 1 or not seen
    for turn in range(16):
        qt = qt_max if high and turn == 0 else rnd.randrange(qt_max // 2, qt_max + 1)
        qt = (qt >> (32 * j)) << (32 * j)
        if seen:
            qt = ((qt >> (32 * (j + 1))) << (32 * (j + 1))) + (rnd.randrange(1, 256) << (32 * j))
        if (qt >> (32 * j)) % B == 0:
            qt += 1 << (32 * j)
        if qt == 0 or qt > qt_max:
            continue
        bound = _unseen(F, j, (qt >> (32 * j)) % B)
        if seen:
            below_top = (F % (1 << (32 * (words(F) - 1)))) << (32 * j)
            assert 64 * bound < below_top // 2
            delta = rnd.randrange(64 * bound, below_top // 2)
        else:
            delta = rnd.randrange(bound // 2, bound) if bound >= 4 else 1
        x = qt * F - delta
        if not 0 <= x < cap:
            continue
        st = mod_stats(x, nx, F)
        if (j in st["addback_at"]) != seen and (not seen or st["overflows"] > 0):
            return x
    raise AssertionError("no operand below a multiple of F at position %d" % j)


def factor_below_multiple(rnd, F, h, nx, j):
    """L < F with L h = Qt F - delta taking the add-back at position j of the reduction modulo F (see the module's docstring)"""
    assert gcd(F, h) == 1 and h < F
    for _ in range(64):
        if j == 0:
            eps = rnd.randrange(1, 1 << 16)
            qt = eps * pow(F, -1, h) % h
            x = qt * F - eps
            assert x % h == 0
            L = x // h
        else:
            qt = (rnd.randrange(h // 2, h) >> (32 * j)) << (32 * j)
            if qt == 0:
                qt = (h >> (32 * j)) << (32 * j)
            L = (qt * F - 1) // h
        if 0 < L < F and j in mod_stats(L * h, nx, F)["addback_at"]:
            return L
    raise AssertionError("no factor whose product is below a multiple of F at position %d" % j)


def crt_pair(p, q, vp, vq):
    return vp + p * ((vq - vp) * pow(p, -1, q) % q)


def _far(rnd, q, hw):
    """v_q for an item with v_p = q - 1 mod q.  Without the add-back the lane keeps q - 1 - q = -1, all ones, and the difference it forms,
    v_q + 1 + q, is the true one plus q — the same recombination — unless it leaves its hw words: v_q is taken at or above B^hw - q, so that
    a missing add-back there shows in the outputs."""
    top = 1 << (32 * hw)
    assert 2 * q > top
    return rnd.randrange(top - q, q)


def _coprime(rnd, n):
    while True:
        r = rnd.randrange(2, n)
        if gcd(r, n) == 1:
            return r


# ---- keys
PRIME_KEYS = ("K0", "K0r", "K1", "K1r", "K3", "S0", "S31")        # (P03 and P12 are crafted in themselves)


@functools.lru_cache(maxsize=None)
def keys_1024():
    """K0: test_key(1024) with p > q (both squares have shift 0; the top words of p^2 and q^2 are 0xe021.. and 0x806e..); K1: a second key
    whose p^2 has shift 1 and the top word 0x6e6d.. — the break fires for one top word and not for the other; S0: a q of 224 bits (7 words,
    shift 0; q^2 14 words) and S31: a q of 225 bits (8 words, shift 31; q^2 15 words) under K0's larger factor — divisors shorter than a
    chunk, divisors whose length is no multiple of it, and a recombination with more than one quotient digit."""
    p0, q0, _ = H.test_key(1024, 0)
    p1, q1, _ = H.test_key(1024, 1)
    hi = max(p0, q0)
    k = dict(K0=(hi, min(p0, q0)), K0r=(min(p0, q0), hi), K1=(p1, q1), K3=H.test_key(1024, 3)[:2], S0=(hi, PC.short_prime(224)),
             S31=(hi, PC.short_prime(225)))
    assert (k["K1"][0] ** 2).bit_length() == 1023 and (k["K1"][1] ** 2).bit_length() == 1024
    assert words(k["S0"][1]) == 7 and words(k["S0"][1] ** 2) == 14 and words(k["S31"][1]) == 8 and words(k["S31"][1] ** 2) == 15
    return k


def _prime_below_multiple(rnd, F, nx, j):
    """a prime of the add-back shape: delta has hundreds of free bits, every few hundredth candidate is prime"""
    for _ in range(4000):
        x = below_multiple(rnd, F, nx, j)
        if x % 2 and H.is_probable_prime(x) and (j in mod_stats(x - 1, nx, F)["addback_at"]):
            return x
    raise AssertionError("no prime below a multiple of F")


@functools.lru_cache(maxsize=None)
def prime_keys_with_add_back(hw=16):
    """the composite keys' shapes with PRIME factors, so that every ciphertext is in the domain and the root exponents d_p, d_q (from rows
    2 and 3) show in the outputs: P03 — a p 12 bits short, q = Qt p - delta prime: rows 0 and 3; P12 — a q of 300 bits, p = Qt q - delta
    prime: rows 1 and 2 at position 3."""
    rnd = random.Random(500 + hw)
    d = H.pm.Drbg(b"paillier-dec-prime-add-back-%d" % hw)
    p = H.gen_prime(d, 32 * hw - 12)
    q = H.gen_prime(d, 300)
    k = dict(P03=(p, _prime_below_multiple(rnd, p, hw, 0)), P12=(_prime_below_multiple(rnd, q, hw, (hw - 10) // 2), q))
    assert all(M.key_constants(*v) is not None for v in k.values())
    return k


def _inverses_exist(p, q):
    return p % 2 == 1 and q % 2 == 1 and gcd(p, q) == 1 and gcd(p - 1, q) == 1 and gcd(q - 1, p) == 1


@functools.lru_cache(maxsize=None)
def composite_keys(hw=16):
    """keys with composite factors inside the domain (every inverse exists):
    A03: q = Qt p - delta with p 12 bits short of its words (shift 12): the add-back in rows 0 and 3, the one digit there is;
    B12: p = Qt q - delta with a q of 300 bits (shift 20, 10 words): the add-back in rows 1 and 2 at a middle position of 7;
    C: p a product of two primes, q prime: nothing special in key preparation — a generic c fails x_p = 1 mod p in the finish."""
    rnd = random.Random(300 + hw)
    bits = 32 * hw
    out = {}
    while "A03" not in out:
        p = rnd.getrandbits(bits - 12) | (1 << (bits - 13)) | 1
        q = below_multiple(rnd, p, hw, 0)
        st = mod_stats(q - 1, hw, p)
        if _inverses_exist(p, q) and st["addback_at"] == [0] and not H.is_probable_prime(p):
            out["A03"] = (p, q)
    while "B12" not in out:
        q = rnd.getrandbits(300) | (1 << 299) | 1
        j = (hw - 10) // 2
        p = below_multiple(rnd, q, hw, j)
        st = mod_stats(p - 1, hw, q)
        if _inverses_exist(p, q) and j in st["addback_at"] and not H.is_probable_prime(q):
            out["B12"] = (p, q)
    if hw == 16:
        d = H.pm.Drbg(b"paillier-dec-composite-%d" % hw)
        p, q = H.gen_prime(d, bits // 2) * H.gen_prime(d, bits // 2), keys_1024()["K0"][1]
        assert _inverses_exist(p, q)
        out["C"] = (p, q)
    return out


# ---- items: (tag, key name, c, truth | None)
def _enc(n, m, r):
    return H.python_enc(n, m, r)


def _split_items(rnd, keys):
    out = []
    kw = 32

    def sq(tag, kn, side, j, **kwargs):
        F = keys[kn][side]
        out.append(("%s %s %s" % (tag, kn, "pq"[side]), kn, below_multiple(rnd, F * F, 2 * kw, j, **kwargs), None,
                    [] if kwargs.get("seen") else [("split_sq_" + "pq"[side], j)]))

    sq("sq@32", "K0", 0, 32)                                     # the top step: c < p^2, the estimate is 1
    sq("sq@15", "K0", 0, 15)
    sq("sq@0", "K0", 0, 0)
    sq("sq@31", "K0", 1, 31)
    sq("sq@1", "K0", 1, 1)
    sq("sq@0", "K0", 1, 0, high=True)
    sq("sq@15 high", "K1", 0, 15, high=True)                     # shift 1 and c in the top of the range: the scratch word x[nx] is not zero
    sq("sq@0 high", "K1", 0, 0, high=True)
    sq("sq@32", "K1", 0, 32)                                     # the top step under shift 1
    sq("sq@20", "K1", 1, 20)
    sq("sq seen@9", "K0", 0, 9, seen=True)                       # no add-back at 9, estimates of 2^32 below it
    sq("sq seen@9", "K0", 1, 9, seen=True)
    sq("sq seen@9", "K1", 0, 9, seen=True)
    sq("sq@12", "K3", 1, 12)                                     # q^2 with v2 >= v1: estimates of 2^32 + 1, two loop turns
    sq("sq@25", "S0", 1, 25)                                     # q^2 of 14 words, shift 0
    sq("sq@50", "S0", 1, 50)
    sq("sq@0", "S31", 1, 0)                                      # q^2 of 15 words
    sq("sq@49", "S31", 1, 49)

    def root(tag, kn, side, j, **kwargs):
        F = keys[kn][side]
        out.append(("%s %s %s" % (tag, kn, "pq"[side]), kn, below_multiple(rnd, F, kw, j, cap=F * F, **kwargs), None,
                    [] if kwargs.get("seen") else [("split_root_" + "pq"[side], j)]))

    root("root@15", "K0", 0, 15, high=True)                      # the highest position a quotient below F has
    root("root@7", "K0", 0, 7)
    root("root@0", "K0", 0, 0)
    root("root@7", "K0", 1, 7)
    root("root@0", "K1", 1, 0)
    root("root@9", "K1", 0, 9)                                   # p with v2 >= v1: two loop turns
    root("root seen@5", "K0", 1, 5, seen=True)
    root("root@6", "S0", 1, 6, high=True)                        # q of 7 words: shorter than a chunk, shift 0
    root("root@3", "S0", 1, 3)
    root("root@7", "S31", 1, 7, high=True)                       # q of 8 words, shift 31
    root("root@0", "S31", 1, 0)
    # the same shape above F^2: the first reduction is an ordinary one, the second sees the crafted value
    F = keys["K0"][0]
    out.append(("root@9 + k p^2 K0 p", "K0", below_multiple(rnd, F, kw, 9, cap=F * F) + rnd.randrange(1, 1 << 900) * F * F, None,
                [("split_root_p", 9)]))
    return out


def _finish_items(rnd, keys):
    out = []
    kw = 32
    for kn, side, j in (("K0", 0, 15), ("K0", 0, 8), ("K0", 0, 0), ("K0", 1, 15), ("K0", 1, 8), ("K0", 1, 0), ("K1", 0, 8), ("K1", 1, 3),
                        ("S0", 1, 6), ("S0", 1, 3), ("S31", 1, 7), ("S31", 1, 0)):
        p, q = keys[kn]
        hp, hq = M.key_constants(p, q)[:2]
        F, h = (p, hp) if side == 0 else (q, hq)
        j = min(j, words(h) - 1)
        L = factor_below_multiple(rnd, F, h, kw, j)
        v = L * h % F
        m = crt_pair(p, q, v, rnd.randrange(q)) if side == 0 else crt_pair(p, q, rnd.randrange(p), v)
        r = _coprime(rnd, p * q)
        out.append(("Lh@%d %s %s" % (j, kn, "pq"[side]), kn, _enc(p * q, m, r), (m, r), [("finish_Lh_" + "pq"[side], j)]))
    # both sides of one item
    p, q = keys["K0"]
    hp, hq = M.key_constants(p, q)[:2]
    m = crt_pair(p, q, factor_below_multiple(rnd, p, hp, kw, 5) * hp % p, factor_below_multiple(rnd, q, hq, kw, 11) * hq % q)
    r = _coprime(rnd, p * q)
    out.append(("Lh@5 p @11 q K0", "K0", _enc(p * q, m, r), (m, r), [("finish_Lh_p", 5), ("finish_Lh_q", 11)]))
    return out


def _crt_items(rnd, keys):
    out = []
    hw, kw = 16, 32

    def put(tag, kn, m, r, claims):
        p, q = keys[kn]
        assert 0 <= m < p * q and gcd(r, p * q) == 1
        out.append((tag + " " + kn, kn, _enc(p * q, m, r), (m, r), claims))

    for kn in ("K0", "K1r"):
        p, q = keys[kn]
        assert p > q
        for tag, vp in (("vp=q-1", q - 1), ("vp=q", q), ("vp=p-1", p - 1)):     # the add-back and its neighbours without it
            put("m " + tag, kn, crt_pair(p, q, vp, _far(rnd, q, hw)), _coprime(rnd, p * q), [("crt_m_vp", 0)] if vp == q - 1 else [])
            put("r " + tag, kn, rnd.randrange(p * q), crt_pair(p, q, vp, _far(rnd, q, hw)), [("crt_r_vp", 0)] if vp == q - 1 else [])
    for kn, js in (("S0", (8, 4, 0)), ("S31", (8, 3, 0))):                   # a short q: 10 and 9 quotient digits
        p, q = keys[kn]
        for j in js:
            vp = below_multiple(rnd, q, hw, j, cap=p, high=j == js[0])
            put("m vp@%d" % j, kn, crt_pair(p, q, vp, rnd.randrange(q)), _coprime(rnd, p * q), [("crt_m_vp", j)])
            vp = below_multiple(rnd, q, hw, j, cap=p, high=j == js[0])
            put("r vp@%d" % j, kn, rnd.randrange(p * q), crt_pair(p, q, vp, rnd.randrange(1, q)), [("crt_r_vp", j)])
    for kn, js in (("K0", (15, 8, 0)), ("K1", (7,)), ("K1r", (4,)), ("S0", (6, 2)), ("S31", (7, 0))):
        p, q = keys[kn]
        pinv = pow(p, -1, q)
        for i, j in enumerate(js):
            j = min(j, words(pinv) - 1)
            for path in "mr":
                d = factor_below_multiple(rnd, q, pinv, kw, j)
                negative = (i + (path == "r")) % 2 == 1                      # the sign of v_q - (v_p mod q): both, on both paths
                a = rnd.randrange(q - d, q) if negative else rnd.randrange(0, q - d)
                vp, vq = a + (q if a + q < p and rnd.random() < 0.5 else 0), (a + d) % q
                assert (vq < a) == negative and vp < p
                v = crt_pair(p, q, vp, vq)
                if path == "m":
                    put("m prod@%d %s" % (j, "-" if negative else "+"), kn, v, _coprime(rnd, p * q), [("crt_m_prod", j)])
                else:
                    assert gcd(v, p * q) == 1
                    put("r prod@%d %s" % (j, "-" if negative else "+"), kn, rnd.randrange(p * q), v, [("crt_r_prod", j)])
    return out




def _key_items(rnd, keys, hw=16, prefix=""):
    """c = 1 + m n under the composite-factor keys (it decrypts under any key inside the domain), and a generic c under C: status 2"""
    out = []
    for kn, rows, j in (("A03", (0, 3), 0), ("B12", (1, 2), (hw - 10) // 2)):
        p, q = keys[kn]
        m = rnd.randrange(p * q)
        out.append((prefix + "key " + kn, kn, 1 + m * p * q, None, [("key_a%d" % row, j) for row in rows]))
    if hw == 16:
        for kn, rows, j in (("P03", (0, 3), 0), ("P12", (1, 2), 3)):
            p, q = keys[kn]
            m, r = rnd.randrange(p * q), _coprime(rnd, p * q)
            out.append(("key " + kn, kn, _enc(p * q, m, r), (m, r), [("key_a%d" % row, j) for row in rows]))
        p, q = keys["ADD_BACK_KEY"]                              # (the list of tests/paillier_dec_cases.py has it; its c takes the split's too)
        out.append(("add-back key", "ADD_BACK_KEY", 1 + 12345 * p * q, None, [("key_a0", 0), ("key_a3", 0), ("split_sq_p", 0)]))
        p, q = keys["C"]
        out.append(("composite p, generic c", "C", _coprime(rnd, p * q), None, []))
    return out


# What the items drive besides the add-backs that their builders certify — read off the word model's records once and held to them by
# tests/test_paillier_dec_branch_model.py: (site, branch), branch one of "overflow" (an estimate with qh >> 32 != 0), "break" (the rh >> 32
# break taken), "two_turns" (two loop turns for one digit).
OTHER_BRANCHES = {
    "sq@32 K0 p": [("split_sq_p", "overflow"), ("split_sq_p", "break")],
    "sq@15 K0 p": [("split_sq_p", "overflow"), ("split_sq_p", "break")],
    "sq@0 K0 p": [("split_sq_p", "break")],
    "sq@31 K0 q": [("split_sq_q", "overflow")],
    "sq@1 K0 q": [("split_sq_q", "overflow")],
    "sq@15 high K1 p": [("split_sq_p", "overflow")],
    "sq@32 K1 p": [("split_sq_p", "overflow")],
    "sq@20 K1 q": [("split_sq_q", "overflow"), ("split_sq_q", "break")],
    "sq seen@9 K0 p": [("split_sq_p", "overflow"), ("split_sq_p", "break")],
    "sq seen@9 K0 q": [("split_sq_q", "overflow")],
    "sq seen@9 K1 p": [("split_sq_p", "overflow")],
    "sq@12 K3 q": [("split_sq_q", "overflow"), ("split_sq_q", "break"), ("split_sq_q", "two_turns")],
    "sq@25 S0 q": [("split_sq_q", "overflow")],
    "sq@50 S0 q": [("split_sq_q", "overflow")],
    "sq@0 S31 q": [("split_sq_q", "break")],
    "sq@49 S31 q": [("split_sq_q", "overflow"), ("split_sq_q", "break")],
    "root@15 K0 p": [("split_root_p", "overflow"), ("split_root_p", "break")],
    "root@7 K0 p": [("split_root_p", "overflow"), ("split_root_p", "break")],
    "root@0 K0 p": [("split_root_p", "break")],
    "root@0 K1 q": [("split_root_q", "break")],
    "root@9 K1 p": [("split_root_p", "overflow"), ("split_root_p", "break"), ("split_root_p", "two_turns")],
    "root seen@5 K0 q": [("split_root_q", "overflow")],
    "root@6 S0 q": [("split_root_q", "overflow"), ("split_root_q", "break")],
    "root@3 S0 q": [("split_root_q", "overflow"), ("split_root_q", "break")],
    "root@7 S31 q": [("split_root_q", "overflow"), ("split_root_q", "break")],
    "root@0 S31 q": [("split_root_q", "break")],
    "root@9 + k p^2 K0 p": [("split_root_p", "overflow"), ("split_root_p", "break")],
    "Lh@15 K0 p": [("finish_Lh_p", "overflow"), ("finish_Lh_p", "break")],
    "Lh@8 K0 p": [("finish_Lh_p", "overflow"), ("finish_Lh_p", "break")],
    "Lh@0 K0 p": [("finish_Lh_p", "break")],
    "Lh@15 K0 q": [("finish_Lh_q", "overflow")],
    "Lh@8 K0 q": [("finish_Lh_q", "overflow")],
    "Lh@8 K1 p": [("finish_Lh_p", "overflow"), ("finish_Lh_p", "break"), ("finish_Lh_p", "two_turns")],
    "Lh@3 K1 q": [("finish_Lh_q", "overflow"), ("finish_Lh_q", "break")],
    "Lh@6 S0 q": [("finish_Lh_q", "overflow"), ("finish_Lh_q", "break")],
    "Lh@3 S0 q": [("finish_Lh_q", "overflow"), ("finish_Lh_q", "break")],
    "Lh@6 S31 q": [("finish_Lh_q", "overflow"), ("finish_Lh_q", "break")],
    "Lh@5 p @11 q K0": [("finish_Lh_p", "overflow"), ("finish_Lh_p", "break"), ("finish_Lh_q", "overflow")],
    "m vp@8 S0": [("crt_m_vp", "overflow"), ("crt_m_vp", "break")],
    "r vp@8 S0": [("crt_r_vp", "overflow"), ("crt_r_vp", "break")],
    "m vp@4 S0": [("crt_m_vp", "overflow"), ("crt_m_vp", "break")],
    "r vp@4 S0": [("crt_r_vp", "overflow"), ("crt_r_vp", "break")],
    "m vp@0 S0": [("crt_m_vp", "break")],
    "m vp@8 S31": [("crt_m_vp", "overflow"), ("crt_m_vp", "break")],
    "r vp@8 S31": [("crt_r_vp", "overflow"), ("crt_r_vp", "break")],
    "m vp@3 S31": [("crt_m_vp", "overflow"), ("crt_m_vp", "break")],
    "r vp@3 S31": [("crt_r_vp", "overflow"), ("crt_r_vp", "break")],
    "m vp@0 S31": [("crt_m_vp", "break")],
    "r vp@0 S31": [("crt_r_vp", "break")],
    "m prod@15 + K0": [("crt_m_prod", "overflow")],
    "r prod@15 - K0": [("crt_r_prod", "overflow")],
    "m prod@8 - K0": [("crt_m_prod", "overflow")],
    "r prod@8 + K0": [("crt_r_prod", "overflow")],
    "m prod@7 + K1": [("crt_m_prod", "overflow"), ("crt_m_prod", "break")],
    "r prod@7 - K1": [("crt_r_prod", "overflow"), ("crt_r_prod", "break")],
    "m prod@4 + K1r": [("crt_m_prod", "overflow"), ("crt_m_prod", "break"), ("crt_m_prod", "two_turns")],
    "r prod@4 - K1r": [("crt_r_prod", "overflow"), ("crt_r_prod", "break"), ("crt_r_prod", "two_turns")],
    "m prod@6 + S0": [("crt_m_prod", "overflow"), ("crt_m_prod", "break")],
    "r prod@6 - S0": [("crt_r_prod", "overflow"), ("crt_r_prod", "break")],
    "m prod@2 - S0": [("crt_m_prod", "overflow"), ("crt_m_prod", "break")],
    "r prod@2 + S0": [("crt_r_prod", "overflow"), ("crt_r_prod", "break")],
    "m prod@7 + S31": [("crt_m_prod", "overflow"), ("crt_m_prod", "break")],
    "r prod@7 - S31": [("crt_r_prod", "overflow"), ("crt_r_prod", "break")],
    "m prod@0 - S31": [("crt_m_prod", "break")],
    "r prod@0 + S31": [("crt_r_prod", "break")],
    "key B12": [("key_a1", "overflow"), ("key_a1", "break"), ("key_a1", "two_turns"),
                ("key_a2", "overflow"), ("key_a2", "break"), ("key_a2", "two_turns")],
    "key P12": [("key_a1", "overflow"), ("key_a1", "break"), ("key_a2", "overflow"), ("key_a2", "break")],
    "w2048 sq@38 p": [("split_sq_p", "overflow"), ("split_sq_p", "break")],
    "w2048 Lh@17 q": [("finish_Lh_q", "overflow"), ("finish_Lh_q", "break"), ("finish_Lh_q", "two_turns")],
    "w2048 sq@3 q": [("split_sq_q", "overflow"), ("split_sq_q", "break"), ("split_sq_q", "two_turns")],
    "w2048 root@20 p": [("split_root_p", "overflow"), ("split_root_p", "break")],
    "w2048 root@0 q": [("split_root_q", "break"), ("split_root_q", "two_turns")],
    "w2048 Lh@31 p": [("finish_Lh_p", "overflow"), ("finish_Lh_p", "break")],
    "w2048 m prod@13": [("crt_m_prod", "overflow"), ("crt_m_prod", "break"), ("crt_m_prod", "two_turns")],
    "w2048 r prod@25": [("crt_r_prod", "overflow"), ("crt_r_prod", "break"), ("crt_r_prod", "two_turns")],
    "w2048 key B12": [("key_a1", "overflow"), ("key_a1", "break"), ("key_a2", "overflow"), ("key_a2", "break")],
    "w4096 sq@70 p": [("split_sq_p", "overflow")],
    "w4096 Lh@33 q": [("finish_Lh_q", "overflow"), ("finish_Lh_q", "break")],
}

# What the mutant test does not assert, with the reason.  A fault alone stands for every site.
UNOBSERVABLE = {
    "no_overflow_clause":
        "the add-back repairs it.  An estimate of 2^32 + 1 always fails the two-digit test ((B + 1) v2 > (x1 - v1) B + x2, as x1 <= v2 and "
        "v1 >= B / 2) and becomes 2^32 with rh = x1; 2^32 passes the test only when x1 = v2, and then the true digit is 2^32 - 1: the "
        "64-bit multiply-subtract takes 2^32 times the divisor, borrows, and the add-back leaves the right remainder.  Every claimed item "
        "(all sites) gives the true outputs without the clause; the clause saves the loop turn, it does not decide a value.",
}
# (tag, site, fault): items whose outputs cannot show that fault at that site
UNOBSERVABLE_ITEMS = {
    (tag, site, fault):
        "c = 1 + m n has the root 1 under any key, so d_p, d_q — all that rows 2 and 3 feed — do not show; a generic c is outside the "
        "domain under composite factors.  The keys P03 and P12 have the same rows with prime factors, and there it shows."
    for tag, site in (("key A03", "key_a3"), ("add-back key", "key_a3"), ("key B12", "key_a2"), ("w2048 key A03", "key_a3"),
                      ("w2048 key B12", "key_a2"))
    for fault in ("no_addback", "no_rh_break")
}


def _assemble(n_bits, keys, name, items, neighbours, prime_keys=PRIME_KEYS, fallback="K0"):
    """every crafted item between two ordinary encrypted items — under its own key where that key has prime factors.  (One key in all: the
    batch layout's shared key, key_stride 0.)"""
    names, rows, claims = [], [], {}

    def add(tag, kn, c, truth):
        if kn not in names:
            names.append(kn)
        rows.append((tag, names.index(kn), c, truth))

    def neighbour(kn):
        kn = kn if kn in prime_keys else fallback                # (an ordinary item has an ordinary key, with prime factors)
        add("ordinary", kn, *neighbours(kn))

    for tag, kn, c, truth, addbacks in items:
        neighbour(kn)
        claims[len(rows)] = [(site, "addback@%d" % j) for site, j in addbacks] + OTHER_BRANCHES.get(tag, [])
        add(tag, kn, c, truth)
    neighbour(items[-1][1])
    b = PC._batch(n_bits, [keys[k] for k in names], rows)
    b["crafted"], b["claims"], b["kname"] = sorted(claims), claims, [names[k] for _, k, _, _ in rows]
    tags = [b["tag"][i] for i in b["crafted"]]
    assert len(set(tags)) == len(tags), "a crafted item's tag names it"
    return name, b


def _fresh_neighbours(rnd, keys):
    def make(kn):
        p, q = keys[kn]
        m, r = rnd.randrange(p * q), _coprime(rnd, p * q)
        return _enc(p * q, m, r), (m, r)
    return make


@functools.lru_cache(maxsize=None)
def list_1024():
    """[(name, batch)]: one key per item, at most 24 crafted items and their neighbours in a batch"""
    keys = dict(keys_1024())
    keys["K1r"] = (max(keys["K1"]), min(keys["K1"]))
    keys.update(composite_keys(16))
    keys.update(prime_keys_with_add_back(16))
    keys["ADD_BACK_KEY"] = PC.ADD_BACK_KEY
    rnd = [random.Random(0xD10 + k) for k in range(4)]           # (one stream per group: a change in one leaves the others' items alone)
    groups = [("split", _split_items(rnd[0], keys)), ("finish", _finish_items(rnd[1], keys)), ("crt", _crt_items(rnd[2], keys)),
              ("keys", _key_items(rnd[3], keys))]
    nb = _fresh_neighbours(random.Random(0xD2), keys)
    out = [_assemble(1024, keys, "%s %d" % (name, at // 24), items[at:at + 24], nb) for name, items in groups for at in range(0, len(items), 24)]
    tags = [b["tag"][i] for _, b in out for i in b["crafted"]]
    assert len(set(tags)) == len(tags)
    return out


@functools.lru_cache(maxsize=None)
def shared_1024():
    """the items of list_1024 under K0, in one batch with one key (key_stride 0): every site that needs no special key"""
    rows = [(b["tag"][i], b["c"][i], b["want"][i], b["truth"][i], b["claims"].get(i))
            for _, b in list_1024() for i in range(len(b["c"])) if b["kname"][i] == "K0" and b["keys"][i] == keys_1024()["K0"]]
    s = dict(n_bits=1024, keys=[keys_1024()["K0"]], c=[r[1] for r in rows], want=[r[2] for r in rows], truth=[r[3] for r in rows],
             tag=[r[0] for r in rows], claims={i: r[4] for i, r in enumerate(rows) if r[4] is not None})
    s["crafted"] = sorted(s["claims"])
    assert all(s["tag"][i - 1] == "ordinary" and s["tag"][i + 1] == "ordinary" for i in s["crafted"])
    assert {site for cl in s["claims"].values() for site, _ in cl} >= set(W.SITES[4:])
    return s


def reversed_batch(b):
    """the same items in the opposite order: every crafted lane at another position of its block"""
    n = len(b["c"])
    r = dict(b, c=b["c"][::-1], want=b["want"][::-1], truth=b["truth"][::-1], tag=b["tag"][::-1],
             claims={n - 1 - i: cl for i, cl in b["claims"].items()}, crafted=sorted(n - 1 - i for i in b["crafted"]))
    if len(b["keys"]) > 1:
        r["keys"] = b["keys"][::-1]
    return r


@functools.lru_cache(maxsize=None)
def wide(n_bits):
    """2048 bits: one add-back item per site; 4096 bits (the benchmark's key: generating 2048-bit primes in Python is too slow): one for the
    split by F^2, one for the finish's L h, one for the recombination.  The chunk loops run 4 and 8 times, nx - nm reaches 128."""
    hw, kw = n_bits // 64, n_bits // 32
    base = PC.one_key(n_bits)                                    # (its ciphertexts are the neighbours: the same n, kept values)
    p, q = max(base["keys"][0]), min(base["keys"][0])
    keys = dict(K=(p, q))
    rnd = random.Random(n_bits + 0xD3)
    hp, hq, pinv = M.key_constants(p, q)[:3]
    items, pre = [], "w%d " % n_bits

    def enc(tag, m, r, claims):
        assert 0 <= m < p * q and gcd(r, p * q) == 1
        items.append((pre + tag, "K", _enc(p * q, m, r), (m, r), claims))

    def raw(tag, c, claims):
        items.append((pre + tag, "K", c, None, claims))

    j = hw + 6
    raw("sq@%d p" % j, below_multiple(rnd, p * p, 2 * kw, j, high=True), [("split_sq_p", j)])
    j = hw // 2 + 1
    Lq = factor_below_multiple(rnd, q, hq, kw, j)
    enc("Lh@%d q" % j, crt_pair(p, q, rnd.randrange(p), Lq * hq % q), _coprime(rnd, p * q), [("finish_Lh_q", j)])
    enc("m vp=q-1", crt_pair(p, q, q - 1, _far(rnd, q, hw)), _coprime(rnd, p * q), [("crt_m_vp", 0)])
    if n_bits == 2048:
        keys.update(composite_keys(hw))
        raw("sq@3 q", below_multiple(rnd, q * q, 2 * kw, 3), [("split_sq_q", 3)])
        raw("root@20 p", below_multiple(rnd, p, kw, 20, cap=p * p), [("split_root_p", 20)])
        raw("root@0 q", below_multiple(rnd, q, kw, 0, cap=q * q), [("split_root_q", 0)])
        Lp = factor_below_multiple(rnd, p, hp, kw, hw - 1)
        enc("Lh@%d p" % (hw - 1), crt_pair(p, q, Lp * hp % p, rnd.randrange(q)), _coprime(rnd, p * q), [("finish_Lh_p", hw - 1)])
        enc("r vp=q-1", rnd.randrange(p * q), crt_pair(p, q, q - 1, _far(rnd, q, hw)), [("crt_r_vp", 0)])
        for path, j, negative in (("m", 13, False), ("r", 25, True)):
            d = factor_below_multiple(rnd, q, pinv, kw, j)
            a = rnd.randrange(q - d, q) if negative else rnd.randrange(0, q - d)
            v = crt_pair(p, q, a, (a + d) % q)
            if path == "m":
                enc("m prod@%d" % j, v, _coprime(rnd, p * q), [("crt_m_prod", j)])
            else:
                enc("r prod@%d" % j, rnd.randrange(p * q), v, [("crt_r_prod", j)])
        items += _key_items(rnd, keys, hw, pre)
    def quiet(c):                                                # (m = n - 1 and its like take an add-back of their own)
        sites = {}
        W.open_words(p, q, c, hw, sites)
        return not any(st.get("addbacks") for st in sites.values())

    pool = itertools.cycle((c, t) for c, t in zip(base["c"], base["truth"]) if quiet(c))     # (4096 bits has three: one comes twice)
    return _assemble(n_bits, keys, "wide %d" % n_bits, items, lambda kn: next(pool), prime_keys=("K",), fallback="K")[1]


def composite_factor_keys():
    """[(name, (p, q))] for zkp_correct_key_ni_prove_batch: key preparation is shared with it"""
    c = composite_keys(16)
    return [("A03", c["A03"]), ("B12", c["B12"]), ("C", c["C"])]
