"""Deterministic inputs for zkp_probable_prime_batch, zkp_next_prime_batch and zkp_paillier_keygen_seeded_batch, built once per process
from the repository's DRBG and classified by tests/prime_model.py.  tests/test_prime_model.py asserts on the CPU that every class below is
non-empty; tests/test_gpu_prime.py runs them on the GPU.

(a) tail classes, 512 bits, base 2: accepted at y == 1, at y == w - 1, at squaring j >= 1; rejected after reaching 1 without -1, rejected
    never reaching either; Proth-shaped k 2^s + 1, prime and composite, s >= 488.
(b) composites (2k + 1)(4k + 1), both factors prime, k of 254 bits, that are strong pseudoprimes to base 2 and have no factor in the table
    — placed in a batch where the model rejects them at round 1, and where it accepts round 1 and rejects at a later round.
(c) next-prime starts: even; two below a class-(b) composite with a prime later in the window; a window with no prime; windows that cross
    2^bits (with and without a prime in front of the limit); start = 0.
(d) keygen batches in which some slot needs attempt t >= 1 and some prime sits behind at least C + 1 survivors of the table for every
    C of SMALL_CHUNKS: the fixed numbers of rows per slot and round that tests/test_gpu_prime.py sets through zkp_diag_prime_search, so
    that a prime is found in a second or later round of its window and (ROUNDS > C) a candidate's bases span two rounds.  Left to
    itself the library gives the few slots of a test batch 64 rows each, and every prime falls in the first round."""
import functools

import helpers as H
import prime_model as M

SEED = bytes((7 * i + 3) & 0xFF for i in range(32))
ROUNDS = 5
SMALL_CHUNKS = (4, 7)           # rows per slot and round, fixed: below ROUNDS, and above it but far below a window's ~65 survivors
FIRST_INDEX = 4000
SMALL = [l for l in M.sieve(200) if l > 2]


def _no_small_factor(w):
    return all(w % l for l in SMALL)


def _fermat_prime(w):
    return _no_small_factor(w) and pow(2, w - 1, w) == 1 and H.is_probable_prime(w)


@functools.lru_cache(maxsize=None)
def family():
    """products (2k + 1)(4k + 1) of two primes, k of 254 bits, sorted by what the base-2 strong test makes of them ->
    dict: 'spsp' (class b), 'hit-one', 'never' — two of each at least"""
    d = H.pm.Drbg(b"prime-cases-family")
    out = {"spsp": [], "hit-one": [], "never": []}
    while min(len(v) for v in out.values()) < 2:
        k = d.bits(254) | (1 << 253)
        p, q = 2 * k + 1, 4 * k + 1
        if not (_no_small_factor(p) and _no_small_factor(q) and pow(2, p - 1, p) == 1 and pow(2, q - 1, q) == 1):
            continue
        if not (H.is_probable_prime(p) and H.is_probable_prime(q)):
            continue
        w = p * q
        ok, how = M.sprp_trace(w, 2)
        out["spsp" if ok else how].append(w)
    return out


@functools.lru_cache(maxsize=None)
def tail_primes():
    """512-bit primes by the way base 2 accepts them -> dict 'one', 'minus', 'square'"""
    d = H.pm.Drbg(b"prime-cases-tail")
    out = {"one": [], "minus": [], "square": []}
    while min(len(v) for v in out.values()) < 2:
        w = d.bits(512) | (1 << 511) | 1
        if not _fermat_prime(w):
            continue
        _, how = M.sprp_trace(w, 2)
        out[how if isinstance(how, str) else "square"].append(w)
    return out


@functools.lru_cache(maxsize=None)
def proth():
    """k 2^490 + 1 below 2^512 without a factor in the table -> (primes, composites), two each"""
    primes, composites = [], []
    k = 1 << 20
    while len(primes) < 2 or len(composites) < 2:
        k += 1
        w = (2 * k + 1) * (1 << 490) + 1
        if any(w % l == 0 for l in M.TABLE):
            continue
        if pow(3, w - 1, w) == 1 and H.is_probable_prime(w):
            primes.append(w)
        elif len(composites) < 2:
            composites.append(w)
    return primes[:2], composites


def ordinary(bits):
    """two primes and a few composites of the full width"""
    p, q = keygen_want(2 * bits, KEYGEN_SHAPES_BY_BITS[2 * bits])[0][0][:2]        # (the model's own keys: no second prime search)
    d = H.pm.Drbg(b"prime-cases-ordinary-%d" % bits)
    comp = []
    while len(comp) < 3:
        w = d.bits(bits) | (1 << (bits - 1)) | 1
        if not H.is_probable_prime(w):
            comp.append(w)
    return [p, q], comp + [p - 1, 6361 * (q >> 13)]            # (an even one; one with a factor in the table)


SMALL_VALUES = [0, 1, 2, 3, 4, 9, 6361, 6367, 6369, 6370, 6373, 6367 * 6367, 6373 * 6373, 6373 * 6379, M.TABLE_BOUND ** 2 - 1, M.TABLE_BOUND ** 2 + 1,
                40576979, 1 << 32, (1 << 32) + 15, (1 << 61) - 1]


@functools.lru_cache(maxsize=None)
def test_batch(bits, count):
    """-> (list of `count` values below 2^bits, dict class name -> positions).  Item i is tested under index FIRST_INDEX + i."""
    fam, tp = family(), tail_primes()
    pr, co = proth()
    primes, comps = ordinary(bits)
    pool = [("prime", primes[0]), ("composite", comps[0])]
    if count > 1:
        pool += [("one", tp["one"][0]), ("minus", tp["minus"][0]), ("square", tp["square"][0]), ("hit-one", fam["hit-one"][0]), ("never", fam["never"][0]),
                 ("proth-prime", pr[0]), ("proth-composite", co[0]), ("prime", primes[1])] + [("composite", c) for c in comps[1:]]
        pool += [("small", v) for v in SMALL_VALUES] + [("one", tp["one"][1]), ("square", tp["square"][1]), ("hit-one", fam["hit-one"][1]),
                                                       ("proth-prime", pr[1]), ("proth-composite", co[1])]
    values = [pool[i % len(pool)] for i in range(count)]
    # class (b): the same composite wherever the model says the position shows the wanted behaviour
    where = {}
    if count > 1:
        X = fam["spsp"]
        free = [i for i in range(count) if values[i][0] in ("small", "composite") and i >= 2]
        for want, name in ((lambda f: f == 1, "b-round-1"), (lambda f: f is not None and f >= 2, "b-later-round")):
            for i in free:
                x = X[i % len(X)]
                if want(M.failing_round(x, ROUNDS, SEED, FIRST_INDEX + i)):
                    values[i] = (name, x)
                    free.remove(i)
                    break
    for i, (name, _) in enumerate(values):
        where.setdefault(name, []).append(i)
    return [v for _, v in values], where


def test_want(bits, count, rounds):
    values, _ = test_batch(bits, count)
    return [M.is_probable_prime(w, rounds, SEED, FIRST_INDEX + i) for i, w in enumerate(values)]


@functools.lru_cache(maxsize=None)
def next_batch():
    """512 bits -> (starts, names, want): want[i] = (prime, j, status) under index FIRST_INDEX + i and ROUNDS rounds"""
    bits = 512
    d = H.pm.Drbg(b"prime-cases-next")
    starts, names = [], []

    def add(name, s):
        starts.append(s)
        names.append(name)

    add("even", (d.bits(bits) | (1 << (bits - 1))) & ~1)
    add("zero", 0)
    add("small", 6370 ** 2 - 40)
    for x in family()["spsp"]:                                # two below a class-(b) composite: c_1 is the composite
        i = len(starts)
        if M.failing_round(x, ROUNDS, SEED, FIRST_INDEX + i) is not None and M.next_prime(x - 2, bits, ROUNDS, SEED, FIRST_INDEX + i)[0] is not None:
            add("behind-b", x - 2)
            break
    while True:                                               # a window without a prime (about one in eighteen at 512 bits)
        s = d.bits(bits) | (1 << (bits - 1))
        if M.next_prime(s, bits, ROUNDS, SEED, FIRST_INDEX + len(starts))[0] is None:
            add("empty", s)
            break
    add("cross-found", (1 << bits) - 600)                     # 2^512 - 569 is the largest prime below 2^512
    add("cross-none", (1 << bits) - 500)
    add("last", (1 << bits) - 1)
    add("ordinary", d.bits(bits) | (1 << (bits - 1)))
    want = []
    for i, s in enumerate(starts):
        p, j = M.next_prime(s, bits, ROUNDS, SEED, FIRST_INDEX + i)
        want.append((p, j, 0) if p is not None else (0, 0, M.MALFORMED))
    return starts, names, want


@functools.lru_cache(maxsize=None)
def next_depths():
    """name -> survivors of the table in front of the prime that next_batch()'s search finds (the cases that find one)"""
    starts, names, _ = next_batch()
    out = {}
    for i, (s, name) in enumerate(zip(starts, names)):
        st = {}
        if M.next_prime(s, 512, ROUNDS, SEED, FIRST_INDEX + i, stats=st)[0] is not None:
            out[name] = st["survivors_before"]
    return out


KEYGEN_SHAPES = [(1024, 1), (1024, 67), (2048, 5), (4096, 2)]
KEYGEN_SHAPES_BY_BITS = {1024: 67, 2048: 5, 4096: 2}
KEYGEN_FIRST_INDEX = {1024: 77, 2048: 9, 4096: 1}


@functools.lru_cache(maxsize=None)
def keygen_want(n_bits, batch, first_index=None):
    """-> (keys [(p, q, n, status)], attempts [(t_p, t_q)], stats per key and factor)"""
    stats = []
    keys, attempts = M.keygen(SEED, KEYGEN_FIRST_INDEX[n_bits] if first_index is None else first_index, batch, n_bits, ROUNDS, stats)
    return keys, attempts, stats
