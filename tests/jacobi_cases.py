"""The (a, n) pairs of tests/test_wbjacobi_model.py (CPU: tools/wbjacobi_model.py against tests/jacobi_model.py) and of
tests/test_gpu_jacobi.py (zkp_jacobi_batch against tests/jacobi_model.py) — a plain module, so that both hold the same hazard classes:
where an approximated binary GCD with a sign bit goes wrong are the low bits a step reads (n mod 8, a mod 4) and the comparisons it
decides on truncated operands (pairs that agree in their top bits)."""
import functools
import random

import helpers as H
from jacobi_model import jacobi

WIDTHS = (1024, 2048, 4096)
RANDOM_PAIRS = 200          # per width

# Found by a search over the trace of tools/wbjacobi_model.py (1024-bit rows) and committed as found: the first round takes all its 28 steps
# and its LAST step (index 27, three exact low bits left) flips the sign by the rule for (2 / b), which reads b mod 8 — and so do more than
# half of the later rounds.  tests/test_wbjacobi_model.py asserts the property on the model.
MOD8_LATE = [
    (0x1807dfaf1f7e42734f56d48f05e1ddfb3c37bb0118b0f10e0eabf94903f33851f72699ec6a1e860d41cd81b0c6db0211e7a82c20e5e6df0cddd284e869616452038d04fb1018d7f54191590c42c79c1c2950e9ae5089be3bee8b9e7c4a815857105cbc52d65f45b6968e485e46db73ab5044df5c81b2499e1b37ca07a14d59fc,
     0xa55c9c8e2f7c9cc7cd64a752b8ec796e5b336bc8c25536590f7815f2af3e7dd91b2528692bd8af216fa12947f472bb6918afaf544382ad47c813063719f900d321f343908e449800ab99436044a23f659015b7c24b71779491e0b53936e53725bb20e1d5916b2b37c051ac7c8e48e48847cd07f7b74c990a9eebba4e1c14df93),
    (0xeac7b9899f76af5bd8b5dfd7af5d8c1654f30e785b59fa18cfbf6c30b5ceb55d20a468411fb3486937d344104f2d11b63a1f3187e28c0c9f598f2e8c5e75636edadc492db4f49e2ad7db35a3307cd804d2be48f8b60c80f8a9e674083d95d25b75581cff80d670c838011be7eb4d4e582b474b1ccfe5c229c8be8b3678b73fc2,
     0xce24bc1b8643e70a06bcdd155942de9e3b03b452c43bba358a42d18fb221f233a9a5e8c91df9b09759675284e237a35f9961f1836b7af802bd4633c6d7645e1926a9e7e62595bdd339547fc4f64e0794ef97c8ff9191f12dd2bbbbe7cca0b2feae9be17558d4863686e1de8475f0971278ca15082d4d3635fde48df178a31235),
    (0x7f483760b6bdd84532155353444a04ea6addce03a7e1e13d033819e69d21eb2f893af923ba1889a8c9c62d45f317dbb01b8aa85fcb0ad3306321e0f02de635c7874a501c8c242d96c7f3e64e22c33e15cbad1c5e58b8fce4378fead71b719fe6d19fbfb0fee96c71a0d5b4d61220e048586fa4adfcc42d94b9750018ffc379f9,
     0xebdaf11cd2e37f3866f563b80224aa9257ef0f17a9a08296272a1a946a44191d519eed18c0d96c6d720bfd961fe696f740aa5fec9ca29b0a7ddb334b07d2e86c602f95c7901dc8a4943c2300d39f715119695b1830035ee19260099b750b53e2c9c61667dbca2969ef760588c3af5cfe9e5b739117a293cb0c62ccbbef49af17),
    (0x9d20ddebd58d75d666f0a633db85fbfd24ba2adda413c35a5ee25397c60bcf98c955fcaf1d505858b92a099e974ed2945e7ceca239dd86a23dcc40f1cad82b5b60c02f99a1410fe69c9bc5047fdd82025bc2e068c959e2430304470e24984e6fcfd81b8c62fcd1a900ff3d6fe01d066074b07b6e4cb82ad8ab0ca019ecd94c29,
     0x9df274af945af439f5b28fb2084d609c90faf95dd6afee1b62c5da8811f82e59f6dc31c3defadae8cd4f6a0eb4ff60285cb37f811432b9b9d5e1ae608584ceefcaf8ed2b193de7791f1ff9cfe90359f36aaba9a5b4299aea87e493aea2292ba65ce81309604b2d67cbe59ab014747a469af6669793342b2e5b53d784de0923bd),
]


def fixture_primes():
    """p, q of the 2048-bit fixture key (tests/golden/reference_constants.json: range_proof_ni.tests.test_keypair)"""
    p, q, _ = H.fixture_key()
    return p, q


def expected(a, n):
    """(symbol, status) of zkp_jacobi_batch"""
    return (0, 2) if n % 2 == 0 else (jacobi(a, n), 0)


@functools.lru_cache(maxsize=None)
def cases(mod_bits):
    """[(class, a, n)] for rows of mod_bits bits: every a and n fits the row; n is odd except in the class "domain" """
    full = 1 << mod_bits
    rnd = random.Random(mod_bits)
    p, q = fixture_primes()
    out = []

    def add(tag, a, n):
        assert 0 <= a < full and 0 <= n < full, tag
        out.append((tag, a, n))

    def odd(bits, mod8=None):
        n = rnd.getrandbits(bits) | (1 << (bits - 1)) | 1
        return n if mod8 is None else (n & ~7) | mod8

    # n mod 8 x a mod 4
    for m8 in (1, 3, 5, 7):
        for a4 in (0, 1, 2, 3):
            n = odd(mod_bits - 1, m8)
            add("mod8xmod4", (rnd.randrange(n) & ~3) | a4, n)
            add("mod8xmod4-small", a4 + 4 * rnd.randrange(64), 8 * rnd.randrange(1, 64) + m8)
    # a in {0, 1, 2, n - 1, n, n + 1, 2n + 1}
    for n in (odd(mod_bits - 2), odd(mod_bits - 2, 3), p * q if mod_bits > 2048 else odd(mod_bits - 2, 5), 3, 1, 0xFFFFFFFF, (1 << 64) + 1):
        for a in (0, 1, 2, n - 1, n, n + 1, 2 * n + 1):
            add("special-a", a, n)
    # a = 2^k, k on each side of every word boundary of a 1024-bit row
    n = odd(mod_bits, 3)
    for j in range(1, 32):
        for k in (32 * j - 1, 32 * j):
            add("pow2", 1 << k, n)
    add("pow2", 1 << (mod_bits - 1), n)
    # symbol 0: a = p t under n = p q
    if mod_bits >= 2048:
        for t in (1, 2, q - 1, rnd.randrange(q), 2 * q + 1 if mod_bits > 2048 else q - 2):
            add("shared-factor", p * t, p * q)
    sp, sq, _ = H.test_key(1024)                                 # two 512-bit primes: their products fit every row
    for t in (1, 3, rnd.randrange(sq), sq + 2):
        add("shared-factor", sp * t, sp * sq)
    # n = 1, 3, 2^k - 1, p^2
    for n in (1, 3, (1 << 31) - 1, (1 << 32) - 1, (1 << 33) - 1, (1 << 64) - 1, (1 << 65) - 1, full - 1, sp * sp, 9, 25):
        for a in (rnd.randrange(full), rnd.randrange(n + 1), 2, n >> 1):
            add("special-n", a, n)
    # operand lengths far apart
    add("far-apart", rnd.getrandbits(20) | (1 << 19), odd(mod_bits))
    add("far-apart", rnd.getrandbits(20) | (1 << 19) | 1, odd(mod_bits, 5))
    add("far-apart", rnd.getrandbits(mod_bits) | (1 << (mod_bits - 1)), odd(33))
    add("far-apart", rnd.getrandbits(mod_bits) | (1 << (mod_bits - 1)) | 1, odd(33, 7))
    add("far-apart", rnd.getrandbits(mod_bits), odd(65))
    add("far-apart", rnd.getrandbits(70), odd(mod_bits - 40))
    # pairs that agree in their top 64, 96 and 128 bits and differ below: both orders; the difference a power of two, and random low bits
    for top in (64, 96, 128):
        for bits in (mod_bits - 1, mod_bits - 37, 300):
            n = odd(bits, rnd.choice((1, 3, 5, 7)))
            for j in (1, 2, 3, 29, 30, 31, 32, 33, bits - top - 2, bits - top - 1):
                add("close-pow2", n + (1 << j), n)           # a > n
                add("close-pow2", n - (1 << j), n)           # a < n
                add("close-pow2", n, n + (1 << j))           # the same pair, roles swapped
                add("close-pow2", n, n - (1 << j)) if n - (1 << j) > 0 else None
            for _ in range(4):
                low = rnd.getrandbits(bits - top) & ~1
                add("close-random", n ^ low, n)
                add("close-random", n, n ^ low)
    # pairs that stay close for several rounds: consecutive Fibonacci-like operands (every quotient is 1)
    f0, f1 = 1, 1
    while f1.bit_length() < mod_bits - 1:
        f0, f1 = f1, f0 + f1
    for a, n in ((f0, f1), (f1, f0), (f1 - f0, f1)):
        if n % 2 == 0:
            a, n = n, a
        if n % 2:
            add("fibonacci", a, n)
    # rounds whose last steps read b mod 8 (found on 1024-bit rows; they fit every width)
    for a, n in MOD8_LATE:
        add("mod8-late", a, n)
    # outside the domain: n even or zero
    for n in (0, 2, odd(mod_bits - 1) - 1, 1 << (mod_bits - 1)):
        add("domain", rnd.randrange(full), n)
    # random pairs
    for i in range(RANDOM_PAIRS):
        nb = mod_bits if i % 4 else rnd.randrange(1, mod_bits + 1)
        ab = mod_bits if i % 3 else rnd.randrange(1, mod_bits + 1)
        add("random", rnd.getrandbits(ab), rnd.getrandbits(nb) | 1)
    return out


@functools.lru_cache(maxsize=None)
def expected_all(mod_bits):
    """the reference of every case, computed once: [(symbol, status)]"""
    return [expected(a, n) for _, a, n in cases(mod_bits)]
