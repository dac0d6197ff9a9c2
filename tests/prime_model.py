"""Python restatement of the probable-prime rule, the next-prime search and seeded Paillier key generation (include/zkp_hip.h:
zkp_probable_prime_batch, zkp_next_prime_batch, zkp_paillier_keygen_seeded_batch), written from the rule and not from
the kernels (csrc/kernels_prime.hpp).  A plain module: tests/test_prime_model.py pins it, tests/test_gpu_prime.py holds the GPU to it bit
for bit.

The stream is that of tests/seeded_nonce_model.py, unchanged: ChaCha20 block function of RFC 8439; key = the 32 seed bytes as 8
little-endian words; state words 13, 14 = (index & 0xffffffff, index >> 32), index = first_index + i; state word 15 = 0x80000000 |
kind << 20 | slot << 4 | field.  One more kind: 9 Keygen.

    kind      slot             field   value
    Keygen    0                0 / 1   start of attempt t for p / q
    Keygen    r (1 .. rounds)  2 / 3   base a_r for p / q        (the test and the search alone: field 2)
"""
import seeded_model as R

KIND_KEYGEN = 9
TABLE_BOUND = 6370
WINDOW = 512
MAX_ATTEMPTS = 128
MAX_ROUNDS = 64
MALFORMED = 2
M32 = 0xFFFFFFFF


def sieve(bound):
    """all primes below bound"""
    flags = bytearray([1]) * bound
    flags[0:2] = b"\0\0"
    for i in range(2, int(bound ** 0.5) + 1):
        if flags[i]:
            flags[i * i::i] = bytearray(len(range(i * i, bound, i)))
    return [i for i in range(bound) if flags[i]]


TABLE = [p for p in sieve(TABLE_BOUND) if p != 2]         # all odd primes below 6370


def block(seed, counter, index, slot, field):
    word15 = 0x80000000 | (KIND_KEYGEN << 20) | (slot << 4) | field
    return R.block_words(list(R.SIGMA) + R.key_words(seed) + [counter & M32, index & M32, (index >> 32) & M32, word15])


def stream_words(seed, index, slot, field, first_block, count):
    words = []
    k = first_block
    while len(words) < count:
        words += block(seed, k, index, slot, field)
        k += 1
    return words[:count]


def base(seed, index, field, r, L):
    """a_r for candidates of L bits: 2 + the first ceil((L - 2) / 32) words of the stream, masked to L - 2 bits"""
    nw = (L - 2 + 31) // 32
    v = sum(w << (32 * i) for i, w in enumerate(stream_words(seed, index, r, field, 0, nw)))
    return 2 + (v & ((1 << (L - 2)) - 1))


def start(seed, index, field, t, bits):
    pw = bits // 32
    nb = (pw + 15) // 16
    v = sum(w << (32 * i) for i, w in enumerate(stream_words(seed, index, 0, field, t * nb, pw)))
    return v | 1 | (1 << (bits - 1))


def sprp_trace(w, a):
    """-> (passes, how): how is 'one' (y == 1), 'minus' (y == w - 1), ('square', j), 'hit-one' (reached 1 without -1) or 'never'"""
    assert w > 3 and w & 1 and 2 <= a <= w - 2
    d, s = w - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    y = pow(a, d, w)
    if y == 1:
        return True, "one"
    if y == w - 1:
        return True, "minus"
    for j in range(1, s):
        y = y * y % w
        if y == w - 1:
            return True, ("square", j)
        if y == 1:
            return False, "hit-one"
    return False, "never"


def sprp(w, a):
    return sprp_trace(w, a)[0]


def failing_round(w, rounds, seed, index, field=2):
    """for a w that reaches the strong tests: None when it passes base 2 and every a_r, else the first failing round (0: base 2)"""
    if not sprp(w, 2):
        return 0
    L = w.bit_length()
    for r in range(1, rounds + 1):
        if not sprp(w, base(seed, index, field, r, L)):
            return r
    return None


def reaches_strong_tests(w):
    return w >= TABLE_BOUND ** 2 and w & 1 and all(w % l for l in TABLE)


def is_probable_prime(w, rounds=0, seed=None, index=0, field=2):
    if w < 2:
        return 0
    if w == 2:
        return 1
    if w % 2 == 0:
        return 0
    for l in TABLE:
        if w == l:
            return 1
        if w % l == 0:
            return 0
    if w < TABLE_BOUND ** 2:
        return 1
    return 1 if failing_round(w, rounds, seed, index, field) is None else 0


def next_prime(start_, bits, rounds=0, seed=None, index=0, field=2, stats=None):
    """-> (prime, j) or (None, None).  stats (a dict): 'strong' counts the candidates that reached the strong tests, 'survivors_before' the
    survivors of the table in front of the result"""
    c0 = start_ | 1
    for j in range(WINDOW):
        c = c0 + 2 * j
        if c >= 1 << bits:
            break
        if stats is not None and reaches_strong_tests(c):
            stats["strong"] = stats.get("strong", 0) + 1
        if is_probable_prime(c, rounds, seed, index, field):
            if stats is not None:
                stats["survivors_before"] = sum(1 for i in range(j) if all((c0 + 2 * i) % l for l in TABLE))
            return c, j
    return None, None


def keygen_factor(seed, index, field, bits, rounds, stats=None):
    """-> (prime or None, attempts used - 1)"""
    for t in range(MAX_ATTEMPTS):
        p, _ = next_prime(start(seed, index, field, t, bits), bits, rounds, seed, index, 2 + field, stats)
        if p is not None:
            return p, t
    return None, MAX_ATTEMPTS


def keygen(seed, first_index, batch, n_bits, rounds=5, stats=None):
    """-> list of (p, q, n, status), and per key the attempt that found (p, q)"""
    out, attempts = [], []
    for b in range(batch):
        st = [dict(), dict()] if stats is not None else [None, None]
        p, tp = keygen_factor(seed, first_index + b, 0, n_bits // 2, rounds, st[0])
        q, tq = keygen_factor(seed, first_index + b, 1, n_bits // 2, rounds, st[1])
        attempts.append((tp, tq))
        if stats is not None:
            stats.append(st)
        if p is None or q is None or p == q:
            out.append((0, 0, 0, MALFORMED))
        else:
            out.append((p, q, p * q, 0))
    return out, attempts
