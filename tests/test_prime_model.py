"""CPU tests of tests/prime_model.py and tests/prime_cases.py: the model is the rule of include/zkp_hip.h (zkp_probable_prime_batch,
zkp_next_prime_batch, zkp_paillier_keygen_seeded_batch), checked against a plain sieve and the suite's Miller-Rabin; the case inventory
holds every class that tests/test_gpu_prime.py must meet — asserted here, so that a GPU test cannot pass by never meeting one; the device
table is the model's."""
import ctypes as C
import math

import helpers as H
import prime_cases as PC
import prime_model as M
from helpers import zkp


def test_table():
    assert M.TABLE[0] == 3 and M.TABLE[-1] == 6367 and len(M.TABLE) == 829 and all(H.is_probable_prime(l) for l in M.TABLE[::40])
    count, last = C.c_uint32(), C.c_uint32()
    assert zkp.load().zkp_diag_prime_table(C.byref(count), C.byref(last)) == zkp.capi.ZKP_OK
    assert (count.value, last.value) == (len(M.TABLE), M.TABLE[-1])


def test_model_is_exact_below_the_square_of_the_bound():
    primes = set(M.sieve(1 << 16))
    assert all(M.is_probable_prime(w) == (w in primes) for w in range(1 << 16))
    lo, hi = M.TABLE_BOUND ** 2 - 200, M.TABLE_BOUND ** 2 + 200
    near = set(p for p in M.sieve(hi + 1) if p >= lo)
    assert all(M.is_probable_prime(w) == (w in near) for w in range(lo, hi + 1))
    assert M.is_probable_prime(6373 * 6379) == 0 and M.is_probable_prime(6373 * 6373) == 0       # the first composites without a factor in the table


def test_model_agrees_with_the_suites_miller_rabin_on_every_case():
    for bits, count in ((512, 130), (1024, 65), (2048, 17)):
        values, _ = PC.test_batch(bits, count)
        assert all(w < 1 << bits for w in values)
        assert PC.test_want(bits, count, PC.ROUNDS) == [int(H.is_probable_prime(w)) for w in values]


def test_stream_and_bases():
    w = PC.tail_primes()["one"][0]
    L = w.bit_length()
    a = [M.base(PC.SEED, 5, 2, r, L) for r in range(1, 6)]
    assert len(set(a)) == 5 and all(2 <= x <= (1 << (L - 2)) + 1 <= w - 2 for x in a)
    assert M.base(PC.SEED, 5, 3, 1, L) != a[0] and M.base(PC.SEED, 6, 2, 1, L) != a[0]
    assert M.base(PC.SEED, 5, 2, 1, 40) == 2 + (M.block(PC.SEED, 0, 5, 1, 2)[0] | M.block(PC.SEED, 0, 5, 1, 2)[1] << 32) % (1 << 38)
    s = M.start(PC.SEED, 5, 0, 3, 2048)                         # 64 words: blocks 12 .. 15 of the stream
    assert s.bit_length() == 2048 and s & 1
    assert s >> 32 & 0xFFFFFFFF == M.block(PC.SEED, 12, 5, 0, 0)[1] and (s >> (32 * 63)) | 1 << 31 == M.block(PC.SEED, 15, 5, 0, 0)[15] | 1 << 31
    assert M.start(PC.SEED, 5, 0, 1, 512) >> 32 & 0xFFFFFFFF == M.block(PC.SEED, 1, 5, 0, 0)[1]


def test_inventory_tail_classes():
    tp, fam = PC.tail_primes(), PC.family()
    assert all(M.sprp_trace(w, 2) == (True, "one") for w in tp["one"]) and all(M.sprp_trace(w, 2) == (True, "minus") for w in tp["minus"])
    assert all(M.sprp_trace(w, 2)[1][0] == "square" and M.sprp_trace(w, 2)[1][1] >= 1 for w in tp["square"])
    assert all(M.sprp_trace(w, 2) == (False, "hit-one") for w in fam["hit-one"]) and all(M.sprp_trace(w, 2) == (False, "never") for w in fam["never"])
    assert all(M.reaches_strong_tests(w) for v in list(tp.values()) + list(fam.values()) for w in v)
    primes, composites = PC.proth()
    for w in primes + composites:
        k, s = w - 1, 0
        while k % 2 == 0:
            k //= 2
            s += 1
        assert s >= 512 - 24 and w.bit_length() <= 512 and M.reaches_strong_tests(w)
    assert all(H.is_probable_prime(w) and M.sprp_trace(w, 2)[0] for w in primes) and not any(H.is_probable_prime(w) or M.sprp(w, 2) for w in composites)
    _, where = PC.test_batch(512, 65)
    for name in ("one", "minus", "square", "hit-one", "never", "proth-prime", "proth-composite", "prime", "composite", "small"):
        assert where.get(name), name


def test_inventory_base_2_pseudoprimes():
    for bits, count in ((512, 65), (512, 130), (1024, 65), (1024, 130), (2048, 17)):
        values, where = PC.test_batch(bits, count)
        (i,), (k,) = where["b-round-1"], where["b-later-round"]
        for pos in (i, k):
            x = values[pos]
            assert x in PC.family()["spsp"] and M.reaches_strong_tests(x) and not H.is_probable_prime(x) and M.is_probable_prime(x, 0) == 1
        assert M.failing_round(values[i], PC.ROUNDS, PC.SEED, PC.FIRST_INDEX + i) == 1
        assert 2 <= M.failing_round(values[k], PC.ROUNDS, PC.SEED, PC.FIRST_INDEX + k) <= PC.ROUNDS
    for x in PC.family()["spsp"]:                               # (2k + 1)(4k + 1), both prime, k of 254 bits
        k = (math.isqrt(8 * x + 1) - 3) // 8
        assert (2 * k + 1) * (4 * k + 1) == x and k.bit_length() == 254 and H.is_probable_prime(2 * k + 1) and H.is_probable_prime(4 * k + 1)


def test_inventory_next_prime_starts():
    starts, names, want = PC.next_batch()
    assert set(names) >= {"even", "zero", "behind-b", "empty", "cross-found", "cross-none", "ordinary"}
    by = dict(zip(names, zip(starts, want)))
    assert by["even"][0] % 2 == 0 and by["even"][1][2] == 0
    assert by["zero"] == (0, (3, 1, 0))
    s, (p, j, st) = by["behind-b"]
    assert s + 2 in PC.family()["spsp"] and st == 0 and j >= 2 and p == s + 2 * j and M.next_prime(s, 512)[1] == 1     # base 2 alone stops AT the composite
    assert by["empty"][1] == (0, 0, 2) and by["cross-none"][1] == (0, 0, 2) and by["last"][1] == (0, 0, 2)
    s, (p, j, st) = by["cross-found"]
    assert st == 0 and p == (1 << 512) - 569 and s + 2 * 511 >= 1 << 512
    assert all(H.is_probable_prime(w[0]) for w in want if w[2] == 0)


def test_inventory_keygen_batches():
    late = 0
    for n_bits, batch in PC.KEYGEN_SHAPES:
        keys, attempts, stats = PC.keygen_want(n_bits, batch)
        assert all(st == 0 and H.is_probable_prime(p) and H.is_probable_prime(q) and p != q and n == p * q and p.bit_length() == q.bit_length() == n_bits // 2
                   for p, q, n, st in keys)
        late += sum(1 for a in attempts if max(a) >= 1)
    assert late
    _, attempts, stats = PC.keygen_want(1024, 67)
    assert any(max(a) >= 1 for a in attempts)
    assert PC.keygen_want(1024, 1)[0] == PC.keygen_want(1024, 67)[0][:1]


def test_inventory_small_chunks():
    """under C rows per slot and round (tests/test_gpu_prime.py: the fixed chunks) the batches hold primes that a second or later round of
    their window finds, windows that several rounds use up, and candidates whose bases span two rounds"""
    assert min(PC.SMALL_CHUNKS) < PC.ROUNDS < max(PC.SMALL_CHUNKS)     # bases in two rounds under the one, in one round under the other
    _, attempts, stats = PC.keygen_want(1024, 67)
    depth = [s["survivors_before"] for k in stats for s in k]
    starts, names, want = PC.next_batch()
    next_depth = PC.next_depths()
    for C in PC.SMALL_CHUNKS:
        assert sum(1 for d in depth if d >= C + 1) >= 10 and any(d >= 3 * C for d in depth), C       # second round, and third or later
        assert any(max(a) >= 1 for a in attempts)                   # a used-up window: more than C survivors, all of them dead
        assert sum(1 for d in next_depth.values() if d >= C + 1) >= 2 and max(next_depth.values()) >= 3 * C, (C, next_depth)
    # the class-(b) composite of the search sits INSIDE the first chunk: it is picked, falls under its bases, and the rows behind it count
    assert want[names.index("behind-b")][1] >= 2 and 1 <= min(PC.SMALL_CHUNKS)
