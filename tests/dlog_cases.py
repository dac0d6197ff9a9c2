"""Case builder for CompositeDLogProof (wi_dlog_proof.rs:46-91) at the shapes tests/test_gpu_dlog.py runs: one batch of 70 rows per
(n_bits, y_bits), the same row order at every shape.

A row is (name, N, g, ni, secret, r | None, x, y, pinned verdict | None).  Rows with a witness (r is not None) carry the x, y the C oracle's
prover computed from exactly these inputs; the verify-only edits of an honest proof have r = None.  The pinned verdict is what the row is
built to be (tests/test_dlog_cases.py checks it against the Python model and the C oracle); None: whatever the oracle says.

What the layout is for (tests/test_dlog_cases.py recomputes every claim made here):
  * rows 0 … 31 are 16 aligned pairs whose two responses y differ in effective length — 0, 1, a middle length (an honest y: r + e·s, 513
    bits at most) or the full y_bits — so that every claim of every kernel family (4 items at the least up to 2048 bits, 2 at 4096 bits)
    holds exponents of different lengths and the window count has to follow the longest one.  Pair 1 is (y = 0, y = 2^y_bits − 1).
  * rows 64 … 69 — the second block of k_dlog_hash (64 proofs per block) and the last, ragged claim — hold ACCEPT, REJECT and MALFORMED rows.
  * rows 32 … 63 hold the rest of the classes and honest / `+secret` fillers on rotating keys.

Moduli cost nothing: 1024-bit keys from helpers.test_key, the reference's fixture key and products of the pooled 1024-bit primes of
bench_keys.json at 2048 bits, the benchmark's 4096-bit key and products of four pooled primes at 4096 bits.  No prime above 1024 bits is
generated."""
import json
import os

import helpers as H
from helpers import pm, L, zkp

ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED
ROWS = 70
HASH_BLOCK = 64               # DLOG_THREADS (csrc/kernels_proofs.hpp): proofs per block of k_dlog_hash
MIXED = 32                    # the rows whose aligned runs hold responses of different lengths
SHORT_X_BOUND = 4096          # tries of the short-x search: each succeeds with probability 1/256
SHAPES = ((1024, 544), (1024, 1024), (2048, 576), (2048, 2048), (4096, 768), (4096, 4096))
N_SMALL = (1 << 128) - 159    # <= 2^128: the reference panics (wi_dlog_proof.rs:69)
N_EDGE = (1 << 128) + 1       # just above the bound: word 4 is 1, the low words are not all zero

_CACHE = {}


def run_of(n_bits):
    """the smallest claim of any kernel family, in items: the aligned runs of the first MIXED rows hold different lengths"""
    return 2 if n_bits == 4096 else 4


def pool1024():
    path = os.path.join(H.ROOT, "zk-paillier_amd", "bench_keys.json")
    return [int(v, 16) for v in json.load(open(path))["pool1024"]]


def pool_product(bits, count, extra=1, skip=0):
    """`count` pooled primes (largest first, the first `skip` left out) times `extra`, of exactly `bits` bits -> (factors, N)"""
    pool = sorted(pool1024(), reverse=True)[skip:]
    for i in range(len(pool) - count + 1):
        fs = pool[i:i + count]
        n = extra
        for f in fs:
            n *= f
        if n.bit_length() == bits:
            return fs, n
    raise AssertionError(f"no {count} pooled primes give {bits} bits")


def keys(n_bits):
    """four (p, N) with p a proper factor of N, N of exactly n_bits bits"""
    if n_bits == 1024:
        return [(p, n) for p, q, n in (H.test_key(1024, tag=20 + t) for t in range(4))]
    if n_bits == 2048:
        out = [(pm.FIXTURE_P, pm.FIXTURE_N)]
        for k in range(3):
            fs, n = pool_product(2048, 2, skip=2 * k)
            out.append((fs[0], n))
        return out
    assert n_bits == 4096
    from importlib import import_module
    p, q, n = import_module("zk-paillier_amd.synth").bench_key_4096()
    out = [(p, n)]
    for k in range(3):
        fs, n = pool_product(4096, 4, skip=4 * k)
        out.append((fs[0], n))
    return out


def short_modulus(n_bits, bits):
    """an odd N of exactly `bits` bits in a field of n_bits: whole zero top words in every hashed operand.  Below 1024 bits a key of
    helpers.test_key; above, pooled primes times such a key (the product has `bits` bits or a few fewer: the tags are tried in turn)"""
    if bits <= 1024:
        return H.test_key(bits, tag=31)[2]
    whole, rest = divmod(bits, 1024)
    assert 64 <= rest
    for tag in range(31, 63):
        try:
            return pool_product(bits, whole, extra=H.test_key(rest, tag=tag)[2])[1]
        except AssertionError:
            continue
    raise AssertionError(f"no short modulus of {bits} bits")


def length_class(y, y_bits):
    """0, 1, 'mid' or 'full': the effective length of a response in a field of y_bits"""
    n = y.bit_length()
    return n if n <= 1 else "full" if n == y_bits else "mid"


def _honest(N, g, s):
    """ni of an honest statement: (g^-1)^s mod N (wi_dlog_proof.rs:117-141)"""
    return pow(pow(g, -1, N), s, N)


def build(n_bits, y_bits, oracle):
    """the 70 rows of one shape (cached per process: the `ctx` fixture runs every test under five kernel families)"""
    key = (n_bits, y_bits)
    if key not in _CACHE:
        _CACHE[key] = _build(n_bits, y_bits, oracle)
    return _CACHE[key]


def _build(n_bits, y_bits, oracle):
    assert (n_bits, y_bits) in SHAPES or (n_bits, y_bits) == (2048, 768)
    kw = n_bits // 32
    d = pm.Drbg(b"dlog-cases-%d" % n_bits)          # the same statements at every y_bits of one key size
    ks = keys(n_bits)
    (p0, N0) = ks[0]
    q0 = N0 // p0
    full = (1 << y_bits) - 1
    wit = []          # (name, N, g, ni, secret, r, pinned): rows the oracle's prover completes

    def honest(name, N, g=None, r=None, s=None, pinned=ACCEPT):
        g = d.range(2, N - 1) if g is None else g
        r = d.bits(512) if r is None else r
        s = d.bits(256) if s is None else s
        wit.append((name, N, g, _honest(N, g, s), s, r, pinned))
        return name

    def plus_secret(name, N):
        g, s = d.range(2, N - 1), d.bits(256) | 1
        wit.append((name, N, g, pow(g, s, N), s, d.bits(512), REJECT))     # +secret instead of -secret (:145-168)
        return name

    # ---- honest proofs
    for k, (_, N) in enumerate(ks):
        honest(f"honest-key{k}", N)
    honest("honest-r-max-s-max", N0, r=(1 << 512) - 1, s=(1 << 256) - 1)   # the longest carry chain of y = r + e*s
    honest("honest-r0", N0, r=0)
    honest("honest-s0", N0, s=0)
    honest("honest-r0-s0", N0, r=0, s=0)                                   # x = 1, y = 0
    honest("honest-r1-s1", N0, r=1, s=1)
    honest("honest-g2", ks[1][1], g=2)
    honest("honest-g-minus-1", ks[2][1], g=ks[2][1] - 1)
    # ---- N narrower than the field
    N_short = short_modulus(n_bits, n_bits - 40)
    assert N_short.bit_length() == n_bits - 40 and N_short & 1
    honest("honest-short-N", N_short)
    extras = []
    if n_bits == 2048:
        N_1100 = short_modulus(2048, 1100)
        assert N_1100.bit_length() == 1100
        extras.append(honest("honest-N-1100-bits", N_1100))
    if n_bits == 1024:
        # an x at least one byte shorter than N: step r until g^r mod N has a zero top byte (Sha256::put_bigint strips it)
        g, s, r0 = d.range(2, N0 - 1), d.bits(256), d.bits(500)
        nbytes = (N0.bit_length() + 7) // 8
        for t in range(SHORT_X_BOUND):
            if (pow(g, r0 + t, N0).bit_length() + 7) // 8 < nbytes:
                break
        else:
            raise AssertionError("no short x within the bound")
        extras.append(honest("honest-short-x", N0, g=g, r=r0 + t, s=s))
        _CACHE[("short-x-tries", n_bits)] = t + 1
    # ---- rows the reference panics on (the prover still computes x and y from them)
    b = dict((w[0], w) for w in wit)["honest-key0"]
    g0, ni0, s0 = b[2], b[3], b[4]
    wit.append(("malformed-N-small", N_SMALL, 5, 7, 3, d.bits(512), MALFORMED))
    wit.append(("malformed-g-zero", N0, 0, ni0, s0, d.bits(512), MALFORMED))
    wit.append(("malformed-ni-zero", N0, g0, 0, s0, d.bits(512), MALFORMED))
    wit.append(("malformed-g-shares-p", N0, p0 * d.range(2, 1 << 64) % N0, ni0, s0, d.bits(512), MALFORMED))
    wit.append(("malformed-ni-shares-q", N0, g0, q0 * 3 % N0, s0, d.bits(512), MALFORMED))
    wit.append(("malformed-g-zero-low-words", N0, N0 - (p0 << 96), ni0, s0, d.bits(512), MALFORMED))   # N - g has 3 zero low words
    # ---- N just above 2^128: not MALFORMED for its size; the verdict is the oracle's
    honest("edge-N-2^128+1", N_EDGE, pinned=None)
    # ---- fillers for rows 32 ... 63
    n_fill = ROWS - 44 - len(extras)
    fillers = [plus_secret(f"fill{i}-plus-secret", ks[i % 4][1]) if i % 3 == 2 else honest(f"fill{i}-honest", ks[i % 4][1]) for i in range(n_fill)]
    tail_ok = honest("tail-honest", ks[1][1])

    N_, g_, ni_ = (L.ints_to_limbs([w[i] for w in wit], kw) for i in (1, 2, 3))
    s_ = L.ints_to_limbs([w[4] for w in wit], 8); r_ = L.ints_to_limbs([w[5] for w in wit], 16)
    xo, yo = oracle.dlog_prove(n_bits, y_bits, N_, g_, ni_, s_, r_)
    rows = {}
    for w, x, y in zip(wit, L.limbs_to_ints(xo), L.limbs_to_ints(yo)):
        rows[w[0]] = (w[0], w[1], w[2], w[3], w[4], w[5], x, y, w[6])

    def edit(name, base, pinned=REJECT, **kv):
        """a verify-only copy of the honest row `base` with some of N, g, ni, x, y replaced"""
        f = dict(zip(("N", "g", "ni", "secret", "r", "x", "y"), rows[base][1:8]))
        for k, v in kv.items():
            f[k] = v(f) if callable(v) else v
        assert f["x"].bit_length() <= n_bits and f["y"].bit_length() <= y_bits
        rows[name] = (name, f["N"], f["g"], f["ni"], f["secret"], None, f["x"], f["y"], pinned)
        return name

    for k in range(4):
        base = f"honest-key{k}"
        edit(f"y-zero-key{k}", base, y=0)
        edit(f"y-one-key{k}", base, y=1)
        edit(f"y-top-bit-key{k}", base, y=lambda f: f["y"] | 1 << (y_bits - 1))
        edit(f"y-all-ones-key{k}", base, y=full)
    edit("y-flip-bit0", "honest-key0", y=lambda f: f["y"] ^ 1)
    edit("x-zero", "honest-key1", x=0)
    edit("x-one", "honest-key2", x=1)
    edit("x-N-minus-1", "honest-key3", x=lambda f: f["N"] - 1)
    edit("x-plus-N", "honest-short-N", x=lambda f: f["x"] + f["N"])        # the same residue, not canonical: fits under the short N
    edit("x-flip-bit1", "honest-key0", x=lambda f: f["x"] ^ 2)
    edit("ni-one", "honest-key1", ni=1)
    edit("ni-random", "honest-key2", ni=d.range(2, ks[2][1] - 1))

    # rows 0 ... 31: 16 aligned pairs, a response of middle length next to one of another length; pair 1 is the shortest next to the longest
    mid = ["honest-key1", "honest-key2", "honest-key3", "honest-r-max-s-max", "honest-r0", "honest-s0", "honest-r1-s1", "honest-g2",
           "honest-g-minus-1", "honest-short-N", "y-flip-bit0", "x-zero", "x-one", "x-N-minus-1"]
    other = ["y-one-key0", "honest-r0-s0"] + [f"y-{e}-key{k}" for k in (1, 2, 3) for e in ("zero", "one", "top-bit", "all-ones")]
    assert len(mid) == len(other) == MIXED // 2 - 2
    order = ["honest-key0", "y-top-bit-key0", "y-zero-key0", "y-all-ones-key0"]
    for i, (m, o) in enumerate(zip(mid, other)):
        order += [o, m] if i % 2 == 0 else [m, o]                            # the other length sits in either lane of a pair
    middle = ["x-plus-N", "ni-one", "malformed-N-small", "malformed-g-zero", "malformed-ni-zero", "malformed-g-shares-p"] + extras + fillers
    assert len(order) == MIXED and len(order) + len(middle) == HASH_BLOCK, (len(order), len(middle))
    # rows 64 ... 69: the second block of k_dlog_hash and the last, ragged claim
    order += middle + [tail_ok, "malformed-ni-shares-q", "x-flip-bit1", "edge-N-2^128+1", "malformed-g-zero-low-words", "ni-random"]
    assert any(n.endswith("plus-secret") for n in order)
    assert len(order) == ROWS and len(set(order)) == ROWS, (len(order), len(set(order)))
    assert set(order) == set(rows), sorted(set(rows) ^ set(order))
    return [rows[n] for n in order]


def arrays(rows, n_bits, y_bits):
    """-> N, g, ni, x, y limb arrays of the whole batch"""
    kw = n_bits // 32
    N, g, ni = (L.ints_to_limbs([r[i] for r in rows], kw) for i in (1, 2, 3))
    return N, g, ni, L.ints_to_limbs([r[6] for r in rows], kw), L.ints_to_limbs([r[7] for r in rows], y_bits // 32)


def witness_arrays(rows, n_bits, y_bits):
    """the rows that have a witness -> N, g, ni, secret, r, x, y limb arrays"""
    w = [r for r in rows if r[5] is not None]
    N, g, ni, x, y = arrays(w, n_bits, y_bits)
    return N, g, ni, L.ints_to_limbs([r[4] for r in w], 8), L.ints_to_limbs([r[5] for r in w], 16), x, y


def oracle_verdicts(n_bits, y_bits, oracle):
    """the C oracle's verdicts on the batch (cached: one computation per process and shape)"""
    key = ("verdicts", n_bits, y_bits)
    if key not in _CACHE:
        _CACHE[key] = oracle.dlog_verify(n_bits, y_bits, *arrays(build(n_bits, y_bits, oracle), n_bits, y_bits))
    return _CACHE[key]


def short_x_tries(n_bits):
    return _CACHE[("short-x-tries", n_bits)]
