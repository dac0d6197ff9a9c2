"""The base-n Paillier kernels (csrc/kernels_basen.hpp, the generated engine csrc/kernels_basen_asm_g*.inc, the ladders of
csrc/kernels_basen_r2l.hpp) under keys AT the digit-sum limit of the FAST Montgomery product.

At 36 limbs per lane a 64-bit column is exact only while every lane's limb sum of the key's Orup multiple M~ = n n1 is within
COL_FAST_SN_LIMIT_BN.  k_setup_basen measures the sums of every key and marks a key over the limit as not qualifying; its items go to the
n^2-sized kernels.  Random keys sit a third below the limit, so none of tests/test_gpu_basen.py comes near the guard or the columns it
protects.  The keys here (tests/limit_keys.py) have one lane at limit + {-1, 0, +1, +2^20, -2^20} with the other lanes random, every lane
at the limit, and every lane at the limit but one at + 1 — with a full-width n1, so that the operands fill the top limbs as well.

What is observed: the guard's verdict per key against the formula of the engine in use (at 18 and 9 limbs per lane no sum can reach the
limit: every key must qualify); the constants and single products at the operands' bounds, limb for limb against tests/basen_model.py;
Enc under a shared key and under per-item keys that mix admitted and rejected keys in one launch (the partition path); the latency
engine's ladders; and whole RangeProofNi proofs.

Every Enc item is compared between two kernels (the base-n launch and the n^2-sized kernels, at 36 limbs per lane; the ladder and the pair
ladder) and between the engines; Python's pow() — the cost of this file, the suite being on a budget (tests/test_gpu_suite_budget.py) —
checks the operand edge cases and random items against (1 + m n) r^n mod n^2, computed once for the three engines."""
import math
import os
import random

import numpy as np
import pytest

import helpers as H
import limit_keys
from basen_model import BaseN, LB, MASK
from limit_keys import DELTAS, qualifies

zkp = H.zkp
pytestmark = pytest.mark.gpu


def limbs(x, L):
    return np.array([(x >> (LB * i)) & MASK for i in range(L)], np.uint32)


def value(arr):
    return sum(int(v) << (LB * i) for i, v in enumerate(arr))


def words(x, n):
    return np.array([(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)], np.uint32)


def from_words(row):
    return sum(int(w) << (32 * j) for j, w in enumerate(row))


@pytest.fixture(scope="module", params=[36, 18, 9], ids=["w36", "w18", "w9"])
def ctx(request):
    """a context of its own per engine, every Paillier launch told to take the base-n form (as tests/test_gpu_basen.py)"""
    c = zkp.Context(0)
    c.set_geometry(request.param)
    c.set_enc_form("basen")
    c.test_geometry = request.param
    yield c
    c.close()


def lanes_per_integer(ctx, n_bits):
    return (72 // ctx.test_geometry) * (n_bits // 2048)


keys_for = limit_keys.guard_key_set       # [(name, lane deltas, n)]; limit_keys.qualifies(n, n_bits, W) is the guard's verdict as the engine of W limbs states it


@pytest.mark.parametrize("n_bits", [2048, 4096])
def test_classification_at_the_limit(ctx, n_bits):
    """the `ok` word of k_setup_basen is 1 exactly when every lane sum is within the limit of the engine; M~ and n1 are the constructor's"""
    L = 72 * (n_bits // 2048)
    got, want = [], []
    for name, deltas, n in keys_for(n_bits):
        n1, Mt = limit_keys.orup(n)
        out = ctx.diag_basen(n_bits, words(n, n_bits // 32), 3)
        assert int(out[4 * L]) == n1, name
        assert value(out[3 * L:4 * L]) == Mt, name
        got.append(int(out[4 * L + 1]))
        want.append(int(qualifies(n, n_bits, ctx.test_geometry)))
    assert got == want, [(k[0], g, w) for k, g, w in zip(keys_for(n_bits), got, want) if g != w]
    if ctx.test_geometry != 36:
        assert all(got)
    else:
        assert 0 in got and 1 in got


@pytest.mark.parametrize("n_bits", [2048, 4096])
def test_single_operations_under_admitted_keys(ctx, n_bits):
    """ops 0 / 1 / 2 of zkp_diag_basen with the operands at their bounds, limb for limb against the value model"""
    G = n_bits // 1024
    ran = 0
    for name, deltas, n in keys_for(n_bits):
        if not qualifies(n, n_bits, ctx.test_geometry):
            continue
        ran += 1
        m = BaseN(n, G)
        L = m.L
        nw = words(n, n_bits // 32)
        out = ctx.diag_basen(n_bits, nw, 3)
        assert int(out[4 * L + 1]) == 1, name
        # the device's representatives of C3 and RR (tests/test_gpu_basen.py): checked, then used by the model
        assert value(out[0:L]) % n == m.C3 % n and value(out[0:L]) <= n, name
        assert (value(out[L:2 * L]) + value(out[2 * L:3 * L]) * n) % (n * n) == (m.R * m.R) % (n * n), name
        rr = (value(out[L:2 * L]), value(out[2 * L:3 * L]))
        m.RR = rr
        m.C3 = value(out[0:L])
        for r in ((1 << n_bits) - 1, n - 1, 0, n):
            o = ctx.diag_basen(n_bits, nw, 0, xa=limbs(r, L))
            assert (value(o[:L]), value(o[L:2 * L])) == m.mul((r, 0), rr), (name, hex(r)[:12])
        ops = limit_keys.worst_operands(m.Mt)           # (tests/test_bn_asm.py runs the same set through the engine's lane model)
        for i, x in enumerate(ops):
            o = ctx.diag_basen(n_bits, nw, 2, xa=limbs(x[0], L), xb=limbs(x[1], L))
            got = (value(o[:L]), value(o[L:2 * L]))
            assert got == m.sqr(x), (name, "square", i)
            assert got[0] < 2 * m.Mt and got[1] < 4 * m.Mt
            for j, y in enumerate(ops):
                if (i + j) % 2 and (i, j) not in ((0, 1), (1, 0)):
                    continue                                    # (the two heaviest pairs in all four orders, the others with themselves and each other)
                o = ctx.diag_basen(n_bits, nw, 1, xa=limbs(x[0], L), xb=limbs(x[1], L), ya=limbs(y[0], L), yb=limbs(y[1], L))
                got = (value(o[:L]), value(o[L:2 * L]))
                # the kernel multiplies the STAGED x by the resident y: mul(y, x) in the model's argument order
                assert got == m.mul(y, x), (name, "product", i, j)
                assert got[0] < 2 * m.Mt and got[1] < 4 * m.Mt
    assert ran == (len(keys_for(n_bits)) if ctx.test_geometry != 36 else 3 * G + 1)


# ---------------------------------------------------------------- Enc
COUNT = {2048: 35, 4096: 17}        # more than one wavefront of groups on every engine (32 / 16 groups at 36 limbs per lane), ragged
# The inputs and Python's values are built once per module run, and the first engine's words of a call become the reference of the engines
# after it (same_on_every_engine): that check is only as strong as the first engine's own checks — against the n^2-sized kernels at 36 limbs
# per lane and against pow() on the sample — and a test run alone compares with nothing there.  Under a key over the limit the launch at 36
# limbs IS the n^2-sized one: for those keys the pow() sample and the two other engines, which admit them, are the independent references.
_CASES, _MIXED, _FIRST = {}, {}, {}


python_enc = H.python_enc


def same_on_every_engine(tag, out):
    """the first engine's words for a call, kept: the other engines — other kernels — have to give the same"""
    first = _FIRST.setdefault(tag, out.copy())
    return np.array_equal(first, out)


def n2_sized(ctx, call):
    """the same call on the n^2-sized kernels of the engine"""
    ctx.set_enc_form("n2")
    try:
        call()
    finally:
        ctx.set_enc_form("basen")


def shared_case(n_bits, k):
    """(ms, rs, mw, rw, {item: (1 + m n) r^n mod n^2 by Python's pow()}) of the call under key k, computed once for all engines.  Items 0 - 3
    are the operand edge cases, the others random.  Python is the time of this file (a third of a second per 4096-bit item), and every
    item is compared between two kernels and between the engines: 2048 bits: the edge cases and a random item under every key; 4096
    bits: r = 0, r = n and one of r = n - 1 / r = 2^4096 - 1 / a random item in turn under every key."""
    if (n_bits, k) not in _CASES:
        n = keys_for(n_bits)[k][2]
        kw = n_bits // 32
        rnd = random.Random(n_bits * 1000 + k)
        count = COUNT[n_bits]
        ms = [rnd.randrange(n) for _ in range(count)]
        rs = [rnd.getrandbits(n_bits) for _ in range(count)]        # r >= n included
        ms[0], rs[0] = n - 1, n - 1
        ms[1], rs[1] = 0, (1 << n_bits) - 1
        ms[2], rs[2] = n - 1, 0                                        # r = 0 and r = n: Enc = 0
        ms[3], rs[3] = 0, n
        ms[4], rs[4] = rnd.randrange(n), rnd.randrange(n)
        mw = np.stack([words(v, kw) for v in ms]); rw = np.stack([words(v, kw) for v in rs])
        sample = (0, 1, 2, 3, 4) if n_bits == 2048 else ((0, 1, 4)[k % 3], 2, 3)
        _CASES[(n_bits, k)] = (ms, rs, mw, rw, {i: python_enc(n, ms[i], rs[i]) for i in sample})
    return _CASES[(n_bits, k)]


def product_form(n_bits, k, out):
    """expected = a * b mod n^2 (the Mask rows of RangeProofNi::verify): a = Enc(m, r) / b for an invertible b, with one a off by one;
    from the words of the call under key k (the same on every engine: computed once)"""
    if ("product", n_bits, k) not in _CASES:
        n = keys_for(n_bits)[k][2]
        nn, kw, count = n * n, n_bits // 32, COUNT[n_bits]
        rnd = random.Random(k)
        bs = []
        while len(bs) < count:
            b = rnd.randrange(2, nn)
            if math.gcd(b, n) == 1:
                bs.append(b)
        a_ = [from_words(out[i]) * pow(bs[i], -1, nn) % nn for i in range(count)]
        wrong = 5 + (k + 3) % (count - 5)
        a_[wrong] = (a_[wrong] + 1) % nn
        _CASES[("product", n_bits, k)] = (np.stack([words(x, 2 * kw) for x in a_]), np.stack([words(x, 2 * kw) for x in bs]), wrong)
    return _CASES[("product", n_bits, k)]


def key_groups(n_bits):
    """the keys of test_enc_under_a_shared_key, lane by lane (one test case per lane: Python's pow() is its time)"""
    G = n_bits // 1024
    return [(f"lane{j}", list(range(j * len(DELTAS), (j + 1) * len(DELTAS)))) for j in range(G)] + [("every-lane", [G * len(DELTAS), G * len(DELTAS) + 1])]


SHARED_PARAMS = [pytest.param(nb, idx, id=f"{nb}-{name}") for nb in (2048, 4096) for name, idx in key_groups(nb)]


@pytest.mark.parametrize("n_bits,key_idx", SHARED_PARAMS)
def test_enc_under_a_shared_key(ctx, n_bits, key_idx):
    """one call per key: the launch reports the form and the guard's verdict as predicted; every item equals the n^2-sized kernels' and the
    other engines', the sample Python's — under a key over the limit the answers come from the n^2-sized launch behind; and Enc-and-compare
    finds the one wrong item in the plain and in the product form"""
    kw = n_bits // 32
    count = COUNT[n_bits]
    for k in key_idx:
        name, deltas, n = keys_for(n_bits)[k]
        ms, rs, mw, rw, py = shared_case(n_bits, k)
        nw = words(n, kw)
        out = np.zeros((count, 2 * kw), np.uint32)
        ctx.paillier_enc(n_bits, count, nw, 0, mw, rw, out)
        lanes, ok = ctx.diag_basen_last()
        want_ok = qualifies(n, n_bits, ctx.test_geometry)
        assert (lanes, ok) == (lanes_per_integer(ctx, n_bits), want_ok), name
        for i, want in py.items():
            assert from_words(out[i]) == want, (name, i)
        if ctx.test_geometry == 36:                  # (the other engines are tied to this one word for word, below)
            out_n2 = np.zeros_like(out)
            n2_sized(ctx, lambda: ctx.paillier_enc(n_bits, count, nw, 0, mw, rw, out_n2))
            bad = [i for i in range(count) if not np.array_equal(out[i], out_n2[i])]
            assert not bad, (name, bad)
        assert same_on_every_engine(("shared", n_bits, k), out), name
        if not want_ok:
            continue
        wrong = 5 + k % (count - 5)
        e2 = out.copy()
        e2[wrong, (7 * k) % (2 * kw)] ^= 1 << (k % 32)
        v = np.full(count, 9, np.uint8)
        ctx.paillier_enc_check(n_bits, count, nw, 0, mw, rw, None, None, e2, v)
        assert list(v) == [0 if i == wrong else 1 for i in range(count)], name
        aw, bw, wrong = product_form(n_bits, k, out)
        v = np.full(count, 9, np.uint8)
        ctx.paillier_enc_check(n_bits, count, nw, 0, mw, rw, aw, bw, None, v)
        assert list(v) == [0 if i == wrong else 1 for i in range(count)], name


def mixed_case(n_bits):
    """per-item keys: the whole key set in turn (admitted, exactly at the limit, over it in lane 0 only / in the last lane only / in one
    lane of an otherwise full key), more items than a wavefront has groups; Python's values for the items of six of the keys"""
    if n_bits not in _MIXED:
        kw = n_bits // 32
        keys = keys_for(n_bits)
        count = {2048: 37, 4096: 23}[n_bits]
        rnd = random.Random(n_bits + 17)
        ks = [i % len(keys) for i in range(count)]
        ns = [keys[k][2] for k in ks]
        ms = [rnd.randrange(n) for n in ns]
        rs = [rnd.getrandbits(n_bits) for _ in range(count)]
        ms[0], rs[0] = ns[0] - 1, ns[0] - 1
        nw = np.stack([words(v, kw) for v in ns]); mw = np.stack([words(v, kw) for v in ms]); rw = np.stack([words(v, kw) for v in rs])
        G = n_bits // 1024
        nd = len(DELTAS)
        # lane 0 at - 1 / at the limit / over it, the last lane over it, the two whole-key shapes
        sample = [0, 1, 2, (G - 1) * nd + 2, G * nd, G * nd + 1]
        _MIXED[n_bits] = (ks, nw, mw, rw, {i: python_enc(ns[i], ms[i], rs[i]) for i in sample})
    return _MIXED[n_bits]


@pytest.mark.parametrize("n_bits", [2048, 4096])
def test_enc_with_per_item_keys_across_the_guard(ctx, n_bits):
    """ONE launch whose keys lie on both sides of the guard: the keys over the limit are partitioned off to the n^2-sized launch behind
    (kernels_basen.hpp: the partition path) — every item right, the batch-wide flag `not ok`, and the clean items word for word those of a
    launch without the rejected keys"""
    kw = n_bits // 32
    keys = keys_for(n_bits)
    ks, nw, mw, rw, py = mixed_case(n_bits)
    count = len(ks)
    admitted = [qualifies(keys[k][2], n_bits, ctx.test_geometry) for k in ks]
    out = np.zeros((count, 2 * kw), np.uint32)
    ctx.paillier_enc(n_bits, count, nw, kw, mw, rw, out)
    lanes, ok = ctx.diag_basen_last()
    assert (lanes, ok) == (lanes_per_integer(ctx, n_bits), all(admitted))
    assert ok == (ctx.test_geometry != 36)
    for i, want in py.items():
        assert from_words(out[i]) == want, (i, keys[ks[i]][0])
    if ctx.test_geometry == 36:
        out_n2 = np.zeros_like(out)
        n2_sized(ctx, lambda: ctx.paillier_enc(n_bits, count, nw, kw, mw, rw, out_n2))
        bad = [(i, keys[ks[i]][0]) for i in range(count) if not np.array_equal(out[i], out_n2[i])]
        assert not bad, bad
    assert same_on_every_engine(("mixed", n_bits), out)
    clean = [i for i in range(count) if admitted[i]]
    out2 = np.zeros((len(clean), 2 * kw), np.uint32)
    ctx.paillier_enc(n_bits, len(clean), np.ascontiguousarray(nw[clean]), kw, np.ascontiguousarray(mw[clean]), np.ascontiguousarray(rw[clean]), out2)
    lanes, ok = ctx.diag_basen_last()
    assert (lanes, ok) == (lanes_per_integer(ctx, n_bits), True)
    assert np.array_equal(out2, out[clean])
    # Enc-and-compare across the guard: one wrong item under an admitted key, one under a rejected one
    e2 = out.copy()
    e2[1, 3] ^= 4; e2[2, 2 * kw - 1] ^= 1                      # (lane 0 at the limit; lane 0 at + 1)
    v = np.full(count, 9, np.uint8)
    ctx.paillier_enc_check(n_bits, count, nw, kw, mw, rw, None, None, e2, v)
    assert list(v) == [0 if i in (1, 2) else 1 for i in range(count)]


@pytest.mark.parametrize("lanes", [12, 36], ids=["12-lanes-x-6-limbs", "five-wavefronts-of-36-lanes-x-2-limbs"])
def test_latency_ladders_under_the_limit_keys(lanes):
    """csrc/kernels_basen_r2l.hpp under the 2048-bit keys (every one of them qualifies at 9 limbs per lane): the ladder against the pair
    ladder it replaces, item by item, against Python on the edge cases and a random item, and against the other engines' words"""
    n_bits, kw = 2048, 64
    count = COUNT[n_bits]
    os.environ["ZKP_R2L_LANES"] = str(lanes)        # (read when the ctx is created)
    try:
        c = zkp.Context(0)
    finally:
        os.environ.pop("ZKP_R2L_LANES", None)
    try:
        c.set_geometry(9)
        for k, (name, deltas, n) in enumerate(keys_for(n_bits)):
            assert qualifies(n, n_bits, 9)
            ms, rs, mw, rw, py = shared_case(n_bits, k)
            nw = words(n, kw)
            outs = []
            for mode in (2, 0):
                c.set_r2l(mode)
                out = np.zeros((count, 2 * kw), np.uint32)
                c.paillier_enc(n_bits, count, nw, 0, mw, rw, out)
                assert c.last_geometry() == 9 and c.r2l_last() == (mode == 2), (name, mode)
                assert c.r2l_lanes_last() == (lanes if mode == 2 else 0), (name, mode, c.r2l_lanes_last())
                outs.append(out)
            assert np.array_equal(outs[0], outs[1]), name
            for i, want in py.items():
                assert from_words(outs[0][i]) == want, (name, i)
            assert same_on_every_engine(("shared", n_bits, k), outs[0]), name
            c.set_r2l(2)
            wrong = 5 + k
            e2 = outs[0].copy(); e2[wrong, k] ^= 2
            v = np.full(count, 9, np.uint8)
            c.paillier_enc_check(n_bits, count, nw, 0, mw, rw, None, None, e2, v)
            assert c.r2l_last() and list(v) == [0 if i == wrong else 1 for i in range(count)], name
    finally:
        c.close()


def test_range_proofs_under_keys_at_and_over_the_limit(oracle):
    """RangeProofNi prove + verify, 2 proofs x 128 rows, throughput engine in base-n form: under ONE key with every lane at the limit, then
    under per-proof keys [at the limit, over it], where the second proof's rows cross to the n^2-sized launch — transcripts byte for byte
    and verdicts (one response tampered with) against the oracle"""
    n_bits, B = 2048, 2
    keys = keys_for(n_bits)
    G = n_bits // 1024
    at_limit, over = keys[G * len(DELTAS)][2], keys[G * len(DELTAS) + 1][2]
    assert qualifies(at_limit, n_bits, 36) and not qualifies(over, n_bits, 36)
    oracle.set_threads(min(16, oracle.max_threads()))
    c = zkp.Context(0)
    try:
        c.set_geometry(36)
        c.set_enc_form("basen")
        for shared, ns in ((True, [at_limit]), (False, [at_limit, over])):
            cases = H.build_range_case(b"limit-keys-%d" % shared, ns, n_bits, B, shared=shared)
            pb_o, wt = H.fill_batch(cases, n_bits, shared, oracle)
            oracle.range_ni_prove(pb_o.struct(), wt.struct(), None, None, None)
            pb = zkp.RangeBatch(n_bits, B, 128, shared_key=shared)
            pb.n[:] = pb_o.n; pb.range[:] = pb_o.range; pb.ciphertext[:] = pb_o.ciphertext
            c.range_ni_prove(pb.struct(), wt.struct(), None, None, None, device=False)
            assert c.last_geometry() == 36
            assert c.diag_basen_last() == (2, shared), shared
            for f in ("c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2"):
                assert np.array_equal(getattr(pb_o, f), getattr(pb, f)), (shared, f)
            for tampered in (None, 0, 1):
                if tampered is not None:
                    pb.resp_r1[tampered, 9, 0] ^= 1
                vo = np.full(B, 9, np.uint8); vg = np.full(B, 9, np.uint8)
                oracle.range_ni_verify(pb.struct(), vo)
                c.range_ni_verify(pb.struct(), vg, device=False)
                assert c.diag_basen_last() == (2, shared), shared
                assert list(vg) == list(vo) == [0 if tampered is not None and b == tampered else 1 for b in range(B)], (shared, tampered)
                if tampered is not None:
                    pb.resp_r1[tampered, 9, 0] ^= 1
    finally:
        c.close()
