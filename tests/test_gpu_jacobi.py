"""GPU tests of zkp_jacobi_batch and zkp_legendre_batch (include/zkp_hip.h; csrc/kernels_jacobi.hpp): the Jacobi kernel on every pair of
tests/jacobi_cases.py — the hazard classes tests/test_wbjacobi_model.py runs its word model through — exactly against tests/jacobi_model.py,
at every row width, batch sizes around a block's edge, a shared and a per-row n, host and device pointers; the reference's legendre_symbol
on the fixture primes and on even, composite and tiny p; and legendre(a, p) legendre(a, q) == jacobi(a, p q) computed on the GPU."""
import random

import numpy as np
import pytest

import jacobi_cases as JC
from helpers import L, zkp
from jacobi_model import jacobi, legendre_symbol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def own_ctx():
    """these entry points run on the throughput library's kernels whatever the geometry: one context, the library's own choices"""
    c = zkp.Context(0)
    yield c
    c.close()


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def run_jacobi(ctx, mod_bits, a_list, n_list, device=False, with_status=True):
    """n_list of length 1: one shared n (stride 0)"""
    kw, B = mod_bits // 32, len(a_list)
    a, n = L.ints_to_limbs(a_list, kw), L.ints_to_limbs(n_list, kw)
    stride = kw if len(n_list) > 1 else 0
    sym, st = np.full(B, 9, np.int32), np.full(B, 9, np.uint8)
    if device:
        import torch
        da, dn, dsym, dst = to_dev(a), to_dev(n), to_dev(sym), to_dev(st)
        torch.cuda.synchronize()
        ctx.jacobi(mod_bits, B, da, dn, stride, dsym, dst if with_status else None)
        ctx.synchronize()
        return list(dsym.cpu().numpy()), list(dst.cpu().numpy())
    ctx.jacobi(mod_bits, B, a, n, stride, sym, st if with_status else None)
    return list(sym), list(st)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mod_bits", JC.WIDTHS + (8192,))
def test_every_case_against_the_definition(own_ctx, mod_bits, device):
    """per-row n, all cases of the width in one call (several blocks, an idle tail).  8192-bit rows (32 KB of LDS per block of 16 lanes)
    take every third non-random pair of the 4096-bit rows, zero-extended, plus random and close pairs of their own full width."""
    if mod_bits == 8192:
        rnd = random.Random(8192)
        cs = [(a, n) for tag, a, n in JC.cases(4096) if tag != "random"][::3] + [(rnd.getrandbits(8192), rnd.getrandbits(8192) | 1) for _ in range(40)]
        m = rnd.getrandbits(4000) | 1
        cs += [((m << 4096) + (1 << j), m << 4096 | 1) for j in (1, 40, 3000)]
        want = [JC.expected(a, n) for a, n in cs]
    else:
        cs = [(a, n) for _, a, n in JC.cases(mod_bits)]
        want = JC.expected_all(mod_bits)
    sym, st = run_jacobi(own_ctx, mod_bits, [a for a, _ in cs], [n for _, n in cs], device)
    bad = [(i, hex(cs[i][0]), hex(cs[i][1]), (sym[i], st[i]), want[i]) for i in range(len(cs)) if (sym[i], st[i]) != want[i]]
    assert not bad, bad[:3]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("mod_bits", [1024, 4096])
def test_batch_sizes_around_a_block(own_ctx, mod_bits, B):
    """a block's last lane, a second block, an idle tail: the cases are taken class by class, so every batch mixes long and short loops"""
    cs, want = JC.cases(mod_bits), JC.expected_all(mod_bits)
    pick = [(i * 7 + B) % len(cs) for i in range(B)]
    sym, st = run_jacobi(own_ctx, mod_bits, [cs[i][1] for i in pick], [cs[i][2] for i in pick])
    assert list(zip(sym, st)) == [want[i] for i in pick]
    sym2, _ = run_jacobi(own_ctx, mod_bits, [cs[i][1] for i in pick], [cs[i][2] for i in pick], with_status=False)       # (out_status is nullable)
    assert sym2 == sym


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mod_bits", JC.WIDTHS)
def test_shared_n(own_ctx, mod_bits, device):
    p, q = JC.fixture_primes()
    rnd = random.Random(mod_bits + 1)
    n = p * q if mod_bits >= 2048 else p
    a_list = [a for a in (0, 1, 2, n - 1, n, n + 1, p, 3 * p) if a < 1 << mod_bits] + [rnd.getrandbits(mod_bits) for _ in range(122)]
    sym, st = run_jacobi(own_ctx, mod_bits, a_list, [n], device)
    assert sym == [jacobi(a, n) for a in a_list] and not any(st)
    assert {-1, 0, 1} <= set(sym)
    sym, st = run_jacobi(own_ctx, mod_bits, a_list[:5], [n - 1], device)          # a shared even n: every row is outside the domain
    assert sym == [0] * 5 and st == [2] * 5


def test_refused_arguments(own_ctx):
    a, sym = np.zeros((2, 32), np.uint32), np.zeros(2, np.int32)
    for bits, stride in ((512, 0), (1024, 31), (3072, 0)):
        with pytest.raises(zkp.ZkpError, match="status 1: zkp_jacobi_batch"):
            own_ctx.jacobi(bits, 2, a, a, stride, sym)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_jacobi_batch"):
        own_ctx.jacobi(1024, 2, a, None, 0, sym)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_legendre_batch"):
        own_ctx.legendre(1024, 2, a, a, 0, sym)                                    # (the widths of zkp_modexp_batch only)
    own_ctx.jacobi(1024, 0, None, None, 0, None)                                   # an empty call is fine


# ---- zkp_legendre_batch -------------------------------------------------------------------------------------------------------------------
def run_legendre(ctx, mod_bits, a_list, p_list, device=False):
    kw, B = mod_bits // 32, len(a_list)
    a, p = L.ints_to_limbs(a_list, kw), L.ints_to_limbs(p_list, kw)
    stride = kw if len(p_list) > 1 else 0
    sym, st = np.full(B, 9, np.int32), np.full(B, 9, np.uint8)
    if device:
        import torch
        da, dp, dsym, dst = to_dev(a), to_dev(p), to_dev(sym), to_dev(st)
        torch.cuda.synchronize()
        ctx.legendre(mod_bits, B, da, dp, stride, dsym, dst)
        ctx.synchronize()
        return list(dsym.cpu().numpy()), list(dst.cpu().numpy())
    ctx.legendre(mod_bits, B, a, p, stride, sym, st)
    return list(sym), list(st)


def legendre_expected(a, p):
    """(symbol, status): the reference's value; status 2 and symbol 0 where it panics (p even) and outside our domain (p < 3, a >= p)"""
    if p < 3 or p % 2 == 0 or a >= p:
        return (0, 2)
    return (legendre_symbol(a, p), 0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_legendre_on_the_fixture_primes_and_on_even_composite_and_tiny_p(own_ctx, device):
    p, q = JC.fixture_primes()
    rnd = random.Random(5)
    pairs = []
    for pr in (p, q):
        pairs += [(a, pr) for a in (0, 1, 2, pr - 1, pr, pr + 1)] + [(rnd.randrange(pr), pr) for _ in range(12)]
    pairs += [(rnd.randrange(p - 1), p - 1), (3, p + 1), (0, 0), (0, 1), (1, 2), (2, 3), (1, 3), (0, 3), (4, 5), (2, 7), (3, 7)]       # even and tiny p
    pairs += [(a, p * q) for a in (0, 1, 2, p, 5 * q, rnd.randrange(p * q), rnd.randrange(p * q))] + [(2, 15), (7, 15), (4, 15), (5, 15)]   # composite p
    sym, st = run_legendre(own_ctx, 2048, [a for a, _ in pairs], [m for _, m in pairs], device)
    want = [legendre_expected(a, m) for a, m in pairs]
    assert list(zip(sym, st)) == want
    assert {w for w in want} >= {(1, 0), (-1, 0), (0, 2)}
    # a shared prime, and a wider row
    a_list = [rnd.randrange(p) for _ in range(5)]
    sym, st = run_legendre(own_ctx, 4096, a_list, [p], device)
    assert list(zip(sym, st)) == [legendre_expected(a, p) for a in a_list]


def test_legendre_product_is_the_jacobi_symbol_on_the_gpu(own_ctx):
    """the reference's route to (a / N) — two legendre_symbol calls with p and q — against the Jacobi kernel, which needs neither"""
    p, q = JC.fixture_primes()
    N = p * q
    rnd = random.Random(6)
    a_list = [rnd.randrange(1, N) for _ in range(130)]
    assert all(a % p and a % q for a in a_list)
    lp, sp = run_legendre(own_ctx, 2048, [a % p for a in a_list], [p])
    lq, sq = run_legendre(own_ctx, 2048, [a % q for a in a_list], [q])
    jn, sn = run_jacobi(own_ctx, 2048, a_list, [N])
    assert not any(sp) and not any(sq) and not any(sn)
    assert [x * y for x, y in zip(lp, lq)] == jn and set(jn) == {-1, 1}
    # the documented difference: for a == 0 mod p the reference's product is -legendre(a, q) — never 0 —, the Jacobi symbol is 0
    shared = [p * t for t in (1, 2, rnd.randrange(1, q))]
    lp, _ = run_legendre(own_ctx, 2048, [a % p for a in shared], [p])
    lq, _ = run_legendre(own_ctx, 2048, [a % q for a in shared], [q])
    jn, _ = run_jacobi(own_ctx, 2048, shared, [N])
    assert lp == [-1] * 3 and all(x in (-1, 1) for x in lq) and jn == [0] * 3
