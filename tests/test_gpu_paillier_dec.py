"""GPU tests of zkp_paillier_open_batch (include/zkp_hip.h; csrc/kernels_paillier_dec.hpp) on the case list of tests/paillier_dec_cases.py,
exactly against tests/paillier_dec_model.py and against the (m0, r0) that were encrypted: round trips under one key at every key size, one key
per item, ciphertexts at and above n^2, the domain rules, device pointers, the wipe.  Through the session `ctx` fixture: every engine runs the
ladder once."""
import numpy as np
import pytest

import paillier_dec_cases as PC
from helpers import L, zkp

pytestmark = pytest.mark.gpu


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def run_open(ctx, b, with_r=True, device=False, with_status=True):
    """-> ([(m, r | None, status)], modexps the ladder ran)"""
    n_bits, B = b["n_bits"], len(b["c"])
    hw, kw = n_bits // 64, n_bits // 32
    shared = len(b["keys"]) == 1
    p, q = L.ints_to_limbs([k[0] for k in b["keys"]], hw), L.ints_to_limbs([k[1] for k in b["keys"]], hw)
    c = L.ints_to_limbs(b["c"], 2 * kw)
    m, r, st = np.full((B, kw), 9, np.uint32), np.full((B, kw), 9, np.uint32), np.full(B, 9, np.uint8)
    ctx.timing_reset(True)
    if device:
        import torch
        dp, dq, dc, dm, dr, dst = (to_dev(a) for a in (p, q, c, m, r, st))
        torch.cuda.synchronize()
        ctx.paillier_open(n_bits, B, dp, dq, 0 if shared else hw, dc, dm, dr if with_r else None, dst if with_status else None, device=True)
        ctx.synchronize()
        m, r, st = dm.cpu().numpy().view(np.uint32), dr.cpu().numpy().view(np.uint32), dst.cpu().numpy()
    else:
        ctx.paillier_open(n_bits, B, p, q, 0 if shared else hw, c, m, r if with_r else None, st if with_status else None)
    modexps = ctx.timing_get()[2]
    ctx.timing_reset(False)
    return [(L.limbs_to_int(m[i]), L.limbs_to_int(r[i]) if with_r else None, int(st[i])) for i in range(B)], modexps


def assert_same(got, b, with_r=True):
    want = b["want"] if with_r else [(m, None, s) for m, _, s in b["want"]]
    bad = [(i, b["tag"][i], got[i][2], want[i][2]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:4]


@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_round_trip_one_key(ctx, n_bits):
    b = PC.one_key(n_bits)
    got, modexps = run_open(ctx, b)
    assert_same(got, b)
    assert [(m, r) for m, r, _ in got] == b["truth"]
    assert modexps == 4 * len(b["c"])
    got, half = run_open(ctx, b, with_r=False)
    assert_same(got, b, with_r=False)
    assert half == 2 * len(b["c"]), "decrypt only: the root ladders must not run"


def test_one_key_per_item(ctx):
    b = PC.per_item_keys()
    got, _ = run_open(ctx, b)
    assert_same(got, b)
    assert [(m, r) for m, r, _ in got] == b["truth"]


@pytest.mark.parametrize("which", ["one key 1024", "one key 2048", "one key 4096", "per-item keys"])
def test_ciphertexts_at_and_above_n_squared(ctx, which):
    b = PC.widened(dict(PC.all_batches())[which])
    got, _ = run_open(ctx, b)
    assert_same(got, b)


def test_domain(ctx):
    """status 2 and zero outputs exactly where the model says; every good neighbour untouched (the add-back key among them)"""
    b = PC.domain()
    got, _ = run_open(ctx, b)
    assert_same(got, b)
    assert sum(g[2] == 2 for g in got) >= 9
    got, _ = run_open(ctx, b, with_status=False)                 # (out_status is nullable)
    assert [g[:2] for g in got] == [w[:2] for w in b["want"]]


def test_bad_key_shared_by_the_whole_call(ctx):
    b = PC.one_key(1024)
    p, q = b["keys"][0]
    bad = dict(b, keys=[(p, p)], c=b["c"][:20], tag=b["tag"][:20], want=[(0, 0, 2)] * 20)
    got, _ = run_open(ctx, bad)
    assert_same(got, bad)


def test_device_pointers_equal_host_pointers(ctx):
    for b in (PC.domain(), PC.per_item_keys()):
        host, _ = run_open(ctx, b)
        dev, _ = run_open(ctx, b, device=True)
        assert host == dev
        assert_same(dev, b)


def test_secrets_are_wiped(ctx):
    """the registered regions are every block of the call that held p, q or something derived from them — the ladder's constants records
    (they hold the moduli p^2, q^2, p, q) and window tables are blocks of the call too, not the ctx's persistent buffers; under a pinned
    secondary engine the whole call, its blocks and this answer are that engine's"""
    b = PC.one_key(1024)
    run_open(ctx, b)
    assert ctx.witness_residue() == 0
    run_open(ctx, PC.domain(), with_r=False)
    assert ctx.witness_residue() == 0


def test_bad_arguments(ctx):
    lib, h = zkp.load(), ctx.h
    a = np.zeros(4096, np.uint32)
    A = a.ctypes.data
    E = zkp.capi.ZKP_EINVAL
    assert lib.zkp_paillier_open_batch(h, 1000, 1, A, A, 0, A, A, None, None, 0) == E
    assert lib.zkp_paillier_open_batch(h, 8192, 1, A, A, 0, A, A, None, None, 0) == E
    assert lib.zkp_paillier_open_batch(h, 1024, 1, A, A, 32, A, A, None, None, 0) == E          # key_stride: 0 or hw = 16
    assert lib.zkp_paillier_open_batch(h, 1024, 1, A, A, 1, A, A, None, None, 0) == E
    for args in ((None, A, A, A), (A, None, A, A), (A, A, None, A), (A, A, A, None)):
        assert lib.zkp_paillier_open_batch(h, 1024, 1, args[0], args[1], 0, args[2], args[3], None, None, 0) == E
    assert lib.zkp_paillier_open_batch(h, 1024, 0, None, None, 0, None, None, None, None, 0) == zkp.capi.ZKP_OK
    assert lib.zkp_paillier_open_batch(h, 1024, 0, None, None, 16, None, None, None, None, 0) == zkp.capi.ZKP_OK
