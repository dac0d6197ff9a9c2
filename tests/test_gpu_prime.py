"""GPU tests of zkp_probable_prime_batch, zkp_next_prime_batch and zkp_paillier_keygen_seeded_batch (include/zkp_hip.h;
csrc/kernels_prime.hpp) on the inputs of tests/prime_cases.py, bit for bit against tests/prime_model.py: the tail classes and the base-2
pseudoprimes of the test, the windows of the search, generated keys, chunk independence, device pointers, the wipe, the argument checks,
and the keys' way through the calls that take them."""
import numpy as np
import pytest

import prime_cases as PC
import prime_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu

SEED, ROUNDS, FI = PC.SEED, PC.ROUNDS, PC.FIRST_INDEX


@pytest.fixture(scope="module")
def pctx():
    c = zkp.Context(0)
    yield c
    c.close()


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def from_dev(t, dtype):
    return t.cpu().numpy().view(dtype)


def run_test(ctx, bits, values, rounds, first_index=FI, device=False):
    pw = bits // 32
    w = L.ints_to_limbs(values, pw)
    v = np.full(len(values), 9, np.uint8)
    seed = SEED if rounds else None
    if device:
        import torch
        dw, dv = to_dev(w), to_dev(v)
        torch.cuda.synchronize()
        ctx.probable_prime(bits, len(values), dw, rounds, seed, first_index, dv)
        ctx.synchronize()
        v = from_dev(dv, np.uint8)
    else:
        ctx.probable_prime(bits, len(values), w, rounds, seed, first_index, v)
    assert ctx.witness_residue() == 0
    return [int(x) for x in v]


def run_next(ctx, bits, starts, rounds, first_index=FI, device=False, with_offset=True, with_status=True):
    pw, B = bits // 32, len(starts)
    s = L.ints_to_limbs(starts, pw)
    p, off, st = np.full((B, pw), 9, np.uint32), np.full(B, 9, np.uint32), np.full(B, 9, np.uint8)
    seed = SEED if rounds else None
    if device:
        import torch
        ds, dp, doff, dst = (to_dev(a) for a in (s, p, off, st))
        torch.cuda.synchronize()
        ctx.next_prime(bits, B, ds, rounds, seed, first_index, dp, doff if with_offset else None, dst if with_status else None)
        ctx.synchronize()
        p, off, st = from_dev(dp, np.uint32), from_dev(doff, np.uint32), from_dev(dst, np.uint8)
    else:
        ctx.next_prime(bits, B, s, rounds, seed, first_index, p, off if with_offset else None, st if with_status else None)
    assert ctx.witness_residue() == 0
    return [(L.limbs_to_int(p[b]), int(off[b]) if with_offset else None, int(st[b]) if with_status else None) for b in range(B)]


def run_keygen(ctx, n_bits, batch, first_index, rounds=ROUNDS, device=False, with_n=True, with_status=True):
    hw, kw = n_bits // 64, n_bits // 32
    p, q, n, st = np.full((batch, hw), 9, np.uint32), np.full((batch, hw), 9, np.uint32), np.full((batch, kw), 9, np.uint32), np.full(batch, 9, np.uint8)
    if device:
        import torch
        dp, dq, dn, dst = (to_dev(a) for a in (p, q, n, st))
        torch.cuda.synchronize()
        ctx.paillier_keygen_seeded(n_bits, batch, rounds, SEED, first_index, dp, dq, dn if with_n else None, dst if with_status else None)
        ctx.synchronize()
        p, q, n, st = from_dev(dp, np.uint32), from_dev(dq, np.uint32), from_dev(dn, np.uint32), from_dev(dst, np.uint8)
    else:
        ctx.paillier_keygen_seeded(n_bits, batch, rounds, SEED, first_index, p, q, n if with_n else None, st if with_status else None)
    assert ctx.witness_residue() == 0
    return [(L.limbs_to_int(p[b]), L.limbs_to_int(q[b]), L.limbs_to_int(n[b]) if with_n else None, int(st[b]) if with_status else None) for b in range(batch)]


# ---- 1. the test
@pytest.mark.parametrize("bits,count", [(512, 1), (512, 65), (512, 130), (1024, 1), (1024, 65), (1024, 130), (2048, 1), (2048, 17)])
def test_probable_prime_matches_the_model(pctx, bits, count):
    values, where = PC.test_batch(bits, count)
    want0, want5 = PC.test_want(bits, count, 0), PC.test_want(bits, count, ROUNDS)
    got0, got5 = run_test(pctx, bits, values, 0), run_test(pctx, bits, values, ROUNDS)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got0, want0)) if g != w] + [(i, g, w) for i, (g, w) in enumerate(zip(got5, want5)) if g != w]
    print(f"bits {bits} count {count}: {sum(got0)} accepted at rounds 0, {sum(got5)} at rounds {ROUNDS}, {len(bad)} differ from the model")
    assert not bad, bad[:6]
    if count > 1:                                               # the base-2 pseudoprimes: accepted by base 2 alone, rejected with the bases
        for name in ("b-round-1", "b-later-round"):
            for i in where[name]:
                assert (got0[i], got5[i]) == (1, 0), (name, i)
        assert [i for i in range(count) if got0[i] != got5[i]] == sorted(where["b-round-1"] + where["b-later-round"])


# ---- 2. the search
def test_next_prime_on_the_window_cases(pctx):
    starts, names, want = PC.next_batch()
    got = run_next(pctx, 512, starts, ROUNDS)
    bad = [(names[i], got[i][1:], want[i][1:]) for i in range(len(starts)) if got[i] != want[i]]
    print("next_prime:", [(names[i], got[i][1], got[i][2]) for i in range(len(starts))])
    assert not bad, bad
    for i, name in enumerate(names):                            # zero outputs at status 2, between intact neighbours
        if want[i][2] == M.MALFORMED:
            assert got[i] == (0, 0, 2), name
    # nullable out_offset / out_status
    bare = run_next(pctx, 512, starts, ROUNDS, with_offset=False, with_status=False)
    assert [g[0] for g in bare] == [w[0] for w in want]


def test_next_prime_alone_and_wider(pctx):
    starts, names, want = PC.next_batch()
    i = names.index("ordinary")
    assert run_next(pctx, 512, [starts[i]], ROUNDS, first_index=FI + i) == [want[i]]
    for bits in (1024, 2048):                                   # the same small starts in wider arrays; a start of the full width
        s = [0, starts[names.index("small")], (1 << bits) - 1, (1 << (bits - 1)) + 12345]
        w = []
        for k, x in enumerate(s):
            p, j = M.next_prime(x, bits, ROUNDS, SEED, FI + k)
            w.append((p, j, 0) if p is not None else (0, 0, 2))
        assert run_next(pctx, bits, s, ROUNDS) == w


# ---- 3. keygen
@pytest.mark.parametrize("n_bits,batch", [(1024, 1), (1024, 67), (2048, 5), (4096, 2)])
def test_keygen_matches_the_model(pctx, n_bits, batch):
    want, attempts, _ = PC.keygen_want(n_bits, batch)
    got = run_keygen(pctx, n_bits, batch, PC.KEYGEN_FIRST_INDEX[n_bits])
    bad = [b for b in range(batch) if got[b] != want[b]]
    print(f"keygen {n_bits} x {batch}: attempts {[a for a in attempts if max(a)]}, {len(bad)} keys differ from the model")
    assert not bad, bad[:4]
    assert all(k[3] == 0 and k[2] == k[0] * k[1] and k[2].bit_length() in (n_bits, n_bits - 1) for k in got)


# ---- 3b. a few rows per slot and round.  Left to itself the library gives the few slots of these batches 64 rows each, so every prime
# falls in a window's first round; with a small fixed chunk the search goes from round to round (dead candidates leave the map, the
# next survivors are chosen behind them) and, below ROUNDS, a candidate's bases span two rounds.  No result may depend on it.
@pytest.fixture(params=PC.SMALL_CHUNKS)
def small_chunk(pctx, request):
    lib = zkp.load()
    assert lib.zkp_diag_prime_search(pctx.h, request.param, 1, None, None) == zkp.capi.ZKP_OK
    yield request.param
    assert lib.zkp_diag_prime_search(pctx.h, 0, 0, None, None) == zkp.capi.ZKP_OK


def last_search(ctx):
    import ctypes as C
    rows, rounds = C.c_uint64(), C.c_uint64()
    assert zkp.load().zkp_diag_prime_search(ctx.h, -1, -1, C.byref(rows), C.byref(rounds)) == zkp.capi.ZKP_OK
    return rows.value, rounds.value


def test_keygen_under_small_chunks(pctx, small_chunk):
    want, _, stats = PC.keygen_want(1024, 67)
    got = run_keygen(pctx, 1024, 67, PC.KEYGEN_FIRST_INDEX[1024])
    rows, rounds = last_search(pctx)
    print(f"keygen 1024 x 67 at {small_chunk} rows per slot and round: {rows} ladder rows in {rounds} rounds")
    assert got == want
    deepest = max(s["survivors_before"] for k in stats for s in k)
    assert rounds >= deepest // small_chunk + 1                   # that prime's window alone takes so many base-2 rounds
    want = PC.keygen_want(2048, 5)[0]
    assert run_keygen(pctx, 2048, 5, PC.KEYGEN_FIRST_INDEX[2048], device=True) == want


def test_next_prime_and_test_under_small_chunks(pctx, small_chunk):
    starts, names, want = PC.next_batch()
    assert run_next(pctx, 512, starts, ROUNDS) == want
    _, rounds = last_search(pctx)
    assert rounds >= max(PC.next_depths().values()) // small_chunk + 1            # the deepest prime's window alone takes so many base-2 rounds
    assert run_next(pctx, 512, starts, 0) == [((p, j, 0) if p is not None else (0, 0, 2)) for p, j in (M.next_prime(s, 512) for s in starts)]
    values, _ = PC.test_batch(512, 65)
    assert run_test(pctx, 512, values, ROUNDS) == PC.test_want(512, 65, ROUNDS)     # (the test's own chunk is 1: five bases, five rounds)


def test_the_built_in_rows_are_back(pctx):
    run_keygen(pctx, 1024, 1, PC.KEYGEN_FIRST_INDEX[1024])
    rows, rounds = last_search(pctx)
    assert rows % 64 == 0 and rounds <= 6, (rows, rounds)          # two slots, 64 rows each per round


# ---- 4. chunks
def test_keygen_chunks_equal_one_call(pctx):
    fi = PC.KEYGEN_FIRST_INDEX[1024]
    whole = run_keygen(pctx, 1024, 130, fi)
    assert whole[:67] == PC.keygen_want(1024, 67)[0]
    assert whole == run_keygen(pctx, 1024, 64, fi) + run_keygen(pctx, 1024, 66, fi + 64)


def test_test_and_search_chunks_equal_one_call(pctx):
    values, _ = PC.test_batch(512, 65)
    assert run_test(pctx, 512, values, ROUNDS) == run_test(pctx, 512, values[:9], ROUNDS) + run_test(pctx, 512, values[9:], ROUNDS, first_index=FI + 9)
    starts, _, want = PC.next_batch()
    assert run_next(pctx, 512, starts[:4], ROUNDS) + run_next(pctx, 512, starts[4:], ROUNDS, first_index=FI + 4) == want


# ---- 5. device tensors, stale outputs (every run_* pre-fills its outputs with 9s and reads the residue)
def test_device_pointers(pctx):
    values, _ = PC.test_batch(512, 65)
    assert run_test(pctx, 512, values, ROUNDS, device=True) == PC.test_want(512, 65, ROUNDS)
    starts, _, want = PC.next_batch()
    assert run_next(pctx, 512, starts, ROUNDS, device=True) == want
    assert run_keygen(pctx, 2048, 5, PC.KEYGEN_FIRST_INDEX[2048], device=True) == PC.keygen_want(2048, 5)[0]
    bare = run_keygen(pctx, 1024, 1, PC.KEYGEN_FIRST_INDEX[1024], device=True, with_n=False, with_status=False)
    assert [k[:2] for k in bare] == [k[:2] for k in PC.keygen_want(1024, 1)[0]]


# ---- 6. end to end: a generated key through the calls that take one
@pytest.mark.parametrize("n_bits,batch", [(1024, 3), (2048, 2)])
def test_generated_keys_serve_the_other_calls(pctx, n_bits, batch):
    ctx = pctx
    hw, kw = n_bits // 64, n_bits // 32
    keys = run_keygen(ctx, n_bits, batch, PC.KEYGEN_FIRST_INDEX[n_bits])
    assert keys == PC.keygen_want(n_bits, PC.KEYGEN_SHAPES_BY_BITS[n_bits])[0][:batch]
    p, q, n = (L.ints_to_limbs([k[i] for k in keys], w) for i, w in ((0, hw), (1, hw), (2, kw)))
    # NiCorrectKeyProof: prove with the factors, verify with n
    salt = b"KZen"
    out_n, sg, st = np.zeros((batch, kw), np.uint32), np.zeros((batch, 11, kw), np.uint32), np.full(batch, 9, np.uint8)
    ctx.correct_key_ni_prove(n_bits, batch, p, q, salt, out_n, sg, st)
    assert list(st) == [0] * batch and np.array_equal(out_n, n)
    v = np.full(batch, 9, np.uint8)
    ctx.correct_key_ni_verify(n_bits, batch, n, sg, salt, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] * batch
    # Paillier: encrypt under n, open with the factors
    ms = [(0x1234567 << (8 * b)) + b for b in range(batch)]
    rs = [((keys[b][2] >> 3) | 1) - 2 * b for b in range(batch)]
    m, r = L.ints_to_limbs(ms, kw), L.ints_to_limbs(rs, kw)
    ct = np.zeros((batch, 2 * kw), np.uint32)
    ctx.paillier_enc(n_bits, batch, n, kw, m, r, ct)
    om, orr, ost = np.zeros((batch, kw), np.uint32), np.zeros((batch, kw), np.uint32), np.full(batch, 9, np.uint8)
    ctx.paillier_open(n_bits, batch, p, q, hw, ct, om, orr, ost)
    assert list(ost) == [0] * batch and L.limbs_to_ints(om) == ms and L.limbs_to_ints(orr) == rs
    # ring-Pedersen parameters over n: seeded set-up, CompositeDLogProof prove and verify
    g, ni, sec, dst = np.zeros((batch, kw), np.uint32), np.zeros((batch, kw), np.uint32), np.zeros((batch, 8), np.uint32), np.full(batch, 9, np.uint8)
    ctx.dlog_statement_setup_seeded(n_bits, batch, n, bytes(range(32)), 5, g, ni, sec, dst)
    assert list(dst) == [0] * batch
    y_bits = 544
    x, y, pst = np.zeros((batch, kw), np.uint32), np.zeros((batch, y_bits // 32), np.uint32), np.full(batch, 9, np.uint8)
    ctx.dlog_prove_seeded(n_bits, y_bits, batch, n, g, ni, sec, bytes(range(1, 33)), 0, x, y, pst)          # (another seed than the set-up's)
    assert not pst.any()
    dv = np.full(batch, 9, np.uint8)
    ctx.dlog_verify(n_bits, y_bits, batch, n, g, ni, x, y, dv)
    assert list(dv) == [zkp.VERDICT_ACCEPT] * batch


# ---- 7. refused arguments
def test_bad_arguments(pctx):
    ctx = pctx
    lib, h = zkp.load(), ctx.h
    a = np.full(4096, 9, np.uint32)
    A = a.ctypes.data
    E, OK = zkp.capi.ZKP_EINVAL, zkp.capi.ZKP_OK
    T, N, K = lib.zkp_probable_prime_batch, lib.zkp_next_prime_batch, lib.zkp_paillier_keygen_seeded_batch
    assert T(None, 512, 1, A, 0, None, 0, A, 0) == E
    assert N(None, 512, 1, A, 0, None, 0, A, A, A, 0) == E
    assert K(None, 1024, 1, 5, SEED, 0, A, A, A, A, 0) == E
    for bits in (0, 256, 768, 4096):
        assert T(h, bits, 1, A, 0, None, 0, A, 0) == E
        assert N(h, bits, 1, A, 0, None, 0, A, A, A, 0) == E
    for n_bits in (512, 1536, 8192):
        assert K(h, n_bits, 1, 5, SEED, 0, A, A, A, A, 0) == E
    assert T(h, 512, 1, None, 0, None, 0, A, 0) == E and T(h, 512, 1, A, 0, None, 0, None, 0) == E
    assert N(h, 512, 1, None, 0, None, 0, A, A, A, 0) == E and N(h, 512, 1, A, 0, None, 0, None, A, A, 0) == E
    assert K(h, 1024, 1, 5, SEED, 0, None, A, A, A, 0) == E and K(h, 1024, 1, 5, SEED, 0, A, None, A, A, 0) == E
    assert T(h, 512, 1, A, 5, None, 0, A, 0) == E                # rounds without a seed
    assert N(h, 512, 1, A, 1, None, 0, A, A, A, 0) == E
    assert K(h, 1024, 1, 0, None, 0, A, A, A, A, 0) == E          # keygen always needs one
    assert T(h, 512, 1, A, 65, SEED, 0, A, 0) == E and N(h, 512, 1, A, 65, SEED, 0, A, A, A, 0) == E and K(h, 1024, 1, 65, SEED, 0, A, A, A, A, 0) == E
    assert T(h, 512, 1, A, 0, None, 0, A, 2) == E and N(h, 512, 1, A, 0, None, 0, A, A, A, 4) == E and K(h, 1024, 1, 5, SEED, 0, A, A, A, A, 2) == E
    big = (1 << 20) + 1
    assert T(h, 512, big, A, 0, None, 0, A, 0) == E and N(h, 512, big, A, 0, None, 0, A, A, A, 0) == E and K(h, 1024, big, 5, SEED, 0, A, A, A, A, 0) == E
    assert lib.zkp_last_error_string(h)
    assert ctx.witness_residue() == 0
    assert T(h, 512, 0, None, 0, None, 0, None, 0) == OK and N(h, 512, 0, None, 0, None, 0, None, None, None, 0) == OK
    assert K(h, 1024, 0, 5, SEED, 0, None, None, None, None, 0) == OK
    assert (a == 9).all()
    assert ctx.witness_residue() == 0


# ---- 8. the C++ host layer
def test_cpp_keypair_and_prime_test():
    """tests/cpp/test_keygen.cpp, built and run the way tests/test_gpu_dlog_setup.py builds test_dlog_setup.cpp"""
    import os
    import subprocess

    import helpers as H
    root, pkg = H.ROOT, os.path.join(H.ROOT, "zk-paillier_amd")
    src, exe = os.path.join(root, "tests", "cpp", "test_keygen.cpp"), os.path.join(root, "build", "test_keygen")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", exe, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 3 and "FAIL" not in out.stdout, out.stdout + out.stderr
