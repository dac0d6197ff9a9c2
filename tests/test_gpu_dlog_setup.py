"""GPU tests of zkp_dlog_statement_setup_seeded_batch (include/zkp_hip.h; csrc/kernels_jacobi.hpp: k_nonce_jacobi, then the inverse and the
ladder): g = h1, ni = h2, secret and status bit for bit against tests/seeded_dlog_setup_model.py at every key width and batch size of
tests/seeded_dlog_setup_cases.py (tests/test_seeded_dlog_setup_model.py asserts on the CPU what those inputs contain), chunk invariance,
the failing rows among intact neighbours, the reference's own two tests end to end, device pointers, the wipe, refused arguments, and the
C++ host class."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import seeded_dlog_setup_cases as DC
import seeded_dlog_setup_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu

SEED = DC.SEED
MALFORMED = zkp.VERDICT_MALFORMED
STALE = 0xA5A5A5A5
Y_BITS = 544


@pytest.fixture(scope="module")
def own_ctx():
    """one context with the library's own routing: the set-up's kernels are the throughput library's whatever the geometry"""
    c = zkp.Context(0)
    yield c
    c.close()


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def setup(ctx, n_bits, N, first_index, seed=SEED, with_status=True):
    B, kw = len(N), n_bits // 32
    g, ni, sec = np.full((B, kw), STALE, np.uint32), np.full((B, kw), STALE, np.uint32), np.full((B, 8), STALE, np.uint32)      # (stale data: unwritten rows would show)
    st = np.full(B, 9, np.uint8)
    ctx.dlog_statement_setup_seeded(n_bits, B, N, seed, first_index, g, ni, sec, st if with_status else None)
    assert ctx.witness_residue() == 0
    return g, ni, sec, st


# ---- 1. against the model, 5. the failing rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", DC.BATCHES)
@pytest.mark.parametrize("n_bits", DC.WIDTHS)
def test_setup_is_bit_exact_against_the_model(own_ctx, n_bits, B):
    N, wg, wni, wsec, wst = DC.arrays(n_bits, B)
    g, ni, sec, st = setup(own_ctx, n_bits, N, DC.first_index(n_bits, B))
    assert list(st) == wst
    for b in range(B):
        assert np.array_equal(g[b], wg[b]) and np.array_equal(sec[b], wsec[b]) and np.array_equal(ni[b], wni[b]), (n_bits, B, "statement", b)
    if B > 1:
        # the square of a prime and the even modulus: MALFORMED with zero outputs, their neighbours intact (compared above)
        for b in (DC.SQUARE_ROW, DC.EVEN_ROW):
            assert st[b] == MALFORMED and not g[b].any() and not ni[b].any() and not sec[b].any()
        assert all(g[b].any() and ni[b].any() and sec[b].any() for b in range(B) if b not in (DC.SQUARE_ROW, DC.EVEN_ROW))
        g2, ni2, sec2, _ = setup(own_ctx, n_bits, N, DC.first_index(n_bits, B), with_status=False)          # (out_status is nullable)
        assert np.array_equal(g, g2) and np.array_equal(ni, ni2) and np.array_equal(sec, sec2)


# ---- 2. chunk invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [1024, 2048])
def test_a_call_split_at_64_equals_the_one_call(own_ctx, n_bits):
    B = 130
    N, wg, wni, wsec, wst = DC.arrays(n_bits, B)
    first = DC.first_index(n_bits, B)
    parts = [setup(own_ctx, n_bits, np.ascontiguousarray(N[lo:hi]), first + lo) for lo, hi in ((0, 64), (64, B))]
    g, ni, sec, st = (np.concatenate([p[k] for p in parts]) for k in range(4))
    assert np.array_equal(g, wg) and np.array_equal(ni, wni) and np.array_equal(sec, wsec) and list(st) == wst


# ---- 3. the reference's tests, end to end ---------------------------------------------------------------------------------------------------
def reference_statements(ctx):
    n_bits, B = DC.E2E
    N = L.ints_to_limbs(list(DC.e2e_moduli()), n_bits // 32)
    g, ni, sec, st = setup(ctx, n_bits, N, 0)
    assert not st.any()
    return n_bits, B, N, g, ni, sec


def prove_and_verify(ctx, n_bits, B, N, g, ni, sec):
    kw = n_bits // 32
    x, y, st = np.zeros((B, kw), np.uint32), np.zeros((B, Y_BITS // 32), np.uint32), np.full(B, 9, np.uint8)
    ctx.dlog_prove_seeded(n_bits, Y_BITS, B, N, g, ni, sec, DC.PROVE_SEED, 0, x, y, st)          # (another seed than the set-up's)
    assert not st.any()
    v = np.full(B, 9, np.uint8)
    ctx.dlog_verify(n_bits, Y_BITS, B, N, g, ni, x, y, v)
    return list(v)


def test_correct_dlog_proof(own_ctx):
    """wi_dlog_proof.rs:117-141: h1 of symbol -1, secret, h2 = (h1^-1)^secret; prove; verify"""
    n_bits, B, N, g, ni, sec = reference_statements(own_ctx)
    assert prove_and_verify(own_ctx, n_bits, B, N, g, ni, sec) == [zkp.VERDICT_ACCEPT] * B


def test_bad_dlog_proof(own_ctx):
    """wi_dlog_proof.rs:143-170: h2 = h1^secret, without the inverse — the proof does not verify"""
    n_bits, B, N, g, ni, sec = reference_statements(own_ctx)
    ns = DC.e2e_moduli()
    bad = L.ints_to_limbs([pow(L.limbs_to_int(g[b]), L.limbs_to_int(sec[b]), ns[b]) for b in range(B)], n_bits // 32)
    assert not np.array_equal(bad, ni)
    assert prove_and_verify(own_ctx, n_bits, B, N, g, bad, sec) == [zkp.VERDICT_REJECT] * B


# ---- 4. device pointers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [1024, 4096])
def test_setup_on_device_tensors(own_ctx, n_bits):
    import torch
    B = 65
    N, wg, wni, wsec, wst = DC.arrays(n_bits, B)
    kw = n_bits // 32
    dN = to_dev(N)
    dg, dni, dsec = (torch.full((B, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for w in (kw, kw, 8))
    dst = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    own_ctx.dlog_statement_setup_seeded(n_bits, B, dN, SEED, DC.first_index(n_bits, B), dg, dni, dsec, dst)
    assert own_ctx.witness_residue() == 0
    own_ctx.synchronize()
    got = [t.cpu().numpy().view(np.uint32) for t in (dg, dni, dsec)]
    assert np.array_equal(got[0], wg) and np.array_equal(got[1], wni) and np.array_equal(got[2], wsec) and list(dst.cpu().numpy()) == wst
    assert np.array_equal(dN.cpu().numpy().view(np.uint32), N)


# ---- 6. refused arguments, the wipe ---------------------------------------------------------------------------------------------------------
def test_refused_arguments(own_ctx):
    B, kw = 2, 32
    N = L.ints_to_limbs([DC.honest(1024, 0)] * B, kw)
    g, ni, sec, st = np.zeros((B, kw), np.uint32), np.zeros((B, kw), np.uint32), np.zeros((B, 8), np.uint32), np.zeros(B, np.uint8)
    name = "status 1: zkp_dlog_statement_setup_seeded_batch"
    with pytest.raises(zkp.ZkpError, match=name):
        own_ctx.dlog_statement_setup_seeded(1024, B, N, None, 0, g, ni, sec, st)          # a null seed
    with pytest.raises(zkp.ZkpError, match=name):
        own_ctx.dlog_statement_setup_seeded(3072, B, N, SEED, 0, g, ni, sec, st)          # a width zkp_dlog_prove_batch does not take
    for k in range(3):
        outs = [g, ni, sec]
        outs[k] = None
        with pytest.raises(zkp.ZkpError, match=name):
            own_ctx.dlog_statement_setup_seeded(1024, B, N, SEED, 0, *outs, st)
    with pytest.raises(zkp.ZkpError, match=name):
        own_ctx.dlog_statement_setup_seeded(1024, B, None, SEED, 0, g, ni, sec, st)
    assert not g.any() and not ni.any() and not sec.any() and not st.any()               # nothing was launched
    own_ctx.dlog_statement_setup_seeded(1024, 0, None, SEED, 0, None, None, None, None)   # an empty call is fine


# ---- 7. the C++ host layer ------------------------------------------------------------------------------------------------------------------
def test_cpp_generate_batch_seeded_then_prove_and_verify():
    """tests/cpp/test_dlog_setup.cpp, built and run the way tests/test_gpu_seeded_coprime.py builds test_seeded_coprime.cpp"""
    root, pkg = H.ROOT, os.path.join(H.ROOT, "zk-paillier_amd")
    src, exe = os.path.join(root, "tests", "cpp", "test_dlog_setup.cpp"), os.path.join(root, "build", "test_dlog_setup")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", exe, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 1 and "FAIL" not in out.stdout, out.stdout + out.stderr
