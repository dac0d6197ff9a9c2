"""GPU tests of seeded proving for VerlinProof and MulProof (include/zkp_hip.h: zkp_nonce_sample_coprime_batch,
zkp_verlin_proof_prove_seeded_batch, zkp_mul_proof_prove_seeded_batch): the device sampler — k_nonce_coprime for r_a / r_d, k_nonce_sample
for the rest — bit for bit against tests/seeded_coprime_model.py, each seeded prove against the nonce-input prove fed the model's nonces
and against the oracle, a modulus 3 q whose gcd-rejected candidates pass through the whole prove, device pointers, chunk invariance, the
wipe of the device blocks, refused arguments, and the C++ host layer."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import seeded_coprime_cases as SC
import seeded_coprime_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu

SEED = SC.SEED
MALFORMED = zkp.VERDICT_MALFORMED
STALE = 0xA5A5A5A5
EXTRA = zkp.capi.Z1_EXTRA_LIMBS


def to_dev(a):
    import torch
    return None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(t, like):
    return t.cpu().numpy().view(like.dtype)


def fresh(*arrays):
    return [np.full_like(a, 7) for a in arrays]


def same(what, *triples):
    for name, a, b in triples:
        assert np.array_equal(a, b), (what, name)


# ---- 1. the sampler against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.sampler_cases()))
def test_sampler_is_bit_exact_against_the_model(ctx, name):
    c = SC.sampler_cases()[name]
    kind, n_bits, B = c["kind"], c["n_bits"], c["B"]
    kw = n_bits // 32
    want_nonces, want_status, _, _ = SC.model_nonces(name)
    want = SC.field_arrays(kind, want_nonces, kw)
    n = L.ints_to_limbs(c["n_list"], kw)
    stride = kw if len(c["n_list"]) > 1 else 0
    got = [None if w is None else np.full(w.shape, STALE, np.uint32) for w in want]      # (stale data: unwritten rows would show)
    status = np.full(B, 9, np.uint8)
    if c["device"]:
        import torch
        dgot, dst, dn = [to_dev(g) for g in got], to_dev(status), to_dev(n)
        torch.cuda.synchronize()
        ctx.nonce_sample_coprime(kind, n_bits, B, dn, stride, SEED, c["first_index"], dgot, dst)
        ctx.synchronize()
        got = [None if g is None else to_host(d, g) for g, d in zip(got, dgot)]
        status = dst.cpu().numpy()
    else:
        ctx.nonce_sample_coprime(kind, n_bits, B, n, stride, SEED, c["first_index"], got, status)
    assert ctx.witness_residue() == 0
    assert list(status) == want_status
    for f, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        for b in range(B):
            assert np.array_equal(g[b], w[b]), (name, "field", f, "proof", b)
            if want_status[b]:
                assert not g[b].any(), "the nonces of a MALFORMED proof are zero"


# ---- 2. the seeded proves against the nonce-input proves and the oracle -----------------------------------------------------------------
PROVE_CASES = [(*s, False) for s in SC.SHAPES] + [(*SC.THREE_Q, True)]
VERLIN_OUT = ("phi_a", "z", "z_prime", "z_double_prime", "r_z")
MUL_OUT = ("f", "z1", "z2", "e_d", "e_db")


@pytest.mark.parametrize("n_bits,B,first_index,three_q", PROVE_CASES)
def test_verlin_proof_seeded_equals_nonce_input_prove_and_the_oracle(ctx, oracle, n_bits, B, first_index, three_q):
    a = SC.verlin_case(n_bits, B, first_index, three_q)
    n, stride, c, cp, phi_x, wit, non = a["n"], a["stride"], a["c"], a["cp"], a["phi_x"], a["wit"], a["nonce"]
    if three_q:
        assert a["not_coprime"][1] + a["not_coprime"][3] >= 1        # a gcd-rejected candidate stands before the r_a of this call
    o = oracle.verlin_proof_prove(n_bits, n, stride, c, cp, phi_x, wit, non)
    w = fresh(*o)
    ctx.verlin_proof_prove(n_bits, B, n, stride, c, cp, phi_x, wit, non, w)
    s, st = fresh(*o), np.full(B, 9, np.uint8)
    ctx.verlin_proof_prove_seeded(n_bits, B, n, stride, c, cp, phi_x, wit, SEED, first_index, s, st)
    assert ctx.witness_residue() == 0
    same("seeded against the nonce-input prove", *zip(VERLIN_OUT, w, s))
    same("seeded against the oracle", *zip(VERLIN_OUT, o, s))
    assert not st.any()
    s2 = fresh(*o)
    ctx.verlin_proof_prove_seeded(n_bits, B, n, stride, c, cp, phi_x, wit, SEED, first_index, s2)        # (out_status is nullable)
    assert ctx.witness_residue() == 0
    same("without a status array", *zip(VERLIN_OUT, s, s2))
    v = np.full(B, 9, np.uint8)
    ctx.verlin_proof_verify(n_bits, B, n, stride, c, cp, phi_x, *s, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] * B


@pytest.mark.parametrize("n_bits,B,first_index,three_q", PROVE_CASES)
def test_mul_proof_seeded_equals_nonce_input_prove_and_the_oracle(ctx, oracle, n_bits, B, first_index, three_q):
    a = SC.mul_case(n_bits, B, first_index, three_q)
    n, stride, e, wit, non = a["n"], a["stride"], a["e"], a["wit"], a["nonce"]
    if three_q:
        assert a["not_coprime"][1] + a["not_coprime"][3] >= 1        # a gcd-rejected candidate stands before the r_d of this call
    *o, so = oracle.mul_proof_prove(n_bits, n, stride, *e, *wit, *non)
    assert not so.any()
    w, sw = fresh(*o), np.full(B, 9, np.uint8)
    ctx.mul_proof_prove(n_bits, B, n, stride, *e, *wit, *non, *w, sw)
    s, ss = fresh(*o), np.full(B, 9, np.uint8)
    ctx.mul_proof_prove_seeded(n_bits, B, n, stride, *e, *wit, SEED, first_index, *s, ss)
    assert ctx.witness_residue() == 0
    same("seeded against the nonce-input prove", *zip(MUL_OUT, w, s), ("status", sw, ss))
    same("seeded against the oracle", *zip(MUL_OUT, o, s), ("status", so, ss))
    v = np.full(B, 9, np.uint8)
    ctx.mul_proof_verify(n_bits, B, n, stride, *e, *s, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] * B


# ---- 3. device pointers -----------------------------------------------------------------------------------------------------------------
def test_mul_proof_seeded_on_device_tensors(ctx, oracle):
    import torch
    n_bits, B, first_index = SC.SHAPES[1]
    a = SC.mul_case(n_bits, B, first_index)
    *o, so = oracle.mul_proof_prove(n_bits, a["n"], a["stride"], *a["e"], *a["wit"], *a["nonce"])
    dn, de, dwit = to_dev(a["n"]), [to_dev(x) for x in a["e"]], [to_dev(x) for x in a["wit"]]
    ds = [to_dev(x) for x in fresh(*o)]
    dst = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.mul_proof_prove_seeded(n_bits, B, dn, a["stride"], *de, *dwit, SEED, first_index, *ds, dst)
    assert ctx.witness_residue() == 0
    ctx.synchronize()
    same("device pointers against the oracle", *zip(MUL_OUT, o, [to_host(t, x) for t, x in zip(ds, o)]), ("status", so, dst.cpu().numpy()))
    # the caller's own witness tensors are not the call's to wipe
    same("the witness tensors", *zip(SC.MUL_WIT, a["wit"], [to_host(t, x) for t, x in zip(dwit, a["wit"])]))


# ---- 4. chunk invariance ----------------------------------------------------------------------------------------------------------------
def test_two_half_calls_equal_one_call(ctx):
    n_bits, B, first_index = SC.SHAPES[1]
    kw, zw = n_bits // 32, n_bits // 32 + EXTRA
    a = SC.verlin_case(n_bits, B, first_index)          # (the statement only: the nonces of this test are those of first_index 5)
    n, stride, c, cp, phi_x, wit = a["n"], a["stride"], a["c"], a["cp"], a["phi_x"], a["wit"]
    one = [np.full((B, w), 7, np.uint32) for w in (2 * kw, zw, zw, zw, 2 * kw)]
    two = fresh(*one)
    ctx.verlin_proof_prove_seeded(n_bits, B, n, stride, c, cp, phi_x, wit, SEED, 5, one)
    for lo in (0, B // 2):
        hi = lo + B // 2
        ctx.verlin_proof_prove_seeded(n_bits, B // 2, n[lo:hi], stride, c[lo:hi], cp[lo:hi], phi_x[lo:hi], [x[lo:hi] for x in wit], SEED, 5 + lo,
                                      [x[lo:hi] for x in two])
    same("VerlinProof: two calls of B / 2 with first_index 5 and 5 + B / 2", *zip(VERLIN_OUT, one, two))
    m = SC.mul_case(n_bits, B, first_index)
    one, s1 = [np.full((B, w), 7, np.uint32) for w in (kw, 2 * kw, 2 * kw, 2 * kw, 2 * kw)], np.full(B, 9, np.uint8)
    two, s2 = fresh(*one), np.full(B, 9, np.uint8)
    ctx.mul_proof_prove_seeded(n_bits, B, m["n"], m["stride"], *m["e"], *m["wit"], SEED, SC.BIG, *one, s1)
    for lo in (0, B // 2):
        hi = lo + B // 2
        ctx.mul_proof_prove_seeded(n_bits, B // 2, m["n"][lo:hi], m["stride"], *[x[lo:hi] for x in m["e"]], *[x[lo:hi] for x in m["wit"]], SEED, SC.BIG + lo,
                                   *[x[lo:hi] for x in two], s2[lo:hi])
    same("MulProof: two calls of B / 2", *zip(MUL_OUT, one, two), ("status", s1, s2))
    assert not s1.any() and any(x.any() for x in one)


# ---- 5. / 6. the wipe on an error path, refused arguments ---------------------------------------------------------------------------------
def test_residue_after_an_error_part_way(ctx):
    n_bits, B, first_index = SC.SHAPES[1]
    kw, zw = n_bits // 32, n_bits // 32 + EXTRA
    a = SC.verlin_case(n_bits, B, first_index)
    outs = [np.zeros((B, w), np.uint32) for w in (2 * kw, zw, zw, zw, 2 * kw)]
    x, xp, xpp, rx = a["wit"]
    # a null witness pointer is found by the nonce-input call, after the sampler ran
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_verlin_proof_prove_batch"):
        ctx.verlin_proof_prove_seeded(n_bits, B, a["n"], a["stride"], a["c"], a["cp"], a["phi_x"], (x, xp, xpp, None), SEED, 0, outs)
    assert ctx.witness_residue() == 0
    m = SC.mul_case(n_bits, B, first_index)
    aa, bb, ra, rb, rc = m["wit"]
    mouts = [np.zeros((B, w), np.uint32) for w in (kw, 2 * kw, 2 * kw, 2 * kw, 2 * kw)]
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_mul_proof_prove_batch"):
        ctx.mul_proof_prove_seeded(n_bits, B, m["n"], m["stride"], *m["e"], aa, None, ra, rb, rc, SEED, 0, *mouts, np.zeros(B, np.uint8))
    assert ctx.witness_residue() == 0
    assert not any(o.any() for o in outs + mouts)


def test_refused_arguments(ctx):
    n_bits, B = 1024, 2
    kw, zw = n_bits // 32, n_bits // 32 + EXTRA
    n = L.ints_to_limbs([H.test_key(1024)[2]], kw)
    wide = np.zeros((B, 2 * kw), np.uint32)
    r = np.zeros((B, kw), np.uint32)
    st = np.zeros(B, np.uint8)
    fields = [r.copy() for _ in range(4)]
    vouts = [np.zeros((B, w), np.uint32) for w in (2 * kw, zw, zw, zw, 2 * kw)]
    mouts = [np.zeros((B, w), np.uint32) for w in (kw, 2 * kw, 2 * kw, 2 * kw, 2 * kw)]
    # a null seed
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_nonce_sample_coprime_batch"):
        ctx.nonce_sample_coprime(M.KIND_VERLIN, n_bits, B, n, 0, None, 0, fields, st)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_verlin_proof_prove_seeded_batch"):
        ctx.verlin_proof_prove_seeded(n_bits, B, n, 0, wide, wide, wide, (r, r, r, r), None, 0, vouts, st)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_mul_proof_prove_seeded_batch"):
        ctx.mul_proof_prove_seeded(n_bits, B, n, 0, wide, wide, wide, r, r, r, r, r, None, 0, *mouts, st)
    # the kinds of zkp_nonce_sample_batch, and unknown ones
    for kind in (0, 4, 7):
        with pytest.raises(zkp.ZkpError, match="status 1: zkp_nonce_sample_coprime_batch"):
            ctx.nonce_sample_coprime(kind, n_bits, B, n, 0, SEED, 0, fields, st)
    # a missing field array
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_nonce_sample_coprime_batch"):
        ctx.nonce_sample_coprime(M.KIND_VERLIN, n_bits, B, n, 0, SEED, 0, fields[:3] + [None], st)
    # nothing was launched: the arrays of these calls are as they were
    assert not any(f.any() for f in fields) and not any(o.any() for o in vouts + mouts) and not st.any()
    # Mul reads two field arrays only
    ctx.nonce_sample_coprime(M.KIND_MUL, n_bits, B, n, 0, SEED, 0, fields[:2] + [None, None], st)
    assert fields[0].any() and fields[1].any() and not fields[2].any() and not st.any()


# ---- 7. the C++ host layer ----------------------------------------------------------------------------------------------------------------
def test_cpp_prove_batch_seeded_then_verify():
    """tests/cpp/test_seeded_coprime.cpp, built and run the way tests/test_gpu_seeded_nonces.py builds test_seeded_sigma.cpp"""
    root, pkg = H.ROOT, os.path.join(H.ROOT, "zk-paillier_amd")
    src, exe = os.path.join(root, "tests", "cpp", "test_seeded_coprime.cpp"), os.path.join(root, "build", "test_seeded_coprime")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", exe, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 1 and "FAIL" not in out.stdout, out.stdout + out.stderr
