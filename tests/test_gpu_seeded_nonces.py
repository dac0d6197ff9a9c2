"""GPU tests of seeded proving for ZeroProof, CiphertextProof, CorrectMessageProof and CompositeDLogProof (include/zkp_hip.h:
zkp_nonce_sample_batch and the four zkp_*_prove_seeded_batch): the device sampler bit for bit against tests/seeded_nonce_model.py, each
seeded prove against the nonce-input prove fed the model's nonces and against the oracle, device pointers, chunk invariance, the wipe of
the device blocks, refused arguments, and the C++ host layer."""
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import seeded_nonce_cases as SC
import seeded_nonce_model as M
from helpers import L, pm, zkp

pytestmark = pytest.mark.gpu

SEED = SC.SEED
MALFORMED = zkp.VERDICT_MALFORMED
STALE = 0xA5A5A5A5
Y_BITS = 768


def to_dev(a):
    import torch
    return None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(t, like):
    return t.cpu().numpy().view(like.dtype)


# ---- 1. the sampler against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.sampler_cases()))
def test_sampler_is_bit_exact_against_the_model(ctx, name):
    c = SC.sampler_cases()[name]
    kind, n_bits, B, K = c["kind"], c["n_bits"], c["B"], c["K"]
    kw = n_bits // 32
    want_nonces, want_status, _ = SC.model_nonces(name)
    want = SC.field_arrays(kind, want_nonces, kw, K)
    n = L.ints_to_limbs(c["n_list"], kw) if c["n_list"] else None
    stride = kw if len(c["n_list"]) > 1 else 0
    got = [None if w is None or w.size == 0 else np.full(w.shape, STALE, np.uint32) for w in want]      # (stale data: unwritten rows would show)
    status = np.full(B, 9, np.uint8)
    if c["device"]:
        import torch
        dgot, dst, dn = [to_dev(g) for g in got], to_dev(status), to_dev(n)
        torch.cuda.synchronize()
        ctx.nonce_sample(kind, n_bits, B, K, dn, stride, SEED, c["first_index"], dgot, dst)
        ctx.synchronize()
        got = [None if g is None else to_host(d, g) for g, d in zip(got, dgot)]
        status = dst.cpu().numpy()
    else:
        ctx.nonce_sample(kind, n_bits, B, K, n, stride, SEED, c["first_index"], got, status)
    assert list(status) == want_status
    for f, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        for b in range(B):
            assert np.array_equal(g[b], w[b]), (name, "field", f, "proof", b)
            if want_status[b]:
                assert not g[b].any(), "the nonces of a MALFORMED proof are zero"


# ---- 2. the seeded proves against the nonce-input proves and the oracle -----------------------------------------------------------------
SHAPES = [(2048, 3, 0), (1024, 4, SC.BIG)]


def keys_for(n_bits, B):
    """the 2048-bit fixture key, shared; two 1024-bit keys, one per proof"""
    if n_bits == 2048:
        return [H.fixture_key()[2]], 0
    return [H.test_key(1024, tag=b % 2)[2] for b in range(B)], n_bits // 32


def fresh(*arrays):
    return [np.full_like(a, 7) for a in arrays]


def same(what, *triples):
    for name, a, b in triples:
        assert np.array_equal(a, b), (what, name)


@functools.lru_cache(maxsize=None)
def sigma_case(n_bits, B, first_index, kind):
    keys, stride = keys_for(n_bits, B)
    kw = n_bits // 32
    d = pm.Drbg(b"seeded-sigma-%d-%d" % (n_bits, kind))
    per = [keys[b % len(keys)] for b in range(B)]
    x = [d.below(n) if kind == M.KIND_CIPHERTEXT else 0 for n in per]
    r = [d.below(n) for n in per]
    nonces, status, _ = M.nonces(kind, SEED, first_index, keys, B)
    assert not any(status)
    a = dict(n=L.ints_to_limbs(keys, kw), c=L.ints_to_limbs([pm.enc(n, m, rr) for n, m, rr in zip(per, x, r)], 2 * kw), x=L.ints_to_limbs(x, kw),
             r=L.ints_to_limbs(r, kw), stride=stride)
    a["nonce"] = SC.field_arrays(kind, nonces, kw, 1)
    return a


@pytest.mark.parametrize("n_bits,B,first_index", SHAPES)
def test_zero_proof_seeded_equals_nonce_input_prove_and_the_oracle(ctx, oracle, n_bits, B, first_index):
    a = sigma_case(n_bits, B, first_index, M.KIND_ZERO)
    n, stride, c, r, rp = a["n"], a["stride"], a["c"], a["r"], a["nonce"][0]
    zo, ao = oracle.zero_proof_prove(n_bits, n, stride, c, r, rp)
    zw, aw = fresh(zo, ao)
    ctx.zero_proof_prove(n_bits, B, n, stride, c, r, rp, zw, aw)
    zs, as_ = fresh(zo, ao)
    st = np.full(B, 9, np.uint8)
    ctx.zero_proof_prove_seeded(n_bits, B, n, stride, c, r, SEED, first_index, zs, as_, st)
    assert ctx.witness_residue() == 0
    same("seeded against the nonce-input prove", ("z", zw, zs), ("a", aw, as_))
    same("seeded against the oracle", ("z", zo, zs), ("a", ao, as_))
    assert not st.any()
    v = np.full(B, 9, np.uint8)
    ctx.zero_proof_verify(n_bits, B, n, stride, c, zs, as_, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] * B


@pytest.mark.parametrize("n_bits,B,first_index", SHAPES)
def test_ciphertext_proof_seeded_equals_nonce_input_prove_and_the_oracle(ctx, oracle, n_bits, B, first_index):
    a = sigma_case(n_bits, B, first_index, M.KIND_CIPHERTEXT)
    n, stride, c, x, r, (xp, rp, _, _) = a["n"], a["stride"], a["c"], a["x"], a["r"], a["nonce"]
    o = oracle.ciphertext_proof_prove(n_bits, n, stride, c, x, r, xp, rp)
    w = fresh(*o)
    ctx.ciphertext_proof_prove(n_bits, B, n, stride, c, x, r, xp, rp, *w)
    s = fresh(*o)
    ctx.ciphertext_proof_prove_seeded(n_bits, B, n, stride, c, x, r, SEED, first_index, *s)        # (out_status is nullable)
    assert ctx.witness_residue() == 0
    names = ("z1", "z2", "c_prime")
    same("seeded against the nonce-input prove", *zip(names, w, s))
    same("seeded against the oracle", *zip(names, o, s))
    v = np.full(B, 9, np.uint8)
    ctx.ciphertext_proof_verify(n_bits, B, n, stride, c, *s, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] * B


CM_K = 4


@functools.lru_cache(maxsize=None)
def message_case(n_bits, B, first_index):
    """K = 4, the real message at position b of proof b; in the 1024-bit case the LAST proof encrypts a message that is not in its list"""
    keys, stride = keys_for(n_bits, B)
    kw = n_bits // 32
    d = pm.Drbg(b"seeded-message-%d" % n_bits)
    valid = [[d.below(1 << 64) + 3 for _ in range(CM_K)] for _ in range(B)]
    msg = [valid[b][b % CM_K] for b in range(B)]
    if n_bits == 1024:
        msg[-1] = valid[-1][0] + 1
    nonces, status, _ = M.nonces(M.KIND_CORRECT_MESSAGE, SEED, first_index, keys, B, CM_K)
    assert not any(status)
    return dict(n=L.ints_to_limbs(keys, kw), stride=stride, valid=np.stack([L.ints_to_limbs(v, kw) for v in valid]), msg=L.ints_to_limbs(msg, kw),
                nonce=SC.field_arrays(M.KIND_CORRECT_MESSAGE, nonces, kw, CM_K), bad_last=n_bits == 1024)


@pytest.mark.parametrize("n_bits,B,first_index", SHAPES)
def test_correct_message_seeded_equals_nonce_input_prove_and_the_oracle(ctx, oracle, n_bits, B, first_index):
    a = message_case(n_bits, B, first_index)
    n, stride, valid, msg, (r, w, e_sim, z_sim) = a["n"], a["stride"], a["valid"], a["msg"], a["nonce"]
    *o, so = oracle.correct_message_prove(n_bits, CM_K, n, stride, valid, msg, r, e_sim, z_sim, w)
    want_status = [0] * (B - 1) + [MALFORMED if a["bad_last"] else 0]
    assert list(so) == want_status
    g, sg = fresh(*o), np.full(B, 9, np.uint8)
    ctx.correct_message_prove(n_bits, B, CM_K, n, stride, valid, msg, r, e_sim, z_sim, w, *g, sg)
    s, ss = fresh(*o), np.full(B, 9, np.uint8)
    ctx.correct_message_prove_seeded(n_bits, B, CM_K, n, stride, valid, msg, SEED, first_index, *s, ss)
    assert ctx.witness_residue() == 0
    names = ("ciphertext", "e_vec", "z_vec", "a_vec")
    same("seeded against the nonce-input prove", *zip(names, g, s), ("status", sg, ss))
    same("seeded against the oracle", *zip(names, o, s), ("status", so, ss))
    v = np.full(B, 9, np.uint8)
    ctx.correct_message_verify(n_bits, B, CM_K, n, stride, valid, *s, v)
    assert list(v[:B - 1]) == [zkp.VERDICT_ACCEPT] * (B - 1) and (v[-1] == zkp.VERDICT_ACCEPT) == (not a["bad_last"])


@functools.lru_cache(maxsize=None)
def dlog_case(n_bits, B, first_index):
    kw = n_bits // 32
    d = pm.Drbg(b"seeded-dlog-%d" % n_bits)
    rows = []
    for b in range(B):
        N = H.fixture_key()[2] if n_bits == 2048 else H.test_key(n_bits, tag=b % 2)[2]
        g = d.range(2, N - 1); s = d.bits(256)
        rows.append((N, g, pow(pow(g, -1, N), s, N), s))
    nonces, _, _ = M.nonces(M.KIND_DLOG, SEED, first_index, [], B)
    N_, g_, ni_ = (L.ints_to_limbs([r[i] for r in rows], kw) for i in range(3))
    return N_, g_, ni_, L.ints_to_limbs([r[3] for r in rows], 8), SC.field_arrays(M.KIND_DLOG, nonces, kw, 1)[0]


@pytest.mark.parametrize("n_bits,B,first_index", SHAPES)
def test_dlog_seeded_equals_nonce_input_prove_and_the_oracle(ctx, oracle, n_bits, B, first_index):
    N, g, ni, secret, r = dlog_case(n_bits, B, first_index)
    o = oracle.dlog_prove(n_bits, Y_BITS, N, g, ni, secret, r)
    w = fresh(*o)
    ctx.dlog_prove(n_bits, Y_BITS, B, N, g, ni, secret, r, *w)
    s, st = fresh(*o), np.full(B, 9, np.uint8)
    ctx.dlog_prove_seeded(n_bits, Y_BITS, B, N, g, ni, secret, SEED, first_index, *s, st)
    assert ctx.witness_residue() == 0
    same("seeded against the nonce-input prove", *zip("xy", w, s))
    same("seeded against the oracle", *zip("xy", o, s))
    assert not st.any()
    v = np.full(B, 9, np.uint8)
    ctx.dlog_verify(n_bits, Y_BITS, B, N, g, ni, *s, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] * B


# ---- 3. device pointers -----------------------------------------------------------------------------------------------------------------
def test_correct_message_seeded_on_device_tensors(ctx, oracle):
    import torch
    n_bits, B, first_index = 1024, 4, SC.BIG
    a = message_case(n_bits, B, first_index)
    n, stride, valid, msg, (r, w, e_sim, z_sim) = a["n"], a["stride"], a["valid"], a["msg"], a["nonce"]
    *o, so = oracle.correct_message_prove(n_bits, CM_K, n, stride, valid, msg, r, e_sim, z_sim, w)
    dn, dvalid, dmsg = to_dev(n), to_dev(valid), to_dev(msg)
    ds = [to_dev(x) for x in fresh(*o)]
    dst = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.correct_message_prove_seeded(n_bits, B, CM_K, dn, stride, dvalid, dmsg, SEED, first_index, *ds, dst)
    assert ctx.witness_residue() == 0
    ctx.synchronize()
    same("device pointers against the oracle", *zip(("ciphertext", "e_vec", "z_vec", "a_vec"), o, [to_host(t, x) for t, x in zip(ds, o)]),
         ("status", so, dst.cpu().numpy()))


# ---- 4. chunk invariance ----------------------------------------------------------------------------------------------------------------
def test_two_half_calls_equal_one_call(ctx):
    n_bits, B = 1024, 4
    kw = n_bits // 32
    a = sigma_case(n_bits, B, SC.BIG, M.KIND_ZERO)          # (the statement only: the nonces of this test are those of first_index 0)
    n, stride, c, r = a["n"], a["stride"], a["c"], a["r"]
    one = [np.full((B, 2 * kw), 7, np.uint32) for _ in range(2)]
    two = fresh(*one)
    ctx.zero_proof_prove_seeded(n_bits, B, n, stride, c, r, SEED, 0, *one)
    for lo in (0, B // 2):
        hi = lo + B // 2
        ctx.zero_proof_prove_seeded(n_bits, B // 2, n[lo:hi], stride, c[lo:hi], r[lo:hi], SEED, lo, *[x[lo:hi] for x in two])
    same("ZeroProof: two calls of B / 2 with first_index 0 and B / 2", *zip("za", one, two))
    m = message_case(n_bits, B, SC.BIG)
    shapes = ((B, 2 * kw), (B, CM_K, 8), (B, CM_K, kw), (B, CM_K, 2 * kw))
    one, s1 = [np.full(s, 7, np.uint32) for s in shapes], np.full(B, 9, np.uint8)
    two, s2 = fresh(*one), np.full(B, 9, np.uint8)
    ctx.correct_message_prove_seeded(n_bits, B, CM_K, m["n"], m["stride"], m["valid"], m["msg"], SEED, 0, *one, s1)
    for lo in (0, B // 2):
        hi = lo + B // 2
        ctx.correct_message_prove_seeded(n_bits, B // 2, CM_K, m["n"][lo:hi], m["stride"], m["valid"][lo:hi], m["msg"][lo:hi], SEED, lo,
                                         *[x[lo:hi] for x in two], s2[lo:hi])
    same("CorrectMessageProof: two calls of B / 2", *zip(("ciphertext", "e_vec", "z_vec", "a_vec"), one, two), ("status", s1, s2))
    assert list(s1) == [0, 0, 0, MALFORMED]


# ---- 5. / 6. the wipe on an error path, refused arguments ---------------------------------------------------------------------------------
def test_residue_after_an_error_part_way(ctx):
    n_bits, B = 1024, 4
    kw = n_bits // 32
    a = sigma_case(n_bits, B, SC.BIG, M.KIND_CIPHERTEXT)
    n, stride, c, x, r = a["n"], a["stride"], a["c"], a["x"], a["r"]
    z1, z2, cp = np.zeros((B, kw + zkp.capi.Z1_EXTRA_LIMBS), np.uint32), np.zeros((B, 2 * kw), np.uint32), np.zeros((B, 2 * kw), np.uint32)
    # a null secret is found by the nonce-input call, after the sampler ran
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_zero_proof_prove_batch"):
        ctx.zero_proof_prove_seeded(n_bits, B, n, stride, c, None, SEED, 0, z2, cp)
    assert ctx.witness_residue() == 0
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_ciphertext_proof_prove_batch"):
        ctx.ciphertext_proof_prove_seeded(n_bits, B, n, stride, c, None, r, SEED, 0, z1, z2, cp)
    assert ctx.witness_residue() == 0
    m = message_case(n_bits, B, SC.BIG)
    outs = [np.zeros(s, np.uint32) for s in ((B, 2 * kw), (B, CM_K, 8), (B, CM_K, kw), (B, CM_K, 2 * kw))]
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_correct_message_prove_batch"):
        ctx.correct_message_prove_seeded(n_bits, B, CM_K, m["n"], m["stride"], m["valid"], None, SEED, 0, *outs, np.zeros(B, np.uint8))
    assert ctx.witness_residue() == 0
    N, g, ni, secret, _ = dlog_case(n_bits, B, SC.BIG)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_dlog_prove_batch"):
        ctx.dlog_prove_seeded(n_bits, Y_BITS, B, N, g, ni, None, SEED, 0, np.zeros((B, kw), np.uint32), np.zeros((B, Y_BITS // 32), np.uint32))
    assert ctx.witness_residue() == 0


def test_refused_arguments(ctx):
    n_bits, B = 1024, 2
    kw = n_bits // 32
    n = L.ints_to_limbs([H.test_key(1024)[2]], kw)
    z = np.zeros((B, 2 * kw), np.uint32)
    r = np.zeros((B, kw), np.uint32)
    st = np.zeros(B, np.uint8)
    valid = np.zeros((B, 2, kw), np.uint32)
    cm_outs = [np.zeros(s, np.uint32) for s in ((B, 2 * kw), (B, 2, 8), (B, 2, kw), (B, 2, 2 * kw))]
    fields = [r.copy(), r.copy(), np.zeros((B, 1, 8), np.uint32), np.zeros((B, 1, kw), np.uint32)]
    # a null seed
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_nonce_sample_batch"):
        ctx.nonce_sample(M.KIND_ZERO, n_bits, B, 1, n, 0, None, 0, fields[:1] + [None] * 3, st)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_zero_proof_prove_seeded_batch"):
        ctx.zero_proof_prove_seeded(n_bits, B, n, 0, z, r, None, 0, z.copy(), z.copy())
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_ciphertext_proof_prove_seeded_batch"):
        ctx.ciphertext_proof_prove_seeded(n_bits, B, n, 0, z, r, r, None, 0, np.zeros((B, kw + 16), np.uint32), z.copy(), z.copy())
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_correct_message_prove_seeded_batch"):
        ctx.correct_message_prove_seeded(n_bits, B, 2, n, 0, valid, r, None, 0, *cm_outs, st)
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_dlog_prove_seeded_batch"):
        ctx.dlog_prove_seeded(n_bits, Y_BITS, B, r, r, r, np.zeros((B, 8), np.uint32), None, 0, r.copy(), np.zeros((B, Y_BITS // 32), np.uint32))
    # an unknown kind
    for kind in (0, 5):
        with pytest.raises(zkp.ZkpError, match="status 1: zkp_nonce_sample_batch"):
            ctx.nonce_sample(kind, n_bits, B, 1, n, 0, SEED, 0, fields[:1] + [None] * 3, st)
    # K = 0 and K > 65536
    for K in (0, 65537):
        with pytest.raises(zkp.ZkpError, match="status 1: zkp_nonce_sample_batch"):
            ctx.nonce_sample(M.KIND_CORRECT_MESSAGE, n_bits, 1, K, n, 0, SEED, 0, fields, st)
        with pytest.raises(zkp.ZkpError, match="status 1: zkp_correct_message_prove_seeded_batch"):
            ctx.correct_message_prove_seeded(n_bits, 1, K, n, 0, valid, r, SEED, 0, *cm_outs, st)
    # nothing was launched: the arrays of these calls are as they were
    assert not any(f.any() for f in fields) and not any(o.any() for o in cm_outs) and not st.any()


# ---- 7. the C++ host layer ----------------------------------------------------------------------------------------------------------------
def test_cpp_prove_batch_seeded_then_verify_batch():
    """tests/cpp/test_seeded_sigma.cpp, built and run the way tests/test_gpu_seeded_prove.py builds test_seeded.cpp"""
    root, pkg = H.ROOT, os.path.join(H.ROOT, "zk-paillier_amd")
    src, exe = os.path.join(root, "tests", "cpp", "test_seeded_sigma.cpp"), os.path.join(root, "build", "test_seeded_sigma")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", exe, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 1 and "FAIL" not in out.stdout, out.stdout + out.stderr
