"""ZeroProof (zero_enc_proof.rs) and CiphertextProof (correct_ciphertext.rs): oracle vs python model on the CPU,
HIP engine vs oracle on the GPU (SURVEY §8(f) rank 1 — compositions of the hot-path kernels)."""
import numpy as np
import pytest

import helpers as H
import small_proof_cases as SC
from helpers import pm, L, zkp


def make_cases(n_bits, keys, B, seed):
    d = pm.Drbg(seed)
    kw = n_bits // 32
    rows = []
    for b in range(B):
        n = keys[b % len(keys)]
        x, r, xp, rp = d.below(n), d.below(n), d.below(n), d.below(n)
        rows.append(dict(n=n, x=x, r=r, xp=xp, rp=rp, c0=pm.enc(n, 0, r), c1=pm.enc(n, 1, r), cx=pm.enc(n, x, r)))
    arr = lambda k, w: L.ints_to_limbs([q[k] for q in rows], w)
    return rows, dict(n=arr("n", kw), x=arr("x", kw), r=arr("r", kw), xp=arr("xp", kw), rp=arr("rp", kw),
                      c0=arr("c0", 2 * kw), c1=arr("c1", 2 * kw), cx=arr("cx", 2 * kw))


def test_oracle_matches_python_model(oracle):
    n_bits, kw = 1024, 32
    keys = [H.test_key(1024, tag=t)[2] for t in range(2)]
    rows, a = make_cases(n_bits, keys, 4, b"sigma-cpu")
    z, aa = oracle.zero_proof_prove(n_bits, a["n"], kw, a["c0"], a["r"], a["rp"])
    z1, z2, cp = oracle.ciphertext_proof_prove(n_bits, a["n"], kw, a["cx"], a["x"], a["r"], a["xp"], a["rp"])
    for b, q in enumerate(rows):
        assert (L.limbs_to_int(z[b]), L.limbs_to_int(aa[b])) == pm.zero_proof_prove(q["n"], q["c0"], q["r"], q["rp"])
        assert (L.limbs_to_int(z1[b]), L.limbs_to_int(z2[b]), L.limbs_to_int(cp[b])) == pm.ciphertext_proof_prove(q["n"], q["cx"], q["x"], q["r"], q["xp"], q["rp"])
        assert pm.zero_proof_verify(q["n"], q["c0"], L.limbs_to_int(z[b]), L.limbs_to_int(aa[b]))
        assert pm.ciphertext_proof_verify(q["n"], q["cx"], L.limbs_to_int(z1[b]), L.limbs_to_int(z2[b]), L.limbs_to_int(cp[b]))
    assert list(oracle.zero_proof_verify(n_bits, a["n"], kw, a["c0"], z, aa)) == [1] * 4            # test_zero_proof, zero_enc_proof.rs:112-131
    assert list(oracle.ciphertext_proof_verify(n_bits, a["n"], kw, a["cx"], z1, z2, cp)) == [1] * 4  # test_ciphertext_proof, correct_ciphertext.rs:113-134
    # test_one_proof (zero_enc_proof.rs:134-155): c encrypts 1 -> rejected
    z_, a_ = oracle.zero_proof_prove(n_bits, a["n"], kw, a["c1"], a["r"], a["rp"])
    assert list(oracle.zero_proof_verify(n_bits, a["n"], kw, a["c1"], z_, a_)) == [0] * 4
    # test_bad_ciphertext_proof (correct_ciphertext.rs:137-162): witness r + 1 -> rejected
    r_bad = L.ints_to_limbs([q["r"] + 1 for q in rows], kw)
    z1b, z2b, cpb = oracle.ciphertext_proof_prove(n_bits, a["n"], kw, a["cx"], a["x"], r_bad, a["xp"], a["rp"])
    assert list(oracle.ciphertext_proof_verify(n_bits, a["n"], kw, a["cx"], z1b, z2b, cpb)) == [0] * 4


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits,shared", [(1024, False), (2048, True), (4096, True)])
def test_gpu_sigma_proofs_match_oracle(ctx, oracle, n_bits, shared):
    kw = n_bits // 32
    if n_bits == 2048:
        keys = [H.fixture_key()[2]]
    else:
        keys = [H.test_key(n_bits, tag=t)[2] for t in range(1 if shared else 3)]
    B = 5 if n_bits < 4096 else 3
    rows, a = make_cases(n_bits, keys, B, b"sigma-gpu-%d" % n_bits)
    n_arr = a["n"][:1] if shared else a["n"]
    stride = 0 if shared else kw
    oracle.set_threads(min(8, oracle.max_threads()))
    # ---- ZeroProof: honest statement c0, dishonest statement c1 (encrypts 1)
    for cc, expect in ((a["c0"], 1), (a["c1"], 0)):
        zo, ao = oracle.zero_proof_prove(n_bits, n_arr, stride, cc, a["r"], a["rp"])
        zg = np.zeros_like(zo); ag = np.zeros_like(ao)
        ctx.zero_proof_prove(n_bits, B, n_arr, stride, cc, a["r"], a["rp"], zg, ag)
        assert np.array_equal(zo, zg) and np.array_equal(ao, ag)
        # tamper the last proof's z
        zt = zg.copy(); zt[B - 1, 0] ^= 1
        vo = oracle.zero_proof_verify(n_bits, n_arr, stride, cc, zt, ag)
        vg = np.full(B, 9, np.uint8)
        ctx.zero_proof_verify(n_bits, B, n_arr, stride, cc, zt, ag, vg)
        assert np.array_equal(vo, vg) and list(vo) == [expect] * (B - 1) + [0]
    # ---- CiphertextProof
    z1o, z2o, cpo = oracle.ciphertext_proof_prove(n_bits, n_arr, stride, a["cx"], a["x"], a["r"], a["xp"], a["rp"])
    z1g = np.zeros_like(z1o); z2g = np.zeros_like(z2o); cpg = np.zeros_like(cpo)
    ctx.ciphertext_proof_prove(n_bits, B, n_arr, stride, a["cx"], a["x"], a["r"], a["xp"], a["rp"], z1g, z2g, cpg)
    assert np.array_equal(z1o, z1g) and np.array_equal(z2o, z2g) and np.array_equal(cpo, cpg)
    z1t = z1g.copy(); z1t[0, 3] ^= 2            # tamper z1 of proof 0
    cpt = cpg.copy(); cpt[1, 5] ^= 1            # tamper c' of proof 1 (changes the challenge)
    vo = oracle.ciphertext_proof_verify(n_bits, n_arr, stride, a["cx"], z1t, z2g, cpt)
    vg = np.full(B, 9, np.uint8)
    ctx.ciphertext_proof_verify(n_bits, B, n_arr, stride, a["cx"], z1t, z2g, cpt, vg)
    assert np.array_equal(vo, vg) and list(vo) == [0, 0] + [1] * (B - 2)


# ================================================================== wide batches and operand edges (tests/small_proof_cases.py)
def _zero_wide(oracle, shared):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.sigma_wide(oracle, shared)
        bt, a = cs["bt"], cs["a"]
        z, aa = oracle.zero_proof_prove(*bt.key(), a["c0"], a["r"], a["rp"])
        zt = SC.flip(z, cs["tamper"])
        return cs, z, aa, oracle.zero_proof_verify(*bt.key(), a["c0"], z, aa), zt, oracle.zero_proof_verify(*bt.key(), a["c0"], zt, aa)
    return SC.cached("zero-wide-%d" % shared, build)


def _ciphertext_wide(oracle, shared):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = _zero_wide(oracle, shared)[0]               # (one set of inputs for both kinds)
        bt, a = cs["bt"], cs["a"]
        z1, z2, cp = oracle.ciphertext_proof_prove(*bt.key(), a["cx"], a["x"], a["r_ct"], a["xp"], a["rp"])
        half = len(cs["tamper"]) // 2
        z1t, z2t = SC.flip(z1, cs["tamper"][:half]), SC.flip(z2, cs["tamper"][half:])
        return (cs, z1, z2, cp, oracle.ciphertext_proof_verify(*bt.key(), a["cx"], z1, z2, cp), z1t, z2t,
                oracle.ciphertext_proof_verify(*bt.key(), a["cx"], z1t, z2t, cp))
    return SC.cached("ciphertext-wide-%d" % shared, build)


@pytest.mark.parametrize("shared", [False, True], ids=["per-proof-keys", "shared-key"])
def test_wide_sigma_cases_are_what_they_claim(oracle, shared):
    """CPU: the oracle's verdicts on the 300-proof batches are ACCEPT / REJECT exactly where the builder put honest / dishonest items"""
    cs, z, aa, vh, zt, vt = _zero_wide(oracle, shared)
    SC.check_wide_verdicts(cs, vh, vt)
    cs, z1, z2, cp, vh, z1t, z2t, vt = _ciphertext_wide(oracle, shared)
    SC.check_wide_verdicts(cs, vh, vt)


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["per-proof-keys", "shared-key"])
def test_gpu_zero_proof_wide_batch(ctx, oracle, shared):
    """300 ZeroProofs at n = 1024: a second, partial 256-thread block in k_sigma_hash / k_words_compare, a GROUPS_PER_BLOCK tail in k_enc,
    modexp_core (256-bit per-item exponents) and k_modmul.  shared-key: the sliding-window schedule path of enc_launch."""
    cs, zo, ao, vh, zt, vt = _zero_wide(oracle, shared)
    bt, a = cs["bt"], cs["a"]
    assert bt.B > 256
    SC.check_wide_verdicts(cs, vh, vt)
    zg, ag = SC.sentinel(zo.shape), SC.sentinel(ao.shape)
    ctx.zero_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["c0"], a["r"], a["rp"], zg, ag)
    SC.assert_same(ao, ag, "a")
    SC.assert_same(zo, zg, "z")
    for z, want in ((zg, vh), (zt, vt)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.zero_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["c0"], z, ag, vg)
        SC.assert_same(want, vg, "verdict")


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["per-proof-keys", "shared-key"])
def test_gpu_ciphertext_proof_wide_batch(ctx, oracle, shared):
    """300 CiphertextProofs at n = 1024 (see test_gpu_zero_proof_wide_batch); z1 = x' + x e is k_sigma_hash's multiply-add in both blocks"""
    cs, z1o, z2o, cpo, vh, z1t, z2t, vt = _ciphertext_wide(oracle, shared)
    bt, a = cs["bt"], cs["a"]
    assert bt.B > 256
    SC.check_wide_verdicts(cs, vh, vt)
    z1g, z2g, cpg = SC.sentinel(z1o.shape), SC.sentinel(z2o.shape), SC.sentinel(cpo.shape)
    ctx.ciphertext_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["cx"], a["x"], a["r_ct"], a["xp"], a["rp"], z1g, z2g, cpg)
    for name, x, y in (("c_prime", cpo, cpg), ("z1", z1o, z1g), ("z2", z2o, z2g)):
        SC.assert_same(x, y, name)
    for z1, z2, want in ((z1g, z2g, vh), (z1t, z2t, vt)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.ciphertext_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["cx"], z1, z2, cpg, vg)
        SC.assert_same(want, vg, "verdict")


# ---- operand edges
def _zero_edges(oracle, n_bits):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.cached("sigma-edges-%d" % n_bits, lambda: SC.sigma_edges(oracle, n_bits))
        bt, a = cs["bt"], cs["a"]
        z, aa = oracle.zero_proof_prove(*bt.key(), a["c0"], a["r"], a["rp"])
        vh = oracle.zero_proof_verify(*bt.key(), a["c0"], z, aa)
        ed, over = SC.zero_edits(cs, z, aa)
        return cs, z, aa, vh, ed, over, oracle.zero_proof_verify(*bt.key(), ed["c"], ed["z"], ed["a"])
    return SC.cached("zero-edges-%d" % n_bits, build)


def _ciphertext_edges(oracle, n_bits):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.cached("sigma-edges-%d" % n_bits, lambda: SC.sigma_edges(oracle, n_bits))
        bt, a = cs["bt"], cs["a"]
        z1, z2, cp = oracle.ciphertext_proof_prove(*bt.key(), a["cx"], a["x"], a["r"], a["xp"], a["rp"])
        vh = oracle.ciphertext_proof_verify(*bt.key(), a["cx"], z1, z2, cp)
        ed, over = SC.ciphertext_edits(cs, z1, z2, cp)
        return cs, z1, z2, cp, vh, ed, over, oracle.ciphertext_proof_verify(*bt.key(), ed["c"], ed["z1"], ed["z2"], ed["cp"])
    return SC.cached("ciphertext-edges-%d" % n_bits, build)


def test_sigma_edge_cases_oracle_matches_python_model(oracle):
    """CPU: the operand edges of tests/small_proof_cases.py (n = 1024) through the C oracle and through oracle/py_model.py — outputs and
    verdicts, honest and edited.  The reference decides: z1 = x' + x e over the integers and z2 = r' r^e mod n^2 for ANY x, r
    (correct_ciphertext.rs:59-60; zero_enc_proof.rs:59-60); the verifier reduces nothing it reads except through Paillier's own
    arithmetic modulo n^2 and hashes n, c, c' as they are (correct_ciphertext.rs:67-96; zero_enc_proof.rs:67-93)."""
    cs, z, aa, vh, ed, over, ve = _zero_edges(oracle, 1024)
    bt, a = cs["bt"], cs["a"]
    SC.check_edge_verdicts(cs, vh, over, ve, rejected=cs["ragged_statements"])
    for b, n in enumerate(bt.ns):
        assert (SC.get_int(z, b), SC.get_int(aa, b)) == pm.zero_proof_prove(n, SC.get_int(a["c0"], b), SC.get_int(a["r"], b), SC.get_int(a["rp"], b)), b
        assert pm.zero_proof_verify(n, SC.get_int(ed["c"], b), SC.get_int(ed["z"], b), SC.get_int(ed["a"], b)) == (ve[b] == SC.ACCEPT), b
    b = cs["short"]["zero"]
    assert pm.compute_digest([bt.ns[b], SC.get_int(a["c0"], b), SC.get_int(aa, b)]) >> 248 == 0
    cs, z1, z2, cp, vh, ed, over, ve = _ciphertext_edges(oracle, 1024)
    SC.check_edge_verdicts(cs, vh, over, ve, rejected=cs["ragged_statements"])
    for b, n in enumerate(bt.ns):
        want = pm.ciphertext_proof_prove(n, SC.get_int(a["cx"], b), SC.get_int(a["x"], b), SC.get_int(a["r"], b), SC.get_int(a["xp"], b), SC.get_int(a["rp"], b))
        assert (SC.get_int(z1, b), SC.get_int(z2, b), SC.get_int(cp, b)) == want, b
        assert pm.ciphertext_proof_verify(n, SC.get_int(ed["c"], b), SC.get_int(ed["z1"], b), SC.get_int(ed["z2"], b), SC.get_int(ed["cp"], b)) == (ve[b] == SC.ACCEPT), b
    b = cs["short"]["ciphertext"]
    assert pm.compute_digest([bt.ns[b], SC.get_int(a["cx"], b), SC.get_int(cp, b)]) >> 248 == 0
    assert SC.get_int(z1, 9) >> (1024 + 248) != 0          # x = x' = 2^n_bits - 1: the maximal honest z1 reaches the extra limbs


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_gpu_zero_proof_operand_edges(ctx, oracle, n_bits):
    """r, r' in {1, n - 1, 2^n_bits - 1}; z >= n^2, all ones, 0; c and a >= n^2, 0, 1 and of ragged byte length; a short challenge"""
    cs, zo, ao, vh, ed, over, ve = _zero_edges(oracle, n_bits)
    bt, a = cs["bt"], cs["a"]
    SC.check_edge_verdicts(cs, vh, over, ve, rejected=cs["ragged_statements"])
    zg, ag = SC.sentinel(zo.shape), SC.sentinel(ao.shape)
    ctx.zero_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["c0"], a["r"], a["rp"], zg, ag)
    SC.assert_same(ao, ag, "a")
    SC.assert_same(zo, zg, "z")
    if n_bits == 1024:
        b = cs["short"]["zero"]
        assert pm.compute_digest([bt.ns[b], SC.get_int(a["c0"], b), SC.get_int(ag, b)]) >> 248 == 0
    for c, z, aa, want in ((a["c0"], zg, ag, vh), (ed["c"], ed["z"], ed["a"], ve)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.zero_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, c, z, aa, vg)
        SC.assert_same(want, vg, "verdict")


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_gpu_ciphertext_proof_operand_edges(ctx, oracle, n_bits):
    """x, x' in {0, 1, n - 1, 2^n_bits - 1} (both at the top: the maximal honest z1); z1 with all kw + 16 limbs set, z1 + k n (accepted);
    z2 >= n^2, all ones, 0; c and c' >= n^2, 0, 1 and of ragged byte length; a short challenge"""
    cs, z1o, z2o, cpo, vh, ed, over, ve = _ciphertext_edges(oracle, n_bits)
    bt, a = cs["bt"], cs["a"]
    SC.check_edge_verdicts(cs, vh, over, ve, rejected=cs["ragged_statements"])
    z1g, z2g, cpg = SC.sentinel(z1o.shape), SC.sentinel(z2o.shape), SC.sentinel(cpo.shape)
    ctx.ciphertext_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["cx"], a["x"], a["r"], a["xp"], a["rp"], z1g, z2g, cpg)
    for name, x, y in (("c_prime", cpo, cpg), ("z1", z1o, z1g), ("z2", z2o, z2g)):
        SC.assert_same(x, y, name)
    if n_bits == 1024:
        b = cs["short"]["ciphertext"]
        assert pm.compute_digest([bt.ns[b], SC.get_int(a["cx"], b), SC.get_int(cpg, b)]) >> 248 == 0
    for c, z1, z2, cp, want in ((a["cx"], z1g, z2g, cpg, vh), (ed["c"], ed["z1"], ed["z2"], ed["cp"], ve)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.ciphertext_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, c, z1, z2, cp, vg)
        SC.assert_same(want, vg, "verdict")
