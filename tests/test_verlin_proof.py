"""VerlinProof (verlin_proof.rs:35-165): oracle vs python model (CPU); HIP engine vs oracle (GPU)."""
import numpy as np
import pytest

import helpers as H
import small_proof_cases as SC
from helpers import pm, L, zkp


def make(n_bits, keys, B, seed, bad_last=True, oracle=None):
    """B statements with witness and nonces.  The statements (c, c', phi_x) are computed by the Python model, or — `oracle` given: the GPU
    tests at 4096 bits, where one Enc takes CPython 0.7 s and gen_phi three times that — by the C oracle from the same inputs"""
    d = pm.Drbg(seed)
    kw = n_bits // 32
    enc = (lambda n, m, r: (m, r)) if oracle else pm.enc
    rows = []
    for b in range(B):
        n = keys[b % len(keys)]
        c, cp = enc(n, d.below(n), d.below(n)), enc(n, d.below(n), d.below(n))             # the two public ciphertexts (verlin_proof.rs tests)
        x, xp, xpp, rx = d.below(n), d.below(n), d.below(n), d.below(n)
        rows.append(dict(n=n, c=c, cp=cp, phi_x=0, x=x, xp=xp, xpp=xpp, rx=rx, a=d.below(n), ap=d.below(n), app=d.below(n), ra=d.below(n)))
    if oracle:
        ns = L.ints_to_limbs([q["n"] for q in rows], kw)
        wit = tuple(L.ints_to_limbs([q[k] for q in rows], kw) for k in ("x", "xp", "xpp", "rx"))
        cs = [oracle.paillier_enc(n_bits, ns, kw, *(L.ints_to_limbs([q[k][i] for q in rows], kw) for i in (0, 1))) for k in ("c", "cp")]
        # phi_x = gen_phi(c, c', x, x', x'', r_x): what the oracle's prover computes of its nonces (verlin_proof.rs:138-165)
        phi = oracle.verlin_proof_prove(n_bits, ns, kw, cs[0], cs[1], np.zeros_like(cs[0]), wit, wit)[0]
        for b, q in enumerate(rows):
            q.update(c=L.limbs_to_int(cs[0][b]), cp=L.limbs_to_int(cs[1][b]), phi_x=L.limbs_to_int(phi[b]))
    for b, q in enumerate(rows):
        if not oracle:
            q["phi_x"] = pm.gen_phi(q["n"], q["c"], q["cp"], q["x"], q["xp"], q["xpp"], q["rx"])
        if bad_last and b == B - 1:
            q["phi_x"] = (q["phi_x"] * 2) % (q["n"] * q["n"])                               # statement no longer matches the witness
    arr = lambda k, w: L.ints_to_limbs([q[k] for q in rows], w)
    a = {k: arr(k, 2 * kw if k in ("c", "cp", "phi_x") else kw) for k in rows[0]}
    return rows, a


def test_oracle_matches_python_model(oracle):
    n_bits, kw = 1024, 32
    keys = [H.test_key(1024, tag=t)[2] for t in range(2)]
    rows, a = make(n_bits, keys, 3, b"verlin-cpu")
    phi_a, z, zp, zpp, rz = oracle.verlin_proof_prove(n_bits, a["n"], kw, a["c"], a["cp"], a["phi_x"], (a["x"], a["xp"], a["xpp"], a["rx"]), (a["a"], a["ap"], a["app"], a["ra"]))
    for b, q in enumerate(rows):
        exp = pm.verlin_prove(q["n"], q["c"], q["cp"], q["phi_x"], q["x"], q["xp"], q["xpp"], q["rx"], q["a"], q["ap"], q["app"], q["ra"])
        got = tuple(L.limbs_to_int(v[b]) for v in (phi_a, z, zp, zpp, rz))
        assert got == exp
        assert pm.verlin_verify(q["n"], q["c"], q["cp"], q["phi_x"], *got) == (b != 2)
    assert list(oracle.verlin_proof_verify(n_bits, a["n"], kw, a["c"], a["cp"], a["phi_x"], phi_a, z, zp, zpp, rz)) == [1, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits,shared", [(1024, False), (2048, True), (4096, True)])
def test_gpu_verlin_matches_oracle(ctx, oracle, n_bits, shared):
    """(4096: the benchmark's key — 8192-bit n^2, the widest kernel geometry under the composition)"""
    kw = n_bits // 32
    B = 4
    oracle.set_threads(min(8, oracle.max_threads()))
    if n_bits == 4096:
        rows, a = SC.cached("verlin-gpu-4096", lambda: make(n_bits, [SC.keys_for(4096, 1)[0][2]], B, b"verlin-gpu-%d" % n_bits, oracle=oracle))
    else:
        keys = [H.fixture_key()[2]] if n_bits == 2048 else [H.test_key(1024, tag=t)[2] for t in range(3)]
        rows, a = make(n_bits, keys, B, b"verlin-gpu-%d" % n_bits)
    n_arr = a["n"][:1] if shared else a["n"]
    stride = 0 if shared else kw
    wit, non = (a["x"], a["xp"], a["xpp"], a["rx"]), (a["a"], a["ap"], a["app"], a["ra"])
    o = oracle.verlin_proof_prove(n_bits, n_arr, stride, a["c"], a["cp"], a["phi_x"], wit, non)
    g = tuple(np.zeros_like(v) for v in o)
    ctx.verlin_proof_prove(n_bits, B, n_arr, stride, a["c"], a["cp"], a["phi_x"], wit, non, g)
    for vo, vg in zip(o, g):
        assert np.array_equal(vo, vg)
    zt = g[1].copy(); zt[0, 0] ^= 1                       # tamper z of proof 0
    vo = oracle.verlin_proof_verify(n_bits, n_arr, stride, a["c"], a["cp"], a["phi_x"], g[0], zt, g[2], g[3], g[4])
    vg = np.full(B, 9, np.uint8)
    ctx.verlin_proof_verify(n_bits, B, n_arr, stride, a["c"], a["cp"], a["phi_x"], g[0], zt, g[2], g[3], g[4], vg)
    assert np.array_equal(vo, vg) and list(vo) == [0, 1, 1, 0]


# ================================================================== wide batch and operand edges (tests/small_proof_cases.py)
def _io(cs):
    a = cs["a"]
    return tuple(a[k] for k in SC.VERLIN_WIT), tuple(a[k] for k in SC.VERLIN_NON)


def _verlin_wide(oracle):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.verlin_wide(oracle)
        bt, a = cs["bt"], cs["a"]
        wit, non = _io(cs)
        o = oracle.verlin_proof_prove(*bt.key(), a["c"], a["cp"], a["phi_x"], wit, non)
        third = -(-len(cs["tamper"]) // 3)
        t = list(o)                                     # z, z', z'' tampered in different proofs
        for k in range(3):
            t[1 + k] = SC.flip(o[1 + k], cs["tamper"][k * third:(k + 1) * third], salt=k)
        vh = oracle.verlin_proof_verify(*bt.key(), a["c"], a["cp"], a["phi_x"], *o)
        vt = oracle.verlin_proof_verify(*bt.key(), a["c"], a["cp"], a["phi_x"], *t)
        return cs, o, vh, tuple(t), vt
    return SC.cached("verlin-wide", build)


def test_wide_verlin_case_is_what_it_claims(oracle):
    """CPU: the oracle rejects the 300-proof batch exactly at the false statements, and at the tampered responses as well"""
    cs, o, vh, t, vt = _verlin_wide(oracle)
    SC.check_wide_verdicts(cs, vh, vt)


@pytest.mark.gpu
def test_gpu_verlin_wide_batch(ctx, oracle):
    """300 VerlinProofs under one 1024-bit key: a second, partial 256-thread block in k_verlin_hash / k_words_compare; a GROUPS_PER_BLOCK
    tail in modexp_core (kw- and (kw + 16)-word per-item exponents), k_enc with m_words / r_words set, and k_modmul"""
    cs, o, vh, t, vt = _verlin_wide(oracle)
    bt, a = cs["bt"], cs["a"]
    assert bt.B > 256
    SC.check_wide_verdicts(cs, vh, vt)
    wit, non = _io(cs)
    g = tuple(SC.sentinel(v.shape) for v in o)
    ctx.verlin_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["c"], a["cp"], a["phi_x"], wit, non, g)
    for name, vo, vg in zip(SC.VERLIN_OUT, o, g):
        SC.assert_same(vo, vg, name)
    for proof, want in ((g, vh), (t, vt)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.verlin_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["c"], a["cp"], a["phi_x"], *proof, vg)
        SC.assert_same(want, vg, "verdict")


def _verlin_edges(oracle, n_bits):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.verlin_edges(oracle, n_bits)
        bt, a = cs["bt"], cs["a"]
        wit, non = _io(cs)
        o = oracle.verlin_proof_prove(*bt.key(), a["c"], a["cp"], a["phi_x"], wit, non)
        vh = oracle.verlin_proof_verify(*bt.key(), a["c"], a["cp"], a["phi_x"], *o)
        ed, over = SC.verlin_edits(cs, o)
        ve = oracle.verlin_proof_verify(*bt.key(), ed["c"], ed["cp"], ed["phi_x"], *[ed[k] for k in SC.VERLIN_OUT])
        return cs, o, vh, ed, over, ve
    return SC.cached("verlin-edges-%d" % n_bits, build)


def test_verlin_edge_cases_oracle_matches_python_model(oracle):
    """CPU: the operand edges of tests/small_proof_cases.py (n = 1024) through the C oracle and through oracle/py_model.py.  The reference
    decides: z = x e + a over the integers for any x and a, r_z = r_x^e r_a mod n^2 (verlin_proof.rs:85-89); gen_phi raises c and c' to the
    responses as they are and encrypts z'' under r_z (:138-165), so z'' + k n and r_z + n^2 give the same phi_z while z + k n does not;
    the challenge hashes n, c, c', phi_x, phi_a as they are (:102-108)."""
    cs, o, vh, ed, over, ve = _verlin_edges(oracle, 1024)
    bt, a = cs["bt"], cs["a"]
    SC.check_edge_verdicts(cs, vh, over, ve)
    for b, n in enumerate(bt.ns):
        st = [SC.get_int(a[k], b) for k in ("c", "cp", "phi_x")]
        assert tuple(SC.get_int(v, b) for v in o) == pm.verlin_prove(n, *st, *[SC.get_int(a[k], b) for k in SC.VERLIN_WIT + SC.VERLIN_NON]), b
        got = pm.verlin_verify(n, *[SC.get_int(ed[k], b) for k in ("c", "cp", "phi_x") + SC.VERLIN_OUT])
        assert got == (ve[b] == SC.ACCEPT), b
    b = cs["short"]["verlin"]
    assert pm.compute_digest([bt.ns[b]] + [SC.get_int(a[k], b) for k in ("c", "cp", "phi_x")] + [SC.get_int(o[0], b)]) >> 248 == 0
    assert all(SC.get_int(o[k], 9) >> (1024 + 248) != 0 for k in (1, 2, 3))      # witness and nonces at 2^n_bits - 1: the maximal honest responses


def test_verlin_edge_cases_at_4096_bits_oracle_matches_python_model(oracle):
    """CPU: the 4096-bit edge batch (per-proof keys: the benchmark's key and two products of pooled primes) is what it claims — honest
    proofs accepted, the over-wide z'' and r_z accepted, ACCEPT and REJECT both among the edited proofs — and the C oracle agrees with
    oracle/py_model.py on three of its items, proving and verifying: witness and nonces with every limb set, witness and nonces at n - 1,
    and an ordinary proof, which in the edited batch carries the z with all kw + 16 limbs set.  (Three items: one Enc takes CPython 0.7 s
    at this width; the whole batch is compared at 1024 bits above.)"""
    cs, o, vh, ed, over, ve = _verlin_edges(oracle, 4096)
    bt, a = cs["bt"], cs["a"]
    assert bt.n_bits == 4096 and not bt.shared and len(set(bt.ns)) == 3
    SC.check_edge_verdicts(cs, vh, over, ve)
    b_all, b_n1, b_ord = cs["all_set"], cs["n_minus_1"], cs["free"][0]
    assert all(SC.get_int(a[k], b_all) == bt.top for k in SC.VERLIN_WIT + SC.VERLIN_NON)
    assert all(SC.get_int(a[k], b_n1) == bt.ns[b_n1] - 1 for k in ("x", "xp", "xpp", "a", "ap", "app"))
    assert SC.get_int(ed["z"], b_ord) == SC.ones(bt.kw + SC.EXTRA) and ve[b_ord] == SC.REJECT
    for b in (b_all, b_n1, b_ord):
        n = bt.ns[b]
        st = [SC.get_int(a[k], b) for k in ("c", "cp", "phi_x")]
        assert tuple(SC.get_int(v, b) for v in o) == pm.verlin_prove(n, *st, *[SC.get_int(a[k], b) for k in SC.VERLIN_WIT + SC.VERLIN_NON]), b
        got = pm.verlin_verify(n, *[SC.get_int(ed[k], b) for k in ("c", "cp", "phi_x") + SC.VERLIN_OUT])
        assert got == (ve[b] == SC.ACCEPT), b
    assert all(SC.get_int(o[k], b_all) >> (4096 + 248) != 0 for k in (1, 2, 3))      # the maximal honest responses reach the extra limbs


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_gpu_verlin_operand_edges(ctx, oracle, n_bits):
    """witness and nonces in {0, 1, n - 1, 2^n_bits - 1}; z, z', z'' with all kw + 16 limbs set and k n higher (z'': accepted);
    r_z >= n^2, all ones, 0; c, c', phi_x, phi_a >= n^2, 0, 1, of ragged byte length; a short challenge"""
    cs, o, vh, ed, over, ve = _verlin_edges(oracle, n_bits)
    bt, a = cs["bt"], cs["a"]
    SC.check_edge_verdicts(cs, vh, over, ve)
    wit, non = _io(cs)
    g = tuple(SC.sentinel(v.shape) for v in o)
    ctx.verlin_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["c"], a["cp"], a["phi_x"], wit, non, g)
    for name, vo, vg in zip(SC.VERLIN_OUT, o, g):
        SC.assert_same(vo, vg, name)
    if n_bits == 1024:
        b = cs["short"]["verlin"]
        assert pm.compute_digest([bt.ns[b]] + [SC.get_int(a[k], b) for k in ("c", "cp", "phi_x")] + [SC.get_int(g[0], b)]) >> 248 == 0
    for st, proof, want in ((a, g, vh), (ed, [ed[k] for k in SC.VERLIN_OUT], ve)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.verlin_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, st["c"], st["cp"], st["phi_x"], *proof, vg)
        SC.assert_same(want, vg, "verdict")
