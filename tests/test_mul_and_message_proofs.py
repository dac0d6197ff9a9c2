"""mod_inv, MulProof (multiplication_proof.rs) and CorrectMessageProof (correct_message.rs) — SURVEY §8(f) rank 4.
CPU: the C oracle against the pure-Python model (and the reference's own accept / reject behaviours,
multiplication_proof.rs:172-290, correct_message.rs:169-200).  GPU: the HIP engine against the oracle, byte-exact."""
import math

import numpy as np
import pytest

import helpers as H
import small_proof_cases as SC
from helpers import pm, L, zkp

ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED


# ------------------------------------------------------------------ mod_inv
def inv_cases(mod, kw, seed, count):
    d = pm.Drbg(seed)
    vals = [0, 1, 2, mod - 1, mod - 2, (mod + 1) // 2, 1 << 31, 1 << 32, (1 << 64) - 1, 1 << (mod.bit_length() - 1)]
    # a == M modulo 2^32 / 2^64 / 2^96: the first difference has whole zero low words (the unfused path of k_modinv)
    vals += [mod - (3 << 32), mod - (5 << 64), mod - (7 << 96), mod - (d.below(1 << 200) << 64)]
    vals += [d.below(mod) for _ in range(count - len(vals))]
    # a = M - r for small even r: the values whose cofactor can end below -M (tests/modinv_class_cases.py has vectors that do); on top of `count`
    vals += [mod - r for r in (14, 30, 42, 46, 62) if math.gcd(mod - r, mod) == 1]
    return vals


def check_inverse(vals, mod, out, st):
    for i, a in enumerate(vals):
        inv = pm.mod_inv(a, mod) if a < mod and mod % 2 == 1 and mod >= 3 else None
        if a >= mod or mod % 2 == 0 or mod < 3:
            assert st[i] == zkp.INV_DOMAIN, i
        elif inv is None:
            assert st[i] == zkp.INV_NONE, i
        else:
            assert st[i] == zkp.INV_OK and L.limbs_to_int(out[i]) == inv, i
        if st[i] != zkp.INV_OK:
            assert not out[i].any()


def test_oracle_modinv(oracle):
    p_, q_, n = H.test_key(512)
    nn = n * n
    kw = 64
    vals = inv_cases(nn, kw, b"inv-cpu", 40) + [p_, q_ * 7, n, n * p_, nn + 5 if (nn + 5).bit_length() <= 2048 else 3]
    a = L.ints_to_limbs(vals, kw)
    out, st = oracle.modinv(2048, a, L.int_to_limbs(nn, kw)[None, :], 0)
    check_inverse(vals, nn, out, st)
    assert st[vals.index(p_)] == zkp.INV_NONE and st[0] == zkp.INV_NONE
    # per-item moduli, one of them even
    mods = [nn, nn - 1, 3 * 5 * 7, 3]
    vals2 = [5, 5, 10, 2]
    out, st = oracle.modinv(2048, L.ints_to_limbs(vals2, kw), L.ints_to_limbs(mods, kw), kw)
    assert list(st) == [zkp.INV_OK, zkp.INV_DOMAIN, zkp.INV_NONE, zkp.INV_OK]
    assert L.limbs_to_int(out[3]) == 2


# ------------------------------------------------------------------ MulProof
MUL_IN = ("e_a", "e_b", "e_c", "a", "b", "r_a", "r_b", "r_c", "d", "r_d")


def mul_cases(n_bits, keys, B, seed, honest=True, oracle=None):
    """the three ciphertexts of a row are computed by the Python model, or — `oracle` given: the GPU tests at 4096 bits, where one Enc
    takes CPython 0.7 s — by the C oracle from the same inputs"""
    d = pm.Drbg(seed)
    kw = n_bits // 32
    rows = []
    for i in range(B):
        n = keys[i % len(keys)]
        a, b = d.below(n), d.below(n)
        c = a * b % n if honest else (a * b + 1) % n
        r_a, r_b, r_c, dd, r_d = (d.below(n) for _ in range(5))
        rows.append(dict(n=n, a=a, b=b, c=c, r_a=r_a, r_b=r_b, r_c=r_c, d=dd, r_d=r_d))
    ns = L.ints_to_limbs([q["n"] for q in rows], kw)
    for m, r in (("a", "r_a"), ("b", "r_b"), ("c", "r_c")):
        if oracle:
            e = L.limbs_to_ints(oracle.paillier_enc(n_bits, ns, kw, L.ints_to_limbs([q[m] for q in rows], kw), L.ints_to_limbs([q[r] for q in rows], kw)))
        else:
            e = [pm.enc(q["n"], q[m], q[r]) for q in rows]
        for q, v in zip(rows, e):
            q["e_" + m] = v
    arr = {k: L.ints_to_limbs([q[k] for q in rows], 2 * kw if k.startswith("e_") else kw) for k in ("n",) + MUL_IN}
    return rows, arr


def test_oracle_mul_proof_matches_python_model(oracle):
    n_bits, kw = 1024, 32
    keys = [H.test_key(1024, tag=t)[2] for t in range(2)]
    rows, a = mul_cases(n_bits, keys, 4, b"mul-cpu")
    f, z1, z2, e_d, e_db, st = oracle.mul_proof_prove(n_bits, a["n"], kw, *[a[k] for k in MUL_IN])
    assert list(st) == [0] * 4
    for i, q in enumerate(rows):
        exp = pm.mul_proof_prove(q["n"], q["e_a"], q["e_b"], q["e_c"], q["a"], q["b"], q["r_a"], q["r_b"], q["r_c"], q["d"], q["r_d"])
        got = tuple(L.limbs_to_int(x[i]) for x in (f, z1, z2, e_d, e_db))
        assert got == exp
        assert pm.mul_proof_verify(q["n"], q["e_a"], q["e_b"], q["e_c"], *got)
    assert list(oracle.mul_proof_verify(n_bits, a["n"], kw, a["e_a"], a["e_b"], a["e_c"], f, z1, z2, e_d, e_db)) == [1] * 4   # test_mul_proof :172-229
    # test_bad_mul_proof (:232-290): c = a*b + 1
    rows, a = mul_cases(n_bits, keys, 3, b"mul-bad", honest=False)
    f, z1, z2, e_d, e_db, st = oracle.mul_proof_prove(n_bits, a["n"], kw, *[a[k] for k in MUL_IN])
    assert list(oracle.mul_proof_verify(n_bits, a["n"], kw, a["e_a"], a["e_b"], a["e_c"], f, z1, z2, e_d, e_db)) == [0] * 3
    # r_c sharing a factor with n: mod_inv(...).unwrap() panics in prove (:95)
    p_, q_, n = H.test_key(1024, tag=0)
    rows, a = mul_cases(n_bits, [n], 2, b"mul-panic")
    a["r_c"][1] = L.int_to_limbs(p_, kw)
    f, z1, z2, e_d, e_db, st = oracle.mul_proof_prove(n_bits, a["n"], kw, *[a[k] for k in MUL_IN])
    assert list(st) == [0, MALFORMED]
    with pytest.raises(pm.Panic):
        q = rows[1]
        pm.mul_proof_prove(q["n"], q["e_a"], q["e_b"], q["e_c"], q["a"], q["b"], q["r_a"], q["r_b"], p_, q["d"], q["r_d"])
    # e_db = a multiple of p: the verifier's mod_inv(...).unwrap() panics (:135)
    e_db2 = e_db.copy(); e_db2[0] = L.int_to_limbs(p_ * 12345, 2 * kw)
    assert list(oracle.mul_proof_verify(n_bits, a["n"], kw, a["e_a"], a["e_b"], a["e_c"], f, z1, z2, e_d, e_db2))[0] == MALFORMED


# ------------------------------------------------------------------ CorrectMessageProof
def cm_cases(n_bits, keys, B, K, seed, pick=None):
    d = pm.Drbg(seed)
    kw = n_bits // 32
    rows = []
    for i in range(B):
        n = keys[i % len(keys)]
        valid = [d.below(1 << 64) + 3 for _ in range(K)]
        idx = (i % K) if pick is None else pick
        msg = valid[idx] if idx is not None and idx >= 0 else valid[0] + 1
        rows.append(dict(n=n, valid=valid, msg=msg, r=d.below(n), w=d.below(n), e_sim=[d.bits(256) for _ in range(K - 1)],
                         z_sim=[d.below(n) for _ in range(K - 1)]))
    arr = dict(n=L.ints_to_limbs([q["n"] for q in rows], kw),
               valid=np.stack([L.ints_to_limbs(q["valid"], kw) for q in rows]),
               msg=L.ints_to_limbs([q["msg"] for q in rows], kw), r=L.ints_to_limbs([q["r"] for q in rows], kw),
               w=L.ints_to_limbs([q["w"] for q in rows], kw),
               e_sim=np.stack([L.ints_to_limbs(q["e_sim"], 8) if K > 1 else np.zeros((0, 8), np.uint32) for q in rows]),
               z_sim=np.stack([L.ints_to_limbs(q["z_sim"], kw) if K > 1 else np.zeros((0, kw), np.uint32) for q in rows]))
    return rows, arr


@pytest.mark.parametrize("K", [1, 3])
def test_oracle_correct_message_matches_python_model(oracle, K):
    n_bits, kw = 1024, 32
    keys = [H.test_key(1024, tag=t)[2] for t in range(2)]
    B = 4
    rows, a = cm_cases(n_bits, keys, B, K, b"cm-cpu-%d" % K)
    ct, e_vec, z_vec, a_vec, st = oracle.correct_message_prove(n_bits, K, a["n"], kw, a["valid"], a["msg"], a["r"], a["e_sim"], a["z_sim"], a["w"])
    assert list(st) == [0] * B
    for b, q in enumerate(rows):
        exp = pm.correct_message_prove(q["n"], q["valid"], q["msg"], q["r"], q["e_sim"], q["z_sim"], q["w"])
        assert L.limbs_to_int(ct[b]) == exp[0]
        assert [L.limbs_to_int(x) for x in e_vec[b]] == exp[1]
        assert [L.limbs_to_int(x) for x in z_vec[b]] == exp[2]
        assert [L.limbs_to_int(x) for x in a_vec[b]] == exp[3]
        assert pm.correct_message_verify(q["n"], q["valid"], *exp)
    v = oracle.correct_message_verify(n_bits, K, a["n"], kw, a["valid"], ct, e_vec, z_vec, a_vec)
    assert list(v) == [1] * B                                        # test_correct_message_zk_proof :169-181
    # a tampered z: rejected; a tampered e: the assert_eq! panics
    z2 = z_vec.copy(); z2[0, 0, 0] ^= 1
    e2 = e_vec.copy(); e2[1, 0, 0] ^= 1
    assert oracle.correct_message_verify(n_bits, K, a["n"], kw, a["valid"], ct, e_vec, z2, a_vec)[0] == 0
    assert oracle.correct_message_verify(n_bits, K, a["n"], kw, a["valid"], ct, e2, z_vec, a_vec)[1] == MALFORMED


def test_oracle_correct_message_wrong_message(oracle):
    """test_incorrect_message_zk_proof (correct_message.rs:184-200, #[should_panic]): the encrypted message is not in the list"""
    n_bits, kw, K = 1024, 32, 3
    keys = [H.test_key(1024)[2]]
    rows, a = cm_cases(n_bits, keys, 2, K, b"cm-bad", pick=-1)
    ct, e_vec, z_vec, a_vec, st = oracle.correct_message_prove(n_bits, K, a["n"][:1], 0, a["valid"], a["msg"], a["r"], a["e_sim"], a["z_sim"], a["w"])
    assert list(st) == [MALFORMED] * 2
    with pytest.raises(pm.Panic):
        q = rows[0]
        pm.correct_message_prove(q["n"], q["valid"], q["msg"], q["r"], q["e_sim"], q["z_sim"], q["w"])


# ================================================================== GPU parity
@pytest.mark.gpu
@pytest.mark.parametrize("mod_bits", [2048, 4096, 8192])
def test_gpu_modinv_matches_oracle(ctx, oracle, mod_bits):
    kw = mod_bits // 32
    p_, q_, n = H.test_key(mod_bits // 2)
    nn = n * n
    vals = inv_cases(nn, kw, b"inv-gpu-%d" % mod_bits, 150) + [p_, q_ * 7, n, n * p_, p_ * p_, nn - n]
    # values that stress the word-level paths: long runs of trailing zeros (whole zero words), tiny values
    vals += [1 << 32, 1 << 64, 3 << 96, (d_ := pm.Drbg(b"z")).below(nn) >> 70 << 70, 5, nn - (1 << 40)]
    a = L.ints_to_limbs(vals, kw)
    m = L.int_to_limbs(nn, kw)[None, :]
    oo, so = oracle.modinv(mod_bits, a, m, 0)
    og = np.full_like(a, 0xA5A5A5A5); sg = np.full(len(vals), 9, np.uint8)
    ctx.modinv(mod_bits, len(vals), a, m, 0, og, sg)
    assert np.array_equal(so, sg) and np.array_equal(oo, og)
    check_inverse(vals, nn, og, sg)
    # per-item moduli, including an even one and a = modulus
    mods = [nn, nn - 1, 3 * 5 * 7, 3, n * 3, (1 << (mod_bits - 1)) + 1]
    vals2 = [5, 5, 10, 2, p_, 12345]
    a2 = L.ints_to_limbs(vals2, kw); m2 = L.ints_to_limbs(mods, kw)
    oo, so = oracle.modinv(mod_bits, a2, m2, kw)
    og = np.zeros_like(a2); sg = np.full(len(vals2), 9, np.uint8)
    ctx.modinv(mod_bits, len(vals2), a2, m2, kw, og, sg)
    assert np.array_equal(so, sg) and np.array_equal(oo, og)


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits,shared", [(1024, False), (2048, True), (4096, True)])
def test_gpu_mul_proof_matches_oracle(ctx, oracle, n_bits, shared):
    """(4096: the benchmark's key — 8192-bit n^2, the widest kernel geometry under the composition)"""
    kw = n_bits // 32
    if n_bits == 2048:
        pq = [H.fixture_key()]
    elif n_bits == 4096:
        pq = SC.keys_for(4096, 1)
    else:
        pq = [H.test_key(n_bits, tag=t) for t in range(1 if shared else 3)]
    keys = [k[2] for k in pq]
    B = 6
    oracle.set_threads(min(8, oracle.max_threads()))
    by = oracle if n_bits == 4096 else None
    rows, a = mul_cases(n_bits, keys, B, b"mul-gpu-%d" % n_bits, oracle=by)
    bad_rows, bad = mul_cases(n_bits, keys, B, b"mul-gpu-bad-%d" % n_bits, honest=False, oracle=by)
    for k in MUL_IN:                      # proofs 4 and 5 are about a false statement (test_bad_mul_proof)
        a[k][4:] = bad[k][4:]
    a["r_c"][3] = L.int_to_limbs(pq[3 % len(pq)][0], kw)   # r_c = p: the prover's mod_inv has no result
    n_arr = a["n"][:1] if shared else a["n"]
    stride = 0 if shared else kw
    ins = [a[k] for k in MUL_IN]
    fo, z1o, z2o, edo, edbo, so = oracle.mul_proof_prove(n_bits, n_arr, stride, *ins)
    fg = np.full((B, kw), 7, np.uint32); z1g, z2g, edg, edbg = (np.full((B, 2 * kw), 7, np.uint32) for _ in range(4)); sg = np.full(B, 9, np.uint8)
    ctx.mul_proof_prove(n_bits, B, n_arr, stride, *ins, fg, z1g, z2g, edg, edbg, sg)
    if n_bits == 4096:
        assert ctx.last_geometry() == ctx.test_geometry, "the call ran on another engine than the one this family pins"
    assert list(so) == [0, 0, 0, MALFORMED, 0, 0] and np.array_equal(so, sg)
    for name, x, y in (("f", fo, fg), ("z1", z1o, z1g), ("z2", z2o, z2g), ("e_d", edo, edg), ("e_db", edbo, edbg)):
        assert np.array_equal(x, y), name
    # verify: honest, panicked-in-prove (zeros), false statement; then tampered copies
    def both(f, z1, z2, e_d, e_db):
        vo = oracle.mul_proof_verify(n_bits, n_arr, stride, a["e_a"], a["e_b"], a["e_c"], f, z1, z2, e_d, e_db)
        vg = np.full(B, 9, np.uint8)
        ctx.mul_proof_verify(n_bits, B, n_arr, stride, a["e_a"], a["e_b"], a["e_c"], f, z1, z2, e_d, e_db, vg)
        assert n_bits != 4096 or ctx.last_geometry() == ctx.test_geometry
        assert np.array_equal(vo, vg), (vo, vg)
        return list(vo)
    assert both(fo, z1o, z2o, edo, edbo) == [1, 1, 1, 0, 0, 0]
    f2 = fo.copy(); f2[0, 0] ^= 1
    z12 = z1o.copy(); z12[1, 5] ^= 4
    z22 = z2o.copy(); z22[2, kw] ^= 1
    assert both(f2, z12, z22, edo, edbo) == [0, 0, 0, 0, 0, 0]
    # e_db sharing a factor with n: the verifier's unwrap panics; e_d out of range (>= n^2): hashed as is, used modulo n^2
    edb2 = edbo.copy(); edb2[0] = L.int_to_limbs(pq[0][0] * 98765, 2 * kw)
    ed2 = edo.copy(); ed2[1] = L.int_to_limbs(L.limbs_to_int(edo[1]) + keys[1 % len(keys)] ** 2, 2 * kw) if n_bits == 1024 else edo[1]
    v = both(fo, z1o, z2o, ed2, edb2)
    assert v[0] == MALFORMED


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits,shared,K", [(1024, False, 3), (2048, True, 2), (1024, True, 1), (4096, True, 2)])
def test_gpu_correct_message_matches_oracle(ctx, oracle, n_bits, shared, K):
    kw = n_bits // 32
    if n_bits == 2048:
        pq = [H.fixture_key()]
    elif n_bits == 4096:
        pq = SC.keys_for(4096, 1)                  # the benchmark's key
    else:
        pq = [H.test_key(n_bits, tag=t) for t in range(1 if shared else 3)]
    keys = [k[2] for k in pq]
    B = 5
    oracle.set_threads(min(8, oracle.max_threads()))
    rows, a = cm_cases(n_bits, keys, B, K, b"cm-gpu-%d-%d" % (n_bits, K))
    # proof 3: the message is not in the list (the reference panics); proof 4: r = p, so u^e has no inverse
    a["msg"][3] = L.int_to_limbs(rows[3]["valid"][0] + 1, kw)
    a["r"][4] = L.int_to_limbs(pq[4 % len(pq)][0], kw)
    n_arr = a["n"][:1] if shared else a["n"]
    stride = 0 if shared else kw
    cto, evo, zvo, avo, so = oracle.correct_message_prove(n_bits, K, n_arr, stride, a["valid"], a["msg"], a["r"], a["e_sim"], a["z_sim"], a["w"])
    ctg = np.full((B, 2 * kw), 7, np.uint32); evg = np.full((B, K, 8), 7, np.uint32); zvg = np.full((B, K, kw), 7, np.uint32)
    avg = np.full((B, K, 2 * kw), 7, np.uint32); sg = np.full(B, 9, np.uint8)
    ctx.correct_message_prove(n_bits, B, K, n_arr, stride, a["valid"], a["msg"], a["r"], a["e_sim"], a["z_sim"], a["w"], ctg, evg, zvg, avg, sg)
    assert np.array_equal(so, sg), (so, sg)
    assert list(so[:4]) == [0, 0, 0, MALFORMED] and (so[4] == MALFORMED) == (K > 1)
    for name, x, y in (("ciphertext", cto, ctg), ("e_vec", evo, evg), ("z_vec", zvo, zvg), ("a_vec", avo, avg)):
        assert np.array_equal(x, y), name

    def both(ct, ev, zv, av):
        vo = oracle.correct_message_verify(n_bits, K, n_arr, stride, a["valid"], ct, ev, zv, av)
        vg = np.full(B, 9, np.uint8)
        ctx.correct_message_verify(n_bits, B, K, n_arr, stride, a["valid"], ct, ev, zv, av, vg)
        assert np.array_equal(vo, vg), (vo, vg)
        return list(vo)
    v = both(cto, evo, zvo, avo)
    assert v[:3] == [1, 1, 1]
    zv2 = zvo.copy(); zv2[0, K - 1, 0] ^= 1
    ev2 = evo.copy(); ev2[1, 0, 7] ^= 0x80000000
    av2 = avo.copy(); av2[2, 0, 3] ^= 2
    v = both(cto, ev2, zv2, av2)
    assert v[0] == 0 and v[1] == MALFORMED and v[2] == MALFORMED      # a_vec feeds the challenge: the sum check fails first
    ct2 = cto.copy(); ct2[0, 0] ^= 1
    assert both(ct2, evo, zvo, avo)[0] == 0


# ================================================================== wide batches and operand edges (tests/small_proof_cases.py)
# ---- MulProof
def _mul_prove_verify(oracle, cs):
    bt, a = cs["bt"], cs["a"]
    *o, st = oracle.mul_proof_prove(*bt.key(), *[a[k] for k in SC.MUL_IN])
    return tuple(o), st, oracle.mul_proof_verify(*bt.key(), a["e_a"], a["e_b"], a["e_c"], *o)


def _mul_wide(oracle):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.mul_wide(oracle)
        bt, a = cs["bt"], cs["a"]
        o, st, vh = _mul_prove_verify(oracle, cs)
        t = list(o)
        for k in range(3):                              # f, z1, z2 tampered in different proofs
            t[k] = SC.flip(o[k], cs["tamper"][2 * k:2 * k + 2], salt=k)
        t[4] = o[4].copy()
        for b in cs["bad_edb"]:
            SC.set_int(t[4], b, bt.pq[b][0] * (98765 + b))
        return cs, o, st, vh, tuple(t), oracle.mul_proof_verify(*bt.key(), a["e_a"], a["e_b"], a["e_c"], *t)
    return SC.cached("mul-wide", build)


def _check_mul_wide(cs, st, vh, vt):
    B = cs["bt"].B
    dishonest = cs["false"] + cs["no_inverse"] + cs["bad_edb"]
    assert B > 256 and {0, 63, 64, 255, 256, B - 1} <= set(dishonest)
    for group in (cs["false"], cs["no_inverse"], cs["bad_edb"], cs["tamper"]):
        assert any(b < 256 for b in group) and any(b >= 256 for b in group)
    assert [int(v) for v in st] == [MALFORMED if b in cs["no_inverse"] else 0 for b in range(B)]
    assert [int(v) for v in vh] == [REJECT if b in cs["false"] + cs["no_inverse"] else ACCEPT for b in range(B)]      # (a panicked prove leaves zeros)
    want = [MALFORMED if b in cs["bad_edb"] else REJECT if b in cs["false"] + cs["no_inverse"] + cs["tamper"] else ACCEPT for b in range(B)]
    assert [int(v) for v in vt] == want


def test_wide_mul_case_is_what_it_claims(oracle):
    """CPU: status and verdicts of the 300-proof batch are ACCEPT, REJECT and MALFORMED exactly where the builder put each kind"""
    cs, o, st, vh, t, vt = _mul_wide(oracle)
    _check_mul_wide(cs, st, vh, vt)


@pytest.mark.gpu
def test_gpu_mul_proof_wide_batch(ctx, oracle):
    """300 MulProofs under four 1024-bit keys: a second, partial 256-thread block in k_hash_list, k_modadd, k_mul_finish and
    k_mul_verdict; a GROUPS_PER_BLOCK tail in the limb kernels; false statements, r_c = p and e_db = k p on both sides of the boundary"""
    cs, o, st, vh, t, vt = _mul_wide(oracle)
    bt, a = cs["bt"], cs["a"]
    assert bt.B > 256
    _check_mul_wide(cs, st, vh, vt)
    g = tuple(SC.sentinel(v.shape) for v in o)
    sg = SC.sentinel(bt.B, np.uint8)
    ctx.mul_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, *[a[k] for k in SC.MUL_IN], *g, sg)
    SC.assert_same(st, sg, "status")
    for name, x, y in zip(SC.MUL_OUT, o, g):
        SC.assert_same(x, y, name)
    for proof, want in ((g, vh), (t, vt)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.mul_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, a["e_a"], a["e_b"], a["e_c"], *proof, vg)
        SC.assert_same(want, vg, "verdict")


def _mul_edges(oracle, n_bits):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.mul_edges(oracle, n_bits)
        o, st, vh = _mul_prove_verify(oracle, cs)
        ed, over, wide_ed = SC.mul_edits(cs, o)
        ve = oracle.mul_proof_verify(*cs["bt"].key(), *[ed[k] for k in ("e_a", "e_b", "e_c") + SC.MUL_OUT])
        return cs, o, st, vh, ed, over, wide_ed, ve
    return SC.cached("mul-edges-%d" % n_bits, build)


def _check_mul_edges(cs, o, st, vh, ed, over, wide_ed, ve):
    """every honest proof of edge inputs is accepted; f reaches 0 and n - 1; at a = d = n - 1 the sum e a mod n + d mod n carries out of
    the kw words (k_modadd's carry branch); z1 + n^2 and z2 + n^2 are ACCEPTED; an e_d >= n^2 is in the batch; the edited batch holds all
    three verdicts"""
    bt, a = cs["bt"], cs["a"]
    b = cs["carry"]
    e = pm.compute_digest([bt.ns[b]] + [SC.get_int(a[k], b) for k in ("e_a", "e_b", "e_c")] + [SC.get_int(o[3], b), SC.get_int(o[4], b)])
    assert e * SC.get_int(a["a"], b) % bt.ns[b] + SC.get_int(a["d"], b) % bt.ns[b] >= 1 << bt.n_bits
    assert [int(v) for v in st] == [0] * bt.B and [int(v) for v in vh] == [ACCEPT] * bt.B
    assert SC.get_int(o[0], cs["f_zero"]) == 0 and SC.get_int(o[0], cs["f_top"]) == bt.ns[cs["f_top"]] - 1
    assert len(over) == 2 and all(ve[b] == ACCEPT for b in over)
    assert SC.get_int(ed["e_d"], wide_ed) >= bt.ns[wide_ed] ** 2
    assert {ACCEPT, REJECT, MALFORMED} <= set(int(v) for v in ve)


def test_mul_edge_cases_oracle_matches_python_model(oracle):
    """CPU: the operand edges of tests/small_proof_cases.py (n = 1024) through the C oracle and through oracle/py_model.py.  The reference
    decides: d b and r_d r_b enter Enc unreduced (multiplication_proof.rs:69-76), f = e a + d mod n (:87-88); the verifier hashes e_d and
    e_db as they are (:107-114), uses them modulo n^2 (:131-134) and panics where e_db e_c^e has no inverse (:135)."""
    cs, o, st, vh, ed, over, wide_ed, ve = _mul_edges(oracle, 1024)
    bt, a = cs["bt"], cs["a"]
    _check_mul_edges(cs, o, st, vh, ed, over, wide_ed, ve)
    for b, n in enumerate(bt.ns):
        assert tuple(SC.get_int(v, b) for v in o) == pm.mul_proof_prove(n, *[SC.get_int(a[k], b) for k in SC.MUL_IN]), b
        try:
            got = ACCEPT if pm.mul_proof_verify(n, *[SC.get_int(ed[k], b) for k in ("e_a", "e_b", "e_c") + SC.MUL_OUT]) else REJECT
        except pm.Panic:
            got = MALFORMED
        assert got == ve[b], b
    b = cs["short"]["mul"]
    assert pm.compute_digest([bt.ns[b]] + [SC.get_int(a[k], b) for k in ("e_a", "e_b", "e_c")] + [SC.get_int(o[3], b), SC.get_int(o[4], b)]) >> 248 == 0


def test_keys_for_4096_bits_are_what_the_cases_need():
    """CPU: the four 4096-bit moduli of small_proof_cases.keys_for — no prime is generated for them.  What the cases rely on: distinct odd
    moduli of exactly 4096 bits, p a proper factor of n (r_c = p and e_db = k p then have no inverse modulo n^2), and p a factor of no
    other key's modulus (an item built to have no inverse under its own key is an ordinary one under a neighbour's)"""
    from importlib import import_module
    ks = SC.keys_for(4096, 4)
    assert len(ks) == 4 and len(set(n for p, q, n in ks)) == 4
    assert ks[0] == tuple(import_module("zk-paillier_amd.synth").bench_key_4096())
    for i, (p, q, n) in enumerate(ks):
        assert n.bit_length() == 4096 and n & 1
        assert 1 < p < n and n % p == 0 and q == n // p and p * q == n
        assert H.is_probable_prime(p, rounds=4)
        assert all(math.gcd(m, p) == 1 for j, (_, _, m) in enumerate(ks) if j != i)
    assert [k[2] for k in SC.keys_for(4096, 3)] == [k[2] for k in ks[:3]]


def test_mul_edge_cases_at_4096_bits_oracle_matches_python_model(oracle):
    """CPU: the 4096-bit edge batch (per-proof keys: the benchmark's key and two products of pooled primes) is what it claims
    (_check_mul_edges: f reaches 0 and n - 1, the sum that carries out of 128 words, z + n^2 accepted, all three verdicts among the edited
    proofs), and the C oracle agrees with oracle/py_model.py on three of its items, proving and verifying: a, b, d with every limb set, the
    `carry` item (a = b = d = n - 1) and an ordinary proof, whose f is 0 in the edited batch.  (Three items: one Enc takes CPython 0.7 s at
    this width; the whole batch is compared at 1024 bits above.)"""
    cs, o, st, vh, ed, over, wide_ed, ve = _mul_edges(oracle, 4096)
    bt, a = cs["bt"], cs["a"]
    assert bt.n_bits == 4096 and not bt.shared and len(set(bt.ns)) == 3
    _check_mul_edges(cs, o, st, vh, ed, over, wide_ed, ve)
    b_all, b_carry, b_ord = cs["all_set"], cs["carry"], cs["free"][0]
    assert all(SC.get_int(a[k], b_all) == bt.top for k in ("a", "b", "d"))
    assert all(SC.get_int(a[k], b_carry) == bt.ns[b_carry] - 1 for k in ("a", "b", "d"))
    assert SC.get_int(ed["f"], b_ord) == 0 and SC.get_int(o[0], b_ord) != 0
    for b in (b_all, b_carry, b_ord):
        n = bt.ns[b]
        assert tuple(SC.get_int(v, b) for v in o) == pm.mul_proof_prove(n, *[SC.get_int(a[k], b) for k in SC.MUL_IN]), b
        got = ACCEPT if pm.mul_proof_verify(n, *[SC.get_int(ed[k], b) for k in ("e_a", "e_b", "e_c") + SC.MUL_OUT]) else REJECT
        assert got == ve[b], b


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_gpu_mul_proof_operand_edges(ctx, oracle, n_bits):
    """a, b, d in {0, 1, n - 1, 2^n_bits - 1}, r_* in {1, n - 1, 2^n_bits - 1}, f = 0 and n - 1, a sum that carries out of kw words (k_modadd);
    z1, z2 >= n^2 (accepted), all ones, 0; e_d, e_db >= n^2, 0, 1, ragged, e_db = k p; a short challenge"""
    cs, o, st, vh, ed, over, wide_ed, ve = _mul_edges(oracle, n_bits)
    bt, a = cs["bt"], cs["a"]
    _check_mul_edges(cs, o, st, vh, ed, over, wide_ed, ve)
    g = tuple(SC.sentinel(v.shape) for v in o)
    sg = SC.sentinel(bt.B, np.uint8)
    ctx.mul_proof_prove(bt.n_bits, bt.B, bt.n_arr, bt.stride, *[a[k] for k in SC.MUL_IN], *g, sg)
    if n_bits == 4096:
        assert ctx.last_geometry() == ctx.test_geometry, "the call ran on another engine than the one this family pins"
    SC.assert_same(st, sg, "status")
    for name, x, y in zip(SC.MUL_OUT, o, g):
        SC.assert_same(x, y, name)
    if n_bits == 1024:
        b = cs["short"]["mul"]
        assert pm.compute_digest([bt.ns[b]] + [SC.get_int(a[k], b) for k in ("e_a", "e_b", "e_c")] + [SC.get_int(g[3], b), SC.get_int(g[4], b)]) >> 248 == 0
    for stmt, proof, want in ((a, g, vh), (ed, [ed[k] for k in SC.MUL_OUT], ve)):
        vg = SC.sentinel(bt.B, np.uint8)
        ctx.mul_proof_verify(bt.n_bits, bt.B, bt.n_arr, bt.stride, stmt["e_a"], stmt["e_b"], stmt["e_c"], *proof, vg)
        assert n_bits != 4096 or ctx.last_geometry() == ctx.test_geometry
        SC.assert_same(want, vg, "verdict")


# ---- CorrectMessageProof
def _cm_prove(oracle, cs):
    bt, a = cs["bt"], cs["a"]
    return oracle.correct_message_prove(bt.n_bits, cs["K"], bt.n_arr, bt.stride, a["valid"], a["msg"], a["r"], a["e_sim"], a["z_sim"], a["w"])


def _cm_verify(oracle, cs, ct, ev, zv, av):
    bt = cs["bt"]
    return oracle.correct_message_verify(bt.n_bits, cs["K"], bt.n_arr, bt.stride, cs["a"]["valid"], ct, ev, zv, av)


def _gpu_cm_prove(ctx, cs, like):
    bt, a, K = cs["bt"], cs["a"], cs["K"]
    g = tuple(SC.sentinel(v.shape) for v in like[:4])
    sg = SC.sentinel(bt.B, np.uint8)
    ctx.correct_message_prove(bt.n_bits, bt.B, K, bt.n_arr, bt.stride, a["valid"], a["msg"], a["r"], a["e_sim"], a["z_sim"], a["w"], *g, sg)
    SC.assert_same(like[4], sg, "status")
    for name, x, y in zip(("ciphertext", "e_vec", "z_vec", "a_vec"), like[:4], g):
        SC.assert_same(x, y, name)
    return g


def _gpu_cm_verify(ctx, cs, proof, want):
    bt = cs["bt"]
    vg = SC.sentinel(bt.B, np.uint8)
    ctx.correct_message_verify(bt.n_bits, bt.B, cs["K"], bt.n_arr, bt.stride, cs["a"]["valid"], *proof, vg)
    SC.assert_same(want, vg, "verdict")


def _cm_wide(oracle, K):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.cm_wide(K)
        o = _cm_prove(oracle, cs)
        t = (o[0], SC.flip(o[1], cs["tamper_e"]), SC.flip(o[2], cs["tamper_z"]), o[3])
        return cs, o, _cm_verify(oracle, cs, *o[:4]), t, _cm_verify(oracle, cs, *t)
    return SC.cached("cm-wide-%d" % K, build)


def _check_cm_wide(cs, o, vh, vt):
    B, K = cs["bt"].B, cs["K"]
    assert B * K > 256 and (K > 1 or B > 256)
    panicked = cs["not_listed"] + cs["no_inverse"]
    row_owners = {0, 63, 64, B - 1} | ({255, 256} if K == 1 else {255 // K, 256 // K})
    assert row_owners <= set(panicked + cs["tamper_z"])
    assert [int(v) for v in o[4]] == [MALFORMED if b in panicked else 0 for b in range(B)]
    # a panicked prove leaves zeros: 0 != H(0 ...) mod 2^256, the assert_eq! of correct_message.rs:138
    assert [int(v) for v in vh] == [MALFORMED if b in panicked else ACCEPT for b in range(B)]
    assert [int(v) for v in vt] == [MALFORMED if b in panicked + cs["tamper_e"] else REJECT if b in cs["tamper_z"] else ACCEPT for b in range(B)]
    assert {ACCEPT, REJECT, MALFORMED} <= set(int(v) for v in vt)


@pytest.mark.parametrize("K", [3, 1])
def test_wide_correct_message_case_is_what_it_claims(oracle, K):
    """CPU: status and verdicts of the wide batches are ACCEPT, REJECT and MALFORMED exactly where the builder put each kind"""
    cs, o, vh, t, vt = _cm_wide(oracle, K)
    _check_cm_wide(cs, o, vh, vt)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 1])
def test_gpu_correct_message_wide_batch(ctx, oracle, K):
    """K = 3: 130 proofs, 390 rows — the per-row kernels (k_repeat_rows, k_add_one, k_cm_gather, k_cm_scatter, k_square_words; rows
    b * K + i and b * (K - 1) + j) cross the 256-thread block boundary.  K = 1: 300 proofs — the per-proof kernels (k_cm_plan, k_cm_ei,
    k_cm_verdict) cross it, and no row is simulated."""
    cs, o, vh, t, vt = _cm_wide(oracle, K)
    assert cs["bt"].B * K > 256
    _check_cm_wide(cs, o, vh, vt)
    g = _gpu_cm_prove(ctx, cs, o)
    _gpu_cm_verify(ctx, cs, g, vh)
    _gpu_cm_verify(ctx, cs, t, vt)


def _cm_edges(oracle, n_bits):
    def build():
        oracle.set_threads(min(8, oracle.max_threads()))
        cs = SC.cm_edges(n_bits)
        o = _cm_prove(oracle, cs)
        vh = _cm_verify(oracle, cs, *o[:4])
        ed, over, rebalanced = SC.cm_edits(cs, *o[:4])
        proof = (ed["ct"], ed["e_vec"], ed["z_vec"], ed["a_vec"])
        k1 = SC.cm_k1()
        o1 = _cm_prove(oracle, k1)
        return cs, o, vh, proof, over, rebalanced, _cm_verify(oracle, cs, *proof), k1, o1, _cm_verify(oracle, k1, *o1[:4])
    return SC.cached("cm-edges-%d" % n_bits, build)


def _check_cm_edges(cs, o, vh, proof, over, rebalanced, ve, k1, o1, v1):
    """honest proofs of edge inputs are accepted; a message listed twice proves without a panic, and the reference's own verifier then
    panics on it (both rows take e_i, :95-106, the unused simulated e stays in the sum, :88: the sums differ, :138); an unlisted message
    panics (:74), at K = 1 too; z + n and ciphertext + n^2 are ACCEPTED; a rebalanced e_vec passes the sum check and is REJECTED"""
    B = cs["bt"].B
    dup, nl = cs["duplicate"], cs["not_listed"]
    assert [int(v) for v in o[4]] == [MALFORMED if b == nl else 0 for b in range(B)]
    assert [int(v) for v in vh] == [MALFORMED if b in (dup, nl) else ACCEPT for b in range(B)]
    assert len(over) == 2 and all(ve[b] == ACCEPT for b in over)
    assert len(rebalanced) == 3 and all(ve[b] == REJECT for b in rebalanced)
    assert {ACCEPT, REJECT, MALFORMED} <= set(int(v) for v in ve)
    assert [int(v) for v in o1[4]] == [0, MALFORMED, 0, MALFORMED] and [int(v) for v in v1] == [ACCEPT, MALFORMED, ACCEPT, MALFORMED]


def _model_cm_verify(n, valid, ct, ev, zv, av, b):
    try:
        ok = pm.correct_message_verify(n, valid, SC.get_int(ct, b), [SC.get_int(ev[b], k) for k in range(len(valid))],
                                       [SC.get_int(zv[b], k) for k in range(len(valid))], [SC.get_int(av[b], k) for k in range(len(valid))])
        return ACCEPT if ok else REJECT
    except pm.Panic:
        return MALFORMED


def test_correct_message_edge_cases_oracle_matches_python_model(oracle):
    """CPU: the operand edges of tests/small_proof_cases.py (n = 1024; K = 3, and K = 1) through the C oracle and through
    oracle/py_model.py.  The reference decides: every valid message equal to the encrypted one takes the real branch (correct_message.rs:71,
    98, 111), so a duplicate uses one simulated row less while e_i is still the challenge minus ALL K - 1 simulated e (:88-91); a message
    in no row indexes zi_vec past its end (:74); e_i = chal - sum modulo 2^256 (:91); the verifier compares the sums modulo 2^256 (:135-138)
    and raises each z to n modulo n^2 as it is (:151)."""
    cs, o, vh, proof, over, rebalanced, ve, k1, o1, v1 = _cm_edges(oracle, 1024)
    _check_cm_edges(cs, o, vh, proof, over, rebalanced, ve, k1, o1, v1)
    for c, out, vv in ((cs, o, None), (k1, o1, v1)):
        bt = c["bt"]
        for b, (n, q) in enumerate(zip(bt.ns, c["rows"])):
            try:
                want = pm.correct_message_prove(n, q["valid"], q["msg"], q["r"], q["e_sim"], q["z_sim"], q["w"])
            except pm.Panic:
                assert out[4][b] == MALFORMED and not out[1][b].any() and not out[2][b].any() and not out[3][b].any(), b
                assert SC.get_int(out[0], b) == pm.enc(n, q["msg"], q["r"])
                continue
            K = len(q["valid"])
            got = (SC.get_int(out[0], b), [SC.get_int(out[1][b], k) for k in range(K)], [SC.get_int(out[2][b], k) for k in range(K)], [SC.get_int(out[3][b], k) for k in range(K)])
            assert out[4][b] == 0 and got == want, b
            if vv is not None:
                assert _model_cm_verify(n, q["valid"], *out[:4], b) == vv[b], b
    for b, (n, q) in enumerate(zip(cs["bt"].ns, cs["rows"])):
        assert _model_cm_verify(n, q["valid"], *proof, b) == ve[b], b
        assert _model_cm_verify(n, q["valid"], *o[:4], b) == vh[b], b
    b = cs["short"]["cm"]
    chal = pm.compute_digest([SC.get_int(o[3][b], k) for k in range(3)])
    assert chal >> 248 == 0 and SC.get_int(o[1][b], cs["rows"][b]["valid"].index(cs["rows"][b]["msg"])) == chal


def test_correct_message_edge_cases_at_4096_bits_oracle_matches_python_model(oracle):
    """CPU: the 4096-bit edge batch (K = 3, per-proof keys: the benchmark's key and two products of pooled primes) is what it claims
    (_check_cm_edges: the duplicate and the unlisted message, z + n and ciphertext + n^2 accepted, a rebalanced e_vec rejected, all three
    verdicts among the edited proofs), and the C oracle agrees with oracle/py_model.py on three of its items, proving and verifying: the
    simulated z at n - 1 and with every limb set, r = w = n - 1, and an ordinary proof, whose simulated z is n higher in the edited batch.
    (Three items: one Enc takes CPython 0.7 s at this width; the whole batch is compared at 1024 bits above.)"""
    cs, o, vh, proof, over, rebalanced, ve, k1, o1, v1 = _cm_edges(oracle, 4096)
    bt, K = cs["bt"], cs["K"]
    assert bt.n_bits == 4096 and not bt.shared and len(set(bt.ns)) == 3
    _check_cm_edges(cs, o, vh, proof, over, rebalanced, ve, k1, o1, v1)
    b_all, b_n1, b_ord = cs["all_set"], cs["n_minus_1"], cs["free"][0]
    assert cs["rows"][b_all]["z_sim"] == [bt.ns[b_all] - 1, bt.top]
    assert cs["rows"][b_n1]["r"] == cs["rows"][b_n1]["w"] == bt.ns[b_n1] - 1
    assert b_ord == over[0] and any(SC.get_int(proof[2][b_ord], k) > bt.ns[b_ord] for k in range(K))
    for b in (b_all, b_n1, b_ord):
        n, q = bt.ns[b], cs["rows"][b]
        want = pm.correct_message_prove(n, q["valid"], q["msg"], q["r"], q["e_sim"], q["z_sim"], q["w"])
        got = (SC.get_int(o[0], b), [SC.get_int(o[1][b], k) for k in range(K)], [SC.get_int(o[2][b], k) for k in range(K)], [SC.get_int(o[3][b], k) for k in range(K)])
        assert o[4][b] == 0 and got == want, b
        assert _model_cm_verify(n, q["valid"], *proof, b) == ve[b], b


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_gpu_correct_message_operand_edges(ctx, oracle, n_bits):
    """e_sim rows of 0 and 2^256 - 1 (k_cm_ei's borrow), r, w, z_sim at 0, 1, n - 1, 2^n_bits - 1, message 0, a message listed twice, an
    unlisted one (K = 3 and K = 1); e_vec rebalanced through 2^256 (k_cm_verdict's carry: REJECT, not MALFORMED), z + n and
    ciphertext + n^2 (accepted), a_vec >= n^2, 0, 1 and of ragged byte length (k_hash_list); a short challenge as the real row's exponent"""
    cs, o, vh, proof, over, rebalanced, ve, k1, o1, v1 = _cm_edges(oracle, n_bits)
    _check_cm_edges(cs, o, vh, proof, over, rebalanced, ve, k1, o1, v1)
    g = _gpu_cm_prove(ctx, cs, o)
    if n_bits == 1024:
        b = cs["short"]["cm"]
        assert pm.compute_digest([SC.get_int(g[3][b], k) for k in range(3)]) >> 248 == 0
    _gpu_cm_verify(ctx, cs, g, vh)
    _gpu_cm_verify(ctx, cs, proof, ve)
    g1 = _gpu_cm_prove(ctx, k1, o1)
    _gpu_cm_verify(ctx, k1, g1, v1)
