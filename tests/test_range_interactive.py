"""The three functions of the interactive RangeProof on their own — generate_encrypted_pairs
(range_proof.rs:128-193), generate_proof (:210-252), verifier_output (:254-355) — with the
challenge supplied by the caller and an error factor other than 128 (range_proof.rs:431-525 and
benches/all.rs:10-53 run them with 40 / 120).  CPU tests: C oracle against the pure-Python model.
GPU tests: HIP path against the C oracle, byte-exact."""
import numpy as np
import pytest

import helpers as H
import small_proof_cases as SC
from helpers import pm, L, zkp

OUT_FIELDS = ("c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")


def challenge(seed, B, ef, short=()):
    """[B][32] challenge bytes, ceil(ef/8) of them used (verifier_commit samples ef bits); proofs in
    `short` get one byte fewer than needed."""
    d = pm.Drbg(seed)
    e = np.zeros((B, 32), np.uint8); elen = np.zeros(B, np.uint8)
    for b in range(B):
        k = (ef + 7) // 8 - (1 if b in short else 0)
        e[b, :k] = np.frombuffer(d.bytes(k), np.uint8)
        elen[b] = k
    return e, elen


def clone_inputs(pb):
    q = zkp.RangeBatch(pb.n_bits, pb.batch, pb.ef, shared_key=pb.shared_key)
    q.n[:] = pb.n; q.range[:] = pb.range; q.ciphertext[:] = pb.ciphertext
    return q


def run_interactive(impl, pb, wt, e, elen, gpu):
    B = pb.batch
    st = np.full(B, 9, np.uint8); v = np.full(B, 7, np.uint8)
    kw = dict(device=False) if gpu else {}
    impl.range_generate_encrypted_pairs(pb.struct(), wt.struct(), **kw)
    impl.range_generate_proof(pb.struct(), wt.struct(), e, elen, st, **kw)
    impl.range_verifier_output(pb.struct(), e, elen, v, **kw)
    return st, v


@pytest.mark.parametrize("ef", [40, 120])
def test_oracle_interactive_matches_python_model(oracle, ef):
    n_bits, B = 1024, 3
    n = H.test_key(512)[2]
    cases = H.build_range_case(b"interactive-%d" % ef, [n], n_bits, B, ef=ef)
    cases[-1] = H.build_range_case(b"interactive-bad", [n], n_bits, 1, honest=False, ef=ef)[0]
    pb, wt = H.fill_batch(cases, n_bits, True, oracle)
    e, elen = challenge(b"chal-%d" % ef, B, ef)
    st, v = run_interactive(oracle, pb, wt, e, elen, gpu=False)
    assert list(st) == [0] * B
    assert list(v) == [zkp.VERDICT_ACCEPT] * (B - 1) + [zkp.VERDICT_REJECT]
    for b, c in enumerate(cases):
        eb = bytes(e[b, :elen[b]])
        c1, c2 = pm.generate_encrypted_pairs(n, c["w1"], c["w2"], c["r1"], c["r2"])
        assert [L.limbs_to_int(r) for r in pb.c1[b]] == c1
        assert [L.limbs_to_int(r) for r in pb.c2[b]] == c2
        resp = pm.generate_proof(n, c["x"], c["r"], eb, c["range"], c["w1"], c["w2"], c["r1"], c["r2"], ef)
        assert H.responses_from_batch(pb, b) == resp
        cx = L.limbs_to_int(pb.ciphertext[b])
        assert pm.verifier_output(n, eb, c1, c2, resp, c["range"], cx, ef) == (v[b] == zkp.VERDICT_ACCEPT)


def test_oracle_split_phases_equal_ni_prove(oracle):
    """RangeProofNi::prove == generate_encrypted_pairs ; compute_digest ; generate_proof (range_proof_ni.rs:47-82)"""
    n_bits, B = 1024, 2
    n = H.test_key(512)[2]
    cases = H.build_range_case(b"split-phases", [n], n_bits, B)
    pa, wt = H.fill_batch(cases, n_bits, True, oracle)
    pb = clone_inputs(pa)
    e = np.zeros((B, 32), np.uint8); elen = np.zeros(B, np.uint8); st = np.zeros(B, np.uint8)
    oracle.range_ni_prove(pa.struct(), wt.struct(), e, elen, st)
    st2 = np.full(B, 9, np.uint8)
    oracle.range_generate_encrypted_pairs(pb.struct(), wt.struct())
    oracle.range_generate_proof(pb.struct(), wt.struct(), e, elen, st2)
    assert list(st2) == [0] * B
    for f in OUT_FIELDS:
        assert np.array_equal(getattr(pa, f), getattr(pb, f)), f
    v1 = np.zeros(B, np.uint8); v2 = np.zeros(B, np.uint8)
    oracle.range_ni_verify(pa.struct(), v1)
    oracle.range_verifier_output(pb.struct(), e, elen, v2)
    assert list(v1) == list(v2) == [zkp.VERDICT_ACCEPT] * B


def test_oracle_short_challenge_is_malformed(oracle):
    n_bits, B, ef = 1024, 2, 40
    n = H.test_key(512)[2]
    cases = H.build_range_case(b"short-chal", [n], n_bits, B, ef=ef)
    pb, wt = H.fill_batch(cases, n_bits, True, oracle)
    e, elen = challenge(b"short", B, ef, short={1})
    st, v = run_interactive(oracle, pb, wt, e, elen, gpu=False)
    assert list(st) == [0, zkp.VERDICT_MALFORMED]
    assert list(v) == [zkp.VERDICT_ACCEPT, zkp.VERDICT_MALFORMED]


@pytest.mark.gpu
@pytest.mark.parametrize("n_bits,key_bits,ef,shared", [(1024, 512, 40, True), (1024, 1024, 120, False), (2048, 2048, 40, True), (1024, 512, 1, True),
                                                        (1024, 512, 256, True), (4096, 4096, 3, True)])
def test_gpu_interactive_matches_oracle(ctx, oracle, n_bits, key_bits, ef, shared):
    B = 4
    if key_bits == 2048:
        keys = [H.fixture_key()[2]]
    elif key_bits == 4096:
        keys = [SC.keys_for(4096, 1)[0][2]]        # the benchmark's key (no 2048-bit prime is generated here); 3 rows per proof: 24 Enc
    else:
        keys = [H.test_key(key_bits, tag=i)[2] for i in range(1 if shared else B)]
    cases = H.build_range_case(b"gpu-inter-%d-%d" % (n_bits, ef), keys, n_bits, B, shared=shared, ef=ef)
    cases[1] = H.build_range_case(b"gpu-inter-bad", [cases[1]["n"]], n_bits, 1, honest=False, ef=ef)[0]
    po, wt = H.fill_batch(cases, n_bits, shared, oracle)
    pg = clone_inputs(po)
    e, elen = challenge(b"gpu-chal-%d" % ef, B, ef, short={3} if ef > 8 else ())
    so, vo = run_interactive(oracle, po, wt, e, elen, gpu=False)
    # the proof with the short challenge: the reference panics in generate_proof; the rows the two sides leave
    # behind for it are unspecified, so give both the same content before comparing
    pg.resp_w1[:] = 0xA5A5A5A5; pg.resp_kind[:] = 77
    ctx.range_generate_encrypted_pairs(pg.struct(), wt.struct(), device=False)
    assert (pg.resp_w1 == 0xA5A5A5A5).all() and (pg.resp_kind == 77).all()     # phase 1 writes c1 / c2 only
    c1_before = pg.c1.copy()
    sg, vg = run_interactive(ctx, pg, wt, e, elen, gpu=True)
    assert np.array_equal(c1_before, pg.c1)
    assert np.array_equal(so, sg) and np.array_equal(vo, vg)
    ok = so == 0
    for f in OUT_FIELDS:
        a, b = getattr(po, f), getattr(pg, f)
        sel = slice(None) if f in ("c1", "c2") else ok
        assert np.array_equal(a[sel], b[sel]), f
    assert vo[0] == zkp.VERDICT_ACCEPT and vo[1] == zkp.VERDICT_REJECT


@pytest.mark.gpu
def test_gpu_verifier_output_tampered_challenge(ctx, oracle):
    """flipping challenge bits after the proof was made turns Open rows into Mask rows and the other way round:
    the response enum no longer matches the bit (range_proof.rs:270-348 falls to the `_ => false` arm)"""
    n_bits, B, ef = 1024, 6, 40
    n = H.test_key(512)[2]
    cases = H.build_range_case(b"gpu-flip", [n], n_bits, B, ef=ef)
    po, wt = H.fill_batch(cases, n_bits, True, oracle)
    e, elen = challenge(b"gpu-flip-chal", B, ef)
    st = np.zeros(B, np.uint8)
    oracle.range_generate_encrypted_pairs(po.struct(), wt.struct())
    oracle.range_generate_proof(po.struct(), wt.struct(), e, elen, st)
    e2 = e.copy()
    e2[1, 0] ^= 0x80          # first bit
    e2[2, 4] ^= 0x01          # bit 39: the last one used
    e2[3, 5] ^= 0xFF          # beyond error_factor: unused, still accepts
    e2[4, 2] ^= 0x10
    vo = np.zeros(B, np.uint8); vg = np.full(B, 7, np.uint8)
    oracle.range_verifier_output(po.struct(), e2, elen, vo)
    ctx.range_verifier_output(po.struct(), e2, elen, vg, device=False)
    assert np.array_equal(vo, vg)
    assert list(vo) == [1, 0, 0, 1, 0, 1]
