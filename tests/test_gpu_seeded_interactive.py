"""GPU tests of the two seeded prover steps of the interactive RangeProof (include/zkp_hip.h: zkp_range_generate_encrypted_pairs_seeded_batch,
zkp_range_generate_proof_seeded_batch): byte for byte against the unseeded GPU steps fed the model's witness (tests/seeded_model.py) and
against the oracle, what each step writes and leaves alone, the wipe, device pointers, chunk invariance, the non-interactive seeded prove at
128 rows, the sampler's MALFORMED cases, refused arguments and the library's own routing."""
import numpy as np
import pytest

import helpers as H
import seeded_interactive_cases as IC
from helpers import L, zkp

pytestmark = pytest.mark.gpu

SEED, FIRST = IC.SEED, IC.FIRST_INDEX
MALFORMED = zkp.VERDICT_MALFORMED


def stale(pb, fields):
    word = {f: (getattr(pb, f) == (77 if f in ("resp_kind", "resp_j") else 0xA5A5A5A5)).all() for f in fields}
    return [f for f, ok in word.items() if not ok]


def seeded_steps(ctx, pb, wt, e, elen, first_index=FIRST, seed=SEED):
    """step 1 and step 2 on host arrays, with everything the issue says about what a step writes; -> (status of step 1, status of step 2)"""
    B = pb.batch
    s1, s2 = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
    ctx.range_generate_encrypted_pairs_seeded(pb.struct(), seed, first_index, s1)
    assert ctx.witness_residue() == 0
    assert stale(pb, IC.RESP_FIELDS) == [], "step 1 writes c1 and c2 only"
    c1, c2 = pb.c1.copy(), pb.c2.copy()
    ctx.range_generate_proof_seeded(pb.struct(), wt.x, wt.r, seed, first_index, e, elen, s2)
    assert ctx.witness_residue() == 0
    assert np.array_equal(c1, pb.c1) and np.array_equal(c2, pb.c2), "step 2 writes resp_* only"
    return s1, s2


def unseeded_steps(ctx, pb, wt, e, elen):
    st = np.full(pb.batch, 9, np.uint8)
    ctx.range_generate_encrypted_pairs(pb.struct(), wt.struct(), device=False)
    ctx.range_generate_proof(pb.struct(), wt.struct(), e, elen, st, device=False)
    return st


def assert_sessions_equal(a, b, ok, what):
    """c1 / c2 of every session; the responses of the sessions whose status is 0 (what is left behind for a MALFORMED one is unspecified)"""
    for f in IC.OUT_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        sel = slice(None) if f in ("c1", "c2") else ok
        assert np.array_equal(x[sel], y[sel]), (what, f)


# ---- 1. the two steps against the model, the unseeded calls and the oracle ------------------------------------------------------------
@pytest.mark.parametrize("shape", IC.SHAPES, ids=IC.SHAPE_IDS)
def test_seeded_steps_equal_the_unseeded_steps_on_the_models_witness_and_the_oracle(ctx, oracle, shape):
    n_bits, key_bits, ef, shared = shape
    B = 4
    cases = IC.session_cases(*shape)
    po, wt = H.fill_batch(cases, n_bits, shared, oracle)
    e, elen = IC.session_challenge(ef, B, short={3} if ef > 8 else ())
    so = IC.oracle_steps(oracle, po, wt, e, elen)
    want = [0, 0, 0, MALFORMED if ef > 8 else 0]
    assert list(so) == want
    pu = IC.fresh(po)
    su = unseeded_steps(ctx, pu, wt, e, elen)
    ps = IC.fresh(po)
    s1, s2 = seeded_steps(ctx, ps, wt, e, elen)
    assert list(s1) == [0] * B and list(s2) == list(su) == want
    ok = so == 0
    assert_sessions_equal(pu, ps, ok, "seeded against the unseeded GPU steps")
    assert_sessions_equal(po, ps, ok, "seeded against the oracle")
    v = np.full(B, 7, np.uint8)
    ctx.range_verifier_output(ps.struct(), e, elen, v, device=False)
    assert v[0] == zkp.VERDICT_ACCEPT and (ef <= 8 or (v[1] == zkp.VERDICT_REJECT and v[3] == MALFORMED))


# ---- 2. device pointers ------------------------------------------------------------------------------------------------------------------
def test_seeded_steps_with_device_pointers_and_their_residue(ctx, oracle):
    import torch
    shape = IC.SHAPES[0]
    n_bits, _, ef, shared = shape
    B = 4
    cases = IC.session_cases(*shape)
    po, wt = H.fill_batch(cases, n_bits, shared, oracle)
    e, elen = IC.session_challenge(ef, B, short={3})
    so = IC.oracle_steps(oracle, po, wt, e, elen)
    dpb = IC.fresh(po).to("cuda")
    dx, dr = torch.from_numpy(wt.x.view(np.int32)).cuda(), torch.from_numpy(wt.r.view(np.int32)).cuda()
    de, dl = torch.from_numpy(e).cuda(), torch.from_numpy(elen).cuda()
    d1, d2 = (torch.full((B,), 9, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    ctx.range_generate_encrypted_pairs_seeded(dpb.struct(), SEED, FIRST, d1, device=True)
    assert ctx.witness_residue() == 0
    ctx.synchronize()
    mid = dpb.to(None)
    assert stale(mid, IC.RESP_FIELDS) == []
    ctx.range_generate_proof_seeded(dpb.struct(), dx, dr, SEED, FIRST, de, dl, d2, device=True)
    assert ctx.witness_residue() == 0
    ctx.synchronize()
    got = dpb.to(None)
    assert np.array_equal(mid.c1, got.c1) and np.array_equal(mid.c2, got.c2)
    assert list(d1.cpu().numpy()) == [0] * B and np.array_equal(d2.cpu().numpy(), so)
    assert_sessions_equal(po, got, so == 0, "device pointers against the oracle")


# ---- 3. chunk invariance -----------------------------------------------------------------------------------------------------------------
def test_two_half_calls_equal_one_call_in_both_steps(ctx, oracle):
    n_bits, ef, B = 1024, 40, 4
    cases = IC.session_cases(1024, 512, ef, True, first_index=0)
    po, wt = H.fill_batch(cases, n_bits, True, oracle)
    e, elen = IC.session_challenge(ef, B)
    one = IC.fresh(po)
    s1, s2 = seeded_steps(ctx, one, wt, e, elen, first_index=0)
    two = IC.fresh(po)
    t1, t2 = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
    for lo in (0, B // 2):
        hi = lo + B // 2
        ctx.range_generate_encrypted_pairs_seeded(two.slice(lo, hi).struct(), SEED, lo, t1[lo:hi])
    for lo in (0, B // 2):
        hi = lo + B // 2
        ctx.range_generate_proof_seeded(two.slice(lo, hi).struct(), wt.x[lo:hi], wt.r[lo:hi], SEED, lo, e[lo:hi], elen[lo:hi], t2[lo:hi])
    for f in IC.OUT_FIELDS:
        assert np.array_equal(getattr(one, f), getattr(two, f)), f
    assert np.array_equal(s1, t1) and np.array_equal(s2, t2) and not s2.any()
    so = IC.oracle_steps(oracle, po, wt, e, elen)
    assert_sessions_equal(po, two, so == 0, "two calls of B / 2 against the oracle")


# ---- 4. the non-interactive seeded prove is the two steps around the Fiat-Shamir challenge ----------------------------------------------
def test_steps_at_128_rows_equal_the_seeded_range_proof_ni(ctx, oracle):
    n_bits, ef, B = 1024, 128, 2
    cases = IC.session_cases(1024, 512, ef, True, B=B, dishonest=None)
    po, wt = H.fill_batch(cases, n_bits, True, oracle)
    ni = IC.fresh(po, fill=False)
    ne, nl, ns = np.full((B, 32), 7, np.uint8), np.full(B, 7, np.uint8), np.full(B, 9, np.uint8)
    ctx.range_ni_prove_seeded(ni.struct(), wt.x, wt.r, SEED, FIRST, ne, nl, ns, device=False)
    pb = IC.fresh(po)
    s1 = np.full(B, 9, np.uint8)
    ctx.range_generate_encrypted_pairs_seeded(pb.struct(), SEED, FIRST, s1)
    e, elen = np.full((B, 32), 7, np.uint8), np.full(B, 7, np.uint8)
    ctx.range_challenge(pb.struct(), e, elen, device=False)
    assert np.array_equal(e, ne) and np.array_equal(elen, nl)
    s2 = np.full(B, 9, np.uint8)
    ctx.range_generate_proof_seeded(pb.struct(), wt.x, wt.r, SEED, FIRST, e, elen, s2)
    assert ctx.witness_residue() == 0
    for f in IC.OUT_FIELDS:
        assert np.array_equal(getattr(ni, f), getattr(pb, f)), f
    assert not s1.any() and np.array_equal(s2, ns) and not ns.any()


# ---- 5. the sampler's MALFORMED cases -----------------------------------------------------------------------------------------------------
def test_a_range_of_two_is_malformed_and_leaves_its_neighbours_alone(ctx, oracle):
    n_bits, ef, B = 1024, 40, 4
    kw = n_bits // 32
    cases = IC.session_cases(1024, 512, ef, True, dishonest=None)
    po, wt = H.fill_batch(cases, n_bits, True, oracle)
    e, elen = IC.session_challenge(ef, B)
    honest = IC.fresh(po)
    h1, h2 = seeded_steps(ctx, honest, wt, e, elen)
    assert not h1.any() and not h2.any()
    bad = IC.fresh(po)
    bad.range[2] = L.int_to_limbs(2, kw)
    b1, b2 = seeded_steps(ctx, bad, wt, e, elen)
    assert list(b1) == [0, 0, MALFORMED, 0] and list(b2) == [0, 0, MALFORMED, 0]
    others = [0, 1, 3]
    for f in IC.OUT_FIELDS:
        assert np.array_equal(getattr(honest, f)[others], getattr(bad, f)[others]), f
    # its witness is all zero: c1 = c2 = Enc(0, 0) = 0 in every row, which is what the unseeded call writes for a zero witness
    zero = zkp.make_range_witness(n_bits, 1, ef)
    zb = zkp.RangeBatch(n_bits, 1, ef, shared_key=True)
    zb.n[:] = po.n; zb.range[0] = bad.range[2]
    ctx.range_generate_encrypted_pairs(zb.struct(), zero.struct(), device=False)
    assert np.array_equal(zb.c1[0], bad.c1[2]) and np.array_equal(zb.c2[0], bad.c2[2])


# ---- 6. refused arguments -----------------------------------------------------------------------------------------------------------------
def test_refused_arguments_name_the_entry_point_and_leave_no_residue(ctx, oracle):
    n_bits, ef, B = 1024, 40, 4
    cases = IC.session_cases(1024, 512, ef, True, dishonest=None)
    po, wt = H.fill_batch(cases, n_bits, True, oracle)
    e, elen = IC.session_challenge(ef, B)
    pb = IC.fresh(po)
    seeded_steps(ctx, pb, wt, e, elen)                    # (the blocks whose residue is counted below)
    step1, step2 = "status 1: zkp_range_generate_encrypted_pairs_seeded_batch", "status 1: zkp_range_generate_proof_seeded_batch"
    with pytest.raises(zkp.ZkpError, match=step1):
        ctx.range_generate_encrypted_pairs_seeded(pb.struct(), None, 0)
    with pytest.raises(zkp.ZkpError, match=step2):
        ctx.range_generate_proof_seeded(pb.struct(), wt.x, wt.r, None, 0, e, elen)
    for bad_ef in (0, 257):
        s = pb.struct()
        s.error_factor = bad_ef
        with pytest.raises(zkp.ZkpError, match=step1):
            ctx.range_generate_encrypted_pairs_seeded(s, SEED, 0)
        with pytest.raises(zkp.ZkpError, match=step2):
            ctx.range_generate_proof_seeded(s, wt.x, wt.r, SEED, 0, e, elen)
    with pytest.raises(zkp.ZkpError, match=step2):
        ctx.range_generate_proof_seeded(pb.struct(), wt.x, wt.r, SEED, 0, None, elen)
    with pytest.raises(zkp.ZkpError, match=step2):
        ctx.range_generate_proof_seeded(pb.struct(), wt.x, wt.r, SEED, 0, e, None)
    assert ctx.witness_residue() == 0
    empty = pb.struct()
    empty.batch = 0
    ctx.range_generate_encrypted_pairs_seeded(empty, SEED, 0)
    ctx.range_generate_proof_seeded(empty, None, None, SEED, 0, e, elen)


# ---- 7. the library's own routing ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def actx():
    """nothing pinned: the library's own routing (the sizes are two engines of tests/test_gpu_routing.py)"""
    c = zkp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("B", [2, 70])
def test_seeded_step_one_takes_the_route_of_the_unseeded_call(actx, oracle, B):
    n_bits, ef = 2048, 40
    cases = IC.session_cases(2048, 2048, ef, True, B=B, first_index=5, dishonest=None)
    oracle.set_threads(min(16, oracle.max_threads()))
    po, wt = H.fill_batch(cases, n_bits, True, oracle)
    actx.set_geometry(0)
    actx.set_enc_form("auto")
    pu = IC.fresh(po)
    actx.range_generate_encrypted_pairs(pu.struct(), wt.struct(), device=False)
    route = (actx.last_geometry(), actx.last_split())
    ps = IC.fresh(po)
    st = np.full(B, 9, np.uint8)
    actx.range_generate_encrypted_pairs_seeded(ps.struct(), SEED, 5, st)
    assert (actx.last_geometry(), actx.last_split()) == route, "the seeded call takes the route of the unseeded call"
    assert actx.witness_residue() == 0
    assert not st.any()
    assert np.array_equal(pu.c1, ps.c1) and np.array_equal(pu.c2, ps.c2)
    assert stale(ps, IC.RESP_FIELDS) == []
    # a sample of the batch against the oracle
    idx = sorted({0, B // 2, B - 1})
    so = zkp.RangeBatch(n_bits, len(idx), ef, shared_key=True)
    so.n[:] = po.n
    sw = zkp.make_range_witness(n_bits, len(idx), ef)
    for k, b in enumerate(idx):
        so.range[k] = po.range[b]
        for f in IC.WIT:
            getattr(sw, f)[k] = getattr(wt, f)[b]
    oracle.range_generate_encrypted_pairs(so.struct(), sw.struct())
    for k, b in enumerate(idx):
        assert np.array_equal(so.c1[k], ps.c1[b]) and np.array_equal(so.c2[k], ps.c2[b]), (B, b)
