"""GPU tests of the seeded samplers where the G = kw / 16 lanes of a value must agree (csrc/kernels_sample.hpp: k_range_sample<G>,
k_nonce_sample<G>; G = 2, 4, 8): the comparison decided by a lane below the top one, equality, bounds with idle top lanes, and the carry of
third + s across lanes — on the crafted batches of tests/sampler_lane_cases.py, whose coverage table tests/test_sampler_lane_cases.py
asserts on the CPU.  Bit for bit against the value-level models (tests/seeded_model.py, tests/seeded_nonce_model.py), a property check in
plain integers that depends on no model, chunk invariance (half-calls move every group to other lanes of its wavefront), and one seeded
prove over a range of full width.  The exhaustion of all 128 attempts is not reachable by any constructible input and is not tested."""
import functools

import numpy as np
import pytest

import helpers as H
import sampler_lane_cases as C
import seeded_model as M
import seeded_nonce_cases as NC
import seeded_nonce_model as NM
from helpers import L, zkp

pytestmark = pytest.mark.gpu

OUT_FIELDS = ("c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")
WIT = ("w1", "w2", "r1", "r2")
STALE = 0xA5A5A5A5


def sample_range(ctx, c, lo=0, hi=None):
    """zkp_range_sample_witness_batch on proofs [lo, hi) of a batch, outputs pre-filled with a stale pattern -> ([w1, w2, r1, r2], status)"""
    B = len(c["ranges"])
    hi = B if hi is None else hi
    n_bits, ef, kw = c["n_bits"], c["ef"], c["n_bits"] // 32
    shared = len(c["n_list"]) == 1
    pb = zkp.RangeBatch(n_bits, hi - lo, ef, shared_key=shared)
    for k, n in enumerate(c["n_list"] if shared else c["n_list"][lo:hi]):
        pb.n[k] = L.int_to_limbs(n, kw)
    for k, r in enumerate(c["ranges"][lo:hi]):
        pb.range[k] = L.int_to_limbs(r, kw)
    got = [np.full((hi - lo, ef, kw), STALE, np.uint32) for _ in WIT]
    status = np.full(hi - lo, 9, np.uint8)
    if not c["device"]:
        ctx.range_sample_witness(pb.struct(), C.RANGE_SEED, c["first_index"] + lo, *got, status, device=False)
        return got, status
    import torch
    dpb = pb.to("cuda")
    out = [torch.from_numpy(g.view(np.int32)).cuda() for g in got]
    st = torch.from_numpy(status).cuda()
    torch.cuda.synchronize()
    ctx.range_sample_witness(dpb.struct(), C.RANGE_SEED, c["first_index"] + lo, *out, st, device=True)
    ctx.synchronize()
    return [o.cpu().numpy().view(np.uint32) for o in out], st.cpu().numpy()


def sample_nonces(ctx, c, lo=0, hi=None):
    """zkp_nonce_sample_batch on proofs [lo, hi) of a batch -> (the four arrays by field id, status)"""
    hi = c["B"] if hi is None else hi
    kind, n_bits, K, kw, B = c["kind"], c["n_bits"], c["K"], c["n_bits"] // 32, hi - lo
    n = L.ints_to_limbs(c["n_list"][lo:hi], kw)
    shapes = {NM.KIND_ZERO: [(B, kw), None, None, None], NM.KIND_CIPHERTEXT: [(B, kw), (B, kw), None, None],
              NM.KIND_CORRECT_MESSAGE: [(B, kw), (B, kw), (B, K - 1, 8), (B, K - 1, kw)]}[kind]
    got = [None if s is None else np.full(s, STALE, np.uint32) for s in shapes]
    status = np.full(B, 9, np.uint8)
    if not c["device"]:
        ctx.nonce_sample(kind, n_bits, B, K, n, kw, C.NONCE_SEED, c["first_index"] + lo, got, status)
        return got, status
    import torch
    dev = [None if g is None else torch.from_numpy(g.view(np.int32)).cuda() for g in got]
    dn, st = torch.from_numpy(n.view(np.int32)).cuda(), torch.from_numpy(status).cuda()
    torch.cuda.synchronize()
    ctx.nonce_sample(kind, n_bits, B, K, dn, kw, C.NONCE_SEED, c["first_index"] + lo, dev, st)
    ctx.synchronize()
    return [None if d is None else d.cpu().numpy().view(np.uint32) for d in dev], st.cpu().numpy()


# ---- 1. bit for bit against the value-level models, and the properties that need no model ---------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.range_cases()))
def test_range_sampler_on_crafted_bounds(ctx, name):
    c = C.range_cases()[name]
    B, ef, kw = len(c["ranges"]), c["ef"], c["n_bits"] // 32
    want, want_status, _, _ = C.model_witness(name)
    got, status = sample_range(ctx, c)
    assert list(status) == want_status
    for f, g in zip(WIT, got):
        exp = M.to_limbs(want[f], kw)
        for b in range(B):
            assert np.array_equal(g[b], exp[b]), (name, f, "proof", b, "rows", [r for r in range(ef) if not np.array_equal(g[b, r], exp[b, r])])
    # from the outputs alone, in plain integers: third <= max(w1, w2) < 2 third, {w1, w2} = {a, a - third}, r1, r2 < n
    for b in range(B):
        n = c["n_list"][0 if len(c["n_list"]) == 1 else b]
        third = c["ranges"][b] // 3
        for row in range(ef):
            w1, w2, r1, r2 = (L.limbs_to_int(g[b, row]) for g in got)
            if want_status[b]:
                assert (w1, w2, r1, r2) == (0, 0, 0, 0), "the rows of a MALFORMED proof are zero"
                continue
            a = max(w1, w2)
            assert third <= a < 2 * third and {w1, w2} == {a, a - third} and r1 < n and r2 < n, (name, b, row)


@pytest.mark.parametrize("name", sorted(C.nonce_cases()))
def test_nonce_sampler_on_crafted_bounds(ctx, name):
    c = C.nonce_cases()[name]
    kind, B, K, kw = c["kind"], c["B"], c["K"], c["n_bits"] // 32
    want_nonces, want_status, _ = C.model_nonces(name)
    want = NC.field_arrays(kind, want_nonces, kw, K)
    got, status = sample_nonces(ctx, c)
    assert list(status) == want_status == [0] * B
    for f, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None)
        if g is None:
            continue
        for b in range(B):
            assert np.array_equal(g[b], w[b]), (name, "field", f, "proof", b)
    # from the outputs alone: every sample_below nonce is below its n
    for f in (0, 1, 3):
        if got[f] is not None:
            for b in range(B):
                for v in got[f][b].reshape(-1, kw):
                    assert L.limbs_to_int(v) < c["n_list"][b], (name, "field", f, "proof", b)


# ---- 2. chunk invariance on crafted batches -------------------------------------------------------------------------------------------------
def test_two_half_calls_equal_one_call_on_crafted_batches(ctx):
    c = C.range_cases()["range-2048-carry"]
    B = len(c["ranges"])
    assert B % 2 == 0
    one, s1 = sample_range(ctx, c)
    halves = [sample_range(ctx, c, lo, lo + B // 2) for lo in (0, B // 2)]
    for k, f in enumerate(WIT):
        assert np.array_equal(one[k], np.concatenate([h[0][k] for h in halves])), f
    assert np.array_equal(s1, np.concatenate([h[1] for h in halves]))
    c = C.nonce_cases()["message-4096"]
    B = c["B"]
    assert B % 2 == 0
    one, s1 = sample_nonces(ctx, c)
    halves = [sample_nonces(ctx, c, lo, lo + B // 2) for lo in (0, B // 2)]
    for f in range(4):
        assert np.array_equal(one[f], np.concatenate([h[0][f] for h in halves])), ("field", f)
    assert np.array_equal(s1, np.concatenate([h[1] for h in halves]))


# ---- 3. a seeded prove over a range of full width --------------------------------------------------------------------------------------------
E2E_FIRST_INDEX = 40


@functools.lru_cache(maxsize=None)
def e2e_case():
    """n_bits = 1024, B = 2: proof 0 a 256-bit range, proof 1 a range of 1024 bits whose third makes the full carry chain in one of its rows"""
    n_bits, G = 1024, 2
    n = H.test_key(n_bits)[2]
    index = E2E_FIRST_INDEX + 1
    row, third = C.first_fit(range(128), lambda r: C.craft_third(C.range_candidate(index, r, 0, C.carry_bits(G)), G, C.carry_lanes(("full",), G)))
    cases = H.build_range_case(b"sampler-lanes-e2e", [n], n_bits, 2)
    cases[1]["range"] = 3 * third + 1
    cases[1]["x"] = H.pm.Drbg(b"sampler-lanes-e2e-x").below(third)
    wit, status, _, _ = M.witness(C.RANGE_SEED, E2E_FIRST_INDEX, [n], [k["range"] for k in cases], 128)
    assert not any(status)
    for b, k in enumerate(cases):
        for f in WIT:
            k[f] = wit[f][b]
    assert C.carry_cells(third, min(wit["w1"][1][row], wit["w2"][1][row]), G, 0)[1] == [0, 1]
    return n, cases


def fresh(pb):
    q = zkp.RangeBatch(pb.n_bits, pb.batch, pb.ef, shared_key=pb.shared_key)
    q.n[:] = pb.n; q.range[:] = pb.range; q.ciphertext[:] = pb.ciphertext
    return q


def outs(B):
    return np.full((B, 32), 7, np.uint8), np.full(B, 7, np.uint8), np.full(B, 9, np.uint8)


def assert_same(a, b, ea, eb, what):
    for f in OUT_FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    for x, y, nm in zip(ea, eb, ("out_e", "out_e_len", "out_status")):
        assert np.array_equal(x, y), (what, nm)


def test_seeded_prove_over_a_range_of_full_width(ctx, oracle):
    """range_ni_prove_seeded at n_bits = 1024 with a 1024-bit range (third of 1022 bits, the carry of third + s crossing into lane 1):
    equal to range_ni_prove on the model's witness and to the oracle, after the pattern of
    test_seeded_prove_equals_prove_on_the_models_witness_and_the_oracle.  Neither prover restricts `range`: the statement is well formed
    (status 0 on the oracle and on the GPU), and with x < third under a key of 1024 bits the proof verifies."""
    n_bits, B = 1024, 2
    n, cases = e2e_case()
    pb_o, wt = H.fill_batch(cases, n_bits, True, oracle)
    eo = outs(B)
    oracle.range_ni_prove(pb_o.struct(), wt.struct(), *eo)
    pb_w, ew = fresh(pb_o), outs(B)
    ctx.range_ni_prove(pb_w.struct(), wt.struct(), *ew, device=False)
    pb_s, es = fresh(pb_o), outs(B)
    ctx.range_ni_prove_seeded(pb_s.struct(), wt.x, wt.r, C.RANGE_SEED, E2E_FIRST_INDEX, *es, device=False)
    assert ctx.witness_residue() == 0
    assert_same(pb_w, pb_s, ew, es, "seeded against witness-input prove")
    assert_same(pb_o, pb_s, eo, es, "seeded against the oracle")
    assert list(es[2]) == [0, 0]
    vo, v = np.full(B, 7, np.uint8), np.full(B, 7, np.uint8)
    oracle.range_ni_verify(pb_o.struct(), vo)
    ctx.range_ni_verify(pb_s.struct(), v, device=False)
    assert list(v) == list(vo)
