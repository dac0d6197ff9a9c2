"""GPU tests of seeded RangeProofNi proving (include/zkp_hip.h: zkp_range_sample_witness_batch, zkp_range_ni_prove_seeded_batch,
zkp_multi_range_ni_prove_seeded_batch): the device sampler bit for bit against tests/seeded_model.py, the seeded prove against the
witness-input prove fed the model's witness and against the oracle, chunk invariance, and the wipe of the device blocks."""
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import seeded_cases as SC
import seeded_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu

OUT_FIELDS = ("c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")
WIT = ("w1", "w2", "r1", "r2")
SEED = SC.SEED


# ---- 1. the sampler against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.sampler_cases()))
def test_sampler_is_bit_exact_against_the_model(ctx, name):
    c = SC.sampler_cases()[name]
    n_bits, ef, B = c["n_bits"], c["ef"], len(c["ranges"])
    kw = n_bits // 32
    shared = len(c["n_list"]) == 1
    want, want_status, _, _ = SC.model_witness(name)
    pb = zkp.RangeBatch(n_bits, B, ef, shared_key=shared)
    for b, n in enumerate(c["n_list"]):
        pb.n[b] = L.int_to_limbs(n, kw)
    for b, r in enumerate(c["ranges"]):
        pb.range[b] = L.int_to_limbs(r, kw)
    if c["device"]:
        import torch
        dpb = pb.to("cuda")
        out = [torch.from_numpy(np.full((B, ef, kw), 0xA5A5A5A5, np.uint32).view(np.int32)).cuda() for _ in WIT]      # (stale data: the MALFORMED rows must be written)
        st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.range_sample_witness(dpb.struct(), SEED, c["first_index"], *out, st, device=True)
        ctx.synchronize()
        got = [o.cpu().numpy().view(np.uint32) for o in out]
        status = st.cpu().numpy()
    else:
        got = [np.full((B, ef, kw), 0xA5A5A5A5, np.uint32) for _ in WIT]
        status = np.full(B, 9, np.uint8)
        ctx.range_sample_witness(pb.struct(), SEED, c["first_index"], *got, status, device=False)
    assert list(status) == want_status
    for f, g in zip(WIT, got):
        exp = M.to_limbs(want[f], kw)
        for b in range(B):
            assert np.array_equal(g[b], exp[b]), (name, f, b)
    for b in range(B):
        if want_status[b]:
            assert not any(g[b].any() for g in got), "a MALFORMED proof has a zero witness"


# ---- 2. the seeded prove against the witness-input prove and the oracle ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prove_case(n_bits, B, first_index, dishonest_last=True):
    n = H.fixture_key()[2] if n_bits == 2048 else H.test_key(n_bits)[2]
    cases = H.build_range_case(b"seeded-prove-%d-%d" % (n_bits, B), [n], n_bits, B)
    if dishonest_last:
        cases[-1] = H.build_range_case(b"seeded-prove-bad", [n], n_bits, 1, honest=False)[0]
    wit, status, _, _ = M.witness(SEED, first_index, [n], [c["range"] for c in cases], 128)
    assert not any(status)
    for b, c in enumerate(cases):
        for f in WIT:
            c[f] = wit[f][b]
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


@pytest.mark.parametrize("n_bits,B,first_index", [(2048, 3, 0), (1024, 4, (1 << 32) + 7)])
def test_seeded_prove_equals_prove_on_the_models_witness_and_the_oracle(ctx, oracle, n_bits, B, first_index):
    n, cases = prove_case(n_bits, B, first_index)
    pb_o, wt = H.fill_batch(cases, n_bits, True, oracle)
    eo = outs(B)
    oracle.range_ni_prove(pb_o.struct(), wt.struct(), *eo)
    pb_w, ew = fresh(pb_o), outs(B)
    ctx.range_ni_prove(pb_w.struct(), wt.struct(), *ew, device=False)
    pb_s, es = fresh(pb_o), outs(B)
    ctx.range_ni_prove_seeded(pb_s.struct(), wt.x, wt.r, SEED, first_index, *es, device=False)
    assert ctx.witness_residue() == 0
    assert_same(pb_w, pb_s, ew, es, "seeded against witness-input prove")
    assert_same(pb_o, pb_s, eo, es, "seeded against the oracle")
    v = np.full(B, 7, np.uint8)
    ctx.range_ni_verify(pb_s.struct(), v, device=False)
    assert list(v) == [zkp.VERDICT_ACCEPT] * (B - 1) + [zkp.VERDICT_REJECT]


def test_seeded_prove_with_device_pointers_and_its_residue(ctx, oracle):
    import torch
    n_bits, B = 1024, 4
    n, cases = prove_case(n_bits, B, (1 << 32) + 7)
    pb_o, wt = H.fill_batch(cases, n_bits, True, oracle)
    eo = outs(B)
    oracle.range_ni_prove(pb_o.struct(), wt.struct(), *eo)
    dpb = fresh(pb_o).to("cuda")
    dx, dr = torch.from_numpy(wt.x.view(np.int32)).cuda(), torch.from_numpy(wt.r.view(np.int32)).cuda()
    de, dl, ds = (torch.full(s, 7, dtype=torch.uint8, device="cuda") for s in ((B, 32), (B,), (B,)))
    torch.cuda.synchronize()
    ctx.range_ni_prove_seeded(dpb.struct(), dx, dr, SEED, (1 << 32) + 7, de, dl, ds, device=True)
    assert ctx.witness_residue() == 0
    ctx.synchronize()
    assert_same(pb_o, dpb.to(None), eo, (de.cpu().numpy(), dl.cpu().numpy(), ds.cpu().numpy()), "device pointers against the oracle")


@pytest.fixture(scope="module")
def actx():
    """nothing pinned: the library's own routing (the proof counts are those of tests/test_gpu_routing.py)"""
    c = zkp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("B", [2, 64, 136, 300])      # latency engine | mid engine | 128 + 8 as two concurrent calls | throughput engine
def test_seeded_prove_on_the_librarys_own_routes(actx, oracle, B):
    n_bits = 2048
    n, cases = prove_case(n_bits, B, 5, dishonest_last=False)
    oracle.set_threads(min(16, oracle.max_threads()))
    pb_o, wt = H.fill_batch(cases, n_bits, True, oracle)
    actx.set_geometry(0)
    actx.set_enc_form("auto")
    pb_w, ew = fresh(pb_o), outs(B)
    actx.range_ni_prove(pb_w.struct(), wt.struct(), *ew, device=False)
    route_w = (actx.last_geometry(), actx.last_split())
    pb_s, es = fresh(pb_o), outs(B)
    actx.range_ni_prove_seeded(pb_s.struct(), wt.x, wt.r, SEED, 5, *es, device=False)
    assert (actx.last_geometry(), actx.last_split()) == route_w, "the seeded call takes the route of the witness-input call"
    if B == 136:
        assert actx.last_split() > 0
    assert actx.witness_residue() == 0
    assert_same(pb_w, pb_s, ew, es, B)
    assert not es[2].any()
    # a sample of the batch against the oracle, byte for byte
    idx = sorted({0, 1, B // 2, B - 1})
    so = zkp.RangeBatch(n_bits, len(idx), 128, shared_key=True)
    so.n[:] = pb_o.n
    sw = zkp.make_range_witness(n_bits, len(idx))
    for k, b in enumerate(idx):
        so.range[k] = pb_o.range[b]; so.ciphertext[k] = pb_o.ciphertext[b]
        for f in ("x", "r") + WIT:
            getattr(sw, f)[k] = getattr(wt, f)[b]
    oracle.range_ni_prove(so.struct(), sw.struct(), None, None, None)
    for k, b in enumerate(idx):
        for f in OUT_FIELDS:
            assert np.array_equal(getattr(so, f)[k], getattr(pb_s, f)[b]), (B, b, f)
    v = np.full(B, 7, np.uint8)
    actx.range_ni_verify(pb_s.struct(), v, device=False)
    assert (v == zkp.VERDICT_ACCEPT).all()


# ---- 3. chunk invariance ---------------------------------------------------------------------------------------------------------------
def test_two_half_calls_and_two_contexts_equal_one_call(ctx, oracle):
    n_bits, B = 1024, 4
    n, cases = prove_case(n_bits, B, 0)
    pb_o, wt = H.fill_batch(cases, n_bits, True, oracle)
    one, e1 = fresh(pb_o), outs(B)
    ctx.range_ni_prove_seeded(one.struct(), wt.x, wt.r, SEED, 0, *e1, device=False)
    two, e2 = fresh(pb_o), outs(B)
    for lo in (0, B // 2):
        hi = lo + B // 2
        ctx.range_ni_prove_seeded(two.slice(lo, hi).struct(), wt.x[lo:hi], wt.r[lo:hi], SEED, lo, e2[0][lo:hi], e2[1][lo:hi], e2[2][lo:hi], device=False)
    assert_same(one, two, e1, e2, "two calls of B / 2 with first_index 0 and B / 2")
    m = zkp.MultiContext([0, 0])
    try:
        three, e3 = fresh(pb_o), outs(B)
        m.range_ni_prove_seeded(three.struct(), wt.x, wt.r, SEED, 0, *e3)
        assert [t[1:] for t in m.last_timing()] == [(0, B // 2), (B // 2, B)]
    finally:
        m.close()
    assert_same(one, three, e1, e3, "MultiContext([0, 0]), host gather")


# ---- 4. / 5. the wipe on an error path, refused arguments -----------------------------------------------------------------------------
def test_residue_after_an_error_part_way_and_refused_arguments(ctx, oracle):
    n_bits, B = 1024, 4
    n, cases = prove_case(n_bits, B, 0)
    pb_o, wt = H.fill_batch(cases, n_bits, True, oracle)
    pb = fresh(pb_o)
    with pytest.raises(zkp.ZkpError, match="status 1"):          # a null x is found by the prove step, after the sampler ran
        ctx.range_ni_prove_seeded(pb.struct(), None, wt.r, SEED, 0, None, None, None, device=False)
    assert ctx.witness_residue() == 0
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_ni_prove_seeded_batch"):
        ctx.range_ni_prove_seeded(pb.struct(), wt.x, wt.r, None, 0, None, None, None, device=False)
    wide = zkp.RangeBatch(n_bits, 1, 128, shared_key=True)
    wide.n[:] = pb.n; wide.range[:] = pb.range[:1]
    s = wide.struct()
    s.error_factor = 257
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_ni_prove_seeded_batch"):
        ctx.range_ni_prove_seeded(s, wt.x, wt.r, SEED, 0, None, None, None, device=False)
    w = [np.zeros((1, 257, n_bits // 32), np.uint32) for _ in WIT]
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_sample_witness_batch"):
        ctx.range_sample_witness(s, SEED, 0, *w, None, device=False)
    s.error_factor = 128
    with pytest.raises(zkp.ZkpError, match="status 1: zkp_range_sample_witness_batch"):
        ctx.range_sample_witness(s, None, 0, *w, None, device=False)


# ---- 6. the C++ host layer ---------------------------------------------------------------------------------------------------------------
def test_cpp_prove_batch_seeded_then_verify_batch():
    """tests/cpp/test_seeded.cpp, built and run the way tests/test_cpp_host.py builds test_zkproofs.cpp"""
    root, pkg = H.ROOT, os.path.join(H.ROOT, "zk-paillier_amd")
    src, exe = os.path.join(root, "tests", "cpp", "test_seeded.cpp"), os.path.join(root, "build", "test_seeded")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", exe, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 1 and "FAIL" not in out.stdout, out.stdout + out.stderr
