"""The range proofs at row counts other than 128, on every path the library routes them to.

Everything that decides how a RangeProof call runs is a function of its items, 2 per row (csrc/route_plan.hpp), and every kernel behind
those decisions turns a flat row index back into (proof, row) by the error factor.  The other GPU files hold all of that at 128 rows per
proof, where a 256-thread block of k_verify_plan never holds rows of two proofs and the windows of range_split divide evenly.  This file
lets the library choose (nothing pinned) at 1, 7, 40, 120 and 256 rows per proof, at batch sizes taken from tests/routing_model.py for
the device — the smallest batch of every kernel family, one batch inside every window in which a verify is cut in two — and checks against
the C/GMP oracle on samples, against the other form's bytes on the whole batch, and with tampered rows on both sides of a proof boundary
that falls inside a wavefront.

What "prove" is here.  zkp_range_ni_prove_batch always writes ZKP_SECURITY_PARAMETER = 128 rows, whatever error factor the struct holds
(include/zkp_hip.h; RangeProofNi::prove of the reference does the same), so a proof of another row count is made by the three entry points
the reference's benchmark uses at 40 rows: generate_encrypted_pairs — the Enc launch, routed by its items and never cut —, the
Fiat-Shamir challenge, generate_proof.  That composition, challenge included, is what `prove` below runs and what is compared with the
oracle's; range_ni_verify takes the row count of the struct and is the call that is cut.

Which windows exist.  At 40 rows and 256 compute units a verify is cut at 52 ... 64 proofs (4 ... 5 items per SIMD: the head on the latency
engine's window ladder) and at 263 ... 307 (16 ... 24 per SIMD: the head on the mid engine).  The window in between, 8 ... 9 items per SIMD
(103 ... 115 proofs), cuts a prove of 128 rows only: a verify of that size fits the latency engine's one round by its EXPECTED items and
runs as one call, as 33 ... 36 proofs do at 128 rows; one batch inside it pins that."""
import os

import numpy as np
import pytest

import helpers as H
import routing_model as R
import small_proof_cases as S
from helpers import pm, L, zkp
from test_gpu_routing import FIELDS, compute_units, family_that_ran, sub_batch

pytestmark = pytest.mark.gpu

N_BITS, KW = 2048, 64
ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED
WIT_FIELDS = ("x", "r", "w1", "w2", "r1", "r2")


@pytest.fixture(scope="module")
def actx():
    assert "ZKP_BASEN" not in os.environ, "this file tests the library's default routing: unset ZKP_BASEN"
    c = zkp.Context(0)
    assert c.enc_form() == zkp.capi.ENC_FORM_AUTO
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------- sizes, from the model
def engines(c):
    return c.latency_limbs_per_lane(), c.mid_limbs_per_lane()


def model(c, ef, B, verify):
    """(family, tail) tests/routing_model.py expects for B proofs of ef rows: a verify is range_ni_verify, a prove generate_encrypted_pairs"""
    lat, mid = engines(c)
    fam = R.expected_family(compute_units(), lat, mid, 2 * ef * B, listed=verify, rows_per_proof=2 * ef, never_split=not verify)
    return fam, (R.expected_tail(compute_units(), B, 2 * ef, True) if fam == "split" else 0)


def last_batch(ef):
    return 48 * 4 * compute_units() // (2 * ef) + 1          # the first batch beyond 48 items per SIMD: no rule looks at the size from there on


def smallest(c, ef, families, verify=False):
    for B in range(1, last_batch(ef) + 1):
        if model(c, ef, B, verify)[0] in families:
            return B
    raise AssertionError("the model places no batch of %d rows in %s" % (ef, families))


def verify_windows(c, ef):
    """[(first, last)] of the runs of batch sizes whose verify the model cuts in two"""
    runs = []
    for B in range(1, last_batch(ef) + 1):
        if model(c, ef, B, True)[0] == "split":
            if runs and runs[-1][1] == B - 1:
                runs[-1][1] = B
            else:
                runs.append([B, B])
    return runs


def inside(window):
    return (window[0] + window[1] + 1) // 2


A_LABELS = ("r2l5", "lat-r2l", "lat-n2", "lat-basen", "mid-basen", "base-n", "window-4", "window-8", "window-16")


def size_a(c, label):
    """the batch sizes of part (a) at 40 rows — on 256 compute units 3, 4, 26, 52, 129, 308, 58, 109 and 285 proofs"""
    cus, ef = compute_units(), 40
    if label == "r2l5":                                       # the largest call that leaves every Enc a compute unit: five wavefronts per Enc
        return max(1, cus // (2 * ef))
    if label == "lat-r2l":                                    # ... and the first beyond: one wavefront per Enc
        return max(1, cus // (2 * ef)) + 1
    if label == "window-8":                                   # 8 ... 9 items per SIMD: where a prove of 128 rows is cut and no call of another row count is
        return (17 * 4 * cus // 2) // (2 * ef)
    if label.startswith("window-"):
        per_simd = int(label[7:])
        w = [w for w in verify_windows(c, ef) if R.expected_split(cus, w[0], 2 * ef, True)[2] == per_simd]
        assert len(w) == 1, (label, verify_windows(c, ef))
        return inside(w[0])
    return smallest(c, ef, (label,))


# ---------------------------------------------------------------------------------------------------------------- inputs, once per module
_POOL = {}
POOL_PROOFS = {1: lambda: 4 * compute_units() + 1, 7: lambda: 150, 256: lambda: 10}


def pool(oracle, c, ef):
    """(RangeBatch with n, range, ciphertext; witness; the python-int cases) of the most proofs any test of this file asks for at `ef` rows —
    every test takes the FIRST B of them (proofs are independent), so each row count is built once"""
    if ef not in _POOL:
        if ef == 40:
            B = max(size_a(c, label) for label in A_LABELS)
        elif ef == 120:
            B = inside(verify_windows(c, ef)[0])
        else:
            B = POOL_PROOFS[ef]()
        oracle.set_threads(min(16, oracle.max_threads()))
        cases = H.build_range_case(b"error-factor-%d" % ef, [H.fixture_key()[2]], N_BITS, B, ef=ef)
        pb, wt = H.fill_batch(cases, N_BITS, True, oracle)
        _POOL[ef] = (pb, wt, cases)
    return _POOL[ef]


def first_proofs(pb0, wt0, B):
    """a fresh batch over the statements of the first B proofs of the pool (outputs marked: a row no kernel writes differs from the oracle's) and their witness"""
    assert B <= pb0.batch
    pb = zkp.RangeBatch(N_BITS, B, pb0.ef, shared_key=True)
    pb.n[:] = pb0.n; pb.range[:] = pb0.range[:B]; pb.ciphertext[:] = pb0.ciphertext[:B]
    for f in FIELDS:
        getattr(pb, f)[:] = 0xA5
    return pb, wt0.slice(0, B)


def sub_witness(wt, idx, ef, n_bits=N_BITS):
    sw = zkp.make_range_witness(n_bits, len(idx), ef)
    for k, b in enumerate(idx):
        for f in WIT_FIELDS:
            getattr(sw, f)[k] = getattr(wt, f)[b]
    return sw


def reset_last_split(c, pb):
    """zkp_diag_last_split is set by range_ni_prove / range_ni_verify alone: a verify of no rows in front of an interactive call sets it to 0,
    so that a cut of THAT call would show"""
    z = zkp.RangeBatch(pb.n_bits, 1, 0, shared_key=True)
    z.n[:] = pb.n[:1]
    v = np.full(1, 9, np.uint8)
    c.range_ni_verify(z.struct(), v, device=False)
    assert c.last_split() == 0 and v[0] == ACCEPT


def prove(c, pb, wt):
    """RangeProofNi::prove at pb.ef rows: generate_encrypted_pairs; the Fiat-Shamir challenge; generate_proof
    -> (e, e_len, status, family of the Enc launch, lanes of its one-Enc-per-wavefront ladder or 0)"""
    B = pb.batch
    e = np.zeros((B, 32), np.uint8); elen = np.zeros(B, np.uint8); st = np.full(B, 9, np.uint8)
    reset_last_split(c, pb)
    c.range_generate_encrypted_pairs(pb.struct(), wt.struct(), device=False)
    fam, lanes = family_that_ran(c), c.r2l_lanes_last()
    c.range_challenge(pb.struct(), e, elen, device=False)
    c.range_generate_proof(pb.struct(), wt.struct(), e, elen, st, device=False)
    return e, elen, st, fam, lanes


def oracle_prove(oracle, pb, wt, idx, e=None, elen=None):
    """the same composition by the oracle for the proofs `idx` -> (their batch, e, e_len, status); e given: generate_proof under that challenge"""
    so, sw = sub_batch(pb, idx, pb.n_bits), sub_witness(wt, idx, pb.ef, pb.n_bits)
    oracle.range_generate_encrypted_pairs(so.struct(), sw.struct())
    if e is None:
        e = np.zeros((len(idx), 32), np.uint8); elen = np.zeros(len(idx), np.uint8)
        for k in range(len(idx)):
            d = oracle.fs_challenge(pb.n_bits, pb.ef, so.n[0], so.c1[k], so.c2[k])
            e[k, :len(d)] = np.frombuffer(d, np.uint8); elen[k] = len(d)
    else:
        e, elen = np.ascontiguousarray(e[idx]), np.ascontiguousarray(elen[idx])
    st = np.full(len(idx), 9, np.uint8)
    oracle.range_generate_proof(so.struct(), sw.struct(), e, elen, st)
    return so, e, elen, st


def sample_of(B, most, extra=()):
    """first, second, B/3, B/2, the last two — and `extra` in front when the sample has room for them"""
    base = [0, 1, B // 3, B // 2, B - 2, B - 1]
    out = []
    for b in list(extra) + base:
        if 0 <= b < B and b not in out and len(out) < most:
            out.append(b)
    return sorted(out)


def check_prove(c, oracle, pb0, wt0, B, most=6, extra=()):
    """prove the first B proofs under default routing: the family of the model, never cut, a sample byte for byte against the oracle, the whole
    batch against the other form on the throughput engine -> the proved batch"""
    ef = pb0.ef
    pb, wt = first_proofs(pb0, wt0, B)
    c.set_geometry(0); c.set_enc_form("auto")
    e, elen, st, fam, lanes = prove(c, pb, wt)
    want = model(c, ef, B, False)[0]
    assert want != "split" and c.last_split() == 0, (ef, B)                  # (today's rule: only a prove of 128 rows is cut)
    assert fam == want, (ef, B, fam, want)
    if want == "lat-r2l":
        assert lanes == (36 if 2 * ef * B <= compute_units() else 12), (ef, B, lanes)
    assert not st.any(), (ef, B, np.nonzero(st)[0][:8])
    idx = sample_of(B, most, extra)
    so, eo, elo, sto = oracle_prove(oracle, pb, wt, idx)
    assert not sto.any()
    for k, b in enumerate(idx):
        assert elen[b] == elo[k] and np.array_equal(e[b], eo[k]), (ef, B, b, "challenge")
        for f in FIELDS:
            assert np.array_equal(getattr(so, f)[k], getattr(pb, f)[b]), (ef, B, b, f)
    # the whole batch against other kernels: the throughput engine's n^2-sized ones (its base-n ones when those were the choice)
    other, _ = first_proofs(pb0, wt0, B)
    try:
        c.set_geometry(zkp.load().zkp_build_limbs_per_lane())
        c.set_enc_form("basen" if want == "n2" else "n2")
        e2, elen2, st2, fam2, _ = prove(c, other, wt)
        assert fam2 == ("base-n" if want == "n2" else "n2"), (ef, B, fam2)
    finally:
        c.set_geometry(0); c.set_enc_form("auto")
    assert np.array_equal(e, e2) and np.array_equal(elen, elen2) and np.array_equal(st, st2)
    for f in FIELDS:
        S.assert_same(getattr(other, f), getattr(pb, f), (ef, B, f))
    return pb


EDITS = ("resp_r1", "c2", "resp_w1")


def edit_row(pb, b, row, k):
    """one of three edits of one row of proof b: a response's randomness, a commitment (the challenge changes with it), a response's value"""
    f = EDITS[k % 3]
    if f == "resp_r1":
        pb.resp_r1[b, row, 0] ^= 1
    elif f == "c2":
        pb.c2[b, row, 7] ^= 0x10
    else:
        pb.resp_w1[b, row, 1] ^= 2


def boundary_edits(B, ef, near, taken=()):
    """[(proof, row)] — for each b of `near` (moved up to the next b whose first row shares a 64-thread wavefront of k_verify_plan with the last
    row of proof b - 1: ef * b % 64 != 0) alternately row 0 of proof b and the last row of proof b - 1; no two edited proofs are neighbours"""
    out, used = [], set(taken)
    for k, b in enumerate(near):
        while b < B and (ef * b % 64 == 0 or b < 1 or {b - 2, b - 1, b, b + 1} & used):
            b += 1
        if b >= B:
            continue
        t = (b, 0) if k % 2 == 0 else (b - 1, ef - 1)
        if {t[0] - 1, t[0] + 1} & used:
            continue
        out.append(t)
        used.add(t[0])
    return out


def check_verify(c, oracle, pb, edits, sample, kinds=None):
    """range_ni_verify under default routing of a batch with the rows `edits` tampered: the family and the tail of the model, REJECT exactly at the
    edited proofs, and the oracle's verdicts on the sample and on the edited proofs"""
    B, ef = pb.batch, pb.ef
    for k, (b, row) in enumerate(edits):
        edit_row(pb, b, row, kinds[k] if kinds else k)
    bad = sorted({b for b, _ in edits})
    c.set_geometry(0); c.set_enc_form("auto")
    v = np.full(B, 9, np.uint8)
    c.range_ni_verify(pb.struct(), v, device=False)
    want, tail = model(c, ef, B, True)
    assert family_that_ran(c) == want, (ef, B, "verify", family_that_ran(c), want)
    assert c.last_split() == tail, (ef, B, c.last_split(), tail)
    expect = np.full(B, ACCEPT, np.uint8); expect[bad] = REJECT
    S.assert_same(expect, v, (ef, B, "verdicts", edits))
    vidx = sorted(set(sample) | set(bad))
    sv = sub_batch(pb, vidx, pb.n_bits)                      # (kept alive across the call: struct() holds raw pointers into its arrays)
    vo = np.full(len(vidx), 9, np.uint8)
    oracle.range_ni_verify(sv.struct(), vo)
    assert list(vo) == [int(v[b]) for b in vidx], (ef, B, vidx)
    return want, tail


# ---------------------------------------------------------------------------------------------------------------- (a) 40 rows, every family
def test_the_sizes_of_the_model_reach_every_family_and_both_verify_windows(actx):
    """the sizes the next test runs, by the model alone: between prove and verify they name every family the library can choose, and a verify
    inside each of its two windows (the head on the latency engine's window ladder | on the mid engine); the next test holds the device
    to the model at each of them"""
    if engines(actx) != (9, 18):
        pytest.fail("both secondary engines belong to a build: libzkp_hip_lat.so / libzkp_hip_mid.so are not loaded")
    cus, seen, heads = compute_units(), set(), set()
    sizes = [size_a(actx, label) for label in A_LABELS]
    assert len(set(sizes)) == len(sizes) and max(sizes) <= last_batch(40), sizes
    for B in sizes:
        seen.add(model(actx, 40, B, False)[0])
        fam, tail = model(actx, 40, B, True)
        seen.add(fam)
        if fam == "split":
            assert 0 < tail < B
            heads.add(R.expected_split(cus, B, 80, True)[1:])
    assert {"lat-r2l", "lat-n2", "lat-basen", "mid-basen", "base-n", "split"} <= seen, seen
    assert heads == {("lat", 4), ("mid", 16)}, heads
    B8 = size_a(actx, "window-8")
    assert 8 * 4 * cus < 80 * B8 <= 9 * 4 * cus and model(actx, 40, B8, True)[0] == "lat-basen" and model(actx, 40, B8, False)[0] == "lat-basen"
    assert R.expected_split(cus, B8, 80, False) is not None and R.expected_split(cus, B8, 80, True) is None      # (the window itself: a prove that asks — one of 128 rows)


@pytest.mark.parametrize("label", A_LABELS)
def test_40_rows_on_every_family(actx, oracle, label):
    ef = 40
    pb0, wt0, _ = pool(oracle, actx, ef)
    B = size_a(actx, label)
    cut = R.expected_split(compute_units(), B, 2 * ef, True) if model(actx, ef, B, True)[0] == "split" else None
    head = cut[0] if cut else None
    pb = check_prove(actx, oracle, pb0, wt0, B, most=6, extra=(head, B - 1) if cut else ())
    # one proof on each side of the cut, then three pairs whose boundary lies inside a wavefront of the plan kernel
    edits = [(head - 1, ef - 1), (head, 0)] if cut and head >= 2 else []
    edits += boundary_edits(B, ef, [max(1, B // 4), B // 2 + 1, B - 1], taken=[b for b, _ in edits])
    if B > 2:
        assert edits and all(ef * (b + (1 if row else 0)) % 64 for b, row in edits[2 if cut else 0:]), edits
    want, tail = check_verify(actx, oracle, pb, edits, sample_of(B, 6, (head, B - 1) if cut else ()))
    if label.startswith("window-") and label != "window-8":
        assert want == "split" and tail == B - head
    elif label not in ("r2l5", "window-8"):
        assert label in (want, model(actx, ef, B, False)[0])


# ---------------------------------------------------------------------------------------------------------------- (b) the composition
def sizes_b(c):
    """128 rows, the one row count range_ni_prove writes: the first prove the model cuts with its head on the mid engine, the first it sends there whole"""
    cus = compute_units()
    cut = next(B for B in range(1, last_batch(128) + 1) if (R.expected_split(cus, B, 256, False) or (0, ""))[1] == "mid")
    lat, mid = engines(c)
    whole = next(B for B in range(1, last_batch(128) + 1) if R.expected_family(cus, lat, mid, 256 * B) == "mid-basen")
    return {"split": cut, "mid-basen": whole}


@pytest.mark.parametrize("which", ["split", "mid-basen"])
def test_the_composition_equals_range_ni_prove_at_128_rows(actx, oracle, which):
    """generate_encrypted_pairs; range_challenge; generate_proof — the prove of every other test of this file — gives the bytes of
    range_ni_prove on the same inputs, at a size where that call is cut in two and at one it runs whole on the mid engine: GPU against GPU"""
    sizes = sizes_b(actx)
    if 128 not in _POOL:
        oracle.set_threads(min(16, oracle.max_threads()))
        cases = H.build_range_case(b"error-factor-128", [H.fixture_key()[2]], N_BITS, max(sizes.values()))
        _POOL[128] = H.fill_batch(cases, N_BITS, True, oracle) + (cases,)
    pb0, wt0, _ = _POOL[128]
    B = sizes[which]
    pa, wt = first_proofs(pb0, wt0, B)
    actx.set_geometry(0); actx.set_enc_form("auto")
    ea = np.zeros((B, 32), np.uint8); la = np.zeros(B, np.uint8); sa = np.full(B, 9, np.uint8)
    actx.range_ni_prove(pa.struct(), wt.struct(), ea, la, sa, device=False)
    assert family_that_ran(actx) == which, (B, family_that_ran(actx))
    if which == "split":
        assert actx.last_split() == R.expected_tail(compute_units(), B)
    pc, _ = first_proofs(pb0, wt0, B)
    ec, lc, sc, fam, _ = prove(actx, pc, wt)
    assert actx.last_split() == 0 and fam != "split"
    assert not sa.any() and not sc.any()
    S.assert_same(ea, ec, "challenge"); S.assert_same(la, lc, "challenge length")
    for f in FIELDS:
        S.assert_same(getattr(pa, f), getattr(pc, f), (which, B, f))


# ---------------------------------------------------------------------------------------------------------------- (c) the interactive verifier
def challenges(pattern, B, ef, seed):
    nbytes = (ef + 7) // 8
    e = np.zeros((B, 32), np.uint8); elen = np.full(B, nbytes, np.uint8)
    if pattern == "random":
        d = pm.Drbg(seed)
        for b in range(B):
            e[b, :nbytes] = np.frombuffer(d.bytes(nbytes), np.uint8)
    elif pattern == "ones":
        e[:, :nbytes] = 0xFF
    return e, elen


@pytest.mark.parametrize("pattern", ["random", "zeros", "ones"])
@pytest.mark.parametrize("label", ["window-16", "mid-basen"])
def test_interactive_verifier_at_routed_sizes(actx, oracle, label, pattern):
    """generate_proof and verifier_output under challenges the CALLER chooses, at two routed sizes: all bits zero makes every row an Open row — the
    work list of the verify reaches its bound of 2 Enc per row, a third more than the items its grid was sized for —, all bits one every row a
    Mask row, half the bound.  One proof has a challenge one byte short (MALFORMED on both sides), one dishonest proof sits in the last
    wavefront's worth of rows (with every row Open nothing looks at x: the oracle accepts it there, and so must the library)."""
    ef = 40
    pb0, wt0, cases = pool(oracle, actx, ef)
    B = size_a(actx, label)
    short, crook = B // 2 + 1, B - 1
    pb, wt_view = first_proofs(pb0, wt0, B)
    wt = sub_witness(wt_view, range(B), ef)                  # (a copy: the pool stays as it is)
    x_bad = 100 * cases[crook]["range"] + 12345              # far outside the range (range_proof_ni.rs:184-187)
    wt.x[crook] = L.int_to_limbs(x_bad, KW)
    pb.ciphertext[crook] = oracle.paillier_enc(N_BITS, pb.n, KW, wt.x[crook:crook + 1], wt.r[crook:crook + 1])[0]
    e, elen = challenges(pattern, B, ef, b"interactive-%s-%d" % (label.encode(), ef))
    elen[short] -= 1
    actx.set_geometry(0); actx.set_enc_form("auto")
    reset_last_split(actx, pb)
    actx.range_generate_encrypted_pairs(pb.struct(), wt.struct(), device=False)
    st = np.full(B, 9, np.uint8)
    actx.range_generate_proof(pb.struct(), wt.struct(), e, elen, st, device=False)
    expect_st = np.zeros(B, np.uint8); expect_st[short] = MALFORMED
    S.assert_same(expect_st, st, (label, pattern, "status"))
    kinds = set(np.unique(np.delete(pb.resp_kind, short, axis=0)))
    assert kinds == {"random": {zkp.RESP_OPEN, zkp.RESP_MASK}, "zeros": {zkp.RESP_OPEN}, "ones": {zkp.RESP_MASK}}[pattern], kinds
    # the oracle on the sample, the short and the dishonest proof: the same rows, the same status
    idx = sample_of(B, 6, (short, crook))
    so, _, _, sto = oracle_prove(oracle, pb, wt, idx, e, elen)
    assert list(sto) == [int(st[b]) for b in idx]
    for k, b in enumerate(idx):
        if b == short:                                       # the reference panics in generate_proof: what either side leaves behind is unspecified — the same content for both
            for f in FIELDS[2:]:
                getattr(so, f)[k] = 0; getattr(pb, f)[b] = 0
        for f in FIELDS:
            assert np.array_equal(getattr(so, f)[k], getattr(pb, f)[b]), (label, pattern, b, f)
    v = np.full(B, 9, np.uint8)
    actx.range_verifier_output(pb.struct(), e, elen, v, device=False)
    assert actx.last_split() == 0                            # (the interactive entry points never cut a call)
    ran = family_that_ran(actx)
    vo = np.full(len(idx), 9, np.uint8)
    oracle.range_verifier_output(so.struct(), np.ascontiguousarray(e[idx]), np.ascontiguousarray(elen[idx]), vo)
    assert list(vo) == [int(v[b]) for b in idx], (label, pattern, idx, list(vo))
    assert v[short] == MALFORMED and v[crook] == (ACCEPT if pattern == "zeros" else REJECT)
    expect = np.full(B, ACCEPT, np.uint8); expect[short] = MALFORMED; expect[crook] = vo[idx.index(crook)]
    S.assert_same(expect, v, (label, pattern, "verdicts", ran))
    # the whole vector against the throughput engine's n^2-sized kernels
    try:
        actx.set_geometry(zkp.load().zkp_build_limbs_per_lane()); actx.set_enc_form("n2")
        v2 = np.full(B, 9, np.uint8)
        actx.range_verifier_output(pb.struct(), e, elen, v2, device=False)
        assert family_that_ran(actx) == "n2" and ran != "n2"
    finally:
        actx.set_geometry(0); actx.set_enc_form("auto")
    S.assert_same(v2, v, (label, pattern, "pinned"))


# ---------------------------------------------------------------------------------------------------------------- (d) other error factors
def sizes_d(c, ef):
    cus = compute_units()
    if ef == 1:      # 64 proofs per wavefront of the plan kernel: the largest verify that takes its hashes aboard (far more of them than Enc workgroups) | just past two items per SIMD
        return [cus - 1, 4 * cus + 1]
    if ef == 7:      # 1050 rows: no multiple of 64, five blocks of the plan kernel
        return [150]
    if ef == 120:    # a verify inside its first window
        return [inside(verify_windows(c, ef)[0])]
    # 256 rows: the last challenge bit decides a row; 2 proofs | the smallest batch on 8 Enc per wavefront (or the mid engine), whose verify is cut
    return [2, smallest(c, ef, ("lat-basen", "mid-basen"))]


@pytest.mark.parametrize("ef,k", [(1, 0), (1, 1), (7, 0), (120, 0), (256, 0), (256, 1)])
def test_other_error_factors(actx, oracle, ef, k):
    pb0, wt0, _ = pool(oracle, actx, ef)
    B = sizes_d(actx, ef)[k]
    pb = check_prove(actx, oracle, pb0, wt0, B, most=4)
    if ef == 7:
        assert (ef * B) % 64 and ef * B > 4 * 256
    if ef in (120, 256) and B > 2:
        assert model(actx, ef, B, True)[0] == "split", (ef, B)
    # the first and the last row of the batch, and the boundaries inside a wavefront in between
    edits = [(B - 1, ef - 1), (0, 0)]
    edits += boundary_edits(B, ef, [B // 3, 2 * B // 3], taken=[0, B - 1])
    kinds = None
    if ef == 1:      # one row per proof: both sides of a wavefront of 64 proofs; responses only (a one-row transcript keeps its challenge bit every other time)
        edits = [(b, 0) for b in (0, 62, 64, 127, B - 1) if b < B]
        kinds = [0, 2, 0, 2, 0]
    want, tail = check_verify(actx, oracle, pb, edits, sample_of(B, 4), kinds)
    if ef == 1 and k == 0:
        assert want == "lat-r2l" and actx.last_fused_hash()


def test_the_last_challenge_bit_decides_a_row(actx, oracle):
    """256 rows: bit 255 of the challenge — bit 0 of byte 31 — belongs to the last row.  Proofs made under a caller's challenge verify under it
    and are rejected once that one bit is flipped (the response kind of row 255 no longer matches): the first and the last proof of the batch"""
    ef = 256
    pb0, wt0, _ = pool(oracle, actx, ef)
    B = sizes_d(actx, ef)[1]
    pb, wt = first_proofs(pb0, wt0, B)
    e, elen = challenges("random", B, ef, b"bit-255")
    assert (elen == 32).all()
    actx.set_geometry(0); actx.set_enc_form("auto")
    actx.range_generate_encrypted_pairs(pb.struct(), wt.struct(), device=False)
    st = np.full(B, 9, np.uint8)
    actx.range_generate_proof(pb.struct(), wt.struct(), e, elen, st, device=False)
    assert not st.any()
    flipped = [0, B - 1]
    e2 = e.copy()
    for b in flipped:
        e2[b, 31] ^= 1
    for ee, bad in ((e, []), (e2, flipped)):
        v = np.full(B, 9, np.uint8)
        actx.range_verifier_output(pb.struct(), ee, elen, v, device=False)
        idx = [0, 1, B - 1]
        sv = sub_batch(pb, idx, N_BITS)
        vo = np.full(len(idx), 9, np.uint8)
        oracle.range_verifier_output(sv.struct(), np.ascontiguousarray(ee[idx]), np.ascontiguousarray(elen[idx]), vo)
        expect = np.full(B, ACCEPT, np.uint8); expect[bad] = REJECT
        assert list(vo) == [int(expect[b]) for b in idx] and list(v) == list(expect), (bad, list(v), list(vo))


# ---------------------------------------------------------------------------------------------------------------- (e) per-proof keys
def test_per_proof_keys_at_40_rows(actx, oracle):
    """about 70 proofs under three 2048-bit keys in turn — the key-partition path of the base-n launch — and one proof under a key the form does
    not take (a short one): its items go to the n^2-sized launch behind.  Prove and verify against the oracle on a sample, the whole batch
    against the n^2-sized form on the throughput engine."""
    import importlib
    synth = importlib.import_module("zk-paillier_amd.synth")
    ef, B, outside = 40, 70, 37
    three = synth.distinct_keys_2048(3)
    keys = [three[b % 3] for b in range(B)]
    keys[outside] = H.test_key(1000, tag=1)[2]
    oracle.set_threads(min(16, oracle.max_threads()))
    cases = H.build_range_case(b"error-factor-keys", keys, N_BITS, B, shared=False, ef=ef)
    pb, wt = H.fill_batch(cases, N_BITS, False, oracle)

    def run(form, geometry):
        q = zkp.RangeBatch(N_BITS, B, ef, shared_key=False)
        q.n[:] = pb.n; q.range[:] = pb.range; q.ciphertext[:] = pb.ciphertext
        actx.set_geometry(geometry); actx.set_enc_form(form)
        e, elen, st, _, _ = prove(actx, q, wt)
        assert not st.any()
        return q, e, elen

    def some(src, idx, with_rows):
        s = zkp.RangeBatch(N_BITS, len(idx), ef, shared_key=False)
        for k, b in enumerate(idx):
            for f in ("n", "range", "ciphertext") + (FIELDS if with_rows else ()):
                getattr(s, f)[k] = getattr(src, f)[b]
        return s

    try:
        got, e, elen = run("auto", 0)
        other, e2, elen2 = run("n2", zkp.load().zkp_build_limbs_per_lane())
        assert np.array_equal(e, e2) and np.array_equal(elen, elen2)
        for f in FIELDS:
            S.assert_same(getattr(other, f), getattr(got, f), f)
        idx = sample_of(B, 5, (outside,))
        so, sw = some(pb, idx, False), sub_witness(wt, idx, ef)
        oracle.range_generate_encrypted_pairs(so.struct(), sw.struct())
        eo = np.zeros((len(idx), 32), np.uint8); elo = np.zeros(len(idx), np.uint8)
        for k in range(len(idx)):
            d = oracle.fs_challenge(N_BITS, ef, so.n[k], so.c1[k], so.c2[k])
            eo[k, :len(d)] = np.frombuffer(d, np.uint8); elo[k] = len(d)
        sto = np.full(len(idx), 9, np.uint8)
        oracle.range_generate_proof(so.struct(), sw.struct(), eo, elo, sto)
        assert not sto.any()
        for k, b in enumerate(idx):
            assert elen[b] == elo[k] and np.array_equal(e[b], eo[k]), (b, "challenge")
            for f in FIELDS:
                assert np.array_equal(getattr(so, f)[k], getattr(got, f)[b]), (b, f)
        # verify: rows tampered on both sides of boundaries inside a wavefront, the short-key proof among the edited ones
        edits = [(outside, ef - 1)] + boundary_edits(B, ef, [B // 4, B // 2 + 5, B - 1], taken=[outside])
        for k, (b, row) in enumerate(edits):
            edit_row(got, b, row, k)
        bad = sorted({b for b, _ in edits})
        expect = np.full(B, ACCEPT, np.uint8); expect[bad] = REJECT
        for form, geometry in (("auto", 0), ("n2", zkp.load().zkp_build_limbs_per_lane())):
            actx.set_geometry(geometry); actx.set_enc_form(form)
            v = np.full(B, 9, np.uint8)
            actx.range_ni_verify(got.struct(), v, device=False)
            assert actx.last_split() == 0                    # (per-proof keys: never cut)
            S.assert_same(expect, v, (form, "verdicts"))
        vidx = sorted(set(idx) | set(bad))
        sv = some(got, vidx, True)
        vo = np.full(len(vidx), 9, np.uint8)
        oracle.range_ni_verify(sv.struct(), vo)
        assert list(vo) == [int(expect[b]) for b in vidx]
    finally:
        actx.set_geometry(0); actx.set_enc_form("auto")


# ---------------------------------------------------------------------------------------------------------------- (f) pinned families, whole batch
def wide_7_rows(oracle):
    """300 proofs of 7 rows at n = 1024 under one key — 2100 rows: nine 256-thread blocks of the plan kernel, the last one partial, and a
    GROUPS_PER_BLOCK tail of the response kernel —, dishonest proofs at small_proof_cases.marked(300), and the oracle's whole transcript and
    verdicts, honest and with tampered rows"""
    n_bits, B, ef = 1024, 300, 7
    n = H.test_key(1024)[2]
    oracle.set_threads(min(16, oracle.max_threads()))
    cases = H.build_range_case(b"wide-7-rows", [n], n_bits, B, ef=ef)
    crooks = S.marked(B)
    for b, bad in zip(crooks, H.build_range_case(b"wide-7-rows-bad", [n], n_bits, len(crooks), honest=False, ef=ef)):
        cases[b] = bad
    pb, wt = H.fill_batch(cases, n_bits, True, oracle)
    oracle.range_generate_encrypted_pairs(pb.struct(), wt.struct())
    e = np.zeros((B, 32), np.uint8); elen = np.zeros(B, np.uint8)
    for b in range(B):
        d = oracle.fs_challenge(n_bits, ef, pb.n[0], pb.c1[b], pb.c2[b])
        e[b, :len(d)] = np.frombuffer(d, np.uint8); elen[b] = len(d)
    st = np.full(B, 9, np.uint8)
    oracle.range_generate_proof(pb.struct(), wt.struct(), e, elen, st)
    v = np.full(B, 9, np.uint8)
    oracle.range_ni_verify(pb.struct(), v)
    # rows tampered on both sides of boundaries inside a wavefront (7 b % 64 != 0) and of the 256-thread blocks (rows 255 | 256: proof 36, rows 3 | 4)
    edits = [(36, 3), (37, 0), (72, 6), (109, 6), (110, 0), (145, 6), (183, 0), (B - 1, 6)]
    tampered = zkp.RangeBatch(n_bits, B, ef, shared_key=True)
    for f in ("n", "range", "ciphertext") + FIELDS:
        getattr(tampered, f)[:] = getattr(pb, f)
    for k, (b, row) in enumerate(edits):
        edit_row(tampered, b, row, k)
    vt = np.full(B, 9, np.uint8)
    oracle.range_ni_verify(tampered.struct(), vt)
    return dict(pb=pb, wt=wt, e=e, elen=elen, st=st, v=v, crooks=crooks, edits=edits, tampered=tampered, vt=vt)


def test_pinned_families_whole_batch_at_7_rows(ctx, oracle):
    cs = S.cached("wide-7-rows", lambda: wide_7_rows(oracle))
    po, wt, B = cs["pb"], cs["wt"], cs["pb"].batch
    # the oracle's own vectors: honest proofs accepted, dishonest ones rejected unless every one of their 7 rows is an Open row
    assert not cs["st"].any()
    open_only = [b for b in cs["crooks"] if (po.resp_kind[b] == zkp.RESP_OPEN).all()]
    assert [int(x) for x in cs["v"]] == [REJECT if b in cs["crooks"] and b not in open_only else ACCEPT for b in range(B)]
    assert len(open_only) < len(cs["crooks"]) // 2
    edited = {b for b, _ in cs["edits"]}
    assert [int(x) for x in cs["vt"]] == [REJECT if (b in edited or cs["v"][b] == REJECT) else ACCEPT for b in range(B)]
    pg = zkp.RangeBatch(po.n_bits, B, po.ef, shared_key=True)
    pg.n[:] = po.n; pg.range[:] = po.range; pg.ciphertext[:] = po.ciphertext
    for f in FIELDS:
        getattr(pg, f)[:] = 0xA5
    e, elen, st, _, _ = prove(ctx, pg, wt)
    S.assert_same(cs["st"], st, "status")
    S.assert_same(cs["e"], e, "challenge")
    S.assert_same(cs["elen"], elen, "challenge length")
    for f in FIELDS:
        S.assert_same(getattr(po, f), getattr(pg, f), f)
    for batch, want in ((pg, cs["v"]), (cs["tampered"], cs["vt"])):
        v = np.full(B, 9, np.uint8)
        ctx.range_ni_verify(batch.struct(), v, device=False)
        S.assert_same(want, v, "verdicts")
