"""RangeProofNi verify of crafted proofs (tests/crafted_range.py) on every path the library routes a verify to.

Two things no honest-shaped batch exercises:
  * the binding of a row's response kind to its challenge bit (range_proof.rs:270-348, the `_ => false` arm): a crafted row passes its
    Enc checks and its range predicate, only the bit rejects it (flip_*, all_open, all_mask);
  * a work list longer than the launch was sized for.  Routing and grids of a verify are judged by expected_items() — three quarters
    of the bound, + 3 % (csrc/zkp_api.hip) — while the two-stream shape of a small or very large call builds its list from the response
    kinds alone (k_verify_plan with e == nullptr: 2 items per Open row, 1 per Mask row).  Batches of half all_open proofs make that list
    overrun the expected items; two forged proofs at the end, behind a run of all_open, put failing Enc checks at its tail, where a claim
    loop that stopped early would leave them unchecked.
Every verdict vector is compared with the labels, which the C/GMP oracle confirms on every proof of the pool the batches are drawn from."""
import math

import numpy as np
import pytest

import crafted_range as CR
import helpers as H
from helpers import zkp
from test_gpu_routing import compute_units, expected_family, expected_tail, family_that_ran

pytestmark = pytest.mark.gpu

N_BITS, EF = 2048, 128
POOL_BASES = 6
# the batch sizes the routing judges by expected items (tests/test_gpu_routing.py); the borders of every family are added to them
SIZES = (1, 2, 4, 5, 8, 9, 10, 17, 20, 34, 40, 41, 64, 65, 72, 81, 82, 96, 192)
OTHER = ("honest", "flip_open", "all_mask", "flip_mask", "bad_kind2", "honest", "bad_kindFF", "all_open")
ENGINE = {"lat-r2l": 9, "lat-basen": 9, "lat-n2": 9, "mid-basen": 18, "mid-n2": 18, "base-n": 36, "n2": 36}


def gpu_prove(c):
    def prove(pb, wt):
        e = np.zeros((pb.batch, 32), np.uint8); elen = np.zeros(pb.batch, np.uint8); st = np.full(pb.batch, 9, np.uint8)
        c.range_ni_prove(pb.struct(), wt.struct(), e, elen, st, device=False)
        assert not st.any()
        return e, elen
    return prove


def compose(B):
    """labels of a batch of B: other labels first, then a run of all_open (half the batch), the forged proofs last"""
    if B == 1:
        return [["all_open"], ["forged"]]
    nf = 2 if B >= 4 else 1
    run = math.ceil(B / 2)
    head = B - nf - run
    return [[OTHER[k % len(OTHER)] for k in range(head)] + ["all_open"] * run + ["forged"] * nf]


def two_rule(W, B, cus):
    """csrc/zkp_api_proofs.inc range_verify_impl: does a call of B proofs on the engine of W limbs per lane take the two-stream shape?
    (its Enc launch: k_enc over n^2, 256 / (144 / W) groups of a workgroup)"""
    enc_blocks = -(-2 * EF * B // (256 // (144 // W)))
    if W == 36:
        return enc_blocks <= 3 * cus // 2 or enc_blocks >= 12 * cus
    if W == 9:
        return enc_blocks <= 5 * cus // 2
    return enc_blocks <= 11 * cus // 4


def segments(c, B):
    """[(lo, hi, two-stream)] of the calls a verify of B proofs under the library's routing becomes"""
    cus = compute_units()
    fam = expected_family(c, 2 * EF * B, listed=True)
    if fam == "split":
        tail = expected_tail(B)
        head_w = 18 if 2 * EF * B > 16 * 4 * cus else 9
        return [(0, B - tail, two_rule(head_w, B - tail, cus)), (B - tail, B, two_rule(9, tail, cus))]
    return [(0, B, two_rule(ENGINE[fam], B, cus))]


def list_length(kind, bits, segs, force=None):
    n = 0
    for lo, hi, two in segs:
        two = two if force is None else force
        n += CR.kind_items(kind[lo:hi]) if two else CR.matched_items(kind[lo:hi], bits[lo:hi])
    return n


def expected_items(bound):
    return (3 * bound + 3) // 4 + bound // 32                 # csrc/zkp_api.hip


@pytest.fixture(scope="module")
def pool(oracle):
    """POOL_BASES honest proofs under the fixture key, proved on the GPU, and every label made of each — confirmed by the oracle"""
    oracle.set_threads(min(16, oracle.max_threads()))
    c = zkp.Context(0)
    try:
        cases = H.build_range_case(b"crafted-gpu", [H.fixture_key()[2]], N_BITS, POOL_BASES)
        pb, labels, bits, _ = CR.make_pool(cases, N_BITS, oracle, gpu_prove(c))
    finally:
        c.close()
    ov = CR.oracle_verdicts(oracle, pb)
    assert list(ov) == [CR.WANT[lab] for lab in labels], list(zip(labels, ov))
    return dict(pb=pb, labels=labels, bits=bits, oracle=ov, cache={})


def assemble(pool, labels, cache=True):
    key = tuple(labels)
    if key in pool["cache"]:
        return pool["cache"][key]
    idx = np.array([CR.LABELS.index(lab) * POOL_BASES + k % POOL_BASES for k, lab in enumerate(labels)])
    pb = zkp.RangeBatch(N_BITS, len(labels), EF, shared_key=True)
    pb.n[:] = pool["pb"].n
    CR.copy_proofs(pb, pool["pb"], idx)
    out = (pb, pool["oracle"][idx], pool["bits"][idx])
    if cache:
        pool["cache"][key] = out
    return out


def all_sizes(c):
    cus = compute_units()
    fam = lambda B: expected_family(c, 2 * EF * B, listed=True)
    sizes = set(SIZES)
    for B in range(2, 8 * cus // 10):                         # the borders of every family up to the throughput engine's base-n kernels
        if fam(B) != fam(B - 1):
            sizes |= {B - 1, B}
    sizes.add(6 * cus)                                        # inside the throughput engine's upper two-stream window (enc_blocks >= 12 * cus)
    return sorted(sizes)


SWITCHES = ("default", "fuse_off", "two_streams_0", "two_streams_1", "grid_expected_0", "split_off", "device")


@pytest.mark.parametrize("switch", SWITCHES)
def test_crafted_verdicts_on_every_routed_path(pool, monkeypatch, switch):
    """(a) verdicts = labels = oracle, (b) the family that ran is the one the routing expects by the BOUND of the list (its contents
    do not move the route), (c) the hashes aboard the r2l launch where the rule fuses, (d) the list length read back from the
    work-list counter is what the plan builds from the kinds (two-stream) or from kinds and bits (one-stream) — beyond the expected
    items of the bound on every two-stream call.  The same verdicts with each of the library's switches turned."""
    import os
    assert "ZKP_BASEN" not in os.environ
    monkeypatch.delenv("ZKP_TWO_STREAMS", raising=False)
    if switch == "grid_expected_0":
        monkeypatch.setenv("ZKP_GRID_EXPECTED", "0")          # (read at zkp_ctx_create)
    c = zkp.Context(0)
    monkeypatch.delenv("ZKP_GRID_EXPECTED", raising=False)
    try:
        assert c.enc_form() == zkp.capi.ENC_FORM_AUTO
        c.set_geometry(0)
        if switch == "fuse_off":
            c.set_fuse_hash(False)
        if switch == "split_off":
            c.set_split(False)
        if switch.startswith("two_streams_"):
            monkeypatch.setenv("ZKP_TWO_STREAMS", switch[-1])  # (read on every call)
        force = {"two_streams_0": False, "two_streams_1": True}.get(switch)
        routed = switch in ("default", "fuse_off", "two_streams_0", "two_streams_1", "device")
        sizes = all_sizes(c)
        big = max(sizes)
        for B in sizes:
            for labels in compose(B):
                pb, ov, bits = assemble(pool, labels, cache=B != big)
                want = np.array([CR.WANT[lab] for lab in labels], np.uint8)
                assert np.array_equal(ov, want)
                c.timing_reset(True)
                if switch == "device":
                    import torch
                    dpb = pb.to(torch.device("cuda", 0))
                    dv = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    c.range_ni_verify(dpb.struct(), dv, device=True)
                    c.synchronize()
                    v = dv.cpu().numpy()
                else:
                    v = np.full(B, 9, np.uint8)
                    c.range_ni_verify(pb.struct(), v, device=False)
                count = c.timing_get()[2]
                c.timing_reset(False)
                bad = [(k, labels[k], int(v[k])) for k in range(B) if v[k] != want[k]]
                assert not bad, (switch, B, bad)
                fam = expected_family(c, 2 * EF * B, listed=True)
                if routed:
                    assert family_that_ran(c) == fam, (switch, B, family_that_ran(c), fam)
                    if fam == "split":
                        assert c.last_split() == expected_tail(B), (switch, B)
                    segs = segments(c, B)
                    fused = switch != "fuse_off" and force is not False and fam == "lat-r2l"
                    if fam == "lat-r2l" or switch == "fuse_off":
                        assert c.last_fused_hash() == fused, (switch, B)
                    want_count = list_length(pb.resp_kind, bits, segs, force)
                    assert count == want_count, (switch, B, count, want_count, segs)
                    if all(two for _, _, two in segs) if force is None else force:
                        assert count > expected_items(2 * EF * B), (switch, B, count)      # the list overruns what the grid was sized for
                elif switch == "split_off":
                    assert c.last_split() == 0
    finally:
        c.close()


def test_crafted_verdicts_on_pinned_families(ctx, pool):
    """one mixed batch of 10 under each pinned family (tests/conftest.py ctx)"""
    labels = ["honest", "flip_open", "all_mask", "flip_mask", "bad_kind2", "bad_kindFF", "all_open", "all_open", "forged", "forged"]
    pb, ov, _ = assemble(pool, labels)
    v = np.full(len(labels), 9, np.uint8)
    ctx.range_ni_verify(pb.struct(), v, device=False)
    assert list(v) == list(ov) == [CR.WANT[lab] for lab in labels], (ctx.test_geometry, ctx.test_form, list(v))


def test_crafted_verdicts_n4096(oracle):
    """n = 4096 under the library's routing: calls of 2 and 8 proofs"""
    synth = __import__("importlib").import_module("zk-paillier_amd.synth")
    n_bits = 4096
    n = synth.bench_key_4096()[2]
    labels_used = ("honest", "all_open", "flip_open", "flip_mask", "forged")
    oracle.set_threads(min(16, oracle.max_threads()))
    c = zkp.Context(0)
    try:
        cases = H.build_range_case(b"crafted-4096", [n], n_bits, 1)
        p, plabels, _, _ = CR.make_pool(cases, n_bits, oracle, gpu_prove(c), labels_used)
        ov = CR.oracle_verdicts(oracle, p)
        assert list(ov) == [CR.WANT[lab] for lab in plabels]
        for labels in (["all_open", "forged"], ["honest", "flip_open", "flip_mask", "all_open", "all_open", "all_open", "forged", "forged"]):
            pb = zkp.RangeBatch(n_bits, len(labels), EF, shared_key=True)
            pb.n[:] = p.n
            CR.copy_proofs(pb, p, [labels_used.index(lab) for lab in labels])
            v = np.full(len(labels), 9, np.uint8)
            c.range_ni_verify(pb.struct(), v, device=False)
            assert list(v) == [CR.WANT[lab] for lab in labels], (labels, list(v))
    finally:
        c.close()


def test_crafted_verdicts_under_per_proof_keys(oracle):
    """per-proof keys, four of them outside the base-n form (short keys): the base-n launch takes the other proofs' items, those of the
    four go on the list the n^2-sized launch behind it works off (bn_left) — all_open proofs on both sides, a forged proof last on each"""
    import importlib
    synth = importlib.import_module("zk-paillier_amd.synth")
    B = 24
    outside = (3, 9, 16, 23)
    labels = ["honest", "flip_open", "all_mask", "all_open", "flip_mask", "bad_kind2", "all_open", "all_open", "honest", "all_open",
              "bad_kindFF", "all_open", "all_open", "flip_open", "all_open", "all_open", "all_open", "honest", "all_open", "all_open",
              "all_open", "all_open", "forged", "forged"]
    keys = synth.distinct_keys_2048(B)
    for k, b in enumerate(outside):
        keys[b] = H.test_key(1000 + 24 * k, tag=k + 1)[2]
    oracle.set_threads(min(16, oracle.max_threads()))
    cases = H.build_range_case(b"crafted-keys", keys, N_BITS, B, shared=False)
    pb, wt = H.fill_batch(cases, N_BITS, False, oracle)
    c = zkp.Context(0)
    try:
        c.set_geometry(zkp.load().zkp_build_limbs_per_lane())
        e, elen = gpu_prove(c)(pb, wt)
        bits = CR.challenge_bits(e, elen, EF)
        for b, lab in enumerate(labels):
            CR.craft(pb, b, cases[b], bits[b], lab)
        want = [CR.WANT[lab] for lab in labels]
        ov = CR.oracle_verdicts(oracle, pb)
        assert list(ov) == want
        for geometry in (36, 18, 9):
            c.set_geometry(geometry)
            c.set_enc_form("basen")
            v = np.full(B, 9, np.uint8)
            c.range_ni_verify(pb.struct(), v, device=False)
            lanes, ok = c.diag_basen_last()
            assert lanes == 72 // geometry and not ok, (geometry, lanes, ok)
            assert list(v) == want, (geometry, list(v))
    finally:
        c.close()


def test_even_key_kinds_against_bits_in_both_shapes(oracle, monkeypatch):
    """an even key (the engine answers MALFORMED where it would have to compute under it): a proof whose every row's kind
    contradicts its bit schedules no Enc in the one-stream plan and is REJECTED — and so in the two-stream shape, whose kind-derived list
    does hold its rows (k_verdict_merge); a proof with one bit-matched row is MALFORMED in both"""
    d = H.pm.Drbg(b"even-key-crafted")
    n_even = (d.bits(1024) | (1 << 1023)) & ~1
    n_bits = 1024
    cases = H.build_range_case(b"even-key-crafted", [n_even], n_bits, 2)
    pb, wt = H.fill_batch(cases, n_bits, True, oracle)
    e = np.zeros((2, 32), np.uint8); elen = np.zeros(2, np.uint8)
    oracle.range_ni_prove(pb.struct(), wt.struct(), e, elen, None)
    bits = CR.challenge_bits(e, elen, EF)
    CR.craft(pb, 0, cases[0], bits[0], "all_flip")
    CR.craft(pb, 1, cases[1], bits[1], "one_match")
    c = zkp.Context(0)
    try:
        got = {}
        for two in ("0", "1"):
            monkeypatch.setenv("ZKP_TWO_STREAMS", two)
            v = np.full(2, 9, np.uint8)
            c.range_ni_verify(pb.struct(), v, device=False)
            got[two] = list(v)
        assert got["0"] == got["1"] == [zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED], got
    finally:
        c.close()
