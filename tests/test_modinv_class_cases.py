"""CPU: the vectors of tests/golden/modinv_classes.json and the batches tests/modinv_class_cases.py lays them out in are what they claim.
Every vector goes through tools/wbgcd_model.py — the word-for-word model of wb_gcd and of k_modinv's finalisation loop — and must land in
the class, with the events, that the fixture records; the C oracle (mpz_invert) and pow(a, -1, M) must agree on every item of every
batch; the coverage cells below are conditions, not measurements.

What the search of tests/golden/make_modinv_classes.py visited (its printed counts; also kept in the fixture under "search").  The
classes are those of the cofactor v before the finalisation: in_range 0 <= v < M, neg -M <= v < 0, below_neg_m v < -M (two passes: the
class a single conditional add got wrong), ge_m M <= v < 2^(32 kw), ge_m_signword v >= 2^(32 kw).

    small 34-90 bits       tried  200013  in_range 93743  neg 106167  below_neg_m 103  ge_m 0  ge_m_signword 0
    2048 full width        tried    1173  in_range 528  neg 645  below_neg_m 0  ge_m 0  ge_m_signword 0
    2048 lengths -31..-1   tried    3754  in_range 1754  neg 1995  below_neg_m 5  ge_m 0  ge_m_signword 0
    2048 lengths 1..6 mod 30 tried    2550  in_range 1152  neg 1391  below_neg_m 7  ge_m 0  ge_m_signword 0
    2048 full-width events tried      46  in_range 18  neg 28  below_neg_m 0  ge_m 0  ge_m_signword 0
    4096 full width        tried    1157  in_range 574  neg 583  below_neg_m 0  ge_m 0  ge_m_signword 0
    4096 lengths -31..-1   tried    3707  in_range 1834  neg 1871  below_neg_m 2  ge_m 0  ge_m_signword 0
    4096 lengths 1..6 mod 30 tried    1309  in_range 603  neg 699  below_neg_m 7  ge_m 0  ge_m_signword 0
    4096 full-width events tried      71  in_range 35  neg 36  below_neg_m 0  ge_m 0  ge_m_signword 0
    8192 full width        tried     181  in_range 82  neg 98  below_neg_m 1  ge_m 0  ge_m_signword 0
    8192 lengths -31..-1   tried    3466  in_range 1737  neg 1720  below_neg_m 9  ge_m 0  ge_m_signword 0
    8192 lengths 1..6 mod 30 tried    2549  in_range 1107  neg 1433  below_neg_m 9  ge_m 0  ge_m_signword 0
    8192 full-width events tried      55  in_range 31  neg 24  below_neg_m 0  ge_m 0  ge_m_signword 0
    8192 shared modulus    tried    2902  in_range 1274  neg 1622  below_neg_m 6  ge_m 0  ge_m_signword 0
    ALL                    tried  222933  in_range 104472  neg 118312  below_neg_m 149  ge_m 0  ge_m_signword 0

No candidate gave v >= M: the two `ge_m` classes have no vector, the fixture claims NO coverage of the subtract branch of the
finalisation loop, and this file asserts that the fixture does not pretend otherwise.  Whether that branch is dead is still open."""
import os
import sys

import numpy as np
import pytest

import modinv_class_cases as MC
import small_proof_cases as SC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wbgcd_model as W  # noqa: E402

GOLDEN = os.path.dirname(MC.FIXTURE)


def derived(mod_bits):
    """[(item, the model's summary of it)] of the fixture vectors of one width: one model run each, kept for the process"""
    def build():
        out = []
        for it in MC.vectors(mod_bits):
            st = {"maxcof": 0}
            g, inv = W.wbgcd(it["a"], it["M"], mod_bits // 32, True, st)
            assert g == 1 and inv == it["inv"] and it["status"] == MC.zkp.INV_OK, it["name"]
            out.append((it, MC.summary(st["call"])))
        return out
    return SC.cached("modinv-classes-derived-%d" % mod_bits, build)


def test_fixture_is_small_and_claims_no_more_than_it_has():
    assert os.path.getsize(MC.FIXTURE) <= os.path.getsize(os.path.join(GOLDEN, "modexp_kat.json"))
    fx = MC.fixture()
    tried = sum(r["tried"] for r in fx["search"])
    small = sum(r["tried"] for r in fx["search"] if r["region"].startswith("small"))
    assert small >= 200000 and tried > small
    for cls in ("ge_m", "ge_m_signword"):
        found = sum(r[cls] for r in fx["search"])
        have = sum(v["v_class"] == cls for w in MC.WIDTHS for v in fx["wide"][str(w)] + fx["small"])
        assert (found > 0) == (have > 0)          # a class that was found is in the fixture (and then in the cells below); one that was not is not claimed


@pytest.mark.parametrize("mod_bits", MC.WIDTHS)
def test_every_vector_is_in_its_recorded_class(mod_bits):
    for it, s in derived(mod_bits):
        assert s == it["rec"], it["name"]
        assert (s["final_passes"], s["v_class"]) in ((0, "in_range"), (1, "neg"), (2, "below_neg_m"), (1, "ge_m"), (1, "ge_m_signword")), it["name"]


@pytest.mark.parametrize("mod_bits", MC.WIDTHS)
def test_coverage_cells(mod_bits):
    kw = mod_bits // 32
    ss = derived(mod_bits)
    count = lambda f: sum(1 for it, s in ss if f(it, s))
    for cls in ("in_range", "neg", "below_neg_m"):
        assert count(lambda it, s: s["v_class"] == cls) >= 2, cls
    for cls in ("ge_m", "ge_m_signword"):          # required as soon as the search has found one
        if any(r[cls] for r in MC.fixture()["search"]):
            assert count(lambda it, s: s["v_class"] == cls) >= 1, cls
    assert count(lambda it, s: s["neg_a"]) >= 2 and count(lambda it, s: s["neg_b"]) >= 2
    assert count(lambda it, s: s["signword"]) >= 2
    assert all(it["M"] >> (32 * kw - 1) == 1 for it, s in ss if s["signword"])      # only a modulus with its top bit set gets there
    assert count(lambda it, s: s["cross_le64"]) >= 1 and count(lambda it, s: s["start_le64"]) >= 1
    # below_neg_m under wide moduli too, not only under the zero padded small ones
    assert count(lambda it, s: s["v_class"] == "below_neg_m" and it["M"].bit_length() > mod_bits - 32) >= 2


def test_shared_modulus_holds_the_rare_class():
    """8192 bits, mod_stride = 0: several a = M - r under ONE full-width modulus end with v < -M"""
    M, f, rare, plain = MC.shared_modulus()
    assert M.bit_length() == 8192 and M % f == 0 and len(rare) >= 4
    for r in rare[:3]:                             # (a model run at 8192 bits is a third of a second; the minting script ran all of them)
        st = {"maxcof": 0}
        g, inv = W.wbgcd(M - r, M, 256, True, st)
        assert g == 1 and inv == pow(M - r, -1, M) and st["call"]["v_class"] == "below_neg_m" and st["call"]["final_passes"] == 2


@pytest.mark.parametrize("mod_bits", MC.WIDTHS)
def test_batches_oracle_python_and_layout(oracle, mod_bits):
    """the C oracle and pow(a, -1, M) agree with each other and with the status each item was built for; every below_neg_m vector shares
    its block of 16 with a domain lane, an a == 0 lane, a common-factor lane, a tiny-modulus lane and a full-length lane"""
    bs = MC.batches(mod_bits)
    assert set(bs) == {"per_item", "rare_last"} | ({"shared"} if mod_bits == 8192 else set())
    names = {it["name"] for it in MC.vectors(mod_bits)}
    rare = {it["name"] for it in MC.vectors(mod_bits) if it["rec"]["v_class"] == MC.RARE}
    for name, (items, stride) in bs.items():
        assert not MC.placement_problems(items, shared=stride == 0), name
        assert len(items) % MC.BLOCK and len(items) <= 104
        a, m, inv, st = MC.arrays(items, mod_bits, stride)
        oo, so = oracle.modinv(mod_bits, a, m, stride)
        SC.assert_same(st, so, name + ": status")
        SC.assert_same(inv, oo, name + ": inverse")
        assert {0, 1, 2} == set(int(v) for v in st)
        assert not oo[st != 0].any()
        last = {it["name"] for it in items[len(items) // MC.BLOCK * MC.BLOCK:]}
        if stride:
            assert len(items) > 64 and names <= {it["name"] for it in items}
            assert rare <= last if name == "rare_last" else not rare & last
        else:
            assert sum(it["rec"] is not None for it in items[:MC.BLOCK]) >= 2 and sum(it["rec"] is not None for it in items[-(len(items) % MC.BLOCK):]) >= 2
    # a wrong placement is noticed
    items = [it for it in bs["per_item"][0] if it["kind"] != "tiny"]
    assert MC.placement_problems(items)
