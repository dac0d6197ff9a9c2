"""The crafted RangeProofNi proofs of tests/crafted_range.py against the C/GMP oracle (no GPU): every label gets the verdict of the
reference, and the fixtures isolate the binding of a row's kind to its challenge bit — every crafted row passes its Enc checks and
its range predicate on its own, and the honest proof it was made from is accepted, so the bit check is the only one that fails."""
import numpy as np
import pytest

import crafted_range as CR
import helpers as H
from helpers import pm, L, zkp


def oracle_prove(oracle):
    def prove(pb, wt):
        e = np.zeros((pb.batch, 32), np.uint8); elen = np.zeros(pb.batch, np.uint8); st = np.full(pb.batch, 9, np.uint8)
        oracle.range_ni_prove(pb.struct(), wt.struct(), e, elen, st)
        assert not st.any()
        return e, elen
    return prove


@pytest.fixture(scope="module")
def oracle():
    import oracle_lib
    o = oracle_lib.Oracle()
    o.set_threads(min(16, o.max_threads()))
    return o


@pytest.mark.parametrize("n_bits", [1024, 2048])
def test_crafted_labels_get_the_reference_verdict(oracle, n_bits):
    n = H.test_key(1024)[2] if n_bits == 1024 else H.fixture_key()[2]
    cases = H.build_range_case(b"crafted-cpu-%d" % n_bits, [n], n_bits, 2)
    pool, labels, bits, _ = CR.make_pool(cases, n_bits, oracle, oracle_prove(oracle), CR.LABELS + ("all_flip", "one_match"))
    v = CR.oracle_verdicts(oracle, pool)
    assert list(v) == [CR.WANT[lab] for lab in labels], list(zip(labels, v))
    # what makes each label what it is, on the arrays themselves
    for k, lab in enumerate(labels):
        kind, b = pool.resp_kind[k], bits[k]
        matched = ((kind == zkp.RESP_OPEN) & (b == 0)) | ((kind == zkp.RESP_MASK) & (b == 1))
        want_mismatch = {"honest": 0, "all_open": int(b.sum()), "all_mask": int((b == 0).sum()), "flip_open": 1, "flip_mask": 1,
                         "bad_kind2": 1, "bad_kindFF": 1, "forged": 0, "all_flip": pool.ef, "one_match": pool.ef - 1}[lab]
        assert int((~matched).sum()) == want_mismatch, (lab, k)
    # the kind-derived plan of all_open holds the most items a proof can put on a list: 2 per row
    for k, lab in enumerate(labels):
        if lab == "all_open":
            assert CR.kind_items(pool.resp_kind[k]) == 2 * pool.ef


def test_crafted_rows_pass_every_check_but_the_bit(oracle):
    """n = 1024: each crafted Open / Mask row, on its own, passes its Enc checks (pm.enc) and its range predicate
    (range_proof.rs:300-305, :338); a forged proof's tampered rows fail exactly their Enc check"""
    n_bits, kw = 1024, 32
    n = H.test_key(1024)[2]
    nn = n * n
    cases = H.build_range_case(b"crafted-isolate", [n], n_bits, 2)
    pool, labels, bits, pcases = CR.make_pool(cases, n_bits, oracle, oracle_prove(oracle), CR.LABELS + ("all_flip",))
    v = CR.oracle_verdicts(oracle, pool)
    assert all(v[k] == zkp.VERDICT_ACCEPT for k, lab in enumerate(labels) if lab == "honest")
    checked = 0
    for k, lab in enumerate(labels):
        case = pcases[k]
        third = case["range"] // 3
        cipher_x = L.limbs_to_int(pool.ciphertext[k])
        rows = CR.crafted_rows(lab, bits[k])
        if lab == "forged":
            rows = range(pool.ef - CR.FORGED_ROWS, pool.ef)
        for i in rows:
            c1, c2 = L.limbs_to_int(pool.c1[k, i]), L.limbs_to_int(pool.c2[k, i])
            w1, r1 = L.limbs_to_int(pool.resp_w1[k, i]), L.limbs_to_int(pool.resp_r1[k, i])
            if pool.resp_kind[k, i] == zkp.RESP_OPEN:
                w2, r2 = L.limbs_to_int(pool.resp_w2[k, i]), L.limbs_to_int(pool.resp_r2[k, i])
                assert (w2 < third < w1 < 2 * third) or (w1 < third < w2 < 2 * third), (lab, k, i)
                assert pm.enc(n, w2, r2) == c2, (lab, k, i)
                assert (pm.enc(n, w1, r1) == c1) == (lab != "forged"), (lab, k, i)
                if lab != "forged":
                    assert bits[k, i] == 1          # an Open answer to a 1 bit
            else:
                j = int(pool.resp_j[k, i])
                assert third <= w1 <= 2 * third, (lab, k, i)
                cj = c1 if j == 1 else c2
                assert ((cj * cipher_x % nn) == pm.enc(n, w1, r1)) == (lab != "forged"), (lab, k, i)
                if lab != "forged":
                    assert bits[k, i] == 0          # a Mask answer to a 0 bit
            checked += 1
    assert checked > 4 * 64


def test_crafted_work_list_counts():
    """the two plan lengths the GPU tests compare the engine's counter with"""
    kind = np.array([zkp.RESP_OPEN, zkp.RESP_MASK, zkp.RESP_OPEN, zkp.RESP_MASK, 2, 0xFF], np.uint8)
    bits = np.array([0, 1, 1, 0, 0, 1], np.uint8)
    assert CR.kind_items(kind) == 2 + 1 + 2 + 1
    assert CR.matched_items(kind, bits) == 2 + 1
