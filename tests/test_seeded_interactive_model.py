"""CPU tests of the yardstick behind tests/test_gpu_seeded_interactive.py: the witness tests/seeded_model.py expands from a seed, at the row
counts the interactive RangeProof is run with, fed to the oracle's generate_encrypted_pairs and generate_proof — and held against the pure
Python model of the protocol — plus the two properties of the stream that let the interactive steps reuse it: 128 rows are the RangeProofNi
witness, and a row does not depend on how many rows there are."""
import numpy as np
import pytest

import helpers as H
import seeded_interactive_cases as IC
import seeded_model as M
from helpers import L, pm, zkp


@pytest.mark.parametrize("shape", IC.SHAPES[:4], ids=IC.SHAPE_IDS[:4])      # ef 40, 129, 1, 256
def test_oracle_steps_on_the_models_witness_match_the_python_model(oracle, shape):
    n_bits, key_bits, ef, shared = shape
    B = 4
    cases = IC.session_cases(*shape)
    po, wt = H.fill_batch(cases, n_bits, shared, oracle)
    for f in IC.WIT:                                                          # the batch carries the model's rows, not the DRBG's
        assert np.array_equal(getattr(wt, f), M.to_limbs([c[f] for c in cases], n_bits // 32)), f
    e, elen = IC.session_challenge(ef, B, short={3} if ef > 8 else ())
    st = IC.oracle_steps(oracle, po, wt, e, elen)
    assert list(st) == [0, 0, 0, zkp.VERDICT_MALFORMED if ef > 8 else 0]
    v = np.full(B, 7, np.uint8)
    oracle.range_verifier_output(po.struct(), e, elen, v)
    for b, c in enumerate(cases):
        n = c["n"]
        c1, c2 = pm.generate_encrypted_pairs(n, c["w1"], c["w2"], c["r1"], c["r2"])
        assert [L.limbs_to_int(r) for r in po.c1[b]] == c1 and [L.limbs_to_int(r) for r in po.c2[b]] == c2, b
        # the model's rows are a witness the protocol accepts: w1, w2 a third of the range apart, inside [0, 2 third)
        third = c["range"] // 3
        assert all(abs(a - d) == third and third <= max(a, d) < 2 * third for a, d in zip(c["w1"], c["w2"]))
        if st[b]:
            assert v[b] == zkp.VERDICT_MALFORMED
            continue
        eb = bytes(e[b, :elen[b]])
        resp = pm.generate_proof(n, c["x"], c["r"], eb, c["range"], c["w1"], c["w2"], c["r1"], c["r2"], ef)
        assert H.responses_from_batch(po, b) == resp, b
        cx = L.limbs_to_int(po.ciphertext[b])
        assert pm.verifier_output(n, eb, c1, c2, resp, c["range"], cx, ef) == (v[b] == zkp.VERDICT_ACCEPT)
    # an honest session accepts; the dishonest one (session 1) is caught by a Mask row unless its challenge has none (ef = 1: one bit)
    assert v[0] == v[2] == zkp.VERDICT_ACCEPT
    if ef > 8:
        assert v[1] == zkp.VERDICT_REJECT


def test_128_rows_are_the_witness_of_the_seeded_range_proof_ni_cases():
    import test_gpu_seeded_prove as NI
    n_bits, B, first_index = 1024, 4, (1 << 32) + 7
    n, ni_cases = NI.prove_case(n_bits, B, first_index)
    wit, status, _, _ = M.witness(IC.SEED, first_index, [n], [c["range"] for c in ni_cases], 128)
    assert IC.SEED == NI.SEED and not any(status)
    for b, c in enumerate(ni_cases):
        for f in IC.WIT:
            assert c[f] == wit[f][b], (b, f)
    # chunked: session 2 alone at its own index has the rows it had in the batch
    one, _, _, _ = M.witness(IC.SEED, first_index + 2, [n], [ni_cases[2]["range"]], 128)
    for f in IC.WIT:
        assert one[f][0] == ni_cases[2][f], f


def test_a_row_does_not_depend_on_the_number_of_rows():
    """the nonce carries (index, row, field) only: the first 40 rows of an ef = 129 witness are the ef = 40 witness"""
    n = H.test_key(512)[2]
    ranges = [c["range"] for c in IC.session_cases(1024, 512, 40, True)]
    short, s1, _, _ = M.witness(IC.SEED, IC.FIRST_INDEX, [n], ranges, 40)
    long_, s2, _, _ = M.witness(IC.SEED, IC.FIRST_INDEX, [n], ranges, 129)
    assert not any(s1) and not any(s2)
    for f in IC.WIT:
        for b in range(len(ranges)):
            assert long_[f][b][:40] == short[f][b], (f, b)
            assert long_[f][b][40:] != short[f][b][:89]
