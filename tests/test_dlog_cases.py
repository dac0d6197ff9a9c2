"""The CompositeDLogProof cases of tests/dlog_cases.py, checked on the CPU: the C oracle against the Python model on every row, the verdicts the
rows are built to have, and the layout the GPU tests (tests/test_gpu_dlog.py) rely on — recomputed here from the rows, so that a later edit of
the builder cannot quietly turn the cases into easy ones."""
import numpy as np
import pytest

import dlog_cases as D
from helpers import pm, L

ACCEPT, REJECT, MALFORMED = D.ACCEPT, D.REJECT, D.MALFORMED


def model_verdict(row):
    """pm.dlog_verify, the reference's three panics (wi_dlog_proof.rs:69,72,73) as MALFORMED"""
    name, N, g, ni, s, r, x, y, pinned = row
    try:
        return ACCEPT if pm.dlog_verify(x, y, N, g, ni) else REJECT
    except AssertionError:
        return MALFORMED


@pytest.mark.parametrize("n_bits,y_bits", [(1024, 544), (2048, 768), (4096, 768)])
def test_oracle_matches_model(oracle, n_bits, y_bits):
    rows = D.build(n_bits, y_bits, oracle)
    vo = D.oracle_verdicts(n_bits, y_bits, oracle)
    vm = [model_verdict(r) for r in rows]
    assert list(vo) == vm, [(r[0], int(a), b) for r, a, b in zip(rows, vo, vm) if a != b]
    # the prover: the x, y of the rows with a witness are the oracle's; the model computes the same
    for name, N, g, ni, s, r, x, y, pinned in rows:
        if r is not None:
            assert (x, y) == pm.dlog_prove(N, g, ni, s, r), name


@pytest.mark.parametrize("n_bits,y_bits", D.SHAPES)
def test_pinned_verdicts(oracle, n_bits, y_bits):
    rows = D.build(n_bits, y_bits, oracle)
    vo = D.oracle_verdicts(n_bits, y_bits, oracle)
    for row, v in zip(rows, vo):
        name, pinned = row[0], row[8]
        assert pinned is None or v == pinned, (name, int(v), pinned)
        if pinned is not None:
            assert (pinned == ACCEPT) == (name.startswith("honest") or name.endswith("-honest")), name
            assert (pinned == MALFORMED) == name.startswith("malformed"), name
        else:
            assert name == "edge-N-2^128+1"
    by = {r[0]: (r, int(v)) for r, v in zip(rows, vo)}
    # N = 2^128 + 1 is large enough: the oracle does not call it MALFORMED (the honest proof under it is accepted)
    assert by["edge-N-2^128+1"][0][1] == (1 << 128) + 1 and by["edge-N-2^128+1"][1] == ACCEPT
    assert by["malformed-N-small"][0][1] == (1 << 128) - 159
    # every class of the builder is in the batch
    for name in ("honest-r-max-s-max", "honest-r0", "honest-s0", "honest-r0-s0", "honest-r1-s1", "honest-g2", "honest-g-minus-1", "honest-short-N",
                 "y-zero-key0", "y-one-key0", "y-flip-bit0", "y-top-bit-key0", "y-all-ones-key0", "x-zero", "x-one", "x-N-minus-1", "x-plus-N",
                 "x-flip-bit1", "ni-one", "ni-random", "malformed-N-small", "malformed-g-zero", "malformed-ni-zero", "malformed-g-shares-p",
                 "malformed-ni-shares-q", "malformed-g-zero-low-words"):
        assert name in by, name
    assert any(n.endswith("plus-secret") and v == REJECT for n, (r, v) in by.items())
    assert len({r[1] for r in rows if r[8] == ACCEPT}) >= 5          # honest proofs under several keys


def nbytes(v):
    return len(pm.to_bytes(v))


@pytest.mark.parametrize("n_bits,y_bits", D.SHAPES)
def test_layout(oracle, n_bits, y_bits):
    rows = D.build(n_bits, y_bits, oracle)
    vo = [int(v) for v in D.oracle_verdicts(n_bits, y_bits, oracle)]
    by = {r[0]: r for r in rows}
    assert len(rows) == D.ROWS == 70 and len(by) == 70
    for name, N, g, ni, s, r, x, y, pinned in rows:                 # every value fits its field of the ABI
        assert max(N, g, ni, x).bit_length() <= n_bits and y.bit_length() <= y_bits and s.bit_length() <= 256, name
        assert r is None or r.bit_length() <= 512, name
        assert N & 1, name
    # row 0 is an honest proof with its witness
    assert rows[0][8] == ACCEPT and rows[0][5] is not None and vo[0] == ACCEPT
    # rows 64 ... 69: the second block of k_dlog_hash and the last, ragged claim hold all three verdicts
    assert D.HASH_BLOCK == 64 and {MALFORMED, REJECT, ACCEPT} <= set(vo[64:])
    assert all(v != MALFORMED for v in vo[:D.MIXED])                # the mixed-length runs are all exponentiated and compared
    # every aligned run of the first 32 rows holds responses of different effective lengths, drawn from {0, 1, ~513, y_bits}
    run = D.run_of(n_bits)
    assert run == (2 if n_bits == 4096 else 4)
    seen, extremes = set(), 0
    for at in range(0, D.MIXED, run):
        lens = [rows[i][7].bit_length() for i in range(at, at + run)]
        classes = {D.length_class(rows[i][7], y_bits) for i in range(at, at + run)}
        assert len(classes) >= 2 and len(set(lens)) >= 2, (at, lens)
        for i in range(at, at + run, 2):                            # (and so does every aligned pair, at every key size)
            assert rows[i][7].bit_length() != rows[i + 1][7].bit_length(), i
        seen |= classes
        extremes += (0 in classes and "full" in classes)
    assert seen == {0, 1, "mid", "full"} and extremes >= 1
    for i in range(D.MIXED):
        n = rows[i][7].bit_length()
        assert n in (0, 1, y_bits) or 200 <= n <= 513, (i, n)
    assert by["honest-r-max-s-max"][7].bit_length() == 513            # the longest honest response
    assert by["y-all-ones-key0"][7] == (1 << y_bits) - 1 and by["y-top-bit-key0"][7].bit_length() == y_bits
    # N narrower than its field: whole zero top words in all four hashed operands
    short = by["honest-short-N"]
    assert short[1].bit_length() == n_bits - 40
    assert all(nbytes(v) <= (n_bits - 40) // 8 for v in (short[1], short[2], short[3], short[6]))
    assert by["x-plus-N"][6] >= by["x-plus-N"][1] and by["x-plus-N"][6] % short[1] == short[6]
    if n_bits == 2048:
        r1100 = by["honest-N-1100-bits"]
        assert r1100[1].bit_length() == 1100 and all(v.bit_length() <= 1100 for v in (r1100[2], r1100[3], r1100[6]))
    if n_bits == 1024:
        sx = by["honest-short-x"]
        assert nbytes(sx[6]) < nbytes(sx[1]) == 128                  # put_bigint strips at least one leading zero byte of x
        assert 1 <= D.short_x_tries(n_bits) <= D.SHORT_X_BOUND == 4096
    # the crafted MALFORMED operands are what their names say
    import math
    N0 = by["honest-key0"][1]
    assert 1 < math.gcd(by["malformed-g-shares-p"][2], N0) < N0 and 1 < math.gcd(by["malformed-ni-shares-q"][3], N0) < N0
    assert math.gcd(by["malformed-g-shares-p"][2], N0) != math.gcd(by["malformed-ni-shares-q"][3], N0)
    gz = by["malformed-g-zero-low-words"][2]
    assert (N0 - gz) % (1 << 96) == 0 and 1 < math.gcd(gz, N0) < N0
    # the prover's carry chain and its zero operands
    assert by["honest-r-max-s-max"][5] == (1 << 512) - 1 and by["honest-r-max-s-max"][4] == (1 << 256) - 1
    assert by["honest-r0"][5] == 0 and by["honest-s0"][4] == 0 and (by["honest-r0-s0"][6], by["honest-r0-s0"][7]) == (1, 0)
    assert by["honest-g2"][2] == 2 and by["honest-g-minus-1"][2] == by["honest-g-minus-1"][1] - 1
    # the arrays the GPU tests pass are these rows
    N_, g_, ni_, x_, y_ = D.arrays(rows, n_bits, y_bits)
    assert N_.shape == (70, n_bits // 32) and y_.shape == (70, y_bits // 32) and N_.dtype == np.uint32
    assert L.limbs_to_ints(y_) == [r[7] for r in rows] and L.limbs_to_ints(x_) == [r[6] for r in rows]
    w = D.witness_arrays(rows, n_bits, y_bits)
    assert w[0].shape[0] == sum(r[5] is not None for r in rows) >= 40
