"""GPU parity: CompositeDLogProof prove / verify (wi_dlog_proof.rs:46-91) against the oracle and the goldens."""
import json
import os

import numpy as np
import pytest

import helpers as H
from helpers import pm, L, zkp

pytestmark = pytest.mark.gpu


def test_dlog_goldens(ctx):
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dlog.json")))
    iv = lambda s: int(s, 16)
    B = len(gold)
    arr = lambda k, w: L.ints_to_limbs([iv(g[k]) for g in gold], w)
    N, g, ni, s, r = arr("N", 64), arr("g", 64), arr("ni", 64), arr("secret", 8), arr("r", 16)
    x = np.zeros((B, 64), np.uint32); y = np.zeros((B, 24), np.uint32)
    ctx.dlog_prove(2048, 768, B, N, g, ni, s, r, x, y)
    assert L.limbs_to_ints(x) == [iv(k["x"]) for k in gold] and L.limbs_to_ints(y) == [iv(k["y"]) for k in gold]
    v = np.full(B, 9, np.uint8)
    ctx.dlog_verify(2048, 768, B, N, g, ni, x, y, v)
    assert list(v) == [k["verdict"] for k in gold]


@pytest.mark.parametrize("n_bits", [1024, 2048])
def test_dlog_matches_oracle(ctx, oracle, n_bits):
    kw, yb = n_bits // 32, 768
    d = pm.Drbg(b"gpu-dlog-%d" % n_bits)
    rows = []
    for t in range(3):
        p, q, N = H.test_key(n_bits, tag=20 + t)
        g = d.range(2, N - 1); s = d.bits(256)
        rows.append((N, g, pow(pow(g, -1, N), s, N), s, d.bits(512)))     # honest (wi_dlog_proof.rs:117-141)
        rows.append((N, g, pow(g, s, N), s, d.bits(512)))                 # +s instead of -s (:145-168)
    p, q, N = H.test_key(n_bits, tag=20)
    rows.append((N, p, rows[0][2], rows[0][3], d.bits(512)))              # gcd(g, N) != 1 -> panic in the reference (:72)
    rows.append((N, rows[0][1], q * 3, rows[0][3], d.bits(512)))          # gcd(ni, N) != 1 (:73)
    rows.append(((1 << 128) - 159, 5, 7, 3, d.bits(512)))                 # N <= 2^128 (:69)
    rows.append((N, 0, rows[0][2], rows[0][3], d.bits(512)))              # g = 0: gcd(0, N) = N
    # g == N modulo 2^64 (and a multiple of p next to it): the first difference of the binary GCD has zero low words
    g_z = N - (d.bits(300) << 64); s_z = d.bits(256)
    rows.append((N, g_z, pow(pow(g_z, -1, N), s_z, N), s_z, d.bits(512)))
    rows.append((N, N - (p << 96), rows[0][2], rows[0][3], d.bits(512)))
    B = len(rows)
    N_, g_, ni_ = (L.ints_to_limbs([r[i] for r in rows], kw) for i in range(3))
    s_ = L.ints_to_limbs([r[3] for r in rows], 8); r_ = L.ints_to_limbs([r[4] for r in rows], 16)
    xo, yo = oracle.dlog_prove(n_bits, yb, N_, g_, ni_, s_, r_)
    xg = np.zeros_like(xo); yg = np.zeros_like(yo)
    ctx.dlog_prove(n_bits, yb, B, N_, g_, ni_, s_, r_, xg, yg)
    assert np.array_equal(xo, xg) and np.array_equal(yo, yg)
    # extra verify-side cases built from the honest proof 0: x + N (non-canonical x never equals a residue), y + 1
    N2, g2, ni2, x2, y2 = (np.concatenate([a, a[:1], a[:1]]) for a in (N_, g_, ni_, xo, yo))
    v = L.limbs_to_int(x2[B]) + rows[0][0]
    if v.bit_length() <= n_bits:
        x2[B] = L.int_to_limbs(v, kw)
    y2[B + 1, 0] ^= 1
    vo = oracle.dlog_verify(n_bits, yb, N2, g2, ni2, x2, y2)
    vg = np.full(B + 2, 9, np.uint8)
    ctx.dlog_verify(n_bits, yb, B + 2, N2, g2, ni2, x2, y2, vg)
    assert np.array_equal(vo, vg), (list(vo), list(vg))
    assert vo[0] == zkp.VERDICT_ACCEPT and vo[1] == zkp.VERDICT_REJECT and vo[6] == zkp.VERDICT_MALFORMED and vo[8] == zkp.VERDICT_MALFORMED
    # the same proofs tiled to a batch that fills the GPU: one launch per exponentiation, pre-checks on the one stream (the
    # small call above took the merged launch with the pre-checks on the second stream, zkp_api_proofs.inc:dlog_verify_impl)
    tiles = 3000
    big = [np.tile(a, (tiles, 1)) for a in (N2, g2, ni2, x2, y2)]
    vb = np.full((B + 2) * tiles, 9, np.uint8)
    ctx.dlog_verify(n_bits, yb, (B + 2) * tiles, *big, vb)
    assert np.array_equal(vb, np.tile(vo, tiles))


# ---- the shapes the tests above leave out (tests/dlog_cases.py; the cases themselves are checked on the CPU by tests/test_dlog_cases.py) ----
# One batch of 70 rows per shape: honest proofs under several keys and at the prover's arithmetic edges, verify-only edits, the rows the
# reference panics on, N = 2^128 + 1.  Responses of length 0, 1, ~513 and y_bits sit side by side in every claim of the first 32 rows, and
# rows 64 ... 69 — the second block of k_dlog_hash, the last and ragged claim of the merged launch — hold all three verdicts.

import dlog_cases as D  # noqa: E402


@pytest.mark.parametrize("n_bits,y_bits", D.SHAPES)
def test_dlog_prove_cases(ctx, oracle, n_bits, y_bits):
    """x = g^r mod N and y = r + e*s of every row with a witness, byte for byte the oracle's; every word of both outputs is written"""
    N, g, ni, s, r, xo, yo = D.witness_arrays(D.build(n_bits, y_bits, oracle), n_bits, y_bits)
    B = N.shape[0]
    xg = np.full_like(xo, 0xA5A5A5A5); yg = np.full_like(yo, 0xA5A5A5A5)
    ctx.dlog_prove(n_bits, y_bits, B, N, g, ni, s, r, xg, yg)
    bad = [b for b in range(B) if not (np.array_equal(xo[b], xg[b]) and np.array_equal(yo[b], yg[b]))]
    assert not bad, bad


@pytest.mark.parametrize("n_bits,y_bits", D.SHAPES)
def test_dlog_verify_cases(ctx, oracle, n_bits, y_bits):
    """the verdicts of the whole batch (two blocks of k_dlog_hash, a ragged last claim of both segments of the merged launch) and of its
    prefixes one item past one claim — claims are 32 / 16 / 8 / 4 items up to 2048 bits, 16 / 8 / 4 / 2 at 4096 — and of one proof alone"""
    rows = D.build(n_bits, y_bits, oracle)
    arrs = D.arrays(rows, n_bits, y_bits)
    vo = D.oracle_verdicts(n_bits, y_bits, oracle)
    for B in (D.ROWS, 17 if n_bits == 4096 else 33, 1):
        vg = np.full(B, 9, np.uint8)
        ctx.dlog_verify(n_bits, y_bits, B, *(a[:B] for a in arrs), vg)
        assert np.array_equal(vo[:B], vg), (B, [(rows[b][0], int(vo[b]), int(vg[b])) for b in range(B) if vo[b] != vg[b]])


def test_dlog_verify_cases_one_stream(ctx, oracle):
    """4096-bit keys on the path of a call that fills the GPU (batch > 16 CUs): pre-checks and challenge in one k_dlog_hash launch on the one
    stream, one launch per exponentiation.  The smallest number of tiles of the batch of 70 that crosses that bound on this board."""
    import torch
    n_bits, y_bits = 4096, 768
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = 16 * cus // D.ROWS + 1
    assert tiles * D.ROWS > 16 * cus >= (tiles - 1) * D.ROWS
    big = [np.tile(a, (tiles, 1)) for a in D.arrays(D.build(n_bits, y_bits, oracle), n_bits, y_bits)]
    vo = np.tile(D.oracle_verdicts(n_bits, y_bits, oracle), tiles)
    vg = np.full(tiles * D.ROWS, 9, np.uint8)
    ctx.dlog_verify(n_bits, y_bits, tiles * D.ROWS, *big, vg)
    bad = np.nonzero(vo != vg)[0]
    assert bad.size == 0, (bad.size, [(int(b), int(vo[b]), int(vg[b])) for b in bad[:8]])
