"""A/B record of seeded proving for the sigma proofs, one board, order A B A B, for ZeroProof and for
CorrectMessageProof with K = 4:
  A  the nonce-input call (zkp_zero_proof_prove_batch / zkp_correct_message_prove_batch) on pageable host arrays that hold every nonce (the
     call as it was), second call onwards;
  B  the seeded call on the same statements: the nonces are expanded on the device.
The host sampling that A needs on top is NOT in A's figure.  A's nonces are the ones B expands (zkp_nonce_sample_batch), so both write the
same bytes.  Appends one JSON line per proof kind to profiles/seeded_sigma/ab.jsonl (or --out).
Usage: python tools/dev/seeded_sigma_ab.py [--proofs 4096] [--rounds 2]"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
zkp = importlib.import_module("zk-paillier_amd")
L = zkp.limbs


def record(ctx, what, B, rounds, run_a, run_b, outputs):
    run_a(); ref = [o.copy() for o in outputs]
    run_b()
    same = all(np.array_equal(r, o) for r, o in zip(ref, outputs))
    A, Bs = [], []
    for _ in range(rounds):
        A.append(run_a()); Bs.append(run_b())
    return dict(what=what, proofs=B, n_bits=2048, order="A B " * rounds, a_ms=A, b_ms=Bs, a_median=float(np.median(A)), b_median=float(np.median(Bs)),
                a_spread=float(max(A) - min(A)), b_spread=float(max(Bs) - min(Bs)), same_bytes=bool(same), residue=ctx.witness_residue(),
                geometry=ctx.last_geometry())


def timed(f):
    def run():
        t = time.perf_counter()
        f()
        return (time.perf_counter() - t) * 1e3
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_sigma", "ab.jsonl"))
    a = ap.parse_args()
    n_bits, kw, B, K = 2048, 64, a.proofs, 4
    from oracle import py_model as pm      # (the fixture key only: range_proof_ni.rs:141-145)
    n = L.int_to_limbs(pm.FIXTURE_N, kw)[None, :]
    rng = np.random.default_rng(7)
    seed = hashlib.sha256(b"seeded-sigma-ab").digest()
    ctx = zkp.Context(0)
    recs = []

    # ZeroProof: c is any value below n^2 (the prover does not check its statement), r < 2^2016 < n
    c = np.zeros((B, 2 * kw), np.uint32); c[:, :2 * kw - 1] = rng.integers(0, 2 ** 32, (B, 2 * kw - 1), dtype=np.uint32)
    r = np.zeros((B, kw), np.uint32); r[:, :63] = rng.integers(0, 2 ** 32, (B, 63), dtype=np.uint32)
    rp = np.zeros((B, kw), np.uint32)
    ctx.nonce_sample(zkp.SEEDED_KIND_ZERO, n_bits, B, 1, n, 0, seed, 0, [rp, None, None, None], None)
    z, aa, st = np.zeros((B, 2 * kw), np.uint32), np.zeros((B, 2 * kw), np.uint32), np.zeros(B, np.uint8)
    recs.append(record(ctx, "zero", B, a.rounds, timed(lambda: ctx.zero_proof_prove(n_bits, B, n, 0, c, r, rp, z, aa)),
                       timed(lambda: ctx.zero_proof_prove_seeded(n_bits, B, n, 0, c, r, seed, 0, z, aa, st)), [z, aa]))

    # CorrectMessageProof, K = 4: the message of proof b is entry b % 4 of its list
    valid = np.zeros((B, K, kw), np.uint32); valid[:, :, :2] = rng.integers(1, 2 ** 32, (B, K, 2), dtype=np.uint32)
    msg = np.ascontiguousarray(valid[np.arange(B), np.arange(B) % K])
    f = [np.zeros((B, kw), np.uint32), np.zeros((B, kw), np.uint32), np.zeros((B, K - 1, 8), np.uint32), np.zeros((B, K - 1, kw), np.uint32)]
    ctx.nonce_sample(zkp.SEEDED_KIND_CORRECT_MESSAGE, n_bits, B, K, n, 0, seed, 0, f, None)
    outs = [np.zeros(s, np.uint32) for s in ((B, 2 * kw), (B, K, 8), (B, K, kw), (B, K, 2 * kw))]
    st = np.zeros(B, np.uint8)
    recs.append(record(ctx, "correct_message_k4", B, a.rounds,
                       timed(lambda: ctx.correct_message_prove(n_bits, B, K, n, 0, valid, msg, f[0], f[2], f[3], f[1], *outs, st)),
                       timed(lambda: ctx.correct_message_prove_seeded(n_bits, B, K, n, 0, valid, msg, seed, 0, *outs, st)), outs))
    assert not st.any()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fo:
        for rec in recs:
            print(json.dumps(rec))
            fo.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
