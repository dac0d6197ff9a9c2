"""A/B record of seeded proving for VerlinProof and MulProof, one board, order A B A B:
  A  the nonce-input call (zkp_verlin_proof_prove_batch / zkp_mul_proof_prove_batch) on pageable host arrays that hold every nonce (the
     call as it was), second call onwards;
  B  the seeded call on the same statements: the nonces are expanded on the device, r_a / r_d by k_nonce_coprime.
The host sampling and the host GCD loop that A needs on top are NOT in A's figure.  A's nonces are the ones B expands
(zkp_nonce_sample_coprime_batch), so both write the same bytes.  Appends one JSON line per proof kind to profiles/seeded_coprime/ab.jsonl
(or --out).  Under `rocprofv3 --kernel-trace --stats` (no counters in that run) the same program gives the time of k_nonce_coprime.
Usage: python tools/dev/seeded_coprime_ab.py [--proofs 4096] [--rounds 2]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_coprime", "ab.jsonl"))
    a = ap.parse_args()
    n_bits, kw, B = 2048, 64, a.proofs
    zw = kw + zkp.capi.Z1_EXTRA_LIMBS
    from oracle import py_model as pm      # (the fixture key only: range_proof_ni.rs:141-145)
    n = L.int_to_limbs(pm.FIXTURE_N, kw)[None, :]
    rng = np.random.default_rng(7)
    seed = hashlib.sha256(b"seeded-coprime-ab").digest()
    ctx = zkp.Context(0)
    recs = []

    def below_n():         # < 2^2016 < n; a random value of that size is coprime to the fixture key
        v = np.zeros((B, kw), np.uint32); v[:, :63] = rng.integers(0, 2 ** 32, (B, 63), dtype=np.uint32)
        return v

    def below_nn():        # any value below n^2: the provers do not check their statements
        v = np.zeros((B, 2 * kw), np.uint32); v[:, :2 * kw - 1] = rng.integers(0, 2 ** 32, (B, 2 * kw - 1), dtype=np.uint32)
        return v

    # VerlinProof
    c, cp, phi_x = below_nn(), below_nn(), below_nn()
    wit = [below_n() for _ in range(4)]
    non = [np.zeros((B, kw), np.uint32) for _ in range(4)]
    st = np.full(B, 9, np.uint8)
    ctx.nonce_sample_coprime(zkp.SEEDED_KIND_VERLIN, n_bits, B, n, 0, seed, 0, non, st)
    assert not st.any()
    outs = [np.zeros((B, w), np.uint32) for w in (2 * kw, zw, zw, zw, 2 * kw)]
    recs.append(record(ctx, "verlin", B, a.rounds, timed(lambda: ctx.verlin_proof_prove(n_bits, B, n, 0, c, cp, phi_x, wit, non, outs)),
                       timed(lambda: ctx.verlin_proof_prove_seeded(n_bits, B, n, 0, c, cp, phi_x, wit, seed, 0, outs, st)), outs))
    assert not st.any()

    # MulProof
    e = [below_nn() for _ in range(3)]
    mwit = [below_n() for _ in range(5)]
    mnon = [np.zeros((B, kw), np.uint32) for _ in range(2)]
    ctx.nonce_sample_coprime(zkp.SEEDED_KIND_MUL, n_bits, B, n, 0, seed, 0, mnon + [None, None], st)
    assert not st.any()
    mouts = [np.zeros((B, w), np.uint32) for w in (kw, 2 * kw, 2 * kw, 2 * kw, 2 * kw)]
    recs.append(record(ctx, "mul", B, a.rounds, timed(lambda: ctx.mul_proof_prove(n_bits, B, n, 0, *e, *mwit, *mnon, *mouts, st)),
                       timed(lambda: ctx.mul_proof_prove_seeded(n_bits, B, n, 0, *e, *mwit, seed, 0, *mouts, st)), mouts))
    assert not st.any()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fo:
        for rec in recs:
            print(json.dumps(rec))
            fo.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
