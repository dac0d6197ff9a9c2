"""A/B record of seeded proving, one board, order A B A B:
  A  zkp_range_ni_prove_batch on pageable host arrays that hold the whole witness (the call as it was), second call onwards;
  B  zkp_range_ni_prove_seeded_batch on the same statements: the witness is expanded on the device.
The host sampling that A needs on top (host_api.prove in profiles/bench_r06_final.json: 36.6 ms) is NOT in A's figure here.
Writes one JSON line to profiles/seeded_prove/ab.jsonl (or --out).  Usage: python tools/dev/seeded_prove_ab.py [--proofs 4096] [--rounds 2]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_prove", "ab.jsonl"))
    a = ap.parse_args()
    n_bits, kw, B, EF = 2048, 64, a.proofs, 128
    from oracle import py_model as pm      # (the fixture key only: range_proof_ni.rs:141-145)
    n = pm.FIXTURE_N
    rng = np.random.default_rng(7)
    seed = hashlib.sha256(b"seeded-prove-ab").digest()
    ctx = zkp.Context(0)
    pb = zkp.RangeBatch(n_bits, B, EF, shared_key=True)
    pb.n[0] = L.int_to_limbs(n, kw)
    pb.range[:, :8] = rng.integers(0, 2 ** 32, (B, 8), dtype=np.uint32)
    pb.range[:, 7] |= 0x80000000
    wt = zkp.make_range_witness(n_bits, B, EF)
    wt.x[:, :7] = rng.integers(0, 2 ** 32, (B, 7), dtype=np.uint32)          # x < 2^224 < range / 3
    wt.r[:, :63] = rng.integers(0, 2 ** 32, (B, 63), dtype=np.uint32)        # r < 2^2016 < n
    ctx.range_sample_witness(pb.struct(), seed, 0, wt.w1, wt.w2, wt.r1, wt.r2, None, device=False)      # A's witness: the one B expands
    status = np.zeros(B, np.uint8)

    def run_a():
        t = time.perf_counter()
        ctx.range_ni_prove(pb.struct(), wt.struct(), None, None, status, device=False)
        return (time.perf_counter() - t) * 1e3

    def run_b():
        t = time.perf_counter()
        ctx.range_ni_prove_seeded(pb.struct(), wt.x, wt.r, seed, 0, None, None, status, device=False)
        return (time.perf_counter() - t) * 1e3

    run_a(); ref = {f: getattr(pb, f).copy() for f in ("c1", "resp_w1", "resp_kind")}
    run_b()
    same = all(np.array_equal(ref[f], getattr(pb, f)) for f in ref)
    A, Bs = [], []
    for _ in range(a.rounds):
        A.append(run_a()); Bs.append(run_b())
    rec = dict(proofs=B, n_bits=n_bits, order="A B " * a.rounds, a_ms=A, b_ms=Bs, a_median=float(np.median(A)), b_median=float(np.median(Bs)),
               a_spread=float(max(A) - min(A)), b_spread=float(max(Bs) - min(Bs)), same_bytes=bool(same), residue=ctx.witness_residue(),
               geometry=ctx.last_geometry())
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
