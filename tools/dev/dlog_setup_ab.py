"""The set-up of DLogStatements (h1 of Jacobi symbol -1, secret, h2 = (h1^-1)^secret mod N), timed three ways (README):
one board, one process, the 2048-bit fixture modulus N = p q for every statement, host-pointer calls throughout.
  (a) setup    zkp_dlog_statement_setup_seeded_batch: 32 bytes and the moduli in, (g, ni, secret) out — the one call
  (b) symbol   J  zkp_jacobi_batch of `--statements` values under N: no factors, no ladder
               L  the reference's route on the same GPU: two zkp_legendre_batch calls, under p and under q (1024-bit primes in 2048-bit
                  rows, the narrowest the modexp ladder takes), the product on the host
               J and L alternate (J L J L ...) after one warm-up of each; both must give the same symbols
  (c) loop     the host loop of tests/cpp/test_zkproofs.cpp's dlog_statement() for `--loop-statements` statements on one core, per statement:
               G  as that program runs it — every mod_pow a one-item GPU call (two per attempt for the symbol, one for h2), mod_inv on the host
               P  the same loop on CPython integers alone (pow()): a stand-in for the reference's GMP loop, slower than GMP, no GPU
Medians are reported with every sample.  Appends three JSON lines to profiles/dlog_setup/ab.jsonl (or --out).
Usage: python tools/dev/dlog_setup_ab.py [--statements 4096] [--rounds 7] [--loop-statements 64] [--label TEXT]"""
import argparse
import hashlib
import importlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
zkp = importlib.import_module("zk-paillier_amd")
from oracle.py_model import FIXTURE_N, FIXTURE_P, FIXTURE_Q  # noqa: E402


def board():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return {"name": p.name, "arch": getattr(p, "gcnArchName", None), "uuid": str(getattr(p, "uuid", "")), "sclk_mhz": int(torch.cuda.clock_rate())}
    except Exception as err:
        return {"error": str(err)}


def limbs(values, words):
    return np.frombuffer(b"".join(v.to_bytes(4 * words, "little") for v in values), dtype=np.uint32).reshape(len(values), words).copy()


def unlimbs(row):
    return int.from_bytes(row.tobytes(), "little")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--statements", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loop-statements", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dlog_setup", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    n_bits, B = 2048, a.statements
    kw = n_bits // 32
    N, p, q = FIXTURE_N, FIXTURE_P, FIXTURE_Q
    ctx = zkp.Context(0)
    seed = hashlib.sha256(b"dlog-setup-ab").digest()
    common = {"statements": B, "n_bits": n_bits, "pointers": "host", "board": board(), "label": a.label, "rounds": a.rounds}
    records = []

    # ---- (a) the one seeded call
    Nrows = limbs([N] * B, kw)
    g, ni, sec, st = np.zeros((B, kw), np.uint32), np.zeros((B, kw), np.uint32), np.zeros((B, 8), np.uint32), np.zeros(B, np.uint8)

    def setup():
        ctx.dlog_statement_setup_seeded(n_bits, B, Nrows, seed, 0, g, ni, sec, st)

    setup()                                                  # warm-up
    ta = [timed(setup) for _ in range(a.rounds)]
    assert not st.any()
    for b in (0, B // 2, B - 1):                             # spot check on the host: ni g^secret == 1 mod N
        assert unlimbs(ni[b]) * pow(unlimbs(g[b]), unlimbs(sec[b]), N) % N == 1
    records.append({"measurement": "setup_seeded_call", **common, "ms": round(statistics.median(ta), 3), "samples_ms": [round(t, 3) for t in ta],
                    "per_statement_us": round(statistics.median(ta) * 1e3 / B, 2)})

    # ---- (b) the symbol alone
    rnd = random.Random(1)
    vals = [rnd.randrange(1, N) for _ in range(B)]
    av, nv = limbs(vals, kw), limbs([N], kw)
    ap_, aq_ = limbs([v % p for v in vals], kw), limbs([v % q for v in vals], kw)
    pv, qv = limbs([p], kw), limbs([q], kw)
    sj, sp, sq = (np.zeros(B, np.int32) for _ in range(3))

    def jac():
        ctx.jacobi(n_bits, B, av, nv, 0, sj)

    def leg():
        ctx.legendre(n_bits, B, ap_, pv, 0, sp)
        ctx.legendre(n_bits, B, aq_, qv, 0, sq)
        return sp * sq

    jac(); leg()                                             # warm-up of each
    tj, tl = [], []
    for _ in range(a.rounds):
        tj.append(timed(jac)); tl.append(timed(leg))
    assert np.array_equal(sj, sp * sq) and set(sj.tolist()) == {-1, 1}
    records.append({"measurement": "symbol_alone", **common, "jacobi_ms": round(statistics.median(tj), 3), "two_legendre_ms": round(statistics.median(tl), 3),
                    "jacobi_samples_ms": [round(t, 3) for t in tj], "two_legendre_samples_ms": [round(t, 3) for t in tl], "same_symbols": True,
                    "legendre_rows": "1024-bit primes zero-padded in 2048-bit rows"})

    # ---- (c) the host loop, per statement on one core
    S = a.loop_statements
    one_a, one_out, one_e = np.zeros((1, kw), np.uint32), np.zeros((1, kw), np.uint32), np.zeros((1, kw), np.uint32)

    def gpu_pow(base, exp, mod, mod_limbs):
        one_a[:] = limbs([base % mod], kw); one_e[:] = limbs([exp], kw)
        ctx.modexp(n_bits, n_bits, 1, one_a, one_e, kw, mod_limbs, 0, one_out)
        return unlimbs(one_out[0])

    def loop(powmod):
        r = random.Random(2)
        attempts = 0
        for _ in range(S):
            while True:
                h1 = r.randrange(1, N - 1)
                attempts += 1
                lp = 1 if powmod(h1, (p - 1) // 2, p, pv) == 1 else -1
                lq = 1 if powmod(h1, (q - 1) // 2, q, qv) == 1 else -1
                if lp * lq == -1:
                    break
            secret = r.getrandbits(256)
            h2 = powmod(pow(h1, -1, N), secret, N, nv)
            assert 0 < h2 < N
        return attempts

    loop(gpu_pow)                                            # warm-up
    tg = [timed(lambda: loop(gpu_pow)) for _ in range(3)]
    tp = [timed(lambda: loop(lambda b, e, m, _: pow(b, e, m))) for _ in range(3)]
    records.append({"measurement": "host_loop_per_statement", **common, "loop_statements": S, "attempts": loop(lambda b, e, m, _: pow(b, e, m)),
                    "one_item_gpu_calls_ms_per_statement": round(statistics.median(tg) / S, 3), "cpython_pow_ms_per_statement": round(statistics.median(tp) / S, 3),
                    "one_item_gpu_calls_samples_ms": [round(t, 1) for t in tg], "cpython_pow_samples_ms": [round(t, 1) for t in tp],
                    "note": "CPython pow() is slower than the reference's GMP"})

    for rec in records:
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
