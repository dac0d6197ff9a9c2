"""Host time of the small-proof entry points, for whichever build $ZKP_HIP_LIB names (point $ZKP_HIP_LAT_LIB and $ZKP_HIP_MID_LIB at the
same build: calls of a few proofs run there).  The device code of two builds being equal, what can differ between them is the host side of a
call, and that shows in small calls: 2048-bit keys, one shared key, batches of 1, 64 and 4096, pageable host arrays, the host clock around
the synchronising call, second call onwards.  Timed: ZeroProof, MulProof and CorrectMessageProof (K = 4) prove and verify, VerlinProof and
CompositeDLogProof verify, zkp_legendre_batch, zkp_dlog_statement_setup_seeded_batch, zkp_mul_proof_prove_seeded_batch.  The operands are
random values below the modulus from a fixed seed — the same bytes for every build; whether a verdict accepts is the test suite's business,
not this script's.  One process measures one build; a job script runs the builds alternately (A B A B ...) and the same build against
itself (A A A A) for the spread.  Prints — and appends to --out — one JSON line: the label, the board and its clock, the median in ms
per entry point and batch.
Usage: ZKP_HIP_LIB=... python tools/dev/small_proof_ab.py --label parent [--calls 7] [--out profiles/small_proof_layer/ab.jsonl]"""
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
N_BITS, KW, K = 2048, 64, 4
ZW = KW + zkp.capi.Z1_EXTRA_LIMBS


def board():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return {"name": p.name, "arch": getattr(p, "gcnArchName", None), "uuid": str(getattr(p, "uuid", "")), "sclk_mhz": int(torch.cuda.clock_rate())}
    except Exception as e:      # the record says so instead of failing the measurement
        return {"error": repr(e)}


def calls(ctx, B, rng, seed):
    """(name, thunk) per timed entry point at batch B"""
    from oracle import py_model as pm      # (the fixture key only)
    n = L.int_to_limbs(pm.FIXTURE_N, KW)[None, :]
    n_rows = np.ascontiguousarray(np.repeat(n, B, axis=0))

    def below(words, *shape):       # random values with the top word clear: below n (words = KW) or n^2 (words = 2 KW)
        v = np.zeros((B, *shape, words), np.uint32)
        v[..., :words - 1] = rng.integers(0, 2 ** 32, (B, *shape, words - 1), dtype=np.uint32)
        return v

    def out(*shape, dtype=np.uint32):
        return np.zeros((B, *shape), dtype)

    c, r, rp = below(2 * KW), below(KW), below(KW)
    z, a, v = out(2 * KW), out(2 * KW), out(dtype=np.uint8)
    yield "zero_prove", lambda: ctx.zero_proof_prove(N_BITS, B, n, 0, c, r, rp, z, a)
    yield "zero_verify", lambda: ctx.zero_proof_verify(N_BITS, B, n, 0, c, z, a, v)

    ea, eb, ec = below(2 * KW), below(2 * KW), below(2 * KW)
    ma, mb, ra, rb, rc, d, rd = (below(KW) for _ in range(7))
    f, z1, z2, ed, edb, st = out(KW), out(2 * KW), out(2 * KW), out(2 * KW), out(2 * KW), out(dtype=np.uint8)
    yield "mul_prove", lambda: ctx.mul_proof_prove(N_BITS, B, n, 0, ea, eb, ec, ma, mb, ra, rb, rc, d, rd, f, z1, z2, ed, edb, st)
    yield "mul_verify", lambda: ctx.mul_proof_verify(N_BITS, B, n, 0, ea, eb, ec, f, z1, z2, ed, edb, v)
    yield "mul_prove_seeded", lambda: ctx.mul_proof_prove_seeded(N_BITS, B, n, 0, ea, eb, ec, ma, mb, ra, rb, rc, seed, 0, f, z1, z2, ed, edb, st)

    valid = np.zeros((B, K, KW), np.uint32); valid[:, :, :2] = rng.integers(1, 2 ** 32, (B, K, 2), dtype=np.uint32)
    msg = np.ascontiguousarray(valid[np.arange(B), np.arange(B) % K])
    cr, cw, es, zs = below(KW), below(KW), rng.integers(0, 2 ** 32, (B, K - 1, 8), dtype=np.uint32), below(KW, K - 1)
    ct, ev, zv, av = out(2 * KW), out(K, 8), out(K, KW), out(K, 2 * KW)
    yield "correct_message_k4_prove", lambda: ctx.correct_message_prove(N_BITS, B, K, n, 0, valid, msg, cr, es, zs, cw, ct, ev, zv, av, st)
    yield "correct_message_k4_verify", lambda: ctx.correct_message_verify(N_BITS, B, K, n, 0, valid, ct, ev, zv, av, v)

    cp, phx, pha, rz = below(2 * KW), below(2 * KW), below(2 * KW), below(2 * KW)
    zz = [np.zeros((B, ZW), np.uint32) for _ in range(3)]
    for q in zz: q[:, :KW] = rng.integers(0, 2 ** 32, (B, KW), dtype=np.uint32)
    yield "verlin_verify", lambda: ctx.verlin_proof_verify(N_BITS, B, n, 0, c, cp, phx, pha, zz[0], zz[1], zz[2], rz, v)

    y_bits = 544
    g, ni, x, y = below(KW), below(KW), below(KW), below(y_bits // 32)
    yield "dlog_verify", lambda: ctx.dlog_verify(N_BITS, y_bits, B, n_rows, g, ni, x, y, v)

    sym = out(dtype=np.int32)
    yield "legendre", lambda: ctx.legendre(N_BITS, B, r, n, 0, sym, st)
    og, oni, osec = out(KW), out(KW), out(8)
    yield "dlog_statement_setup_seeded", lambda: ctx.dlog_statement_setup_seeded(N_BITS, B, n_rows, seed, 0, og, oni, osec, st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--calls", type=int, default=7, help="timed calls per entry point and batch, after one untimed call")
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_proof_layer", "ab.jsonl"))
    a = ap.parse_args()
    seed = hashlib.sha256(b"small-proof-ab").digest()
    ctx = zkp.Context(0)
    rec = {"label": a.label, "board": board(), "n_bits": N_BITS, "shared_key": True, "pointers": "host",
           "calls": a.calls, "median_ms": {}}
    for B in (int(b) for b in a.batches.split(",")):
        for name, call in calls(ctx, B, np.random.default_rng(11), seed):
            try:
                call()
            except Exception as e:      # recorded, and the other entry points are still measured
                rec.setdefault("errors", {})[f"{name}/{B}"] = repr(e)
                continue
            samples = []
            for _ in range(a.calls):
                t = time.perf_counter()
                call()
                samples.append(round((time.perf_counter() - t) * 1e3, 3))
            rec["median_ms"][f"{name}/{B}"] = round(float(np.median(samples)), 3)
    ctx.close()
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fo:
        fo.write(line + "\n")


if __name__ == "__main__":
    main()
