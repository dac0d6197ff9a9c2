"""NiCorrectKeyProof proving for a batch of distinct keys, timed three ways (README): one board, one process, host
arrays, the median of `--rounds` warmed calls with every sample, at each shape of --shapes (n_bits:keys, default 2048:4096,4096:512).
  (A) the new call   zkp_correct_key_ni_prove_batch: n, rho, key preparation, 22 half-width ladder rows per key and the CRT on the GPU; with the
                     share of the call that is not the ladder (wall time against the ladder's time between HIP events, zkp_timing_get)
  (B) alternative    the strongest route without it on the same GPU: rho (oracle/py_model.correct_key_rho) and d = n^-1 mod phi in host
                     integers, then ONE zkp_modexp_batch of 11 B rows at mod_bits = n_bits with per-row exponent and modulus; the host part and
                     the GPU call reported separately
  (C) shipped route  NiCorrectKeyProof::proof (host/zkproofs.hpp) once per key on a SAMPLE of --sample keys: tools/dev/ck_prove_ab_host.cpp,
                     compiled by this tool; reported per key, with proof_batch over the same sample
The keys are DISTINCT but not independent: ordered pairs (p, q), p != q, of a small pool of random primes (65 primes of 1024 bits give 4160
keys) — the arithmetic does not care, and generating 8192 primes in CPython would take longer than the measurement.  The pool is kept in
--pool (a JSON file, made on first use).  Every output of (A) is compared with (B)'s.  The board and its clock are read AFTER the runs.
Appends JSON lines to profiles/ck_prove/ab.jsonl (or --out).
Usage: python tools/dev/ck_prove_ab.py [--shapes 2048:4096,4096:512] [--rounds 7] [--sample 64] [--label TEXT] [--prepare] [--only-a]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
zkp = importlib.import_module("zk-paillier_amd")
from oracle import py_model as pm  # noqa: E402

HOST_SRC = os.path.join(ROOT, "tools", "dev", "ck_prove_ab_host.cpp")
HOST_EXE = os.path.join(ROOT, "build", "ck_prove_ab_host")


def board():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return {"name": p.name, "arch": getattr(p, "gcnArchName", None), "uuid": str(getattr(p, "uuid", "")), "sclk_mhz": int(torch.cuda.clock_rate())}
    except Exception as err:
        return {"error": str(err)}


def limbs(values, words):
    return np.frombuffer(b"".join(v.to_bytes(4 * words, "little") for v in values), dtype=np.uint32).reshape(len(values), words).copy()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "samples_ms": [round(t, 3) for t in ts]}


def prime_pool(path, bits, count):
    import helpers as H
    pool = json.load(open(path)) if os.path.exists(path) else {}
    have = [int(x) for x in pool.get(str(bits), [])]
    if len(have) < count:
        d = pm.Drbg(b"ck-prove-ab-%d" % bits)
        have = []
        while len(have) < count:
            c = H.gen_prime(d, bits)
            if c not in have:
                have.append(c)
        pool[str(bits)] = [str(x) for x in have]
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(pool, f)
    return have[:count]


def pool_size(keys):
    k = 2
    while k * (k - 1) < keys:
        k += 1
    return k


def keys_from(pool, count):
    out = [(p, q) for p in pool for q in pool if p != q][:count]
    assert len(out) == count == len(set(out))
    return out


def build_host():
    pkg = os.path.join(ROOT, "zk-paillier_amd")
    if os.path.exists(HOST_EXE) and os.path.getmtime(HOST_EXE) >= max(os.path.getmtime(HOST_SRC), os.path.getmtime(os.path.join(pkg, "host", "zkproofs.hpp"))):
        return
    os.makedirs(os.path.dirname(HOST_EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", HOST_SRC, "-o", HOST_EXE, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])


def measure(ctx, n_bits, B, a):
    kw, hw = n_bits // 32, n_bits // 64
    keys = keys_from(prime_pool(a.pool, n_bits // 2, pool_size(B)), B)
    salt = pm.SALT_STRING
    common = {"n_bits": n_bits, "keys": B, "pointers": "host", "label": a.label, "rounds": a.rounds, "distinct_keys_from_primes": pool_size(B)}
    records = []

    # ---- (A)
    pv, qv = limbs([k[0] for k in keys], hw), limbs([k[1] for k in keys], hw)
    on, osg, ost = np.zeros((B, kw), np.uint32), np.zeros((B, 11, kw), np.uint32), np.zeros(B, np.uint8)

    def new_call():
        ctx.correct_key_ni_prove(n_bits, B, pv, qv, salt, on, osg, ost)

    new_call()
    ta = [timed(new_call) for _ in range(a.rounds)]
    assert not ost.any()
    walls, ladders = [], []
    for _ in range(a.rounds):
        ctx.timing_reset(True)
        walls.append(timed(new_call))
        ladder_ms, _, modexps = ctx.timing_get()
        assert modexps == 22 * B, modexps
        ladders.append(ladder_ms)
    ctx.timing_reset(False)
    w, l = statistics.median(walls), statistics.median(ladders)
    records.append({"measurement": "A_new_call", **common, **stats(ta), "per_key_us": round(statistics.median(ta) * 1e3 / B, 2), "ladder_rows": 22 * B,
                    "ladder_mod_bits": 2048, "ladder_exp_bits": n_bits // 2,
                    "timed": {"call_ms": round(w, 3), "ladder_ms": round(l, 3), "not_ladder_ms": round(w - l, 3), "not_ladder_share": round((w - l) / w, 4)},
                    "note": "not_ladder = n, hash, key preparation, split, finish, the ladder's set-up kernel, launches, copies"})
    if a.only_a:
        return records

    # ---- (B)
    host = {}

    def host_part():
        ns = [p * q for p, q in keys]
        host["rho"] = [pm.correct_key_rho(n, salt) for n in ns]
        host["d"] = [pow(n, -1, (p - 1) * (q - 1)) for n, (p, q) in zip(ns, keys)]
        host["n"] = ns

    th = [timed(host_part) for _ in range(3)]
    base = limbs([r for rho in host["rho"] for r in rho], kw)
    ex = np.repeat(limbs(host["d"], kw), 11, axis=0)
    md = np.repeat(limbs(host["n"], kw), 11, axis=0)
    out = np.zeros((11 * B, kw), np.uint32)

    def ladder():
        ctx.modexp(n_bits, n_bits, 11 * B, base, ex, kw, md, kw, out)

    ladder()
    tb = [timed(ladder) for _ in range(a.rounds)]
    assert np.array_equal(out.reshape(B, 11, kw), osg) and np.array_equal(on, limbs(host["n"], kw)), "(A) and (B) differ"
    records.append({"measurement": "B_host_d_one_modexp", **common, "modexp": stats(tb), "host_rho_and_d": stats(th), "rows": 11 * B, "mod_bits": n_bits,
                    "exp_bits": n_bits, "total_ms": round(statistics.median(tb) + statistics.median(th), 3),
                    "a_over_b_gpu_call": round(statistics.median(ta) / statistics.median(tb), 4),
                    "a_over_b_total": round(statistics.median(ta) / (statistics.median(tb) + statistics.median(th)), 4),
                    "note": "host part: CPython integers and hashlib on one core; d is a secret in host memory on this route"})

    # ---- (C)
    S = min(a.sample, B)
    with tempfile.NamedTemporaryFile("w", suffix=".keys", delete=False) as f:
        for p, q in keys[:S]:
            f.write("%d %d\n" % (p, q))
    try:
        res = subprocess.run([HOST_EXE, f.name], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(f.name)
    assert res.returncode == 0, res.stdout + res.stderr
    host_result = {k: v for k, v in json.loads(res.stdout).items() if k != "keys"}
    records.append({"measurement": "C_shipped_proof_per_key_SAMPLE", **common, "sample_keys": S, **host_result,
                    "note": "a SAMPLE of the keys, one run: NiCorrectKeyProof::proof per key (host hash, host d, one 11-row zkp_modexp_batch each); per key"})
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048:4096,4096:512")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--pool", default=os.path.join(ROOT, "build", "ck_prove_ab_primes.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ck_prove", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    ap.add_argument("--prepare", action="store_true", help="make the prime pool and the host program, measure nothing (needs no GPU)")
    ap.add_argument("--only-a", action="store_true", help="measurement (A) alone (under a profiler)")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    build_host()
    if a.prepare:
        for n_bits, B in shapes:
            prime_pool(a.pool, n_bits // 2, pool_size(B))
        return
    ctx = zkp.Context(0)
    records = []
    for n_bits, B in shapes:
        records += measure(ctx, n_bits, B, a)
    b = board()
    for rec in records:
        rec["board_after_run"] = b
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
