"""Seeded Paillier key generation for a batch of keys, timed (README): one board, one process, host arrays, the median of
`--rounds` warmed calls with every sample, at each shape of --shapes (n_bits:keys, default 2048:4096,4096:512).
  (A) the call       zkp_paillier_keygen_seeded_batch at every setting of --chunks (the tuning quantities of csrc/zkp_api_prime.inc: the
                     least rows per slot and round and the rows a round aims at, set through zkp_diag_prime_search; the results are
                     compared: they must not depend on them), the settings alternating inside one process.  Per record: the call's time and the time per key; the ladder rows the call ran per prime found; the
                     share of the call that is not the ladder (wall time against the ladder's time between HIP events, zkp_timing_get).
  (B) one CPU core   the same rule in tests/prime_model.py (with its count of candidates that reach the strong tests per prime: what the
                     ladder rows per prime exceed by the filler rows of chunking), and gen_prime of tools/make_bench_keys.py, each on a
                     sample of --sample keys.  --cpu runs (B) alone and needs no GPU; it says which machine it ran on.
The model's keys of the sample are compared with the call's.  The board and its clock are read AFTER the runs.
Appends JSON lines to profiles/keygen/ab.jsonl (or --out).
A GPU run with --no-cpu leaves the first --sample keys in --keys; a later --cpu run holds the model to them.
Usage: python tools/dev/keygen_ab.py [--shapes 2048:4096,4096:512] [--chunks 4/32768,16/1] [--rounds 5] [--sample 16] [--label TEXT] [--cpu | --no-cpu] [--keys DIR]"""
import argparse
import importlib
import json
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
zkp = importlib.import_module("zk-paillier_amd")

SEED = bytes((11 * i + 5) & 0xFF for i in range(32))
FIRST_INDEX = 1 << 33
MR_ROUNDS = 5


def board():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return {"name": p.name, "arch": getattr(p, "gcnArchName", None), "uuid": str(getattr(p, "uuid", "")), "sclk_mhz": int(torch.cuda.clock_rate())}
    except Exception as err:
        return {"error": str(err)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "samples_ms": [round(t, 3) for t in ts]}


def to_ints(a):
    return [int.from_bytes(row.tobytes(), "little") for row in a]


def measure_gpu(ctx, n_bits, B, a):
    import ctypes as C
    hw, kw = n_bits // 64, n_bits // 32
    p, q, n, st = np.zeros((B, hw), np.uint32), np.zeros((B, hw), np.uint32), np.zeros((B, kw), np.uint32), np.zeros(B, np.uint8)
    lib = zkp.load()

    def call():
        ctx.paillier_keygen_seeded(n_bits, B, MR_ROUNDS, SEED, FIRST_INDEX, p, q, n, st)

    chunks = [tuple(int(v) for v in x.split("/")) for x in a.chunks.split(",")]           # (least rows per slot, rows a round aims at)
    times = {c: [] for c in chunks}
    walls = {c: [] for c in chunks}
    ladders = {c: [] for c in chunks}
    rows, rounds, first = {}, {}, None
    for c in chunks:                                            # warm every shape, and hold the results to each other
        assert lib.zkp_diag_prime_search(ctx.h, c[0], c[1], None, None) == 0
        call()
        assert not st.any()
        got = (p.copy(), q.copy(), n.copy())
        if first is None:
            first = got
        assert all(np.array_equal(x, y) for x, y in zip(first, got)), "the keys depend on the chunk size"
        r, k = C.c_uint64(), C.c_uint64()
        assert lib.zkp_diag_prime_search(ctx.h, -1, -1, C.byref(r), C.byref(k)) == 0
        rows[c], rounds[c] = r.value, k.value
    for _ in range(a.rounds):                                   # alternating
        for c in chunks:
            lib.zkp_diag_prime_search(ctx.h, c[0], c[1], None, None)
            times[c].append(timed(call))
    for _ in range(a.rounds):
        for c in chunks:
            lib.zkp_diag_prime_search(ctx.h, c[0], c[1], None, None)
            ctx.timing_reset(True)
            walls[c].append(timed(call))
            ladder_ms, _, modexps = ctx.timing_get()
            assert modexps == rows[c], (modexps, rows[c])
            ladders[c].append(ladder_ms)
    ctx.timing_reset(False)
    lib.zkp_diag_prime_search(ctx.h, 0, 0, None, None)
    records = []
    for c in chunks:
        w, l = statistics.median(walls[c]), statistics.median(ladders[c])
        records.append({"measurement": "A_keygen_call", "n_bits": n_bits, "keys": B, "mr_rounds": MR_ROUNDS, "pointers": "host", "label": a.label, "rounds": a.rounds,
                        "chunk_C": c[0], "target_rows": c[1], **stats(times[c]), "per_key_us": round(statistics.median(times[c]) * 1e3 / B, 2),
                        "ladder_rows": rows[c], "ladder_rounds": rounds[c], "ladder_rows_per_prime": round(rows[c] / (2 * B), 2),
                        "ladder_mod_bits": 2048, "ladder_exp_bits": n_bits // 2,
                        "timed": {"call_ms": round(w, 3), "ladder_ms": round(l, 3), "not_ladder_ms": round(w - l, 3), "not_ladder_share": round((w - l) / w, 4)},
                        "note": "not_ladder = starts, sieve, rows, tail, pick, the ladder's set-up kernel, one host read per round, launches, copies"})
    return records, (to_ints(first[0]), to_ints(first[1]))


def measure_cpu(n_bits, S, a, gpu_keys=None):
    import make_bench_keys as MB
    import prime_model as M
    st = []
    t0 = time.perf_counter()
    keys, _ = M.keygen(SEED, FIRST_INDEX, S, n_bits, MR_ROUNDS, st)
    model_ms = (time.perf_counter() - t0) * 1e3
    if gpu_keys is not None:
        assert [k[0] for k in keys] == gpu_keys[0][:S] and [k[1] for k in keys] == gpu_keys[1][:S], "the model's keys differ from the call's"
    strong = [s.get("strong", 0) for k in st for s in k]
    stream = MB.Stream(b"keygen-ab-%d" % n_bits)
    t0 = time.perf_counter()
    for _ in range(2 * S):
        MB.gen_prime(stream, n_bits // 2)
    bench_ms = (time.perf_counter() - t0) * 1e3
    return {"measurement": "B_one_cpu_core_SAMPLE", "n_bits": n_bits, "sample_keys": S, "mr_rounds": MR_ROUNDS, "label": a.label,
            "python_model_ms": round(model_ms, 1), "python_model_per_key_ms": round(model_ms / S, 2),
            "model_candidates_to_strong_tests_per_prime": round(sum(strong) / len(strong), 2),
            "make_bench_keys_gen_prime_ms": round(bench_ms, 1), "make_bench_keys_per_key_ms": round(bench_ms / S, 2),
            "checked_against_the_call": gpu_keys is not None,
            "cpu": platform.processor() or platform.machine(), "python": platform.python_version(),
            "note": "CPython integers on one core, one run; gen_prime draws afresh per candidate and runs 32 Miller-Rabin rounds on a survivor"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048:4096,4096:512")
    ap.add_argument("--chunks", default="4/32768,8/32768,4/16384,4/65536,16/1", help="C/target pairs: the least rows per slot and round, the rows a round aims at (1: a fixed chunk)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keygen", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    ap.add_argument("--cpu", action="store_true", help="measurement (B) alone; needs no GPU")
    ap.add_argument("--no-cpu", action="store_true", help="measurement (A) alone")
    ap.add_argument("--keys", default=os.path.join(ROOT, "build", "keygen_ab_keys"), help="directory: --no-cpu leaves the call's first --sample keys there, --cpu compares the model's with them")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    records = []
    if a.cpu:
        for n_bits, B in shapes:
            path = os.path.join(a.keys, "%d.json" % n_bits)
            keys = [[int(x) for x in col] for col in json.load(open(path))] if os.path.exists(path) else None
            records.append(measure_cpu(n_bits, min(a.sample, B, len(keys[0]) if keys else B), a, keys))
    else:
        ctx = zkp.Context(0)
        for n_bits, B in shapes:
            recs, keys = measure_gpu(ctx, n_bits, B, a)
            records += recs
            if not a.no_cpu:
                records.append(measure_cpu(n_bits, min(a.sample, B), a, keys))
            else:
                os.makedirs(a.keys, exist_ok=True)
                with open(os.path.join(a.keys, "%d.json" % n_bits), "w") as f:
                    json.dump([[str(x) for x in col[:a.sample]] for col in keys], f)
        b = board()
        for rec in records:
            rec["board_after_run"] = b
        ctx.close()
    for rec in records:
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
