"""The interactive CorrectKey for a batch of sessions under distinct keys, timed three ways (README): one board, one
process, host arrays, K = 40, the median of `--rounds` warmed calls with every sample, at each shape of --shapes (n_bits:sessions, default
2048:512,4096:64).
  (A) the new calls  zkp_correct_key_challenge_seeded_batch and zkp_correct_key_prove_batch, each with the share of the call that is not the
                     ladder (wall time against the ladder's time between HIP events, zkp_timing_get), and zkp_correct_key_verify_seeded_batch
  (B1) host route    CorrectKey::challenge / CorrectKey::prove (host/zkproofs.hpp) once per session on a SAMPLE of --sample sessions:
                     tools/dev/ck_inter_ab_host.cpp, compiled by this tool; reported per session
  (B2) GPU route     the fairest route without the new calls on the same GPU: one zkp_modexp_batch per exponent shape over all sessions'
                     full-width rows with per-row moduli — verifier: 2 K B rows under the exponent n, then K B rows under the 256-bit e;
                     prover: 3 K B rows (z^n, sn^(phi - e mod phi), sn^(n^-1 mod phi)) — plus the host integers each needs (sampling, hashes,
                     products; phi, the two exponents, the gcds, the recombination's product), timed separately in CPython
The keys are the ordered pairs of a small pool of random primes, as tools/dev/ck_prove_ab.py makes them (its pool file is shared).  The
digests of (A) are compared with (B2)'s.  The board and its clock are read AFTER the runs.  Appends JSON lines to
profiles/ck_interactive/ab.jsonl (or --out).
Usage: python tools/dev/ck_inter_ab.py [--shapes 2048:512,4096:64] [--rounds 5] [--sample 8] [--label TEXT] [--prepare]"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
from math import gcd

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("ck_prove_ab", os.path.join(HERE, "ck_prove_ab.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)                      # (puts the repository root and tests/ on sys.path)
ROOT, zkp, pm = P.ROOT, P.zkp, P.pm
import ck_inter_model as M  # noqa: E402

HOST_SRC = os.path.join(ROOT, "tools", "dev", "ck_inter_ab_host.cpp")
HOST_EXE = os.path.join(ROOT, "build", "ck_inter_ab_host")
K = 40


def build_host():
    pkg = os.path.join(ROOT, "zk-paillier_amd")
    if os.path.exists(HOST_EXE) and os.path.getmtime(HOST_EXE) >= max(os.path.getmtime(HOST_SRC), os.path.getmtime(os.path.join(pkg, "host", "zkproofs.hpp"))):
        return
    os.makedirs(os.path.dirname(HOST_EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", HOST_SRC, "-o", HOST_EXE, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])


def with_ladder_share(ctx, fn, rounds, rows):
    walls, ladders = [], []
    for _ in range(rounds):
        ctx.timing_reset(True)
        walls.append(P.timed(fn))
        ladder_ms, _, modexps = ctx.timing_get()
        assert modexps == rows, (modexps, rows)
        ladders.append(ladder_ms)
    ctx.timing_reset(False)
    w, l = statistics.median(walls), statistics.median(ladders)
    return {"call_ms": round(w, 3), "ladder_ms": round(l, 3), "not_ladder_ms": round(w - l, 3), "not_ladder_share": round((w - l) / w, 4)}


def measure(ctx, n_bits, B, a):
    kw, hw = n_bits // 32, n_bits // 64
    keys = P.keys_from(P.prime_pool(a.pool, n_bits // 2, P.pool_size(B)), B)
    ns = [p * q for p, q in keys]
    common = {"n_bits": n_bits, "sessions": B, "K": K, "pointers": "host", "label": a.label, "rounds": a.rounds}
    seed = os.urandom(32)
    records = []

    # ---- (A)
    nv, pv, qv = P.limbs(ns, kw), P.limbs([k[0] for k in keys], hw), P.limbs([k[1] for k in keys], hw)
    sn, z = np.zeros((B, K, kw), np.uint32), np.zeros((B, K, kw), np.uint32)
    e, aid, proof = np.zeros((B, 8), np.uint32), np.zeros((B, 8), np.uint32), np.zeros((B, 8), np.uint32)
    st, err, verdict = np.zeros(B, np.uint8), np.zeros(B, np.uint8), np.zeros(B, np.uint8)

    def challenge():
        ctx.correct_key_challenge_seeded(n_bits, B, K, nv, kw, seed, 0, sn, e, z, aid, st)

    def prove():
        ctx.correct_key_prove(n_bits, B, K, pv, qv, sn, e, z, proof, err)

    def verify():
        ctx.correct_key_verify_seeded(n_bits, B, K, nv, kw, seed, 0, proof, verdict)

    challenge(); prove(); verify()
    assert not st.any() and not err.any() and np.array_equal(proof, aid) and (verdict == 1).all()
    ta = {name: [P.timed(f) for _ in range(a.rounds)] for name, f in (("challenge", challenge), ("prove", prove), ("verify", verify))}
    shares = {"challenge": with_ladder_share(ctx, challenge, a.rounds, 3 * K * B), "prove": with_ladder_share(ctx, prove, a.rounds, 6 * K * B)}
    records.append({"measurement": "A_new_calls", **common, "challenge_seeded": P.stats(ta["challenge"]), "prove": P.stats(ta["prove"]),
                    "verify_seeded": P.stats(ta["verify"]), "timed": shares,
                    "ladder_rows": {"challenge": "%d rows of %d-bit exponents and %d of 256 at mod_bits %d" % (2 * K * B, n_bits, K * B, max(n_bits, 2048)),
                                    "prove": "%d rows of %d-bit exponents at mod_bits 2048" % (6 * K * B, n_bits // 2)},
                    "note": "not_ladder = sampler, reductions, hashes, key preparation, split, finish, gcd, the ladder's set-up kernel, launches, copies"})

    # ---- (B2): the same sessions (the s, r of (A)'s stream), the GPU for the ladders, CPython for the rest
    host = {}

    def verifier_sampling():
        host["s"] = [[M.sample_below(seed, b, i, 0, ns[b]) for i in range(K)] for b in range(min(B, a.sample))]

    t_sampling = P.timed(verifier_sampling)       # (a SAMPLE: the ChaCha model in CPython is slow; the stream is needed only to compare)
    S = len(host["s"])
    snl = [[int.from_bytes(sn[b, i].tobytes(), "little") for i in range(K)] for b in range(B)]
    zl = [[int.from_bytes(z[b, i].tobytes(), "little") for i in range(K)] for b in range(B)]
    el = [int.from_bytes(e[b].tobytes(), "little") for b in range(B)]
    assert all(pow(host["s"][b][i], ns[b], ns[b]) == snl[b][i] for b in range(S) for i in (0, K - 1)), "(A)'s sn is not s^n of its stream"
    # verifier: stand-in operands of the right shape (random values below n), since s and r never leave the device in (A)
    rng = np.random.default_rng(1)
    vals = [[int.from_bytes(rng.bytes(kw * 4), "little") % ns[b] for _ in range(2 * K)] for b in range(B)]
    mb = max(n_bits, 2048)
    mw = mb // 32
    base_v = P.limbs([v for b in range(B) for v in vals[b][:K]] + [v for b in range(B) for v in vals[b][K:]], mw)
    mod_v = np.tile(np.repeat(P.limbs(ns, mw), K, axis=0), (2, 1))
    out_v, out_e = np.zeros((2 * K * B, mw), np.uint32), np.zeros((K * B, mw), np.uint32)

    def verifier_ladders():
        ctx.modexp(mb, n_bits, 2 * K * B, base_v, mod_v, mw, mod_v, mw, out_v)
        ctx.modexp(mb, 256, K * B, base_v[:K * B], erow, 8, mod_v[:K * B], mw, out_e)

    erow = np.repeat(e, K, axis=0).copy()
    verifier_ladders()
    tvl = [P.timed(verifier_ladders) for _ in range(a.rounds)]

    def verifier_host():
        for b in range(B):
            row = [int.from_bytes(out_v[b * K + i].tobytes(), "little") for i in range(K)]
            rn = [int.from_bytes(out_v[(B + b) * K + i].tobytes(), "little") for i in range(K)]
            pm.compute_digest([ns[b]] + row + rn)
            se = [int.from_bytes(out_e[b * K + i].tobytes(), "little") for i in range(K)]
            [(vals[b][K + i] * se[i]) % ns[b] for i in range(K)]
            pm.compute_digest(vals[b][:K])

    tvh = [P.timed(verifier_host) for _ in range(3)]
    records.append({"measurement": "B2_verifier_two_modexp_calls", **common, "modexp_calls": P.stats(tvl), "host_hashes_and_products": P.stats(tvh),
                    "host_sampling_model_ms_for_sample": round(t_sampling, 3), "sample_sessions": S,
                    "a_over_b_gpu_calls": round(statistics.median(ta["challenge"]) / statistics.median(tvl), 4),
                    "a_over_b_total": round(statistics.median(ta["challenge"]) / (statistics.median(tvl) + statistics.median(tvh)), 4),
                    "note": "host part: CPython integers and hashlib on one core, sampling NOT included (the OS RNG's cost is not this model's)"})

    def prover_host_before():
        host["exp"] = []
        for (p, q), n, ee in zip(keys, ns, el):
            phi = (p - 1) * (q - 1)
            host["exp"].append((n, phi - ee % phi, pow(n, -1, phi)))
        host["coprime"] = all(gcd(n, v) == 1 for n, row, zr in zip(ns, snl, zl) for v in row + zr)

    tpb = [P.timed(prover_host_before) for _ in range(3)]
    base_p = P.limbs([v for b in range(B) for v in zl[b]] + [v for b in range(B) for v in snl[b]] * 2, mw)
    exp_p = P.limbs([host["exp"][b][t] for t in range(3) for b in range(B) for _ in range(K)], mw)
    mod_p = np.tile(np.repeat(P.limbs(ns, mw), K, axis=0), (3, 1))
    out_p = np.zeros((3 * K * B, mw), np.uint32)

    def prover_ladder():
        ctx.modexp(mb, n_bits, 3 * K * B, base_p, exp_p, mw, mod_p, mw, out_p)

    prover_ladder()
    tpl = [P.timed(prover_ladder) for _ in range(a.rounds)]

    def prover_host_after():
        host["digest"] = []
        for b in range(B):
            o = [[int.from_bytes(out_p[(t * B + b) * K + i].tobytes(), "little") for i in range(K)] for t in range(3)]
            rn = [(x * y) % ns[b] for x, y in zip(o[0], o[1])]
            assert all(gcd(ns[b], v) == 1 for v in rn) and el[b] == pm.compute_digest([ns[b]] + snl[b] + rn)
            host["digest"].append(pm.compute_digest(o[2]))

    tpa = [P.timed(prover_host_after) for _ in range(3)]
    assert host["coprime"] and all(host["digest"][b] == int.from_bytes(proof[b].tobytes(), "little") for b in range(B)), "(A) and (B2) differ"
    th = statistics.median(tpb) + statistics.median(tpa)
    records.append({"measurement": "B2_prover_one_modexp_call", **common, "modexp_call": P.stats(tpl), "host_before": P.stats(tpb), "host_after": P.stats(tpa),
                    "rows": 3 * K * B, "mod_bits": mb, "exp_bits": n_bits,
                    "a_over_b_gpu_call": round(statistics.median(ta["prove"]) / statistics.median(tpl), 4),
                    "a_over_b_total": round(statistics.median(ta["prove"]) / (statistics.median(tpl) + th), 4),
                    "note": "host part: CPython integers and hashlib on one core; phi and both secret exponents are in host memory on this route"})

    # ---- (B1)
    with tempfile.NamedTemporaryFile("w", suffix=".keys", delete=False) as f:
        for p, q in keys[:min(a.sample, B)]:
            f.write("%d %d\n" % (p, q))
    try:
        res = subprocess.run([HOST_EXE, f.name], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(f.name)
    assert res.returncode == 0, res.stdout + res.stderr
    records.append({"measurement": "B1_host_composition_per_session_SAMPLE", **common, **json.loads(res.stdout),
                    "note": "a SAMPLE of the sessions, one run: CorrectKey::challenge and CorrectKey::prove per session (host sampling, hashes and "
                            "exponents, zkp_modexp_batch calls of 80 / 40 rows), against the batched host calls over the same sample"})
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048:512,4096:64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--pool", default=os.path.join(ROOT, "build", "ck_prove_ab_primes.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ck_interactive", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    ap.add_argument("--prepare", action="store_true", help="make the prime pool and the host program, measure nothing (needs no GPU)")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    build_host()
    if a.prepare:
        for n_bits, B in shapes:
            P.prime_pool(a.pool, n_bits // 2, P.pool_size(B))
        return
    ctx = zkp.Context(0)
    records = []
    for n_bits, B in shapes:
        records += measure(ctx, n_bits, B, a)
    b = P.board()
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
