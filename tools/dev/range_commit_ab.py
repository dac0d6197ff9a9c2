"""The verifier's commitment step of the interactive RangeProof, timed four ways (README): one board, one process, one
2048-bit shared key, e_len = 5, host-pointer calls throughout (what a service holds is bytes and limbs in host memory).
  commit   N  zkp_range_verifier_commit_seeded_batch: 32 bytes in, the commitments out
           C  the best composition without it: r sampled beforehand (not timed), SHA-256 of every e on the host (hashlib), the digests turned
              into limbs, one zkp_paillier_enc_batch
           S  one session at a time, as the single-session verifier_commit of the host API does it: SHA-256 on the host and ONE one-item
              zkp_paillier_enc_batch per session (the sampling and the host API's own BigInt conversions are not in the figure)
  verify   N  zkp_range_verify_commit_batch on the revealed (r, e)
           C  SHA-256 on the host, one zkp_paillier_enc_check_batch against the commitments
           S  one session at a time, as verify_commit does it: SHA-256 on the host, one one-item zkp_paillier_enc_batch, the comparison on the host
N and C alternate (N C N C ...) after one warm-up of each, `--rounds` timed calls each, medians reported with every sample; S is a loop of
`--sessions` calls, timed `--single-rounds` times after one warm-up loop.  All three must produce the same commitments and accept every session.
Appends two JSON lines to profiles/range_commit/ab.jsonl (or --out).
Usage: python tools/dev/range_commit_ab.py [--sessions 4096] [--rounds 7] [--single-rounds 3] [--label TEXT]"""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
zkp = importlib.import_module("zk-paillier_amd")
from oracle.py_model import FIXTURE_N  # noqa: E402


def board():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return {"name": p.name, "arch": getattr(p, "gcnArchName", None), "uuid": str(getattr(p, "uuid", "")), "sclk_mhz": int(torch.cuda.clock_rate())}
    except Exception as err:
        return {"error": str(err)}


def limbs(values, words):
    return np.frombuffer(b"".join(v.to_bytes(4 * words, "little") for v in values), dtype=np.uint32).reshape(len(values), words).copy()


def digest_limbs(e_rows, e_len, kw):
    """SHA-256 of every e on the host -> m [B][kw]"""
    out = np.zeros((len(e_rows), kw), np.uint32)
    for b, row in enumerate(e_rows):
        out[b, :8] = np.frombuffer(hashlib.sha256(row[:e_len].tobytes()).digest()[::-1], dtype=np.uint32)
    return out


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--single-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_commit", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    n_bits, e_len, B = 2048, 5, a.sessions
    kw = n_bits // 32
    ctx = zkp.Context(0)
    n = limbs([FIXTURE_N], kw)
    seed = hashlib.sha256(b"range-commit-ab").digest()

    # the (r, e) of the sessions: revealed once, so that all three routes commit to the same values
    r, e, st = np.zeros((B, kw), np.uint32), np.zeros((B, 32), np.uint8), np.zeros(B, np.uint8)
    ctx.range_verifier_reveal_seeded(n_bits, B, n, 0, e_len, seed, 0, r, e, st)
    assert not st.any()
    elen = np.full(B, e_len, np.uint8)

    com_n, com_c, com_s = (np.zeros((B, 2 * kw), np.uint32) for _ in range(3))
    v_n, v_c = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    one_c = np.zeros((1, 2 * kw), np.uint32)

    def commit_new():
        ctx.range_verifier_commit_seeded(n_bits, B, n, 0, e_len, seed, 0, com_n, st)

    def commit_composed():
        ctx.paillier_enc(n_bits, B, n, 0, digest_limbs(e, e_len, kw), r, com_c)

    def commit_single():
        for b in range(B):
            ctx.paillier_enc(n_bits, 1, n, 0, digest_limbs(e[b:b + 1], e_len, kw), r[b:b + 1], com_s[b:b + 1])

    def verify_new():
        ctx.range_verify_commit(n_bits, B, n, 0, com_n, r, e, elen, v_n)

    def verify_composed():
        ctx.paillier_enc_check(n_bits, B, n, 0, digest_limbs(e, e_len, kw), r, None, None, com_n, v_c)

    ok_single = [0]

    def verify_single():
        good = 0
        for b in range(B):
            ctx.paillier_enc(n_bits, 1, n, 0, digest_limbs(e[b:b + 1], e_len, kw), r[b:b + 1], one_c)
            good += bool(np.array_equal(one_c[0], com_n[b]))
        ok_single[0] = good

    records = []
    for step, new, composed, single in (("commit", commit_new, commit_composed, commit_single), ("verify_commit", verify_new, verify_composed, verify_single)):
        new(); composed(); single()                          # warm-up of each
        tn, tc = [], []
        for _ in range(a.rounds):
            tn.append(timed(new)); tc.append(timed(composed))
        ts = [timed(single) for _ in range(a.single_rounds)]
        if step == "commit":
            assert np.array_equal(com_n, com_c) and np.array_equal(com_n, com_s) and com_n.any()
        else:
            assert (v_n == zkp.VERDICT_ACCEPT).all() and (v_c == 1).all() and ok_single[0] == B
        rec = {"step": step, "sessions": B, "n_bits": n_bits, "e_len": e_len, "shared_key": True, "pointers": "host", "board": board(), "label": a.label,
               "new_ms": round(statistics.median(tn), 3), "composed_ms": round(statistics.median(tc), 3), "single_session_loop_ms": round(statistics.median(ts), 1),
               "new_samples_ms": [round(t, 3) for t in tn], "composed_samples_ms": [round(t, 3) for t in tc], "single_session_loop_samples_ms": [round(t, 1) for t in ts],
               "rounds": a.rounds, "single_rounds": a.single_rounds, "same_results": True}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
