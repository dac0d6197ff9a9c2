"""A/B/C record of the CompositeDLogProof document verifier, one board, one process, order A B C A B C after one
warm-up of each:
  A  the three-call route: zkp_json_dlog_statement_batch and zkp_json_dlog_proof_batch with flags 0 (tokenised and converted on the host,
     host arrays), then zkp_dlog_verify_batch on those host arrays;
  B  zkp_dlog_verify_json_batch: the text uploaded once, both documents scanned on the device, no limb on the host;
  C  zkp_dlog_verify_batch on the device-resident limbs the documents were written from: the floor.
The pairs are honest proofs: a handful of moduli (products of two random odd numbers: the verifier's work does not depend on the
factorisation), g random below N, ni = g^-s mod N, the proofs made by zkp_dlog_prove_batch on the device and written from there by
the two writers, decimal form.  Every verdict must be ACCEPT on all three routes.  B's split (upload, statements, proofs, domain check and
verify) comes from HIP events on the ctx stream (zkp_diag_last_json_scan_ms).  Appends one JSON line to profiles/json_reader/dlog_ab.jsonl
(or --out).
Usage: python tools/dev/json_dlog_ab.py [--pairs 65536] [--rounds 2] [--label TEXT]"""
import argparse
import importlib
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
zkp = importlib.import_module("zk-paillier_amd")


def sclk_mhz():
    """the board's current shader clock, read only (None when the query is not available)"""
    try:
        import torch
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def limbs(values, words):
    return np.frombuffer(b"".join(v.to_bytes(4 * words, "little") for v in values), dtype=np.uint32).reshape(len(values), words).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_reader", "dlog_ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    import torch
    n_bits, y_bits, B = 2048, 768, a.pairs
    kw, yw = n_bits // 32, y_bits // 32
    rnd = random.Random(4)
    moduli = [(rnd.getrandbits(1024) | (1 << 1023) | 1) * (rnd.getrandbits(1024) | (1 << 1023) | 1) for _ in range(8)]
    rows = []
    for k in range(256):                       # 256 distinct statements, tiled to the batch (the kernels do not notice)
        N = moduli[k % len(moduli)]
        while True:
            g = rnd.randrange(2, N)
            try:
                inv = pow(g, -1, N)
                break
            except ValueError:
                pass
        s = rnd.getrandbits(256)
        rows.append((N, g, pow(inv, s, N), s))
    pick = [rows[b % len(rows)] for b in range(B)]
    cuda = lambda arr: torch.from_numpy(arr.view(np.int32)).cuda()
    dN, dg, dni = (cuda(limbs([r[i] for r in pick], kw)) for i in range(3))
    dsec = cuda(limbs([r[3] for r in pick], 8))
    dr = cuda(np.random.default_rng(5).integers(0, 2 ** 32, (B, 16), dtype=np.uint32))
    dx = torch.zeros((B, kw), dtype=torch.int32, device="cuda"); dy = torch.zeros((B, yw), dtype=torch.int32, device="cuda")
    ctx = zkp.Context(0)
    ctx.dlog_prove(n_bits, y_bits, B, dN, dg, dni, dsec, dr, dx, dy)
    ts, os_, _ = ctx.json_write_dlog_statement(n_bits, B, dN, dg, dni)
    tp, op, _ = ctx.json_write_dlog_proof(n_bits, y_bits, B, dx, dy)
    text = np.concatenate([ts, tp])
    st_off = np.ascontiguousarray(os_[:-1]); st_len = np.ascontiguousarray(os_[1:] - os_[:-1])
    pf_off = np.ascontiguousarray(op[:-1] + np.uint64(ts.size)); pf_len = np.ascontiguousarray(op[1:] - op[:-1])
    lib, P = ctx.lib, zkp.capi.ptr

    def run_a():
        N_, g_, ni_, x_ = (np.empty((B, kw), np.uint32) for _ in range(4)); y_ = np.empty((B, yw), np.uint32)
        s1 = np.full(B, 9, np.uint8); s2 = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
        t = time.perf_counter()
        ctx.check(lib.zkp_json_dlog_statement_batch(ctx.h, P(text), P(st_off), P(st_len), n_bits, B, 0, P(N_), P(g_), P(ni_), P(s1), 0))
        ctx.check(lib.zkp_json_dlog_proof_batch(ctx.h, P(text), P(pf_off), P(pf_len), n_bits, y_bits, B, 0, P(x_), P(y_), P(s2), 0))
        t_read = time.perf_counter()
        ctx.check(lib.zkp_dlog_verify_batch(ctx.h, n_bits, y_bits, B, P(N_), P(g_), P(ni_), P(x_), P(y_), P(v), 0))
        t_end = time.perf_counter()
        return (t_end - t) * 1e3, (t_read - t) * 1e3, np.maximum(s1, s2), v

    def run_b():
        st = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
        t = time.perf_counter()
        ctx.check(lib.zkp_dlog_verify_json_batch(ctx.h, P(text), P(st_off), P(st_len), P(pf_off), P(pf_len), B, n_bits, y_bits, 0, P(st), P(v), 0))
        ms = (time.perf_counter() - t) * 1e3
        return ms, ctx.last_json_scan_ms(), ctx.last_json_scan(), st, v

    def run_c():
        v = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        ctx.synchronize()
        t = time.perf_counter()
        ctx.check(lib.zkp_dlog_verify_batch(ctx.h, n_bits, y_bits, B, P(dN), P(dg), P(dni), P(dx), P(dy), P(v), zkp.capi.ZKP_F_DEVICE_PTRS))
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, v.cpu().numpy()

    _, _, sta, va = run_a()
    _, _, scan, stb, vb = run_b()
    _, vc = run_c()
    same = bool(np.array_equal(sta, stb) and np.array_equal(va, vb) and np.array_equal(va, vc) and not sta.any())
    A, Ar, Bs, Bsplit, Cs = [], [], [], [], []
    for _ in range(a.rounds):
        ms, read, st_, v_ = run_a(); A.append(ms); Ar.append(read)
        same = same and bool(np.array_equal(st_, sta) and np.array_equal(v_, va))
        ms, split, scan, st_, v_ = run_b(); Bs.append(ms); Bsplit.append(dict(zip(("upload_ms", "statements_ms", "proofs_ms", "check_and_verify_ms"), split)))
        same = same and bool(np.array_equal(st_, sta) and np.array_equal(v_, va))
        ms, v_ = run_c(); Cs.append(ms)
        same = same and bool(np.array_equal(v_, va))
    rec = dict(pairs=B, n_bits=n_bits, y_bits=y_bits, form="dec", text_bytes=int(text.size), order="A B C " * a.rounds,
               warm_up="one A, one B and one C before the timed rounds", a_ms=A, a_read_ms=Ar, b_ms=Bs, b_split=Bsplit, c_ms=Cs, a_median=float(np.median(A)),
               b_median=float(np.median(Bs)), c_median=float(np.median(Cs)), fast_docs=scan[0], fallback_docs=scan[1], same_statuses_and_verdicts=same,
               accepted=int((va == 1).sum()), sclk_mhz=sclk_mhz())
    if a.label is not None:
        rec["label"] = a.label
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ctx.close()
    if not same or rec["accepted"] != B:
        sys.exit("A, B and C disagree on a status or a verdict, or an honest proof was not accepted")


if __name__ == "__main__":
    main()
