"""A/B/C record of the document verifier, one board, one process, order A B A B after one warm-up of each:
  A  the two-call route: zkp_json_range_proof_ni_batch into host arrays (tokenised on the host), then zkp_range_ni_verify_batch on them;
  B  zkp_range_ni_verify_json_batch: the text uploaded once and tokenised on the device, no limb on the host;
  C  zkp_range_ni_verify_batch on the device-resident batch the documents were written from: the floor.
The documents are the writer's (zkp_json_write_range_proof_ni_batch on a seeded, device-resident prove result).  B's split (upload, scan,
convert, verify) comes from HIP events on the ctx stream (zkp_diag_last_json_scan_ms).  Appends one JSON line to
profiles/json_reader/ab.jsonl (or --out).
Usage: python tools/dev/json_reader_ab.py [--proofs 4096] [--rounds 2] [--label TEXT]"""
import argparse
import ctypes as C
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


def sclk_mhz():
    """the board's current shader clock, read only (None when the query is not available)"""
    try:
        import torch
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_reader", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    import torch
    n_bits, kw, B, EF = 2048, 64, a.proofs, 128
    from oracle import py_model as pm      # (the fixture key only)
    rng = np.random.default_rng(7)
    seed = hashlib.sha256(b"json-reader-ab").digest()
    ctx = zkp.Context(0)
    host = zkp.RangeBatch(n_bits, B, EF, shared_key=True)
    host.n[0] = L.int_to_limbs(pm.FIXTURE_N, kw)
    host.range[:, :8] = rng.integers(0, 2 ** 32, (B, 8), dtype=np.uint32)
    host.range[:, 7] |= 0x80000000
    x = np.zeros((B, kw), np.uint32); r = np.zeros((B, kw), np.uint32)
    x[:, :7] = rng.integers(0, 2 ** 32, (B, 7), dtype=np.uint32)
    x[:, 6] &= 0x0FFFFFFF                                                  # x < range / 3: honest statements
    r[:, :63] = rng.integers(0, 2 ** 32, (B, 63), dtype=np.uint32)
    pb = host.to("cuda")
    dx = torch.from_numpy(x.view(np.int32)).cuda(); dr = torch.from_numpy(r.view(np.int32)).cuda()
    ctx.paillier_enc(n_bits, B, pb.n, 0, dx, dr, pb.ciphertext)
    ctx.range_ni_prove_seeded(pb.struct(), dx, dr, seed, 0, None, None, None, device=True)
    text, off, _ = ctx.json_write_range_proof_ni(pb.struct(), 0, None, device=True)
    doc_off = np.ascontiguousarray(off[:-1]); doc_len = np.ascontiguousarray(off[1:] - off[:-1])
    vn = np.ascontiguousarray(host.n[0])
    lib, P = ctx.lib, zkp.capi.ptr

    def run_a():
        back = zkp.RangeBatch(n_bits, B, EF, shared_key=True)
        back.n[:] = host.n
        st = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
        s = back.struct()
        t = time.perf_counter()
        ctx.check(lib.zkp_json_range_proof_ni_batch(ctx.h, P(text), P(doc_off), P(doc_len), 0, C.byref(s), P(st), 0))
        t_read = time.perf_counter()
        ctx.check(lib.zkp_range_ni_verify_batch(ctx.h, C.byref(s), P(v), 0))
        t_end = time.perf_counter()
        return (t_end - t) * 1e3, (t_read - t) * 1e3, st, v

    def run_b():
        st = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
        t = time.perf_counter()
        ctx.check(lib.zkp_range_ni_verify_json_batch(ctx.h, P(text), P(doc_off), P(doc_len), B, n_bits, EF, 0, P(vn), P(st), P(v), 0))
        ms = (time.perf_counter() - t) * 1e3
        return ms, ctx.last_json_scan_ms(), ctx.last_json_scan(), st, v

    def run_c():
        v = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        s = pb.struct()
        ctx.synchronize()
        t = time.perf_counter()
        ctx.check(lib.zkp_range_ni_verify_batch(ctx.h, C.byref(s), P(v), zkp.capi.ZKP_F_DEVICE_PTRS))
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, v.cpu().numpy()

    _, _, sta, va = run_a()
    _, _, scan, stb, vb = run_b()
    _, vc = run_c()
    same = bool(np.array_equal(sta, stb) and np.array_equal(va, vb) and np.array_equal(va, vc) and not sta.any())
    A, Ar, Bs, Bsplit, Cs = [], [], [], [], []
    for _ in range(a.rounds):
        ms, read, _, _ = run_a(); A.append(ms); Ar.append(read)
        ms, split, scan, _, _ = run_b(); Bs.append(ms); Bsplit.append(dict(zip(("upload_ms", "scan_ms", "convert_ms", "verify_ms"), split)))
        Cs.append(run_c()[0])
    rec = dict(proofs=B, n_bits=n_bits, error_factor=EF, text_bytes=int(off[-1]), order="A B C " * a.rounds, warm_up="one A, one B and one C before the timed rounds",
               a_ms=A, a_read_ms=Ar, b_ms=Bs, b_split=Bsplit, c_ms=Cs, a_median=float(np.median(A)), b_median=float(np.median(Bs)), c_median=float(np.median(Cs)),
               fast_docs=scan[0], fallback_docs=scan[1], same_statuses_and_verdicts=same, accepted=int((va == 1).sum()), sclk_mhz=sclk_mhz())
    if a.label is not None:
        rec["label"] = a.label
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
