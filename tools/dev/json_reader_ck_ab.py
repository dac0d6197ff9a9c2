"""A/B/C record of the NiCorrectKeyProof document verifier, one board, one process, order A B C A B C after one
warm-up of each:
  A  the two-call route: zkp_json_correct_key_proof_batch into a host array (tokenised on the host), then zkp_correct_key_ni_verify_batch
     on host arrays;
  B  zkp_correct_key_ni_verify_json_batch: the text uploaded once and tokenised on the device, no limb on the host;
  C  zkp_correct_key_ni_verify_batch on the device-resident batch the documents were written from: the floor.
Keys and roots are the benchmark's distinct-key material (bench.py configs[3]: random odd 2048-bit moduli, random roots below them — every
proof is rejected, and k_ck_check does the same work whatever the verdict); the documents are the writer's
(zkp_json_write_correct_key_proof_batch on the device-resident roots).  B's split (upload, scan, convert, verify) comes from HIP events on
the ctx stream (zkp_diag_last_json_scan_ms).  Appends one JSON line to profiles/json_reader/ck_ab.jsonl (or --out).
Usage: python tools/dev/json_reader_ck_ab.py [--keys 65536] [--rounds 2] [--label TEXT]"""
import argparse
import importlib
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_reader", "ck_ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    import torch
    n_bits, kw, B, M2 = 2048, 64, a.keys, 11
    salt = b"KZen"
    rng = np.random.default_rng(11)
    n = rng.integers(0, 2 ** 32, (B, kw), dtype=np.uint32)
    n[:, 0] |= 1; n[:, -1] |= 0x80000000
    sigma = rng.integers(0, 2 ** 32, (B, M2, kw), dtype=np.uint32)
    sigma[:, :, -1] &= 0x3FFFFFFF
    ctx = zkp.Context(0)
    dn = torch.from_numpy(n.view(np.int32)).cuda(); dsig = torch.from_numpy(sigma.view(np.int32)).cuda()
    text, off, _ = ctx.json_write_correct_key_proof(n_bits, B, dsig, None)
    doc_off = np.ascontiguousarray(off[:-1]); doc_len = np.ascontiguousarray(off[1:] - off[:-1])
    sb = (zkp.capi.C.c_uint8 * len(salt)).from_buffer_copy(salt)
    lib, P = ctx.lib, zkp.capi.ptr

    def run_a():
        back = np.empty((B, M2, kw), np.uint32)
        st = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
        t = time.perf_counter()
        ctx.check(lib.zkp_json_correct_key_proof_batch(ctx.h, P(text), P(doc_off), P(doc_len), n_bits, B, P(back), P(st), 0))
        t_read = time.perf_counter()
        ctx.check(lib.zkp_correct_key_ni_verify_batch(ctx.h, n_bits, B, P(n), P(back), sb, len(salt), P(v), 0))
        t_end = time.perf_counter()
        return (t_end - t) * 1e3, (t_read - t) * 1e3, st, v

    def run_b():
        st = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
        t = time.perf_counter()
        ctx.check(lib.zkp_correct_key_ni_verify_json_batch(ctx.h, P(text), P(doc_off), P(doc_len), B, n_bits, P(n), sb, len(salt), P(st), P(v), 0))
        ms = (time.perf_counter() - t) * 1e3
        return ms, ctx.last_json_scan_ms(), ctx.last_json_scan(), st, v

    def run_c():
        v = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        ctx.synchronize()
        t = time.perf_counter()
        ctx.check(lib.zkp_correct_key_ni_verify_batch(ctx.h, n_bits, B, P(dn), P(dsig), sb, len(salt), P(v), zkp.capi.ZKP_F_DEVICE_PTRS))
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
        ms, split, scan, st_, v_ = run_b(); Bs.append(ms); Bsplit.append(dict(zip(("upload_ms", "scan_ms", "convert_ms", "verify_ms"), split)))
        same = same and bool(np.array_equal(st_, sta) and np.array_equal(v_, va))
        ms, v_ = run_c(); Cs.append(ms)
        same = same and bool(np.array_equal(v_, va))
    rec = dict(keys=B, n_bits=n_bits, text_bytes=int(off[-1]), order="A B C " * a.rounds, warm_up="one A, one B and one C before the timed rounds",
               a_ms=A, a_read_ms=Ar, b_ms=Bs, b_split=Bsplit, c_ms=Cs, a_median=float(np.median(A)), b_median=float(np.median(Bs)), c_median=float(np.median(Cs)),
               fast_docs=scan[0], fallback_docs=scan[1], same_statuses_and_verdicts=same, accepted=int((va == 1).sum()), sclk_mhz=sclk_mhz())
    if a.label is not None:
        rec["label"] = a.label
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ctx.close()
    if not same:
        sys.exit("A, B and C disagree on a status or a verdict")


if __name__ == "__main__":
    main()
