"""A/B record of the JSON writers, one board, one process, order A B A B after one warm-up of each:
  A  what a caller can do without them: download the limbs of a device-resident prove result, convert every number with
     zkp_limbs_to_decimal_batch (one call per width: kw and 2 kw limbs), assemble the 4096 whole RangeProofNi documents on the host
     (bytes.join over slices of the padded rows, one thread);
  B  zkp_json_write_range_proof_ni_batch reading the same device-resident batch: sizing call + writing call.
Both end with the same bytes in host memory (checked).  Writes one JSON line to profiles/json_writer/ab.jsonl (or --out).
Usage: python tools/dev/json_writer_ab.py [--proofs 4096] [--rounds 2] [--label TEXT]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_writer", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    import torch
    n_bits, kw, B, EF = 2048, 64, a.proofs, 128
    from oracle import py_model as pm      # (the fixture key only: range_proof_ni.rs:141-145)
    rng = np.random.default_rng(7)
    seed = hashlib.sha256(b"json-writer-ab").digest()
    ctx = zkp.Context(0)
    host = zkp.RangeBatch(n_bits, B, EF, shared_key=True)
    host.n[0] = L.int_to_limbs(pm.FIXTURE_N, kw)
    host.range[:, :8] = rng.integers(0, 2 ** 32, (B, 8), dtype=np.uint32)
    host.range[:, 7] |= 0x80000000
    x = np.zeros((B, kw), np.uint32); r = np.zeros((B, kw), np.uint32)
    x[:, :7] = rng.integers(0, 2 ** 32, (B, 7), dtype=np.uint32)
    r[:, :63] = rng.integers(0, 2 ** 32, (B, 63), dtype=np.uint32)
    host.ciphertext[:] = rng.integers(0, 2 ** 32, host.ciphertext.shape, dtype=np.uint32)      # (the statement's ciphertext is only written out here)
    pb = host.to("cuda")
    dx = torch.from_numpy(x.view(np.int32)).cuda(); dr = torch.from_numpy(r.view(np.int32)).cuda()
    t = time.perf_counter()
    ctx.range_ni_prove_seeded(pb.struct(), dx, dr, seed, 0, None, None, None, device=True)
    ctx.synchronize()
    prove_ms = (time.perf_counter() - t) * 1e3

    def decimals(arr):
        rows = arr.reshape(-1, arr.shape[-1])
        pitch = ctx.decimal_pitch(rows.shape[1])
        out = np.zeros((rows.shape[0], pitch), np.uint8); ln = np.zeros(rows.shape[0], np.uint32)
        ctx.check(ctx.lib.zkp_limbs_to_decimal_batch(ctx.h, zkp.capi.ptr(rows), rows.shape[1], rows.shape[1], rows.shape[0], zkp.capi.ptr(out), pitch, zkp.capi.ptr(ln), 0))
        flat = out.reshape(-1).tobytes()
        start = (np.arange(rows.shape[0], dtype=np.int64) + 1) * pitch - ln
        return [flat[s:s + n] for s, n in zip(start.tolist(), ln.tolist())]

    def run_a():
        t = time.perf_counter()
        h = pb.to(None)                                               # D2H of every limb
        for f in ("n", "range", "ciphertext", "c1", "c2", "resp_w1", "resp_r1", "resp_w2", "resp_r2"):
            setattr(h, f, getattr(h, f).view(np.uint32))
        narrow = decimals(np.concatenate([h.n.reshape(-1, kw), h.range, h.resp_w1.reshape(-1, kw), h.resp_r1.reshape(-1, kw), h.resp_w2.reshape(-1, kw),
                                          h.resp_r2.reshape(-1, kw)]))
        wide = decimals(np.concatenate([h.ciphertext, h.c1.reshape(-1, 2 * kw), h.c2.reshape(-1, 2 * kw)]))
        t_conv = time.perf_counter()
        rows = B * EF
        n_s, rg = narrow[0], narrow[1:1 + B]
        w1, r1, w2, r2 = (narrow[1 + B + k * rows:1 + B + (k + 1) * rows] for k in range(4))
        ct, c1, c2 = wide[:B], wide[B:B + rows], wide[B + rows:]
        kind = h.resp_kind.reshape(-1).tolist(); jj = h.resp_j.reshape(-1).tolist()
        docs = []
        for b in range(B):
            lo, hi = b * EF, (b + 1) * EF
            resp = [b'{"Open":{"w1":"%s","r1":"%s","w2":"%s","r2":"%s"}}' % (w1[i], r1[i], w2[i], r2[i]) if kind[i] == 0 else
                    b'{"Mask":{"j":%d,"masked_x":"%s","masked_r":"%s"}}' % (jj[i], w1[i], r1[i]) for i in range(lo, hi)]
            docs.append(b'{"ek":{"n":"%s"},"range":"%s","ciphertext":"%s","encrypted_pairs":{"c1":["%s"],"c2":["%s"]},"proof":[%s],"error_factor":%d}' % (
                n_s, rg[b], ct[b], b'","'.join(c1[lo:hi]), b'","'.join(c2[lo:hi]), b",".join(resp), EF))
        text = b"".join(docs)
        t_end = time.perf_counter()
        return (t_end - t) * 1e3, (t_conv - t) * 1e3, text

    def run_b():
        t = time.perf_counter()
        text, off, _ = ctx.json_write_range_proof_ni(pb.struct(), 0, None, device=True)
        return (time.perf_counter() - t) * 1e3, text

    _, _, ta = run_a()
    _, tb = run_b()
    same = ta == tb.tobytes()
    A, Ac, Bs = [], [], []
    for _ in range(a.rounds):
        ms, conv, _ = run_a(); A.append(ms); Ac.append(conv)
        Bs.append(run_b()[0])
    rec = dict(proofs=B, n_bits=n_bits, error_factor=EF, text_bytes=len(ta), order="A B " * a.rounds, warm_up="one A and one B before the timed rounds",
               a_ms=A, a_download_and_convert_ms=Ac, a_assembly="python bytes.join, one thread", b_ms=Bs, a_median=float(np.median(A)), b_median=float(np.median(Bs)),
               a_spread=float(max(A) - min(A)), b_spread=float(max(Bs) - min(Bs)), same_bytes=bool(same), prove_seeded_device_ms=prove_ms,
               b_share_of_1575_ms_prove=float(np.median(Bs)) / 1575.0)
    if a.label is not None:
        rec["label"] = a.label
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
