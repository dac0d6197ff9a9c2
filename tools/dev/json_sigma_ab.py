"""A/B/C record of the sigma-proof document verifier for ZeroProof, CiphertextProof, VerlinProof and MulProof, one board, one
process, order A B C A B C after one warm-up of each, per proof type:
  A  zkp_sigma_verify_json_batch: the text uploaded once, both documents scanned on the device, no limb on the host;
  B  the type's zkp_*_verify_batch on the device-resident limbs the documents were written from — code that this feature does not touch: the floor;
  C  the three-call route: zkp_json_sigma_batch twice with flags 0 (tokenised and converted on the host, host arrays), then the type's
     zkp_*_verify_batch on those host arrays.
What a reader cares about is A - B, the cost of reading text on the device, and its ratio to C - B, the cost of reading it on the host.
The pairs are honest proofs under the reference's 2048-bit fixture key, one key row per pair, made by the type's zkp_*_prove_batch on the device and
written from there by zkp_json_write_sigma_batch, decimal form.  Every verdict must be ACCEPT on all three routes.  A's split (upload, statements,
proofs, domain check and verify) comes from HIP events on the ctx stream (zkp_diag_last_json_scan_ms).  Appends one JSON line per proof type to
profiles/json_reader/sigma_ab.jsonl (or --out).
Usage: python tools/dev/json_sigma_ab.py [--pairs 4096] [--rounds 3] [--label TEXT]"""
import argparse
import ctypes as C
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
from oracle.py_model import FIXTURE_N  # noqa: E402

NAMES = {9: "ZeroProof", 11: "CiphertextProof", 13: "VerlinProof", 15: "MulProof"}
EXTRA = zkp.capi.Z1_EXTRA_LIMBS


def sclk_mhz():
    """the board's current shader clock, read only (None when the query is not available)"""
    try:
        import torch
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def limbs(values, words):
    return np.frombuffer(b"".join(v.to_bytes(4 * words, "little") for v in values), dtype=np.uint32).reshape(len(values), words).copy()


def make_pairs(ctx, kind, B, n_bits, rnd):
    """-> (statement fields, proof fields): torch cuda tensors, honest proofs made on the device"""
    n, kw = FIXTURE_N, n_bits // 32
    st, pf = _make_pairs(ctx, kind, B, n, kw, rnd, keep := [])
    ctx.synchronize()              # the calls run on the ctx stream: every operand stays allocated (keep) until they have finished
    del keep
    return st, pf


def _make_pairs(ctx, kind, B, n, kw, rnd, keep):
    import torch
    n_bits = 32 * kw

    def hold(t):
        keep.append(t)
        torch.cuda.synchronize()   # torch fills its tensors on its own stream: done before the ctx stream reads or writes them
        return t
    cuda = lambda arr: hold(torch.from_numpy(arr.view(np.int32)).cuda())
    below = lambda: [rnd.randrange(2, n) for _ in range(B)]
    col = lambda v: cuda(limbs(v, kw))
    out = lambda w: hold(torch.zeros((B, w), dtype=torch.int32, device="cuda"))
    dn = col([n] * B)

    def enc(m, r):
        c = out(2 * kw)
        ctx.paillier_enc(n_bits, B, dn, kw, col(m), col(r), c)
        return c
    if kind == 9:
        r = below()
        c, z, a = enc([0] * B, r), out(2 * kw), out(2 * kw)
        ctx.zero_proof_prove(n_bits, B, dn, kw, c, col(r), col(below()), z, a)
        return [dn, c], [z, a]
    if kind == 11:
        x, r = below(), below()
        c, z1, z2, cp = enc(x, r), out(kw + EXTRA), out(2 * kw), out(2 * kw)
        ctx.ciphertext_proof_prove(n_bits, B, dn, kw, c, col(x), col(r), col(below()), col(below()), z1, z2, cp)
        return [dn, c], [z1, z2, cp]
    if kind == 13:
        wit, non = [col(below()) for _ in range(4)], [col(below()) for _ in range(4)]
        c, cp = enc(below(), below()), enc(below(), below())
        phi_x = [out(2 * kw), out(kw + EXTRA), out(kw + EXTRA), out(kw + EXTRA), out(2 * kw)]
        ctx.verlin_proof_prove(n_bits, B, dn, kw, c, cp, out(2 * kw), wit, wit, phi_x)          # phi_x = gen_phi of the witness: the prover's phi_a of its "nonces"
        pf = [out(2 * kw), out(kw + EXTRA), out(kw + EXTRA), out(kw + EXTRA), out(2 * kw)]
        ctx.verlin_proof_prove(n_bits, B, dn, kw, c, cp, phi_x[0], wit, non, pf)
        return [dn, c, cp, phi_x[0]], pf
    a, b = below(), below()
    r_a, r_b, r_c = below(), below(), below()
    e = [enc(a, r_a), enc(b, r_b), enc([x * y % n for x, y in zip(a, b)], r_c)]
    pf = [out(kw)] + [out(2 * kw) for _ in range(4)]
    st = hold(torch.zeros(B, dtype=torch.uint8, device="cuda"))
    ctx.mul_proof_prove(n_bits, B, dn, kw, *e, col(a), col(b), col(r_a), col(r_b), col(r_c), col(below()), col(below()), *pf, st)
    assert not st.cpu().numpy().any()
    return [dn] + e, pf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_reader", "sigma_ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    import torch
    n_bits, B = 2048, a.pairs
    kw = n_bits // 32
    ctx = zkp.Context(0)
    lib, P, DEV = ctx.lib, zkp.capi.ptr, zkp.capi.ZKP_F_DEVICE_PTRS
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    failed = False
    for kind, name in NAMES.items():
        st_dev, pf_dev = make_pairs(ctx, kind, B, n_bits, random.Random(kind))
        ts, os_, _ = ctx.json_write_sigma(kind - 1, n_bits, B, st_dev)
        tp, op, _ = ctx.json_write_sigma(kind, n_bits, B, pf_dev)
        text = np.concatenate([ts, tp])
        st_off = np.ascontiguousarray(os_[:-1]); st_len = np.ascontiguousarray(os_[1:] - os_[:-1])
        pf_off = np.ascontiguousarray(op[:-1] + np.uint64(ts.size)); pf_len = np.ascontiguousarray(op[1:] - op[:-1])
        verify = getattr(lib, {9: "zkp_zero_proof_verify_batch", 11: "zkp_ciphertext_proof_verify_batch", 13: "zkp_verlin_proof_verify_batch",
                               15: "zkp_mul_proof_verify_batch"}[kind])

        def run_a():
            st = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
            t = time.perf_counter()
            ctx.check(lib.zkp_sigma_verify_json_batch(ctx.h, kind, P(text), P(st_off), P(st_len), P(pf_off), P(pf_len), B, n_bits, 0, P(st), P(v), 0))
            ms = (time.perf_counter() - t) * 1e3
            return ms, ctx.last_json_scan_ms(), ctx.last_json_scan(), st, v

        def run_b():
            v = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
            ctx.synchronize()
            t = time.perf_counter()
            ctx.check(verify(ctx.h, n_bits, B, P(st_dev[0]), kw, *[P(x) for x in st_dev[1:] + pf_dev], P(v), DEV))
            ctx.synchronize()
            return (time.perf_counter() - t) * 1e3, v.cpu().numpy()

        def run_c():
            sh = [np.empty(tuple(x.shape), np.uint32) for x in st_dev]; ph = [np.empty(tuple(x.shape), np.uint32) for x in pf_dev]
            s1 = np.full(B, 9, np.uint8); s2 = np.full(B, 9, np.uint8); v = np.full(B, 9, np.uint8)
            fs, fp = ctx._sigma_fields(kind - 1, sh), ctx._sigma_fields(kind, ph)
            t = time.perf_counter()
            ctx.check(lib.zkp_json_sigma_batch(ctx.h, kind - 1, P(text), P(st_off), P(st_len), n_bits, B, 0, C.byref(fs), P(s1), 0))
            ctx.check(lib.zkp_json_sigma_batch(ctx.h, kind, P(text), P(pf_off), P(pf_len), n_bits, B, 0, C.byref(fp), P(s2), 0))
            t_read = time.perf_counter()
            ctx.check(verify(ctx.h, n_bits, B, P(sh[0]), kw, *[P(x) for x in sh[1:] + ph], P(v), 0))
            t_end = time.perf_counter()
            return (t_end - t) * 1e3, (t_read - t) * 1e3, np.maximum(s1, s2), v

        _, _, scan, sta, va = run_a()
        _, vb = run_b()
        _, _, stc, vc = run_c()
        same = bool(np.array_equal(sta, stc) and np.array_equal(va, vb) and np.array_equal(va, vc) and not sta.any())
        A, Asplit, Bs, Cs, Cr = [], [], [], [], []
        for _ in range(a.rounds):
            ms, split, scan, st_, v_ = run_a(); A.append(ms); Asplit.append(dict(zip(("upload_ms", "statements_ms", "proofs_ms", "check_and_verify_ms"), split)))
            same = same and bool(np.array_equal(st_, sta) and np.array_equal(v_, va))
            ms, v_ = run_b(); Bs.append(ms)
            same = same and bool(np.array_equal(v_, va))
            ms, read, st_, v_ = run_c(); Cs.append(ms); Cr.append(read)
            same = same and bool(np.array_equal(st_, sta) and np.array_equal(v_, va))
        am, bm, cm = float(np.median(A)), float(np.median(Bs)), float(np.median(Cs))
        rec = dict(proof=name, pairs=B, n_bits=n_bits, form="dec", text_bytes=int(text.size), order="A B C " * a.rounds,
                   warm_up="one A, one B and one C before the timed rounds", a_ms=A, a_split=Asplit, b_ms=Bs, c_ms=Cs, c_read_ms=Cr, a_median=am, b_median=bm,
                   c_median=cm, device_text_cost_ms=am - bm, host_text_cost_ms=cm - bm, fast_docs=scan[0], fallback_docs=scan[1], same_statuses_and_verdicts=same,
                   accepted=int((va == 1).sum()), sclk_mhz=sclk_mhz())
        if a.label is not None:
            rec["label"] = a.label
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        failed = failed or not same or rec["accepted"] != B
        del st_dev, pf_dev
    ctx.close()
    if failed:
        sys.exit("A, B and C disagree on a status or a verdict, or an honest proof was not accepted")


if __name__ == "__main__":
    main()
