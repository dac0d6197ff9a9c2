"""Paillier decryption of a batch, timed five ways (README): one board, one process, `--items` ciphertexts under the
2048-bit fixture key, host arrays, the median of `--rounds` warmed calls with every sample.
  (a) decrypt   zkp_paillier_open_batch with out_r = NULL: the two ladders under p^2 and q^2
  (b) open      the same with out_r: four ladder rows per item
  (c) parent    the route a caller had before this entry point: zkp_modexp_batch at mod_bits = 4096 with the exponent lambda under n^2, then
                L and the product by mu in Python integers on the host — the GPU call and the host part reported separately
  (d) cpython   the CRT formulas with CPython's pow() on one core, per item (a stand-in for a GMP loop, slower than GMP, no GPU)
  (e) share     what of (a) is not the ladder — key preparation, split, finish, and for host arrays the copies: the call's wall time against
                the ladder's time between HIP events (zkp_timing_get), with host arrays and with device arrays
Every output of (a), (b) and (c) is compared with what was encrypted.  Appends five JSON lines to profiles/paillier_dec/ab.jsonl (or --out).
Usage: python tools/dev/paillier_dec_ab.py [--items 4096] [--rounds 7] [--cpython-items 64] [--label TEXT]"""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time
from math import gcd

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
zkp = importlib.import_module("zk-paillier_amd")
from oracle.py_model import FIXTURE_N, FIXTURE_P, FIXTURE_Q  # noqa: E402


def board():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return {"name": p.name, "arch": getattr(p, "gcnArchName", None), "uuid": str(getattr(p, "uuid", "")), "sclk_mhz": int(torch.cuda.clock_rate())}
    except Exception as err:
        return {"error": str(err)}


def limbs(values, words):
    return np.frombuffer(b"".join(v.to_bytes(4 * words, "little") for v in values), dtype=np.uint32).reshape(len(values), words).copy()


def unlimbs(row):
    return int.from_bytes(row.tobytes(), "little")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(ts):
    return round(statistics.median(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cpython-items", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paillier_dec", "ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    n_bits, B = 2048, a.items
    kw, hw = n_bits // 32, n_bits // 64
    n, p, q = FIXTURE_N, FIXTURE_P, FIXTURE_Q
    nn = n * n
    ctx = zkp.Context(0)
    common = {"items": B, "n_bits": n_bits, "pointers": "host", "board": board(), "label": a.label, "rounds": a.rounds}
    records = []

    rnd = random.Random(7)
    ms = [rnd.randrange(n) for _ in range(B)]
    rs = [rnd.randrange(1, n) for _ in range(B)]
    assert all(gcd(r, n) == 1 for r in rs)
    mv, rv, nv = limbs(ms, kw), limbs(rs, kw), limbs([n], kw)
    cv = np.zeros((B, 2 * kw), np.uint32)
    ctx.paillier_enc(n_bits, B, nv, 0, mv, rv, cv)
    assert unlimbs(cv[0]) == (1 + ms[0] * n) * pow(rs[0], n, nn) % nn
    pv, qv = limbs([p], hw), limbs([q], hw)
    om, orr, st = np.zeros((B, kw), np.uint32), np.zeros((B, kw), np.uint32), np.zeros(B, np.uint8)

    # ---- (a), (b)
    def decrypt():
        ctx.paillier_open(n_bits, B, pv, qv, 0, cv, om, None, st)

    def open_():
        ctx.paillier_open(n_bits, B, pv, qv, 0, cv, om, orr, st)

    decrypt(); open_()                                       # warm-up of each
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(decrypt)); tb.append(timed(open_))
    assert not st.any() and np.array_equal(om, mv) and np.array_equal(orr, rv)
    records.append({"measurement": "a_decrypt_only", **common, "ms": med(ta), "samples_ms": [round(t, 3) for t in ta], "per_item_us": round(med(ta) * 1e3 / B, 2)})
    records.append({"measurement": "b_open_with_r", **common, "ms": med(tb), "samples_ms": [round(t, 3) for t in tb], "per_item_us": round(med(tb) * 1e3 / B, 2)})

    # ---- (c) c^lambda mod n^2 on the GPU, L and mu on the host
    lam = (p - 1) * (q - 1) // gcd(p - 1, q - 1)
    mu = pow((pow(1 + n, lam, nn) - 1) // n, -1, n)
    lv, nnv = limbs([lam], kw), limbs([nn], 2 * kw)
    u = np.zeros((B, 2 * kw), np.uint32)
    got = []

    def ladder():
        ctx.modexp(2 * n_bits, n_bits, B, cv, lv, 0, nnv, 0, u)

    def host_part():
        got[:] = [(unlimbs(u[i]) - 1) // n * mu % n for i in range(B)]

    ladder()
    tc, th = [], []
    for _ in range(a.rounds):
        tc.append(timed(ladder)); th.append(timed(host_part))
    assert got == ms
    records.append({"measurement": "c_parent_route", **common, "modexp_4096_exp_lambda_ms": med(tc), "host_L_and_mu_ms": med(th),
                    "modexp_samples_ms": [round(t, 3) for t in tc], "host_samples_ms": [round(t, 3) for t in th], "exp_bits": n_bits,
                    "note": "decrypt only: the parent commit has no batched route to r short of an n-sized ladder with a full-width exponent"})

    # ---- (d) CPython on one core
    S = min(a.cpython_items, B)
    hp, hq, pinv = pow(p - q % p, -1, p), pow(q - p % q, -1, q), pow(p, -1, q)
    dp, dq = pow(q, -1, p - 1), pow(p, -1, q - 1)
    cs = [unlimbs(cv[i]) for i in range(S)]

    def cpy(with_r):
        out = []
        for c in cs:
            mp = (pow(c % (p * p), p - 1, p * p) - 1) // p * hp % p
            mq = (pow(c % (q * q), q - 1, q * q) - 1) // q * hq % q
            m = mp + p * ((mq - mp) * pinv % q)
            if with_r:
                rp, rq = pow(c % p, dp, p), pow(c % q, dq, q)
                out.append((m, rp + p * ((rq - rp) * pinv % q)))
            else:
                out.append(m)
        return out

    assert cpy(False) == ms[:S] and cpy(True) == list(zip(ms[:S], rs[:S]))
    td = [timed(lambda: cpy(False)) for _ in range(3)]
    tdr = [timed(lambda: cpy(True)) for _ in range(3)]
    records.append({"measurement": "d_cpython_crt_one_core", **common, "cpython_items": S, "decrypt_ms_per_item": round(statistics.median(td) / S, 3),
                    "open_ms_per_item": round(statistics.median(tdr) / S, 3), "decrypt_ms_scaled_to_items": round(statistics.median(td) / S * B, 1),
                    "note": "CPython pow() is slower than GMP"})

    # ---- (e) what of (a) is not the ladder
    import torch

    def dev(x):
        return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()

    dpv, dqv, dcv, dom, dst = dev(pv), dev(qv), dev(cv), dev(om), dev(st)

    def decrypt_dev():
        ctx.paillier_open(n_bits, B, dpv, dqv, 0, dcv, dom, None, dst, device=True)
        ctx.synchronize()

    decrypt_dev()
    share = {}
    for name, fn in (("host_arrays", decrypt), ("device_arrays", decrypt_dev)):
        walls, ladders = [], []
        for _ in range(a.rounds):
            ctx.timing_reset(True)
            walls.append(timed(fn))
            ladder_ms, _, modexps = ctx.timing_get()
            assert modexps == 2 * B
            ladders.append(ladder_ms)
        ctx.timing_reset(False)
        w, l = statistics.median(walls), statistics.median(ladders)
        share[name] = {"call_ms": round(w, 3), "ladder_ms": round(l, 3), "not_ladder_ms": round(w - l, 3), "not_ladder_share": round((w - l) / w, 4)}
    assert np.array_equal(dom.cpu().numpy().view(np.uint32), mv)
    records.append({"measurement": "e_split_and_finish_share_of_a", **common, **share,
                    "note": "not_ladder = key preparation (one key), split, finish, the ladder's set-up kernel, launches; with host arrays also the copies"})

    for rec in records:
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
