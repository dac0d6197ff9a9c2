"""A/B/C record of the interactive RangeProof's verify on documents, and one line for its seeded prover steps: one board,
one process, order A B C A B C A B C after one warm-up of each.
  A  zkp_range_verifier_output_json_batch: the text of both documents of every session uploaded once, scanned on the device, no limb on the host;
  B  zkp_range_verifier_output_batch on the device-resident limbs the documents were written from — code this feature does not touch: the floor;
  C  the route a verifier chained by hand before: zkp_json_encrypted_pairs_batch and zkp_json_range_proof_batch with ZKP_F_DEVICE_PTRS into a
     device batch, then zkp_range_verifier_output_batch on it.
What a reader cares about is A - B, the cost of reading text, and A against C.  The sessions are honest: 256-bit ranges under the reference's
2048-bit fixture key (one shared key), error factor 40, the shape of bench.py's interactive leg; proved on the device by the two seeded steps and
written from there by zkp_json_write_encrypted_pairs_batch / zkp_json_write_range_proof_batch.  Every status must be ZKP_DOC_OK and every verdict
ACCEPT on all three routes, and every document must stay on the device route (fast_docs == 2 * sessions).  A's split (upload, pairs, proofs,
verify) comes from HIP events on the ctx stream (zkp_diag_last_json_scan_ms).
The prover line: S = the two seeded steps (32 bytes in), U = the two unseeded steps fed a device-resident witness (the floor: the same launches
without the sampler), order S U S U S U after one warm-up of each; both must write the same bytes.
Appends two JSON lines to profiles/json_reader/range_inter_ab.jsonl (or --out).
Usage: python tools/dev/json_range_inter_ab.py [--sessions 4096] [--rounds 3] [--label TEXT]"""
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

OUT_FIELDS = ("c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")


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
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_reader", "range_inter_ab.jsonl"))
    ap.add_argument("--label", default=None, help="written into the record (which build this run measured)")
    a = ap.parse_args()
    import torch
    n_bits, ef, B = 2048, 40, a.sessions
    kw = n_bits // 32
    rnd = random.Random(40)
    ctx = zkp.Context(0)
    lib, P, DEV = ctx.lib, zkp.capi.ptr, zkp.capi.ZKP_F_DEVICE_PTRS
    cuda = lambda arr: torch.from_numpy(arr.view(np.int32) if arr.dtype == np.uint32 else arr).cuda()

    # ---- the sessions: statements, secrets, the verifier's challenges; everything device-resident from here on
    ranges = [rnd.getrandbits(256) | (1 << 255) for _ in range(B)]
    xs = [rnd.randrange(q // 3) for q in ranges]
    rs = [rnd.randrange(2, FIXTURE_N) for _ in range(B)]
    pb = zkp.RangeBatch(n_bits, B, ef, shared_key=True)
    pb.n[0] = limbs([FIXTURE_N], kw)[0]
    pb.range[:] = limbs(ranges, kw)
    dpb = pb.to("cuda")
    dx, dr = cuda(limbs(xs, kw)), cuda(limbs(rs, kw))
    e = np.zeros((B, 32), np.uint8); e[:, :ef // 8] = np.frombuffer(rnd.randbytes(B * (ef // 8)), np.uint8).reshape(B, ef // 8)
    de, dl = cuda(e), cuda(np.full(B, ef // 8, np.uint8))
    seed = bytes(rnd.randbytes(32))
    torch.cuda.synchronize()
    ctx.paillier_enc(n_bits, B, dpb.n, 0, dx, dr, dpb.ciphertext)

    # ---- the prover line: S against U
    wit = [torch.zeros((B, ef, kw), dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    ctx.range_sample_witness(dpb.struct(), seed, 0, *wit, None, device=True)
    ctx.synchronize()
    w = zkp.capi.RangeNiWitness()
    w.x, w.r, w.w1, w.w2, w.r1, w.r2 = (P(t) for t in (dx, dr, *wit))
    dpu = pb.to("cuda")
    dpu.ciphertext.copy_(dpb.ciphertext)
    torch.cuda.synchronize()

    def run_s():
        st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize(); ctx.synchronize()      # (torch fills its tensors on its own stream: done before the ctx stream writes them)
        t = time.perf_counter()
        ctx.range_generate_encrypted_pairs_seeded(dpb.struct(), seed, 0, None, device=True)
        ctx.synchronize()
        t1 = time.perf_counter()
        ctx.range_generate_proof_seeded(dpb.struct(), dx, dr, seed, 0, de, dl, st, device=True)
        ctx.synchronize()
        t2 = time.perf_counter()
        return (t2 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3, st.cpu().numpy(), ctx.witness_residue()

    def run_u():
        st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize(); ctx.synchronize()      # (torch fills its tensors on its own stream: done before the ctx stream writes them)
        t = time.perf_counter()
        ctx.range_generate_encrypted_pairs(dpu.struct(), w, device=True)
        ctx.synchronize()
        t1 = time.perf_counter()
        ctx.range_generate_proof(dpu.struct(), w, de, dl, st, device=True)
        ctx.synchronize()
        t2 = time.perf_counter()
        return (t2 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3, st.cpu().numpy()

    run_s(); run_u()
    S, S1, S2, U, U1, U2, residue = [], [], [], [], [], [], 0
    clean = True
    for _ in range(a.rounds):
        ms, m1, m2, st, res = run_s(); S.append(ms); S1.append(m1); S2.append(m2); residue = max(residue, res); clean = clean and not st.any()
        ms, m1, m2, st = run_u(); U.append(ms); U1.append(m1); U2.append(m2); clean = clean and not st.any()
    same_bytes = all(bool(torch.equal(getattr(dpb, f), getattr(dpu, f))) for f in OUT_FIELDS)
    prover = dict(record="prover", sessions=B, n_bits=n_bits, error_factor=ef, order="S U " * a.rounds, warm_up="one S and one U before the timed rounds",
                  seeded_ms=S, seeded_step1_ms=S1, seeded_step2_ms=S2, unseeded_ms=U, unseeded_step1_ms=U1, unseeded_step2_ms=U2,
                  seeded_median=float(np.median(S)), unseeded_median=float(np.median(U)), sampler_cost_ms=float(np.median(S) - np.median(U)),
                  kept_between_messages_bytes=32, witness_bytes=4 * B * ef * kw * 4, same_bytes=same_bytes, statuses_clean=bool(clean), witness_residue=int(residue),
                  sclk_mhz=sclk_mhz())

    # ---- the documents, written where the prover left the batch
    tp, op, _ = ctx.json_write_encrypted_pairs(dpb.struct(), device=True)
    tr, orr, _ = ctx.json_write_range_proof(dpb.struct(), device=True)
    text = np.concatenate([tp, tr])
    a_off = np.ascontiguousarray(op[:-1]); a_len = np.ascontiguousarray(op[1:] - op[:-1])
    b_off = np.ascontiguousarray(orr[:-1] + np.uint64(tp.size)); b_len = np.ascontiguousarray(orr[1:] - orr[:-1])
    del tp, tr
    dq = pb.to("cuda")                  # C's destination: the statement, empty pairs and responses
    dq.ciphertext.copy_(dpb.ciphertext)
    torch.cuda.synchronize()

    def run_a():
        st = torch.full((B,), 9, dtype=torch.uint8, device="cuda"); v = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize(); ctx.synchronize()      # (torch fills its tensors on its own stream: done before the ctx stream writes them)
        t = time.perf_counter()
        ctx.check(lib.zkp_range_verifier_output_json_batch(ctx.h, P(text), P(a_off), P(a_len), P(b_off), P(b_len), B, n_bits, ef, P(dpb.n), 0, P(dpb.range),
                                                           P(dpb.ciphertext), P(de), P(dl), P(st), P(v), DEV))
        ctx.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        return ms, ctx.last_json_scan_ms(), ctx.last_json_scan(), st.cpu().numpy(), v.cpu().numpy()

    def run_b():
        v = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize(); ctx.synchronize()      # (torch fills its tensors on its own stream: done before the ctx stream writes them)
        t = time.perf_counter()
        ctx.range_verifier_output(dpb.struct(), de, dl, v, device=True)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, v.cpu().numpy()

    def run_c():
        s1, s2, v = (torch.full((B,), 9, dtype=torch.uint8, device="cuda") for _ in range(3))
        q = dq.struct()
        torch.cuda.synchronize(); ctx.synchronize()      # (torch fills its tensors on its own stream: done before the ctx stream writes them)
        t = time.perf_counter()
        ctx.check(lib.zkp_json_encrypted_pairs_batch(ctx.h, P(text), P(a_off), P(a_len), C.byref(q), P(s1), DEV))
        ctx.check(lib.zkp_json_range_proof_batch(ctx.h, P(text), P(b_off), P(b_len), C.byref(q), P(s2), DEV))
        ctx.synchronize()
        t_read = time.perf_counter()
        ctx.range_verifier_output(q, de, dl, v, device=True)
        ctx.synchronize()
        t_end = time.perf_counter()
        return (t_end - t) * 1e3, (t_read - t) * 1e3, torch.maximum(s1, s2).cpu().numpy(), v.cpu().numpy()

    _, _, scan, sta, va = run_a()
    _, vb = run_b()
    _, _, stc, vc = run_c()
    same = bool(np.array_equal(sta, stc) and np.array_equal(va, vb) and np.array_equal(va, vc) and not sta.any())
    A, Asplit, Bs, Cs, Cr = [], [], [], [], []
    for _ in range(a.rounds):
        ms, split, scan, st_, v_ = run_a(); A.append(ms); Asplit.append(dict(zip(("upload_ms", "pairs_ms", "proofs_ms", "verify_ms"), split)))
        same = same and bool(np.array_equal(st_, sta) and np.array_equal(v_, va))
        ms, v_ = run_b(); Bs.append(ms)
        same = same and bool(np.array_equal(v_, va))
        ms, read, st_, v_ = run_c(); Cs.append(ms); Cr.append(read)
        same = same and bool(np.array_equal(st_, sta) and np.array_equal(v_, va))
    am, bm, cm = float(np.median(A)), float(np.median(Bs)), float(np.median(Cs))
    verify = dict(record="verify", sessions=B, n_bits=n_bits, error_factor=ef, text_bytes=int(text.size), order="A B C " * a.rounds,
                  warm_up="one A, one B and one C before the timed rounds", a_ms=A, a_split=Asplit, b_ms=Bs, c_ms=Cs, c_read_ms=Cr, a_median=am, b_median=bm, c_median=cm,
                  text_cost_ms=am - bm, two_reader_text_cost_ms=cm - bm, fast_docs=scan[0], fallback_docs=scan[1], same_statuses_and_verdicts=same,
                  accepted=int((va == 1).sum()), sclk_mhz=sclk_mhz())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for rec in (verify, prover):
        if a.label is not None:
            rec["label"] = a.label
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    ctx.close()
    if not same or verify["accepted"] != B or verify["fast_docs"] != 2 * B or not same_bytes or not clean or residue:
        sys.exit("the routes disagree, an honest session was not accepted, a document left the device route, or the prover steps differ")


if __name__ == "__main__":
    main()
