"""Crafted RangeProofNi proofs: rows that answer their challenge bit with a VALID response of the wrong kind.

A prover who knows the witness (x, r, w1, w2, r1, r2) can answer any row either way — Open with (w1, r1, w2, r2), Mask with the
honest j rule of generate_proof (range_proof.rs:226-246) — and both pass their Enc checks and range predicates.  Only the binding
of the kind to the challenge bit (range_proof.rs:270-348, the `_ => false` arm) rejects such a row.  The commitments c1, c2 are
left alone, so the Fiat-Shamir challenge of a crafted proof is that of the honest proof it was made from.

Labels (the reference verdict in WANT):
  honest     as proved
  all_open   every row Open with a valid opening: 2 Enc checks per row, the largest list a kind-derived plan can be made to build
  all_mask   every row a valid Mask
  flip_open  one challenge-1 row answered Open (its valid opening)
  flip_mask  one challenge-0 row answered Mask (its valid masked value)
  bad_kind2  one row with kind byte 2, data otherwise honest
  bad_kindFF one row with kind byte 0xFF, data otherwise honest
  forged     kinds honest, the Enc of the last FORGED_ROWS rows off by one bit (r1 of an Open row: its c1 check; masked_r of a Mask row)
  all_flip   every row answered with the other kind (a plan that follows the bits schedules no Enc at all)
  one_match  as all_flip but for one row, which keeps its honest response
"""
import numpy as np

import helpers as H
from helpers import pm, L, zkp

LABELS = ("honest", "all_open", "all_mask", "flip_open", "flip_mask", "bad_kind2", "bad_kindFF", "forged")
WANT = {"honest": zkp.VERDICT_ACCEPT, "all_open": zkp.VERDICT_REJECT, "all_mask": zkp.VERDICT_REJECT, "flip_open": zkp.VERDICT_REJECT,
        "flip_mask": zkp.VERDICT_REJECT, "bad_kind2": zkp.VERDICT_REJECT, "bad_kindFF": zkp.VERDICT_REJECT, "forged": zkp.VERDICT_REJECT,
        "all_flip": zkp.VERDICT_REJECT, "one_match": zkp.VERDICT_REJECT}
FIELDS = ("range", "ciphertext", "c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")
FORGED_ROWS = 3


def challenge_bits(e, elen, ef):
    """[B][ef] challenge bits of the transcripts e / elen (prove's out_e / out_e_len)"""
    out = np.zeros((len(elen), ef), np.uint8)
    for b in range(len(elen)):
        eb = bytes(e[b, :elen[b]])
        out[b] = [pm.challenge_bit(eb, i) for i in range(ef)]
    return out


def open_response(case, i):
    """(w1, r1, w2, r2): the opening of row i (range_proof.rs:226-232)"""
    return case["w1"][i], case["r1"][i], case["w2"][i], case["r2"][i]


def mask_response(case, i):
    """(j, masked_x, masked_r) by the honest j rule (range_proof.rs:233-246)"""
    third = case["range"] // 3
    x, r, n = case["x"], case["r"], case["n"]
    if third < x + case["w1"][i] < 2 * third:
        return 1, x + case["w1"][i], r * case["r1"][i] % n
    return 2, x + case["w2"][i], r * case["r2"][i] % n


def write_open(pb, b, i, case):
    kw = pb.kw
    w1, r1, w2, r2 = open_response(case, i)
    pb.resp_kind[b, i] = zkp.RESP_OPEN; pb.resp_j[b, i] = 0
    pb.resp_w1[b, i] = L.int_to_limbs(w1, kw); pb.resp_r1[b, i] = L.int_to_limbs(r1, kw)
    pb.resp_w2[b, i] = L.int_to_limbs(w2, kw); pb.resp_r2[b, i] = L.int_to_limbs(r2, kw)


def write_mask(pb, b, i, case):
    kw = pb.kw
    j, mx, mr = mask_response(case, i)
    pb.resp_kind[b, i] = zkp.RESP_MASK; pb.resp_j[b, i] = j
    pb.resp_w1[b, i] = L.int_to_limbs(mx, kw); pb.resp_r1[b, i] = L.int_to_limbs(mr, kw)
    pb.resp_w2[b, i] = 0; pb.resp_r2[b, i] = 0


def crafted_rows(label, bits):
    """rows of a proof with challenge bits `bits` whose response `label` replaces by one of the other kind"""
    ef = len(bits)
    ones = [i for i in range(ef) if bits[i]]
    zeros = [i for i in range(ef) if not bits[i]]
    if label == "all_open":
        return ones
    if label == "all_mask":
        return zeros
    if label == "flip_open":
        return ones[-1:]
    if label == "flip_mask":
        return zeros[-1:]
    if label == "all_flip":
        return list(range(ef))
    if label == "one_match":
        return list(range(ef - 1))
    return []


def craft(pb, b, case, bits, label):
    """turn honest proof b of `pb` (challenge bits `bits`) into `label`, in place"""
    ef = pb.ef
    for i in crafted_rows(label, bits):
        (write_mask if pb.resp_kind[b, i] == zkp.RESP_OPEN else write_open)(pb, b, i, case)
    if label == "bad_kind2":
        pb.resp_kind[b, ef // 2] = 2
    elif label == "bad_kindFF":
        pb.resp_kind[b, ef // 3] = 0xFF
    elif label == "forged":
        for i in range(ef - FORGED_ROWS, ef):
            pb.resp_r1[b, i, 0] ^= 1


def copy_proofs(dst, src, idx):
    """dst[k] = src[idx[k]] for every proof field (the key stays dst's)"""
    for f in FIELDS:
        getattr(dst, f)[:] = getattr(src, f)[np.asarray(idx)]


def make_pool(cases, n_bits, oracle, prove, labels=LABELS):
    """honest proofs of `cases` (one shared key) proved by `prove(pb, wt) -> (e, elen)`, and every label made of each:
    -> (pool RangeBatch, labels of its proofs, challenge bits [P][ef], the case of each proof).  Pool proof k * len(cases) + b is
    labels[k] made of case b."""
    nb = len(cases)
    base, wt = H.fill_batch(cases, n_bits, True, oracle)
    e, elen = prove(base, wt)
    bits = challenge_bits(e, elen, base.ef)
    pool = zkp.RangeBatch(n_bits, nb * len(labels), base.ef, shared_key=True)
    pool.n[:] = base.n
    copy_proofs(pool, base, [b for _ in labels for b in range(nb)])
    pool_labels, pool_bits, pool_cases = [], [], []
    for k, label in enumerate(labels):
        for b in range(nb):
            craft(pool, k * nb + b, cases[b], bits[b], label)
            pool_labels.append(label); pool_bits.append(bits[b]); pool_cases.append(cases[b])
    return pool, pool_labels, np.array(pool_bits), pool_cases


def kind_items(kind):
    """work-list length of the kind-derived plan (k_verify_plan with e == nullptr): 2 per Open row, 1 per Mask row"""
    return int(2 * np.count_nonzero(kind == zkp.RESP_OPEN) + np.count_nonzero(kind == zkp.RESP_MASK))


def matched_items(kind, bits):
    """work-list length of the plan that follows the challenge bits: 2 per Open row on a 0 bit, 1 per Mask row on a 1 bit"""
    return int(2 * np.count_nonzero((kind == zkp.RESP_OPEN) & (bits == 0)) + np.count_nonzero((kind == zkp.RESP_MASK) & (bits == 1)))


def oracle_verdicts(oracle, pb):
    v = np.full(pb.batch, 9, np.uint8)
    oracle.range_ni_verify(pb.struct(), v)
    return v
