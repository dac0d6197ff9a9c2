"""GPU tests of the device scanner (csrc/kernels_serde_scan.hpp) behind zkp_json_correct_key_proof_batch, zkp_json_encrypted_pairs_batch and
zkp_json_range_proof_batch with ZKP_F_DEVICE_PTRS.  The yardstick is the same reader with flags == 0: arrays and statuses must be its, byte
for byte, for canonical documents (read on the device) and for everything else (left to the host tokeniser and merged).  Which
documents are canonical is tests/json_scan_doc_model.py's to say, never the kernel's.

These tests are about text: they run on a context of their own with the library's routing."""
import ctypes as C
import json
import random

import numpy as np
import pytest

import helpers as H
import json_scan_cases as K
import json_scan_doc_model as D
import json_writer_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu
CK, PAIRS, PROOF = D.DOC_CK, D.DOC_PAIRS, D.DOC_PROOF
KIND_IDS = {CK: "correct-key", PAIRS: "pairs", PROOF: "proof"}
FIELDS = {CK: ("sigma",), PAIRS: ("c1", "c2"), PROOF: ("resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")}


@pytest.fixture(scope="module")
def sctx():
    c = zkp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ documents
def count_of(kind, ef):
    return D.SIGMA_COUNT if kind == CK else ef


def build(kind, a, b=None):
    """a document from number STRINGS (so that leading zeros survive).  CK: a = sigma; PAIRS: a = c1, b = c2; PROOF: a = rows"""
    return M.correct_key_doc(a) if kind == CK else M.pairs_doc(a, b) if kind == PAIRS else M.proof_doc(a)


def random_doc(kind, rnd, n_bits, ef, kinds="mixed", j_values=(0, 1, 2, 255), first=None, pad=False, count=None):
    """a canonical document (unless `first` / `count` say otherwise) with numbers over the whole width; first: the text of the first number;
    pad: every number has exactly max_digits digits through leading zeros"""
    kw = n_bits // 32
    count = count_of(kind, ef) if count is None else count

    def num(words):
        v = str(rnd.getrandbits(32 * words - rnd.choice((0, 0, 1, 7, 32 * words - 9))))
        return v.rjust(D.max_digits(words), "0") if pad else v
    if kind == PROOF:
        rows = []
        for r in range(count):
            mask = kinds == "mask" or (kinds == "mixed" and rnd.random() < 0.5) or (kinds == "alternating" and r % 2 == 1)
            rows.append(("mask", j_values[r % len(j_values)], num(kw), num(kw)) if mask else ("open", num(kw), num(kw), num(kw), num(kw)))
        if first is not None and rows:
            rows[0] = rows[0][:2] + (first,) + rows[0][3:] if rows[0][0] == "mask" else ("open", first) + rows[0][2:]
        return build(kind, rows)
    words = kw if kind == CK else 2 * kw
    a = [num(words) for _ in range(count)]
    if first is not None and a:
        a[0] = first
    return build(kind, a, [num(words) for _ in range(count)])


def first_words(kind, n_bits):
    return n_bits // 32 * (2 if kind == PAIRS else 1)


def mixed_docs(kind, seed, n_bits, ef):
    """canonical documents and everything around them -> {name: document}, in batch order"""
    rnd = random.Random(seed)
    dig = D.max_digits(first_words(kind, n_bits))
    docs = {"random": random_doc(kind, rnd, n_bits, ef),
            "zero": random_doc(kind, rnd, n_bits, ef, first="0"),
            "padded": random_doc(kind, rnd, n_bits, ef, pad=True),
            "overflow": random_doc(kind, rnd, n_bits, ef, first="9" * dig)}       # as long as the field and too large for it: k_dec2bin's overflow
    if kind == PROOF:
        docs.update({k: random_doc(kind, rnd, n_bits, ef, kinds=k) for k in ("open", "mask", "alternating")})
    good = random_doc(kind, rnd, n_bits, ef, first="15", kinds="alternating")      # (row 0 is Open)
    assert all(D.is_canonical(kind, d, n_bits, ef) for d in list(docs.values()) + [good])
    docs["pretty"] = json.dumps(json.loads(good), indent=1).encode()
    if kind == PAIRS:
        v = json.loads(good)
        docs["reordered"] = json.dumps({"c2": v["c2"], "c1": v["c1"]}, separators=(",", ":")).encode()
    docs["extra-field"] = good.replace(b'{"w1":', b'{"extra":null,"w1":', 1) if kind == PROOF else good[:-1] + b',"extra":[1,{"a":"b"}]}'
    docs["escape"] = good.replace(b'"15"', b'"\\u00315"', 1)
    docs["sign"] = good.replace(b'"15"', b'"-5"', 1)
    docs["too-long"] = good.replace(b'"15"', b'"1' + b"0" * dig + b'"', 1)                  # one digit longer than the field, and too large
    docs["too-long-zeros"] = good.replace(b'"15"', b'"' + b"0" * (dig - 1) + b'15"', 1)     # one digit longer, the value fits: the host reader takes it
    docs["one-less"] = random_doc(kind, rnd, n_bits, ef, count=count_of(kind, ef) - 1)      # 10 entries / EF - 1 rows
    docs["one-more"] = random_doc(kind, rnd, n_bits, ef, count=count_of(kind, ef) + 1)
    docs.update({"brackets": b"[]", "truncated": good[:-1], "empty": b"", "half": good[:len(good) // 2], "trailing-space": good + b" "})
    assert json.loads(docs["escape"]) == json.loads(good) and json.loads(docs["extra-field"]) != json.loads(good)
    return docs


# ------------------------------------------------------------------ the two routes
def read(ctx, kind, packed, n_bits, ef, device):
    """-> ({field: numpy array}, statuses, (fast, fallback) of the call or None)"""
    text, off, ln = packed
    B, kw = len(off), n_bits // 32
    fill = 0x5A if device else 0xA5
    buf = (C.c_char * len(text)).from_buffer_copy(text)
    off_a, ln_a = np.array(off, np.uint64), np.array(ln, np.uint64)
    flags = zkp.capi.ZKP_F_DEVICE_PTRS if device else 0
    P = zkp.capi.ptr
    if device:
        import torch
        st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    else:
        st = np.full(B, 9, np.uint8)
    if kind == CK:
        if device:
            sigma = torch.full((B, D.SIGMA_COUNT, kw), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        else:
            sigma = np.full((B, D.SIGMA_COUNT, kw), 0xA5A5A5A5, np.uint32)
        ctx.check(ctx.lib.zkp_json_correct_key_proof_batch(ctx.h, C.cast(buf, C.c_void_p), P(off_a), P(ln_a), n_bits, B, P(sigma), P(st), flags))
        arrays = {"sigma": sigma.cpu().numpy().view(np.uint32) if device else sigma}
    else:
        pb = zkp.RangeBatch(n_bits, B, ef, shared_key=True, device="cuda" if device else None)
        for f in FIELDS[PAIRS] + FIELDS[PROOF]:
            getattr(pb, f).fill_(fill) if device else getattr(pb, f).fill(fill)
        s = pb.struct()
        fn = ctx.lib.zkp_json_encrypted_pairs_batch if kind == PAIRS else ctx.lib.zkp_json_range_proof_batch
        ctx.check(fn(ctx.h, C.cast(buf, C.c_void_p), P(off_a), P(ln_a), C.byref(s), P(st), flags))
        if device:
            ctx.synchronize()
            pb = pb.to(None)
        arrays = {f: np.array(getattr(pb, f)) for f in FIELDS[kind]}
        # the reader of one half of a proof leaves the other half alone
        for f in FIELDS[PAIRS if kind == PROOF else PROOF]:
            assert (np.array(getattr(pb, f)) == fill).all(), f
    if device:
        ctx.synchronize()
        return arrays, st.cpu().numpy(), ctx.last_json_scan()
    return arrays, st, None


def check_parity(ctx, kind, docs, n_bits, ef, layout="gaps"):
    packed = K.pack(docs, layout) if isinstance(layout, str) else layout
    host = read(ctx, kind, packed, n_bits, ef, False)
    dev = read(ctx, kind, packed, n_bits, ef, True)
    assert list(dev[1]) == list(host[1])
    for f in FIELDS[kind]:
        assert np.array_equal(host[0][f], dev[0][f]), f
    canonical = sum(D.is_canonical(kind, d, n_bits, ef) for d in docs)
    print(f"{KIND_IDS[kind]}: {len(docs)} documents, {canonical} canonical, scanner {dev[2]}, statuses {sorted(set(host[1].tolist()))}")
    assert dev[2] == (canonical, len(docs) - canonical)
    return host[1]


# ------------------------------------------------------------------ 1. parity with the flags-0 reader
SHAPES = [(kind, n_bits, ef, layout) for n_bits, ef, layout in ((1024, 1, "gaps"), (1024, 4, "reverse"), (1024, 128, "gaps"), (2048, 4, "reverse"))
          for kind in (CK, PAIRS, PROOF) if not (kind == CK and ef == 128)]      # (a NiCorrectKeyProof has no error factor: three shapes)


@pytest.mark.parametrize("kind,n_bits,ef,layout", SHAPES, ids=[f"{KIND_IDS[k]}-{n}-ef{e}" for k, n, e, _ in SHAPES])
def test_mixed_documents_are_read_as_the_host_reader_reads_them(sctx, kind, n_bits, ef, layout):
    named = mixed_docs(kind, b"mixed-%d-%d-%d" % (kind, n_bits, ef), n_bits, ef)
    names, docs = list(named), list(named.values())
    st = dict(zip(names, check_parity(sctx, kind, docs, n_bits, ef, layout)))
    print(st)
    assert set(st.values()) == {zkp.DOC_OK, zkp.DOC_INVALID, zkp.DOC_HOST_PATH}
    assert st["random"] == st["zero"] == st["padded"] == st["pretty"] == st["escape"] == zkp.DOC_OK
    assert st["overflow"] == st["sign"] == st["too-long"] == zkp.DOC_HOST_PATH and st["empty"] == st["truncated"] == zkp.DOC_INVALID
    # batches of one and of three: a canonical document, fall-backs, the overflow
    for name in ("random", "overflow", "too-long", "empty", "pretty"):
        assert check_parity(sctx, kind, [named[name]], n_bits, ef, "packed")[0] == st[name]
    three = ("sign", "zero", "overflow")
    assert list(check_parity(sctx, kind, [named[k] for k in three], n_bits, ef, "reverse")) == [st[k] for k in three]
    # all canonical: nothing falls back
    canon = [d for d in docs if D.is_canonical(kind, d, n_bits, ef)]
    assert len(canon) >= 4
    check_parity(sctx, kind, canon, n_bits, ef, "packed")
    assert sctx.last_json_scan() == (len(canon), 0)


@pytest.mark.parametrize("kind", [CK, PAIRS, PROOF], ids=list(KIND_IDS.values()))
def test_three_hundred_documents(sctx, kind):
    """more documents than k_scan_merge has threads in a block, canonical and other ones interleaved"""
    n_bits, ef = 1024, 4
    pool = list(mixed_docs(kind, b"300-%d" % kind, n_bits, ef).values())
    rnd = random.Random(300 + kind)
    docs = [pool[(b // 2) % len(pool)] if b % 2 else random_doc(kind, rnd, n_bits, ef) for b in range(300)]
    check_parity(sctx, kind, docs, n_bits, ef, "gaps")


@pytest.mark.parametrize("kind", [CK, PAIRS, PROOF], ids=list(KIND_IDS.values()))
def test_every_residue_of_the_scanners_step(sctx, kind):
    """64 documents, the first number of document k has k + 1 digits: every later number boundary lands on every residue of the 64-byte step"""
    n_bits, ef = 1024, 4
    rnd = random.Random(64 + kind)
    docs = [random_doc(kind, rnd, n_bits, ef, first="7" * (k + 1), kinds="alternating") for k in range(64)]
    st = check_parity(sctx, kind, docs, n_bits, ef, "packed")
    assert list(st) == [0] * 64 and sctx.last_json_scan() == (64, 0)


def test_a_document_ends_where_its_length_says(sctx):
    n_bits, ef = 1024, 3
    rnd = random.Random(7)
    for kind in (CK, PAIRS, PROOF):
        a, b_ = random_doc(kind, rnd, n_bits, ef), random_doc(kind, rnd, n_bits, ef)
        # the first document one byte short: the well-formed text goes on behind its length, and is not read
        for cut in (1, 2, len(a) // 3):
            st = check_parity(sctx, kind, [a[:-cut], b_], n_bits, ef, (a + b_, [0, len(a)], [len(a) - cut, len(b_)]))
            assert list(st) == [zkp.DOC_INVALID, zkp.DOC_OK]
        # the second one short, at the very end of the text
        st = check_parity(sctx, kind, [a, b_[:-1]], n_bits, ef, (a + b_, [0, len(a)], [len(a), len(b_) - 1]))
        assert list(st) == [zkp.DOC_OK, zkp.DOC_INVALID]
        # a canonical document followed by text that would continue it
        more = a + b',"x":["1"]}'
        st = check_parity(sctx, kind, [a], n_bits, ef, (more, [0], [len(a)]))
        assert list(st) == [zkp.DOC_OK] and sctx.last_json_scan() == (1, 0)


# ------------------------------------------------------------------ 2. round trips with the writers, on device-resident batches
def test_round_trip_of_sigma(sctx):
    import torch
    n_bits, kw, B = 2048, 64, 5
    rnd = random.Random(11)
    sig = np.stack([L.ints_to_limbs([rnd.getrandbits(n_bits - 8 * i) for i in range(11)], kw) for _ in range(B)])
    sig[2, 4] = 0
    dev = torch.from_numpy(sig.view(np.int32)).cuda()
    text, off, _ = sctx.json_write_correct_key_proof(n_bits, B, dev, None)
    docs = [bytes(text[int(off[b]):int(off[b + 1])]) for b in range(B)]
    assert all(D.is_canonical(CK, d, n_bits) for d in docs)
    back = torch.full_like(dev, 0x5A5A5A5A); st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    sctx.json_correct_key_proof(docs, n_bits, back, st)
    sctx.synchronize()
    assert st.cpu().tolist() == [0] * B and torch.equal(back, dev)
    assert sctx.last_json_scan() == (B, 0)


def test_round_trip_of_pairs_and_proof(sctx, oracle):
    n_bits, ef, B = 1024, 128, 3
    keys = [H.test_key(1024, tag=0)[2]]
    cases = H.build_range_case(b"scan-docs-rt", keys * B, n_bits, B, shared=False)
    pb, wt = H.fill_batch(cases, n_bits, True, oracle)
    oracle.set_threads(min(oracle.max_threads(), 16))
    oracle.range_ni_prove(pb.struct(), wt.struct(), None, None, None)
    dev = pb.to("cuda")
    back = zkp.RangeBatch(n_bits, B, ef, shared_key=True, device="cuda")
    import torch
    st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    for kind, write, reader in ((PAIRS, sctx.json_write_encrypted_pairs, sctx.json_encrypted_pairs), (PROOF, sctx.json_write_range_proof, sctx.json_range_proof)):
        text, off, _ = write(dev.struct(), None, device=True)
        docs = [bytes(text[int(off[b]):int(off[b + 1])]) for b in range(B)]
        assert docs == [M.batch_doc(pb, b, kind) for b in range(B)] and all(D.is_canonical(kind, d, n_bits, ef) for d in docs)
        reader(docs, back.struct(), st, device=True)
        sctx.synchronize()
        assert st.cpu().tolist() == [0] * B and sctx.last_json_scan() == (B, 0)
    got = back.to(None)
    for f in FIELDS[PAIRS] + FIELDS[PROOF]:
        assert np.array_equal(getattr(got, f), getattr(pb, f)), f
