"""GPU tests of the device scanner (csrc/kernels_serde_scan.hpp) behind zkp_json_range_proof_ni_batch with ZKP_F_DEVICE_PTRS and
zkp_range_ni_verify_json_batch.  The yardstick is the host reader (flags == 0): arrays and statuses must be its, byte for byte, for
canonical documents (read on the device) and for everything else (left to the host tokeniser and merged).

The parity tests carry the name of the whole-document reader tests on purpose: tests/conftest.py runs those under one kernel family
(they are about text, not arithmetic).  The verdict tests run under every family of the session ctx."""
import ctypes as C
import json

import numpy as np
import pytest

import helpers as H
import json_scan_cases as K
import json_scan_model as S
import json_writer_model as M
import test_wire_format as WF
from helpers import L, zkp

pytestmark = pytest.mark.gpu
FIELDS = ("range", "ciphertext", "c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")
FORM_PAIRS = [(zkp.BIGINT_DEC, zkp.BIGINT_DEC), (zkp.BIGINT_HEX, zkp.BIGINT_HEX), (zkp.BIGINT_BYTES, zkp.BIGINT_BYTES), (zkp.BIGINT_DEC, zkp.BIGINT_HEX),
              (zkp.BIGINT_HEX, zkp.BIGINT_BYTES)]
FORM_IDS = ["dec", "hex", "bytes", "key-dec+bare-hex", "key-hex+bare-bytes"]


@pytest.fixture(scope="module")
def sctx():
    """a context with the library's own routing, for the tests that are about text only or about the default route"""
    c = zkp.Context(0)
    yield c
    c.close()


def flip_digit(doc, marker, skip):
    """another digit `skip` bytes into the number behind the first `marker`"""
    at = doc.index(marker) + len(marker) + skip
    assert doc[at:at + 1].isdigit()
    return doc[:at] + (b"4" if doc[at:at + 1] != b"4" else b"6") + doc[at + 1:]


def read_host(ctx, packed, forms, n_bits, ef, verifier_n):
    """the yardstick: zkp_json_range_proof_ni_batch with flags == 0 -> (host RangeBatch, statuses)"""
    text, off, ln = packed
    B = len(off)
    pb = zkp.RangeBatch(n_bits, B, ef, shared_key=verifier_n is not None)
    for f in FIELDS:
        getattr(pb, f)[...] = 0xA5
    pb.n[...] = 0xA5A5A5A5
    if verifier_n is not None:
        pb.n[0] = L.int_to_limbs(verifier_n, n_bits // 32)
    st = np.full(B, 9, np.uint8)
    buf = (C.c_char * len(text)).from_buffer_copy(text)
    off_a, ln_a = np.array(off, np.uint64), np.array(ln, np.uint64)       # (kept alive over the call: ptr() is only an address)
    s = pb.struct()
    ctx.check(ctx.lib.zkp_json_range_proof_ni_batch(ctx.h, C.cast(buf, C.c_void_p), zkp.capi.ptr(off_a), zkp.capi.ptr(ln_a),
                                                    forms, C.byref(s), zkp.capi.ptr(st), 0))
    return pb, st


def read_device(ctx, packed, forms, n_bits, ef, verifier_n):
    """the same call with ZKP_F_DEVICE_PTRS -> (the batch copied back to the host, statuses, (fast, fallback))"""
    import torch
    text, off, ln = packed
    B = len(off)
    pd = zkp.RangeBatch(n_bits, B, ef, shared_key=verifier_n is not None, device="cuda")
    for f in FIELDS + ("n",):
        getattr(pd, f).fill_(0x5A)
    if verifier_n is not None:
        pd.n.copy_(torch.from_numpy(L.int_to_limbs(verifier_n, n_bits // 32).view(np.int32)).reshape(1, -1))
    st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    buf = (C.c_char * len(text)).from_buffer_copy(text)
    off_a, ln_a = np.array(off, np.uint64), np.array(ln, np.uint64)
    s = pd.struct()
    ctx.check(ctx.lib.zkp_json_range_proof_ni_batch(ctx.h, C.cast(buf, C.c_void_p), zkp.capi.ptr(off_a), zkp.capi.ptr(ln_a),
                                                    forms, C.byref(s), zkp.capi.ptr(st), zkp.capi.ZKP_F_DEVICE_PTRS))
    ctx.synchronize()
    return pd.to(None), st.cpu().numpy(), ctx.last_json_scan()


def assert_same(host, dev, shared):
    (ph, sh), (pd, sd) = host, dev[:2]
    assert list(sd) == list(sh)
    for f in FIELDS + ("n",):
        assert np.array_equal(getattr(ph, f), getattr(pd, f)), f
    bad = np.nonzero(sh)[0]
    for f in FIELDS + (() if shared else ("n",)):
        assert not getattr(pd, f)[bad].any(), f           # nothing of a document that is not converted as a whole stays behind


def check_parity(ctx, docs, forms, n_bits, ef, verifier_n, layout, canonical):
    packed = K.pack(docs, layout)
    host = read_host(ctx, packed, forms, n_bits, ef, verifier_n)
    dev = read_device(ctx, packed, forms, n_bits, ef, verifier_n)
    assert_same(host, dev, verifier_n is not None)
    fast, fallback = dev[2]
    print(f"{len(docs)} documents ({layout}): {fast} scanned on the device, {fallback} left to the host tokeniser; statuses {sorted(set(host[1].tolist()))}")
    assert fast + fallback == len(docs) and fast >= canonical
    return host[1]


# ------------------------------------------------------------------ 1. parity with the host reader
@pytest.mark.parametrize("key_enc,enc", FORM_PAIRS, ids=FORM_IDS)
@pytest.mark.parametrize("n_bits,ef", [(1024, 4), (1024, 128)])
def test_gpu_whole_range_proof_ni_documents_scanned_on_the_device(ctx, n_bits, ef, key_enc, enc):
    forms = zkp.bigint_forms(key_enc, enc)
    n0 = H.test_key(1024, tag=0)[2]
    vs = K.variants(b"parity-%d" % ef, n_bits, ef, key_enc, enc, n=n0)
    docs = [d for _, d in vs]
    # more canonical documents: all-Open, all-Mask, and one under another key (the verifier's assert_eq!(ek))
    for kinds, n in (("open", n0), ("mask", n0), ("mixed", H.test_key(1024, tag=1)[2])):
        case, pr = K.synthetic(b"parity-more-" + kinds.encode(), n_bits, ef, n=n, kinds=kinds)
        docs.append(WF.range_ni_document(case, pr, enc, ef, key_enc=key_enc))
    case, pr = K.synthetic(b"parity-other-key-pretty", n_bits, ef, n=H.test_key(1024, tag=1)[2])
    docs.append(WF.range_ni_document(case, pr, enc, ef, key_enc=key_enc, pretty=True))
    canonical = sum(S.is_canonical(d, n_bits, ef, key_enc, enc) for d in docs)
    assert 5 <= canonical < len(docs)
    st_self = check_parity(ctx, docs, forms, n_bits, ef, None, "gaps", canonical)
    st_key = check_parity(ctx, docs, forms, n_bits, ef, n0, "reverse", canonical)
    assert set(st_self.tolist()) == {zkp.DOC_OK, zkp.DOC_INVALID, zkp.DOC_HOST_PATH}
    assert st_self[-2] == zkp.DOC_OK and st_key[-2] == zkp.DOC_INVALID and st_self[-1] == zkp.DOC_OK and st_key[-1] == zkp.DOC_INVALID
    # every document on its own (B = 1) has the status it has in the batch
    for b in (0, 1, len(vs) - 1, len(docs) - 2):
        assert check_parity(ctx, [docs[b]], forms, n_bits, ef, None, "packed", int(S.is_canonical(docs[b], n_bits, ef, key_enc, enc)))[0] == st_self[b]


def test_gpu_whole_range_proof_ni_documents_three_hundred_on_the_device(ctx):
    """B = 300: more documents than a launch of the converter has lanes, good and bad ones interleaved"""
    n_bits, ef = 1024, 4
    vs = [d for _, d in K.variants(b"parity-300", n_bits, ef, 0, 0)]
    docs = []
    for b in range(300):
        if b % 3 == 2:
            docs.append(vs[(b // 3) % len(vs)])
        else:
            case, pr = K.synthetic(b"parity-300-%d" % b, n_bits, ef)
            docs.append(WF.range_ni_document(case, pr, 0, ef))
    canonical = sum(S.is_canonical(d, n_bits, ef) for d in docs)
    assert canonical >= 200
    check_parity(ctx, docs, 0, n_bits, ef, None, "gaps", canonical)


# ------------------------------------------------------------------ 2. verdicts
@pytest.fixture(scope="module")
def proved(oracle):
    """six proofs under two keys (honest, dishonest), their documents, and documents around them; the oracle's verdicts"""
    n_bits, ef, kw = 1024, 128, 32
    keys = [H.test_key(1024, tag=t)[2] for t in range(2)]
    cases = []
    for b in range(6):
        cases.append(H.build_range_case(b"verify-json-%d" % b, [keys[b % 2]], n_bits, 1, honest=(b != 3))[0])
    pb, wt = H.fill_batch(cases, n_bits, False, oracle)
    oracle.set_threads(min(oracle.max_threads(), 16))
    oracle.range_ni_prove(pb.struct(), wt.struct(), None, None, None)
    docs = [M.batch_doc(pb, b, M.DOC_NI) for b in range(6)]
    # tampered: one digit of a response, one digit of a commitment
    t1 = flip_digit(docs[0], b'"r1":"', 10)
    t2 = flip_digit(docs[2], b'"c2":["', 10)
    pretty = json.dumps(json.loads(docs[4]), indent=1).encode()
    all_docs = docs + [t1, t2, pretty, docs[0][:-1], docs[0].replace(b'"masked_r":"', b'"masked_r":"-', 1), b""]
    return n_bits, ef, keys, all_docs


@pytest.mark.parametrize("device", [False, True], ids=["host-out", "device-out"])
@pytest.mark.parametrize("mode", ["verify_self", "verifier_n"])
def test_verdicts_of_documents(ctx, oracle, proved, mode, device):
    n_bits, ef, keys, docs = proved
    B = len(docs)
    verifier_n = keys[0] if mode == "verifier_n" else None
    host, st = read_host(ctx, K.pack(docs), 0, n_bits, ef, verifier_n)
    ok = np.nonzero(st == zkp.DOC_OK)[0]
    want = np.zeros(B, np.uint8)
    vo = np.full(B, 9, np.uint8)
    if verifier_n is None:
        host.n[st != zkp.DOC_OK] = L.int_to_limbs(keys[0], n_bits // 32)      # (rows of unread documents are zero and their verdicts are not used: any key will do)
    oracle.range_ni_verify(host.struct(), vo)
    want[ok] = vo[ok]
    if verifier_n is None:
        assert list(st) == [0] * 9 + [zkp.DOC_INVALID, zkp.DOC_HOST_PATH, zkp.DOC_INVALID]
        assert list(want) == [1, 1, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0]
    else:
        assert list(st) == [0, 2, 0, 2, 0, 2, 0, 0, 0, zkp.DOC_INVALID, zkp.DOC_HOST_PATH, zkp.DOC_INVALID]
        assert list(want) == [1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    vn = None if verifier_n is None else L.int_to_limbs(verifier_n, n_bits // 32)
    if device:
        import torch
        os_, ov = torch.full((B,), 9, dtype=torch.uint8, device="cuda"), torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    else:
        os_, ov = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
    ctx.range_ni_verify_json(docs, 0, n_bits, ef, vn, device=device, out_status=os_, out_verdict=ov)
    ctx.synchronize()
    got_s, got_v = (os_.cpu().numpy(), ov.cpu().numpy()) if device else (os_, ov)
    assert list(got_s) == list(st) and list(got_v) == list(want)
    fast, fallback = ctx.last_json_scan()
    assert fast + fallback == B and fast >= 8


# ------------------------------------------------------------------ 3. round trip with the writer, on the default route
@pytest.mark.parametrize("shared", [True, False], ids=["shared-key", "per-proof-keys"])
def test_round_trip_with_the_writer(sctx, oracle, shared):
    import torch
    n_bits, ef, B, kw = 2048, 128, 8, 64
    keys = [H.test_key(2048, tag=t)[2] for t in range(1 if shared else 2)]
    cases = H.build_range_case(b"json-rt", [keys[b % len(keys)] for b in range(B)], n_bits, B, shared=False)
    pb, wt = H.fill_batch(cases, n_bits, shared, oracle)
    dev = pb.to("cuda")
    x, r = torch.from_numpy(wt.x.view(np.int32)).cuda(), torch.from_numpy(wt.r.view(np.int32)).cuda()
    stp = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    sctx.range_ni_prove_seeded(dev.struct(), x, r, bytes(range(32)), 0, None, None, stp, device=True)
    text, off, _ = sctx.json_write_range_proof_ni(dev.struct(), 0, None, device=True)
    docs = [bytes(text[int(off[b]):int(off[b + 1])]) for b in range(B)]
    assert stp.cpu().tolist() == [0] * B and all(S.is_canonical(d, n_bits, ef) for d in docs)
    vn = L.int_to_limbs(keys[0], kw) if shared else None
    st, v = sctx.range_ni_verify_json(docs, 0, n_bits, ef, vn)
    assert list(st) == [0] * B and list(v) == [1] * B
    assert sctx.last_json_scan() == (B, 0)
    # one digit of one document: only that verdict flips
    docs[5] = flip_digit(docs[5], b'"c1":["', 20)
    st, v = sctx.range_ni_verify_json(docs, 0, n_bits, ef, vn)
    assert list(st) == [0] * B and list(v) == [1, 1, 1, 1, 1, 0, 1, 1]
    assert sctx.last_json_scan() == (B, 0)


# ------------------------------------------------------------------ 4. the fast path really ran
@pytest.mark.parametrize("key_enc,enc", FORM_PAIRS, ids=FORM_IDS)
def test_canonical_batches_never_fall_back(sctx, key_enc, enc):
    """compact json.dumps documents, and the writers' own, are read on the device alone: in every form, Open-only, Mask-only and mixed"""
    n_bits, ef = 1024, 5
    forms = zkp.bigint_forms(key_enc, enc)
    docs = []
    for b, kinds in enumerate(("mixed", "open", "mask", "mixed")):
        case, pr = K.synthetic(b"fast-%d" % b, n_bits, ef, kinds=kinds)
        docs.append(WF.range_ni_document(case, pr, enc, ef, key_enc=key_enc))
    host = read_host(sctx, K.pack(docs), forms, n_bits, ef, None)
    dev = read_device(sctx, K.pack(docs), forms, n_bits, ef, None)
    assert_same(host, dev, False)
    assert list(host[1]) == [0] * 4 and dev[2] == (4, 0)
    # the writer's documents of that batch
    text, off, _ = sctx.json_write_range_proof_ni(host[0].struct(), forms, None)
    written = [bytes(text[int(off[b]):int(off[b + 1])]) for b in range(4)]
    assert written == docs
    dev = read_device(sctx, (bytes(text), [int(o) for o in off[:-1]], [len(d) for d in written]), forms, n_bits, ef, None)
    assert_same(host, dev, False)
    assert dev[2] == (4, 0)


# ------------------------------------------------------------------ 5. bounds
def test_a_document_ends_where_its_length_says(sctx):
    n_bits, ef = 1024, 3
    a, b_ = [WF.range_ni_document(*K.synthetic(b"bounds-%d" % k, n_bits, ef), 0, ef) for k in range(2)]
    text = a + b_
    cut = a.index(b'"c2":["') + 40                            # inside a number of the first document
    unclosed = a.replace(b'}}],"error_factor"', b'}},"error_factor"', 1)[:-1]      # the last row without its closing `]` ... `}`
    assert len(unclosed) == len(a) - 2
    for first, lengths in ((a, [cut, len(b_)]), (a, [len(a) - 2, len(b_)]), (unclosed + b"]}", [len(a) - 2, len(b_)])):
        packed = (first + b_, [0, len(a)], lengths)
        host = read_host(sctx, packed, 0, n_bits, ef, None)
        dev = read_device(sctx, packed, 0, n_bits, ef, None)
        assert_same(host, dev, False)
        assert list(dev[1]) == [zkp.DOC_INVALID, zkp.DOC_OK] and dev[2] == (1, 1)
    # the first document whole, the second one cut: the text behind a document's end is never its business
    packed = (text, [0, len(a)], [len(a), len(b_) - 1])
    dev = read_device(sctx, packed, 0, n_bits, ef, None)
    assert_same(read_host(sctx, packed, 0, n_bits, ef, None), dev, False)
    assert list(dev[1]) == [zkp.DOC_OK, zkp.DOC_INVALID]


def test_arguments(sctx):
    lib, EINVAL = sctx.lib, zkp.capi.ZKP_EINVAL
    st = np.zeros(1, np.uint8); v = np.zeros(1, np.uint8)
    off = np.zeros(1, np.uint64); ln = np.ones(1, np.uint64)
    buf = C.create_string_buffer(b"{}")
    args = lambda **k: [sctx.h, k.get("text", C.cast(buf, C.c_void_p)), zkp.capi.ptr(off), zkp.capi.ptr(ln), k.get("B", 1), k.get("n_bits", 1024), k.get("ef", 4),
                        k.get("forms", 0), None, zkp.capi.ptr(st), k.get("v", zkp.capi.ptr(v)), k.get("flags", 0)]
    assert lib.zkp_range_ni_verify_json_batch(*args()) == zkp.capi.ZKP_OK and st[0] == zkp.DOC_INVALID and v[0] == zkp.VERDICT_REJECT
    assert lib.zkp_range_ni_verify_json_batch(*args(B=0)) == zkp.capi.ZKP_OK
    for bad in (dict(text=None), dict(n_bits=3072), dict(ef=0), dict(ef=257), dict(forms=zkp.bigint_forms(3, 0)), dict(v=None), dict(flags=2)):
        assert lib.zkp_range_ni_verify_json_batch(*args(**bad)) == EINVAL, bad
