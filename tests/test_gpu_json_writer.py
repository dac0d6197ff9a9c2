"""GPU tests of the JSON writers (zkp_json_write_*_batch): the SoA batch -> serde_json documents, byte for byte against the Python
model (tests/json_writer_model.py), round trips through the existing readers, the capacity protocol, bad kind bytes, offsets beyond
2^32, and independence from the internal chunking."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import helpers as H
import json_writer_model as M
from helpers import pm, L, zkp

pytestmark = pytest.mark.gpu
FORMS = (zkp.BIGINT_DEC, zkp.BIGINT_HEX, zkp.BIGINT_BYTES)
_WRITERS = {M.DOC_PAIRS: "json_write_encrypted_pairs", M.DOC_PROOF: "json_write_range_proof", M.DOC_NI: "json_write_range_proof_ni"}


@pytest.fixture(scope="module")
def wctx():
    """the writers are not modexp work and are never routed: the tests that prove nothing use one context of their own instead of
    running once per kernel family of the session ctx"""
    c = zkp.Context(0)
    yield c
    c.close()


def docs_of(text, off):
    return [bytes(text[int(off[b]):int(off[b + 1])]) for b in range(len(off) - 1)]


def write(ctx, pb, kind, forms=0, status=None, device=False):
    if kind == M.DOC_NI:
        return ctx.json_write_range_proof_ni(pb.struct(), forms, status, device=device)
    return getattr(ctx, _WRITERS[kind])(pb.struct(), status, device=device)


def check_batch(ctx, pb, kinds=(M.DOC_PAIRS, M.DOC_PROOF, M.DOC_NI), forms_list=((0, 0),), sample=None, dev=None):
    """every writer over host batch pb (dev: the same batch in device memory, written from there) against the model"""
    idx = range(pb.batch) if sample is None else sample
    for kind in kinds:
        for kf, bf in (forms_list if kind == M.DOC_NI else ((0, 0),)):
            st = np.full(pb.batch, 9, np.uint8)
            if dev is not None:
                import torch
                dst = torch.full((pb.batch,), 9, dtype=torch.uint8, device="cuda")
                text, off, _ = write(ctx, dev, kind, zkp.bigint_forms(kf, bf), dst, device=True)
                st = dst.cpu().numpy()
            else:
                text, off, _ = write(ctx, pb, kind, zkp.bigint_forms(kf, bf), st)
            assert list(st) == [zkp.DOC_OK] * pb.batch
            assert off[0] == 0 and len(text) == off[-1]
            for b in idx:
                got = bytes(text[int(off[b]):int(off[b + 1])])
                assert got == M.batch_doc(pb, b, kind, kf, bf), (kind, kf, bf, b)
                assert len(got) <= zkp.json_doc_bound(kind, pb.n_bits, pb.ef, zkp.bigint_forms(kf, bf))


def random_batch(seed, n_bits, B, ef, shared):
    """pseudo-random limbs in every field (no proving): kinds and j random too"""
    rng = np.random.default_rng(seed)
    pb = zkp.RangeBatch(n_bits, B, ef, shared_key=shared)
    for f in ("n", "range", "ciphertext", "c1", "c2", "resp_w1", "resp_r1", "resp_w2", "resp_r2"):
        a = getattr(pb, f)
        a[...] = rng.integers(0, 1 << 32, size=a.shape, dtype=np.uint32)
    pb.resp_kind[...] = rng.integers(0, 2, size=pb.resp_kind.shape, dtype=np.uint8)
    pb.resp_j[...] = np.where(pb.resp_kind == 1, rng.integers(0, 256, size=pb.resp_j.shape, dtype=np.uint8), 0)
    mask = pb.resp_kind == 1
    pb.resp_w2[mask] = 0; pb.resp_r2[mask] = 0
    return pb


# ------------------------------------------------------------------ 1. byte-exact, proved batches
@pytest.mark.parametrize("n_bits,ef,shared,B", [(1024, 128, True, 5), (1024, 40, False, 3), (2048, 128, True, 3), (2048, 4, False, 7), (2048, 1, True, 2),
                                                (4096, 4, True, 2)])
def test_written_documents_of_a_proved_batch(ctx, oracle, n_bits, ef, shared, B):
    """a real prove (host arrays), and the same prove with its outputs left on the device, written from there"""
    import torch
    keys = [H.test_key(n_bits, tag=t)[2] for t in range(1 if shared else B)]
    cases = H.build_range_case(b"writer-%d-%d" % (n_bits, ef), keys, n_bits, B, shared=shared, ef=ef)
    pb, wt = H.fill_batch(cases, n_bits, shared, oracle)
    if ef == zkp.SECURITY_PARAMETER:
        ctx.range_ni_prove(pb.struct(), wt.struct(), None, None, None, device=False)
        dev = pb.to("cuda")
        for f in ("c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2"):
            getattr(dev, f).zero_()
        ctx.range_ni_prove(dev.struct(), wt.to("cuda").struct(), None, None, None, device=True)      # nothing is downloaded before the writer runs
    else:
        e = np.zeros((B, 32), np.uint8); e_len = np.zeros(B, np.uint8)
        ctx.range_generate_encrypted_pairs(pb.struct(), wt.struct(), device=False)
        ctx.range_challenge(pb.struct(), e, e_len, device=False)
        ctx.range_generate_proof(pb.struct(), wt.struct(), e, e_len, np.zeros(B, np.uint8), device=False)
        dev = pb.to("cuda")
    check_batch(ctx, pb, forms_list=((0, 0), (1, 2)), dev=None)
    check_batch(ctx, pb, forms_list=((0, 0),), dev=dev)
    torch.cuda.synchronize()


def test_a_few_hundred_documents(wctx):
    pb = random_batch(11, 2048, 300, 128, False)
    check_batch(wctx, pb, sample=[0, 1, 63, 64, 150, 299])
    check_batch(wctx, pb, kinds=(M.DOC_NI,), sample=[0, 299], dev=pb.to("cuda"))
    pb = random_batch(12, 1024, 200, 40, True)
    check_batch(wctx, pb, sample=[0, 77, 199], forms_list=((2, 1),))


# ------------------------------------------------------------------ 2. edge numbers in every field position
@pytest.mark.parametrize("n_bits", [1024, 2048, 4096])
def test_edge_numbers_in_every_field(wctx, n_bits):
    kw = n_bits // 32
    def edges(words):
        k = int(32 * words * 0.30102999566398)          # the largest k with 10^k < 2^(32 words)
        while 10 ** (k + 1) < 1 << (32 * words):
            k += 1
        top = (1 << (32 * words)) - 1
        return [0, 1, 10 ** 9 - 1, 10 ** 9, 10 ** 18 - 1, 10 ** 18, 10 ** k - 1, 10 ** k, top, (1 << (32 * (words - 1))) - 1, 1 << (32 * (words - 1) - 1), 255, 256]
    en, ec = edges(kw), edges(2 * kw)
    ef = len(en)
    B = ef + 2                        # proof b rotates the edge list by b; the last two are all-Open and all-Mask
    pb = zkp.RangeBatch(n_bits, B, ef, shared_key=False)
    js = [0, 1, 2, 255]
    for b in range(B):
        pb.n[b] = L.int_to_limbs(en[b % ef], kw); pb.range[b] = L.int_to_limbs(en[(b + 1) % ef], kw)
        pb.ciphertext[b] = L.int_to_limbs(ec[b % ef], 2 * kw)
        for i in range(ef):
            pb.c1[b, i] = L.int_to_limbs(ec[(b + i) % ef], 2 * kw); pb.c2[b, i] = L.int_to_limbs(ec[(b + i + 3) % ef], 2 * kw)
            kind = zkp.RESP_OPEN if b == B - 2 else zkp.RESP_MASK if b == B - 1 else (b + i) % 2
            pb.resp_kind[b, i] = kind
            pb.resp_w1[b, i] = L.int_to_limbs(en[(b + i) % ef], kw); pb.resp_r1[b, i] = L.int_to_limbs(en[(b + i + 1) % ef], kw)
            if kind == zkp.RESP_OPEN:
                pb.resp_w2[b, i] = L.int_to_limbs(en[(b + i + 2) % ef], kw); pb.resp_r2[b, i] = L.int_to_limbs(en[(b + i + 5) % ef], kw)
            else:
                pb.resp_j[b, i] = js[(b + i // 2) % 4]
    check_batch(wctx, pb, forms_list=list(itertools.product(FORMS, FORMS)))
    # NiCorrectKeyProof documents over the same edge values
    sig = np.zeros((3, 11, kw), np.uint32)
    vals = [[en[(b * 5 + i) % ef] for i in range(11)] for b in range(3)]
    for b in range(3):
        sig[b] = L.ints_to_limbs(vals[b], kw)
    text, off, _ = wctx.json_write_correct_key_proof(n_bits, 3, sig, np.zeros(3, np.uint8))
    assert docs_of(text, off) == [M.correct_key_doc(v) for v in vals]
    assert max(len(d) for d in docs_of(text, off)) <= zkp.json_doc_bound(M.DOC_CK, n_bits)


# ------------------------------------------------------------------ 3. round trip through the readers
def test_round_trip_through_the_readers(ctx, oracle):
    n_bits, ef, B, kw = 1024, 128, 4, 32
    n = H.test_key(1024)[2]
    cases = H.build_range_case(b"writer-rt", [n], n_bits, B)
    cases[2] = H.build_range_case(b"writer-rt-bad", [n], n_bits, 1, honest=False)[0]
    pb, wt = H.fill_batch(cases, n_bits, True, oracle)
    ctx.range_ni_prove(pb.struct(), wt.struct(), None, None, None, device=False)
    v0 = np.full(B, 9, np.uint8)
    ctx.range_ni_verify(pb.struct(), v0, device=False)
    fields = ("range", "ciphertext", "c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")
    # the two sub-documents
    back = zkp.RangeBatch(n_bits, B, ef, shared_key=True)
    back.n[:] = pb.n; back.range[:] = pb.range; back.ciphertext[:] = pb.ciphertext
    for kind, reader in ((M.DOC_PAIRS, ctx.json_encrypted_pairs), (M.DOC_PROOF, ctx.json_range_proof)):
        text, off, _ = write(ctx, pb, kind)
        st = np.full(B, 9, np.uint8)
        reader(docs_of(text, off), back.struct(), st, device=False)
        assert list(st) == [0] * B
    for f in fields:
        assert np.array_equal(getattr(back, f), getattr(pb, f)), f
    v1 = np.full(B, 9, np.uint8)
    ctx.range_ni_verify(back.struct(), v1, device=False)
    assert list(v1) == list(v0) == [1, 1, 0, 1]
    # whole documents: three key forms x three bare forms, read back under per-proof keys and under the verifier's shared key
    for kf, bf in itertools.product(FORMS, FORMS):
        forms = zkp.bigint_forms(kf, bf)
        text, off, _ = write(ctx, pb, M.DOC_NI, forms)
        docs = docs_of(text, off)
        for shared in (False, True):
            rb = zkp.RangeBatch(n_bits, B, ef, shared_key=shared)
            if shared:
                rb.n[:] = pb.n
            st = np.full(B, 9, np.uint8)
            ctx.json_range_proof_ni(docs, forms, rb.struct(), st)
            assert list(st) == [0] * B, (kf, bf, shared)
            for f in fields:
                assert np.array_equal(getattr(rb, f), getattr(pb, f)), (f, kf, bf)
            assert all(np.array_equal(row, pb.n[0]) for row in rb.n)
        if (kf, bf) in ((0, 0), (1, 2)):
            v2 = np.full(B, 9, np.uint8)
            ctx.range_ni_verify(rb.struct(), v2, device=False)
            assert list(v2) == list(v0)


def test_correct_key_documents_round_trip(wctx):
    n_bits, kw = 1024, 32
    keys = [H.test_key(1024, tag=t) for t in range(3)]
    sig = [pm.correct_key_proof(p_, q_, b"KZen") for p_, q_, _ in keys]
    arr = np.stack([L.ints_to_limbs(s, kw) for s in sig])
    text, off, st = wctx.json_write_correct_key_proof(n_bits, 3, arr, np.full(3, 9, np.uint8))
    assert list(st) == [0, 0, 0] and docs_of(text, off) == [M.correct_key_doc(s) for s in sig]
    back = np.zeros_like(arr); rs = np.full(3, 9, np.uint8)
    wctx.json_correct_key_proof(docs_of(text, off), n_bits, back, rs)
    assert list(rs) == [0, 0, 0] and np.array_equal(back, arr)
    import torch
    dev = torch.from_numpy(arr.view(np.int32)).cuda()
    text2, off2, _ = wctx.json_write_correct_key_proof(n_bits, 3, dev, None)
    assert bytes(text2) == bytes(text) and np.array_equal(off, off2)


# ------------------------------------------------------------------ 4. capacity protocol
def test_capacity_protocol(wctx):
    lib = wctx.lib
    pb = random_batch(21, 1024, 5, 4, True)
    s = pb.struct()
    B = pb.batch
    sized = np.full(B + 1, 7, np.uint64)
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(s), 0, None, 0, zkp.capi.ptr(sized), None, 0) == zkp.capi.ZKP_OK
    total = int(sized[B])
    assert sized[0] == 0 and all(sized[b] < sized[b + 1] for b in range(B))
    # one byte short: ZKP_EINVAL, offsets written, not a byte of the buffer touched, both numbers named
    buf = np.full(total + 16, 0xEE, np.uint8); off = np.full(B + 1, 7, np.uint64)
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(s), 0, zkp.capi.ptr(buf), total - 1, zkp.capi.ptr(off), None, 0) == zkp.capi.ZKP_EINVAL
    msg = lib.zkp_last_error_string(wctx.h).decode()
    assert str(total) in msg and str(total - 1) in msg
    assert np.array_equal(off, sized) and (buf == 0xEE).all()
    # the exact capacity: the text, and nothing behind it
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(s), 0, zkp.capi.ptr(buf), total, zkp.capi.ptr(off), None, 0) == zkp.capi.ZKP_OK
    assert np.array_equal(off, sized) and (buf[total:] == 0xEE).all()
    assert docs_of(buf, off) == [M.batch_doc(pb, b, M.DOC_NI) for b in range(B)]
    # one allocation from the bound, no sizing call
    bound = zkp.json_doc_bound(M.DOC_NI, 1024, 4)
    big = np.zeros(B * bound, np.uint8)
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(s), 0, zkp.capi.ptr(big), big.size, zkp.capi.ptr(off), None, 0) == zkp.capi.ZKP_OK
    assert bytes(big[:total]) == bytes(buf[:total])
    # B = 0
    empty = zkp.RangeBatch(1024, 0, 4, shared_key=True)
    off0 = np.full(1, 7, np.uint64)
    for fn in (lib.zkp_json_write_encrypted_pairs_batch, lib.zkp_json_write_range_proof_batch):
        es = empty.struct()
        assert fn(wctx.h, C.byref(es), None, 0, zkp.capi.ptr(off0), None, 0) == zkp.capi.ZKP_OK and off0[0] == 0
    assert lib.zkp_json_write_correct_key_proof_batch(wctx.h, 1024, 0, None, None, 0, zkp.capi.ptr(off0), None, 0) == zkp.capi.ZKP_OK
    # null pointers and widths
    EINVAL = zkp.capi.ZKP_EINVAL
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(s), 0, None, 0, None, None, 0) == EINVAL
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, None, 0, None, 0, zkp.capi.ptr(off), None, 0) == EINVAL
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(s), zkp.bigint_forms(3, 0), None, 0, zkp.capi.ptr(off), None, 0) == EINVAL
    assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(s), 0, None, 0, zkp.capi.ptr(off), None, 2) == EINVAL
    for field, value in (("n_bits", 512), ("n_bits", 3072), ("error_factor", 0), ("error_factor", 257), ("c1", None), ("resp_kind", None), ("n", None), ("n_stride", 5)):
        t = pb.struct()
        setattr(t, field, value)
        assert lib.zkp_json_write_range_proof_ni_batch(wctx.h, C.byref(t), 0, None, 0, zkp.capi.ptr(off), None, 0) == EINVAL, field
    assert lib.zkp_json_write_correct_key_proof_batch(wctx.h, 1000, 1, zkp.capi.ptr(pb.resp_w1), None, 0, zkp.capi.ptr(off), None, 0) == EINVAL
    assert lib.zkp_json_write_correct_key_proof_batch(wctx.h, 1024, 1, None, None, 0, zkp.capi.ptr(off), None, 0) == EINVAL


# ------------------------------------------------------------------ 5. a kind byte no Response has
def test_bad_kind_byte_empties_that_document_only(wctx):
    pb = random_batch(31, 1024, 6, 8, False)
    pb.resp_kind[2, 5] = 2; pb.resp_kind[4, 0] = 255
    for kind in (M.DOC_PROOF, M.DOC_NI):
        st = np.full(6, 9, np.uint8)
        text, off, _ = write(wctx, pb, kind, 0, st)
        assert list(st) == [0, 0, zkp.DOC_INVALID, 0, zkp.DOC_INVALID, 0]
        assert off[3] == off[2] and off[5] == off[4]
        for b in (0, 1, 3, 5):
            assert bytes(text[int(off[b]):int(off[b + 1])]) == M.batch_doc(pb, b, kind)
    # the pairs carry no kind: every document is written
    st = np.full(6, 9, np.uint8)
    text, off, _ = write(wctx, pb, M.DOC_PAIRS, 0, st)
    assert list(st) == [0] * 6 and docs_of(text, off) == [M.batch_doc(pb, b, M.DOC_PAIRS) for b in range(6)]


# ------------------------------------------------------------------ 6. offsets beyond 2^32
def test_offsets_beyond_32_bits(wctx):
    """8500 documents of pseudo-random limbs at n = 2048, EF = 128: more than 2^32 bytes of text"""
    n_bits, ef, B = 2048, 128, 8500
    pb = random_batch(41, n_bits, B, ef, True)
    text, off, st = wctx.json_write_range_proof_ni(pb.struct(), 0, np.full(B, 9, np.uint8))
    off = off.astype(np.uint64)
    total = int(off[B])
    print(f"large batch: {B} documents, {total} bytes")
    assert total > 1 << 32 and len(text) == total and not st.any()
    assert (off[1:] > off[:-1]).all()
    straddle = [int(np.searchsorted(off, np.uint64(1 << k), side="right")) - 1 for k in (31, 32)]
    for b in straddle:
        assert off[b] <= 1 << (31 if b == straddle[0] else 32) < off[b + 1]
    for b in sorted({0, 1, B - 1, *straddle, straddle[0] + 1, straddle[1] - 1}):
        assert bytes(text[int(off[b]):int(off[b + 1])]) == M.batch_doc(pb, b, M.DOC_NI), b
    starts = off[:-1].astype(np.int64); ends = off[1:].astype(np.int64) - 1
    assert (text[starts] == ord("{")).all() and (text[ends] == ord("}")).all()
    assert text.min() > 0            # no byte was left unwritten, no NUL anywhere


# ------------------------------------------------------------------ 7. independence from chunking
def test_text_does_not_depend_on_chunking(wctx, monkeypatch):
    pb = random_batch(51, 1024, 40, 16, False)
    pb.resp_kind[7, 3] = 9                                   # an empty document in the middle
    whole, off, _ = write(wctx, pb, M.DOC_NI, zkp.bigint_forms(2, 1))
    # the library's own runs, forced small: ~3 documents per run, then one document per run
    for chunk in (3 * int(off[1]), 1):
        monkeypatch.setenv("ZKP_JSON_WRITE_CHUNK", str(chunk))
        t2, o2, _ = write(wctx, pb, M.DOC_NI, zkp.bigint_forms(2, 1))
        assert np.array_equal(o2, off) and bytes(t2) == bytes(whole)
    monkeypatch.delenv("ZKP_JSON_WRITE_CHUNK")
    # several calls over sub-ranges
    parts = b"".join(bytes(write(wctx, pb.slice(lo, hi), M.DOC_NI, zkp.bigint_forms(2, 1))[0]) for lo, hi in ((0, 1), (1, 17), (17, 40)))
    assert parts == bytes(whole)


# ------------------------------------------------------------------ 8. the C++ host layer
def test_cpp_to_string_batch():
    """tests/cpp/test_json_writer.cpp, built the way tests/test_gpu_seeded_prove.py builds test_seeded.cpp"""
    import subprocess
    root, pkg = H.ROOT, os.path.join(H.ROOT, "zk-paillier_amd")
    src, exe = os.path.join(root, "tests", "cpp", "test_json_writer.cpp"), os.path.join(root, "build", "test_json_writer")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", src, "-o", exe, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 2 and "FAIL" not in out.stdout, out.stdout + out.stderr
