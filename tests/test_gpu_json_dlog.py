"""GPU tests of the DLog document readers and writers: zkp_json_dlog_statement_batch, zkp_json_dlog_proof_batch and their two writers.
tests/json_dlog_model.py says what every document reads to and which documents are canonical; the flags-0 reader is held against the model,
the device route (csrc/kernels_serde_scan.hpp) against the flags-0 reader byte for byte, and the number of documents the scanner leaves
to the host tokeniser against the model's canonical().

These tests are about text: they run on a context of their own with the library's routing."""
import ctypes as C
import random

import numpy as np
import pytest

import helpers as H
import json_dlog_model as D
import json_scan_cases as K
from helpers import pm, L, zkp

pytestmark = pytest.mark.gpu
PROOF, STATEMENT = D.PROOF, D.STATEMENT
KIND_IDS = {PROOF: "proof", STATEMENT: "statement"}
FORM_IDS = {D.BIGINT_DEC: "dec", D.BIGINT_HEX: "hex", D.BIGINT_BYTES: "bytes"}
# the smallest widths, every form; the second width once
SHAPES = [(1024, 544, D.BIGINT_DEC), (1024, 544, D.BIGINT_HEX), (1024, 544, D.BIGINT_BYTES), (2048, 768, D.BIGINT_DEC)]
SHAPE_IDS = [f"{n}-{y}-{FORM_IDS[f]}" for n, y, f in SHAPES]


@pytest.fixture(scope="module")
def sctx():
    c = zkp.Context(0)
    yield c
    c.close()


def random_ints(rnd, words):
    return [rnd.getrandbits(32 * w - rnd.choice((0, 0, 1, 7, 32 * w - 20))) | (1 << 16) for w in words]


def mixed_batch(kind, form, words, seed, count):
    """`count` documents: the mutants of the model, then canonical documents of random values"""
    rnd = random.Random(seed)
    docs = [d for _, d, _ in D.mutants(kind, form, words, [rnd.getrandbits(32 * w - 3) | (1 << (32 * w - 4)) for w in words])]
    assert len(docs) <= count
    while len(docs) < count:
        docs.append(D.write(random_ints(rnd, words), kind, form))
    rnd.shuffle(docs)
    return docs


def read(ctx, kind, packed, n_bits, y_bits, form, device):
    """-> ([uint32 array per field], statuses, (fast, fallback) of the call or None)"""
    text, off, ln = packed
    B = len(off)
    words = D.field_words(kind, n_bits, y_bits)
    buf = (C.c_char * len(text)).from_buffer_copy(text)
    off_a, ln_a = np.array(off, np.uint64), np.array(ln, np.uint64)
    P = zkp.capi.ptr
    if device:
        import torch
        st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        arrs = [torch.full((B, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for w in words]
    else:
        st = np.full(B, 9, np.uint8)
        arrs = [np.full((B, w), 0xA5A5A5A5, np.uint32) for w in words]
    flags = zkp.capi.ZKP_F_DEVICE_PTRS if device else 0
    head = [ctx.h, C.cast(buf, C.c_void_p), P(off_a), P(ln_a), n_bits]
    if kind == PROOF:
        ctx.check(ctx.lib.zkp_json_dlog_proof_batch(*head, y_bits, B, form, *[P(a) for a in arrs], P(st), flags))
    else:
        ctx.check(ctx.lib.zkp_json_dlog_statement_batch(*head, B, form, *[P(a) for a in arrs], P(st), flags))
    if device:
        ctx.synchronize()
        return [a.cpu().numpy().view(np.uint32) for a in arrs], st.cpu().numpy(), ctx.last_json_scan()
    return arrs, st, None


def check(ctx, kind, docs, n_bits, y_bits, form, layout="gaps"):
    """flags 0 against the model, the device route against flags 0, the fall-back count against canonical()"""
    words = D.field_words(kind, n_bits, y_bits)
    packed = K.pack(docs, layout)
    host = read(ctx, kind, packed, n_bits, y_bits, form, False)
    want = [D.read(d, kind, form, words) for d in docs]
    assert list(host[1]) == [w[0] for w in want]
    for f, w in enumerate(words):
        assert np.array_equal(host[0][f], L.ints_to_limbs([x[1][f] for x in want], w)), D.FIELDS[kind][f]
    dev = read(ctx, kind, packed, n_bits, y_bits, form, True)
    assert list(dev[1]) == list(host[1])
    for f in range(len(words)):
        assert np.array_equal(dev[0][f], host[0][f]), D.FIELDS[kind][f]
    canonical = sum(D.canonical(d, kind, form, words) for d in docs)
    print(f"{KIND_IDS[kind]} {FORM_IDS[form]}: {len(docs)} documents, {canonical} canonical, scanner {dev[2]}, statuses {sorted(set(host[1].tolist()))}")
    assert dev[2] == (canonical, len(docs) - canonical)
    return host[1]


# ------------------------------------------------------------------ 1. readers
@pytest.mark.parametrize("kind", [PROOF, STATEMENT], ids=list(KIND_IDS.values()))
@pytest.mark.parametrize("n_bits,y_bits,form", SHAPES, ids=SHAPE_IDS)
def test_readers_agree_with_the_model_and_with_each_other(sctx, n_bits, y_bits, form, kind):
    words = D.field_words(kind, n_bits, y_bits)
    docs = mixed_batch(kind, form, words, b"dlog-docs-%d-%d-%d" % (kind, n_bits, form), 130)
    st = check(sctx, kind, docs, n_bits, y_bits, form, "gaps")
    assert set(st) == {zkp.DOC_OK, zkp.DOC_INVALID, zkp.DOC_HOST_PATH}
    # 65, 3 and 1 documents; other layouts
    check(sctx, kind, docs[:65], n_bits, y_bits, form, "reverse")
    check(sctx, kind, docs[40:43], n_bits, y_bits, form, "packed")
    named = {n: d for n, d, _ in D.mutants(kind, form, words, random_ints(random.Random(5), words))}
    for name in ("canonical", "pretty", "empty", "last field one bit too wide", "last field far too wide"):
        check(sctx, kind, [named[name]], n_bits, y_bits, form, "packed")
    # all canonical: nothing falls back
    canon = [d for d in docs if D.canonical(d, kind, form, words)]
    assert len(canon) >= 100
    check(sctx, kind, canon, n_bits, y_bits, form, "packed")
    assert sctx.last_json_scan() == (len(canon), 0)


def test_a_document_ends_where_its_length_says(sctx):
    n_bits, y_bits, form = 1024, 544, D.BIGINT_DEC
    rnd = random.Random(3)
    for kind in (PROOF, STATEMENT):
        words = D.field_words(kind, n_bits, y_bits)
        a, b_ = (D.write(random_ints(rnd, words), kind, form) for _ in range(2))
        for packed, want in (((a + b_, [0, len(a)], [len(a) - 1, len(b_)]), [zkp.DOC_INVALID, zkp.DOC_OK]),
                             ((a + b_, [0, len(a)], [len(a), len(b_) - 1]), [zkp.DOC_OK, zkp.DOC_INVALID]),
                             ((a + b',"q":"1"}', [0], [len(a)]), [zkp.DOC_OK])):
            host, dev = read(sctx, kind, packed, n_bits, y_bits, form, False), read(sctx, kind, packed, n_bits, y_bits, form, True)
            assert list(host[1]) == want and list(dev[1]) == want
            assert all(np.array_equal(x, y) for x, y in zip(host[0], dev[0]))
            assert dev[2] == (want.count(zkp.DOC_OK), want.count(zkp.DOC_INVALID))


def test_reader_arguments(sctx):
    lib, EINVAL, P = sctx.lib, zkp.capi.ZKP_EINVAL, zkp.capi.ptr
    doc = D.write([1 << 20, 5], PROOF, D.BIGINT_DEC)
    buf = C.create_string_buffer(doc)
    off = np.zeros(1, np.uint64); ln = np.array([len(doc)], np.uint64)
    x = np.full((1, 32), 7, np.uint32); y = np.full((1, 17), 7, np.uint32); st = np.full(1, 9, np.uint8)
    args = lambda **k: [sctx.h, k.get("text", C.cast(buf, C.c_void_p)), P(off), P(ln), k.get("n_bits", 1024), k.get("y_bits", 544), k.get("B", 1),
                        k.get("form", 0), k.get("x", P(x)), P(y), k.get("st", P(st)), k.get("flags", 0)]
    assert lib.zkp_json_dlog_proof_batch(*args(B=0)) == zkp.capi.ZKP_OK and st[0] == 9
    for bad in (dict(text=None), dict(x=None), dict(st=None), dict(n_bits=1536), dict(y_bits=512), dict(y_bits=560), dict(y_bits=1056), dict(form=3),
                dict(B=(1 << 24) + 1), dict(flags=2)):
        assert lib.zkp_json_dlog_proof_batch(*args(**bad)) == EINVAL, bad
        assert st[0] == 9 and (x == 7).all(), bad
    assert lib.zkp_json_dlog_proof_batch(*args()) == zkp.capi.ZKP_OK and st[0] == 0 and L.limbs_to_ints(x) == [1 << 20] and L.limbs_to_ints(y) == [5]


# ------------------------------------------------------------------ 2. writers
def edge_values(rnd, words, B):
    rows = [[0] * len(words), [(1 << (32 * w)) - 1 for w in words], [rnd.getrandbits(32 * w - 8) | (1 << (32 * w - 9)) for w in words],   # zero, widest, a 00 top byte
            [1, 255, 256][:len(words)], [(1 << (32 * w - 1)) for w in words]]
    while len(rows) < B:
        rows.append(random_ints(rnd, words))
    return rows[:B]


def write(ctx, kind, n_bits, y_bits, B, arrs, form):
    if kind == PROOF:
        return ctx.json_write_dlog_proof(n_bits, y_bits, B, arrs[0], arrs[1], form)
    return ctx.json_write_dlog_statement(n_bits, B, arrs[0], arrs[1], arrs[2], form)


@pytest.mark.parametrize("kind", [PROOF, STATEMENT], ids=list(KIND_IDS.values()))
@pytest.mark.parametrize("n_bits,y_bits,form", SHAPES, ids=SHAPE_IDS)
def test_writers_emit_the_models_text(sctx, n_bits, y_bits, form, kind):
    import torch
    words = D.field_words(kind, n_bits, y_bits)
    for B in (1, 3, 65, 130):
        rows = edge_values(random.Random(B + form), words, B)
        arrs = [L.ints_to_limbs([r[f] for r in rows], w) for f, w in enumerate(words)]
        text, off, _ = write(sctx, kind, n_bits, y_bits, B, arrs, form)          # (sizing call, writing call; their offsets are compared inside)
        docs = [bytes(text[int(off[b]):int(off[b + 1])]) for b in range(B)]
        assert docs == [D.write(r, kind, form) for r in rows]
        assert all(D.canonical(d, kind, form, words) for d in docs)
        assert max(len(d) for d in docs) <= zkp.json_doc_bound(kind, n_bits, 0, form)
        # the same from device memory, and back through the device reader: nothing falls back
        dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in arrs]
        text2, off2, _ = write(sctx, kind, n_bits, y_bits, B, dev, form)
        assert np.array_equal(off, off2) and np.array_equal(text, text2)
        back, st, scan = read(sctx, kind, (bytes(text), [int(o) for o in off[:-1]], [len(d) for d in docs]), n_bits, y_bits, form, True)
        assert list(st) == [0] * B and scan == (B, 0)
        assert all(np.array_equal(a, b_) for a, b_ in zip(arrs, back))


def test_writer_sizes_and_refuses_a_short_buffer(sctx):
    n_bits, y_bits, B = 1024, 544, 3
    lib, P = sctx.lib, zkp.capi.ptr
    rows = edge_values(random.Random(1), (32, 17), B)
    x, y = L.ints_to_limbs([r[0] for r in rows], 32), L.ints_to_limbs([r[1] for r in rows], 17)
    off = np.zeros(B + 1, np.uint64)
    assert lib.zkp_json_write_dlog_proof_batch(sctx.h, n_bits, y_bits, B, P(x), P(y), 0, None, 0, P(off), None, 0) == zkp.capi.ZKP_OK
    total = int(off[B])
    assert total == sum(len(D.write(r, PROOF, 0)) for r in rows)
    text = np.full(total, 0x23, np.uint8); off2 = np.zeros(B + 1, np.uint64)
    assert lib.zkp_json_write_dlog_proof_batch(sctx.h, n_bits, y_bits, B, P(x), P(y), 0, P(text), total - 1, P(off2), None, 0) == zkp.capi.ZKP_EINVAL
    assert (text == 0x23).all() and np.array_equal(off, off2) and str(total).encode() in lib.zkp_last_error_string(sctx.h)
    assert lib.zkp_json_write_dlog_proof_batch(sctx.h, n_bits, y_bits, B, P(x), P(y), 0, P(text), total, P(off2), None, 0) == zkp.capi.ZKP_OK
    assert bytes(text) == b"".join(D.write(r, PROOF, 0) for r in rows)
    # arguments
    for bad in (dict(n_bits=1536), dict(y_bits=512), dict(form=3), dict(x=None), dict(off=None), dict(flags=2)):
        a = dict(n_bits=n_bits, y_bits=y_bits, form=0, x=P(x), off=P(off2), flags=0); a.update(bad)
        assert lib.zkp_json_write_dlog_proof_batch(sctx.h, a["n_bits"], a["y_bits"], B, a["x"], P(y), a["form"], None, 0, a["off"], None, a["flags"]) == zkp.capi.ZKP_EINVAL, bad
    assert lib.zkp_json_write_dlog_statement_batch(sctx.h, n_bits, 0, None, None, None, 0, None, 0, P(off2), None, 0) == zkp.capi.ZKP_OK and off2[0] == 0
    assert zkp.json_doc_bound(PROOF, 1536, 0, 0) == 0 and zkp.json_doc_bound(STATEMENT, 1024, 0, 3) == 0 and zkp.json_doc_bound(7, 1024, 0, 0) == 0 and zkp.json_doc_bound(4, 1024, 0, 0) == 0


def test_proofs_are_written_where_the_prover_left_them(sctx):
    """zkp_dlog_prove_batch on device arrays, both documents written from them, read back on the device, verified"""
    import torch
    n_bits, y_bits, kw, B = 1024, 544, 32, 5
    d = pm.Drbg(b"dlog-write-resident")
    rows = []
    for t in range(B):
        p, q, N = H.test_key(n_bits, tag=20 + t % 3)
        g = d.range(2, N - 1); s = d.bits(256)
        rows.append((N, g, pow(pow(g, -1, N), s, N), s, d.bits(512)))
    cuda = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    N_, g_, ni_ = (cuda(L.ints_to_limbs([r[i] for r in rows], kw)) for i in range(3))
    s_, r_ = cuda(L.ints_to_limbs([r[3] for r in rows], 8)), cuda(L.ints_to_limbs([r[4] for r in rows], 16))
    x = torch.zeros((B, kw), dtype=torch.int32, device="cuda"); y = torch.zeros((B, y_bits // 32), dtype=torch.int32, device="cuda")
    sctx.dlog_prove(n_bits, y_bits, B, N_, g_, ni_, s_, r_, x, y)
    for form in FORM_IDS:
        tp, op, _ = sctx.json_write_dlog_proof(n_bits, y_bits, B, x, y, form)
        ts, os_, _ = sctx.json_write_dlog_statement(n_bits, B, N_, g_, ni_, form)
        proofs = [bytes(tp[int(op[b]):int(op[b + 1])]) for b in range(B)]
        statements = [bytes(ts[int(os_[b]):int(os_[b + 1])]) for b in range(B)]
        want = [pm.dlog_prove(*r) for r in rows]
        assert proofs == [D.write(list(w), PROOF, form) for w in want] and statements == [D.write(list(r[:3]), STATEMENT, form) for r in rows]
        st, v = sctx.dlog_verify_json(statements, proofs, n_bits, y_bits, form)
        assert list(st) == [0] * B and list(v) == [zkp.VERDICT_ACCEPT] * B and sctx.last_json_scan() == (2 * B, 0)
