"""GPU tests of the sigma-proof document readers and writers: zkp_json_sigma_batch and zkp_json_write_sigma_batch for the eight kinds
ZeroStatement .. MulProof.  tests/json_sigma_model.py says what every document reads to and which documents are canonical; the writer is held
against the model's text, the flags-0 reader against the model, the device route (csrc/kernels_serde_scan.hpp) against the flags-0 reader byte
for byte, and the number of documents the scanner leaves to the host tokeniser against the model's canonical().

These tests are about text: they run on a context of their own with the library's routing."""
import ctypes as C
import random

import numpy as np
import pytest

import json_scan_cases as K
import json_sigma_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu
# the three text forms, and decimal under a hex key: the two forms are independent
FORMS = {0x00: "dec", 0x11: "hex", 0x22: "bytes", 0x10: "hexkey-dec"}
KIND_IDS = [M.NAMES[k] for k in M.KINDS]
P = zkp.capi.ptr


@pytest.fixture(scope="module")
def sctx():
    c = zkp.Context(0)
    yield c
    c.close()


def random_ints(rnd, words):
    return [rnd.getrandbits(32 * w - rnd.choice((0, 0, 1, 7, 32 * w - 20))) | (1 << 16) for w in words]


def edge_rows(rnd, words, B):
    """zero, the widest values, a 00 top byte, small values, the top bit alone, then random rows"""
    rows = [[0] * len(words), [(1 << (32 * w)) - 1 for w in words], [rnd.getrandbits(32 * w - 8) | (1 << (32 * w - 9)) for w in words],
            [1, 255, 256, 65535, 65536][:len(words)], [1 << (32 * w - 1) for w in words]]
    while len(rows) < B:
        rows.append(random_ints(rnd, words))
    return rows[:B]


def read(ctx, kind, packed, n_bits, forms, device):
    """-> ([uint32 array per field], statuses, (fast, fallback) of the call or None)"""
    text, off, ln = packed
    B = len(off)
    words = M.field_words(kind, n_bits)
    buf = (C.c_char * len(text)).from_buffer_copy(text)
    off_a, ln_a = np.array(off, np.uint64), np.array(ln, np.uint64)
    if device:
        import torch
        st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        arrs = [torch.full((B, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for w in words]
    else:
        st = np.full(B, 9, np.uint8)
        arrs = [np.full((B, w), 0xA5A5A5A5, np.uint32) for w in words]
    f = ctx._sigma_fields(kind, arrs)
    ctx.check(ctx.lib.zkp_json_sigma_batch(ctx.h, kind, C.cast(buf, C.c_void_p), P(off_a), P(ln_a), n_bits, B, forms, C.byref(f), P(st),
                                           zkp.capi.ZKP_F_DEVICE_PTRS if device else 0))
    if device:
        ctx.synchronize()
        return [a.cpu().numpy().view(np.uint32) for a in arrs], st.cpu().numpy(), ctx.last_json_scan()
    return arrs, st, None


def check(ctx, kind, docs, n_bits, forms, layout="gaps"):
    """flags 0 against the model, the device route against flags 0, the fall-back count against canonical()"""
    words = M.field_words(kind, n_bits)
    packed = K.pack(docs, layout)
    host = read(ctx, kind, packed, n_bits, forms, False)
    want = [M.read(d, kind, forms, n_bits) for d in docs]
    assert list(host[1]) == [w[0] for w in want]
    for f, w in enumerate(words):
        assert np.array_equal(host[0][f], L.ints_to_limbs([x[1][f] for x in want], w)), M.FIELDS[kind][f]
    dev = read(ctx, kind, packed, n_bits, forms, True)
    assert list(dev[1]) == list(host[1])
    for f in range(len(words)):
        assert np.array_equal(dev[0][f], host[0][f]), M.FIELDS[kind][f]
    canonical = sum(M.canonical(d, kind, forms, n_bits) for d in docs)
    print(f"{M.NAMES[kind]} {FORMS.get(forms, forms)}: {len(docs)} documents, {canonical} canonical, scanner {dev[2]}, statuses {sorted(set(host[1].tolist()))}")
    assert dev[2] == (canonical, len(docs) - canonical)
    return host[1]


def written(ctx, kind, n_bits, rows, forms, device):
    words = M.field_words(kind, n_bits)
    arrs = [L.ints_to_limbs([r[f] for r in rows], w) for f, w in enumerate(words)]
    if device:
        import torch
        arrs = [torch.from_numpy(a.view(np.int32)).cuda() for a in arrs]
    text, off, _ = ctx.json_write_sigma(kind, n_bits, len(rows), arrs, forms)           # (sizing call, writing call; their offsets are compared inside)
    return text, off, [bytes(text[int(off[b]):int(off[b + 1])]) for b in range(len(rows))]


# ------------------------------------------------------------------ 1. writer round trip, canonical batch, mixed batch
@pytest.mark.parametrize("forms", FORMS, ids=FORMS.values())
@pytest.mark.parametrize("kind", M.KINDS, ids=KIND_IDS)
def test_writer_round_trip_and_mixed_batch(sctx, kind, forms):
    n_bits = 1024
    words = M.field_words(kind, n_bits)
    rnd = random.Random(kind * 64 + forms)
    # the writer's bytes are the model's, from host arrays and from device arrays; a batch past one wavefront of documents
    rows = edge_rows(rnd, words, 70)
    text, off, docs = written(sctx, kind, n_bits, rows, forms, False)
    assert docs == [M.write(r, kind, forms) for r in rows]
    assert max(len(d) for d in docs) <= zkp.json_doc_bound(kind, n_bits, 0, forms) == M.doc_bound(kind, n_bits, forms)
    text2, off2, _ = written(sctx, kind, n_bits, rows, forms, True)
    assert np.array_equal(off, off2) and np.array_equal(text, text2)
    # the readers give the arrays back on both routes, and every canonical document is scanned on the device
    st = check(sctx, kind, docs, n_bits, forms, "packed")
    assert list(st) == [0] * len(rows) and sctx.last_json_scan() == (len(rows), 0)
    # a mixed batch: the model's mutants next to canonical documents
    mixed = [d for _, d, _ in M.mutants(kind, forms, n_bits, [rnd.getrandbits(32 * w - 3) | (1 << (32 * w - 4)) for w in words])] + docs[:16]
    assert 36 <= len(mixed) <= 48
    rnd.shuffle(mixed)
    st = check(sctx, kind, mixed, n_bits, forms, "gaps")
    assert set(st) == {zkp.DOC_OK, zkp.DOC_INVALID, zkp.DOC_HOST_PATH}
    check(sctx, kind, mixed[:3], n_bits, forms, "reverse")
    check(sctx, kind, [b""], n_bits, forms, "packed")


# ------------------------------------------------------------------ 2. the other key widths
@pytest.mark.parametrize("n_bits,forms", [(4096, 0x22), (4096, 0x00), (2048, 0x11)], ids=["4096-bytes", "4096-dec", "2048-hex"])
def test_key_widths(sctx, n_bits, forms):
    """8192-bit fields: in the byte-array form the all-ones value fills the scanner's byte buffer (SCAN_MAX_BYTES) to its last byte"""
    for kind in (M.VERLIN_STATEMENT, M.VERLIN_PROOF, M.MUL_PROOF, M.CIPHERTEXT_PROOF):
        words = M.field_words(kind, n_bits)
        rows = edge_rows(random.Random(n_bits + kind), words, 6)
        text, off, docs = written(sctx, kind, n_bits, rows, forms, True)
        assert docs == [M.write(r, kind, forms) for r in rows]
        assert max(len(d) for d in docs) <= zkp.json_doc_bound(kind, n_bits, 0, forms)
        wide = M.write([1 << (32 * w) for w in words], kind, forms)                 # every field one bit too wide
        st = check(sctx, kind, docs + [wide, json_pretty(docs[1])], n_bits, forms, "gaps")
        assert list(st) == [0] * 6 + [zkp.DOC_HOST_PATH, 0]


def json_pretty(doc):
    import json
    return json.dumps(json.loads(doc), indent=1).encode()


# ------------------------------------------------------------------ 3. arguments
def test_arguments(sctx):
    lib, OK, EINVAL = sctx.lib, zkp.capi.ZKP_OK, zkp.capi.ZKP_EINVAL
    kind, n_bits, B = M.CIPHERTEXT_PROOF, 1024, 3
    words = M.field_words(kind, n_bits)
    rows = edge_rows(random.Random(1), words, B)
    arrs = [L.ints_to_limbs([r[f] for r in rows], w) for f, w in enumerate(words)]
    fields = sctx._sigma_fields(kind, arrs)
    off = np.zeros(B + 1, np.uint64)
    write = lambda **k: lib.zkp_json_write_sigma_batch(sctx.h, k.get("kind", kind), k.get("n_bits", n_bits), k.get("B", B), k.get("f", C.byref(fields)), k.get("forms", 0),
                                                       k.get("text"), k.get("cap", 0), k.get("off", P(off)), None, k.get("flags", 0))
    assert write() == OK
    total = int(off[B])
    assert total == sum(len(M.write(r, kind, 0)) for r in rows)
    text = np.full(total, 0x23, np.uint8); off2 = np.zeros(B + 1, np.uint64)
    assert write(text=P(text), cap=total - 1, off=P(off2)) == EINVAL                  # a short buffer: offsets written, no byte touched
    assert (text == 0x23).all() and np.array_equal(off, off2) and str(total).encode() in lib.zkp_last_error_string(sctx.h)
    assert write(text=P(text), cap=total, off=P(off2)) == OK and bytes(text) == b"".join(M.write(r, kind, 0) for r in rows)
    missing = sctx._sigma_fields(kind, arrs)
    missing.f[2] = None
    for bad in (dict(kind=3), dict(kind=4), dict(kind=7), dict(kind=16), dict(kind=5), dict(n_bits=1536), dict(forms=0x03), dict(forms=0x30), dict(forms=0x100),
                dict(f=None), dict(f=C.byref(missing)), dict(off=None), dict(flags=2), dict(B=(1 << 24) + 1)):
        assert write(**bad) == EINVAL, bad
    assert write(B=0, f=None, off=P(off2)) == OK and off2[0] == 0
    # the reader
    doc = M.write(rows[0], kind, 0)
    buf = C.create_string_buffer(doc)
    o1 = np.zeros(1, np.uint64); l1 = np.array([len(doc)], np.uint64); st = np.full(1, 9, np.uint8)
    outs = [np.full((1, w), 7, np.uint32) for w in words]
    fo = sctx._sigma_fields(kind, outs)
    fm = sctx._sigma_fields(kind, outs)
    fm.f[1] = None
    rd = lambda **k: lib.zkp_json_sigma_batch(sctx.h, k.get("kind", kind), k.get("text", C.cast(buf, C.c_void_p)), P(o1), P(l1), k.get("n_bits", n_bits), k.get("B", 1),
                                              k.get("forms", 0), k.get("f", C.byref(fo)), k.get("st", P(st)), k.get("flags", 0))
    assert rd(B=0) == OK and st[0] == 9
    for bad in (dict(kind=3), dict(kind=4), dict(kind=7), dict(kind=16), dict(kind=6), dict(text=None), dict(n_bits=1536), dict(forms=0x03), dict(forms=0x30),
                dict(f=None), dict(f=C.byref(fm)), dict(st=None), dict(flags=2), dict(B=(1 << 24) + 1)):
        assert rd(**bad) == EINVAL, bad
        assert st[0] == 9 and all((o == 7).all() for o in outs), bad
    assert rd() == OK and st[0] == 0 and [L.limbs_to_ints(o)[0] for o in outs] == rows[0]
    # the verify entry point takes the four proof kinds only
    vs = np.full(1, 9, np.uint8); vv = np.full(1, 9, np.uint8)
    vf = lambda **k: lib.zkp_sigma_verify_json_batch(sctx.h, k.get("kind", kind), C.cast(buf, C.c_void_p), P(o1), P(l1), P(o1), P(l1), 1, k.get("n_bits", n_bits),
                                                     k.get("forms", 0), k.get("vs", P(vs)), P(vv), k.get("flags", 0))
    for bad in (dict(kind=M.CIPHERTEXT_STATEMENT), dict(kind=4), dict(kind=7), dict(kind=5), dict(kind=16), dict(n_bits=3072), dict(forms=0x33), dict(vs=None), dict(flags=4)):
        assert vf(**bad) == EINVAL, bad
        assert vs[0] == 9 and vv[0] == 9
    assert vf() == OK and (vs[0], vv[0]) == (zkp.DOC_INVALID, zkp.VERDICT_REJECT)        # a proof is no statement: a missing field
    # zkp_json_doc_bound: the eight kinds, nothing for the holes in the numbering or for arguments no writer accepts
    for k in M.KINDS:
        for forms in FORMS:
            assert zkp.json_doc_bound(k, 2048, 0, forms) == M.doc_bound(k, 2048, forms) > 0
    assert [zkp.json_doc_bound(k, 1024, 0, 0) for k in (4, 7, 16)] == [0, 0, 0]
    assert zkp.json_doc_bound(8, 1536, 0, 0) == 0 and zkp.json_doc_bound(9, 1024, 0, 0x03) == 0 and zkp.json_doc_bound(9, 1024, 0, 0x100) == 0


# ------------------------------------------------------------------ 4. a prover's output is serialised where it lies
def test_proofs_are_written_where_the_prover_left_them(sctx):
    import torch
    import sigma_json_cases as S
    n_bits, kw, B = 1024, 32, 5
    cs = S.honest_pairs(M.ZERO_PROOF, 6)
    d = random.Random(9)
    ns = [r[0] for r in cs["st_ints"][:B]]
    r, rp = [d.randrange(2, n) for n in ns], [d.randrange(2, n) for n in ns]
    cuda = lambda ints, w: torch.from_numpy(L.ints_to_limbs(ints, w).view(np.int32)).cuda()
    n_, r_, rp_ = cuda(ns, kw), cuda(r, kw), cuda(rp, kw)
    c_ = cuda([pow(x, n, n * n) for x, n in zip(r, ns)], 2 * kw)
    z = torch.zeros((B, 2 * kw), dtype=torch.int32, device="cuda"); a = torch.zeros_like(z)
    sctx.zero_proof_prove(n_bits, B, n_, kw, c_, r_, rp_, z, a)
    for forms in FORMS:
        tp, op, _ = sctx.json_write_sigma(M.ZERO_PROOF, n_bits, B, [z, a], forms)
        ts, os_, _ = sctx.json_write_sigma(M.ZERO_STATEMENT, n_bits, B, [n_, c_], forms)
        proofs = [bytes(tp[int(op[b]):int(op[b + 1])]) for b in range(B)]
        statements = [bytes(ts[int(os_[b]):int(os_[b + 1])]) for b in range(B)]
        assert statements == [M.write([n, pow(x, n, n * n)], M.ZERO_STATEMENT, forms) for x, n in zip(r, ns)]
        assert all(M.canonical(p, M.ZERO_PROOF, forms, n_bits) for p in proofs)
        st, v = sctx.sigma_verify_json(M.ZERO_PROOF, statements, proofs, n_bits, forms)
        assert list(st) == [0] * B and list(v) == [zkp.VERDICT_ACCEPT] * B and sctx.last_json_scan() == (2 * B, 0)
