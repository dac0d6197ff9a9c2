"""GPU tests of zkp_range_verifier_output_json_batch: RangeProof::verifier_output on the two received documents of a session.  The yardstick
is the route a verifier chains by hand — the flags-0 readers of EncryptedPairs and Proof, then zkp_range_verifier_output_batch — with the
worse of the two reader statuses and the verdicts of unread sessions masked, plus the oracle's range_verifier_output on the converted
arrays.  Documents come from oracle-made sessions through the helpers of tests/test_wire_format.py and tests/json_writer_model.py."""
import ctypes as C
import re

import numpy as np
import pytest

import helpers as H
import json_scan_cases as JS
import json_writer_model as JW
import seeded_interactive_cases as IC
import test_wire_format as WF
from helpers import L, zkp

pytestmark = pytest.mark.gpu
OK, INVALID, HOST = zkp.DOC_OK, zkp.DOC_INVALID, zkp.DOC_HOST_PATH
ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED
N_BITS = 1024
NAME = "zkp_range_verifier_output_json_batch"


@pytest.fixture(scope="module")
def sctx():
    c = zkp.Context(0)
    yield c
    c.close()


_SESSIONS = {}


def sessions(oracle, ef, shared, B=6, dishonest=None):
    """B oracle-made sessions -> (po after both prover steps, e, e_len, canonical pairs documents, canonical proof documents)"""
    key = (ef, shared, B, dishonest)
    if key not in _SESSIONS:
        keys = IC.keys_for(512 if shared else 1024, shared, B)
        cases = H.build_range_case(b"json-inter-%d-%d" % (ef, B), keys, N_BITS, B, shared=shared, ef=ef)
        if dishonest is not None:
            cases[dishonest] = H.build_range_case(b"json-inter-bad", [cases[dishonest]["n"]], N_BITS, 1, honest=False, ef=ef)[0]
        po, wt = H.fill_batch(cases, N_BITS, shared, oracle)
        e, elen = IC.session_challenge(ef, B)
        assert not IC.oracle_steps(oracle, po, wt, e, elen).any()
        pairs = [JW.batch_doc(po, b, JW.DOC_PAIRS) for b in range(B)]
        proofs = [JW.batch_doc(po, b, JW.DOC_PROOF) for b in range(B)]
        _SESSIONS[key] = (po, e, elen, pairs, proofs)
    return _SESSIONS[key]


def pretty(po, b):
    c1 = [L.limbs_to_int(x) for x in po.c1[b]]; c2 = [L.limbs_to_int(x) for x in po.c2[b]]
    return WF.pairs_json(c1, c2, pretty=True), WF.proof_json(H.responses_from_batch(po, b), pretty=True)


def worse(s1, s2):
    return [INVALID if INVALID in (a, b) else HOST if (a or b) else OK for a, b in zip(s1, s2)]


_YARDSTICK = {}


def yardstick(ctx, oracle, po, pairs, proofs, e, elen, key=None):
    """the readers with flags 0, zkp_range_verifier_output_batch on what they converted, the masking rule; the oracle agrees on the verdicts.
    key: the name of the documents, for the tests that ask for the same ones again — computed once per kernel family"""
    if key is not None:
        key = (getattr(ctx, "test_geometry", None), getattr(ctx, "test_form", None), key)
        if key not in _YARDSTICK:
            _YARDSTICK[key] = yardstick(ctx, oracle, po, pairs, proofs, e, elen)
        return _YARDSTICK[key]
    B, ef = po.batch, po.ef
    pg = IC.clone_inputs(po)
    s1, s2 = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
    ctx.json_encrypted_pairs(pairs, pg.struct(), s1, device=False)
    ctx.json_range_proof(proofs, pg.struct(), s2, device=False)
    v, vo = np.full(B, 7, np.uint8), np.full(B, 7, np.uint8)
    ctx.range_verifier_output(pg.struct(), e, elen, v, device=False)
    oracle.range_verifier_output(pg.struct(), e, elen, vo)
    status = worse(s1, s2)
    ok = [b for b in range(B) if status[b] == OK]
    assert [int(v[b]) for b in ok] == [int(vo[b]) for b in ok]
    return status, [int(v[b]) if status[b] == OK else REJECT for b in range(B)]


def run(ctx, po, pairs, proofs, e, elen, device=False, layout="packed", ef=None):
    """-> (status, verdict) lists.  packed: through Context.range_verifier_output_json; gaps / reverse: the entry point itself on
    json_scan_cases.pack's text, the two lists of spans interleaved in one text"""
    B = len(pairs)
    ef = po.ef if ef is None else ef
    arrs = [po.n, po.range, po.ciphertext, e, elen]
    if device:
        import torch
        arrs = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in arrs]
        torch.cuda.synchronize()
    if layout == "packed":
        st, v = ctx.range_verifier_output_json(pairs, proofs, N_BITS, ef, *arrs, device=device)
    else:
        text, off, ln = JS.pack(list(pairs) + list(proofs), layout)
        off, ln = np.array(off, np.uint64), np.array(ln, np.uint64)
        a_off, a_len, b_off, b_len = (np.ascontiguousarray(a) for a in (off[:B], ln[:B], off[B:], ln[B:]))
        buf = (C.c_char * len(text)).from_buffer_copy(text)
        if device:
            import torch
            st, v = (torch.full((B,), 9, dtype=torch.uint8, device="cuda") for _ in range(2))
        else:
            st, v = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
        p = zkp.capi.ptr
        ctx.check(ctx.lib.zkp_range_verifier_output_json_batch(ctx.h, C.cast(buf, C.c_void_p), p(a_off), p(a_len), p(b_off), p(b_len), B, N_BITS, ef, p(arrs[0]),
                                                               0 if po.shared_key else N_BITS // 32, p(arrs[1]), p(arrs[2]), p(arrs[3]), p(arrs[4]), p(st), p(v),
                                                               zkp.capi.ZKP_F_DEVICE_PTRS if device else 0))
    if device:
        ctx.synchronize()
        st, v = st.cpu().numpy(), v.cpu().numpy()
    return [int(x) for x in st], [int(x) for x in v]


# ------------------------------------------------------------------ 1. verdicts and statuses against the yardstick
def tampered_sessions(oracle, ef, shared):
    po, e, elen, pairs, proofs = sessions(oracle, ef, shared, dishonest=2)
    pairs, proofs, e, elen = list(pairs), list(proofs), e.copy(), elen.copy()
    m = re.match(rb'\{"c1":\["(\d+)"', pairs[1])
    last = m.end(1) - 1
    pairs[1] = pairs[1][:last] + b"%d" % ((int(pairs[1][last:last + 1]) + 1) % 10) + pairs[1][last + 1:]      # one digit of c1[0]
    pairs[3], proofs[3] = pretty(po, 3)
    e[4, (ef - 1) // 8] ^= 0x80 >> ((ef - 1) % 8)                                                            # bit ef - 1: the last one used
    elen[5] -= 1
    return po, e, elen, pairs, proofs


@pytest.mark.parametrize("layout", ["packed", "gaps", "reverse"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("ef,shared", [(40, True), (129, False)], ids=["ef40-shared", "ef129-perkey"])
def test_verdicts_and_statuses_against_the_readers_and_verifier_output(ctx, oracle, ef, shared, device, layout):
    po, e, elen, pairs, proofs = tampered_sessions(oracle, ef, shared)
    want_st, want_v = yardstick(ctx, oracle, po, pairs, proofs, e, elen, key=("tampered", ef, shared))
    assert want_st == [OK] * 6 and want_v == [ACCEPT, REJECT, REJECT, ACCEPT, REJECT, MALFORMED]
    got_st, got_v = run(ctx, po, pairs, proofs, e, elen, device, layout)
    assert got_st == want_st and got_v == want_v, (got_st, got_v)
    assert ctx.last_json_scan() == (10, 2)               # (session 3 is pretty-printed: the host tokeniser, merged in)


# ------------------------------------------------------------------ 2. status merging and masking
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_worse_status_wins_and_unread_sessions_are_rejected(sctx, oracle, device):
    ef, kw = 40, N_BITS // 32
    po, e, elen, pairs, proofs = sessions(oracle, ef, True)
    pairs, proofs = list(pairs), list(proofs)
    proofs[1] = JW.proof_doc(H.responses_from_batch(po, 1)[:-1])                                             # (a) ef - 1 rows
    cut = len(pairs[2]) // 2 + re.search(rb"\d{40}", pairs[2][len(pairs[2]) // 2:]).end()
    assert pairs[2][cut - 1:cut].isdigit() and pairs[2][cut:cut + 1].isdigit()
    pairs[2] = pairs[2][:cut]                                                                                # (b) truncated mid-number
    assert b'"masked_x":"' in proofs[4]
    proofs[4] = re.sub(rb'"masked_x":"\d+"', b'"masked_x":"%d"' % (1 << (32 * kw)), proofs[4], count=1)     # (c) one bit too wide
    pairs[5] = pairs[5].replace(b'"c1":["', b'"c1":["-', 1); proofs[5] = b"["                                # (d) HOST_PATH pairs, INVALID proof
    want_st, want_v = yardstick(sctx, oracle, po, pairs, proofs, e, elen, key="statuses")
    assert want_st == [OK, HOST, INVALID, OK, HOST, INVALID]
    assert want_v == [ACCEPT, REJECT, REJECT, ACCEPT, REJECT, REJECT]
    for layout in ("packed", "gaps"):
        got_st, got_v = run(sctx, po, pairs, proofs, e, elen, device, layout)
        assert got_st == want_st and got_v == want_v, (layout, got_st, got_v)


# ------------------------------------------------------------------ 3. the device route is taken
def test_canonical_documents_stay_on_the_device_route(sctx, oracle):
    po, e, elen, pairs, proofs = sessions(oracle, 40, True)
    B = len(pairs)
    st, v = run(sctx, po, pairs, proofs, e, elen, device=True)
    assert st == [OK] * B and v == [ACCEPT] * B
    assert sctx.last_json_scan() == (2 * B, 0)
    ms = sctx.last_json_scan_ms()
    assert len(ms) == 4 and all(t >= 0 for t in ms) and ms[3] > 0      # upload | pairs read | proofs read | verify
    pairs, proofs = list(pairs), list(proofs)
    k = 2
    for b in (1, 4):
        pairs[b], proofs[b] = pretty(po, b)
    st, v = run(sctx, po, pairs, proofs, e, elen, device=True)
    assert st == [OK] * B and v == [ACCEPT] * B
    fast, fallback = sctx.last_json_scan()
    assert fallback <= 2 * k and fast + fallback == 2 * B      # only text that is not canonical may leave the device route


# ------------------------------------------------------------------ 4. the whole protocol on one context, device-resident
def test_round_trip_from_a_seed_to_a_verdict_on_the_device(ctx, oracle):
    import torch
    ef, B, first = 40, 3, 11
    po, _, _, _, _ = sessions(oracle, ef, True)              # (statements of honest sessions: n, range, ciphertext; x and r below are theirs)
    cases = H.build_range_case(b"json-inter-%d-%d" % (ef, 6), IC.keys_for(512, True, 6), N_BITS, 6, shared=True, ef=ef)[:B]
    kw = N_BITS // 32
    x = np.stack([L.int_to_limbs(c["x"], kw) for c in cases]); r = np.stack([L.int_to_limbs(c["r"], kw) for c in cases])
    pb = zkp.RangeBatch(N_BITS, B, ef, shared_key=True)
    pb.n[:] = po.n; pb.range[:] = po.range[:B]; pb.ciphertext[:] = po.ciphertext[:B]
    dpb = pb.to("cuda")
    dx, dr = torch.from_numpy(x.view(np.int32)).cuda(), torch.from_numpy(r.view(np.int32)).cuda()
    e, elen = IC.session_challenge(ef, B)
    de, dl = torch.from_numpy(e).cuda(), torch.from_numpy(elen).cuda()
    ds = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.range_generate_encrypted_pairs_seeded(dpb.struct(), IC.SEED, first, ds, device=True)
    t1, o1, _ = ctx.json_write_encrypted_pairs(dpb.struct(), device=True)
    ctx.range_generate_proof_seeded(dpb.struct(), dx, dr, IC.SEED, first, de, dl, ds, device=True)
    assert ctx.witness_residue() == 0
    t2, o2, _ = ctx.json_write_range_proof(dpb.struct(), device=True)
    assert not ds.cpu().numpy().any()
    pairs = [bytes(t1[int(o1[b]):int(o1[b + 1])]) for b in range(B)]
    proofs = [bytes(t2[int(o2[b]):int(o2[b + 1])]) for b in range(B)]
    st, v = ctx.range_verifier_output_json(pairs, proofs, N_BITS, ef, dpb.n, dpb.range, dpb.ciphertext, de, dl, device=True)
    ctx.synchronize()
    assert list(st.cpu().numpy()) == [OK] * B and list(v.cpu().numpy()) == [ACCEPT] * B
    assert ctx.last_json_scan() == (2 * B, 0)


# ------------------------------------------------------------------ 5. refused arguments and batch == 0
def test_refused_arguments_and_an_empty_batch(sctx, oracle):
    po, e, elen, pairs, proofs = sessions(oracle, 40, True)
    refused = "status 1: " + NAME
    good = dict(n=po.n, range=po.range, ciphertext=po.ciphertext, e=e, e_len=elen)
    for name in good:
        with pytest.raises(zkp.ZkpError, match=refused):
            sctx.range_verifier_output_json(pairs, proofs, N_BITS, 40, **dict(good, **{name: None}))
    for n_bits, ef in ((N_BITS, 0), (N_BITS, 257), (1000, 40), (3072, 40)):
        with pytest.raises(zkp.ZkpError, match=refused):
            sctx.range_verifier_output_json(pairs, proofs, n_bits, ef, **good)
    B = len(pairs)
    text, off, ln = JS.pack(list(pairs) + list(proofs))
    off, ln = np.array(off, np.uint64), np.array(ln, np.uint64)
    a_off, a_len, b_off, b_len = (np.ascontiguousarray(a) for a in (off[:B], ln[:B], off[B:], ln[B:]))
    buf = (C.c_char * len(text)).from_buffer_copy(text)
    p = zkp.capi.ptr
    st, v = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)

    def call(text=C.cast(buf, C.c_void_p), spans=(a_off, a_len, b_off, b_len), batch=B, n_stride=0, out=(st, v), flags=0):
        return sctx.lib.zkp_range_verifier_output_json_batch(sctx.h, text, *[p(a) for a in spans], batch, N_BITS, 40, p(po.n), n_stride, p(po.range), p(po.ciphertext),
                                                             p(e), p(elen), p(out[0]), p(out[1]), flags)

    bad = [dict(text=None), dict(spans=(None, a_len, b_off, b_len)), dict(spans=(a_off, a_len, b_off, None)), dict(n_stride=5), dict(out=(None, v)), dict(out=(st, None)),
           dict(flags=2), dict(batch=(1 << 24) + 1)]
    for kw in bad:
        assert call(**kw) == zkp.capi.ZKP_EINVAL, kw
        assert NAME in sctx.lib.zkp_last_error_string(sctx.h).decode(), kw
    assert list(st) == [9] * B and list(v) == [9] * B
    assert call(text=None, spans=(None, None, None, None), batch=0, out=(None, None)) == zkp.capi.ZKP_OK
    assert call() == zkp.capi.ZKP_OK and list(st) == [OK] * B and list(v) == [ACCEPT] * B
    s0, v0 = sctx.range_verifier_output_json([], [], N_BITS, 40, **good)
    assert len(s0) == 0 and len(v0) == 0
