"""GPU tests of zkp_correct_key_ni_verify_json_batch: NiCorrectKeyProof::verify (correct_key_ni.rs:73-100) on documents.  The cases are those
of tests/test_gpu_correct_key.py, written as documents; statuses are the flags-0 reader's, verdicts the oracle's where a document was
converted and REJECT everywhere else."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import helpers as H
import json_writer_model as M
from helpers import pm, L, zkp

pytestmark = pytest.mark.gpu
SALTS = [pm.SALT_STRING, b"", b"\x00\x00ab"]


@functools.lru_cache(maxsize=None)
def cases(n_bits, salt):
    """-> (n [B][kw], documents, sigma [B][11][kw] of the cases that are documents of this width) — built once per shape"""
    import oracle_lib
    oracle = oracle_lib.Oracle()
    kw = n_bits // 32
    keys = [H.test_key(n_bits, tag=t) for t in range(3)] if n_bits == 1024 else [H.fixture_key(), H.test_key(2048, 1)]
    ns, sigmas = [], []
    for p, q, n in keys:
        nl, sg = oracle.correct_key_ni_prove(n_bits, L.int_to_limbs(p, kw // 2), L.int_to_limbs(q, kw // 2), salt)
        ns.append(nl); sigmas.append(sg)
    # tampered sigma, sigma + n (same residue: still accepted), sigma = 0 row, modulus with a small factor, short key
    ns.append(ns[0]); bad = sigmas[0].copy(); bad[7, 1] ^= 4; sigmas.append(bad)
    ns.append(ns[1]); plus = sigmas[1].copy()
    v = L.limbs_to_int(plus[2]) + keys[1][2]
    if v.bit_length() <= n_bits:
        plus[2] = L.int_to_limbs(v, kw)
    sigmas.append(plus)
    ns.append(ns[0]); z = sigmas[0].copy(); z[0] = 0; sigmas.append(z)
    n_small = 6361 * H.gen_prime(pm.Drbg(b"sf-%d" % n_bits), n_bits - 16)
    ns.append(L.int_to_limbs(n_small, kw)); sigmas.append(L.ints_to_limbs(pm.correct_key_rho(n_small, salt), kw))
    pk, qk, nk = H.test_key(n_bits - 64, tag=9)      # n shorter than the ABI width: key_length drives the MGF length
    ns.append(L.int_to_limbs(nk, kw))
    sigmas.append(L.ints_to_limbs(pm.correct_key_proof(pk, qk, salt), kw))
    docs = [M.correct_key_doc([L.limbs_to_int(x) for x in s]) for s in sigmas]
    # around them: an honest proof pretty-printed (falls back, still accepted), one over-wide root, and no NiCorrectKeyProof at all
    honest = [L.limbs_to_int(x) for x in sigmas[0]]
    ns += [ns[0]] * 3
    docs.append(json.dumps(json.loads(docs[0]), indent=2).encode())
    docs.append(M.correct_key_doc(honest[:5] + [honest[5] + (1 << n_bits)] + honest[6:]))
    docs.append(b"[]")
    return np.stack(ns), docs, len(keys)


def flags0_reader(ctx, docs, n_bits):
    sigma = np.full((len(docs), 11, n_bits // 32), 0xA5A5A5A5, np.uint32); st = np.full(len(docs), 9, np.uint8)
    ctx.json_correct_key_proof(docs, n_bits, sigma, st)
    return sigma, st


@pytest.mark.parametrize("device", [False, True], ids=["host-out", "device-out"])
@pytest.mark.parametrize("salt", SALTS, ids=["kzen", "empty", "zero-bytes"])
@pytest.mark.parametrize("n_bits", [1024, 2048])
def test_verdicts_of_documents(ctx, oracle, n_bits, salt, device):
    n_arr, docs, honest = cases(n_bits, salt)
    B = len(docs)
    sigma, st = flags0_reader(ctx, docs, n_bits)
    assert list(st) == [0] * (B - 3) + [zkp.DOC_OK, zkp.DOC_HOST_PATH, zkp.DOC_INVALID]
    ok = st == zkp.DOC_OK
    want = np.full(B, zkp.VERDICT_REJECT, np.uint8)
    want[ok] = oracle.correct_key_ni_verify(n_bits, np.ascontiguousarray(n_arr[ok]), np.ascontiguousarray(sigma[ok]), salt)
    assert list(want[:honest]) == [zkp.VERDICT_ACCEPT] * honest and want[honest] == zkp.VERDICT_REJECT and want[honest + 1] == zkp.VERDICT_ACCEPT
    assert list(want[B - 6:]) == [zkp.VERDICT_REJECT] * 2 + [zkp.VERDICT_ACCEPT] * 2 + [zkp.VERDICT_REJECT] * 2
    if device:
        import torch
        os_, ov = torch.full((B,), 9, dtype=torch.uint8, device="cuda"), torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        n_in = torch.from_numpy(n_arr.view(np.int32)).cuda()
    else:
        os_, ov, n_in = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8), n_arr
    rs, rv = ctx.correct_key_ni_verify_json(docs, n_bits, n_in, salt, device=device, out_status=os_, out_verdict=ov)
    assert rs is os_ and rv is ov
    ctx.synchronize()
    got_s, got_v = (os_.cpu().numpy(), ov.cpu().numpy()) if device else (os_, ov)
    assert list(got_s) == list(st) and list(got_v) == list(want), (list(got_s), list(got_v), list(want))
    assert ctx.last_json_scan() == (B - 2, 2)          # the pretty-printed document and `[]`; the over-wide root has as many digits as the field


def test_outputs_made_by_the_call(ctx):
    n_arr, docs, _ = cases(1024, pm.SALT_STRING)
    st, v = ctx.correct_key_ni_verify_json(docs[:4], 1024, np.ascontiguousarray(n_arr[:4]), pm.SALT_STRING)
    assert list(st) == [0] * 4 and list(v) == [1, 1, 1, 0]
    assert ctx.last_json_scan() == (4, 0) and ctx.last_json_scan_ms()[3] > 0
    st, v = ctx.correct_key_ni_verify_json(docs[:4], 1024, np.ascontiguousarray(n_arr[:4]), pm.SALT_STRING, device=False)
    assert list(v) == [1, 1, 1, 0]


def test_arguments(ctx):
    lib, EINVAL = ctx.lib, zkp.capi.ZKP_EINVAL
    P = zkp.capi.ptr
    n_arr, docs, _ = cases(1024, pm.SALT_STRING)
    st = np.full(1, 9, np.uint8); v = np.full(1, 9, np.uint8)
    off = np.zeros(1, np.uint64); ln = np.array([len(docs[0])], np.uint64)
    buf = C.create_string_buffer(docs[0])
    n0 = np.ascontiguousarray(n_arr[:1])
    salt = (C.c_uint8 * 4).from_buffer_copy(pm.SALT_STRING)
    args = lambda **k: [ctx.h, k.get("text", C.cast(buf, C.c_void_p)), P(off), P(ln), k.get("B", 1), k.get("n_bits", 1024), k.get("n", P(n0)),
                        C.cast(salt, C.c_void_p), 4, k.get("st", P(st)), k.get("v", P(v)), k.get("flags", 0)]
    assert lib.zkp_correct_key_ni_verify_json_batch(*args(B=0)) == zkp.capi.ZKP_OK and st[0] == 9 and v[0] == 9
    for bad in (dict(text=None), dict(n=None), dict(st=None), dict(v=None), dict(n_bits=1536), dict(B=(1 << 24) + 1), dict(flags=2)):
        assert lib.zkp_correct_key_ni_verify_json_batch(*args(**bad)) == EINVAL, bad
        assert lib.zkp_last_error_string(ctx.h), bad
        assert st[0] == 9 and v[0] == 9, bad
    assert lib.zkp_correct_key_ni_verify_json_batch(*args()) == zkp.capi.ZKP_OK and st[0] == zkp.DOC_OK and v[0] == zkp.VERDICT_ACCEPT
