"""GPU tests of zkp_correct_key_ni_prove_batch (include/zkp_hip.h; csrc/kernels_ck_prove.hpp) on the case list of tests/ck_prove_cases.py,
exactly against tests/ck_prove_model.py: every batch on host arrays, device pointers, the round trip through the verifier, the chain into the
document writer and the document verifier, the wipe, chunk independence, the argument checks.  Through the session `ctx` fixture: every
engine runs the ladder once.  Items are 11 per key, so the 16-lane blocks of the split and finish kernels change key mid-block in every
batch of more than one key."""
import numpy as np
import pytest

import ck_prove_cases as CC
from helpers import L, zkp

pytestmark = pytest.mark.gpu


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def run_prove(ctx, n_bits, keys, salt, device=False, with_n=True, with_status=True, keep_device=False):
    """-> [(n, [sigma_i], status)]; keep_device: the device tensors (n, sigma, status) instead"""
    B, hw, kw = len(keys), n_bits // 64, n_bits // 32
    p, q = L.ints_to_limbs([k[0] for k in keys], hw), L.ints_to_limbs([k[1] for k in keys], hw)
    n, sg, st = np.full((B, kw), 9, np.uint32), np.full((B, 11, kw), 9, np.uint32), np.full(B, 9, np.uint8)
    if device:
        import torch
        dp, dq, dn, dsg, dst = (to_dev(a) for a in (p, q, n, sg, st))
        torch.cuda.synchronize()
        ctx.correct_key_ni_prove(n_bits, B, dp, dq, salt, dn if with_n else None, dsg, dst if with_status else None)
        ctx.synchronize()
        if keep_device:
            return dn, dsg, dst
        n, sg, st = dn.cpu().numpy().view(np.uint32), dsg.cpu().numpy().view(np.uint32), dst.cpu().numpy()
    else:
        ctx.correct_key_ni_prove(n_bits, B, p, q, salt, n if with_n else None, sg, st if with_status else None)
    return [(L.limbs_to_int(n[b]) if with_n else None, L.limbs_to_ints(sg[b]), int(st[b]) if with_status else None) for b in range(B)]


def assert_same(got, b, salt):
    want = b["want"][salt]
    bad = [(i, b["tag"][i], got[i][2], want[i][2]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:4]


@pytest.mark.parametrize("name", [n for n, _ in CC.all_batches()])
def test_parity_with_the_model(ctx, name):
    b = dict(CC.all_batches())[name]
    got = run_prove(ctx, b["n_bits"], b["keys"], CC.SALTS[0])
    assert_same(got, b, CC.SALTS[0])


def test_nullable_outputs_and_empty_salt(ctx):
    b = CC.domain()
    got = run_prove(ctx, 1024, b["keys"], CC.SALTS[1], with_n=False, with_status=False)
    assert [g[1] for g in got] == [w[1] for w in b["want"][CC.SALTS[1]]]
    b = CC.one_1024()
    got = run_prove(ctx, 1024, b["keys"], b"")
    assert got == [CC.M.prove(*b["keys"][0], b"")]


def test_device_pointers(ctx):
    b = CC.five_2048()
    got = run_prove(ctx, 2048, b["keys"], CC.SALTS[0], device=True)
    assert_same(got, b, CC.SALTS[0])


@pytest.mark.parametrize("name", ["1024 B=3", "2048 B=5"])
@pytest.mark.parametrize("salt", CC.SALTS, ids=["KZen", "salt8"])
def test_round_trip_through_verify(ctx, name, salt):
    """zkp_correct_key_ni_verify_batch accepts the call's own (out_n, out_sigma) for every good key"""
    b = dict(CC.all_batches())[name]
    B, kw = len(b["keys"]), b["n_bits"] // 32
    assert all(b["prime"]) and all(w[2] == 0 for w in b["want"][salt])
    got = run_prove(ctx, b["n_bits"], b["keys"], salt)
    assert_same(got, b, salt)
    n = L.ints_to_limbs([g[0] for g in got], kw)
    sg = np.stack([L.ints_to_limbs(g[1], kw) for g in got])
    v = np.full(B, 9, np.uint8)
    ctx.correct_key_ni_verify(b["n_bits"], B, n, sg, salt, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] * B
    sg[1, 4, 0] ^= 1                                             # (and the verifier does look at them)
    ctx.correct_key_ni_verify(b["n_bits"], B, n, sg, salt, v)
    assert list(v) == [zkp.VERDICT_ACCEPT] + [zkp.VERDICT_REJECT] + [zkp.VERDICT_ACCEPT] * (B - 2)


def test_chain_into_the_document_writer_and_verifier(ctx):
    """device-resident out_sigma -> zkp_json_write_correct_key_proof_batch -> zkp_correct_key_ni_verify_json_batch"""
    b = CC.three_1024()
    salt = CC.SALTS[0]
    dn, dsg, dst = run_prove(ctx, 1024, b["keys"], salt, device=True, keep_device=True)
    assert list(dst.cpu().numpy()) == [0, 0, 0]
    text, off, _ = ctx.json_write_correct_key_proof(1024, 3, dsg, None)
    docs = [bytes(text[int(off[i]):int(off[i + 1])]) for i in range(3)]
    st, v = ctx.correct_key_ni_verify_json(docs, 1024, dn.cpu().numpy().view(np.uint32), salt)
    assert list(st) == [zkp.DOC_OK] * 3 and list(v) == [zkp.VERDICT_ACCEPT] * 3


def test_secrets_are_wiped(ctx):
    """every block of the call that held p, q or something derived from them is registered and zeroed — after a call that ran, and the
    answer stays 0 after a call that was refused"""
    b = CC.three_1024()
    run_prove(ctx, 1024, b["keys"], CC.SALTS[0])
    assert ctx.witness_residue() == 0
    run_prove(ctx, 1024, CC.domain()["keys"], CC.SALTS[0])
    assert ctx.witness_residue() == 0
    a = np.zeros(4096, np.uint32)
    A = a.ctypes.data
    assert ctx.lib.zkp_correct_key_ni_prove_batch(ctx.h, 1536, 1, A, A, None, 0, A, A, None, 0) == zkp.capi.ZKP_EINVAL
    assert ctx.witness_residue() == 0


def test_chunk_independence(ctx):
    b = CC.five_2048()
    salt = CC.SALTS[0]
    whole = run_prove(ctx, 2048, b["keys"], salt)
    assert whole == run_prove(ctx, 2048, b["keys"][:2], salt) + run_prove(ctx, 2048, b["keys"][2:], salt)


def test_bad_arguments(ctx):
    lib, h = zkp.load(), ctx.h
    a = np.zeros(4096, np.uint32)
    A = a.ctypes.data
    E = zkp.capi.ZKP_EINVAL
    assert lib.zkp_correct_key_ni_prove_batch(None, 1024, 1, A, A, None, 0, A, A, None, 0) == E
    assert lib.zkp_correct_key_ni_prove_batch(h, 1000, 1, A, A, None, 0, A, A, None, 0) == E
    assert lib.zkp_correct_key_ni_prove_batch(h, 8192, 1, A, A, None, 0, A, A, None, 0) == E
    for p, q, sg in ((None, A, A), (A, None, A), (A, A, None)):
        assert lib.zkp_correct_key_ni_prove_batch(h, 1024, 1, p, q, None, 0, A, sg, None, 0) == E
    assert lib.zkp_correct_key_ni_prove_batch(h, 1024, 1, A, A, None, 4, A, A, None, 0) == E          # salt_len without salt
    assert lib.zkp_correct_key_ni_prove_batch(h, 1024, 1, A, A, None, 0, A, A, None, 2) == E          # an unknown flag bit
    assert lib.zkp_correct_key_ni_prove_batch(h, 1024, (1 << 24) + 1, A, A, None, 0, A, A, None, 0) == E
    assert lib.zkp_last_error_string(h)
    assert lib.zkp_correct_key_ni_prove_batch(h, 1024, 0, None, None, None, 0, None, None, None, 0) == zkp.capi.ZKP_OK
    assert not a.any()
