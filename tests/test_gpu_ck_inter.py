"""GPU tests of the interactive CorrectKey calls (include/zkp_hip.h; csrc/kernels_ck_inter.hpp) on the case list of tests/ck_inter_cases.py,
exactly against tests/ck_inter_model.py (which tests/test_ck_inter_model.py holds to the reference and the C oracle): the challenge with given
nonces, the seeded challenge, the prove in every error class and at every width, the round trip on device memory, the wipe, the argument
checks.  Through the session `ctx` fixture: every engine runs the ladder once.  Items are K per session, so the 16-lane blocks change
session mid-block whenever K is no multiple of 16."""
import numpy as np
import pytest

import ck_inter_cases as CC
import ck_inter_model as M
from helpers import L, zkp

pytestmark = pytest.mark.gpu

CHAL_NAMES = ["1024 B=3 K=3", "2048 shared B=2 K=40", "4096 B=1 K=2", "domain"]
PROVE_NAMES = ["1024 classes", "2048 honest K=40", "4096 honest"]


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def rows(vals, words):
    """[B][K] integers -> [B][K][words] limbs"""
    return np.stack([L.ints_to_limbs(v, words) for v in vals])


def unpack(B, sn, e, z, sd, st):
    return [(L.limbs_to_ints(sn[b]), L.limbs_to_int(e[b]), L.limbs_to_ints(z[b]), L.limbs_to_int(sd[b]) if sd is not None else None,
             int(st[b]) if st is not None else None) for b in range(B)]


def run_challenge(ctx, b, lo=0, hi=None, seed=None, device=False, with_digest=True, with_status=True):
    """given nonces (b has s, r) or seeded -> [(sn, e, z, s_digest, status)] of sessions lo .. hi"""
    n_bits, K, kw = b["n_bits"], b["K"], b["n_bits"] // 32
    hi = len(b["want"]) if hi is None else hi
    B = hi - lo
    n = L.ints_to_limbs(b["n"] if b["shared"] else b["n"][lo:hi], kw)
    stride = 0 if b["shared"] else kw
    sn, z = np.full((B, K, kw), 9, np.uint32), np.full((B, K, kw), 9, np.uint32)
    e, sd, st = np.full((B, 8), 9, np.uint32), np.full((B, 8), 9, np.uint32), np.full(B, 9, np.uint8)
    ins = [n] if seed else [n, rows(b["s"][lo:hi], kw), rows(b["r"][lo:hi], kw)]
    outs = [sn, e, z, sd if with_digest else None, st if with_status else None]
    if device:
        import torch
        ins = [to_dev(a) for a in ins]
        outs = [to_dev(a) if a is not None else None for a in outs]
        torch.cuda.synchronize()
    if seed:
        ctx.correct_key_challenge_seeded(n_bits, B, K, ins[0], stride, seed, CC.FIRST_INDEX + lo, *outs)
    else:
        ctx.correct_key_challenge(n_bits, B, K, ins[0], stride, ins[1], ins[2], *outs)
    if device:
        ctx.synchronize()
        outs = [to_host(a) if a is not None else None for a in outs]
    return unpack(B, *outs)


def run_prove(ctx, b, lo=0, hi=None, device=False, with_error=True):
    """-> [(code, s_digest)] of sessions lo .. hi"""
    n_bits, K, hw, kw = b["n_bits"], b["K"], b["n_bits"] // 64, b["n_bits"] // 32
    hi = len(b["want"]) if hi is None else hi
    B = hi - lo
    keys = b["keys"][lo:hi]
    ins = [L.ints_to_limbs([k[0] for k in keys], hw), L.ints_to_limbs([k[1] for k in keys], hw), rows(b["sn"][lo:hi], kw), L.ints_to_limbs(b["e"][lo:hi], 8),
           rows(b["z"][lo:hi], kw)]
    sd, err = np.full((B, 8), 9, np.uint32), np.full(B, 9, np.uint8)
    outs = [sd, err if with_error else None]
    if device:
        import torch
        ins = [to_dev(a) for a in ins]
        outs = [to_dev(a) if a is not None else None for a in outs]
        torch.cuda.synchronize()
    ctx.correct_key_prove(n_bits, B, K, *ins, *outs)
    if device:
        ctx.synchronize()
        outs = [to_host(a) if a is not None else None for a in outs]
    return [(int(outs[1][i]) if with_error else None, L.limbs_to_int(outs[0][i])) for i in range(B)]


BATCHES = {"1024 B=3 K=3": CC.chal_1024, "2048 shared B=2 K=40": CC.chal_2048_shared, "4096 B=1 K=2": CC.chal_4096, "domain": CC.chal_domain,
           "1024 classes": CC.prove_1024, "2048 honest K=40": CC.prove_2048, "4096 honest": CC.prove_4096}
assert list(BATCHES) == CHAL_NAMES + PROVE_NAMES


def batch_by_name(name):
    """(built on first use and kept: the reference is computed once for all engines)"""
    return BATCHES[name]()


# ---- challenge with given nonces

@pytest.mark.parametrize("name", CHAL_NAMES)
def test_challenge_equals_the_oracle(ctx, name):
    b = batch_by_name(name)
    got = run_challenge(ctx, b)
    bad = [(i, b["tag"][i]) for i in range(len(got)) if got[i] != b["want"][i]]
    assert not bad, bad


def test_challenge_nullable_outputs_and_device_pointers(ctx):
    b = CC.chal_domain()
    got = run_challenge(ctx, b, with_digest=False, with_status=False)
    assert [g[:3] for g in got] == [w[:3] for w in b["want"]]
    assert run_challenge(ctx, b, device=True) == b["want"]


# ---- seeded challenge

@pytest.mark.parametrize("case", ["seeded_1024", "seeded_2048_shared"])
def test_seeded_challenge_equals_the_model(ctx, case):
    b = getattr(CC, case)()
    assert run_challenge(ctx, b, seed=CC.SEED) == b["want"]


def test_seeded_challenge_chunks_null_digest_device(ctx):
    b = CC.seeded_1024()
    assert run_challenge(ctx, b, 0, 2, seed=CC.SEED) + run_challenge(ctx, b, 2, 4, seed=CC.SEED) == b["want"]
    got = run_challenge(ctx, b, seed=CC.SEED, with_digest=False)
    assert [g[:3] + g[4:] for g in got] == [w[:3] + w[4:] for w in b["want"]]
    assert run_challenge(ctx, b, seed=CC.SEED, device=True) == b["want"]
    other = run_challenge(ctx, b, seed=CC.OTHER_SEED)
    assert all(o[4] == w[4] and (o == w) == (w[4] != 0) for o, w in zip(other, b["want"]))


# ---- prove

@pytest.mark.parametrize("name", PROVE_NAMES)
def test_prove_equals_the_model(ctx, name):
    b = batch_by_name(name)
    got = run_prove(ctx, b)
    bad = [(i, b["tag"][i], got[i][0], b["want"][i][0]) for i in range(len(got)) if got[i] != b["want"][i]]
    assert not bad, bad


def test_prove_device_pointers_null_error_chunks(ctx):
    b = CC.prove_1024()
    assert run_prove(ctx, b, device=True) == b["want"]
    assert [g[1] for g in run_prove(ctx, b, with_error=False)] == [w[1] for w in b["want"]]
    assert run_prove(ctx, b, 0, 5) + run_prove(ctx, b, 5) == b["want"]


# ---- the three messages on device memory

def test_round_trip_on_device_memory(ctx):
    import torch
    n_bits, K, B = 1024, 3, 3
    hw, kw = n_bits // 64, n_bits // 32
    keys = [CC.H.test_key(1024, t) for t in range(3)]
    dn = to_dev(L.ints_to_limbs([k[2] for k in keys], kw))
    dp, dq = to_dev(L.ints_to_limbs([k[0] for k in keys], hw)), to_dev(L.ints_to_limbs([k[1] for k in keys], hw))
    dsn, dz = torch.zeros((B, K, kw), dtype=torch.int32, device="cuda"), torch.zeros((B, K, kw), dtype=torch.int32, device="cuda")
    de, dproof = torch.zeros((B, 8), dtype=torch.int32, device="cuda"), torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    dst, derr, dv = (torch.full((B,), 9, dtype=torch.uint8, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    ctx.correct_key_challenge_seeded(n_bits, B, K, dn, kw, CC.SEED, CC.FIRST_INDEX, dsn, de, dz, None, dst)      # (the aid is not even asked for)
    ctx.correct_key_prove(n_bits, B, K, dp, dq, dsn, de, dz, dproof, derr)
    ctx.correct_key_verify_seeded(n_bits, B, K, dn, kw, CC.SEED, CC.FIRST_INDEX, dproof, dv)
    ctx.synchronize()
    assert list(to_host(dst)) == [0] * B and list(to_host(derr)) == [0] * B and list(to_host(dv)) == [zkp.VERDICT_ACCEPT] * B
    proof = to_host(dproof)
    assert [L.limbs_to_int(proof[b]) for b in range(B)] == [M.challenge_seeded(keys[b][2], CC.SEED, CC.FIRST_INDEX + b, K)[3] for b in range(B)]
    flipped = proof.copy()
    flipped[1, 5] ^= 1 << 9
    v = np.full(B, 9, np.uint8)
    n = L.ints_to_limbs([k[2] for k in keys], kw)
    ctx.correct_key_verify_seeded(n_bits, B, K, n, kw, CC.SEED, CC.FIRST_INDEX, flipped, v)
    assert list(v) == [zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_ACCEPT]
    ctx.correct_key_verify_seeded(n_bits, B, K, n, kw, CC.OTHER_SEED, CC.FIRST_INDEX, proof, v)
    assert list(v) == [zkp.VERDICT_REJECT] * B
    n[1, 0] ^= 1                                                   # an even n: where the seeded challenge is MALFORMED, so is the verdict
    ctx.correct_key_verify_seeded(n_bits, B, K, n, kw, CC.SEED, CC.FIRST_INDEX, proof, v)
    assert list(v) == [zkp.VERDICT_ACCEPT, zkp.VERDICT_MALFORMED, zkp.VERDICT_ACCEPT]


# ---- wipe, arguments

def test_secrets_are_wiped(ctx):
    run_challenge(ctx, CC.chal_1024())
    assert ctx.witness_residue() == 0
    run_challenge(ctx, CC.seeded_1024(), seed=CC.SEED)
    assert ctx.witness_residue() == 0
    run_prove(ctx, CC.prove_1024())                                # (bad keys among them)
    assert ctx.witness_residue() == 0
    a = np.zeros(4096, np.uint32)
    A = a.ctypes.data
    assert ctx.lib.zkp_correct_key_prove_batch(ctx.h, 1536, 1, 3, A, A, A, A, A, A, None, 0) == zkp.capi.ZKP_EINVAL
    assert ctx.witness_residue() == 0


def test_bad_arguments(ctx):
    lib, h = zkp.load(), ctx.h
    a = np.zeros(8192, np.uint32)
    A = a.ctypes.data
    E = zkp.capi.ZKP_EINVAL
    seed = bytes(32)

    def chal(c=h, n_bits=1024, B=1, K=3, n=A, stride=0, s=A, r=A, sn=A, e=A, z=A, flags=0):
        return lib.zkp_correct_key_challenge_batch(c, n_bits, B, K, n, stride, s, r, sn, e, z, A, None, flags)

    def seeded(c=h, n_bits=1024, B=1, K=3, n=A, stride=0, sd=seed, sn=A, e=A, z=A, flags=0):
        return lib.zkp_correct_key_challenge_seeded_batch(c, n_bits, B, K, n, stride, sd, 0, sn, e, z, A, None, flags)

    def prove(c=h, n_bits=1024, B=1, K=3, p=A, q=A, sn=A, e=A, z=A, out=A, flags=0):
        return lib.zkp_correct_key_prove_batch(c, n_bits, B, K, p, q, sn, e, z, out, None, flags)

    def verify(c=h, n_bits=1024, B=1, K=3, n=A, stride=0, sd=seed, proof=A, v=A, flags=0):
        return lib.zkp_correct_key_verify_seeded_batch(c, n_bits, B, K, n, stride, sd, 0, proof, v, flags)

    required = {chal: ("n", "s", "r", "sn", "e", "z"), seeded: ("n", "sd", "sn", "e", "z"), prove: ("p", "q", "sn", "e", "z", "out"), verify: ("n", "sd", "proof", "v")}
    for f, ptrs in required.items():
        assert f(c=None) == E
        for n_bits in (1000, 1536, 8192):
            assert f(n_bits=n_bits) == E
        assert f(K=0) == E and f(K=257) == E
        assert f(B=(1 << 24) // 3 + 1) == E and f(B=(1 << 24) + 1, K=1) == E
        for name in ptrs:
            assert f(**{name: None}) == E, (f.__name__, name)
        assert f(flags=2) == E and f(flags=1 << 31) == E
        assert lib.zkp_last_error_string(h)
        assert f(B=0) == zkp.capi.ZKP_OK
    for f in (chal, seeded, verify):
        assert f(stride=16) == E
    assert not a.any()
