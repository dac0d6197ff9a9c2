"""GPU tests of zkp_dlog_verify_json_batch: CompositeDLogProof::verify (wi_dlog_proof.rs:67-91) on (statement, proof) document pairs.
Statuses are the model's (tests/json_dlog_model.py) plus the domain rule of the header — N odd and non-zero, g, ni, x < N, else
ZKP_DOC_HOST_PATH —, verdicts the oracle's on the pairs inside the domain and REJECT everywhere else."""
import ctypes as C
import functools
import json
import random

import numpy as np
import pytest

import helpers as H
import json_dlog_model as D
from helpers import pm, L, zkp

pytestmark = pytest.mark.gpu
OK, INVALID, HOST = zkp.DOC_OK, zkp.DOC_INVALID, zkp.DOC_HOST_PATH
ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED
SHAPES = [(1024, 544), (2048, 768)]


@functools.lru_cache(maxsize=None)
def classes(n_bits, y_bits):
    """-> [(name, (N, g, ni), (x, y), status, verdict or None = the oracle's)]: one pair of every class, proofs made by the oracle's prover"""
    import oracle_lib
    oracle = oracle_lib.Oracle()
    kw = n_bits // 32
    d = pm.Drbg(b"dlog-verify-json-%d" % n_bits)

    def prove(N, g, ni, s):
        x, y = oracle.dlog_prove(n_bits, y_bits, *(L.ints_to_limbs([v], kw) for v in (N, g, ni)), L.ints_to_limbs([s], 8), L.ints_to_limbs([d.bits(512)], 16))
        return L.limbs_to_int(x[0]), L.limbs_to_int(y[0])
    honest = []
    for t in range(3):
        p, q, N = H.test_key(n_bits, tag=20 + t)
        g = d.range(2, N - 1); s = d.bits(256)
        ni = pow(pow(g, -1, N), s, N)
        honest.append(((N, g, ni), prove(N, g, ni, s), s))
    (N, g, ni), (x, y), s = honest[0]
    p, q, _ = H.test_key(n_bits, tag=20)
    out = [("honest %d" % t, st, pf, OK, ACCEPT) for t, (st, pf, _) in enumerate(honest)]
    out += [("tampered x", (N, g, ni), (x ^ 2, y), OK, REJECT), ("tampered y", (N, g, ni), (x, y ^ 1), OK, REJECT)]
    plus = (N, g, pow(g, s, N))                                             # :145-168, "+secret"
    out.append(("+secret", plus, prove(*plus, s), OK, REJECT))
    rand = (N, g, d.range(2, N - 1))                                        # :172-196, a random ni
    out.append(("random ni", rand, prove(*rand, s), OK, REJECT))
    out += [("N <= 2^128", ((1 << 128) - 159, 5, 7), (3, 4), OK, MALFORMED),
            ("gcd(g, N) != 1", (N, p, ni), (x, y), OK, MALFORMED),
            ("gcd(ni, N) != 1", (N, g, q * 3), (x, y), OK, MALFORMED)]
    # outside the limb kernels' domain: the caller's host path decides, here REJECT
    out += [("even N", (N + 1, g, ni), (x, y), HOST, REJECT),
            ("N = 0", (0, g, ni), (x, y), HOST, REJECT),
            ("g = N", (N, N, ni), (x, y), HOST, REJECT),
            ("ni = N + 1", (N, g, N + 1), (x, y), HOST, REJECT),
            ("x = N", (N, g, ni), (N, y), HOST, REJECT),
            ("x = 2^n_bits - 1", (N, g, ni), ((1 << n_bits) - 1, y), HOST, REJECT),
            ("y of y_bits + 1 bits", (N, g, ni), (x, y | (1 << y_bits)), HOST, REJECT),
            ("y of y_bits bits", (N, g, ni), (x, y | (1 << (y_bits - 1))), OK, REJECT)]
    return out


def documents(cls, form):
    return [D.write(list(st), D.STATEMENT, form) for _, st, _, _, _ in cls], [D.write(list(pf), D.PROOF, form) for _, _, pf, _, _ in cls]


def in_domain(st, pf):
    N, g, ni = st
    return N % 2 == 1 and g < N and ni < N and pf[0] < N


def expected(oracle, statements, proofs, n_bits, y_bits, form):
    """statuses from the model and the domain rule; verdicts from the oracle on the pairs that are OK, REJECT elsewhere"""
    kw = n_bits // 32
    ws, wp = D.field_words(D.STATEMENT, n_bits, y_bits), D.field_words(D.PROOF, n_bits, y_bits)
    status, rows = [], []
    for s, p in zip(statements, proofs):
        (a, st), (b, pf) = D.read(s, D.STATEMENT, form, ws), D.read(p, D.PROOF, form, wp)
        both = INVALID if INVALID in (a, b) else HOST if HOST in (a, b) else OK
        if both == OK and not in_domain(st, pf):
            both = HOST
        status.append(both)
        if both == OK:
            rows.append(st + pf)
    verdict = np.full(len(status), REJECT, np.uint8)
    if rows:
        arrs = [L.ints_to_limbs([r[i] for r in rows], w) for i, w in enumerate((kw, kw, kw, kw, y_bits // 32))]
        verdict[np.array(status) == OK] = oracle.dlog_verify(n_bits, y_bits, *arrs)
    return status, list(verdict)


def run(ctx, statements, proofs, n_bits, y_bits, form, device):
    B = len(statements)
    if device:
        import torch
        os_, ov = torch.full((B,), 9, dtype=torch.uint8, device="cuda"), torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    else:
        os_, ov = np.full(B, 9, np.uint8), np.full(B, 9, np.uint8)
    rs, rv = ctx.dlog_verify_json(statements, proofs, n_bits, y_bits, form, device=device, out_status=os_, out_verdict=ov)
    assert rs is os_ and rv is ov
    ctx.synchronize()
    return (os_.cpu().tolist(), ov.cpu().tolist()) if device else (list(os_), list(ov))


# ------------------------------------------------------------------ 1. every class, next to honest neighbours
@pytest.mark.parametrize("form", [D.BIGINT_DEC, D.BIGINT_HEX, D.BIGINT_BYTES], ids=["dec", "hex", "bytes"])
@pytest.mark.parametrize("n_bits,y_bits", SHAPES)
def test_verdicts_of_every_class(ctx, oracle, n_bits, y_bits, form):
    cls = classes(n_bits, y_bits)
    # every class between two honest proofs
    order = []
    for c in cls[3:]:
        order += [cls[len(order) % 3], c]
    order.append(cls[0])
    sd, pd = documents(order, form)
    want_s, want_v = expected(oracle, sd, pd, n_bits, y_bits, form)
    assert want_s == [c[3] for c in order] and want_v == [c[4] for c in order], [(c[0], s, v) for c, s, v in zip(order, want_s, want_v) if (s, v) != (c[3], c[4])]
    got = run(ctx, sd, pd, n_bits, y_bits, form, False)
    assert got == (want_s, want_v), [(c[0], s, v) for c, s, v in zip(order, *got) if (s, v) != (c[3], c[4])]
    # every document here is canonical except where a value is wider than its field (hex / bytes: the text is too long for the scanner)
    canon = sum(D.canonical(s, D.STATEMENT, form, D.field_words(D.STATEMENT, n_bits, y_bits)) for s in sd) + \
        sum(D.canonical(p, D.PROOF, form, D.field_words(D.PROOF, n_bits, y_bits)) for p in pd)
    assert ctx.last_json_scan() == (canon, 2 * len(sd) - canon) and canon >= 2 * len(sd) - 2
    # batches of 1 and 3
    for lo, hi in ((0, 1), (1, 2), (3, 4), (0, 3), (20, 23)):
        assert run(ctx, sd[lo:hi], pd[lo:hi], n_bits, y_bits, form, False) == (want_s[lo:hi], want_v[lo:hi])


# ------------------------------------------------------------------ 2. one mixed batch of 130, 65 of it, host and device outputs
@functools.lru_cache(maxsize=None)
def mixed(n_bits, y_bits, form):
    cls = classes(n_bits, y_bits)
    rnd = random.Random(130 + form)
    ws, wp = D.field_words(D.STATEMENT, n_bits, y_bits), D.field_words(D.PROOF, n_bits, y_bits)
    (N, g, ni), (x, y) = cls[0][1], cls[0][2]
    sm = [m[1] for m in D.mutants(D.STATEMENT, form, ws, [N, g, ni])]
    pmut = [m[1] for m in D.mutants(D.PROOF, form, wp, [x, y])]
    good_s, good_p = D.write([N, g, ni], D.STATEMENT, form), D.write([x, y], D.PROOF, form)
    sd, pd = [], []
    for m in sm:                       # a mutated statement with the honest proof, a mutated proof with the honest statement
        sd.append(m); pd.append(good_p)
    for m in pmut:
        sd.append(good_s); pd.append(m)
    cs, cp = documents(cls, form)
    while len(sd) < 130:
        k = rnd.randrange(len(cls))
        sd.append(cs[k]); pd.append(cp[k])
    order = list(range(130)); rnd.shuffle(order)
    return [sd[k] for k in order], [pd[k] for k in order]


@pytest.mark.parametrize("device", [False, True], ids=["host-out", "device-out"])
@pytest.mark.parametrize("n_bits,y_bits,form", [(1024, 544, D.BIGINT_DEC), (1024, 544, D.BIGINT_HEX), (1024, 544, D.BIGINT_BYTES), (2048, 768, D.BIGINT_DEC)],
                         ids=["1024-dec", "1024-hex", "1024-bytes", "2048-dec"])
def test_mixed_batch(ctx, oracle, n_bits, y_bits, form, device):
    sd, pd = mixed(n_bits, y_bits, form)
    want_s, want_v = expected(oracle, sd, pd, n_bits, y_bits, form)
    assert {OK, INVALID, HOST} == set(want_s) and {ACCEPT, REJECT, MALFORMED} == set(want_v)
    for B in (130, 65):
        assert run(ctx, sd[:B], pd[:B], n_bits, y_bits, form, device) == (want_s[:B], want_v[:B])
    # equal to the flags-0 readers plus zkp_dlog_verify_batch on the pairs inside the domain
    kw, yw = n_bits // 32, y_bits // 32
    N_, g_, ni_, x_ = (np.zeros((130, kw), np.uint32) for _ in range(4)); y_ = np.zeros((130, yw), np.uint32)
    s1, s2 = np.full(130, 9, np.uint8), np.full(130, 9, np.uint8)
    ctx.json_dlog_statement(sd, n_bits, form, N_, g_, ni_, s1)
    ctx.json_dlog_proof(pd, n_bits, y_bits, form, x_, y_, s2)
    ints = [L.limbs_to_ints(a) for a in (N_, g_, ni_, x_)]
    ok = np.array([a == OK and b == OK and in_domain((ints[0][k], ints[1][k], ints[2][k]), (ints[3][k],)) for k, (a, b) in enumerate(zip(s1, s2))])
    assert list(ok) == [s == OK for s in want_s]
    v = np.full(int(ok.sum()), 9, np.uint8)
    ctx.dlog_verify(n_bits, y_bits, len(v), *(np.ascontiguousarray(a[ok]) for a in (N_, g_, ni_, x_, y_)), v)
    assert list(v) == [w for w, s in zip(want_v, want_s) if s == OK]


def test_all_canonical_pairs_are_scanned_on_the_device(ctx):
    cls = classes(1024, 544)
    sd, pd = documents(cls[:11] * 6, D.BIGINT_DEC)
    st, v = ctx.dlog_verify_json(sd, pd, 1024, 544)
    assert list(st) == [c[3] for c in cls[:11]] * 6 and list(v) == [c[4] for c in cls[:11]] * 6
    assert ctx.last_json_scan() == (2 * 66, 0)
    ms = ctx.last_json_scan_ms()
    assert ms[3] > 0 and all(m >= 0 for m in ms)


def test_arguments(ctx):
    lib, EINVAL, P = ctx.lib, zkp.capi.ZKP_EINVAL, zkp.capi.ptr
    cls = classes(1024, 544)
    s, p = D.write(list(cls[0][1]), D.STATEMENT, 0), D.write(list(cls[0][2]), D.PROOF, 0)
    buf = C.create_string_buffer(s + p)
    so, sl, po, pl = (np.array([v], np.uint64) for v in (0, len(s), len(s), len(p)))
    st = np.full(1, 9, np.uint8); v = np.full(1, 9, np.uint8)
    args = lambda **k: [ctx.h, k.get("text", C.cast(buf, C.c_void_p)), k.get("so", P(so)), P(sl), k.get("po", P(po)), P(pl), k.get("B", 1), k.get("n_bits", 1024),
                        k.get("y_bits", 544), k.get("form", 0), k.get("st", P(st)), k.get("v", P(v)), k.get("flags", 0)]
    assert lib.zkp_dlog_verify_json_batch(*args(B=0)) == zkp.capi.ZKP_OK and st[0] == 9 and v[0] == 9
    for bad in (dict(text=None), dict(so=None), dict(po=None), dict(st=None), dict(v=None), dict(n_bits=1536), dict(y_bits=512), dict(y_bits=1056), dict(y_bits=550),
                dict(form=3), dict(B=(1 << 24) + 1), dict(flags=2)):
        assert lib.zkp_dlog_verify_json_batch(*args(**bad)) == EINVAL, bad
        assert lib.zkp_last_error_string(ctx.h), bad
        assert st[0] == 9 and v[0] == 9, bad
    assert lib.zkp_dlog_verify_json_batch(*args()) == zkp.capi.ZKP_OK and st[0] == OK and v[0] == ACCEPT
