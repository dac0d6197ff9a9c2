"""GPU tests of zkp_paillier_open_batch (csrc/kernels_paillier_dec.hpp) on the crafted list of tests/paillier_dec_branch_cases.py: items that
take pd_mod — Knuth's algorithm D — through its add-back, its estimates of 2^32 and more, its rh break and its second loop turn at every
call site (key preparation, the split by F^2 and by F, the finish's L h mod F, both reductions of both recombinations), at quotient positions
from the top step to 0, under shifts 0 .. 31 and divisor lengths on and off the 8-word chunks.  Everything is exactly equal to
tests/paillier_dec_model.py (Python integers); tests/test_paillier_dec_branch_model.py certifies on the CPU which branch each item takes
where, and that the item would expose the branch's defect.  Through the session `ctx` fixture: every engine runs the ladder once."""
import numpy as np
import pytest

import ck_prove_model as CM
import helpers as H
import paillier_dec_branch_cases as BC
import paillier_dec_cases as PC
from ck_prove_cases import SALTS
from helpers import L

pytestmark = pytest.mark.gpu


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def run_open(ctx, b, with_r=True, device=False):
    """-> [(m, r | None, status)]"""
    n_bits, B = b["n_bits"], len(b["c"])
    hw, kw = n_bits // 64, n_bits // 32
    shared = len(b["keys"]) == 1
    p, q = L.ints_to_limbs([k[0] for k in b["keys"]], hw), L.ints_to_limbs([k[1] for k in b["keys"]], hw)
    c = L.ints_to_limbs(b["c"], 2 * kw)
    m, r, st = np.full((B, kw), 9, np.uint32), np.full((B, kw), 9, np.uint32), np.full(B, 9, np.uint8)
    if device:
        import torch
        dp, dq, dc, dm, dr, dst = (to_dev(a) for a in (p, q, c, m, r, st))
        torch.cuda.synchronize()
        ctx.paillier_open(n_bits, B, dp, dq, 0 if shared else hw, dc, dm, dr if with_r else None, dst, device=True)
        ctx.synchronize()
        m, r, st = dm.cpu().numpy().view(np.uint32), dr.cpu().numpy().view(np.uint32), dst.cpu().numpy()
    else:
        ctx.paillier_open(n_bits, B, p, q, 0 if shared else hw, c, m, r if with_r else None, st)
    return [(L.limbs_to_int(m[i]), L.limbs_to_int(r[i]) if with_r else None, int(st[i])) for i in range(B)]


def assert_same(got, b, with_r=True):
    want = b["want"] if with_r else [(m, None, s) for m, _, s in b["want"]]
    bad = [(i, b["tag"][i], b["claims"].get(i), got[i][2], want[i][2]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:4]


@pytest.mark.parametrize("name", ["split 0", "split 1", "finish 0", "crt 0", "crt 1", "keys 0"])
def test_crafted_list_1024(ctx, name):
    """one key per item; with roots and without, on host pointers and on device pointers"""
    b = dict(BC.list_1024())[name]
    assert b["crafted"] and len(b["keys"]) == len(b["c"])
    for with_r in (True, False):
        for device in (False, True):
            got = run_open(ctx, b, with_r=with_r, device=device)
            assert_same(got, b, with_r=with_r)
    bad = [i for i, w in enumerate(b["want"]) if w[2] == 2]
    assert len(bad) == (1 if name == "keys 0" else 0)
    assert all(got[i] == (0, None, 2) for i in bad)              # status 2 and zero outputs exactly where the model says
    assert [g[0] for i, g in enumerate(got) if b["truth"][i]] == [t[0] for t in b["truth"] if t]


def test_shared_key_forward_and_reversed(ctx):
    """key_stride 0: the items of every site that needs no special key; reversed, each crafted lane sits elsewhere in its 16-lane block"""
    b = BC.shared_1024()
    assert_same(run_open(ctx, b), b)
    r = BC.reversed_batch(b)
    assert_same(run_open(ctx, r), r)
    assert_same(run_open(ctx, r, with_r=False, device=True), r, with_r=False)
    per_item = dict(BC.list_1024())["split 0"]
    r = BC.reversed_batch(per_item)
    assert_same(run_open(ctx, r), r)


@pytest.mark.parametrize("n_bits", [2048, 4096])
def test_wide_repeats(ctx, n_bits):
    """hw = 32: every site's add-back, one key per item; hw = 64: the split, the finish and the recombination under the benchmark's key"""
    b = BC.wide(n_bits)
    assert len(b["c"]) <= (27 if n_bits == 2048 else 7)
    got = run_open(ctx, b)
    assert_same(got, b)
    assert all(g[2] == 0 for g in got)


def test_secrets_are_wiped_after_a_crafted_batch(ctx):
    b = dict(BC.list_1024())["keys 0"]
    assert sum(w[2] == 2 for w in b["want"]) == 1
    assert_same(run_open(ctx, b), b)
    assert ctx.witness_residue() == 0


def test_keys_with_add_backs_in_correct_key_prove(ctx):
    """key preparation is shared with zkp_correct_key_ni_prove_batch: the keys whose rows take the add-back (composite factors, inverses
    exist; and the two with prime factors) beside ordinary ones, against tests/ck_prove_model.py — and one bad key among them"""
    good = [H.test_key(1024, t)[:2] for t in range(3)]
    odd = BC.composite_factor_keys() + sorted(BC.prime_keys_with_add_back(16).items()) + [("add-back key", PC.ADD_BACK_KEY)]
    keys = []
    for i, (_, k) in enumerate(odd):
        keys += [good[i % 3], k]
    keys += [(good[0][0], good[0][0]), good[1]]                 # p = q: status 2
    B, hw, kw = len(keys), 16, 32
    p, q = L.ints_to_limbs([k[0] for k in keys], hw), L.ints_to_limbs([k[1] for k in keys], hw)
    n, sg, st = np.full((B, kw), 9, np.uint32), np.full((B, 11, kw), 9, np.uint32), np.full(B, 9, np.uint8)
    ctx.correct_key_ni_prove(1024, B, p, q, SALTS[0], n, sg, st)
    got = [(L.limbs_to_int(n[b]), L.limbs_to_ints(sg[b]), int(st[b])) for b in range(B)]
    want = [CM.prove(a, b, SALTS[0]) for a, b in keys]
    assert [w[2] for w in want] == [0] * (B - 2) + [2, 0]
    bad = [i for i in range(B) if got[i] != want[i]]
    assert not bad, bad
