"""zkp_modinv_batch on the GPU in every finalisation class of k_modinv that the search of tests/golden/make_modinv_classes.py reached —
the cofactor in range, negative, and below -M (two passes of the loop that a single conditional add once stood for) — with the per-round
events (a negated, b negated, a sign word carrying magnitude, the step into the n <= 64 branch) and the lanes of different trip counts
that share a block with them.  The vectors, the batches and their layout are tests/modinv_class_cases.py;
tests/test_modinv_class_cases.py holds them to the model of the kernel on the CPU.  Nothing here reached v >= M: the subtract branch is
NOT covered.

Context: one context of this module's own, not the five-fold `ctx` fixture.  zkp_modinv_batch stages its buffers and calls launch_modinv,
which launches k_modinv with blocks of 16 lanes whatever the context's geometry, Enc form or ladder setting is: no kernel family changes
its path, and four more runs would repeat this one."""
import numpy as np
import pytest

import modinv_class_cases as MC
import small_proof_cases as SC
from helpers import L, zkp


@pytest.fixture(scope="module")
def own_ctx():
    c = zkp.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mod_bits", MC.WIDTHS)
def test_gpu_modinv_in_every_class(own_ctx, oracle, mod_bits):
    """status and every output word against the C oracle (mpz_invert) and against pow(a, -1, M); outputs pre-filled with sentinels;
    items without an inverse and out-of-domain items come back as zeros.  Batches: per-item moduli, 71 items (a partial last block);
    75 items with the rare vectors in the last, partial block; at 8192 bits 39 items under one shared modulus (mod_stride = 0) with
    below_neg_m values in its first and in its partial last block."""
    bs = MC.batches(mod_bits)
    assert set(bs) == {"per_item", "rare_last"} | ({"shared"} if mod_bits == 8192 else set())
    for name, (items, stride) in bs.items():
        assert not MC.placement_problems(items, shared=stride == 0), name
        assert len(items) > 64 or stride == 0
        assert len(items) % MC.BLOCK and len(items) <= 104
        a, m, inv, st = MC.arrays(items, mod_bits, stride)
        oo, so = oracle.modinv(mod_bits, a, m, stride)
        SC.assert_same(st, so, name + ": oracle status against Python")
        SC.assert_same(inv, oo, name + ": oracle inverse against pow(a, -1, M)")
        og, sg = SC.sentinel(a.shape), SC.sentinel(len(items), np.uint8)
        own_ctx.modinv(mod_bits, len(items), a, m, stride, og, sg)
        SC.assert_same(st, sg, name + ": status")
        SC.assert_same(inv, og, name + ": inverse")
        for i, it in enumerate(items):
            if it["status"] == zkp.INV_OK:
                assert L.limbs_to_int(og[i]) * it["a"] % it["M"] == 1, (name, i)
            else:
                assert not og[i].any(), (name, i)
