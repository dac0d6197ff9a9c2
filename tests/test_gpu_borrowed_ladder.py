"""A call that runs the ladder under SECRET moduli (csrc/zkp_api_paillier_dec.inc: SecretLadder) lends the ctx two blocks of its own for
the constants records and the window tables and takes them back when the launch is enqueued: the ctx's own buffers — the cached record of
a key among them (tests/test_gpu_key_cache.py) — are as they were.  Here a one-key Paillier Enc call caches its key's record, each of the
five calls that borrow runs once at its smallest shape of at least two ladder rows, and afterwards the key-cache diagnostic reads the same,
the same Enc call finds its record (no set-up is computed) and returns the same ciphertexts, and nothing is left in the call's blocks.

Everything is 1024-bit, so every ladder row is a zero-padded one and the Enc (n^2 of 2048 bits) uses the lane group of the ladder: the
borrowed buffers are the very ones its record lives in.  The ctx is pinned to the throughput engine: the diagnostic of a ctx whose last
call went to a secondary engine is that engine's twin's, while the prime calls always run on the ctx that receives them."""
import random

import numpy as np
import pytest

import ck_inter_cases as CI
import ck_inter_model as CIM
import ck_prove_cases as CK
import helpers as H
import paillier_dec_cases as PD
import prime_cases as PR
from helpers import L, zkp

pytestmark = pytest.mark.gpu

N_BITS, HW, KW = 1024, 16, 32
ENC_COUNT = 3


@pytest.fixture(scope="module")
def lctx():
    c = zkp.Context(0)
    c.set_geometry(zkp.load().zkp_build_limbs_per_lane())
    c.set_enc_form("n2")             # the n^2-sized kernels: their one record is in the buffer the ladder borrows (diagnostic 0)
    c.set_key_cache(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def enc_case():
    """(n, m, r as limbs, the ciphertexts of the model) of the one Enc call"""
    n = H.test_key(N_BITS, 2)[2]
    ms, rs = [11 + i for i in range(ENC_COUNT)], [(5 + i) | (0x89ABCDE << (32 * 20)) for i in range(ENC_COUNT)]
    return n, L.ints_to_limbs(ms, KW), L.ints_to_limbs(rs, KW), [H.python_enc(n, m, r) for m, r in zip(ms, rs)]


def enc(c, enc_case):
    n, m, r, _ = enc_case
    out = np.zeros((ENC_COUNT, 2 * KW), np.uint32)
    c.paillier_enc(N_BITS, ENC_COUNT, L.int_to_limbs(n, KW), 0, m, r, out)
    return L.limbs_to_ints(out)


def diagnostic(c):
    return [c.key_cache_state(which) for which in range(4)]


def call_open(c):
    """count = 1 with roots: 4 rows"""
    b = PD.one_key(N_BITS)
    (p, q), m, r, st = b["keys"][0], np.full((1, KW), 9, np.uint32), np.full((1, KW), 9, np.uint32), np.full(1, 9, np.uint8)
    c.paillier_open(N_BITS, 1, L.ints_to_limbs([p], HW), L.ints_to_limbs([q], HW), 0, L.ints_to_limbs(b["c"][:1], 2 * KW), m, r, st)
    assert (L.limbs_to_int(m[0]), L.limbs_to_int(r[0]), int(st[0])) == b["want"][0]


def call_ni_prove(c):
    """batch = 1: 22 rows"""
    b, salt = CK.one_1024(), CK.SALTS[0]
    (p, q), n, sg, st = b["keys"][0], np.full((1, KW), 9, np.uint32), np.full((1, 11, KW), 9, np.uint32), np.full(1, 9, np.uint8)
    c.correct_key_ni_prove(N_BITS, 1, L.ints_to_limbs([p], HW), L.ints_to_limbs([q], HW), salt, n, sg, st)
    assert (L.limbs_to_int(n[0]), L.limbs_to_ints(sg[0]), int(st[0])) == b["want"][salt][0]


def call_prove(c):
    """batch = 1, K = 1: 6 rows"""
    p, q = H.test_key(N_BITS, 0)[:2]
    sn, e, z = CI.honest(random.Random(1), p, q, 1)
    sd, err = np.full((1, 8), 9, np.uint32), np.full(1, 9, np.uint8)
    c.correct_key_prove(N_BITS, 1, 1, L.ints_to_limbs([p], HW), L.ints_to_limbs([q], HW), L.ints_to_limbs(sn, KW).reshape(1, 1, KW), L.ints_to_limbs([e], 8),
                        L.ints_to_limbs(z, KW).reshape(1, 1, KW), sd, err)
    want = CIM.prove(p, q, sn, e, z)
    assert want[0] == 0 and (int(err[0]), L.limbs_to_int(sd[0])) == want


def call_next_prime(c):
    """count = 1, 512 bits: a round is never less than two rows"""
    starts, names, want = PR.next_batch()
    i = names.index("ordinary")
    p, off, st = np.full((1, 16), 9, np.uint32), np.full(1, 9, np.uint32), np.full(1, 9, np.uint8)
    c.next_prime(512, 1, L.ints_to_limbs([starts[i]], 16), PR.ROUNDS, PR.SEED, PR.FIRST_INDEX + i, p, off, st)
    assert (L.limbs_to_int(p[0]), int(off[0]), int(st[0])) == want[i]


def call_keygen(c):
    """batch = 1: two slots"""
    want = PR.keygen_want(N_BITS, 1)[0]
    p, q, n, st = np.full((1, HW), 9, np.uint32), np.full((1, HW), 9, np.uint32), np.full((1, KW), 9, np.uint32), np.full(1, 9, np.uint8)
    c.paillier_keygen_seeded(N_BITS, 1, PR.ROUNDS, PR.SEED, PR.KEYGEN_FIRST_INDEX[N_BITS], p, q, n, st)
    assert (L.limbs_to_int(p[0]), L.limbs_to_int(q[0]), L.limbs_to_int(n[0]), int(st[0])) == want[0]


CALLS = {"paillier_open": call_open, "correct_key_ni_prove": call_ni_prove, "correct_key_prove": call_prove, "next_prime": call_next_prime,
         "paillier_keygen_seeded": call_keygen}


@pytest.mark.parametrize("name", list(CALLS))
def test_the_ctx_buffers_are_as_they_were(lctx, enc_case, name):
    c = lctx
    assert enc(c, enc_case) == enc_case[3]
    before = diagnostic(c)
    assert before[0][0], "the Enc call's record is not in the buffer the ladder borrows: this test would show nothing"
    CALLS[name](c)
    assert c.witness_residue() == 0
    assert diagnostic(c) == before
    assert enc(c, enc_case) == enc_case[3]
    valid, hit, epoch = c.key_cache_state(0)
    assert (valid, hit, epoch) == (True, True, before[0][2]), "the key's record did not survive the call: the set-up was computed again"
