"""Sessions of the interactive RangeProof whose witness is the one a seed expands to (tests/seeded_model.py) — a plain module: the CPU test
tests/test_seeded_interactive_model.py pins these cases against the oracle and the Python model, tests/test_gpu_seeded_interactive.py holds
the two seeded prover steps of the GPU to them byte for byte.

A case is the list of dicts helpers.build_range_case returns (statement and secrets drawn by its DRBG), with w1 / w2 / r1 / r2 replaced by
seeded_model.witness(SEED, first_index, keys, ranges, ef): what zkp_range_generate_*_seeded_batch must use for (SEED, first_index + b)."""
import functools

import numpy as np

import helpers as H
import seeded_cases as SC
import seeded_model as M
from test_range_interactive import challenge, clone_inputs

SEED = SC.SEED
FIRST_INDEX = (1 << 32) + 7
WIT = ("w1", "w2", "r1", "r2")
OUT_FIELDS = ("c1", "c2", "resp_kind", "resp_j", "resp_w1", "resp_r1", "resp_w2", "resp_r2")
RESP_FIELDS = OUT_FIELDS[2:]
# (n_bits, key bits, error factor, one key for the batch)
SHAPES = [(1024, 512, 40, True), (1024, 1024, 129, False), (1024, 512, 1, True), (1024, 512, 256, True), (2048, 2048, 40, True)]
SHAPE_IDS = ["n%d-key%d-ef%d-%s" % (s[0], s[1], s[2], "shared" if s[3] else "perkey") for s in SHAPES]


def keys_for(key_bits, shared, B):
    if key_bits == 2048:
        return [H.fixture_key()[2]]
    return [H.test_key(key_bits, tag=i)[2] for i in range(1 if shared else B)]


@functools.lru_cache(maxsize=None)
def session_cases(n_bits, key_bits, ef, shared, B=4, first_index=FIRST_INDEX, dishonest=1):
    """B sessions, session `dishonest` (None: no session) with x far outside the range; the witness is the model's"""
    keys = keys_for(key_bits, shared, B)
    cases = H.build_range_case(b"seeded-inter-%d-%d-%d-%d" % (n_bits, key_bits, ef, B), keys, n_bits, B, shared=shared, ef=ef)
    if dishonest is not None:
        cases[dishonest] = H.build_range_case(b"seeded-inter-bad", [cases[dishonest]["n"]], n_bits, 1, honest=False, ef=ef)[0]
    wit, status, _, _ = M.witness(SEED, first_index, keys, [c["range"] for c in cases], ef)
    assert not any(status)
    for b, c in enumerate(cases):
        for f in WIT:
            c[f] = wit[f][b]
    return cases


def session_challenge(ef, B, short=()):
    """the verifier's challenge of a session batch: ceil(ef / 8) bytes, one fewer for the sessions in `short`"""
    return challenge(b"seeded-inter-chal-%d" % ef, B, ef, short=short)


def oracle_steps(oracle, po, wt, e, elen):
    """generate_encrypted_pairs and generate_proof of the oracle on (po, wt) -> status [B]"""
    st = np.full(po.batch, 9, np.uint8)
    oracle.range_generate_encrypted_pairs(po.struct(), wt.struct())
    oracle.range_generate_proof(po.struct(), wt.struct(), e, elen, st)
    return st


def prefill(pb, word=0xA5A5A5A5, byte=77):
    """stale content in every output array: a step must leave the other step's arrays exactly so"""
    for f in ("c1", "c2", "resp_w1", "resp_r1", "resp_w2", "resp_r2"):
        getattr(pb, f)[:] = word
    pb.resp_kind[:] = byte; pb.resp_j[:] = byte
    return pb


def fresh(po, fill=True):
    q = clone_inputs(po)
    return prefill(q) if fill else q
