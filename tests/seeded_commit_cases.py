"""Shapes and tamper lists of the verifier's seeded commitment (include/zkp_hip.h: zkp_range_verifier_commit_seeded_batch and its two
neighbours) — a plain module: tests/test_seeded_commit_model.py checks the conditions it promises, tests/test_gpu_seeded_commit.py runs the
GPU on the shapes.

Keys are odd integers drawn by the repository's DRBG, not products of two primes: Enc and sample_below read n as a number, and a session
of this protocol step never decrypts.  Three shapes per width:
    full    bit_length(n) == n_bits
    narrow  bit_length(n) == n_bits - 45: not a multiple of 32, so the mask of the sampler's top limb matters
    pow2    n = 2^(n_bits - 24) + a (n_bits - 32)-bit number: just above a power of two, about half the attempts are rejected"""
import functools

import numpy as np

import helpers as H
import seeded_commit_model as M
from helpers import L

SEED = bytes(range(7, 39))
BIG = (1 << 32) + 11           # an index whose high word is not zero
KEY_SHAPES = ("full", "narrow", "pow2")


def key(n_bits, shape, tag=0):
    d = H.pm.Drbg(b"commit-key-%d-%s-%d" % (n_bits, shape.encode(), tag))
    if shape == "full":
        return d.bits(n_bits) | (1 << (n_bits - 1)) | 1
    if shape == "narrow":
        return d.bits(n_bits - 45) | (1 << (n_bits - 46)) | 1
    assert shape == "pow2"
    return (1 << (n_bits - 24)) + (d.bits(n_bits - 32) | 1)


def _leading_zero_index(e_len, start):
    """the first index >= start whose SHA256(e) begins with a 00 byte"""
    i = start
    while M.digest_int(M.challenge_bytes(SEED, i, e_len)) >> 248:
        i += 1
    return i


ZERO_DIGEST_INDEX = _leading_zero_index(5, BIG)

# id -> (n_bits, key shape, one key for the batch, e_len, B, first_index).  Every width with every key shape, both key modes, every e_len of
# {1, 5, 31, 32} and every B of {1, 4, 70, 300}: one item (the latency path), a small group, more than one block of the sampler at every
# width (256 / G sessions per block, G = n_bits / 512), the throughput engine.  4096-bit shapes stop at 70 sessions.
SHAPES = {
    "1024-full-shared-e5-B1": (1024, "full", True, 5, 1, 0),
    "1024-narrow-perkey-e1-B4": (1024, "narrow", False, 1, 4, BIG),
    "1024-pow2-shared-e31-B70": (1024, "pow2", True, 31, 70, 3),
    "1024-full-perkey-e32-B300": (1024, "full", False, 32, 300, BIG),
    "2048-full-shared-e5-B300": (2048, "full", True, 5, 300, BIG),
    "2048-narrow-perkey-e32-B70": (2048, "narrow", False, 32, 70, 1),
    "2048-pow2-perkey-e5-B4": (2048, "pow2", False, 5, 4, ZERO_DIGEST_INDEX - 1),      # session 1: SHA256(e) begins with 00
    "2048-pow2-shared-e31-B1": (2048, "pow2", True, 31, 1, BIG),
    "4096-full-shared-e32-B4": (4096, "full", True, 32, 4, BIG),
    "4096-narrow-perkey-e5-B70": (4096, "narrow", False, 5, 70, 2),
    "4096-pow2-shared-e1-B1": (4096, "pow2", True, 1, 1, BIG),
}
ZERO_DIGEST_SHAPE, ZERO_DIGEST_SESSION = "2048-pow2-perkey-e5-B4", 1
# the shapes the pinned engines of the `ctx` fixture run (every key shape, every width, both key modes) and the ones verify_commit is tampered on
PINNED_SHAPES = ("1024-narrow-perkey-e1-B4", "2048-pow2-perkey-e5-B4", "4096-full-shared-e32-B4")
VERIFY_SHAPES = ("1024-narrow-perkey-e1-B4", "2048-pow2-perkey-e5-B4", "2048-full-shared-e5-B300", "2048-narrow-perkey-e32-B70", "4096-full-shared-e32-B4")
TAMPERS = ("com+1", "com=0", "com+nn", "r+1", "e-bit", "e_len-1")


def keys_of(name):
    n_bits, shape, shared, _, B, _ = SHAPES[name]
    return [key(n_bits, shape, t) for t in range(1 if shared else B)]


@functools.lru_cache(maxsize=None)
def model(name):
    """-> (keys, the model's sessions without com)"""
    n_bits, shape, shared, e_len, B, first = SHAPES[name]
    keys = keys_of(name)
    return keys, M.sessions(SEED, first, keys, B, e_len, with_com=False)


def key_limbs(keys, n_bits):
    return L.ints_to_limbs(keys, n_bits // 32)


def e_rows(es):
    """byte strings -> ([B][32] left aligned, [B] lengths)"""
    out = np.zeros((len(es), 32), np.uint8)
    for b, e in enumerate(es):
        out[b, :len(e)] = np.frombuffer(bytes(e), np.uint8)
    return out, np.array([len(e) for e in es], np.uint8)


def tampered(n_bits, n, com, r, e):
    """the tampered copies of one accepted session -> list of (tamper, com, r, e); com + n^2 only where it fits in 2 n_bits bits"""
    out = [("com+1", com + 1, r, e), ("com=0", 0, r, e)]
    if com + n * n < 1 << (2 * n_bits):
        out.append(("com+nn", com + n * n, r, e))
    out.append(("r+1", com, r + 1, e))
    flipped = bytearray(e)
    flipped[len(e) // 2] ^= 0x10
    out += [("e-bit", com, r, bytes(flipped)), ("e_len-1", com, r, e[:-1])]
    return out
