"""The inputs of tests/test_gpu_seeded_nonces.py — a plain module, so that tests/test_seeded_nonce_model.py (CPU) can assert on the model
what the GPU cases rely on: that the bounds n = 5 and n = 2^1023 + 1155 really send the sampler through a rejected attempt.

The sampler reads n only as a bound, so the "keys" of the sampler cases need not be Paillier keys."""
import functools
import hashlib

import numpy as np

import helpers as H
import seeded_nonce_model as M
from helpers import L

SEED = hashlib.sha256(b"seeded-nonce-tests").digest()
BIG = (1 << 32) + 7
N_HALF = (1 << 1023) + 1155          # 1024 bits: about half of all attempts are rejected, and the deciding limb is the lowest or the highest
FIELD_NAMES = {M.KIND_ZERO: ("r_prime", None, None, None), M.KIND_CIPHERTEXT: ("x_prime", "r_prime", None, None),
               M.KIND_CORRECT_MESSAGE: ("r", "w", "e_sim", "z_sim"), M.KIND_DLOG: ("r", None, None, None)}


def _bound(tag, bits):
    return H.pm.Drbg(b"seeded-nonce-" + tag).bits(bits) | (1 << (bits - 1)) | 1


def sampler_cases():
    """name -> dict(kind, n_bits, n_list (one = shared), B, K, first_index, device)"""
    k1024 = H.test_key(1024)[2]
    fix = H.fixture_key()[2]
    c = {
        # per-proof bounds in one block of 5 x 2 lanes: a key, 5, 0 in the MIDDLE, 2^1023 + 1155, 1019 bits (a masked top limb)
        "zero-1024-perkey-B5-host": dict(kind=M.KIND_ZERO, n_bits=1024, n_list=[k1024, 5, 0, N_HALF, (k1024 >> 5) | 1], first_index=BIG, device=False),
        "ciphertext-2048-shared-B3-device": dict(kind=M.KIND_CIPHERTEXT, n_bits=2048, n_list=[fix], B=3, first_index=0, device=True),
        # a 2048-bit-wide call: 501 bits (one block, lanes 1 .. 3 idle), 2^2040 + 1 (2041 bits), 5
        "ciphertext-2048-perkey-B3-host": dict(kind=M.KIND_CIPHERTEXT, n_bits=2048, n_list=[(1 << 500) + 1, (1 << 2040) + 1, 5], first_index=BIG, device=False),
        "message-1024-K5-perkey-B3-device": dict(kind=M.KIND_CORRECT_MESSAGE, n_bits=1024, n_list=[k1024, 0, N_HALF], K=5, first_index=BIG, device=True),
        "message-2048-K2-shared-B5-host": dict(kind=M.KIND_CORRECT_MESSAGE, n_bits=2048, n_list=[fix], B=5, K=2, first_index=3, device=False),
        "message-1024-K2-perkey-B3-host": dict(kind=M.KIND_CORRECT_MESSAGE, n_bits=1024, n_list=[5, N_HALF, _bound(b"m", 999)], K=2, first_index=0, device=False),
        "message-4096-K1-shared-B3-host": dict(kind=M.KIND_CORRECT_MESSAGE, n_bits=4096, n_list=[_bound(b"k1", 4096)], B=3, K=1, first_index=0, device=False),
        # 8 lanes per value: 4090 bits, 5, 2^4000 + 1 (lane 7 holds the deciding limb or nothing)
        "zero-4096-perkey-B3-device": dict(kind=M.KIND_ZERO, n_bits=4096, n_list=[_bound(b"z", 4090), 5, (1 << 4000) + 1], first_index=BIG, device=True),
        "dlog-B5-device": dict(kind=M.KIND_DLOG, n_bits=2048, n_list=[], B=5, first_index=BIG, device=True),
        "dlog-B3-host": dict(kind=M.KIND_DLOG, n_bits=1024, n_list=[], B=3, first_index=0, device=False),
    }
    for v in c.values():
        v.setdefault("B", len(v["n_list"]))
        v.setdefault("K", 1)
    return c


@functools.lru_cache(maxsize=None)
def model_nonces(name):
    c = sampler_cases()[name]
    return M.nonces(c["kind"], SEED, c["first_index"], c["n_list"], c["B"], c["K"])


def field_arrays(kind, nonces, kw, K):
    """the model's nonces of a batch -> the four arrays by field id (None where the kind has none): uint32 limbs in the shapes of the C ABI"""
    out = []
    for f, name in enumerate(FIELD_NAMES[kind]):
        if name is None:
            out.append(None)
        elif name in ("e_sim", "z_sim"):
            w = 8 if name == "e_sim" else kw
            out.append(np.stack([L.ints_to_limbs(d[name], w) if K > 1 else np.zeros((0, w), np.uint32) for d in nonces]))
        else:
            out.append(L.ints_to_limbs([d[name] for d in nonces], 16 if kind == M.KIND_DLOG else kw))
    return out
