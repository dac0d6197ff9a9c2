"""The inputs of tests/test_gpu_seeded_prove.py's sampler cases — a plain module, so that tests/test_seeded_model.py (CPU) can assert that
they really exercise the rejection path of sample_below and stay far from its 128-attempt cap.

The sampler reads n only as a bound, so the per-proof "keys" of these cases need not be Paillier keys: 2^k + 1 as a bound rejects about
half of all attempts, a bit length that is no multiple of 32 exercises the top-limb mask."""
import functools
import hashlib

import helpers as H
import seeded_model as M

SEED = hashlib.sha256(b"seeded-prove-tests").digest()


def _rng(tag, bits):
    return H.pm.Drbg(b"seeded-range-" + tag).bits(bits) | (1 << (bits - 1))


def sampler_cases():
    """name -> dict(n_bits, n_list (one = shared), ranges, ef, first_index, device)"""
    n1024 = H.test_key(1024)[2]
    fix = H.fixture_key()[2]
    return {
        # a 256-bit range, range 2 (an empty interval) in the MIDDLE of the batch, 250 bits, third = 2^200 + 1
        "n1024-shared-ef40-host": dict(n_bits=1024, n_list=[n1024], ranges=[_rng(b"a0", 256), 2, _rng(b"a2", 250), 3 * ((1 << 200) + 1)], ef=40,
                                       first_index=5, device=False),
        # per-proof bounds: the fixture key, 2^2040 + 1 (2041 bits: masked top limb, half the attempts rejected), a 2043-bit odd number
        "n2048-perkey-ef128-device": dict(n_bits=2048, n_list=[fix, (1 << 2040) + 1, (fix >> 5) | 1],
                                          ranges=[3 * ((1 << 255) + 1), _rng(b"b1", 256), 3 * ((1 << 64) + 1) + 2], ef=128, first_index=(1 << 32) + 7, device=True),
        # third = 2^256 + 1: 257 bits, nine words
        "n2048-shared-ef256-host": dict(n_bits=2048, n_list=[fix], ranges=[_rng(b"c0", 256), 3 * ((1 << 256) + 1) + 1], ef=256, first_index=0, device=False),
        "n1024-perkey-ef128-device": dict(n_bits=1024, n_list=[H.test_key(1024, tag=0)[2], (1 << 1000) + 1], ranges=[_rng(b"d0", 256), _rng(b"d1", 250)], ef=128,
                                          first_index=0, device=True),
    }


@functools.lru_cache(maxsize=None)
def model_witness(name):
    c = sampler_cases()[name]
    return M.witness(SEED, c["first_index"], c["n_list"], c["ranges"], c["ef"])
