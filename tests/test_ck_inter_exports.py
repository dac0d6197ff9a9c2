"""The four calls of the interactive CorrectKey without a GPU: the three libraries — the throughput engine and the two secondary engines a
small call is forwarded to — are built from the same sources and all export them, and each refuses a null context with ZKP_EINVAL before it
touches a device or a byte.  The other argument checks need a context: tests/test_gpu_ck_inter.py."""
import ctypes as C
import os

import pytest

from helpers import ROOT, zkp

PKG = os.path.join(ROOT, "zk-paillier_amd")
CALLS = {"zkp_correct_key_challenge_batch": "correct_key_challenge", "zkp_correct_key_challenge_seeded_batch": "correct_key_challenge_seeded",
         "zkp_correct_key_prove_batch": "correct_key_prove", "zkp_correct_key_verify_seeded_batch": "correct_key_verify_seeded"}


@pytest.mark.parametrize("name", ["libzkp_hip.so", "libzkp_hip_lat.so", "libzkp_hip_mid.so"])
def test_exported_and_null_context_refused(name):
    zkp.load()
    lib = C.CDLL(os.path.join(PKG, name))
    buf = (C.c_uint32 * 512)()
    seed = bytes(32)
    args = {"zkp_correct_key_challenge_batch": (None, 1024, 1, 3, buf, 0, buf, buf, buf, buf, buf, buf, None, 0),
            "zkp_correct_key_challenge_seeded_batch": (None, 1024, 1, 3, buf, 0, seed, 0, buf, buf, buf, buf, None, 0),
            "zkp_correct_key_prove_batch": (None, 1024, 1, 3, buf, buf, buf, buf, buf, buf, None, 0),
            "zkp_correct_key_verify_seeded_batch": (None, 1024, 1, 3, buf, 0, seed, 0, buf, buf, 0)}
    for call in CALLS:
        fn = getattr(lib, call)
        fn.restype, fn.argtypes = zkp.capi.EXPORTS[call]
        assert fn(*args[call]) == zkp.capi.ZKP_EINVAL, call
    assert not any(buf)


def test_python_binding_declares_them():
    for call, method in CALLS.items():
        assert call in zkp.capi.EXPORTS and hasattr(zkp.Context, method)
    assert zkp.capi.SEEDED_KIND_CORRECT_KEY == 10 and zkp.capi.CORRECT_KEY_ROUNDS == 40 and zkp.capi.CK_PROVE_BAD_KEY == 5
