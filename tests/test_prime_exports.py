"""zkp_probable_prime_batch, zkp_next_prime_batch and zkp_paillier_keygen_seeded_batch without a GPU: the three libraries are built from
the same sources and all export them, and each refuses a null context with ZKP_EINVAL before it touches a device or a buffer.  The other
argument checks need a context: tests/test_gpu_prime.py."""
import ctypes as C
import os

import pytest

from helpers import ROOT, zkp

PKG = os.path.join(ROOT, "zk-paillier_amd")
NAMES = ("zkp_probable_prime_batch", "zkp_next_prime_batch", "zkp_paillier_keygen_seeded_batch")


@pytest.mark.parametrize("name", ["libzkp_hip.so", "libzkp_hip_lat.so", "libzkp_hip_mid.so"])
def test_exported_and_null_context_refused(name):
    zkp.load()
    lib = C.CDLL(os.path.join(PKG, name))
    for fn_name in NAMES:
        fn = getattr(lib, fn_name)
        fn.restype, fn.argtypes = zkp.capi.EXPORTS[fn_name]
    buf = (C.c_uint32 * 512)()
    A = C.addressof(buf)
    seed = bytes(range(32))
    assert lib.zkp_probable_prime_batch(None, 512, 1, A, 5, seed, 0, A, 0) == zkp.capi.ZKP_EINVAL
    assert lib.zkp_next_prime_batch(None, 512, 1, A, 5, seed, 0, A, A, A, 0) == zkp.capi.ZKP_EINVAL
    assert lib.zkp_paillier_keygen_seeded_batch(None, 1024, 1, 5, seed, 0, A, A, A, A, 0) == zkp.capi.ZKP_EINVAL
    assert not any(buf)


def test_python_binding_declares_them():
    assert all(n in zkp.capi.EXPORTS for n in NAMES)
    assert all(hasattr(zkp.Context, m) for m in ("probable_prime", "next_prime", "paillier_keygen_seeded"))
    header = open(os.path.join(ROOT, "include", "zkp_hip.h")).read()
    assert "#define ZKP_SEEDED_KIND_KEYGEN 9u" in header
