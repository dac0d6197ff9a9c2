"""zkp_correct_key_ni_prove_batch without a GPU: the three libraries — the throughput engine and the two secondary engines a small call is
forwarded to — are built from the same sources and all export it, and each refuses a null context with ZKP_EINVAL before it touches a
device.  The other argument checks need a context: tests/test_gpu_ck_prove.py."""
import ctypes as C
import os

import pytest

from helpers import ROOT, zkp

PKG = os.path.join(ROOT, "zk-paillier_amd")


@pytest.mark.parametrize("name", ["libzkp_hip.so", "libzkp_hip_lat.so", "libzkp_hip_mid.so"])
def test_exported_and_null_context_refused(name):
    zkp.load()
    lib = C.CDLL(os.path.join(PKG, name))
    fn = lib.zkp_correct_key_ni_prove_batch
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    buf = (C.c_uint32 * 512)()
    assert fn(None, 1024, 1, buf, buf, b"KZen", 4, buf, buf, None, 0) == zkp.capi.ZKP_EINVAL
    assert not any(buf)


def test_python_binding_declares_it():
    assert "zkp_correct_key_ni_prove_batch" in zkp.capi.EXPORTS and hasattr(zkp.Context, "correct_key_ni_prove")
