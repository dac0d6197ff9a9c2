"""The sigma proofs' verify_json_batch of the C++ host mirror (zk-paillier_amd/host/zkproofs.hpp): tests/cpp/test_verify_json_sigma.cpp must compile
and link on any machine (CPU test) and pass on the GPU (-m gpu)."""
import os
import subprocess

import pytest

import helpers as H

ROOT = H.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "test_verify_json_sigma.cpp")
EXE = os.path.join(ROOT, "build", "test_verify_json_sigma")
PKG = os.path.join(ROOT, "zk-paillier_amd")


def build_exe():
    if not os.path.exists(H.zkp.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC] + [os.path.join(PKG, "host", h) for h in ("zkproofs.hpp", "bigint.hpp", "staging.hpp")] + [H.zkp.LIB_PATH]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", SRC, "-o", EXE, "-L" + PKG, "-lzkp_hip",
                               "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_verify_json_sigma_compiles_and_links():
    build_exe()


@pytest.mark.gpu
def test_cpp_verify_json_sigma_batch():
    exe = build_exe()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 5 and "FAIL" not in out.stdout, out.stdout + out.stderr
