"""The batch forms of the verifier's commitment of the interactive RangeProof in the C++ host mirror (zk-paillier_amd/host/zkproofs.hpp:
VerifierSeed, verifier_commit_batch_seeded, verifier_reveal_batch_seeded, verify_commit_batch): tests/cpp/test_range_commit_batch.cpp must
compile and link on any machine (CPU test) and pass on the GPU (-m gpu)."""
import os
import subprocess

import pytest

import helpers as H

ROOT = H.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "test_range_commit_batch.cpp")
EXE = os.path.join(ROOT, "build", "test_range_commit_batch")
PKG = os.path.join(ROOT, "zk-paillier_amd")


def build_exe():
    if not os.path.exists(H.zkp.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC] + [os.path.join(PKG, "host", h) for h in ("zkproofs.hpp", "range_batch.hpp", "bigint.hpp", "staging.hpp")] + [H.zkp.LIB_PATH]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", SRC, "-o", EXE, "-L" + PKG, "-lzkp_hip",
                               "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_range_commit_batch_compiles_and_links():
    build_exe()


@pytest.mark.gpu
def test_cpp_range_commit_batch():
    exe = build_exe()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 3 and "FAIL" not in out.stdout, out.stdout + out.stderr
