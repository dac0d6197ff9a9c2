"""The host API of batched NiCorrectKeyProof proving (zk-paillier_amd/host/zkproofs.hpp: NiCorrectKeyProof::proof_batch):
tests/cpp/test_ck_prove_batch.cpp compiles and links against the built library without a GPU, and runs on one — proof_batch over three keys
equals three proof() calls, each result verifies, a malformed key panics with its index."""
import os
import subprocess

import pytest

import helpers as H

ROOT = H.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "test_ck_prove_batch.cpp")
EXE = os.path.join(ROOT, "build", "test_ck_prove_batch")


def _build(extra=()):
    H.zkp.load()
    pkg = os.path.join(ROOT, "zk-paillier_amd")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-pthread", SRC, "-o", EXE, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_ck_prove_batch_test_compiles_and_links():
    _build(["-Werror"])


@pytest.mark.gpu
def test_cpp_proof_batch_equals_proofs_and_verifies():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 2 and "FAIL" not in out.stdout, out.stdout + out.stderr
