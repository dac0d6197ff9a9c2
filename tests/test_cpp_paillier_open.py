"""The host API of Paillier decryption (zk-paillier_amd/host/zkproofs.hpp: Paillier::open, decrypt, verify_opening, open_batch, decrypt_batch):
tests/cpp/test_paillier_open.cpp compiles and links against the built library without a GPU, and runs on one — the port of the reference's
test of verify_opening (correct_opening.rs:48-56), decrypt_batch of 17 ciphertexts, the Panic of a one-item open on c = 0."""
import os
import subprocess

import pytest

import helpers as H

ROOT = H.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "test_paillier_open.cpp")
EXE = os.path.join(ROOT, "build", "test_paillier_open")


def _build(extra=()):
    H.zkp.load()
    pkg = os.path.join(ROOT, "zk-paillier_amd")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-pthread", SRC, "-o", EXE, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_paillier_open_test_compiles_and_links():
    _build(["-Werror"])


@pytest.mark.gpu
def test_cpp_open_decrypt_and_verify_opening():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 3 and "FAIL" not in out.stdout, out.stdout + out.stderr
