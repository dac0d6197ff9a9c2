"""The host API of the batched interactive CorrectKey (zk-paillier_amd/host/zkproofs.hpp: CorrectKey::challenge_batch_seeded, prove_batch,
verify_batch_seeded): tests/cpp/test_ck_inter_batch.cpp compiles and links against the built library without a GPU, and runs on one —
prove_batch over three keys equals three prove() calls, the seeded round trip accepts, a ragged session takes the single-session path."""
import os
import subprocess

import pytest

import helpers as H

ROOT = H.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "test_ck_inter_batch.cpp")
EXE = os.path.join(ROOT, "build", "test_ck_inter_batch")


def _build(extra=()):
    H.zkp.load()
    pkg = os.path.join(ROOT, "zk-paillier_amd")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-pthread", SRC, "-o", EXE, "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_ck_inter_batch_test_compiles_and_links():
    _build(["-Werror"])


@pytest.mark.gpu
def test_cpp_prove_batch_round_trip_and_fallback():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.count("PASS") == 3 and "FAIL" not in out.stdout, out.stdout + out.stderr
