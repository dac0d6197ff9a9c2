"""The plain-C++ half of DLogStatement::generate_batch_seeded (zk-paillier_amd/host/range_batch.hpp: DLogSetupBatch) as a program of its
own, under the address and undefined-behaviour sanitizers (tests/cpp/test_dlog_setup_host.cpp; no GPU, no library, nothing loaded into this
process):

  width            the narrowest kernel width that takes the widest modulus of the batch; a negative modulus and one above 4096 bits refused
  flattening       every word of every [B][kw] row written (short moduli zero-extended), at kw = 32, 64 and 128
  status           the first failing statement is the one reported
  columns          g, ni and the secrets read back as written; the secret column alone reads as zeros after its wipe

and the GPU-side program of the host class (tests/cpp/test_dlog_setup.cpp) compiles and links against the built library; it RUNS in
tests/test_gpu_dlog_setup.py."""
import os
import subprocess

import helpers as H

ROOT = H.ROOT


def test_dlog_setup_host_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "test_dlog_setup_host.cpp")
    exe = os.path.join(ROOT, "build", "test_dlog_setup_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dlog_setup_host ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_cpp_dlog_setup_test_compiles_and_links():
    H.zkp.load()
    pkg = os.path.join(ROOT, "zk-paillier_amd")
    exe = os.path.join(ROOT, "build", "test_dlog_setup")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_dlog_setup.cpp"), "-o", exe,
                           "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
