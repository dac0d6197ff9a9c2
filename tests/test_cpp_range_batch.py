"""The host batch header (zk-paillier_amd/host/range_batch.hpp) as a program of its own, under the address and undefined-behaviour
sanitizers (tests/cpp/test_range_batch.cpp; no GPU, no library, nothing loaded into this process), at kw = 32, EF = 3, two proofs:

  response write / read   identity for an Open row, Mask rows with j = 1 and j = 2, an all-zero row and rows of 2^(32 kw) - 1 — through the
                          allocating read and through the one that fills storage that is already there (no BigInt changes its block)
  stale memory            a slab first filled with 0xFF: a Mask row stores zero limbs in w2 / r2 and its j, an Open row j = 0
  carry predicate         true for those rows; false for a negative field, one of 32 kw + 1 bits, a pair of 64 kw + 1 bits and a
                          row-count mismatch, each alone; "exactly EF" against "at least EF" rows
  ABI struct              the pointers land on the arrays, batch / error_factor / n_bits / n_stride as given, absent groups null
  columns                 N / NN / Z / explicit widths round-trip for B = 2; a secret column reads as zeros after its wipe"""
import os
import subprocess

import helpers as H

ROOT = H.ROOT


def test_range_batch_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "test_range_batch.cpp")
    exe = os.path.join(ROOT, "build", "test_range_batch")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "range_batch ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
