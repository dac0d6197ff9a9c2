"""CPU tests of the seeded RangeProofNi witness: the Python restatement of the stream (tests/seeded_model.py) against RFC 8439's own test
vector and against the ChaCha20 block function the C++ host layer already ships (host/bigint.hpp, written independently of the sampler
kernel), the properties the reference's sampling has (range_proof.rs:133-159), the new entry points in the built library, and the
statement that the inputs of the GPU tests exercise the retry path."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import seeded_cases as SC
import seeded_model as M

ROOT = H.ROOT
zkp = H.zkp


def test_block_function_against_rfc8439_section_2_3_2():
    # RFC 8439, 2.3.2: key 00 01 .. 1f, nonce 00 00 00 09 00 00 00 4a 00 00 00 00, block counter 1
    key = struct.unpack("<8I", bytes(range(32)))
    state = list(M.SIGMA) + list(key) + [1, 0x09000000, 0x4A000000, 0x00000000]
    want = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
            0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]
    assert M.block_words(state) == want
    # the serialised block begins 10 f1 e7 e4 d1 3b 59 15 (same section)
    assert struct.pack("<16I", *M.block_words(state))[:8] == bytes.fromhex("10f1e7e4d13b5915")


def test_state_layout_and_numpy_blocks_agree_with_the_scalar_ones():
    seed = bytes(range(32))
    index = (0x4A000000 << 32) | 0x09000000
    assert M.state_for(seed, 1, index, 0, 0) == list(M.SIGMA) + list(struct.unpack("<8I", seed)) + [1, 0x09000000, 0x4A000000, 0]
    assert M.state_for(seed, 7, 5, 255, 3)[12:] == [7, 5, 0, (255 << 2) | 3]
    got = M.blocks_np(SC.SEED, [0, 1, 9, 2 ** 32 - 1], (1 << 32) + 7, [0, 3, 200, 255], 2)
    for k, (ctr, row) in enumerate([(0, 0), (1, 3), (9, 200), (2 ** 32 - 1, 255)]):
        assert got[k].tolist() == M.block(SC.SEED, ctr, (1 << 32) + 7, row, 2)


def test_block_function_against_the_host_layers_chacha(tmp_path):
    """detail::ChaChaRng::block of host/bigint.hpp on a fixed state (next() hands the buffer out back to front)"""
    state = M.state_for(SC.SEED, 3, (1 << 32) + 7, 77, 1)
    src = tmp_path / "chacha_host.cpp"
    src.write_text('#include <cstdio>\n#include "%s"\nint main() {\n  zkproofs::detail::ChaChaRng g;\n  const uint32_t st[16] = {%s};\n'
                   '  for (int i = 0; i < 16; i++) g.st[i] = st[i];\n  g.have = 0; g.blocks_left = 2;\n'
                   '  for (int i = 0; i < 16; i++) std::printf("%%u\\n", g.next());\n  return 0;\n}\n'
                   % (os.path.join(ROOT, "zk-paillier_amd", "host", "bigint.hpp"), ", ".join("%du" % v for v in state)))
    exe = tmp_path / "chacha_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[::-1] == M.block_words(state)


def test_sample_below_definition():
    u = (1 << 200) + 1
    bits, nw = 201, 7
    v, rejected = M.sample_below(SC.SEED, 9, 4, M.FIELD_W, u)
    # attempt t is block t alone (nb = 1): its first seven words, the top one cut to 201 - 192 = 9 bits
    for t in range(rejected + 1):
        w = M.block(SC.SEED, t, 9, 4, M.FIELD_W)[:nw]
        w[-1] &= (1 << (bits - 192)) - 1
        cand = sum(x << (32 * i) for i, x in enumerate(w))
        assert (cand < u) == (t == rejected)
    assert cand == v
    # a bound of more than 16 words: attempt t reads blocks [t nb, (t + 1) nb)
    n = H.fixture_key()[2]
    v, rejected = M.sample_below(SC.SEED, 1, 0, M.FIELD_R1, n)
    words = sum((M.block(SC.SEED, 4 * rejected + k, 1, 0, M.FIELD_R1) for k in range(4)), [])
    assert v == sum(x << (32 * i) for i, x in enumerate(words)) & ((1 << 2048) - 1) < n
    vals, rej = M.sample_below_rows(SC.SEED, 9, range(12), M.FIELD_W, u)
    for row in range(12):
        assert (vals[row], rej[row]) == M.sample_below(SC.SEED, 9, row, M.FIELD_W, u)


def test_witness_properties():
    n = H.test_key(1024)[2]
    rng = SC._rng(b"props", 256)
    third = rng // 3
    wit, status, _, _ = M.witness(SC.SEED, 11, [n], [rng, 2, 0], 64)
    assert status == [0, M.MALFORMED, M.MALFORMED]
    coins = set()
    for row in range(64):
        w1, w2, r1, r2 = (wit[f][0][row] for f in ("w1", "w2", "r1", "r2"))
        a = max(w1, w2)
        assert third <= a < 2 * third and {w1, w2} == {a, a - third} and r1 < n and r2 < n
        coins.add(w1 < w2)
        assert (w1 < w2) == bool(M.coin(SC.SEED, 11, row))
        assert ((w1, w2, r1, r2), ) == (M.witness_row(SC.SEED, 11, row, n, rng)[0], )
    assert coins == {False, True}
    assert all(v == 0 for f in wit for b in (1, 2) for v in wit[f][b])
    # streams are per (index, row, field): another index, another witness; the index of proof b of a call is first_index + b
    again, _, _, _ = M.witness(SC.SEED, 12, [n], [rng], 4)
    assert again["r1"][0] != wit["r1"][0][:4]
    shifted, _, _, _ = M.witness(SC.SEED, 10, [n], [rng, rng], 4)
    assert shifted["r1"][1] == wit["r1"][0][:4] and shifted["w1"][1] == wit["w1"][0][:4]
    limbs = M.to_limbs(wit["r1"], 32)
    assert limbs.shape == (3, 64, 32) and H.L.limbs_to_int(limbs[0, 5]) == wit["r1"][0][5]


def test_a_bound_of_the_form_2_to_the_k_plus_1_rejects_about_half():
    u = (1 << 200) + 1
    _, rej = M.sample_below_rows(SC.SEED, 3, range(256), M.FIELD_W, u)
    total = sum(rej.values())
    # 256 values, each attempt accepted with probability (2^200 + 1) / 2^201: 256 rejections expected, standard deviation 22.6
    assert 150 <= total <= 370, total


def test_sample_below_rejects_a_candidate_equal_to_the_bound_and_takes_the_next_attempt():
    """a crafted bound: u IS the candidate of attempt 0 (1019 bits, two blocks per attempt, a masked top limb; the first row whose candidate
    has its top bit set, so that bit_length(u) is the 1019 the candidate was cut to).  `v < u` is strict: attempt 0 is rejected."""
    bits, nw, index = 1019, 32, 9

    def cand(row, t):
        words = M.block(SC.SEED, 2 * t, index, row, M.FIELD_R1) + M.block(SC.SEED, 2 * t + 1, index, row, M.FIELD_R1)
        return sum(x << (32 * i) for i, x in enumerate(words[:nw])) & ((1 << bits) - 1)

    row = next(r for r in range(64) if cand(r, 0) >> (bits - 1))
    u = cand(row, 0)
    assert u.bit_length() == bits
    v, rejected = M.sample_below(SC.SEED, index, row, M.FIELD_R1, u)
    assert rejected >= 1 and v == cand(row, rejected) < u and all(cand(row, t) >= u for t in range(rejected))
    assert M.sample_below(SC.SEED, index, row, M.FIELD_R1, u + 1) == (u, 0)          # one more, and attempt 0 is taken
    vals, rej = M.sample_below_rows(SC.SEED, index, [row], M.FIELD_R1, u)
    assert (vals[row], rej[row]) == (v, rejected)


# rejected attempts of the sampler cases of the GPU tests, counted once and pinned: the retry path is exercised by them for certain
REJECTED = {"n1024-shared-ef40-host": 205, "n2048-perkey-ef128-device": 722, "n2048-shared-ef256-host": 808, "n1024-perkey-ef128-device": 464}


@pytest.mark.parametrize("name", sorted(SC.sampler_cases()))
def test_the_gpu_test_inputs_contain_rejected_attempts_and_stay_far_from_the_cap(name):
    c = SC.sampler_cases()[name]
    wit, status, rejected, worst = SC.model_witness(name)
    want_status = [M.MALFORMED if r // 3 == 0 else 0 for r in c["ranges"]]
    assert status == want_status
    values = 3 * c["ef"] * status.count(0)
    print(name, "values", values, "rejected attempts", rejected, "worst", worst)
    assert rejected == REJECTED[name], (name, rejected)
    assert rejected >= values // 8, "the case would hardly exercise the retry loop"
    assert 2 <= worst <= 40 < M.MAX_ATTEMPTS          # some value needed a third attempt at least; nothing comes near the cap of 128


def test_new_entry_points_are_exported_and_refuse_bad_arguments_without_a_gpu():
    lib = zkp.load()
    for name in ("zkp_range_sample_witness_batch", "zkp_range_ni_prove_seeded_batch", "zkp_multi_range_ni_prove_seeded_batch", "zkp_diag_witness_residue"):
        assert hasattr(lib, name), name
    assert "zkp_range_ni_prove_seeded_batch" in zkp.EXPORTS and "zkp_diag_witness_residue" in zkp.capi.DIAG_EXPORTS
    for method in ("range_sample_witness", "range_ni_prove_seeded", "witness_residue"):
        assert callable(getattr(zkp.Context, method))
    assert callable(zkp.MultiContext.range_ni_prove_seeded)
    # a null ctx is refused before anything touches a device
    pb = zkp.RangeBatch(1024, 1, 128, shared_key=True)
    assert lib.zkp_range_ni_prove_seeded_batch(None, pb.struct(), None, None, bytes(32), 0, None, None, None, 0) == zkp.capi.ZKP_EINVAL
    assert lib.zkp_range_sample_witness_batch(None, pb.struct(), bytes(32), 0, None, None, None, None, None, 0) == zkp.capi.ZKP_EINVAL
    assert lib.zkp_multi_range_ni_prove_seeded_batch(None, pb.struct(), None, None, bytes(32), 0, None, None, None) == zkp.capi.ZKP_EINVAL
    with pytest.raises(ValueError):
        zkp.capi._seed(b"short")


def test_the_sampler_kernel_is_in_every_engine_and_free_of_scratch():
    """k_range_sample is part of the three builds' sources (one include in csrc/zkp_api.hip); in the throughput engine's device assembly
    its three instantiations exist and keep their state in registers"""
    isa = os.path.join(ROOT, "build", "v_isa", "isa.s")
    if not os.path.exists(isa):
        import __graft_entry__ as g
        g.build(force=True)
    text = open(isa).read()
    import re
    for g_lanes in (2, 4, 8):
        m = re.search(r"^(_ZN3zkp14k_range_sampleILi%dEEEvNS_15RangeSampleArgsE):[^\n]*\n(.*?)\n\s*\.end_amdhsa_kernel" % g_lanes, text, re.S | re.M)
        assert m, f"k_range_sample<{g_lanes}> is not in the device assembly"
        body = m.group(2)
        assert "scratch_" not in body, f"k_range_sample<{g_lanes}> spills"
        assert re.search(r"v_alignbit_b32|v_perm_b32|v_rot", body), "no rotate instruction in the block function"


def test_cpp_seeded_test_compiles_and_links():
    """tests/cpp/test_seeded.cpp (RangeProofNi::prove_batch_seeded of host/zkproofs.hpp) against the built library; it RUNS in
    tests/test_gpu_seeded_prove.py"""
    zkp.load()
    pkg = os.path.join(ROOT, "zk-paillier_amd")
    exe = os.path.join(ROOT, "build", "test_seeded")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_seeded.cpp"), "-o", exe, "-L" + pkg, "-lzkp_hip",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
