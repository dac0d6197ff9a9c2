"""CPU tests of the seeded nonces of ZeroProof, CiphertextProof, CorrectMessageProof and CompositeDLogProof: the Python restatement of the
stream (tests/seeded_nonce_model.py) against RFC 8439's own vector, the separation of its streams from one another and from the
RangeProofNi streams, one sample_below rule and not two, the model's nonces through the Python model of the four proves, the statement
that the GPU cases exercise the retry path, and the new entry points in the built library."""
import struct

import pytest

import helpers as H
import seeded_model as R
import seeded_nonce_cases as SC
import seeded_nonce_model as M
from helpers import pm

zkp = H.zkp
SEED = SC.SEED


def test_block_function_against_rfc8439_section_2_3_2():
    # RFC 8439, 2.3.2: key 00 01 .. 1f, nonce 00 00 00 09 00 00 00 4a 00 00 00 00, block counter 1
    key = struct.unpack("<8I", bytes(range(32)))
    state = list(R.SIGMA) + list(key) + [1, 0x09000000, 0x4A000000, 0x00000000]
    want = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
            0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]
    assert M.block_words(state) == want
    # the model's own state layout: counter in word 12, the index in 13 and 14, word 15 as published
    seed = bytes(range(32))
    index = (0x4A000000 << 32) | 0x09000000
    got = M.block(seed, 1, index, M.KIND_CORRECT_MESSAGE, 3, 2)
    assert got == M.block_words(list(R.SIGMA) + list(key) + [1, 0x09000000, 0x4A000000, 0x80000000 | (3 << 20) | (3 << 4) | 2])


def test_word_15_of_every_stream_of_a_call_is_unique_and_has_bit_31_set():
    seen = set()
    for kind in (M.KIND_ZERO, M.KIND_CIPHERTEXT, M.KIND_CORRECT_MESSAGE, M.KIND_DLOG):
        for slot, field, name, j, below in M.fields_of(kind, K=5):
            w = M.word15(kind, slot, field)
            assert w >> 31 == 1 and w < 1 << 32 and w not in seen, (kind, slot, field)
            seen.add(w)
    assert len(seen) == 1 + 2 + (2 + 2 * 4) + 1
    # the range streams stay below 1024 (row < 256, field < 4): no word 15 is shared with them
    assert max((row << 2) | f for row in (0, 255) for f in range(4)) < 1024 <= min(seen)
    # the extremes of the published ranges still fit and stay apart
    assert M.word15(4, 65535, 15) == 0x804FFFFF and M.word15(1, 0, 0) == 0x80100000
    with pytest.raises(AssertionError):
        M.word15(3, 65536, 0)


@pytest.mark.parametrize("n", [5, (1 << 200) + 1, SC.N_HALF, H.fixture_key()[2]])
def test_sample_below_is_the_range_samplers_rule(n):
    """equal nonce words -> equal draws: the range model's sample_below on the range model's state, with word 15 swapped in"""
    index, kind, slot, field = SC.BIG + 2, M.KIND_CORRECT_MESSAGE, 3, 3
    v, rejected = M.sample_below(SEED, index, kind, slot, field, n)
    assert v is not None and v < n
    # seeded_model.block builds word 15 as row << 2 | field: (row, field) = (w15 >> 2, w15 & 3) gives the same state
    w15 = M.word15(kind, slot, field)
    assert R.state_for(SEED, 9, index, w15 >> 2, w15 & 3) == list(R.SIGMA) + R.key_words(SEED) + [9, index & M.M32, index >> 32, w15]
    assert R.sample_below(SEED, index, w15 >> 2, w15 & 3, n) == (v, rejected)


def test_sample_below_rejects_a_candidate_equal_to_the_bound_and_takes_the_next_attempt():
    """a crafted bound: n IS the candidate of attempt 0 (2043 bits, four blocks per attempt, a masked top limb; the first z_sim slot whose
    candidate has its top bit set, so that bit_length(n) is the 2043 the candidate was cut to).  `v < n` is strict: attempt 0 is rejected."""
    bits, nw, index, kind, field = 2043, 64, SC.BIG + 5, M.KIND_CORRECT_MESSAGE, 3

    def cand(slot, t):
        words = sum((M.block(SEED, 4 * t + k, index, kind, slot, field) for k in range(4)), [])
        return sum(x << (32 * i) for i, x in enumerate(words[:nw])) & ((1 << bits) - 1)

    slot = next(j for j in range(1, 64) if cand(j, 0) >> (bits - 1))
    n = cand(slot, 0)
    assert n.bit_length() == bits
    v, rejected = M.sample_below(SEED, index, kind, slot, field, n)
    assert rejected >= 1 and v == cand(slot, rejected) < n and all(cand(slot, t) >= n for t in range(rejected))
    assert M.sample_below(SEED, index, kind, slot, field, n + 1) == (n, 0)          # one more, and attempt 0 is taken


def test_values_are_below_n_and_streams_are_per_index_slot_and_field():
    n = H.test_key(1024)[2]
    out, status, _ = M.nonces(M.KIND_CORRECT_MESSAGE, SEED, 11, [n], 3, K=4)
    assert status == [0, 0, 0]
    flat = []
    for d in out:
        assert d["r"] < n and d["w"] < n and all(z < n for z in d["z_sim"]) and all(e < 1 << 256 for e in d["e_sim"])
        assert len(d["e_sim"]) == len(d["z_sim"]) == 3
        flat += [d["r"], d["w"]] + d["e_sim"] + d["z_sim"]
    assert len(set(flat)) == len(flat)
    # the index of proof b of a call is first_index + b: a call that starts one later is the same call shifted
    shifted, _, _ = M.nonces(M.KIND_CORRECT_MESSAGE, SEED, 12, [n], 2, K=4)
    assert shifted == out[1:]
    # e_sim and the DLog r are the keystream words themselves
    assert out[0]["e_sim"][1] == sum(w << (32 * i) for i, w in enumerate(M.block(SEED, 0, 11, M.KIND_CORRECT_MESSAGE, 2, 2)[:8]))
    r = M.nonces(M.KIND_DLOG, SEED, 11, [], 1)[0][0]["r"]
    assert r == sum(w << (32 * i) for i, w in enumerate(M.block(SEED, 0, 11, M.KIND_DLOG, 0, 0))) and r < 1 << 512
    # n == 0: every nonce of that proof is zero, the neighbours are what they are without it
    mixed, status, _ = M.nonces(M.KIND_CORRECT_MESSAGE, SEED, 11, [n, 0, n], 3, K=4)
    assert status == [0, M.MALFORMED, 0] and mixed[0] == out[0] and mixed[2] == out[2]
    assert mixed[1] == dict(r=0, w=0, e_sim=[0, 0, 0], z_sim=[0, 0, 0])


def test_the_models_nonces_give_proofs_the_models_verify_accepts():
    p, q, n = H.test_key(1024)
    d = pm.Drbg(b"seeded-nonce-model-proofs")
    # ZeroProof: c = Enc(0, r)
    r = d.below(n)
    c = pm.enc(n, 0, r)
    z = M.nonces(M.KIND_ZERO, SEED, 0, [n], 1)[0][0]
    assert pm.zero_proof_verify(n, c, *pm.zero_proof_prove(n, c, r, z["r_prime"]))
    # CiphertextProof
    x = d.below(n)
    c = pm.enc(n, x, r)
    z = M.nonces(M.KIND_CIPHERTEXT, SEED, 0, [n], 1)[0][0]
    assert pm.ciphertext_proof_verify(n, c, *pm.ciphertext_proof_prove(n, c, x, r, z["x_prime"], z["r_prime"]))
    # CorrectMessageProof, the real message in every position of a list of four, and a list of one
    valid = [d.below(1 << 64) + 3 for _ in range(4)]
    for b, z in enumerate(M.nonces(M.KIND_CORRECT_MESSAGE, SEED, 7, [n], 4, K=4)[0]):
        proof = pm.correct_message_prove(n, valid, valid[b], z["r"], z["e_sim"], z["z_sim"], z["w"])
        assert pm.correct_message_verify(n, valid, *proof)
    z = M.nonces(M.KIND_CORRECT_MESSAGE, SEED, 7, [n], 1, K=1)[0][0]
    assert z["e_sim"] == z["z_sim"] == []
    assert pm.correct_message_verify(n, valid[:1], *pm.correct_message_prove(n, valid[:1], valid[0], z["r"], [], [], z["w"]))
    # CompositeDLogProof: g of order dividing phi, ni = g^-s
    g = pow(d.below(n), 2, n)
    s = d.bits(256)
    ni = pow(pm.mod_inv(g, n), s, n)
    z = M.nonces(M.KIND_DLOG, SEED, 0, [], 1)[0][0]
    assert pm.dlog_verify(*pm.dlog_prove(n, g, ni, s, z["r"]), n, g, ni)


@pytest.mark.parametrize("name", sorted(SC.sampler_cases()))
def test_the_gpu_sampler_cases_reject_where_they_say_and_stay_far_from_the_cap(name):
    c = SC.sampler_cases()[name]
    out, status, rejected = SC.model_nonces(name)
    n_list = c["n_list"] * (c["B"] if len(c["n_list"]) == 1 else 1)
    assert status == [M.MALFORMED if n == 0 else 0 for n in n_list] if n_list else status == [0] * c["B"]
    print(name, "rejected attempts per proof", rejected)
    for b, n in enumerate(n_list):
        if n in (5, SC.N_HALF):
            assert rejected[b] >= 1, f"{name}: proof {b} (n = {n if n == 5 else '2^1023 + 1155'}) never takes the retry path under this seed"
        if n == 0:
            assert all(v == 0 or v == [0] * (c["K"] - 1) for v in out[b].values())
    draws = sum(1 for f in M.fields_of(c["kind"], c["K"]) if f[4])
    assert max(rejected) <= 40 * max(draws, 1) < M.MAX_ATTEMPTS * max(draws, 1)


def test_new_entry_points_are_exported_and_refuse_bad_arguments_without_a_gpu():
    lib = zkp.load()
    names = ("zkp_nonce_sample_batch", "zkp_zero_proof_prove_seeded_batch", "zkp_ciphertext_proof_prove_seeded_batch",
             "zkp_correct_message_prove_seeded_batch", "zkp_dlog_prove_seeded_batch")
    for name in names:
        assert hasattr(lib, name) and name in zkp.EXPORTS, name
    for method in ("nonce_sample", "zero_proof_prove_seeded", "ciphertext_proof_prove_seeded", "correct_message_prove_seeded", "dlog_prove_seeded"):
        assert callable(getattr(zkp.Context, method))
    assert (zkp.SEEDED_KIND_ZERO, zkp.SEEDED_KIND_CIPHERTEXT, zkp.SEEDED_KIND_CORRECT_MESSAGE, zkp.SEEDED_KIND_DLOG) == \
        (M.KIND_ZERO, M.KIND_CIPHERTEXT, M.KIND_CORRECT_MESSAGE, M.KIND_DLOG)
    # a null ctx is refused before anything touches a device
    E = zkp.capi.ZKP_EINVAL
    assert lib.zkp_nonce_sample_batch(None, 1, 1024, 1, 1, None, 0, bytes(32), 0, None, None, 0) == E
    assert lib.zkp_zero_proof_prove_seeded_batch(None, 1024, 1, None, 0, None, None, bytes(32), 0, None, None, None, 0) == E
    assert lib.zkp_ciphertext_proof_prove_seeded_batch(None, 1024, 1, None, 0, None, None, None, bytes(32), 0, None, None, None, None, 0) == E
    assert lib.zkp_correct_message_prove_seeded_batch(None, 1024, 1, 2, None, 0, None, None, bytes(32), 0, None, None, None, None, None, 0) == E
    assert lib.zkp_dlog_prove_seeded_batch(None, 1024, 768, 1, None, None, None, None, bytes(32), 0, None, None, None, 0) == E


def test_the_nonce_sampler_is_in_the_device_assembly_and_free_of_scratch():
    """as the range sampler: the three instantiations of k_nonce_sample keep their state in registers"""
    import os
    import re
    isa = os.path.join(H.ROOT, "build", "v_isa", "isa.s")
    if not os.path.exists(isa):
        import __graft_entry__ as g
        g.build(force=True)
    text = open(isa).read()
    for g_lanes in (2, 4, 8):
        m = re.search(r"^(_ZN3zkp14k_nonce_sampleILi%dEEEvNS_15NonceSampleArgsE):[^\n]*\n(.*?)\n\s*\.end_amdhsa_kernel" % g_lanes, text, re.S | re.M)
        assert m, f"k_nonce_sample<{g_lanes}> is not in the device assembly"
        assert "scratch_" not in m.group(2), f"k_nonce_sample<{g_lanes}> spills"
    for name in ("k_nonce_raw", "k_nonce_fixup", "k_nonce_prep"):
        m = re.search(r"^(_ZN3zkp\d+%sENS_15NonceSampleArgsE):[^\n]*\n(.*?)\n\s*\.end_amdhsa_kernel" % name, text, re.S | re.M)
        assert m, f"{name} is not in the device assembly"
        assert "scratch_" not in m.group(2), f"{name} spills"


def test_cpp_seeded_sigma_test_compiles_and_links():
    """tests/cpp/test_seeded_sigma.cpp (prove_batch_seeded of the four proofs in host/zkproofs.hpp) against the built library; it RUNS in
    tests/test_gpu_seeded_nonces.py"""
    import os
    import subprocess
    zkp.load()
    pkg = os.path.join(H.ROOT, "zk-paillier_amd")
    exe = os.path.join(H.ROOT, "build", "test_seeded_sigma")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", os.path.join(H.ROOT, "tests", "cpp", "test_seeded_sigma.cpp"), "-o", exe,
                           "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
