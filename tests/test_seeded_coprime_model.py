"""CPU tests of the seeded nonces of VerlinProof and MulProof: the Python restatement of the rule (tests/seeded_coprime_model.py) against
hand-built candidates, the statement that the GPU cases exercise both sorts of rejection and stay far from the cap, the word-for-word model
of the device GCD (tools/wbgcd_model.py) on the very candidates the kernel will test, the model's nonces through the Python model of the
two proves, and the new entry points in the built library."""
import importlib.util
import math
import os
import subprocess

import pytest

import helpers as H
import seeded_coprime_cases as SC
import seeded_coprime_model as M
import seeded_nonce_model as N
from helpers import pm

zkp = H.zkp
SEED = SC.SEED


def test_word_15_of_the_new_streams():
    seen = {M.word15(kind, 0, f) for kind, names in M.FIELDS.items() for f in range(len(names))}
    assert len(seen) == 4 + 2 and all(w >> 31 == 1 for w in seen)
    assert M.word15(M.KIND_VERLIN, 0, 3) == 0x80500003 and M.word15(M.KIND_MUL, 0, 1) == 0x80600001
    # apart from every stream of kinds 1 .. 4 (slot < 65536, field < 16)
    assert min(seen) > N.word15(4, 65535, 15)
    with pytest.raises(AssertionError):
        M.word15(M.KIND_MUL, 0, 2)
    # the state layout: counter in word 12, the index in 13 and 14
    index = SC.BIG + 3
    assert M.block(SEED, 9, index, M.KIND_VERLIN, 3) == \
        M.R.block_words(list(M.R.SIGMA) + M.R.key_words(SEED) + [9, index & M.M32, index >> 32, 0x80500003])


@pytest.mark.parametrize("n", [15, SC.HALF105(1024), SC.SMOOTH(2043), H.fixture_key()[2]])
def test_the_plain_fields_are_the_nonce_samplers_rule(n):
    """equal state words -> equal draws: seeded_nonce_model's sample_below, with the word 15 of kind 5 swapped in through the range model"""
    index, kind, field = SC.BIG + 2, M.KIND_VERLIN, 2
    v, rejected = M.sample_below(SEED, index, kind, field, n)
    w15 = M.word15(kind, 0, field)
    assert (v, rejected) == M.R.sample_below(SEED, index, w15 >> 2, w15 & 3, n)


def hand_built(index, kind, field, bits, t):
    """candidate t from the block function alone"""
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    words = sum((M.block(SEED, t * nb + k, index, kind, field) for k in range(nb)), [])
    return sum(x << (32 * i) for i, x in enumerate(words[:nw])) & ((1 << bits) - 1)


@pytest.mark.parametrize("n", [15, 3, SC.HALF105(1024), SC.SMOOTH(1019), SC.SMOOTH(2048)])
def test_attempt_order_and_the_shared_counter(n):
    """the accepted value is the first candidate, in attempt order, that is below n and coprime to it; every earlier attempt counts
    once, as not below n or as not coprime — one counter for both"""
    kind, field = M.KIND_MUL, 1
    for index in (5, SC.BIG + 1):
        v, not_below, not_coprime = M.sample_coprime_below(SEED, index, kind, field, n)
        t = not_below + not_coprime
        cands = [hand_built(index, kind, field, n.bit_length(), k) for k in range(t + 1)]
        assert v == cands[t] and v < n and math.gcd(v, n) == 1
        assert sum(1 for x in cands[:t] if x >= n) == not_below
        assert sum(1 for x in cands[:t] if x < n and math.gcd(x, n) != 1) == not_coprime
        # the candidates are those of sample_below(n) on the same stream: its value is the first one below n
        assert M.sample_below(SEED, index, kind, field, n)[0] == next(x for x in cands if x < n)


def test_candidate_zero_even_and_zero_bounds():
    # n == 1: one bit, the candidate below 1 is 0, gcd(0, 1) == 1
    v, not_below, not_coprime = M.sample_coprime_below(SEED, 0, M.KIND_VERLIN, 3, 1)
    assert v == 0 and not_coprime == 0
    # n == 3: candidate 0 is rejected by the gcd test (gcd(0, 3) == 3), so the value is 1 or 2
    for index in range(12):
        v, _, _ = M.sample_coprime_below(SEED, index, M.KIND_VERLIN, 3, 3)
        assert v in (1, 2)
    # n == 0 and an even n: every nonce zero, MALFORMED, the neighbours what they are without it
    n = H.test_key(1024)[2]
    alone, st, _, _ = M.nonces(M.KIND_VERLIN, SEED, 11, [n], 4)
    mixed, status, _, _ = M.nonces(M.KIND_VERLIN, SEED, 11, [n, 0, n - 1, n], 4)
    assert st == [0] * 4 and status == [0, M.MALFORMED, M.MALFORMED, 0]
    assert mixed[0] == alone[0] and mixed[3] == alone[3] and mixed[1] == mixed[2] == dict(a=0, a_prime=0, a_double_prime=0, r_a=0)
    # the index of proof b is first_index + b
    assert M.nonces(M.KIND_VERLIN, SEED, 12, [n], 3)[0] == alone[1:]


def test_exhaustion_marks_the_proof_malformed(monkeypatch):
    """with the cap at 3, the HALF105(1024) proofs that need a fourth attempt in either field come back zero and MALFORMED, the others as they were"""
    n, B = SC.HALF105(1024), 12
    full, _, not_below, not_coprime = M.nonces(M.KIND_MUL, SEED, 0, [n], B)
    monkeypatch.setattr(M, "MAX_ATTEMPTS", 3)
    cut, status, _, _ = M.nonces(M.KIND_MUL, SEED, 0, [n], B)
    assert any(status) and not all(status)
    for b in range(B):
        assert cut[b] == (dict(d=0, r_d=0) if status[b] else full[b])
        if not_below[b] + not_coprime[b] < 3:          # (fewer than three rejections in both fields together: neither field ran out)
            assert status[b] == 0


SPECIAL = {"SMOOTH": lambda n: n > 15 and n % SC.P_SMOOTH == 0, "HALF105": lambda n: n > 105 and n % 105 == 0 and n % SC.P_SMOOTH != 0, "15": lambda n: n == 15}


@pytest.mark.parametrize("name", sorted(SC.sampler_cases()))
def test_the_gpu_sampler_cases_reject_where_they_say_and_stay_far_from_the_cap(name):
    c = SC.sampler_cases()[name]
    out, status, not_below, not_coprime = SC.model_nonces(name)
    n_list = c["n_list"] * (c["B"] if len(c["n_list"]) == 1 else 1)
    assert status == [M.MALFORMED if n % 2 == 0 else 0 for n in n_list]
    print(name, "not below n", not_below, "not coprime", not_coprime)
    # the SMOOTH / HALF105 / 15 proofs of a batch take a gcd rejection somewhere among them, the HALF105 proofs a below-n rejection too
    special = {tag: [b for b, n in enumerate(n_list) if is_it(n)] for tag, is_it in SPECIAL.items()}
    if any(special.values()):
        assert sum(not_coprime[b] for idx in special.values() for b in idx) >= 1, f"{name}: no gcd rejection under this seed"
    if special["HALF105"]:
        assert sum(not_below[b] for b in special["HALF105"]) >= 1, f"{name}: no HALF105 proof takes a below-n rejection under this seed"
    names = M.FIELDS[c["kind"]]
    for b, n in enumerate(n_list):
        if status[b]:
            assert all(v == 0 for v in out[b].values())
            continue
        assert all(out[b][k] < n for k in names) and math.gcd(out[b][names[-1]], n) == 1
        # a condition on the inputs, not on the kernel: no value needs more than 40 attempts
        for f in range(len(names) - 1):
            assert M.sample_below(SEED, c["first_index"] + b, c["kind"], f, n)[1] + 1 <= 40
        _, k, g = M.sample_coprime_below(SEED, c["first_index"] + b, c["kind"], len(names) - 1, n)
        assert k + g + 1 <= 40 < M.MAX_ATTEMPTS, (name, b, k, g)
    if c["B"] == 130:
        assert sum(not_coprime) >= 100
        diff = sum(1 for b in range(129) if not_below[b] + not_coprime[b] != not_below[b + 1] + not_coprime[b + 1])
        assert diff >= 64, "neighbouring lanes are to need different numbers of attempts"


def test_every_sort_of_bound_takes_a_gcd_rejection_in_some_case():
    hits = {tag: 0 for tag in SPECIAL}
    for name, c in SC.sampler_cases().items():
        n_list = c["n_list"] * (c["B"] if len(c["n_list"]) == 1 else 1)
        not_coprime = SC.model_nonces(name)[3]
        for tag, is_it in SPECIAL.items():
            hits[tag] += sum(not_coprime[b] for b, n in enumerate(n_list) if is_it(n))
    assert all(hits.values()), hits


def wbgcd_model():
    spec = importlib.util.spec_from_file_location("wbgcd_model", os.path.join(H.ROOT, "tools", "wbgcd_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", sorted(SC.sampler_cases()))
def test_the_device_gcd_model_agrees_on_the_candidates_the_kernel_tests(name):
    """tools/wbgcd_model.py is kernels_gcd.hpp word for word; k_nonce_coprime calls wb_gcd<false>(candidate, n) with b = n odd, at the
    call's kernel width"""
    W = wbgcd_model()
    kw = SC.sampler_cases()[name]["n_bits"] // 32
    cands = SC.gcd_candidates(name)
    assert cands
    for b, n, v, ok in cands:
        g, _ = W.wbgcd(v, n, kw, cof=False)
        assert g == math.gcd(v, n) and (g == 1) == ok, (name, b)


def test_the_models_nonces_give_proofs_the_models_verify_accepts():
    for shape, three_q in [(SC.SHAPES[1], False), (SC.THREE_Q, True)]:
        v = SC.verlin_case(*shape, three_q)
        for b, n in enumerate(v["ns"]):
            i, z = v["ints"], v["ints"]["nonces"][b]
            proof = pm.verlin_prove(n, i["c"][b], i["cp"][b], i["phi_x"][b], *i["wit"][b], z["a"], z["a_prime"], z["a_double_prime"], z["r_a"])
            assert pm.verlin_verify(n, i["c"][b], i["cp"][b], i["phi_x"][b], *proof)
        m = SC.mul_case(*shape, three_q)
        for b, n in enumerate(m["ns"]):
            i, z = m["ints"], m["ints"]["nonces"][b]
            proof = pm.mul_proof_prove(n, *i["e"][b], *[i["wit"][b][k] for k in SC.MUL_WIT], z["d"], z["r_d"])
            assert pm.mul_proof_verify(n, *i["e"][b], *proof)


def test_the_three_q_case_sends_a_gcd_rejected_candidate_through_the_whole_prove():
    n_bits, B, first_index = SC.THREE_Q
    keys, stride = SC.keys_for(n_bits, B, True)
    assert stride == n_bits // 32 and all(n % 2 == 1 and n.bit_length() == 1024 for n in keys)
    q = keys[1] // 3
    assert keys[1] == 3 * q and q.bit_length() == 1022 and H.is_probable_prime(q) and keys[1] == keys[3] and keys[0] == keys[2] != keys[1]
    for kind in (M.KIND_VERLIN, M.KIND_MUL):
        _, status, _, not_coprime = M.nonces(kind, SEED, first_index, keys, B)
        assert not any(status)
        assert not_coprime[1] + not_coprime[3] >= 1 and not_coprime[0] == not_coprime[2] == 0, (kind, not_coprime)


def test_new_entry_points_are_exported_and_refuse_bad_arguments_without_a_gpu():
    lib = zkp.load()
    for name in ("zkp_nonce_sample_coprime_batch", "zkp_verlin_proof_prove_seeded_batch", "zkp_mul_proof_prove_seeded_batch"):
        assert hasattr(lib, name) and name in zkp.EXPORTS, name
    for method in ("nonce_sample_coprime", "verlin_proof_prove_seeded", "mul_proof_prove_seeded"):
        assert callable(getattr(zkp.Context, method))
    assert (zkp.SEEDED_KIND_VERLIN, zkp.SEEDED_KIND_MUL) == (M.KIND_VERLIN, M.KIND_MUL) == (5, 6)
    # a null ctx is refused before anything touches a device
    E = zkp.capi.ZKP_EINVAL
    assert lib.zkp_nonce_sample_coprime_batch(None, 5, 1024, 1, None, 0, bytes(32), 0, None, None, 0) == E
    assert lib.zkp_verlin_proof_prove_seeded_batch(None, 1024, 1, None, 0, *[None] * 7, bytes(32), 0, *[None] * 6, 0) == E
    assert lib.zkp_mul_proof_prove_seeded_batch(None, 1024, 1, None, 0, *[None] * 8, bytes(32), 0, *[None] * 6, 0) == E


def test_cpp_seeded_coprime_test_compiles_and_links():
    """tests/cpp/test_seeded_coprime.cpp (prove_batch_seeded of VerlinProof and MulProof in host/zkproofs.hpp) against the built library; it
    RUNS in tests/test_gpu_seeded_coprime.py"""
    zkp.load()
    pkg = os.path.join(H.ROOT, "zk-paillier_amd")
    exe = os.path.join(H.ROOT, "build", "test_seeded_coprime")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", os.path.join(H.ROOT, "tests", "cpp", "test_seeded_coprime.cpp"), "-o", exe,
                           "-L" + pkg, "-lzkp_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
