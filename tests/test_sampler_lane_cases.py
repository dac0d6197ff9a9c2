"""CPU statement that the inputs of tests/test_gpu_sampler_lanes.py (tests/sampler_lane_cases.py) reach what they aim at:

(a) the lane model (tests/sampler_lane_model.py: the group logic of the two sampler kernels, word for word) equals the value-level models
    (tests/seeded_model.py, tests/seeded_nonce_model.py: plain integers) on every sampler case, old and new;
(b) the coverage table, computed from the new cases by the value-level models alone, has every cell for both kernels at G = 2, 4, 8;
(c) four mutants of the lane model differ from the value models on the new cases, and reproduce them on the OLD cases — which is why the
    old inputs could not see such a fault (one exception, named in its test: the old bound n = 5 sees "accept-equal" inside one word);
(d) the rejected attempts of every new case are pinned and no value comes near the cap of 128 attempts.

The exhaustion of all 128 attempts is out of reach of any input one can construct and is not simulated."""
import random

import pytest

import sampler_lane_cases as C
import sampler_lane_model as LM
import seeded_cases as RC
import seeded_model as R
import seeded_nonce_cases as NC
import seeded_nonce_model as N

LANE = C.LANE
OLD_RANGE = sorted(RC.sampler_cases())
OLD_NONCE = sorted(k for k, c in NC.sampler_cases().items() if c["kind"] != N.KIND_DLOG)          # (DLog has no sample_below field)
NEW_RANGE = sorted(C.range_cases())
NEW_NONCE = sorted(C.nonce_cases())


def lane_witness(c, mutant=None):
    return LM.witness(RC.SEED, c["first_index"], c["n_list"], c["ranges"], c["ef"], c["n_bits"] // LANE, mutant)


def lane_nonces(c, mutant=None):
    return LM.nonces(c["kind"], NC.SEED, c["first_index"], c["n_list"], c["B"], c["K"], c["n_bits"] // LANE, mutant)


# ---- the pieces of the lane model against plain integers -----------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 4, 8])
def test_group_less_is_the_integer_comparison_at_every_place_in_the_wavefront(G):
    rnd = random.Random(G)
    for k in range(400):
        u = rnd.getrandbits(LANE * G)
        v = u
        for lane in rnd.sample(range(G), rnd.randint(0, G)):          # differ in a few lanes, one word each; none: equality
            v ^= (rnd.getrandbits(32) or 1) << (LANE * lane + 32 * rnd.randrange(16))
        g0 = G * rnd.randrange(64 // G)
        assert LM.group_less(LM.to_lanes(v, G), LM.to_lanes(u, G), g0, G, G) == (v < u), (k, g0)
    assert LM.from_lanes(LM.to_lanes(u, G)) == u


@pytest.mark.parametrize("G", [2, 4, 8])
def test_group_add_is_the_integer_sum_for_every_pattern_of_generate_and_propagate(G):
    """every lane one of: no carry, a generate, exactly 2^512, all ones, 2^512 - 2 — all 5^G patterns at G = 2 and 4, 3000 drawn ones at G = 8"""
    rnd = random.Random(100 + G)
    kinds = ("plain", "gen", "zero", "prop", "near")
    patterns = [[kinds[(p // 5 ** i) % 5] for i in range(G)] for p in range(5 ** G)] if G < 8 else [[rnd.choice(kinds) for _ in range(G)] for _ in range(3000)]
    for pat in patterns:
        s = rnd.getrandbits(LANE * G) | sum(2 << (LANE * i) for i in range(G))
        t = sum(C.lane_addend(k, sl) << (LANE * i) for i, (k, sl) in enumerate(zip(pat, C.lanes_of(s, G))))
        g0 = G * rnd.randrange(64 // G)
        got = LM.from_lanes(LM.group_add(LM.to_lanes(s, G), LM.to_lanes(t, G), g0, G))
        assert got == (s + t) & ((1 << (LANE * G)) - 1), pat


# ---- (a) the lane model equals the value-level models ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OLD_RANGE + NEW_RANGE)
def test_lane_model_equals_the_range_model(name):
    old = name in RC.sampler_cases()
    c = RC.sampler_cases()[name] if old else C.range_cases()[name]
    assert lane_witness(c) == (RC.model_witness(name) if old else C.model_witness(name))


@pytest.mark.parametrize("name", OLD_NONCE + NEW_NONCE)
def test_lane_model_equals_the_nonce_model(name):
    old = name in NC.sampler_cases()
    c = NC.sampler_cases()[name] if old else C.nonce_cases()[name]
    assert lane_nonces(c) == (NC.model_nonces(name) if old else C.model_nonces(name))


# ---- (b) the coverage table ------------------------------------------------------------------------------------------------------------
def table(kernel, n_bits):
    names, cover = (NEW_RANGE, C.range_coverage) if kernel == "range" else (NEW_NONCE, C.nonce_coverage)
    cells = set()
    for name in names:
        if name.endswith("-%d" % n_bits) or "-%d-" % n_bits in name:
            cells |= cover(name)
    return cells


@pytest.mark.parametrize("n_bits", C.WIDTHS)
@pytest.mark.parametrize("kernel", ["range", "nonce"])
def test_coverage_table_has_every_cell(kernel, n_bits):
    """Every deciding lane with accept and with reject (the deciding word in the middle of its lane, everything below it saying the
    opposite), equality at full width, a bound with idle top lanes, one crafted comparison in each of Zero / Ciphertext field 1 / a
    z_sim slot j >= 1; for the range kernel a generate into each single lane, the full chain, the stopped chain, the ripple inside a
    lane and the near miss, each under both coins; a wavefront with two fields and one with all three, groups of different nb in one
    wavefront, the groups of a MALFORMED proof among live ones, a crafted group at lane >= 32 of its wavefront.
    At G = 2 no lane can receive a carry AND propagate or nearly propagate (lane 0 has no carry-in, lane 1 is the top lane and its sum is below 2^511),
    so there "stopped" is lane 0 all ones without a carry-in and "near" is lane 0 = 2^512 - 2, both with no carry into lane 1."""
    G = n_bits // LANE
    have, want = table(kernel, n_bits), C.required_cells(kernel, G)
    print(kernel, G, sorted(map(str, have)))
    assert not want - have, sorted(map(str, want - have))


def test_targets_are_what_they_were_crafted_for():
    """the crafted (proof, row | slot, field) of every batch, by the value-level models: accepted or rejected at attempt 0 as crafted, the
    deciding lane, bit_length(u) as the candidate was computed with, the full chain's carry-ins [0, 1, ..., 1]"""
    for name, c in C.range_cases().items():
        G = c["n_bits"] // LANE
        for t in c["targets"]:
            b, row, f, case = t["b"], t["row"], t["field"], t["case"]
            index = c["first_index"] + b
            u = c["n_list"][b if len(c["n_list"]) > 1 else 0] if f else c["ranges"][b] // 3
            v, rejected = R.sample_below(RC.SEED, index, row, f, u)
            v0 = C.range_candidate(index, row, f, u.bit_length())
            if case[0] in ("decide", "short"):
                d, accept = (case[1], case[2]) if case[0] == "decide" else (case[2], True)
                assert u.bit_length() == (C.full_bits(G) if case[0] == "decide" else case[1])
                assert (rejected == 0) == accept and (v == v0) == accept and ((v0 ^ u).bit_length() - 1) // LANE == d, (name, t)
            elif case[0] == "equal":
                assert v0 == u and rejected >= 1 and v < u
            else:
                assert rejected == 0 and v == v0 and u.bit_length() == C.carry_bits(G) and c["ranges"][b] < 1 << (LANE * G)
                cells, cin = C.carry_cells(u, v, G, C.range_coin(index, row))
                assert (case + (C.range_coin(index, row),)) in cells, (name, t)
                if case[0] == "full":
                    assert cin == [0] + [1] * (G - 1)
                if "coin" in t:
                    assert C.range_coin(index, row) == t["coin"] == R.coin(RC.SEED, index, row)
    for name, c in C.nonce_cases().items():
        G = c["n_bits"] // LANE
        for t in c["targets"]:
            b, slot, f, case = t["b"], t["slot"], t["field"], t["case"]
            u = c["n_list"][b]
            v, rejected = N.sample_below(NC.SEED, c["first_index"] + b, c["kind"], slot, f, u)
            v0 = C.nonce_candidate(c["first_index"] + b, c["kind"], slot, f, u.bit_length())
            if case[0] == "equal":
                assert v0 == u and rejected >= 1 and v < u
            else:
                d, accept = (case[1], case[2]) if case[0] == "decide" else (case[2], True)
                assert (rejected == 0) == accept and (v == v0) == accept and ((v0 ^ u).bit_length() - 1) // LANE == d, (name, t)
            assert c["kind"] != N.KIND_CORRECT_MESSAGE or slot >= 1


# ---- (c) the mutants ---------------------------------------------------------------------------------------------------------------------
# the new batches on which a mutant gives another witness / other nonces than the value model
def caught_by(mutant):
    out = [n for n in NEW_RANGE if lane_witness(C.range_cases()[n], mutant) != C.model_witness(n)]
    return out + [n for n in NEW_NONCE if lane_nonces(C.nonce_cases()[n], mutant) != C.model_nonces(n)]


def old_cases_that_differ(mutant):
    out = [n for n in OLD_RANGE if lane_witness(RC.sampler_cases()[n], mutant) != RC.model_witness(n)]
    return out + [n for n in OLD_NONCE if lane_nonces(NC.sampler_cases()[n], mutant) != NC.model_nonces(n)]


def test_the_two_carry_mutants():
    # a third of full width carries from lane to lane in about every second row, crafted or not: every new range batch sees "cin0"
    assert caught_by("cin0") == NEW_RANGE
    # a carry that crosses ONE lane is right under "gen-only"; it fails where a carry has to pass a lane of all ones, which takes three lanes:
    # the full and the stopped chain at G = 4 and 8.  At G = 2 the mutant IS the kernel's formula (lane 1 is the only receiver).
    assert caught_by("gen-only") == [n for n in NEW_RANGE if "1024" not in n and not n.endswith("compare")]
    # the old cases keep third and s in lane 0 (ranges of at most 258 bits): no carry leaves it, and neither mutant shows
    assert old_cases_that_differ("cin0") == [] and old_cases_that_differ("gen-only") == []


def test_the_two_comparison_mutants():
    """"top-lane" rejects when the top occupied lane is equal, so it shows where a lower lane ACCEPTS (a crafted rejection it gets right by
    accident); "accept-equal" shows on the crafted equality and on any other candidate that equals its bound."""
    got = caught_by("top-lane")
    for kernel_names in (NEW_RANGE, NEW_NONCE):
        for n_bits in C.WIDTHS:
            assert any(str(n_bits) in n for n in got if n in kernel_names), (n_bits, got)
    assert all(n in got for n in NEW_RANGE if n.endswith("compare")) and all(n in got for n in NEW_NONCE if n.startswith("zero"))
    # the old bounds are random, 2^k + 1 or tiny: the top occupied lane always differs
    assert old_cases_that_differ("top-lane") == []
    got = caught_by("accept-equal")
    for kernel_names in (NEW_RANGE, NEW_NONCE):
        for n_bits in C.WIDTHS:
            assert any(str(n_bits) in n for n in got if n in kernel_names), (n_bits, got)
    # The old RANGE cases cannot see it.  One old NONCE case can, and the claim that none does is dropped for this mutant:
    # ciphertext-2048-perkey-B3-host has the bound n = 5, three bits in ONE word of lane 0, and a candidate of its stream equals 5.  That is
    # equality inside a lane (`c == 0` after the word loop); equality of a value that spans every lane (`m == 0` over the ballots) is new here.
    assert old_cases_that_differ("accept-equal") == ["ciphertext-2048-perkey-B3-host"]


# ---- (d) the cap, and the batches as they are ------------------------------------------------------------------------------------------------
# (first_index, rejected attempts in all) of every new batch, counted once by the value-level models and pinned
PINNED_RANGE = {"range-1024-carry": (1001, 20), "range-1024-compare": ((1 << 32) + 100, 3), "range-1024-five": ((1 << 32) + 7, 35), "range-1024-one": (7, 4),
                "range-2048-carry": (1267, 8), "range-2048-compare": ((1 << 32) + 106, 22), "range-2048-five": ((1 << 32) + 7, 19), "range-2048-one": (7, 0),
                "range-4096-carry": (2394, 28), "range-4096-compare": ((1 << 32) + 100, 31), "range-4096-five": ((1 << 32) + 7, 26), "range-4096-one": (7, 1)}
PINNED_NONCE = {"ciphertext-1024": ((1 << 32) + 2007, 8), "ciphertext-2048": ((1 << 32) + 2017, 2), "ciphertext-4096": ((1 << 32) + 2029, 7),
                "message-1024": ((1 << 32) + 3007, 7), "message-2048": ((1 << 32) + 3007, 8), "message-4096": ((1 << 32) + 3007, 20),
                "zero-1024": ((1 << 32) + 1011, 2), "zero-2048": ((1 << 32) + 1031, 2), "zero-4096": ((1 << 32) + 1157, 7)}


@pytest.mark.parametrize("name", NEW_RANGE)
def test_range_batches_are_pinned_and_stay_far_from_the_cap(name):
    c = C.range_cases()[name]
    _, status, rejected, worst = C.model_witness(name)
    print(name, "first_index", c["first_index"], "rejected", rejected, "worst", worst)
    assert status == [R.MALFORMED if r // 3 == 0 else 0 for r in c["ranges"]]
    assert (c["first_index"], rejected) == PINNED_RANGE[name]
    assert worst <= 40 < R.MAX_ATTEMPTS
    lanes = 3 * len(c["ranges"]) * c["ef"] * c["n_bits"] // LANE
    assert c["ef"] <= 8 and lanes <= 1024, lanes


@pytest.mark.parametrize("name", NEW_NONCE)
def test_nonce_batches_are_pinned_and_stay_far_from_the_cap(name):
    c = C.nonce_cases()[name]
    _, status, rejected = C.model_nonces(name)
    print(name, "first_index", c["first_index"], "rejected per proof", rejected)
    assert status == [0] * c["B"]
    assert (c["first_index"], sum(rejected)) == PINNED_NONCE[name]
    # no VALUE needs more than 40 attempts: checked value by value
    for b, n in enumerate(c["n_list"]):
        for slot, f, _, _, below in N.fields_of(c["kind"], c["K"]):
            assert not below or N.sample_below(NC.SEED, c["first_index"] + b, c["kind"], slot, f, n)[1] <= 40 < N.MAX_ATTEMPTS
