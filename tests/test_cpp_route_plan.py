"""The routing header (zk-paillier_amd/csrc/route_plan.hpp) as a program of its own, under the address and undefined-behaviour sanitizers
(tests/cpp/test_route_plan.cpp; no GPU, no library, nothing loaded into this process): the full decision for every RangeProofNi prove and
verify call of 1 ... 400 proofs under one 2048-bit key, for 256, 64 and 304 compute units and for every switch and engine set.

  against the model    family and tail equal tests/routing_model.py at every size (the device test compares the model at 16 sizes)
  against the parent   the decisions equal tests/golden/route_plan.json, recorded from the expressions the header replaced
  one rule, two callers   "takes the hashes" as range_verify_impl asks it ahead of the launch = the hash placement of the launch's own plan
  no hidden state      computed twice, the second time in the opposite order: the same lines
  other row counts     the same program at 1, 7, 40, 120 and 256 rows per proof, every batch up to 48 items per SIMD on the three chips, against
                       the model — with what no size may break: a head inside the batch and inside its engine's one round, a grid for every
                       launch the plan takes, the hashes aboard within the bound their branch states"""
import functools
import json
import os
import re
import subprocess

import pytest

import helpers as H
import routing_model as R

ROOT = H.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "route_plan.json")
NUMBER = re.compile(r"\d+")
MAX_B = 400


@functools.lru_cache(maxsize=None)
def built_program():
    src = os.path.join(ROOT, "tests", "cpp", "test_route_plan.cpp")
    exe = os.path.join(ROOT, "build", "test_route_plan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    return exe


def run_program(*args):
    out = subprocess.run([built_program()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def parse(lines):
    """{config: {"prove": {B: decision}, "verify": {B: decision}, "takes": [(w, B, asked, placed)]}}"""
    configs, cur = {}, None
    for line in lines:
        word, _, rest = line.partition(" ")
        if word == "config":
            cur = configs[rest] = {"prove": {}, "verify": {}, "takes": []}
        elif word == "takes":
            cur["takes"].append(tuple(int(x) for x in rest.split()))
        else:
            b, _, decision = rest.partition(" ")
            cur[word][int(b)] = decision
    return configs


def run_lengths(decisions):
    """{B: decision} for B = 1 ... as intervals [first B, decision at first B, {index of a number in it: its step per proof}]: a decision belongs to the
    interval while its text is the same but for the numbers and every number goes on in its arithmetic progression (a grid that grows with B)"""
    runs = []
    for b in sorted(decisions):
        d = decisions[b]
        shape, nums = NUMBER.sub("#", d), [int(x) for x in NUMBER.findall(d)]
        if runs:
            first, d0, steps = runs[-1]
            nums0 = [int(x) for x in NUMBER.findall(d0)]
            if NUMBER.sub("#", d0) == shape:
                if steps is None and b == first + 1:
                    runs[-1][2] = steps = [x - y for x, y in zip(nums, nums0)]
                if steps is not None and nums == [y + s * (b - first) for y, s in zip(nums0, steps)]:
                    continue
        runs.append([b, d, None])
    return [[first, d, {str(i): s for i, s in enumerate(steps or []) if s}] for first, d, steps in runs]      # (the numbers that move: index -> step)


def expand(runs, last):
    out = {}
    for k, (first, d, steps) in enumerate(runs):
        end = runs[k + 1][0] if k + 1 < len(runs) else last + 1
        nums = [int(x) for x in NUMBER.findall(d)]
        for b in range(first, end):
            vals = iter([y + steps.get(str(i), 0) * (b - first) for i, y in enumerate(nums)])
            out[b] = NUMBER.sub(lambda m: str(next(vals)), d)
    return out


def family_and_tail(decision):
    """the names of tests/routing_model.py for a printed decision (the key qualifies for the base-n form)"""
    if decision.startswith("cut "):
        return "split", int(re.search(r"tail=(\d+)", decision).group(1))
    engine = re.match(r"whole @(\w+)", decision).group(1)
    form, r2l = (int(re.search(r"%s=(\d)" % f, decision).group(1)) for f in ("form", "r2l"))
    if engine == "mid":
        return ("mid-basen" if form else "mid-n2"), 0
    if engine == "lat":
        return ("lat-r2l" if r2l else "lat-basen" if form else "lat-n2"), 0
    return ("base-n" if form else "n2"), 0


def test_route_plan_under_sanitizers():
    text = run_program().splitlines()
    cut = text.index("pass 2")
    first, second = text[:cut], text[cut + 1:]
    # no hidden state
    assert first == second
    got = parse(first)
    # against the model: every size, both call kinds, all three chips — and the engine sets the model knows
    engines = {"no_lat": (0, 18), "no_mid": (9, 0), "no_engines": (0, 0)}
    wrong = []
    for name in ("cus256", "cus64", "cus304", "no_lat", "no_mid", "no_engines"):
        cus = int(name[3:]) if name.startswith("cus") else 256
        lat, mid = engines.get(name, (9, 18))
        for kind in ("prove", "verify"):
            for b in range(1, MAX_B + 1):
                fam, tail = family_and_tail(got[name][kind][b])
                want = R.expected_family(cus, lat, mid, 2 * 128 * b, listed=kind == "verify")
                if fam != want or (fam == "split" and tail != R.expected_tail(cus, b)):
                    wrong.append((name, kind, b, fam, tail, want))
    assert not wrong, wrong[:20]
    # against the parent
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(got)
    for name, kinds in golden.items():
        for kind in ("prove", "verify"):
            want = expand(kinds[kind], MAX_B)
            assert sorted(want) == list(range(1, MAX_B + 1))
            diff = [(b, got[name][kind][b], want[b]) for b in want if got[name][kind][b] != want[b]]
            assert not diff, (name, kind, diff[:5])
    # one rule, two callers
    for name, c in got.items():
        assert c["takes"], name
        assert all(asked == (placed != 0) for _, _, asked, placed in c["takes"]), (name, [t for t in c["takes"] if t[2] != (t[3] != 0)][:10])
    assert any(placed == 16 for _, _, _, placed in got["cus256"]["takes"]) and any(placed == 64 for _, _, _, placed in got["cus256"]["takes"])


PART = re.compile(r"\[w=(\d+) pair=(\d) form=(\d) r2l=(\d) lanes=(\d+) blocks=(\d+) wgs=(\d+) hash=(\d+) two=(\d) side=(\d)\]")
HEAD_ENGINE = {"mid": 18, "lat": 9, "own": 36}


def parts_of(decision, batch):
    """[(proofs of the part, its printed plan as a dict)] of a decision: one part, or the head and the tail of a cut call"""
    plans = [dict(zip(("w", "pair", "form", "r2l", "lanes", "blocks", "wgs", "hash", "two", "side"), (int(x) for x in m))) for m in PART.findall(decision)]
    if decision.startswith("cut "):
        head, tail = int(re.search(r"head=(\d+)@", decision).group(1)), int(re.search(r"tail=(\d+)", decision).group(1))
        assert len(plans) == 2, decision
        return [(head, plans[0]), (tail, plans[1])]
    assert len(plans) == 1, decision
    return [(batch, plans[0])]


def check_decisions(got, ef, last_of):
    """every decision of the three chips at `ef` rows per proof against the model, and the invariants no size may break"""
    rows = 2 * ef
    wrong = []
    for name in ("cus256", "cus64", "cus304"):
        cus = int(name[3:])
        simds = 4 * cus
        last = last_of(cus)
        for kind in ("prove", "verify"):
            listed = kind == "verify"
            never = kind == "prove" and ef != 128                 # (generate_encrypted_pairs: routed by its items, never cut)
            assert sorted(got[name][kind]) == list(range(1, last + 1)), (name, kind, ef)
            for b in range(1, last + 1):
                d = got[name][kind][b]
                at = (ef, name, kind, b, d)
                fam, tail = family_and_tail(d)
                want = R.expected_family(cus, 9, 18, rows * b, listed=listed, rows_per_proof=rows, never_split=never)
                cut = None if never else R.expected_split(cus, b, rows, listed)
                if fam != want or (fam == "split") != (cut is not None):
                    wrong.append((at, fam, want))
                    continue
                parts = parts_of(d, b)
                if cut:
                    head, engine, per_simd = cut
                    got_head, got_engine = re.search(r"head=(\d+)@(\w+)", d).groups()
                    assert 0 < int(got_head) < b and int(got_head) + tail == b, at
                    assert int(got_head) * rows <= per_simd * simds, at          # the head fits the one round it was cut for
                    assert (int(got_head), got_engine) == (head, engine) and tail == R.expected_tail(cus, b, rows, listed), (at, cut)
                    assert parts[0][1]["w"] == HEAD_ENGINE[engine] and parts[1][1]["w"] == 9, at
                else:
                    assert not d.startswith("cut "), at
                for proofs, p in parts:
                    assert proofs > 0, at
                    if p["form"]:
                        assert p["blocks"] > 0, at                               # a launch the plan takes has a grid
                        if p["r2l"]:
                            assert p["wgs"] > 0 and p["lanes"] in (36, 12, 8), at
                    if p["hash"]:                                                # the transcript hashes aboard: one workgroup each, in front of the Enc workgroups
                        assert p["form"] and p["r2l"] and p["hash"] in (16, 64), at
                        bound = cus if p["lanes"] == 36 else simds if p["hash"] == 64 else 2 * simds
                        assert proofs + p["wgs"] <= bound, (at, bound)
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("ef", [1, 7, 40, 120, 256])
def test_route_plan_at_other_row_counts(ef):
    """the same program at another error factor: every batch from 1 to the first one beyond 48 items per SIMD, on the three chips — the
    model is the reference (tests/test_gpu_range_error_factors.py holds the model against the device)"""
    text = run_program(ef).splitlines()
    cut = text.index("pass 2")
    assert text[:cut] == text[cut + 1:]
    got = parse(text[:cut])
    assert sorted(got) == ["cus256", "cus304", "cus64"]
    check_decisions(got, ef, lambda cus: 48 * 4 * cus // (2 * ef) + 1)
    for name, c in got.items():
        assert c["takes"], name
        assert all(asked == (placed != 0) for _, _, asked, placed in c["takes"]), (ef, name, [t for t in c["takes"] if t[2] != (t[3] != 0)][:10])
    # the sweep reaches what it is about: at 40 rows a verify is cut in both of its windows — 4 ... 5 and 16 ... 24 items per SIMD; the third,
    # 8 ... 9 per SIMD (103 ... 115 proofs), is a window of proves only: a verify of that size fits the latency engine's one round by its
    # expected items, as 33 ... 36 proofs of 128 rows do — and a prove never is
    if ef == 40:
        cuts = {b: re.search(r"head=(\d+)@(\w+)", d).groups() for b, d in got["cus256"]["verify"].items() if d.startswith("cut ")}
        assert sorted(cuts) == list(range(52, 65)) + list(range(263, 308))
        assert {cuts[b] for b in range(52, 65)} == {("51", "lat")} and {cuts[b] for b in range(263, 308)} == {("204", "mid")}
        assert not any(d.startswith("cut ") for d in got["cus256"]["prove"].values())


def test_route_plan_invariants_at_128_rows():
    text = run_program().splitlines()
    got = parse(text[:text.index("pass 2")])
    check_decisions(got, 128, lambda cus: MAX_B)
