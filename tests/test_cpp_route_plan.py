"""The routing header (zk-paillier_amd/csrc/route_plan.hpp) as a program of its own, under the address and undefined-behaviour sanitizers
(tests/cpp/test_route_plan.cpp; no GPU, no library, nothing loaded into this process): the full decision for every RangeProofNi prove and
verify call of 1 ... 400 proofs under one 2048-bit key, for 256, 64 and 304 compute units and for every switch and engine set.

  against the model    family and tail equal tests/routing_model.py at every size (the device test compares the model at 16 sizes)
  against the parent   the decisions equal tests/golden/route_plan.json, recorded from the expressions the header replaced
  one rule, two callers   "takes the hashes" as range_verify_impl asks it ahead of the launch = the hash placement of the launch's own plan
  no hidden state      computed twice, the second time in the opposite order: the same lines"""
import json
import os
import re
import subprocess

import helpers as H
import routing_model as R

ROOT = H.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "route_plan.json")
NUMBER = re.compile(r"\d+")
MAX_B = 400


def run_program():
    src = os.path.join(ROOT, "tests", "cpp", "test_route_plan.cpp")
    exe = os.path.join(ROOT, "build", "test_route_plan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
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
