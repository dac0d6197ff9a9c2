"""Inputs that reach the places where the G = kw / 16 lanes of one sampled value have to agree (csrc/kernels_sample.hpp: k_range_sample<G>,
k_nonce_sample<G>): the comparison `v < u` decided by a lane BELOW the top one, equality, a bound whose top lanes are empty, and the carry
of a = third + s across lanes.  A plain module in the style of tests/seeded_cases.py: tests/test_sampler_lane_cases.py (CPU) asserts with
the value-level models that every case reaches what it aims at, tests/test_gpu_sampler_lanes.py holds the GPU to the models on them.

Why crafting: against a random bound the top occupied lane differs with probability 1 - 2^-512, and a range of 258 bits keeps third and s in
lane 0.  The stream is a published function of (seed, index, row | slot, field, attempt), so a bound can be built AROUND the candidate v0
that attempt 0 will offer:

* craft_bound(v0, bits, d, accept): bit_length(u) == bits (the top bit of v0 is set: nw, nb and the mask stay what v0 was computed
  with), u == v0 in every lane above lane d, u differs from v0 in word 7 of lane d (neither the first nor the last word of the lane),
  upward for "accepted at attempt 0", downward for "rejected at attempt 0", and everything below that word says the opposite (zeros under
  an accepted v0, ones under a rejected one), so a kernel that lets a lower lane or a lower word win gets the case wrong.
* craft_third(s, G, lanes): third with bit_length 32 kw - 2 (range = 3 third + k fits kw words), third > s decided in the top lane, and
  the sum of every lower lane chosen: a generate, an exact 2^512, all ones (propagate), 2^512 - 2 (one short of propagating), or low words
  of all ones that a carry-in ripples through.

The rows (and, where a batch has no fitting row, the first_index) are found by a deterministic search; nothing is skipped.  The sampler
reads n only as a bound, so these bounds need not be Paillier keys.  The exhaustion of all 128 attempts is not reachable by any input one
can construct (an attempt accepts with probability >= 1/2, independently) and is not simulated."""
import functools

import seeded_cases as RC
import seeded_model as R
import seeded_nonce_cases as NC
import seeded_nonce_model as N
from helpers import pm

RANGE_SEED = RC.SEED
NONCE_SEED = NC.SEED
WIDTHS = (1024, 2048, 4096)
LANE = 512
LANE_MASK = (1 << LANE) - 1
M32 = 0xFFFFFFFF
MESSAGE_K = 8               # z_sim slots 1 .. 7: a crafted slot j >= 1, and enough groups that one of them starts at lane >= 32 of its wavefront


class NoFit(Exception):
    """this candidate cannot carry the case (its top bit is clear, a word is at its limit, ...): the search goes on"""


# ---- the stream, value by value -------------------------------------------------------------------------------------------------------
def candidate(blockf, bits, t=0):
    """what attempt t of sample_below offers under a bound of `bits` bits; blockf(counter) -> the 16 words of that block"""
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    words = []
    for k in range(t * nb, (t + 1) * nb):
        words += blockf(k)
    return sum(w << (32 * i) for i, w in enumerate(words[:nw])) & ((1 << bits) - 1)


@functools.lru_cache(maxsize=None)
def range_block(counter, index, row, field):
    return tuple(R.block(RANGE_SEED, counter, index, row, field))


@functools.lru_cache(maxsize=None)
def nonce_block(counter, index, kind, slot, field):
    return tuple(N.block(NONCE_SEED, counter, index, kind, slot, field))


def range_candidate(index, row, field, bits, t=0):
    return candidate(lambda k: range_block(k, index, row, field), bits, t)


def nonce_candidate(index, kind, slot, field, bits, t=0):
    return candidate(lambda k: nonce_block(k, index, kind, slot, field), bits, t)


def range_coin(index, row):
    return range_block(0, index, row, R.FIELD_COIN)[0] & 1


def plain_bound(tag, bits):
    return pm.Drbg(b"sampler-lanes-" + tag).bits(bits) | (1 << (bits - 1)) | 1


# ---- crafting ---------------------------------------------------------------------------------------------------------------------------
def craft_bound(v0, bits, d, accept):
    if not (v0 >> (bits - 1)) & 1:
        raise NoFit("the top bit of v0 is clear: a bound that equals it above lane d would be shorter")
    w = 16 * d + 7
    assert w < (bits + 31) // 32 - 1
    vw = (v0 >> (32 * w)) & M32
    if vw == (M32 if accept else 0):
        raise NoFit("word 7 of lane d cannot move")
    u = (v0 >> (32 * (w + 1)) << (32 * (w + 1))) | ((vw + (1 if accept else -1)) << (32 * w)) | (0 if accept else (1 << (32 * w)) - 1)
    assert u.bit_length() == bits and (v0 < u) == accept and u >> (LANE * (d + 1)) == v0 >> (LANE * (d + 1))
    return u


def craft_equal(v0, bits):
    if not (v0 >> (bits - 1)) & 1:
        raise NoFit("the top bit of v0 is clear")
    return v0


def compare_cases(G):
    """every deciding lane with accept and with reject, equality, and a bound of 512 k - 3 bits, k = G - 1 (G = 2: one lane of two),
    decided in lane (k - 1) // 2"""
    k = G - 1
    return [("decide", d, a) for d in range(G) for a in (True, False)] + [("equal",), ("short", LANE * k - 3, (k - 1) // 2)]


def full_bits(G):
    return LANE * G - 5          # 32 kw - 5: the masked top limb is in play


def craft_for(case, v_of_bits, G):
    """-> the bound of `case` around the candidate v_of_bits(bits)"""
    if case[0] == "decide":
        return craft_bound(v_of_bits(full_bits(G)), full_bits(G), case[1], case[2])
    if case[0] == "equal":
        return craft_equal(v_of_bits(full_bits(G)), full_bits(G))
    return craft_bound(v_of_bits(case[1]), case[1], case[2], True)


def lanes_of(x, G):
    return [(x >> (LANE * i)) & LANE_MASK for i in range(G)]


def lane_addend(kind, s):
    """the lane of third that gives lane sum `kind` with the lane s of the sampled value"""
    if kind == "plain":                      # no carry out, not all ones
        t = LANE_MASK - (1 << 160)
        if s > t:
            raise NoFit
        return t - s
    if kind == "gen":                        # carry out, the words that remain are not all ones
        if s < 2:
            raise NoFit
        return LANE_MASK - (s >> 1)
    if kind == "zero":                       # exactly 2^512: zero words and a carry out
        if s == 0:
            raise NoFit
        return (1 << LANE) - s
    if kind == "prop":                       # all ones
        return LANE_MASK - s
    if kind == "near":                       # 2^512 - 2: with a carry-in all ones, which must not travel on
        if s > LANE_MASK - 1:
            raise NoFit
        return LANE_MASK - 1 - s
    if kind == "ripple":                     # words 0 .. 7 all ones before the carry-in, no carry out
        hi = (s >> 256) + 1
        if hi >= (1 << 256) - 1:
            raise NoFit
        return ((hi << 256) | ((1 << 256) - 1)) - s
    if kind == "top":                        # the top lane: 2^509 <= third_top < 2^510 and third_top > s_top, decided in word 7
        t = (s | (1 << 509)) + (1 << 224)
        if t >> 510:
            raise NoFit
        return t
    assert kind == "top-ripple"              # the same with words 0 .. 7 of the sum all ones
    hi = ((s >> 256) | (1 << 253)) + 1
    if hi >> 254:
        raise NoFit
    return (hi << 256) | (~s & ((1 << 256) - 1))


def carry_lanes(case, G):
    """the lane sums of a carry case, lane 0 first (the last one is the top lane)"""
    kinds = ["plain"] * (G - 1) + ["top"]
    if case[0] == "gen":                     # a generate into lane i alone; the receiving lane has words of all ones to ripple through
        i = case[1]
        kinds[i - 1] = "gen"
        kinds[i] = "ripple" if i < G - 1 else "top-ripple"
    elif case[0] == "full":                  # lane 0 sums to exactly 2^512, lanes 1 .. G - 2 propagate, the carry arrives in lane G - 1
        kinds[0] = "zero"
        for i in range(1, G - 1):
            kinds[i] = "prop"
    elif case[0] == "stopped":               # a propagate lane followed by a lane that absorbs the carry; at G = 2 no lane can both receive a
        if G == 2:                           # carry and propagate (lane 1 is the top lane, its sum is below 2^511): all ones WITHOUT a carry-in,
            kinds[0] = "prop"                # which must give lane 1 nothing
        else:
            kinds[0], kinds[1] = "gen", "prop"
    else:
        assert case[0] == "near"             # 2^512 - 2 + carry-in (at G = 2 lane 0, which has no carry-in)
        if G == 2:
            kinds[0] = "near"
        else:
            kinds[0], kinds[1] = "gen", "near"
    return kinds


def carry_cases(G):
    return [("gen", i) for i in range(1, G)] + [("full",), ("stopped",), ("near",)]


def carry_bits(G):
    return LANE * G - 2          # bit_length(third): range = 3 third + k, k < 3, fits kw words


def craft_third(s, G, kinds):
    third = sum(lane_addend(k, sl) << (LANE * i) for i, (k, sl) in enumerate(zip(kinds, lanes_of(s, G))))
    assert third.bit_length() == carry_bits(G) and s < third and third + s < 1 << (LANE * G) and 3 * third + 2 < 1 << (LANE * G)
    return third


# ---- geometry: where a group sits in its wavefront -------------------------------------------------------------------------------------
def range_task(c, b, row, field):
    return field * len(c["ranges"]) * c["ef"] + b * c["ef"] + row


def nonce_task(c, b, slot, field):
    """k_nonce_sample numbers its tasks field-major over the sample_below fields: (0, 1 per proof), (1, 1 per proof), (3, K - 1 per proof)"""
    B, K, kind = c["B"], c["K"], c["kind"]
    if kind == N.KIND_ZERO or field == 0:
        return b
    if field == 1:
        return B + b
    return 2 * B + b * (K - 1) + (slot - 1)


def g0_of(task, G):
    return (task * G) % 64


# ---- the batches ------------------------------------------------------------------------------------------------------------------------
# where the search for a first_index at which every proof of a batch has a fitting row ends when it begins at `base`: written here so that
# building the cases costs a few hundred blocks and not a few thousand (the search still runs, from there; tests/test_sampler_lane_cases.py
# pins the first_index of every batch)
START = {"range-2048-compare": (1 << 32) + 106, "range-1024-carry": 1001, "range-2048-carry": 1267, "range-4096-carry": 2394,
         "zero-1024": (1 << 32) + 1011, "zero-2048": (1 << 32) + 1031, "zero-4096": (1 << 32) + 1157,
         "ciphertext-1024": (1 << 32) + 2007, "ciphertext-2048": (1 << 32) + 2017, "ciphertext-4096": (1 << 32) + 2029}


def _search(name, base, build):
    for first_index in range(START.get(name, base), base + (1 << 16)):
        try:
            return build(first_index)
        except NoFit:
            continue
    raise AssertionError(name + ": no first_index fits")


def first_fit(candidates, make):
    for cand in candidates:
        try:
            return cand, make(cand)
        except NoFit:
            continue
    raise NoFit


def _range_compare(n_bits):
    """B = G + 1 proofs, ef = 3: proof b has case b crafted into its n (fields 1 / 2) and case b + G + 1 into its third (field 0)"""
    G, kw, ef = n_bits // LANE, n_bits // 32, 3
    cases = compare_cases(G)
    B = len(cases) // 2

    def build(first_index):
        n_list, ranges, targets = [], [], []
        for b in range(B):
            index = first_index + b
            spots = [(row, f) for f in ((1, 2) if b % 2 == 0 else (2, 1)) for row in range(ef)]
            (row, f), n = first_fit(spots, lambda s: craft_for(cases[b], lambda bits: range_candidate(index, s[0], s[1], bits), G))
            targets.append(dict(b=b, row=row, field=f, case=cases[b]))
            row, third = first_fit(range(ef), lambda r: craft_for(cases[b + B], lambda bits: range_candidate(index, r, 0, bits), G))
            targets.append(dict(b=b, row=row, field=0, case=cases[b + B]))
            n_list.append(n); ranges.append(3 * third + b % 3)
        c = dict(n_bits=n_bits, n_list=n_list, ranges=ranges, ef=ef, first_index=first_index, device=n_bits == 4096, targets=targets)
        if not any(g0_of(range_task(c, t["b"], t["row"], t["field"]), G) >= 32 for t in targets):
            raise NoFit
        return c
    return _search("range-%d-compare" % n_bits, (1 << 32) + 100, build)


def _carry_target(index, ef, G, case, want_coin):
    def make(row):
        if range_coin(index, row) != want_coin:
            raise NoFit
        return craft_third(range_candidate(index, row, 0, carry_bits(G)), G, carry_lanes(case, G))
    return first_fit(range(ef), make)


def _range_carry(n_bits):
    """2 (G + 2) proofs under one n: every carry case with the coin of its row 0 and 1.  ef = 2 (3 at G = 2, so that field 0 passes lane 32)"""
    G, ef = n_bits // LANE, 3 if n_bits == 1024 else 2
    cases = [(c, coin) for c in carry_cases(G) for coin in (0, 1)]

    def build(first_index):
        ranges, targets = [], []
        for b, (case, coin) in enumerate(cases):
            row, third = _carry_target(first_index + b, ef, G, case, coin)
            targets.append(dict(b=b, row=row, field=0, case=case, coin=coin))
            ranges.append(3 * third + b % 3)
        return dict(n_bits=n_bits, n_list=[plain_bound(b"carry-n-%d" % n_bits, full_bits(G))], ranges=ranges, ef=ef, first_index=first_index,
                    device=n_bits == 4096, targets=targets)
    return _search("range-%d-carry" % n_bits, 1000, build)


def _range_one(n_bits):
    """B = 1, ef = 3: the groups of all three fields in ONE wavefront, the full carry chain in a row of field 0"""
    G = n_bits // LANE

    def build(first_index):
        row, third = first_fit(range(3), lambda r: craft_third(range_candidate(first_index, r, 0, carry_bits(G)), G, carry_lanes(("full",), G)))
        return dict(n_bits=n_bits, n_list=[plain_bound(b"one-n-%d" % n_bits, full_bits(G))], ranges=[3 * third + 2], ef=3, first_index=first_index,
                    device=False, targets=[dict(b=0, row=row, field=0, case=("full",))])
    return _search("range-%d-one" % n_bits, 7, build)


def _range_five(n_bits):
    """B = 5, ef = 3, per-proof bounds of different lengths, an empty interval (range = 2) as proof 2: the field boundaries fall inside a
    wavefront, the groups of the dead proof sit among live ones, and the groups of one wavefront run with different bits / nb"""
    G, ef = n_bits // LANE, 3
    short = compare_cases(G)[-1]

    def build(first_index):
        r0, t0 = first_fit(range(ef), lambda r: craft_third(range_candidate(first_index, r, 0, carry_bits(G)), G, carry_lanes(("stopped",), G)))
        r3, t3 = first_fit(range(ef), lambda r: craft_for(short, lambda bits: range_candidate(first_index + 3, r, 0, bits), G))
        r4, t4 = first_fit(range(ef), lambda r: craft_third(range_candidate(first_index + 4, r, 0, carry_bits(G)), G, carry_lanes(("gen", G - 1), G)))
        n_list = [plain_bound(b"five-n0-%d" % n_bits, full_bits(G)), (1 << (LANE * G - 8)) + 1, plain_bound(b"five-n2-%d" % n_bits, full_bits(G)),
                  plain_bound(b"five-n3-%d" % n_bits, short[1]), 5]
        return dict(n_bits=n_bits, n_list=n_list, ranges=[3 * t0, RC._rng(b"five-%d" % n_bits, 256), 2, 3 * t3 + 1, 3 * t4 + 2], ef=ef,
                    first_index=first_index, device=False,
                    targets=[dict(b=0, row=r0, field=0, case=("stopped",)), dict(b=3, row=r3, field=0, case=short), dict(b=4, row=r4, field=0, case=("gen", G - 1))])
    return _search("range-%d-five" % n_bits, NC.BIG, build)


@functools.lru_cache(maxsize=None)
def range_cases():
    """name -> dict(n_bits, n_list (one = shared), ranges, ef, first_index, device, targets): the keys of seeded_cases.sampler_cases(),
    and `targets`, the (proof, row, field) each crafted bound was built around"""
    out = {}
    for n_bits in WIDTHS:
        out["range-%d-compare" % n_bits] = _range_compare(n_bits)
        out["range-%d-carry" % n_bits] = _range_carry(n_bits)
        out["range-%d-one" % n_bits] = _range_one(n_bits)
        out["range-%d-five" % n_bits] = _range_five(n_bits)
    return out


NONCE_KINDS = ((N.KIND_ZERO, "zero"), (N.KIND_CIPHERTEXT, "ciphertext"), (N.KIND_CORRECT_MESSAGE, "message"))


def _nonce_batch(kind, tag, n_bits, cases):
    """one proof per case, its n crafted around: Zero slot 0 field 0 | Ciphertext field 1 | a CorrectMessage z_sim slot j >= 1 (K = 8, the
    highest slot that fits, and one of the batch's crafted groups at lane >= 32 of its wavefront)"""
    G = n_bits // LANE
    K = MESSAGE_K if kind == N.KIND_CORRECT_MESSAGE else 1
    spots = {N.KIND_ZERO: [(0, 0)], N.KIND_CIPHERTEXT: [(0, 1)], N.KIND_CORRECT_MESSAGE: [(j, 3) for j in range(K - 1, 0, -1)]}[kind]

    def build(first_index):
        n_list, targets = [], []
        for b, case in enumerate(cases):
            (slot, f), n = first_fit(spots, lambda s: craft_for(case, lambda bits: nonce_candidate(first_index + b, kind, s[0], s[1], bits), G))
            n_list.append(n); targets.append(dict(b=b, slot=slot, field=f, case=case))
        c = dict(kind=kind, n_bits=n_bits, n_list=n_list, B=len(cases), K=K, first_index=first_index, device=n_bits == 4096, targets=targets)
        if kind == N.KIND_CORRECT_MESSAGE and not any(g0_of(nonce_task(c, t["b"], t["slot"], t["field"]), G) >= 32 for t in targets):
            raise NoFit
        return c
    return _search("%s-%d" % (tag, n_bits), NC.BIG + 1000 * kind, build)


@functools.lru_cache(maxsize=None)
def nonce_cases():
    """name -> dict(kind, n_bits, n_list (one per proof), B, K, first_index, device, targets): the keys of seeded_nonce_cases.sampler_cases().
    The 2 G + 2 comparison cases of a width go round the three kinds."""
    out = {}
    for n_bits in WIDTHS:
        cases = compare_cases(n_bits // LANE)
        for k, (kind, tag) in enumerate(NONCE_KINDS):
            out["%s-%d" % (tag, n_bits)] = _nonce_batch(kind, tag, n_bits, cases[k::3])
    return out


@functools.lru_cache(maxsize=None)
def model_witness(name):
    c = range_cases()[name]
    return R.witness(RANGE_SEED, c["first_index"], c["n_list"], c["ranges"], c["ef"])


@functools.lru_cache(maxsize=None)
def model_nonces(name):
    c = nonce_cases()[name]
    return N.nonces(c["kind"], NONCE_SEED, c["first_index"], c["n_list"], c["B"], c["K"])


# ---- the coverage table: what the cases reach, by the value-level models and plain integers alone ------------------------------------------
def compare_cells(v0, u, G):
    """the cells one (candidate of attempt 0, bound) pair fills.  A deciding lane counts only when the deciding WORD is neither the first nor
    the last of its lane and everything below that word says the opposite — the way craft_bound builds it, and what a random bound never
    gives (there the top word differs)."""
    bits = u.bit_length()
    if v0 == u:
        return {"equal"} if bits > LANE * (G - 1) else set()          # (every lane occupied: not the 5 == 5 of a three-bit bound)
    w = ((v0 ^ u).bit_length() - 1) // 32
    d, accept = w // 16, v0 < u
    low = (1 << (32 * w)) - 1
    if w % 16 in (0, 15) or (v0 & low) == (u & low) or ((v0 & low) > (u & low)) != accept:
        return set()
    cells = {("decide", d, "accept" if accept else "reject")} if bits > LANE * (G - 1) else set()
    top = (bits - 1) // LANE
    if bits <= LANE * (G - 1) and (d < top or top == 0):          # nb < G: the idle lanes hold zeros on both sides
        cells.add("short")
    return cells


def carry_cells(third, s, G, coin):
    """the cells a = third + s fills: per lane the sum before the carry-in, generate, propagate, and the carry-in the integers give"""
    pre = [a + b for a, b in zip(lanes_of(third, G), lanes_of(s, G))]
    gen = [p >> LANE for p in pre]
    prop = [(p & LANE_MASK) == LANE_MASK for p in pre]
    cin = [((third & ((1 << (LANE * i)) - 1)) + (s & ((1 << (LANE * i)) - 1))) >> (LANE * i) for i in range(G)] + [0]
    cells = set()
    if sum(cin) == 1:
        i = cin.index(1)
        if gen[i - 1]:
            cells.add(("gen", i, coin))
    if pre[0] == 1 << LANE and all(prop[1:G - 1]) and cin[:G] == [0] + [1] * (G - 1):
        cells.add(("full", coin))
    if G == 2:
        if prop[0] and cin[:2] == [0, 0]:
            cells.add(("stopped", coin))
        if pre[0] == LANE_MASK - 1 and cin[1] == 0:
            cells.add(("near", coin))
    for i in range(1, G - 1):
        if prop[i] and cin[i] and cin[i + 1] and not gen[i + 1] and not prop[i + 1] and not cin[i + 2]:
            cells.add(("stopped", coin))
        if pre[i] == LANE_MASK - 1 and cin[i] and not cin[i + 1]:
            cells.add(("near", coin))
    for i in range(1, G):
        if cin[i] and pre[i] & ((1 << 64) - 1) == (1 << 64) - 1 and not prop[i]:          # the carry-in crosses words inside the lane
            cells.add(("ripple", coin))
    return cells, cin[:G]


def _wave_cells(groups, G, kernel):
    """groups: (task, field, alive, nb, crafted comparison, carried) -> the cells that are about a wavefront"""
    cells, waves = set(), {}
    for g in groups:
        waves.setdefault(g[0] * G // 64, []).append(g)
        if g[2] and g0_of(g[0], G) >= 32:
            if g[4]:
                cells.add("g0>=32-compare")
            if g[5]:
                cells.add("g0>=32-carry")
    for w in waves.values():
        live = [g for g in w if g[2]]
        fields = {g[1] for g in live}
        marked = any(g[5] for g in live) if kernel == "range" else any(g[4] for g in live)
        if len(fields) >= 2 and marked:
            cells.add("mixed-field-wave")
        if len(fields) == 3 and marked:
            cells.add("all-fields-wave")
        if len({g[3] for g in live}) >= 2:
            cells.add("mixed-nb-wave")
        if live and len(live) < len(w):
            cells.add("dead-among-live")
    return cells


def _nb(u):
    return ((u.bit_length() + 31) // 32 + 15) // 16


def range_coverage(name):
    """the cells of one range batch"""
    c = range_cases()[name]
    G = c["n_bits"] // LANE
    wit, status, _, _ = model_witness(name)
    cells, groups = set(), []
    for b, rng in enumerate(c["ranges"]):
        n = c["n_list"][0] if len(c["n_list"]) == 1 else c["n_list"][b]
        third, index = rng // 3, c["first_index"] + b
        for row in range(c["ef"]):
            for f in range(3):
                task = range_task(c, b, row, f)
                if status[b]:
                    groups.append((task, f, False, 0, False, False))
                    continue
                u = n if f else third
                cmp_cells = compare_cells(range_candidate(index, row, f, u.bit_length()), u, G)
                carried = False
                if f == 0:
                    w1, w2 = wit["w1"][b][row], wit["w2"][b][row]
                    cc, cin = carry_cells(third, min(w1, w2), G, int(w1 < w2))
                    cells |= cc
                    carried = any(cin)
                cells |= cmp_cells
                groups.append((task, f, True, _nb(u), bool(cmp_cells), carried))
    return cells | _wave_cells(groups, G, "range")


def nonce_coverage(name):
    """the cells of one nonce batch; ("kind", kind, field) where a crafted comparison sits in that kind's field"""
    c = nonce_cases()[name]
    G, kind = c["n_bits"] // LANE, c["kind"]
    cells, groups = set(), []
    for b, n in enumerate(c["n_list"]):
        for slot, f, _, _, below in N.fields_of(kind, c["K"]):
            if not below:
                continue
            cmp_cells = compare_cells(nonce_candidate(c["first_index"] + b, kind, slot, f, n.bit_length()), n, G)
            cells |= cmp_cells
            if cmp_cells and (slot >= 1 or kind != N.KIND_CORRECT_MESSAGE):
                cells.add(("kind", kind, f))
            groups.append((nonce_task(c, b, slot, f), f, True, _nb(n), bool(cmp_cells), False))
    return cells | _wave_cells(groups, G, "nonce")


def required_cells(kernel, G):
    cells = {("decide", d, a) for d in range(G) for a in ("accept", "reject")} | {"equal", "short", "mixed-field-wave", "mixed-nb-wave", "g0>=32-compare"}
    if kernel == "range":
        cells |= {(k, coin) for k in ("full", "stopped", "near", "ripple") for coin in (0, 1)} | {("gen", i, coin) for i in range(1, G) for coin in (0, 1)}
        cells |= {"all-fields-wave", "dead-among-live", "g0>=32-carry"}
    else:
        cells |= {("kind", N.KIND_ZERO, 0), ("kind", N.KIND_CIPHERTEXT, 1), ("kind", N.KIND_CORRECT_MESSAGE, 3)}
    return cells
