"""The group logic of k_range_sample<G> and k_nonce_sample<G> (csrc/kernels_sample.hpp) restated word for word in Python, and only that:
per lane a 16-word compare -> the `ne` / `lt` ballots -> the most significant lane that differs; per lane a 16-word sum -> the generate /
propagate ballots -> the one-addition lookahead -> the ripple of the carry-in inside the lane.  It works on lists of lanes (16 words each)
with the group's place in its wavefront, g0, as a parameter, in the tradition of tests/test_lane_model.py and tools/wbgcd_model.py.

It is NOT the definition (tests/seeded_model.py and tests/seeded_nonce_model.py are, on plain integers): tests/test_sampler_lane_cases.py
holds it to them on every sampler case, and uses its four mutants to show which inputs can tell a wrong group logic from the right one.

Mutants: "cin0" (no carry crosses a lane), "gen-only" (cin = gen << 1: a carry crosses one lane but is not propagated), "top-lane" (the top
occupied lane alone decides the comparison), "accept-equal" (v == u is accepted)."""
import functools

import seeded_model as R
import seeded_nonce_model as N

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
MUTANTS = ("cin0", "gen-only", "top-lane", "accept-equal")
NOISE = 0x9E3779B97F4A7C15          # what the other groups of the wavefront put into a ballot: any bits outside [g0, g0 + G)


@functools.lru_cache(maxsize=None)
def _range_block(seed, counter, index, row, field):
    return tuple(R.block(seed, counter, index, row, field))


@functools.lru_cache(maxsize=None)
def _nonce_block(seed, counter, index, kind, slot, field):
    return tuple(N.block(seed, counter, index, kind, slot, field))


def to_lanes(x, G):
    return [[(x >> (512 * l + 32 * i)) & M32 for i in range(16)] for l in range(G)]


def from_lanes(lanes):
    return sum(w << (512 * l + 32 * i) for l, lane in enumerate(lanes) for i, w in enumerate(lane))


def clz32(m):
    return 32 - m.bit_length()


def ballot(bits_of_group, g0, G):
    """the 64-bit ballot of a wavefront in which this group's lanes are bits [g0, g0 + G) and the others hold noise"""
    mine = sum(1 << (g0 + l) for l, bit in enumerate(bits_of_group) if bit)
    return (NOISE & ~(((1 << G) - 1) << g0) & M64) | mine


def lane_compare(v, uw):
    c = 0
    for i in range(15, -1, -1):
        if c == 0 and v[i] != uw[i]:
            c = -1 if v[i] < uw[i] else 1
    return c


def group_less(v_lanes, u_lanes, g0, G, nb, mutant=None):
    """lines 88-95 / 231-238: is the value of the group below the bound?"""
    GM = (1 << G) - 1
    c = [lane_compare(v, uw) for v, uw in zip(v_lanes, u_lanes)]
    if mutant == "top-lane":
        return c[nb - 1] < 0
    ne, lt = ballot([x != 0 for x in c], g0, G), ballot([x < 0 for x in c], g0, G)
    ok = mutant == "accept-equal"
    m = (ne >> g0) & GM
    if m:
        ok = (lt >> (g0 + (31 - clz32(m)))) & 1 != 0
    return ok


def group_add(v_lanes, u_lanes, g0, G, mutant=None):
    """lines 110-122: the lanes of v + u"""
    GM = (1 << G) - 1
    sums, carries, ones = [], [], []
    for v, uw in zip(v_lanes, u_lanes):
        s, carry, all_ones = [0] * 16, 0, True
        for i in range(16):
            x = v[i] + uw[i] + carry
            s[i] = x & M32; carry = x >> 32
            all_ones = all_ones and s[i] == M32
        sums.append(s); carries.append(carry != 0); ones.append(all_ones)
    gen, prop = (ballot(carries, g0, G) >> g0) & GM, (ballot(ones, g0, G) >> g0) & GM
    for l, s in enumerate(sums):
        cin = ((((gen << 1) + prop) ^ prop) >> l) & 1
        if mutant == "cin0":
            cin = 0
        elif mutant == "gen-only":
            cin = ((gen << 1) >> l) & 1
        for i in range(16):
            s[i] = (s[i] + cin) & M32
            cin = 1 if cin and s[i] == 0 else 0
    return sums


def sample_below_lanes(blockf, u, G, g0, mutant=None):
    """the attempt loop of one group (lines 68-98) -> (the lanes of the accepted value, rejected attempts) or (None, 128).
    blockf(counter) -> the 16 words of that block of the group's stream"""
    bits = u.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    topmask = (1 << (bits & 31)) - 1 if bits & 31 else M32
    u_lanes = to_lanes(u, G)
    v = [[0] * 16 for _ in range(G)]
    for t in range(R.MAX_ATTEMPTS):
        for l in range(nb):
            v[l] = list(blockf(t * nb + l))
            for i in range(16):
                wi = 16 * l + i
                if wi >= nw:
                    v[l][i] = 0
                elif wi == nw - 1:
                    v[l][i] &= topmask
        if group_less(v, u_lanes, g0, G, nb, mutant):
            return v, t
    return None, R.MAX_ATTEMPTS


def witness(seed, first_index, n_list, range_list, ef, G, mutant=None):
    """seeded_model.witness through the lanes, every group at the place k_range_sample gives it (tasks field-major, G lanes each)"""
    B = len(range_list)
    out = {f: [[0] * ef for _ in range(B)] for f in ("w1", "w2", "r1", "r2")}
    status, rejected, worst = [0] * B, 0, 0
    for b in range(B):
        n = n_list[0] if len(n_list) == 1 else n_list[b]
        third = range_list[b] // 3
        if third == 0 or n == 0:
            status[b] = R.MALFORMED
            continue
        index = first_index + b
        rows = []
        for row in range(ef):
            vals = []
            for f, u in ((0, third), (1, n), (2, n)):
                g0 = ((f * B * ef + b * ef + row) * G) % 64
                v, k = sample_below_lanes(lambda ctr: _range_block(seed, ctr, index, row, f), u, G, g0, mutant)
                rejected += k; worst = max(worst, k)
                vals.append((v, g0))
            rows.append(vals)
        if any(v is None for vals in rows for v, _ in vals):
            status[b] = R.MALFORMED
            continue
        for row, ((s, g0), (r1, _), (r2, _)) in enumerate(rows):
            a = from_lanes(group_add(s, to_lanes(third, G), g0, G, mutant))
            s = from_lanes(s)
            coin = _range_block(seed, 0, index, row, R.FIELD_COIN)[0] & 1
            out["w1"][b][row], out["w2"][b][row] = (s, a) if coin else (a, s)
            out["r1"][b][row], out["r2"][b][row] = from_lanes(r1), from_lanes(r2)
    return out, status, rejected, worst


def nonces(kind, seed, first_index, n_list, B, K, G, mutant=None):
    """seeded_nonce_model.nonces through the lanes, every sample_below group at the place k_nonce_sample gives it"""
    out, status, rejected = [], [0] * B, [0] * B
    for b in range(B):
        n = None if kind == N.KIND_DLOG else (n_list[0] if len(n_list) == 1 else n_list[b])
        index = first_index + b
        d = {"e_sim": [0] * (K - 1), "z_sim": [0] * (K - 1)} if kind == N.KIND_CORRECT_MESSAGE else {}
        bad = n == 0
        for slot, field, name, j, below in N.fields_of(kind, K):
            if bad:
                v = 0
            elif below:
                task = b if field == 0 else B + b if field == 1 else 2 * B + b * (K - 1) + slot - 1
                v, k = sample_below_lanes(lambda ctr: _nonce_block(seed, ctr, index, kind, slot, field), n, G, (task * G) % 64, mutant)
                rejected[b] += k
                bad = v is None
                v = 0 if bad else from_lanes(v)
            else:
                v = N.raw_bits(seed, index, kind, slot, field, 16 if kind == N.KIND_DLOG else 8)
            if j is None:
                d[name] = v
            else:
                d[name][j] = v
        if bad:
            status[b] = N.MALFORMED
            d = {k: ([0] * len(v) if isinstance(v, list) else 0) for k, v in d.items()}
        out.append(d)
    return out, status, rejected
