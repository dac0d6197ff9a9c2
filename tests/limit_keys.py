"""Keys at the digit-sum limit of the FAST Montgomery product (bigint29.hpp "column capacity").

At 36 limbs per lane a 64-bit column takes 72 products of 29-bit limbs and is exact only while every lane's limb sum of the key's Orup
multiple M~ = n * n1 (n1 = -n^-1 mod 2^29) stays within a limit: COL_FAST_SN_LIMIT for the modexp kernels (k_setup), COL_FAST_SN_LIMIT_BN
for the base-n Paillier kernels (k_setup_basen).  A random key has a mean limb of 0.5 * 2^29 and the limits sit near 0.75 * 2^29, so no
random key comes near them; `limit_key` builds keys whose M~ has chosen lane sums, with a full-width n1, so that the ladder's operands fill
the top limbs as well (tests/test_gpu_soak.py limit_modulus is the n1 = 1 case: M~ = M, 29 bits shorter).

Construction: pick an odd n1; write the target T = M~ limb by limb (limb 0 = 2^29 - 1: T == -1 mod 2^29; the top limb inside
[n1 2^(n_bits - 1), n1 2^n_bits)); hold two limbs of one lane back for the values k and 2^29 - 1 - k, k solved from T == 0 (mod n1) — the
lane's sum does not depend on k; then n = T / n1 is odd, has n_bits bits, and -n^-1 mod 2^29 = n1."""
import math
import random

LB = 29
MASK = (1 << LB) - 1


def fast_sn_limit(W=36):
    """bigint29.hpp COL_FAST_SN_LIMIT"""
    return ((1 << 64) - 1 - (1 << 36) - ((1 << LB) + 16) * (W * (1 << LB) + 16)) >> LB


def sn_limit_basen(W=36):
    """kernels_basen.hpp COL_FAST_SN_LIMIT_BN"""
    return ((1 << 64) - 1 - (1 << 36) - ((1 << LB) + 16) * (W * (1 << LB) + 16) - (1 << (2 * LB)) - (1 << LB)) >> LB


def orup(n):
    """(n1, M~) of an odd n"""
    n1 = (-pow(n, -1, 1 << LB)) % (1 << LB)
    return n1, n * n1


def lane_sums(x, W, lanes):
    """limb sums of x over `lanes` blocks of W limbs"""
    assert x >> (LB * W * lanes) == 0
    return [sum((x >> (LB * i)) & MASK for i in range(j * W, (j + 1) * W)) for j in range(lanes)]


def limit_key(n_bits, W, lane_deltas, limit, rnd, n1=None):
    """odd n of exactly n_bits bits whose Orup multiple M~ = n * n1 has, over lane j (limbs [j W, (j + 1) W)), the limb sum
    limit + lane_deltas[j]; lanes given as None get random limbs.  len(lane_deltas) lanes hold M~.  n1: an odd value below 2^29 (default:
    random with the top bit set, so that M~ has n_bits + 29 bits); n1 = 1 gives M~ = n."""
    G = len(lane_deltas)
    L = G * W
    if n1 is None:
        n1 = rnd.getrandbits(LB) | (1 << (LB - 1)) | 1
    assert n1 & 1 and 0 < n1 <= MASK
    lo_bound, hi_bound = n1 << (n_bits - 1), n1 << n_bits           # n1 2^(n_bits - 1) <= T < n1 2^n_bits  <=>  n has n_bits bits
    assert hi_bound <= 1 << (LB * L), "M~ does not fit the lanes"
    limbs = [rnd.getrandbits(LB) for _ in range(L)]
    # the top limb: the largest index t with a value v such that [v, v + 1) 2^(29 t) lies inside the bounds whatever the limbs below are
    t = ((hi_bound - 1).bit_length() - 1) // LB
    while True:
        v_lo, v_hi = -((-lo_bound) >> (LB * t)), min(MASK, (hi_bound >> (LB * t)) - 1)
        if v_lo <= v_hi:
            break
        t -= 1
    for i in range(t + 1, L):
        limbs[i] = 0
    limbs[t] = rnd.randint(v_lo, v_hi)
    limbs[0] = MASK
    fixed = set([0] + list(range(t, L)))
    # the lane that solves the congruence: the last constrained one (lane 0 when there is none), two of its free limbs held back
    jc = max([j for j, d in enumerate(lane_deltas) if d is not None], default=0)
    free_c = [i for i in range(jc * W, (jc + 1) * W) if i not in fixed]
    pair = None
    for a in range(len(free_c)):
        for b in range(a + 1, len(free_c)):
            coef = (pow(2, LB * free_c[a], n1) - pow(2, LB * free_c[b], n1)) % n1
            if math.gcd(coef, n1) == 1:
                pair = (free_c[a], free_c[b])
                break
        if pair:
            break
    assert pair, "no two limbs of the lane solve T == 0 (mod n1) for this n1"
    fix, comp = pair
    for j, delta in enumerate(lane_deltas):
        if delta is None:
            continue
        lane = range(j * W, (j + 1) * W)
        body = [i for i in lane if i not in fixed and i not in pair]
        want = limit + delta - sum(limbs[i] for i in lane if i in fixed) - (MASK if j == jc else 0)
        assert 0 <= want <= len(body) * MASK, f"lane {j}: the target digit sum is out of reach"
        full, part = divmod(want, MASK)
        vals = [MASK] * full + ([part] if full < len(body) else []) + [0] * (len(body) - full - 1)
        assert len(vals) == len(body) and sum(vals) == want
        rnd.shuffle(vals)
        for i, v in zip(body, vals):
            limbs[i] = v
    # k at `fix`, 2^29 - 1 - k at `comp`:  T0 + k (B^fix - B^comp) == 0 (mod n1), T0 holding 0 at fix and 2^29 - 1 at comp
    limbs[fix], limbs[comp] = 0, MASK
    T0 = sum(v << (LB * i) for i, v in enumerate(limbs))
    coef = (pow(2, LB * fix, n1) - pow(2, LB * comp, n1)) % n1
    k = (-T0) * pow(coef, -1, n1) % n1
    assert 0 <= k <= MASK
    limbs[fix], limbs[comp] = k, MASK - k
    T = sum(v << (LB * i) for i, v in enumerate(limbs))
    # postconditions
    assert T % n1 == 0
    n = T // n1
    assert n & 1 and n.bit_length() == n_bits
    assert orup(n) == (n1, T)
    sums = lane_sums(T, W, G)
    for j, delta in enumerate(lane_deltas):
        assert delta is None or sums[j] == limit + delta, (j, delta, sums[j] - limit)
    return n


DELTAS = (-1, 0, 1, 1 << 20, -(1 << 20))
_KEY_SETS = {}


def guard_key_set(n_bits):
    """[(name, lane deltas, n)], the keys of tests/test_gpu_basen_limit.py: lane j of M~ (36 limbs per lane) at COL_FAST_SN_LIMIT_BN + delta
    for every lane and every delta of DELTAS, the other lanes random; every lane at the limit; every lane at the limit but the last at + 1"""
    if n_bits not in _KEY_SETS:
        G = n_bits // 1024
        rnd = random.Random(n_bits * 31)
        lim = sn_limit_basen(36)
        shapes = [(f"lane {j} at {d:+d}", [d if i == j else None for i in range(G)]) for j in range(G) for d in DELTAS]
        shapes.append(("every lane at the limit", [0] * G))
        shapes.append(("every lane at the limit, the last at +1", [0] * (G - 1) + [1]))
        _KEY_SETS[n_bits] = [(name, deltas, limit_key(n_bits, 36, deltas, lim, rnd)) for name, deltas in shapes]
    return _KEY_SETS[n_bits]


def qualifies(n, n_bits, W):
    """k_setup_basen's digit-sum test as the engine of W limbs per lane states it: every lane's limb sum of M~ within that engine's limit"""
    L = 72 * (n_bits // 2048)
    return all(s <= sn_limit_basen(W) for s in lane_sums(orup(n)[1], W, L // W))


def worst_operands(Mt):
    """pairs (a, b) at the bounds the base-n ladder keeps (a < 2 M~, b < 4 M~): the bounds themselves; the largest values within them whose
    limbs below the top one are all 2^29 - 1; and each part alone"""
    def all_max(bound):
        sh = LB * ((bound.bit_length() - 1) // LB)
        x = bound if (bound + 1) & ((1 << sh) - 1) == 0 else ((bound >> sh) << sh) - 1
        assert x <= bound and all((x >> (LB * i)) & MASK == MASK for i in range(sh // LB))
        return x
    ta, tb = 2 * Mt - 1, 4 * Mt - 1
    return [(ta, tb), (all_max(ta), all_max(tb)), (0, tb), (ta, 0)]
