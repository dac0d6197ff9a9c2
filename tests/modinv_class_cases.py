"""Case builder for zkp_modinv_batch in every finalisation class of k_modinv (csrc/kernels_inv.hpp) that a search has reached: the
vectors of tests/golden/modinv_classes.json (minted by tests/golden/make_modinv_classes.py, which imports the decoders below), laid
out in the batches tests/test_gpu_modinv_classes.py runs.  tests/test_modinv_class_cases.py holds every claim made here to the Python
model of the kernel (tools/wbgcd_model.py), to the C oracle and to pow(a, -1, M).

The fixture stores descriptors, not operands:
  modulus  {"hex": ...}  or  {"bits": L, "tag": t}: M = Drbg(t).bits(L) with bit L - 1 and bit 0 set
  value    {"hex": ...}, {"m_minus": r}: a = M - r,  or  {"tag": t}: a = Drbg(t).below(M)
and, per vector, what the model said of it when it was minted (CLASS_KEYS): the class of the cofactor v before the finalisation, the
number of finalisation passes, the rounds, whether a / b was negated in some round, whether the sign word of u or v held magnitude,
whether the run started in / crossed into the n <= 64 branch.  "small" vectors (operands of 34 ... 90 bits, zero padded) serve every
field width; "wide" vectors belong to one.

Layout.  launch_modinv runs 16 items per block in thread-interleaved LDS, each lane with its own trip count.  Every block that holds a
`below_neg_m` vector also holds the lanes of COMPANIONS: one that leaves at the domain check, one that leaves at a == 0, one that runs
the whole GCD and ends without an inverse, one under a tiny modulus that is done in a few rounds and one full-length inverse
(placement_problems() checks it).  Per field width:
  per_item   71 items under per-item moduli: the rare vectors in the first blocks, two to a block, every other vector of the
             fixture around them; four full blocks and a partial one of 7
  rare_last  75 items: four full blocks of everything else, then the rare vectors and their companions alone in the partial block of 11
  shared     (8192 bits) 39 items under ONE full-width modulus, mod_stride = 0: rare vectors in the first block and in the partial last
             one.  No lane can have a tiny modulus there; the other four companions are present."""
import json
import math
import os

import numpy as np

import helpers as H
from helpers import pm, L, zkp

FIXTURE = os.path.join(H.ROOT, "tests", "golden", "modinv_classes.json")
WIDTHS = (2048, 4096, 8192)
BLOCK = 16                     # items per block of k_modinv (launch_modinv: lanes = 16 at every field width)
CLASS_KEYS = ("v_class", "final_passes", "rounds", "neg_a", "neg_b", "signword", "start_le64", "cross_le64")
COMPANIONS = ("domain", "none_early", "none_late", "tiny", "full")
RARE = "below_neg_m"

_CACHE = {}


def modulus_of(d):
    if "hex" in d:
        return int(d["hex"], 16)
    return pm.Drbg(d["tag"].encode()).bits(d["bits"]) | 1 | 1 << (d["bits"] - 1)


def value_of(d, M):
    if "hex" in d:
        return int(d["hex"], 16)
    if "m_minus" in d:
        return M - d["m_minus"]
    return pm.Drbg(d["tag"].encode()).below(M)


def summary(call):
    """the record of one model run (stats["call"] of tools/wbgcd_model.wbgcd) in the fixture's terms"""
    return dict(v_class=call["v_class"], final_passes=call["final_passes"], rounds=call["rounds"], neg_a=call["neg_a_rounds"] > 0,
                neg_b=call["neg_b_rounds"] > 0, signword=call["signword_magnitude"], start_le64=call["start_le64"], cross_le64=call["cross_le64"])


def fixture():
    if "fixture" not in _CACHE:
        _CACHE["fixture"] = json.load(open(FIXTURE))
    return _CACHE["fixture"]


def expected(a, M):
    """(status, inverse) as zkp_modinv_batch defines them: M odd and >= 3 and a < M, else DOMAIN; no inverse: NONE; zeros unless OK"""
    if M % 2 == 0 or M < 3 or a >= M:
        return zkp.INV_DOMAIN, 0
    if math.gcd(a, M) != 1:
        return zkp.INV_NONE, 0
    return zkp.INV_OK, pow(a, -1, M)


def _item(name, kind, a, M, rec=None):
    st, inv = expected(a, M)
    return dict(name=name, kind=kind, a=a, M=M, status=st, inv=inv, rec=rec)


def vectors(mod_bits):
    """the fixture's vectors of one field width: items of kind "vector" whose `rec` is the recorded model summary"""
    key = ("vectors", mod_bits)
    if key not in _CACHE:
        fx = fixture()
        out = []
        for i, v in enumerate(fx["wide"][str(mod_bits)] + fx["small"]):
            M = modulus_of(v["m"])
            out.append(_item("v%d-%s" % (i, v["v_class"]), "vector", value_of(v["a"], M), M, {k: v[k] for k in CLASS_KEYS}))
        _CACHE[key] = out
    return _CACHE[key]


def shared_modulus():
    """the 8192-bit modulus of the shared batch, a factor of it, and the r of its below_neg_m values a = M - r"""
    s = fixture()["shared_8192"]
    return modulus_of(s["m"]), s["factor"], s["rare"], s["plain"]


def _companions(mod_bits, d, salt):
    """the five lanes that go with a rare vector, fresh operands for every block"""
    full = lambda: d.bits(mod_bits) | 1 | 1 << (mod_bits - 1)
    M = full()
    f = d.bits(mod_bits // 3) | 1
    x = d.bits(mod_bits - mod_bits // 3 - 1) | 1 | 1 << (mod_bits - mod_bits // 3 - 2)
    Mf = full()
    a_full = d.below(Mf)
    while math.gcd(a_full, Mf) != 1:
        a_full = d.below(Mf)
    domain = [("a-eq-M", M, M), ("even-M", d.below(M - 1), M - 1), ("a-above-M", M + 2 * d.below(1 << 40), M - (1 << (mod_bits - 2)))][salt % 3]
    tiny = [(2, 105), (2, 3), (52, 105), (101, 255)][salt % 4]
    return [_item("domain-" + domain[0], "domain", domain[1], domain[2]),
            _item("none-a-zero", "none_early", 0, full()),
            _item("none-common-factor", "none_late", f * d.range(1 << (mod_bits - mod_bits // 3 - 3), x), f * x),
            _item("tiny-modulus", "tiny", *tiny),
            _item("full-length", "full", a_full, Mf)]


def _filler(mod_bits, d):
    M = d.bits(mod_bits) | 1 | 1 << (mod_bits - 1)
    return _item("filler", "filler", d.below(M), M)


def batches(mod_bits):
    """-> {name: (items, mod_stride)}; every fixture vector of this width is in `per_item` and in `rare_last`"""
    key = ("batches", mod_bits)
    if key in _CACHE:
        return _CACHE[key]
    kw = mod_bits // 32
    d = pm.Drbg(b"modinv-class-batches-%d" % mod_bits)
    vs = vectors(mod_bits)
    rare = [v for v in vs if v["rec"]["v_class"] == RARE]
    plain = [v for v in vs if v["rec"]["v_class"] != RARE]
    out = {}

    # per_item: the rare vectors two to a block, at different lanes in each, with the companions and the other vectors around them
    todo = list(plain)
    blocks = []
    for i in range(0, len(rare), 2):
        blk = _companions(mod_bits, d, i) + [todo.pop(0) if todo else _filler(mod_bits, d) for _ in range(BLOCK - 5 - len(rare[i:i + 2]))]
        for k, r in enumerate(rare[i:i + 2]):
            blk.insert((3 + 5 * i + 11 * k) % (len(blk) + 1), r)
        blocks.append(blk)
    while len(blocks) < 4 or todo:
        blocks.append([todo.pop(0) if todo else _filler(mod_bits, d) for _ in range(BLOCK)])
    tail = _companions(mod_bits, d, 1)[:2] + [_filler(mod_bits, d) for _ in range(5)]
    items = [it for blk in blocks for it in blk] + tail
    assert len(items) > 64 and len(items) % BLOCK == 7 and len(items) <= 104
    out["per_item"] = (items, kw)

    # rare_last: full blocks of everything else, then the rare vectors and their companions alone in the partial block
    head = list(plain) + _companions(mod_bits, d, 2)
    while len(head) < 64 or len(head) % BLOCK:
        head.append(_filler(mod_bits, d))
    last = _companions(mod_bits, d, 3)
    for k, r in enumerate(rare[:8]):
        last.insert((2 * k + 1) % (len(last) + 1), r)
    assert len(rare) <= 8 and len(last) < BLOCK
    out["rare_last"] = (head + last, kw)

    if mod_bits == 8192:
        M, f, rs, ps = shared_modulus()
        assert M % f == 0 and M.bit_length() == mod_bits and len(rs) >= 4

        def four(salt):                      # the companions a shared modulus allows
            a_full = d.below(M)
            while math.gcd(a_full, M) != 1:
                a_full = d.below(M)
            dom = M if salt % 2 == 0 else M + 2
            return [_item("domain-shared", "domain", dom, M), _item("none-a-zero", "none_early", 0, M),
                    _item("none-common-factor", "none_late", f * d.range(M // (4 * f), M // f), M), _item("full-length", "full", a_full, M)]
        r_items = [_item("shared-rare-r%d" % r, "vector", M - r, M, dict(v_class=RARE)) for r in rs]
        p_items = [_item("shared-plain-r%d" % r, "shared_plain", M - r, M) for r in ps]
        half = len(r_items) // 2
        first = four(0) + r_items[:half] + p_items
        first += [_item("filler", "filler", d.below(M), M) for _ in range(BLOCK - len(first))]
        first = first[5:] + first[:5]
        middle = [_item("filler", "filler", d.below(M), M) for _ in range(BLOCK)]
        last = r_items[half:] + four(1) + [_item("filler", "filler", d.below(M), M)]
        assert len(first) == BLOCK and len(last) < BLOCK
        out["shared"] = (first + middle + last, 0)
    _CACHE[key] = out
    return out


def placement_problems(items, shared=False):
    """every block of 16 with a below_neg_m vector in it must hold all the companion kinds (all but `tiny` under a shared modulus), and the
    companions must be what their kind says; -> list of complaints"""
    bad = []
    need = set(COMPANIONS) - ({"tiny"} if shared else set())
    width = max(it["M"].bit_length() for it in items)
    for b in range(0, len(items), BLOCK):
        blk = items[b:b + BLOCK]
        if not any(it["rec"] and it["rec"]["v_class"] == RARE for it in blk):
            continue
        missing = need - {it["kind"] for it in blk}
        if missing:
            bad.append("block %d lacks %s" % (b // BLOCK, sorted(missing)))
    for i, it in enumerate(items):
        a, M, k = it["a"], it["M"], it["kind"]
        ok = {"domain": it["status"] == zkp.INV_DOMAIN,
              "none_early": it["status"] == zkp.INV_NONE and a == 0,
              "none_late": it["status"] == zkp.INV_NONE and a.bit_length() > width - 64 and M.bit_length() > width - 64,
              "tiny": it["status"] == zkp.INV_OK and M.bit_length() <= 8,
              "full": it["status"] == zkp.INV_OK and a.bit_length() > width - 64 and M.bit_length() == width}.get(k, True)
        if not ok:
            bad.append("item %d (%s) is not a %s lane" % (i, it["name"], k))
    return bad


def arrays(items, mod_bits, mod_stride):
    """-> a, moduli, expected inverses (limb arrays) and expected status of one batch"""
    kw = mod_bits // 32
    a = L.ints_to_limbs([it["a"] for it in items], kw)
    if mod_stride:
        m = L.ints_to_limbs([it["M"] for it in items], kw)
    else:
        assert len({it["M"] for it in items}) == 1
        m = L.int_to_limbs(items[0]["M"], kw)[None, :]
    inv = L.ints_to_limbs([it["inv"] for it in items], kw)
    return a, np.ascontiguousarray(m), inv, np.array([it["status"] for it in items], np.uint8)
