#!/usr/bin/env python3
"""Mint tests/golden/modinv_classes.json (run from the repo root: python tests/golden/make_modinv_classes.py; CPU only, a few minutes).

k_modinv (csrc/kernels_inv.hpp) ends with a data-dependent loop: add M while the cofactor v is negative, subtract M while v >= M.  Which
way a run goes — and whether a round negates a or b, whether the sign word of a cofactor carries magnitude — depends on the operands,
and the interesting class (v < -M, two passes) comes up about once in a thousand targeted inputs.  This script SEARCHES for
representatives of every class with fixed seeds and writes them as descriptors (tests/modinv_class_cases.py decodes them).

The search runs on `twin`, the round loop of tools/wbgcd_model.py restated over Python integers instead of word arrays (the same
approximations, the same matrices, the same balanced correction: 30 to 100 times faster).  The twin only FINDS candidates: every vector
that is written was re-run through the word-for-word model, and what the fixture records is the model's answer, asserted equal to the
twin's.  Of every region the script prints how many candidates it tried and how many fell into each class."""
import json
import math
import os
import sys
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools"))
import modinv_class_cases as MC  # noqa: E402
import wbgcd_model as W  # noqa: E402
from helpers import pm  # noqa: E402

K, MK = W.K, W.MK
SMALL_CANDIDATES = 200000          # the least the bounded search for v >= M tries among operands of 34 ... 90 bits
R_EVEN = tuple(range(2, 130, 2))   # a = M - r


def twin(y, m, kw):
    """tools/wbgcd_model.wbgcd(y, m, kw) over integers -> the summary of MC.summary, or None when gcd(y, m) != 1"""
    a, b, u, v = y, m, 1, 0
    minv = (-pow(m, -1, 1 << K)) % (1 << K)
    half = 1 << (32 * kw - 1)
    rounds = neg_a = neg_b = 0
    signword = start = cross = False
    while a:
        n = max(a.bit_length(), b.bit_length())
        if n <= 64:
            if rounds == 0: start = True
            elif not start: cross = True
            xa, xb = a, b
        else:
            xa = ((a >> (n - 34)) << 30) | (a & MK)
            xb = ((b >> (n - 34)) << 30) | (b & MK)
        f0, g0, f1, g1 = 1, 0, 0, 1
        for _ in range(K):
            if xa & 1:
                if xa < xb: xa, xb, f0, g0, f1, g1 = xb, xa, f1, g1, f0, g0
                xa -= xb; f0 -= f1; g0 -= g1
            xa >>= 1; f1 <<= 1; g1 <<= 1
        a, b = (f0 * a + g0 * b) >> K, (f1 * a + g1 * b) >> K
        if a < 0: a, f0, g0 = -a, -f0, -g0; neg_a += 1
        if b < 0: b, f1, g1 = -b, -f1, -g1; neg_b += 1
        cu = (((f0 * u + g0 * v) & 0xFFFFFFFF) * minv) & MK
        cv = (((f1 * u + g1 * v) & 0xFFFFFFFF) * minv) & MK
        if cu >> (K - 1): cu -= 1 << K
        if cv >> (K - 1): cv -= 1 << K
        u, v = (f0 * u + g0 * v + cu * m) >> K, (f1 * u + g1 * v + cv * m) >> K
        if not (-half <= u < half and -half <= v < half): signword = True
        rounds += 1
    if b != 1:
        return None
    cls = W.v_class(v, m, kw)
    passes = 0
    while v < 0: v += m; passes += 1
    while v >= m: v -= m; passes += 1
    return dict(v_class=cls, final_passes=passes, rounds=rounds, neg_a=neg_a > 0, neg_b=neg_b > 0, signword=signword, start_le64=start, cross_le64=cross)


def model(a, M, kw):
    st = {"maxcof": 0}
    g, inv = W.wbgcd(a, M, kw, True, st)
    assert g == 1 and inv == pow(a, -1, M)
    return MC.summary(st["call"])


class Region:
    """one place of the search: counts what it visits, keeps the candidates of the classes asked for"""
    def __init__(self, name, kw):
        self.name, self.kw, self.tried, self.found, self.kept = name, kw, 0, Counter(), []

    def visit(self, m_desc, a_desc, keep=(MC.RARE, "ge_m", "ge_m_signword")):
        M = MC.modulus_of(m_desc)
        a = MC.value_of(a_desc, M)
        if not 0 < a < M or math.gcd(a, M) != 1:
            return None
        s = twin(a, M, self.kw)
        self.tried += 1
        self.found[s["v_class"]] += 1
        if s["v_class"] in keep or keep == "all":
            self.kept.append((m_desc, a_desc, s))
        return s

    def report(self):
        print("%-22s tried %7d  " % (self.name, self.tried) + "  ".join("%s %d" % (c, self.found[c]) for c in W.V_CLASSES), flush=True)
        return dict(region=self.name, tried=self.tried, **{c: self.found[c] for c in W.V_CLASSES})


def vector(m_desc, a_desc, s, kw):
    """a fixture entry: the descriptors plus the model's record, which must be the twin's"""
    M = MC.modulus_of(m_desc)
    rec = model(MC.value_of(a_desc, M), M, kw)
    assert rec == s, (rec, s)
    return dict(m=m_desc, a=a_desc, **rec)


def near(tag):
    """M minus a small random value (up to 40 bits)"""
    return {"m_minus": pm.Drbg(tag.encode()).bits(pm.Drbg((tag + "/len").encode()).bits(5) + 9)}


def search_small():
    """operands of 34 ... 90 bits: at least SMALL_CANDIDATES runs, a = M - r for small even r, M minus a small random value, random values"""
    reg = Region("small 34-90 bits", 64)
    hx = lambda v: {"hex": format(v, "x")}
    M0, a0 = 2202345323848701257, 2202345323848701167               # a 61-bit below_neg_m pair known before this search
    reg.visit(hx(M0), hx(a0))
    i = 0
    while reg.tried < SMALL_CANDIDATES:
        bits = 34 + i % 57
        M = pm.Drbg(b"mic-small-%d" % i).bits(bits) | 1 | 1 << (bits - 1)
        for r in R_EVEN[:24]:
            reg.visit(hx(M), hx(M - r))
        for k in range(4):
            reg.visit(hx(M), hx(M - near("mic-small-near-%d-%d" % (i, k))["m_minus"] % M))
            reg.visit(hx(M), hx(pm.Drbg(b"mic-small-rand-%d-%d" % (i, k)).below(M)))
        i += 1
    return reg


def search_wide(mod_bits, name, lengths, per_length, want, first=0):
    """moduli of the given bit lengths in a field of mod_bits (per length: moduli first ... first + per_length - 1): a = M - r, M minus a
    small random value; a length is left once it has given `want` hits"""
    reg = Region("%d %s" % (mod_bits, name), mod_bits // 32)
    for bits in lengths:
        have = 0
        for i in range(first, first + per_length):
            m_desc = {"bits": bits, "tag": "mic-%d-%d-%d" % (mod_bits, bits, i)}
            for r in R_EVEN:
                s = reg.visit(m_desc, {"m_minus": r})
                have += s is not None and s["v_class"] == MC.RARE
            for k in range(8):
                s = reg.visit(m_desc, near("mic-near-%d-%d-%d-%d" % (mod_bits, bits, i, k)))
                have += s is not None and s["v_class"] == MC.RARE
            if have >= want:
                break
    return reg


def search_events(mod_bits, count):
    """the common classes and the per-round events under random full-width moduli.  Random values give neither negation nor a sign
    word with magnitude often; values close to M do: a = M - (odd << j) negates a, M minus a random value of 20 ... 120 bits negates b"""
    reg = Region("%d full-width events" % mod_bits, mod_bits // 32)
    for i in range(count):
        m_desc = {"bits": mod_bits, "tag": "mic-%d-ev-m-%d" % (mod_bits, i)}
        reg.visit(m_desc, {"tag": "mic-%d-ev-a-%d" % (mod_bits, i)}, keep="all")
        for j in (5, 31, 32, 61, 64):
            reg.visit(m_desc, {"m_minus": (2 * (i % 3) + 1) << j}, keep="all")
        for k in range(6):
            reg.visit(m_desc, {"m_minus": pm.Drbg(b"mic-%d-ev-r-%d-%d" % (mod_bits, i, k)).bits(20 + 20 * k)}, keep="all")
    return reg


def search_shared(want):
    """one full-width 8192-bit modulus with a known factor and `want` below_neg_m values a = M - r under it"""
    reg = Region("8192 shared modulus", 256)
    for i in range(64):
        m_desc = {"bits": 8192, "tag": "mic-8192-shared-%d" % i}
        M = MC.modulus_of(m_desc)
        if M % 3:
            continue
        reg.kept = []
        plain = []
        for r in range(2, 4098, 2):
            s = reg.visit(m_desc, {"m_minus": r})
            if s is not None and s["v_class"] != MC.RARE and len(plain) < 2:
                plain.append(r)
            if len(reg.kept) >= want:
                return reg, dict(m=m_desc, factor=3, rare=[k[1]["m_minus"] for k in reg.kept], plain=plain)
    raise AssertionError("no shared modulus with %d below_neg_m values" % want)


def pick_common(reg, kw):
    """from the full-width runs: two vectors for each of in_range, neg, a negated, b negated, sign word with magnitude"""
    need = {"in_range": 2, "neg": 2, "neg_a": 2, "neg_b": 2, "signword": 2}
    out = []
    for m_desc, a_desc, s in reg.kept:
        hits = [k for k in need if need[k] > 0 and (s["v_class"] == k or s.get(k) is True)]
        if hits:
            for k in hits:
                need[k] -= 1
            out.append(vector(m_desc, a_desc, s, kw))
    assert not any(v > 0 for v in need.values()), need
    return out


def main():
    counts = []
    small = search_small()
    counts.append(small.report())
    rare_small = [k for k in small.kept if k[2]["v_class"] == MC.RARE]
    ge_small = [k for k in small.kept if k[2]["v_class"].startswith("ge_m")]
    # the pair known beforehand, the first hit of the search, one that starts above 64 bits and one common vector of each kind
    picked = rare_small[:2] + [k for k in rare_small[2:] if not k[2]["start_le64"]][:1] + ge_small[:2]
    reg = Region("small, common classes", 64)
    for i in range(40):
        bits = (34, 61, 64, 65, 90)[i % 5]
        M = pm.Drbg(b"mic-small-common-%d" % i).bits(bits) | 1 | 1 << (bits - 1)
        reg.visit({"hex": format(M, "x")}, {"hex": format(pm.Drbg(b"mic-small-common-a-%d" % i).below(M), "x")}, keep="all")
    for cls, start in (("in_range", True), ("neg", True), ("in_range", False), ("neg", False)):
        picked.append(next(k for k in reg.kept if k[2]["v_class"] == cls and k[2]["start_le64"] == start))
    out = dict(note="minted by tests/golden/make_modinv_classes.py; decoded by tests/modinv_class_cases.py", wide={})
    out["small"] = [vector(m, a, s, 64) for m, a, s in picked]
    for mod_bits in MC.WIDTHS:
        kw = mod_bits // 32
        for m, a, s in picked:                                         # the small vectors are the same in every field
            assert model(MC.value_of(a, MC.modulus_of(m)), MC.modulus_of(m), kw) == s
        # every length once, lightly; then the lengths congruent to 1 ... 6 modulo 30 (tests/test_wbgcd_model.py: where the class shows)
        # until each has given a hit
        full = search_wide(mod_bits, "full width", [mod_bits], 20, 1)
        counts.append(full.report())
        sweep = search_wide(mod_bits, "lengths -31..-1", range(mod_bits - 31, mod_bits), 2, 1 << 30)
        counts.append(sweep.report())
        short = search_wide(mod_bits, "lengths 1..6 mod 30", [b for b in range(mod_bits - 31, mod_bits) if 1 <= b % 30 <= 6], 80, 1, first=2)
        counts.append(short.report())
        short.kept = sweep.kept + short.kept
        rnd = search_events(mod_bits, 6)
        counts.append(rnd.report())
        rare = [k for k in full.kept + short.kept if k[2]["v_class"] == MC.RARE]
        ge = [k for k in full.kept + short.kept if k[2]["v_class"].startswith("ge_m")]
        assert len(rare) >= 2, "fewer than two wide below_neg_m vectors at %d bits" % mod_bits
        chosen = []                                                    # three below_neg_m vectors, the longest moduli first, no length twice
        for k in sorted(rare, key=lambda k: -k[0]["bits"]):
            if len(chosen) < 3 and k[0]["bits"] not in [c[0]["bits"] for c in chosen]:
                chosen.append(k)
        assert len(chosen) >= 2
        out["wide"][str(mod_bits)] = [vector(m, a, s, kw) for m, a, s in chosen + ge[:2]] + pick_common(rnd, kw)
    shared_reg, shared = search_shared(4)
    counts.append(shared_reg.report())
    M = MC.modulus_of(shared["m"])
    for r in shared["rare"]:
        assert model(M - r, M, 256)["v_class"] == MC.RARE
    out["shared_8192"] = shared
    out["search"] = counts
    total = Counter()
    for c in counts:
        for k in ("tried",) + W.V_CLASSES:
            total[k] += c[k]
    print("%-22s tried %7d  " % ("ALL", total["tried"]) + "  ".join("%s %d" % (c, total[c]) for c in W.V_CLASSES))
    path = os.path.join(HERE, "modinv_classes.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
