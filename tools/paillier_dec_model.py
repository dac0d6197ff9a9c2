"""Word-for-word model of the routines of csrc/kernels_paillier_dec.hpp on lists of 32-bit words (least significant first), with the integer
ranges the kernel relies on asserted: pd_mul, pd_mod (Knuth's algorithm D), pd_divexact (digit-serial division by an odd divisor through its
inverse modulo 2^32) and the inverse modulo an even M = p - 1 from an inverse modulo the odd q.  tests/test_paillier_dec_model.py holds them to
Python's own integer arithmetic.  pd_mod and pd_divexact record which of their data-dependent branches a call took, open_words gathers
the records per call site, and pd_mod can leave out one of those branches' lines (fault=): tests/test_paillier_dec_branch_model.py uses
both to certify the crafted operands of tests/paillier_dec_branch_cases.py."""

B = 1 << 32
M32 = B - 1
M64 = (1 << 64) - 1


def to_words(v, n):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & M32 for i in range(n)]


def from_words(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def clz32(v):
    assert 0 < v < B
    return 32 - v.bit_length()


def inv32(d0):
    assert d0 & 1
    v = d0
    for _ in range(5):
        v = v * ((2 - d0 * v) & M32) & M32
    assert v * d0 & M32 == 1
    return v


def pd_mul(a, b):
    na, nb = len(a), len(b)
    out = [0] * (na + nb)
    for i in range(nb):
        carry = 0
        for j in range(na):
            t = b[i] * a[j] + out[i + j] + carry
            assert t <= M64
            out[i + j] = t & M32
            carry = t >> 32
        out[i + na] = carry
    return out


FAULTS = ("no_addback", "no_overflow_clause", "no_rh_break")


def pd_mod(x, nx, m, stats=None, fault=None):
    """x: nx + 1 words (word nx scratch), consumed; m: nmf words, non-zero, nx >= nmf.  Returns x with the remainder in words 0 .. nx.

    stats (a dict, filled): the counts add up over the calls that share it — corrections (loop turns), addbacks, overflows (estimates with
    qh >> 32 != 0), breaks (the rh >> 32 break taken), digits — max_loops is the largest number of loop turns for one digit, addback_at
    gathers the quotient positions j of the add-backs, and s, nm are those of the last call.

    fault: one of FAULTS — what the kernel would compute with that one line removed (the add-back block, the `(qh >> 32) != 0 ||` clause,
    the `if (rh >> 32) break;`), 64-bit wrap-around included.  The range assertions hold until the missing line would have run for the
    first time (stats["derailed"] counts those); from there on they are skipped, since the values are no longer those of a division."""
    assert fault is None or fault in FAULTS
    derailed = False
    nmf = len(m)
    assert len(x) == nx + 1 and nx >= nmf and any(m)
    nm = nmf
    while nm > 1 and m[nm - 1] == 0:
        nm -= 1
    s = clz32(m[nm - 1])
    mn = [0] * nm
    for w in range(nm - 1, -1, -1):
        hi, lo = m[w], m[w - 1] if w else 0
        mn[w] = ((hi << s) & M32) | (lo >> (32 - s)) if s else hi
    x[nx] = x[nx - 1] >> (32 - s) if s else 0
    for w in range(nx - 1, -1, -1):
        hi, lo = x[w], x[w - 1] if w else 0
        x[w] = ((hi << s) & M32) | (lo >> (32 - s)) if s else hi
    v1, v2 = mn[nm - 1], mn[nm - 2] if nm > 1 else 0
    assert v1 >> 31 == 1
    for j in range(nx - nm, -1, -1):
        assert derailed or from_words(x[j:j + nm + 1]) < from_words(mn) << 32   # the running remainder's window is below mn 2^32
        num = (x[j + nm] << 32) | x[j + nm - 1]
        qh, rh = num // v1, num % v1
        assert derailed or qh <= B + 1
        x2 = x[j + nm - 2] if j + nm >= 2 else 0
        loops = overflow = broke = 0
        while True:
            over = (qh >> 32) != 0
            two_digit = (qh * v2 & M64) > (((rh << 32) & M64) | x2)         # (the kernel's uint64_t arithmetic wraps)
            overflow |= over
            if over and not two_digit and fault == "no_overflow_clause":
                derailed = True
                over = False
            if not (over or two_digit):
                break
            assert derailed or (qh >> 32) != 0 or (qh * v2 <= M64 and rh < B)
            qh = (qh - 1) & M64
            rh = (rh + v1) & M64
            loops += 1
            assert loops < 1 << 16                              # (a derailed estimate: the kernel's loop ends too; this bounds the model's)
            if rh >> 32:
                if fault == "no_rh_break":
                    derailed = True
                else:
                    broke = 1
                    break
        assert derailed or (qh < B and loops <= 3)
        carry = borrow = 0
        for i in range(nm):
            p = qh * mn[i] + carry
            assert derailed or p <= M64
            p &= M64
            carry = p >> 32
            t = (x[j + i] - (p & M32) - borrow) & M64
            x[j + i] = t & M32
            borrow = t >> 63
        t = (x[j + nm] - carry - borrow) & M64
        x[j + nm] = t & M32
        addback = t >> 63
        if addback and fault == "no_addback":
            derailed = True
        elif addback:
            c = 0
            for i in range(nm):
                u = x[j + i] + mn[i] + c
                x[j + i] = u & M32
                c = u >> 32
            x[j + nm] = (x[j + nm] + c) & M32
        assert derailed or x[j + nm] == 0                                   # the digit is settled: the window shrinks by one word
        if stats is not None:
            stats["digits"] = stats.get("digits", 0) + 1
            stats["corrections"] = stats.get("corrections", 0) + loops
            stats["addbacks"] = stats.get("addbacks", 0) + addback
            stats["overflows"] = stats.get("overflows", 0) + overflow
            stats["breaks"] = stats.get("breaks", 0) + broke
            stats["max_loops"] = max(stats.get("max_loops", 0), loops)
            if addback:
                stats.setdefault("addback_at", []).append(j)
    if stats is not None:
        stats.setdefault("addback_at", [])
        stats["s"], stats["nm"], stats["nx"] = s, nm, nx
        stats["derailed"] = stats.get("derailed", 0) + derailed
    for w in range(nm):
        lo, hi = x[w], x[w + 1] if w + 1 < nm else 0
        x[w] = (lo >> s) | ((hi << (32 - s)) & M32) if s else lo
    for w in range(nm, nx + 1):
        x[w] = 0
    return x


def pd_divexact(x, d, nq, stats=None):
    """x: nx words, consumed; d: nd words, odd; nx >= nq + nd.  Returns (quotient words, exact).
    stats (a dict, filled): propagation_steps — the turns of the loop that carries a step's borrow past word i + nd — and reached_top —
    whether one of them wrote word nx - 1."""
    nx, nd = len(x), len(d)
    assert nx >= nq + nd and d[0] & 1
    dinv = inv32(d[0])
    q = [0] * nq
    for i in range(nq):
        qi = x[i] * dinv & M32
        q[i] = qi
        carry = borrow = 0
        for k in range(nd):
            assert i + k < nx
            p = qi * d[k] + carry
            assert p <= M64
            carry = p >> 32
            t = (x[i + k] - (p & M32) - borrow) & M64
            x[i + k] = t & M32
            borrow = t >> 63
        assert x[i] == 0
        w = i + nd
        while w < nx and (carry | borrow):
            t = (x[w] - carry - borrow) & M64
            x[w] = t & M32
            borrow = t >> 63
            carry = 0
            if stats is not None:
                stats["propagation_steps"] = stats.get("propagation_steps", 0) + 1
                stats["reached_top"] = stats.get("reached_top", False) or w == nx - 1
            w += 1
    if stats is not None:
        stats.setdefault("propagation_steps", 0)
        stats.setdefault("reached_top", False)
    return q, not any(x)


def inv_even(F, y, O, hw, check=True):
    """O^-1 mod the even M = F - 1, from y = M^-1 mod the odd O, as k_pdec_key_b does it: M y = 1 + t O exactly, and the inverse is M - t.
    check=False (a y that is no such inverse: open_words under an injected fault): the same words without the assertions, wrapping."""
    mm = to_words(F - 1, hw)
    x = pd_mul(mm, to_words(y, hw))
    assert any(x) or not check
    for w in range(2 * hw):
        was = x[w]
        x[w] = (x[w] - 1) & M32
        if was:
            break
    t, exact = pd_divexact(x, to_words(O, hw), hw)
    tv = from_words(t)
    assert not check or (exact and 0 < tv < F - 1)
    d, borrow = [0] * hw, 0
    for w in range(hw):
        v = (mm[w] - t[w] - borrow) & M64
        d[w] = v & M32
        borrow = v >> 63
    assert borrow == 0 or not check
    return from_words(d)


SITES = ("key_a0", "key_a1", "key_a2", "key_a3", "split_sq_p", "split_sq_q", "split_root_p", "split_root_q", "finish_Lh_p", "finish_Lh_q",
         "crt_m_vp", "crt_m_prod", "crt_r_vp", "crt_r_prod")


def open_words(p, q, c, hw, sites=None, fault=None):
    """the whole item as the kernels compute it (the ladder is Python's pow): (m, r, status).
    sites (a dict, filled): one pd_mod stats record for each call of the item that is reached, under the names of SITES — key preparation's
    four rows, the split by F^2 and by F, the finish's L h mod F, the two reductions of each recombination — and pd_divexact's records of
    the finish under divexact_p, divexact_q.  fault: (site, one of FAULTS) — that call runs with the line removed."""
    from math import gcd
    kw = 2 * hw
    if p < 3 or q < 3 or p % 2 == 0 or q % 2 == 0:
        return 0, 0, 2
    assert fault is None or (fault[0] in SITES and fault[1] in FAULTS)
    P, Q = to_words(p, hw), to_words(q, hw)
    full = (1 << (32 * hw)) - 1

    def mod(site, v, nx, m_words):
        st = {}
        out = from_words(pd_mod(to_words(v, nx) + [0], nx, m_words, st, fault[1] if fault and fault[0] == site else None))
        if sites is not None:
            sites[site] = st
        return out

    rows = [(mod("key_a0", q, hw, P), p), (mod("key_a1", p, hw, Q), q), (mod("key_a2", p - 1, hw, Q), q), (mod("key_a3", q - 1, hw, P), p)]
    if any(gcd(a, m) != 1 or a == 0 for a, m in rows):                      # (the inverse kernel's status; its own model is tools/wbgcd_model.py)
        return 0, 0, 2
    inv = [pow(a, -1, m) for a, m in rows]
    hp, hq, pinv = p - inv[0], q - inv[1], inv[1]
    check = fault is None or not fault[0].startswith("key_a")
    dp, dq = inv_even(p, inv[2], q, hw, check), inv_even(q, inv[3], p, hw, check)
    ok, half = True, []
    P2, Q2 = to_words(p * p, kw), to_words(q * q, kw)
    for side, F, Fw, F2w, h in (("p", p, P, P2, hp), ("q", q, Q, Q2, hq)):
        base = mod("split_sq_" + side, c, 2 * kw, F2w)
        xs = pow(base, F - 1, F * F)
        x = to_words(xs, kw)
        zero = not any(x)
        for w in range(kw):
            was = x[w]
            x[w] = (x[w] - 1) & M32
            if was:
                break
        st = {}
        Lw, exact = pd_divexact(x, Fw, hw, st)
        if sites is not None:
            sites["divexact_" + side] = st
        ok = ok and exact and not zero
        half.append(mod("finish_Lh_" + side, from_words(pd_mul(Lw, to_words(h, hw))), kw, Fw))
        half.append(pow(mod("split_root_" + side, base, kw, Fw), dp if F == p else dq, F))

    def crt(name, vp, vq):
        d = vq - mod("crt_%s_vp" % name, vp, hw, Q)
        if d < 0:                                                           # the kernel: the borrow out of hw words, then + q in hw words
            d = (d + q) & full
        u = mod("crt_%s_prod" % name, from_words(pd_mul(to_words(d, hw), to_words(pinv, hw))), kw, Q)
        out = from_words(pd_mul(to_words(u, hw), P)) + vp
        assert fault is not None or (d < q and out < 1 << (32 * kw))
        return out & ((1 << (32 * kw)) - 1)

    m, r = crt("m", half[0], half[2]), crt("r", half[1], half[3])
    return (m, r, 0) if ok else (0, 0, 2)
