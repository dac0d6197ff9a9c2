"""Word-for-word model of the routines of csrc/kernels_paillier_dec.hpp on lists of 32-bit words (least significant first), with the integer
ranges the kernel relies on asserted: pd_mul, pd_mod (Knuth's algorithm D), pd_divexact (digit-serial division by an odd divisor through its
inverse modulo 2^32) and the inverse modulo an even M = p - 1 from an inverse modulo the odd q.  tests/test_paillier_dec_model.py holds them to
Python's own integer arithmetic."""

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


def pd_mod(x, nx, m, stats=None):
    """x: nx + 1 words (word nx scratch), consumed; m: nmf words, non-zero, nx >= nmf.  Returns x with the remainder in words 0 .. nx."""
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
        assert from_words(x[j:j + nm + 1]) < from_words(mn) << 32          # the running remainder's window is below mn 2^32
        num = (x[j + nm] << 32) | x[j + nm - 1]
        qh, rh = num // v1, num % v1
        assert qh <= B + 1
        x2 = x[j + nm - 2] if j + nm >= 2 else 0
        loops = 0
        while (qh >> 32) != 0 or qh * v2 > ((rh << 32) | x2):
            assert (qh >> 32) != 0 or (qh * v2 <= M64 and rh < B)
            qh -= 1
            rh += v1
            loops += 1
            if rh >> 32:
                break
        assert qh < B and loops <= 3
        carry = borrow = 0
        for i in range(nm):
            p = qh * mn[i] + carry
            assert p <= M64
            carry = p >> 32
            t = (x[j + i] - (p & M32) - borrow) & M64
            x[j + i] = t & M32
            borrow = t >> 63
        t = (x[j + nm] - carry - borrow) & M64
        x[j + nm] = t & M32
        addback = t >> 63
        if addback:
            c = 0
            for i in range(nm):
                u = x[j + i] + mn[i] + c
                x[j + i] = u & M32
                c = u >> 32
            x[j + nm] = (x[j + nm] + c) & M32
        assert x[j + nm] == 0                                               # the digit is settled: the window shrinks by one word
        if stats is not None:
            stats["corrections"] = stats.get("corrections", 0) + loops
            stats["addbacks"] = stats.get("addbacks", 0) + addback
    for w in range(nm):
        lo, hi = x[w], x[w + 1] if w + 1 < nm else 0
        x[w] = (lo >> s) | ((hi << (32 - s)) & M32) if s else lo
    for w in range(nm, nx + 1):
        x[w] = 0
    return x


def pd_divexact(x, d, nq):
    """x: nx words, consumed; d: nd words, odd; nx >= nq + nd.  Returns (quotient words, exact)."""
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
            w += 1
    return q, not any(x)


def inv_even(F, y, O, hw):
    """O^-1 mod the even M = F - 1, from y = M^-1 mod the odd O, as k_pdec_key_b does it: M y = 1 + t O exactly, and the inverse is M - t"""
    mm = to_words(F - 1, hw)
    x = pd_mul(mm, to_words(y, hw))
    assert any(x)
    for w in range(2 * hw):
        was = x[w]
        x[w] = (x[w] - 1) & M32
        if was:
            break
    t, exact = pd_divexact(x, to_words(O, hw), hw)
    assert exact
    tv = from_words(t)
    assert 0 < tv < F - 1
    d, borrow = [0] * hw, 0
    for w in range(hw):
        v = (mm[w] - t[w] - borrow) & M64
        d[w] = v & M32
        borrow = v >> 63
    assert borrow == 0
    return from_words(d)


def open_words(p, q, c, hw):
    """the whole item as the kernels compute it (the ladder is Python's pow): (m, r, status)"""
    from math import gcd
    kw = 2 * hw
    if p < 3 or q < 3 or p % 2 == 0 or q % 2 == 0:
        return 0, 0, 2
    P, Q = to_words(p, hw), to_words(q, hw)

    def mod(v, nx, m_words):
        return from_words(pd_mod(to_words(v, nx) + [0], nx, m_words))

    rows = [(mod(q, hw, P), p), (mod(p, hw, Q), q), (mod(p - 1, hw, Q), q), (mod(q - 1, hw, P), p)]
    if any(gcd(a, m) != 1 or a == 0 for a, m in rows):                      # (the inverse kernel's status; its own model is tools/wbgcd_model.py)
        return 0, 0, 2
    inv = [pow(a, -1, m) for a, m in rows]
    hp, hq, pinv = p - inv[0], q - inv[1], inv[1]
    dp, dq = inv_even(p, inv[2], q, hw), inv_even(q, inv[3], p, hw)
    ok, half = True, []
    P2, Q2 = to_words(p * p, kw), to_words(q * q, kw)
    for F, Fw, F2w, h in ((p, P, P2, hp), (q, Q, Q2, hq)):
        base = mod(c, 2 * kw, F2w)
        xs = pow(base, F - 1, F * F)
        x = to_words(xs, kw)
        zero = not any(x)
        for w in range(kw):
            was = x[w]
            x[w] = (x[w] - 1) & M32
            if was:
                break
        Lw, exact = pd_divexact(x, Fw, hw)
        ok = ok and exact and not zero
        half.append(mod(from_words(pd_mul(Lw, to_words(h, hw))), kw, Fw))
        half.append(pow(mod(base, kw, Fw), dp if F == p else dq, F))

    def crt(vp, vq):
        d = (vq - mod(vp, hw, Q)) % q
        u = mod(from_words(pd_mul(to_words(d, hw), to_words(pinv, hw))), kw, Q)
        out = from_words(pd_mul(to_words(u, hw), P)) + vp
        assert out < 1 << (32 * kw)
        return out

    m, r = crt(half[0], half[2]), crt(half[1], half[3])
    return (m, r, 0) if ok else (0, 0, 2)
