"""Python model of wb_jacobi (csrc/kernels_jacobi.hpp): the Jacobi symbol (a / b) for odd b by the word-batched binary algorithm — up to
K = 28 steps per round on 64-bit approximations, each step taken only while it is a step of the exact algorithm (30 - i >= 3 exact low
bits; Lehmer's condition |xa - xb| >= 2^31 at odd steps, an exact comparison where it fails at a round's first step) — with the same
word-level pass and the integer ranges of the kernel asserted.  The counterpart of tools/wbgcd_model.py, whose helpers it uses."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wbgcd_model import words, unwords, bitlen_words, extract, i64  # noqa: E402

K = 28
LOW = 30
MLOW = (1 << LOW) - 1
MARGIN = 1 << 31
CH = 8


def u64(x):
    assert 0 <= x < 1 << 64, x
    return x


def i32(x):
    assert -(1 << 31) <= x < 1 << 31, x
    return x


def lincomb_shift(f, g, A, B, n, sh):
    """(f*A + g*B) >> sh over n words, 1 <= sh <= K; the result is a non-negative number of n words"""
    assert 1 <= sh <= K
    acc = 0
    T = []
    for w in range(n):
        acc = i64(acc + f * A[w] + g * B[w])
        T.append(acc & 0xFFFFFFFF)
        acc >>= 32
    assert 0 <= acc < 1 << sh, (acc, sh)           # never negative (nothing to negate), and the shifted value fits the n words
    assert T[0] & ((1 << sh) - 1) == 0             # the division is exact
    T.append(acc & 0xFFFFFFFF)
    return [((T[w] >> sh) | (T[w + 1] << (32 - sh))) & 0xFFFFFFFF for w in range(n)]


def wbjacobi(x, m, kw, trace=None):
    """(x / m) for an odd m > 0 and 0 <= x < 2^(32 kw).  trace (a list) receives one dict per round: steps taken, whether the round ended
    early (Lehmer's condition failed after its first step), whether its one step was decided on the full operands, and i_mod8 — the
    largest step index at which the halving rule flipped the sign (it read b mod 8 there), or -1."""
    assert m & 1 and m > 0 and kw % CH == 0
    a, b = words(x, kw), words(m, kw)
    na = nb = kw
    t = 0
    rounds = 0
    while True:
        assert rounds < 64 * kw
        na, la = bitlen_words(a, na)
        if la == 0:
            break
        nb, lb = bitlen_words(b, nb)
        nb = max(nb, 1)
        n = max(la, lb)
        exact = n <= 64
        if exact:
            xa, xb = unwords(a[:2]), unwords(b[:2])
        else:
            xa = (extract(a, n - 34, 34, kw) << LOW) | (a[0] & MLOW)
            xb = (extract(b, n - 34, 34, kw) << LOW) | (b[0] & MLOW)
        nw0 = max(na, nb)
        va, vb = unwords(a), unwords(b)            # (the model's own check of every step against the operands it stands for)
        f0, g0, f1, g1 = 1, 0, 0, 1
        sh = 0
        rec = dict(steps=0, early=False, exact_step=False, i_mod8=-1)
        for i in range(K):
            odd = xa & 1
            sw = bool(odd and xa < xb)
            last = False
            if odd and not exact and abs(xa - xb) < MARGIN:
                if i > 0:
                    rec["early"] = True
                    break
                c = 0
                for w in range(nw0 - 1, -1, -1):
                    if a[w] != b[w]:
                        c = -1 if a[w] < b[w] else 1
                        break
                sw = c < 0
                last = True
                rec["exact_step"] = True
            # the step is the exact algorithm's: the parity, the comparison and the low bits it reads are those of the true operands
            assert (va & 1) == odd and (not odd or sw == (va < vb)), (x, m, i)
            assert (xa & 7) == (va & 7) and (xb & 7) == (vb & 7), (x, m, i)
            t ^= int(sw) & (xa >> 1) & (xb >> 1) & 1
            if sw:
                xa, xb, f0, g0, f1, g1 = xb, xa, f1, g1, f0, g0
                va, vb = vb, va
            flip = ((xb >> 1) ^ (xb >> 2)) & 1
            if flip:
                rec["i_mod8"] = i
            t ^= flip
            if odd:
                xa = (xa - xb) & ((1 << 64) - 1) if last else u64(xa - xb)
                va -= vb
                f0 = i32(f0 - f1)
                g0 = i32(g0 - g1)
            assert va >= 0 and va % 2 == 0
            xa >>= 1
            va >>= 1
            f1 = i32(f1 * 2)
            g1 = i32(g1 * 2)
            sh = i + 1
            assert abs(f0) + abs(g0) <= 1 << sh and abs(f1) + abs(g1) <= 1 << sh
            if last:
                break
        rec["steps"] = sh
        nw = (nw0 + CH - 1) // CH * CH
        assert nw <= kw
        A2 = lincomb_shift(f0, g0, a, b, nw, sh)
        B2 = lincomb_shift(f1, g1, a, b, nw, sh)
        a[:nw] = A2
        b[:nw] = B2
        assert unwords(a) == va and unwords(b) == vb and vb & 1
        na = nb = nw
        rounds += 1
        if trace is not None:
            trace.append(rec)
    g = unwords(b)
    return (-1 if t & 1 else 1) if g == 1 else 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from jacobi_model import jacobi
    rnd = random.Random(1)
    for kw in (8, 32, 64, 128):
        bits = 32 * kw
        rounds = 0
        for trial in range(200):
            m = rnd.getrandbits(rnd.randrange(1, bits + 1)) | 1
            a = rnd.getrandbits(rnd.randrange(1, bits + 1))
            if trial % 5 == 0:
                a = m ^ (rnd.getrandbits(rnd.randrange(1, bits)) & ~1 & ((1 << max(1, m.bit_length() - 40)) - 1))
            tr = []
            assert wbjacobi(a, m, kw, tr) == jacobi(a, m), (a, m)
            rounds = max(rounds, len(tr))
        print(kw, "max rounds", rounds)
    print("ok")
