"""Python restatement of the seeded set-up of a DLogStatement (include/zkp_hip.h: zkp_dlog_statement_setup_seeded_batch; DESIGN.md
section 4), written from the rule and not from the kernel (csrc/kernels_jacobi.hpp: k_nonce_jacobi).  A plain module:
tests/test_seeded_dlog_setup_model.py pins it, tests/test_gpu_dlog_setup.py holds the GPU to it bit for bit.

The stream is that of tests/seeded_nonce_model.py and tests/seeded_coprime_model.py, unchanged: ChaCha20 block function of RFC 8439; key =
the 32 seed bytes as 8 little-endian words; state words 13, 14 = (index & 0xffffffff, index >> 32), index = first_index + b; state word
15 = 0x80000000 | kind << 20 | slot << 4 | field.  One more kind: 8 DLogSetup.

    kind        slot  field  value    draw
    DLogSetup   0     0      h1       sample_jacobi_minus_below(N)
    DLogSetup   0     1      secret   words 0 .. 7 of block 0: uniform on [0, 2^256)

sample_jacobi_minus_below(N): attempts t = 0, 1, ... produce exactly the candidates of sample_below(N) (seeded_coprime_model.candidate's
construction: the nw first words of blocks [t nb, (t + 1) nb), the top limb masked to bit_length(N)); candidate v is accepted when
v + 1 < N AND the Jacobi symbol (v / N) == -1; at most 128 attempts, rejections of both sorts share the one counter t.
Then h2 = (h1^-1)^secret mod N.  N == 0, N even, or 128 rejections in a row (certain for a square N): g = h1, ni = h2 and secret are zero
and the status is MALFORMED."""
import seeded_model as R
from jacobi_model import jacobi

MAX_ATTEMPTS = R.MAX_ATTEMPTS
MALFORMED = R.MALFORMED
KIND_DLOG_SETUP = 8
FIELD_H1, FIELD_SECRET = 0, 1
M32 = 0xFFFFFFFF


def word15(field):
    assert field in (FIELD_H1, FIELD_SECRET)
    return 0x80000000 | (KIND_DLOG_SETUP << 20) | (0 << 4) | field


def block(seed, counter, index, field):
    return R.block_words(list(R.SIGMA) + R.key_words(seed) + [counter & M32, index & M32, (index >> 32) & M32, word15(field)])


def candidate(seed, index, n, t):
    """what attempt t of sample_below(N) looks at on the h1 stream (the construction of seeded_coprime_model.candidate under word 15 of kind 8)"""
    bits = n.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    words = []
    for k in range(t * nb, (t + 1) * nb):
        words += block(seed, k, index, FIELD_H1)
    return sum(w << (32 * i) for i, w in enumerate(words[:nw])) & ((1 << bits) - 1)


def sample_jacobi_minus_below(seed, index, n):
    """-> (value, attempts rejected as not below N - 1, attempts rejected for their symbol); value None after MAX_ATTEMPTS rejections.
    N odd and positive."""
    assert n > 0 and n & 1
    not_below = symbol = 0
    for t in range(MAX_ATTEMPTS):
        v = candidate(seed, index, n, t)
        if v + 1 >= n:
            not_below += 1
        elif jacobi(v, n) != -1:
            symbol += 1
        else:
            return v, not_below, symbol
    return None, not_below, symbol


def secret(seed, index):
    return sum(w << (32 * i) for i, w in enumerate(block(seed, 0, index, FIELD_SECRET)[:8]))


def statements(seed, first_index, n_list):
    """statements first_index .. first_index + B - 1, one N each ->
    (list of B dicts g / ni / secret; status [B]; attempts rejected as not below N - 1 [B]; attempts rejected for their symbol [B])"""
    out, status, not_below, symbol = [], [], [], []
    for b, n in enumerate(n_list):
        index = first_index + b
        h1, k, s = (None, 0, 0) if n == 0 or n % 2 == 0 else sample_jacobi_minus_below(seed, index, n)
        not_below.append(k)
        symbol.append(s)
        if h1 is None:
            status.append(MALFORMED)
            out.append(dict(g=0, ni=0, secret=0))
            continue
        x = secret(seed, index)
        status.append(0)
        out.append(dict(g=h1, ni=pow(pow(h1, -1, n), x, n), secret=x))
    return out, status, not_below, symbol
