"""Python restatement of the seeded nonces of VerlinProof and MulProof (include/zkp_hip.h), written from the rule and
not from the kernel (csrc/kernels_coprime.hpp).  A plain module: tests/test_seeded_coprime_model.py pins it,
tests/test_gpu_seeded_coprime.py holds the GPU to it bit for bit.

The stream is that of tests/seeded_nonce_model.py, unchanged: ChaCha20 block function of RFC 8439; key = the 32 seed bytes as 8
little-endian words; state words 13, 14 = (index & 0xffffffff, index >> 32), index = first_index + b; state word 15 =
0x80000000 | kind << 20 | slot << 4 | field.  Two more kinds: 5 Verlin, 6 Mul.

    kind      slot  field  value            draw
    Verlin    0     0      a                sample_below(n)
    Verlin    0     1      a_prime          sample_below(n)
    Verlin    0     2      a_double_prime   sample_below(n)
    Verlin    0     3      r_a              sample_coprime_below(n)
    Mul       0     0      d                sample_below(n)
    Mul       0     1      r_d              sample_coprime_below(n)

sample_coprime_below(n): attempts t = 0, 1, ... produce exactly the candidates of sample_below(n) (the nw first words of blocks
[t nb, (t + 1) nb), the top limb masked to bit_length(n)); candidate t is accepted when it is < n AND gcd(candidate, n) == 1; at most 128
attempts in all, rejections of both sorts share the one counter t.  n == 0, n even, or 128 rejections in a row in any field: every nonce
of the proof is zero and its status is MALFORMED."""
import math

import seeded_model as R

MAX_ATTEMPTS = R.MAX_ATTEMPTS
MALFORMED = R.MALFORMED
KIND_VERLIN, KIND_MUL = 5, 6
M32 = 0xFFFFFFFF
FIELDS = {KIND_VERLIN: ("a", "a_prime", "a_double_prime", "r_a"), KIND_MUL: ("d", "r_d")}      # by field id; the last one is the coprime draw


def word15(kind, slot, field):
    assert kind in FIELDS and slot == 0 and 0 <= field < len(FIELDS[kind])
    return 0x80000000 | (kind << 20) | (slot << 4) | field


def block(seed, counter, index, kind, field):
    return R.block_words(list(R.SIGMA) + R.key_words(seed) + [counter & M32, index & M32, (index >> 32) & M32, word15(kind, 0, field)])


def candidate(seed, index, kind, field, n, t):
    """what attempt t of sample_below(n) looks at"""
    bits = n.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    words = []
    for k in range(t * nb, (t + 1) * nb):
        words += block(seed, k, index, kind, field)
    return sum(w << (32 * i) for i, w in enumerate(words[:nw])) & ((1 << bits) - 1)


def sample_below(seed, index, kind, field, n):
    """-> (value, attempts rejected as not below n); (None, MAX_ATTEMPTS) when every attempt was rejected.  n > 0."""
    assert n > 0
    for t in range(MAX_ATTEMPTS):
        v = candidate(seed, index, kind, field, n, t)
        if v < n:
            return v, t
    return None, MAX_ATTEMPTS


def sample_coprime_below(seed, index, kind, field, n):
    """-> (value, attempts rejected as not below n, attempts rejected as not coprime to n); value None after MAX_ATTEMPTS rejections.  n > 0."""
    assert n > 0
    not_below = not_coprime = 0
    for t in range(MAX_ATTEMPTS):
        v = candidate(seed, index, kind, field, n, t)
        if v >= n:
            not_below += 1
        elif math.gcd(v, n) != 1:
            not_coprime += 1
        else:
            return v, not_below, not_coprime
    return None, not_below, not_coprime


def nonces(kind, seed, first_index, n_list, B):
    """proofs first_index .. first_index + B - 1 (n_list: one shared n or one per proof) ->
    (list of B dicts name -> int; status [B]; attempts rejected as not below n, per proof [B]; attempts rejected as not coprime [B])"""
    names = FIELDS[kind]
    out, status, not_below, not_coprime = [], [0] * B, [0] * B, [0] * B
    for b in range(B):
        n = n_list[0] if len(n_list) == 1 else n_list[b]
        index = first_index + b
        d = {}
        bad = n == 0 or n % 2 == 0
        for field, name in enumerate(names):
            if bad:
                break
            if field + 1 < len(names):
                v, k = sample_below(seed, index, kind, field, n)
                not_below[b] += k
            else:
                v, k, g = sample_coprime_below(seed, index, kind, field, n)
                not_below[b] += k
                not_coprime[b] += g
            bad = v is None
            d[name] = v
        if bad:                                     # every nonce of the proof is zero
            status[b] = MALFORMED
            d = {name: 0 for name in names}
        out.append(d)
    return out, status, not_below, not_coprime
