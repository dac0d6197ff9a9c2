"""Python restatement of the verifier's seeded commitment of the interactive RangeProof (include/zkp_hip.h:
zkp_range_verifier_commit_seeded_batch, zkp_range_verifier_reveal_seeded_batch, zkp_range_verify_commit_batch), written
from the definition and not from the kernel (csrc/kernels_sample.hpp: k_range_commit).  A plain module: tests/test_seeded_commit_model.py
pins it, tests/test_gpu_seeded_commit.py holds the GPU to it bit for bit.

The stream is the construction of tests/seeded_nonce_model.py (its ChaCha block and its sample_below) under a kind of its own:
state word 15 = 0x80000000 | 7 << 20 | slot << 4 | field, slot 0.

    field  value  draw
    0      r      sample_below(n), at most 128 attempts
    1      e      the first e_len bytes of block 0; byte k = bits 8 (k % 4) .. of word k / 4; no rejection; 1 <= e_len <= 32

m = the 32 bytes of SHA256(e) read big-endian (no to_bytes in between: leading zero bytes make a smaller integer); com = Enc(m, r) =
(1 + m n) r^n mod n^2 (range_proof.rs:118-126).  verify_commit (range_proof.rs:195-208): com == Enc(from(SHA256(e)), r), com compared as
it is stored.

OUR rules.  Key domain: n odd and bit_length(n) > 256.  A session whose key is outside it, n == 0 included, or whose 128 attempts were all
rejected is MALFORMED: r = e = 0 and com = 0."""
import hashlib

import seeded_nonce_model as N

KIND_RANGE_COMMIT = 7
MALFORMED = N.MALFORMED
ACCEPT, REJECT = 1, 0
MAX_ATTEMPTS = N.MAX_ATTEMPTS
M32 = 0xFFFFFFFF


def word15(field, slot=0, kind=KIND_RANGE_COMMIT):
    assert 0 <= slot < N.MAX_SLOTS and 0 <= field < 16
    return 0x80000000 | (kind << 20) | (slot << 4) | field


def block(seed, counter, index, field, kind=KIND_RANGE_COMMIT):
    return N.block_words(list(N.R.SIGMA) + N.key_words(seed) + [counter & M32, index & M32, (index >> 32) & M32, word15(field, 0, kind)])


def sample_below(seed, index, n, kind=KIND_RANGE_COMMIT):
    """field 0: the rule of seeded_nonce_model.sample_below on the blocks of kind 7 -> (value or None, rejected attempts).  (That function
    refuses kinds above 4, so the rule is written out; tests/test_seeded_commit_model.py runs both on a kind both take.)"""
    bits = n.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    for t in range(MAX_ATTEMPTS):
        words = []
        for k in range(t * nb, (t + 1) * nb):
            words += block(seed, k, index, 0, kind)
        v = sum(w << (32 * i) for i, w in enumerate(words[:nw])) & ((1 << bits) - 1)
        if v < n:
            return v, t
    return None, MAX_ATTEMPTS


def challenge_bytes(seed, index, e_len):
    assert 1 <= e_len <= 32
    words = block(seed, 0, index, 1)
    return bytes((words[k // 4] >> (8 * (k % 4))) & 0xFF for k in range(e_len))


def digest_int(e):
    return int.from_bytes(hashlib.sha256(bytes(e)).digest(), "big")


def key_in_domain(n):
    return n % 2 == 1 and n.bit_length() > 256


def enc(n, m, r):
    return (1 + m * n) * pow(r, n, n * n) % (n * n)


def sessions(seed, first_index, n_list, B, e_len, with_com=True):
    """sessions first_index .. first_index + B - 1 (n_list: one shared n or one per session) ->
    list of B dicts r, e (bytes of length e_len), m, com (None unless with_com), status, rejected"""
    out = []
    for b in range(B):
        n = n_list[0] if len(n_list) == 1 else n_list[b]
        index = first_index + b
        r, rejected = (None, 0)
        if key_in_domain(n):
            r, rejected = sample_below(seed, index, n)
        if r is None:
            out.append(dict(r=0, e=bytes(e_len), m=0, com=0 if with_com else None, status=MALFORMED, rejected=rejected))
            continue
        e = challenge_bytes(seed, index, e_len)
        m = digest_int(e)
        out.append(dict(r=r, e=e, m=m, com=enc(n, m, r) if with_com else None, status=0, rejected=rejected))
    return out


def verify_commit(n, com, r, e):
    """-> ACCEPT / REJECT / MALFORMED for one session; e: the bytes as sent (0 .. 32 of them)"""
    if not key_in_domain(n) or len(e) > 32:
        return MALFORMED
    return ACCEPT if com == enc(n, digest_int(e), r) else REJECT
