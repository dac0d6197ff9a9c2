"""Python restatement of the seeded nonces of ZeroProof, CiphertextProof, CorrectMessageProof and CompositeDLogProof (include/zkp_hip.h,
DESIGN.md section 4), written from the definition and not from the kernel (csrc/kernels_sample.hpp).  A plain module:
tests/test_seeded_nonce_model.py pins it, tests/test_gpu_seeded_nonces.py holds the GPU to it bit for bit.

The stream: ChaCha20 block function of RFC 8439 (20 rounds, 32-bit block counter in state word 12); key = the 32 seed bytes as 8
little-endian words; state words 13, 14 = (index & 0xffffffff, index >> 32), index = first_index + b; state word 15 =
0x80000000 | kind << 20 | slot << 4 | field (bit 31 keeps these streams apart from the RangeProofNi streams of tests/seeded_model.py, whose
word 15 is row << 2 | field < 1024).  kind: 1 Zero, 2 Ciphertext, 3 CorrectMessage, 4 DLog; slot < 65536; field < 16.

    kind             slot                field  value      draw
    Zero             0                   0      r_prime    sample_below(n)
    Ciphertext       0                   0      x_prime    sample_below(n)
    Ciphertext       0                   1      r_prime    sample_below(n)
    CorrectMessage   0                   0      r          sample_below(n)
    CorrectMessage   0                   1      w          sample_below(n)
    CorrectMessage   j + 1, j < K - 1    2      e_sim[j]   words 0 .. 7 of block 0, no rejection
    CorrectMessage   j + 1, j < K - 1    3      z_sim[j]   sample_below(n)
    DLog             0                   0      r          words 0 .. 15 of block 0

sample_below(n): bits = bit_length(n), nw = ceil(bits / 32), nb = ceil(nw / 16); attempt t reads the nw first words of blocks
[t nb, (t + 1) nb) as limbs 0 .. nw - 1, clears the bits of the top limb above `bits`, and is accepted when the value is < n; at most
128 attempts.  n == 0, or 128 rejections in a row: every nonce of the proof is zero and its status is MALFORMED."""
import seeded_model as R

MAX_ATTEMPTS = R.MAX_ATTEMPTS
MALFORMED = R.MALFORMED
KIND_ZERO, KIND_CIPHERTEXT, KIND_CORRECT_MESSAGE, KIND_DLOG = 1, 2, 3, 4
MAX_SLOTS = 65536
M32 = 0xFFFFFFFF

block_words = R.block_words          # the RFC 8439 block function is the one the range model is pinned with
key_words = R.key_words


def word15(kind, slot, field):
    assert 1 <= kind <= 4 and 0 <= slot < MAX_SLOTS and 0 <= field < 16
    return 0x80000000 | (kind << 20) | (slot << 4) | field


def block(seed, counter, index, kind, slot, field):
    return block_words(list(R.SIGMA) + key_words(seed) + [counter & M32, index & M32, (index >> 32) & M32, word15(kind, slot, field)])


def sample_below(seed, index, kind, slot, field, n):
    """-> (value, rejected attempts); (None, MAX_ATTEMPTS) when every attempt was rejected.  n > 0."""
    assert n > 0
    bits = n.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    for t in range(MAX_ATTEMPTS):
        words = []
        for k in range(t * nb, (t + 1) * nb):
            words += block(seed, k, index, kind, slot, field)
        v = sum(w << (32 * i) for i, w in enumerate(words[:nw])) & ((1 << bits) - 1)
        if v < n:
            return v, t
    return None, MAX_ATTEMPTS


def raw_bits(seed, index, kind, slot, field, words):
    """the first `words` words of block 0 as one integer"""
    return sum(w << (32 * i) for i, w in enumerate(block(seed, 0, index, kind, slot, field)[:words]))


def fields_of(kind, K=1):
    """every (slot, field, name, j, is a sample_below draw) of one proof, in the order of the table above"""
    if kind == KIND_ZERO:
        return [(0, 0, "r_prime", None, True)]
    if kind == KIND_CIPHERTEXT:
        return [(0, 0, "x_prime", None, True), (0, 1, "r_prime", None, True)]
    if kind == KIND_DLOG:
        return [(0, 0, "r", None, False)]
    assert kind == KIND_CORRECT_MESSAGE and 1 <= K <= MAX_SLOTS
    out = [(0, 0, "r", None, True), (0, 1, "w", None, True)]
    for j in range(K - 1):
        out += [(j + 1, 2, "e_sim", j, False), (j + 1, 3, "z_sim", j, True)]
    return out


def nonces(kind, seed, first_index, n_list, B, K=1):
    """proofs first_index .. first_index + B - 1 (n_list: one shared n or one per proof; ignored for DLog) ->
    (list of B dicts name -> int, or list of ints for e_sim / z_sim; status [B]; rejected attempts per proof [B])"""
    out, status, rejected = [], [0] * B, [0] * B
    for b in range(B):
        n = None if kind == KIND_DLOG else (n_list[0] if len(n_list) == 1 else n_list[b])
        index = first_index + b
        d = {"e_sim": [0] * (K - 1), "z_sim": [0] * (K - 1)} if kind == KIND_CORRECT_MESSAGE else {}
        bad = n == 0
        for slot, field, name, j, below in fields_of(kind, K):
            if bad:
                v = 0
            elif below:
                v, k = sample_below(seed, index, kind, slot, field, n)
                rejected[b] += k
                bad = v is None
            else:
                v = raw_bits(seed, index, kind, slot, field, 16 if kind == KIND_DLOG else 8)
            if j is None:
                d[name] = v
            else:
                d[name][j] = v
        if bad:                                     # every nonce of the proof is zero
            status[b] = MALFORMED
            d = {k: ([0] * len(v) if isinstance(v, list) else 0) for k, v in d.items()}
        out.append(d)
    return out, status, rejected
