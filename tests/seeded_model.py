"""Python restatement of the seeded RangeProofNi witness (include/zkp_hip.h), written from the definition and not
from the kernel (csrc/kernels_sample.hpp).  A plain module: tests/test_seeded_model.py pins it, tests/test_gpu_seeded_prove.py holds the
GPU to it bit for bit.

The stream: ChaCha20 block function of RFC 8439 (20 rounds, 32-bit block counter in state word 12); key = the 32 seed bytes as 8
little-endian words; nonce words (state 13, 14, 15) = (index & 0xffffffff, index >> 32, row << 2 | field); field 0 = w, 1 = r1, 2 = r2,
3 = coin.  sample_below(u): bits = bit_length(u), nw = ceil(bits / 32), nb = ceil(nw / 16); attempt t reads the nw first words of blocks
[t nb, (t + 1) nb) as limbs 0 .. nw - 1, clears the bits of the top limb above `bits`, and is accepted when the value is < u; at most
128 attempts."""
import struct

import numpy as np

MAX_ATTEMPTS = 128
MALFORMED = 2
FIELD_W, FIELD_R1, FIELD_R2, FIELD_COIN = 0, 1, 2, 3
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
M32 = 0xFFFFFFFF


def _rotl(v, c):
    return ((v << c) & M32) | (v >> (32 - c))


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def block_words(state):
    """RFC 8439 section 2.3: 16 state words -> the 16 output words (python ints)"""
    x = list(state)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, state)]


def key_words(seed: bytes):
    assert len(seed) == 32
    return list(struct.unpack("<8I", seed))


def state_for(seed, counter, index, row, field):
    return list(SIGMA) + key_words(seed) + [counter & M32, index & M32, (index >> 32) & M32, (row << 2) | field]


def block(seed, counter, index, row, field):
    return block_words(state_for(seed, counter, index, row, field))


def blocks_np(seed, counters, index, rows, field):
    """the same blocks, many (counter, row) pairs at once (numpy): -> uint32 [len(counters), 16]"""
    counters = np.asarray(counters, dtype=np.uint32)
    rows = np.broadcast_to(np.asarray(rows, dtype=np.uint32), counters.shape)
    init = np.empty((16, counters.size), np.uint32)
    for i, v in enumerate(state_for(seed, 0, index, 0, field)):
        init[i] = v
    init[12] = counters
    init[15] = (rows << np.uint32(2)) | np.uint32(field)
    x = init.copy()

    def rot(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def q(a, b, c, d):
        x[a] += x[b]; x[d] = rot(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rot(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rot(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rot(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            q(0, 4, 8, 12); q(1, 5, 9, 13); q(2, 6, 10, 14); q(3, 7, 11, 15)
            q(0, 5, 10, 15); q(1, 6, 11, 12); q(2, 7, 8, 13); q(3, 4, 9, 14)
        x += init
    return np.ascontiguousarray(x.T)


def sample_below(seed, index, row, field, u):
    """-> (value, rejected attempts); (None, MAX_ATTEMPTS) when every attempt was rejected.  u > 0.  (One value, block by block.)"""
    assert u > 0
    bits = u.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    for t in range(MAX_ATTEMPTS):
        words = []
        for k in range(t * nb, (t + 1) * nb):
            words += block(seed, k, index, row, field)
        v = sum(w << (32 * i) for i, w in enumerate(words[:nw])) & ((1 << bits) - 1)
        if v < u:
            return v, t
    return None, MAX_ATTEMPTS


def sample_below_rows(seed, index, rows, field, u):
    """sample_below for every row of `rows` (the attempts of all rows still pending computed in one numpy call) ->
    ({row: value or None}, {row: rejected attempts})"""
    assert u > 0
    bits = u.bit_length()
    nw = (bits + 31) // 32
    nb = (nw + 15) // 16
    values, rejected = {}, {}
    pending = list(rows)
    for t in range(MAX_ATTEMPTS):
        if not pending:
            break
        counters = np.tile(np.arange(t * nb, (t + 1) * nb, dtype=np.uint32), len(pending))
        ks = blocks_np(seed, counters, index, np.repeat(np.asarray(pending, dtype=np.uint32), nb), field).reshape(len(pending), nb * 16)
        raw = ks[:, :nw].astype("<u4")
        still = []
        for k, row in enumerate(pending):
            v = int.from_bytes(raw[k].tobytes(), "little") & ((1 << bits) - 1)
            if v < u:
                values[row], rejected[row] = v, t
            else:
                still.append(row)
        pending = still
    for row in pending:
        values[row], rejected[row] = None, MAX_ATTEMPTS
    return values, rejected


def coin(seed, index, row):
    return block(seed, 0, index, row, FIELD_COIN)[0] & 1


def witness_row(seed, index, row, n, rng):
    """-> ((w1, w2, r1, r2), rejected attempts per field [w, r1, r2]) or (None, ...) when a field ran out of attempts"""
    third = rng // 3
    s, k0 = sample_below(seed, index, row, FIELD_W, third)
    r1, k1 = sample_below(seed, index, row, FIELD_R1, n)
    r2, k2 = sample_below(seed, index, row, FIELD_R2, n)
    if s is None or r1 is None or r2 is None:
        return None, [k0, k1, k2]
    a = third + s
    w1, w2 = (a, a - third) if coin(seed, index, row) == 0 else (a - third, a)
    return (w1, w2, r1, r2), [k0, k1, k2]


def witness(seed, first_index, n_list, range_list, ef):
    """proofs first_index .. first_index + B - 1 (n_list: one shared n or one per proof) ->
    (dict of python-int rows w1/w2/r1/r2 [B][ef], status [B], rejected attempts in all, the largest number of rejections of one value)"""
    B = len(range_list)
    out = {f: [[0] * ef for _ in range(B)] for f in ("w1", "w2", "r1", "r2")}
    status, rejected, worst = [0] * B, 0, 0
    rows = list(range(ef))
    for b in range(B):
        n = n_list[0] if len(n_list) == 1 else n_list[b]
        third = range_list[b] // 3
        if third == 0 or n == 0:
            status[b] = MALFORMED
            continue
        index = first_index + b
        s, k0 = sample_below_rows(seed, index, rows, FIELD_W, third)
        r1, k1 = sample_below_rows(seed, index, rows, FIELD_R1, n)
        r2, k2 = sample_below_rows(seed, index, rows, FIELD_R2, n)
        coins = blocks_np(seed, np.zeros(ef, np.uint32), index, rows, FIELD_COIN)[:, 0] & 1 if ef else []
        for k in (k0, k1, k2):
            rejected += sum(k.values()); worst = max([worst] + list(k.values()))
        if any(v is None for d in (s, r1, r2) for v in d.values()):
            status[b] = MALFORMED
            continue
        for row in rows:
            a = third + s[row]
            w1, w2 = (a, a - third) if int(coins[row]) == 0 else (a - third, a)
            out["w1"][b][row] = w1; out["w2"][b][row] = w2; out["r1"][b][row] = r1[row]; out["r2"][b][row] = r2[row]
    return out, status, rejected, worst


def to_limbs(rows, kw):
    """python ints [B][ef] -> uint32 [B, ef, kw], little-endian limbs"""
    B, ef = len(rows), len(rows[0]) if rows else 0
    buf = b"".join(v.to_bytes(4 * kw, "little") for per in rows for v in per)
    return np.frombuffer(buf, dtype="<u4").astype(np.uint32).reshape(B, ef, kw)
