"""Case builders for the five secondary proofs behind the C ABI — ZeroProof, CiphertextProof, VerlinProof, MulProof, CorrectMessageProof
(tests/test_sigma_proofs.py, test_verlin_proof.py, test_mul_and_message_proofs.py).

Two families of cases:
  wide  — n = 1024, 300 proofs (CorrectMessage: 130 proofs of 3 rows, and 300 of 1): a full 256-thread block and a partial one, so that the
          per-proof kernels (b = blockIdx.x * 256 + threadIdx.x) run a second block and the limb kernels under them a GROUPS_PER_BLOCK tail;
          dishonest items on both sides of the wavefront boundary and of the block boundary (`marked`).
  edges — a few dozen proofs, operand edges next to ordinary items: prover inputs 0, 1, n - 1, 2^n_bits - 1; verifier inputs an adversary
          chooses (responses with every limb set, the same residue k * n higher, values >= n^2, 0, 1, values of ragged byte length), and one
          proof per kind whose challenge has a zero top byte (found by a seeded search here, nothing is stored; n = 1024 only).
          Built at 1024 and 4096 bits under per-proof keys (three, cycled) and at 2048 bits under one shared key.  At 4096 bits the
          modulus n^2 has 8192 bits — the widest kernel geometry, a pair of groups per item and one item per wavefront on the latency
          engine — and a batch still crosses a wavefront's claim and the block of every engine.

The statements are computed with the C oracle (threads), everything else comes from the repo's DRBG.  The oracle results of a case are
computed ONCE per process (`cached`): the `ctx` fixture runs every GPU test under several kernel families and must not multiply that work."""
import numpy as np

import helpers as H
from helpers import pm, L, zkp

ACCEPT, REJECT, MALFORMED = zkp.VERDICT_ACCEPT, zkp.VERDICT_REJECT, zkp.VERDICT_MALFORMED
EXTRA = 16                    # ZKP_Z1_EXTRA_LIMBS (include/zkp_hip.h)
SENTINEL = 0xA5A5A5A5

_CACHE = {}


def cached(name, build):
    """the value of build(), computed on first use and kept for the process (keyed by case name)"""
    if name not in _CACHE:
        _CACHE[name] = build()
    return _CACHE[name]


def marked(B):
    """the dishonest items of a wide batch: first and last, both sides of the wavefront boundary (63 | 64) and of the 256-thread
    block boundary (255 | 256), and a few in between"""
    return [i for i in (0, 63, 64, 255, 256, B - 1, 31, 128, 200, 257) if i < B]


def sentinel(shape, dtype=np.uint32):
    """an output buffer no kernel has written yet: an item the GPU skips then differs from the oracle"""
    return np.full(shape, SENTINEL if dtype == np.uint32 else 9, dtype)


def ones(words):
    return (1 << (32 * words)) - 1


def keys_for(n_bits, count):
    """(p, q, n) triples: `count` deterministic 1024-bit keys, or the reference's fixture key at 2048 bits.  At 4096 bits no prime is
    generated (two 2048-bit primes take CPython as long as the CPU part of the suite): the moduli of dlog_cases.keys(4096) — the
    benchmark's key first, then products of four pooled 1024-bit primes, four in all — with p a proper prime factor of n and q = n / p,
    which is composite in the pooled ones.  The `no_inverse` and "multiple of p" items need no more than gcd(p, n) = p."""
    if n_bits == 2048:
        return [H.fixture_key()]
    if n_bits == 4096:
        import dlog_cases
        ks = dlog_cases.keys(4096)
        assert count <= len(ks)
        return [(p, n // p, n) for p, n in ks[:count]]
    return [H.test_key(n_bits, tag=t) for t in range(count)]


class Batch:
    """B proofs under per-proof keys (cycled from `pq`) or one shared key"""

    def __init__(self, n_bits, B, pq, shared):
        assert not shared or len(pq) == 1
        self.n_bits, self.kw, self.B, self.shared = n_bits, n_bits // 32, B, shared
        self.pq = [pq[b % len(pq)] for b in range(B)]
        self.ns = [k[2] for k in self.pq]
        self.n_full = L.ints_to_limbs(self.ns, self.kw)
        self.n_arr = self.n_full[:1] if shared else self.n_full
        self.stride = 0 if shared else self.kw
        self.top = (1 << n_bits) - 1

    def key(self):
        return self.n_bits, self.n_arr, self.stride

    def enc(self, oracle, m, r):
        """Enc(m[b], r[b]) under n[b] for lists of ints, by the C oracle"""
        return oracle.paillier_enc(self.n_bits, self.n_full, self.kw, L.ints_to_limbs(m, self.kw), L.ints_to_limbs(r, self.kw))


def set_int(arr, i, v):
    arr[i] = L.int_to_limbs(v, arr.shape[-1])


def get_int(arr, i):
    return L.limbs_to_int(arr[i])


def flip(arr, idx, salt=0):
    """a copy with one bit flipped in each listed item (a different word and bit per item)"""
    out = arr.copy()
    w = arr.shape[-1]
    for i in idx:
        out[i].reshape(-1)[(7 * i + salt) % w] ^= np.uint32(1 << ((5 * i + salt) % 32))
    return out


def ragged(words, drbg):
    """values whose minimal big-endian byte forms are ragged (Sha256::put_bigint: the byte path for the top word, then whole words):
    three leading zero words, a single byte, one byte above a word boundary, zero"""
    return [drbg.bits(32 * (words - 3)) | (1 << (32 * (words - 3) - 1)), 0x7F, (0xA5 << (32 * (words // 2))) | drbg.bits(32 * (words // 2)), 0]


def assert_same(want, got, what):
    """array_equal that names the items that differ"""
    want, got = np.asarray(want), np.asarray(got)
    assert want.shape == got.shape, what
    assert np.array_equal(want, got), (what, np.nonzero((want != got).reshape(len(want), -1).any(axis=1))[0])


def check_wide_verdicts(cs, v_honest, v_tampered):
    """sigma and Verlin wide batches — the expected vectors themselves: the batch crosses 256 items, REJECT exactly at the dishonest items,
    and those sit at 0, 63, 64, 255, 256, B - 1: both sides of the wavefront boundary and of the block boundary"""
    B = cs["bt"].B
    assert B > 256 and {0, 63, 64, 255, 256, B - 1} <= set(cs["false"] + cs["tamper"])
    for group in (cs["false"], cs["tamper"]):
        assert any(b < 256 for b in group) and any(b >= 256 for b in group)
    assert [int(v) for v in v_honest] == [REJECT if b in cs["false"] else ACCEPT for b in range(B)]
    assert [int(v) for v in v_tampered] == [REJECT if b in cs["false"] + cs["tamper"] else ACCEPT for b in range(B)]


def check_edge_verdicts(cs, v_honest, over, v_edited, rejected=()):
    """sigma and Verlin edge batches: the honest proofs of edge inputs are accepted (all but `rejected`), an over-wide response of the
    same residue is ACCEPTED, and the edited batch holds both verdicts"""
    assert [int(v) for v in v_honest] == [REJECT if b in rejected else ACCEPT for b in range(cs["bt"].B)]
    assert over and all(v_edited[b] == ACCEPT for b in over)
    assert {ACCEPT, REJECT} <= set(int(v) for v in v_edited)


class Free:
    """the ordinary (honest, random) items of an edge batch, handed out one per verifier edit"""

    def __init__(self, idx):
        self.idx = list(idx)

    def take(self, pred=lambda i: True):
        for k, i in enumerate(self.idx):
            if pred(i):
                return self.idx.pop(k)
        raise AssertionError("no ordinary item left for this edit: enlarge the edge batch")


def short_challenge(trial, tries=8192):
    """the first k in 0, 1, 2, ... whose challenge trial(k) has a zero top byte (one in 256)"""
    for k in range(tries):
        if trial(k) >> 248 == 0:
            return k
    raise AssertionError("no challenge with a zero top byte found")


# ====================================================================== ZeroProof / CiphertextProof
def _sigma_arrays(bt, x, r, xp, rp):
    a = lambda v: L.ints_to_limbs(v, bt.kw)
    return dict(x=a(x), r=a(r), xp=a(xp), rp=a(rp))


def sigma_wide(oracle, shared):
    """300 proofs at n = 1024.  c0 = Enc(0, r) (ZeroProof), cx = Enc(x, r) (CiphertextProof); at `false` ZeroProof's statement encrypts 1
    (test_one_proof, zero_enc_proof.rs:134-155) and CiphertextProof's witness is r + 1 (test_bad_ciphertext_proof, correct_ciphertext.rs:137-162);
    `tamper` lists the responses a test flips a bit in."""
    bt = Batch(1024, 300, keys_for(1024, 1 if shared else 4), shared)
    d = pm.Drbg(b"sigma-wide-%d" % shared)
    x, r, xp, rp = ([d.below(n) for n in bt.ns] for _ in range(4))
    D = marked(bt.B)
    false, tamper = D[::2], D[1::2]
    c0 = bt.enc(oracle, [1 if b in false else 0 for b in range(bt.B)], r)
    cx = bt.enc(oracle, x, r)
    a = _sigma_arrays(bt, x, r, xp, rp)
    a["r_ct"] = a["r"].copy()
    for b in false:
        set_int(a["r_ct"], b, r[b] + 1)
    a.update(c0=c0, cx=cx)
    return dict(bt=bt, a=a, false=false, tamper=tamper)


def sigma_edges(oracle, n_bits):
    """40 proofs.  Odd items 1 ... 15: prover inputs at their edges; 17 / 19 (n = 1024): ZeroProof / CiphertextProof with a short
    challenge; 32 ... 38: statements of ragged byte length; the rest (`free`) are ordinary and carry one verifier edit each."""
    shared = n_bits == 2048
    bt = Batch(n_bits, 40, keys_for(n_bits, 3), shared)
    d = pm.Drbg(b"sigma-edges-%d" % n_bits)
    x, r, xp, rp = ([d.below(n) for n in bt.ns] for _ in range(4))
    top, cols = bt.top, dict(x=x, r=r, xp=xp, rp=rp)
    for k, e in enumerate([dict(x=0), dict(xp=0), dict(x=1, xp=1), dict(x="n-1", xp="n-1"), dict(x=top, xp=top, r=top, rp=top),
                           dict(x=top, xp=0, r=1, rp="n-1"), dict(r="n-1", rp=1), dict(x=0, xp=0, r=1, rp=1)]):
        b = 2 * k + 1
        for f, v in e.items():
            cols[f][b] = bt.ns[b] - 1 if v == "n-1" else v
    c0 = bt.enc(oracle, [0] * bt.B, r)
    cx = bt.enc(oracle, x, r)
    short = {}
    if n_bits == 1024:
        # ZeroProof, item 17: r' = r0 * 2^k mod n, so a = r'^n = r0^n * (2^n)^k mod n^2 ((r + t n)^n == r^n mod n^2)
        b, n = 17, bt.ns[17]
        nn, c = n * n, get_int(c0, 17)
        a0, g = pow(rp[b], n, nn), pow(2, n, nn)
        k = short_challenge(lambda k: pm.compute_digest([n, c, a0 * pow(g, k, nn) % nn]))
        rp[b] = rp[b] * pow(2, k, n) % n
        short["zero"] = b
        # CiphertextProof, item 19: x' = x0 + k, c' = (1 + x' n) * r'^n mod n^2
        b, n = 19, bt.ns[19]
        nn, c = n * n, get_int(cx, 19)
        rn = pow(rp[b], n, nn)
        k = short_challenge(lambda k: pm.compute_digest([n, c, (1 + (xp[b] + k) * n) % nn * rn % nn]))
        xp[b] += k
        short["ciphertext"] = b
    stmt = [32, 34, 36, 38]
    for b, v in zip(stmt, ragged(2 * bt.kw, d)):
        set_int(c0, b, v)
        set_int(cx, b, v)
    a = _sigma_arrays(bt, x, r, xp, rp)
    a.update(c0=c0, cx=cx)
    free = [b for b in range(bt.B) if (b % 2 == 0 or b > 19) and b not in stmt]
    return dict(bt=bt, a=a, free=free, short=short, ragged_statements=stmt)


def _commit_edits(bt, free, d, arrs, field, out):
    """edits of a hashed 2kw-word value (statement or commitment): + n^2 where it fits, 0, 1, and three ragged byte lengths.
    -> the item that got + n^2"""
    w = 2 * bt.kw
    i = free.take(lambda i: get_int(arrs[field], i) + bt.ns[i] ** 2 <= ones(w))
    out.append((i, field, get_int(arrs[field], i) + bt.ns[i] ** 2))
    for v in [0, 1] + ragged(w, d)[:3]:
        out.append((free.take(), field, v))
    return i


def apply_edits(arrs, edits):
    out = {k: v.copy() for k, v in arrs.items()}
    for i, f, v in edits:
        set_int(out[f], i, v)
    return out


def zero_edits(cs, z, a):
    """-> (edited arrays, indices of the proofs whose response is >= n^2 yet the same residue)"""
    bt, d, free = cs["bt"], pm.Drbg(b"zero-edits"), Free(cs["free"])
    arrs = dict(c=cs["a"]["c0"], z=z, a=a)
    w = 2 * bt.kw
    edits, over = [], []
    i = free.take(lambda i: get_int(z, i) + bt.ns[i] ** 2 <= ones(w))
    edits.append((i, "z", get_int(z, i) + bt.ns[i] ** 2)); over.append(i)
    edits += [(free.take(), "z", ones(w)), (free.take(), "z", 0)]
    _commit_edits(bt, free, d, arrs, "c", edits)
    _commit_edits(bt, free, d, arrs, "a", edits)
    return apply_edits(arrs, edits), over


def ciphertext_edits(cs, z1, z2, cp):
    bt, d, free = cs["bt"], pm.Drbg(b"ciphertext-edits"), Free(cs["free"])
    arrs = dict(c=cs["a"]["cx"], z1=z1, z2=z2, cp=cp)
    w = 2 * bt.kw
    edits, over = [(free.take(), "z1", ones(bt.kw + EXTRA))], []
    for bits in (300, 500):                                     # the same residue modulo n, 300 ... 500 bits higher
        i = free.take()
        edits.append((i, "z1", get_int(z1, i) + (d.bits(bits) | 1 << (bits - 1)) * bt.ns[i])); over.append(i)
    i = free.take(lambda i: get_int(z2, i) + bt.ns[i] ** 2 <= ones(w))
    edits.append((i, "z2", get_int(z2, i) + bt.ns[i] ** 2)); over.append(i)
    edits += [(free.take(), "z2", ones(w)), (free.take(), "z2", 0)]
    _commit_edits(bt, free, d, arrs, "c", edits)
    _commit_edits(bt, free, d, arrs, "cp", edits)
    return apply_edits(arrs, edits), over


# ====================================================================== VerlinProof
VERLIN_WIT, VERLIN_NON = ("x", "xp", "xpp", "rx"), ("a", "ap", "app", "ra")


def _verlin_finish(oracle, bt, v, c, cp):
    a = {k: L.ints_to_limbs(v[k], bt.kw) for k in VERLIN_WIT + VERLIN_NON}
    a.update(c=c, cp=cp)
    wit = tuple(a[k] for k in VERLIN_WIT)
    # phi_x = gen_phi(c, c', x, x', x'', r_x) (verlin_proof.rs:138-165): the oracle's prover computes exactly that of its nonces
    a["phi_x"] = oracle.verlin_proof_prove(*bt.key(), c, cp, np.zeros_like(c), wit, wit)[0]
    return a


def verlin_wide(oracle):
    """300 proofs under ONE 1024-bit key; at `false` the statement phi_x is doubled (it no longer matches the witness)"""
    bt = Batch(1024, 300, keys_for(1024, 1), True)
    d = pm.Drbg(b"verlin-wide")
    v = {k: [d.below(n) for n in bt.ns] for k in VERLIN_WIT + VERLIN_NON}
    c = bt.enc(oracle, [d.below(n) for n in bt.ns], [d.below(n) for n in bt.ns])
    cp = bt.enc(oracle, [d.below(n) for n in bt.ns], [d.below(n) for n in bt.ns])
    a = _verlin_finish(oracle, bt, v, c, cp)
    D = marked(bt.B)
    false, tamper = D[::2], D[1::2]
    for b in false:
        set_int(a["phi_x"], b, get_int(a["phi_x"], b) * 2 % bt.ns[b] ** 2)
    return dict(bt=bt, a=a, false=false, tamper=tamper)


def verlin_edges(oracle, n_bits):
    """48 proofs, laid out like sigma_edges: odd items 1 ... 15 prover edges, 17 (n = 1024) a short challenge, 40 ... 46 ragged statements"""
    shared = n_bits == 2048
    bt = Batch(n_bits, 48, keys_for(n_bits, 3), shared)
    d = pm.Drbg(b"verlin-edges-%d" % n_bits)
    v = {k: [d.below(n) for n in bt.ns] for k in VERLIN_WIT + VERLIN_NON}
    top = bt.top
    allw, alln = ("x", "xp", "xpp"), ("a", "ap", "app")
    for k, e in enumerate([{f: 0 for f in allw}, {f: 0 for f in alln}, {f: 1 for f in allw + alln}, {f: "n-1" for f in allw + alln},
                           {f: top for f in VERLIN_WIT + VERLIN_NON}, dict(x=top, a=0, xp=0, ap=top, rx=1, ra="n-1"), dict(rx="n-1", ra=1),
                           {**{f: 0 for f in allw + alln}, "rx": 1, "ra": 1}]):
        b = 2 * k + 1
        for f, val in e.items():
            v[f][b] = bt.ns[b] - 1 if val == "n-1" else val
    c = bt.enc(oracle, [d.below(n) for n in bt.ns], [d.below(n) for n in bt.ns])
    cp = bt.enc(oracle, [d.below(n) for n in bt.ns], [d.below(n) for n in bt.ns])
    stmt = [40, 42, 44, 46]
    for b, val in zip(stmt, ragged(2 * bt.kw, d)):
        set_int(c, b, val)
    a = _verlin_finish(oracle, bt, v, c, cp)
    short = {}
    if n_bits == 1024:
        # item 17: a'' = a0 + k; phi_a = c^a c'^a' r_a^n * (1 + a'' n) mod n^2
        b, n = 17, bt.ns[17]
        nn = n * n
        ci, cpi, phx = get_int(c, b), get_int(cp, b), get_int(a["phi_x"], b)
        base = pow(ci, v["a"][b], nn) * pow(cpi, v["ap"][b], nn) % nn * pow(v["ra"][b], n, nn) % nn
        k = short_challenge(lambda k: pm.compute_digest([n, ci, cpi, phx, base * ((1 + (v["app"][b] + k) * n) % nn) % nn]))
        v["app"][b] += k
        set_int(a["app"], b, v["app"][b])
        short["verlin"] = b
    free = [b for b in range(bt.B) if (b % 2 == 0 or b > 17) and b not in stmt]
    return dict(bt=bt, a=a, free=free, short=short, ragged_statements=stmt, n_minus_1=7, all_set=9)


VERLIN_OUT = ("phi_a", "z", "zp", "zpp", "rz")


def verlin_edits(cs, outs):
    bt, d, free = cs["bt"], pm.Drbg(b"verlin-edits"), Free(cs["free"])
    arrs = dict(c=cs["a"]["c"], cp=cs["a"]["cp"], phi_x=cs["a"]["phi_x"], **dict(zip(VERLIN_OUT, outs)))
    w, zw = 2 * bt.kw, bt.kw + EXTRA
    edits, over = [], []
    for f in ("z", "zp", "zpp"):
        edits.append((free.take(), f, ones(zw)))
    for f, bits in (("zpp", 300), ("zpp", 500), ("z", 400), ("zp", 400)):
        # z'' is the plaintext of Enc(z'', r_z): k * n higher is the same ciphertext.  z and z' are exponents of c and c': it is not.
        i = free.take()
        edits.append((i, f, get_int(arrs[f], i) + (d.bits(bits) | 1 << (bits - 1)) * bt.ns[i]))
        if f == "zpp":
            over.append(i)
    i = free.take(lambda i: get_int(arrs["rz"], i) + bt.ns[i] ** 2 <= ones(w))
    edits.append((i, "rz", get_int(arrs["rz"], i) + bt.ns[i] ** 2)); over.append(i)
    edits += [(free.take(), "rz", ones(w)), (free.take(), "rz", 0)]
    for f in ("c", "cp", "phi_x"):
        i = free.take(lambda i: get_int(arrs[f], i) + bt.ns[i] ** 2 <= ones(w))
        edits += [(i, f, get_int(arrs[f], i) + bt.ns[i] ** 2), (free.take(), f, 0), (free.take(), f, 1)]
    _commit_edits(bt, free, d, arrs, "phi_a", edits)
    for f, v in zip(("phi_x", "cp", "phi_x"), ragged(w, d)[:3]):               # (ragged c: the statements of verlin_edges)
        edits.append((free.take(), f, v))
    return apply_edits(arrs, edits), over


# ====================================================================== MulProof
MUL_IN = ("e_a", "e_b", "e_c", "a", "b", "r_a", "r_b", "r_c", "d", "r_d")
MUL_OUT = ("f", "z1", "z2", "e_d", "e_db")


def _mul_finish(oracle, bt, v, false=()):
    c = [(v["a"][i] * v["b"][i] + (1 if i in false else 0)) % bt.ns[i] for i in range(bt.B)]
    a = {k: L.ints_to_limbs(v[k], bt.kw) for k in ("a", "b", "r_a", "r_b", "r_c", "d", "r_d")}
    a.update(e_a=bt.enc(oracle, v["a"], v["r_a"]), e_b=bt.enc(oracle, v["b"], v["r_b"]), e_c=bt.enc(oracle, c, v["r_c"]))
    return a


def mul_wide(oracle):
    """300 proofs under four 1024-bit keys.  `false`: c = a b + 1 (test_bad_mul_proof, multiplication_proof.rs:232-290); `no_inverse`:
    r_c = p, the prover's mod_inv(..).unwrap() panics (:95); `bad_edb`: the items whose e_db a test replaces by a multiple of p (:135)"""
    bt = Batch(1024, 300, keys_for(1024, 4), False)
    d = pm.Drbg(b"mul-wide")
    v = {k: [d.below(n) for n in bt.ns] for k in ("a", "b", "r_a", "r_b", "r_c", "d", "r_d")}
    D = marked(bt.B)
    false, no_inverse, bad_edb = D[::3], D[1::3], D[2::3]
    a = _mul_finish(oracle, bt, v, false)
    for b in no_inverse:
        set_int(a["r_c"], b, bt.pq[b][0])
    return dict(bt=bt, a=a, false=false, no_inverse=no_inverse, bad_edb=bad_edb, tamper=[1, 62, 65, 254, 258, bt.B - 2])


def mul_edges(oracle, n_bits):
    """40 proofs: odd items 1 ... 19 prover edges (f = 0 at 1, f = n - 1 at 3; a = d = n - 1 at 7, where e a mod n + d = 2 n - e - 1 needs
    more than n_bits bits), 21 (n = 1024) a short challenge"""
    shared = n_bits == 2048
    bt = Batch(n_bits, 40, keys_for(n_bits, 3), shared)
    d = pm.Drbg(b"mul-edges-%d" % n_bits)
    names = ("a", "b", "r_a", "r_b", "r_c", "d", "r_d")
    v = {k: [d.below(n) for n in bt.ns] for k in names}
    top = bt.top
    for k, e in enumerate([dict(a=0, d=0), dict(a=0, d="n-1"), dict(a=1, b=1, d=1), dict(a="n-1", b="n-1", d="n-1"), dict(a=top, b=top, d=top),
                           dict(b=0), dict(r_a=1, r_b=1, r_c=1, r_d=1), dict(r_a="n-1", r_b="n-1", r_c="n-1", r_d="n-1"),
                           dict(r_a=top, r_b=top, r_c=top, r_d=top), dict(a=top, b=0, d=1, r_b=top, r_d="n-1")]):
        b = 2 * k + 1
        for f, val in e.items():
            v[f][b] = bt.ns[b] - 1 if val == "n-1" else val
    short = {}
    if n_bits == 1024:
        # item 21: d = d0 + k; e_d = (1 + d n) r_d^n, e_db = (1 + d b n) (r_d r_b)^n mod n^2 (:63-76)
        b, n = 21, bt.ns[21]
        nn = n * n
        e3 = [pm.enc(n, v["a"][b], v["r_a"][b]), pm.enc(n, v["b"][b], v["r_b"][b]), pm.enc(n, v["a"][b] * v["b"][b] % n, v["r_c"][b])]
        rdn, rdbn = pow(v["r_d"][b], n, nn), pow(v["r_d"][b] * v["r_b"][b], n, nn)
        k = short_challenge(lambda k: pm.compute_digest([n] + e3 + [(1 + (v["d"][b] + k) * n) % nn * rdn % nn,
                                                                    (1 + (v["d"][b] + k) * v["b"][b] * n) % nn * rdbn % nn]))
        v["d"][b] += k
        short["mul"] = b
    a = _mul_finish(oracle, bt, v)
    free = [b for b in range(bt.B) if b % 2 == 0 or b > 21]
    return dict(bt=bt, a=a, free=free, short=short, f_zero=1, f_top=3, carry=7, all_set=9)


def mul_edits(cs, outs):
    bt, d, free = cs["bt"], pm.Drbg(b"mul-edits"), Free(cs["free"])
    arrs = dict(e_a=cs["a"]["e_a"], e_b=cs["a"]["e_b"], e_c=cs["a"]["e_c"], **dict(zip(MUL_OUT, outs)))
    w = 2 * bt.kw
    fits = lambda f: (lambda i: get_int(arrs[f], i) + bt.ns[i] ** 2 <= ones(w))
    edits, over = [(free.take(), "f", 0)], []
    i = free.take()
    edits.append((i, "f", bt.ns[i] - 1))
    for f in ("z1", "z2"):
        i = free.take(fits(f))
        edits.append((i, f, get_int(arrs[f], i) + bt.ns[i] ** 2)); over.append(i)
    edits += [(free.take(), "z1", ones(w)), (free.take(), "z1", 0), (free.take(), "z2", 0)]
    wide_ed = _commit_edits(bt, free, d, arrs, "e_d", edits)                   # (e_d >= n^2: hashed as it is, used modulo n^2)
    i, j = free.take(fits("e_db")), free.take()
    edits += [(i, "e_db", get_int(arrs["e_db"], i) + bt.ns[i] ** 2), (free.take(), "e_db", 0), (free.take(), "e_db", 1),
              (j, "e_db", bt.pq[j][0] * 98765)]                                # a multiple of p: the verifier's mod_inv(..).unwrap() panics (:135)
    i = free.take(fits("e_a"))
    edits += [(i, "e_a", get_int(arrs["e_a"], i) + bt.ns[i] ** 2), (free.take(), "e_c", 0), (free.take(), "e_b", 1)]
    return apply_edits(arrs, edits), over, wide_ed


# ====================================================================== CorrectMessageProof
def _cm_arrays(bt, K, rows):
    kw = bt.kw
    none = lambda w: np.zeros((0, w), np.uint32)
    return dict(valid=np.stack([L.ints_to_limbs(q["valid"], kw) for q in rows]), msg=L.ints_to_limbs([q["msg"] for q in rows], kw),
                r=L.ints_to_limbs([q["r"] for q in rows], kw), w=L.ints_to_limbs([q["w"] for q in rows], kw),
                e_sim=np.stack([L.ints_to_limbs(q["e_sim"], 8) if K > 1 else none(8) for q in rows]),
                z_sim=np.stack([L.ints_to_limbs(q["z_sim"], kw) if K > 1 else none(kw) for q in rows]))


def _cm_rows(bt, K, d):
    rows = []
    for i, n in enumerate(bt.ns):
        valid = [d.below(1 << 64) + 3 for _ in range(K)]
        rows.append(dict(valid=valid, msg=valid[i % K], r=d.below(n), w=d.below(n), e_sim=[d.bits(256) for _ in range(K - 1)],
                         z_sim=[d.below(n) for _ in range(K - 1)]))
    return rows


def cm_wide(K):
    """K = 3: 130 proofs (390 rows) under ONE 1024-bit key; K = 1: 300 proofs under four keys.  `not_listed`: the message is in no row
    (test_incorrect_message_zk_proof, correct_message.rs:184-200); `no_inverse` (K > 1): r = p, so u_i^e_i has no inverse (:76);
    `tamper_z` / `tamper_e`: responses a test flips a bit in (REJECT; the assert_eq! of :138 panics)"""
    B = 130 if K == 3 else 300
    bt = Batch(1024, B, keys_for(1024, 1 if K == 3 else 4), K == 3)
    rows = _cm_rows(bt, K, pm.Drbg(b"cm-wide-%d" % K))
    D = sorted(set(marked(B) + [85, 86]))          # (K = 3: rows 255 and 256 belong to proof 85, row 258 to proof 86)
    not_listed, no_inverse = D[::3], (D[1::3] if K > 1 else [])
    for b in not_listed:
        rows[b]["msg"] = rows[b]["valid"][0] + 1
    for b in no_inverse:
        rows[b]["r"] = bt.pq[b][0]
    rest = [b for b in D if b not in not_listed and b not in no_inverse]
    return dict(bt=bt, K=K, a=_cm_arrays(bt, K, rows), not_listed=not_listed, no_inverse=no_inverse, tamper_z=rest + [1, B - 4], tamper_e=[2, 62, 65, B - 3])


def cm_edges(n_bits):
    """K = 3, 32 proofs: odd items 1 ... 21 prover edges, 23 (n = 1024) a short challenge with e_sim = 0 (so the real row's exponent is the
    short challenge itself)"""
    K = 3
    shared = n_bits == 2048
    bt = Batch(n_bits, 32, keys_for(n_bits, 3), shared)
    d = pm.Drbg(b"cm-edges-%d" % n_bits)
    rows = _cm_rows(bt, K, d)
    top, e_top = bt.top, (1 << 256) - 1
    n_of = lambda b: bt.ns[b]
    edge = [dict(e_sim=[0, 0]), dict(e_sim=[e_top, e_top]), dict(e_sim=[0, e_top]), "duplicate", "not-listed", dict(r=1, w=1), dict(r="n-1", w="n-1"),
            dict(r=top), dict(z_sim=[0, 1]), dict(z_sim=["n-1", top]), "zero-message"]
    for k, e in enumerate(edge):
        b = 2 * k + 1
        q = rows[b]
        if e == "duplicate":                       # the message appears twice in valid_messages (correct_message.rs:68-80, 95-119)
            q["valid"][(b + 1) % K] = q["msg"]
        elif e == "not-listed":
            q["msg"] = q["valid"][0] + 1
        elif e == "zero-message":
            q["valid"][b % K] = q["msg"] = 0
        else:
            for f, val in e.items():
                q[f] = [n_of(b) - 1 if x == "n-1" else x for x in val] if isinstance(val, list) else (n_of(b) - 1 if val == "n-1" else val)
    short = {}
    if n_bits == 1024:
        b, n = 23, bt.ns[23]
        nn = n * n
        q = rows[b]
        q["e_sim"] = [0, 0]
        real = q["valid"].index(q["msg"])
        a_vec = pm.correct_message_prove(n, q["valid"], q["msg"], q["r"], q["e_sim"], q["z_sim"], q["w"])[3]
        a0, g = a_vec[real], pow(2, n, nn)          # w = w0 * 2^k mod n: a = w^n = w0^n * (2^n)^k mod n^2
        k = short_challenge(lambda k: pm.compute_digest(a_vec[:real] + [a0 * pow(g, k, nn) % nn] + a_vec[real + 1:]))
        q["w"] = q["w"] * pow(2, k, n) % n
        short["cm"] = b
    # ordinary items whose simulated z leave room for z + n in kw words (an over-wide response of the same residue: (z + n)^n == z^n mod n^2)
    free = [b for b in range(bt.B) if b % 2 == 0 or b > 23]
    for b in free[:4]:
        rows[b]["z_sim"] = [d.below(1 << (n_bits - 8)) for _ in range(K - 1)]
    return dict(bt=bt, K=K, a=_cm_arrays(bt, K, rows), rows=rows, free=free, short=short, duplicate=7, not_listed=9, roomy=free[:4], n_minus_1=13, all_set=19)


def cm_k1():
    """K = 1, four proofs: the only valid message matches (proofs 0 and 2, the second with message 0) or does not (1 and 3): with no
    simulated row to index, the reference panics (zi_vec[0], correct_message.rs:74)"""
    bt = Batch(1024, 4, keys_for(1024, 2), False)
    rows = _cm_rows(bt, 1, pm.Drbg(b"cm-k1"))
    rows[1]["msg"] = rows[1]["valid"][0] + 1
    rows[2]["valid"][0] = rows[2]["msg"] = 0
    rows[3]["msg"] = 0
    return dict(bt=bt, K=1, a=_cm_arrays(bt, 1, rows), rows=rows)


def cm_edits(cs, ct, e_vec, z_vec, a_vec):
    """one edit per ordinary proof -> (edited arrays, over-wide responses of the same residue, proofs whose e_vec was rebalanced)"""
    bt, K, d, free = cs["bt"], cs["K"], pm.Drbg(b"cm-edits"), Free(cs["free"])
    out = dict(ct=ct.copy(), e_vec=e_vec.copy(), z_vec=z_vec.copy(), a_vec=a_vec.copy())
    w, two = 2 * bt.kw, 1 << 256
    over, rebalanced = [], []
    # z + n in the simulated row (it fits: `roomy`), and ciphertext + n^2 (not hashed: u_i is the same residue)
    i = free.take(lambda i: i in cs["roomy"])
    sim = next(k for k in range(K) if get_int(z_vec[i], k) >> (bt.n_bits - 8) == 0)
    set_int(out["z_vec"][i], sim, get_int(z_vec[i], sim) + bt.ns[i]); over.append(i)
    i = free.take(lambda i: get_int(ct, i) + bt.ns[i] ** 2 <= ones(w))
    set_int(out["ct"], i, get_int(ct, i) + bt.ns[i] ** 2); over.append(i)
    set_int(out["z_vec"][free.take()], 1, bt.top)
    set_int(out["ct"], free.take(), 0)
    # e_vec edits that keep the sum modulo 2^256: the row checks decide (:149-161), not the assert_eq! (:138)
    for kind in ("move-one", "wrap-half", "wrap-one"):
        i = free.take()
        e = [get_int(e_vec[i], k) for k in range(K)]
        if kind == "move-one":
            e[0], e[1] = (e[0] + 1) % two, (e[1] - 1) % two
        elif kind == "wrap-half":
            e[0], e[2] = (e[0] + (1 << 255)) % two, (e[2] + (1 << 255)) % two
        else:
            e[1], e[2] = two - 1, (e[2] + e[1] + 1) % two         # row 1 to 2^256 - 1, row 2 takes the difference: the sum wraps once more
        for k in range(K):
            set_int(out["e_vec"][i], k, e[k])
        rebalanced.append(i)
    i = free.take(lambda i: get_int(a_vec[i], 0) + bt.ns[i] ** 2 <= ones(w))
    set_int(out["a_vec"][i], 0, get_int(a_vec[i], 0) + bt.ns[i] ** 2)
    for k, v in enumerate([0, 1] + ragged(w, d)[:3]):
        set_int(out["a_vec"][free.take()], k % K, v)
    return out, over, rebalanced
