"""CPU tests of the verifier's seeded commitment: the model (tests/seeded_commit_model.py) against the oracle and against the model it is
built on, the stream's separation from every other seeded stream, chunk invariance, the conditions tests/seeded_commit_cases.py promises,
and the three entry points' presence and argument checks in the built library (no GPU needed for a refusal)."""
import hashlib

import helpers as H
import seeded_commit_cases as CC
import seeded_commit_model as M
import seeded_coprime_model as CO
import seeded_nonce_model as N
from helpers import L, zkp


def test_kind_seven_streams_collide_with_no_other_seeded_stream():
    mine = {M.word15(f) for f in range(16)}
    assert M.word15(0) == 0x80700000 and M.word15(1) == 0x80700001 and len(mine) == 16
    others = set()
    for kind in (N.KIND_ZERO, N.KIND_CIPHERTEXT, N.KIND_CORRECT_MESSAGE, N.KIND_DLOG):
        for slot in (0, 1, N.MAX_SLOTS - 1):
            others |= {N.word15(kind, slot, f) for f in range(16)}
    for kind, fields in CO.FIELDS.items():
        others |= {CO.word15(kind, 0, f) for f in range(len(fields))}
    assert not mine & others
    # kinds 1 .. 6 over EVERY slot and field: bits 20 .. 30 of word 15 hold the kind, and slot << 4 | field stays below 2^20
    assert (N.MAX_SLOTS - 1) << 4 | 15 < 1 << 20 and all((w >> 20) & 0x7FF == 7 for w in mine)
    assert all(1 <= kind <= 6 for kind in list(CO.FIELDS) + [1, 2, 3, 4])
    # the RangeProofNi streams: word 15 = row << 2 | field < 1024, bit 31 clear
    assert all(w >> 31 for w in mine)
    assert zkp.SEEDED_KIND_RANGE_COMMIT == M.KIND_RANGE_COMMIT == 7


def test_sample_below_is_the_rule_of_the_nonce_model():
    """the same function on a kind both models take: kind 1 (ZeroProof), slot 0, field 0"""
    for n in (CC.key(1024, "pow2"), CC.key(1024, "narrow"), 5, (1 << 600) + 1):
        for index in (0, CC.BIG):
            assert M.sample_below(CC.SEED, index, n, kind=N.KIND_ZERO) == N.sample_below(CC.SEED, index, N.KIND_ZERO, 0, 0, n)
    assert M.sample_below(CC.SEED, 0, CC.key(1024, "pow2")) != M.sample_below(CC.SEED, 0, CC.key(1024, "pow2"), kind=N.KIND_ZERO)


def test_challenge_bytes_are_the_first_bytes_of_block_zero_of_field_one():
    words = M.block(CC.SEED, 0, CC.BIG, 1)
    raw = b"".join(int(w).to_bytes(4, "little") for w in words)
    for e_len in (1, 5, 31, 32):
        assert M.challenge_bytes(CC.SEED, CC.BIG, e_len) == raw[:e_len]


def test_model_commitments_equal_the_oracles_enc_on_the_models_m_and_r(oracle):
    for name in ("1024-narrow-perkey-e1-B4", "2048-pow2-perkey-e5-B4", "1024-full-shared-e5-B1"):
        n_bits, _, shared, e_len, B, first = CC.SHAPES[name]
        keys = CC.keys_of(name)
        ses = M.sessions(CC.SEED, first, keys, B, e_len)
        kw = n_bits // 32
        assert not any(s["status"] for s in ses)
        for s in ses:
            assert s["m"] == int.from_bytes(hashlib.sha256(s["e"]).digest(), "big") and len(s["e"]) == e_len
        com = oracle.paillier_enc(n_bits, CC.key_limbs(keys, n_bits), 0 if shared else kw, L.ints_to_limbs([s["m"] for s in ses], kw),
                                  L.ints_to_limbs([s["r"] for s in ses], kw))
        assert L.limbs_to_ints(com) == [s["com"] for s in ses], name
        for b, s in enumerate(ses):
            n = keys[0] if shared else keys[b]
            assert s["r"] < n and M.verify_commit(n, s["com"], s["r"], s["e"]) == M.ACCEPT
            for what, c2, r2, e2 in CC.tampered(n_bits, n, s["com"], s["r"], s["e"]):
                assert M.verify_commit(n, c2, r2, e2) == M.REJECT, (name, b, what)


def test_model_is_chunk_invariant():
    name = "1024-narrow-perkey-e1-B4"
    n_bits, _, _, e_len, B, first = CC.SHAPES[name]
    keys, one = CC.model(name)
    two = M.sessions(CC.SEED, first, keys[:3], 3, e_len, with_com=False) + M.sessions(CC.SEED, first + 3, keys[3:], B - 3, e_len, with_com=False)
    assert one == two


def test_malformed_sessions_of_the_model():
    good = CC.key(1024, "full")
    keys = [good, 0, good - 1, (1 << 199) + 1, (1 << 256) + 1]
    ses = M.sessions(CC.SEED, 0, keys, 5, 5)
    assert [s["status"] for s in ses] == [0, M.MALFORMED, M.MALFORMED, M.MALFORMED, 0]
    for s in ses[1:4]:
        assert s["r"] == 0 and s["e"] == bytes(5) and s["com"] == 0
    assert M.verify_commit(good - 1, 0, 0, b"") == M.MALFORMED and M.verify_commit(good, 0, 0, bytes(33)) == M.MALFORMED


def test_the_cases_modules_own_conditions():
    widths, shapes, modes, lens, sizes = set(), set(), set(), set(), set()
    for name, (n_bits, shape, shared, e_len, B, first) in CC.SHAPES.items():
        widths.add(n_bits); shapes.add((n_bits, shape)); modes.add(shared); lens.add(e_len); sizes.add(B)
        assert n_bits != 4096 or B <= 70
        for n in CC.keys_of(name):
            assert M.key_in_domain(n) and n.bit_length() <= n_bits
            assert {"full": n.bit_length() == n_bits, "narrow": n.bit_length() % 32 != 0 and n.bit_length() < n_bits - 32,
                    "pow2": n >> (n.bit_length() - 8) == 0x80}[shape], name
    assert widths == {1024, 2048, 4096} and shapes == {(w, s) for w in widths for s in CC.KEY_SHAPES} and modes == {True, False}
    assert lens == {1, 5, 31, 32} and sizes == {1, 4, 70, 300}
    # a key just above a power of two rejects about half the attempts
    _, ses = CC.model("1024-pow2-shared-e31-B70")
    assert 15 <= sum(1 for s in ses if s["rejected"]) <= 55
    # the leading-zero digest
    _, ses = CC.model(CC.ZERO_DIGEST_SHAPE)
    s = ses[CC.ZERO_DIGEST_SESSION]
    assert hashlib.sha256(s["e"]).digest()[0] == 0 and s["m"] < 1 << 248 and s["status"] == 0
    # com + n^2 fits where the key leaves room (not under a key that fills the width), and every tamper is listed
    for name in CC.VERIFY_SHAPES:
        n_bits, shape = CC.SHAPES[name][:2]
        n = CC.keys_of(name)[0]
        names = [t[0] for t in CC.tampered(n_bits, n, n * n - 1, 1, b"\x01\x02")]
        assert ("com+nn" in names) == (shape != "full") and set(names) <= set(CC.TAMPERS)
    assert any(CC.SHAPES[name][1] == "narrow" for name in CC.VERIFY_SHAPES)
    assert set(CC.PINNED_SHAPES) | set(CC.VERIFY_SHAPES) <= set(CC.SHAPES)


def test_new_entry_points_are_exported_and_refuse_bad_arguments_without_a_gpu():
    lib = zkp.load()
    names = ("zkp_range_verifier_commit_seeded_batch", "zkp_range_verifier_reveal_seeded_batch", "zkp_range_verify_commit_batch")
    for name in names:
        assert name in zkp.EXPORTS and hasattr(lib, name)
    E = zkp.capi.ZKP_EINVAL
    assert lib.zkp_range_verifier_commit_seeded_batch(None, 1024, 1, None, 0, 5, bytes(32), 0, None, None, 0) == E
    assert lib.zkp_range_verifier_reveal_seeded_batch(None, 1024, 1, None, 0, 5, bytes(32), 0, None, None, None, 0) == E
    assert lib.zkp_range_verify_commit_batch(None, 1024, 1, None, 0, None, None, None, None, None, 0) == E
    for m in ("range_verifier_commit_seeded", "range_verifier_reveal_seeded", "range_verify_commit"):
        assert callable(getattr(zkp.Context, m))
    header = open(H.ROOT + "/include/zkp_hip.h").read()
    assert "#define ZKP_SEEDED_KIND_RANGE_COMMIT 7u" in header
