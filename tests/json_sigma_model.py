"""The eight sigma-proof document kinds in plain Python (zero_enc_proof.rs:26-41, correct_ciphertext.rs:22-39, verlin_proof.rs:34-57,
multiplication_proof.rs:32-57; serde defaults of the derives, fields in declaration order):

  ZeroStatement        {"ek":{"n":K},"c":X}                                       n [kw], c [2kw]
  ZeroProof            {"z":X,"a":X}                                              z, a [2kw]
  CiphertextStatement  {"ek":{"n":K},"c":X}                                       n [kw], c [2kw]
  CiphertextProof      {"z1":X,"z2":X,"c_prime":X}                                z1 [zw], z2, c_prime [2kw]
  VerlinStatement      {"ek":{"n":K},"c":X,"c_prime":X,"phi_x":X}                 n [kw], c, c_prime, phi_x [2kw]
  VerlinProof          {"phi_a":X,"z":X,"z_prime":X,"z_double_prime":X,"r_z":X}   phi_a, r_z [2kw]; z, z_prime, z_double_prime [zw]
  MulStatement         {"ek":{"n":K},"e_a":X,"e_b":X,"e_c":X}                     n [kw], e_a, e_b, e_c [2kw]
  MulProof             {"f":X,"z1":X,"z2":X,"e_d":X,"e_db":X}                     f [kw]; z1, z2, e_d, e_db [2kw]

kw = n_bits / 32, zw = kw + 16 (ZKP_Z1_EXTRA_LIMBS).  K is ek.n in the batch's KEY form, every X a bare curv BigInt in its BARE form; the
three forms are those of tests/json_dlog_model.py, whose value rules this module reuses.  A document's values are a flat list in the order
above: a statement's first value is its key.

canonical() / scan() is the grammar the device scanner reads itself, byte for byte what write() and the GPU writer emit; read() is what
every reader must answer for ANY document; pair_status() is the status of a (statement, proof) pair in zkp_sigma_verify_json_batch,
domain rule included."""
import json

import json_dlog_model as D
from json_dlog_model import BIGINT_DEC, BIGINT_HEX, BIGINT_BYTES, DOC_OK, DOC_INVALID, DOC_HOST_PATH, max_digits, enc_bigint  # noqa: F401

(ZERO_STATEMENT, ZERO_PROOF, CIPHERTEXT_STATEMENT, CIPHERTEXT_PROOF, VERLIN_STATEMENT, VERLIN_PROOF, MUL_STATEMENT, MUL_PROOF) = KINDS = tuple(range(8, 16))
NAMES = {ZERO_STATEMENT: "ZeroStatement", ZERO_PROOF: "ZeroProof", CIPHERTEXT_STATEMENT: "CiphertextStatement", CIPHERTEXT_PROOF: "CiphertextProof",
         VERLIN_STATEMENT: "VerlinStatement", VERLIN_PROOF: "VerlinProof", MUL_STATEMENT: "MulStatement", MUL_PROOF: "MulProof"}
PROOF_KINDS = (ZERO_PROOF, CIPHERTEXT_PROOF, VERLIN_PROOF, MUL_PROOF)
Z1_EXTRA_LIMBS = 16
N, NN, Z = "n", "nn", "z"                       # widths: kw, 2 kw, kw + Z1_EXTRA_LIMBS
# (field name, width); "ek" is the key: the object {"n":K}
FIELDS = {
    ZERO_STATEMENT: (("ek", N), ("c", NN)),
    ZERO_PROOF: (("z", NN), ("a", NN)),
    CIPHERTEXT_STATEMENT: (("ek", N), ("c", NN)),
    CIPHERTEXT_PROOF: (("z1", Z), ("z2", NN), ("c_prime", NN)),
    VERLIN_STATEMENT: (("ek", N), ("c", NN), ("c_prime", NN), ("phi_x", NN)),
    VERLIN_PROOF: (("phi_a", NN), ("z", Z), ("z_prime", Z), ("z_double_prime", Z), ("r_z", NN)),
    MUL_STATEMENT: (("ek", N), ("e_a", NN), ("e_b", NN), ("e_c", NN)),
    MUL_PROOF: (("f", N), ("z1", NN), ("z2", NN), ("e_d", NN), ("e_db", NN)),
}


def is_statement(kind):
    return kind % 2 == 0


def field_words(kind, n_bits):
    kw = n_bits // 32
    return tuple({N: kw, NN: 2 * kw, Z: kw + Z1_EXTRA_LIMBS}[w] for _, w in FIELDS[kind])


def forms_of(kind, forms):
    """the text form of every field: forms = (key_form << 4) | bare_form"""
    return tuple(forms >> 4 if name == "ek" else forms & 15 for name, _ in FIELDS[kind])


# ------------------------------------------------------------------ write
def as_dict(ints, kind, forms):
    """the obvious dict: what serde_json serialises"""
    assert len(ints) == len(FIELDS[kind])
    return {name: {"n": enc_bigint(v, f)} if name == "ek" else enc_bigint(v, f) for (name, _), v, f in zip(FIELDS[kind], ints, forms_of(kind, forms))}


def write(ints, kind, forms):
    """the canonical text, put together from the grammar's literals (test_json_sigma_model.py holds it against json.dumps of as_dict())"""
    out = b""
    for i, ((name, _), v, f) in enumerate(zip(FIELDS[kind], ints, forms_of(kind, forms))):
        lit = b'{"ek":{"n":' if name == "ek" else (b"{" if i == 0 else b"}," if FIELDS[kind][i - 1][0] == "ek" else b",") + b'"' + name.encode() + b'":'
        out += lit + json.dumps(enc_bigint(v, f), separators=(",", ":")).encode()
    return out + b"}"


def doc_bound(kind, n_bits, forms):
    """zkp_json_doc_bound: every literal, every number at its widest between its quotes or brackets, the closing brace"""
    def widest(words, form):
        nb = 4 * words
        return max_digits(words) if form == BIGINT_DEC else 2 * nb if form == BIGINT_HEX else 4 * nb - 1
    if kind not in KINDS or n_bits not in (1024, 2048, 4096) or forms >> 8 or forms >> 4 > BIGINT_BYTES or forms & 15 > BIGINT_BYTES:
        return 0
    zero = write([0] * len(FIELDS[kind]), kind, 0)                       # every number is "0": three bytes
    return len(zero) - 3 * len(FIELDS[kind]) + sum(2 + widest(w, f) for w, f in zip(field_words(kind, n_bits), forms_of(kind, forms)))


# ------------------------------------------------------------------ canonical
def scan(doc, kind, forms, n_bits):
    """what the device scanner does: None for a document that is not canonical, else the integers at the grammar's positions"""
    t, p, out = bytes(doc), 0, []
    fs, ws = forms_of(kind, forms), field_words(kind, n_bits)
    for i, (name, _) in enumerate(FIELDS[kind]):
        lit = b'{"ek":{"n":' if name == "ek" else (b"{" if i == 0 else b"}," if FIELDS[kind][i - 1][0] == "ek" else b",") + b'"' + name.encode() + b'":'
        if t[p:p + len(lit)] != lit:
            return None
        a = p + len(lit)
        p = D._value(t, a, fs[i], ws[i])
        if p is None:
            return None
        body = t[a + 1:p - 1]
        out.append(int(body, 10) if fs[i] == BIGINT_DEC else int(body, 16) if fs[i] == BIGINT_HEX else int.from_bytes(bytes(int(b) for b in body.split(b",")), "big"))
    return out if t[p:] == b"}" else None


def canonical(doc, kind, forms, n_bits):
    return scan(doc, kind, forms, n_bits) is not None


# ------------------------------------------------------------------ read
def _unique(obj, names):
    """{name: value} of the known fields of a JSON object, or None when one is missing or there twice"""
    known = [k for k, _ in obj if k in names]
    return {k: v for k, v in obj if k in names} if sorted(known) == sorted(names) else None


def read(doc, kind, forms, n_bits):
    """-> (status, [int per field]); an invalid document reads as zeros, a field the layout cannot carry as zero next to the others"""
    names = [name for name, _ in FIELDS[kind]]
    zeros = [0] * len(names)
    try:
        top = json.loads(bytes(doc).decode("utf-8"), object_pairs_hook=D._Obj, parse_constant=lambda s: (_ for _ in ()).throw(ValueError(s)))
    except (ValueError, RecursionError):
        return DOC_INVALID, zeros
    got = _unique(top, names) if isinstance(top, D._Obj) else None
    if got is None:
        return DOC_INVALID, zeros
    status, out = DOC_OK, []
    for name, form, words in zip(names, forms_of(kind, forms), field_words(kind, n_bits)):
        v = got[name]
        if name == "ek":                                   # EncryptionKey: an object with a field "n" (its other fields are skipped)
            v = _unique(v, ["n"]) if isinstance(v, D._Obj) else None
            if v is None:
                return DOC_INVALID, zeros
            v = v["n"]
        st, x = D._field(v, form, words)
        if st == DOC_INVALID:
            return DOC_INVALID, zeros
        if st == DOC_HOST_PATH:
            status = DOC_HOST_PATH
        out.append(x)
    return status, out


# ------------------------------------------------------------------ a (statement, proof) pair
def in_domain(proof_kind, st_ints, pf_ints):
    """the domain of the limb kernels: an odd key of at least 2 bits... that is n >= 3; every 2 kw field below n^2; MulProof.f below n"""
    n = st_ints[0]
    if n < 2 or n % 2 == 0:
        return False
    fields = list(zip(FIELDS[proof_kind - 1][1:], st_ints[1:])) + list(zip(FIELDS[proof_kind], pf_ints))
    return all(v < n * n for (_, w), v in fields if w == NN) and all(v < n for (name, w), v in fields if w == N)


def pair_status(proof_kind, statement, proof, forms, n_bits):
    """-> (status, statement ints, proof ints) as zkp_sigma_verify_json_batch sees the pair: the worse of the two documents' statuses, then
    the domain rule; a pair that is not OK has no values"""
    s1, a = read(statement, proof_kind - 1, forms, n_bits)
    s2, b = read(proof, proof_kind, forms, n_bits)
    st = DOC_INVALID if DOC_INVALID in (s1, s2) else DOC_HOST_PATH if DOC_HOST_PATH in (s1, s2) else DOC_OK
    if st == DOC_OK and not in_domain(proof_kind, a, b):
        st = DOC_HOST_PATH
    return (st, a, b) if st == DOC_OK else (st, None, None)


# ------------------------------------------------------------------ the documents around a canonical one
def mutants(kind, forms, n_bits, ints):
    """[(name, document, status)] — documents near write(ints), each with the status every reader must give it.  ints: values inside their
    fields, every one at least 2^16"""
    names = [name for name, _ in FIELDS[kind]]
    ws, fs = field_words(kind, n_bits), forms_of(kind, forms)
    good = write(ints, kind, forms)
    assert canonical(good, kind, forms, n_bits) and min(ints) >= 1 << 16
    v = as_dict(ints, kind, forms)
    dumps = lambda o: json.dumps(o, separators=(",", ":")).encode()
    last, wl, fl = names[-1], ws[-1], fs[-1]
    with_last = lambda x: dumps({**v, last: enc_bigint(x, fl)})
    raw_last = lambda raw: good[:good.rindex(b'"%s":' % last.encode()) + len(last) + 3] + raw + b"}"
    first = b'"%s":' % names[0].encode()
    out = [("canonical", good, DOC_OK),
           ("pretty", json.dumps(v, indent=2).encode(), DOC_OK),
           ("reordered", dumps({k: v[k] for k in reversed(names)}), DOC_OK),
           ("unknown field", good[:-1] + b',"extra":[1,{"a":"b"}]}', DOC_OK),
           ("escaped key", good.replace(first, b'"\\u%04x%s":' % (ord(names[0][0]), names[0][1:].encode()), 1), DOC_OK),
           ("duplicate field", good[:-1] + b',"%s":' % last.encode() + dumps(v[last]) + b"}", DOC_INVALID),
           ("missing field", good.replace(b'"%s":' % last.encode(), b'"q":', 1), DOC_INVALID),
           ("number for a value", raw_last(b"5"), DOC_INVALID),
           ("object for a value", raw_last(b'{"n":"5"}'), DOC_INVALID),
           ("trailing bytes", good + b"x", DOC_INVALID),
           ("trailing space", good + b" ", DOC_OK),
           ("truncated", good[:-1], DOC_INVALID),
           ("empty", b"", DOC_INVALID),
           ("zero", with_last(0), DOC_OK),
           ("last field fills its width", with_last((1 << (32 * wl)) - 1), DOC_OK),
           ("last field one bit too wide", with_last(1 << (32 * wl)), DOC_HOST_PATH),
           ("last field far too wide", with_last(1 << (64 * wl + 40)), DOC_HOST_PATH)]
    if fl == BIGINT_BYTES:
        out += [("sign", raw_last(b"[-5]"), DOC_INVALID), ("no bytes", raw_last(b"[]"), DOC_OK), ("byte 256", raw_last(b"[256]"), DOC_INVALID),
                ("leading zero byte", raw_last(b"[0," + dumps(v[last])[1:]), DOC_OK), ("string for bytes", raw_last(b'"12"'), DOC_INVALID)]
    else:
        out += [("negative", raw_last(b'"-5"'), DOC_HOST_PATH), ("minus zero", raw_last(b'"-0"'), DOC_OK), ("empty string", raw_last(b'""'), DOC_INVALID),
                ("not a digit", raw_last(b'"12g4"'), DOC_INVALID), ("bytes for a string", raw_last(b"[1,2]"), DOC_INVALID)]
    if fl == BIGINT_DEC:
        digits = dumps(v[last])[1:-1]
        out += [("padded to the field", raw_last(b'"' + digits.rjust(max_digits(wl), b"0") + b'"'), DOC_OK),
                ("padded past the field", raw_last(b'"' + digits.rjust(max_digits(wl) + 1, b"0") + b'"'), DOC_OK),
                ("all nines", raw_last(b'"' + b"9" * max_digits(wl) + b'"'), DOC_HOST_PATH)]
    if fl == BIGINT_HEX:
        out += [("upper-case hex", raw_last(dumps(v[last]).upper()), DOC_OK), ("odd-length hex", raw_last(b'"0' + dumps(v[last])[1:]), DOC_OK)]
    if is_statement(kind):
        key = dumps(v["ek"]["n"])
        ek = lambda raw: good.replace(b'{"ek":{"n":' + key + b"}", b'{"ek":' + raw, 1)
        out += [("key with other fields", ek(b'{"nn":"9","n":' + key + b"}"), DOC_OK),
                ("key without n", ek(b'{"nn":"9"}'), DOC_INVALID),
                ("key with n twice", ek(b'{"n":' + key + b',"n":' + key + b"}"), DOC_INVALID),
                ("key not an object", ek(key), DOC_INVALID),
                ("key one bit too wide", ek(dumps({"n": enc_bigint(1 << (32 * ws[0]), fs[0])})), DOC_HOST_PATH)]
    return out
