"""The two DLog document kinds in plain Python (wi_dlog_proof.rs:32-43, field order of the derives):

  CompositeDLogProof   {"x":X,"y":X}
  DLogStatement        {"N":X,"g":X,"ni":X}

Every X is an un-annotated curv BigInt in ONE text form per batch (include/zkp_hip.h: ZKP_BIGINT_*):
  DEC    "D"        1 .. max_digits(words) of 0-9 (leading zeros allowed, as for mpz_set_str)
  HEX    "hh.."     lower case, even length, at most 8 * words characters
  BYTES  [U,U,..]   big-endian byte values 0 .. 255 without leading zeros, at least one, at most 4 * words of them
`words` is the width of the field's array in 32-bit limbs: kw for N, g, ni, x and y_bits / 32 for y.

canonical() / scan() is the grammar the device scanner reads itself (csrc/kernels_serde_scan.hpp): byte for byte what serde_json::to_string gives and
what write() and the GPU writers emit.  read() is what every reader must answer for ANY document: Python's json with duplicate-key
detection, then the value rules of the flags-0 reader.  Statuses as in include/zkp_hip.h."""
import json
import re
import sys

sys.set_int_max_str_digits(0)

BIGINT_DEC, BIGINT_HEX, BIGINT_BYTES = 0, 1, 2
DOC_OK, DOC_INVALID, DOC_HOST_PATH = 0, 2, 3
PROOF, STATEMENT = 5, 6                              # ZKP_JSON_DOC_DLOG_PROOF, ZKP_JSON_DOC_DLOG_STATEMENT
FIELDS = {PROOF: ("x", "y"), STATEMENT: ("N", "g", "ni")}
_DIGITS = b"0123456789"
_HEX = b"0123456789abcdef"


def max_digits(words):
    """zkp_decimal_pitch(words) - 1: no value of `words` 32-bit limbs has more decimal digits"""
    return words * 32 * 30103 // 100000 + 1


def field_words(kind, n_bits, y_bits):
    kw = n_bits // 32
    return (kw, y_bits // 32) if kind == PROOF else (kw, kw, kw)


# ------------------------------------------------------------------ write
def enc_bigint(v, form):
    if form == BIGINT_DEC:
        return str(v)
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return b.hex() if form == BIGINT_HEX else list(b)


def write(ints, kind, form):
    assert len(ints) == len(FIELDS[kind])
    return json.dumps({k: enc_bigint(v, form) for k, v in zip(FIELDS[kind], ints)}, separators=(",", ":")).encode()


# ------------------------------------------------------------------ canonical
def _run(t, p, alphabet):
    q = p
    while q < len(t) and t[q] in alphabet:
        q += 1
    return q


def _value(t, p, form, words):
    """-> position behind the canonical value at t[p], or None"""
    if form == BIGINT_BYTES:
        if t[p:p + 1] != b"[":
            return None
        p += 1
        count = 0
        while True:
            q = _run(t, p, _DIGITS)
            d = t[p:q]
            if not (1 <= len(d) <= 3) or int(d) > 255 or (len(d) > 1 and d[:1] == b"0"):
                return None
            count += 1
            p = q
            if t[p:p + 1] != b",":
                break
            p += 1
        return p + 1 if count <= 4 * words and t[p:p + 1] == b"]" else None
    if t[p:p + 1] != b'"':
        return None
    q = _run(t, p + 1, _DIGITS if form == BIGINT_DEC else _HEX)
    n = q - p - 1
    if n == 0 or t[q:q + 1] != b'"':
        return None
    if form == BIGINT_DEC:
        return q + 1 if n <= max_digits(words) else None
    return q + 1 if n % 2 == 0 and n <= 8 * words else None


def scan(doc, kind, form, words):
    """what the device scanner does: None for a document that is not canonical, else the integers at the grammar's positions (a decimal
    number may still be too large for its field: that is k_dec2bin's overflow, not the grammar's business)"""
    t, p, out = bytes(doc), 0, []
    for i, (name, w) in enumerate(zip(FIELDS[kind], words)):
        lit = (b"{" if i == 0 else b",") + b'"' + name.encode() + b'":'
        if t[p:p + len(lit)] != lit:
            return None
        a = p + len(lit)
        p = _value(t, a, form, w)
        if p is None:
            return None
        body = t[a + 1:p - 1]
        out.append(int(body, 10) if form == BIGINT_DEC else int(body, 16) if form == BIGINT_HEX else int.from_bytes(bytes(int(b) for b in body.split(b",")), "big"))
    return out if t[p:] == b"}" else None


def canonical(doc, kind, form, words):
    return scan(doc, kind, form, words) is not None


# ------------------------------------------------------------------ read
class _Obj(list):
    """the (name, value) pairs of a JSON object, duplicates kept"""


def _field(v, form, words):
    """-> (status, int)"""
    if form == BIGINT_BYTES:
        if not isinstance(v, list) or isinstance(v, _Obj) or any(type(b) is not int or not 0 <= b <= 255 for b in v):
            return DOC_INVALID, 0
        x, neg = int.from_bytes(bytes(v), "big"), False
    else:
        if not isinstance(v, str) or not re.fullmatch(r"-?[0-9]+" if form == BIGINT_DEC else r"-?[0-9a-fA-F]+", v, re.A):
            return DOC_INVALID, 0
        neg = v[0] == "-"
        x = int(v.lstrip("-"), 10 if form == BIGINT_DEC else 16)
    if (neg and x) or x.bit_length() > 32 * words:
        return DOC_HOST_PATH, 0
    return DOC_OK, x


def read(doc, kind, form, words):
    """-> (status, [int per field]); an invalid document reads as zeros, a field the layout cannot carry as zero next to the others"""
    names = FIELDS[kind]
    zeros = [0] * len(names)
    try:
        top = json.loads(bytes(doc).decode("utf-8"), object_pairs_hook=_Obj, parse_constant=lambda s: (_ for _ in ()).throw(ValueError(s)))
    except (ValueError, RecursionError):
        return DOC_INVALID, zeros
    if not isinstance(top, _Obj):
        return DOC_INVALID, zeros
    known = [k for k, _ in top if k in names]
    if sorted(known) != sorted(names):                 # a missing or a duplicate field
        return DOC_INVALID, zeros
    status, out = DOC_OK, dict.fromkeys(names, 0)
    for k, v in top:
        if k not in names:
            continue
        st, x = _field(v, form, words[names.index(k)])
        if st == DOC_INVALID:
            return DOC_INVALID, zeros
        if st == DOC_HOST_PATH:
            status = DOC_HOST_PATH
        out[k] = x
    return status, [out[k] for k in names]


# ------------------------------------------------------------------ the documents around a canonical one
def mutants(kind, form, words, ints):
    """[(name, document, status)] — documents near write(ints), each with the status every reader must give it.  ints: values inside
    their fields, the first one at least 2^16"""
    names = FIELDS[kind]
    good = write(ints, kind, form)
    assert canonical(good, kind, form, words) and ints[0] >= 1 << 16
    v = json.loads(good)
    first = b'"%s":' % names[0].encode()
    val0 = json.dumps(v[names[0]], separators=(",", ":")).encode()
    with_first = lambda raw: good.replace(first + val0, first + raw, 1)
    with_last = lambda x: json.dumps({**v, names[-1]: enc_bigint(x, form)}, separators=(",", ":")).encode()
    wl = words[-1]
    out = [("canonical", good, DOC_OK),
           ("pretty", json.dumps(v, indent=2).encode(), DOC_OK),
           ("reordered", json.dumps({k: v[k] for k in reversed(names)}, separators=(",", ":")).encode(), DOC_OK),
           ("unknown field", good[:-1] + b',"extra":[1,{"a":"b"}]}', DOC_OK),
           ("escaped key", good.replace(first, b'"\\u%04x%s":' % (ord(names[0][0]), names[0][1:].encode()), 1), DOC_OK),
           ("duplicate field", good[:-1] + b"," + first + val0 + b"}", DOC_INVALID),
           ("missing field", good.replace(first, b'"q":', 1), DOC_INVALID),
           ("number for a value", with_first(b"5"), DOC_INVALID),
           ("trailing bytes", good + b"x", DOC_INVALID),
           ("trailing space", good + b" ", DOC_OK),
           ("truncated", good[:-1], DOC_INVALID),
           ("empty", b"", DOC_INVALID),
           ("zero", with_first(json.dumps(enc_bigint(0, form), separators=(",", ":")).encode()), DOC_OK),
           ("first field one bit too wide", with_first(json.dumps(enc_bigint(1 << (32 * words[0]), form), separators=(",", ":")).encode()), DOC_HOST_PATH),
           ("last field fills its width", with_last((1 << (32 * wl)) - 1), DOC_OK),
           ("last field one bit too wide", with_last(1 << (32 * wl)), DOC_HOST_PATH),
           ("last field far too wide", with_last(1 << (64 * wl + 40)), DOC_HOST_PATH)]
    if form == BIGINT_BYTES:
        out += [("sign", with_first(b"[-5]"), DOC_INVALID),
                ("no bytes", with_first(b"[]"), DOC_OK),
                ("byte 256", with_first(b"[256]"), DOC_INVALID),
                ("byte 01", with_first(b"[01]"), DOC_INVALID),
                ("leading zero byte", with_first(b"[0," + val0[1:]), DOC_OK),
                ("string for bytes", with_first(b'"12"'), DOC_INVALID)]
    else:
        out += [("sign", with_first(b'"-5"'), DOC_HOST_PATH),
                ("minus zero", with_first(b'"-0"'), DOC_OK),
                ("empty string", with_first(b'""'), DOC_INVALID),
                ("not a digit", with_first(b'"12g4"'), DOC_INVALID),
                ("bytes for a string", with_first(b"[1,2]"), DOC_INVALID)]
    if form == BIGINT_DEC:
        out += [("leading zeros", with_first(b'"00' + val0[1:]), DOC_OK),
                ("padded to the field", with_first(b'"' + val0[1:-1].rjust(max_digits(words[0]), b"0") + b'"'), DOC_OK),
                ("padded past the field", with_first(b'"' + val0[1:-1].rjust(max_digits(words[0]) + 1, b"0") + b'"'), DOC_OK),
                ("all nines", with_first(b'"' + b"9" * max_digits(words[0]) + b'"'), DOC_HOST_PATH)]
    if form == BIGINT_HEX:
        out += [("upper-case hex", with_first(val0.upper()), DOC_OK),
                ("odd-length hex", with_first(b'"0' + val0[1:]), DOC_OK),
                ("hex leading zero byte", with_first(b'"00' + val0[1:]), DOC_OK)]
    return out
