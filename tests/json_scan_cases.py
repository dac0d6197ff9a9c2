"""Documents for the tests of the device scanner: synthetic RangeProofNi values (no proving: the readers do not care), the variants
tests/test_wire_format.py already builds — through its generators — and the edge cases of the canonical grammar.  Every entry is
(name, document bytes); whether it is canonical is json_scan_model.is_canonical's business, what status it has is the host reader's."""
import json
import random
import re

import json_scan_model as S
import test_wire_format as WF


def synthetic(seed, n_bits, ef, n=None, kinds="mixed"):
    """-> (case, pr) in the shape test_wire_format.range_ni_document takes; j is 1 or 2; kinds: "mixed" | "open" | "mask" """
    rnd = random.Random(seed)
    kw = n_bits // 32
    top, top2 = 1 << (32 * kw), 1 << (64 * kw)
    n = n if n is not None else rnd.randrange(top // 2, top) | 1
    resp = []
    for i in range(ef):
        mask = kinds == "mask" or (kinds == "mixed" and (i == 1 or (i > 1 and rnd.random() < 0.5)))
        if mask:
            resp.append(("mask", 1 + (i & 1), rnd.randrange(top), rnd.randrange(top)))
        else:
            resp.append(("open", rnd.randrange(top), rnd.randrange(top), rnd.randrange(top), rnd.randrange(top)))
    case = {"n": n, "range": rnd.randrange(top)}
    pr = {"ciphertext": rnd.randrange(top2), "c1": [rnd.randrange(top2) for _ in range(ef)], "c2": [rnd.randrange(top2) for _ in range(ef)], "responses": resp}
    return case, pr


def variants(seed, n_bits, ef, key_enc, enc, n=None):
    """one canonical document and everything around it.  ef >= 2 (row 0 is Open, row 1 is Mask)"""
    kw = n_bits // 32
    case, pr = synthetic(seed, n_bits, ef, n)
    doc = lambda c=case, p=pr, **kw_: WF.range_ni_document(c, p, enc, ef, key_enc=key_enc, **kw_)
    good = doc()
    out = [("canonical", good), ("pretty", doc(pretty=True)), ("extra field in ek", doc(extra=True))]
    d = json.loads(good)
    out.append(("reordered fields", json.dumps({k: d[k] for k in ("range", "ek", "proof", "encrypted_pairs", "error_factor", "ciphertext")}, separators=(",", ":")).encode()))
    out.append(("escape in a number", good.replace(b'"w1":"', b'"w1":"\\u0030', 1)))
    out.append(("escape in a name", good.replace(b'"range"', b'"\\u0072ange"', 1)))
    out.append(("duplicate field", good.replace(b'"ek"', b'"ek":{"n":"1"},"ek"', 1)))
    out.append(("missing field", good.replace(b'"range"', b'"rnge"', 1)))
    out.append(("truncated by one byte", good[:-1]))
    out.append(("trailing byte", good + b"x"))
    out.append(("trailing space", good + b" "))
    out.append(("space inside", good.replace(b'"c2":[', b'"c2": [', 1)))
    out.append(("negative masked_r", good.replace(b'"masked_r":"', b'"masked_r":"-', 1)))
    out.append(("negative c1", good.replace(b'"c1":["', b'"c1":["-', 1)))
    wide = dict(pr); wide["c1"] = [1 << (64 * kw)] + pr["c1"][1:]
    out.append(("c1 one bit too wide", doc(p=wide)))
    wide = dict(pr); wide["c2"] = pr["c2"][:-1] + [10 ** (S.max_digits(2 * kw) + 5)]
    out.append(("c2 far too long", doc(p=wide)))
    wide = dict(case); wide["range"] = 1 << (32 * kw + 6)
    out.append(("range too wide", doc(c=wide)))
    fewer = dict(pr); fewer["responses"] = pr["responses"][:-1]
    out.append(("one row less", doc(p=fewer)))
    more = dict(pr); more["c1"] = pr["c1"] + [1]
    out.append(("one c1 more", doc(p=more)))
    other_ef = 40 if ef != 40 else 41
    out.append(("error_factor %d" % other_ef, good.replace(b'"error_factor":%d' % ef, b'"error_factor":%d' % other_ef)))
    for name, j in (("j 256", b"256"), ("j a string", b'"2"'), ("j 1.0", b"1.0"), ("j 01", b"01"), ("j 255", b"255"), ("j 0", b"0")):
        out.append((name, re.sub(rb'"j":\d+', b'"j":' + j, good, count=1)))
    out.append(("unknown variant", good.replace(b'"Open"', b'"Opem"', 1)))
    out.append(("row missing its closing", good.replace(b'}}],"error_factor"', b'],"error_factor"', 1)))
    # edge numbers in every position: "0", "7", "007", and the longest number a field may have (zero padded: a value that fits; all nines: one that does not)
    c1_0, c2_0 = b'"%d"' % pr["c1"][0], b'"%d"' % pr["c2"][0]
    w1_0, mx_1 = b'"w1":"%d"' % pr["responses"][0][1], b'"masked_x":"%d"' % pr["responses"][1][2]
    r2_0 = b'"r2":"%d"' % pr["responses"][0][4]
    dn, dc = S.max_digits(kw), S.max_digits(2 * kw)
    out.append(("small numbers", good.replace(c1_0, b'"0"', 1).replace(c2_0, b'"7"', 1).replace(w1_0, b'"w1":"007"', 1).replace(mx_1, b'"masked_x":"0"', 1)))
    out.append(("longest numbers", good.replace(c1_0, b'"' + str(pr["c1"][0]).zfill(dc).encode() + b'"', 1).replace(w1_0, b'"w1":"' + b"0" * (dn - 1) + b'5"', 1)
                .replace(mx_1, b'"masked_x":"' + str(pr["responses"][1][2]).zfill(dn).encode() + b'"', 1).replace(r2_0, b'"r2":"' + b"0" * dn + b'"', 1)))
    out.append(("one digit too long", good.replace(w1_0, b'"w1":"' + b"0" * dn + b'5"', 1)))
    out.append(("all nines", good.replace(c2_0, b'"' + b"9" * dc + b'"', 1)))
    if enc == S.BIGINT_DEC:
        out.append(("longest head numbers", good.replace(b'"range":"%d"' % case["range"], b'"range":"' + str(case["range"]).zfill(dn).encode() + b'"', 1)))
        out.append(("head one digit too long", good.replace(b'"range":"', b'"range":"' + b"0" * dn, 1)))
    if enc == S.BIGINT_HEX:
        out.append(("upper-case hex", good.replace(b'"range":"%s"' % WF._enc_bigint(case["range"], enc).encode(), b'"range":"%s"' % WF._enc_bigint(case["range"], enc).upper().encode(), 1)))
        out.append(("odd-length hex", good.replace(b'"range":"', b'"range":"0', 1)))
        out.append(("hex leading zeros", good.replace(b'"range":"', b'"range":"00', 1)))
    if enc == S.BIGINT_BYTES:
        out.append(("byte 256", good.replace(b'"range":[', b'"range":[256,', 1)))
        out.append(("byte 007", good.replace(b'"range":[', b'"range":[007,', 1)))
        out.append(("empty byte array", re.sub(rb'"range":\[[0-9,]*\]', b'"range":[]', good, count=1)))
        out.append(("leading zero byte", good.replace(b'"range":[', b'"range":[0,', 1)))
    out.append(("empty", b""))
    return out


def pack(docs, layout="packed"):
    """-> (text bytes, offsets, lengths): "packed" back to back from 0; "gaps": odd offsets, junk between the documents;
    "reverse": as gaps, the documents laid out in reverse order (offsets descending)"""
    order = list(range(len(docs)))
    if layout == "reverse":
        order.reverse()
    text = bytearray()
    off = [0] * len(docs)
    for k, b in enumerate(order):
        if layout != "packed":
            text += b'#"{7' * (k % 3) + b"#"
            if len(text) % 2 == 0:
                text += b"#"
        off[b] = len(text)
        text += docs[b]
    if layout != "packed":
        text += b'"}#'
    return bytes(text) or b" ", off, [len(d) for d in docs]
