"""The host tokeniser of the wire-format readers (zk-paillier_amd/csrc/json_host.hpp) as a program of its own, under the address and
undefined-behaviour sanitizers (tests/cpp/test_json_host.cpp; no GPU, no library, nothing loaded into this process).  It is the only code of
the library that parses untrusted text: every document is read from a heap block of exactly its length.

  heads-only kinds   the models' mutants of the two DLog and the eight sigma kinds, three text forms, 1024-bit keys: statuses and limbs against
                     the models' read() — what test_gpu_json_sigma.py and test_gpu_json_dlog.py ask of the flags-0 reader on the GPU machine
  range kinds        json_scan_cases.variants for the nine (key form, bare form) pairs through the RangeProofNi top-level tokeniser, then the
                     EncryptedPairs and Proof tokenisers on the spans it names; the expected status of every variant is listed below
  truncation         one canonical document of every kind of the table (fourteen: 0 - 3, 5, 6, 8 - 15): EVERY strict prefix is
                     ZKP_DOC_INVALID and leaves nothing appended — the last byte of a canonical document is the one that closes it"""
import json
import os
import random
import struct
import subprocess

import helpers as H
import json_dlog_model as D
import json_scan_cases as K
import json_sigma_model as M
from helpers import L

ROOT = H.ROOT
OK, INVALID, HOST_PATH = D.DOC_OK, D.DOC_INVALID, D.DOC_HOST_PATH
N_BITS, Y_BITS, EF = 1024, 544, 2
FORMS = (D.BIGINT_DEC, D.BIGINT_HEX, D.BIGINT_BYTES)
PAIRS, PROOF, RANGE_NI, CORRECT_KEY = 0, 1, 2, 3

# What the three tokenisers make of every variant of json_scan_cases.variants, by what its name says.  The numbers of encrypted_pairs and proof
# are strings to the tokeniser — their sign, width and digits are judged by the conversion on the GPU — so a variant that only changes such a
# number is ZKP_DOC_OK here; ek.n, range and ciphertext are converted by the tokeniser itself.
RANGE_STATUS = {
    "canonical": OK, "pretty": OK, "extra field in ek": OK, "reordered fields": OK, "escape in a number": OK, "escape in a name": OK,
    "duplicate field": INVALID, "missing field": INVALID, "truncated by one byte": INVALID, "trailing byte": INVALID, "trailing space": OK, "space inside": OK,
    "negative masked_r": OK, "negative c1": OK, "c1 one bit too wide": OK, "c2 far too long": OK,
    "range too wide": HOST_PATH,                                    # a head the width cannot carry
    "one row less": HOST_PATH, "one c1 more": HOST_PATH, "error_factor 40": HOST_PATH,     # valid values of the type outside the batch layout
    "j 256": INVALID, "j a string": INVALID, "j 1.0": INVALID, "j 01": INVALID, "j 255": OK, "j 0": OK,      # j is a u8
    "unknown variant": INVALID, "row missing its closing": INVALID,
    "small numbers": OK, "longest numbers": OK, "one digit too long": OK, "all nines": OK,
    "longest head numbers": OK, "head one digit too long": OK,      # zero padded: the value fits
    "upper-case hex": OK, "odd-length hex": OK, "hex leading zeros": OK,
    "byte 256": INVALID, "byte 007": INVALID,                       # no u8 / no JSON number
    "empty byte array": OK, "leading zero byte": OK,
    "empty": INVALID,
}


def record(mode, kind, forms, status, limbs, name, doc, ef=EF, y_bits=Y_BITS):
    out = struct.pack("<8I", mode, kind, forms, N_BITS, ef, y_bits, status, len(limbs))
    for row in limbs:
        out += struct.pack("<I", len(row)) + row.astype("<u4").tobytes()
    name = name.encode()
    return out + struct.pack("<I", len(name)) + name + struct.pack("<Q", len(doc)) + bytes(doc)


def heads_cases():
    out = []
    for form in FORMS:
        for kind in (D.PROOF, D.STATEMENT):
            words = D.field_words(kind, N_BITS, Y_BITS)
            rnd = random.Random(kind * 16 + form)
            ints = [rnd.getrandbits(32 * w - 3) | (1 << (32 * w - 4)) for w in words]
            for name, doc, status in D.mutants(kind, form, words, ints):
                st, vals = D.read(doc, kind, form, words)
                assert st == status, (kind, form, name)
                out.append(record(0, kind, form, st, [L.ints_to_limbs([v], w)[0] for v, w in zip(vals, words)], "dlog %d form %d: %s" % (kind, form, name), doc))
        for kind in M.KINDS:
            forms = form << 4 | form
            words = M.field_words(kind, N_BITS)
            rnd = random.Random(kind * 64 + forms)
            ints = [rnd.getrandbits(32 * w - 3) | (1 << (32 * w - 4)) for w in words]
            for name, doc, status in M.mutants(kind, forms, N_BITS, ints):
                st, vals = M.read(doc, kind, forms, N_BITS)
                assert st == status, (kind, forms, name)
                out.append(record(0, kind, forms, st, [L.ints_to_limbs([v], w)[0] for v, w in zip(vals, words)], "%s forms %#x: %s" % (M.NAMES[kind], forms, name), doc))
    return out


def range_cases():
    out = []
    for key_enc in FORMS:
        for enc in FORMS:
            seen = set()
            for name, doc in K.variants(key_enc * 3 + enc, N_BITS, EF, key_enc, enc):
                seen.add(name)
                out.append(record(1, RANGE_NI, key_enc << 4 | enc, RANGE_STATUS[name], [], "RangeProofNi forms %#x: %s" % (key_enc << 4 | enc, name), doc))
            assert {"canonical", "duplicate field", "range too wide", "empty"} <= seen
    return out


def canonical_documents():
    """(kind, forms, document): one of every kind, byte for byte what serde_json::to_string writes"""
    rnd = random.Random(5)
    kw = N_BITS // 32
    ni = dict(K.variants(1, N_BITS, EF, D.BIGINT_HEX, D.BIGINT_DEC))["canonical"]
    parts = json.loads(ni)
    dumps = lambda o: json.dumps(o, separators=(",", ":")).encode()
    docs = [(PAIRS, 0, dumps(parts["encrypted_pairs"])), (PROOF, 0, dumps(parts["proof"])), (RANGE_NI, D.BIGINT_HEX << 4 | D.BIGINT_DEC, ni),
            (CORRECT_KEY, 0, dumps({"sigma_vec": [str(rnd.getrandbits(32 * kw)) for _ in range(11)]}))]
    for i, kind in enumerate((D.PROOF, D.STATEMENT)):
        form = FORMS[i]
        words = D.field_words(kind, N_BITS, Y_BITS)
        docs.append((kind, form, D.write([rnd.getrandbits(32 * w) | 1 << 16 for w in words], kind, form)))
    for i, kind in enumerate(M.KINDS):
        forms = FORMS[i % 3] << 4 | FORMS[(i // 2 + 1) % 3]
        doc = M.write([rnd.getrandbits(32 * w) | 1 << 16 for w in M.field_words(kind, N_BITS)], kind, forms)
        assert M.canonical(doc, kind, forms, N_BITS)
        docs.append((kind, forms, doc))
    assert sorted(k for k, _, _ in docs) == [0, 1, 2, 3, 5, 6] + list(range(8, 16))
    return docs


def test_json_host_tokeniser_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_json_host.cpp")
    exe = os.path.join(ROOT, "build", "test_json_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    cases = heads_cases() + range_cases() + [record(2, kind, forms, OK, [], "prefixes of kind %d forms %#x" % (kind, forms), doc) for kind, forms, doc in canonical_documents()]
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:], out.stderr[-4000:])
    assert out.returncode == 0 and "json host ok" in out.stdout and "0 failures" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
