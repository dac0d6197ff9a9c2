"""The canonical grammars of the three smaller document kinds, as the device scanner (csrc/kernels_serde_scan.hpp) accepts them: byte for
byte what serde_json::to_string writes for the reference's derives and what the writers emit (tests/json_writer_model.py).

  NiCorrectKeyProof  {"sigma_vec":["D",..11]}
  EncryptedPairs     {"c1":["D",..EF],"c2":["D",..EF]}
  Proof              [ROW,..EF]
  ROW = {"Open":{"w1":"D","r1":"D","w2":"D","r2":"D"}} | {"Mask":{"j":U,"masked_x":"D","masked_r":"D"}}
  D   = 1 .. max_digits(field) of 0-9 (leading zeros allowed, as for mpz_set_str); U = 0 .. 255, no leading zero

scan(kind, doc, n_bits, ef) is the whole interface: None = fall back (the host tokeniser reads the document and decides its status), else
the list of (position, length) of the document's numbers, in document order — which is the order of the scanner's items: sigma_vec[i];
c1[0..EF) then c2[0..EF); per row w1, r1, w2, r2 or masked_x, masked_r.  rows() gives the other half of a Proof: (is_mask, j) per row."""

DOC_PAIRS, DOC_PROOF, DOC_CK = 0, 1, 3      # include/zkp_hip.h: ZKP_JSON_DOC_*
SIGMA_COUNT = 11                           # ZKP_CORRECT_KEY_M2
_DIGITS = b"0123456789"


def max_digits(words):
    """zkp_decimal_pitch(words) - 1: no value of `words` 32-bit limbs has more decimal digits"""
    return words * 32 * 30103 // 100000 + 1


class _Cur:
    def __init__(self, doc):
        self.t, self.p, self.numbers, self.rows = bytes(doc), 0, [], []

    def lit(self, s):
        if self.t[self.p:self.p + len(s)] != s:
            return False
        self.p += len(s)
        return True

    def digits(self):
        q = self.p
        while q < len(self.t) and self.t[q] in _DIGITS:
            q += 1
        out, self.p = self.t[self.p:q], q
        return out

    def dec(self, words):
        if not self.lit(b'"'):
            return False
        at = self.p
        d = self.digits()
        if not d or len(d) > max_digits(words) or not self.lit(b'"'):
            return False
        self.numbers.append((at, len(d)))
        return True

    def u8(self):
        d = self.digits()
        if not (1 <= len(d) <= 3) or int(d) > 255 or (len(d) > 1 and d[:1] == b"0"):
            return None
        return int(d)

    def array(self, count, words):
        """"D","D",.. without the brackets"""
        for i in range(count):
            if (i and not self.lit(b",")) or not self.dec(words):
                return False
        return True

    def row(self, kw):
        if self.lit(b'{"Open":{"w1":'):
            ok = self.dec(kw) and self.lit(b',"r1":') and self.dec(kw) and self.lit(b',"w2":') and self.dec(kw) and self.lit(b',"r2":') and self.dec(kw)
            self.rows.append((False, 0))
        elif self.lit(b'{"Mask":{"j":'):
            j = self.u8()
            ok = j is not None and self.lit(b',"masked_x":') and self.dec(kw) and self.lit(b',"masked_r":') and self.dec(kw)
            self.rows.append((True, j))
        else:
            return False
        return ok and self.lit(b"}}")


def doc_bound(kind, n_bits, ef):
    """zkp_json_doc_bound for the three kinds"""
    kw = n_bits // 32
    dn, dc = max_digits(kw), max_digits(2 * kw)
    if kind == DOC_CK:
        return len(b'{"sigma_vec":[') + SIGMA_COUNT * (dn + 3) - 1 + len(b"]}")
    if kind == DOC_PAIRS:
        return len(b'{"c1":[') + len(b'],"c2":[') + len(b"]}") + 2 * (ef * (dc + 3) - 1)
    open_row = len(b'{"Open":{"w1":"","r1":"","w2":"","r2":""}}') + 4 * dn
    mask_row = len(b'{"Mask":{"j":255,"masked_x":"","masked_r":""}}') + 2 * dn
    return 2 + ef * (max(open_row, mask_row) + 1) - 1


def _scan(kind, doc, n_bits, ef):
    kw = n_bits // 32
    c = _Cur(doc)
    if len(c.t) == 0 or len(c.t) > doc_bound(kind, n_bits, ef):
        return None
    if kind == DOC_CK:
        ok = c.lit(b'{"sigma_vec":[') and c.array(SIGMA_COUNT, kw) and c.lit(b"]}")
    elif kind == DOC_PAIRS:
        ok = c.lit(b'{"c1":[') and c.array(ef, 2 * kw) and c.lit(b'],"c2":[') and c.array(ef, 2 * kw) and c.lit(b"]}")
    elif kind == DOC_PROOF:
        ok = c.lit(b"[")
        for i in range(ef):
            ok = ok and (i == 0 or c.lit(b",")) and c.row(kw)
        ok = ok and c.lit(b"]")
    else:
        raise ValueError(kind)
    return c if ok and c.p == len(c.t) else None


def scan(kind, doc, n_bits, ef=0):
    c = _scan(kind, doc, n_bits, ef)
    return None if c is None else c.numbers


def rows(doc, n_bits, ef):
    c = _scan(DOC_PROOF, doc, n_bits, ef)
    return None if c is None else c.rows


def is_canonical(kind, doc, n_bits, ef=0):
    return _scan(kind, doc, n_bits, ef) is not None
