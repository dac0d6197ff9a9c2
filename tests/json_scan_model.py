"""The canonical grammar of a RangeProofNi document, as the device scanner (csrc/kernels_serde_scan.hpp) accepts it: byte for byte what
serde_json::to_string writes for the reference's derives, and what the writers emit.  is_canonical() is the acceptance predicate the tests
use: a document it accepts must be read on the device (no fall back), a document it refuses must end up with the host reader's status.

  {"ek":{"n":X},"range":X,"ciphertext":X,"encrypted_pairs":{"c1":["D",..],"c2":["D",..]},"proof":[ROW,..],"error_factor":N}
  ROW = {"Open":{"w1":"D","r1":"D","w2":"D","r2":"D"}} | {"Mask":{"j":U,"masked_x":"D","masked_r":"D"}}
  D   = 1 .. max_digits(field) of 0-9 (leading zeros allowed, as for mpz_set_str)
  U   = 0 .. 255, one to three digits, no leading zero
  N   = the batch's error_factor; exactly error_factor entries in c1, in c2 and in proof
  X   = "D" | "hex": lower case, even length, at most two characters per byte of the field | [U,U,..]: at most as many bytes as the field has"""

BIGINT_DEC, BIGINT_HEX, BIGINT_BYTES = 0, 1, 2
_DIGITS = b"0123456789"
_HEX = b"0123456789abcdef"


def max_digits(words):
    """zkp_decimal_pitch(words) - 1: no value of `words` 32-bit limbs has more decimal digits"""
    return words * 32 * 30103 // 100000 + 1


class _Cur:
    def __init__(self, doc):
        self.t, self.p = doc, 0

    def lit(self, s):
        if self.t[self.p:self.p + len(s)] != s:
            return False
        self.p += len(s)
        return True

    def run(self, alphabet):
        q = self.p
        while q < len(self.t) and self.t[q] in alphabet:
            q += 1
        out, self.p = self.t[self.p:q], q
        return out

    def dec(self, words):
        d = self.lit(b'"') and self.run(_DIGITS)
        return bool(d) and len(d) <= max_digits(words) and self.lit(b'"')

    def u8(self):
        d = self.run(_DIGITS)
        return 1 <= len(d) <= 3 and int(d) <= 255 and not (len(d) > 1 and d[:1] == b"0")

    def head(self, form, words):
        if form == BIGINT_DEC:
            return self.dec(words)
        if form == BIGINT_HEX:
            h = self.lit(b'"') and self.run(_HEX)
            return bool(h) and len(h) % 2 == 0 and len(h) <= 8 * words and self.lit(b'"')
        if not self.lit(b"["):
            return False
        count = 0
        while True:
            if not self.u8():
                return False
            count += 1
            if not self.lit(b","):
                break
        return count <= 4 * words and self.lit(b"]")


def is_canonical(doc: bytes, n_bits: int, ef: int, key_form: int = BIGINT_DEC, bare_form: int = BIGINT_DEC) -> bool:
    kw = n_bits // 32
    c = _Cur(bytes(doc))
    ok = (c.lit(b'{"ek":{"n":') and c.head(key_form, kw) and c.lit(b'},"range":') and c.head(bare_form, kw) and c.lit(b',"ciphertext":')
          and c.head(bare_form, 2 * kw) and c.lit(b',"encrypted_pairs":{"c1":['))
    if not ok:
        return False
    for which in range(2):
        for i in range(ef):
            if (i and not c.lit(b",")) or not c.dec(2 * kw):
                return False
        if not c.lit(b'],"c2":[' if which == 0 else b']},"proof":['):
            return False
    for i in range(ef):
        if i and not c.lit(b","):
            return False
        if c.lit(b'{"Open":{"w1":'):
            ok = c.dec(kw) and c.lit(b',"r1":') and c.dec(kw) and c.lit(b',"w2":') and c.dec(kw) and c.lit(b',"r2":') and c.dec(kw)
        elif c.lit(b'{"Mask":{"j":'):
            ok = c.u8() and c.lit(b',"masked_x":') and c.dec(kw) and c.lit(b',"masked_r":') and c.dec(kw)
        else:
            return False
        if not ok or not c.lit(b"}}"):
            return False
    return c.lit(b'],"error_factor":' + str(ef).encode() + b"}") and c.p == len(c.t)
