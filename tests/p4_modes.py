"""Reads the mode of 64-bit P4 blocks from their bytes (header byte, bx / xn
byte, first vbyte byte), so that tests can assert which encoder and decoder
paths their inputs reach -- from the oracle's bytes, before any device runs.
Test infrastructure only.

Layouts (oracle/tpf_oracle.h): "64" holds n values in its base payload,
pad8(n * b) bytes; "128v64" holds 128, 16 * b bytes at every width."""
import collections

MODES64 = ("zero", "plain", "plain63", "const", "const63", "bitmap", "bx0", "vb_raw", "vb_comp")


def marker_len64(m):
    """Bytes of one vbEnc64 value from its first byte (vbGet64Inline)."""
    return 1 if m < 0x98 else 2 if m < 0xD8 else 3 if m < 0xF8 else m - 0xF8 + 4


def parse64(enc, pos, n, base_n=None):
    """One block at enc[pos:]: -> (mode, marker lengths of a compressed vbyte
    stream, end).  base_n: values in the base payload (None: n, the "64"
    layout; 128 for a 128v64 block)."""
    base_n = n if base_n is None else base_n
    h = int(enc[pos])
    b = h & 0x3F
    top = b == 63
    bits = 64 if top else b
    bb = (base_n * bits + 7) // 8
    if h & 0xC0 == 0xC0:
        return ("const63" if top else "const"), [], pos + 1 + (bits + 7) // 8
    if h & 0xC0 == 0x40:
        xn = int(enc[pos + 1])
        v0 = pos + 2 + bb
        if enc[v0] == 0xFF:
            return "vb_raw", [], v0 + 1 + 8 * xn + xn
        lens, c = [], v0
        for _ in range(xn):
            lens.append(marker_len64(int(enc[c])))
            c += lens[-1]
        return "vb_comp", lens, c + xn
    if h & 0x80:
        bx = int(enc[pos + 1])
        if bx == 0:
            return "bx0", [], pos + 2 + bb
        nbm = (n + 7) // 8
        bm = int.from_bytes(bytes(enc[pos + 2: pos + 2 + nbm]), "little") & ((1 << n) - 1)
        xn = bin(bm).count("1")
        return "bitmap", [], pos + 2 + nbm + (xn * bx + 7) // 8 + bb
    return ("zero" if h == 0 else "plain63" if top else "plain"), [], pos + 1 + bb


def census64(enc, off, n, halves=1, base_n=None):
    """Mode counts and compressed-marker length counts over the blocks
    enc[off[i]:off[i+1]]; halves=2 reads a 256v64 unit as two 128v64 blocks.
    Every parse must end exactly at the next offset."""
    modes, lens = collections.Counter(), collections.Counter()
    for i in range(len(off) - 1):
        p = int(off[i])
        for _ in range(halves):
            m, ls, p = parse64(enc, p, n, base_n)
            modes[m] += 1
            lens.update(ls)
        assert p == int(off[i + 1]), (i, p, int(off[i + 1]))
    return modes, lens
