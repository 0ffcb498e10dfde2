"""Reads the mode of P4 blocks from their bytes (header byte, bx / xn byte,
first vbyte byte), so that tests can assert which encoder and decoder paths
their inputs reach -- from the oracle's bytes, before any device runs.
Test infrastructure only.

Layouts (oracle/tpf_oracle.h): "64" and "32" hold n values in their base
payload, pad8(n * b) bytes; "128v64" and "128v32" hold 128, 16 * b bytes at
every width and every n; "256v32" holds 256, 32 * b bytes."""
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


MODES32 = ("zero", "plain", "plain32", "const", "const32", "bitmap", "bx0", "vb_raw", "vb_comp")
BASE_N32 = {"32": None, "128v32": 128, "256v32": 256}


def marker_len32(m):
    """Bytes of one vbEnc32 value from its first byte (vbGet32Inline)."""
    return 1 if m < 0x9C else 2 if m < 0xDC else 3 if m < 0xFC else 4 if m == 0xFC else 5


def parse32(enc, pos, n, base_n=None):
    """One 32-bit block at enc[pos:]: -> (mode, marker lengths of a compressed
    vbEnc32 stream, end).  base_n: values in the base payload (None: n, the
    horizontal "32" layout, pad8(n * b) bytes; 128 for 128v32, 16 * b bytes;
    256 for 256v32, 32 * b bytes).  The bitmap holds n bits at every layout."""
    base_n = n if base_n is None else base_n
    h = int(enc[pos])
    b = h & 0x3F
    assert b <= 32, (pos, h)
    bb = (base_n * b + 7) // 8
    if h & 0xC0 == 0xC0:
        return ("const32" if b == 32 else "const"), [], pos + 1 + (b + 7) // 8
    if h & 0xC0 == 0x40:
        xn = int(enc[pos + 1])
        v0 = pos + 2 + bb
        if enc[v0] == 0xFF:
            return "vb_raw", [], v0 + 1 + 4 * xn + xn
        lens, c = [], v0
        for _ in range(xn):
            lens.append(marker_len32(int(enc[c])))
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
    return ("zero" if h == 0 else "plain32" if b == 32 else "plain"), [], pos + 1 + bb


def census32(enc, off, n, base_n=None):
    """Mode counts and compressed-marker length counts over the 32-bit blocks
    enc[off[i]:off[i+1]].  Every parse must end exactly at the next offset."""
    modes, lens = collections.Counter(), collections.Counter()
    for i in range(len(off) - 1):
        m, ls, p = parse32(enc, int(off[i]), n, base_n)
        modes[m] += 1
        lens.update(ls)
        assert p == int(off[i + 1]), (i, m, p, int(off[i + 1]))
    return modes, lens


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
