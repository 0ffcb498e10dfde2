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


VB64_BOUNDS = (151, 152, 16535, 16536, 2113687, 2113688)  # the last value of each vbEnc64 form and the first of the next


def vbyte_values64(enc, v0, lens):
    """The values of a compressed vbEnc64 stream at enc[v0:] from its marker
    lengths (vbGet64Inline)."""
    out, c = [], v0
    for ln in lens:
        m = int(enc[c])
        rest = int.from_bytes(bytes(enc[c + 1: c + ln]), "little")
        out.append(m if ln == 1 else ((m - 0x98) << 8) + rest + 152 if m < 0xD8 else ((m - 0xD8) << 16) + rest + 16536 if m < 0xF8 else rest)
        c += ln
    return out


class Block64(tuple):
    """parse64's result: the triple (mode, marker lengths, end), and as
    attributes b (the header's width field: 63 stands for 63 and 64), bx (the
    patch width of a bitmap block, else 0), xn (exceptions) and base (the byte
    range [lo, hi) of the base payload, empty for zero and constant blocks)."""

    def __new__(cls, mode, lens, end, b, bx, xn, base):
        self = tuple.__new__(cls, (mode, lens, end))
        self.mode, self.lens, self.end, self.b, self.bx, self.xn, self.base = mode, lens, end, b, bx, xn, base
        return self

    @property
    def split(self):
        """The mode split by the 128v64 base layout: vertical (the
        pair-swapped 128v32 layout, b <= 32, b = 0 included) or horizontal
        (b > 32).  Width 63 / 64 is always horizontal and keeps its name."""
        if self.mode in ("plain", "bitmap", "vb_raw", "vb_comp"):
            return self.mode + ("_v" if self.b <= 32 else "_h")
        return self.mode


def parse64(enc, pos, n, base_n=None):
    """One block at enc[pos:]: -> Block64, which unpacks as (mode, marker
    lengths of a compressed vbyte stream, end).  base_n: values in the base
    payload (None: n, the "64" layout; 128 for a 128v64 block)."""
    base_n = n if base_n is None else base_n
    h = int(enc[pos])
    b = h & 0x3F
    top = b == 63
    bits = 64 if top else b
    bb = (base_n * bits + 7) // 8
    if h & 0xC0 == 0xC0:
        end = pos + 1 + (bits + 7) // 8
        return Block64("const63" if top else "const", [], end, b, 0, 0, (end, end))
    if h & 0xC0 == 0x40:
        xn = int(enc[pos + 1])
        v0 = pos + 2 + bb
        if enc[v0] == 0xFF:
            return Block64("vb_raw", [], v0 + 1 + 8 * xn + xn, b, 0, xn, (pos + 2, v0))
        lens, c = [], v0
        for _ in range(xn):
            lens.append(marker_len64(int(enc[c])))
            c += lens[-1]
        return Block64("vb_comp", lens, c + xn, b, 0, xn, (pos + 2, v0))
    if h & 0x80:
        bx = int(enc[pos + 1])
        if bx == 0:
            return Block64("bx0", [], pos + 2 + bb, b, 0, 0, (pos + 2, pos + 2 + bb))
        nbm = (n + 7) // 8
        bm = int.from_bytes(bytes(enc[pos + 2: pos + 2 + nbm]), "little") & ((1 << n) - 1)
        xn = bin(bm).count("1")
        end = pos + 2 + nbm + (xn * bx + 7) // 8 + bb
        return Block64("bitmap", [], end, b, bx, xn, (end - bb, end))
    end = pos + 1 + bb
    return Block64("zero" if h == 0 else "plain63" if top else "plain", [], end, b, 0, 0, (pos + 1, end))


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


SPLIT64 = ("zero", "const", "const63", "plain_v", "plain_h", "plain63", "bitmap_v", "bitmap_h",
           "vb_raw_v", "vb_raw_h", "vb_comp_v", "vb_comp_h")


def count64(enc, blocks, split=False):
    """Mode counts and compressed-marker length counts over parsed Block64s
    of enc.  split: the modes are Block64.split's (SPLIT64, by base layout),
    the bitmap blocks are counted once more by patch width, as "bx_le32" and
    "bx_gt32", and the compressed-vbyte exceptions equal to a VB64_BOUNDS
    value k as ("vb", k)."""
    modes, lens = collections.Counter(), collections.Counter()
    for blk in blocks:
        modes[blk.split if split else blk.mode] += 1
        lens.update(blk.lens)
        if split and blk.mode == "bitmap":
            modes["bx_le32" if blk.bx <= 32 else "bx_gt32"] += 1
        if split and blk.mode == "vb_comp":
            modes.update(("vb", k) for k in vbyte_values64(enc, blk.base[1], blk.lens) if k in VB64_BOUNDS)
    return modes, lens


def census64(enc, off, n, halves=1, base_n=None, split=False):
    """count64 over the blocks enc[off[i]:off[i+1]]; halves=2 reads a 256v64
    unit as two 128v64 blocks.  Every parse must end exactly at the next
    offset."""
    blocks = []
    for i in range(len(off) - 1):
        p = int(off[i])
        for _ in range(halves):
            blocks.append(parse64(enc, p, n, base_n))
            p = blocks[-1].end
        assert p == int(off[i + 1]), (i, p, int(off[i + 1]))
    return count64(enc, blocks, split)
