"""Where the values of a compressed vbyte stream fall: layout classes read from
the oracle's bytes, one seeded family of units per (fmt, n) that holds every
class the encoder reaches there, a decode-only family beyond the encoder's
reach, and deliberately wrong restatements of the device's parses (MUTANTS) --
the inputs of tests/test_vbyte_layouts_cpu.py and tests/test_gpu_vbyte_layouts.py.

A block with compressed vbyte exceptions is header 0x40 | b, xn, the base
payload, the vbEnc stream V of the xn excess values and the xn positions.  Every
device parse of V works in 64-byte windows (p4_block32.h vbyte_exceptions,
p4_generic.h vbyte_exceptions_g) or, for the phase-A lane sums, takes a short
form when V is 64 bytes or shorter and every value 1 or 2 bytes long
(p4_dsum_lanes.h).  The classes (facts) name what those parses can get wrong:

  ("W", w)            V spans w windows, w = (|V| - 1) // 64 + 1
  ("end", L, s)       a value of L bytes ends s bytes past a multiple of 64 of V (s = 0: on the boundary)
  ("short", k)        every value 1 or 2 bytes, |V| = k, k = 62..66: either side of the short form's length rule
  ("one_long", w)     |V| <= 64 and exactly one value of 3 bytes or more, the first, a middle or the last one
  ("run", k, par)     32-bit, short form only: a maximal run of bytes in [0x9C, 0xDC) of length k (1..8, "9-15",
                      "16+") that starts at an even (0) or odd (1) offset of V
  ("run_at", e)       ... a run that begins at V's byte 0 ("start") or ends at its last byte ("end")
  ("run_last", w)     ... a run whose last byte is a marker, or a data byte
  ("xn", k)           k exceptions, k in XN
  ("v1024",)          256v32: at some placement of the unit V holds byte 1024 of the 16-byte-aligned block image
  ("vb_raw",)         the raw escape (0xFF, the excess values as words): its length rule, for the size mutant

A family is built by direction and rejection: per class, units are drawn (a
grid over the cost model's inputs where the class is a matter of size, then
tries(class) random draws) with the exceptions laid out in position order so that the excess values
appear in V in the order drawn, encoded by the oracle, and kept if the oracle's
bytes hold the class (the encoder is free to choose another width or the bitmap
patch).  A class no draw reaches stands in UNREACHED; tests assert that table
exactly and repeat the draws that missed.  Test infrastructure
only."""
import functools
import zlib

import numpy as np

import oracle_lib as orc
import p4_modes

R = 3              # units per class and case
TRIES = 150        # directed draws per class
MAX_UNITS = 1500
XN = (63, 64, 65, 127, 128, 129)
WCAP = {32: (10, 6, 3), 64: (12, 7, 4)}  # window counts stated for blocks of 200 values and more, of 127 / 128, of 64 / 65
CASES = [("256v32", 256), ("256v32", 200), ("128v32", 128), ("32", 255), ("32", 127), ("32", 64),
         ("64", 256), ("64", 65), ("128v64", 128), ("256v64", 256)]
FULL_WIDTH32 = [("256v32", 256), ("32", 255)]
DECODE_ONLY_CASES = [("256v32", 256), ("32", 255)]
WBITS = {"32": 32, "128v32": 32, "256v32": 32, "64": 64, "128v64": 64, "256v64": 64}
BASE_N = {"32": None, "64": None, "128v32": 128, "256v32": 256, "128v64": 128, "256v64": 128}
WIDTH = {"128v32": 128, "256v32": 256, "128v64": 128, "256v64": 256}
_FCODE = {"32": 0, "128v32": 1, "256v32": 2, "64": 3, "128v64": 4, "256v64": 5}
_VB_STEP = {32: (156, 16540, 2113692), 64: (152, 16536, 2113688)}  # first value of the 2-, 3- and 4-byte forms
A_LO, A_HI = 0x9C, 0xDC  # the 2-byte markers of vbEnc32
CHAIN_START0 = {32: 0xFFFFF000, 64: (1 << 64) - 4096}  # the chained delta-1 list wraps


def block_ns(fmt, n):
    """The n of each block of one unit (a 256v64 unit: a 128v64 block of 128 and one of n - 128)."""
    return [n] if fmt != "256v64" else [min(128, n - c) for c in range(0, n, 128)]


def value_lens(W):
    return tuple(range(1, 6)) if W == 32 else tuple(range(1, 10))


# ---- the layout of a unit, from its bytes ---------------------------------------------------------
class VBlock:
    """One block of a unit: mode, xn, v0 (V's first byte in the stream), lens (compressed marker lengths), pos (the
    block's first byte) and end."""

    def __init__(self, mode, xn, v0, lens, pos, end):
        self.mode, self.xn, self.v0, self.lens, self.pos, self.end = mode, xn, v0, lens, pos, end
        self.vlen = sum(lens)


def blocks_of_unit(fmt, enc, pos, n):
    """The blocks of the unit at enc[pos:], read with p4_modes.parse32 / parse64."""
    out = []
    for bn in block_ns(fmt, n):
        if WBITS[fmt] == 32:
            mode, lens, end = p4_modes.parse32(enc, pos, bn, BASE_N[fmt])
            xn = v0 = 0
            if mode in ("vb_comp", "vb_raw"):
                b = int(enc[pos]) & 0x3F
                xn, v0 = int(enc[pos + 1]), pos + 2 + ((BASE_N[fmt] or bn) * b + 7) // 8
        else:
            blk = p4_modes.parse64(enc, pos, bn, BASE_N[fmt])
            mode, lens, end, xn, v0 = blk.mode, blk.lens, blk.end, blk.xn, blk.base[1]
        out.append(VBlock(mode, xn, v0, lens, pos, end))
        pos = end
    return out


def _bucket(k):
    return k if k <= 8 else "9-15" if k <= 15 else "16+"


def stream_facts(V, lens, W):
    """The classes of one compressed stream V (bytes) whose values have the lengths `lens`."""
    nv, xn, tags = len(V), len(lens), set()
    assert sum(lens) == nv and xn
    tags.add(("W", (nv - 1) // 64 + 1))
    e = 0
    for L in lens:
        e += L
        if e >= 64 and e % 64 < L:
            tags.add(("end", L, e % 64))
    if xn in XN:
        tags.add(("xn", xn))
    longs = [k for k, L in enumerate(lens) if L >= 3]
    if not longs and 62 <= nv <= 66:
        tags.add(("short", nv))
    if nv <= 64 and len(longs) == 1:
        tags.add(("one_long", "first" if longs[0] == 0 else "last" if longs[0] == xn - 1 else "middle"))
    if W == 32 and not longs and nv <= 64:
        starts = set(np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist())
        k = 0
        while k < nv:
            if not A_LO <= V[k] < A_HI:
                k += 1
                continue
            j = k
            while j < nv and A_LO <= V[j] < A_HI:
                j += 1
            tags.add(("run", _bucket(j - k), k & 1))
            if k == 0:
                tags.add(("run_at", "start"))
            if j == nv:
                tags.add(("run_at", "end"))
            tags.add(("run_last", "marker" if (j - 1) in starts else "data"))
            k = j
    return tags


def unit_facts(fmt, enc, pos, n):
    """The classes of the unit at enc[pos:], the union over its blocks."""
    tags = set()
    for blk in blocks_of_unit(fmt, enc, pos, n):
        if blk.mode == "vb_raw":
            tags.add(("vb_raw",))
        if blk.mode != "vb_comp":
            continue
        tags |= stream_facts(bytes(enc[blk.v0: blk.v0 + blk.vlen]), blk.lens, WBITS[fmt])
        rel = blk.v0 - blk.pos
        if fmt == "256v32" and rel <= 1024 < rel + blk.vlen + 15:
            tags.add(("v1024",))
    return tags


def all_classes(fmt, n):
    """Every class that is stated for the case, reachable or not."""
    W, bn = WBITS[fmt], max(block_ns(fmt, n))
    wcap = WCAP[W][(bn < 200) + (bn < 127)]
    tags = [("W", w) for w in range(1, wcap + 1)]
    tags += [("end", L, s) for L in value_lens(W) for s in range(L)]
    tags += [("short", k) for k in range(62, 67)] + [("one_long", w) for w in ("first", "middle", "last")]
    if W == 32:
        tags += [("run", k, par) for k in list(range(1, 9)) + ["9-15", "16+"] for par in (0, 1)]
        tags += [("run_at", "start"), ("run_at", "end"), ("run_last", "marker"), ("run_last", "data")]
    tags += [("xn", k) for k in XN if k <= bn]
    if fmt == "256v32":
        tags.append(("v1024",))
    tags.append(("vb_raw",))
    return tags


# ---- directed draws ----------------------------------------------------------------------------
ONE_BYTE = [(64, 128)] * 4 + [(1, 156), (128, 156), (100, 156)] + [(1 << (w - 1), 1 << w) for w in range(1, 7)]


def value_of_len(rng, L, W, b0=0, low=False, one=(64, 128)):
    """An excess value whose vbEnc form has L bytes and that fits above a base of b0 bits.  low: a 2- or 3-byte
    value from the part of its range that the encoder's estimate (steps at 8, 15, 19 and 25 bits of excess) prices
    at its true length, not one byte over, and a longer value from the lowest bit width of its form (two 5-byte
    values of 25 bits leave a list far from wrapping).  one: the range of a one-byte value, which one draw in eight
    leaves for any one-byte value."""
    s = _VB_STEP[W]
    if low and L in (2, 3):
        return int(rng.integers(s[L - 2], 1 << (14 if L == 2 else 18)))
    if L == 1:
        return int(rng.integers(*(one if rng.integers(0, 8) else (1, s[0]))))
    if L <= 3:
        return int(rng.integers(s[L - 2], s[L - 1]))
    if W == 32:
        lo, hi = (s[2], 1 << 24) if L == 4 else (1 << 24, 1 << 32)
    else:
        lo, hi = max(s[2], 1 << (8 * (L - 2))), 1 << (8 * (L - 1))
    if low:
        hi = 2 * lo
    hi = min(hi, 1 << (W - b0))
    assert lo < hi, (L, W, b0)
    return int(rng.integers(lo, hi, dtype=np.uint64))


def _shorts(rng, total, twos=None):
    """Lengths 1 and 2 that add up to `total` bytes, `twos` of them 2 (default: a random share), shuffled."""
    k = int(rng.integers(0, total // 2 + 1)) if twos is None else min(twos, total // 2)
    lens = [2] * k + [1] * (total - 2 * k)
    return [lens[i] for i in rng.permutation(len(lens))]


def _in_run_pair(rng):
    """A 2-byte vbEnc32 value whose marker and data byte both lie in [0x9C, 0xDC)."""
    return 156 + ((int(rng.integers(A_LO, A_HI)) - A_LO) << 8) + int(rng.integers(A_LO, A_HI))


def _run_end_marker(rng):
    """A 2-byte vbEnc32 value whose data byte lies outside [0x9C, 0xDC)."""
    d = int(rng.choice([int(rng.integers(0, A_LO)), int(rng.integers(A_HI, 256))]))
    return 156 + ((int(rng.integers(A_LO, A_HI)) - A_LO) << 8) + d


def _outlier_len(rng, W):
    return 5 if W == 32 else int(rng.integers(5, 10))


def aim(tag, rng, bn, W):
    """One draw aimed at class `tag` for a block of bn values: a list of items in V's order, each a byte length
    (a random value of that length) or ("v", value).  None: the class is not drawn for at this size."""
    nfill = int(rng.integers(bn // 8 + 8, bn // 4 + 9))
    kind = tag[0]
    if kind == "W":
        total = (tag[1] - 1) * 64 + 1 + int(64 * rng.random() ** 3)  # the short end of the range more often: the last reachable w
        outl = [_outlier_len(rng, W) for _ in range(int(rng.integers(0, 3)))]
        if total - sum(outl) < 11:
            outl = []
        # some share of the bytes in values of one longer form (a wide excess is dearer to absorb in the base), the
        # rest in 1- and 2-byte values
        rest = total - sum(outl)
        Lw = int(rng.choice(value_lens(W)[1:]))
        kw = int(rest * rng.choice([0.0, 0.3, 0.6, 0.9, 1.0])) // Lw
        rest -= kw * Lw
        items = outl + [Lw] * kw + _shorts(rng, rest, int(rest * 0.5 * rng.random()))
        return [items[i] for i in rng.permutation(len(items))]
    if kind == "end":
        _, L, s = tag
        mmax = 5 if bn >= 200 else 2 if bn >= 127 else 1
        m = int(rng.integers(1, mmax + 1))
        pre_bytes = 64 * m + s - L
        ol = _outlier_len(rng, W)
        where = int(rng.integers(0, 3)) if L < 3 else 2  # an outlier before, after, or none beside the value itself
        pre = [ol] if where == 0 and pre_bytes - ol >= 8 else []
        share = rng.choice([0.0, 0.1, 0.3] if bn >= 127 else [0.1, 0.3, 0.4, 0.45, 0.5])
        pre += _shorts(rng, pre_bytes - sum(pre), int((pre_bytes - sum(pre)) * share))
        pre = [pre[i] for i in rng.permutation(len(pre))]
        post = [1] * int(rng.integers(0, max(1, nfill - len(pre) // 2))) + ([ol] if where == 1 else [])
        return pre + [L] + [post[i] for i in rng.permutation(len(post))]
    if kind == "short":
        return _shorts(rng, tag[1], int(rng.integers(0, tag[1] // 2 + 1)))
    if kind == "one_long":
        L = int(rng.integers(3, value_lens(W)[-1] + 1))
        rest = _shorts(rng, int(rng.integers(30, 65 - L)), int(rng.integers(0, 8)))
        at = 0 if tag[1] == "first" else len(rest) if tag[1] == "last" else int(rng.integers(1, len(rest)))
        return rest[:at] + [L] + rest[at:]
    if kind in ("run", "run_at", "run_last"):
        if kind == "run":
            k = tag[1]
            rl = k if isinstance(k, int) else int(rng.integers(9, 16)) if k == "9-15" else int(rng.choice([16, 17, 24, 40]))
            par = tag[2]
        else:
            rl = int(rng.integers(1, 12))
            rl += (rl & 1) if tag[1] in ("end", "data") else 1 - (rl & 1) if tag[1] == "marker" else 0
            par = int(rng.integers(0, 2))
        run = [("v", _in_run_pair(rng)) for _ in range(rl // 2)] + ([("v", _run_end_marker(rng))] if rl & 1 else [])
        nrun = rl + (rl & 1)
        total = int(rng.integers(max(nrun + par + 2, 28), 65)) if bn >= 127 else int(rng.integers(nrun + par + 2, max(nrun + par + 3, 35)))
        npre = 0 if tag == ("run_at", "start") else par + 2 * int(rng.integers(0, (total - nrun - par) // 2 + 1))
        npre = total - nrun if tag == ("run_at", "end") else npre
        return [1] * npre + run + [1] * (total - nrun - npre)
    if kind == "xn":
        k = tag[1]
        outl = [_outlier_len(rng, W) for _ in range(int(rng.integers(0, 3)))]
        rest = k - len(outl)
        twos = int(rest * rng.random())
        threes = int((rest - twos) * rng.random()) if rng.integers(0, 2) else 0
        items = outl + [2] * twos + [3] * threes + [1] * (rest - twos - threes)
        return [items[i] for i in rng.permutation(len(items))]
    if kind == "vb_raw":
        return [_outlier_len(rng, W)] * int(rng.integers(1, 5)) + [1] * int(rng.integers(0, 5))
    if kind == "v1024":
        return [1] * int(rng.integers(11, 120))
    raise KeyError(tag)


def _of_width(rng, w, L, W):
    """An excess value of exactly w bits whose vbEnc form has L bytes (w = 1..8 for L = 1, 8..15 for L = 2, 15..21 for L = 3)."""
    s = (1,) + _VB_STEP[W]
    return int(rng.integers(max(1 << (w - 1), s[L - 1]), min(1 << w, s[L])))


def grid(tag, rng, bn, W):
    """The draws for a window count, a short-form length or an exception count that are made before the random ones: a
    grid over what the cost model reads -- how many exceptions have 1, 2 and 3 (or, for the windows, one longer
    length of) bytes, the bit widths of the 1-, 2- and 3-byte values, how many outliers and the base width -- so
    that whether such a class is reached does not hang on a lucky draw.  Yields (items, b0)."""
    kind, k = tag[0], tag[1]
    top = value_lens(W)[-1]
    for b0 in (0, 2):
        for w1 in (1, 4, 6, 7, 8):
            for w2 in (8, 9, 12, 14, 15):
                if kind == "short":
                    combos = [((k - 2 * x2, x2, 0, 0), 0, 0) for x2 in range(0, k // 2 + 1)]
                elif kind == "xn":
                    combos = [((k - no - x2 - x3, x2, x3, 0), no, top) for no in (0, 1, 2) for x3 in (0, 8, 32)
                              for x2 in range(0, k - no - x3 + 1, 8)]
                else:
                    combos = []
                    for total in ((k - 1) * 64 + 1, (k - 1) * 64 + 24):
                        for no in (0, 1, 2):
                            for Lw in range(2, top + 1):
                                room = total - no * top
                                for kw in sorted({room // Lw, 3 * room // (4 * Lw), room // (2 * Lw), room // (4 * Lw)}):
                                    rest = room - kw * Lw
                                    for x2 in sorted({0, rest // 4, rest // 2}):
                                        c = [rest - 2 * x2, x2, 0, 0]
                                        c[min(Lw, 4) - 1] += kw
                                        combos.append((tuple(c), no, Lw))
                for (x1, x2, x3, xl), no, Lw in combos:
                    if min(x1, x2, x3, xl) < 0 or not 0 < x1 + x2 + x3 + xl + no <= bn:
                        continue
                    items = [("v", _of_width(rng, w1, 1, W)) for _ in range(x1)] + [("v", _of_width(rng, w2, 2, W)) for _ in range(x2)]
                    items += [("v", _of_width(rng, 17, 3, W)) for _ in range(x3)] + [Lw] * xl + [top] * no
                    yield [items[i] for i in rng.permutation(len(items))], b0


def draw_values(rng, W, items, b0):
    """The excess values of `items` (see aim) over a base of b0 bits; None when one does not fit above the base."""
    low = bool(rng.integers(0, 2))
    one = ONE_BYTE[int(rng.integers(0, len(ONE_BYTE)))]
    out = []
    for it in items:
        if isinstance(it, int):
            if it >= 4 and (1 << (W - b0)) <= (_VB_STEP[W][2] if it == 4 else 1 << (8 * (it - 2 if W == 64 else 3))):
                return None
            it = ("v", value_of_len(rng, it, W, b0, low, one))
        if it[1] >> (W - b0):
            return None
        out.append(it[1])
    return out


def block_row(rng, bn, W, E, b0):
    """bn values: a base of b0 bits and, at ascending positions, the excess values E over it, in order."""
    dt = np.uint32 if W == 32 else np.uint64
    v = (rng.integers(0, 1 << 63, size=bn, dtype=np.uint64) >> np.uint64(63 - b0) >> np.uint64(1)).astype(dt) if b0 else np.zeros(bn, dt)
    pos = np.sort(rng.choice(bn, size=len(E), replace=False))
    for p, e in zip(pos, E):
        v[p] = dt((e << b0) | int(v[p]))
    return v


def _filler(rng, bn, W):
    """The other half of a 256v64 unit: an ordinary compressed vbyte block."""
    b0 = int(rng.integers(0, 4))
    return block_row(rng, bn, W, draw_values(rng, W, [_outlier_len(rng, W)] + _shorts(rng, int(rng.integers(20, 50)), 4), b0), b0)


def base_width(rng, W):
    """The base width of a draw: narrow in half of the draws, else anything that leaves 15 bits of excess."""
    return int(rng.choice([0, 0, 0, 1, 2, 3, 5, 7])) if rng.integers(0, 2) else int(rng.integers(0, W - 14))


def tries(tag):
    """Directed draws for a class before it counts as unreached; the window counts, the short-form lengths and the
    exception counts get more: the last reachable ones are narrow targets."""
    return TRIES * (8 if tag[0] in ("W", "short", "xn", "run") else 2)


class Family:
    """The reachable family of one case: gaps (nu, n); tags[i], the classes of unit i by the oracle's bytes;
    count[tag], units that hold it; aimed[tag] / hit[tag], directed draws for the class and those that reached it.
    A class that its draws reach fewer than R times is filled up with the draw that reached it, laid out again at
    other positions over another base: the same V in another block."""

    def __init__(self, fmt, n, only=None):
        self.fmt, self.n, self.W = fmt, n, WBITS[fmt]
        self.bns = block_ns(fmt, n)
        classes = all_classes(fmt, n)
        self.count = {t: 0 for t in classes}
        self.aimed = {t: 0 for t in classes}
        self.hit = {t: 0 for t in classes}
        self.rows, self.tags, self.recipe, self.grid = [], [], [], {}
        for k, tag in enumerate(classes):
            # every class draws from a generator of its own, so the classes of UNREACHED, which add no unit, can be
            # left out (only: the classes to draw for; default: all but UNREACHED's)
            if tag not in only if only is not None else tag in UNREACHED.get((fmt, n), ()):
                continue
            self.rng = np.random.default_rng([8100, _FCODE[fmt], n, zlib.crc32(repr(tag).encode())])
            draws = grid(tag, self.rng, min(self.bns), self.W) if tag[0] in ("W", "short", "xn") else iter(())
            for _ in range(10 ** 6):
                if self.count[tag] >= R:
                    break
                half = int(self.rng.integers(0, len(self.bns)))
                items, b0 = next(draws, (None, 0))
                if items is None:
                    if self.aimed[tag] - self.grid.get(tag, 0) >= tries(tag):
                        break
                    items = aim(tag, self.rng, self.bns[half], self.W)
                    b0 = int(self.rng.integers(24, 32)) if tag == ("v1024",) else base_width(self.rng, self.W)
                else:
                    self.grid[tag] = self.grid.get(tag, 0) + 1
                E = draw_values(self.rng, self.W, items, b0) if 0 < len(items) <= self.bns[half] else None
                self.aimed[tag] += 1
                if E is not None:
                    self._take(tag, half, E, b0)
            if tag[0] == "run" and self.count[tag] == 0:
                # a run at the other parity: the same values with the first moved to the end or the last to the front,
                # which the cost model, reading only bit widths, cannot tell from the unit that holds the sibling class
                for half, E, b0 in [self.recipe[i] for i, t in enumerate(self.tags) if (tag[0], tag[1], 1 - tag[2]) in t]:
                    for E2 in (E[1:] + E[:1], E[-1:] + E[:-1]):
                        self.aimed[tag] += 1
                        if self.count[tag] < R:
                            self._take(tag, half, E2, b0)
            held = [self.recipe[i] for i, t in enumerate(self.tags) if tag in t]
            for k in range(8 * R if held else 0):
                if self.count[tag] >= R:
                    break
                self._take(tag, *held[k % len(held)])
        assert len(self.rows) <= MAX_UNITS
        self.gaps = np.stack(self.rows) if self.rows else None
        self.nu = len(self.rows)

    def _take(self, tag, half, E, b0):
        """lay E out, encode, and keep the unit if the oracle's bytes hold the class"""
        parts = [block_row(self.rng, bn, self.W, E, b0) if h == half else _filler(self.rng, bn, self.W) for h, bn in enumerate(self.bns)]
        row = np.concatenate(parts)
        facts = unit_facts(self.fmt, np.frombuffer(orc.encode(self.fmt, row), dtype=np.uint8), 0, self.n)
        if tag not in facts:
            return False
        self.hit[tag] += 1
        self.rows.append(row)
        self.tags.append(facts)
        self.recipe.append((half, E, b0))
        for t in facts:
            if t in self.count:
                self.count[t] += 1
        return True

    def unreached(self):
        return sorted((t for t, c in self.count.items() if c == 0), key=str)


def directed_misses(fmt, n):
    """The directed search behind UNREACHED[(fmt, n)]: -> {class: (draws, units that hold it)}"""
    f = Family(fmt, n, only=UNREACHED[(fmt, n)])
    return {t: (f.aimed[t], f.count[t]) for t in UNREACHED[(fmt, n)]}


@functools.lru_cache(maxsize=None)
def family(fmt, n):
    """Cached: callers leave the arrays unchanged."""
    return Family(fmt, n)


def d1_list(gaps, W):
    """The delta-1 list whose gaps are `gaps` (nu, n), from CHAIN_START0, mod 2^W, and each unit's start."""
    nu, n = gaps.shape
    dt = np.uint32 if W == 32 else np.uint64
    x = np.cumsum(gaps.ravel().astype(np.uint64) + np.uint64(1), dtype=np.uint64) + np.uint64(CHAIN_START0[W])
    x = x.astype(dt).reshape(nu, n)
    starts = np.empty(nu, dtype=dt)
    starts[0] = CHAIN_START0[W]
    starts[1:] = x[:-1, -1]
    return x, starts


def oracle_stream(fmt, vals, starts=None):
    encs = [orc.encode(fmt, row, d1=starts is not None, start=0 if starts is None else int(starts[i])) for i, row in enumerate(vals)]
    off = np.concatenate([[0], np.cumsum([len(e) for e in encs])]).astype(np.uint64)
    return np.frombuffer(b"".join(encs), dtype=np.uint8).copy(), off


class Case:
    """One (fmt, n, d1) form of a family with the oracle's stream of it: gaps, vals (the gaps, or with d1 the one
    chained list they span from CHAIN_START0, which wraps), starts (d1: the value before each unit), units (vals at
    the layout's stride, zero past n), packed / off, tags (per unit) and start0."""

    def __init__(self, fmt, n, d1, gaps, tags):
        self.fmt, self.n, self.d1, self.gaps, self.tags = fmt, n, d1, gaps, tags
        self.W, self.nu = WBITS[fmt], len(gaps)
        self.start0 = CHAIN_START0[self.W]
        self.vals, self.starts = d1_list(gaps, self.W) if d1 else (gaps, None)
        self.units = np.zeros((self.nu, WIDTH.get(fmt, n)), dtype=gaps.dtype)
        self.units[:, :n] = self.vals
        self.packed, self.off = oracle_stream(fmt, self.vals, self.starts)

    def names(self, units):
        return [(int(u), sorted(self.tags[int(u)], key=str)) for u in list(units)[:5]]

    def units_of_bytes(self, at):
        return np.unique(np.searchsorted(self.off, np.asarray(at).astype(np.uint64), side="right") - 1)


@functools.lru_cache(maxsize=None)
def layout_case(fmt, n, d1):
    """Cached: callers leave the arrays unchanged."""
    f = family(fmt, n)
    return Case(fmt, n, d1, f.gaps, f.tags)


# Classes no draw reaches, per case; test_vbyte_layouts_cpu.py holds the table to the families: a class listed here has
# no unit in any of its draws (directed_misses repeats them), every other class R units or more.  The encoder's choice
# (p4Bits32 / p4Bits64) reads only the bit widths of the values, and vbEnc's raw escape only the byte count of V, so for
# the classes that are a matter of size -- the window counts, the short-form lengths, the exception counts -- the draws
# begin with a grid over exactly those inputs (grid(): 1,600 to 11,000 draws per class: the counts of 1-, 2-, 3-byte and
# longer values, the widths of the short ones, 0..2 outliers, two base widths), then tries(class) random ones with the
# base width, the two-byte share and the value ranges drawn over their whole range.  What is left is monotone: past a
# case's last window count, short-form length or exception count nothing is reached, because an exception costs 1 + its
# vbyte bytes and a base bit n / 8 bytes, so past some |V| a wider base is cheaper, the sooner the smaller n.
#  * runs of 16 bytes and more at 64 values: 8 two-byte values and more, whose 15 bits of excess the bitmap patch
#    carries more cheaply there.
#  * ("v1024",): V starts at byte 2 + 32 b of a 256v32 block, so b >= 24 and the excess has at most 8 bits: xn
#    one-byte exceptions cost 2 xn bytes against 32 per base bit, and the 11..15 of them that pay at b = 31 end at
#    byte 1023 of the image at the most.  The decode-only family holds the class.
UNREACHED = {
    ("256v32", 256): [("W", 9), ("W", 10), ("v1024",)],
    ("256v32", 200): [("W", 7), ("W", 8), ("W", 9), ("W", 10), ("v1024",)],
    ("128v32", 128): [("W", 5), ("W", 6), ("xn", 127), ("xn", 128)],
    ("32", 255): [("W", 9), ("W", 10)],
    ("32", 127): [("W", 5), ("W", 6), ("xn", 127)],
    ("32", 64): [("W", 3), ("run", "16+", 0), ("run", "16+", 1), ("short", 62), ("short", 63), ("short", 64), ("short", 65), ("short", 66),
                 ("xn", 63), ("xn", 64)],
    ("64", 256): [("W", 11), ("W", 12)],
    ("64", 65): [("W", 4), ("short", 62), ("short", 63), ("short", 64), ("short", 65), ("short", 66), ("xn", 63), ("xn", 64), ("xn", 65)],
    ("128v64", 128): [("W", 6), ("W", 7), ("xn", 127), ("xn", 128)],
    ("256v64", 256): [("W", 6), ("W", 7), ("xn", 127), ("xn", 128)],
}


def required_classes(fmt, n):
    return [t for t in all_classes(fmt, n) if t not in UNREACHED.get((fmt, n), ())]


# ---- the decode-only family ---------------------------------------------------------------------
DO_XN = (128, 200, 255)
DO_KINDS = ("all2", "all3", "all4", "mixed")


class DecodeOnly:
    """Units the reference decodes and its encoder never writes: an oracle-encoded compressed vbyte unit of the
    reachable family (base of at most 7 bits) whose xn, V and positions are replaced -- xn in DO_XN, V the canonical
    vbEnc32 of excess values whose forms are all 2, all 3, all 4 bytes or mixed 1..5 (up to 16 windows), the
    positions distinct and ascending.  packed / off, label[i] = (xn, kind, windows), vals (nu, n): the oracle
    decoder's output, d1 False; with per-unit starts `starts` and chained from CHAIN_START0, d1 True."""

    def __init__(self, fmt, n, reps=3):
        self.fmt, self.n, self.W = fmt, n, 32
        rng = np.random.default_rng([8200, _FCODE[fmt], n])
        src = layout_case(fmt, n, False)
        donors = []
        for i in range(src.nu):
            blk = blocks_of_unit(fmt, src.packed, int(src.off[i]), n)[0]
            if blk.mode == "vb_comp" and (int(src.packed[blk.pos]) & 0x3F) <= 7:
                donors.append(blk)
        flat = [blk for blk in donors if (int(src.packed[blk.pos]) & 0x3F) == 0]
        parts, self.label, self.tags = [], [], []
        for xn in DO_XN:
            if xn > n:
                continue
            for kind in DO_KINDS:
                for rep in range(reps + 1):
                    # the last one over a base of no bits with values from the low end of their forms: a unit whose
                    # values add up to less than 3 * 2^30, for the set operations (ascending_lists)
                    low = rep == reps
                    blk = (flat if low else donors)[int(rng.integers(0, len(flat if low else donors)))]
                    b = int(src.packed[blk.pos]) & 0x3F
                    lens = [int(kind[3])] * xn if kind != "mixed" else [int(x) for x in rng.integers(1, 6, size=xn)]
                    V = np.concatenate([_vbput32(value_of_len(rng, L, 32, b, low)) for L in lens])
                    pos = np.sort(rng.choice(n, size=xn, replace=False)).astype(np.uint8)
                    unit = np.concatenate([src.packed[blk.pos: blk.pos + 1], np.array([xn], np.uint8), src.packed[blk.pos + 2: blk.v0], V, pos])
                    parts.append(unit)
                    self.label.append((xn, kind, (len(V) - 1) // 64 + 1))
        self.nu = len(parts)
        self.packed = np.concatenate(parts)
        self.off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
        self.gaps = np.stack([orc.decode(fmt, bytes(p), n)[0] for p in parts])
        for i, p in enumerate(parts):
            assert orc.decode(fmt, bytes(p), n)[1] == len(p)
            self.tags.append(unit_facts(fmt, self.packed, int(self.off[i]), n))
        self.units = np.zeros((self.nu, WIDTH.get(fmt, n)), dtype=np.uint32)
        self.units[:, :n] = self.gaps
        self.start0 = CHAIN_START0[32]
        self.chained, self.starts = d1_list(self.gaps, 32)

    def names(self, units):
        return [(int(u), self.label[int(u)]) for u in list(units)[:5]]


def _vbput32(x):
    """vbPut32: the canonical form of one value."""
    if x < 156:
        return np.array([x], np.uint8)
    if x < 16540:
        d = x - 156
        return np.array([0x9C + (d >> 8), d & 0xFF], np.uint8)
    if x < 2113692:
        d = x - 16540
        return np.array([0xDC + (d >> 16), d & 0xFF, (d >> 8) & 0xFF], np.uint8)
    if x <= 0xFFFFFF:
        return np.array([0xFC, x & 0xFF, (x >> 8) & 0xFF, (x >> 16) & 0xFF], np.uint8)
    return np.array([0xFD, x & 0xFF, (x >> 8) & 0xFF, (x >> 16) & 0xFF, x >> 24], np.uint8)


@functools.lru_cache(maxsize=None)
def decode_only(fmt, n):
    """Cached: callers leave the arrays unchanged."""
    return DecodeOnly(fmt, n)


# ---- the parses restated, with wrong variants ---------------------------------------------------------
def vb_len32(m):
    return p4_modes.marker_len32(m)


def vb_val32(V, c):
    """vbGet32Inline at V[c] (bytes past V read as 0)."""
    m = V[c] if c < len(V) else 0
    d = [V[c + k] if c + k < len(V) else 0 for k in range(1, 5)]
    if m < 0x9C:
        return m
    if m < 0xDC:
        return ((m - 0x9C) << 8) + d[0] + 156
    if m < 0xFC:
        return (d[0] | (d[1] << 8)) + ((m - 0xDC) << 16) + 16540
    if m == 0xFC:
        return d[0] | (d[1] << 8) | (d[2] << 16)
    return d[0] | (d[1] << 8) | (d[2] << 16) | (d[3] << 24)


def serial_parse(V, xn):
    """The definition (vbDec32): -> (the xn values, the bytes they use)."""
    out, c = [], 0
    for _ in range(xn):
        out.append(vb_val32(V, c))
        c += vb_len32(V[c])
    return out, c


def windowed_parse(V, xn, rule=None):
    """vbyte_exceptions' walk of V (bytes from V's first, the positions and whatever follows included): windows of
    64 bytes at c, the first value of a window at sp, every value that starts inside the window decoded by one lane
    into the ring tmp[(found + t) & 255]; the next window starts 64 bytes on and carries the straddle of the last
    value.  rule: a WINDOW_MUTANTS key.  -> (values, bytes used)"""
    ring = {"ring_64": 64, "ring_128": 128}.get(rule, 256)
    tmp = [0] * 256
    c = sp = found = vend = windows = 0
    while found < xn:
        if rule == "two_windows" and windows == 2:
            break
        starts, p = [], sp
        while p < 64:
            starts.append(p)
            p += vb_len32(V[c + p] if c + p < len(V) else 0)
        cnt = min(len(starts), xn - found)
        for t in range(cnt):
            tmp[(found + t) % ring] = vb_val32(V, c + starts[t])
        e_last = starts[cnt - 1] + vb_len32(V[c + starts[cnt - 1]] if c + starts[cnt - 1] < len(V) else 0)
        found += cnt
        vend = c + e_last
        if e_last >= 64:
            sp = 0 if rule == "straddle_dropped" else e_last - 64 + (rule == "straddle_off_by_one")
            c += 64
        else:
            sp = e_last
        windows += 1
    return tmp[:xn], vend


WINDOW_MUTANTS = ("straddle_dropped", "straddle_off_by_one", "two_windows", "ring_64", "ring_128")


def _m32(x):
    return x & 0xFFFFFFFF


def _alignbyte(hi, lo, k):
    return _m32(((hi << 32) | lo) >> (8 * k))


def _sad_u8(x):
    return sum((x >> (8 * k)) & 0xFF for k in range(4))


def short_form_sum(V, xn, v0=0, rule=None):
    """The phase-A lane sum of a compressed stream (dsum_lanes): the short form when V is 64 bytes or shorter --
    markers from the run parities of the bytes in [0x9C, 0xDC), four bytes per step, carried across steps by cin,
    aprev and mprev -- taken only if it finds xn values of 1 or 2 bytes in exactly |V| bytes; else the serial walk.
    v0: V's byte address (only the wrong "parity in the dword" variant reads it).  rule: a SHORT_MUTANTS key.
    -> (path, sum of the values mod 2^32)"""
    lr = len(V)
    exact = sum(serial_parse(V, xn)[0]) & 0xFFFFFFFF
    if not (lr < 64 if rule == "lt_64" else lr <= 64) or lr < xn:
        return "walk", exact
    even, evenb = 0x00010001, 0x00FF00FF
    if rule == "parity_in_dword" and (v0 & 1):
        even = 0x01000100  # a run's start judged by its offset in the aligned dword; the markers still by their offset in V
    aprev = mprev = cin = tsum = s2 = nm8 = n28 = bad = 0
    for j in range((lr + 3) // 4):
        x = int.from_bytes(bytes(V[4 * j: 4 * j + 4]).ljust(4, b"\0"), "little")
        sh = min(max(8 * lr - 32 * j, 0), 32)
        rm = _m32(((0xFFFFFFFF << sh) & 0xFFFFFFFFFFFFFFFF) >> 32)
        hi, y = x & 0x80808080, x & 0x7F7F7F7F
        gedc = (y + 0x24242424) & hi
        a80 = (y + 0x64646464) & hi & ~gedc & 0xFFFFFFFF
        am = a80 | (a80 - (a80 >> 7))
        sha = _alignbyte(am, aprev, 3)
        aprev = am
        t0 = am + ((am & ~sha) & even)
        c1, xs0 = t0 >> 32, _m32(t0)
        t1 = xs0 + cin
        c2, xs = t1 >> 32, _m32(t1)
        cin = 0 if rule == "carry_dropped" else (c1 | c2)
        re = am & ~xs & 0xFFFFFFFF
        mr = (re & evenb) | (am & ~re & ~evenb & 0xFFFFFFFF)
        shm = _alignbyte(mr, mprev, 3)
        mprev = mr
        mk = (mr | (~am if rule == "after_run_marker" else ~(am | shm))) & rm & 0xFFFFFFFF
        ma = mk & am
        tsum += _sad_u8(x & rm)
        s2 += _sad_u8(x & ma)
        nm8 += bin(mk).count("1")
        n28 += bin(ma).count("1")
        bad |= mk & gedc
    if bad == 0 and nm8 == 8 * xn and 8 * xn + n28 == 8 * lr:
        return "fast", (tsum + 255 * s2 - 39780 * (n28 >> 3)) & 0xFFFFFFFF
    return "walk", exact


SHORT_MUTANTS = ("lt_64", "after_run_marker", "carry_dropped", "parity_in_dword")


def unit_size32(enc, pos, n, base_n, rule=None):
    """The byte length of a 32-bit vbyte block from its header, as the offsets scan sizes it; rule "raw_5xn": the
    raw escape taken for 5 * xn bytes, its 0xFF byte forgotten."""
    b, xn = int(enc[pos]) & 0x3F, int(enc[pos + 1])
    v0 = pos + 2 + ((base_n or n) * b + 7) // 8
    if enc[v0] == 0xFF:
        return v0 + (5 * xn if rule == "raw_5xn" else 1 + 5 * xn) - pos
    return v0 + _serial_len(enc, v0, xn) + xn - pos


def _serial_len(enc, v0, xn):
    c = v0
    for _ in range(xn):
        c += vb_len32(int(enc[c]))
    return c - v0


# "lt_64" changes only which path sums the block: the serial walk gives the same sum, so no decode can show it (a
# kernel with that mistake is slower at |V| = 64, not wrong).  Its count in the tests says that the families hold
# blocks on that boundary, not that a wrong decode is caught; every other variant changes values or sizes.
MUTANTS = WINDOW_MUTANTS + SHORT_MUTANTS + ("raw_5xn",)


def misparsed(fmt, n, enc, off, rule, shift=0):
    """The units of a 32-bit stream that the wrong variant `rule` parses differently from the right one (windowed
    parse, short-form sum with V at its stream address + shift, or unit size)."""
    bad = []
    for i in range(len(off) - 1):
        for blk in blocks_of_unit(fmt, enc, int(off[i]), n):
            if blk.mode == "vb_raw" and rule == "raw_5xn":
                if unit_size32(enc, blk.pos, n, BASE_N[fmt], rule) != unit_size32(enc, blk.pos, n, BASE_N[fmt]):
                    bad.append(i)
            if blk.mode != "vb_comp" or rule == "raw_5xn":
                continue
            if rule in WINDOW_MUTANTS:
                V = bytes(enc[blk.v0: blk.end])
                if windowed_parse(V, blk.xn, rule) != windowed_parse(V, blk.xn):
                    bad.append(i)
            else:
                V = bytes(enc[blk.v0: blk.v0 + blk.vlen])
                if short_form_sum(V, blk.xn, blk.v0 + shift, rule) != short_form_sum(V, blk.xn, blk.v0 + shift):
                    bad.append(i)
    return bad


def stream_census(fmt, n, packed, off):
    """-> {class: units of the stream that hold it}, over all_classes(fmt, n) and whatever else the units hold"""
    count = {t: 0 for t in all_classes(fmt, n)}
    for i in range(len(off) - 1):
        for t in unit_facts(fmt, packed, int(off[i]), n):
            count[t] = count.get(t, 0) + 1
    return count


def survivors(fmt, n, packed, off):
    """The MUTANTS that parse every unit of a 32-bit stream as the right parse does (at either parity of V's address)."""
    return [r for r in MUTANTS if not any(misparsed(fmt, n, packed, off, r, s) for s in ((0, 1) if r == "parity_in_dword" else (0,)))]


# ---- a lists stream of the 32-bit families ------------------------------------------------------------
class LayoutLists:
    """One lists stream (n / 256 p4Enc256v32 blocks and a p4Enc32 tail per list) whose units are those of the
    ("256v32", 256) family and of the ("32", 255 / 127 / 64) families -- kind "reachable" -- or of the two decode-only
    families (tails of 255 values).  Every tail unit ends one list, behind 0, 1 or 2 full blocks; one list holds 70
    full blocks and a tail; every full block is in some list.  The stream is the units' bytes end to end: a unit's
    bytes are the same in the plain stream of the gaps and in the delta-1 stream of start0 + cumsum(gap + 1).
    gaps[j], start0, packed, offs, ptr, unit_label[u] = (family n, unit), lists(d1)."""

    def __init__(self, kind):
        rng = np.random.default_rng([8300, kind == "reachable"])
        src = (lambda fmt, n: layout_case(fmt, n, False)) if kind == "reachable" else decode_only
        fam = {256: src("256v32", 256)}
        fam.update({n: src("32", n) for n in ((255, 127, 64) if kind == "reachable" else (255,))})
        self.fam = fam
        tails = [(n, i) for n in fam if n != 256 for i in range(fam[n].nu)]
        tails = [tails[i] for i in rng.permutation(len(tails))]
        nfull, at, self.label = fam[256].nu, 0, []
        for k, t in enumerate(tails):
            take = 70 if k == 5 else (0, 1, 2)[k % 3]
            self.label.append([(256, (at + x) % nfull) for x in range(take)] + [t])
            at += take
        while at < nfull:  # the rest of the full blocks: lists without a tail
            self.label.append([(256, at + x) for x in range(min(2, nfull - at))])
            at += 2
        self.unit_label = [x for lab in self.label for x in lab]
        self.gaps = [np.concatenate([fam[n].gaps[i] for n, i in lab]) for lab in self.label]
        self.nlists, self.nunits = len(self.gaps), len(self.unit_label)
        self.start0 = rng.integers(0, 1 << 32, size=self.nlists, dtype=np.uint64).astype(np.uint32)
        parts = [fam[n].packed[int(fam[n].off[i]): int(fam[n].off[i + 1])] for n, i in self.unit_label]
        self.packed = np.concatenate(parts)
        self.offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
        self.ptr = np.concatenate([[0], np.cumsum([len(g) for g in self.gaps])]).astype(np.uint64)
        self.base = np.concatenate([[0], np.cumsum([len(lab) for lab in self.label])]).astype(np.uint32)
        self.list_byte = self.offs[self.base]

    def lists(self, d1):
        if not d1:
            return self.gaps
        return [(np.cumsum(g.astype(np.uint64) + np.uint64(1)) + np.uint64(s)).astype(np.uint32) for g, s in zip(self.gaps, self.start0)]

    def names(self, units):
        return [(n, i, sorted(self.fam[n].tags[i], key=str)) for n, i in (self.unit_label[int(u)] for u in list(units)[:5])]


@functools.lru_cache(maxsize=None)
def layout_lists(kind):
    """Cached: callers leave the arrays unchanged."""
    return LayoutLists(kind)


ASC_CAP = 1 << 28  # the gap sum of a unit of ascending_lists("reachable")


@functools.lru_cache(maxsize=None)
def ascending_lists(kind="reachable"):
    """Lists for the set operations, whose numpy definitions want strictly ascending lists.
    "reachable": the units of the 32-bit reachable families whose gaps add up to less than ASC_CAP (outliers of 25 bits
    over a narrow base, none of 32), every such tail unit behind 0, 1 or 2 such full blocks, the other full blocks in
    lists of two; start0 < 2^31, so that no list wraps.
    "decode_only": the units of the two decode-only families whose gaps add up to less than 3 * 2^30, each as a list
    of its own (a full block, or a tail of 255 values) and, where the sums allow, a full block in front of a tail;
    start0 < 2^29.  Their stream is the units' own bytes: no encoder writes them.
    -> (delta-1 lists, start0, label[j] = the (family n, unit) of list j's units, the families by n)"""
    rng = np.random.default_rng([8400, kind == "reachable"])
    if kind == "reachable":
        fam = {256: layout_case("256v32", 256, False)}
        fam.update({n: layout_case("32", n, False) for n in (255, 127, 64)})
        light = {n: [i for i in range(c.nu) if int(c.gaps[i].astype(np.uint64).sum()) + n < ASC_CAP] for n, c in fam.items()}
        tails = [(n, i) for n in (255, 127, 64) for i in light[n]]
        tails = [tails[i] for i in rng.permutation(len(tails))]
        full, at, label = light[256], 0, []
        for k, t in enumerate(tails):
            take = (0, 1, 2)[k % 3]
            label.append([(256, full[(at + x) % len(full)]) for x in range(take)] + [t])
            at += take
        while at < len(full):
            label.append([(256, i) for i in full[at: at + 2]])
            at += 2
        start0 = rng.integers(0, 1 << 31, size=len(label), dtype=np.uint64).astype(np.uint32)
    else:
        fam = {256: decode_only("256v32", 256), 255: decode_only("32", 255)}
        total = {n: [int(c.gaps[i].astype(np.uint64).sum()) + n for i in range(c.nu)] for n, c in fam.items()}
        cap = 3 << 30
        label = [[(n, i)] for n in fam for i in range(fam[n].nu) if total[n][i] < cap]
        label += [[(256, i), (255, j)] for i in range(fam[256].nu) for j in range(fam[255].nu) if total[256][i] + total[255][j] < cap][:40]
        start0 = rng.integers(0, 1 << 29, size=len(label), dtype=np.uint64).astype(np.uint32)
    lists = [(np.cumsum(np.concatenate([fam[n].gaps[i] for n, i in lab]).astype(np.uint64) + np.uint64(1)) + np.uint64(s)).astype(np.uint32)
             for lab, s in zip(label, start0)]
    return lists, start0, label, fam


def layout_record(fmt, n, packed, off):
    """What a stream holds, for the record of the older inputs: -> (compressed vbyte blocks, {windows of V: blocks},
    [units in which a value ends 1, 2, 3, 4 bytes past a window boundary], the most exceptions of such a block, classes
    of required_classes(fmt, n) in fewer than R units, classes in none)"""
    cen, wins, strad, comp, xmax = stream_census(fmt, n, packed, off), {}, [0, 0, 0, 0], 0, 0
    for i in range(len(off) - 1):
        for b in blocks_of_unit(fmt, packed, int(off[i]), n):
            if b.mode == "vb_comp":
                comp, xmax = comp + 1, max(xmax, b.xn)
                wins[(b.vlen - 1) // 64 + 1] = wins.get((b.vlen - 1) // 64 + 1, 0) + 1
        ends = {t[2] for t in unit_facts(fmt, packed, int(off[i]), n) if t[0] == "end"}
        for s in (1, 2, 3, 4):
            strad[s - 1] += s in ends
    need = required_classes(fmt, n)
    return comp, dict(sorted(wins.items())), strad, xmax, len([t for t in need if cen[t] < R]), len([t for t in need if cen[t] == 0])
