"""The streams of the offsets scan's tests (tests/test_lists_scan_cpu.py,
tests/test_gpu_lists_scan.py): lists streams composed by the oracle
(tests/lists_ref.py) whose offsets the scan has to reproduce from the lists'
byte spans alone -- the tail families at every count and mode
(tests/lists_tails.py), the shape matrix in both forms, lists of constant gaps,
full blocks of every 32-bit mode and of compressed vbyte with every marker
length (tests/v32_inputs.py), a stream rewritten to the decode-only bx = 0 form,
and runs of empty lists -- the census of their full blocks, the numpy statement
of what the scan writes around a bad unit, and the single-byte corruptions the
device is held to the host on.  Test infrastructure only."""
import collections
import functools

import numpy as np

import lists_ref as ref
import lists_tails as lt
import p4_modes
import v32_inputs as vi

Stream = collections.namedtuple("Stream", "name packed offs ptr")
CLEAN = -1


def unit_base(ptr):
    return np.asarray(ref.units_loop(ptr)[1], dtype=np.int64)


def list_byte(s):
    """The first byte of every list and the stream's end: offs[list_unit[j]]."""
    return np.asarray(s.offs, dtype=np.uint64)[unit_base(s.ptr)]


def _composed(name, lists, d1, rng, ptr0=0):
    start0 = rng.integers(0, 1 << 32, size=len(lists), dtype=np.uint64).astype(np.uint32) if d1 else None
    if d1:  # the lists as delta-1 lists after their starts
        lists = [((np.cumsum(g.astype(np.uint64) + np.uint64(1)) + np.uint64(s)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                 for g, s in zip(lists, start0)]
    packed, offs, ptr, _ = ref.compose(lists, d1, start0, ptr0=ptr0)
    return Stream(name, packed, offs, ptr)


@functools.lru_cache(maxsize=None)
def small_streams():
    """Everything but the tail families: a few hundred units each."""
    rng = np.random.default_rng(8100)
    out = []
    lists = [ref.d1_values(n, 0, rng, outliers=True) for n in ref.MATRIX]
    gaps = [np.diff(np.concatenate([[np.uint32(0)], v]).astype(np.uint32)) - np.uint32(1) for v in lists]
    out.append(_composed("matrix_d1", gaps, True, rng, ptr0=7))
    out.append(_composed("matrix_plain", [ref.plain_values(n, rng) for n in ref.MATRIX], False, rng))
    # constant gaps: the full blocks of a delta-1 list are constant blocks, one byte long for gap 1
    out.append(_composed("const_gaps", [np.full(n, g, np.uint32) for g in (0, 6, 0x12345) for n in (256, 512 + 7, 256 * 3, 70)], True, rng))
    # compressed vbyte with every marker length, and every other 32-bit mode, in full blocks
    vb = vi.vbyte32_gaps("256v32", 256, 24)
    allm = vi.v32_values(rng, 40, 256)
    out.append(_composed("vbyte_blocks", [vb[:16].ravel(), np.concatenate([vb[16:].ravel(), vb[0, :5]]), allm[:17].ravel(),
                                          np.concatenate([allm[17:].ravel(), allm[3, :200]])], False, rng))
    # the decode-only form 0x80 | b with bx = 0: a stream of full blocks only, its plain blocks rewritten
    plain = [vi._below(rng, (n,), int(rng.integers(1, 20))) for n in (256, 512, 256 * 5, 256)]
    s = _composed("bx0", plain, False, rng)
    packed, offs, k = vi.as_bx0(s.packed, s.offs, 256, 256)
    assert k >= 5
    out.append(Stream("bx0", packed, offs, s.ptr))
    # runs of empty lists around and between short ones
    e = np.zeros(0, np.uint32)
    out.append(_composed("empty_runs", [e, e, e, vb[1, :9], e, e, vb[2], e, vb[3, :255], vb[4], e, e], False, rng))
    out.append(_composed("only_empty", [e] * 5, False, rng))
    return out


@functools.lru_cache(maxsize=None)
def family_streams():
    out = []
    for name in lt.FAMILIES:
        fam = lt.family(name)
        for d1 in (True, False):
            s = fam.form(d1)
            out.append(Stream(f"{name}_{'d1' if d1 else 'plain'}", s.packed, s.offs, s.ptr))
    return out


def all_streams():
    return small_streams() + family_streams()


def full_block_census(streams):
    """Modes and compressed-marker lengths of every full block, read with p4_modes.parse32."""
    modes, lens = collections.Counter(), collections.Counter()
    for s in streams:
        base = unit_base(s.ptr)
        for j in range(len(s.ptr) - 1):
            for u in range(int(base[j]), int(base[j]) + (int(s.ptr[j + 1]) - int(s.ptr[j])) // 256):
                m, ls, end = p4_modes.parse32(s.packed, int(s.offs[u]), 256, 256)
                assert end == int(s.offs[u + 1]), (s.name, u, m)
                modes[m] += 1
                lens.update(ls)
    return modes, lens


def joined(streams, prefix=0, seed=1):
    """Several streams as one index: their bytes after `prefix` junk bytes, the
    lists in order.  -> (Stream, list_byte)"""
    rng = np.random.default_rng(seed)
    parts, offs, ptr, at, pv = [rng.integers(0, 256, size=prefix, dtype=np.uint8)], [], [np.zeros(1, np.uint64)], prefix, 0
    for s in streams:
        parts.append(s.packed)
        offs.append(np.asarray(s.offs[:-1], dtype=np.uint64) + np.uint64(at))
        at += len(s.packed)
        p = np.asarray(s.ptr, dtype=np.uint64)
        ptr.append(p[1:] - p[0] + np.uint64(pv))
        pv += int(p[-1] - p[0])
    offs.append(np.array([at], dtype=np.uint64))
    s = Stream("+".join(x.name for x in streams), np.concatenate(parts), np.concatenate(offs), np.concatenate(ptr))
    return s, list_byte(s)


def parse_sites(s):
    """Byte positions the scan's answer depends on, by what they hold: {kind:
    [position]} for header, bx, xn, bitmap, marker bytes and the last byte of
    every list."""
    sites = collections.defaultdict(list)
    base = unit_base(s.ptr)
    for j in range(len(s.ptr) - 1):
        n = int(s.ptr[j + 1]) - int(s.ptr[j])
        for i, u in enumerate(range(int(base[j]), int(base[j + 1]))):
            full = i < n // 256
            cnt = 256 if full else n % 256
            pos = int(s.offs[u])
            h = int(s.packed[pos])
            sites["header"].append(pos)
            mode, ls, end = p4_modes.parse32(s.packed, pos, cnt, 256 if full else None)
            if mode == "bitmap":
                sites["bx"].append(pos + 1)
                sites["bitmap"] += [pos + 2, pos + 2 + (cnt + 7) // 8 - 1]
            elif mode in ("vb_raw", "vb_comp"):
                sites["xn"].append(pos + 1)
                v0 = pos + 2 + ((256 if full else cnt) * (h & 0x3F) + 7) // 8
                sites["marker"].append(v0)
                if ls:
                    sites["marker"].append(v0 + sum(ls[:-1]))
        if n:
            sites["last"].append(int(s.offs[base[j + 1]]) - 1)
    return sites


def corruptions(s, count, seed=2):
    """`count` seeded (position, new byte) pairs over the parse sites, every kind in turn."""
    rng = np.random.default_rng(seed)
    sites = parse_sites(s)
    kinds = sorted(sites)
    assert set(kinds) == {"header", "bx", "xn", "bitmap", "marker", "last"}, kinds
    out = []
    for k in range(count):
        pos = int(rng.choice(sites[kinds[k % len(kinds)]]))
        old = int(s.packed[pos])
        new = int(rng.choice([0x3F, 0x7F, 0xBF, 0xFF, 0x21, 0xA1, 0x61, 0xE1, 0x40, 0x80, 0xC0])) if k % 3 == 0 else int(rng.integers(0, 256))
        out.append((pos, new if new != old else old ^ 0x55))
    return out


def want_with_bad(s, lbyte, bad_units):
    """What the scan writes for a stream whose units `bad_units` (the first bad
    unit of each offending list) are refused: the oracle's offsets, and in an
    offending list the end of its span after the bad unit."""
    want = np.asarray(s.offs, dtype=np.uint64).copy()
    want[-1] = lbyte[-1]
    base = unit_base(s.ptr)
    for u in bad_units:
        j = int(np.searchsorted(base, u, side="right")) - 1
        want[u + 1: int(base[j + 1])] = lbyte[j + 1]
    return want
