"""Expected streams of the many-lists decode (tpf_p4ndec256v32_lists): every
list's stream is the oracle's n-variant composition (oracle_lib.encn256v32,
pinned to the reference call by call in tests/test_nstream_cpu.py), the lists
laid end to end with their offsets shifted.  The expected decode is the
original values.  Test infrastructure only."""
import numpy as np

import oracle_lib as orc

# the list lengths of the shape matrix: around one unit, around the 16-unit
# decode runs, the 64-unit sum runs and the 4 x 16-unit workgroups
MATRIX = [0, 1, 5, 255, 256, 257, 511, 512, 513, 256 * 15, 256 * 16, 256 * 16 + 1, 256 * 17 + 3, 256 * 63 + 255, 256 * 64,
          256 * 64 + 1, 256 * 130 + 77]


def n_units(n):
    return n // 256 + (1 if n % 256 else 0)


def units_loop(list_ptr):
    """Plain-loop statement of turbopfor_amd.lists_units."""
    units, base = [], [0]
    for j in range(len(list_ptr) - 1):
        n = int(list_ptr[j + 1]) - int(list_ptr[j])
        units.append(n_units(n))
        base.append(base[-1] + units[-1])
    return units, base


def compose(lists, d1=False, start0=None, ptr0=0):
    """lists: sequence of uint32 arrays.  -> (packed u8, offsets u64 [nunits+1],
    list_ptr u64 [nlists+1] starting at ptr0, values u32 concatenated)."""
    parts, offs, ptr, total = [], [np.zeros(1, np.uint64)], [ptr0], 0
    for j, v in enumerate(lists):
        s0 = int(start0[j]) if (d1 and start0 is not None) else 0
        p, o = orc.encn256v32(v, d1=d1, start0=s0)
        assert len(o) == n_units(len(v)) + 1
        parts.append(np.asarray(p, dtype=np.uint8))
        offs.append(np.asarray(o[1:], dtype=np.uint64) + np.uint64(total))
        total += int(o[-1])
        ptr.append(ptr[-1] + len(v))
    packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    vals = np.concatenate([np.asarray(v, dtype=np.uint32) for v in lists]) if lists else np.zeros(0, np.uint32)
    return packed, np.concatenate(offs), np.asarray(ptr, dtype=np.uint64), vals


def plain_values(n, rng):
    """test_gpu_nstream.py's _values: mixed widths per 64 values, 5 % outliers."""
    bw = rng.integers(0, 33, size=n // 64 + 1)
    raw = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    mask = np.array([(1 << int(b)) - 1 for b in bw], dtype=np.uint64).repeat(64)[:n]
    v = (raw & mask).astype(np.uint32)
    hit = rng.random(n) < 0.05
    v[hit] = rng.integers(0, 1 << 32, size=int(hit.sum()), dtype=np.uint64).astype(np.uint32)
    return v


def d1_values(n, start0, rng, outliers=False):
    """A posting list after start0: gaps >= 1 (mod 2^32).  outliers: per
    256-value block a gap width and an outlier rate from 0.5 % to 30 %, so the
    encoder picks vbyte exceptions for some blocks and bitmaps for others."""
    if not outliers:
        gaps = rng.integers(1, 1 << 14, size=n, dtype=np.uint64)
    else:
        nb = n // 256 + 1
        bw = rng.integers(1, 12, size=nb).repeat(256)[:n]
        rate = rng.choice([0.005, 0.03, 0.1, 0.3], size=nb).repeat(256)[:n]
        gaps = (rng.integers(0, 1 << 62, size=n, dtype=np.uint64) & ((np.uint64(1) << bw.astype(np.uint64)) - np.uint64(1))) + np.uint64(1)
        hit = rng.random(n) < rate
        big = rng.integers(12, 31, size=n)
        gaps[hit] = (rng.integers(0, 1 << 62, size=n, dtype=np.uint64) & ((np.uint64(1) << big.astype(np.uint64)) - np.uint64(1)))[hit] + np.uint64(1)
    return ((np.cumsum(gaps) + np.uint64(start0)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def block_kinds(packed, offsets, list_ptr):
    """Counts of the full blocks' exception kinds by header byte: 'vbyte'
    (0x40 set), 'bitmap' (0x80 set, 0x40 clear), 'const' (both), 'plain'."""
    kinds = {"vbyte": 0, "bitmap": 0, "const": 0, "plain": 0}
    _, base = units_loop(list_ptr)
    for j in range(len(list_ptr) - 1):
        nfull = (int(list_ptr[j + 1]) - int(list_ptr[j])) // 256
        for u in range(base[j], base[j] + nfull):
            h = int(packed[int(offsets[u])])
            kinds["const" if h & 0xC0 == 0xC0 else "vbyte" if h & 0x40 else "bitmap" if h & 0x80 else "plain"] += 1
    return kinds
