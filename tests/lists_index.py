"""A resident index for the intersection tests (tests/test_gpu_lists_intersect.py):
the oracle's composition of a set of lists (tests/lists_ref.py) with its unit
directory and the skip table its values imply, the sentinel-guarded device
buffers the outputs are written into, and the numpy restatement of
tpf_lists_intersect's definition for lists that ascend.  Test infrastructure
only."""
import numpy as np

import lists_ref as ref

DEV = "cuda:0"
SENT = 0xA5A5A5A5
SENT64 = 0x5A5A5A5A5A5A5A5A
CLEAN = -1  # UINT64_MAX read back as int64
PADV = 64   # sentinel values before and after an output


class Index:
    """A composed delta-1 stream with its directory and the skip table its values imply."""

    def __init__(self, lens, rng, ptr0=0, start0=None, start_bits=32, lists=None):
        nl = len(lens) if lists is None else len(lists)
        self.start0 = rng.integers(0, 1 << start_bits, size=nl, dtype=np.uint64).astype(np.uint32) if start0 is None else start0
        self.lists = [ref.d1_values(n, int(self.start0[j]), rng) for j, n in enumerate(lens)] if lists is None else lists
        self.packed, self.offs, self.ptr, self.vals = ref.compose(self.lists, True, self.start0, ptr0=ptr0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.lens = [len(v) for v in self.lists]
        self.nlists, self.nunits = len(self.lens), len(self.offs) - 1
        # the definition: entry u = the last value of unit i of list j, position min(256 (i + 1), n) - 1
        self.table = np.array([v[min(256 * (i + 1), len(v)) - 1] for v in self.lists for i in range(ref.n_units(len(v)))], dtype=np.uint32)
        assert len(self.table) == self.nunits

    def of_len(self, n):
        return self.lens.index(n)

    def units(self, j):
        return ref.n_units(self.lens[j])

    def ascends(self):
        """no list wraps mod 2^32: every list is strictly increasing from its start"""
        return all(len(v) == 0 or (int(v[0]) > int(s) and (np.diff(v.astype(np.int64)) > 0).all()) for v, s in zip(self.lists, self.start0))


def dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def dev64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev8(torch, a, shift=0, pad=64):
    """packed bytes on the device, `shift` bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    buf = torch.zeros(len(a) + pad + 32, dtype=torch.uint8, device=DEV)
    s = (shift - buf.data_ptr()) % 16
    view = buf[s: s + len(a) + pad]
    assert view.data_ptr() % 16 == shift % 16
    view[: len(a)] = torch.from_numpy(a).to(DEV)
    return view


class Guarded32:
    """n uint32 values, the first 4 bytes past a 16-byte boundary, inside a sentinel-filled buffer"""

    def __init__(self, torch, n):
        self.n = n
        self.big = torch.full((n + 2 * PADV + 8,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
        self.s = PADV + ((4 - self.big.data_ptr() - 4 * PADV) % 16) // 4
        self.view = self.big[self.s: self.s + n]
        assert self.view.data_ptr() % 16 == 4 or n == 0

    def read(self):
        """-> (the n values, True when every value around them is still the sentinel)"""
        got = self.big.cpu().numpy().view(np.uint32)
        return got[self.s: self.s + self.n], bool((got[:self.s] == SENT).all() and (got[self.s + self.n:] == SENT).all())


class Guarded64:
    def __init__(self, torch, n):
        self.n = n
        self.big = torch.full((n + 16,), SENT64, dtype=torch.int64, device=DEV)
        self.view = self.big[8: 8 + n]

    def read(self):
        got = self.big.cpu().numpy()
        return got[8: 8 + self.n], bool((got[:8] == SENT64).all() and (got[8 + self.n:] == SENT64).all())


def want_hits(ix, queries, ptr0):
    """The definition for an ascending index with a correct table: v is a hit
    iff it is in list j, at the position np.searchsorted finds.  queries:
    [(list, probe values)] in call order, the probe laid end to end from index
    ptr0.  -> (values, out_ptr, pidx, tpos)"""
    vals, pidx, tpos, out_ptr, at = [], [], [], [0], ptr0
    for j, pv in queries:
        pv = np.asarray(pv, dtype=np.uint32)
        lst = ix.lists[j]
        hit = np.isin(pv, lst)
        vals.append(pv[hit])
        pidx.append(at + np.nonzero(hit)[0])
        tpos.append(np.searchsorted(lst, pv[hit]))
        out_ptr.append(out_ptr[-1] + int(hit.sum()))
        at += len(pv)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return cat(vals, np.uint32), np.asarray(out_ptr, dtype=np.int64), cat(pidx, np.uint32), cat(tpos, np.uint32)
