"""The numpy restatement of tpf_lists_remove (include/turbopfor_gpu.h): np.delete
per list, then the oracle's composition of the shortened lists
(tests/lists_ref.py), with the skip table from its definition.  Also the case
matrix the CPU and the GPU tests of the call share.  Test infrastructure only."""
import numpy as np

import lists_ref as ref

LENS = [0, 1, 255, 256, 257, 511, 512, 513, 256 * 17 + 3]
PATTERNS = ["none", "first", "last", "p255", "p256", "p255_256", "tail", "lastfull", "unit", "all", "tenth"]
PTR0, POS0, PTRAIL = 37, 5, 7  # d_list_ptr[0], d_pos_ptr[0], unread entries after the positions
JUNK = 0xDEADBEEF


def positions(pattern, n, rng):
    """The removed positions of `pattern` in a list of n values, or None where the pattern does not apply."""
    full = n // 256
    if pattern == "none":
        return np.zeros(0, np.uint32)  # targeted, with an empty segment
    if n == 0:
        return None
    got = {
        "first": [0],
        "last": [n - 1],
        "p255": [255] if n > 255 else None,
        "p256": [256] if n > 256 else None,
        "p255_256": [255, 256] if n > 256 else None,
        "tail": list(range(256 * full, n)) if n % 256 else None,          # the list ends on a full block
        "lastfull": [256 * (full - 1) + 100] if full else None,           # the tail shrinks by one, or appears
        "unit": list(range(256 * (full // 2), 256 * (full // 2 + 1))) if full else None,
        "all": list(range(n)),
        "tenth": sorted(rng.choice(n, size=max(1, n // 10), replace=False).tolist()),
    }[pattern]
    return None if got is None else np.asarray(got, dtype=np.uint32)


def table(lists):
    """The skip table by its definition: the last value of every unit."""
    return np.array([v[min(256 * (i + 1), len(v)) - 1] for v in lists for i in range(ref.n_units(len(v)))], dtype=np.uint32)


def remove(lists, removals):
    """removals: {list: ascending positions}.  -> the shortened lists (list ids are stable)."""
    return [np.delete(v, np.asarray(removals[j], dtype=np.int64)) if j in removals else v for j, v in enumerate(lists)]


class Case:
    """An old index (the oracle's composition of `lists`), removals {list: positions} and the expected new index."""

    def __init__(self, lists, removals, d1, start0=None, ptr0=PTR0, pos0=POS0):
        self.d1, self.lists, self.removals, self.start0 = d1, lists, removals, start0 if d1 else None
        self.nlists = len(lists)
        self.packed, self.offs, self.ptr, _ = ref.compose(lists, d1, self.start0, ptr0=ptr0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.nunits = len(self.offs) - 1
        self.table = table(lists)
        self.qlist = np.asarray(sorted(removals), dtype=np.uint32)
        self.nq = len(self.qlist)
        segs = [np.asarray(removals[int(j)], dtype=np.uint32) for j in self.qlist]
        self.pos = np.concatenate([np.full(pos0, JUNK, np.uint32)] + segs + [np.full(PTRAIL, JUNK, np.uint32)])
        self.pptr = pos0 + np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
        self.u0 = {int(j): int(s[0]) // 256 for j, s in zip(self.qlist, segs) if len(s)}
        self.staged = sum(len(lists[j]) - 256 * u for j, u in self.u0.items())
        self.targeted = sum(len(lists[int(j)]) for j in self.qlist)
        # the expected index
        self.new = remove(lists, removals)
        self.xpacked, self.xoffs, self.xptr, self.xvals = ref.compose(self.new, d1, self.start0)
        self.xbase = np.asarray(ref.units_loop(self.xptr)[1], dtype=np.uint32)
        self.xunits = len(self.xoffs) - 1
        self.xtable = table(self.new)

    def list_bytes(self, j, new=False):
        offs, base, packed = (self.xoffs, self.xbase, self.xpacked) if new else (self.offs, self.base, self.packed)
        return packed[int(offs[base[j]]): int(offs[base[j + 1]])]


def values(n, d1, s0, rng):
    return ref.d1_values(n, int(s0), rng, outliers=True) if d1 else ref.plain_values(n, rng)


def matrix_plan(rng):
    """[(length, pattern or None)]: every applicable (length, pattern) pair in a seeded order, an untargeted list
    (pattern None) of a length of LENS after every second targeted one, untargeted empties at both ends."""
    pairs = [(n, p) for n in LENS for p in PATTERNS if positions(p, n, np.random.default_rng(0)) is not None]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    plan = [(0, None)] * 2
    for i, pr in enumerate(pairs):
        plan.append(pr)
        if i % 2:
            plan.append((LENS[(i // 2) % len(LENS)], None))
    return plan + [(0, None)] * 2


def matrix_case(d1, st, seed=4321):
    rng = np.random.default_rng(seed + 2 * d1 + st)
    plan = matrix_plan(rng)
    start0 = rng.integers(0, 1 << 31, size=len(plan), dtype=np.uint64).astype(np.uint32) if (d1 and st) else None
    s0 = start0 if start0 is not None else np.zeros(len(plan), np.uint32)
    lists = [values(n, d1, s0[j], rng) for j, (n, _) in enumerate(plan)]
    removals = {j: positions(p, n, rng) for j, (n, p) in enumerate(plan) if p is not None}
    c = Case(lists, removals, d1, start0)
    c.plan = plan
    return c
