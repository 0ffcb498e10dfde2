"""The numpy restatement of tpf_lists_union's definition
(include/turbopfor_gpu.h) for an index that ascends with a correct table and
probes that ascend strictly: np.searchsorted, np.isin and slices of the
original lists, never the code under test.  Test infrastructure only
(tests/test_lists_union_cpu.py holds it against np.union1d)."""
import numpy as np

NONE = 0xFFFFFFFF  # TPF_LISTS_NONE


def union_one(lst, pv, at):
    """One query by the definition's formula: list `lst`, probe values `pv` at
    probe indices at, at + 1, ...  -> (values, pidx, tpos), every slot written
    exactly once."""
    lst = np.asarray(lst, dtype=np.uint32)
    pv = np.asarray(pv, dtype=np.uint32)
    n = len(lst)
    hit = np.isin(pv, lst)
    L = np.searchsorted(lst, pv, side="left")   # min(256 (u - ua) + q, n); n where no unit's last value reaches v
    M = np.cumsum(~hit) - ~hit                  # misses before every probe index
    total = n + int((~hit).sum())
    vals = np.zeros(total, np.uint32)
    pidx = np.full(total, NONE, np.uint32)
    tpos = np.full(total, NONE, np.uint32)
    written = np.zeros(total, np.int64)
    # misses: slot L + M
    ms = (L + M)[~hit]
    vals[ms] = pv[~hit]
    pidx[ms] = at + np.nonzero(~hit)[0]
    np.add.at(written, ms, 1)
    # list values: slot p + #{misses with L <= p}
    p = np.arange(n)
    ls = p + np.searchsorted(L[~hit], p, side="right")
    vals[ls] = lst
    tpos[ls] = p
    np.add.at(written, ls, 1)
    # hits: their probe index at slot L + M, the slot of the list value they equal
    hs = (L + M)[hit]
    assert np.array_equal(vals[hs], pv[hit])
    pidx[hs] = at + np.nonzero(hit)[0]
    assert (written == 1).all()
    return vals, pidx, tpos


def want_union(ix, queries, ptr0):
    """queries: [(list, probe values)] in call order, the probe laid end to end
    from index ptr0.  -> (values, out_ptr, pidx, tpos)"""
    vals, pidx, tpos, out_ptr, at = [], [], [], [0], ptr0
    for j, pv in queries:
        v, pi, tp = union_one(ix.lists[j], pv, at)
        vals.append(v)
        pidx.append(pi)
        tpos.append(tp)
        out_ptr.append(out_ptr[-1] + len(v))
        at += len(pv)
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)
    return cat(vals), np.asarray(out_ptr, dtype=np.int64), cat(pidx), cat(tpos)


def clip(x):
    return min(max(x, 0), 0xFFFFFFFF)


def edge_probe(ix, j):
    """A strictly ascending probe at the edges of the definition for list j:
    0, 0xFFFFFFFF, start0[j], each unit's last value and the next unit's first
    value, the list's first and last value and the last value + 1, each +- 1."""
    v = ix.lists[j]
    n = len(v)
    marks = {int(ix.start0[j]), 0, 0xFFFFFFFF}
    if n:
        marks |= {int(v[0]), int(v[-1]), int(v[-1]) + 1}
        for i in range((n + 255) // 256):
            if 256 * (i + 1) < n:
                marks |= {int(v[256 * (i + 1) - 1]), int(v[256 * (i + 1)])}
    return np.array(sorted({clip(m + d) for m in marks for d in (-1, 0, 1)}), dtype=np.uint32)


def want_union_keys(ix, qlist, probe_ptr, probe):
    """The same for a whole request at once, for the tests with many queries:
    query k's list values and probe values as keys (k << 32) | value, both
    ascending as a whole, merged by np.union1d.  `ix`: anything with ptr and
    vals (lists_scale.ScaleIndex, lists_index.Index); probe_ptr: int64
    [nq + 1] into `probe`.  -> (values, out_ptr, pidx, tpos)"""
    r = (np.asarray(ix.ptr, dtype=np.uint64) - np.uint64(ix.ptr[0])).astype(np.int64)
    q = np.asarray(qlist, dtype=np.int64)
    nq = len(q)
    pp = np.asarray(probe_ptr, dtype=np.int64)
    a, b = (int(pp[0]), int(pp[-1])) if nq else (0, 0)
    n = r[q + 1] - r[q]
    at = np.cumsum(n) - n
    inlist = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(at, n)  # the position of every list value in its list
    lvals = np.asarray(ix.vals, dtype=np.uint32)[np.repeat(r[q], n) + inlist]
    key = lambda k, v: (np.asarray(k, dtype=np.uint64) << np.uint64(32)) | np.asarray(v, dtype=np.uint32).astype(np.uint64)
    lkeys = key(np.repeat(np.arange(nq), n), lvals)
    pkeys = key(np.repeat(np.arange(nq), np.diff(pp)), np.asarray(probe, dtype=np.uint32)[a:b])
    assert (lkeys[1:] > lkeys[:-1]).all() and (pkeys[1:] > pkeys[:-1]).all()  # the precondition
    ukeys = np.union1d(lkeys, pkeys)
    out_ptr = np.searchsorted(ukeys, key(np.arange(nq + 1), 0)).astype(np.int64)
    pidx = np.full(len(ukeys), NONE, np.uint32)
    tpos = np.full(len(ukeys), NONE, np.uint32)
    pidx[np.searchsorted(ukeys, pkeys)] = a + np.arange(len(pkeys))
    tpos[np.searchsorted(ukeys, lkeys)] = inlist
    return (ukeys & np.uint64(0xFFFFFFFF)).astype(np.uint32), out_ptr, pidx, tpos
