"""The numpy restatement of tpf_lists_difference's definition
(include/turbopfor_gpu.h) for an index that ascends with a correct table:
np.isin, np.searchsorted(lst, v, "left") and slices of the original lists,
never the code under test.  The probe may be in any order and may repeat
values: the definition is per value.  Test infrastructure only
(tests/test_lists_difference_cpu.py holds it against np.setdiff1d and against
the union's reference, tests/lists_union_ref.py)."""
import numpy as np

from lists_union_ref import edge_probe  # noqa: F401  (the probe at the edges of the shared definition)


def difference_one(lst, pv, at):
    """One query: list `lst`, probe values `pv` at probe indices at, at + 1, ...
    -> (values, pidx, tpos): the probe values that are not in the list, in
    probe order, their probe indices and the number of list values below them."""
    lst = np.asarray(lst, dtype=np.uint32)
    pv = np.asarray(pv, dtype=np.uint32)
    miss = ~np.isin(pv, lst)
    L = np.searchsorted(lst, pv, side="left")  # min(256 (u - ua) + q, n); n where no unit's last value reaches v
    return pv[miss], (at + np.nonzero(miss)[0]).astype(np.uint32), L[miss].astype(np.uint32)


def want_difference(ix, queries, ptr0):
    """queries: [(list, probe values)] in call order, the probe laid end to end
    from index ptr0.  -> (values, out_ptr, pidx, tpos)"""
    vals, pidx, tpos, out_ptr, at = [], [], [], [0], ptr0
    for j, pv in queries:
        v, pi, tp = difference_one(ix.lists[j], pv, at)
        vals.append(v)
        pidx.append(pi)
        tpos.append(tp)
        out_ptr.append(out_ptr[-1] + len(v))
        at += len(pv)
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)
    return cat(vals), np.asarray(out_ptr, dtype=np.int64), cat(pidx), cat(tpos)


def want_difference_keys(ix, qlist, probe_ptr, probe):
    """The same for a whole request at once, for the tests with many queries:
    every list value and every probe value as a key (k << 32) | value, k its
    query for the probe and its list for the index; a probe value is a miss
    iff (list << 32) | value is no key of the index, and its L is the number
    of keys of its list below it.  `ix`: anything with ptr, vals and nlists
    (lists_scale.ScaleIndex, lists_index.Index) whose lists ascend; probe_ptr:
    int64 [nq + 1] into `probe`.  -> (values, out_ptr, pidx, tpos)"""
    r = (np.asarray(ix.ptr, dtype=np.uint64) - np.uint64(ix.ptr[0])).astype(np.int64)
    key = lambda k, v: (np.asarray(k, dtype=np.uint64) << np.uint64(32)) | np.asarray(v, dtype=np.uint32).astype(np.uint64)
    keys = key(np.repeat(np.arange(ix.nlists), np.diff(r)), ix.vals)
    assert (keys[1:] > keys[:-1]).all()  # the precondition
    pp = np.asarray(probe_ptr, dtype=np.int64)
    nq = len(pp) - 1
    a, b = (int(pp[0]), int(pp[-1])) if nq else (0, 0)
    ql = np.repeat(np.asarray(qlist, dtype=np.int64), np.diff(pp))
    pv = np.asarray(probe, dtype=np.uint32)[a:b]
    pk = key(ql, pv)
    miss = ~np.isin(pk, keys)
    tpos = np.searchsorted(keys, pk[miss], side="left") - r[ql[miss]]
    out_ptr = np.concatenate([[0], np.cumsum(miss)]).astype(np.int64)[pp - a] if nq else np.zeros(1, np.int64)
    return pv[miss], out_ptr, (a + np.nonzero(miss)[0]).astype(np.uint32), tpos.astype(np.uint32)
