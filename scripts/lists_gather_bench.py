#!/usr/bin/env python
"""Measurement of the positional read of a resident index (tpf_lists_gather);
recorded in profiles/lists_gather_bench.json, not gated.  Timed the way
bench.py times its steps (scripts/lists_bench.py's `timed`): warm-up, HIP
events around every call on the launch stream, median over the steps; the
calls of a leg -- the gather and what it is held against -- alternate step by
step.  All legs in one process on one box.  The index is scripts/lists_intersect_bench.py's
Zipf(1.5) delta-1 index plus a plain stream of term frequencies with the same
list structure.  Every result is checked at full size on the device against a
torch gather from the fully decoded stream (tpf_p4ndec256v32_lists).  Every leg
is timed against what the library could do for the same request before this
entry point, never against the code under test.

(a) sparse: the frequencies of the hits of lists_intersect_bench.py's leg (a)
    -- 4,096 queries, the positions are the intersection's d_out_tpos, fed with
    d_out_ptr and d_qlist unchanged (`chained`: pos_values is the capacity of
    d_out_tpos, the probe's length) and with the position array cut to the hits
    (`trimmed`, which needs the host to know their number).  Against: the plain
    units decode of the unit each position names, one selection per position
    (the host knows the number of hits here too), plus the torch index
    arithmetic before it (the query of every position, its unit) and the torch
    gather after it.
(b) one random position per block of the same 4,096 long target lists.
    Against: the plain units decode of those lists, whole, plus the torch
    arithmetic and gather.
(c) dense: every position of a list of about 2.09M values (the dense index of
    lists_intersect_bench.py).  Against the plain units decode of the whole
    list, which IS the answer.
(d) the delta-1 form of (a): the doc ids at the hits' positions.

    python scripts/lists_gather_bench.py [--nblocks N] [--steps K] [--warmup W] [--legs sparse,perblock,dense,sparse_d1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "turbopfor-cpp_amd", "python"))

import bench_data  # noqa: E402
import lists_bench as lb  # noqa: E402
import lists_intersect_bench as lxb  # noqa: E402
from lists_intersect_bench import u32  # noqa: E402
from lists_select_bench import Index  # noqa: E402


def frequencies(nv, dev, seed):
    """term frequencies: 1..8, about 3 % of them up to 1,031 -- generated in chunks"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = torch.empty(nv, dtype=torch.int32, device=dev)
    for a in range(0, nv, bench_data.CHUNK):
        b = min(a + bench_data.CHUNK, nv)
        r = torch.randint(0, 1 << 30, (b - a,), generator=g, device=dev, dtype=torch.int32)
        out[a:b] = 1 + (r & 7) + torch.where(((r >> 3) & 31) == 0, (r >> 8) & 1023, torch.zeros_like(r))
    return out


class Streams:
    """the delta-1 index (with its skip table), the plain stream over the same directory, and both fully decoded"""

    def __init__(self, tpf, flat, ptr, fflat):
        self.tpf, self.ptr = tpf, ptr
        self.d = Index(tpf, flat, ptr, True)
        self.table = tpf.lists_unit_last(self.d.packed, self.d.offs, ptr, start0=self.d.start0)
        self.f = Index(tpf, fflat, ptr, False)
        assert torch.equal(self.d.unit, self.f.unit) and self.d.nu == self.f.nu
        err = torch.zeros(2, dtype=torch.int64, device=flat.device)
        dec = tpf.decn256v32_lists(self.d.packed, self.d.offs, ptr, d1=True, start0=self.d.start0, out=torch.empty_like(flat), err=err[0:1])
        self.decoded_ok = bool(torch.equal(dec, flat))
        del dec
        self.fdec = tpf.decn256v32_lists(self.f.packed, self.f.offs, ptr, d1=False, out=torch.empty_like(fflat), err=err[1:2])
        self.decoded_ok = self.decoded_ok and bool(torch.equal(self.fdec, fflat)) and err.tolist() == [-1, -1]
        self.ddec = flat  # bit for bit the full decode, checked above

    def gather(self, d1, pos, pptr, qlist, out, err=None, ws=None):
        ix = self.d if d1 else self.f
        return self.tpf.lists_gather(ix.packed, ix.offs, self.ptr, ix.unit, pos, pptr, qlist, d1=d1, start0=ix.start0 if d1 else None,
                                     unit_last=self.table if d1 else None, out=out, err=err, ws=ws)

    def units(self, d1, sel, uf, uc, out, optr, err=None, ws=None):
        ix = self.d if d1 else self.f
        return self.tpf.decn256v32_lists_units(ix.packed, ix.offs, self.ptr, ix.unit, sel, uf, uc, d1=d1, start0=ix.start0 if d1 else None,
                                               unit_last=self.table if d1 else None, out=out, out_ptr=optr, err=err, ws=ws)

    def want(self, d1, pos, pptr, qlist):
        """the torch gather from the fully decoded stream -> (first index, end, values)"""
        a, b = int(pptr[0].item()), int(pptr[-1].item())
        i = torch.arange(a, b, dtype=torch.int64, device=pos.device)
        k = torch.searchsorted(pptr[1:].contiguous(), i, right=True)
        return a, b, (self.ddec if d1 else self.fdec)[self.ptr[qlist.long()[k]] + u32(pos[a:b])]


def timed_alternately(fns, steps, warmup):
    """lists_bench.timed for several calls at once: every step runs each of them in turn, each between its own pair of events, so a
    drift of the clocks or of the host over the run falls on all of them alike -> one timing per call"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for _ in fns]
    for k in range(steps):
        for fn, ev in zip(fns, evs):
            ev[k][0].record(stream)
            fn()
            ev[k][1].record(stream)
    torch.cuda.synchronize()
    res = []
    for ev in evs:
        ms = [a.elapsed_time(b) for a, b in ev]
        res.append({"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4)})
    return res


def prep_gather(S, L, d1, pos, pptr, qlist):
    """-> (verified, the call to time, workspace bytes) of one gather call, checked at full size"""
    dev, nq = pos.device, qlist.numel()
    out = torch.full_like(pos, -1)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(L.tpf_lists_gather_workspace_size(nq, pos.numel())), 1), dtype=torch.uint8, device=dev)
    S.gather(d1, pos, pptr, qlist, out, err=err, ws=ws)
    a, b, want = S.want(d1, pos, pptr, qlist)
    ok = int(err.item()) == -1 and bool(torch.equal(out[a:b], want)) and bool((out[:a] == -1).all()) and bool((out[b:] == -1).all())
    return ok, lambda: S.gather(d1, pos, pptr, qlist, out, ws=ws), ws.numel()


def prep_unit_per_position(S, L, d1, pos, pptr, qlist, npos):
    """what the library offered before: the unit of every position decoded to memory, torch before and after"""
    dev = pos.device
    ones = torch.ones(npos, dtype=torch.int32, device=dev)
    idx = torch.arange(npos, dtype=torch.int64, device=dev) + pptr[0]
    cap = 256 * npos
    bout = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)[:cap]
    bptr = torch.zeros(npos + 1, dtype=torch.int64, device=dev)
    bws = torch.empty(max(int(L.tpf_p4ndec256v32_lists_units_workspace_size(npos, cap)), 1), dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    ends = pptr[1:].contiguous()
    res = {}

    def run(e=None):
        p = pos[idx]
        sel = qlist[torch.searchsorted(ends, idx, right=True)]
        S.units(d1, sel, p >> 8, ones, bout, bptr, err=e, ws=bws)
        res["v"] = bout[bptr[:-1] + (p & 255)]

    run(err)
    _, _, want = S.want(d1, pos, pptr, qlist)
    ok = int(err.item()) == -1 and bool(torch.equal(res["v"], want))
    return ok, run, int(bptr[-1].item())


def sparse_leg(S, L, args, d1, tpos, optr, qlist, nhits):
    chained = prep_gather(S, L, d1, tpos, optr, qlist)
    trimmed = prep_gather(S, L, d1, tpos[:nhits].contiguous(), optr, qlist)
    base = prep_unit_per_position(S, L, d1, tpos, optr, qlist, nhits)
    t_c, t_t, t_b = timed_alternately([chained[1], trimmed[1], base[1]], args.steps, args.warmup)
    return {"verified": chained[0] and trimmed[0] and base[0], "queries": qlist.numel(), "positions": nhits, "pos_values_chained": tpos.numel(),
            "gather_chained": t_c, "gather_trimmed": t_t, "units_decode_plus_torch": t_b,
            "values_decoded_by_baseline": base[2], "gather_workspace_bytes_chained": chained[2],
            "ratio_gather_chained_over_baseline_time": round(t_c["ms_median"] / t_b["ms_median"], 4),
            "ratio_gather_trimmed_over_baseline_time": round(t_t["ms_median"] / t_b["ms_median"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_gather_bench.json"))
    ap.add_argument("--legs", default="sparse,perblock,dense,sparse_d1", help="the legs to run (a per-kernel profile wants one at a time)")
    args = ap.parse_args()
    args.legs = args.legs.split(",")
    import turbopfor_amd as tpf

    dev = "cuda:0"
    L = tpf.lib()
    nb, nv = args.nblocks, args.nblocks * 256
    out = {"nblocks": nb, "values": nv, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "kernel_md5": tpf.kernel_md5(),
           "generator": f"scripts/lists_bench.py: bounded Zipf(s={lb.ZIPF_S}) on [1, {lb.ZIPF_MAX}] over bench_data.gen_c3(nblocks, seed=7); "
                        "frequencies: scripts/lists_gather_bench.py frequencies(seed=19)"}
    t0 = time.time()
    vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
    flat = vals.view(-1)
    ptr = lb.zipf_lengths(nv, 7, dev)
    nl = ptr.numel() - 1
    ln = ptr[1:] - ptr[:-1]
    out["lists"] = nl
    flatok = torch.ones(nl, dtype=torch.bool, device=dev)  # lists that hold no wrap (lists_intersect_bench.py)
    for a in range(0, nv - 1, bench_data.CHUNK):
        x = flat[a: min(a + bench_data.CHUNK + 1, nv)] ^ -(1 << 31)
        w = torch.nonzero(x[1:] < x[:-1]).view(-1) + a + 1
        j = torch.searchsorted(ptr, w, right=True) - 1
        flatok[j[w > ptr[j]]] = False
    fflat = frequencies(nv, dev, 19)
    S = Streams(tpf, flat, ptr, fflat)
    del fflat
    out["units"] = S.d.nu
    out["bytes_per_int"] = {"doc_ids": round(S.d.packed.numel() / nv, 4), "frequencies": round(S.f.packed.numel() / nv, 4)}
    ok_all = S.decoded_ok
    rng = np.random.default_rng(11)

    # the queries of lists_intersect_bench.py's leg (a), and their hits
    probes, targets, _ = lxb.sparse_queries(flat, ptr, flatok, rng)
    nq = len(probes)
    psel = torch.tensor(probes, dtype=torch.int32, device=dev)
    qlist = torch.tensor(targets, dtype=torch.int32, device=dev)
    total = int(ln[psel.long()].sum().item())
    probe = torch.zeros(total, dtype=torch.int32, device=dev)
    pptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    S.d.select(psel, probe, pptr)
    hit = torch.zeros(total, dtype=torch.int32, device=dev)
    tpos = torch.full((total,), -1, dtype=torch.int32, device=dev)
    optr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    tpf.lists_intersect(S.d.packed, S.d.offs, ptr, S.d.unit, S.table, probe, pptr, qlist, start0=S.d.start0, out=hit, out_ptr=optr, tpos=tpos,
                        err=err)
    nhits = int(optr[-1].item())
    ok_all = ok_all and nq == lxb.NQ and int(err.item()) == -1 and nhits > 0

    for name, d1 in (("sparse", False), ("sparse_d1", True)):
        if name in args.legs:
            r = sparse_leg(S, L, args, d1, tpos, optr, qlist, nhits)
            if d1:  # the doc ids at the hits' positions are the hits
                got = torch.empty_like(tpos)
                S.gather(True, tpos, optr, qlist, got)
                r["verified"] = r["verified"] and bool(torch.equal(got[:nhits], hit[:nhits]))
            out[name] = r
            ok_all = ok_all and r["verified"]
            print(f"[lists_gather_bench] {name}:", json.dumps(r), flush=True)

    # ---- (b) one random position per block of the same targets
    if "perblock" in args.legs:
        n_t = ln[qlist.long()]
        units = (n_t + 255) // 256
        bptr_q = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        bptr_q[1:] = torch.cumsum(units, 0)
        npos = int(bptr_q[-1].item())
        k = torch.repeat_interleave(torch.arange(nq, device=dev), units)
        u = torch.arange(npos, dtype=torch.int64, device=dev) - bptr_q[:-1][k]
        width = torch.clamp(n_t[k] - 256 * u, max=256)
        g = torch.Generator(device=dev)
        g.manual_seed(23)
        pos = (256 * u + (torch.rand(npos, generator=g, device=dev, dtype=torch.float64) * width).to(torch.int64)).to(torch.int32)
        okg, call_g, wsb = prep_gather(S, L, False, pos, bptr_q, qlist)
        # before: the lists decoded whole, then the query of every position, its index and the gather with torch
        uf, uc = torch.zeros(nq, dtype=torch.int32, device=dev), units.to(torch.int32)
        cap = int(n_t.sum().item())
        bout, bp = torch.zeros(cap, dtype=torch.int32, device=dev), torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        bws = torch.empty(int(L.tpf_p4ndec256v32_lists_units_workspace_size(nq, cap)), dtype=torch.uint8, device=dev)
        idx, ends, res = torch.arange(npos, dtype=torch.int64, device=dev), bptr_q[1:].contiguous(), {}

        def whole(e=None):
            S.units(False, qlist, uf, uc, bout, bp, err=e, ws=bws)
            res["v"] = bout[bp[torch.searchsorted(ends, idx, right=True)] + pos]

        whole(err)
        _, _, want = S.want(False, pos, bptr_q, qlist)
        okb = int(err.item()) == -1 and bool(torch.equal(res["v"], want))
        t_g, t_b = timed_alternately([call_g, whole], args.steps, args.warmup)
        out["perblock"] = {"verified": okg and okb, "queries": nq, "positions": npos, "gather": t_g, "units_decode_of_the_lists_plus_torch": t_b,
                           "values_decoded_by_baseline": cap, "gather_workspace_bytes": wsb,
                           "gather_M_positions_s": round(npos / (t_g["ms_median"] * 1e-3) / 1e6, 1),
                           "ratio_gather_over_baseline_time": round(t_g["ms_median"] / t_b["ms_median"], 4)}
        ok_all = ok_all and okg and okb
        print("[lists_gather_bench] perblock:", json.dumps(out["perblock"]), flush=True)
        del bout, res, want, pos, idx, k, u
    del S, flat, vals, probe, hit, tpos
    if "dense" not in args.legs:
        return lxb.finish(out, args, t0, ok_all)

    # ---- (c) dense: every position of one list of lists_intersect_bench.py's dense index
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    universe = torch.unique(torch.randint(1, 1 << 31, (1 << 22,), generator=g, device=dev, dtype=torch.int64))
    lists = [universe[torch.rand(universe.numel(), generator=g, device=dev) < 0.5] for _ in range(3)]
    dflat = torch.cat(lists).to(torch.int32)
    dptr = torch.tensor(np.concatenate([[0], np.cumsum([v.numel() for v in lists])]), dtype=torch.int64, device=dev)
    D = Streams(tpf, dflat, dptr, frequencies(dflat.numel(), dev, 29))
    n1 = lists[1].numel()
    q1 = torch.tensor([1], dtype=torch.int32, device=dev)
    pos = torch.arange(n1, dtype=torch.int32, device=dev)
    pp = torch.tensor([0, n1], dtype=torch.int64, device=dev)
    okg, call_g, wsb = prep_gather(D, L, False, pos, pp, q1)
    units1 = (n1 + 255) // 256
    uf, uc = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([units1], dtype=torch.int32, device=dev)
    bout, bp = torch.zeros(n1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    bws = torch.empty(int(L.tpf_p4ndec256v32_lists_units_workspace_size(1, n1)), dtype=torch.uint8, device=dev)
    D.units(False, q1, uf, uc, bout, bp, err=err, ws=bws)
    okb = int(err.item()) == -1 and D.decoded_ok and bool(torch.equal(bout, D.fdec[int(dptr[1].item()): int(dptr[2].item())]))
    t_g, t_b = timed_alternately([call_g, lambda: D.units(False, q1, uf, uc, bout, bp, ws=bws)], args.steps, args.warmup)
    out["dense"] = {"verified": okg and okb, "positions": n1, "units": units1, "gather": t_g, "units_decode_of_the_whole_list": t_b,
                    "gather_workspace_bytes": wsb, "gather_G_positions_s": lb.rate(n1, t_g),
                    "ratio_gather_over_decode_time": round(t_g["ms_median"] / t_b["ms_median"], 4)}
    ok_all = ok_all and okg and okb
    print("[lists_gather_bench] dense:", json.dumps(out["dense"]), flush=True)
    return lxb.finish(out, args, t0, ok_all)


if __name__ == "__main__":
    sys.exit(main())
