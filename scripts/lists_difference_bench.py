#!/usr/bin/env python
"""Measurement of the difference with a resident index (tpf_lists_difference);
recorded in profiles/lists_difference_bench.json, not gated.  Timed the way
bench.py times its steps (scripts/lists_bench.py's `timed`): warm-up, HIP
events around every call on the launch stream, median over the steps.  All
legs in one process on one box, on the index and the queries of
scripts/lists_intersect_bench.py.  Every result is checked at full size on the
device against ~torch.isin (values, pointers, probe indices) and
torch.searchsorted (the insertion positions).

Every leg is timed against two things:
  - tpf_lists_intersect of the same library on the same arguments: the floor,
    the same lookup with another compaction;
  - what a user does without the call: the intersection with d_out_pidx, then
    torch -- a mask over the probe, the compaction, the pointers rebuilt from a
    prefix sum (the mask's compaction reads its size back, as torch does).

(a) sparse: the intersection bench's 4,096 queries, short lists of the index
    as probes against long lists that cover them.
(a') spread: the same targets, each probed with 128 values spread over the
    whole list, half of them members.
(b) dense: a list of about 2.09M values minus another over the same universe.
(c) tombstones: the 4,096-query result of (a')'s intersection minus one long
    list of deleted ids, about 1 % of the index's values, in an index of its
    own: every query names the same target.
(d) (A AND B) AND NOT C over the three lists of (b): an intersection and a
    difference chained on the device.

    python scripts/lists_difference_bench.py [--nblocks N] [--steps K] [--warmup W] [--legs sparse,spread,tombstones,dense,chain] [--out FILE]

--legs runs a subset (the committed JSON holds all): a rocprofv3
--kernel-trace --stats run of one leg gives that leg's per-kernel times.
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
from lists_intersect_bench import Resident, finish, u32  # noqa: E402


def difference(res, probe, probe_ptr, qlist, out, out_ptr, pidx=None, tpos=None, err=None, ws=None):
    ix = res.ix
    return res.tpf.lists_difference(ix.packed, ix.offs, ix.ptr, ix.unit, res.table, probe, probe_ptr, qlist, start0=ix.start0, out=out,
                                    out_ptr=out_ptr, pidx=pidx, tpos=tpos, err=err, ws=ws)


def bits(x):
    """uint32 values held in int64 -> their int32 bit patterns"""
    return (x - ((x >> 31) << 32)).to(torch.int32)


def check(res, probe, probe_ptr, qlist, out, out_ptr, pidx, tpos):
    """every query against ~torch.isin over its whole target list -> (verified, misses)"""
    pp, ql = probe_ptr.tolist(), qlist.long()
    la, lb_ = res.ptr[ql].tolist(), res.ptr[ql + 1].tolist()
    nq = ql.numel()
    # queries that name the same target in a row are checked as one: the definition is per value
    same = bool((ql == ql[0]).all().item())
    groups = [(0, nq)] if same else [(k, k + 1) for k in range(nq)]
    ok, at, miss_all = True, 0, []
    for k0, k1 in groups:
        a, b = pp[k0], pp[k1]
        pv = u32(probe[a:b])
        tgt = u32(res.flat[la[k0]: lb_[k0]])
        miss = ~torch.isin(pv, tgt)
        n = int(miss.sum().item())
        ok = ok and bool(torch.equal(u32(out[at: at + n]), pv[miss]))
        ok = ok and bool(torch.equal(u32(pidx[at: at + n]), a + torch.nonzero(miss).view(-1)))
        ok = ok and bool(torch.equal(u32(tpos[at: at + n]), torch.searchsorted(tgt, pv[miss])))
        miss_all.append(miss)
        at += n
    csum = torch.zeros(pp[-1] - pp[0] + 1, dtype=torch.int64, device=probe.device)
    csum[1:] = torch.cumsum(torch.cat(miss_all), 0)
    ok = ok and bool(torch.equal(out_ptr, csum[probe_ptr - pp[0]]))
    return ok, at


def measure(res, L, args, probe, probe_ptr, qlist, name):
    """one set of queries: the difference, the intersection on the same arguments, and the intersection plus torch"""
    dev, nq, pv = probe.device, qlist.numel(), probe.numel()
    new = lambda: torch.zeros(pv, dtype=torch.int32, device=dev)
    out, pidx, tpos, hit = new(), new(), new(), new()
    optr, hptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev), torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(L.tpf_lists_difference_workspace_size(nq, pv)), int(L.tpf_lists_intersect_workspace_size(nq, pv))),
                     dtype=torch.uint8, device=dev)
    difference(res, probe, probe_ptr, qlist, out, optr, pidx=pidx, tpos=tpos, err=err, ws=ws)
    ok, misses = check(res, probe, probe_ptr, qlist, out, optr, pidx, tpos)
    ok = ok and int(err.item()) == -1
    # (one untimed pass of both calls first: the leg's first timed call otherwise pays for clocks and caches that are still cold)
    lb.timed(lambda: (difference(res, probe, probe_ptr, qlist, out, optr, ws=ws), res.intersect(probe, probe_ptr, qlist, hit, hptr, ws=ws)),
             args.steps, args.warmup)
    t_df = lb.timed(lambda: difference(res, probe, probe_ptr, qlist, out, optr, ws=ws), args.steps, args.warmup)
    t_dfp = lb.timed(lambda: difference(res, probe, probe_ptr, qlist, out, optr, pidx=pidx, tpos=tpos, ws=ws), args.steps, args.warmup)
    t_ix = lb.timed(lambda: res.intersect(probe, probe_ptr, qlist, hit, hptr, ws=ws), args.steps, args.warmup)
    t_ixp = lb.timed(lambda: res.intersect(probe, probe_ptr, qlist, hit, hptr, pidx=pidx, tpos=tpos, ws=ws), args.steps, args.warmup)
    a0 = int(probe_ptr[0].item())
    got = {}

    def today():
        res.intersect(probe, probe_ptr, qlist, hit, hptr, pidx=pidx, ws=ws)
        mask = torch.zeros(pv, dtype=torch.bool, device=dev)
        mask[a0: int(probe_ptr[-1].item())] = True
        mask[pidx[: int(hptr[-1].item())].long()] = False
        got["out"] = probe[mask]
        csum = torch.zeros(pv + 1, dtype=torch.int64, device=dev)
        csum[1:] = torch.cumsum(mask, 0)
        got["ptr"] = csum[probe_ptr] - csum[a0]

    today()
    ok = ok and bool(torch.equal(got["out"], out[:misses])) and bool(torch.equal(got["ptr"], optr))
    t_today = lb.timed(today, args.steps, args.warmup)
    r = {"verified": ok, "queries": nq, "probe_values": int(probe_ptr[-1].item()) - a0, "misses": misses,
         "difference": t_df, "difference_with_pidx_and_tpos": t_dfp, "intersect_same_arguments": t_ix,
         "intersect_with_pidx_and_tpos": t_ixp, "intersect_pidx_plus_torch_mask_compaction_pointers": t_today,
         "workspace_bytes": int(L.tpf_lists_difference_workspace_size(nq, pv)),
         "ratio_difference_over_intersect_time": round(t_df["ms_median"] / t_ix["ms_median"], 4),
         "ratio_with_positions_over_intersect_with_positions_time": round(t_dfp["ms_median"] / t_ixp["ms_median"], 4),
         "ratio_difference_over_today_time": round(t_df["ms_median"] / t_today["ms_median"], 4)}
    print(f"[lists_difference_bench] {name}:", json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_difference_bench.json"))
    ap.add_argument("--legs", default="sparse,spread,tombstones,dense,chain", help="the legs to run (a per-kernel profile wants one at a time)")
    args = ap.parse_args()
    args.legs = args.legs.split(",")
    import turbopfor_amd as tpf

    dev = "cuda:0"
    L = tpf.lib()
    nb, nv = args.nblocks, args.nblocks * 256
    out = {"nblocks": nb, "values": nv, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "kernel_md5": tpf.kernel_md5(),
           "generator": f"scripts/lists_bench.py: bounded Zipf(s={lb.ZIPF_S}) on [1, {lb.ZIPF_MAX}] over bench_data.gen_c3(nblocks, seed=7)"}
    t0 = time.time()
    ok_all = True
    if {"sparse", "spread", "tombstones"} & set(args.legs):
        # ---- the index and the queries of scripts/lists_intersect_bench.py
        vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
        flat = vals.view(-1)
        ptr = lb.zipf_lengths(nv, 7, dev)
        nl = ptr.numel() - 1
        ln = ptr[1:] - ptr[:-1]
        out["lists"] = nl
        flatok = torch.ones(nl, dtype=torch.bool, device=dev)  # lists that hold no wrap (scripts/lists_intersect_bench.py)
        for a in range(0, nv - 1, bench_data.CHUNK):
            x = flat[a: min(a + bench_data.CHUNK + 1, nv)] ^ -(1 << 31)
            w = torch.nonzero(x[1:] < x[:-1]).view(-1) + a + 1
            j = torch.searchsorted(ptr, w, right=True) - 1
            flatok[j[w > ptr[j]]] = False
        res = Resident(tpf, flat, ptr)
        out["units"] = res.ix.nu
        rng = np.random.default_rng(11)
        probes, targets, _ = lxb.sparse_queries(flat, ptr, flatok, rng)
        nq = len(probes)
        psel = torch.tensor(probes, dtype=torch.int32, device=dev)
        qlist = torch.tensor(targets, dtype=torch.int32, device=dev)
        probe = torch.zeros(int(ln[psel.long()].sum().item()), dtype=torch.int32, device=dev)
        pptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        res.ix.select(psel, probe, pptr)
        ok_all = ok_all and nq == lxb.NQ
        # ---- (a) sparse
        if "sparse" in args.legs:
            out["sparse"] = measure(res, L, args, probe, pptr, qlist, "sparse")
            ok_all = ok_all and out["sparse"]["verified"]
        # ---- (a') spread: 128 values over the whole of every target
        n_t = ln[qlist.long()]
        pos = (torch.arange(64, device=dev, dtype=torch.float64)[None, :] + 0.5) / 64.0 * n_t[:, None].to(torch.float64)
        members = u32(flat[ptr[qlist.long()][:, None] + pos.to(torch.int64)])
        probe2 = bits(torch.stack([members, torch.clamp(members + 1, max=0xFFFFFFFF)], dim=2).reshape(-1))
        pptr2 = torch.arange(nq + 1, dtype=torch.int64, device=dev) * 128
        if "spread" in args.legs:
            out["spread"] = measure(res, L, args, probe2, pptr2, qlist, "spread")
            ok_all = ok_all and out["spread"]["verified"]
        # ---- (c) tombstones: the result of (a')'s intersection minus one long list of deleted ids
        if "tombstones" in args.legs:
            result, rptr = res.intersect(probe2, pptr2, qlist, torch.zeros_like(probe2), torch.zeros(nq + 1, dtype=torch.int64, device=dev))
            dead = torch.unique(u32(flat[::100]))  # about 1 % of the index's values, ascending
            dead = bits(dead[dead > 0])
            tres = Resident(tpf, dead, torch.tensor([0, dead.numel()], dtype=torch.int64, device=dev))
            r = measure(tres, L, args, result, rptr, torch.zeros(nq, dtype=torch.int32, device=dev), "tombstones")
            r["tombstones"] = int(dead.numel())
            r["deleted_from_the_result"] = r["probe_values"] - r["misses"]
            out["tombstones"] = r
            ok_all = ok_all and r["verified"] and 0 < r["deleted_from_the_result"] < r["probe_values"]
            del tres, dead, result
        del res, probe, probe2, vals, flat
    if "dense" not in args.legs and "chain" not in args.legs:
        return finish(out, args, t0, ok_all)

    # ---- (b), (d): the three lists over one universe of scripts/lists_intersect_bench.py, an index of their own
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    universe = torch.unique(torch.randint(1, 1 << 31, (1 << 22,), generator=g, device=dev, dtype=torch.int64))
    lists = [universe[torch.rand(universe.numel(), generator=g, device=dev) < 0.5] for _ in range(3)]
    dflat = torch.cat(lists).to(torch.int32)
    dptr = torch.tensor(np.concatenate([[0], np.cumsum([v.numel() for v in lists])]), dtype=torch.int64, device=dev)
    dres = Resident(tpf, dflat, dptr)
    n0 = lists[0].numel()
    probe = dflat[:n0].clone()
    pptr = torch.tensor([0, n0], dtype=torch.int64, device=dev)
    q1 = torch.tensor([1], dtype=torch.int32, device=dev)
    q2 = torch.tensor([2], dtype=torch.int32, device=dev)
    if "dense" in args.legs:
        r = measure(dres, L, args, probe, pptr, q1, "dense")
        r["target_values"] = lists[1].numel()
        r["difference_G_probe_values_s"] = lb.rate(n0, r["difference"])
        out["dense"] = r
        ok_all = ok_all and r["verified"]
    if "chain" in args.legs:
        err = torch.zeros(2, dtype=torch.int64, device=dev)
        ws = torch.empty(max(int(L.tpf_lists_intersect_workspace_size(1, n0)), int(L.tpf_lists_difference_workspace_size(1, n0))),
                         dtype=torch.uint8, device=dev)
        out1, ptr1 = torch.zeros(n0, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        out2, ptr2 = torch.zeros(n0, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)

        def chain(second, e1=None, e2=None):
            dres.intersect(probe, pptr, q1, out1, ptr1, err=e1, ws=ws)
            second(dres, out1, ptr1, q2, out2, ptr2, err=e2, ws=ws)  # the output of the first call is the probe of the second

        chain(difference, err[0:1], err[1:2])
        ab = lists[0][torch.isin(lists[0], lists[1])]
        want = ab[~torch.isin(ab, lists[2])]
        okc = err.tolist() == [-1, -1] and int(ptr2[1].item()) == want.numel() and bool(torch.equal(u32(out2[: want.numel()]), want))
        okc = okc and 0 < want.numel() < ab.numel()
        t_chain = lb.timed(lambda: chain(difference), args.steps, args.warmup)
        t_and3 = lb.timed(lambda: chain(lambda r, *a, **k: r.intersect(*a, **k)), args.steps, args.warmup)
        out["chain"] = {"verified": okc, "list_values": [v.numel() for v in lists], "after_a_and_b": int(ab.numel()),
                        "after_and_not_c": int(want.numel()), "intersect_then_difference": t_chain, "intersect_then_intersect": t_and3,
                        "ratio_over_the_3_term_and_time": round(t_chain["ms_median"] / t_and3["ms_median"], 4)}
        ok_all = ok_all and okc
        print("[lists_difference_bench] chain:", json.dumps(out["chain"]), flush=True)
    return finish(out, args, t0, ok_all)


if __name__ == "__main__":
    sys.exit(main())
