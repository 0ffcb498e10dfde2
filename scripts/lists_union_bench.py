#!/usr/bin/env python
"""Measurement of the union with a resident index (tpf_lists_union); recorded
in profiles/lists_union_bench.json, not gated.  Timed the way bench.py times
its steps (scripts/lists_bench.py's `timed`): warm-up, HIP events around every
call on the launch stream, median over the steps.  All legs in one process on
one box.  Only lists that ascend without wrapping mod 2^32 are used, and every
result is checked at full size on the device against torch.unique before it is
timed.

(a) short: 4,096 queries on the Zipf(1.5) delta-1 index of
    scripts/lists_select_bench.py.  Each probe is a list of 64 to 256 values
    (128 on average), decoded with the selective decode; each target is a list
    of 16 to 64 units.
(b) dense: three lists of about 2.09M values drawn from one universe of 4M doc
    ids (scripts/lists_intersect_bench.py's), in an index of their own: one
    whole list OR another.
(c) or3: a 3-term OR over those three lists, two calls chained on the device.

Each against
  today: what a caller does without the entry point -- the selective decode of
    the targets, then torch.unique (a sort) of (query << 32 | value) keys over
    the decoded targets and the probe laid end to end, the query of every value
    from torch.repeat_interleave with a known output size (no synchronisation);
  floor: tpf_p4ndec256v32_lists_units over the same whole targets plus a device
    copy of the probe: every answer reads and writes at least that.

    python scripts/lists_union_bench.py [--nblocks N] [--steps K] [--warmup W] [--legs short,dense,or3] [--out FILE]

--legs runs a subset (the committed JSON holds all three): a rocprofv3
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
from lists_intersect_bench import Resident, finish, u32  # noqa: E402

NQ = 4096


def union(res, probe, probe_ptr, qlist, out, out_ptr, pidx=None, tpos=None, err=None, ws=None):
    ix = res.ix
    return res.tpf.lists_union(ix.packed, ix.offs, ix.ptr, ix.unit, res.table, probe, probe_ptr, qlist, start0=ix.start0, out=out,
                               out_ptr=out_ptr, pidx=pidx, tpos=tpos, err=err, ws=ws)


def keys_of(values, lens, total):
    """(query << 32) | value for values laid end to end in segments of `lens`"""
    q = torch.repeat_interleave(torch.arange(lens.numel(), device=values.device), lens, output_size=total)
    return (q << 32) | u32(values)


def measure(res, L, args, probe, probe_ptr, qlist, name):
    """one set of queries: the union, what a caller does today, and the floor"""
    tpf, dev, nq = res.tpf, probe.device, qlist.numel()
    ql = qlist.long()
    tlen = res.ptr[ql + 1] - res.ptr[ql]
    plen = probe_ptr[1:] - probe_ptr[:-1]
    tv, pv = int(tlen.sum().item()), probe.numel()
    cap = tv + pv
    out = torch.zeros(cap, dtype=torch.int32, device=dev)
    pidx = torch.zeros(cap, dtype=torch.int32, device=dev)
    tpos = torch.zeros(cap, dtype=torch.int32, device=dev)
    optr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.tpf_lists_union_workspace_size(nq, pv, cap)), dtype=torch.uint8, device=dev)
    union(res, probe, probe_ptr, qlist, out, optr, pidx=pidx, tpos=tpos, err=err[0:1], ws=ws)
    # ---- today: decode the targets, sort the keys
    dec = torch.zeros(tv, dtype=torch.int32, device=dev)
    dptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    sws = torch.empty(int(L.tpf_p4ndec256v32_lists_select_workspace_size(nq, tv)), dtype=torch.uint8, device=dev)

    def today(e=None):
        res.ix.select(qlist, dec, dptr, err=e, ws=sws)
        k = torch.cat([keys_of(dec, tlen, tv), keys_of(probe, plen, pv)])
        return torch.unique(k)  # sorted; its size comes back to the host, as the caller's allocation needs it

    want = today(err[1:2])
    total = want.numel()
    ok = err.tolist() == [-1, -1] and int(optr[-1].item()) == total and bool(torch.equal(u32(out[:total]), want & 0xFFFFFFFF))
    bounds = torch.searchsorted(want, torch.arange(nq + 1, device=dev) << 32)
    ok = ok and bool(torch.equal(optr, bounds))
    # provenance: every value the list holds sits at its position, every value of the probe at its index
    fl, fp = u32(tpos[:total]) != 0xFFFFFFFF, u32(pidx[:total]) != 0xFFFFFFFF
    ok = ok and int(fl.sum().item()) == tv and int(fp.sum().item()) == pv
    ok = ok and bool(torch.equal(u32(probe)[u32(pidx[:total])[fp]], u32(out[:total])[fp]))
    t_un = lb.timed(lambda: union(res, probe, probe_ptr, qlist, out, optr, pidx=pidx, tpos=tpos, ws=ws), args.steps, args.warmup)
    t_un_values = lb.timed(lambda: union(res, probe, probe_ptr, qlist, out, optr, ws=ws), args.steps, args.warmup)
    t_today = lb.timed(today, args.steps, args.warmup)
    # ---- the floor: the whole targets decoded to memory, the probe copied
    uf = torch.zeros(nq, dtype=torch.int32, device=dev)
    uc = ((tlen + 255) // 256).to(torch.int32)
    bptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    bws = torch.empty(int(L.tpf_p4ndec256v32_lists_units_workspace_size(nq, tv)), dtype=torch.uint8, device=dev)
    pcopy = torch.zeros(pv, dtype=torch.int32, device=dev)

    def floor(e=None):
        res.units(qlist, uf, uc, dec, bptr, err=e, ws=bws)
        pcopy.copy_(probe)

    floor(err[0:1])
    ok = ok and int(err[0].item()) == -1 and int(bptr[-1].item()) == tv
    t_floor = lb.timed(floor, args.steps, args.warmup)
    r = {"verified": ok, "queries": nq, "probe_values": pv, "target_values": tv, "union_values": total, "common_values": tv + pv - total,
         "union": t_un, "union_values_only": t_un_values, "select_decode_plus_torch_unique": t_today,
         "units_decode_plus_probe_copy": t_floor, "union_workspace_bytes": ws.numel(), "union_G_values_out_s": lb.rate(total, t_un),
         "ratio_union_over_today_time": round(t_un["ms_median"] / t_today["ms_median"], 4),
         "ratio_union_over_floor_time": round(t_un["ms_median"] / t_floor["ms_median"], 4)}
    print(f"[lists_union_bench] {name}:", json.dumps(r), flush=True)
    return r, out, optr, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_union_bench.json"))
    ap.add_argument("--legs", default="short,dense,or3", help="the legs to run (a per-kernel profile wants one at a time)")
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
    if "short" in args.legs:
        vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
        flat = vals.view(-1)
        ptr = lb.zipf_lengths(nv, 7, dev)
        nl = ptr.numel() - 1
        ln = ptr[1:] - ptr[:-1]
        out["lists"] = nl
        # lists that hold no wrap of the one sorted list they are cut from (scripts/lists_range_bench.py)
        flatok = torch.ones(nl, dtype=torch.bool, device=dev)
        for a in range(0, nv - 1, bench_data.CHUNK):
            x = flat[a: min(a + bench_data.CHUNK + 1, nv)] ^ -(1 << 31)
            w = torch.nonzero(x[1:] < x[:-1]).view(-1) + a + 1
            j = torch.searchsorted(ptr, w, right=True) - 1
            flatok[j[w > ptr[j]]] = False
        res = Resident(tpf, flat, ptr)
        out["units"] = res.ix.nu
        rng = np.random.default_rng(11)
        short_ids = torch.nonzero(flatok & (ln >= 64) & (ln <= 256)).view(-1).cpu().numpy()
        long_ids = torch.nonzero(flatok & (ln >= 256 * 16) & (ln <= 256 * 64)).view(-1).cpu().numpy()
        psel = torch.tensor(short_ids[rng.permutation(len(short_ids))[:NQ]], dtype=torch.int32, device=dev)
        qlist = torch.tensor(long_ids[rng.integers(0, len(long_ids), size=NQ)], dtype=torch.int32, device=dev)
        total = int(ln[psel.long()].sum().item())
        probe = torch.zeros(total, dtype=torch.int32, device=dev)
        pptr = torch.zeros(NQ + 1, dtype=torch.int64, device=dev)
        res.ix.select(psel, probe, pptr)
        r, _, _, _ = measure(res, L, args, probe, pptr, qlist, "short")
        r["lists_of_16_to_64_units"] = int(len(long_ids))
        r["distinct_targets"] = int(torch.unique(qlist).numel())
        r["mean_probe_values"] = round(total / NQ, 1)
        out["short"] = r
        ok_all = ok_all and r["verified"] and psel.numel() == NQ
        del res, probe, vals, flat
    if "dense" not in args.legs and "or3" not in args.legs:
        return finish(out, args, t0, ok_all)

    # ---- (b), (c): three lists over one universe, an index of their own
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
    r, out1, ptr1, n01 = measure(dres, L, args, probe, pptr, q1, "dense")
    r["bytes_per_int"] = round(dres.ix.packed.numel() / dflat.numel(), 4)
    out["dense"] = r
    ok_all = ok_all and r["verified"]
    if "or3" in args.legs:
        n2 = lists[2].numel()
        cap2 = out1.numel() + n2
        out2, ptr2 = torch.zeros(cap2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        err = torch.zeros(2, dtype=torch.int64, device=dev)
        ws = torch.empty(max(int(L.tpf_lists_union_workspace_size(1, n0, out1.numel())),
                             int(L.tpf_lists_union_workspace_size(1, out1.numel(), cap2))), dtype=torch.uint8, device=dev)

        def chain(e1=None, e2=None):
            union(dres, probe, pptr, q1, out1, ptr1, err=e1, ws=ws)
            union(dres, out1, ptr1, q2, out2, ptr2, err=e2, ws=ws)  # the output of the first call is the probe of the second

        chain(err[0:1], err[1:2])
        want = torch.unique(torch.cat(lists))
        okc = err.tolist() == [-1, -1] and int(ptr2[1].item()) == want.numel() and bool(torch.equal(u32(out2[: want.numel()]), want))
        t_chain = lb.timed(chain, args.steps, args.warmup)
        t_today = lb.timed(lambda: torch.unique(torch.cat([u32(dflat)])), args.steps, args.warmup)
        out["or3"] = {"verified": okc, "list_values": [v.numel() for v in lists], "values_after_two_terms": n01,
                      "union_values": int(want.numel()), "two_chained_calls": t_chain,
                      "torch_unique_of_the_three_decoded_lists": t_today,
                      "ratio_chain_over_torch_unique_time": round(t_chain["ms_median"] / t_today["ms_median"], 4)}
        ok_all = ok_all and okc
        print("[lists_union_bench] or3:", json.dumps(out["or3"]), flush=True)
    return finish(out, args, t0, ok_all)


if __name__ == "__main__":
    sys.exit(main())
