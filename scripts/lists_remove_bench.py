#!/usr/bin/env python
"""Measurement of the delete from a resident index (tpf_lists_remove); recorded
in profiles/lists_remove_bench.json, not gated.  Timed the way
scripts/lists_append_bench.py times: warm-up, HIP events around every call on
the launch stream, median over the steps; the calls of a leg alternate step by
step.  All legs in one process on one box.  The index is
scripts/lists_bench.py's Zipf(1.5) delta-1 index (2.5M lists at the default
size) with its skip table.  Every result is checked at full size on the device
against the rebuild: bytes, offsets, both directories and the table.

(a) spread: 1 % of the values, from the lists in proportion to their length,
    evenly spaced inside each list.
(b) hot: the same count (as far as the lists hold it) from the 4,096 longest lists.
(c) ones: 10,000 one-value lists, emptied.
(d) end: one value near the end of each of the 4,096 longest lists.
(e) start: one value near the start of each of the same lists.

Each leg is held against
  - the rebuild, what the library offered before: tpf_p4ndec256v32_lists of the
    whole index, a torch mask and compaction, tpf_p4nenc256v32_lists of
    everything, tpf_lists_unit_base and tpf_lists_unit_last, buffers allocated
    beforehand;
  - tpf_copy_async of in_bytes, the floor of the stitch pass;
  - tpf_lists_append of the same number of values to the same lists.

    python scripts/lists_remove_bench.py [--nblocks N] [--steps K] [--warmup W] [--legs spread,hot,ones,end,start]
        [--no-rebuild-timing] [--kernel-stats CSV] [--out FILE]

--kernel-stats merges the per-kernel rows of a `rocprofv3 --kernel-trace
--stats` run of this script (one leg, --no-rebuild-timing) into the JSON.
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "turbopfor-cpp_amd", "python"))

import bench_data  # noqa: E402
import lists_bench as lb  # noqa: E402
import lists_intersect_bench as lxb  # noqa: E402
from lists_append_bench import additions, csr  # noqa: E402
from lists_gather_bench import timed_alternately  # noqa: E402
from lists_select_bench import Index  # noqa: E402

HOT_LISTS = 4096
ONE_LISTS = 10_000
LEGS = ("spread", "hot", "ones", "end", "start")
STAGE_MAX = 0x7FFFFFFF  # stage_values of one call


def spaced(ln, counts):
    """counts[j] positions of list j, evenly spaced from 0: floor(k n_j / c_j) -> (qlist int32, pos int32, pos_ptr) over the lists
    that lose something"""
    q = torch.nonzero(counts > 0).view(-1)
    c, n = counts[q], ln[q]
    pptr = csr(c)
    k = torch.arange(int(pptr[-1].item()), dtype=torch.int64, device=ln.device) - torch.repeat_interleave(pptr[:-1], c)
    pos = k * torch.repeat_interleave(n, c) // torch.repeat_interleave(c, c)
    return q.to(torch.int32), pos.to(torch.int32), pptr


class Rebuild:
    """decode everything, mask and compact with torch, encode everything, rebuild both tables"""

    def __init__(self, tpf, ix, qlist, pos, pptr):
        self.tpf, self.ix = tpf, ix
        dev, nl = pos.device, ix.nl
        self.nv = int(ix.ptr[-1].item())
        c = torch.zeros(nl, dtype=torch.int64, device=dev)
        c[qlist.long()] = pptr[1:] - pptr[:-1]
        self.nptr = ix.ptr - csr(c)  # known on the host side of a real caller too: lengths only
        self.total = int(self.nptr[-1].item())
        self.nunits = int(tpf.lists_units(self.nptr.cpu())[1][-1])
        self.gone = ix.ptr[torch.repeat_interleave(qlist.long(), pptr[1:] - pptr[:-1])] + pos.long()
        # where every chunk of the old values lands: the values before it minus the removed ones among them (host side, once)
        cuts = list(range(0, self.nv, bench_data.CHUNK)) + [self.nv]
        lost = torch.searchsorted(torch.sort(self.gone)[0], torch.tensor(cuts, dtype=torch.int64, device=dev)).tolist()
        self.chunks = [(a, b, a - la, b - lb) for a, b, la, lb in zip(cuts[:-1], cuts[1:], lost[:-1], lost[1:])]
        self.dec = torch.empty(self.nv, dtype=torch.int32, device=dev)
        self.mask = torch.empty(self.nv, dtype=torch.bool, device=dev)
        self.flat = torch.empty(self.total, dtype=torch.int32, device=dev)
        self.out = torch.empty(tpf.lists_enc_bound(max(self.total, 1), nl), dtype=torch.uint8, device=dev)
        self.offs = torch.empty(self.nunits + 1, dtype=torch.int64, device=dev)
        self.unit = torch.empty(nl + 1, dtype=torch.int32, device=dev)
        self.table = torch.empty(max(self.nunits, 1), dtype=torch.int32, device=dev)
        L = tpf.lib()
        self.ws = torch.empty(max(int(L.tpf_p4nenc256v32_lists_workspace_size(self.nunits, nl)),
                                  int(L.tpf_p4ndec256v32_lists_workspace_size(ix.nu, nl)),
                                  int(L.tpf_lists_unit_last_workspace_size(self.nunits, nl))), dtype=torch.uint8, device=dev)

    def run(self, err=None):
        tpf, ix = self.tpf, self.ix
        tpf.decn256v32_lists(ix.packed, ix.offs, ix.ptr, d1=True, start0=ix.start0, out=self.dec, err=err, ws=self.ws)
        self.mask.fill_(True)
        self.mask[self.gone] = False
        for a, b, oa, ob in self.chunks:  # in chunks: the compaction's index arithmetic stays below 2^31
            torch.masked_select(self.dec[a:b], self.mask[a:b], out=self.flat[oa:ob])
        tpf.encn256v32_lists(self.flat, self.nptr, d1=True, start0=ix.start0, nunits=self.nunits, out=self.out, offsets=self.offs, err=err,
                             ws=self.ws)
        tpf.lists_unit_base(self.nptr, out=self.unit, ws=self.ws)
        tpf.lists_unit_last(self.out, self.offs, self.nptr, start0=ix.start0, out=self.table, err=err, ws=self.ws)


def leg(tpf, L, ix, table, flat, qlist, pos, pptr, seed, args):
    dev = flat.device
    ln = ix.ptr[1:] - ix.ptr[:-1]
    nq, npos = qlist.numel(), pos.numel()
    in_bytes = ix.packed.numel()
    u0 = (pos[pptr[:-1].clamp(max=max(npos - 1, 0))].long() >> 8) if npos else torch.zeros(nq, dtype=torch.int64, device=dev)
    per = torch.where(pptr[1:] > pptr[:-1], ln[qlist.long()] - 256 * u0, torch.zeros_like(u0))
    wanted = {"queries": nq, "removed_values": npos, "staged_values": int(per.sum().item())}
    if wanted["staged_values"] > STAGE_MAX:
        # one call stages at most 0x7FFFFFFF values: the leg keeps the queries, in list order, whose suffixes fit
        nq = int((torch.cumsum(per, 0) <= STAGE_MAX).sum().item())
        qlist, pptr, per = qlist[:nq], pptr[: nq + 1].clone(), per[:nq]
        pos = pos[: int(pptr[-1].item())]
        npos = pos.numel()
    staged = int(per.sum().item())
    out_cap = tpf.lists_remove_bound(in_bytes, nq, staged)
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    out_offs = torch.empty(ix.nu + 1, dtype=torch.int64, device=dev)
    ws_bytes = int(L.tpf_lists_remove_workspace_size(ix.nu, ix.nl, nq, npos, staged))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    res = {}

    def remove(e=None):
        res["r"] = tpf.lists_remove(ix.packed, ix.offs, ix.ptr, ix.unit, pos, pptr, qlist, staged, d1=True, start0=ix.start0,
                                    unit_last=table, out=out, out_offsets=out_offs, units_cap=ix.nu, err=e, ws=ws)

    remove(err)
    ok = int(err.item()) == -1
    rb = Rebuild(tpf, ix, qlist, pos, pptr)
    rerr = torch.zeros(1, dtype=torch.int64, device=dev)
    rb.run(rerr)
    ok = ok and int(rerr.item()) == -1
    o, oo, lp, lu, ul = res["r"]
    nu = rb.nunits
    nbytes = int(rb.offs[-1].item())
    ok = ok and bool(torch.equal(lp, rb.nptr)) and bool(torch.equal(lu, rb.unit)) and bool(torch.equal(oo[: nu + 1], rb.offs))
    ok = ok and bool(torch.equal(o[:nbytes], rb.out[:nbytes])) and bool(torch.equal(ul[:nu], rb.table[:nu]))
    copy_dst = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src_p, dst_p = ctypes.c_void_p(ix.packed.data_ptr()), ctypes.c_void_p(copy_dst.data_ptr())

    def copy():
        assert L.tpf_copy_async(dst_p, src_p, in_bytes, stream) == 0

    # the append of as many values to the same lists
    counts = torch.zeros(ix.nl, dtype=torch.int64, device=dev)
    counts[qlist.long()] = pptr[1:] - pptr[:-1]
    add, aptr, st_out = additions(flat, ix.ptr, ix.start0, counts, seed)
    a_out = torch.empty(tpf.lists_append_bound(in_bytes, ix.nl, npos), dtype=torch.uint8, device=dev)
    a_cap = tpf.lists_append_units_bound(ix.nu, ix.nl, npos)
    a_offs = torch.empty(a_cap + 1, dtype=torch.int64, device=dev)
    a_ws = torch.empty(int(L.tpf_lists_append_workspace_size(ix.nu, ix.nl, npos)), dtype=torch.uint8, device=dev)

    def append():
        tpf.lists_append(ix.packed, ix.offs, ix.ptr, ix.unit, add, aptr, d1=True, start0=st_out, unit_last=table, out=a_out,
                         out_offsets=a_offs, units_cap=a_cap, ws=a_ws)

    fns = [remove, copy, append] + ([] if args.no_rebuild_timing else [rb.run])
    ts = timed_alternately(fns, args.steps, args.warmup)
    r = {"verified": ok, "cut_to_fit_stage_values": wanted if wanted["queries"] != nq else None, "queries": nq, "removed_values": npos, "staged_values": staged, "in_bytes": in_bytes, "out_bytes": nbytes,
         "units_out": nu, "remove_workspace_bytes": ws_bytes, "out_cap": out_cap, "remove": ts[0], "copy_of_in_bytes": ts[1],
         "append_of_as_many": ts[2],
         "ratio_remove_over_copy_time": round(ts[0]["ms_median"] / ts[1]["ms_median"], 3),
         "ratio_remove_over_append_time": round(ts[0]["ms_median"] / ts[2]["ms_median"], 3),
         "copy_GB_s": round(in_bytes / (ts[1]["ms_median"] * 1e-3) / 1e9, 1)}
    if not args.no_rebuild_timing:
        r["rebuild"] = ts[3]
        r["ratio_rebuild_over_remove_time"] = round(ts[3]["ms_median"] / ts[0]["ms_median"], 2)
    return r


def kernel_stats(path):
    rows = []
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if any(s in name for s in ("k_rem_", "k_un_", "k_sel_heads", "k_lenc_", "k_run_scan", "k_copy16", "k_app_")):
                rows.append({"kernel": name.split("(")[0], "calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--no-rebuild-timing", action="store_true", help="time the remove, the copy and the append only (profiling runs)")
    ap.add_argument("--kernel-stats", default=None, help="merge a rocprofv3 kernel stats CSV into the JSON instead of measuring")
    ap.add_argument("--kernel-stats-leg", default="spread")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_remove_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as fh:
            out = json.load(fh)
        out["kernels_" + args.kernel_stats_leg] = kernel_stats(args.kernel_stats)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        return 0
    args.legs = args.legs.split(",")
    import turbopfor_amd as tpf

    dev = "cuda:0"
    L = tpf.lib()
    nb, nv = args.nblocks, args.nblocks * 256
    out = {"nblocks": nb, "values": nv, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "boxes": 1,
           "kernel_md5": tpf.kernel_md5(), "stitch_tile_bytes": tpf.LISTS_APPEND_TILE,
           "generator": f"scripts/lists_bench.py: bounded Zipf(s={lb.ZIPF_S}) on [1, {lb.ZIPF_MAX}] over bench_data.gen_c3(nblocks, seed=7); "
                        "removals: scripts/lists_remove_bench.py"}
    t0 = time.time()
    vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
    flat = vals.view(-1)
    ptr = lb.zipf_lengths(nv, 7, dev)
    nl = ptr.numel() - 1
    ln = ptr[1:] - ptr[:-1]
    ix = Index(tpf, flat, ptr, True)
    table = tpf.lists_unit_last(ix.packed, ix.offs, ptr, start0=ix.start0)
    out["lists"], out["units"], out["in_bytes"] = nl, ix.nu, ix.packed.numel()
    nrem = nv // 100
    longest = torch.sort(torch.argsort(ln, descending=True)[:HOT_LISTS])[0]
    zeros = lambda: torch.zeros(nl, dtype=torch.int64, device=dev)
    if "spread" in args.legs:
        # in proportion to the lengths: floor(n_j / 100), the rest one each to the longest lists
        counts = ln // 100
        rest = nrem - int(counts.sum().item())
        counts[torch.argsort(ln, descending=True)[:rest]] += 1
        out["spread"] = leg(tpf, L, ix, table, flat, *spaced(ln, torch.minimum(counts, ln)), 41, args)
    if "hot" in args.legs:
        counts = zeros()
        share = ln[longest] * nrem // int(ln[longest].sum().item())
        counts[longest] = torch.minimum(share, ln[longest])
        out["hot"] = leg(tpf, L, ix, table, flat, *spaced(ln, counts), 45, args)
    if "ones" in args.legs:
        counts = zeros()
        counts[torch.nonzero(ln == 1).view(-1)[:ONE_LISTS]] = 1
        out["ones"] = leg(tpf, L, ix, table, flat, *spaced(ln, counts), 47, args)
    for name, at in (("end", lambda n: n - 2), ("start", lambda n: torch.ones_like(n))):
        if name in args.legs:
            n = ln[longest]
            assert int(n.min().item()) >= 3
            out[name] = leg(tpf, L, ix, table, flat, longest.to(torch.int32), at(n).to(torch.int32), csr(torch.ones_like(n)), 49, args)
    ok_all = True
    for k in LEGS:
        if k in out:
            ok_all = ok_all and out[k]["verified"]
            print(f"[lists_remove_bench] {k}:", json.dumps(out[k]), flush=True)
    return lxb.finish(out, args, t0, ok_all)


if __name__ == "__main__":
    sys.exit(main())
