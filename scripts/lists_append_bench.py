#!/usr/bin/env python
"""Measurement of the append to a resident index (tpf_lists_append); recorded
in profiles/lists_append_bench.json, not gated.  Timed the way
scripts/lists_gather_bench.py times: warm-up, HIP events around every call on
the launch stream, median over the steps; the calls of a leg alternate step by
step.  All legs in one process on one box.  The index is
scripts/lists_bench.py's Zipf(1.5) delta-1 index (2.5M lists at the default
size) with its skip table.  Every result is checked at full size on the device
against the rebuild: bytes, offsets, both directories and the table.

(a) spread: 1 % more values, spread over the lists in proportion to their length.
(b) hot: the same number of values given to 4,096 lists.
(c) new: 10,000 new one-value lists.

Each leg is held against
  - the rebuild, what the library offered before: tpf_p4ndec256v32_lists of the
    whole index, the torch interleave of old and new values,
    tpf_p4nenc256v32_lists of everything, tpf_lists_unit_base and
    tpf_lists_unit_last;
  - tpf_copy_async of in_bytes, the floor of the stitch pass.

    python scripts/lists_append_bench.py [--nblocks N] [--steps K] [--warmup W] [--legs spread,hot,new] [--no-rebuild-timing]
        [--kernel-stats CSV] [--out FILE]

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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "turbopfor-cpp_amd", "python"))

import bench_data  # noqa: E402
import lists_bench as lb  # noqa: E402
import lists_intersect_bench as lxb  # noqa: E402
from lists_gather_bench import timed_alternately  # noqa: E402
from lists_select_bench import Index  # noqa: E402

HOT_LISTS = 4096
NEW_LISTS = 10_000


def csr(counts):
    p = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    p[1:] = torch.cumsum(counts, 0)
    return p


def additions(flat, ptr, start0, counts, seed):
    """counts[j] values for list j (lists past the old index are new and start from 0): ascending past the list's last value,
    gaps 1 .. 2^10, mod 2^32 -> (add int32, add_ptr, start0 of the result's lists)"""
    dev, nl, nout = flat.device, ptr.numel() - 1, counts.numel()
    aptr = csr(counts)
    n = int(aptr[-1].item())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    gaps = torch.randint(1, 1 << 10, (n,), generator=g, device=dev, dtype=torch.int64)
    c = torch.cumsum(gaps, 0)
    ln = ptr[1:] - ptr[:-1]
    st = torch.zeros(nout, dtype=torch.int64, device=dev)
    st[:nl] = start0.to(torch.int64) & 0xFFFFFFFF
    last = torch.where(ln > 0, flat[torch.clamp(ptr[1:] - 1, min=0)].to(torch.int64) & 0xFFFFFFFF, st[:nl])
    base = st.clone()
    base[:nl] = last
    j = torch.repeat_interleave(torch.arange(nout, device=dev), counts)
    before = torch.where(aptr[:-1] > 0, c[torch.clamp(aptr[:-1] - 1, min=0)], torch.zeros_like(aptr[:-1]))
    v = (base[j] + c - before[j]) & 0xFFFFFFFF
    st32 = torch.where(st >= (1 << 31), st - (1 << 32), st).to(torch.int32)
    return torch.where(v >= (1 << 31), v - (1 << 32), v).to(torch.int32), aptr, st32


class Rebuild:
    """decode everything, interleave with torch, encode everything, rebuild both tables"""

    def __init__(self, tpf, ix, table, add, aptr, st_out):
        self.tpf, self.ix, self.add, self.aptr, self.st = tpf, ix, add, aptr, st_out
        dev, nl, nout = add.device, ix.nl, aptr.numel() - 1
        self.nv = int(ix.ptr[-1].item())
        oldoff = torch.full((nout + 1,), self.nv, dtype=torch.int64, device=dev)
        oldoff[: nl + 1] = ix.ptr
        self.nptr = oldoff + aptr  # known on the host side of a real caller too: lengths only
        self.oldoff = oldoff
        self.total = int(self.nptr[-1].item())
        self.nunits = int(tpf.lists_units(self.nptr.cpu())[1][-1])
        self.dec = torch.empty(self.nv, dtype=torch.int32, device=dev)
        self.flat = torch.empty(self.total, dtype=torch.int32, device=dev)
        self.out = torch.empty(tpf.lists_enc_bound(self.total, nout), dtype=torch.uint8, device=dev)
        self.offs = torch.empty(self.nunits + 1, dtype=torch.int64, device=dev)
        self.unit = torch.empty(nout + 1, dtype=torch.int32, device=dev)
        self.table = torch.empty(self.nunits, dtype=torch.int32, device=dev)
        L = tpf.lib()
        self.ws = torch.empty(max(int(L.tpf_p4nenc256v32_lists_workspace_size(self.nunits, nout)),
                                  int(L.tpf_p4ndec256v32_lists_workspace_size(ix.nu, nl)),
                                  int(L.tpf_lists_unit_last_workspace_size(self.nunits, nout))), dtype=torch.uint8, device=dev)

    def interleave(self):
        """new[nptr[j] + k] = old[ptr[j] + k]; new[nptr[j] + n_j + k] = add[aptr[j] + k] -- in chunks, int64 index arithmetic"""
        ix = self.ix
        for a in range(0, self.nv, bench_data.CHUNK):
            i = torch.arange(a, min(a + bench_data.CHUNK, self.nv), dtype=torch.int64, device=self.dec.device)
            j = torch.searchsorted(ix.ptr, i, right=True) - 1
            self.flat[i + self.aptr[j]] = self.dec[i]
        na = self.add.numel()
        for a in range(0, na, bench_data.CHUNK):
            i = torch.arange(a, min(a + bench_data.CHUNK, na), dtype=torch.int64, device=self.dec.device)
            j = torch.searchsorted(self.aptr, i, right=True) - 1
            self.flat[i + self.oldoff[j + 1]] = self.add[i]

    def run(self, err=None):
        tpf, ix = self.tpf, self.ix
        tpf.decn256v32_lists(ix.packed, ix.offs, ix.ptr, d1=True, start0=ix.start0, out=self.dec, err=err, ws=self.ws)
        self.interleave()
        tpf.encn256v32_lists(self.flat, self.nptr, d1=True, start0=self.st, nunits=self.nunits, out=self.out, offsets=self.offs, err=err,
                             ws=self.ws)
        tpf.lists_unit_base(self.nptr, out=self.unit, ws=self.ws)
        tpf.lists_unit_last(self.out, self.offs, self.nptr, start0=self.st, out=self.table, err=err, ws=self.ws)


def leg(tpf, L, ix, table, flat, counts, seed, args):
    dev = flat.device
    add, aptr, st_out = additions(flat, ix.ptr, ix.start0, counts, seed)
    nout, nadd = counts.numel(), add.numel()
    in_bytes = ix.packed.numel()
    out_cap = tpf.lists_append_bound(in_bytes, nout, nadd)
    units_cap = tpf.lists_append_units_bound(ix.nu, nout, nadd)
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    out_offs = torch.empty(units_cap + 1, dtype=torch.int64, device=dev)
    ws_bytes = int(L.tpf_lists_append_workspace_size(ix.nu, nout, nadd))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    res = {}

    def append(e=None):
        res["r"] = tpf.lists_append(ix.packed, ix.offs, ix.ptr, ix.unit, add, aptr, d1=True, start0=st_out, unit_last=table, out=out,
                                    out_offsets=out_offs, units_cap=units_cap, err=e, ws=ws)

    append(err)
    ok = int(err.item()) == -1
    rb = Rebuild(tpf, ix, table, add, aptr, st_out)
    rerr = torch.zeros(1, dtype=torch.int64, device=dev)
    rb.run(rerr)
    ok = ok and int(rerr.item()) == -1
    o, oo, lp, lu, ul = res["r"]
    nu = rb.nunits
    nbytes = int(rb.offs[-1].item())
    ok = ok and bool(torch.equal(lp, rb.nptr)) and bool(torch.equal(lu, rb.unit)) and bool(torch.equal(oo[: nu + 1], rb.offs))
    ok = ok and bool(torch.equal(o[:nbytes], rb.out[:nbytes])) and bool(torch.equal(ul[:nu], rb.table))
    copy_dst = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src_p, dst_p = ctypes.c_void_p(ix.packed.data_ptr()), ctypes.c_void_p(copy_dst.data_ptr())

    def copy():
        assert L.tpf_copy_async(dst_p, src_p, in_bytes, stream) == 0

    fns = [append, copy] + ([] if args.no_rebuild_timing else [rb.run])
    ts = timed_alternately(fns, args.steps, args.warmup)
    r = {"verified": ok, "lists_out": nout, "lists_with_additions": int((counts > 0).sum().item()), "add_values": nadd,
         "in_bytes": in_bytes, "out_bytes": nbytes, "units_out": nu, "append_workspace_bytes": ws_bytes, "out_cap": out_cap,
         "append": ts[0], "copy_of_in_bytes": ts[1],
         "ratio_append_over_copy_time": round(ts[0]["ms_median"] / ts[1]["ms_median"], 3),
         "copy_GB_s": round(in_bytes / (ts[1]["ms_median"] * 1e-3) / 1e9, 1)}
    if not args.no_rebuild_timing:
        r["rebuild"] = ts[2]
        r["ratio_rebuild_over_append_time"] = round(ts[2]["ms_median"] / ts[0]["ms_median"], 2)
    return r


def kernel_stats(path):
    rows = []
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if "k_app_" in name or "k_lenc_" in name or "k_run_scan" in name or "k_copy16" in name:
                rows.append({"kernel": name.split("(")[0], "calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="spread,hot,new")
    ap.add_argument("--no-rebuild-timing", action="store_true", help="time the append and the copy only (profiling runs)")
    ap.add_argument("--kernel-stats", default=None, help="merge a rocprofv3 kernel stats CSV into the JSON instead of measuring")
    ap.add_argument("--kernel-stats-leg", default="spread")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_append_bench.json"))
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
                        "additions: scripts/lists_append_bench.py additions()"}
    t0 = time.time()
    vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
    flat = vals.view(-1)
    ptr = lb.zipf_lengths(nv, 7, dev)
    nl = ptr.numel() - 1
    ln = ptr[1:] - ptr[:-1]
    ix = Index(tpf, flat, ptr, True)
    table = tpf.lists_unit_last(ix.packed, ix.offs, ptr, start0=ix.start0)
    out["lists"], out["units"], out["in_bytes"] = nl, ix.nu, ix.packed.numel()
    ok_all = True
    nadd = nv // 100
    if "spread" in args.legs:
        # in proportion to the lengths: floor(n_j / 100), the rest one each to the longest lists
        counts = ln // 100
        rest = nadd - int(counts.sum().item())
        counts[torch.argsort(ln, descending=True)[:rest]] += 1
        out["spread"] = leg(tpf, L, ix, table, flat, counts, 41, args)
    if "hot" in args.legs:
        g = torch.Generator(device=dev)
        g.manual_seed(43)
        hot = torch.randperm(nl, generator=g, device=dev)[:HOT_LISTS]
        counts = torch.zeros(nl, dtype=torch.int64, device=dev)
        counts[hot] = nadd // HOT_LISTS
        counts[hot[0]] += nadd - int(counts.sum().item())
        out["hot"] = leg(tpf, L, ix, table, flat, counts, 45, args)
    if "new" in args.legs:
        counts = torch.zeros(nl + NEW_LISTS, dtype=torch.int64, device=dev)
        counts[nl:] = 1
        out["new"] = leg(tpf, L, ix, table, flat, counts, 47, args)
    for k in ("spread", "hot", "new"):
        if k in out:
            ok_all = ok_all and out[k]["verified"]
            print(f"[lists_append_bench] {k}:", json.dumps(out[k]), flush=True)
    return lxb.finish(out, args, t0, ok_all)


if __name__ == "__main__":
    sys.exit(main())
