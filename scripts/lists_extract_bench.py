#!/usr/bin/env python
"""Measurement of the sub-index of a resident index (tpf_lists_extract);
recorded in profiles/lists_extract_bench.json, not gated.  Timed the way
scripts/lists_append_bench.py times: warm-up, HIP events around every call on
the launch stream, median over the steps; the calls of a leg alternate step by
step.  All legs in one process on one box.  The index is
scripts/lists_bench.py's Zipf(1.5) delta-1 index (2.5M lists at the default
size) with its skip table, plus lists_gather_bench.py's frequency stream over
the same directory for leg (d).  Every result is checked at full size on the
device against the rebuild -- the selected values decoded
(tpf_p4ndec256v32_lists_units), encoded again (tpf_p4nenc256v32_lists with the
starts the definition gives), tpf_lists_unit_base and tpf_lists_unit_last --
bytes, offsets, both directories, the starts and the table.

(a) all: every list in order, against tpf_copy_async of the index and against
    tpf_lists_remove with nq == 0, the existing plain restitch.
(b) random: 4,096 random lists, against today's route (select-decode,
    tpf_p4nenc256v32_lists, tpf_lists_unit_base, tpf_lists_unit_last).
(c) shard: shard 0 of 8 by term (tpf_shard.term_shard).
(d) window: a doc-id window on every list through tpf_lists_range_units, the
    doc ids and the frequencies.

    python scripts/lists_extract_bench.py [--nblocks N] [--steps K] [--warmup W] [--legs all,random,shard,window] [--out FILE]
"""
import argparse
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
from lists_gather_bench import frequencies, timed_alternately  # noqa: E402
from lists_select_bench import Index  # noqa: E402

RANDOM_LISTS = 4096
WORLD = 8


class Case:
    """One selection on one stream of the index: the buffers of the call, sized once by the binding's default path."""

    def __init__(self, tpf, ix, ptr, table, d1, sel, uf=None, uc=None):
        self.tpf, self.ix, self.ptr, self.table, self.d1, self.sel, self.uf, self.uc = tpf, ix, ptr, table, d1, sel, uf, uc
        self.err = torch.zeros(1, dtype=torch.int64, device=sel.device)
        self.res = self.call(err=self.err)  # the synchronous default: sizes out and out_offsets
        self.ok = int(self.err.item()) == -1
        self.out, self.offs = self.res[0], self.res[1]
        self.ws = torch.empty(max(int(tpf.lib().tpf_lists_extract_workspace_size(sel.numel())), 1), dtype=torch.uint8, device=sel.device)

    def call(self, out=None, offs=None, err=None, ws=None):
        ix = self.ix
        return self.tpf.lists_extract(ix.packed, ix.offs, self.ptr, ix.unit, self.sel, self.uf, self.uc, d1=self.d1,
                                      start0=ix.start0 if self.d1 else None, unit_last=self.table if self.d1 else None, out=out,
                                      out_offsets=offs, err=err, ws=ws)

    def run(self):
        self.res = self.call(self.out, self.offs, None, self.ws)

    def ranges(self):
        if self.uf is not None:
            return self.uf, self.uc
        j = self.sel.long()
        return torch.zeros_like(self.sel), (self.ix.unit[j + 1] - self.ix.unit[j])

    def starts(self):
        """d_start0_out by its definition, in torch"""
        uf, _ = self.ranges()
        j = self.sel.long()
        before = (self.ix.unit[j].long() + (uf.long() & 0xFFFFFFFF) - 1).clamp(min=0)
        return torch.where(uf == 0, self.ix.start0[j], self.table[before])

    def rebuild(self, select=False):
        """-> the rebuild's (packed, offsets, list_ptr, list_unit, start0, table); select: today's route for whole lists"""
        tpf, ix, d1 = self.tpf, self.ix, self.d1
        uf, uc = self.ranges()
        if select:
            vals, optr = tpf.decn256v32_lists_select(ix.packed, ix.offs, self.ptr, ix.unit, self.sel, d1=d1, start0=ix.start0 if d1 else None)
        else:
            vals, optr = tpf.decn256v32_lists_units(ix.packed, ix.offs, self.ptr, ix.unit, self.sel, uf, uc, d1=d1,
                                                    start0=ix.start0 if d1 else None, unit_last=self.table if d1 else None)
        st = self.starts() if d1 else None
        packed, offs = tpf.encn256v32_lists(vals, optr, d1=d1, start0=st)
        unit = tpf.lists_unit_base(optr)
        tab = tpf.lists_unit_last(packed, offs, optr, start0=st) if d1 else None
        return packed, offs, optr, unit, st, tab

    def verify(self, rb=None):
        rb = self.rebuild() if rb is None else rb
        o, oo, lp, lu, st, ul = self.res
        nu, nb = rb[1].numel() - 1, rb[0].numel()
        ok = self.ok and int(lu[-1].item()) == nu and bool(torch.equal(lp, rb[2])) and bool(torch.equal(lu, rb[3]))
        ok = ok and bool(torch.equal(oo[: nu + 1], rb[1])) and bool(torch.equal(o[:nb], rb[0]))
        if self.d1:
            ok = ok and bool(torch.equal(st, rb[4])) and bool(torch.equal(ul[:nu], rb[5]))
        self.units, self.bytes = nu, nb
        return ok

    def facts(self):
        return {"selections": self.sel.numel(), "units_out": self.units, "out_bytes": self.bytes, "workspace_bytes": self.ws.numel()}


def leg_all(tpf, L, ix, ptr, table, args):
    dev, nl = ptr.device, ptr.numel() - 1
    c = Case(tpf, ix, ptr, table, True, torch.arange(nl, dtype=torch.int32, device=dev))
    # the index is the encoder's own output for these values: the rebuild of the identity is the index
    c.units, c.bytes = ix.nu, ix.packed.numel()
    o, oo, lp, lu, st, ul = c.res
    ok = c.ok and bool(torch.equal(o, ix.packed)) and bool(torch.equal(oo, ix.offs)) and bool(torch.equal(lp, ptr - ptr[0]))
    ok = ok and bool(torch.equal(lu, ix.unit)) and bool(torch.equal(st, ix.start0)) and bool(torch.equal(ul, table))
    in_bytes = ix.packed.numel()
    dst = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src_p, dst_p = ctypes.c_void_p(ix.packed.data_ptr()), ctypes.c_void_p(dst.data_ptr())

    def copy():
        assert L.tpf_copy_async(dst_p, src_p, in_bytes, stream) == 0

    rout, roffs = torch.empty(in_bytes, dtype=torch.uint8, device=dev), torch.empty(ix.nu + 1, dtype=torch.int64, device=dev)
    rws = torch.empty(max(int(L.tpf_lists_remove_workspace_size(ix.nu, nl, 0, 0, 0)), 1), dtype=torch.uint8, device=dev)
    rerr = torch.zeros(1, dtype=torch.int64, device=dev)
    none32, none64 = torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)

    def restitch(e=None):
        return tpf.lists_remove(ix.packed, ix.offs, ptr, ix.unit, none32, none64, none32, 0, d1=True, start0=ix.start0, unit_last=table,
                                out=rout, out_offsets=roffs, units_cap=ix.nu, err=e, ws=rws)

    r = restitch(rerr)
    ok = ok and int(rerr.item()) == -1 and bool(torch.equal(r[0], ix.packed)) and bool(torch.equal(r[1], ix.offs))
    ts = timed_alternately([c.run, restitch, copy], args.steps, args.warmup)
    return dict(c.facts(), verified=ok, extract=ts[0], restitch_by_remove_nq0=ts[1], copy_of_in_bytes=ts[2],
                ratio_extract_over_restitch_time=round(ts[0]["ms_median"] / ts[1]["ms_median"], 3),
                ratio_extract_over_copy_time=round(ts[0]["ms_median"] / ts[2]["ms_median"], 3))


def leg_lists(tpf, ix, ptr, table, sel, args, todays_route):
    c = Case(tpf, ix, ptr, table, True, sel)
    ok = c.verify(c.rebuild(select=todays_route))
    fns = [c.run] + ([lambda: c.rebuild(select=True)] if todays_route else [])
    ts = timed_alternately(fns, args.steps, args.warmup)
    r = dict(c.facts(), verified=ok, extract=ts[0], values=int(c.res[2][-1].item()))
    if todays_route:
        r["todays_route"] = ts[1]  # its default paths read sizes back, as a caller of today has to
        r["ratio_todays_route_over_extract_time"] = round(ts[1]["ms_median"] / ts[0]["ms_median"], 2)
    return r


def leg_window(tpf, ix, fx, ptr, table, flat, args):
    """every list: the doc ids between the values at 40 % and 60 % of the list"""
    dev, nl = ptr.device, ptr.numel() - 1
    ln = ptr[1:] - ptr[:-1]
    some = ln > 0
    at = lambda f: flat[(ptr[:-1] + (ln.double() * f).long()).clamp(max=flat.numel() - 1)]
    qlo, qhi = torch.where(some, at(0.4), torch.ones_like(at(0.4))), torch.where(some, at(0.6), torch.zeros_like(at(0.6)))
    qlist = torch.arange(nl, dtype=torch.int32, device=dev)
    uf, uc = torch.empty_like(qlist), torch.empty_like(qlist)

    def search():
        tpf.lists_range_units(ix.unit, table, qlist, qlo, qhi, ufirst=uf, ucount=uc)

    search()
    d, f = Case(tpf, ix, ptr, table, True, qlist, uf, uc), Case(tpf, fx, ptr, table, False, qlist, uf, uc)
    ok = d.verify() and f.verify()
    ts = timed_alternately([search, d.run, f.run], args.steps, args.warmup)
    return dict(d.facts(), verified=ok, frequencies_out_bytes=f.bytes, values=int(d.res[2][-1].item()), range_search=ts[0],
                extract_doc_ids=ts[1], extract_frequencies=ts[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="all,random,shard,window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_extract_bench.json"))
    args = ap.parse_args()
    args.legs = args.legs.split(",")
    import tpf_shard
    import turbopfor_amd as tpf

    dev = "cuda:0"
    L = tpf.lib()
    nb, nv = args.nblocks, args.nblocks * 256
    out = {"nblocks": nb, "values": nv, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "boxes": 1,
           "runs": 1, "kernel_md5": tpf.kernel_md5(), "tile_bytes": tpf.LISTS_APPEND_TILE,
           "generator": f"scripts/lists_bench.py: bounded Zipf(s={lb.ZIPF_S}) on [1, {lb.ZIPF_MAX}] over bench_data.gen_c3(nblocks, seed=7); "
                        "frequencies: scripts/lists_gather_bench.py frequencies(seed=19)"}
    t0 = time.time()
    vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
    flat = vals.view(-1)
    ptr = lb.zipf_lengths(nv, 7, dev)
    nl = ptr.numel() - 1
    ix = Index(tpf, flat, ptr, True)
    table = tpf.lists_unit_last(ix.packed, ix.offs, ptr, start0=ix.start0)
    out["lists"], out["units"], out["in_bytes"] = nl, ix.nu, ix.packed.numel()
    legs = {}
    if "all" in args.legs:
        legs["all"] = leg_all(tpf, L, ix, ptr, table, args)
    if "random" in args.legs:
        g = torch.Generator(device=dev)
        g.manual_seed(43)
        sel = torch.randperm(nl, generator=g, device=dev)[:RANDOM_LISTS].to(torch.int32)
        legs["random"] = leg_lists(tpf, ix, ptr, table, sel, args, todays_route=True)
    if "shard" in args.legs:
        legs["shard"] = leg_lists(tpf, ix, ptr, table, tpf_shard.term_shard(nl, WORLD, 0, device=dev), args, todays_route=False)
    if "window" in args.legs:
        fx = Index(tpf, frequencies(nv, dev, 19), ptr, False)
        legs["window"] = leg_window(tpf, ix, fx, ptr, table, flat, args)
    ok_all = True
    for k, v in legs.items():
        out[k] = v
        ok_all = ok_all and v["verified"]
        print(f"[lists_extract_bench] {k}:", json.dumps(v), flush=True)
    return lxb.finish(out, args, t0, ok_all)


if __name__ == "__main__":
    sys.exit(main())
