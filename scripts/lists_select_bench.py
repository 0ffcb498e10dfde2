#!/usr/bin/env python
"""Measurement of the selective lists decode (tpf_p4ndec256v32_lists_select);
recorded in profiles/lists_select_bench.json, not gated.  Timed the way
bench.py times its steps (scripts/lists_bench.py's `timed`): warm-up, HIP
events around every call on the launch stream, median over the steps.  All in
one process on one box.

The index is the Zipf(1.5) lists stream of scripts/lists_bench.py (2.5M lists
at the default size), once delta-1 (every list chained from the value before
it) and once plain (the same values).

(1) everything: all lists selected in order against tpf_p4ndec256v32_lists on
    the same stream -- the price of the indirection, as a ratio.
(2) query shapes: selections of 1, 64 and 4,096 random lists, each with and
    without the longest list of the index, against (a) the full lists call
    (the only one-call way before this entry) and (b) a loop of
    tpf_p4ndec256v32, one call per selected list.
(3) index size: one selection of 4,096 lists drawn from the first tenth of the
    lists, decoded from the whole index and from the index that is only that
    tenth; the ratio of the two times.

    python scripts/lists_select_bench.py [--nblocks N] [--steps K] [--warmup W] [--out FILE]
"""
import argparse
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

SHAPES = (1, 64, 4096)


def expected(flat, ptr, sel):
    """the selected lists' values, concatenated in selection order"""
    a, n = ptr[sel], ptr[sel + 1] - ptr[sel]
    optr = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=flat.device)
    optr[1:] = torch.cumsum(n, 0)
    k = torch.repeat_interleave(torch.arange(sel.numel(), device=flat.device), n)
    idx = a[k] + (torch.arange(int(optr[-1].item()), dtype=torch.int64, device=flat.device) - optr[:-1][k])
    return flat[idx], optr


class Index:
    def __init__(self, tpf, flat, ptr, d1):
        self.tpf, self.d1, self.ptr = tpf, d1, ptr
        enc_full = lambda v, st: tpf.enc256v32(v, d1=d1, starts=st if d1 else None)
        enc_tail = lambda v, w, st: tpf.enc_batch("32", v.reshape(-1), v.shape[0], w, d1=d1, starts=st if d1 else None)
        self.packed, self.offs, self.start0 = lb.build_lists_stream(flat, ptr, enc_full, enc_tail)
        self.unit = tpf.lists_unit_base(ptr)
        self.nl, self.nu = ptr.numel() - 1, self.offs.numel() - 1

    def prefix(self, ns):
        """the index that holds only the first ns lists"""
        sub = object.__new__(Index)
        sub.tpf, sub.d1, sub.nl = self.tpf, self.d1, ns
        sub.nu = int(self.unit[ns].item())
        sub.ptr, sub.unit, sub.offs = self.ptr[: ns + 1].clone(), self.unit[: ns + 1].clone(), self.offs[: sub.nu + 1].clone()
        sub.packed, sub.start0 = self.packed[: int(sub.offs[-1].item())].clone(), self.start0[:ns].clone()
        return sub

    def select(self, sel, out, optr, err=None, ws=None):
        return self.tpf.decn256v32_lists_select(self.packed, self.offs, self.ptr, self.unit, sel, d1=self.d1, start0=self.start0, out=out,
                                                out_ptr=optr, err=err, ws=ws)


def measure_select(ix, flat, sel, args, L):
    """-> (verified, timing, values) of one selection, output and workspace sized for it"""
    want, want_ptr = expected(flat, ix.ptr, sel.long())
    nv = want.numel()
    out = torch.zeros(nv, dtype=torch.int32, device=flat.device)
    optr = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=flat.device)
    err = torch.zeros(1, dtype=torch.int64, device=flat.device)
    ws = torch.empty(int(L.tpf_p4ndec256v32_lists_select_workspace_size(sel.numel(), nv)), dtype=torch.uint8, device=flat.device)
    ix.select(sel, out, optr, err=err, ws=ws)
    ok = bool(torch.equal(out, want)) and bool(torch.equal(optr, want_ptr)) and int(err.item()) == -1
    t = lb.timed(lambda: ix.select(sel, out, optr, ws=ws), args.steps, args.warmup)
    return ok, t, nv


def measure_loop(ix, flat, sel, args, L):
    """one tpf_p4ndec256v32 call per selected list into the same dense output"""
    hs = sel.cpu().numpy().astype(np.int64)
    hp, hu = ix.ptr.cpu().numpy(), ix.unit.cpu().numpy().astype(np.int64)
    n = hp[hs + 1] - hp[hs]
    opos = np.concatenate([[0], np.cumsum(n)])
    out = torch.zeros(max(int(opos[-1]), 1), dtype=torch.int32, device=flat.device)
    hs0 = ix.start0.cpu().numpy().view(np.uint32)
    lws = torch.empty(int(L.tpf_p4ndec256v32_workspace_size(int(n.max()))), dtype=torch.uint8, device=flat.device)
    calls = [(ix.offs.data_ptr() + 8 * int(hu[j]), int(n[k]), int(hs0[j]), out.data_ptr() + 4 * int(opos[k])) for k, j in enumerate(hs)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f, pin, nbytes, pws, nws, d1 = L.tpf_p4ndec256v32, ix.packed.data_ptr(), ix.packed.numel(), lws.data_ptr(), lws.numel(), int(ix.d1)

    def loop():
        for o, cnt, st, dst in calls:
            f(pin, nbytes, o, cnt, d1, st, dst, pws, nws, None, s)

    t = lb.timed(loop, args.steps, min(args.warmup, 2))
    want, _ = expected(flat, ix.ptr, sel.long())
    return bool(torch.equal(out[: want.numel()], want)), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_select_bench.json"))
    args = ap.parse_args()
    import turbopfor_amd as tpf

    dev = "cuda:0"
    L = tpf.lib()
    nb, nv = args.nblocks, args.nblocks * 256
    res = {"nblocks": nb, "values": nv, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "kernel_md5": tpf.kernel_md5(),
           "generator": f"scripts/lists_bench.py: bounded Zipf(s={lb.ZIPF_S}) on [1, {lb.ZIPF_MAX}] over bench_data.gen_c3(nblocks, seed=7)"}
    t0 = time.time()
    vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
    flat = vals.view(-1)
    ptr = lb.zipf_lengths(nv, 7, dev)
    nl = ptr.numel() - 1
    ln = ptr[1:] - ptr[:-1]
    longest = int(torch.argmax(ln).item())
    res["lists"], res["longest_list_values"] = nl, int(ln[longest].item())
    rng = np.random.default_rng(7)
    picks = {m: torch.from_numpy(rng.choice(nl, size=min(m, nl), replace=False).astype(np.int32)).to(dev) for m in SHAPES}
    tenth = max(nl // 10, 1)
    pick10 = torch.from_numpy(rng.choice(tenth, size=min(4096, tenth), replace=False).astype(np.int32)).to(dev)
    ok_all = True
    out = torch.empty(nv, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)

    for d1 in (True, False):
        mode = "delta1" if d1 else "plain"
        ix = Index(tpf, flat, ptr, d1)
        r = {"units": ix.nu, "bytes_per_int": round(ix.packed.numel() / nv, 4)}
        # ---- (1) everything, in order, against the full lists call
        ws = torch.empty(int(L.tpf_p4ndec256v32_lists_workspace_size(ix.nu, nl)), dtype=torch.uint8, device=dev)
        out.zero_()
        tpf.decn256v32_lists(ix.packed, ix.offs, ptr, d1=d1, start0=ix.start0, out=out, err=err, ws=ws)
        ok = bool(torch.equal(out, flat)) and int(err.item()) == -1
        t_full = lb.timed(lambda: tpf.decn256v32_lists(ix.packed, ix.offs, ptr, d1=d1, start0=ix.start0, out=out, ws=ws), args.steps, args.warmup)
        del ws
        every = torch.arange(nl, dtype=torch.int32, device=dev)
        optr = torch.zeros(nl + 1, dtype=torch.int64, device=dev)
        sws = torch.empty(int(L.tpf_p4ndec256v32_lists_select_workspace_size(nl, nv)), dtype=torch.uint8, device=dev)
        out.zero_()
        ix.select(every, out, optr, err=err, ws=sws)
        ok = ok and bool(torch.equal(out, flat)) and bool(torch.equal(optr, ptr)) and int(err.item()) == -1
        t_sel = lb.timed(lambda: ix.select(every, out, optr, ws=sws), args.steps, args.warmup)
        del sws, every, optr
        r["everything"] = {"verified": ok, "full_lists_call": t_full, "select_all_in_order": t_sel,
                           "full_G_int32_s": lb.rate(nv, t_full), "select_G_int32_s": lb.rate(nv, t_sel),
                           "ratio_select_over_full_time": round(t_sel["ms_median"] / t_full["ms_median"], 4)}
        ok_all = ok_all and ok
        print(f"[lists_select_bench] {mode} everything:", json.dumps(r["everything"]), flush=True)

        # ---- (2) query shapes
        r["queries"] = []
        for m in SHAPES:
            for with_longest in (False, True):
                sel = picks[m].clone()
                if with_longest:
                    sel[sel.numel() // 2] = longest
                elif bool((sel == longest).any()):
                    sel[sel == longest] = (longest + 1) % nl
                ok, t, snv = measure_select(ix, flat, sel, args, L)
                okl, tl = measure_loop(ix, flat, sel, args, L)
                q = {"lists": int(sel.numel()), "with_longest": with_longest, "values": snv, "fraction_of_index_values": round(snv / nv, 8),
                     "verified": ok and okl, "select": t, "per_list_loop": tl, "full_lists_call_ms_median": t_full["ms_median"],
                     "select_over_full_time": round(t["ms_median"] / t_full["ms_median"], 6),
                     "loop_over_select_time": round(tl["ms_median"] / t["ms_median"], 2)}
                ok_all = ok_all and ok and okl
                r["queries"].append(q)
                print(f"[lists_select_bench] {mode} query:", json.dumps(q), flush=True)

        # ---- (3) the same selection from an index one tenth the size
        ok_big, t_big, snv = measure_select(ix, flat, pick10, args, L)
        sub = ix.prefix(tenth)
        ok_small, t_small, _ = measure_select(sub, flat, pick10, args, L)
        r["index_size"] = {"lists_selected": int(pick10.numel()), "values": snv, "verified": ok_big and ok_small,
                           "whole_index": {"lists": nl, "units": ix.nu, **t_big}, "tenth_index": {"lists": tenth, "units": sub.nu, **t_small},
                           "ratio_whole_over_tenth_time": round(t_big["ms_median"] / t_small["ms_median"], 4)}
        ok_all = ok_all and ok_big and ok_small
        print(f"[lists_select_bench] {mode} index size:", json.dumps(r["index_size"]), flush=True)
        res[mode] = r
        del ix, sub

    res["verified"] = ok_all
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
