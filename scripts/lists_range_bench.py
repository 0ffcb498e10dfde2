#!/usr/bin/env python
"""Measurement of the block-range reads of a resident index (tpf_lists_unit_last,
tpf_lists_range_units, tpf_p4ndec256v32_lists_units); recorded in
profiles/lists_range_bench.json, not gated.  Timed the way bench.py times its
steps (scripts/lists_bench.py's `timed`): warm-up, HIP events around every call
on the launch stream, median over the steps.  All legs in one process on one
box, on the Zipf(1.5) index of scripts/lists_select_bench.py, delta-1 and plain
(the same values).

(a) build time: tpf_lists_unit_last against the full tpf_p4ndec256v32_lists
    call on the same stream (delta-1), the table checked entry by entry.
(b) all lists, all units: the units decode against the selective decode and
    against the full call, delta-1 and plain -- whether delta-1's second decode
    is gone.
(c) narrow ranges: 4,096 random lists with the longest list forced in, each
    with a [lo, hi] that covers about one block (the values at a random position
    and 255 positions on); range search plus units decode against the selective
    decode of the same whole lists.  Values decoded and time for both.  (A list
    that wraps mod 2^32 is outside the range search's precondition: the one
    sorted list the index is cut from wraps every 2.6M values or so, and a pick
    that holds a wrap is replaced by the next list that does not.)
(d) plain companion: the plain index decoded over the unit ranges found in (c).

    python scripts/lists_range_bench.py [--nblocks N] [--steps K] [--warmup W] [--out FILE]
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
from lists_select_bench import Index  # noqa: E402

NQ = 4096


def u32(t):
    return t.to(torch.int64) & 0xFFFFFFFF


def units_of(ptr):
    n = ptr[1:] - ptr[:-1]
    return n, (n + 255) // 256


def expected_table(flat, ptr):
    n, units = units_of(ptr)
    lst = torch.repeat_interleave(torch.arange(n.numel(), device=flat.device), units)
    ubase = torch.cumsum(units, 0) - units
    i = torch.arange(int(units.sum().item()), dtype=torch.int64, device=flat.device) - ubase[lst]
    return flat[ptr[:-1][lst] + torch.minimum(256 * (i + 1), n[lst]) - 1]


def expected_units(flat, ptr, sel, uf, uc):
    """the values of units [uf, uf + uc) of the selected lists, concatenated in selection order"""
    n, units = units_of(ptr)
    sel, uf, uc = sel.long(), u32(uf), u32(uc)
    ns = n[sel]
    nv = torch.clamp(torch.minimum(256 * (uf + uc), ns) - 256 * uf, min=0)
    optr = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=flat.device)
    optr[1:] = torch.cumsum(nv, 0)
    k = torch.repeat_interleave(torch.arange(sel.numel(), device=flat.device), nv)
    idx = ptr[sel][k] + 256 * uf[k] + (torch.arange(int(optr[-1].item()), dtype=torch.int64, device=flat.device) - optr[:-1][k])
    return flat[idx], optr, k


def units_call(ix, table, sel, uf, uc, out, optr, err=None, ws=None):
    return ix.tpf.decn256v32_lists_units(ix.packed, ix.offs, ix.ptr, ix.unit, sel, uf, uc, d1=ix.d1, start0=ix.start0, unit_last=table,
                                         out=out, out_ptr=optr, err=err, ws=ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_range_bench.json"))
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
    ln, units = units_of(ptr)
    res["lists"] = nl
    # lists that hold no wrap of the one sorted list they are cut from: a wrap is a descent between two values of one list
    flatok = torch.ones(nl, dtype=torch.bool, device=dev)
    for a in range(0, nv - 1, bench_data.CHUNK):
        x = flat[a: min(a + bench_data.CHUNK + 1, nv)] ^ -(1 << 31)  # unsigned order as signed
        w = torch.nonzero(x[1:] < x[:-1]).view(-1) + a + 1            # position of the value after the wrap
        j = torch.searchsorted(ptr, w, right=True) - 1
        flatok[j[w > ptr[j]]] = False
    longest = int(torch.argmax(torch.where(flatok, ln, torch.zeros_like(ln))).item())
    res["longest_list_values"], res["longest_ascending_list_values"] = int(ln.max().item()), int(ln[longest].item())
    res["lists_holding_a_wrap"] = int((~flatok).sum().item())
    rng = np.random.default_rng(11)
    pick = torch.from_numpy(rng.choice(nl, size=min(NQ, nl), replace=False).astype(np.int64)).to(dev)
    pick[pick.numel() // 2] = longest
    for _ in range(8):  # a pick that holds a wrap: the next list
        bad = ~flatok[pick]
        if not bool(bad.any()):
            break
        pick[bad] = (pick[bad] + 1) % nl
    assert bool(flatok[pick].all())
    pos = torch.from_numpy(rng.random(pick.numel())).to(dev)
    p = torch.clamp((pos * ln[pick].to(torch.float64)).to(torch.int64), max=ln[pick] - 1)
    pe = torch.minimum(p + 255, ln[pick] - 1)
    qlist = pick.to(torch.int32)
    qlo, qhi = flat[ptr[pick] + p].clone(), flat[ptr[pick] + pe].clone()
    in_range = pe - p + 1
    ok_all = True
    out = torch.empty(nv, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    found = None

    for d1 in (True, False):
        mode = "delta1" if d1 else "plain"
        ix = Index(tpf, flat, ptr, d1)
        r = {"units": ix.nu, "bytes_per_int": round(ix.packed.numel() / nv, 4)}
        ws = torch.empty(int(L.tpf_p4ndec256v32_lists_workspace_size(ix.nu, nl)), dtype=torch.uint8, device=dev)
        out.zero_()
        tpf.decn256v32_lists(ix.packed, ix.offs, ptr, d1=d1, start0=ix.start0, out=out, err=err, ws=ws)
        ok = bool(torch.equal(out, flat)) and int(err.item()) == -1
        t_full = lb.timed(lambda: tpf.decn256v32_lists(ix.packed, ix.offs, ptr, d1=d1, start0=ix.start0, out=out, ws=ws), args.steps, args.warmup)
        del ws
        table = None
        if d1:
            # ---- (a) the skip table, once per index
            table = torch.zeros(ix.nu, dtype=torch.int32, device=dev)
            tws = torch.empty(int(L.tpf_lists_unit_last_workspace_size(ix.nu, nl)), dtype=torch.uint8, device=dev)
            tpf.lists_unit_last(ix.packed, ix.offs, ptr, start0=ix.start0, out=table, err=err, ws=tws)
            okt = bool(torch.equal(table, expected_table(flat, ptr))) and int(err.item()) == -1
            t_tab = lb.timed(lambda: tpf.lists_unit_last(ix.packed, ix.offs, ptr, start0=ix.start0, out=table, ws=tws), args.steps, args.warmup)
            r["build"] = {"verified": okt, "unit_last": t_tab, "full_lists_call": t_full, "workspace_bytes": tws.numel(),
                          "table_bytes": 4 * ix.nu, "ratio_build_over_full_time": round(t_tab["ms_median"] / t_full["ms_median"], 4)}
            ok = ok and okt
            del tws
            print(f"[lists_range_bench] {mode} build:", json.dumps(r["build"]), flush=True)

        # ---- (b) all lists, all units
        every = torch.arange(nl, dtype=torch.int32, device=dev)
        optr = torch.zeros(nl + 1, dtype=torch.int64, device=dev)
        sws = torch.empty(int(L.tpf_p4ndec256v32_lists_select_workspace_size(nl, nv)), dtype=torch.uint8, device=dev)
        out.zero_()
        ix.select(every, out, optr, err=err, ws=sws)
        ok = ok and bool(torch.equal(out, flat)) and bool(torch.equal(optr, ptr)) and int(err.item()) == -1
        t_sel = lb.timed(lambda: ix.select(every, out, optr, ws=sws), args.steps, args.warmup)
        del sws
        uws = torch.empty(int(L.tpf_p4ndec256v32_lists_units_workspace_size(nl, nv)), dtype=torch.uint8, device=dev)
        uf0, ucall = torch.zeros(nl, dtype=torch.int32, device=dev), units.to(torch.int32)
        out.zero_()
        optr.zero_()
        units_call(ix, table, every, uf0, ucall, out, optr, err=err, ws=uws)
        ok = ok and bool(torch.equal(out, flat)) and bool(torch.equal(optr, ptr)) and int(err.item()) == -1
        t_un = lb.timed(lambda: units_call(ix, table, every, uf0, ucall, out, optr, ws=uws), args.steps, args.warmup)
        r["everything"] = {"verified": ok, "full_lists_call": t_full, "select_all_in_order": t_sel, "units_all_in_order": t_un,
                           "units_workspace_bytes": uws.numel(), "full_G_int32_s": lb.rate(nv, t_full),
                           "select_G_int32_s": lb.rate(nv, t_sel), "units_G_int32_s": lb.rate(nv, t_un),
                           "ratio_select_over_full_time": round(t_sel["ms_median"] / t_full["ms_median"], 4),
                           "ratio_units_over_full_time": round(t_un["ms_median"] / t_full["ms_median"], 4),
                           "ratio_units_over_select_time": round(t_un["ms_median"] / t_sel["ms_median"], 4)}
        del uws, every, optr, uf0, ucall
        ok_all = ok_all and ok
        print(f"[lists_range_bench] {mode} everything:", json.dumps(r["everything"]), flush=True)

        nq = qlist.numel()
        cap = 3 * 256 * nq  # 256 values span at most two units, the top end adds at most one
        qout = torch.zeros(cap, dtype=torch.int32, device=dev)
        qptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        qws = torch.empty(int(L.tpf_p4ndec256v32_lists_units_workspace_size(nq, cap)), dtype=torch.uint8, device=dev)
        if d1:
            # ---- (c) narrow ranges: search + units decode against the selective decode of the same whole lists
            uf = torch.zeros(nq, dtype=torch.int32, device=dev)
            uc = torch.zeros(nq, dtype=torch.int32, device=dev)
            err2 = torch.zeros(1, dtype=torch.int64, device=dev)

            def search_and_decode(e1=None, e2=None):
                tpf.lists_range_units(ix.unit, table, qlist, qlo, qhi, ufirst=uf, ucount=uc, err=e1)
                units_call(ix, table, qlist, uf, uc, qout, qptr, err=e2, ws=qws)

            search_and_decode(err, err2)
            want, want_ptr, k = expected_units(flat, ptr, qlist, uf, uc)
            got = qout[: want.numel()]
            inside = (u32(got) >= u32(qlo)[k]) & (u32(got) <= u32(qhi)[k])
            okc = (int(err.item()) == -1 and int(err2.item()) == -1 and bool(torch.equal(qptr, want_ptr)) and bool(torch.equal(got, want))
                   and bool(torch.equal(torch.bincount(k[inside], minlength=nq), in_range)))
            t_rs = lb.timed(lambda: tpf.lists_range_units(ix.unit, table, qlist, qlo, qhi, ufirst=uf, ucount=uc), args.steps, args.warmup)
            t_sd = lb.timed(search_and_decode, args.steps, args.warmup)
            found = (uf.clone(), uc.clone())
            whole = int(ln[pick].sum().item())
            wout = torch.zeros(whole, dtype=torch.int32, device=dev)
            wptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            wws = torch.empty(int(L.tpf_p4ndec256v32_lists_select_workspace_size(nq, whole)), dtype=torch.uint8, device=dev)
            ix.select(qlist, wout, wptr, err=err, ws=wws)
            okc = okc and int(err.item()) == -1 and int(wptr[-1].item()) == whole
            t_whole = lb.timed(lambda: ix.select(qlist, wout, wptr, ws=wws), args.steps, args.warmup)
            r["narrow_ranges"] = {"verified": okc, "queries": nq, "values_in_range": int(in_range.sum().item()),
                                  "units_named": int(u32(uc).sum().item()), "values_decoded_by_units": int(want.numel()),
                                  "values_decoded_by_select": whole, "range_search": t_rs, "range_search_plus_units_decode": t_sd,
                                  "select_whole_lists": t_whole,
                                  "select_over_search_plus_units_time": round(t_whole["ms_median"] / t_sd["ms_median"], 2)}
            ok_all = ok_all and okc
            del wout, wptr, wws
            print(f"[lists_range_bench] {mode} narrow ranges:", json.dumps(r["narrow_ranges"]), flush=True)
        else:
            # ---- (d) the plain companion over the unit ranges found for (c)
            uf, uc = found
            units_call(ix, None, qlist, uf, uc, qout, qptr, err=err, ws=qws)
            want, want_ptr, _ = expected_units(flat, ptr, qlist, uf, uc)
            okd = int(err.item()) == -1 and bool(torch.equal(qptr, want_ptr)) and bool(torch.equal(qout[: want.numel()], want))
            t_pc = lb.timed(lambda: units_call(ix, None, qlist, uf, uc, qout, qptr, ws=qws), args.steps, args.warmup)
            r["plain_companion"] = {"verified": okd, "queries": nq, "values_decoded": int(want.numel()), "units_decode": t_pc}
            ok_all = ok_all and okd
            print(f"[lists_range_bench] {mode} companion:", json.dumps(r["plain_companion"]), flush=True)
        res[mode] = r
        del ix, qout, qptr, qws, table

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
