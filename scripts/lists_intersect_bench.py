#!/usr/bin/env python
"""Measurement of the intersection with a resident index (tpf_lists_intersect);
recorded in profiles/lists_intersect_bench.json, not gated.  Timed the way
bench.py times its steps (scripts/lists_bench.py's `timed`): warm-up, HIP
events around every call on the launch stream, median over the steps.  All
legs in one process on one box.  Only lists that ascend without wrapping mod
2^32 are used (the precondition of the skip-table search), and every result is
checked at full size on the device against torch.isin.

(a) sparse: 4,096 queries on the Zipf(1.5) delta-1 index of
    scripts/lists_select_bench.py.  Each probe is a list of 8 to 256 values,
    decoded with the selective decode; each target is a list of at least 256
    units whose doc-id range covers the probe's.  The intersection against
    what the library could do before it for the same queries:
    tpf_lists_range_units over [probe first, probe last] plus the delta-1
    units decode -- which yields a superset of blocks, not the answer.
(a') spread: the same targets, each probed with 128 values spread over the
    whole list (64 members at even positions and the 64 values after them), so
    the one [lo, hi] of the range search names every unit of the target.
(b) dense: three lists of about 2M values drawn from one universe of 4M doc
    ids (each id kept with probability 1/2, so two lists share about half
    their members), in an index of their own.  The probe is one whole list,
    the target another; against the units decode of the whole target, which
    any answer has to pay at least once.
(c) a 3-term AND over those three lists: two calls chained on the device, the
    output of the first the probe of the second.

    python scripts/lists_intersect_bench.py [--nblocks N] [--steps K] [--warmup W] [--legs sparse,spread,dense,and3] [--out FILE]

--legs runs a subset (the committed JSON holds all four): a rocprofv3
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
from lists_select_bench import Index  # noqa: E402

NQ = 4096


def u32(t):
    return t.to(torch.int64) & 0xFFFFFFFF


class Resident:
    """an Index with its skip table and the buffers one intersect call needs"""

    def __init__(self, tpf, flat, ptr):
        self.tpf, self.flat, self.ptr = tpf, flat, ptr
        self.ix = Index(tpf, flat, ptr, True)
        self.table = tpf.lists_unit_last(self.ix.packed, self.ix.offs, ptr, start0=self.ix.start0)

    def intersect(self, probe, probe_ptr, qlist, out, out_ptr, pidx=None, tpos=None, err=None, ws=None):
        ix = self.ix
        return self.tpf.lists_intersect(ix.packed, ix.offs, ix.ptr, ix.unit, self.table, probe, probe_ptr, qlist, start0=ix.start0, out=out,
                                        out_ptr=out_ptr, pidx=pidx, tpos=tpos, err=err, ws=ws)

    def units(self, sel, uf, uc, out, optr, err=None, ws=None):
        ix = self.ix
        return self.tpf.decn256v32_lists_units(ix.packed, ix.offs, ix.ptr, ix.unit, sel, uf, uc, d1=True, start0=ix.start0,
                                               unit_last=self.table, out=out, out_ptr=optr, err=err, ws=ws)


def check(res, probe, probe_ptr, qlist, out, out_ptr, tpos=None):
    """every query against torch.isin over its whole target list -> (verified, hits, units a probe value lands in)"""
    pp, ql = probe_ptr.tolist(), qlist.long()
    la, lb_ = res.ptr[ql].tolist(), res.ptr[ql + 1].tolist()
    uas, ubs = res.ix.unit[ql].tolist(), res.ix.unit[ql + 1].tolist()
    ok, want_ptr, at, landed = True, [0], 0, 0
    for k in range(ql.numel()):
        pv = u32(probe[pp[k]: pp[k + 1]])
        tgt = u32(res.flat[la[k]: lb_[k]])
        hit = torch.isin(pv, tgt)
        n = int(hit.sum().item())
        ok = ok and bool(torch.equal(u32(out[at: at + n]), pv[hit]))
        u = torch.searchsorted(u32(res.table[uas[k]: ubs[k]]), pv)  # the definition: the first unit whose last value is >= v
        landed += int(torch.unique(u[u < ubs[k] - uas[k]]).numel())
        if tpos is not None:
            ok = ok and bool(torch.equal(tgt[u32(tpos[at: at + n])], pv[hit]))
        at += n
        want_ptr.append(at)
    ok = ok and bool(torch.equal(out_ptr, torch.tensor(want_ptr, dtype=torch.int64, device=probe.device)))
    return ok, at, landed


def measure(res, L, args, probe, probe_ptr, qlist, qlo, qhi, name):
    """one set of queries: the intersection, and range search + units decode over [qlo, qhi] of every query"""
    tpf, dev, nq = res.tpf, probe.device, qlist.numel()
    if name not in args.legs:
        return {"verified": True, "skipped": True}
    out = torch.zeros(probe.numel(), dtype=torch.int32, device=dev)
    tpos = torch.zeros(probe.numel(), dtype=torch.int32, device=dev)
    optr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.tpf_lists_intersect_workspace_size(nq, probe.numel())), dtype=torch.uint8, device=dev)
    res.intersect(probe, probe_ptr, qlist, out, optr, tpos=tpos, err=err[0:1], ws=ws)
    ok, hits, landed = check(res, probe, probe_ptr, qlist, out, optr, tpos)
    ok = ok and int(err[0].item()) == -1
    t_ix = lb.timed(lambda: res.intersect(probe, probe_ptr, qlist, out, optr, ws=ws), args.steps, args.warmup)
    # what the library could do before: one [lo, hi] per query, then the blocks it names decoded to memory
    uf = torch.zeros(nq, dtype=torch.int32, device=dev)
    uc = torch.zeros(nq, dtype=torch.int32, device=dev)
    tpf.lists_range_units(res.ix.unit, res.table, qlist, qlo, qhi, ufirst=uf, ucount=uc, err=err[0:1])
    named = int(u32(uc).sum().item())
    cap = 256 * named
    bout = torch.zeros(cap, dtype=torch.int32, device=dev)
    bptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    bws = torch.empty(int(L.tpf_p4ndec256v32_lists_units_workspace_size(nq, cap)), dtype=torch.uint8, device=dev)

    def search_and_decode(e1=None, e2=None):
        tpf.lists_range_units(res.ix.unit, res.table, qlist, qlo, qhi, ufirst=uf, ucount=uc, err=e1)
        res.units(qlist, uf, uc, bout, bptr, err=e2, ws=bws)

    search_and_decode(err[0:1], err[1:2])
    ok = ok and err.tolist() == [-1, -1] and landed <= named
    t_base = lb.timed(search_and_decode, args.steps, args.warmup)
    r = {"verified": ok, "queries": nq, "probe_values": int(probe_ptr[-1].item() - probe_ptr[0].item()), "hits": hits,
         "units_decoded_by_intersect": landed, "units_named_by_range_search": named, "values_decoded_by_baseline": int(bptr[-1].item()),
         "intersect": t_ix, "range_search_plus_units_decode": t_base, "intersect_workspace_bytes": ws.numel(),
         "ratio_intersect_over_baseline_time": round(t_ix["ms_median"] / t_base["ms_median"], 4)}
    print(f"[lists_intersect_bench] {name}:", json.dumps(r), flush=True)
    return r


def sparse_queries(flat, ptr, flatok, rng):
    """(probe lists, targets): short ascending lists, each with a random ascending list of >= 256 units that covers its range"""
    ln = ptr[1:] - ptr[:-1]
    first, last = u32(flat[ptr[:-1]]), u32(flat[ptr[1:] - 1])
    long_ids = torch.nonzero(flatok & (ln >= 256 * 255 + 1)).view(-1)
    short_ids = torch.nonzero(flatok & (ln >= 8) & (ln <= 256)).view(-1)
    tf, tl, tid = first[long_ids].cpu().numpy(), last[long_ids].cpu().numpy(), long_ids.cpu().numpy()
    cand = short_ids[torch.from_numpy(rng.permutation(short_ids.numel())[: 64 * NQ]).to(flat.device)]
    cf, cl, cid = first[cand].cpu().numpy(), last[cand].cpu().numpy(), cand.cpu().numpy()
    probes, targets = [], []
    for f, l, c in zip(cf, cl, cid):
        cover = np.nonzero((tf <= f) & (tl >= l))[0]
        if len(cover):
            probes.append(int(c))
            targets.append(int(tid[cover[rng.integers(0, len(cover))]]))
            if len(probes) == NQ:
                break
    return probes, targets, int(long_ids.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_intersect_bench.json"))
    ap.add_argument("--legs", default="sparse,spread,dense,and3", help="the legs to run (a per-kernel profile wants one at a time)")
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
    ok_all = True

    # ---- (a) sparse: short probe lists against long targets that cover them
    probes, targets, nlong = sparse_queries(flat, ptr, flatok, rng)
    nq = len(probes)
    psel = torch.tensor(probes, dtype=torch.int32, device=dev)
    qlist = torch.tensor(targets, dtype=torch.int32, device=dev)
    total = int(ln[psel.long()].sum().item())
    probe = torch.zeros(total, dtype=torch.int32, device=dev)
    pptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    res.ix.select(psel, probe, pptr)
    qlo, qhi = probe[pptr[:-1]].clone(), probe[pptr[1:] - 1].clone()
    r = measure(res, L, args, probe, pptr, qlist, qlo, qhi, "sparse")
    r["lists_of_at_least_256_units"] = nlong
    r["distinct_targets"] = len(set(targets))
    r["mean_target_units"] = round(float(((ln[qlist.long()] + 255) // 256).double().mean().item()), 1)
    out["sparse"] = r
    ok_all = ok_all and r["verified"] and nq == NQ

    # ---- (a') spread: 128 values over the whole of every target
    n_t = ln[qlist.long()]
    pos = (torch.arange(64, device=dev, dtype=torch.float64)[None, :] + 0.5) / 64.0 * n_t[:, None].to(torch.float64)
    idx = ptr[qlist.long()][:, None] + pos.to(torch.int64)
    members = u32(flat[idx])
    # ascending: the value after a member is at most the next pick, thousands of positions on
    spread = torch.stack([members, torch.clamp(members + 1, max=0xFFFFFFFF)], dim=2).reshape(-1)
    probe2 = (spread - ((spread >> 31) << 32)).to(torch.int32)  # the uint32 bit patterns
    pptr2 = torch.arange(nq + 1, dtype=torch.int64, device=dev) * 128
    r = measure(res, L, args, probe2, pptr2, qlist, probe2[pptr2[:-1]].clone(), probe2[pptr2[1:] - 1].clone(), "spread")
    out["spread"] = r
    ok_all = ok_all and r["verified"]
    del res, probe, probe2, vals, flat
    if "dense" not in args.legs and "and3" not in args.legs:
        return finish(out, args, t0, ok_all)

    # ---- (b), (c): three lists over one universe, an index of their own
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    universe = torch.unique(torch.randint(1, 1 << 31, (1 << 22,), generator=g, device=dev, dtype=torch.int64))
    lists = [universe[torch.rand(universe.numel(), generator=g, device=dev) < 0.5] for _ in range(3)]
    dflat = torch.cat(lists).to(torch.int32)
    dptr = torch.tensor(np.concatenate([[0], np.cumsum([v.numel() for v in lists])]), dtype=torch.int64, device=dev)
    dres = Resident(tpf, dflat, dptr)
    n0, n1 = lists[0].numel(), lists[1].numel()
    probe = dflat[:n0].clone()
    pptr = torch.tensor([0, n0], dtype=torch.int64, device=dev)
    q1 = torch.tensor([1], dtype=torch.int32, device=dev)
    q2 = torch.tensor([2], dtype=torch.int32, device=dev)
    err = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.tpf_lists_intersect_workspace_size(1, n0)), dtype=torch.uint8, device=dev)
    out1, ptr1 = torch.zeros(n0, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    out2, ptr2 = torch.zeros(n0, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    dres.intersect(probe, pptr, q1, out1, ptr1, err=err[0:1], ws=ws)
    want1 = lists[0][torch.isin(lists[0], lists[1])]
    okb = int(err[0].item()) == -1 and int(ptr1[1].item()) == want1.numel() and bool(torch.equal(u32(out1[: want1.numel()]), want1))
    t_ix = lb.timed(lambda: dres.intersect(probe, pptr, q1, out1, ptr1, ws=ws), args.steps, args.warmup)
    units1 = (n1 + 255) // 256
    uf, uc = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([units1], dtype=torch.int32, device=dev)
    bout, bptr = torch.zeros(n1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    bws = torch.empty(int(L.tpf_p4ndec256v32_lists_units_workspace_size(1, n1)), dtype=torch.uint8, device=dev)
    dres.units(q1, uf, uc, bout, bptr, err=err[1:2], ws=bws)
    okb = okb and int(err[1].item()) == -1 and bool(torch.equal(u32(bout), lists[1]))
    t_dec = lb.timed(lambda: dres.units(q1, uf, uc, bout, bptr, ws=bws), args.steps, args.warmup)
    out["dense"] = {"verified": okb, "probe_values": n0, "target_values": n1, "target_units": units1, "hits": int(want1.numel()),
                    "bytes_per_int": round(dres.ix.packed.numel() / dflat.numel(), 4), "intersect": t_ix,
                    "units_decode_of_the_whole_target": t_dec, "intersect_G_probe_values_s": lb.rate(n0, t_ix),
                    "ratio_intersect_over_decode_time": round(t_ix["ms_median"] / t_dec["ms_median"], 4)}
    ok_all = ok_all and okb
    print("[lists_intersect_bench] dense:", json.dumps(out["dense"]), flush=True)

    def chain(e1=None, e2=None):
        dres.intersect(probe, pptr, q1, out1, ptr1, err=e1, ws=ws)
        dres.intersect(out1, ptr1, q2, out2, ptr2, err=e2, ws=ws)  # the output of the first call is the probe of the second

    if "and3" in args.legs:
        chain(err[0:1], err[1:2])
        want2 = want1[torch.isin(want1, lists[2])]
        okc = err.tolist() == [-1, -1] and int(ptr2[1].item()) == want2.numel() and bool(torch.equal(u32(out2[: want2.numel()]), want2))
        okc = okc and 0 < want2.numel() < min(v.numel() for v in lists)
        t_chain = lb.timed(chain, args.steps, args.warmup)
        out["and3"] = {"verified": okc, "list_values": [v.numel() for v in lists], "hits_after_two_terms": int(want1.numel()),
                       "hits": int(want2.numel()), "two_chained_calls": t_chain}
        ok_all = ok_all and okc
        print("[lists_intersect_bench] and3:", json.dumps(out["and3"]), flush=True)
    return finish(out, args, t0, ok_all)


def finish(out, args, t0, ok_all):
    out["verified"] = ok_all
    out["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
