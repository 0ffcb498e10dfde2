#!/usr/bin/env python
"""Measurement of the many-lists decode (tpf_p4ndec256v32_lists); recorded in
profiles/lists_bench.json, not gated.  Timed the way bench.py times its steps:
warm-up, HIP events around every call on the launch stream, median over the
steps.

(a) one list: the C3 posting list of bench_data.py at the bench's default size
    as a single list -- the lists call against tpf_p4d1dec256v32_chained (the
    parent commit's way to decode one list) in the same process.
(b) Zipf lists: the same values cut into consecutive lists whose lengths are
    bounded Zipf(s = ZIPF_S) on [1, ZIPF_MAX] (floored; inverse CDF of a
    counter-keyed splitmix64 draw per list, bench_data.rand64 under key
    seed * 1000 + 911), tails included.  List j is chained from the value
    before it.  The lists call on all of it; on the first SUBSET lists also
    the lists call against a loop of tpf_p4ndec256v32, one call per list (the
    only way to do the job at the parent commit).

    python scripts/lists_bench.py [--nblocks N] [--steps K] [--warmup W] [--no-loop] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "turbopfor-cpp_amd", "python"))

import bench_data  # noqa: E402

ZIPF_S = 1.5
ZIPF_MAX = 1 << 20
SUBSET = 20_000


def zipf_lengths(total, seed, dev):
    """Consecutive list lengths adding up to `total` values (the last list is
    cut to fit): list j's length from a counter-keyed draw, so any prefix of
    the lists is reproducible on its own."""
    s = ZIPF_S
    lens = []
    have, j0 = 0, 0
    while have < total:
        m = 1 << 22
        idx = torch.arange(j0, j0 + m, dtype=torch.int64, device=dev)
        r = bench_data.rand64(idx, seed * 1000 + 911)
        u = bench_data._srl(r, 11).to(torch.float64) * (1.0 / (1 << 53))
        x = (1.0 + u * (float(ZIPF_MAX + 1) ** (1 - s) - 1.0)) ** (1.0 / (1 - s))
        ln = torch.clamp(torch.floor(x), 1, ZIPF_MAX).to(torch.int64)
        lens.append(ln)
        have += int(ln.sum().item())
        j0 += m
    ln = torch.cat(lens)
    ends = torch.cumsum(ln, 0)
    nl = int(torch.searchsorted(ends, torch.tensor([total], device=dev, dtype=torch.int64)).item()) + 1
    ptr = torch.zeros(nl + 1, dtype=torch.int64, device=dev)
    ptr[1:] = ends[:nl]
    ptr[nl] = total
    return ptr


def _gather_rows(flat, pos, width, chunk=1 << 20):
    """rows[i] = flat[pos[i] : pos[i] + width], gathered in chunks of rows"""
    out = torch.empty((pos.numel(), width), dtype=flat.dtype, device=flat.device)
    ar = torch.arange(width, dtype=torch.int64, device=flat.device)
    for a in range(0, pos.numel(), chunk):
        p = pos[a:a + chunk]
        out[a:a + chunk] = flat[(p[:, None] + ar[None, :]).reshape(-1)].view(-1, width)
    return out


def _before(flat, pos):
    """value before position pos (0 before position 0), int32 bit patterns"""
    st = flat[torch.clamp(pos - 1, min=0)].clone()
    st[pos == 0] = 0
    return st


def build_lists_stream(flat, ptr, enc_full, enc_tail, byte_chunk=256 << 20):
    """The lists stream of the consecutive slices flat[ptr[j]:ptr[j+1]], every
    list chained from the value before it: full blocks through enc_full(values
    [nb,256], starts) and the tails of n values through enc_tail(values [k,n],
    n, starts), each -> (packed, offsets); then the units are laid out in list
    order.  -> (packed, offsets [nunits+1], start0 [nlists])."""
    dev = flat.device
    n = ptr[1:] - ptr[:-1]
    nfull, tail = n // 256, n % 256
    units = nfull + (tail != 0).to(torch.int64)
    ubase = torch.cumsum(units, 0) - units
    nunits = int(units.sum().item())
    fbase = torch.cumsum(nfull, 0) - nfull
    nf = int(nfull.sum().item())
    unit_len = torch.zeros(nunits, dtype=torch.int64, device=dev)
    unit_src = torch.zeros(nunits, dtype=torch.int64, device=dev)
    parts, src0 = [], 0
    if nf:
        lst = torch.repeat_interleave(torch.arange(n.numel(), device=dev), nfull)
        f = torch.arange(nf, dtype=torch.int64, device=dev)
        k = f - fbase[lst]
        pos = ptr[:-1][lst] + 256 * k
        packed, offs = enc_full(_gather_rows(flat, pos, 256), _before(flat, pos))
        u = ubase[lst] + k
        unit_len[u] = offs[1:] - offs[:-1]
        unit_src[u] = offs[:-1] + src0
        parts.append(packed)
        src0 += packed.numel()
        del lst, f, k, pos, u
    for w in range(1, 256):
        js = torch.nonzero(tail == w).view(-1)
        if js.numel() == 0:
            continue
        pos = ptr[1:][js] - w
        packed, offs = enc_tail(_gather_rows(flat, pos, w), w, _before(flat, pos))
        u = ubase[js] + nfull[js]
        unit_len[u] = offs[1:] - offs[:-1]
        unit_src[u] = offs[:-1] + src0
        parts.append(packed)
        src0 += packed.numel()
    src = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.uint8, device=dev)
    del parts
    offsets = torch.zeros(nunits + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(unit_len, 0)
    total = int(offsets[-1].item())
    dst = torch.empty(total, dtype=torch.uint8, device=dev)
    shift = unit_src - offsets[:-1]
    a = 0
    while a < nunits:
        lim = offsets[a] + byte_chunk
        b = max(a + 1, int(torch.searchsorted(offsets, lim.view(1), right=True).item()) - 1)
        b = min(b, nunits)
        lo, hi = int(offsets[a].item()), int(offsets[b].item())
        idx = torch.repeat_interleave(shift[a:b], unit_len[a:b]) + torch.arange(lo, hi, dtype=torch.int64, device=dev)
        dst[lo:hi] = src[idx]
        a = b
    return dst, offsets, _before(flat, ptr[:-1])


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in evs:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4)}


def rate(nvalues, t):
    return round(nvalues / (t["ms_median"] * 1e-3) / 1e9, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true", help="skip the per-list loop (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_bench.json"))
    args = ap.parse_args()
    import turbopfor_amd as tpf

    dev = "cuda:0"
    nb, nv = args.nblocks, args.nblocks * 256
    res = {"nblocks": nb, "values": nv, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "kernel_md5": tpf.kernel_md5()}
    t0 = time.time()
    vals, starts = bench_data.gen_c3(nb, seed=7, dev=dev)
    flat = vals.view(-1)
    out = torch.empty(nv, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)

    # ---- (a) one list
    packed, offs = tpf.enc256v32(vals, d1=True, starts=starts)
    packed = packed.clone()
    ptr1 = torch.tensor([0, nv], dtype=torch.int64, device=dev)
    L = tpf.lib()
    ws = torch.empty(int(L.tpf_p4ndec256v32_lists_workspace_size(nb, 1)), dtype=torch.uint8, device=dev)
    cws = torch.empty(int(L.tpf_p4d1dec256v32_chain_workspace_size(nb)), dtype=torch.uint8, device=dev)
    tpf.decn256v32_lists(packed, offs, ptr1, d1=True, out=out, err=err, ws=ws)
    ok_a = bool(torch.equal(out, flat)) and int(err.item()) == -1
    out.zero_()
    t_lists = timed(lambda: tpf.decn256v32_lists(packed, offs, ptr1, d1=True, out=out, ws=ws), args.steps, args.warmup)
    t_chain = timed(lambda: tpf.dec256v32_chained(packed, offs, nb, 0, out=out.view(nb, 256), ws=cws), args.steps, args.warmup)
    res["one_list"] = {"verified": ok_a, "lists": t_lists, "chained": t_chain, "lists_G_int32_s": rate(nv, t_lists),
                       "chained_G_int32_s": rate(nv, t_chain), "ratio_lists_over_chained": round(t_chain["ms_median"] / t_lists["ms_median"], 4),
                       "stream": "bench_data.gen_c3(nblocks, seed=7), one list, start0 = 0"}
    print("[lists_bench] one list:", json.dumps(res["one_list"]), flush=True)
    del packed, offs, ws, cws

    # ---- (b) Zipf lists over the same values
    ptr = zipf_lengths(nv, 7, dev)
    nl = ptr.numel() - 1
    enc_full = lambda v, st: tpf.enc256v32(v, d1=True, starts=st)
    enc_tail = lambda v, w, st: tpf.enc_batch("32", v.reshape(-1), v.shape[0], w, d1=True, starts=st)
    packed, offs, start0 = build_lists_stream(flat, ptr, enc_full, enc_tail)
    nu = offs.numel() - 1
    ln = (ptr[1:] - ptr[:-1])
    ws = torch.empty(int(L.tpf_p4ndec256v32_lists_workspace_size(nu, nl)), dtype=torch.uint8, device=dev)
    out.zero_()
    tpf.decn256v32_lists(packed, offs, ptr, d1=True, start0=start0, out=out, err=err, ws=ws)
    ok_b = bool(torch.equal(out, flat)) and int(err.item()) == -1
    t_all = timed(lambda: tpf.decn256v32_lists(packed, offs, ptr, d1=True, start0=start0, out=out, ws=ws), args.steps, args.warmup)
    res["zipf"] = {"verified": ok_b, "generator": f"bounded Zipf(s={ZIPF_S}) on [1, {ZIPF_MAX}], floored, splitmix64 per list (key seed*1000+911, seed 7)",
                   "lists": nl, "units": nu, "tails": int((ln % 256 != 0).sum().item()), "tail_only_lists": int((ln < 256).sum().item()),
                   "longest": int(ln.max().item()), "median_len": int(ln.median().item()), "bytes_per_int": round(packed.numel() / nv, 4),
                   "all": t_all, "all_G_int32_s": rate(nv, t_all)}
    print("[lists_bench] zipf, all lists:", json.dumps(res["zipf"]), flush=True)

    # ---- the first SUBSET lists: one call against one call per list
    ns = min(SUBSET, nl)
    hp = ptr[: ns + 1].cpu().numpy()
    units = np.diff(hp) // 256 + (np.diff(hp) % 256 != 0)
    ub = np.concatenate([[0], np.cumsum(units)])
    sub_nu, sub_nv = int(ub[-1]), int(hp[-1])
    sub_ptr, sub_offs = ptr[: ns + 1], offs[: sub_nu + 1]
    sub_bytes = int(sub_offs[-1].item())
    out.zero_()
    t_sub = timed(lambda: tpf.decn256v32_lists(packed[:sub_bytes], sub_offs, sub_ptr, d1=True, start0=start0, out=out[:sub_nv], ws=ws),
                  args.steps, args.warmup)
    ok_sub = bool(torch.equal(out[:sub_nv], flat[:sub_nv]))
    if args.no_loop:
        print(json.dumps(res))
        return 0 if (ok_a and ok_b and ok_sub) else 1
    out.zero_()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lws = torch.empty(int(L.tpf_p4ndec256v32_workspace_size(int(np.diff(hp).max()))), dtype=torch.uint8, device=dev)
    hs0 = start0[:ns].cpu().numpy().view(np.uint32)
    calls = [(offs.data_ptr() + 8 * int(ub[j]), int(hp[j + 1] - hp[j]), int(hs0[j]), out.data_ptr() + 4 * int(hp[j])) for j in range(ns)]
    f, pin, pws, nws = L.tpf_p4ndec256v32, packed.data_ptr(), lws.data_ptr(), lws.numel()

    def loop():
        for o, n, st, dst in calls:
            f(pin, sub_bytes, o, n, 1, st, dst, pws, nws, None, s)

    t_loop = timed(loop, args.steps, min(args.warmup, 2))
    ok_loop = bool(torch.equal(out[:sub_nv], flat[:sub_nv]))
    res["zipf_subset"] = {"lists": ns, "units": sub_nu, "values": sub_nv, "verified": ok_sub and ok_loop, "one_call": t_sub, "per_list_loop": t_loop,
                          "one_call_G_int32_s": rate(sub_nv, t_sub), "per_list_loop_G_int32_s": rate(sub_nv, t_loop),
                          "speedup": round(t_loop["ms_median"] / t_sub["ms_median"], 1)}
    print("[lists_bench] zipf, first lists:", json.dumps(res["zipf_subset"]), flush=True)
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0 if (ok_a and ok_b and ok_sub and ok_loop) else 1


if __name__ == "__main__":
    sys.exit(main())
