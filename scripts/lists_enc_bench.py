#!/usr/bin/env python
"""Measurement of the many-lists encode (tpf_p4nenc256v32_lists); recorded in
profiles/lists_enc_bench.json, not gated.  Streams and timing are
scripts/lists_bench.py's: warm-up, HIP events around every call on the launch
stream, median over the steps; every call is given its buffers (nunits, out,
offsets, workspace), so nothing in a timed step synchronises.

(a) one list: the C3 posting list of bench_data.py at the bench's default size
    as a single list -- the lists call against tpf_p4d1enc256v32_batch chained
    (no starts: bench.py's c3enc path) in the same process.
(b) Zipf lists: the same values cut into lists_bench.zipf_lengths' lists, list
    j chained from the value before it.  The one-call output is asserted equal,
    bytes and offsets, to lists_bench.build_lists_stream's (composed from the
    batch encoders, which the tests pin to the reference).
(c) the first SUBSET lists: one call against a loop of tpf_p4nenc256v32, one
    call per list.

    python scripts/lists_enc_bench.py [--nblocks N] [--steps K] [--warmup W] [--no-loop] [--no-one-list] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_data  # noqa: E402
from lists_bench import SUBSET, ZIPF_MAX, ZIPF_S, build_lists_stream, rate, timed, zipf_lengths  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true", help="skip the per-list loop (profiling runs)")
    ap.add_argument("--no-one-list", action="store_true", help="skip the one-list comparison (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_enc_bench.json"))
    args = ap.parse_args()
    import turbopfor_amd as tpf

    dev = "cuda:0"
    nb, nv = args.nblocks, args.nblocks * 256
    res = {"nblocks": nb, "values": nv, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "kernel_md5": tpf.kernel_md5()}
    t0 = time.time()
    vals, _ = bench_data.gen_c3(nb, seed=7, dev=dev)
    flat = vals.view(-1)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    L = tpf.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok_a = True

    # ---- (a) one list
    if not args.no_one_list:
        ptr1 = torch.tensor([0, nv], dtype=torch.int64, device=dev)
        cap = max(tpf.lists_enc_bound(nv, 1), int(L.tpf_p4enc256v32_bound(nb)))
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        ref = torch.empty(cap, dtype=torch.uint8, device=dev)
        offs = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        roffs = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(int(L.tpf_p4nenc256v32_lists_workspace_size(nb, 1)), dtype=torch.uint8, device=dev)
        bws = torch.empty(int(L.tpf_p4enc256v32_workspace_size(nb)), dtype=torch.uint8, device=dev)

        def one_list():
            tpf.encn256v32_lists(flat, ptr1, d1=True, nunits=nb, out=out, offsets=offs, ws=ws)

        def chained():
            rc = L.tpf_p4d1enc256v32_batch(flat.data_ptr(), nb, None, ctypes.c_uint32(0), ref.data_ptr(), cap, roffs.data_ptr(),
                                           bws.data_ptr(), bws.numel(), s)
            assert rc == 0

        tpf.encn256v32_lists(flat, ptr1, d1=True, nunits=nb, out=out, offsets=offs, err=err, ws=ws)
        chained()
        total = int(roffs[-1].item())
        ok_a = int(err.item()) == -1 and bool(torch.equal(offs, roffs)) and bool(torch.equal(out[:total], ref[:total]))
        t_lists = timed(one_list, args.steps, args.warmup)
        t_chain = timed(chained, args.steps, args.warmup)
        res["one_list"] = {"verified": ok_a, "lists": t_lists, "chained_batch": t_chain, "lists_G_int32_s": rate(nv, t_lists),
                           "chained_batch_G_int32_s": rate(nv, t_chain),
                           "ratio_lists_over_chained": round(t_chain["ms_median"] / t_lists["ms_median"], 4),
                           "bytes_per_int": round(total / nv, 4),
                           "stream": "bench_data.gen_c3(nblocks, seed=7), one list, start0 = 0"}
        print("[lists_enc_bench] one list:", json.dumps(res["one_list"]), flush=True)
        del out, ref, offs, roffs, ws, bws

    # ---- (b) Zipf lists over the same values
    ptr = zipf_lengths(nv, 7, dev)
    nl = ptr.numel() - 1
    enc_full = lambda v, st: tpf.enc256v32(v, d1=True, starts=st)
    enc_tail = lambda v, w, st: tpf.enc_batch("32", v.reshape(-1), v.shape[0], w, d1=True, starts=st)
    rpacked, roffs, start0 = build_lists_stream(flat, ptr, enc_full, enc_tail)
    nu = roffs.numel() - 1
    total = rpacked.numel()
    ln = ptr[1:] - ptr[:-1]
    cap = tpf.lists_enc_bound(nv, nl)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(nu + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.tpf_p4nenc256v32_lists_workspace_size(nu, nl)), dtype=torch.uint8, device=dev)
    tpf.encn256v32_lists(flat, ptr, d1=True, start0=start0, nunits=nu, out=out, offsets=offs, err=err, ws=ws)
    ok_b = int(err.item()) == -1 and bool(torch.equal(offs, roffs)) and bool(torch.equal(out[:total], rpacked))
    assert ok_b, "the one-call stream differs from build_lists_stream's"
    t_all = timed(lambda: tpf.encn256v32_lists(flat, ptr, d1=True, start0=start0, nunits=nu, out=out, offsets=offs, ws=ws),
                  args.steps, args.warmup)
    res["zipf"] = {"verified_equal_to_build_lists_stream": ok_b,
                   "generator": f"bounded Zipf(s={ZIPF_S}) on [1, {ZIPF_MAX}], floored, splitmix64 per list (key seed*1000+911, seed 7)",
                   "lists": nl, "units": nu, "tails": int((ln % 256 != 0).sum().item()), "tail_only_lists": int((ln < 256).sum().item()),
                   "longest": int(ln.max().item()), "median_len": int(ln.median().item()), "bytes_per_int": round(total / nv, 4),
                   "bound_bytes": cap, "workspace_bytes": ws.numel(), "all": t_all, "all_G_int32_s": rate(nv, t_all)}
    print("[lists_enc_bench] zipf, all lists:", json.dumps(res["zipf"]), flush=True)

    # ---- (c) the first SUBSET lists: one call against one call per list
    ns = min(SUBSET, nl)
    hp = ptr[: ns + 1].cpu().numpy()
    hn = np.diff(hp)
    units = hn // 256 + (hn % 256 != 0)
    ub = np.concatenate([[0], np.cumsum(units)])
    sub_nu, sub_nv = int(ub[-1]), int(hp[-1])
    sub_ptr = ptr[: ns + 1]
    sub_bytes = int(roffs[sub_nu].item())
    out[:sub_bytes + 64].zero_()
    t_sub = timed(lambda: tpf.encn256v32_lists(flat[:sub_nv], sub_ptr, d1=True, start0=start0, nunits=sub_nu, out=out,
                                               offsets=offs[: sub_nu + 1], ws=ws), args.steps, args.warmup)
    ok_sub = bool(torch.equal(offs[: sub_nu + 1], roffs[: sub_nu + 1])) and bool(torch.equal(out[:sub_bytes], rpacked[:sub_bytes]))
    res["zipf_subset"] = {"lists": ns, "units": sub_nu, "values": sub_nv, "verified": ok_sub, "one_call": t_sub,
                          "one_call_G_int32_s": rate(sub_nv, t_sub)}
    ok_loop = True
    if not args.no_loop:
        # every list into its own slice of a bound-sized buffer, its offsets into its own nunits_j + 1 entries
        bounds = np.array([int(L.tpf_p4nenc256v32_bound(int(n))) for n in hn], dtype=np.int64)
        bbase = np.concatenate([[0], np.cumsum(bounds)])
        lout = torch.empty(int(bbase[-1]), dtype=torch.uint8, device=dev)
        loffs = torch.zeros(sub_nu + ns + 1, dtype=torch.int64, device=dev)
        lws = torch.empty(int(L.tpf_p4nenc256v32_workspace_size(int(hn.max()))), dtype=torch.uint8, device=dev)
        hs0 = start0[:ns].cpu().numpy().view(np.uint32)
        calls = [(flat.data_ptr() + 4 * int(hp[j]), int(hn[j]), ctypes.c_uint32(int(hs0[j])), lout.data_ptr() + int(bbase[j]), int(bounds[j]),
                  loffs.data_ptr() + 8 * (int(ub[j]) + j)) for j in range(ns)]
        f, pws, nws = L.tpf_p4nenc256v32, lws.data_ptr(), lws.numel()

        def loop():
            for src, n, st, dst, cp, o in calls:
                f(src, n, 1, st, dst, cp, o, pws, nws, s)

        t_loop = timed(loop, min(args.steps, 5), 1)
        # the loop's streams, list by list, against the one call's (a sample: the first, the last, the longest)
        ho = loffs.cpu().numpy()
        for j in sorted({0, ns - 1, int(np.argmax(hn))}):
            lo = int(roffs[int(ub[j])].item())
            sz = int(ho[int(ub[j + 1]) + j])
            ok_loop = ok_loop and bool(torch.equal(lout[int(bbase[j]): int(bbase[j]) + sz], rpacked[lo: lo + sz]))
        res["zipf_subset"].update({"per_list_loop": t_loop, "per_list_loop_G_int32_s": rate(sub_nv, t_loop), "loop_sample_verified": ok_loop,
                                   "speedup": round(t_loop["ms_median"] / t_sub["ms_median"], 1)})
    print("[lists_enc_bench] zipf, first lists:", json.dumps(res["zipf_subset"]), flush=True)
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0 if (ok_a and ok_b and ok_sub and ok_loop) else 1


if __name__ == "__main__":
    sys.exit(main())
