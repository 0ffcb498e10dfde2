#!/usr/bin/env python
"""Measurement of opening a lists stream that has no offsets
(tpf_lists_unit_offsets against the host scan tpf_lists_scan_offsets);
recorded in profiles/lists_scan_bench.json, not gated.  Timed the way bench.py
times its steps (scripts/lists_bench.py's `timed`): warm-up, HIP events around
every call on the launch stream, median over the steps.  All legs in one
process on one box, on the delta-1 Zipf(1.5) index of
scripts/lists_select_bench.py, whose own offsets are the expected result.

(a) the device call: list_ptr and list_byte (lists_list_byte of the index's
    offsets) in, d_off and d_list_unit out, checked entry by entry.
(b) the host way: tpf_lists_scan_offsets over the same bytes in host memory
    (one thread, wall clock, with the anchors and without) plus the upload of
    its 8 bytes per unit.
(c) tpf_lists_unit_last on the same index: a pass that also reads the whole
    index once, as a yardstick.
(d) the dependent-chain floor: the same values as ONE list, whose walk is one
    wave and one step per unit; the time per step is what the longest list of
    any index costs.  One timed call (--one-list-blocks 0 skips it).

    python scripts/lists_scan_bench.py [--nblocks N] [--steps K] [--warmup W] [--one-list-blocks M] [--out FILE]
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


def device_leg(tpf, L, ix, steps, warmup):
    """-> (verified, timing, workspace bytes, list_byte) of tpf_lists_unit_offsets on index ix"""
    dev = ix.packed.device
    lbyte = tpf.lists_list_byte(ix.offs, ix.unit)
    off = torch.zeros(ix.nu + 1, dtype=torch.int64, device=dev)
    unit = torch.zeros(ix.nl + 1, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.tpf_lists_unit_offsets_workspace_size(ix.nu, ix.nl)), dtype=torch.uint8, device=dev)
    call = lambda e=None: tpf.lists_unit_offsets(ix.packed, ix.ptr, lbyte, nunits=ix.nu, out=off, list_unit=unit, err=e, ws=ws)
    call(err)
    ok = int(err.item()) == -1 and bool(torch.equal(off, ix.offs)) and bool(torch.equal(unit, ix.unit))
    return ok, lb.timed(call, steps, warmup), ws.numel(), lbyte


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nblocks", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--one-list-blocks", type=int, default=None, help="blocks of the one-list leg (default: --nblocks; 0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_scan_bench.json"))
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
    ix = Index(tpf, flat, ptr, True)
    units = (ptr[1:] - ptr[:-1] + 255) // 256
    res.update({"lists": ix.nl, "units": ix.nu, "stream_bytes": ix.packed.numel(), "lists_of_one_unit": int((units == 1).sum().item()),
                "lists_walked": int((units >= 2).sum().item()), "longest_list_units": int(units.max().item())})

    # ---- (a) the device call
    ok_a, t_dev, ws_bytes, lbyte = device_leg(tpf, L, ix, args.steps, args.warmup)
    res["device_call"] = {"verified": ok_a, "unit_offsets": t_dev, "workspace_bytes": ws_bytes, "offsets_bytes": 8 * (ix.nu + 1),
                     "units_per_us": round(ix.nu / (t_dev["ms_median"] * 1e3), 2)}
    print("[lists_scan_bench] device:", json.dumps(res["device_call"]), flush=True)

    # ---- (b) the host scan and the upload of its offsets
    h_in, h_ptr, h_lb = ix.packed.cpu().numpy(), ptr.cpu().numpy().astype(np.uint64), lbyte.cpu().numpy().astype(np.uint64)
    h_off = np.zeros(ix.nu + 1, dtype=np.uint64)
    host = {}
    for name, anchors in (("with_list_byte", h_lb), ("chained_from_byte_0", None)):
        a = time.perf_counter()
        r = L.tpf_lists_scan_offsets(h_in.ctypes.data, h_in.size, h_ptr.ctypes.data, ix.nl, None if anchors is None else anchors.ctypes.data,
                                     h_off.ctypes.data, ix.nu)
        host[name + "_ms"] = round((time.perf_counter() - a) * 1e3, 2)
        host[name + "_verified"] = r == ix.packed.numel() and bool(np.array_equal(h_off.view(np.int64), ix.offs.cpu().numpy()))
    pinned = torch.from_numpy(h_off.view(np.int64)).pin_memory()
    d_off = torch.empty(ix.nu + 1, dtype=torch.int64, device=dev)
    host["upload_pinned"] = lb.timed(lambda: d_off.copy_(pinned, non_blocking=True), args.steps, args.warmup)
    host["scan_plus_upload_ms"] = round(host["with_list_byte_ms"] + host["upload_pinned"]["ms_median"], 2)
    host["host_over_device_time"] = round(host["scan_plus_upload_ms"] / t_dev["ms_median"], 1)
    res["host"] = host
    ok_b = host["with_list_byte_verified"] and host["chained_from_byte_0_verified"]
    del h_in, pinned, d_off
    print("[lists_scan_bench] host:", json.dumps(host), flush=True)

    # ---- (c) the skip-table build on the same index
    table = torch.zeros(ix.nu, dtype=torch.int32, device=dev)
    tws = torch.empty(int(L.tpf_lists_unit_last_workspace_size(ix.nu, ix.nl)), dtype=torch.uint8, device=dev)
    t_tab = lb.timed(lambda: tpf.lists_unit_last(ix.packed, ix.offs, ptr, start0=ix.start0, out=table, ws=tws), args.steps, args.warmup)
    res["unit_last"] = {"unit_last": t_tab, "unit_offsets_over_unit_last_time": round(t_dev["ms_median"] / t_tab["ms_median"], 3)}
    del table, tws, ix
    print("[lists_scan_bench] unit_last:", json.dumps(res["unit_last"]), flush=True)

    # ---- (d) one list: the dependent chain
    ok_d = True
    ob = nb if args.one_list_blocks is None else args.one_list_blocks
    if ob:
        one = Index(tpf, flat[: ob * 256], torch.tensor([0, ob * 256], dtype=torch.int64, device=dev), True)
        ok_d, t_one, _, _ = device_leg(tpf, L, one, 1, 0)
        res["one_list"] = {"verified": ok_d, "blocks": ob, "units": one.nu, "stream_bytes": one.packed.numel(), "unit_offsets": t_one,
                           "us_per_step": round(t_one["ms_median"] * 1e3 / one.nu, 4)}
        print("[lists_scan_bench] one list:", json.dumps(res["one_list"]), flush=True)

    res["verified"] = bool(ok_a and ok_b and ok_d)
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0 if res["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
