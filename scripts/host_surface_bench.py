#!/usr/bin/env python
"""Host time per call of the launch-bound entry points (DESIGN.md 4.14 names
them), binding included; recorded in profiles/host_surface_ab.json, not gated.
What a change of the binding or of capi.cpp can move is the time the host
spends per call, so every leg is timed by the host's clock around a run of
calls on preallocated buffers: `host_us` is the time to enqueue one call,
`wall_us` the time per call once the stream has drained.  Median over the
rounds.  One process, one box.

Legs, on a small delta-1 index of 4,096 lists plus one list of 2M values:
  select_1 / select_64   decn256v32_lists_select of 1 and of 64 lists
  gather_dense           lists_gather of every position of the long list
  intersect_spread       lists_intersect, 4,096 queries of 128 values spread over their targets
  decn_short             decn256v32 of one list of 1,000 values

An A/B of two builds runs this once per build and process, alternately:
TPF_LIB names the library, --binding the directory turbopfor_amd.py is
imported from (default: the tree's).  The host's clock drifts between
processes by more than a binding can cost, so --against DIR:LIB loads a second
binding and library into the same process and times the two sides alternately,
round by round, each on buffers of its own.

    python scripts/host_surface_bench.py [--calls N] [--rounds R] [--warmup W] [--binding DIR] [--against DIR:LIB] [--out FILE]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_lists(rng):
    """4,096 lists of 1 .. 3,000 values and one of 2M, ascending doc ids: (values uint32, ptr int64)"""
    n = np.minimum((rng.zipf(1.3, 4096) * 40) % 3000 + 1, 3000).astype(np.int64)
    n[::8] = np.maximum(n[::8], 200)  # every eighth list can take a spread probe of 128 values
    n = np.append(n, 1 << 21)
    ptr = np.zeros(n.size + 1, dtype=np.int64)
    np.cumsum(n, out=ptr[1:])
    gaps = rng.integers(1, 17, int(ptr[-1]), dtype=np.int64)
    vals = np.cumsum(gaps)
    vals -= np.repeat(vals[ptr[:-1]] - gaps[ptr[:-1]], n)  # every list restarts from its own first gap
    assert int(vals.max()) < 1 << 31
    return vals.astype(np.uint32), ptr


def timed(fns, calls, rounds, warmup):
    """fns: the same leg of every side; the sides take turns within each round"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    host, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[i].append((t1 - t0) / calls * 1e6)
            wall[i].append((t2 - t0) / calls * 1e6)
    return [{"host_us": round(statistics.median(h), 3), "wall_us": round(statistics.median(w), 3),
             "host_us_rounds": [round(x, 3) for x in h], "wall_us_rounds": [round(x, 3) for x in w]} for h, w in zip(host, wall)]


def load(binding_dir, lib_path, name):
    """turbopfor_amd.py of binding_dir as module `name`, over lib_path (None: the binding's own choice)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(binding_dir, "turbopfor_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if lib_path:
        mod.LIB_PATH = lib_path
    return mod


def make_legs(tpf, vals, ptr, dev):
    """the five legs on one side's binding and buffers: ({name: call}, {name: check}, err)"""
    rng = np.random.default_rng(12)
    nl = ptr.size - 1
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).to(dev)
    flat, lptr = i32(vals), torch.from_numpy(ptr).to(dev)
    packed, offs = tpf.encn256v32_lists(flat, lptr, d1=True)
    lunit = tpf.lists_unit_base(lptr)
    ulast = tpf.lists_unit_last(packed, offs, lptr)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    legs, checks = {}, {}

    def select_leg(name, sel_np):
        sel = i32(sel_np)
        total = int((ptr[sel_np + 1] - ptr[sel_np]).sum())
        out = torch.empty(total, dtype=torch.int32, device=dev)
        optr = torch.empty(sel_np.size + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(int(tpf.lib().tpf_p4ndec256v32_lists_select_workspace_size(sel_np.size, total)), dtype=torch.uint8, device=dev)
        legs[name] = lambda: tpf.decn256v32_lists_select(packed, offs, lptr, lunit, sel, d1=True, out=out, out_ptr=optr, err=err, ws=ws)
        want = np.concatenate([vals[ptr[j]:ptr[j + 1]] for j in sel_np])
        checks[name] = lambda: np.array_equal(out.cpu().numpy().view(np.uint32), want)

    select_leg("select_1", np.array([8], dtype=np.int64))
    select_leg("select_64", rng.choice(nl - 1, 64, replace=False).astype(np.int64))

    # every position of the long list
    npos = int(ptr[nl] - ptr[nl - 1])
    pos = torch.arange(npos, dtype=torch.int32, device=dev)
    pptr = torch.tensor([0, npos], dtype=torch.int64, device=dev)
    ql = i32(np.array([nl - 1]))
    gout = torch.empty_like(pos)
    gws = torch.empty(int(tpf.lib().tpf_lists_gather_workspace_size(1, npos)), dtype=torch.uint8, device=dev)
    legs["gather_dense"] = lambda: tpf.lists_gather(packed, offs, lptr, lunit, pos, pptr, ql, d1=True, unit_last=ulast, out=gout, err=err,
                                                    ws=gws)
    checks["gather_dense"] = lambda: np.array_equal(gout.cpu().numpy().view(np.uint32), vals[ptr[nl - 1]:])

    # 4,096 queries of 128 values spread over the whole of their targets: 64 members and 64 values one above a member
    targets = np.arange(0, nl - 1, 8)[rng.integers(0, (nl - 1) // 8, 4096)]
    probe_np = np.empty((4096, 128), dtype=np.uint32)
    for k, j in enumerate(targets):
        m = vals[ptr[j]:ptr[j + 1]][np.linspace(0, ptr[j + 1] - ptr[j] - 1, 64).astype(np.int64)]
        probe_np[k, 0::2], probe_np[k, 1::2] = m, m + 1
    probe = i32(probe_np.reshape(-1))
    qptr = torch.arange(0, 4096 * 128 + 1, 128, dtype=torch.int64, device=dev)
    qlist = i32(targets)
    iout = torch.empty_like(probe)
    ioptr = torch.empty(4097, dtype=torch.int64, device=dev)
    iws = torch.empty(int(tpf.lib().tpf_lists_intersect_workspace_size(4096, probe.numel())), dtype=torch.uint8, device=dev)
    legs["intersect_spread"] = lambda: tpf.lists_intersect(packed, offs, lptr, lunit, ulast, probe, qptr, qlist, out=iout, out_ptr=ioptr,
                                                           err=err, ws=iws)

    def check_intersect():
        o, op = iout.cpu().numpy().view(np.uint32), ioptr.cpu().numpy()
        return all(np.array_equal(o[op[k]:op[k + 1]], probe_np[k][np.isin(probe_np[k], vals[ptr[j]:ptr[j + 1]])])
                   for k, j in enumerate(targets[:256]))

    checks["intersect_spread"] = check_intersect

    # one short list through the single-list entry point
    short = vals[ptr[8]:ptr[8] + 1000] if ptr[9] - ptr[8] >= 1000 else vals[ptr[nl - 1]:ptr[nl - 1] + 1000]
    sp, so = tpf.encn256v32(i32(short), d1=True)
    sout = torch.empty(1000, dtype=torch.int32, device=dev)
    sws = torch.empty(int(tpf.lib().tpf_p4ndec256v32_workspace_size(1000)), dtype=torch.uint8, device=dev)
    legs["decn_short"] = lambda: tpf.decn256v32(sp, so, 1000, d1=True, out=sout, err=err, ws=sws)
    checks["decn_short"] = lambda: np.array_equal(sout.cpu().numpy().view(np.uint32), short)

    return legs, checks, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--binding", default=os.path.join(ROOT, "turbopfor-cpp_amd", "python"))
    ap.add_argument("--against", default=None, help="DIR:LIB of a second binding and library, timed alternately in this process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mods = [load(args.binding, None, "tpf_side0")]
    if args.against:
        mods.append(load(*args.against.split(":"), "tpf_side1"))
    dev = "cuda:0"
    vals, ptr = build_lists(np.random.default_rng(11))
    sides = [make_legs(m, vals, ptr, dev) for m in mods]
    rel = lambda f: os.path.relpath(os.path.realpath(f), ROOT)
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "rounds": args.rounds,
           "sides": [{"library": rel(m.LIB_PATH), "binding": rel(m.__file__), "legs": {}} for m in mods]}
    ok_all = True
    for name in sides[0][0]:
        rs = timed([legs[name] for legs, _, _ in sides], args.calls, args.rounds, args.warmup)
        torch.cuda.synchronize()
        for side, (_, checks, err), r in zip(res["sides"], sides, rs):
            r["verified"] = bool(checks[name]()) and int(err.item()) == -1
            ok_all &= r["verified"]
            side["legs"][name] = r
            print(f"[host_surface_bench] {side['binding']} {name}: host {r['host_us']} us, wall {r['wall_us']} us, "
                  f"verified {r['verified']}", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
