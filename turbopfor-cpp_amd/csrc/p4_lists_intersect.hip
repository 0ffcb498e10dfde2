// p4_lists_intersect.hip -- membership of probe doc ids in resident posting
// lists (p4_lists.h): tpf_lists_intersect takes sorted CSR
// segments of probe values, one target list per segment, and returns the
// values that are also in the target, with their positions.  Every probe value
// is looked up in the skip table (the first unit of its list whose last value
// is >= it); consecutive probe values that land in the same unit form an ITEM
// (p4_lists_items.hip), and every item's unit is decoded once -- by the item
// drivers (p4_lists_items.h), the start taken from the table -- into the
// wave's LDS, where the item's probe values are searched 64 at a time.  No
// decoded block goes to global memory.  Nothing here is sized by the index:
// grids and the workspace follow nq and probe_values.
#include "p4_lists.h"

#include "p4_lists_host.h"
#include "p4_lists_items.h"

namespace tpf::dev
{

constexpr uint32_t kIxMiss = kItemNone; // result word before the hits pass: not a member
constexpr uint32_t kIxHit = 0x100u;     // result word after the hits pass: bits 0-7 p, bit 8 hit, bits 16-22 hits before it in its run
// (EVERY, the union's lookup: every probe value of an item gets q | kIxFound, p4_lists.h)

// Full blocks (item_full_units): items per wave and chunks in flight.  A wave
// waits for its item's probe values once per block, so short runs over many
// waves hide the wait better than k_un_dec's 16 blocks per wave; DESIGN.md
// 4.11 has both timings.
constexpr uint32_t kIxRun = 4;
constexpr uint32_t kIxNC = 4;

// Plan.  One thread per QUERY: check_queries (p4_lists_dev.h).  One thread per
// PROBE INDEX: its query by a search over d_probe_ptr, that query's own checks
// again -- the verdict of the other threads is not known yet -- and the lower
// bound of the value over the list's slice of the skip table, as
// k_range_units does it.
__global__ __launch_bounds__(256) void k_ix_plan(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                                  uint64_t nunits, const uint32_t * __restrict unit_last,
                                                  const uint32_t * __restrict probe, uint64_t pv, const uint64_t * __restrict probe_ptr,
                                                  const uint32_t * __restrict qlist, uint64_t nq, ItemHdr * __restrict hdr,
                                                  uint32_t * __restrict pu, uint32_t * __restrict pl)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    check_queries(ptr, list_unit, nlists, nunits, probe_ptr, pv, qlist, nq, &hdr->bad, gid, gsz);
    for (uint64_t i = gid; i < pv; i += gsz)
    {
        uint32_t unit = kItemNone, list = kItemNone;
        const uint32_t k = segment_of(probe_ptr, nq, i);
        const uint32_t j = k != kItemNone ? qlist[k] : kItemNone;
        // (k_ix_plan keeps its own check here, the unit directory alone, not
        // list_dir_ok: the pointers are read only for a probe value that lands
        // in its list's last unit; read for every value they cost the dense
        // probe 1%, profiles/lists_refactor_ab.json)
        if (j < nlists)
        {
            const uint32_t ua = list_unit[j], ub = list_unit[j + 1u];
            if (ua <= ub && ub <= nunits)
            {
                const uint32_t v = probe[i];
                uint32_t a = ua, x = ub;
                while (a < x)
                {
                    const uint32_t m = a + (x - a) / 2u;
                    if (unit_last[m] >= v)
                        x = m;
                    else
                        a = m + 1u;
                }
                if (a < ub)
                {
                    // the list's last unit is a p4Enc32 tail when its length is no multiple of 256
                    const bool tail = a + 1u == ub && ((ptr[j + 1u] - ptr[j]) & 255u) != 0u;
                    unit = a | (tail ? kRecTail : 0u);
                    list = j;
                }
            }
        }
        pu[i] = unit;
        pl[i] = list;
    }
}

// The probe values [h, e) of one item against the 256 values the wave has just
// decoded into `vals` (entries past the unit's count hold 0xFFFFFFFF), 64 at a
// time: a lower bound over the block and an equality check, so a reported hit
// is an equality whatever the block holds.  EVERY (the union's lookup): the
// lower bound q, clamped to cnt, is recorded for every value, a member's with
// kIxFound.
template <bool EVERY>
__device__ __forceinline__ void ix_test(const uint32_t * vals, uint32_t cnt, const uint32_t * __restrict probe, uint32_t * __restrict res,
                                        uint32_t h, uint32_t e, uint32_t t)
{
    for (uint32_t c = h; c < e; c += 64u)
    {
        const uint32_t i = c + t;
        if (i < e)
        {
            const uint32_t v = probe[i];
            uint32_t pos = 0u;
#pragma unroll
            for (uint32_t step = 128u; step != 0u; step >>= 1)
                pos += vals[pos + step - 1u] < v ? step : 0u;
            const bool hit = pos < cnt && vals[pos] == v;
            if constexpr (EVERY)
                res[i] = umin32(pos, cnt) | (hit ? kIxFound : 0u);
            else
                res[i] = hit ? pos : kIxMiss;
        }
    }
}

// Full blocks and tails: the item drivers (p4_lists_items.h) with ix_test as
// what is done with an item's decoded unit.  A tail's words past its count
// hold 0xFFFFFFFF, so the lower bound of every value lies inside the count.
template <uint32_t RUN, uint32_t NC, int MINW, bool EVERY>
__global__ __launch_bounds__(256, MINW) void k_ix_dec(const IxArgs A)
{
    if (!items_go(A.it.hdr))
        return;
    constexpr uint32_t kRun = RUN;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 4u * kRun;
    item_full_units<true, RUN, NC>(A.it, stride, [&](const uint32_t * vals, uint32_t cnt, uint32_t h, uint32_t e, uint32_t t) {
        ix_test<EVERY>(vals, cnt, A.probe, A.res, h, e, t);
    });
}

template <uint32_t NC, bool EVERY>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_ix_tails(const IxArgs A)
{
    if (!items_go(A.it.hdr))
        return;
    item_tail_units<true, NC>(A.it, 0xFFFFFFFFu, [&](const uint32_t * vals, uint32_t cnt, uint32_t h, uint32_t e, uint32_t t) {
        ix_test<EVERY>(vals, cnt, A.probe, A.res, h, e, t);
    });
}

// Hits: every wave owns 64 consecutive probe indices again; the hit flags'
// total goes to the second run scan, and the result word is rewritten as
// p | kIxHit | (hits before it in its run) << 16, or 0 for a miss with the
// same count, so the compaction reads one word per index.
__global__ __launch_bounds__(256) void k_ix_hits(uint64_t pv, const ItemHdr * __restrict hdr, uint32_t * __restrict res,
                                                  uint32_t * __restrict tot)
{
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    const uint32_t r = (i < pv && items_go(hdr)) ? res[i] : kIxMiss;
    const uint32_t hit = r != kIxMiss ? 1u : 0u;
    const uint32_t incl = wave_incl_scan(hit);
    if (i < pv)
        res[i] = (hit != 0u ? (r & 255u) | kIxHit : 0u) | ((incl - hit) << 16);
    if (t == 0)
        tot[run] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
}

// hits at probe indices below p
__device__ __forceinline__ uint32_t ix_prefix(const uint32_t * __restrict res, const uint32_t * __restrict pre,
                                              const uint32_t * __restrict tile, uint64_t p)
{
    return run_base(pre, tile, p / 64u) + (res[p] >> 16);
}

// Compaction: the verdict (a refused query; hits that do not fit, by
// atomicMin under a parse error the probe kernels may have left), d_out_ptr[k]
// = the hits before probe_ptr[k], then every hit's value, probe index and
// list position scattered to its place.
__global__ __launch_bounds__(256) void k_ix_out(const uint32_t * __restrict list_unit, uint64_t nunits, const uint32_t * __restrict probe,
                                                uint64_t pv, const uint64_t * __restrict probe_ptr, uint64_t nq,
                                                const ItemHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                const uint32_t * __restrict pl, const uint32_t * __restrict res,
                                                const uint32_t * __restrict pre, const uint32_t * __restrict tile,
                                                uint32_t * __restrict out, uint64_t out_values, uint64_t * __restrict out_ptr,
                                                uint32_t * __restrict out_pidx, uint32_t * __restrict out_tpos,
                                                unsigned long long * __restrict err)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    if (!items_go(hdr))
    {
        if (gid == 0 && err != nullptr)
            *err = nunits + hdr->bad;
        return;
    }
    const uint64_t total = hdr->spare;
    for (uint64_t k = gid; k <= nq; k += gsz)
    {
        const uint64_t p = probe_ptr[k]; // <= pv: the plan checked it
        out_ptr[k] = p < pv ? ix_prefix(res, pre, tile, p) : total;
    }
    if (total > out_values)
    {
        if (gid == 0 && err != nullptr)
            atomicMin(err, static_cast<unsigned long long>(nunits + nq));
        return;
    }
    for (uint64_t i = gid; i < pv; i += gsz)
    {
        const uint32_t r = res[i];
        if ((r & kIxHit) == 0u)
            continue;
        const uint64_t pos = ix_prefix(res, pre, tile, i); // < total <= out_values
        out[pos] = probe[i];
        if (out_pidx != nullptr)
            out_pidx[pos] = static_cast<uint32_t>(i);
        if (out_tpos != nullptr)
            out_tpos[pos] = 256u * ((pu[i] & kRecList) - list_unit[pl[i]]) + (r & 255u);
    }
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
// Workspace of the intersection: header | two run scans over the 64-value
// runs of the probe (item heads, hits) | per probe value its unit word, its
// list and its result | per item its first probe index and its end, each
// 256-byte aligned.  There is at most one item per probe value.
struct IxWs
{
    dev::ItemHdr * hdr;
    RunScanWs<uint32_t> scani, scanh;
    uint32_t *pu, *pl, *res, *ihead, *iend;
    size_t bytes;

    IxWs(void * ws, uint64_t pv)
    {
        WsCarver c(ws);
        const uint64_t nruns = (pv + 63u) / 64u;
        hdr = c.take<dev::ItemHdr>(1);
        scani = c.scan<uint32_t>(nruns);
        scanh = c.scan<uint32_t>(nruns);
        for (uint32_t ** a : {&pu, &pl, &res, &ihead, &iend})
            *a = c.take<uint32_t>(pv);
        bytes = c.used;
    }
};
} // namespace

// nq sizes no array: the queries are read where they lie
size_t lists_intersect_workspace(uint64_t /*nq*/, uint64_t probe_values) { return IxWs(nullptr, probe_values).bytes; }

hipError_t launch_ix_plan(const ListsIndex & X, const uint32_t * probe, uint64_t pv, const uint64_t * probe_ptr, const uint32_t * qlist,
                          uint64_t nq, dev::ItemHdr * hdr, uint32_t * pu, uint32_t * pl, hipStream_t s)
{
    return launch(dev::k_ix_plan, flat_grid(std::max(nq, pv), s), 256, s, X.ptr, X.list_unit, X.nlists, X.nunits, X.unit_last, probe, pv,
                  probe_ptr, qlist, nq, hdr, pu, pl);
}

hipError_t launch_ix_lookup(const dev::IxArgs & A, bool every, hipStream_t s)
{
    const uint64_t pv = A.pv;
    // one wave per kRunDefault items: at least one workgroup for an empty probe
    const uint32_t igrid = std::max(1u, wave_grid(pv, dev::kRunDefault));
    // the cap is one item per probe value, a dense probe holds hundreds of times fewer: at most kListsMinW
    // workgroups per CU, whose waves stride over the real items (k_ix_tails: a wave per 16 items of the cap)
    const uint32_t dgrid = static_cast<uint32_t>(std::max<uint64_t>(
        1, std::min<uint64_t>((pv + 4u * dev::kIxRun - 1u) / (4u * dev::kIxRun), grid_cap(s, dev::kListsMinW))));
    const hipError_t e
        = launch_by(every, [](auto EVERY) { return dev::k_ix_dec<dev::kIxRun, dev::kIxNC, dev::kListsMinW, EVERY>; }, dgrid, 256, s, A);
    if (e != hipSuccess)
        return e;
    return launch_by(every, [](auto EVERY) { return dev::k_ix_tails<dev::kTailsNC, EVERY>; }, igrid, 256, s, A);
}

hipError_t launch_lists_intersect(const ListsIndex & X, const uint32_t * probe, uint64_t pv, const uint64_t * probe_ptr,
                                  const uint32_t * qlist, uint64_t nq, uint32_t * out, uint64_t out_values, uint64_t * out_ptr,
                                  uint32_t * out_pidx, uint32_t * out_tpos, void * ws, unsigned long long * err, hipStream_t s)
{
    if (nq == 0)
    {
        hipError_t e = err ? fill_u32(err, 0xFFFFFFFFu, 2, s) : hipSuccess;
        return e != hipSuccess ? e : (out_ptr ? fill_u32(out_ptr, 0u, 2, s) : hipSuccess);
    }
    if (nq > 0x7FFFFFFFull || pv > 0x7FFFFFFFull || X.nlists > 0x7FFFFFFFull || X.nunits > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const IxWs W(ws, pv);
    const uint64_t nruns = (pv + 63u) / 64u;
    // one wave per 64 probe indices: at least one workgroup for an empty probe
    const uint32_t rgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (nruns + 3u) / 4u));
    hipError_t e = launch_items_reset(err, W.hdr, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch_ix_plan(X, probe, pv, probe_ptr, qlist, nq, W.hdr, W.pu, W.pl, s)) != hipSuccess)
        return e;
    if ((e = launch_items(pv, W.hdr, W.pu, W.pl, W.scani, W.ihead, W.iend, W.res, s)) != hipSuccess)
        return e;
    const dev::IxArgs A{.it = {.ix = X, .hdr = W.hdr, .pu = W.pu, .pl = W.pl, .ihead = W.ihead, .iend = W.iend, .err = err},
                        .probe = probe,
                        .pv = pv,
                        .res = W.res};
    if ((e = launch_ix_lookup(A, false, s)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_ix_hits, rgrid, 256, s, pv, W.hdr, W.res, W.scanh.tot)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u32_single(W.scanh.tot, nruns, W.scanh.pre, W.scanh.tile, &W.hdr->spare, s)) != hipSuccess)
        return e;
    return launch(dev::k_ix_out, flat_grid(std::max(nq + 1u, pv), s), 256, s, X.list_unit, X.nunits, probe, pv, probe_ptr, nq, W.hdr, W.pu,
                  W.pl, W.res, W.scanh.pre, W.scanh.tile, out, out_values, out_ptr, out_pidx, out_tpos, err);
}

} // namespace tpf
