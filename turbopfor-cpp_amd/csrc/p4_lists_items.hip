// p4_lists_items.hip -- the item layer the intersection (p4_lists_intersect.hip)
// and the gather (p4_lists_gather.hip) share (p4_lists.h): the
// entry's plan leaves, per request index, the source unit and the list it
// names; consecutive indices that name the same unit of the same list form an
// ITEM, whose unit the entry's decode kernels then decode once (the item
// drivers, p4_lists_items.h).
#include "p4_lists.h"

#include "p4_lists_host.h"

namespace tpf::dev
{

// Reset of d_err and of the header's verdict in one launch (the other entries
// spend a k_fill_u32 on each; these calls are launch-bound for small requests).
__global__ __launch_bounds__(64) void k_items_reset(unsigned long long * __restrict err, ItemHdr * __restrict hdr)
{
    if (threadIdx.x == 0)
    {
        if (err != nullptr)
            *err = ~0ull;
        hdr->bad = ~0ull;
    }
}

// A request index heads an item when it names a unit and the index before it
// names another unit or another list; it ends one when the index after does.
__device__ __forceinline__ bool item_head(const uint32_t * __restrict pu, const uint32_t * __restrict pl, uint64_t i, uint32_t u, uint32_t l)
{
    return u != kItemNone && (i == 0u || pu[i - 1u] != u || pl[i - 1u] != l);
}

// Heads: every wave owns 64 consecutive request indices; the head flags' total
// goes to the run scan.  RES: every result word starts as kItemNone.
template <bool RES>
__global__ __launch_bounds__(256) void k_item_heads(uint64_t pv, const ItemHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                     const uint32_t * __restrict pl, uint32_t * __restrict tot, uint32_t * __restrict res)
{
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    bool head = false;
    if (i < pv)
    {
        if constexpr (RES)
            res[i] = kItemNone;
        if (items_go(hdr))
            head = item_head(pu, pl, i, pu[i], pl[i]);
    }
    publish_run_total(tot, run, head ? 1u : 0u, t);
}

// Items: item r is the r-th head in request order; the request index that ends
// its run has counted the same r heads, so it knows where to leave the end.
__global__ __launch_bounds__(256) void k_item_items(uint64_t pv, const ItemHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                     const uint32_t * __restrict pl, const uint32_t * __restrict pre,
                                                     const uint32_t * __restrict tile, uint32_t * __restrict ihead,
                                                     uint32_t * __restrict iend)
{
    if (!items_go(hdr))
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    const bool valid = i < pv;
    const uint32_t u = valid ? pu[i] : kItemNone;
    const uint32_t l = valid ? pl[i] : kItemNone;
    const bool head = valid && item_head(pu, pl, i, u, l);
    const uint32_t cnt = run_base(pre, tile, run) + wave_incl_scan(head ? 1u : 0u); // heads up to and including i
    if (head)
        ihead[cnt - 1u] = static_cast<uint32_t>(i);
    if (valid && u != kItemNone && (i + 1u == pv || pu[i + 1u] != u || pl[i + 1u] != l))
        iend[cnt - 1u] = static_cast<uint32_t>(i + 1u);
}

} // namespace tpf::dev

namespace tpf
{

hipError_t launch_items_reset(unsigned long long * err, dev::ItemHdr * hdr, hipStream_t s)
{
    return launch(dev::k_items_reset, 1, 64, s, err, hdr);
}

hipError_t launch_items(uint64_t pv, dev::ItemHdr * hdr, const uint32_t * pu, const uint32_t * pl, const RunScanWs<uint32_t> & scan,
                        uint32_t * ihead, uint32_t * iend, uint32_t * res, hipStream_t s)
{
    const uint64_t nruns = (pv + 63u) / 64u;
    // one wave per 64 request indices: at least one workgroup for an empty request
    const uint32_t rgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (nruns + 3u) / 4u));
    hipError_t e = launch_by(res != nullptr, [](auto RES) { return dev::k_item_heads<RES>; }, rgrid, 256, s, pv, hdr, pu, pl, scan.tot, res);
    if (e != hipSuccess)
        return e;
    if ((e = launch_run_scan_u32_single(scan.tot, nruns, scan.pre, scan.tile, &hdr->nitems, s)) != hipSuccess)
        return e;
    return launch(dev::k_item_items, rgrid, 256, s, pv, hdr, pu, pl, scan.pre, scan.tile, ihead, iend);
}

} // namespace tpf
