// p4_lists_difference.hip -- the probe doc ids that are NOT in resident
// posting lists (p4_lists.h): tpf_lists_difference takes the
// intersection's arguments -- CSR segments of probe values, one target list
// per segment -- and returns, per segment, the values the target does not
// hold, in probe order, with their probe index and the list position L they
// would be inserted at (the number of list values below them).  It is the
// intersection's pipeline (p4_lists_intersect.hip) with the other side of the
// lookup compacted: the plan, the item layer and the lookup's EVERY form, which
// leaves the lower bound q of every probe value that has a unit, then a flags
// pass over the misses, its run scan and a compaction.  A value no unit holds
// (past its list's last value, or aimed at an empty list) is a miss the plan
// already decided: it costs no decode.  Nothing here is sized by the index:
// grids and the workspace follow probe_values.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

// The result word after the flags pass: bits 0-8 q as the lookup left it,
// kDfMiss for a miss, kDfNone for a miss no unit holds (L = n), bits 16-22 the
// misses before it in its 64-index run.  An index outside every segment is
// neither a member nor a miss: its word is the count alone.
constexpr uint32_t kDfMiss = 0x400u;
constexpr uint32_t kDfNone = 0x800u;

// Flags: every wave owns 64 consecutive probe indices, as k_ix_hits does; the
// miss flags' total goes to the run scan and the result word is rewritten as
// above, so the compaction reads one word per index.  Whether an index has a
// unit at all is the plan's word pu -- the lookup wrote the result word of
// exactly the indices that have one, and the word of the others is not read.
__global__ __launch_bounds__(256) void k_df_flags(uint64_t pv, const uint64_t * __restrict probe_ptr, uint64_t nq,
                                                   const ItemHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                   uint32_t * __restrict res, uint32_t * __restrict tot)
{
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    uint32_t w = 0u;
    // the plan checked the segment pointers: they ascend and end inside the probe
    if (i < pv && items_go(hdr) && i >= probe_ptr[0] && i < probe_ptr[nq])
    {
        if (pu[i] == kItemNone)
            w = kDfMiss | kDfNone;
        else
        {
            const uint32_t r = res[i];
            w = (r & kIxFound) != 0u ? 0u : (umin32(r & kIxQ, 256u) | kDfMiss);
        }
    }
    const uint32_t miss = (w & kDfMiss) != 0u ? 1u : 0u;
    const uint32_t incl = wave_incl_scan(miss);
    if (i < pv)
        res[i] = w | ((incl - miss) << 16);
    if (t == 0)
        tot[run] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
}

// misses at probe indices below p
__device__ __forceinline__ uint32_t df_prefix(const uint32_t * __restrict res, const uint32_t * __restrict pre,
                                              const uint32_t * __restrict tile, uint64_t p)
{
    return run_base(pre, tile, p / 64u) + ((res[p] >> 16) & 127u);
}

// Compaction: the verdict (a refused query; misses that do not fit, by
// atomicMin under a parse error the lookup may have left), d_out_ptr[k] = the
// misses before probe_ptr[k], then every miss's value, probe index and L
// scattered to its place.  L needs the list's length, and its first unit where
// the miss has a unit: both are read for misses only, and only when
// d_out_tpos is there.  A miss without a unit finds its list through its
// segment; the plan left it none.
__global__ __launch_bounds__(256) void k_df_out(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nunits,
                                                const uint32_t * __restrict probe, uint64_t pv, const uint64_t * __restrict probe_ptr,
                                                const uint32_t * __restrict qlist, uint64_t nq, const ItemHdr * __restrict hdr,
                                                const uint32_t * __restrict pu, const uint32_t * __restrict pl,
                                                const uint32_t * __restrict res, const uint32_t * __restrict pre,
                                                const uint32_t * __restrict tile, uint32_t * __restrict out, uint64_t out_values,
                                                uint64_t * __restrict out_ptr, uint32_t * __restrict out_pidx,
                                                uint32_t * __restrict out_tpos, unsigned long long * __restrict err)
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
        out_ptr[k] = p < pv ? df_prefix(res, pre, tile, p) : total;
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
        if ((r & kDfMiss) == 0u)
            continue;
        const uint64_t pos = df_prefix(res, pre, tile, i); // < total <= out_values
        out[pos] = probe[i];
        if (out_pidx != nullptr)
            out_pidx[pos] = static_cast<uint32_t>(i);
        if (out_tpos != nullptr)
        {
            uint64_t l = 0u;
            if ((r & kDfNone) != 0u)
            {
                // (the flags pass left no flag outside the segments, and the plan checked qlist[k])
                const uint32_t k = segment_of(probe_ptr, nq, i);
                if (k != kItemNone)
                {
                    const uint32_t j = qlist[k];
                    l = ptr[j + 1u] - ptr[j];
                }
            }
            else
            {
                const uint32_t j = pl[i]; // the plan checked it where it gave a unit
                l = min_u64(256ull * ((pu[i] & kRecList) - list_unit[j]) + (r & kIxQ), ptr[j + 1u] - ptr[j]);
            }
            out_tpos[pos] = static_cast<uint32_t>(l);
        }
    }
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
// Workspace of the difference, the intersection's: header | two run scans over
// the 64-value runs of the probe (item heads, misses) | per probe value its
// unit word, its list and its result | per item its first probe index and its
// end, each 256-byte aligned.  There is at most one item per probe value.
struct DfWs
{
    dev::ItemHdr * hdr;
    RunScanWs<uint32_t> scani, scanm;
    uint32_t *pu, *pl, *res, *ihead, *iend;
    size_t bytes;

    DfWs(void * ws, uint64_t pv)
    {
        WsCarver c(ws);
        const uint64_t nruns = (pv + 63u) / 64u;
        hdr = c.take<dev::ItemHdr>(1);
        scani = c.scan<uint32_t>(nruns);
        scanm = c.scan<uint32_t>(nruns);
        for (uint32_t ** a : {&pu, &pl, &res, &ihead, &iend})
            *a = c.take<uint32_t>(pv);
        bytes = c.used;
    }
};
} // namespace

// nq sizes no array: the queries are read where they lie
size_t lists_difference_workspace(uint64_t /*nq*/, uint64_t probe_values) { return DfWs(nullptr, probe_values).bytes; }

hipError_t launch_lists_difference(const ListsIndex & X, const uint32_t * probe, uint64_t pv, const uint64_t * probe_ptr,
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
    const DfWs W(ws, pv);
    const uint64_t nruns = (pv + 63u) / 64u;
    // one wave per 64 probe indices: at least one workgroup for an empty probe
    const uint32_t rgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (nruns + 3u) / 4u));
    hipError_t e = launch_items_reset(err, W.hdr, s);
    if (e != hipSuccess)
        return e;
    // ---- the lookup: the intersection's plan, items and decode, every probe value's q recorded
    if ((e = launch_ix_plan(X, probe, pv, probe_ptr, qlist, nq, W.hdr, W.pu, W.pl, s)) != hipSuccess)
        return e;
    if ((e = launch_items(pv, W.hdr, W.pu, W.pl, W.scani, W.ihead, W.iend, W.res, s)) != hipSuccess)
        return e;
    const dev::IxArgs A{.it = {.ix = X, .hdr = W.hdr, .pu = W.pu, .pl = W.pl, .ihead = W.ihead, .iend = W.iend, .err = err},
                        .probe = probe,
                        .pv = pv,
                        .res = W.res};
    if ((e = launch_ix_lookup(A, true, s)) != hipSuccess)
        return e;
    // ---- the misses: flags, their run scan (hdr->spare = d_out_ptr[nq]), the compaction
    if ((e = launch(dev::k_df_flags, rgrid, 256, s, pv, probe_ptr, nq, W.hdr, W.pu, W.res, W.scanm.tot)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u32_single(W.scanm.tot, nruns, W.scanm.pre, W.scanm.tile, &W.hdr->spare, s)) != hipSuccess)
        return e;
    return launch(dev::k_df_out, flat_grid(std::max(nq + 1u, pv), s), 256, s, X.ptr, X.list_unit, X.nunits, probe, pv, probe_ptr, qlist, nq,
                  W.hdr, W.pu, W.pl, W.res, W.scanm.pre, W.scanm.tile, out, out_values, out_ptr, out_pidx, out_tpos, err);
}

} // namespace tpf
