// p4_lists_gather.hip -- values at given list positions of a resident index
// (p4_lists.h): tpf_lists_gather takes CSR segments of
// list-relative positions, one target list per segment, and returns the value
// at every position, for delta-1 and for plain streams.  It is the positional
// twin of the intersection (p4_lists_intersect.hip) and keeps its pass
// structure: consecutive request indices that name the same unit of the same
// list form an ITEM (p4_lists_items.hip), and every item's unit is decoded
// once -- by the item drivers the lookup runs too (p4_lists_items.h) -- into
// the wave's LDS, from which the item's requests are served 64 at a time.  A
// position names its unit directly, so there is no search over the skip table,
// and the output is parallel to the request, so there is no compaction.  No
// decoded block goes to global memory.  Nothing here is sized by the index:
// grids and the workspace follow pos_values.
#include "p4_lists.h"

#include "p4_lists_host.h"
#include "p4_lists_items.h"

namespace tpf::dev
{

// Full blocks (item_full_units): items per wave and chunks in flight, the
// lookup's -- a wave waits for its item's positions once per block, as the
// lookup waits for its probe values, so short runs over many waves hide that
// wait.
constexpr uint32_t kGaRun = 4;
constexpr uint32_t kGaNC = 4;

struct GaArgs
{
    ItemArgs it; // hdr->bad: first refused query k, else nq + the lowest request index with a position past its list
    const uint32_t * pos;
    uint32_t * out;
};

// Plan.  One thread per QUERY: check_queries (p4_lists_dev.h).  One thread per
// REQUEST INDEX: its query by the search over d_pos_ptr, that query's own
// checks again -- the verdict of the other threads is not known yet; a query
// that fails them is reported by its own thread, with a code below every nq +
// i -- then the position against n_j, the lowest offender as nq + i into the
// same word, and the unit the position names.
__global__ __launch_bounds__(256) void k_ga_plan(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                                  uint64_t nunits, const uint32_t * __restrict pos, uint64_t pv,
                                                  const uint64_t * __restrict pos_ptr, const uint32_t * __restrict qlist, uint64_t nq,
                                                  ItemHdr * __restrict hdr, uint32_t * __restrict pu, uint32_t * __restrict pl)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    check_queries(ptr, list_unit, nlists, nunits, pos_ptr, pv, qlist, nq, &hdr->bad, gid, gsz);
    for (uint64_t i = gid; i < pv; i += gsz)
    {
        uint32_t unit = kItemNone, list = kItemNone;
        const uint32_t k = segment_of(pos_ptr, nq, i);
        uint64_t n;
        uint32_t ua, ub;
        if (k != kItemNone && list_dir_ok(ptr, list_unit, nlists, nunits, qlist[k], &n, &ua, &ub))
        {
            const uint32_t p = pos[i];
            if (p < n)
            {
                // p / 256 < ub - ua: a unit of list j.  The list's last unit is a p4Enc32 tail when n is no multiple of 256
                const uint32_t su = ua + (p >> 8);
                const bool tail = su + 1u == ub && (n & 255u) != 0u;
                unit = su | (tail ? kRecTail : 0u);
                list = qlist[k];
            }
            else
                atomicMin(&hdr->bad, static_cast<unsigned long long>(nq + i));
        }
        pu[i] = unit;
        pl[i] = list;
    }
}

// The request indices [h, e) of one item from the 256 values the wave has just
// decoded into `vals`, 64 at a time.  Every position of an item names the
// item's unit, so its low 8 bits are the index inside it (below the unit's
// count: the plan held the position against n_j); the mask keeps the LDS read
// inside the wave's 1 KB whatever d_pos holds by now.
__device__ __forceinline__ void ga_serve(const uint32_t * vals, const uint32_t * __restrict pos, uint32_t * __restrict out, uint32_t h,
                                         uint32_t e, uint32_t t)
{
    for (uint32_t c = h; c < e; c += 64u)
    {
        const uint32_t i = c + t;
        if (i < e)
            out[i] = vals[pos[i] & 255u];
    }
}

// Full blocks and tails: the item drivers (p4_lists_items.h) with ga_serve as
// what is done with an item's decoded unit; the plain form skips the start's
// loads.  A tail's words past its count hold 0 (the plan held every position
// below the count: they are not read).
template <bool D1, uint32_t RUN, uint32_t NC, int MINW>
__global__ __launch_bounds__(256, MINW) void k_ga_dec(const GaArgs A)
{
    if (!items_go(A.it.hdr))
        return;
    constexpr uint32_t kRun = RUN;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 4u * kRun;
    item_full_units<D1, RUN, NC>(A.it, stride, [&](const uint32_t * vals, uint32_t, uint32_t h, uint32_t e, uint32_t t) {
        ga_serve(vals, A.pos, A.out, h, e, t);
    });
}

// The tails kernel is the last launch of the call, so it also carries the
// verdict: on a refusal its first thread writes the error word (nothing else
// has written d_err since the reset) and nothing runs.
template <bool D1, uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_ga_tails(const GaArgs A)
{
    if (!items_go(A.it.hdr))
    {
        if (blockIdx.x == 0 && threadIdx.x == 0 && A.it.err != nullptr)
            *A.it.err = A.it.ix.nunits + A.it.hdr->bad;
        return;
    }
    item_tail_units<D1, NC>(A.it, 0u, [&](const uint32_t * vals, uint32_t, uint32_t h, uint32_t e, uint32_t t) {
        ga_serve(vals, A.pos, A.out, h, e, t);
    });
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
// Workspace of the gather: header | the run scan over the 64-index runs of the
// request (item heads) | per request index its unit word and its list | per
// item its first request index and its end, each 256-byte aligned.  There is
// at most one item per request index.
struct GaWs
{
    dev::ItemHdr * hdr;
    RunScanWs<uint32_t> scan;
    uint32_t *pu, *pl, *ihead, *iend;
    size_t bytes;

    GaWs(void * ws, uint64_t pv)
    {
        WsCarver c(ws);
        hdr = c.take<dev::ItemHdr>(1);
        scan = c.scan<uint32_t>((pv + 63u) / 64u);
        for (uint32_t ** a : {&pu, &pl, &ihead, &iend})
            *a = c.take<uint32_t>(pv);
        bytes = c.used;
    }
};

} // namespace

// nq sizes no array: the queries are read where they lie
size_t lists_gather_workspace(uint64_t /*nq*/, uint64_t pos_values) { return GaWs(nullptr, pos_values).bytes; }

hipError_t launch_lists_gather(const ListsIndex & X, bool d1, const uint32_t * pos, uint64_t pv, const uint64_t * pos_ptr,
                               const uint32_t * qlist, uint64_t nq, uint32_t * out, void * ws, unsigned long long * err, hipStream_t s)
{
    if (nq == 0)
        return err ? fill_u32(err, 0xFFFFFFFFu, 2, s) : hipSuccess;
    if (nq > 0x7FFFFFFFull || pv > 0x7FFFFFFFull || X.nlists > 0x7FFFFFFFull || X.nunits > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const GaWs W(ws, pv);
    // one wave per kRunDefault items: at least one workgroup for an empty request
    const uint32_t tgrid = std::max(1u, wave_grid(pv, dev::kRunDefault));
    hipError_t e = launch_items_reset(err, W.hdr, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch(dev::k_ga_plan, flat_grid(std::max(nq, pv), s), 256, s, X.ptr, X.list_unit, X.nlists, X.nunits, pos, pv, pos_ptr, qlist, nq,
                    W.hdr, W.pu, W.pl))
        != hipSuccess)
        return e;
    if ((e = launch_items(pv, W.hdr, W.pu, W.pl, W.scan, W.ihead, W.iend, nullptr, s)) != hipSuccess)
        return e;
    const dev::GaArgs A{.it = {.ix = X, .hdr = W.hdr, .pu = W.pu, .pl = W.pl, .ihead = W.ihead, .iend = W.iend, .err = err},
                        .pos = pos,
                        .out = out};
    // the cap is one item per request index, a dense request holds hundreds of times fewer: at most kListsMinW
    // workgroups per CU, whose waves stride over the real items (k_ga_tails: a wave per 16 items of the cap)
    const uint32_t dgrid = static_cast<uint32_t>(std::max<uint64_t>(
        1, std::min<uint64_t>((pv + 4u * dev::kGaRun - 1u) / (4u * dev::kGaRun), grid_cap(s, dev::kListsMinW))));
    if ((e = launch_by(d1, [](auto D1) { return dev::k_ga_dec<D1, dev::kGaRun, dev::kGaNC, dev::kListsMinW>; }, dgrid, 256, s, A)) != hipSuccess)
        return e;
    return launch_by(d1, [](auto D1) { return dev::k_ga_tails<D1, dev::kTailsNC>; }, tgrid, 256, s, A);
}

} // namespace tpf
