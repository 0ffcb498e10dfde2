// p4_lists_gather.hip -- values at given list positions of a resident index
// (p4_lists.h): tpf_lists_gather takes CSR segments of
// list-relative positions, one target list per segment, and returns the value
// at every position, for delta-1 and for plain streams.  It is the positional
// twin of the intersection (p4_lists_intersect.hip) and keeps its pass
// structure: consecutive request indices that name the same unit of the same
// list form an ITEM, and every item's unit is decoded once -- with k_ix_dec's
// and k_ix_tails's pipelines -- into the wave's LDS, from which the item's
// requests are served 64 at a time.  A position names its unit directly, so
// there is no search over the skip table, and the output is parallel to the
// request, so there is no compaction.  No decoded block goes to global memory.
// Nothing here is sized by the index: grids and the workspace follow
// pos_values.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_generic.h"
#include "p4_scan.h"
#include "tpf_kernels.h"

namespace tpf::dev
{

constexpr uint32_t kGaNone = 0xFFFFFFFFu; // unit word / list word: the request index lies in no segment

// Full blocks: items per wave and chunks in flight, k_ix_dec's shape -- a wave
// waits for its item's positions once per block, as k_ix_dec waits for its
// probe values, so short runs over many waves hide that wait.
constexpr uint32_t kGaRun = 4;
constexpr uint32_t kGaNC = 4;

struct GaHdr
{
    unsigned long long bad; // first refused query k, else nq + the lowest request index with a position past its list (~0: none)
    uint32_t nitems;        // items: runs of request indices with one list and one source unit
    uint32_t pad;
};

// go / no-go of everything after the plan: nothing was refused
__device__ __forceinline__ bool ga_go(const GaHdr * h) { return h->bad == ~0ull; }

struct GaArgs
{
    const uint8_t * in;
    uint64_t in_bytes;
    const uint64_t * off;
    uint64_t nunits;
    const uint64_t * ptr;
    const uint32_t * list_unit;
    const uint32_t * start0;
    const uint32_t * unit_last; // the skip table (values, never indices); delta-1 only
    const uint32_t * pos;
    const GaHdr * hdr;
    const uint32_t * pu;        // per request index: source unit | kRecTail, or kGaNone
    const uint32_t * pl;        // per request index: target list, or kGaNone
    const uint32_t * ihead;     // per item: its first request index ...
    const uint32_t * iend;      // ... and one past its last
    uint32_t * out;
    unsigned long long * err;
};

// Reset of d_err and of the header's verdict in one launch, as k_ix_reset.
__global__ __launch_bounds__(64) void k_ga_reset(unsigned long long * __restrict err, GaHdr * __restrict hdr)
{
    if (threadIdx.x == 0)
    {
        if (err != nullptr)
            *err = ~0ull;
        hdr->bad = ~0ull;
    }
}

// Plan.  One thread per QUERY: k_ix_plan's checks (the values are checked,
// never followed), the first refused query by atomicMin.  One thread per
// REQUEST INDEX: its query by the search over d_pos_ptr (the last k with
// ptr[k] <= i, then i < ptr[k+1] held against it), that query's own checks
// again -- the verdict of the other threads is not known yet; a query that
// fails them is reported by its own thread, with a code below every nq + i --
// then the position against n_j, the lowest offender as nq + i into the same
// word, and the unit the position names.
__global__ __launch_bounds__(256) void k_ga_plan(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                                  uint64_t nunits, const uint32_t * __restrict pos, uint64_t pv,
                                                  const uint64_t * __restrict pos_ptr, const uint32_t * __restrict qlist, uint64_t nq,
                                                  GaHdr * __restrict hdr, uint32_t * __restrict pu, uint32_t * __restrict pl)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t k = gid; k < nq; k += gsz)
    {
        const uint32_t j = qlist[k];
        const uint64_t pa = pos_ptr[k], pb = pos_ptr[k + 1u];
        bool bad = j >= nlists || pb < pa || pb > pv;
        if (!bad)
        {
            const uint64_t a = ptr[j], b = ptr[j + 1u];
            const uint32_t ua = list_unit[j], ub = list_unit[j + 1u];
            bad = b < a || ub < ua || ub > nunits || ub - ua != list_units(b - a);
        }
        if (bad)
            atomicMin(&hdr->bad, static_cast<unsigned long long>(k));
    }
    for (uint64_t i = gid; i < pv; i += gsz)
    {
        uint32_t unit = kGaNone, list = kGaNone;
        // the last k of [0, nq) with pos_ptr[k] <= i
        uint64_t lo = 0u, hi = nq;
        while (lo < hi)
        {
            const uint64_t m = lo + (hi - lo) / 2u;
            if (pos_ptr[m] <= i)
                lo = m + 1u;
            else
                hi = m;
        }
        if (lo != 0u && i < pos_ptr[lo])
        {
            const uint32_t j = qlist[lo - 1u];
            if (j < nlists)
            {
                const uint64_t a = ptr[j], b = ptr[j + 1u];
                const uint32_t ua = list_unit[j], ub = list_unit[j + 1u];
                if (a <= b && ua <= ub && ub <= nunits && ub - ua == list_units(b - a))
                {
                    const uint64_t n = b - a;
                    const uint32_t p = pos[i];
                    if (p < n)
                    {
                        // p / 256 < ub - ua: a unit of list j.  The list's last unit is a p4Enc32 tail when n is no multiple of 256
                        const uint32_t su = ua + (p >> 8);
                        const bool tail = su + 1u == ub && (n & 255u) != 0u;
                        unit = su | (tail ? kRecTail : 0u);
                        list = j;
                    }
                    else
                        atomicMin(&hdr->bad, static_cast<unsigned long long>(nq + i));
                }
            }
        }
        pu[i] = unit;
        pl[i] = list;
    }
}

// A request index heads an item when it names a unit and the index before it
// names another unit or another list; it ends one when the index after does.
__device__ __forceinline__ bool ga_head(const uint32_t * __restrict pu, const uint32_t * __restrict pl, uint64_t i, uint32_t u, uint32_t l)
{
    return u != kGaNone && (i == 0u || pu[i - 1u] != u || pl[i - 1u] != l);
}

// Heads: every wave owns 64 consecutive request indices; the head flags' total
// goes to the run scan (k_ix_heads without the result words).
__global__ __launch_bounds__(256) void k_ga_heads(uint64_t pv, const GaHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                   const uint32_t * __restrict pl, uint32_t * __restrict tot)
{
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    bool head = false;
    if (i < pv && ga_go(hdr))
        head = ga_head(pu, pl, i, pu[i], pl[i]);
    publish_run_total(tot, run, head ? 1u : 0u, t);
}

// Items: item r is the r-th head in request order; the request index that ends
// its run has counted the same r heads, so it knows where to leave the end.
__global__ __launch_bounds__(256) void k_ga_items(uint64_t pv, const GaHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                   const uint32_t * __restrict pl, const uint32_t * __restrict pre,
                                                   const uint32_t * __restrict tile, uint32_t * __restrict ihead,
                                                   uint32_t * __restrict iend)
{
    if (!ga_go(hdr))
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    const bool valid = i < pv;
    const uint32_t u = valid ? pu[i] : kGaNone;
    const uint32_t l = valid ? pl[i] : kGaNone;
    const bool head = valid && ga_head(pu, pl, i, u, l);
    const uint32_t cnt = run_base(pre, tile, run) + wave_incl_scan(head ? 1u : 0u); // heads up to and including i
    if (head)
        ihead[cnt - 1u] = static_cast<uint32_t>(i);
    if (valid && u != kGaNone && (i + 1u == pv || pu[i + 1u] != u || pl[i + 1u] != l))
        iend[cnt - 1u] = static_cast<uint32_t>(i + 1u);
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

// Full blocks: k_ix_dec's pipeline.  Every wave takes runs of RUN consecutive
// ITEMS; lane t gathers item first + t: its head's unit word and list, the
// offsets of the source unit and, with D1, its start -- start0[list] for the
// list's first unit, else unit_last[su - 1] (a unit of the same list: in range
// whatever the table holds).  The plain form skips both loads.  The plan
// checked list < nlists and list_unit[list] <= su < list_unit[list + 1] <=
// nunits for every index it gave a unit.  The block stays in 1 KB of LDS per
// wave.
template <bool D1, uint32_t RUN, uint32_t NC, int MINW>
__global__ __launch_bounds__(256, MINW) void k_ga_dec(const GaArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    __shared__ uint32_t vals[4][256];
    // per item of the run, read back wave-uniformly: the source unit (for the
    // error report only), the request range and the start, as k_ix_dec keeps them
    __shared__ uint32_t srcu[4][RUN], itemh[4][RUN], iteme[4][RUN], starts[4][D1 ? RUN : 1];
    if (!ga_go(A.hdr))
        return;
    constexpr uint32_t kRun = RUN;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    uint32_t * slot = slots[wv];
    uint32_t * scr = scratch[wv];
    const uint64_t in_base = reinterpret_cast<uint64_t>(A.in);
    const uint64_t in_end = in_base + A.in_bytes;
    const uint64_t nit = A.hdr->nitems;
    // the host knows only the cap of one item per request index: the grid covers
    // the device and every wave strides over the runs of the real item count
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 4u * kRun;
    for (uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kRun; first < nit; first += stride)
    {
        const uint32_t n = static_cast<uint32_t>(min_u64(kRun, nit - first));
        const bool valid = t < n;
        const uint32_t ih = valid ? A.ihead[first + t] : 0u;
        const uint32_t ie = valid ? A.iend[first + t] : 0u;
        const uint32_t w = valid ? A.pu[ih] : kGaNone;
        const bool full = valid && (w & kRecTail) == 0u;
        const uint64_t fullmask = __ballot(full);
        if (fullmask == 0ull)
            continue; // a run of tails only
        const uint32_t su = w & kRecList;
        const uint64_t o = full ? A.off[su] : 0ull;
        const uint64_t e = full ? A.off[su + 1u] : 0ull;
        RunPlaneT<kSlotBytes, true> P;
        P.init(in_base, in_end, o, e, full);
        if (t < kRun)
        {
            srcu[wv][t] = full ? su : 0xFFFFFFFFu;
            itemh[wv][t] = ih;
            iteme[wv][t] = ie;
        }
        if constexpr (D1)
        {
            uint32_t startv = 0u;
            if (full)
            {
                const uint32_t lj = A.pl[ih];
                startv = su == A.list_unit[lj] ? (A.start0 != nullptr ? A.start0[lj] : 0u) : A.unit_last[su - 1u];
            }
            if (t < kRun)
                starts[wv][t] = startv;
        }
        wave_lds_sync();
        Chunk C[NC];
#pragma unroll
        for (uint32_t q = 0; q + 1 < NC; ++q)
            P.template issue<0>(C[q], q, t);

        uint64_t badmask = 0u;
        auto consume = [&](const Chunk & c, uint32_t jj) {
            if (((fullmask >> jj) & 1ull) == 0ull)
                return;
            const uint32_t ctl = P.stage(c, jj, slot, t);
            u32x4 x;
            const uint32_t used = decode_block256v32(slot, (ctl >> kCtlShift) & 15u, P.head(c, ctl, slot), scr, t, x);
            if constexpr (D1)
                apply_delta1_256(x, uni(starts[wv][jj]));
            reinterpret_cast<u32x4 *>(vals[wv])[t] = x;
            wave_lds_sync();
            ga_serve(vals[wv], A.pos, A.out, uni(itemh[wv][jj]), uni(iteme[wv][jj]), t);
            wave_lds_sync();
            if (used != rl(P.len, jj))
                badmask |= 1ull << jj;
        };

        bool more = true;
        for (uint32_t j = 0; more; j += NC)
        {
#pragma unroll
            for (uint32_t q = 0; q < NC; ++q)
            {
                if (more)
                {
                    P.template issue<0>(C[(q + NC - 1) % NC], j + q + NC - 1, t);
                    consume(C[q], j + q);
                    more = j + q + 1 < n;
                }
            }
        }
        if (A.err != nullptr && badmask != 0u)
        {
            // in stream numbering; the source units of a run need not ascend
            const uint32_t m = wave_min((t < kRun && ((badmask >> t) & 1ull) != 0ull) ? srcu[wv][t] : 0xFFFFFFFFu);
            if (t == 0)
                atomicMin(A.err, static_cast<unsigned long long>(m));
        }
        wave_lds_sync(); // the item words are rewritten by the next run
    }
}

// Tails: k_ix_tails's pipeline.  Every wave owns kRunDefault consecutive ITEMS
// with the generic decoder; lane t holds item first + t when its unit is its
// list's p4Enc32 tail, n % 256 values.  This is the last launch of the call, so
// it also carries the verdict: on a refusal its first thread writes the error
// word (nothing else has written d_err since the reset) and nothing runs.
template <bool D1, uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_ga_tails(const GaArgs A)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    __shared__ uint32_t vals[4][256];
    if (!ga_go(A.hdr))
    {
        if (blockIdx.x == 0 && threadIdx.x == 0 && A.err != nullptr)
            *A.err = A.nunits + A.hdr->bad;
        return;
    }
    constexpr uint32_t kRun = kRunDefault;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    uint32_t * slot = slots[wv];
    const uint64_t in_base = reinterpret_cast<uint64_t>(A.in);
    const uint64_t in_end = in_base + A.in_bytes;
    const uint64_t nit = A.hdr->nitems;
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kRun;
    if (first >= nit)
        return;
    const uint32_t n = static_cast<uint32_t>(min_u64(kRun, nit - first));
    const bool valid = t < n;
    const uint32_t ih = valid ? A.ihead[first + t] : 0u;
    const uint32_t ie = valid ? A.iend[first + t] : 0u;
    const uint32_t w = valid ? A.pu[ih] : 0u;
    const bool has = valid && (w & kRecTail) != 0u;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0ull)
        return;
    const uint32_t su = w & kRecList;
    const uint32_t lj = has ? A.pl[ih] : 0u;
    const uint32_t cnt = has ? static_cast<uint32_t>((A.ptr[lj + 1u] - A.ptr[lj]) & 255u) : 0u; // != 0: the plan saw a tail
    const uint64_t o = has ? A.off[su] : 0ull;
    const uint64_t e = has ? A.off[su + 1u] : 0ull;
    RunPlaneT<kListSlot> P;
    P.init(in_base, in_end, o, e, has);
    uint32_t startv = 0u;
    if constexpr (D1)
    {
        if (has)
            startv = su == A.list_unit[lj] ? (A.start0 != nullptr ? A.start0[lj] : 0u) : A.unit_last[su - 1u];
    }
    uint64_t badmask = 0u;
    auto consume = [&](const Chunk & c, uint32_t jj) {
        if (((hasmask >> jj) & 1ull) == 0ull)
            return;
        const uint32_t ctl = P.stage(c, jj, slot, t);
        const uint32_t cj = rl(cnt, jj);
        uint32_t x[4], cm;
        const uint32_t used = decode_block_g<Fmt::H32>(slot, (ctl >> kCtlShift) & 15u, cj, scratch[wv], t, x, &cm);
        if constexpr (D1)
            (void)delta1_g<uint32_t>(x, cj, rl(startv, jj), t);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            vals[wv][t + 64u * q] = t + 64u * q < cj ? x[q] : 0u;
        wave_lds_sync();
        ga_serve(vals[wv], A.pos, A.out, rl(ih, jj), rl(ie, jj), t);
        wave_lds_sync();
        if (used != rl(P.len, jj))
            badmask |= 1ull << jj;
    };
    Chunk C[NC];
#pragma unroll
    for (uint32_t q = 0; q + 1 < NC; ++q)
        P.template issue<0>(C[q], q, t);
    bool more = true;
    for (uint32_t jb = 0; more; jb += NC)
    {
#pragma unroll
        for (uint32_t q = 0; q < NC; ++q)
        {
            if (more)
            {
                P.template issue<0>(C[(q + NC - 1) % NC], jb + q + NC - 1, t);
                consume(C[q], jb + q);
                more = jb + q + 1 < n;
            }
        }
    }
    if (A.err != nullptr && badmask != 0u)
    {
        const uint32_t m = wave_min(((badmask >> t) & 1ull) != 0ull ? su : 0xFFFFFFFFu);
        if (t == 0)
            atomicMin(A.err, static_cast<unsigned long long>(m));
    }
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
size_t al256(size_t x) { return (x + 255u) & ~size_t(255); }

// Workspace of the gather: header | the run scan over the 64-index runs of the
// request (item heads) | per request index its unit word and its list | per
// item its first request index and its end, each 256-byte aligned.  There is
// at most one item per request index.
struct GaWs
{
    dev::GaHdr * hdr;
    RunScanWs<uint32_t> scan;
    uint32_t *pu, *pl, *ihead, *iend;
    size_t bytes;

    GaWs(void * ws, uint64_t pv)
    {
        auto * p = static_cast<uint8_t *>(ws);
        const uint64_t nruns = (pv + 63u) / 64u;
        size_t x = 0;
        hdr = reinterpret_cast<dev::GaHdr *>(p + x);
        x += 256u;
        scan = RunScanWs<uint32_t>::carve(p + x, nruns);
        x += al256(RunScanWs<uint32_t>::bytes(nruns));
        uint32_t ** arr[4] = {&pu, &pl, &ihead, &iend};
        for (uint32_t ** a : arr)
        {
            *a = reinterpret_cast<uint32_t *>(p + x);
            x += al256(4u * pv);
        }
        bytes = x;
    }
};

template <bool D1>
hipError_t launch_ga_decode(const dev::GaArgs & A, uint32_t dgrid, uint32_t tgrid, hipStream_t s)
{
    hipLaunchKernelGGL((dev::k_ga_dec<D1, dev::kGaRun, dev::kGaNC, dev::kListsMinW>), dim3(dgrid), dim3(256), 0, s, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL((dev::k_ga_tails<D1, dev::kTailsNC>), dim3(tgrid), dim3(256), 0, s, A);
    return hipGetLastError();
}
} // namespace

// nq sizes no array: the queries are read where they lie
size_t lists_gather_workspace(uint64_t /*nq*/, uint64_t pos_values) { return GaWs(nullptr, pos_values).bytes; }

hipError_t launch_lists_gather(const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nunits, const uint64_t * ptr,
                               const uint32_t * list_unit, uint64_t nlists, bool d1, const uint32_t * start0,
                               const uint32_t * unit_last, const uint32_t * pos, uint64_t pv, const uint64_t * pos_ptr,
                               const uint32_t * qlist, uint64_t nq, uint32_t * out, void * ws, unsigned long long * err, hipStream_t s)
{
    if (nq == 0)
        return err ? fill_u32(err, 0xFFFFFFFFu, 2, s) : hipSuccess;
    if (nq > 0x7FFFFFFFull || pv > 0x7FFFFFFFull || nlists > 0x7FFFFFFFull || nunits > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const GaWs W(ws, pv);
    const uint64_t nruns = (pv + 63u) / 64u;
    // one wave per 64 request indices, one wave per kRunDefault items: at least one workgroup for an empty request
    const uint32_t rgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (nruns + 3u) / 4u));
    const uint32_t tgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (pv + 4u * dev::kRunDefault - 1u) / (4u * dev::kRunDefault)));
    const uint32_t pgrid = static_cast<uint32_t>(
        std::max<uint64_t>(1, std::min<uint64_t>((std::max(nq, pv) + 255u) / 256u, grid_cap(s, 8))));
    hipLaunchKernelGGL(dev::k_ga_reset, dim3(1), dim3(64), 0, s, err, W.hdr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ga_plan, dim3(pgrid), dim3(256), 0, s, ptr, list_unit, nlists, nunits, pos, pv, pos_ptr, qlist, nq, W.hdr,
                       W.pu, W.pl);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ga_heads, dim3(rgrid), dim3(256), 0, s, pv, W.hdr, W.pu, W.pl, W.scan.tot);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    if ((e = ix_scan(W.scan.tot, nruns, W.scan.pre, W.scan.tile, &W.hdr->nitems, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ga_items, dim3(rgrid), dim3(256), 0, s, pv, W.hdr, W.pu, W.pl, W.scan.pre, W.scan.tile, W.ihead, W.iend);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    const dev::GaArgs A{in, in_bytes, off, nunits, ptr, list_unit, start0, unit_last, pos, W.hdr, W.pu, W.pl, W.ihead, W.iend, out, err};
    // the cap is one item per request index, a dense request holds hundreds of times fewer: at most kListsMinW
    // workgroups per CU, whose waves stride over the real items (k_ga_tails: a wave per 16 items of the cap)
    const uint32_t dgrid = static_cast<uint32_t>(std::max<uint64_t>(
        1, std::min<uint64_t>((pv + 4u * dev::kGaRun - 1u) / (4u * dev::kGaRun), grid_cap(s, dev::kListsMinW))));
    return d1 ? launch_ga_decode<true>(A, dgrid, tgrid, s) : launch_ga_decode<false>(A, dgrid, tgrid, s);
}

} // namespace tpf
