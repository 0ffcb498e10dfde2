// p4_lists_gather.hip -- values at given list positions of a resident index
// (p4_lists.h): tpf_lists_gather takes CSR segments of
// list-relative positions, one target list per segment, and returns the value
// at every position, for delta-1 and for plain streams.  It is the positional
// twin of the intersection (p4_lists_intersect.hip) and keeps its pass
// structure: consecutive request indices that name the same unit of the same
// list form an ITEM (p4_lists_items.hip), and every item's unit is decoded
// once -- with k_ix_dec's and k_ix_tails's pipelines -- into the wave's LDS,
// from which the item's requests are served 64 at a time.  A position names
// its unit directly, so there is no search over the skip table, and the output
// is parallel to the request, so there is no compaction.  No decoded block
// goes to global memory.  Nothing here is sized by the index: grids and the
// workspace follow pos_values.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

// Full blocks: items per wave and chunks in flight, k_ix_dec's shape -- a wave
// waits for its item's positions once per block, as k_ix_dec waits for its
// probe values, so short runs over many waves hide that wait.
constexpr uint32_t kGaRun = 4;
constexpr uint32_t kGaNC = 4;

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
    const ItemHdr * hdr;        // bad: first refused query k, else nq + the lowest request index with a position past its list
    const uint32_t * pu;        // per request index: source unit | kRecTail, or kItemNone
    const uint32_t * pl;        // per request index: target list, or kItemNone
    const uint32_t * ihead;     // per item: its first request index ...
    const uint32_t * iend;      // ... and one past its last
    uint32_t * out;
    unsigned long long * err;
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

// Full blocks: k_ix_dec's pipeline.  Every wave takes runs of RUN consecutive
// ITEMS; lane t gathers item first + t: its head's unit word and list, the
// offsets of the source unit and, with D1, its start (unit_start,
// p4_lists_dev.h).  The plain form skips both loads.  The plan checked list <
// nlists and list_unit[list] <= su < list_unit[list + 1] <= nunits for every
// index it gave a unit.  The block stays in 1 KB of LDS per wave.
template <bool D1, uint32_t RUN, uint32_t NC, int MINW>
__global__ __launch_bounds__(256, MINW) void k_ga_dec(const GaArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    __shared__ uint32_t vals[4][256];
    // per item of the run, read back wave-uniformly: the source unit (for the
    // error report only), the request range and the start, as k_ix_dec keeps them
    __shared__ uint32_t srcu[4][RUN], itemh[4][RUN], iteme[4][RUN], starts[4][D1 ? RUN : 1];
    if (!items_go(A.hdr))
        return;
    constexpr uint32_t kRun = RUN;
    const uint64_t nit = A.hdr->nitems;
    WaveRun R = wave_run(A.in, A.in_bytes, kRun, nit);
    const uint32_t t = R.t, wv = R.wv;
    uint32_t * slot = slots[wv];
    uint32_t * scr = scratch[wv];
    // the host knows only the cap of one item per request index: the grid covers
    // the device and every wave strides over the runs of the real item count
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 4u * kRun;
    for (; R.first < nit; R.seek(R.first + stride, kRun, nit))
    {
        const uint64_t first = R.first;
        const bool valid = t < R.n;
        const uint32_t ih = valid ? A.ihead[first + t] : 0u;
        const uint32_t ie = valid ? A.iend[first + t] : 0u;
        const uint32_t w = valid ? A.pu[ih] : kItemNone;
        const bool full = valid && (w & kRecTail) == 0u;
        const uint64_t fullmask = __ballot(full);
        if (fullmask == 0ull)
            continue; // a run of tails only
        const uint32_t su = w & kRecList;
        const uint64_t o = full ? A.off[su] : 0ull;
        const uint64_t e = full ? A.off[su + 1u] : 0ull;
        RunPlaneT<kSlotBytes, true> P;
        P.init(R.in_base, R.in_end, o, e, full);
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
                startv = unit_start(A.list_unit, A.start0, A.unit_last, A.pl[ih], su);
            if (t < kRun)
                starts[wv][t] = startv;
        }
        wave_lds_sync();
        Chunk C[NC];
        pipe_prime<NC>(P, C, t);

        uint64_t badmask = 0u;
        pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
            if (((fullmask >> jj) & 1ull) == 0ull)
                return;
            u32x4 x;
            decode_full_unit<D1>(P, c, jj, slot, scr, D1 ? uni(starts[wv][jj]) : 0u, t, x, badmask);
            reinterpret_cast<u32x4 *>(vals[wv])[t] = x;
            wave_lds_sync();
            ga_serve(vals[wv], A.pos, A.out, uni(itemh[wv][jj]), uni(iteme[wv][jj]), t);
            wave_lds_sync();
        });
        report_bad_units(A.err, badmask, t < kRun ? srcu[wv][t] : 0xFFFFFFFFu, t);
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
    if (!items_go(A.hdr))
    {
        if (blockIdx.x == 0 && threadIdx.x == 0 && A.err != nullptr)
            *A.err = A.nunits + A.hdr->bad;
        return;
    }
    const uint64_t nit = A.hdr->nitems;
    const WaveRun R = wave_run(A.in, A.in_bytes, kRunDefault, nit);
    const uint32_t t = R.t, wv = R.wv;
    if (R.first >= nit)
        return;
    uint32_t * slot = slots[wv];
    const bool valid = t < R.n;
    const uint32_t ih = valid ? A.ihead[R.first + t] : 0u;
    const uint32_t ie = valid ? A.iend[R.first + t] : 0u;
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
    P.init(R.in_base, R.in_end, o, e, has);
    uint32_t startv = 0u;
    if constexpr (D1)
    {
        if (has)
            startv = unit_start(A.list_unit, A.start0, A.unit_last, lj, su);
    }
    uint64_t badmask = 0u;
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((hasmask >> jj) & 1ull) == 0ull)
            return;
        const uint32_t cj = rl(cnt, jj);
        TailVals x;
        decode_tail_unit<D1>(P, c, jj, slot, scratch[wv], cj, rl(startv, jj), t, x, badmask);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            vals[wv][t + 64u * q] = t + 64u * q < cj ? x.v[q] : 0u;
        wave_lds_sync();
        ga_serve(vals[wv], A.pos, A.out, rl(ih, jj), rl(ie, jj), t);
        wave_lds_sync();
    });
    report_bad_units(A.err, badmask, su, t);
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
    // one wave per kRunDefault items: at least one workgroup for an empty request
    const uint32_t tgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (pv + 4u * dev::kRunDefault - 1u) / (4u * dev::kRunDefault)));
    hipError_t e = launch_items_reset(err, W.hdr, s);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ga_plan, dim3(flat_grid(std::max(nq, pv), s)), dim3(256), 0, s, ptr, list_unit, nlists, nunits, pos, pv, pos_ptr,
                       qlist, nq, W.hdr, W.pu, W.pl);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    if ((e = launch_items(pv, W.hdr, W.pu, W.pl, W.scan, W.ihead, W.iend, nullptr, s)) != hipSuccess)
        return e;
    const dev::GaArgs A{in, in_bytes, off, nunits, ptr, list_unit, start0, unit_last, pos, W.hdr, W.pu, W.pl, W.ihead, W.iend, out, err};
    // the cap is one item per request index, a dense request holds hundreds of times fewer: at most kListsMinW
    // workgroups per CU, whose waves stride over the real items (k_ga_tails: a wave per 16 items of the cap)
    const uint32_t dgrid = static_cast<uint32_t>(std::max<uint64_t>(
        1, std::min<uint64_t>((pv + 4u * dev::kGaRun - 1u) / (4u * dev::kGaRun), grid_cap(s, dev::kListsMinW))));
    return d1 ? launch_ga_decode<true>(A, dgrid, tgrid, s) : launch_ga_decode<false>(A, dgrid, tgrid, s);
}

} // namespace tpf
