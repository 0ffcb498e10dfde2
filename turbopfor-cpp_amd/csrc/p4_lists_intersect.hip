// p4_lists_intersect.hip -- membership of probe doc ids in resident posting
// lists (p4_lists.h): tpf_lists_intersect takes sorted CSR
// segments of probe values, one target list per segment, and returns the
// values that are also in the target, with their positions.  Every probe value
// is looked up in the skip table (the first unit of its list whose last value
// is >= it); consecutive probe values that land in the same unit form an ITEM
// (p4_lists_items.hip), and every item's unit is decoded once -- with
// k_un_dec's and k_un_tails's pipelines (p4_lists_units.hip), the start taken
// from the table -- into the wave's LDS, where the item's probe values are
// searched 64 at a time.  No decoded block goes to global memory.  Nothing
// here is sized by the index: grids and the workspace follow nq and
// probe_values.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

constexpr uint32_t kIxMiss = kItemNone; // result word before the hits pass: not a member
constexpr uint32_t kIxHit = 0x100u;     // result word after the hits pass: bits 0-7 p, bit 8 hit, bits 16-22 hits before it in its run
// (EVERY, the union's lookup: every probe value of an item gets q | kIxFound, p4_lists.h)

// Full blocks: items per wave and chunks in flight.  A wave waits for its
// item's probe values once per block (that load sits behind the chunk loads in
// issue order), so short runs over many waves hide the wait better than
// k_un_dec's 16 blocks per wave; DESIGN.md 4.11 has both timings.
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

// Full blocks: every wave takes runs of RUN consecutive ITEMS through the
// k_dec256v32w pipeline, as k_un_dec does with virtual units.  Lane t
// gathers item first + t: its head's unit word and list, the offsets of the
// source unit and its start (unit_start, p4_lists_dev.h).  The plan checked
// list < nlists and list_unit[list] <= su < list_unit[list + 1] <= nunits for
// every value it gave a unit.  Where k_un_dec stores the block, this keeps it
// in 1 KB of LDS per wave.
template <uint32_t RUN, uint32_t NC, int MINW, bool EVERY>
__global__ __launch_bounds__(256, MINW) void k_ix_dec(const IxArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    __shared__ uint32_t vals[4][256];
    // per item of the run, read back wave-uniformly: the source unit (for the
    // error report only, as in k_un_dec), the probe range and the start -- held
    // in registers across the pipeline they cost spilled VGPRs at 7 waves
    __shared__ uint32_t srcu[4][RUN], itemh[4][RUN], iteme[4][RUN], starts[4][RUN];
    if (!items_go(A.hdr))
        return;
    constexpr uint32_t kRun = RUN;
    const uint64_t nit = A.hdr->nitems;
    WaveRun R = wave_run(A.in, A.in_bytes, kRun, nit);
    const uint32_t t = R.t, wv = R.wv;
    uint32_t * slot = slots[wv];
    uint32_t * scr = scratch[wv];
    // the host knows only the cap of one item per probe value: the grid covers
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
        const uint32_t lj = full ? A.pl[ih] : 0u;
        const uint64_t o = full ? A.off[su] : 0ull;
        const uint64_t e = full ? A.off[su + 1u] : 0ull;
        RunPlaneT<kSlotBytes, true> P;
        P.init(R.in_base, R.in_end, o, e, full);
        {
            uint32_t startv = 0u;
            if (full)
                startv = unit_start(A.list_unit, A.start0, A.unit_last, lj, su);
            if (t < kRun)
            {
                srcu[wv][t] = full ? su : 0xFFFFFFFFu;
                itemh[wv][t] = ih;
                iteme[wv][t] = ie;
                starts[wv][t] = startv;
            }
        }
        wave_lds_sync();
        Chunk C[NC];
        pipe_prime<NC>(P, C, t);

        uint64_t badmask = 0u;
        pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
            if (((fullmask >> jj) & 1ull) == 0ull)
                return;
            u32x4 x;
            decode_full_unit<true>(P, c, jj, slot, scr, uni(starts[wv][jj]), t, x, badmask);
            reinterpret_cast<u32x4 *>(vals[wv])[t] = x;
            wave_lds_sync();
            ix_test<EVERY>(vals[wv], 256u, A.probe, A.res, uni(itemh[wv][jj]), uni(iteme[wv][jj]), t);
            wave_lds_sync();
        });
        report_bad_units(A.err, badmask, t < kRun ? srcu[wv][t] : 0xFFFFFFFFu, t);
        wave_lds_sync(); // the item words are rewritten by the next run
    }
}

// Tails: every wave owns kRunDefault consecutive ITEMS with the generic
// decoder's pipeline, as k_un_tails does for selections; lane t holds item
// first + t when its unit is its list's p4Enc32 tail, n % 256 values.
template <uint32_t NC, bool EVERY>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_ix_tails(const IxArgs A)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    __shared__ uint32_t vals[4][256];
    if (!items_go(A.hdr))
        return;
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
    if (has)
        startv = unit_start(A.list_unit, A.start0, A.unit_last, lj, su);
    uint64_t badmask = 0u;
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((hasmask >> jj) & 1ull) == 0ull)
            return;
        const uint32_t cj = rl(cnt, jj);
        TailVals x;
        decode_tail_unit<true>(P, c, jj, slot, scratch[wv], cj, rl(startv, jj), t, x, badmask);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            vals[wv][t + 64u * q] = t + 64u * q < cj ? x.v[q] : 0xFFFFFFFFu;
        wave_lds_sync();
        ix_test<EVERY>(vals[wv], cj, A.probe, A.res, rl(ih, jj), rl(ie, jj), t);
        wave_lds_sync();
    });
    report_bad_units(A.err, badmask, su, t);
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

hipError_t launch_ix_plan(const uint64_t * ptr, const uint32_t * list_unit, uint64_t nlists, uint64_t nunits, const uint32_t * unit_last,
                          const uint32_t * probe, uint64_t pv, const uint64_t * probe_ptr, const uint32_t * qlist, uint64_t nq,
                          dev::ItemHdr * hdr, uint32_t * pu, uint32_t * pl, hipStream_t s)
{
    hipLaunchKernelGGL(dev::k_ix_plan, dim3(flat_grid(std::max(nq, pv), s)), dim3(256), 0, s, ptr, list_unit, nlists, nunits, unit_last,
                       probe, pv, probe_ptr, qlist, nq, hdr, pu, pl);
    return hipGetLastError();
}

namespace
{
template <bool EVERY>
hipError_t ix_lookup(const dev::IxArgs & A, uint32_t dgrid, uint32_t igrid, hipStream_t s)
{
    hipLaunchKernelGGL((dev::k_ix_dec<dev::kIxRun, dev::kIxNC, dev::kListsMinW, EVERY>), dim3(dgrid), dim3(256), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL((dev::k_ix_tails<dev::kTailsNC, EVERY>), dim3(igrid), dim3(256), 0, s, A);
    return hipGetLastError();
}
} // namespace

hipError_t launch_ix_lookup(const dev::IxArgs & A, bool every, hipStream_t s)
{
    const uint64_t pv = A.pv;
    // one wave per kRunDefault items: at least one workgroup for an empty probe
    const uint32_t igrid = static_cast<uint32_t>(std::max<uint64_t>(1, (pv + 4u * dev::kRunDefault - 1u) / (4u * dev::kRunDefault)));
    // the cap is one item per probe value, a dense probe holds hundreds of times fewer: at most kListsMinW
    // workgroups per CU, whose waves stride over the real items (k_ix_tails: a wave per 16 items of the cap)
    const uint32_t dgrid = static_cast<uint32_t>(std::max<uint64_t>(
        1, std::min<uint64_t>((pv + 4u * dev::kIxRun - 1u) / (4u * dev::kIxRun), grid_cap(s, dev::kListsMinW))));
    return every ? ix_lookup<true>(A, dgrid, igrid, s) : ix_lookup<false>(A, dgrid, igrid, s);
}

hipError_t launch_lists_intersect(const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nunits, const uint64_t * ptr,
                                  const uint32_t * list_unit, uint64_t nlists, const uint32_t * start0, const uint32_t * unit_last,
                                  const uint32_t * probe, uint64_t pv, const uint64_t * probe_ptr, const uint32_t * qlist, uint64_t nq,
                                  uint32_t * out, uint64_t out_values, uint64_t * out_ptr, uint32_t * out_pidx, uint32_t * out_tpos,
                                  void * ws, unsigned long long * err, hipStream_t s)
{
    if (nq == 0)
    {
        hipError_t e = err ? fill_u32(err, 0xFFFFFFFFu, 2, s) : hipSuccess;
        return e != hipSuccess ? e : (out_ptr ? fill_u32(out_ptr, 0u, 2, s) : hipSuccess);
    }
    if (nq > 0x7FFFFFFFull || pv > 0x7FFFFFFFull || nlists > 0x7FFFFFFFull || nunits > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const IxWs W(ws, pv);
    const uint64_t nruns = (pv + 63u) / 64u;
    // one wave per 64 probe indices: at least one workgroup for an empty probe
    const uint32_t rgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (nruns + 3u) / 4u));
    hipError_t e = launch_items_reset(err, W.hdr, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch_ix_plan(ptr, list_unit, nlists, nunits, unit_last, probe, pv, probe_ptr, qlist, nq, W.hdr, W.pu, W.pl, s)) != hipSuccess)
        return e;
    if ((e = launch_items(pv, W.hdr, W.pu, W.pl, W.scani, W.ihead, W.iend, W.res, s)) != hipSuccess)
        return e;
    const dev::IxArgs A{in, in_bytes, off, nunits, ptr, list_unit, start0, unit_last, probe, pv, W.hdr, W.pu, W.pl, W.ihead, W.iend,
                        W.res, err};
    if ((e = launch_ix_lookup(A, false, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ix_hits, dim3(rgrid), dim3(256), 0, s, pv, W.hdr, W.res, W.scanh.tot);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u32_single(W.scanh.tot, nruns, W.scanh.pre, W.scanh.tile, &W.hdr->spare, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ix_out, dim3(flat_grid(std::max(nq + 1u, pv), s)), dim3(256), 0, s, list_unit, nunits, probe, pv, probe_ptr,
                       nq, W.hdr, W.pu, W.pl, W.res, W.scanh.pre, W.scanh.tile, out, out_values, out_ptr, out_pidx, out_tpos, err);
    return hipGetLastError();
}

} // namespace tpf
