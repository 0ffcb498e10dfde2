// p4_lists_items.h -- the item drivers: how the entries that serve a request
// item by item (the intersection's lookup, p4_lists_intersect.hip, which the
// union and the difference run too; the gather, p4_lists_gather.hip) decode
// every item's unit once into the wave's LDS and hand it to the entry's
// `serve`.  The item layer itself -- heads, items -- is p4_lists_items.hip.
// serve(vals, cnt, h, e, t): the unit's cnt values in vals[0 .. 256), the rest
// padded, for the request indices [h, e) of the item, lane t of the wave.
// Device code only: included by *.hip files (internal).
#pragma once

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"

namespace tpf::dev
{

// Full blocks: every wave takes runs of RUN consecutive ITEMS through the
// k_dec256v32w pipeline, as k_un_dec does with virtual units.  Lane t gathers
// item first + t: its head's unit word, the offsets of the source unit and,
// with D1, its list and its start (unit_start, p4_lists_dev.h); the plain form
// skips both loads.  The plan checked list < nlists and list_unit[list] <= su
// < list_unit[list + 1] <= nunits for every request index it gave a unit.
// Where k_un_dec stores the block, this keeps it in 1 KB of LDS per wave.  A
// wave waits for its item's request once per block (that load sits behind the
// chunk loads in issue order), so callers take short runs over many waves.
// `stride`: the items the grid takes per trip (the kernel states it: it is
// what the host's cap on the grid is held against).
template <bool D1, uint32_t RUN, uint32_t NC, class Serve>
__device__ __forceinline__ void item_full_units(const ItemArgs & A, uint64_t stride, Serve && serve)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    __shared__ uint32_t vals[4][256];
    // per item of the run, read back wave-uniformly: the source unit (for the
    // error report only, as in k_sel_dec), the request range and the start --
    // held in registers across the pipeline they cost spilled VGPRs at 7 waves
    __shared__ uint32_t srcu[4][RUN], itemh[4][RUN], iteme[4][RUN], starts[4][D1 ? RUN : 1];
    const ListsIndex & X = A.ix;
    constexpr uint32_t kRun = RUN;
    const uint64_t nit = A.hdr->nitems;
    WaveRun R = wave_run(X.in, X.in_bytes, kRun, nit);
    const uint32_t t = R.t, wv = R.wv;
    uint32_t * slot = slots[wv];
    uint32_t * scr = scratch[wv];
    // the host knows only the cap of one item per request index: the grid covers
    // the device and every wave strides over the runs of the real item count
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
        // (the list is gathered before the offsets and the four words are
        // written together, after the start: with the words first and the list
        // behind the offsets the lookup's 150 us legs ran 1 us slower,
        // DESIGN.md 4.19)
        uint32_t lj = 0u;
        if constexpr (D1)
            lj = full ? A.pl[ih] : 0u;
        const uint64_t o = full ? X.off[su] : 0ull;
        const uint64_t e = full ? X.off[su + 1u] : 0ull;
        RunPlaneT<kSlotBytes, true> P;
        P.init(R.in_base, R.in_end, o, e, full);
        {
            uint32_t startv = 0u;
            if constexpr (D1)
            {
                if (full)
                    startv = unit_start(X.list_unit, X.start0, X.unit_last, lj, su);
            }
            if (t < kRun)
            {
                srcu[wv][t] = full ? su : 0xFFFFFFFFu;
                itemh[wv][t] = ih;
                iteme[wv][t] = ie;
                if constexpr (D1)
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
            decode_full_unit<D1>(P, c, jj, slot, scr, D1 ? uni(starts[wv][jj]) : 0u, t, x, badmask);
            reinterpret_cast<u32x4 *>(vals[wv])[t] = x;
            wave_lds_sync();
            serve(vals[wv], 256u, uni(itemh[wv][jj]), uni(iteme[wv][jj]), t);
            wave_lds_sync();
        });
        report_bad_units(A.err, badmask, t < kRun ? srcu[wv][t] : 0xFFFFFFFFu, t);
        wave_lds_sync(); // the item words are rewritten by the next run
    }
}

// Tails: every wave owns kRunDefault consecutive ITEMS through the tails driver
// (tail_units, p4_lists_dev.h); lane t holds item first + t when its unit is
// its list's p4Enc32 tail, n % 256 values.  The words of vals past the unit's
// count hold `pad`.
template <bool D1, uint32_t NC, class Serve>
__device__ __forceinline__ void item_tail_units(const ItemArgs & A, uint32_t pad, Serve && serve)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    __shared__ uint32_t vals[4][256];
    const ListsIndex & X = A.ix;
    const uint64_t nit = A.hdr->nitems;
    const WaveRun R = wave_run(X.in, X.in_bytes, kRunDefault, nit);
    const uint32_t t = R.t, wv = R.wv;
    if (R.first >= nit)
        return;
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
    const uint32_t cnt = has ? static_cast<uint32_t>((X.ptr[lj + 1u] - X.ptr[lj]) & 255u) : 0u; // != 0: the plan saw a tail
    tail_units<D1, NC>(
        R, X.off, has, hasmask, su, cnt, slots[wv], scratch[wv], A.err,
        [&] { return D1 && has ? unit_start(X.list_unit, X.start0, X.unit_last, lj, su) : 0u; },
        [&](uint32_t jj, uint32_t cj, const TailVals & x) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                vals[wv][t + 64u * q] = t + 64u * q < cj ? x.v[q] : pad;
            wave_lds_sync();
            serve(vals[wv], cj, rl(ih, jj), rl(ie, jj), t);
        });
}

} // namespace tpf::dev
