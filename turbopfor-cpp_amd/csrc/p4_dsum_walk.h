// p4_dsum_walk.h -- the phase-A walk of both chained delta-1 decodes
// (k_dsum256v32_lanes / k_dsum256v32_lists, p4_dec256v32.hip;
// k_dsum128v64_lanes, p4_dec256v64.hip): the delta sums of 64-unit runs, one
// lane per unit, and the totals the run scan needs.
//
// A wave stages a run's bytes into its LDS window with coalesced 16-byte
// loads -- in passes of at most WB bytes starting at the first unit not yet
// summed, each pass summing every unit that lies wholly inside it -- and the
// units the lane path declines go through the wave decoder one at a time.
// Waves walk the runs grid-stride and load the NEXT pass (the same run's next
// window, or the next run's first) into registers while they sum the current
// one, so the loads of one pass overlap the arithmetic of the previous
// (measured without that overlap: staging alone 0.46 ms, staging + sums
// 1.30 ms per 10M C3 blocks).  Phase B's 16-unit runs nest in the 64-unit runs.
//
// What differs between the widths is a policy P:
//   Sum                 uint32_t / uint64_t
//   WB, LIM             window bytes per pass; last LDS byte a lane sum may clamp to
//   kSlot, kFbBytes     the wave decoder's staged bytes per unit; slot + scratch bytes
//   A                   the args: in, in_bytes, off, sums, err; count() its units
//   lists, go(), tail() the many-lists decode's hook (p4_dec256v32.hip)
//   lane_sum(win, p, len, in_win, tab, s)   the lane path; false: declined
//   wave_unit(win, sb, t, sum)              the exact decode of one unit staged at
//                                           byte sb of win: bytes used | width flags
//   publish(first, sum_or_zero, t)          the run's total(s) for the run scan
#pragma once

#include "p4_dsum_lanes.h"

// Phase-A ablation (measurement builds only, scripts/chain_phase_probe.py;
// the library is built with 0): TPF_DSUM_ABLATE bits 1 / 2 / 4 / 8 skip the
// base-payload sums / compressed vbyte / raw vbyte / position checks
// (p4_dsum_lanes.h), 16 stages only, 32 sends no unit to the wave decoder,
// 64 counts the fallback units and staging passes (tpf_dsum_counters).
namespace tpf::dev
{

#if TPF_DSUM_ABLATE & 64
static __device__ unsigned long long g_dsum_count[2]; // units sent to the wave decoder, staging passes
#endif

// One 64-unit run of phase A as lanes see it.
struct DsumRun
{
    uint64_t first = 0, o = 0, e = 0, rend = 0;
    uint32_t n = 0, len = 0;
    bool valid = false, fb = false, done = true;

    template <class P>
    __device__ __forceinline__ void load(const P & pol, uint64_t run, uint32_t t)
    {
        first = run * kLaneRun;
        n = static_cast<uint32_t>(min_u64(kLaneRun, pol.count() - first));
        valid = t < n;
        o = valid ? pol.A.off[first + t] : 0ull;
        e = valid ? pol.A.off[first + t + 1u] : 0ull;
        len = (e >= o && e - o < 0x10000ull) ? static_cast<uint32_t>(e - o) : 0xFFFFFFFFu;
        // units larger than a window (or with implausible offsets) go to the wave decoder
        fb = valid && (len > P::WB - 32u || e > pol.A.in_bytes);
        done = !valid || fb;
        // end of the run's bytes: a pass never stages past it, so neighbouring
        // runs do not re-read each other's bytes (offsets ascend in a valid stream)
        rend = readlane_u64(e, n - 1u);
        // a lists stream's tails start out done with sum 0
        if constexpr (P::lists)
            if (valid && pol.tail(first + t))
            {
                fb = false;
                done = true;
            }
    }

    // The next staging pass: [wbase, wbase + span) starting at the first unit
    // not yet summed (it always fits); false when every unit is done.
    template <uint32_t WB>
    __device__ __forceinline__ bool pass(uint64_t in_bytes, uint64_t & wbase, uint32_t & span, uint32_t & avail) const
    {
        const uint64_t pend = __ballot(!done);
        if (pend == 0ull)
            return false;
        const uint32_t lead = static_cast<uint32_t>(__builtin_ctzll(pend));
        const uint64_t ws = readlane_u64(o, lead);
        const uint64_t we = readlane_u64(e, lead);
        wbase = ws & ~15ull;
        span = static_cast<uint32_t>(min_u64(wbase + WB, rend > we ? rend : we) - wbase);
        avail = static_cast<uint32_t>(min_u64(sub_sat(in_bytes, wbase), WB));
        return true;
    }
};

template <class P>
__device__ __forceinline__ void dsum_walk(const P & pol)
{
    using Sum = typename P::Sum;
    constexpr uint32_t WB = P::WB;
    const auto & A = pol.A;
    if (!pol.go())
        return;
    static_assert(WB % 1024u == 0u && WB + 64u >= P::kFbBytes, "the window also hosts the fallback's slot and scratch");
    constexpr uint32_t NL = WB / 1024u; // 16-byte loads per lane per pass
    __shared__ uint32_t tab[33 * kSumTabRow];
    __shared__ __attribute__((aligned(16))) uint32_t win_all[4][(WB + 64u) / 4u];
    if (threadIdx.x < 33u)
        build_sum_row(tab + threadIdx.x * kSumTabRow, threadIdx.x);
    __syncthreads();
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint64_t nruns = (pol.count() + kLaneRun - 1u) / kLaneRun;
    const uint64_t rstride = static_cast<uint64_t>(gridDim.x) * 4u;
    uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + wv;
    if (run >= nruns)
        return;
    uint32_t * win = win_all[wv];
    const uint64_t in_base = reinterpret_cast<uint64_t>(A.in);
    const uint64_t in_end = in_base + A.in_bytes;

    // the pass in flight: its loads land in r[]
    u32x4 r[NL];
    uint64_t wbase = 0;
    uint32_t span = 0, avail = 0;
    auto issue = [&]() {
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(A.in + wbase, avail);
#pragma unroll
        for (uint32_t i = 0; i < NL; ++i)
        {
            // unconditional: chunks past the span get an out-of-range offset
            // (zeros, no traffic); a chunk straddling the end of the stream
            // reads zeros and is patched byte-wise when staged
            const uint32_t x = 16u * t + 1024u * i;
            r[i] = buf_load16(rs, x < span ? x : 0x80000000u);
        }
    };

    DsumRun cur;
    cur.load(pol, run, t);
    Sum sumv = 0;
    cur.pass<WB>(A.in_bytes, wbase, span, avail); // the lead lane of a fresh run is pending or every lane declined
    issue();
    for (;;)
    {
        // ---- stage the pass in flight
        const uint64_t pbase = wbase;
        const uint32_t pspan = span;
        // unconditional (round 6): chunks past the span hold the zeros their
        // out-of-range loads returned, and no unit summed from this pass
        // reaches them (a per-chunk test cost an exec-mask branch per chunk)
#pragma unroll
        for (uint32_t i = 0; i < NL; ++i)
            reinterpret_cast<u32x4 *>(win)[(16u * t + 1024u * i) >> 4] = r[i];
        {
            const uint32_t xs = avail & ~15u;
            if (xs < pspan && (avail & 15u) != 0u && t == ((xs >> 4) & 63u))
                reinterpret_cast<u32x4 *>(win)[xs >> 4] =
                    load16_guarded(A.in + pbase, make_rsrc(A.in + pbase, avail), xs, avail);
        }
        wave_lds_sync();
#if TPF_DSUM_ABLATE & 64
        if (t == 0)
            atomicAdd(&g_dsum_count[1], 1ull);
#endif
        const bool in_win = !cur.done && cur.o >= pbase && cur.e <= pbase + pspan;
        cur.done = cur.done || in_win;
        // ---- put the next pass in flight: the same run's next window, or the next run's first
        DsumRun nxt;
        bool run_end = false, last = false;
        if (!cur.pass<WB>(A.in_bytes, wbase, span, avail))
        {
            run_end = true;
            const uint64_t nrun = run + rstride;
            last = nrun >= nruns;
            if (!last)
            {
                nxt.load(pol, nrun, t);
                if (!nxt.pass<WB>(A.in_bytes, wbase, span, avail))
                    span = 0u; // every unit of that run declined: nothing to stage
            }
            else
                span = 0u;
        }
        if (span != 0u)
            issue();
        // ---- sum the staged pass
        const uint32_t p = in_win ? static_cast<uint32_t>(cur.o - pbase) : 0u;
        Sum s = 0;
#if TPF_DSUM_ABLATE & 16
        const bool ok = true;
#else
        const bool ok = pol.lane_sum(win, p, cur.len, in_win, tab, s);
#endif
        sumv = in_win ? s : sumv;
        cur.fb = cur.fb || (in_win && !ok);
        if (!run_end)
        {
            wave_lds_sync(); // the window is restaged next
            continue;
        }
        wave_lds_sync();
        // ---- the run is summed: the declined units, one at a time through
        // the wave decoder (exact: duplicate vbyte positions OR, as in the
        // reference, and the plain decode's length check); the next pass is in
        // registers, so the window is free
        uint64_t fbm = __ballot(cur.fb);
#if TPF_DSUM_ABLATE & 64
        if (t == 0)
            atomicAdd(&g_dsum_count[0], static_cast<unsigned long long>(__builtin_popcountll(fbm)));
#endif
#if TPF_DSUM_ABLATE & 32
        fbm = 0ull;
#endif
        uint64_t badmask = 0ull;
        while (fbm != 0ull)
        {
            const uint32_t j = static_cast<uint32_t>(__builtin_ctzll(fbm));
            fbm &= fbm - 1ull;
            const uint64_t ab = in_base + readlane_u64(cur.o, j);
            const uint64_t cb = ab & ~15ull;
            // the plain decode stages at most kSlot - 64 bytes of a unit (RunPlaneT)
            const uint32_t sp = static_cast<uint32_t>(min_u64(sub_sat(in_base + readlane_u64(cur.e, j), cb), P::kSlot - 64u));
            const uint32_t av = static_cast<uint32_t>(min_u64(sub_sat(in_end, cb), P::kSlot));
            const __amdgpu_buffer_rsrc_t rb = make_rsrc(reinterpret_cast<const void *>(cb), av);
            for (uint32_t x = 16u * t; x < sp; x += 1024u)
                reinterpret_cast<u32x4 *>(win)[x >> 4] = load16_guarded(reinterpret_cast<const uint8_t *>(cb), rb, x, av);
            wave_lds_sync();
            Sum usum;
            const uint32_t used = pol.wave_unit(win, static_cast<uint32_t>(ab & 15u), t, usum);
            sumv = t == j ? usum : sumv;
            if (used != rl(cur.len, j))
                badmask |= 1ull << j;
            wave_lds_sync();
        }
        if (cur.valid)
            A.sums[cur.first + t] = sumv;
        pol.publish(cur.first, cur.valid ? sumv : Sum(0), t);
        if (A.err != nullptr && t == 0 && badmask != 0ull)
            atomicMin(A.err, static_cast<unsigned long long>(cur.first + __builtin_ctzll(badmask)));
        if (last)
            break;
        run += rstride;
        cur = nxt;
        sumv = 0;
        if (span == 0u)
        {
            // the new run has nothing to stage (all declined): an empty pass
            wbase = 0;
            avail = 0;
        }
    }
}

} // namespace tpf::dev
