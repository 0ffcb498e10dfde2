// p4_dec256v32.hip -- launches of the 256v32 decode kernel (p4_dec256v32.h)
// and the chained delta-1 decode: phase A
// (k_dsum256v32_lanes: p4_dsum_walk.h, p4_dsum_lanes.h), the run scan, phase B.
#include "p4_dec256v32.h"
#include "p4_dsum_walk.h"
#include "tpf_kernels.h"

#include "p4_lists.h"
#include "p4_scan.h"

namespace tpf::dev
{

// Last LDS byte position dsum_lanes may clamp to: its widest read is 9
// dwords from a clamped position (base_sum_lanes, the raw-vbyte loop), and
// the wave's window holds (WB + 64) / 4 dwords, so clamped reads stay inside
// the wave's own window (WB + 40 let them run 3 dwords into the
// next wave's).  Valid blocks lie inside [0, WB) and never reach the clamp.
template <uint32_t WB>
constexpr uint32_t kDsumLim = WB + 28u;
static_assert(kDsumLim<16384u> / 4u + 9u <= (16384u + 64u) / 4u, "clamped phase-A reads stay in the wave's window");

// LISTS (the many-lists decode, p4_lists.h): the units of a lists stream
// whose record carries kRecTail are p4Enc32 tails.  They are never parsed as
// 256v32: their lanes start out done with sum 0 (a tail is the last unit of
// its list, so its sum enters no start), and the kernel does nothing at all
// when the plan pass refused the list structure.
struct DsumNoLists
{
    static constexpr bool lists = false;
};
struct DsumLists
{
    static constexpr bool lists = true;
    const uint32_t * rec;  // one record per unit (kRecTail)
    const ListsHdr * hdr;  // go / no-go
    uint64_t nlists;
};

// Phase A of the chained decode (round 3) as the walk's policy
// (p4_dsum_walk.h): 256v32 blocks, u32 sums, one total per 64-block run.
template <uint32_t WB_, class X>
struct Dsum32
{
    using Sum = uint32_t;
    static constexpr bool lists = X::lists;
    static constexpr uint32_t WB = WB_, LIM = kDsumLim<WB_>, kSlot = kSlotBytes, kFbBytes = kSlotBytes + 4u * kWaveScratchU32;
    const DecArgs & A;
    const X & L;

    __device__ __forceinline__ uint64_t count() const { return A.nblocks; }
    __device__ __forceinline__ bool go() const
    {
        if constexpr (lists)
            return lists_go(L.hdr, A.nblocks);
        else
            return true;
    }
    __device__ __forceinline__ bool tail(uint64_t unit) const { return (L.rec[unit] & kRecTail) != 0u; }
    __device__ __forceinline__ bool lane_sum(const uint32_t * win, uint32_t p, uint32_t len, bool in_win, const uint32_t * tab,
                                             uint32_t & s) const
    {
        return dsum_lanes<LIM>(win, p, len, in_win, tab, s);
    }
    __device__ __forceinline__ uint32_t wave_unit(uint32_t * win, uint32_t sb, uint32_t t, uint32_t & sum) const
    {
        u32x4 v;
        const uint32_t used = decode_block256v32(win, sb, uni(lds_u32(win, sb)), win + kSlotBytes / 4u, t, v);
        sum = wave_sum(v.x + v.y + v.z + v.w + 4u);
        return used;
    }
    __device__ __forceinline__ void publish(uint64_t first, uint32_t sum_or_zero, uint32_t t) const
    {
        publish_run_total(A.run_tot, first / kLaneRun, sum_or_zero, t);
    }
};

template <uint32_t WB>
__global__ __launch_bounds__(256, 2) void k_dsum256v32_lanes(const DecArgs A)
{
    dsum_walk(Dsum32<WB, DsumNoLists>{A, DsumNoLists{}});
}

// phase A of the many-lists decode: the same sums, tails skipped
template <uint32_t WB>
__global__ __launch_bounds__(256, 2) void k_dsum256v32_lists(const DecArgs A, const DsumLists L)
{
    dsum_walk(Dsum32<WB, DsumLists>{A, L});
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
template <dev::StartMode SM>
hipError_t launch_mode(const dev::DecArgs & A, hipStream_t stream)
{
    constexpr uint32_t run = dev::kRunDefault;
    constexpr uint64_t per_wg = 4ull * run;
    const uint32_t grid = static_cast<uint32_t>((A.nblocks + per_wg - 1) / per_wg);
    // (plain decode only: the delta-1 modes' grouped form spills at 7 waves/SIMD)
    using dev::kDecPol, dev::kDecNC, dev::kDecMinW;
    if (SM == dev::StartMode::None && dev::dec_grouped(A.in_bytes, A.nblocks))
        hipLaunchKernelGGL((dev::k_dec256v32w<SM, run, kDecPol, kDecNC, kDecMinW, true, SM == dev::StartMode::None ? 1024u : 0u>),
                           dim3(grid), dim3(256), 0, stream, A);
    else
        hipLaunchKernelGGL((dev::k_dec256v32w<SM, run, kDecPol, kDecNC, kDecMinW, true, 0>), dim3(grid), dim3(256), 0, stream, A);
    return hipGetLastError();
}
} // namespace

hipError_t launch_dec256v32(const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nblocks, uint32_t * out,
                            const uint32_t * starts, unsigned long long * err, hipStream_t stream)
{
    if (nblocks == 0)
        return hipSuccess;
    const dev::DecArgs A{in, in_bytes, off, nblocks, out, starts, 0u, nullptr, err};
    return starts ? launch_mode<dev::StartMode::PerBlock>(A, stream) : launch_mode<dev::StartMode::None>(A, stream);
}

// Chained delta-1: phase A computes every block's sum of
// (v+1) and one sum per 16-block wave run, the run sums are scanned
// (p4_scan.h, mod 2^32); phase B decodes with start(i) = base + the run's
// base + the sums of the run's blocks before i.  A shard of a multi-GPU list
// runs A, exchanges its total with the other ranks, then B with its base.
static_assert(ChainWs<uint32_t>::kRun == dev::kRunDefault, "the chain workspace holds one scan entry per phase-B run");

// LDS staging window per wave of phase A (bytes)
constexpr uint32_t kDsumWindow = 16384;
constexpr uint32_t kDsumWgPerCu = (160u * 1024u) / (4u * (kDsumWindow + 64u) + 33u * 64u);

// Workspace: block sums (u32) + the run scan; both phases carve the same layout
// (phase A scans only its nblocks / kSumRun run sums).
size_t d1chain_workspace(uint64_t nblocks) { return ChainWs<uint32_t>::bytes(nblocks); }

hipError_t launch_d1chain_sums(const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nblocks, void * ws, size_t ws_bytes,
                               uint32_t * total, unsigned long long * err, hipStream_t stream)
{
    if (nblocks == 0)
        return total ? fill_u32(total, 0u, 1, stream) : hipSuccess;
    if (nblocks > 0x7FFFFFFFull || ws_bytes < d1chain_workspace(nblocks))
        return hipErrorInvalidValue;
    const ChainWs<uint32_t> w = ChainWs<uint32_t>::carve(ws, nblocks);
    const RunScanWs<uint32_t> & rs = w.scan;
    dev::DecArgs A{in, in_bytes, off, nblocks, nullptr, nullptr, 0u, w.sums, err};
    A.run_tot = rs.tot;
    // grid-stride over the runs: two workgroups per CU (the LDS windows admit two)
    constexpr uint64_t per_wg = 4ull * dev::kSumRun;
    const uint64_t wgs = std::min<uint64_t>((nblocks + per_wg - 1) / per_wg, grid_cap(stream, kDsumWgPerCu));
    hipLaunchKernelGGL((dev::k_dsum256v32_lanes<kDsumWindow>), dim3(static_cast<uint32_t>(wgs)), dim3(256), 0, stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    return launch_run_scan_u32(rs.tot, (nblocks + dev::kSumRun - 1u) / dev::kSumRun, rs.pre, rs.tile, total, stream);
}

// Phase A over a lists stream (p4_lists.hip): the chained decode's workspace
// layout and run scan, tails skipped through the unit records.
hipError_t launch_lists_sums(const ListsIndex & X, const uint32_t * rec, const dev::ListsHdr * hdr, void * ws, ChainView * view,
                             unsigned long long * err, hipStream_t stream)
{
    const uint64_t nunits = X.nunits;
    const ChainWs<uint32_t> w = ChainWs<uint32_t>::carve(ws, nunits);
    const RunScanWs<uint32_t> & rs = w.scan;
    dev::DecArgs A{X.in, X.in_bytes, X.off, nunits, nullptr, nullptr, 0u, w.sums, err};
    A.run_tot = rs.tot;
    *view = ChainView{w.sums, rs.pre, rs.tile};
    constexpr uint64_t per_wg = 4ull * dev::kSumRun;
    const uint64_t wgs = std::min<uint64_t>((nunits + per_wg - 1) / per_wg, grid_cap(stream, kDsumWgPerCu));
    hipLaunchKernelGGL((dev::k_dsum256v32_lists<kDsumWindow>), dim3(static_cast<uint32_t>(wgs)), dim3(256), 0, stream, A,
                       dev::DsumLists{rec, hdr, X.nlists});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    return launch_run_scan_u32(rs.tot, (nunits + dev::kSumRun - 1u) / dev::kSumRun, rs.pre, rs.tile, nullptr, stream);
}

hipError_t launch_d1chain_decode(const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nblocks, uint32_t * out,
                                 const void * ws, uint32_t base, unsigned long long * err, hipStream_t stream)
{
    if (nblocks == 0)
        return hipSuccess;
    const ChainWs<uint32_t> w = ChainWs<uint32_t>::carve(ws, nblocks);
    dev::DecArgs A{in, in_bytes, off, nblocks, out, w.sums, base, nullptr, err};
    A.run_pre = w.scan.pre;
    A.run_tile = w.scan.tile;
    return launch_mode<dev::StartMode::Prefix>(A, stream);
}

#if TPF_DSUM_ABLATE & 64
extern "C" int tpf_dsum_counters(unsigned long long * out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(dev::g_dsum_count), 16) == hipSuccess ? 0 : 1;
}
#endif

} // namespace tpf
