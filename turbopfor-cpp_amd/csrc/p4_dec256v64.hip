// p4_dec256v64.hip -- launches of the 128v64 / 256v64 decode kernel
// (p4_dec256v64.h) and the chained 64-bit delta-1 decode: phase A one lane
// per unit (k_dsum128v64_lanes, p4_dsum64_lanes.h), the u64 run scan, phase B.
#include "p4_dec256v64.h"
#include "p4_dsum64_lanes.h"
#include "p4_dsum_walk.h"
#include "tpf_kernels.h"

namespace tpf::dev
{

// Phase A of the chained 64-bit decode, one LANE per unit (round 4,
// p4_dsum64_lanes.h), as the walk's policy (p4_dsum_walk.h): every unit's
// u64 total and one total per 16-unit run (phase B's runs,
// k_dec128v64w<Prefix>) for the u64 run scan.

// Sum over each 16-lane row (u64 mod 2^64), valid in the row's last lane:
// three 32-bit DPP row scans of 16-bit pieces and the high word.
__device__ __forceinline__ uint64_t row16_sum64(uint64_t x)
{
    auto rs = [](uint32_t v) {
        v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false); // row_shr:1
        v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false); // row_shr:2
        v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false); // row_shr:4
        v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false); // row_shr:8
        return v;
    };
    const uint32_t sh = rs(static_cast<uint32_t>(x >> 32));
    const uint32_t sm = rs(static_cast<uint32_t>(x >> 16) & 0xFFFFu);
    const uint32_t sl = rs(static_cast<uint32_t>(x) & 0xFFFFu);
    return (static_cast<uint64_t>(sh) << 32) + (static_cast<uint64_t>(sm) << 16) + sl;
}

template <uint32_t WB>
constexpr uint32_t kDsum64Lim = WB + 28u;
static_assert(kDsum64Lim<16384u> / 4u + 6u <= (16384u + 64u) / 4u, "clamped phase-A reads stay in the wave's window");

template <uint32_t NB, uint32_t WB_>
struct Dsum64
{
    using Sum = uint64_t;
    static constexpr bool lists = false;
    static constexpr uint32_t WB = WB_, LIM = kDsum64Lim<WB_>, kSlot = kSlot64, kFbBytes = kSlot64 + 16u * kPos64;
    const Dec64Args & A;

    __device__ __forceinline__ uint64_t count() const { return A.nunits; }
    __device__ __forceinline__ bool go() const { return true; }
    __device__ __forceinline__ bool lane_sum(const uint32_t * win, uint32_t p, uint32_t len, bool in_win, const uint32_t * tab,
                                             uint64_t & s) const
    {
        return dsum64_lanes<NB, LIM>(win, p, len, in_win, tab, s);
    }
    __device__ __forceinline__ uint32_t wave_unit(uint32_t * win, uint32_t s0, uint32_t t, uint64_t & usum) const
    {
        uint64_t * scr = reinterpret_cast<uint64_t *>(win + kSlot64 / 4u);
        uint32_t sb = s0, wbad = 0u;
        usum = 0ull;
#pragma unroll
        for (uint32_t u = 0; u < NB; ++u)
        {
            uint64_t x0, x1;
            const uint32_t used = decode_block128v64(win, min(sb, kSlot64 - 64u), scr, t, x0, x1);
            sb += used & ~kWidthBad;
            wbad |= used & kWidthBad;
            usum += readlane_u64(wave_incl_scan64(x0 + x1 + 2ull), 63);
            wave_lds_sync();
        }
        return (sb - s0) | wbad;
    }
    // one total per 16-unit run (phase B's runs)
    __device__ __forceinline__ void publish(uint64_t first, uint64_t sum_or_zero, uint32_t t) const
    {
        const uint64_t rt = row16_sum64(sum_or_zero);
        const uint64_t r16 = first / kRun64 + (t >> 4);
        if ((t & 15u) == 15u && r16 < (A.nunits + kRun64 - 1u) / kRun64)
            A.run_tot[r16] = rt;
    }
};

template <uint32_t NB, uint32_t WB>
__global__ __launch_bounds__(256, 2) void k_dsum128v64_lanes(const Dec64Args A)
{
    dsum_walk(Dsum64<NB, WB>{A});
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
template <dev::Start64 SM>
hipError_t launch64(uint32_t nb, const dev::Dec64Args & A, hipStream_t s)
{
    const uint32_t grid = static_cast<uint32_t>((A.nunits + 4u * dev::kRun64 - 1u) / (4u * dev::kRun64));
    if (nb == 2u)
        hipLaunchKernelGGL((dev::k_dec128v64w<2, SM>), dim3(grid), dim3(256), 0, s, A);
    else
        hipLaunchKernelGGL((dev::k_dec128v64w<1, SM>), dim3(grid), dim3(256), 0, s, A);
    return hipGetLastError();
}

static_assert(ChainWs<uint64_t>::kRun == dev::kRun64, "the chain workspace holds one scan entry per phase-B run");
} // namespace

// fmt 128v64 (nb = 1) or 256v64 (nb = 2), n == 128 * nb values per unit.
hipError_t launch_dec128v64(uint32_t nb, const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nunits,
                            uint64_t * out, const uint64_t * starts, unsigned long long * err, hipStream_t s)
{
    if (nunits == 0)
        return hipSuccess;
    dev::Dec64Args A{in, in_bytes, off, nunits, out, starts, 0ull, nullptr, nullptr, nullptr, nullptr, err};
    return starts ? launch64<dev::Start64::PerUnit>(nb, A, s) : launch64<dev::Start64::None>(nb, A, s);
}

// Chained delta-1 decode of a 64-bit list (128v64 / 256v64 units chained the
// way reference callers chain p4D1Enc256v64, README.md:116-123; inside a
// 256v64 unit the second block already starts from the first's last value,
// p4d1dec256v64_scalar.cpp:15-32).  Phase A: every unit's delta total and one
// total per 16-unit run, then the run scan (u64, mod 2^64); phase B decodes
// with start(i) = base + the totals before i.
size_t d1chain64_workspace(uint64_t nunits) { return ChainWs<uint64_t>::bytes(nunits); }

hipError_t launch_d1chain64_sums(uint32_t nb, const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nunits, void * ws,
                                 size_t ws_bytes, uint64_t * total, unsigned long long * err, hipStream_t s)
{
    if (nunits == 0)
        return total ? fill_u32(total, 0u, 2, s) : hipSuccess;
    if (ws_bytes < d1chain64_workspace(nunits))
        return hipErrorInvalidValue;
    const ChainWs<uint64_t> w = ChainWs<uint64_t>::carve(ws, nunits);
    dev::Dec64Args A{in, in_bytes, off, nunits, nullptr, nullptr, 0ull, w.sums, w.scan.tot, nullptr, nullptr, err};
    // lane-per-unit phase A (round 4; the decoder's Sum mode before it:
    // 4.69 -> 1.53 ms per 10M units), grid-stride over 64-unit runs, two
    // workgroups per CU (the LDS windows admit two)
    constexpr uint64_t per_wg = 4ull * dev::kLaneRun;
    const uint64_t wgs = std::min<uint64_t>((nunits + per_wg - 1) / per_wg, grid_cap(s, 2));
    if (nb == 2u)
        hipLaunchKernelGGL((dev::k_dsum128v64_lanes<2, 16384>), dim3(static_cast<uint32_t>(wgs)), dim3(256), 0, s, A);
    else
        hipLaunchKernelGGL((dev::k_dsum128v64_lanes<1, 16384>), dim3(static_cast<uint32_t>(wgs)), dim3(256), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    return launch_run_scan_u64t(w.scan.tot, ChainWs<uint64_t>::runs(nunits), w.scan.pre, w.scan.tile, total, s);
}

hipError_t launch_d1chain64_decode(uint32_t nb, const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nunits,
                                   uint64_t * out, const void * ws, uint64_t base, unsigned long long * err, hipStream_t s)
{
    if (nunits == 0)
        return hipSuccess;
    const ChainWs<uint64_t> w = ChainWs<uint64_t>::carve(ws, nunits);
    dev::Dec64Args A{in, in_bytes, off, nunits, out, w.sums, base, nullptr, nullptr, w.scan.pre, w.scan.tile, err};
    return launch64<dev::Start64::Prefix>(nb, A, s);
}

} // namespace tpf
