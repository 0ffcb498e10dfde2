// p4_lists_dev.h -- device helpers shared by the many-lists decode
// (p4_lists.hip), its selective form (p4_lists_select.hip) and the many-lists
// encode (p4_lists_enc.hip): the pipeline shapes, a list's unit count, and how
// every lane of a wave's run of units finds its list from the unit records
// (p4_lists.h).  Device code only: included by *.hip files (internal).
#pragma once

#include "p4_lists.h"
#include "tpf_device.h"

namespace tpf::dev
{

// pipeline shapes of the lists decodes (p4_lists.hip, p4_lists_select.hip)
constexpr uint32_t kListSlot = 2432;      // tails: the generic decoder's slot (a 2,304-byte image + 128)
constexpr uint32_t kListScratchU32 = 512; // decode_block_g<H32>'s scratch
constexpr uint32_t kListsNC = 6;          // full blocks: the k_dec256v32w pipeline, 7 waves per SIMD
constexpr int kListsMinW = 7;
constexpr uint32_t kTailsNC = 4;          // tails: the k_dec_gr pipeline

__device__ __forceinline__ uint32_t list_units(uint64_t n)
{
    // more units than any stream may hold: clamped, so the total cannot wrap back to nunits
    const uint64_t u = (n >> 8) + ((n & 255u) != 0u ? 1u : 0u);
    return u > 0x80000000ull ? 0x80000000u : static_cast<uint32_t>(u);
}

// Inclusive max-scan over the wave (identity 0).
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x)
{
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xa, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xc, 0xf, false));
    return x;
}

// The list holding unit `first`: the last j with ubase[j] <= first, by a
// cooperative search -- 64 pivots per step, so 2^24 lists take 4 dependent
// loads.  Invariant: ubase[lo] <= first < ubase[hi] (ubase[nlists] = nunits).
__device__ __forceinline__ uint32_t find_list(const uint32_t * __restrict ubase, uint32_t nlists, uint32_t first, uint32_t t)
{
    uint32_t lo = 0u, hi = nlists;
    while (hi - lo > 1u)
    {
        const uint32_t step = (hi - lo + 63u) / 64u;
        const uint64_t p = static_cast<uint64_t>(lo) + static_cast<uint64_t>(t + 1u) * step;
        const bool le = p < hi && ubase[p] <= first;
        const uint32_t c = static_cast<uint32_t>(__builtin_popcountll(__ballot(le))); // ubase ascends: the first c pivots
        lo = uni(lo + c * step);
        hi = uni(umin32(hi, lo + step));
    }
    return lo;
}

} // namespace tpf::dev
