// p4_lists_host.h -- host helpers shared by the launch functions of the lists
// entry points (p4_lists*.hip): the grids, the launch of one kernel with its
// error, and the workspace prefix the selective decode and the units decode
// share (internal; the workspace carver is tpf_ws.h).
#pragma once

#include <type_traits>

#include "p4_lists.h"
#include "p4_scan.h"
#include "tpf_kernels.h"

namespace tpf
{

// workgroups of 256 threads for a grid-stride kernel over `items`
inline uint32_t flat_grid(uint64_t items, hipStream_t s)
{
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((items + 255u) / 256u, grid_cap(s, 8))));
}

// workgroups of 4 waves for a kernel that gives every wave `per_wave` items
inline uint32_t wave_grid(uint64_t items, uint64_t per_wave) { return static_cast<uint32_t>((items + 4u * per_wave - 1u) / (4u * per_wave)); }

// One kernel launch on stream s, and what it left.
template <class... P, class... A>
inline hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, const A &... args)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
    return hipGetLastError();
}

// The same for a kernel whose first template parameter is a runtime flag of
// the call (delta-1 or plain): pick(flag) names the instance, as in
//   launch_by(d1, [](auto D1) { return dev::k_un_tails<D1, dev::kTailsNC>; }, grid, 256, s, A)
template <class Pick, class... A>
inline hipError_t launch_by(bool flag, Pick pick, dim3 grid, dim3 block, hipStream_t s, const A &... args)
{
    return flag ? launch(pick(std::true_type{}), grid, block, s, args...) : launch(pick(std::false_type{}), grid, block, s, args...);
}

// Workspace prefix of a decode over a selection: header | run scan of the
// selections' unit counts | their value counts and that scan (u64) | vbase
// (nsel + 1), each 256-byte aligned.
struct SelPlanWs
{
    dev::SelHdr * hdr;
    RunScanWs<uint64_t> scanu;
    uint64_t *totv, *prev, *tilev;
    uint32_t * vbase;

    SelPlanWs(WsCarver & c, uint64_t nsel)
    {
        hdr = c.take<dev::SelHdr>(1);
        scanu = c.scan<uint64_t>(nsel);
        totv = c.take<uint64_t>(nsel);
        prev = c.take<uint64_t>(nsel);
        tilev = c.bytes<uint64_t>(al256(8u * RunScanWs<uint64_t>::tiles(nsel)) + 256u);
        vbase = c.take<uint32_t>(nsel + 1u);
    }
};

} // namespace tpf
