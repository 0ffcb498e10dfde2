// p4_lists_host.h -- host helpers shared by the launch functions of the lists
// entry points (p4_lists*.hip): the grid of a grid-stride kernel and the
// workspace prefix the selective decode and the units decode share (internal;
// the workspace carver is tpf_ws.h).
#pragma once

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
