// p4_lists_extract.hip -- tpf_lists_extract: a sub-index of a resident index,
// moved as bytes in one submission with no host round trip
// (include/turbopfor_gpu.h).  A unit's bytes depend on its
// values and the value before it only, so units [a, a + c) of
// a list are the encoder's own stream for the values of that range, started
// from d_start0[j] when a == 0 and from the skip table's entry of unit a - 1
// otherwise: nothing is parsed, decoded or encoded.
//   reset  : the header
//   plan   : a thread per selection (grid-stride): the checks, its units c,
//            its values n, its bytes b = off[hi] - off[lo] and the source unit
//            of its first; three run totals per 64 selections
//   scans  : run scans of the three (p4_scan.h)
//   heads  : the verdict, then per selection (grid-stride) d_list_ptr_out,
//            d_list_unit_out, d_start0_out and its first output byte; the
//            thread past the last selection holds the three totals: it writes
//            the stream's length and the capacity verdict (the append's segs
//            pass has the staged encode to wait for, this call has not)
//   offsets: a thread per output unit: d_off_out and d_unit_last_out
//   move   : the output cut into kListsAppendTile-byte tiles of d_out, a wave
//            per tile (stitch_tile, p4_lists_stitch.h, with no new bytes)
// Every kernel after the heads reads the go flag of the header first.
#include "p4_lists.h"

#include "p4_lists_dev.h"
#include "p4_lists_host.h"
#include "p4_lists_stitch.h"
#include "turbopfor_gpu.h"

#include <algorithm>

namespace tpf::dev
{

struct ExtHdr
{
    unsigned long long bad;        // first refused selection (~0: none)
    unsigned long long nu, nv, nb; // totals of the three scans: units, values, bytes
    unsigned long long nunits_out;
    uint32_t go;  // the heads pass: the selections and units_cap are sound
    uint32_t fit; // the heads pass: the stream fits out_cap
};

struct ExtArgs
{
    ListsIndex ix;
    const uint32_t *sel, *ufirst, *ucount; // ufirst == nullptr: whole lists
    uint64_t nsel;
    uint8_t * out;
    uint64_t out_cap;
    uint64_t * off_out;
    uint64_t units_cap;
    uint64_t * lptr_out;
    uint32_t * lunit_out;
    uint32_t * start0_out;
    uint32_t * ulast_out;
    unsigned long long * err;
    // workspace
    ExtHdr * hdr;
    uint64_t *c_tot, *n_tot, *b_tot; // run totals
    const uint64_t *c_pre, *c_tile, *n_pre, *n_tile, *b_pre, *b_tile;
    uint32_t *c, *src0; // per selection: its units, the source unit of its first
    uint64_t *nv, *nb;  // per selection: its values, its bytes
    uint64_t * lstart;  // nsel + 1: first output byte of every selection
};

__device__ __forceinline__ void ext_err(unsigned long long * err, unsigned long long v)
{
    if (err != nullptr)
        atomicMin(err, v);
}

__global__ void k_ext_reset(ExtHdr * hdr)
{
    if (threadIdx.x == 0)
        *hdr = ExtHdr{~0ull, 0ull, 0ull, 0ull, 0ull, 0u, 0u};
}

// nsel == 0: the empty result
__global__ void k_ext_empty(uint64_t * lptr_out, uint32_t * lunit_out, uint64_t * off_out)
{
    if (threadIdx.x == 0)
    {
        lptr_out[0] = 0ull;
        lunit_out[0] = 0u;
        off_out[0] = 0ull;
    }
}

__device__ __forceinline__ void publish_run_total64(uint64_t * __restrict run_tot, uint64_t run, uint64_t x, uint32_t t)
{
    const uint64_t s = readlane_u64(wave_incl_scan64(x), 63);
    if (t == 0)
        run_tot[run] = s;
}

// ---- plan ---------------------------------------------------------------------
// The grid's stride is a multiple of 64: a wave walks whole 64-runs, and k - t,
// the run's first selection, is the same in all its lanes.
__global__ __launch_bounds__(256) void k_ext_plan(const ExtArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    const uint32_t t = threadIdx.x & 63u;
    for (uint64_t k = gid; k - t < A.nsel; k += gsz)
    {
        uint32_t c = 0u;
        uint64_t nv = 0ull, nb = 0ull;
        if (k < A.nsel)
        {
            uint64_t n;
            uint32_t ua, ub, s0 = 0u;
            bool bad = !list_dir_ok(A.ix.ptr, A.ix.list_unit, A.ix.nlists, A.ix.nunits, A.sel[k], &n, &ua, &ub);
            if (!bad)
            {
                const uint32_t units = ub - ua;
                const uint64_t uf = A.ufirst != nullptr ? A.ufirst[k] : 0u;
                const uint64_t uc = A.ufirst != nullptr ? A.ucount[k] : units;
                bad = uf + uc > units;
                if (!bad)
                {
                    s0 = ua + static_cast<uint32_t>(uf); // <= ub <= nunits
                    if (uc != 0u)
                    {
                        // the ends of the copied range
                        const uint64_t o0 = A.ix.off[s0], o1 = A.ix.off[s0 + uc];
                        bad = o0 > o1 || o1 > A.ix.in_bytes;
                        if (!bad)
                        {
                            const uint32_t r = static_cast<uint32_t>(n & 255u);
                            c = static_cast<uint32_t>(uc);
                            nb = o1 - o0;
                            nv = 256ull * uc - (uf + uc == units && r != 0u ? 256u - r : 0u); // the range reaches the tail
                        }
                    }
                }
            }
            if (bad)
                atomicMin(&A.hdr->bad, static_cast<unsigned long long>(k));
            A.c[k] = c;
            A.src0[k] = s0;
            A.nv[k] = nv;
            A.nb[k] = nb;
        }
        const uint64_t run = k / 64u;
        publish_run_total64(A.c_tot, run, c, t);
        publish_run_total64(A.n_tot, run, nv, t);
        publish_run_total64(A.b_tot, run, nb, t);
    }
}

// ---- heads --------------------------------------------------------------------
template <bool D1>
__global__ __launch_bounds__(256) void k_ext_heads(const ExtArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    const uint32_t t = threadIdx.x & 63u;
    const ExtHdr h = *A.hdr;
    const uint64_t ebase = A.ix.nunits;
    if (h.bad != ~0ull)
    {
        if (gid == 0)
            ext_err(A.err, ebase + h.bad);
        return;
    }
    const bool ufit = h.nu <= A.units_cap && h.nu <= 0x7FFFFFFFull;
    for (uint64_t k = gid; k - t <= A.nsel; k += gsz)
    {
        const bool in = k < A.nsel;
        const uint64_t c = in ? A.c[k] : 0u, nv = in ? A.nv[k] : 0ull, nb = in ? A.nb[k] : 0ull;
        // exclusive prefixes: the run's base plus the wave's scan (every lane of the wave takes part)
        uint64_t C = wave_incl_scan64(c) - c, NV = wave_incl_scan64(nv) - nv, NB = wave_incl_scan64(nb) - nb;
        if (k > A.nsel)
            continue;
        if (in)
        {
            const uint64_t run = k / 64u;
            C += run_base(A.c_pre, A.c_tile, run);
            NV += run_base(A.n_pre, A.n_tile, run);
            NB += run_base(A.b_pre, A.b_tile, run);
        }
        else
        {
            C = h.nu, NV = h.nv, NB = h.nb;
        }
        A.lptr_out[k] = NV;
        A.lunit_out[k] = static_cast<uint32_t>(C);
        if constexpr (D1)
        {
            if (in)
            {
                // the range continues its list: from the unit before it, or from start0
                const uint32_t j = A.sel[k];
                const bool first = A.ufirst == nullptr || A.ufirst[k] == 0u;
                A.start0_out[k] = first ? (A.ix.start0 != nullptr ? A.ix.start0[j] : 0u) : A.ix.unit_last[A.src0[k] - 1u];
            }
        }
        if (!ufit)
        {
            if (!in)
                ext_err(A.err, ebase + A.nsel);
            continue;
        }
        A.lstart[k] = NB;
        if (!in)
        {
            A.off_out[h.nu] = NB;
            A.hdr->nunits_out = h.nu;
            A.hdr->go = 1u;
            if (NB > A.out_cap)
                ext_err(A.err, ebase + A.nsel + 1u);
            else
                A.hdr->fit = 1u;
        }
    }
}

// ---- offsets ------------------------------------------------------------------
template <bool UL>
__global__ __launch_bounds__(256) void k_ext_offsets(const ExtArgs A)
{
    if (A.hdr->go == 0u)
        return;
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t nuo = A.hdr->nunits_out;
    if (u - t >= nuo)
        return;
    // the last k with lunit_out[k] <= u (lunit_out[0] = 0 <= u < lunit_out[nsel]), as k_app_offsets finds its list
    const uint32_t k0 = find_list(A.lunit_out, static_cast<uint32_t>(A.nsel), static_cast<uint32_t>(u - t), t); // u - t < nuo < 2^31
    if (u >= nuo)
        return;
    const uint64_t k = gallop(A.lunit_out, static_cast<uint32_t>(A.nsel), k0, u);
    const uint32_t local = static_cast<uint32_t>(u) - A.lunit_out[k];
    const uint32_t su = A.src0[k];
    A.off_out[u] = A.lstart[k] + (A.ix.off[su + local] - A.ix.off[su]);
    if constexpr (UL)
        A.ulast_out[u] = A.ix.unit_last[su + local];
}

// ---- move ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ext_move(const ExtArgs A)
{
    stitch_tile<false>(A.hdr, A.lstart, A.nsel, A.out, [&A](uint32_t k, uint64_t len, uint64_t & kb, uint64_t & ksrc, uint64_t &) {
        kb = len;
        ksrc = reinterpret_cast<uint64_t>(A.ix.in) + A.ix.off[A.src0[k]];
    });
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
uint64_t ext_runs(uint64_t n) { return (n + 63u) / 64u; }

// Workspace: header | three run scans over the selections' 64-runs | c, src0
// (nsel) | nv, nb (nsel, u64) | lstart (nsel + 1, u64), each 256-byte aligned.
struct ExtWs
{
    dev::ExtHdr * hdr;
    RunScanWs<uint64_t, uint64_t> sc, sn, sb;
    uint32_t *c, *src0;
    uint64_t *nv, *nb, *lstart;
    size_t bytes;

    ExtWs(void * ws, uint64_t nsel)
    {
        WsCarver w(ws);
        hdr = w.take<dev::ExtHdr>(1);
        for (RunScanWs<uint64_t, uint64_t> * s : {&sc, &sn, &sb})
            *s = w.scan<uint64_t, uint64_t>(ext_runs(nsel));
        for (uint32_t ** a : {&c, &src0})
            *a = w.take<uint32_t>(nsel);
        for (uint64_t ** a : {&nv, &nb})
            *a = w.take<uint64_t>(nsel);
        lstart = w.take<uint64_t>(nsel + 1u);
        bytes = w.used;
    }
};
} // namespace

size_t lists_extract_workspace(uint64_t nsel)
{
    if (nsel == 0)
        return 0;
    return ExtWs(nullptr, nsel).bytes;
}

// Launches, fixed by the sizes: reset, plan, 3 x 2 run scans, heads,
// [offsets,] [move] -- 11 at the most, 12 with d_err's reset by the entry
// point; nsel == 0: one.
hipError_t launch_lists_extract(const ListsIndex & X, bool d1, const uint32_t * sel, const uint32_t * ufirst, const uint32_t * ucount,
                                uint64_t nsel, uint8_t * out, uint64_t out_cap, uint64_t * off_out, uint64_t units_cap, uint64_t * lptr_out,
                                uint32_t * lunit_out, uint32_t * start0_out, uint32_t * ulast_out, void * ws, unsigned long long * err,
                                hipStream_t s)
{
    hipError_t e;
    if (nsel == 0)
        return launch(dev::k_ext_empty, 1, 64, s, lptr_out, lunit_out, off_out);
    const ExtWs W(ws, nsel);
    const bool ul = d1 && X.unit_last != nullptr && ulast_out != nullptr;
    const dev::ExtArgs A{.ix = X,
                         .sel = sel,
                         .ufirst = ufirst,
                         .ucount = ucount,
                         .nsel = nsel,
                         .out = out,
                         .out_cap = out_cap,
                         .off_out = off_out,
                         .units_cap = units_cap,
                         .lptr_out = lptr_out,
                         .lunit_out = lunit_out,
                         .start0_out = start0_out,
                         .ulast_out = ulast_out,
                         .err = err,
                         .hdr = W.hdr,
                         .c_tot = W.sc.tot,
                         .n_tot = W.sn.tot,
                         .b_tot = W.sb.tot,
                         .c_pre = W.sc.pre,
                         .c_tile = W.sc.tile,
                         .n_pre = W.sn.pre,
                         .n_tile = W.sn.tile,
                         .b_pre = W.sb.pre,
                         .b_tile = W.sb.tile,
                         .c = W.c,
                         .src0 = W.src0,
                         .nv = W.nv,
                         .nb = W.nb,
                         .lstart = W.lstart};
    auto grid = [](uint64_t items, uint64_t per) { return dim3(static_cast<uint32_t>((items + per - 1u) / per)); };
    using u64p = uint64_t *;
    if ((e = launch(dev::k_ext_reset, 1, 64, s, W.hdr)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_ext_plan, flat_grid(nsel, s), 256, s, A)) != hipSuccess)
        return e;
    const uint64_t nr = ext_runs(nsel);
    if ((e = launch_run_scan_u64t(W.sc.tot, nr, W.sc.pre, W.sc.tile, u64p(&W.hdr->nu), s)) != hipSuccess
        || (e = launch_run_scan_u64t(W.sn.tot, nr, W.sn.pre, W.sn.tile, u64p(&W.hdr->nv), s)) != hipSuccess
        || (e = launch_run_scan_u64t(W.sb.tot, nr, W.sb.pre, W.sb.tile, u64p(&W.hdr->nb), s)) != hipSuccess)
        return e;
    if ((e = launch_by(d1, [](auto D1) { return dev::k_ext_heads<D1>; }, flat_grid(nsel + 1u, s), 256, s, A)) != hipSuccess)
        return e;
    if (units_cap != 0u && (e = launch_by(ul, [](auto UL) { return dev::k_ext_offsets<UL>; }, grid(units_cap, 256), 256, s, A)) != hipSuccess)
        return e;
    // a wave per tile of the capacity; no buffer is longer than 2^46 bytes
    const uint64_t span = std::min<uint64_t>(out_cap, 1ull << 46);
    return span != 0u ? launch(dev::k_ext_move, grid(span, 4u * dev::kListsAppendTile), 256, s, A) : hipSuccess;
}

} // namespace tpf
