// p4_lists_intersect.hip -- membership of probe doc ids in resident posting
// lists (p4_lists.h): tpf_lists_intersect takes sorted CSR
// segments of probe values, one target list per segment, and returns the
// values that are also in the target, with their positions.  Every probe value
// is looked up in the skip table (the first unit of its list whose last value
// is >= it); consecutive probe values that land in the same unit form an ITEM,
// and every item's unit is decoded once -- with k_un_dec's and k_un_tails's
// pipelines (p4_lists_units.hip), the start taken from the table -- into the
// wave's LDS, where the item's probe values are searched 64 at a time.  No
// decoded block goes to global memory.  Nothing here is sized by the index:
// grids and the workspace follow nq and probe_values.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_generic.h"
#include "p4_scan.h"
#include "tpf_kernels.h"

namespace tpf::dev
{

constexpr uint32_t kIxNone = 0xFFFFFFFFu; // unit word / list word: the probe value names nothing
constexpr uint32_t kIxMiss = 0xFFFFFFFFu; // result word before the hits pass: not a member
constexpr uint32_t kIxHit = 0x100u;       // result word after the hits pass: bits 0-7 p, bit 8 hit, bits 16-22 hits before it in its run

// Full blocks: items per wave and chunks in flight.  A wave waits for its
// item's probe values once per block (that load sits behind the chunk loads in
// issue order), so short runs over many waves hide the wait better than
// k_un_dec's 16 blocks per wave; DESIGN.md 4.11 has both timings.
constexpr uint32_t kIxRun = 4;
constexpr uint32_t kIxNC = 4;

struct IxHdr
{
    unsigned long long bad; // first refused query k (~0: none)
    uint32_t nitems;        // items: runs of probe values with one list and one source unit
    uint32_t nhits;         // d_out_ptr[nq]
};

// go / no-go of everything after the plan: no query was refused
__device__ __forceinline__ bool ix_go(const IxHdr * h) { return h->bad == ~0ull; }

struct IxArgs
{
    const uint8_t * in;
    uint64_t in_bytes;
    const uint64_t * off;
    uint64_t nunits;
    const uint64_t * ptr;
    const uint32_t * list_unit;
    const uint32_t * start0;
    const uint32_t * unit_last; // the skip table (values, never indices)
    const uint32_t * probe;
    uint64_t pv;                // probe_values
    const IxHdr * hdr;
    const uint32_t * pu;        // per probe value: source unit | kRecTail, or kIxNone
    const uint32_t * pl;        // per probe value: target list, or kIxNone
    const uint32_t * ihead;     // per item: its first probe index ...
    const uint32_t * iend;      // ... and one past its last
    uint32_t * res;             // per probe value: p inside the unit, or kIxMiss
    unsigned long long * err;
};

// Reset of d_err and of the header's verdict in one launch (the other entries
// spend a k_fill_u32 on each; this call is launch-bound for small probes).
__global__ __launch_bounds__(64) void k_ix_reset(unsigned long long * __restrict err, IxHdr * __restrict hdr)
{
    if (threadIdx.x == 0)
    {
        if (err != nullptr)
            *err = ~0ull;
        hdr->bad = ~0ull;
    }
}

// The run scan of p4_scan.h for at most ONE tile of run totals (a probe of up
// to 64 kScanTile values), in one launch where k_run_scan_tiles and
// k_run_scan_tops take two: thread i sums its 16 consecutive entries, the 256
// thread sums are scanned, pre[] = the exclusive prefix, tile[0] = 0, *total =
// the sum.
__global__ __launch_bounds__(256) void k_ix_scan1(const uint32_t * __restrict tot, uint32_t nruns, uint32_t * __restrict pre,
                                                   uint32_t * __restrict tile, uint32_t * __restrict total)
{
    __shared__ uint32_t wsum[4];
    const uint32_t t = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t b = 16u * threadIdx.x;
    uint32_t v[16];
    uint32_t s = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
    {
        v[k] = s;
        s += b + k < nruns ? tot[b + k] : 0u;
    }
    const uint32_t incl = wave_incl_scan(s);
    if (t == 63u)
        wsum[w] = incl;
    __syncthreads();
    uint32_t wb = 0u;
    for (uint32_t k = 0; k < w; ++k)
        wb += wsum[k];
    const uint32_t ex = wb + incl - s;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
        if (b + k < nruns)
            pre[b + k] = ex + v[k];
    if (threadIdx.x == 255u)
    {
        tile[0] = 0u;
        *total = wb + incl;
    }
}

// Plan.  One thread per QUERY: everything the later passes index with is
// checked here (the values are checked, never followed), the first refused
// query by atomicMin.  One thread per PROBE INDEX: its query by a search over
// d_probe_ptr (the last k with ptr[k] <= i, then i < ptr[k+1] held against
// it), that query's own checks again -- the verdict of the other threads is
// not known yet -- and the lower bound of the value over the list's slice of
// the skip table, as k_range_units does it.
__global__ __launch_bounds__(256) void k_ix_plan(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                                  uint64_t nunits, const uint32_t * __restrict unit_last,
                                                  const uint32_t * __restrict probe, uint64_t pv, const uint64_t * __restrict probe_ptr,
                                                  const uint32_t * __restrict qlist, uint64_t nq, IxHdr * __restrict hdr,
                                                  uint32_t * __restrict pu, uint32_t * __restrict pl)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t k = gid; k < nq; k += gsz)
    {
        const uint32_t j = qlist[k];
        const uint64_t pa = probe_ptr[k], pb = probe_ptr[k + 1u];
        bool bad = j >= nlists || pb < pa || pb > pv;
        if (!bad)
        {
            const uint64_t a = ptr[j], b = ptr[j + 1u];
            const uint32_t ua = list_unit[j], ub = list_unit[j + 1u];
            bad = b < a || ub < ua || ub > nunits || ub - ua != list_units(b - a);
        }
        if (bad)
            atomicMin(&hdr->bad, static_cast<unsigned long long>(k));
    }
    for (uint64_t i = gid; i < pv; i += gsz)
    {
        uint32_t unit = kIxNone, list = kIxNone;
        // the last k of [0, nq) with probe_ptr[k] <= i
        uint64_t lo = 0u, hi = nq;
        while (lo < hi)
        {
            const uint64_t m = lo + (hi - lo) / 2u;
            if (probe_ptr[m] <= i)
                lo = m + 1u;
            else
                hi = m;
        }
        if (lo != 0u && i < probe_ptr[lo])
        {
            const uint32_t j = qlist[lo - 1u];
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
        }
        pu[i] = unit;
        pl[i] = list;
    }
}

// A probe index heads an item when it names a unit and the index before it
// names another unit or another list; it ends one when the index after does.
__device__ __forceinline__ bool ix_head(const uint32_t * __restrict pu, const uint32_t * __restrict pl, uint64_t i, uint32_t u, uint32_t l)
{
    return u != kIxNone && (i == 0u || pu[i - 1u] != u || pl[i - 1u] != l);
}

// Heads: every wave owns 64 consecutive probe indices; the head flags' total
// goes to the run scan, and every result word starts as a miss.
__global__ __launch_bounds__(256) void k_ix_heads(uint64_t pv, const IxHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                   const uint32_t * __restrict pl, uint32_t * __restrict tot, uint32_t * __restrict res)
{
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    bool head = false;
    if (i < pv)
    {
        res[i] = kIxMiss;
        if (ix_go(hdr))
            head = ix_head(pu, pl, i, pu[i], pl[i]);
    }
    publish_run_total(tot, run, head ? 1u : 0u, t);
}

// Items: item r is the r-th head in probe order; the probe index that ends its
// run has counted the same r heads, so it knows where to leave the end.
__global__ __launch_bounds__(256) void k_ix_items(uint64_t pv, const IxHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                   const uint32_t * __restrict pl, const uint32_t * __restrict pre,
                                                   const uint32_t * __restrict tile, uint32_t * __restrict ihead,
                                                   uint32_t * __restrict iend)
{
    if (!ix_go(hdr))
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    const bool valid = i < pv;
    const uint32_t u = valid ? pu[i] : kIxNone;
    const uint32_t l = valid ? pl[i] : kIxNone;
    const bool head = valid && ix_head(pu, pl, i, u, l);
    const uint32_t cnt = run_base(pre, tile, run) + wave_incl_scan(head ? 1u : 0u); // heads up to and including i
    if (head)
        ihead[cnt - 1u] = static_cast<uint32_t>(i);
    if (valid && u != kIxNone && (i + 1u == pv || pu[i + 1u] != u || pl[i + 1u] != l))
        iend[cnt - 1u] = static_cast<uint32_t>(i + 1u);
}

// The probe values [h, e) of one item against the 256 values the wave has just
// decoded into `vals` (entries past the unit's count hold 0xFFFFFFFF), 64 at a
// time: a lower bound over the block and an equality check, so a reported hit
// is an equality whatever the block holds.
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
            res[i] = (pos < cnt && vals[pos] == v) ? pos : kIxMiss;
        }
    }
}

// Full blocks: every wave takes runs of RUN consecutive ITEMS through the
// k_dec256v32w pipeline, as k_un_dec does with virtual units.  Lane t
// gathers item first + t: its head's unit word and list, the offsets of the
// source unit and its start -- start0[list] for the list's first unit, else
// unit_last[su - 1] (a unit of the same list: in range whatever the table
// holds).  The plan checked list < nlists and list_unit[list] <= su <
// list_unit[list + 1] <= nunits for every value it gave a unit.  Where
// k_un_dec stores the block, this keeps it in 1 KB of LDS per wave.
template <uint32_t RUN, uint32_t NC, int MINW>
__global__ __launch_bounds__(256, MINW) void k_ix_dec(const IxArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    __shared__ uint32_t vals[4][256];
    // per item of the run, read back wave-uniformly: the source unit (for the
    // error report only, as in k_un_dec), the probe range and the start -- held
    // in registers across the pipeline they cost spilled VGPRs at 7 waves
    __shared__ uint32_t srcu[4][RUN], itemh[4][RUN], iteme[4][RUN], starts[4][RUN];
    if (!ix_go(A.hdr))
        return;
    constexpr uint32_t kRun = RUN;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    uint32_t * slot = slots[wv];
    uint32_t * scr = scratch[wv];
    const uint64_t in_base = reinterpret_cast<uint64_t>(A.in);
    const uint64_t in_end = in_base + A.in_bytes;
    const uint64_t nit = A.hdr->nitems;
    // the host knows only the cap of one item per probe value: the grid covers
    // the device and every wave strides over the runs of the real item count
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 4u * kRun;
    for (uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kRun; first < nit; first += stride)
    {
        const uint32_t n = static_cast<uint32_t>(min_u64(kRun, nit - first));
        const bool valid = t < n;
        const uint32_t ih = valid ? A.ihead[first + t] : 0u;
        const uint32_t ie = valid ? A.iend[first + t] : 0u;
        const uint32_t w = valid ? A.pu[ih] : kIxNone;
        const bool full = valid && (w & kRecTail) == 0u;
        const uint64_t fullmask = __ballot(full);
        if (fullmask == 0ull)
            continue; // a run of tails only
        const uint32_t su = w & kRecList;
        const uint32_t lj = full ? A.pl[ih] : 0u;
        const uint64_t o = full ? A.off[su] : 0ull;
        const uint64_t e = full ? A.off[su + 1u] : 0ull;
        RunPlaneT<kSlotBytes, true> P;
        P.init(in_base, in_end, o, e, full);
        {
            uint32_t startv = 0u;
            if (full)
                startv = su == A.list_unit[lj] ? (A.start0 != nullptr ? A.start0[lj] : 0u) : A.unit_last[su - 1u];
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
#pragma unroll
        for (uint32_t q = 0; q + 1 < NC; ++q)
            P.template issue<0>(C[q], q, t);

        uint64_t badmask = 0u;
        auto consume = [&](const Chunk & c, uint32_t jj) {
            if (((fullmask >> jj) & 1ull) == 0ull)
                return;
            const uint32_t ctl = P.stage(c, jj, slot, t);
            u32x4 x;
            const uint32_t used = decode_block256v32(slot, (ctl >> kCtlShift) & 15u, P.head(c, ctl, slot), scr, t, x);
            apply_delta1_256(x, uni(starts[wv][jj]));
            reinterpret_cast<u32x4 *>(vals[wv])[t] = x;
            wave_lds_sync();
            ix_test(vals[wv], 256u, A.probe, A.res, uni(itemh[wv][jj]), uni(iteme[wv][jj]), t);
            wave_lds_sync();
            if (used != rl(P.len, jj))
                badmask |= 1ull << jj;
        };

        bool more = true;
        for (uint32_t j = 0; more; j += NC)
        {
#pragma unroll
            for (uint32_t q = 0; q < NC; ++q)
            {
                if (more)
                {
                    P.template issue<0>(C[(q + NC - 1) % NC], j + q + NC - 1, t);
                    consume(C[q], j + q);
                    more = j + q + 1 < n;
                }
            }
        }
        if (A.err != nullptr && badmask != 0u)
        {
            // in stream numbering; the source units of a run need not ascend
            const uint32_t m = wave_min((t < kRun && ((badmask >> t) & 1ull) != 0ull) ? srcu[wv][t] : 0xFFFFFFFFu);
            if (t == 0)
                atomicMin(A.err, static_cast<unsigned long long>(m));
        }
        wave_lds_sync(); // the item words are rewritten by the next run
    }
}

// Tails: every wave owns kRunDefault consecutive ITEMS with the generic
// decoder's pipeline, as k_un_tails does for selections; lane t holds item
// first + t when its unit is its list's p4Enc32 tail, n % 256 values.
template <uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_ix_tails(const IxArgs A)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    __shared__ uint32_t vals[4][256];
    if (!ix_go(A.hdr))
        return;
    constexpr uint32_t kRun = kRunDefault;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    uint32_t * slot = slots[wv];
    const uint64_t in_base = reinterpret_cast<uint64_t>(A.in);
    const uint64_t in_end = in_base + A.in_bytes;
    const uint64_t nit = A.hdr->nitems;
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kRun;
    if (first >= nit)
        return;
    const uint32_t n = static_cast<uint32_t>(min_u64(kRun, nit - first));
    const bool valid = t < n;
    const uint32_t ih = valid ? A.ihead[first + t] : 0u;
    const uint32_t ie = valid ? A.iend[first + t] : 0u;
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
    P.init(in_base, in_end, o, e, has);
    uint32_t startv = 0u;
    if (has)
        startv = su == A.list_unit[lj] ? (A.start0 != nullptr ? A.start0[lj] : 0u) : A.unit_last[su - 1u];
    uint64_t badmask = 0u;
    auto consume = [&](const Chunk & c, uint32_t jj) {
        if (((hasmask >> jj) & 1ull) == 0ull)
            return;
        const uint32_t ctl = P.stage(c, jj, slot, t);
        const uint32_t cj = rl(cnt, jj);
        uint32_t x[4], cm;
        const uint32_t used = decode_block_g<Fmt::H32>(slot, (ctl >> kCtlShift) & 15u, cj, scratch[wv], t, x, &cm);
        (void)delta1_g<uint32_t>(x, cj, rl(startv, jj), t);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            vals[wv][t + 64u * q] = t + 64u * q < cj ? x[q] : 0xFFFFFFFFu;
        wave_lds_sync();
        ix_test(vals[wv], cj, A.probe, A.res, rl(ih, jj), rl(ie, jj), t);
        wave_lds_sync();
        if (used != rl(P.len, jj))
            badmask |= 1ull << jj;
    };
    Chunk C[NC];
#pragma unroll
    for (uint32_t q = 0; q + 1 < NC; ++q)
        P.template issue<0>(C[q], q, t);
    bool more = true;
    for (uint32_t jb = 0; more; jb += NC)
    {
#pragma unroll
        for (uint32_t q = 0; q < NC; ++q)
        {
            if (more)
            {
                P.template issue<0>(C[(q + NC - 1) % NC], jb + q + NC - 1, t);
                consume(C[q], jb + q);
                more = jb + q + 1 < n;
            }
        }
    }
    if (A.err != nullptr && badmask != 0u)
    {
        const uint32_t m = wave_min(((badmask >> t) & 1ull) != 0ull ? su : 0xFFFFFFFFu);
        if (t == 0)
            atomicMin(A.err, static_cast<unsigned long long>(m));
    }
}

// Hits: every wave owns 64 consecutive probe indices again; the hit flags'
// total goes to the second run scan, and the result word is rewritten as
// p | kIxHit | (hits before it in its run) << 16, or 0 for a miss with the
// same count, so the compaction reads one word per index.
__global__ __launch_bounds__(256) void k_ix_hits(uint64_t pv, const IxHdr * __restrict hdr, uint32_t * __restrict res,
                                                  uint32_t * __restrict tot)
{
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= pv)
        return;
    const uint32_t r = (i < pv && ix_go(hdr)) ? res[i] : kIxMiss;
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
                                                const IxHdr * __restrict hdr, const uint32_t * __restrict pu,
                                                const uint32_t * __restrict pl, const uint32_t * __restrict res,
                                                const uint32_t * __restrict pre, const uint32_t * __restrict tile,
                                                uint32_t * __restrict out, uint64_t out_values, uint64_t * __restrict out_ptr,
                                                uint32_t * __restrict out_pidx, uint32_t * __restrict out_tpos,
                                                unsigned long long * __restrict err)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    if (!ix_go(hdr))
    {
        if (gid == 0 && err != nullptr)
            *err = nunits + hdr->bad;
        return;
    }
    const uint64_t total = hdr->nhits;
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
size_t al256(size_t x) { return (x + 255u) & ~size_t(255); }

// Workspace of the intersection: header | two run scans over the 64-value
// runs of the probe (item heads, hits) | per probe value its unit word, its
// list and its result | per item its first probe index and its end, each
// 256-byte aligned.  There is at most one item per probe value.
struct IxWs
{
    dev::IxHdr * hdr;
    RunScanWs<uint32_t> scani, scanh;
    uint32_t *pu, *pl, *res, *ihead, *iend;
    size_t bytes;

    IxWs(void * ws, uint64_t pv)
    {
        auto * p = static_cast<uint8_t *>(ws);
        const uint64_t nruns = (pv + 63u) / 64u;
        size_t x = 0;
        hdr = reinterpret_cast<dev::IxHdr *>(p + x);
        x += 256u;
        scani = RunScanWs<uint32_t>::carve(p + x, nruns);
        x += al256(RunScanWs<uint32_t>::bytes(nruns));
        scanh = RunScanWs<uint32_t>::carve(p + x, nruns);
        x += al256(RunScanWs<uint32_t>::bytes(nruns));
        uint32_t ** arr[5] = {&pu, &pl, &res, &ihead, &iend};
        for (uint32_t ** a : arr)
        {
            *a = reinterpret_cast<uint32_t *>(p + x);
            x += al256(4u * pv);
        }
        bytes = x;
    }
};

uint32_t flat_grid(uint64_t items, hipStream_t s)
{
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((items + 255u) / 256u, grid_cap(s, 8))));
}
} // namespace

// the run scan over the probe's 64-value runs: one launch while they fit one tile, p4_scan.hip's two beyond
hipError_t ix_scan(const uint32_t * tot, uint64_t nruns, uint32_t * pre, uint32_t * tile, uint32_t * total, hipStream_t s)
{
    if (nruns > dev::kScanTile)
        return launch_run_scan_u32(tot, nruns, pre, tile, total, s);
    hipLaunchKernelGGL(dev::k_ix_scan1, dim3(1), dim3(256), 0, s, tot, static_cast<uint32_t>(nruns), pre, tile, total);
    return hipGetLastError();
}

// nq sizes no array: the queries are read where they lie
size_t lists_intersect_workspace(uint64_t /*nq*/, uint64_t probe_values) { return IxWs(nullptr, probe_values).bytes; }

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
    // one wave per 64 probe indices, one wave per kRunDefault items: at least one workgroup for an empty probe
    const uint32_t rgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (nruns + 3u) / 4u));
    const uint32_t igrid = static_cast<uint32_t>(std::max<uint64_t>(1, (pv + 4u * dev::kRunDefault - 1u) / (4u * dev::kRunDefault)));
    hipLaunchKernelGGL(dev::k_ix_reset, dim3(1), dim3(64), 0, s, err, W.hdr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ix_plan, dim3(flat_grid(std::max(nq, pv), s)), dim3(256), 0, s, ptr, list_unit, nlists, nunits, unit_last,
                       probe, pv, probe_ptr, qlist, nq, W.hdr, W.pu, W.pl);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ix_heads, dim3(rgrid), dim3(256), 0, s, pv, W.hdr, W.pu, W.pl, W.scani.tot, W.res);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    if ((e = ix_scan(W.scani.tot, nruns, W.scani.pre, W.scani.tile, &W.hdr->nitems, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ix_items, dim3(rgrid), dim3(256), 0, s, pv, W.hdr, W.pu, W.pl, W.scani.pre, W.scani.tile, W.ihead, W.iend);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    const dev::IxArgs A{in, in_bytes, off, nunits, ptr, list_unit, start0, unit_last, probe, pv, W.hdr, W.pu, W.pl, W.ihead, W.iend,
                        W.res, err};
    // the cap is one item per probe value, a dense probe holds hundreds of times fewer: at most kListsMinW
    // workgroups per CU, whose waves stride over the real items (k_ix_tails: a wave per 16 items of the cap)
    const uint32_t dgrid = static_cast<uint32_t>(std::max<uint64_t>(
        1, std::min<uint64_t>((pv + 4u * dev::kIxRun - 1u) / (4u * dev::kIxRun), grid_cap(s, dev::kListsMinW))));
    hipLaunchKernelGGL((dev::k_ix_dec<dev::kIxRun, dev::kIxNC, dev::kListsMinW>), dim3(dgrid), dim3(256), 0, s, A);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    hipLaunchKernelGGL((dev::k_ix_tails<dev::kTailsNC>), dim3(igrid), dim3(256), 0, s, A);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ix_hits, dim3(rgrid), dim3(256), 0, s, pv, W.hdr, W.res, W.scanh.tot);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    if ((e = ix_scan(W.scanh.tot, nruns, W.scanh.pre, W.scanh.tile, &W.hdr->nhits, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_ix_out, dim3(flat_grid(std::max(nq + 1u, pv), s)), dim3(256), 0, s, list_unit, nunits, probe, pv, probe_ptr,
                       nq, W.hdr, W.pu, W.pl, W.res, W.scanh.pre, W.scanh.tile, out, out_values, out_ptr, out_pidx, out_tpos, err);
    return hipGetLastError();
}

} // namespace tpf
