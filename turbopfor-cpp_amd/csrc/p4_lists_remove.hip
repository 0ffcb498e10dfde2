// p4_lists_remove.hip -- tpf_lists_remove: the postings at given list positions
// of a resident index deleted in one submission with no host round trip
// (include/turbopfor_gpu.h).  A 256v32 block's bytes depend on
// its 256 values and the value before it only, so every unit of a list before
// the one that holds its first removed position (u0) is moved as bytes, and so
// is every list that loses nothing; the suffix from u0 on is decoded, compacted
// and encoded again.  The append's segment shape (p4_lists_append.hip): a list
// of the result is a run of kept bytes of the old stream and a run of new bytes
// of a staged encode.
//   reset  : the header; the lists' query word (qof) to "none"
//   plan q : a thread per query: the checks, u0, the unit range (j, u0,
//            units(j) - u0) the units decode takes, the compacted count c and
//            its units m, qof[list] = k; run totals of c and m per 64 queries
//   plan p : a thread per position: below |L_j| and above the one before it
//   plan l : a thread per list: the structure checks, the units it keeps, its
//            kept bytes and new unit count; run totals per 64 lists
//   scans  : run scans of the five (p4_scan.h)
//   decode : launch_lists_units (p4_lists_units.hip) over the ranges into the
//            raw staged values; its d_out_ptr is their CSR pointer (dptr)
//   heads q: a thread per query: the compacted lists' pointers (sptr), unit
//            bases, unit records and delta-1 starts -- the encoder's plan
//   heads l: the verdict, then per list d_list_ptr_out, d_list_unit_out, the
//            prefix of the kept bytes and the list's first staged unit
//   compact: a thread per raw staged value: dropped if its position is in the
//            segment, else moved down by the removed positions below it
//   encode : the many-lists encoder's passes (p4_lists_enc.hip) over the
//            compacted lists into a byte buffer of the workspace
//   segs   : a thread per list: where its bytes start in d_out; the capacity
//   offsets: a thread per output unit: d_off_out and d_unit_last_out
//   stitch : stitch_tile (p4_lists_stitch.h)
// Every kernel after the heads reads the go flag of the header first.
#include "p4_lists.h"

#include "p4_lists_dev.h"
#include "p4_lists_host.h"
#include "p4_lists_stitch.h"
#include "turbopfor_gpu.h"

#include <algorithm>

namespace tpf::dev
{

struct RemHdr
{
    unsigned long long bad;  // first list that fails a structure check (~0: none)
    unsigned long long qbad; // first refused query (~0: none)
    unsigned long long uerr; // what the units decode reports: the lowest bad decoded unit, or a code of its own at or past nunits
    unsigned long long c, m; // totals of the query scans: compacted values, their units
    unsigned long long nu, tq, kb; // totals of the list scans: units, targeted lists, kept bytes
    unsigned long long nunits_out;
    uint32_t go;  // the heads pass: structure, queries, staging and units_cap are sound
    uint32_t fit; // the segs pass: the stream fits out_cap
};

struct RemArgs
{
    ListsIndex ix; // (the result has ix.nlists lists too)
    const uint32_t * pos;
    uint64_t pos_values;
    const uint64_t * pptr;
    const uint32_t * qlist;
    uint64_t nq;
    uint64_t stage_values;
    uint8_t * out;
    uint64_t out_cap;
    uint64_t * off_out;
    uint64_t units_cap;
    uint64_t * lptr_out;
    uint32_t * lunit_out;
    uint32_t * ulast_out;
    unsigned long long * err;
    // workspace
    RemHdr * hdr;
    uint32_t *c_tot, *m_tot, *nu_tot, *tq_tot; // run totals
    uint64_t * kb_tot;
    const uint64_t *c_pre, *c_tile, *m_pre, *m_tile, *nu_pre, *nu_tile, *tq_pre, *tq_tile, *kb_pre, *kb_tile;
    uint32_t *qof, *keep;                // per list: its query (kItemNone: none), the units it keeps
    uint32_t * subase;                   // n + 1: first staged unit of every list
    uint64_t *kbpre, *lstart;            // n + 1: kept bytes of the lists before, first output byte
    uint32_t *sel, *ufirst, *ucount;     // per query: the unit range that is decoded
    uint32_t *cq, *mq, *sst;             // per query: compacted values, their units, their delta-1 start
    uint64_t * sptr;                     // nq + 1: the compacted lists
    const uint64_t * dptr;               // nq + 1: the raw staged lists (the units decode's d_out_ptr)
    const uint32_t * raw;                // raw staged values
    uint32_t * stage;                    // compacted values
    uint64_t * noff;                     // offsets of the compacted lists' units in sbytes
    uint8_t * sbytes;                    // their bytes
    ListsHdr * ehdr;                     // the encoder's view (p4_lists.h)
    uint32_t * qsub;                     // nq + 1: first staged unit of every query
    uint32_t * rec;                      // records of the staged units
    uint64_t su_cap;
};

__device__ __forceinline__ void rem_err(unsigned long long * err, unsigned long long v)
{
    if (err != nullptr)
        atomicMin(err, v);
}

// What the heads passes decide from the header, the staged total and the sizes.
enum : uint32_t
{
    kRemGo = 0,
    kRemRefused,  // a list or a query: nothing is written
    kRemStage,    // the staged values exceed stage_values: the directories only
    kRemUnits     // nunits_out > units_cap: the directories only
};

__device__ __forceinline__ uint32_t rem_verdict(const RemArgs & A, const RemHdr & h)
{
    if (h.bad != ~0ull || h.qbad != ~0ull)
        return kRemRefused;
    if (A.nq != 0u && A.dptr[A.nq] > A.stage_values)
        return kRemStage;
    return h.nu > A.units_cap ? kRemUnits : kRemGo;
}

__global__ __launch_bounds__(256) void k_rem_reset(const RemArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    if (gid == 0)
    {
        *A.hdr = RemHdr{~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0u, 0u};
        *A.ehdr = ListsHdr{0ull, 0ull}; // no go until the heads pass says so
    }
    for (uint64_t j = gid; j < A.ix.nlists; j += gsz)
        A.qof[j] = kItemNone;
}

// nlists == 0: the empty result
__global__ void k_rem_empty(uint64_t * lptr_out, uint32_t * lunit_out, uint64_t * off_out)
{
    if (threadIdx.x == 0)
    {
        lptr_out[0] = 0ull;
        lunit_out[0] = 0u;
        off_out[0] = 0ull;
    }
}

// ---- plan over the queries ----------------------------------------------------
__global__ __launch_bounds__(256) void k_rem_plan_q(const RemArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t k = gid;
    uint32_t c32 = 0u, m = 0u;
    if (k < A.nq)
    {
        const uint32_t j = A.qlist[k];
        const uint64_t pa = A.pptr[k], pb = A.pptr[k + 1u];
        bool bad = j >= A.ix.nlists || (k != 0u && j <= A.qlist[k - 1u]) || pb < pa || pb > A.pos_values;
        uint32_t sj = 0u, uf = 0u, uc = 0u;
        if (!bad)
        {
            uint64_t n;
            uint32_t ua, ub;
            // a list that fails here fails the list plan, whose code is the lower one
            const bool dir = list_dir_ok(A.ix.ptr, A.ix.list_unit, A.ix.nlists, A.ix.nunits, j, &n, &ua, &ub);
            if (dir && pb != pa)
            {
                const uint64_t p0 = A.pos[pa];
                bad = p0 >= n;
                if (!bad)
                {
                    uf = static_cast<uint32_t>(p0 >> 8);
                    uc = (ub - ua) - uf;
                    sj = j;
                    const uint64_t s = n - 256ull * uf, nrem = pb - pa;
                    const uint64_t c = s >= nrem ? s - nrem : 0ull; // nrem > s: a position is refused
                    c32 = static_cast<uint32_t>(c);                 // exact whenever the staged values fit stage_values
                    m = list_units(c);
                }
            }
            if (!bad)
                A.qof[j] = static_cast<uint32_t>(k);
        }
        if (bad)
            atomicMin(&A.hdr->qbad, static_cast<unsigned long long>(k));
        A.sel[k] = sj;
        A.ufirst[k] = uf;
        A.ucount[k] = uc;
        A.cq[k] = c32;
        A.mq[k] = m;
    }
    // gid < 64 * runs for every thread of a block up to the run's end
    const uint64_t run = gid / 64u;
    if (run * 64u < A.nq)
    {
        publish_run_total(A.c_tot, run, c32, t);
        publish_run_total(A.m_tot, run, m, t);
    }
    if (gid < A.su_cap)
        A.rec[gid] = 0u;
}

// ---- plan over the positions --------------------------------------------------
__global__ __launch_bounds__(256) void k_rem_plan_p(const RemArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t p = A.pptr[0] + gid;
    if (gid >= A.pos_values || p >= A.pos_values || p >= A.pptr[A.nq])
        return;
    const uint32_t k = segment_of(A.pptr, A.nq, p);
    if (k == kItemNone)
        return; // pointers that descend: the query plan refuses them
    const uint32_t j = A.qlist[k];
    if (j >= A.ix.nlists)
        return;
    const uint64_t n = A.ix.ptr[j + 1u] - A.ix.ptr[j];
    const uint32_t v = A.pos[p];
    if (v >= n || (p > A.pptr[k] && A.pos[p - 1u] >= v))
        atomicMin(&A.hdr->qbad, static_cast<unsigned long long>(k));
}

// ---- plan over the lists ------------------------------------------------------
__global__ __launch_bounds__(256) void k_rem_plan_l(const RemArgs A)
{
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    uint32_t keep = 0u, nu = 0u, tq = 0u;
    uint64_t kb = 0ull;
    if (j < A.ix.nlists)
    {
        const uint64_t p0 = A.ix.ptr[j], p1 = A.ix.ptr[j + 1u];
        const uint64_t oldn = p1 - p0;
        const uint64_t cnt = (oldn >> 8) + ((oldn & 255u) != 0u ? 1u : 0u);
        const uint64_t lu0 = A.ix.list_unit[j], lu1 = A.ix.list_unit[j + 1u];
        bool bad = p1 < p0 || lu1 - lu0 != cnt || lu1 > A.ix.nunits;
        if (!bad)
        {
            keep = static_cast<uint32_t>(cnt);
            uint32_t m = 0u;
            const uint32_t k = A.qof[j];
            if (k != kItemNone)
            {
                tq = 1u;
                if (A.ucount[k] != 0u) // a segment that is not empty: units [u0, cnt) go through the staging
                {
                    keep = A.ufirst[k];
                    m = A.mq[k];
                }
            }
            if (cnt != 0u)
            {
                // the ends of the copied range
                const uint64_t o0 = A.ix.off[lu0], o1 = A.ix.off[lu0 + keep];
                bad = o0 > o1 || o1 > A.ix.in_bytes;
                kb = bad ? 0ull : o1 - o0;
            }
            nu = keep + m;
        }
        if (bad)
            atomicMin(&A.hdr->bad, static_cast<unsigned long long>(j));
        A.keep[j] = keep;
    }
    const uint64_t run = j / 64u;
    if (run * 64u < A.ix.nlists)
    {
        publish_run_total(A.nu_tot, run, nu, t);
        publish_run_total(A.tq_tot, run, tq, t);
        const uint64_t s = readlane_u64(wave_incl_scan64(kb), 63);
        if (t == 0)
            A.kb_tot[run] = s;
    }
}

// ---- heads over the queries: the encoder's plan ------------------------------------
template <bool D1>
__global__ __launch_bounds__(256) void k_rem_heads_q(const RemArgs A)
{
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const RemHdr h = *A.hdr;
    if (rem_verdict(A, h) != kRemGo)
        return;
    const bool in = k < A.nq;
    const uint32_t c = in ? A.cq[k] : 0u, m = in ? A.mq[k] : 0u;
    // exclusive prefixes: the run's base plus the wave's scan (every lane of the wave takes part)
    uint64_t C = wave_incl_scan(c) - c, M = wave_incl_scan(m) - m;
    if (k > A.nq)
        return;
    if (in)
    {
        const uint64_t run = k / 64u;
        C += run_base(A.c_pre, A.c_tile, run);
        M += run_base(A.m_pre, A.m_tile, run);
    }
    else
    {
        C = h.c, M = h.m;
    }
    A.sptr[k] = C;
    A.qsub[k] = static_cast<uint32_t>(M);
    if (in)
    {
        const bool tail = (c & 255u) != 0u;
        if (m == 1u)
            A.rec[M] = static_cast<uint32_t>(k + 1u) | (tail ? kRecTail : 0u);
        else if (m != 0u)
        {
            A.rec[M] = static_cast<uint32_t>(k + 1u);
            if (tail)
                A.rec[M + m - 1u] = kRecTail;
        }
        if constexpr (D1)
        {
            // the staged values continue the list: from the last kept unit, or from start0
            const uint32_t j = A.sel[k], u0 = A.ufirst[k];
            A.sst[k] = u0 == 0u ? (A.ix.start0 != nullptr ? A.ix.start0[j] : 0u) : A.ix.unit_last[A.ix.list_unit[j] + u0 - 1u];
        }
    }
    else
    {
        *A.ehdr = ListsHdr{~0ull, h.m};
        if (h.m == 0u)
            A.noff[0] = 0ull;
    }
}

// ---- heads over the lists: the verdict and the directories ----------------------------
__global__ __launch_bounds__(256) void k_rem_heads_l(const RemArgs A)
{
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const RemHdr h = *A.hdr;
    const uint64_t ebase = A.ix.nunits;
    const uint32_t verdict = rem_verdict(A, h);
    if (verdict == kRemRefused)
    {
        if (j == 0)
            rem_err(A.err, h.bad != ~0ull ? ebase + h.bad : ebase + A.ix.nlists + h.qbad);
        return;
    }
    const bool in = j < A.ix.nlists;
    const uint32_t keep = in ? A.keep[j] : 0u;
    const uint32_t k = in ? A.qof[j] : kItemNone;
    const uint32_t tq = k != kItemNone ? 1u : 0u;
    const uint32_t m = tq != 0u && A.ucount[k] != 0u ? A.mq[k] : 0u;
    const uint32_t nu = keep + m;
    uint64_t kb = 0ull;
    if (in && keep != 0u)
    {
        const uint32_t lu = A.ix.list_unit[j];
        kb = A.ix.off[lu + keep] - A.ix.off[lu];
    }
    uint64_t NU = wave_incl_scan(nu) - nu, TQ = wave_incl_scan(tq) - tq, KB = wave_incl_scan64(kb) - kb;
    if (j > A.ix.nlists)
        return;
    if (in)
    {
        const uint64_t run = j / 64u;
        NU += run_base(A.nu_pre, A.nu_tile, run);
        TQ += run_base(A.tq_pre, A.tq_tile, run);
        KB += run_base(A.kb_pre, A.kb_tile, run);
    }
    else
    {
        NU = h.nu, TQ = h.tq, KB = h.kb;
    }
    // TQ queries name lists before j (every query names a list of its own): their positions are gone
    const uint64_t nr = A.nq != 0u ? A.pptr[TQ] - A.pptr[0] : 0ull;
    A.lptr_out[j] = (A.ix.ptr[j] - A.ix.ptr[0]) - nr;
    A.lunit_out[j] = static_cast<uint32_t>(NU);
    if (verdict != kRemGo)
    {
        if (j == A.ix.nlists)
            rem_err(A.err, ebase + A.ix.nlists + A.nq + (verdict == kRemStage ? 0u : 1u));
        return;
    }
    A.kbpre[j] = KB;
    A.subase[j] = A.nq != 0u ? A.qsub[TQ] : 0u;
    if (!in)
    {
        if (A.nq == 0u)
            A.noff[0] = 0ull;
        A.hdr->nunits_out = h.nu;
        A.hdr->go = 1u;
    }
}

// ---- compaction -----------------------------------------------------------------
// The number of entries of tab[0 .. n) below x (tab ascends), a wave's search:
// 64 pivots per step.  Invariant: tab[i] < x for i < lo, tab[i] >= x for i >= hi.
__device__ __forceinline__ uint32_t wave_lower_bound(const uint32_t * __restrict tab, uint32_t n, uint64_t x, uint32_t t)
{
    uint32_t lo = 0u, hi = n;
    while (hi > lo)
    {
        const uint32_t step = (hi - lo + 63u) / 64u;
        const uint64_t p = static_cast<uint64_t>(lo) + static_cast<uint64_t>(t + 1u) * step - 1u;
        const bool lt = p < hi && tab[p] < x;
        const uint32_t c = static_cast<uint32_t>(__builtin_popcountll(__ballot(lt))); // tab ascends: the first c pivots
        const uint64_t nlo = static_cast<uint64_t>(lo) + static_cast<uint64_t>(c) * step;
        hi = uni(static_cast<uint32_t>(min_u64(hi, nlo + step - 1u)));
        lo = uni(static_cast<uint32_t>(min_u64(nlo, hi)));
    }
    return lo;
}

// The same for one lane, from r0 known to be at or below the answer: a galloping
// search, a probe or two when the answer lies next to r0.
__device__ __forceinline__ uint32_t gallop_lower_bound(const uint32_t * __restrict tab, uint32_t n, uint32_t r0, uint64_t x)
{
    uint32_t lo = r0, step = 1u;
    while (lo + step <= n && tab[lo + step - 1u] < x)
    {
        lo += step;
        step *= 2u;
    }
    uint32_t hi = umin32(lo + step - 1u, n); // tab[hi] >= x, or hi == n
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tab[mid] < x)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// A thread per raw staged value i: its query k (the wave's first value by the
// cooperative search over dptr, the others from it), its list position p = 256
// u0 + (i - dptr[k]) and r = the positions of the segment below p.  The value
// is dropped when the segment holds p, else it moves down by r.  A wave's 64
// consecutive positions share a narrow window of the segment: the lanes of the
// first value's query start from its r, found by the wave; a lane of a later
// query lies among the first 63 staged values of its list and starts from 0.
__global__ __launch_bounds__(256) void k_rem_compact(const RemArgs A)
{
    if (A.hdr->go == 0u)
        return;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t nq = static_cast<uint32_t>(A.nq);
    const uint64_t total = A.dptr[nq];
    const uint64_t iw = i - t; // the wave's first value
    if (iw >= total)
        return;
    const uint32_t k0 = find_list(A.dptr, nq, iw, t);
    const uint64_t pa0 = A.pptr[k0];
    const uint32_t len0 = static_cast<uint32_t>(A.pptr[k0 + 1u] - pa0);
    const uint64_t pw = 256ull * A.ufirst[k0] + (iw - A.dptr[k0]);
    const uint32_t r0 = wave_lower_bound(A.pos + pa0, len0, pw, t);
    if (i >= total)
        return;
    const uint32_t k = gallop(A.dptr, nq, k0, i);
    const uint64_t local = i - A.dptr[k];
    const uint64_t p = 256ull * A.ufirst[k] + local;
    const uint64_t pa = A.pptr[k];
    const uint32_t len = static_cast<uint32_t>(A.pptr[k + 1u] - pa);
    const uint32_t * seg = A.pos + pa;
    const uint32_t r = gallop_lower_bound(seg, len, k == k0 ? r0 : 0u, p);
    if (r < len && seg[r] == p)
        return;
    A.stage[A.sptr[k] + local - r] = A.raw[i];
}

// ---- segs: where every list's bytes start, and the capacity -----------------------
__global__ __launch_bounds__(256) void k_rem_segs(const RemArgs A)
{
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    // what the units decode found: a unit of the stream (its own codes lie at or past nunits)
    if (j == 0 && A.hdr->uerr < A.ix.nunits)
        rem_err(A.err, A.hdr->uerr);
    if (A.hdr->go == 0u)
        return;
    if (j > A.ix.nlists)
        return;
    const uint64_t s = A.kbpre[j] + A.noff[A.subase[j]];
    A.lstart[j] = s;
    if (j == A.ix.nlists)
    {
        A.off_out[A.hdr->nunits_out] = s;
        if (s > A.out_cap)
            rem_err(A.err, A.ix.nunits + A.ix.nlists + A.nq + 2u);
        else
            A.hdr->fit = 1u;
    }
}

// ---- offsets ------------------------------------------------------------------
template <bool D1>
__global__ __launch_bounds__(256) void k_rem_offsets(const RemArgs A)
{
    if (A.hdr->go == 0u)
        return;
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t nuo = A.hdr->nunits_out;
    if (u - t >= nuo)
        return;
    // the last j with lunit_out[j] <= u (lunit_out[0] = 0 <= u < lunit_out[n])
    const uint32_t j0 = find_list(A.lunit_out, static_cast<uint32_t>(A.ix.nlists), static_cast<uint32_t>(u - t), t); // u - t < nuo < 2^31
    if (u >= nuo)
        return;
    const uint64_t j = gallop(A.lunit_out, static_cast<uint32_t>(A.ix.nlists), j0, u);
    const uint32_t local = static_cast<uint32_t>(u) - A.lunit_out[j];
    const uint32_t lu = A.ix.list_unit[j];
    const uint32_t keep = A.keep[j];
    if (local < keep)
    {
        A.off_out[u] = A.lstart[j] + (A.ix.off[lu + local] - A.ix.off[lu]);
        if constexpr (D1)
            A.ulast_out[u] = A.ix.unit_last[lu + local];
    }
    else
    {
        const uint32_t v = local - keep; // the list's staged unit
        A.off_out[u] = A.kbpre[j + 1u] + A.noff[A.subase[j] + v];
        if constexpr (D1)
        {
            const uint32_t k = A.qof[j];
            A.ulast_out[u] = A.stage[min_u64(A.sptr[k] + 256ull * (v + 1u), A.sptr[k + 1u]) - 1u];
        }
    }
}

// ---- stitch -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rem_stitch(const RemArgs A) { stitch_tile(A, A.ix.nlists); }

} // namespace tpf::dev

namespace tpf
{

namespace
{
uint64_t rem_runs(uint64_t n) { return (n + 63u) / 64u; }

// Capacities of the staging, from the sizes alone: nq lists are staged, a list
// of c compacted values as at most c / 256 + 1 units.
struct RemCaps
{
    uint64_t units, bytes;
    RemCaps(uint64_t nq, uint64_t stage_values)
    {
        units = stage_values / 256u + nq + 1u; // never 0
        bytes = tpf_p4nenc256v32_lists_bound(stage_values, nq);
    }
};

// Workspace: header | three run scans over the lists' 64-runs, two over the
// queries' | qof, keep (n), subase (n + 1), kbpre, lstart (n + 1, u64) | sel,
// ufirst, ucount, cq, mq, sst (nq), sptr, dptr (nq + 1, u64) | raw and
// compacted staged values | staged units' offsets | staged bytes (+ 16: the
// stitch reads whole dwords) | the encoder's workspace | the units decode's,
// each 256-byte aligned.
struct RemWs
{
    dev::RemHdr * hdr;
    RunScanWs<uint64_t> snu, stq, sc, sm;
    RunScanWs<uint64_t, uint64_t> skb;
    uint32_t *qof, *keep, *subase, *sel, *ufirst, *ucount, *cq, *mq, *sst, *raw, *stage;
    uint64_t *kbpre, *lstart, *sptr, *dptr, *noff;
    uint8_t * sbytes;
    void *enc, *units;
    size_t bytes;

    RemWs(void * ws, uint64_t n, uint64_t nq, uint64_t stage_values, const RemCaps & C)
    {
        WsCarver c(ws);
        hdr = c.take<dev::RemHdr>(1);
        for (RunScanWs<uint64_t> * s : {&snu, &stq})
            *s = c.scan<uint64_t>(rem_runs(n));
        skb = c.scan<uint64_t, uint64_t>(rem_runs(n));
        for (RunScanWs<uint64_t> * s : {&sc, &sm})
            *s = c.scan<uint64_t>(rem_runs(nq));
        for (uint32_t ** a : {&qof, &keep})
            *a = c.take<uint32_t>(n);
        subase = c.take<uint32_t>(n + 1u);
        for (uint64_t ** a : {&kbpre, &lstart})
            *a = c.take<uint64_t>(n + 1u);
        for (uint32_t ** a : {&sel, &ufirst, &ucount, &cq, &mq, &sst})
            *a = c.take<uint32_t>(nq);
        for (uint64_t ** a : {&sptr, &dptr})
            *a = c.take<uint64_t>(nq + 1u);
        raw = c.take<uint32_t>(stage_values);
        stage = c.take<uint32_t>(stage_values);
        noff = c.take<uint64_t>(C.units + 1u);
        sbytes = c.bytes<uint8_t>(C.bytes + 16u);
        enc = c.bytes<uint8_t>(lists_enc_workspace(C.units, nq));
        units = c.bytes<uint8_t>(nq != 0u ? lists_units_workspace(nq, stage_values) : 0u);
        bytes = c.used;
    }
};
} // namespace

size_t lists_remove_workspace(uint64_t nlists, uint64_t nq, uint64_t stage_values)
{
    if (nlists == 0)
        return 0;
    return RemWs(nullptr, nlists, nq, stage_values, RemCaps(nq, stage_values)).bytes;
}

// Launches, fixed by the sizes: reset, plan l, 3 x 2 run scans, heads l, segs,
// [offsets,] [stitch] -- 12 -- and with nq != 0 plan q, [plan p,] 2 x 2 run
// scans, 9 of the units decode, heads q, [compact,] 6 of the encoder -- 23:
// 35 at the most, 36 with d_err's reset by the entry point.
hipError_t launch_lists_remove(const ListsIndex & X, bool d1, const uint32_t * pos, uint64_t pos_values, const uint64_t * pptr,
                               const uint32_t * qlist, uint64_t nq, uint64_t stage_values, uint8_t * out, uint64_t out_cap,
                               uint64_t * off_out, uint64_t units_cap, uint64_t * lptr_out, uint32_t * lunit_out, uint32_t * ulast_out,
                               void * ws, unsigned long long * err, hipStream_t s)
{
    hipError_t e;
    const uint64_t n = X.nlists;
    if (n == 0)
        return launch(dev::k_rem_empty, 1, 64, s, lptr_out, lunit_out, off_out);
    const RemCaps C(nq, stage_values);
    const RemWs W(ws, n, nq, stage_values, C);
    const ListsEncPlanView V = lists_enc_plan_view(W.enc, C.units, nq);
    const dev::RemArgs A{.ix = X,
                         .pos = pos,
                         .pos_values = pos_values,
                         .pptr = pptr,
                         .qlist = qlist,
                         .nq = nq,
                         .stage_values = stage_values,
                         .out = out,
                         .out_cap = out_cap,
                         .off_out = off_out,
                         .units_cap = units_cap,
                         .lptr_out = lptr_out,
                         .lunit_out = lunit_out,
                         .ulast_out = ulast_out,
                         .err = err,
                         .hdr = W.hdr,
                         .c_tot = W.sc.tot,
                         .m_tot = W.sm.tot,
                         .nu_tot = W.snu.tot,
                         .tq_tot = W.stq.tot,
                         .kb_tot = W.skb.tot,
                         .c_pre = W.sc.pre,
                         .c_tile = W.sc.tile,
                         .m_pre = W.sm.pre,
                         .m_tile = W.sm.tile,
                         .nu_pre = W.snu.pre,
                         .nu_tile = W.snu.tile,
                         .tq_pre = W.stq.pre,
                         .tq_tile = W.stq.tile,
                         .kb_pre = W.skb.pre,
                         .kb_tile = W.skb.tile,
                         .qof = W.qof,
                         .keep = W.keep,
                         .subase = W.subase,
                         .kbpre = W.kbpre,
                         .lstart = W.lstart,
                         .sel = W.sel,
                         .ufirst = W.ufirst,
                         .ucount = W.ucount,
                         .cq = W.cq,
                         .mq = W.mq,
                         .sst = W.sst,
                         .sptr = W.sptr,
                         .dptr = W.dptr,
                         .raw = W.raw,
                         .stage = W.stage,
                         .noff = W.noff,
                         .sbytes = W.sbytes,
                         .ehdr = V.hdr,
                         .qsub = V.ubase,
                         .rec = V.rec,
                         .su_cap = C.units};
    auto grid = [](uint64_t items, uint64_t per) { return dim3(static_cast<uint32_t>((items + per - 1u) / per)); };
    using u64p = uint64_t *;
    if ((e = launch(dev::k_rem_reset, flat_grid(n, s), 256, s, A)) != hipSuccess)
        return e;
    if (nq != 0u)
    {
        if ((e = launch(dev::k_rem_plan_q, grid(std::max(nq, C.units), 256), 256, s, A)) != hipSuccess)
            return e;
        if (pos_values != 0u && (e = launch(dev::k_rem_plan_p, grid(pos_values, 256), 256, s, A)) != hipSuccess)
            return e;
        const uint64_t nqr = rem_runs(nq);
        if ((e = launch_run_scan_u64(W.sc.tot, nqr, W.sc.pre, W.sc.tile, u64p(&W.hdr->c), s)) != hipSuccess
            || (e = launch_run_scan_u64(W.sm.tot, nqr, W.sm.pre, W.sm.tile, u64p(&W.hdr->m), s)) != hipSuccess)
            return e;
    }
    if ((e = launch(dev::k_rem_plan_l, grid(n, 256), 256, s, A)) != hipSuccess)
        return e;
    const uint64_t nr = rem_runs(n);
    if ((e = launch_run_scan_u64(W.snu.tot, nr, W.snu.pre, W.snu.tile, u64p(&W.hdr->nu), s)) != hipSuccess
        || (e = launch_run_scan_u64(W.stq.tot, nr, W.stq.pre, W.stq.tile, u64p(&W.hdr->tq), s)) != hipSuccess
        || (e = launch_run_scan_u64t(W.skb.tot, nr, W.skb.pre, W.skb.tile, u64p(&W.hdr->kb), s)) != hipSuccess)
        return e;
    if (nq != 0u)
    {
        // the suffixes, every block once from the table; a refused plan leaves ranges the decode refuses or empty ones
        if ((e = launch_lists_units(X, d1, W.sel, W.ufirst, W.ucount, nq, W.raw, stage_values, W.dptr, W.units,
                                    reinterpret_cast<unsigned long long *>(&W.hdr->uerr), s))
            != hipSuccess)
            return e;
        if ((e = launch_by(d1, [](auto D1) { return dev::k_rem_heads_q<D1>; }, grid(nq + 1u, 256), 256, s, A)) != hipSuccess)
            return e;
    }
    if ((e = launch(dev::k_rem_heads_l, grid(n + 1u, 256), 256, s, A)) != hipSuccess)
        return e;
    if (nq != 0u)
    {
        if (stage_values != 0u && (e = launch(dev::k_rem_compact, grid(stage_values, 256), 256, s, A)) != hipSuccess)
            return e;
        if ((e = launch_lists_enc_planned(W.stage, W.sptr, nq, d1, d1 ? W.sst : nullptr, W.sbytes, C.bytes, W.noff, C.units, W.enc, s))
            != hipSuccess)
            return e;
    }
    if ((e = launch(dev::k_rem_segs, grid(n + 1u, 256), 256, s, A)) != hipSuccess)
        return e;
    if (units_cap != 0u && (e = launch_by(d1, [](auto D1) { return dev::k_rem_offsets<D1>; }, grid(units_cap, 256), 256, s, A)) != hipSuccess)
        return e;
    // the stream is never longer than the old bytes plus the staged ones
    const uint64_t span = std::min(out_cap, X.in_bytes + C.bytes);
    return span != 0u ? launch(dev::k_rem_stitch, grid(span, 4u * dev::kListsAppendTile), 256, s, A) : hipSuccess;
}

} // namespace tpf
