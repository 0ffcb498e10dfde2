// p4_lists_union.hip -- the sorted union of probe doc ids with resident
// posting lists (p4_lists.h): tpf_lists_union takes the
// intersection's arguments -- sorted CSR segments of probe values, one target
// list per segment -- and returns, per segment, the merged sequence of the
// probe and the list with where every value came from.  A probe value that is
// not in its list is a MISS: it goes L + M slots into its segment, L the list
// position it would be inserted at and M the misses before it.  A list value
// at position p goes p + (the misses with L <= p) slots in.  L comes from the
// intersection's lookup (p4_lists_intersect.hip, its EVERY form): every probe
// value's unit is decoded once into LDS and searched.  The list values come
// from k_un_dec's pipeline (p4_lists_units.hip) and the tails driver
// (p4_lists_dev.h) over the virtual units of the targeted lists, every unit
// decoded once from the skip table; the shift of each of a unit's 256 values
// is a histogram of the misses that land in the unit, in the wave's LDS, and
// its prefix sum.  No decoded value is staged in global memory, and nothing is
// sized by the index.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

// The result word after the flags pass: bits 0-8 q and kIxFound as the lookup
// left them, kUoMiss for a miss, kUoNone for a miss no unit holds (L = n),
// bits 16-22 the misses before it in its 64-index run.  An index outside every
// segment is neither a member nor a miss.
constexpr uint32_t kUoMiss = 0x400u;
constexpr uint32_t kUoNone = 0x800u;
constexpr uint32_t kUoListNone = 0xFFFFFFFFu; // TPF_LISTS_NONE
// k_uo_dec: units per wave and chunks in flight (k_ix_dec's, for its reason), and the workgroups per CU its LDS leaves room for
constexpr uint32_t kUoRun = 4;
constexpr uint32_t kUoNC = 4;
constexpr int kUoMinW = 6;

struct UoHdr
{
    unsigned long long vtotal; // virtual units: the units of the targeted lists
    unsigned long long ototal; // d_out_ptr[nq]: the sum of n_j + M_k
};

struct UoArgs
{
    ListsIndex ix;
    const uint32_t * probe;
    uint64_t pv;
    const uint64_t * probe_ptr;
    const uint32_t * qlist;
    uint64_t nq;
    uint32_t * out;
    uint64_t out_values;
    uint64_t vcap;              // the host's cap on the virtual units: out_values / 256 + nq
    uint64_t * out_ptr;
    uint32_t * out_pidx;
    uint32_t * out_tpos;
    ItemHdr * hdr;              // spare = the misses of the whole probe
    UoHdr * uh;
    const uint32_t * pu;        // per probe value: source unit | kRecTail, or kItemNone
    uint32_t * res;             // per probe value: the result word
    uint32_t * mtot;            // run scan of the miss flags over the probe's 64-index runs
    const uint32_t * mpre;
    const uint32_t * mtile;
    uint32_t * missbase;        // misses before probe_ptr[k], k <= nq
    uint32_t * mlb;             // L of every miss, in probe order: query k's at [missbase[k], missbase[k+1])
    uint32_t * totu;            // per query: the units of its list ...
    uint64_t * totv;            // ... and n_j + M_k
    const uint64_t * preu;
    const uint64_t * tileu;
    const uint64_t * prev;
    const uint64_t * tilev;
    uint32_t * vbase;           // first virtual unit of every query, nq + 1
    uint32_t * rec;             // records of the virtual units (p4_lists.h), the head carries k + 1
    unsigned long long * err;
};

// go / no-go of everything that writes the output: no query was refused and
// the result fits (then vtotal <= vcap follows, n values holding at most n/256
// + 1 units; it is checked all the same: vcap sizes the records)
__device__ __forceinline__ bool uo_go(const UoArgs & A)
{
    return items_go(A.hdr) && A.uh->ototal <= A.out_values && A.uh->vtotal <= A.vcap;
}

// misses at probe indices below p
__device__ __forceinline__ uint32_t uo_prefix(const UoArgs & A, uint64_t p)
{
    return p < A.pv ? run_base(A.mpre, A.mtile, p / 64u) + ((A.res[p] >> 16) & 127u) : A.hdr->spare;
}

// The first index of a[0 .. n) whose entry is >= key (a ascends under the
// precondition; whatever it holds, the answer lies in [0, n]).
__device__ __forceinline__ uint32_t uo_lower_bound(const uint32_t * __restrict a, uint32_t n, uint64_t key)
{
    uint32_t lo = 0u, hi = n;
    while (lo < hi)
    {
        const uint32_t m = lo + (hi - lo) / 2u;
        if (a[m] < key)
            lo = m + 1u;
        else
            hi = m;
    }
    return lo;
}

// Flags: every wave owns 64 consecutive probe indices, as k_ix_hits does; the
// miss flags' total goes to the run scan and the result word gets the flags
// and the misses before it in its run.
__global__ __launch_bounds__(256) void k_uo_flags(const UoArgs A)
{
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t run = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t i = run * 64u + t;
    if (run * 64u >= A.pv)
        return;
    uint32_t w = 0u;
    // the plan checked the segment pointers: they ascend and end inside the probe
    if (i < A.pv && items_go(A.hdr) && i >= A.probe_ptr[0] && i < A.probe_ptr[A.nq])
    {
        const uint32_t r = A.res[i];
        if (r == kItemNone)
            w = kUoMiss | kUoNone;
        else
            w = (r & (kIxQ | kIxFound)) | ((r & kIxFound) != 0u ? 0u : kUoMiss);
    }
    const uint32_t miss = (w & kUoMiss) != 0u ? 1u : 0u;
    const uint32_t incl = wave_incl_scan(miss);
    if (i < A.pv)
        A.res[i] = w | ((incl - miss) << 16);
    if (t == 0)
        A.mtot[run] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
}

// Plan over the QUERIES: the units of the target and n_j + M_k for the two run
// scans, the misses before every segment, and the records of the virtual units
// zeroed for the heads pass, up to the host's cap.  (The intersection's plan
// checked every query: the directory is read at checked indices only.)
__global__ __launch_bounds__(256) void k_uo_plan(const UoArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    const bool go = items_go(A.hdr);
    for (uint64_t k = gid; k <= A.nq; k += gsz)
    {
        const uint32_t mb = go ? uo_prefix(A, A.probe_ptr[k]) : 0u;
        A.missbase[k] = mb;
        if (k == A.nq)
            break;
        uint32_t units = 0u;
        uint64_t nv = 0u;
        if (go)
        {
            const uint32_t j = A.qlist[k];
            units = A.ix.list_unit[j + 1u] - A.ix.list_unit[j];
            nv = A.ix.ptr[j + 1u] - A.ix.ptr[j] + (uo_prefix(A, A.probe_ptr[k + 1u]) - mb);
        }
        A.totu[k] = units;
        A.totv[k] = nv;
    }
    for (uint64_t u = gid; u < A.vcap; u += gsz)
        A.rec[u] = 0u;
}

// Heads: the verdict (a refused query: nothing is written; a result that does
// not fit, by atomicMin under a parse error the lookup may have left),
// d_out_ptr, then per query its virtual unit base and the records of its
// list's first unit and of its tail, as k_sel_heads leaves them.
__global__ __launch_bounds__(256) void k_uo_heads(const UoArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    if (!items_go(A.hdr))
    {
        if (gid == 0 && A.err != nullptr)
            *A.err = A.ix.nunits + A.hdr->bad;
        return;
    }
    const bool go = uo_go(A);
    for (uint64_t k = gid; k < A.nq; k += gsz)
        A.out_ptr[k] = run_base(A.prev, A.tilev, k);
    if (gid == 0)
    {
        A.out_ptr[A.nq] = A.uh->ototal;
        if (!go && A.err != nullptr)
            atomicMin(A.err, static_cast<unsigned long long>(A.ix.nunits + A.nq));
    }
    if (!go)
        return;
    for (uint64_t k = gid; k < A.nq; k += gsz)
    {
        const uint32_t vb = static_cast<uint32_t>(run_base(A.preu, A.tileu, k)); // <= vtotal <= vcap < 2^31
        A.vbase[k] = vb;
        const uint32_t units = A.totu[k];
        const uint32_t j = A.qlist[k];
        const bool tail = ((A.ix.ptr[j + 1u] - A.ix.ptr[j]) & 255u) != 0u;
        if (units == 1u)
            A.rec[vb] = static_cast<uint32_t>(k + 1u) | (tail ? kRecTail : 0u);
        else if (units != 0u)
        {
            A.rec[vb] = static_cast<uint32_t>(k + 1u);
            if (tail)
                A.rec[vb + units - 1u] = kRecTail;
        }
    }
    if (gid == 0)
        A.vbase[A.nq] = static_cast<uint32_t>(A.uh->vtotal);
}

// L of probe index i of query k (list j): n_j where no unit holds the value,
// else the unit's first position plus q, held to n_j.
__device__ __forceinline__ uint32_t uo_pos(const UoArgs & A, uint64_t i, uint32_t r, uint32_t j)
{
    const uint64_t n = A.ix.ptr[j + 1u] - A.ix.ptr[j];
    uint64_t l = n;
    if ((r & kUoNone) == 0u)
        l = min_u64(256ull * ((A.pu[i] & kRecList) - A.ix.list_unit[j]) + (r & kIxQ), n);
    return static_cast<uint32_t>(l);
}

// Misses (HITS = false, before the list values) and the hits' probe indices
// (HITS = true, after them): one thread per probe index.  A miss leaves L in
// mlb, whatever the verdict, and goes to slot L + M of its segment; a hit
// leaves its index in d_out_pidx at the slot its list value took.  A slot
// outside the segment (an unsorted probe) is dropped.
template <bool HITS>
__global__ __launch_bounds__(256) void k_uo_probe(const UoArgs A)
{
    if (!items_go(A.hdr))
        return;
    const bool go = uo_go(A);
    if (HITS && (!go || A.out_pidx == nullptr))
        return;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < A.pv; i += gsz)
    {
        const uint32_t r = A.res[i];
        if ((r & (HITS ? kIxFound : kUoMiss)) == 0u)
            continue;
        const uint32_t k = segment_of(A.probe_ptr, A.nq, i);
        if (k == kItemNone)
            continue; // (the flags pass left no flag outside the segments)
        const uint32_t l = uo_pos(A, i, r, A.qlist[k]);
        const uint32_t mi = uo_prefix(A, i);
        if constexpr (!HITS)
            A.mlb[mi] = l; // mi < the misses <= pv
        if (!go)
            continue;
        const uint64_t slot = static_cast<uint64_t>(l) + (mi - A.missbase[k]);
        const uint64_t o = A.out_ptr[k];
        if (slot >= A.out_ptr[k + 1u] - o)
            continue;
        if constexpr (HITS)
            A.out_pidx[o + slot] = static_cast<uint32_t>(i);
        else
        {
            A.out[o + slot] = A.probe[i];
            if (A.out_pidx != nullptr)
                A.out_pidx[o + slot] = static_cast<uint32_t>(i);
            if (A.out_tpos != nullptr)
                A.out_tpos[o + slot] = kUoListNone;
        }
    }
}

// What a wave knows of one unit it writes, read back wave-uniformly.
struct UoUnit
{
    uint32_t a0, a1;  // the misses that land in the unit: mlb[a0 .. a1)
    uint32_t m0;      // the misses of the query before the unit
    uint32_t p0;      // the list position of the unit's first value
    uint64_t obase;   // the query's slice of the output ...
    uint64_t olen;    // ... and its length
};

// The misses before and inside unit `inl` of query k's list: two searches over
// the query's part of mlb.  `pend`: one past the last position that counts.
__device__ __forceinline__ void uo_unit_plan(const UoArgs & A, uint32_t k, uint32_t inl, uint64_t pend, UoUnit & U)
{
    const uint32_t mb = A.missbase[k];
    const uint32_t mk = A.missbase[k + 1u] - mb; // <= pv - mb: the flags ascend
    U.p0 = 256u * inl;
    U.m0 = uo_lower_bound(A.mlb + mb, mk, 256ull * inl);
    U.a0 = mb + U.m0;
    U.a1 = mb + uo_lower_bound(A.mlb + mb, mk, pend);
    if (U.a1 < U.a0)
        U.a1 = U.a0; // (an unsorted mlb)
    U.obase = A.out_ptr[k];
    U.olen = A.out_ptr[k + 1u] - U.obase;
}

// hist[b] = the misses of mlb[a0 .. a1) with L = p0 + b, 64 at a time, then
// their inclusive prefix over b in place: lane t scans its four counters
// 4t .. 4t + 3 and the lanes' totals.  Returns that prefix at 4t .. 4t + 3.
__device__ __forceinline__ void uo_hist(const UoArgs & A, uint32_t * hist, uint32_t a0, uint32_t a1, uint32_t p0, uint32_t t, uint32_t (&incl)[4])
{
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
        hist[4u * t + q] = 0u;
    wave_lds_sync();
    for (uint32_t c = a0; c < a1; c += 64u)
    {
        if (c + t < a1)
        {
            const uint32_t b = A.mlb[c + t] - p0;
            if (b < 256u)
                atomicAdd(&hist[b], 1u);
        }
    }
    wave_lds_sync();
    uint32_t s = 0u;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
    {
        s += hist[4u * t + q];
        incl[q] = s;
    }
    const uint32_t ex = wave_incl_scan(s) - s;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
        incl[q] += ex;
}

// One list value: position p of the list, `shift` misses at or before it.
__device__ __forceinline__ void uo_store(const UoArgs & A, uint64_t obase, uint64_t olen, uint32_t p, uint32_t shift, uint32_t v)
{
    const uint64_t slot = static_cast<uint64_t>(p) + shift;
    if (slot < olen)
    {
        __builtin_nontemporal_store(v, A.out + obase + slot);
        if (A.out_pidx != nullptr)
            A.out_pidx[obase + slot] = kUoListNone;
        if (A.out_tpos != nullptr)
            A.out_tpos[obase + slot] = p;
    }
}

// One decoded unit of cnt values goes out: lane t holds the values at
// positions r = t + 64q of the unit, so the lanes of one store name
// neighbouring slots.  With misses inside the unit the prefix of their
// histogram goes back to LDS and every value reads its own shift.
__device__ __forceinline__ void uo_write_unit(const UoArgs & A, const UoUnit & U, uint32_t * hist, uint32_t cnt, uint32_t t,
                                              const uint32_t (&v)[4])
{
    const uint32_t a0 = uni(U.a0), a1 = uni(U.a1), m0 = uni(U.m0), p0 = uni(U.p0);
    const uint64_t ob = uni64(U.obase), ol = uni64(U.olen);
    if (a1 != a0)
    {
        uint32_t incl[4];
        uo_hist(A, hist, a0, a1, p0, t, incl);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            hist[4u * t + q] = incl[q];
        wave_lds_sync();
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
        if (t + 64u * q < cnt)
            uo_store(A, ob, ol, p0 + t + 64u * q, m0 + (a1 != a0 ? hist[t + 64u * q] : 0u), v[q]);
}

// Full blocks: every wave owns a run of RUN consecutive VIRTUAL units of the
// targeted lists with the k_dec256v32w pipeline, as k_un_dec does; d_qlist is
// the selection and every list a whole range.  Lane t resolves the query of
// virtual unit first + t, its source unit and start, and the misses before and
// inside the unit; the plan of every unit waits in LDS.  The decoded block,
// lane t holding positions 4t .. 4t + 3, turns through LDS to positions
// t + 64q for the stores.  (Short runs, as in k_ix_dec: a unit with misses
// waits for their L from memory once, behind the chunk loads in issue order.)
template <uint32_t RUN, uint32_t NC, int MINW>
__global__ __launch_bounds__(256, MINW) void k_uo_dec(const UoArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t vals[4][256];
    __shared__ uint32_t srcu[4][RUN], starts[4][RUN];
    __shared__ UoUnit units[4][RUN];
    if (!uo_go(A))
        return;
    constexpr uint32_t kRun = RUN;
    const uint64_t vt = A.uh->vtotal;
    const WaveRun R = wave_run(A.ix.in, A.ix.in_bytes, kRun, vt);
    const uint32_t t = R.t, wv = R.wv;
    const uint64_t first = R.first;
    if (first >= vt)
        return; // the grid is sized by the host's cap
    uint32_t * slot = slots[wv];
    uint32_t * scr = scratch[wv];
    const bool valid = t < R.n;
    const uint64_t v = first + t;
    const uint32_t r = valid ? A.rec[v] : 0u;
    const bool full = valid && (r & kRecTail) == 0u;
    const uint64_t fullmask = __ballot(full);
    if (fullmask == 0ull)
        return; // a run of tails only

    const uint32_t id = run_ids(r, A.vbase, A.nq, first, t); // the query of every unit
    const uint32_t vb = valid ? A.vbase[id] : 0u;
    const uint32_t lj = valid ? A.qlist[id] : 0u;
    const uint32_t inl = static_cast<uint32_t>(v) - vb; // unit v - vb of its list
    // the source unit: the plan checked qlist[k] < nlists and list_unit[j] + units_j <= nunits
    const uint32_t su = full ? A.ix.list_unit[lj] + inl : 0u;
    const uint64_t o = full ? A.ix.off[su] : 0ull;
    const uint64_t e = full ? A.ix.off[su + 1u] : 0ull;
    RunPlaneT<kSlotBytes, true> P;
    P.init(R.in_base, R.in_end, o, e, full);
    if (t < kRun)
    {
        srcu[wv][t] = full ? su : 0xFFFFFFFFu;
        starts[wv][t] = full ? unit_start(A.ix.list_unit, A.ix.start0, A.ix.unit_last, lj, su) : 0u;
        if (full)
            uo_unit_plan(A, id, inl, 256ull * inl + 256u, units[wv][t]);
    }
    wave_lds_sync();
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);

    uint64_t badmask = 0u;
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((fullmask >> jj) & 1ull) == 0ull)
            return;
        u32x4 x;
        decode_full_unit<true>(P, c, jj, slot, scr, uni(starts[wv][jj]), t, x, badmask);
        reinterpret_cast<u32x4 *>(vals[wv])[t] = x;
        wave_lds_sync();
        const uint32_t v[4] = {vals[wv][t], vals[wv][t + 64u], vals[wv][t + 128u], vals[wv][t + 192u]};
        uo_write_unit(A, units[wv][jj], hist[wv], 256u, t, v);
        wave_lds_sync();
    });
    report_bad_units(A.err, badmask, t < kRun ? srcu[wv][t] : 0xFFFFFFFFu, t);
}

// Tails: every wave owns kRunDefault consecutive QUERIES through the tails
// driver (tail_units, p4_lists_dev.h), as k_un_tails does for selections; lane
// t holds query first + t's tail unit -- the list's last unit, n % 256 values
// -- or nothing.  Lane t holds positions t + 64q of the unit, as uo_write_unit
// takes them.
template <uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_uo_tails(const UoArgs A)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    __shared__ uint32_t hist[4][256];
    __shared__ UoUnit units[4][kRunDefault];
    if (!uo_go(A))
        return;
    const WaveRun R = wave_run(A.ix.in, A.ix.in_bytes, kRunDefault, A.nq);
    const uint32_t t = R.t, wv = R.wv;
    if (R.first >= A.nq)
        return;
    const uint64_t k = R.first + t;
    const uint32_t lj = t < R.n ? A.qlist[k] : 0u;
    const uint64_t n = t < R.n ? A.ix.ptr[lj + 1u] - A.ix.ptr[lj] : 0ull;
    const uint32_t cnt = static_cast<uint32_t>(n & 255u);
    const bool has = cnt != 0u;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0ull)
        return;
    const uint32_t inl = static_cast<uint32_t>(n >> 8);
    const uint32_t su = has ? A.ix.list_unit[lj] + inl : 0u; // the list's last unit: the plan checked the unit count
    tail_units<true, NC>(
        R, A.ix.off, has, hasmask, su, cnt, slots[wv], scratch[wv], A.err,
        [&] {
            // with the start, behind the offsets' loads: the plan of every lane's unit, which waits in LDS
            uint32_t startv = 0u;
            if (has)
            {
                startv = unit_start(A.ix.list_unit, A.ix.start0, A.ix.unit_last, lj, su);
                uo_unit_plan(A, static_cast<uint32_t>(k), inl, n, units[wv][t]); // a miss with L = n shifts no list value
            }
            wave_lds_sync();
            return startv;
        },
        [&](uint32_t jj, uint32_t cj, const TailVals & x) { uo_write_unit(A, units[wv][jj], hist[wv], cj, t, x.v); });
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
// Workspace of the union: the item header and the union's | three run scans
// over the 64-value runs of the probe (item heads, misses) and two over the
// queries | per probe value its unit word, its list, its result and the L of a
// miss | per item its first probe index and its end | per query its units,
// n_j + M_k, the misses before it and its virtual unit base | the records of
// the virtual units (vcap), each 256-byte aligned.
struct UoWs
{
    dev::ItemHdr * hdr;
    dev::UoHdr * uh;
    RunScanWs<uint32_t> scani, scanm;
    RunScanWs<uint64_t> scanu;
    uint32_t *pu, *pl, *res, *mlb, *ihead, *iend;
    uint64_t *totv, *prev, *tilev;
    uint32_t *missbase, *vbase, *rec;
    size_t bytes;

    UoWs(void * ws, uint64_t nq, uint64_t pv, uint64_t vcap)
    {
        WsCarver c(ws);
        const uint64_t nruns = (pv + 63u) / 64u;
        hdr = c.take<dev::ItemHdr>(1);
        uh = c.take<dev::UoHdr>(1);
        scani = c.scan<uint32_t>(nruns);
        scanm = c.scan<uint32_t>(nruns);
        scanu = c.scan<uint64_t>(nq);
        for (uint32_t ** a : {&pu, &pl, &res, &mlb, &ihead, &iend})
            *a = c.take<uint32_t>(pv);
        totv = c.take<uint64_t>(nq);
        prev = c.take<uint64_t>(nq);
        tilev = c.bytes<uint64_t>(al256(8u * RunScanWs<uint64_t>::tiles(nq)) + 256u);
        missbase = c.take<uint32_t>(nq + 1u);
        vbase = c.take<uint32_t>(nq + 1u);
        rec = c.take<uint32_t>(vcap);
        bytes = c.used;
    }
};
} // namespace

size_t lists_union_workspace(uint64_t nq, uint64_t probe_values, uint64_t out_values)
{
    return UoWs(nullptr, nq, probe_values, lists_select_unit_cap(nq, out_values)).bytes;
}

hipError_t launch_lists_union(const ListsIndex & X, const uint32_t * probe, uint64_t pv, const uint64_t * probe_ptr, const uint32_t * qlist,
                              uint64_t nq, uint32_t * out, uint64_t out_values, uint64_t * out_ptr, uint32_t * out_pidx, uint32_t * out_tpos,
                              void * ws, unsigned long long * err, hipStream_t s)
{
    if (nq == 0)
    {
        hipError_t e = err ? fill_u32(err, 0xFFFFFFFFu, 2, s) : hipSuccess;
        return e != hipSuccess ? e : (out_ptr ? fill_u32(out_ptr, 0u, 2, s) : hipSuccess);
    }
    const uint64_t vcap = lists_select_unit_cap(nq, out_values);
    if (nq > 0x7FFFFFFFull || pv > 0x7FFFFFFFull || X.nlists > 0x7FFFFFFFull || X.nunits > 0x7FFFFFFFull || vcap > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const UoWs W(ws, nq, pv, vcap);
    const uint64_t nruns = (pv + 63u) / 64u;
    // one wave per 64 probe indices, per kUoRun virtual units, per kRunDefault queries: at least one workgroup for an empty probe
    const uint32_t rgrid = static_cast<uint32_t>(std::max<uint64_t>(1, (nruns + 3u) / 4u));
    const uint32_t vgrid = wave_grid(vcap, dev::kUoRun), tgrid = wave_grid(nq, dev::kRunDefault);
    const uint32_t pgrid = flat_grid(pv, s);
    hipError_t e = launch_items_reset(err, W.hdr, s);
    if (e != hipSuccess)
        return e;
    // ---- the lookup: the intersection's plan, items and decode, every probe value's q recorded
    if ((e = launch_ix_plan(X, probe, pv, probe_ptr, qlist, nq, W.hdr, W.pu, W.pl, s)) != hipSuccess)
        return e;
    if ((e = launch_items(pv, W.hdr, W.pu, W.pl, W.scani, W.ihead, W.iend, W.res, s)) != hipSuccess)
        return e;
    const dev::IxArgs L{.it = {.ix = X, .hdr = W.hdr, .pu = W.pu, .pl = W.pl, .ihead = W.ihead, .iend = W.iend, .err = err},
                        .probe = probe,
                        .pv = pv,
                        .res = W.res};
    if ((e = launch_ix_lookup(L, true, s)) != hipSuccess)
        return e;
    // ---- the misses, the sizes, the verdict
    const dev::UoArgs A{.ix = X,
                        .probe = probe,
                        .pv = pv,
                        .probe_ptr = probe_ptr,
                        .qlist = qlist,
                        .nq = nq,
                        .out = out,
                        .out_values = out_values,
                        .vcap = vcap,
                        .out_ptr = out_ptr,
                        .out_pidx = out_pidx,
                        .out_tpos = out_tpos,
                        .hdr = W.hdr,
                        .uh = W.uh,
                        .pu = W.pu,
                        .res = W.res,
                        .mtot = W.scanm.tot,
                        .mpre = W.scanm.pre,
                        .mtile = W.scanm.tile,
                        .missbase = W.missbase,
                        .mlb = W.mlb,
                        .totu = W.scanu.tot,
                        .totv = W.totv,
                        .preu = W.scanu.pre,
                        .tileu = W.scanu.tile,
                        .prev = W.prev,
                        .tilev = W.tilev,
                        .vbase = W.vbase,
                        .rec = W.rec,
                        .err = err};
    if ((e = launch(dev::k_uo_flags, rgrid, 256, s, A)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u32_single(W.scanm.tot, nruns, W.scanm.pre, W.scanm.tile, &W.hdr->spare, s)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_uo_plan, flat_grid(std::max(nq + 1u, vcap), s), 256, s, A)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64(W.scanu.tot, nq, W.scanu.pre, W.scanu.tile, reinterpret_cast<uint64_t *>(&W.uh->vtotal), s)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64t(W.totv, nq, W.prev, W.tilev, reinterpret_cast<uint64_t *>(&W.uh->ototal), s)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_uo_heads, flat_grid(nq, s), 256, s, A)) != hipSuccess)
        return e;
    // ---- the output: misses, list values, then the hits' probe indices over the list values' words
    if ((e = launch(dev::k_uo_probe<false>, pgrid, 256, s, A)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_uo_dec<dev::kUoRun, dev::kUoNC, dev::kUoMinW>, vgrid, 256, s, A)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_uo_tails<dev::kTailsNC>, tgrid, 256, s, A)) != hipSuccess)
        return e;
    return out_pidx != nullptr ? launch(dev::k_uo_probe<true>, pgrid, 256, s, A) : hipSuccess;
}

} // namespace tpf
