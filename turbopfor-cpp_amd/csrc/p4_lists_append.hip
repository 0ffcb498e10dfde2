// p4_lists_append.hip -- tpf_lists_append: postings appended to the lists of a
// resident index in one submission with no host round trip
// (include/turbopfor_gpu.h).  A 256v32 block's bytes depend on
// its 256 values and the value before it only, so every full block of the old
// stream is moved as bytes; only the p4Enc32 tail of a list that receives
// values is decoded, put in front of the list's additions and encoded again.
//   plan   : a thread per output list: the checks, the values of its old tail
//            that are staged (tv), its new units (m), the bytes of the tail
//            it drops (db); four run totals per 64 lists
//   scans  : run scans of the four (p4_scan.h)
//   heads  : the verdict, then per list d_list_ptr_out, d_list_unit_out, the
//            staged lists' pointers / unit bases / unit records / delta-1
//            starts, and the prefix of the kept bytes
//   stage  : the additions (a thread per value) and the old tails (k_un_tails's
//            pipeline, a wave per 16 lists) into one dense value array
//   encode : the many-lists encoder's passes (p4_lists_enc.hip) over the staged
//            lists into a byte buffer of the workspace, with their offsets
//   segs   : a thread per list: where its bytes start in d_out; the capacity
//   offsets: a thread per output unit: d_off_out and d_unit_last_out
//   stitch : the output stream cut into kListsAppendTile-byte tiles of d_out, a wave
//            per tile: it finds its lists by a search over the lists' starts
//            and moves each list's kept bytes (from d_in) and new bytes (from
//            the workspace) with destination-aligned 16-byte stores
//            (stitch_tile, p4_lists_stitch.h: tpf_lists_remove runs it too)
// Every kernel after the heads reads the go flag of the header first.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_generic.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"
#include "p4_lists_stitch.h"
#include "turbopfor_gpu.h"

#include <algorithm>

namespace tpf::dev
{

constexpr uint32_t kAppTailMax = 4096; // more bytes than a p4Enc32 unit of <= 255 values can have

struct AppHdr
{
    unsigned long long bad;  // first list that fails a structure check (~0: none)
    unsigned long long tbad; // lowest parsed tail unit whose offsets lie outside the stream (~0: none)
    unsigned long long tv, tt, m, db; // totals of the four scans
    unsigned long long nunits_out;
    uint32_t go;  // the heads pass: structure, tails' offsets and units_cap are sound
    uint32_t fit; // the segs pass: the stream fits out_cap
};

struct AppArgs
{
    ListsIndex ix; // the old index; empty: nunits = nlists = in_bytes = 0
    const uint32_t * add;
    uint64_t add_values;
    const uint64_t * aptr;
    uint64_t n; // nlists_out
    uint8_t * out;
    uint64_t out_cap;
    uint64_t * off_out;
    uint64_t units_cap;
    uint64_t * lptr_out;
    uint32_t * lunit_out;
    uint32_t * ulast_out;
    unsigned long long * err;
    // workspace
    AppHdr * hdr;
    uint32_t *tv_tot, *tt_tot, *m_tot, *db_tot; // run totals
    const uint64_t *tv_pre, *tv_tile, *tt_pre, *tt_tile, *m_pre, *m_tile, *db_pre, *db_tile;
    uint32_t *tv, *m, *db;    // per list
    uint32_t * sst;           // per list: delta-1 start of its staged values
    uint64_t * sptr;          // n + 1: staged lists
    uint64_t * kbpre;         // n + 1: kept bytes of the lists before
    uint64_t * lstart;        // n + 1: first output byte of every list
    uint32_t * stage;         // staged values
    uint64_t * noff;          // offsets of the staged lists' units in sbytes
    uint8_t * sbytes;         // their bytes
    ListsHdr * ehdr;          // the encoder's view (p4_lists.h)
    uint32_t * subase;        // n + 1: first staged unit of every list
    uint32_t * rec;           // records of the staged units
    uint64_t su_cap;
    uint64_t ebase; // the caller's nunits: the base of the list codes of d_err
};

__device__ __forceinline__ void app_err(unsigned long long * err, unsigned long long v)
{
    if (err != nullptr)
        atomicMin(err, v);
}

__global__ void k_app_reset(AppHdr * hdr, ListsHdr * ehdr)
{
    if (threadIdx.x == 0)
    {
        *hdr = AppHdr{~0ull, ~0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0u, 0u};
        if (ehdr != nullptr)
            *ehdr = ListsHdr{0ull, 0ull}; // no go until the heads pass says so
    }
}

// nlists_out == 0: the empty result
__global__ void k_app_empty(uint64_t * lptr_out, uint32_t * lunit_out, uint64_t * off_out)
{
    if (threadIdx.x == 0)
    {
        lptr_out[0] = 0ull;
        lunit_out[0] = 0u;
        off_out[0] = 0ull;
    }
}

// ---- plan ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_app_plan(const AppArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t j = gid;
    uint32_t tv = 0u, m = 0u, db = 0u;
    if (j < A.n)
    {
        const bool old = j < A.ix.nlists;
        const uint64_t p0 = old ? A.ix.ptr[j] : 0ull, p1 = old ? A.ix.ptr[j + 1u] : 0ull;
        const uint64_t a0 = A.aptr[j], a1 = A.aptr[j + 1u];
        const uint64_t oldn = p1 - p0;
        const uint64_t cnt = (oldn >> 8) + ((oldn & 255u) != 0u ? 1u : 0u);
        const uint64_t lu0 = old ? A.ix.list_unit[j] : 0u, lu1 = old ? A.ix.list_unit[j + 1u] : 0u;
        bool bad = p1 < p0 || a1 < a0 || a1 > A.add_values || lu1 - lu0 != cnt || lu1 > A.ix.nunits;
        if (!bad)
        {
            const uint64_t addn = a1 - a0; // < 2^31
            const uint32_t r = static_cast<uint32_t>(oldn & 255u);
            const bool tt = r != 0u && addn != 0u;
            const uint64_t keep = cnt - (tt ? 1u : 0u);
            if (cnt != 0u)
            {
                // the ends of the copied range; the dropped tail's offsets
                const uint64_t o0 = A.ix.off[lu0], o1 = A.ix.off[lu0 + keep];
                bad = o0 > o1 || o1 > A.ix.in_bytes;
                if (!bad && tt)
                {
                    const uint64_t o2 = A.ix.off[lu1];
                    if (o2 < o1 || o2 > A.ix.in_bytes || o2 - o1 > kAppTailMax)
                        atomicMin(&A.hdr->tbad, static_cast<unsigned long long>(lu1 - 1u));
                    else
                        db = static_cast<uint32_t>(o2 - o1);
                }
            }
            if (!bad)
            {
                tv = tt ? r : 0u;
                m = static_cast<uint32_t>((tv + addn + 255u) >> 8);
            }
            else
                db = 0u;
        }
        if (bad)
            atomicMin(&A.hdr->bad, static_cast<unsigned long long>(j));
        A.tv[j] = tv;
        A.m[j] = m;
        A.db[j] = db;
    }
    // gid < 64 * runs for every thread of the grid's last block up to the run's end
    const uint64_t run = gid / 64u;
    if (run * 64u < A.n)
    {
        publish_run_total(A.tv_tot, run, tv, t);
        publish_run_total(A.tt_tot, run, tv != 0u ? 1u : 0u, t);
        publish_run_total(A.m_tot, run, m, t);
        publish_run_total(A.db_tot, run, db, t);
    }
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t u = gid; u < A.su_cap; u += gsz)
        A.rec[u] = 0u;
}

// ---- heads --------------------------------------------------------------------
template <bool D1>
__global__ __launch_bounds__(256) void k_app_heads(const AppArgs A)
{
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const AppHdr h = *A.hdr;
    if (h.bad != ~0ull || h.tbad != ~0ull)
    {
        if (j == 0)
            app_err(A.err, h.tbad != ~0ull ? h.tbad : A.ebase + h.bad);
        return;
    }
    const uint64_t lu00 = A.ix.nlists != 0u ? A.ix.list_unit[0] : 0u;
    const uint64_t luN = A.ix.nlists != 0u ? A.ix.list_unit[A.ix.nlists] : 0u;
    const uint64_t nuo = (luN - lu00) - h.tt + h.m;
    const bool ufit = nuo <= A.units_cap && nuo <= 0x7FFFFFFFull;
    const bool in = j < A.n;
    const uint32_t tv = in ? A.tv[j] : 0u, m = in ? A.m[j] : 0u, db = in ? A.db[j] : 0u;
    const uint32_t ttv = tv != 0u ? 1u : 0u;
    // exclusive prefixes: the run's base plus the wave's scan (every lane of the wave takes part)
    uint64_t TV = wave_incl_scan(tv) - tv, TT = wave_incl_scan(ttv) - ttv, M = wave_incl_scan(m) - m, DB = wave_incl_scan(db) - db;
    if (j > A.n)
        return;
    if (in)
    {
        const uint64_t run = j / 64u;
        TV += run_base(A.tv_pre, A.tv_tile, run);
        TT += run_base(A.tt_pre, A.tt_tile, run);
        M += run_base(A.m_pre, A.m_tile, run);
        DB += run_base(A.db_pre, A.db_tile, run);
    }
    else
    {
        TV = h.tv, TT = h.tt, M = h.m, DB = h.db;
    }
    const uint64_t jo = j < A.ix.nlists ? j : A.ix.nlists; // lists past the old index are empty there
    const uint64_t lu = A.ix.nlists != 0u ? A.ix.list_unit[jo] : 0u;
    const uint64_t oldoff = A.ix.nlists != 0u ? A.ix.ptr[jo] - A.ix.ptr[0] : 0ull;
    const uint64_t a0 = A.aptr[j];
    const uint64_t addoff = a0 - A.aptr[0];
    A.lptr_out[j] = oldoff + addoff;
    A.lunit_out[j] = static_cast<uint32_t>((lu - lu00) - TT + M);
    if (!ufit)
    {
        if (j == A.n)
            app_err(A.err, A.ebase + A.n);
        return;
    }
    A.sptr[j] = addoff + TV;
    A.subase[j] = static_cast<uint32_t>(M);
    A.kbpre[j] = (A.ix.nunits != 0u && A.ix.nlists != 0u ? A.ix.off[lu] - A.ix.off[lu00] : 0ull) - DB;
    if (in)
    {
        const uint64_t addn = A.aptr[j + 1u] - a0;
        const bool tail = ((tv + addn) & 255u) != 0u;
        if (m == 1u)
            A.rec[M] = static_cast<uint32_t>(j + 1u) | (tail ? kRecTail : 0u);
        else if (m != 0u)
        {
            A.rec[M] = static_cast<uint32_t>(j + 1u);
            if (tail)
                A.rec[M + m - 1u] = kRecTail;
        }
        if constexpr (D1)
        {
            // the staged values continue the list: from the last kept full block, or from start0
            const uint64_t oldn = j < A.ix.nlists ? A.ix.ptr[j + 1u] - A.ix.ptr[j] : 0ull;
            A.sst[j] = oldn < 256u ? (A.ix.start0 != nullptr ? A.ix.start0[j] : 0u) : A.ix.unit_last[lu + (oldn >> 8) - 1u];
        }
    }
    else
    {
        *A.ehdr = ListsHdr{~0ull, h.m};
        if (h.m == 0u)
            A.noff[0] = 0ull;
        A.hdr->nunits_out = nuo;
        A.hdr->go = 1u;
    }
}

// ---- stage: the additions -----------------------------------------------------
// (find_list, p4_lists_dev.h, for the wave's first value; gallop, p4_lists_stitch.h, for the others)
__global__ __launch_bounds__(256) void k_app_stage_add(const AppArgs A)
{
    if (A.hdr->go == 0u)
        return;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t p = A.aptr[0] + i, end = A.aptr[A.n];
    const uint64_t pw = p - t; // the wave's first value
    if (pw >= end)
        return;
    // the last j with aptr[j] <= p (aptr[0] <= p < aptr[n]): the wave's first value by the cooperative search, the others from it
    const uint32_t j0 = find_list(A.aptr, static_cast<uint32_t>(A.n), pw, t);
    if (i >= A.add_values || p >= end)
        return;
    const uint32_t lo = gallop(A.aptr, static_cast<uint32_t>(A.n), j0, p);
    A.stage[A.sptr[lo] + A.tv[lo] + (p - A.aptr[lo])] = A.add[p];
}

// ---- stage: the old tails -----------------------------------------------------
// Every wave owns kRunDefault consecutive lists through the tails driver
// (tail_units, p4_lists_dev.h); lane t holds list first + t's old tail -- the
// list's last unit, tv values -- or nothing.  The staged values are read again
// at once by the encoder's passes: they are stored plainly.
template <bool D1, uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_app_stage_tails(const AppArgs A)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    if (A.hdr->go == 0u)
        return;
    const WaveRun R = wave_run(A.ix.in, A.ix.in_bytes, kRunDefault, A.ix.nlists);
    const uint32_t t = R.t;
    if (R.first >= A.ix.nlists)
        return;
    const uint64_t k = R.first + t;
    const uint32_t cnt = t < R.n ? A.tv[k] : 0u;
    const bool has = cnt != 0u;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0ull)
        return;
    const uint32_t su = has ? A.ix.list_unit[k + 1u] - 1u : 0u; // the list's last unit
    uint64_t opos = 0ull;
    tail_units<D1, NC>(
        R, A.ix.off, has, hasmask, su, cnt, slots[R.wv], scratch[R.wv], A.err,
        [&] {
            // where the staged list begins, gathered behind the offsets' loads
            opos = has ? A.sptr[k] : 0ull;
            return D1 && has ? A.sst[k] : 0u;
        },
        tail_store<false>(A.stage, opos, t));
}

// ---- segs: where every list's bytes start, and the capacity -----------------------
__global__ __launch_bounds__(256) void k_app_segs(const AppArgs A)
{
    if (A.hdr->go == 0u)
        return;
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j > A.n)
        return;
    const uint64_t s = A.kbpre[j] + A.noff[A.subase[j]];
    A.lstart[j] = s;
    if (j == A.n)
    {
        A.off_out[A.hdr->nunits_out] = s;
        if (s > A.out_cap)
            app_err(A.err, A.ebase + A.n + 1u);
        else
            A.hdr->fit = 1u;
    }
}

// ---- offsets ------------------------------------------------------------------
template <bool D1>
__global__ __launch_bounds__(256) void k_app_offsets(const AppArgs A)
{
    if (A.hdr->go == 0u)
        return;
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t nuo = A.hdr->nunits_out;
    if (u - t >= nuo)
        return;
    // the last j with lunit_out[j] <= u (lunit_out[0] = 0 <= u < lunit_out[n]), as k_app_stage_add finds its list
    const uint32_t j0 = find_list(A.lunit_out, static_cast<uint32_t>(A.n), static_cast<uint32_t>(u - t), t); // u - t < nuo < 2^31
    if (u >= nuo)
        return;
    const uint64_t j = gallop(A.lunit_out, static_cast<uint32_t>(A.n), j0, u);
    const uint32_t local = static_cast<uint32_t>(u) - A.lunit_out[j];
    const bool old = j < A.ix.nlists;
    const uint32_t lu = old ? A.ix.list_unit[j] : 0u;
    const uint32_t keep = old ? A.ix.list_unit[j + 1u] - lu - (A.tv[j] != 0u ? 1u : 0u) : 0u;
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
            A.ulast_out[u] = A.stage[min_u64(A.sptr[j] + 256ull * (v + 1u), A.sptr[j + 1u]) - 1u];
    }
}

// ---- stitch -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_app_stitch(const AppArgs A) { stitch_tile(A, A.n); }

} // namespace tpf::dev

namespace tpf
{

namespace
{
uint64_t app_runs(uint64_t n) { return (n + 63u) / 64u; }

// Capacities of the staging, from the sizes alone: at most T lists receive
// values, at most Tt of them have an old tail (<= 255 values each), and a list
// that receives a values is staged as at most a / 256 + 2 units.
struct AppCaps
{
    uint64_t T, Tt, vals, units, bytes;
    AppCaps(uint64_t nunits, uint64_t n, uint64_t add_values)
    {
        T = std::min(n, add_values);
        Tt = std::min(T, nunits);
        vals = add_values + 255u * Tt;
        units = add_values / 256u + 2u * T + 1u; // never 0: the encoder's passes always run
        bytes = tpf_p4nenc256v32_lists_bound(vals, T);
    }
};

// Workspace: header | four run scans over the lists' 64-runs | tv, m, db, sst
// (n each) | sptr, kbpre, lstart (n + 1 each, u64) | staged values | staged
// units' offsets | staged bytes (+ 16: the stitch reads whole dwords) | the
// encoder's workspace, each 256-byte aligned.
struct AppWs
{
    dev::AppHdr * hdr;
    RunScanWs<uint64_t> stv, stt, sm, sdb;
    uint32_t *tv, *m, *db, *sst, *stage;
    uint64_t *sptr, *kbpre, *lstart, *noff;
    uint8_t * sbytes;
    void * enc;
    size_t bytes;

    AppWs(void * ws, uint64_t n, const AppCaps & C)
    {
        WsCarver c(ws);
        hdr = c.take<dev::AppHdr>(1);
        for (RunScanWs<uint64_t> * s : {&stv, &stt, &sm, &sdb})
            *s = c.scan<uint64_t>(app_runs(n));
        for (uint32_t ** a : {&tv, &m, &db, &sst})
            *a = c.take<uint32_t>(n);
        for (uint64_t ** a : {&sptr, &kbpre, &lstart})
            *a = c.take<uint64_t>(n + 1u);
        stage = c.take<uint32_t>(C.vals);
        noff = c.take<uint64_t>(C.units + 1u);
        sbytes = c.bytes<uint8_t>(C.bytes + 16u);
        enc = c.bytes<uint8_t>(lists_enc_workspace(C.units, n));
        bytes = c.used;
    }
};
} // namespace

size_t lists_append_workspace(uint64_t nunits, uint64_t nlists_out, uint64_t add_values)
{
    if (nlists_out == 0)
        return 0;
    return AppWs(nullptr, nlists_out, AppCaps(nunits, nlists_out, add_values)).bytes;
}

// Launches, fixed by the sizes: reset, plan, 4 x 2 run scans, heads, [stage
// additions, stage tails,] 6 of the encoder, segs, [offsets,] [stitch] -- 22
// at the most, 23 with d_err's reset by the entry point.
hipError_t launch_lists_append(ListsIndex X, bool d1, const uint32_t * add, uint64_t add_values, const uint64_t * aptr, uint64_t n,
                               uint8_t * out, uint64_t out_cap, uint64_t * off_out, uint64_t units_cap, uint64_t * lptr_out,
                               uint32_t * lunit_out, uint32_t * ulast_out, void * ws, unsigned long long * err, hipStream_t s)
{
    hipError_t e;
    const uint64_t ebase = X.nunits;
    if (n == 0)
        return launch(dev::k_app_empty, 1, 64, s, lptr_out, lunit_out, off_out);
    if (X.nunits == 0 || X.nlists == 0) // an empty old index
        X.nunits = 0, X.nlists = 0, X.in_bytes = 0;
    const AppCaps C(X.nunits, n, add_values);
    const AppWs W(ws, n, C);
    const ListsEncPlanView V = lists_enc_plan_view(W.enc, C.units, n);
    const dev::AppArgs A{.ix = X,
                         .add = add,
                         .add_values = add_values,
                         .aptr = aptr,
                         .n = n,
                         .out = out,
                         .out_cap = out_cap,
                         .off_out = off_out,
                         .units_cap = units_cap,
                         .lptr_out = lptr_out,
                         .lunit_out = lunit_out,
                         .ulast_out = ulast_out,
                         .err = err,
                         .hdr = W.hdr,
                         .tv_tot = W.stv.tot,
                         .tt_tot = W.stt.tot,
                         .m_tot = W.sm.tot,
                         .db_tot = W.sdb.tot,
                         .tv_pre = W.stv.pre,
                         .tv_tile = W.stv.tile,
                         .tt_pre = W.stt.pre,
                         .tt_tile = W.stt.tile,
                         .m_pre = W.sm.pre,
                         .m_tile = W.sm.tile,
                         .db_pre = W.sdb.pre,
                         .db_tile = W.sdb.tile,
                         .tv = W.tv,
                         .m = W.m,
                         .db = W.db,
                         .sst = W.sst,
                         .sptr = W.sptr,
                         .kbpre = W.kbpre,
                         .lstart = W.lstart,
                         .stage = W.stage,
                         .noff = W.noff,
                         .sbytes = W.sbytes,
                         .ehdr = V.hdr,
                         .subase = V.ubase,
                         .rec = V.rec,
                         .su_cap = C.units,
                         .ebase = ebase};
    auto grid = [](uint64_t items, uint64_t per) { return dim3(static_cast<uint32_t>((items + per - 1u) / per)); };
    if ((e = launch(dev::k_app_reset, 1, 64, s, W.hdr, V.hdr)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_app_plan, grid(n, 256), 256, s, A)) != hipSuccess)
        return e;
    const uint64_t nr = app_runs(n);
    using u64p = uint64_t *;
    if ((e = launch_run_scan_u64(W.stv.tot, nr, W.stv.pre, W.stv.tile, u64p(&W.hdr->tv), s)) != hipSuccess
        || (e = launch_run_scan_u64(W.stt.tot, nr, W.stt.pre, W.stt.tile, u64p(&W.hdr->tt), s)) != hipSuccess
        || (e = launch_run_scan_u64(W.sm.tot, nr, W.sm.pre, W.sm.tile, u64p(&W.hdr->m), s)) != hipSuccess
        || (e = launch_run_scan_u64(W.sdb.tot, nr, W.sdb.pre, W.sdb.tile, u64p(&W.hdr->db), s)) != hipSuccess)
        return e;
    if ((e = launch_by(d1, [](auto D1) { return dev::k_app_heads<D1>; }, grid(n + 1u, 256), 256, s, A)) != hipSuccess)
        return e;
    if (add_values != 0u)
    {
        if ((e = launch(dev::k_app_stage_add, grid(add_values, 256), 256, s, A)) != hipSuccess)
            return e;
        if (X.nlists != 0u
            && (e = launch_by(d1, [](auto D1) { return dev::k_app_stage_tails<D1, dev::kTailsNC>; }, grid(X.nlists, 4u * dev::kRunDefault), 256,
                              s, A))
                   != hipSuccess)
            return e;
    }
    if ((e = launch_lists_enc_planned(W.stage, W.sptr, n, d1, d1 ? W.sst : nullptr, W.sbytes, C.bytes, W.noff, C.units, W.enc, s))
        != hipSuccess)
        return e;
    if ((e = launch(dev::k_app_segs, grid(n + 1u, 256), 256, s, A)) != hipSuccess)
        return e;
    if (units_cap != 0u && (e = launch_by(d1, [](auto D1) { return dev::k_app_offsets<D1>; }, grid(units_cap, 256), 256, s, A)) != hipSuccess)
        return e;
    // the stream is never longer than the old bytes plus the staged ones
    const uint64_t span = std::min(out_cap, X.in_bytes + C.bytes);
    return span != 0u ? launch(dev::k_app_stitch, grid(span, 4u * dev::kListsAppendTile), 256, s, A) : hipSuccess;
}

} // namespace tpf
