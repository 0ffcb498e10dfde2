// p4_lists_units.hip -- block-range reads of a resident index (p4_lists.h,
// DESIGN.md 4.10): tpf_lists_unit_last builds the SKIP TABLE of a delta-1 lists
// stream once (the last value of every unit), tpf_lists_range_units turns
// doc-id ranges into unit ranges with it, and tpf_p4ndec256v32_lists_units
// decodes unit ranges of selected lists into one dense output.  The decode
// follows the selective decode's virtual-unit scheme (p4_lists_select.hip):
// the selected unit ranges, laid end to end in selection order, are the
// virtual unit sequence; virtual unit v of selection k is source unit
// list_unit[sel[k]] + ufirst[k] + (v - vbase[k]).  With the table every unit
// is decodable alone -- its start is the last value of the unit before it --
// so delta-1 reads and decodes every selected block once, in the plain
// form's launches.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

// ---- the skip table ---------------------------------------------------------
struct UlArgs
{
    ListsIndex ix;             // (no unit directory, and the skip table is what is built)
    const ListsHdr * hdr;
    const uint32_t * rec;      // unit records (p4_lists.h)
    const uint32_t * ubase;    // first unit of every list
    const uint32_t * sums;     // block sums of phase A (tails 0)
    const uint32_t * run_pre;  // run scan of phase A's 64-unit runs
    const uint32_t * run_tile;
    uint32_t * pbase;          // prefix of the block sums at ubase[j], j < nlists
    uint32_t * tsum;           // sum of (v + 1) over list j's tail unit (lists with a tail only)
    uint32_t * unit_last;
    unsigned long long * err;
};

// pbase[j] = P(ubase[j]), P(x) = the sum of every block sum before unit x (mod
// 2^32): the base of phase A's 64-unit run plus at most 63 sums.  (A list that
// starts at nunits holds no unit: its entry is never read.)
__global__ __launch_bounds__(256) void k_ul_pbase(const UlArgs A)
{
    if (!lists_go(A.hdr, A.ix.nunits))
        return;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < A.ix.nlists; j += gsz)
    {
        const uint32_t x = A.ubase[j];
        uint32_t acc = 0u;
        if (x < A.ix.nunits)
        {
            acc = run_base(A.run_pre, A.run_tile, x / kSumRun);
            for (uint32_t q = x / kSumRun * kSumRun; q < x; ++q)
                acc += A.sums[q];
        }
        A.pbase[j] = acc;
    }
}

// The tails' sums: every wave owns kRunDefault consecutive LISTS through the
// tails driver (tail_units, p4_lists_dev.h), as k_lists_tails does; lane t
// holds list first + t's tail unit or nothing.  The decoded gaps are summed,
// not stored.
template <uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_ul_tails(const UlArgs A)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    const ListsIndex & X = A.ix;
    if (!lists_go(A.hdr, X.nunits))
        return;
    const WaveRun R = wave_run(X.in, X.in_bytes, kRunDefault, X.nlists);
    const uint32_t t = R.t;
    if (R.first >= X.nlists)
        return;
    const uint64_t j = R.first + t;
    const uint64_t p0 = t < R.n ? X.ptr[j] : 0ull;
    const uint64_t p1 = t < R.n ? X.ptr[j + 1u] : 0ull;
    const uint32_t cnt = static_cast<uint32_t>((p1 - p0) & 255u);
    const bool has = cnt != 0u;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0ull)
        return;
    const uint32_t u = has ? A.ubase[j] + static_cast<uint32_t>((p1 - p0) >> 8) : 0u;
    uint32_t sumv = 0u;
    tail_units<false, NC>(
        R, X.off, has, hasmask, u, cnt, slots[R.wv], scratch[R.wv], A.err, [] { return 0u; },
        [&](uint32_t jj, uint32_t cj, const TailVals & v) {
            uint32_t loc = 0u;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                loc += t + 64u * q < cj ? v.v[q] + 1u : 0u;
            const uint32_t sm = wave_sum(loc);
            sumv = t == jj ? sm : sumv;
        });
    if (has)
        A.tsum[j] = sumv;
}

// The write pass: every wave owns one of phase A's 64-unit runs, lane t unit
// first + t.  last(u) = start0[list] + P(u + 1) - P(ubase[list]) mod 2^32, a
// tail adding its own sum (phase A counts it 0); the list of every unit by
// run_ids (p4_lists_dev.h).
__global__ __launch_bounds__(256) void k_ul_write(const UlArgs A)
{
    if (!lists_go(A.hdr, A.ix.nunits))
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kSumRun;
    if (first >= A.ix.nunits)
        return;
    const uint32_t n = static_cast<uint32_t>(min_u64(kSumRun, A.ix.nunits - first));
    const bool valid = t < n;
    const uint64_t u = first + t;
    const uint32_t r = valid ? A.rec[u] : 0u;
    const uint32_t id = run_ids(r, A.ubase, A.ix.nlists, first, t);
    const uint32_t sv = valid ? A.sums[u] : 0u;
    const uint32_t p1 = run_base(A.run_pre, A.run_tile, first / kSumRun) + wave_incl_scan(sv);
    if (valid)
    {
        const uint32_t s0 = A.ix.start0 != nullptr ? A.ix.start0[id] : 0u;
        const uint32_t ts = (r & kRecTail) != 0u ? A.tsum[id] : 0u;
        A.unit_last[u] = s0 + p1 - A.pbase[id] + ts;
    }
}

// ---- doc-id ranges to unit ranges -----------------------------------------------
// One thread per query: two binary searches over the list's slice of the skip
// table.  Every index is checked against nlists / nunits before it is used.
__global__ __launch_bounds__(256) void k_range_units(const uint32_t * __restrict list_unit, const uint32_t * __restrict unit_last,
                                                      uint64_t nlists, uint64_t nunits, const uint32_t * __restrict qlist,
                                                      const uint32_t * __restrict qlo, const uint32_t * __restrict qhi, uint64_t nq,
                                                      uint32_t * __restrict ufirst, uint32_t * __restrict ucount,
                                                      unsigned long long * __restrict err)
{
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; k < nq; k += gsz)
    {
        const uint32_t j = qlist[k];
        const uint32_t lo = qlo[k], hi = qhi[k];
        uint32_t uf = 0u, uc = 0u;
        bool bad = j >= nlists;
        if (!bad)
        {
            const uint32_t ua = list_unit[j], ub = list_unit[j + 1u];
            bad = ub < ua || ub > nunits;
            if (!bad && lo <= hi && ua < ub)
            {
                // a: the first unit of [ua, ub) whose last value is >= lo
                uint32_t a = ua, x = ub;
                while (a < x)
                {
                    const uint32_t m = a + (x - a) / 2u;
                    if (unit_last[m] >= lo)
                        x = m;
                    else
                        a = m + 1u;
                }
                if (a < ub)
                {
                    // b: the first unit of [a, ub) whose last value is >= hi, or the list's last unit
                    uint32_t b = a;
                    x = ub;
                    while (b < x)
                    {
                        const uint32_t m = b + (x - b) / 2u;
                        if (unit_last[m] >= hi)
                            x = m;
                        else
                            b = m + 1u;
                    }
                    if (b == ub)
                        b = ub - 1u;
                    uf = a - ua;
                    uc = b - a + 1u;
                }
            }
        }
        ufirst[k] = uf;
        ucount[k] = uc;
        if (bad && err != nullptr)
            atomicMin(err, static_cast<unsigned long long>(k));
    }
}

// ---- the decode of unit ranges -------------------------------------------------
struct UnArgs
{
    ListsIndex ix;
    const uint32_t * sel;
    const uint32_t * ufirst;
    const uint32_t * ucount;
    uint64_t nsel;
    uint32_t * out;
    uint64_t out_values;
    uint64_t vcap;             // the host's cap on the virtual units: out_values / 256 + nsel
    const uint64_t * out_ptr;  // d_out_ptr (written by the heads pass)
    const SelHdr * hdr;
    const uint32_t * rec;      // records of the virtual units (p4_lists.h)
    const uint32_t * vbase;    // first virtual unit of every selection, nsel + 1
    unsigned long long * err;
};

// Plan: one thread per SELECTION -- the unit and value counts of its range for
// the two run scans, and the checks of everything the later passes index with
// (the values are checked here, never followed) -- and the records of the
// virtual units zeroed for the heads pass, up to the host's cap.  A range
// holds 256 values per unit, but n % 256 in the list's p4Enc32 tail unit.
// (k_sel_plan with the range arithmetic; the heads pass is k_sel_heads.)
__global__ __launch_bounds__(256) void k_un_plan(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                                  uint64_t nunits, const uint32_t * __restrict sel, const uint32_t * __restrict ufirst,
                                                  const uint32_t * __restrict ucount, uint64_t nsel, uint32_t * __restrict totu,
                                                  uint64_t * __restrict totv, SelHdr * __restrict hdr, uint32_t * __restrict rec,
                                                  uint64_t vcap)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t k = gid; k < nsel; k += gsz)
    {
        const uint64_t uf = ufirst[k], uc = ucount[k];
        uint64_t n, nv = 0u;
        uint32_t ua, ub;
        bool bad = !list_dir_ok(ptr, list_unit, nlists, nunits, sel[k], &n, &ua, &ub);
        if (!bad)
        {
            const uint32_t units = ub - ua;
            bad = uf + uc > units; // 64-bit: the sum cannot wrap
            if (!bad)
            {
                const uint32_t r = static_cast<uint32_t>(n & 255u);
                nv = 256u * uc - ((uc != 0u && uf + uc == units && r != 0u) ? 256u - r : 0u);
            }
        }
        totu[k] = bad ? 0u : static_cast<uint32_t>(uc);
        totv[k] = bad ? 0ull : nv;
        if (bad)
            atomicMin(&hdr->bad, static_cast<unsigned long long>(k));
    }
    for (uint64_t u = gid; u < vcap; u += gsz)
        rec[u] = 0u;
}

// Full blocks: every wave owns a run of kRunDefault consecutive VIRTUAL units
// with the k_dec256v32w pipeline, as k_sel_dec does.  Lane t resolves the
// selection k of virtual unit first + t from the head records inside the run
// and one search over vbase for the run's first unit, gathers sel[k],
// ufirst[k] and list_unit[sel[k]] and loads the offsets of its SOURCE unit.
// Delta-1: the start of source unit su is one more gather (unit_start,
// p4_lists_dev.h), settled with the output plane's gathers before the chunks
// go in flight.  The output of a run is one contiguous range: one buffer
// descriptor, stores past it dropped.
template <bool D1, uint32_t NC, int MINW>
__global__ __launch_bounds__(256, MINW) void k_un_dec(const UnArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    // the run's source units, for the error report only (k_sel_dec: held in a
    // register across the pipeline they cost spilled VGPRs at 7 waves)
    __shared__ uint32_t srcu[4][kRunDefault];
    const ListsIndex & X = A.ix;
    if (!sel_go(A.hdr, A.out_values, A.vcap))
        return;
    constexpr uint32_t kRun = kRunDefault;
    const uint64_t vt = A.hdr->vtotal;
    const WaveRun R = wave_run(X.in, X.in_bytes, kRun, vt);
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

    const uint32_t id = run_ids(r, A.vbase, A.nsel, first, t); // the selection of every unit
    const uint32_t vb = valid ? A.vbase[id] : 0u;
    const uint32_t lj = valid ? A.sel[id] : 0u;
    const uint32_t inl = static_cast<uint32_t>(v) - vb;          // unit v - vb of its range
    const uint32_t inu = (valid ? A.ufirst[id] : 0u) + inl;      // ... and unit inu of its list
    // the source unit: the plan checked sel[k] < nlists, ufirst + ucount <= units_j and list_unit[j] + units_j <= nunits
    const uint32_t su = full ? X.list_unit[lj] + inu : 0u;
    const uint64_t o = full ? X.off[su] : 0ull;
    const uint64_t e = full ? X.off[su + 1u] : 0ull;
    RunPlaneT<kSlotBytes, true> P;
    P.init(R.in_base, R.in_end, o, e, full);
    if (t < kRun)
        srcu[wv][t] = full ? su : 0xFFFFFFFFu;

    const RunOut O(A.out, (valid ? A.out_ptr[id] : 0ull) + 256ull * inl, fullmask);
    uint32_t startv = 0u;
    if constexpr (D1)
    {
        if (full)
            startv = unit_start(X.list_unit, X.start0, X.unit_last, lj, su);
    }
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);

    uint64_t badmask = 0u;
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((fullmask >> jj) & 1ull) == 0ull)
            return;
        u32x4 x;
        decode_full_unit<D1>(P, c, jj, slot, scr, rl(startv, jj), t, x, badmask);
        O.store(jj, t, x);
        wave_lds_sync();
    });
    report_bad_units(A.err, badmask, t < kRun ? srcu[wv][t] : 0xFFFFFFFFu, t);
}

// Tails: every wave owns kRunDefault consecutive SELECTIONS through the tails
// driver (tail_units, p4_lists_dev.h), as k_sel_tails does; lane t holds
// selection first + t's tail unit -- the last unit of its range, n % 256
// values at the end of the selection's output -- or nothing.  Delta-1: the
// tail starts from the last value of the unit before it, or from start0 in a
// tail-only list.
template <bool D1, uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_un_tails(const UnArgs A)
{
    __shared__ uint32_t slots[4][kListSlot / 4];
    __shared__ uint32_t scratch[4][kListScratchU32];
    const ListsIndex & X = A.ix;
    if (!sel_go(A.hdr, A.out_values, A.vcap))
        return;
    const WaveRun R = wave_run(X.in, X.in_bytes, kRunDefault, A.nsel);
    const uint32_t t = R.t;
    if (R.first >= A.nsel)
        return;
    const uint64_t k = R.first + t;
    const uint64_t p0 = t < R.n ? A.out_ptr[k] : 0ull;
    const uint64_t p1 = t < R.n ? A.out_ptr[k + 1u] : 0ull;
    const uint32_t cnt = static_cast<uint32_t>((p1 - p0) & 255u);
    const bool has = cnt != 0u;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0ull)
        return;
    const uint32_t lj = has ? A.sel[k] : 0u;
    const uint32_t inu = has ? A.ufirst[k] + A.ucount[k] - 1u : 0u; // the list's last unit (ucount >= 1)
    const uint32_t su = has ? X.list_unit[lj] + inu : 0u;
    const uint64_t opos = p1 - cnt;
    tail_units<D1, NC>(
        R, X.off, has, hasmask, su, cnt, slots[R.wv], scratch[R.wv], A.err,
        [&] { return D1 && has ? unit_start(X.list_unit, X.start0, X.unit_last, lj, su) : 0u; }, tail_store<true>(A.out, opos, t));
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
// Workspace of the skip-table build: header | run scan of the lists' unit
// counts | ubase (nlists + 1) | pbase (nlists) | tail sums (nlists) | unit
// records (nunits) | phase A (the chained decode's layout over nunits units),
// each 256-byte aligned.  Nothing in it is sized by the values.
struct UlWs
{
    dev::ListsHdr * hdr;
    RunScanWs<uint64_t> scan;
    uint32_t *ubase, *pbase, *tsum, *rec;
    uint8_t * chain;
    size_t bytes;

    UlWs(void * ws, uint64_t nunits, uint64_t nlists)
    {
        WsCarver c(ws);
        hdr = c.take<dev::ListsHdr>(1);
        scan = c.scan<uint64_t>(nlists);
        ubase = c.take<uint32_t>(nlists + 1u);
        pbase = c.take<uint32_t>(nlists);
        tsum = c.take<uint32_t>(nlists);
        rec = c.take<uint32_t>(nunits);
        chain = c.bytes<uint8_t>(d1chain_workspace(nunits));
        bytes = c.used;
    }
};

// Workspace of the units decode: the selection prefix (p4_lists_host.h) |
// records of the virtual units (vcap), each 256-byte aligned.
struct UnWs
{
    WsCarver c;
    SelPlanWs plan;
    uint32_t * rec;
    size_t bytes;

    UnWs(void * ws, uint64_t nsel, uint64_t vcap) : c(ws), plan(c, nsel)
    {
        rec = c.take<uint32_t>(vcap);
        bytes = c.used;
    }
};
} // namespace

size_t lists_unit_last_workspace(uint64_t nunits, uint64_t nlists) { return UlWs(nullptr, nunits, nlists).bytes; }

hipError_t launch_lists_unit_last(const ListsIndex & X, uint32_t * unit_last, void * ws, unsigned long long * err, hipStream_t s)
{
    const uint64_t nunits = X.nunits, nlists = X.nlists;
    if (nunits == 0 || nlists == 0)
        return hipSuccess;
    if (nunits > 0x7FFFFFFFull || nlists > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const UlWs W(ws, nunits, nlists);
    // no value array to hold the pointers against: only their order is checked
    hipError_t e = launch_lists_structure(X.ptr, nlists, ~0ull, nunits, W.hdr, W.scan, W.ubase, W.rec, err, s);
    if (e != hipSuccess)
        return e;
    ChainView cv;
    if ((e = launch_lists_sums(X, W.rec, W.hdr, W.chain, &cv, err, s)) != hipSuccess)
        return e;
    const dev::UlArgs A{.ix = X,
                        .hdr = W.hdr,
                        .rec = W.rec,
                        .ubase = W.ubase,
                        .sums = cv.sums,
                        .run_pre = cv.pre,
                        .run_tile = cv.tile,
                        .pbase = W.pbase,
                        .tsum = W.tsum,
                        .unit_last = unit_last,
                        .err = err};
    if ((e = launch(dev::k_ul_pbase, flat_grid(nlists, s), 256, s, A)) != hipSuccess)
        return e;
    if ((e = launch(dev::k_ul_tails<dev::kTailsNC>, wave_grid(nlists, dev::kRunDefault), 256, s, A)) != hipSuccess)
        return e;
    return launch(dev::k_ul_write, wave_grid(nunits, dev::kSumRun), 256, s, A);
}

hipError_t launch_lists_range_units(const uint32_t * list_unit, const uint32_t * unit_last, uint64_t nlists, uint64_t nunits,
                                    const uint32_t * qlist, const uint32_t * qlo, const uint32_t * qhi, uint64_t nq, uint32_t * ufirst,
                                    uint32_t * ucount, unsigned long long * err, hipStream_t s)
{
    if (nq == 0)
        return hipSuccess;
    return launch(dev::k_range_units, flat_grid(nq, s), 256, s, list_unit, unit_last, nlists, nunits, qlist, qlo, qhi, nq, ufirst, ucount, err);
}

size_t lists_units_workspace(uint64_t nsel, uint64_t out_values)
{
    return UnWs(nullptr, nsel, lists_select_unit_cap(nsel, out_values)).bytes;
}

hipError_t launch_lists_units(const ListsIndex & X, bool d1, const uint32_t * sel, const uint32_t * ufirst, const uint32_t * ucount,
                              uint64_t nsel, uint32_t * out, uint64_t out_values, uint64_t * out_ptr, void * ws, unsigned long long * err,
                              hipStream_t s)
{
    if (nsel == 0)
        return out_ptr ? fill_u32(out_ptr, 0u, 2, s) : hipSuccess;
    const uint64_t vcap = lists_select_unit_cap(nsel, out_values);
    if (nsel > 0x7FFFFFFFull || vcap > 0x7FFFFFFFull || X.nlists > 0x7FFFFFFFull || X.nunits > 0x7FFFFFFFull
        || (d1 && X.unit_last == nullptr))
        return hipErrorInvalidValue;
    const UnWs W(ws, nsel, vcap);
    const SelPlanWs & S = W.plan;
    hipError_t e = fill_u32(S.hdr, 0xFFFFFFFFu, 2, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch(dev::k_un_plan, flat_grid(std::max(nsel, vcap), s), 256, s, X.ptr, X.list_unit, X.nlists, X.nunits, sel, ufirst, ucount,
                    nsel, S.scanu.tot, S.totv, S.hdr, W.rec, vcap))
        != hipSuccess)
        return e;
    if ((e = launch_sel_heads(nsel, X.nunits, out_values, vcap, S.hdr, S.scanu, S.totv, S.prev, S.tilev, S.vbase, W.rec, out_ptr, err, s))
        != hipSuccess)
        return e;
    const dev::UnArgs A{.ix = X,
                        .sel = sel,
                        .ufirst = ufirst,
                        .ucount = ucount,
                        .nsel = nsel,
                        .out = out,
                        .out_values = out_values,
                        .vcap = vcap,
                        .out_ptr = out_ptr,
                        .hdr = S.hdr,
                        .rec = W.rec,
                        .vbase = S.vbase,
                        .err = err};
    // sized by the host's cap: waves past the real unit count exit
    if ((e = launch_by(d1, [](auto D1) { return dev::k_un_dec<D1, dev::kListsNC, dev::kListsMinW>; }, wave_grid(vcap, dev::kRunDefault), 256, s,
                       A))
        != hipSuccess)
        return e;
    return launch_by(d1, [](auto D1) { return dev::k_un_tails<D1, dev::kTailsNC>; }, wave_grid(nsel, dev::kRunDefault), 256, s, A);
}

} // namespace tpf
