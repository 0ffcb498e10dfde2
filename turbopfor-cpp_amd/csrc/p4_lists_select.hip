// p4_lists_select.hip -- the read side of a resident index (p4_lists.h,
// DESIGN.md 4.9): tpf_lists_unit_base builds the unit directory of a lists
// stream once, tpf_p4ndec256v32_lists_select decodes lists sel[0 .. nsel) of
// it, in the order given, into one dense output.  The selection takes the
// role the index's lists play in p4_lists.hip: the selected lists' units,
// laid end to end in selection order, are the VIRTUAL unit sequence every pass
// after the plan works on; virtual unit v of selection k is source unit
// list_unit[sel[k]] + (v - vbase[k]) of the stream.  No pass is sized by the
// index, and none reads it at a list or unit that is not selected.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

struct SelArgs
{
    ListsIndex ix;             // (no skip table: delta-1 sums the selected blocks)
    const uint32_t * sel;
    uint64_t nsel;
    uint32_t * out;
    uint64_t out_values;
    uint64_t vcap;             // the host's cap on the virtual units: out_values / 256 + nsel
    const uint64_t * out_ptr;  // d_out_ptr (written by the heads pass)
    const SelHdr * hdr;
    const uint32_t * rec;      // records of the virtual units (p4_lists.h)
    const uint32_t * vbase;    // first virtual unit of every selection, nsel + 1
    const uint32_t * pbase;    // delta-1: prefix of the block sums at vbase[k], k <= nsel
    uint32_t * sums;           // delta-1: block sums of the virtual units (tails 0)
    uint32_t * run_tot;        // delta-1: one total per 16-unit decode run
    const uint32_t * run_pre;
    const uint32_t * run_tile;
    unsigned long long * err;
};

// ---- the unit directory ---------------------------------------------------
__global__ __launch_bounds__(256) void k_unit_base_plan(const uint64_t * __restrict ptr, uint64_t nlists, uint32_t * __restrict tot,
                                                         unsigned long long * __restrict bad)
{
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < nlists; j += gsz)
    {
        const uint64_t a = ptr[j], b = ptr[j + 1u];
        tot[j] = b < a ? 0u : list_units(b - a);
        if (b < a)
            atomicMin(bad, static_cast<unsigned long long>(j));
    }
}

// hdr[0]: first decreasing pointer, hdr[1]: the unit total
__global__ __launch_bounds__(256) void k_unit_base_write(uint64_t nlists, const uint64_t * __restrict pre, const uint64_t * __restrict tile,
                                                          const unsigned long long * __restrict hdr, uint32_t * __restrict list_unit,
                                                          unsigned long long * __restrict err)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const unsigned long long bad = hdr[0], total = hdr[1];
    if (bad != ~0ull || total > 0x7FFFFFFFull)
    {
        if (gid == 0 && err != nullptr)
            *err = bad != ~0ull ? bad : nlists;
        return;
    }
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = gid; j < nlists; j += gsz)
        list_unit[j] = static_cast<uint32_t>(run_base(pre, tile, j));
    if (gid == 0)
        list_unit[nlists] = static_cast<uint32_t>(total);
}

// ---- the selective decode ---------------------------------------------------
// Plan: one thread per SELECTION -- its list's unit and value counts for the
// two run scans, and the checks of everything the later passes index with
// (the values are checked here, never followed) -- and the records of the
// virtual units zeroed for the heads pass, up to the host's cap.
__global__ __launch_bounds__(256) void k_sel_plan(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                                   uint64_t nunits, const uint32_t * __restrict sel, uint64_t nsel,
                                                   uint32_t * __restrict totu, uint64_t * __restrict totv, SelHdr * __restrict hdr,
                                                   uint32_t * __restrict rec, uint64_t vcap)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t k = gid; k < nsel; k += gsz)
    {
        uint64_t n;
        uint32_t ua, ub;
        const bool bad = !list_dir_ok(ptr, list_unit, nlists, nunits, sel[k], &n, &ua, &ub);
        totu[k] = bad ? 0u : ub - ua;
        totv[k] = bad ? 0ull : n;
        if (bad)
            atomicMin(&hdr->bad, static_cast<unsigned long long>(k));
    }
    for (uint64_t u = gid; u < vcap; u += gsz)
        rec[u] = 0u;
}

// Heads (the selective decode and the units decode): the verdict (d_err for a
// refused selection or an output that is too small), d_out_ptr, then per
// selection its virtual unit base and the records of its first unit and of its
// tail -- the head carries k + 1, the SELECTION.  A selection has a tail to
// decode exactly when its value count is no multiple of 256: it reaches the
// list's last unit and that unit is a p4Enc32 tail.
__global__ __launch_bounds__(256) void k_sel_heads(uint64_t nsel, uint64_t nunits, uint64_t out_values, uint64_t vcap,
                                                    const uint32_t * __restrict totu, const uint64_t * __restrict totv,
                                                    const uint64_t * __restrict preu, const uint64_t * __restrict tileu,
                                                    const uint64_t * __restrict prev, const uint64_t * __restrict tilev,
                                                    const SelHdr * __restrict hdr, uint32_t * __restrict vbase, uint32_t * __restrict rec,
                                                    uint64_t * __restrict out_ptr, unsigned long long * __restrict err)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    if (hdr->bad != ~0ull)
    {
        if (gid == 0 && err != nullptr)
            *err = nunits + hdr->bad;
        return;
    }
    const bool go = sel_go(hdr, out_values, vcap);
    for (uint64_t k = gid; k < nsel; k += gsz)
        out_ptr[k] = run_base(prev, tilev, k);
    if (gid == 0)
    {
        out_ptr[nsel] = hdr->ototal;
        if (!go && err != nullptr)
            *err = nunits + nsel;
    }
    if (!go)
        return;
    for (uint64_t k = gid; k < nsel; k += gsz)
    {
        const uint32_t vb = static_cast<uint32_t>(run_base(preu, tileu, k)); // <= vtotal <= vcap < 2^31
        vbase[k] = vb;
        const uint32_t units = totu[k];
        const bool tail = (totv[k] & 255u) != 0u;
        if (units == 1u)
            rec[vb] = static_cast<uint32_t>(k + 1u) | (tail ? kRecTail : 0u);
        else if (units != 0u)
        {
            rec[vb] = static_cast<uint32_t>(k + 1u);
            if (tail)
                rec[vb + units - 1u] = kRecTail;
        }
    }
    if (gid == 0)
        vbase[nsel] = static_cast<uint32_t>(hdr->vtotal);
}

// Delta-1: pbase[k] = P(vbase[k]) for k = 0 .. nsel, P(x) = the sum of every
// block sum before virtual unit x (mod 2^32; vbase[nsel] = vtotal): the base of
// the 16-unit run of the sums pass plus at most 16 sums.
__global__ __launch_bounds__(256) void k_sel_pbase(const SelArgs A, uint32_t * __restrict pbase)
{
    if (!sel_go(A.hdr, A.out_values, A.vcap))
        return;
    const uint64_t vt = A.hdr->vtotal;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; k <= A.nsel; k += gsz)
    {
        uint32_t acc = 0u;
        if (vt != 0u)
        {
            const uint32_t x = A.vbase[k];
            const uint32_t y = x < vt ? x : static_cast<uint32_t>(vt - 1u); // the last run exists; P(vtotal) = P(vtotal-1) + its sum
            acc = run_base(A.run_pre, A.run_tile, y / kRunDefault);
            for (uint32_t q = y / kRunDefault * kRunDefault; q < y; ++q)
                acc += A.sums[q];
            if (x >= vt)
                acc += A.sums[y];
        }
        pbase[k] = acc;
    }
}

// Full blocks: every wave owns a run of kRunDefault consecutive VIRTUAL units
// with the k_dec256v32w pipeline, as k_lists_dec does for the units of a
// stream.  Lane t resolves the selection k of virtual unit first + t from the
// head records inside the run and one search over vbase for the run's first
// unit, then gathers sel[k] and list_unit[sel[k]] and loads the offsets of its
// SOURCE unit; the blocks of a run lie anywhere in the stream, which the run
// plane never assumed otherwise.  The output of a run is still one contiguous
// range (the output is dense in selection order): one buffer descriptor.
// SUM (delta-1's first pass): the same decode, but every block's sum of
// (v + 1) goes to sums[] and the run's total to run_tot[] instead of the
// values to the output.  (The lists decode sums a contiguous stream through
// LDS windows of 16 KB, k_dsum256v32_lists; scattered source units have no
// such windows, so this pass pays a full decode per block.)
template <bool D1, uint32_t NC, int MINW, bool SUM>
__global__ __launch_bounds__(256, MINW) void k_sel_dec(const SelArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    // the run's source units, for the error report only: held in a register
    // across the pipeline they cost the delta-1 form 6 spilled VGPRs at 7 waves
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
    {
        // the grid is sized by the host's cap: a wave past the real count has
        // nothing to do but leave its run total defined for the scan
        if (SUM && t == 0 && first < A.vcap)
            A.run_tot[first / kRun] = 0u;
        return;
    }
    uint32_t * slot = slots[wv];
    uint32_t * scr = scratch[wv];
    const bool valid = t < R.n;
    const uint64_t v = first + t;
    const uint32_t r = valid ? A.rec[v] : 0u;
    const bool full = valid && (r & kRecTail) == 0u;
    const uint64_t fullmask = __ballot(full);
    if (fullmask == 0ull)
    {
        if constexpr (SUM)
        {
            if (valid)
                A.sums[v] = 0u;
            if (t == 0)
                A.run_tot[first / kRun] = 0u;
        }
        return; // a run of tails only
    }

    const uint32_t id = run_ids(r, A.vbase, A.nsel, first, t); // the selection of every unit
    const uint32_t vb = valid ? A.vbase[id] : 0u;
    const uint32_t lj = valid ? A.sel[id] : 0u;
    const uint32_t inl = static_cast<uint32_t>(v) - vb; // unit v - vb of its list
    // the source unit: the plan checked sel[k] < nlists and list_unit[j] + units_j <= nunits
    const uint32_t su = full ? X.list_unit[lj] + inl : 0u;
    const uint64_t o = full ? X.off[su] : 0ull;
    const uint64_t e = full ? X.off[su + 1u] : 0ull;
    RunPlaneT<kSlotBytes, true> P;
    P.init(R.in_base, R.in_end, o, e, full);
    if (!SUM && t < kRun)
        srcu[wv][t] = full ? su : 0xFFFFFFFFu;

    // (the output plane's gathers depend on the selection only, like the
    // offsets': they are settled before the chunks go in flight, which keeps
    // the delta-1 form inside the registers of 7 waves per SIMD)
    uint32_t startv = 0u, sumv = 0u;
    RunOut O;
    if constexpr (!SUM)
    {
        O = RunOut(A.out, (valid ? A.out_ptr[id] : 0ull) + 256ull * inl, fullmask);
        if constexpr (D1)
        {
            // start0[list] + P(v) - P(vbase[k]) mod 2^32, P = the prefix of the
            // block sums over the virtual units (tails count 0)
            const uint32_t sv = valid ? A.sums[v] : 0u;
            const uint32_t pu = run_base(A.run_pre, A.run_tile, first / kRun) + wave_incl_scan(sv) - sv;
            const uint32_t s0 = (valid && X.start0 != nullptr) ? X.start0[lj] : 0u;
            startv = valid ? s0 + pu - A.pbase[id] : 0u;
        }
    }
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);

    uint64_t badmask = 0u;
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((fullmask >> jj) & 1ull) == 0ull)
            return;
        u32x4 x;
        decode_full_unit<D1 && !SUM>(P, c, jj, slot, scr, rl(startv, jj), t, x, badmask);
        if constexpr (SUM)
        {
            const uint32_t sm = wave_sum(x.x + x.y + x.z + x.w + 4u);
            sumv = t == jj ? sm : sumv;
        }
        else
            O.store(jj, t, x);
        wave_lds_sync();
    });
    if constexpr (SUM)
    {
        // the decode pass re-checks every unit: parse errors are reported there
        sumv = full ? sumv : 0u;
        if (valid)
            A.sums[v] = sumv;
        publish_run_total(A.run_tot, first / kRun, sumv, t);
    }
    else
        report_bad_units(A.err, badmask, t < kRun ? srcu[wv][t] : 0xFFFFFFFFu, t);
}

// Tails: every wave owns kRunDefault consecutive SELECTIONS through the tails
// driver (tail_units, p4_lists_dev.h), as k_lists_tails does for the lists of
// a stream; lane t holds selection first + t's tail unit -- source unit
// list_unit[sel[k]] + n / 256 of n % 256 values at the end of the selection's
// output -- or nothing.  Delta-1: the tail starts at start0 + P(vbase[k + 1])
// - P(vbase[k]).
// (A kernel of its own for the reason recorded above k_lists_tails.)
template <bool D1, uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_sel_tails(const SelArgs A)
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
    const uint32_t su = has ? X.list_unit[lj] + static_cast<uint32_t>((p1 - p0) >> 8) : 0u;
    const uint64_t opos = p1 - cnt;
    tail_units<D1, NC>(
        R, X.off, has, hasmask, su, cnt, slots[R.wv], scratch[R.wv], A.err,
        [&] { return D1 && has ? (X.start0 != nullptr ? X.start0[lj] : 0u) + A.pbase[k + 1u] - A.pbase[k] : 0u; },
        tail_store<true>(A.out, opos, t));
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
uint64_t sel_runs(uint64_t vcap) { return (vcap + dev::kRunDefault - 1u) / dev::kRunDefault; }

// Workspace of the selective decode: the selection prefix (p4_lists_host.h) |
// pbase (nsel + 1) | records of the virtual units (vcap) | block sums (vcap)
// and the scan of their 16-unit run totals, each 256-byte aligned.
struct SelWs
{
    WsCarver c;
    SelPlanWs plan;
    uint32_t *pbase, *rec, *sums;
    RunScanWs<uint32_t> scans;
    size_t bytes;

    SelWs(void * ws, uint64_t nsel, uint64_t vcap) : c(ws), plan(c, nsel)
    {
        pbase = c.take<uint32_t>(nsel + 1u);
        rec = c.take<uint32_t>(vcap);
        sums = c.take<uint32_t>(vcap);
        scans = c.scan<uint32_t>(sel_runs(vcap));
        bytes = c.used;
    }
};
} // namespace

size_t lists_unit_base_workspace(uint64_t nlists) { return 256u + al256(RunScanWs<uint64_t>::bytes(nlists)); }

hipError_t launch_lists_unit_base(const uint64_t * ptr, uint64_t nlists, uint32_t * list_unit, void * ws, unsigned long long * err,
                                  hipStream_t s)
{
    if (nlists == 0)
        return fill_u32(list_unit, 0u, 1, s);
    auto * hdr = static_cast<unsigned long long *>(ws);
    const RunScanWs<uint64_t> scan = RunScanWs<uint64_t>::carve(static_cast<uint8_t *>(ws) + 256u, nlists);
    hipError_t e = fill_u32(hdr, 0xFFFFFFFFu, 4, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch(dev::k_unit_base_plan, flat_grid(nlists, s), 256, s, ptr, nlists, scan.tot, hdr)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64(scan.tot, nlists, scan.pre, scan.tile, reinterpret_cast<uint64_t *>(hdr + 1), s)) != hipSuccess)
        return e;
    return launch(dev::k_unit_base_write, flat_grid(nlists, s), 256, s, nlists, scan.pre, scan.tile, hdr, list_unit, err);
}

uint64_t lists_select_unit_cap(uint64_t nsel, uint64_t out_values) { return out_values / 256u + nsel; }

size_t lists_select_workspace(uint64_t nsel, uint64_t out_values)
{
    return SelWs(nullptr, nsel, lists_select_unit_cap(nsel, out_values)).bytes;
}

hipError_t launch_sel_heads(uint64_t nsel, uint64_t nunits, uint64_t out_values, uint64_t vcap, dev::SelHdr * hdr,
                            const RunScanWs<uint64_t> & scanu, const uint64_t * totv, uint64_t * prev, uint64_t * tilev, uint32_t * vbase,
                            uint32_t * rec, uint64_t * out_ptr, unsigned long long * err, hipStream_t s)
{
    hipError_t e;
    if ((e = launch_run_scan_u64(scanu.tot, nsel, scanu.pre, scanu.tile, reinterpret_cast<uint64_t *>(&hdr->vtotal), s)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64t(totv, nsel, prev, tilev, reinterpret_cast<uint64_t *>(&hdr->ototal), s)) != hipSuccess)
        return e;
    return launch(dev::k_sel_heads, flat_grid(nsel, s), 256, s, nsel, nunits, out_values, vcap, scanu.tot, totv, scanu.pre, scanu.tile, prev,
                  tilev, hdr, vbase, rec, out_ptr, err);
}

hipError_t launch_lists_select(const ListsIndex & X, bool d1, const uint32_t * sel, uint64_t nsel, uint32_t * out, uint64_t out_values,
                               uint64_t * out_ptr, void * ws, unsigned long long * err, hipStream_t s)
{
    if (nsel == 0)
        return out_ptr ? fill_u32(out_ptr, 0u, 2, s) : hipSuccess;
    const uint64_t vcap = lists_select_unit_cap(nsel, out_values);
    if (nsel > 0x7FFFFFFFull || vcap > 0x7FFFFFFFull || X.nlists > 0x7FFFFFFFull || X.nunits > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const SelWs W(ws, nsel, vcap);
    const SelPlanWs & S = W.plan;
    hipError_t e = fill_u32(S.hdr, 0xFFFFFFFFu, 2, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch(dev::k_sel_plan, flat_grid(std::max(nsel, vcap), s), 256, s, X.ptr, X.list_unit, X.nlists, X.nunits, sel, nsel, S.scanu.tot,
                    S.totv, S.hdr, W.rec, vcap))
        != hipSuccess)
        return e;
    if ((e = launch_sel_heads(nsel, X.nunits, out_values, vcap, S.hdr, S.scanu, S.totv, S.prev, S.tilev, S.vbase, W.rec, out_ptr, err, s))
        != hipSuccess)
        return e;
    const dev::SelArgs A{.ix = X,
                         .sel = sel,
                         .nsel = nsel,
                         .out = out,
                         .out_values = out_values,
                         .vcap = vcap,
                         .out_ptr = out_ptr,
                         .hdr = S.hdr,
                         .rec = W.rec,
                         .vbase = S.vbase,
                         .pbase = W.pbase,
                         .sums = W.sums,
                         .run_tot = W.scans.tot,
                         .run_pre = W.scans.pre,
                         .run_tile = W.scans.tile,
                         .err = err};
    // sized by the host's cap: waves past the real unit count exit
    const uint32_t grid = wave_grid(vcap, dev::kRunDefault), tgrid = wave_grid(nsel, dev::kRunDefault);
    if (d1)
    {
        // the block sums of the virtual units, their run scan, one prefix per selection
        if ((e = launch(dev::k_sel_dec<false, dev::kListsNC, dev::kListsMinW, true>, grid, 256, s, A)) != hipSuccess)
            return e;
        if ((e = launch_run_scan_u32(W.scans.tot, sel_runs(vcap), W.scans.pre, W.scans.tile, nullptr, s)) != hipSuccess)
            return e;
        if ((e = launch(dev::k_sel_pbase, flat_grid(nsel + 1u, s), 256, s, A, W.pbase)) != hipSuccess)
            return e;
    }
    if ((e = launch_by(d1, [](auto D1) { return dev::k_sel_dec<D1, dev::kListsNC, dev::kListsMinW, false>; }, grid, 256, s, A)) != hipSuccess)
        return e;
    return launch_by(d1, [](auto D1) { return dev::k_sel_tails<D1, dev::kTailsNC>; }, tgrid, 256, s, A);
}

} // namespace tpf
