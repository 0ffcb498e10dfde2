// p4_lists.hip -- tpf_p4ndec256v32_lists: many posting lists laid end to end,
// each an n-variant stream (n/256 256v32 blocks + an optional p4Enc32 tail),
// decoded in one submission with no host round trip (p4_lists.h, DESIGN.md
// 4.7).  The list structure (CSR pointers) is checked on the device; every
// kernel after the plan pass reads the go / no-go header first.
#include "p4_lists.h"

#include "p4_dec256v32.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

struct ListsArgs
{
    ListsIndex ix;             // (no unit directory and no skip table: the decode of a whole stream builds its own)
    uint32_t * out;
    const ListsHdr * hdr;
    const uint32_t * rec;      // unit records (p4_lists.h)
    const uint32_t * ubase;    // first unit of every list
    const uint32_t * pbase;    // delta-1: prefix of the block sums at ubase[j], j <= nlists
    const uint32_t * sums;     // delta-1: block sums of phase A (tails 0)
    const uint32_t * run_pre;  // delta-1: run scan of phase A's 64-unit runs
    const uint32_t * run_tile;
    unsigned long long * err;
};

// Plan: one thread per list -- its unit count for the run scan and the
// structure check -- and the unit records zeroed for the heads pass.
__global__ __launch_bounds__(256) void k_lists_plan(const uint64_t * __restrict ptr, uint64_t nlists, uint64_t out_values,
                                                     uint32_t * __restrict tot, ListsHdr * __restrict hdr, uint32_t * __restrict rec,
                                                     uint64_t nunits)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = gid; j < nlists; j += gsz)
    {
        const uint64_t a = ptr[j], b = ptr[j + 1u];
        const bool bad = b < a || b > out_values;
        tot[j] = bad ? 0u : list_units(b - a);
        if (bad)
            atomicMin(&hdr->bad, static_cast<unsigned long long>(j));
    }
    for (uint64_t u = gid; u < nunits; u += gsz)
        rec[u] = 0u;
}

// Heads: the verdict (d_err for a refused structure), then per list its unit
// base and the records of its first unit and of its tail.
__global__ __launch_bounds__(256) void k_lists_heads(const uint64_t * __restrict ptr, uint64_t nlists, uint64_t nunits,
                                                      const uint64_t * __restrict pre, const uint64_t * __restrict tile,
                                                      const ListsHdr * __restrict hdr, uint32_t * __restrict ubase,
                                                      uint32_t * __restrict rec, unsigned long long * __restrict err)
{
    const bool go = lists_go(hdr, nunits);
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (!go)
    {
        if (gid == 0 && err != nullptr)
            *err = hdr->bad != ~0ull ? nunits + hdr->bad : nunits + nlists;
        return;
    }
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = gid; j < nlists; j += gsz)
    {
        const uint32_t ub = static_cast<uint32_t>(run_base(pre, tile, j)); // <= nunits < 2^31
        ubase[j] = ub;
        const uint64_t n = ptr[j + 1u] - ptr[j];
        const uint32_t units = list_units(n);
        const bool tail = (n & 255u) != 0u;
        if (units == 1u)
            rec[ub] = static_cast<uint32_t>(j + 1u) | (tail ? kRecTail : 0u);
        else if (units != 0u)
        {
            rec[ub] = static_cast<uint32_t>(j + 1u);
            if (tail)
                rec[ub + units - 1u] = kRecTail;
        }
    }
    if (gid == 0)
        ubase[nlists] = static_cast<uint32_t>(nunits);
}

// Delta-1: pbase[j] = P(ubase[j]) for j = 0 .. nlists, P(x) = the sum of every
// block sum before unit x (mod 2^32; ubase[nlists] = nunits): the base of
// phase A's 64-unit run plus at most 64 sums.
__global__ __launch_bounds__(256) void k_lists_pbase(uint64_t nlists, uint64_t nunits, const uint32_t * __restrict ubase,
                                                      const uint32_t * __restrict sums, const uint32_t * __restrict run_pre,
                                                      const uint32_t * __restrict run_tile, const ListsHdr * __restrict hdr,
                                                      uint32_t * __restrict pbase)
{
    if (!lists_go(hdr, nunits))
        return;
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j <= nlists; j += gsz)
    {
        const uint32_t x = ubase[j];
        const uint32_t y = x < nunits ? x : static_cast<uint32_t>(nunits - 1u); // the last run exists; P(nunits) = P(nunits-1) + its sum
        uint32_t acc = run_base(run_pre, run_tile, y / kSumRun);
        for (uint32_t k = y / kSumRun * kSumRun; k < y; ++k)
            acc += sums[k];
        if (x >= nunits)
            acc += sums[y];
        pbase[j] = acc;
    }
}

// Decode of the full blocks: every wave owns a run of kRunDefault consecutive
// units with the k_dec256v32w pipeline (one 16-byte load per lane per unit, NC
// units in flight, no workgroup barrier).  Lane t holds unit first + t's
// offsets, start and output position; a tail unit is a lane with nothing to
// load that the run skips (k_lists_tails decodes it).  The output of a lists
// stream is dense, so a run's values are one contiguous range: they go
// through one buffer descriptor over that range, 16 bytes per lane at a
// position that is only 4-byte aligned.
template <bool D1, uint32_t NC, int MINW>
__global__ __launch_bounds__(256, MINW) void k_lists_dec(const ListsArgs A)
{
    __shared__ uint32_t slots[4][kSlotBytes / 4];
    __shared__ uint32_t scratch[4][kWaveScratchU32];
    const ListsIndex & X = A.ix;
    if (!lists_go(A.hdr, X.nunits))
        return;
    constexpr uint32_t kRun = kRunDefault;
    const WaveRun R = wave_run(X.in, X.in_bytes, kRun, X.nunits);
    const uint32_t t = R.t;
    const uint64_t first = R.first;
    if (first >= X.nunits)
        return;
    uint32_t * slot = slots[R.wv];
    uint32_t * scr = scratch[R.wv];
    const bool valid = t < R.n;
    const uint64_t u = first + t;
    const uint32_t r = valid ? A.rec[u] : 0u;
    const bool full = valid && (r & kRecTail) == 0u;
    const uint64_t fullmask = __ballot(full);
    if (fullmask == 0ull)
        return; // a run of tails only
    const uint64_t o = full ? X.off[u] : 0ull;
    const uint64_t e = full ? X.off[u + 1u] : 0ull;
    RunPlaneT<kSlotBytes, true> P;
    P.init(R.in_base, R.in_end, o, e, full);
    // the first NC - 1 units' bytes go in flight before the list plane's
    // dependent gathers (rec -> list -> ubase / ptr / start0), which then
    // overlap them: a wave lives for 16 units only
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);

    const uint32_t id = run_ids(r, A.ubase, X.nlists, first, t); // the list of every unit
    const uint32_t ub = valid ? A.ubase[id] : 0u;
    const uint64_t p0 = valid ? X.ptr[id] : 0ull;
    const RunOut O(A.out, p0 + 256ull * (static_cast<uint32_t>(u) - ub), fullmask); // unit u - ub of its list

    uint32_t startv = 0u;
    if constexpr (D1)
    {
        // start0[list] + P(u) - P(ubase[list]) mod 2^32, P = the prefix of the
        // block sums over the whole stream (tails count 0); P(u) as the chained
        // decode's phase B rebuilds it from phase A's 64-unit runs
        static_assert(kSumRun % kRun == 0u, "decode runs nest in phase A's runs");
        const uint64_t f = first / kSumRun * kSumRun;
        const uint32_t kk = static_cast<uint32_t>(first - f);
        const uint32_t sv = f + t < X.nunits ? A.sums[f + t] : 0u;
        const uint32_t ex = wave_incl_scan(sv) - sv;
        const uint32_t pu = run_base(A.run_pre, A.run_tile, first / kSumRun)
                            + static_cast<uint32_t>(__shfl(static_cast<int>(ex), static_cast<int>((kk + t) & 63u), 64));
        const uint32_t s0 = (valid && X.start0 != nullptr) ? X.start0[id] : 0u;
        startv = valid ? s0 + pu - A.pbase[id] : 0u;
    }

    uint64_t badmask = 0u;
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((fullmask >> jj) & 1ull) == 0ull)
            return;
        u32x4 v;
        decode_full_unit<D1>(P, c, jj, slot, scr, rl(startv, jj), t, v, badmask);
        O.store(jj, t, v);
        wave_lds_sync();
    });
    report_bad_units(A.err, badmask, static_cast<uint32_t>(u), t);
}

// Decode of the tails: every wave owns kRunDefault consecutive LISTS through
// the tails driver (tail_units, p4_lists_dev.h); lane t holds list
// first + t's tail unit -- unit ubase + n / 256 of n % 256 values at the end
// of the list's output -- or nothing when the list has no tail.  Delta-1: the
// tail starts at start0 + P(ubase[j + 1]) - P(ubase[j]), every full block of
// its list (the tail is the list's last unit and its own sum counts 0).
// (Tails as a wave-uniform branch inside k_lists_dec spilled 12-24 VGPRs at 6
// and 7 waves per SIMD: decode_block_g beside the six chunks in flight.)
template <bool D1, uint32_t NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_lists_tails(const ListsArgs A)
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
    const uint64_t opos = p1 - cnt;
    tail_units<D1, NC>(
        R, X.off, has, hasmask, u, cnt, slots[R.wv], scratch[R.wv], A.err,
        [&] { return D1 && has ? (X.start0 != nullptr ? X.start0[j] : 0u) + A.pbase[j + 1u] - A.pbase[j] : 0u; },
        tail_store<true>(A.out, opos, t));
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
// Workspace: header | run scan of the lists' unit counts | ubase (nlists + 1)
// | pbase (nlists + 1) | unit records (nunits) | phase A (the chained decode's
// layout over nunits units), each 256-byte aligned.
struct ListsWs
{
    dev::ListsHdr * hdr;
    RunScanWs<uint64_t> scan;
    uint32_t *ubase, *pbase, *rec;
    uint8_t * chain;
    size_t bytes;

    ListsWs(void * ws, uint64_t nunits, uint64_t nlists)
    {
        WsCarver c(ws);
        hdr = c.take<dev::ListsHdr>(1);
        scan = c.scan<uint64_t>(nlists);
        ubase = c.take<uint32_t>(nlists + 1u);
        pbase = c.take<uint32_t>(nlists + 1u);
        rec = c.take<uint32_t>(nunits);
        chain = c.bytes<uint8_t>(d1chain_workspace(nunits));
        bytes = c.used;
    }
};
} // namespace

size_t lists_workspace(uint64_t nunits, uint64_t nlists) { return ListsWs(nullptr, nunits, nlists).bytes; }

hipError_t launch_lists_structure(const uint64_t * ptr, uint64_t nlists, uint64_t values, uint64_t nunits, dev::ListsHdr * hdr,
                                  const RunScanWs<uint64_t> & scan, uint32_t * ubase, uint32_t * rec, unsigned long long * err,
                                  hipStream_t s)
{
    hipError_t e = fill_u32(hdr, 0xFFFFFFFFu, 4, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch(dev::k_lists_plan, flat_grid(std::max(nunits, nlists), s), 256, s, ptr, nlists, values, scan.tot, hdr, rec, nunits))
        != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64(scan.tot, nlists, scan.pre, scan.tile, reinterpret_cast<uint64_t *>(&hdr->total), s)) != hipSuccess)
        return e;
    return launch(dev::k_lists_heads, flat_grid(nlists, s), 256, s, ptr, nlists, nunits, scan.pre, scan.tile, hdr, ubase, rec, err);
}

hipError_t launch_lists_dec(const ListsIndex & X, bool d1, uint32_t * out, uint64_t out_values, void * ws, unsigned long long * err,
                            hipStream_t s)
{
    const uint64_t nunits = X.nunits, nlists = X.nlists;
    if (nunits == 0 || nlists == 0)
        return hipSuccess;
    if (nunits > 0x7FFFFFFFull || nlists > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const ListsWs W(ws, nunits, nlists);
    hipError_t e = launch_lists_structure(X.ptr, nlists, out_values, nunits, W.hdr, W.scan, W.ubase, W.rec, err, s);
    if (e != hipSuccess)
        return e;
    dev::ListsArgs A{.ix = X, .out = out, .hdr = W.hdr, .rec = W.rec, .ubase = W.ubase, .pbase = W.pbase, .err = err};
    if (d1)
    {
        // phase A keeps the first parse error of a full block; the decode pass
        // re-checks every unit (tails included) into the same word
        ChainView cv;
        if ((e = launch_lists_sums(X, W.rec, W.hdr, W.chain, &cv, err, s)) != hipSuccess)
            return e;
        A.sums = cv.sums;
        A.run_pre = cv.pre;
        A.run_tile = cv.tile;
        if ((e = launch(dev::k_lists_pbase, flat_grid(nlists + 1u, s), 256, s, nlists, nunits, W.ubase, cv.sums, cv.pre, cv.tile, W.hdr, W.pbase))
            != hipSuccess)
            return e;
    }
    if ((e = launch_by(d1, [](auto D1) { return dev::k_lists_dec<D1, dev::kListsNC, dev::kListsMinW>; },
                       wave_grid(nunits, dev::kRunDefault), 256, s, A))
        != hipSuccess)
        return e;
    return launch_by(d1, [](auto D1) { return dev::k_lists_tails<D1, dev::kTailsNC>; }, wave_grid(nlists, dev::kRunDefault), 256, s, A);
}

} // namespace tpf
