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
    const uint8_t * in;
    uint64_t in_bytes;
    const uint64_t * off;
    uint64_t nunits;
    const uint64_t * ptr;
    uint64_t nlists;
    const uint32_t * start0;
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
    if (!lists_go(A.hdr, A.nunits))
        return;
    constexpr uint32_t kRun = kRunDefault;
    const WaveRun R = wave_run(A.in, A.in_bytes, kRun, A.nunits);
    const uint32_t t = R.t;
    const uint64_t first = R.first;
    if (first >= A.nunits)
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
    const uint64_t o = full ? A.off[u] : 0ull;
    const uint64_t e = full ? A.off[u + 1u] : 0ull;
    RunPlaneT<kSlotBytes, true> P;
    P.init(R.in_base, R.in_end, o, e, full);
    // the first NC - 1 units' bytes go in flight before the list plane's
    // dependent gathers (rec -> list -> ubase / ptr / start0), which then
    // overlap them: a wave lives for 16 units only
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);

    // ---- the list of every unit: heads inside the run, the search before it
    const uint32_t r0 = rl(r, 0) & kRecList;
    const uint32_t j0 = r0 != 0u ? r0 - 1u : find_list(A.ubase, static_cast<uint32_t>(A.nlists), static_cast<uint32_t>(first), t);
    const uint32_t id = umax32(wave_incl_max(r & kRecList), j0 + 1u) - 1u;
    const uint32_t ub = valid ? A.ubase[id] : 0u;
    const uint64_t p0 = valid ? A.ptr[id] : 0ull;
    const uint64_t opos = p0 + 256ull * (static_cast<uint32_t>(u) - ub); // unit u - ub of its list
    const uint64_t opos0 = readlane_u64(opos, 0);
    const uint32_t rel = static_cast<uint32_t>(opos - opos0) * 4u; // bytes from the run's first value
    const uint32_t lastf = 63u - static_cast<uint32_t>(__builtin_clzll(fullmask));
    const __amdgpu_buffer_rsrc_t ors = make_rsrc(A.out + opos0, rl(rel, lastf) + 1024u);

    uint32_t startv = 0u;
    if constexpr (D1)
    {
        // start0[list] + P(u) - P(ubase[list]) mod 2^32, P = the prefix of the
        // block sums over the whole stream (tails count 0); P(u) as the chained
        // decode's phase B rebuilds it from phase A's 64-unit runs
        static_assert(kSumRun % kRun == 0u, "decode runs nest in phase A's runs");
        const uint64_t f = first / kSumRun * kSumRun;
        const uint32_t kk = static_cast<uint32_t>(first - f);
        const uint32_t sv = f + t < A.nunits ? A.sums[f + t] : 0u;
        const uint32_t ex = wave_incl_scan(sv) - sv;
        const uint32_t pu = run_base(A.run_pre, A.run_tile, first / kSumRun)
                            + static_cast<uint32_t>(__shfl(static_cast<int>(ex), static_cast<int>((kk + t) & 63u), 64));
        const uint32_t s0 = (valid && A.start0 != nullptr) ? A.start0[id] : 0u;
        startv = valid ? s0 + pu - A.pbase[id] : 0u;
    }

    uint64_t badmask = 0u;
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((fullmask >> jj) & 1ull) == 0ull)
            return;
        u32x4 v;
        decode_full_unit<D1>(P, c, jj, slot, scr, rl(startv, jj), t, v, badmask);
        st16_run(ors, rl(rel, jj) + 16u * t, v);
        wave_lds_sync();
    });
    report_bad_units(A.err, badmask, static_cast<uint32_t>(u), t);
}

// Decode of the tails: every wave owns kRunDefault consecutive LISTS with the
// generic decoder's pipeline (k_dec_gr, p4_generic.hip); lane t holds list
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
    if (!lists_go(A.hdr, A.nunits))
        return;
    const WaveRun R = wave_run(A.in, A.in_bytes, kRunDefault, A.nlists);
    const uint32_t t = R.t;
    if (R.first >= A.nlists)
        return;
    uint32_t * slot = slots[R.wv];
    const uint64_t j = R.first + t;
    const uint64_t p0 = t < R.n ? A.ptr[j] : 0ull;
    const uint64_t p1 = t < R.n ? A.ptr[j + 1u] : 0ull;
    const uint32_t cnt = static_cast<uint32_t>((p1 - p0) & 255u);
    const bool has = cnt != 0u;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0ull)
        return;
    const uint32_t u = has ? A.ubase[j] + static_cast<uint32_t>((p1 - p0) >> 8) : 0u;
    const uint64_t o = has ? A.off[u] : 0ull;
    const uint64_t e = has ? A.off[u + 1u] : 0ull;
    RunPlaneT<kListSlot> P;
    P.init(R.in_base, R.in_end, o, e, has);
    const uint64_t opos = p1 - cnt;
    uint32_t startv = 0u;
    if constexpr (D1)
        startv = has ? (A.start0 != nullptr ? A.start0[j] : 0u) + A.pbase[j + 1u] - A.pbase[j] : 0u;
    uint64_t badmask = 0u;
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((hasmask >> jj) & 1ull) == 0ull)
            return;
        const uint32_t cj = rl(cnt, jj);
        TailVals v;
        decode_tail_unit<D1>(P, c, jj, slot, scratch[R.wv], cj, rl(startv, jj), t, v, badmask);
        uint32_t * op = A.out + readlane_u64(opos, jj);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (t + 64u * q < cj)
                __builtin_nontemporal_store(v.v[q], op + t + 64u * q);
        wave_lds_sync();
    });
    report_bad_units(A.err, badmask, u, t);
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
    hipLaunchKernelGGL(dev::k_lists_plan, dim3(flat_grid(std::max(nunits, nlists), s)), dim3(256), 0, s, ptr, nlists, values, scan.tot,
                       hdr, rec, nunits);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64(scan.tot, nlists, scan.pre, scan.tile, reinterpret_cast<uint64_t *>(&hdr->total), s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::k_lists_heads, dim3(flat_grid(nlists, s)), dim3(256), 0, s, ptr, nlists, nunits, scan.pre, scan.tile, hdr,
                       ubase, rec, err);
    return hipGetLastError();
}

hipError_t launch_lists_dec(const uint8_t * in, uint64_t in_bytes, const uint64_t * off, uint64_t nunits, const uint64_t * ptr,
                            uint64_t nlists, bool d1, const uint32_t * start0, uint32_t * out, uint64_t out_values, void * ws,
                            unsigned long long * err, hipStream_t s)
{
    if (nunits == 0 || nlists == 0)
        return hipSuccess;
    if (nunits > 0x7FFFFFFFull || nlists > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const ListsWs W(ws, nunits, nlists);
    hipError_t e = launch_lists_structure(ptr, nlists, out_values, nunits, W.hdr, W.scan, W.ubase, W.rec, err, s);
    if (e != hipSuccess)
        return e;
    dev::ListsArgs A{in, in_bytes, off, nunits, ptr, nlists, start0, out, W.hdr, W.rec, W.ubase, W.pbase,
                     nullptr, nullptr, nullptr, err};
    const uint32_t grid = static_cast<uint32_t>((nunits + 4u * dev::kRunDefault - 1u) / (4u * dev::kRunDefault));
    const uint32_t tgrid = static_cast<uint32_t>((nlists + 4u * dev::kRunDefault - 1u) / (4u * dev::kRunDefault));
    if (!d1)
    {
        hipLaunchKernelGGL((dev::k_lists_dec<false, dev::kListsNC, dev::kListsMinW>), dim3(grid), dim3(256), 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess)
            return e;
        hipLaunchKernelGGL((dev::k_lists_tails<false, dev::kTailsNC>), dim3(tgrid), dim3(256), 0, s, A);
        return hipGetLastError();
    }
    // phase A keeps the first parse error of a full block; the decode pass
    // re-checks every unit (tails included) into the same word
    ChainView cv;
    if ((e = launch_lists_sums(in, in_bytes, off, nunits, W.rec, W.hdr, nlists, W.chain, &cv, err, s)) != hipSuccess)
        return e;
    A.sums = cv.sums;
    A.run_pre = cv.pre;
    A.run_tile = cv.tile;
    hipLaunchKernelGGL(dev::k_lists_pbase, dim3(flat_grid(nlists + 1u, s)), dim3(256), 0, s, nlists, nunits, W.ubase, cv.sums, cv.pre, cv.tile,
                       W.hdr, W.pbase);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    hipLaunchKernelGGL((dev::k_lists_dec<true, dev::kListsNC, dev::kListsMinW>), dim3(grid), dim3(256), 0, s, A);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    hipLaunchKernelGGL((dev::k_lists_tails<true, dev::kTailsNC>), dim3(tgrid), dim3(256), 0, s, A);
    return hipGetLastError();
}

} // namespace tpf
