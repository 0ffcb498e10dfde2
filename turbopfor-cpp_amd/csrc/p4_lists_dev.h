// p4_lists_dev.h -- device helpers shared by the lists kernels (p4_lists*.hip):
// the pipeline shapes, a wave's run of units / lists / items, how every lane
// of a wave's run of units finds its list from the unit records (run_ids,
// p4_lists.h) and where the run's blocks go (RunOut), the decode of one full
// 256v32 unit and of one p4Enc32 tail unit out of the run plane's pipeline
// (p4_dec_run.h), the error report of a run, the tails driver every tails
// kernel runs (tail_units), and the checks of a list against the unit
// directory.  The item drivers are in p4_lists_items.h.  Device code only:
// included by *.hip files (internal).
#pragma once

#include "p4_lists.h"

#include "p4_dec_run.h"
#include "p4_generic.h"
#include "tpf_device.h"

namespace tpf::dev
{

// pipeline shapes of the lists decodes
constexpr uint32_t kListSlot = 2432;      // tails: the generic decoder's slot (a 2,304-byte image + 128)
constexpr uint32_t kListScratchU32 = 512; // decode_block_g<H32>'s scratch
constexpr uint32_t kListsNC = 6;          // full blocks: the k_dec256v32w pipeline, 7 waves per SIMD
constexpr int kListsMinW = 7;
constexpr uint32_t kTailsNC = 4;          // tails: the k_dec_gr pipeline

__device__ __forceinline__ uint32_t list_units(uint64_t n)
{
    // more units than any stream may hold: clamped, so the total cannot wrap back to nunits
    const uint64_t u = (n >> 8) + ((n & 255u) != 0u ? 1u : 0u);
    return u > 0x80000000ull ? 0x80000000u : static_cast<uint32_t>(u);
}

// Inclusive max-scan over the wave (identity 0).
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x)
{
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xa, 0xf, false));
    x = umax32(x, __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xc, 0xf, false));
    return x;
}

// The last j of [0, n) with tab[j] <= x, for tab[0] <= x < tab[n], by a
// cooperative search -- 64 pivots per step, so 2^24 entries take 4 dependent
// loads.  Invariant: tab[lo] <= x < tab[hi].  (The list holding unit `first`:
// tab = ubase, ubase[nlists] = nunits.)
template <class E>
__device__ __forceinline__ uint32_t find_list(const E * __restrict tab, uint32_t n, E x, uint32_t t)
{
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u)
    {
        const uint32_t step = (hi - lo + 63u) / 64u;
        const uint64_t p = static_cast<uint64_t>(lo) + static_cast<uint64_t>(t + 1u) * step;
        const bool le = p < hi && tab[p] <= x;
        const uint32_t c = static_cast<uint32_t>(__builtin_popcountll(__ballot(le))); // tab ascends: the first c pivots
        lo = uni(lo + c * step);
        hi = uni(umin32(hi, lo + step));
    }
    return lo;
}

// A wave's place in a kernel that gives every wave a run of `run` consecutive
// items (units, lists, selections): its lane and wave, the stream's bounds for
// the run plane, the run's first item and its length.  A run past `items`
// (first >= items) has nothing to do.
struct WaveRun
{
    uint32_t t, wv;
    uint64_t in_base, in_end;
    uint64_t first;
    uint32_t n;

    __device__ __forceinline__ void seek(uint64_t f, uint32_t run, uint64_t items)
    {
        first = f;
        n = static_cast<uint32_t>(min_u64(run, items - f));
    }
};

__device__ __forceinline__ WaveRun wave_run(const uint8_t * in, uint64_t in_bytes, uint32_t run, uint64_t items)
{
    WaveRun R;
    R.t = threadIdx.x & 63u;
    R.wv = uni(threadIdx.x >> 6);
    R.in_base = reinterpret_cast<uint64_t>(in);
    R.in_end = R.in_base + in_bytes;
    R.seek((static_cast<uint64_t>(blockIdx.x) * 4u + R.wv) * run, run, items);
    return R;
}

// The list (selection, query) of every unit of a wave's run of units, from the
// unit records: lane t holds rec_word, the record of unit first + t (0 past
// the run).  A head inside the run names its list, the units after it follow
// by a max-scan, and the units before the run's first head belong to the list
// of unit `first`: its own head, or one search over base_table[0 .. n].
__device__ __forceinline__ uint32_t run_ids(uint32_t rec_word, const uint32_t * __restrict base_table, uint64_t n, uint64_t first, uint32_t t)
{
    const uint32_t r0 = rl(rec_word, 0) & kRecList;
    const uint32_t j0 = r0 != 0u ? r0 - 1u : find_list(base_table, static_cast<uint32_t>(n), static_cast<uint32_t>(first), t);
    return umax32(wave_incl_max(rec_word & kRecList), j0 + 1u) - 1u;
}

// Where a run's full blocks go.  The output of a lists decode is dense, so the
// values of a run are one contiguous range: one buffer descriptor from the
// run's first value to the end of its last full block, 16 bytes per lane at a
// position that is only 4-byte aligned, stores past the range dropped.  Lane
// t's unit starts at value `opos` of `out`.
struct RunOut
{
    __amdgpu_buffer_rsrc_t rs;
    uint32_t rel; // lane t's unit: bytes from the run's first value

    __device__ __forceinline__ RunOut() : rs(make_rsrc(nullptr, 0u)), rel(0u) {} // nothing is stored
    __device__ __forceinline__ RunOut(uint32_t * out, uint64_t opos, uint64_t fullmask)
    {
        const uint64_t opos0 = readlane_u64(opos, 0);
        rel = static_cast<uint32_t>(opos - opos0) * 4u;
        const uint32_t lastf = 63u - static_cast<uint32_t>(__builtin_clzll(fullmask));
        rs = make_rsrc(out + opos0, rl(rel, lastf) + 1024u);
    }
    // unit jj's block, lane t holding values 4t .. 4t + 3
    __device__ __forceinline__ void store(uint32_t jj, uint32_t t, const u32x4 & x) const { st16_run(rs, rl(rel, jj) + 16u * t, x); }
};

// Unit jj of a run out of the pipeline: staged into the wave's slot, decoded
// into registers, delta-1 applied from `start`, and its parsed length held
// against its offsets (a mismatch sets bit jj of badmask).  The caller stores
// or uses the values and then calls wave_lds_sync() before the next unit is
// staged.  Full 256v32 block: lane t holds values 4t .. 4t + 3.
template <bool D1, class Plane>
__device__ __forceinline__ void decode_full_unit(const Plane & P, const Chunk & c, uint32_t jj, uint32_t * slot, uint32_t * scr,
                                                 uint32_t start, uint32_t t, u32x4 & v, uint64_t & badmask)
{
    const uint32_t ctl = P.stage(c, jj, slot, t);
    const uint32_t used = decode_block256v32(slot, (ctl >> kCtlShift) & 15u, P.head(c, ctl, slot), scr, t, v);
    if constexpr (D1)
        apply_delta1_256(v, start);
    if (used != rl(P.len, jj))
        badmask |= 1ull << jj;
}

// p4Enc32 tail of cnt < 256 values: lane t holds values t + 64q.  (cmode
// lives with the values in the caller's frame: as a local of this function it
// cost the delta-1 tails kernels 3 VGPRs and one wave per SIMD.)
struct TailVals
{
    uint32_t v[4];
    uint32_t cmode; // decode_block_g's: 1 for a constant block
};

template <bool D1, class Plane>
__device__ __forceinline__ void decode_tail_unit(const Plane & P, const Chunk & c, uint32_t jj, uint32_t * slot, uint32_t * scr,
                                                 uint32_t cnt, uint32_t start, uint32_t t, TailVals & x, uint64_t & badmask)
{
    const uint32_t ctl = P.stage(c, jj, slot, t);
    const uint32_t used = decode_block_g<Fmt::H32>(slot, (ctl >> kCtlShift) & 15u, cnt, scr, t, x.v, &x.cmode);
    if constexpr (D1)
        (void)delta1_g<uint32_t>(x.v, cnt, start, t);
    if (used != rl(P.len, jj))
        badmask |= 1ull << jj;
}

// The error report of a run: the lowest source unit among the lanes of
// badmask, in stream numbering (`su`: lane t's unit; the units of a run need
// not ascend).
__device__ __forceinline__ void report_bad_units(unsigned long long * err, uint64_t badmask, uint32_t su, uint32_t t)
{
    if (err != nullptr && badmask != 0u)
    {
        const uint32_t m = wave_min(((badmask >> t) & 1ull) != 0ull ? su : 0xFFFFFFFFu);
        if (t == 0)
            atomicMin(err, static_cast<unsigned long long>(m));
    }
}

// The tails driver: a wave's run of up to kRunDefault tail units through the
// generic decoder's pipeline (k_dec_gr, p4_generic.hip).  Lane t of run R
// holds item first + t's tail -- source unit su of cnt values (`has`; hasmask
// its ballot, not 0) -- or nothing.  The offsets of the lanes' units are
// loaded and the run plane is set up, then start() does what else the kernel
// gathers per lane -- behind the offsets' loads -- and gives the lane's
// delta-1 start (any value in the plain form), the first chunks go in flight,
// and every unit of hasmask is decoded into registers and handed to sink(jj,
// cj, vals): unit jj of the run, its count, lane t holding values t + 64q.
// The wave_lds_sync() before the next unit is staged is the driver's; a sink
// that goes through LDS itself keeps its own inner sync.  A lane outside
// hasmask loads nothing.  Parse errors are reported by source unit.  (The
// values stay a local of the consume lambda: see TailVals.)
template <bool D1, uint32_t NC, class Start, class Sink>
__device__ __forceinline__ void tail_units(const WaveRun & R, const uint64_t * __restrict off, bool has, uint64_t hasmask, uint32_t su,
                                           uint32_t cnt, uint32_t * slot, uint32_t * scr, unsigned long long * err, Start && start,
                                           Sink && sink)
{
    const uint32_t t = R.t;
    const uint64_t o = has ? off[su] : 0ull;
    const uint64_t e = has ? off[su + 1u] : 0ull;
    RunPlaneT<kListSlot> P;
    P.init(R.in_base, R.in_end, o, e, has);
    const uint32_t startv = start();
    uint64_t badmask = 0u;
    Chunk C[NC];
    pipe_prime<NC>(P, C, t);
    pipe_drain<NC>(P, C, R.n, t, [&](const Chunk & c, uint32_t jj) {
        if (((hasmask >> jj) & 1ull) == 0ull)
            return;
        const uint32_t cj = rl(cnt, jj);
        TailVals x;
        decode_tail_unit<D1>(P, c, jj, slot, scr, cj, rl(startv, jj), t, x, badmask);
        sink(jj, cj, x);
        wave_lds_sync();
    });
    report_bad_units(err, badmask, su, t);
}

// The sink of a tails kernel that stores the values: unit jj's cj values at
// base + lane jj's opos (read when a unit is stored: start() may set it).  NT:
// non-temporal, for an output that is not read again by the call.
template <bool NT>
__device__ __forceinline__ auto tail_store(uint32_t * base, const uint64_t & opos, uint32_t t)
{
    return [base, &opos, t](uint32_t jj, uint32_t cj, const TailVals & x) {
        uint32_t * op = base + readlane_u64(opos, jj);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (t + 64u * q < cj)
            {
                if constexpr (NT)
                    __builtin_nontemporal_store(x.v[q], op + t + 64u * q);
                else
                    op[t + 64u * q] = x.v[q];
            }
    };
}

// List j against the unit directory: j names a list, its pointers and its
// units ascend, the units lie inside the stream and there are as many as its
// n values need.  Nothing is read at an index that was not checked first.
__device__ __forceinline__ bool list_dir_ok(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                            uint64_t nunits, uint32_t j, uint64_t * n, uint32_t * ua, uint32_t * ub)
{
    if (j >= nlists)
        return false;
    const uint64_t a = ptr[j], b = ptr[j + 1u];
    *ua = list_unit[j];
    *ub = list_unit[j + 1u];
    *n = b - a;
    return a <= b && *ua <= *ub && *ub <= nunits && *ub - *ua == list_units(b - a);
}

// The segment of CSR pointers seg_ptr[0 .. nq] holding index i -- the last k
// with seg_ptr[k] <= i, then i < seg_ptr[k + 1] held against it -- or
// kItemNone when i lies in none.
__device__ __forceinline__ uint32_t segment_of(const uint64_t * __restrict seg_ptr, uint64_t nq, uint64_t i)
{
    uint64_t lo = 0u, hi = nq;
    while (lo < hi)
    {
        const uint64_t m = lo + (hi - lo) / 2u;
        if (seg_ptr[m] <= i)
            lo = m + 1u;
        else
            hi = m;
    }
    return (lo != 0u && i < seg_ptr[lo]) ? static_cast<uint32_t>(lo - 1u) : kItemNone;
}

// The per-query checks of a request against a resident index (one thread per
// QUERY): everything the later passes index with is checked here (the values
// are checked, never followed), the first refused query by atomicMin.
__device__ __forceinline__ void check_queries(const uint64_t * __restrict ptr, const uint32_t * __restrict list_unit, uint64_t nlists,
                                              uint64_t nunits, const uint64_t * __restrict seg_ptr, uint64_t seg_values,
                                              const uint32_t * __restrict qlist, uint64_t nq, unsigned long long * __restrict bad,
                                              uint64_t gid, uint64_t gsz)
{
    for (uint64_t k = gid; k < nq; k += gsz)
    {
        const uint64_t pa = seg_ptr[k], pb = seg_ptr[k + 1u];
        uint64_t n;
        uint32_t ua, ub;
        if (pb < pa || pb > seg_values || !list_dir_ok(ptr, list_unit, nlists, nunits, qlist[k], &n, &ua, &ub))
            atomicMin(bad, static_cast<unsigned long long>(k));
    }
}

// The start of delta-1 source unit su of `list` from the skip table: start0
// for the list's first unit, else the last value of the unit before it (a unit
// of the same list: in range whatever the table holds).
__device__ __forceinline__ uint32_t unit_start(const uint32_t * __restrict list_unit, const uint32_t * __restrict start0,
                                               const uint32_t * __restrict unit_last, uint32_t list, uint32_t su)
{
    return su == list_unit[list] ? (start0 != nullptr ? start0[list] : 0u) : unit_last[su - 1u];
}

} // namespace tpf::dev
