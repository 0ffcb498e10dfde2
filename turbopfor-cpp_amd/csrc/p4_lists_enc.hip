// p4_lists_enc.hip -- tpf_p4nenc256v32_lists: many posting lists laid end to
// end in one dense value array (CSR pointers), each encoded as an n-variant
// stream (n/256 256v32 blocks + an optional p4Enc32 tail) into one byte
// stream, in one submission with no host round trip (include/turbopfor_gpu.h,
// DESIGN.md 4.8).  The mirror of p4_lists.hip: the same plan / run scan /
// heads passes check the list structure and leave the unit records, then
//   tails plan : a wave per 16 lists, lane t plans list first+t's tail
//   full plan  : a wave per 32 units, plans the full blocks of its run, picks
//                up the tails' sizes and publishes the run's byte total
//   run scan   : exclusive prefix of the run totals, the stream's length
//   full write : rebuilds its run's offsets into d_off, checks the capacity,
//                writes the full blocks (sub-runs cut at every tail)
//   tails write: byte-exact copy-out of every tail at its offset
// Sizes and plan words live in the workspace, never in d_off: d_off only ever
// holds final offsets, written once by the full write pass, which the tails
// write pass (a later kernel) reads.  Every kernel reads the go / no-go header
// first; the two write kernels also the capacity verdict (bytes <= out_cap).
#include "p4_lists.h"

#include "p4_enc256v32.h"
#include "p4_generic.h"
#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

constexpr uint32_t kLencRun = 32;       // units per wave of the full-block passes (= the run scan's run)
constexpr uint32_t kLencTailRun = 16;   // lists per wave of the tails passes
constexpr uint32_t kLencTailImgU32 = 2432 / 4 + 8; // k_enc_gr's image of a one-block unit
constexpr uint32_t kLencNC = 3;         // value chunks in flight (kEncNCPlan / kEncNCWrite)

struct ListsEncHdr
{
    ListsHdr h;               // the structure verdict (p4_lists.h)
    unsigned long long bytes; // the stream's length, once the unit sizes are scanned
};

struct ListsEncArgs
{
    const uint32_t * in;
    const uint64_t * ptr;
    uint64_t nlists;
    const uint32_t * start0;
    uint64_t nunits;
    const ListsEncHdr * hdr;
    const uint32_t * rec;   // unit records (p4_lists.h)
    const uint32_t * ubase; // first unit of every list
    uint32_t * sz;          // bytes of every unit
    uint32_t * plan;        // plan word of every unit
    uint32_t * run_tot;     // bytes of every kLencRun-unit run
    const uint64_t * run_pre;
    const uint64_t * run_tile;
    uint8_t * out;
    uint64_t out_cap;
    uint64_t * off;
    unsigned long long * err;
    uint32_t devn; // 1: nunits is a capacity and the unit count is hdr->h.total (the append, p4_lists_append.hip)
};

// The arguments with the unit count the kernels work on: the caller's, or the
// one a device-side plan left in the header (more than the capacity: no go).
__device__ __forceinline__ ListsEncArgs enc_args(const ListsEncArgs & K)
{
    ListsEncArgs A = K;
    if (K.devn != 0u)
        A.nunits = min_u64(K.hdr->h.total, K.nunits + 1u);
    return A;
}

// A wave's run of up to kLencRun consecutive units: lane t holds unit first+t.
// The full blocks' values are one contiguous input range (the tails' values
// lie in between, in order), read through one buffer descriptor from the first
// full block's first value to the last one's last, 16 bytes per lane at
// positions that are only 4-byte aligned.
struct UnitRun
{
    uint32_t n;
    bool valid, full;
    uint64_t fullmask;
    uint32_t r_;    // the unit's record
    uint32_t relin; // bytes from the descriptor's base (kOob: not a full block)
    uint32_t stv;   // delta-1 start of a full block
    __amdgpu_buffer_rsrc_t rs;

    __device__ __forceinline__ void init(const ListsEncArgs & A, uint64_t first, uint32_t t)
    {
        n = static_cast<uint32_t>(min_u64(kLencRun, A.nunits - first));
        valid = t < n;
        r_ = valid ? A.rec[first + t] : 0u;
        full = valid && (r_ & kRecTail) == 0u;
        fullmask = __ballot(full);
    }

    // the list plane: heads inside the run, the search before it (k_lists_dec)
    template <bool D1>
    __device__ __forceinline__ void lists(const ListsEncArgs & A, uint64_t first, uint32_t t)
    {
        const uint32_t u = static_cast<uint32_t>(first) + t;
        // (run_ids, p4_lists_dev.h, stated in place: the encoder's kernels were left as they are)
        const uint32_t r0 = rl32(r_, 0) & kRecList;
        const uint32_t j0 = r0 != 0u ? r0 - 1u : find_list(A.ubase, static_cast<uint32_t>(A.nlists), static_cast<uint32_t>(first), t);
        const uint32_t id = umax32(wave_incl_max(r_ & kRecList), j0 + 1u) - 1u;
        const uint32_t ub = valid ? A.ubase[id] : 0u;
        const uint64_t p0 = valid ? A.ptr[id] : 0ull;
        const uint64_t pos = p0 + 256ull * (u - ub); // unit u - ub of its list
        const uint32_t firstf = static_cast<uint32_t>(__builtin_ctzll(fullmask));
        const uint32_t lastf = 63u - static_cast<uint32_t>(__builtin_clzll(fullmask));
        const uint64_t pos0 = readlane_u64(pos, firstf);
        relin = full ? static_cast<uint32_t>(pos - pos0) * 4u : kOob;
        rs = make_rsrc(A.in + pos0, rl32(relin, lastf) + 1024u);
        stv = 0u;
        if constexpr (D1)
        {
            // a list's first unit starts from start0, every later one from the
            // value before it (inside the list: never the value before a list)
            if (full)
                stv = u == ub ? (A.start0 != nullptr ? A.start0[id] : 0u) : A.in[pos - 1u];
        }
    }

    __device__ __forceinline__ u32x4 load(uint32_t jj, uint32_t t) const
    {
        // lanes past the run and tail units hold kOob: the load returns zeros without traffic
        return __builtin_amdgcn_raw_buffer_load_b128(rs, static_cast<int>(rl32(relin, jj) + 16u * t), 0, 0);
    }

    // body(v, jj) for the full blocks jj of the run, kLencNC units in flight
    template <class Body>
    __device__ __forceinline__ void walk(uint32_t t, Body && body) const
    {
        u32x4 C[kLencNC];
        const auto ld = [&](u32x4 & c, uint32_t jj) { c = load(jj, t); };
        ring_prime<kLencNC>(C, ld);
        ring_drain<kLencNC>(C, n, ld, [&](const u32x4 & c, uint32_t jj) {
            if ((fullmask >> jj) & 1ull)
                body(c, jj);
        });
    }
};

// ---- full blocks: plan --------------------------------------------------------
template <bool D1>
__global__ __launch_bounds__(256) void k_lenc_plan(const ListsEncArgs K)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][kPlanHistU32];
    const ListsEncArgs A = enc_args(K);
    if (!lists_go(&A.hdr->h, A.nunits))
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kLencRun;
    if (first >= A.nunits)
    {
        // a capacity's runs past the stream's end count nothing
        if (K.devn != 0u && first < K.nunits && t == 0u)
            A.run_tot[first / kLencRun] = 0u;
        return;
    }
    UnitRun R;
    R.init(A, first, t);
    // a tail's size: left by the tails plan pass (an earlier kernel)
    uint32_t szv = (R.valid && !R.full) ? A.sz[first + t] : 0u;
    uint32_t pwv = 0u;
    if (R.fullmask != 0ull)
    {
        R.template lists<D1>(A, first, t);
        R.walk(t, [&](u32x4 v, uint32_t jj) {
            if constexpr (D1)
                v = delta_encode(v, rl32(R.stv, jj), t);
            const Plan32 P = plan_block256(v, hist[wv], t);
            szv = t == jj ? P.size : szv;
            pwv = t == jj ? plan_word(P) : pwv;
        });
        if (R.full)
        {
            A.sz[first + t] = szv;
            A.plan[first + t] = pwv;
        }
    }
    publish_run_total(A.run_tot, first / kLencRun, R.valid ? szv : 0u, t);
}

// ---- full blocks: offsets, capacity, write ------------------------------------
// The run's offsets (run base + wave scan of the sizes, tails included) go to
// d_off whatever the capacity says; then, only when the stream fits, the full
// blocks are written.  RunCopyB (p4_enc32.h) assumes adjacent blocks: it stores
// whole 16-byte chunks and carries the chunk a block ends in into the next
// block's image.  Here a tail can sit between two full blocks of a run, and its
// bytes belong to k_lenc_tails: the run is cut into SUB-RUNS of adjacent full
// blocks, each with its own descriptor (base = its first byte rounded down to
// 16, length = its last byte), lead bytes and flush_tail, so every byte outside
// a sub-run is out of the descriptor's range and every shared chunk is written
// byte by byte.
template <bool D1>
__global__ __launch_bounds__(256) void k_lenc_write(const ListsEncArgs K)
{
    __shared__ __attribute__((aligned(16))) uint32_t img_all[4][kImgU32];
    __shared__ __attribute__((aligned(16))) uint32_t val_all[4][kEncValU32];
    const ListsEncArgs A = enc_args(K);
    if (!lists_go(&A.hdr->h, A.nunits))
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kLencRun;
    if (first >= A.nunits)
        return;
    UnitRun R;
    R.init(A, first, t);
    const uint32_t szv = R.valid ? A.sz[first + t] : 0u;
    const uint32_t incl = wave_incl_scan(szv); // a run's bytes fit 32 bits
    const uint64_t ov = run_base(A.run_pre, A.run_tile, first / kLencRun) + (incl - szv);
    if (R.valid)
        A.off[first + t] = ov;
    if (first + R.n == A.nunits && t == R.n - 1u)
        A.off[A.nunits] = ov + szv;
    if (A.hdr->bytes > A.out_cap)
    {
        if (first == 0u && t == 0u && A.err != nullptr)
            *A.err = A.nunits + A.nlists + 1u;
        return;
    }
    if (R.fullmask == 0ull)
        return; // a run of tails only
    R.template lists<D1>(A, first, t);
    const uint32_t pwv = R.full ? A.plan[first + t] : 0u;
    uint32_t * img = img_all[wv];
    uint32_t * val = val_all[wv];
    zero_image(img, kImgU32 / 4u, t);
    wave_lds_sync();
    const uint64_t ab = reinterpret_cast<uint64_t>(A.out) + ov; // lane t: unit first+t's first output byte
    const uint32_t trash_at = static_cast<uint32_t>(reinterpret_cast<uint8_t *>(val + kEncTrash + t) - reinterpret_cast<uint8_t *>(img));
    RunCopyB rc;
    uint64_t sub = 0ull;               // the sub-run's descriptor base
    uint32_t lead = 0u, rel_end = 0u;  // its first byte and its end, relative to sub
    R.walk(t, [&](u32x4 v, uint32_t jj) {
        const uint64_t a = readlane_u64(ab, jj);
        const uint32_t size = rl32(szv, jj);
        if (jj == 0u || ((R.fullmask >> (jj - 1u)) & 1ull) == 0ull)
        {
            // a sub-run starts: the adjacent full blocks from jj on
            const uint32_t last = jj + static_cast<uint32_t>(__builtin_ctzll(~(R.fullmask >> jj))) - 1u;
            sub = a & ~15ull;
            lead = static_cast<uint32_t>(a & 15ull);
            rel_end = static_cast<uint32_t>(readlane_u64(ab, last) - sub) + rl32(szv, last);
            rc.rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(sub), static_cast<short>(0), static_cast<int>(rel_end),
                                                      0x00020000);
            rc.carry = 0u;
        }
        if constexpr (D1)
            v = delta_encode(v, rl32(R.stv, jj), t);
        const uint32_t rel = static_cast<uint32_t>(a - sub);
        const EncGeo G = enc_geo(rl32(pwv, jj), size, rel, lead);
        emit_block256_g<true>(img, val, G, v, t);
        wave_lds_sync();
        // the block that completes the sub-run's partial first chunk stores its bytes [lead, 16)
        rc.put(img, G.c, lead != 0u && rel < 16u && rel + size >= 16u, lead, trash_at, t);
        wave_lds_sync();
        zero_image_n(img, G.c.n16, t); // only [0, sb + size) can be non-zero
        wave_lds_sync();
        if (((R.fullmask >> (jj + 1u)) & 1ull) == 0ull)
            rc.flush_tail(rel_end, lead, t); // the sub-run ends: its partial last chunk
    });
}

// ---- tails: plan (!WRITE) and write ----------------------------------------------
// Every wave owns kLencTailRun consecutive LISTS; lane t holds list first+t's
// tail: n % 256 values at the end of the list, unit ubase + n / 256, started
// (delta-1) from the value before it or, for a tail-only list, from start0.
// The encoder is the generic one-block encoder's (plan_block_g / emit_block_g
// <H32>, p4_generic.h) with the value count per lane; the copy-out is
// k_enc_gr's dword loop with byte stores on the two edge dwords, which the
// full blocks on either side share.
template <bool D1, bool WRITE>
__global__ __launch_bounds__(256) void k_lenc_tails(const ListsEncArgs K)
{
    __shared__ __attribute__((aligned(16))) uint32_t imgs[WRITE ? 4 : 1][WRITE ? kLencTailImgU32 : 1];
    __shared__ __attribute__((aligned(16))) uint32_t hist[WRITE ? 1 : 4][WRITE ? 4 : kPlanGHistU32]; // plan pass only
    const ListsEncArgs A = enc_args(K);
    if (!lists_go(&A.hdr->h, A.nunits))
        return;
    if constexpr (WRITE)
    {
        if (A.hdr->bytes > A.out_cap)
            return;
    }
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kLencTailRun;
    if (first >= A.nlists)
        return;
    const uint32_t nl = static_cast<uint32_t>(min_u64(kLencTailRun, A.nlists - first));
    const uint64_t j = first + t;
    const uint64_t p0 = t < nl ? A.ptr[j] : 0ull;
    const uint64_t p1 = t < nl ? A.ptr[j + 1u] : 0ull;
    const uint32_t cnt = static_cast<uint32_t>((p1 - p0) & 255u);
    const bool has = cnt != 0u;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0ull)
        return;
    const uint32_t nfull = static_cast<uint32_t>((p1 - p0) >> 8); // < 2^31: the structure was checked
    const uint32_t u = has ? A.ubase[j] + nfull : 0u;
    const uint64_t pos = p1 - cnt;
    uint32_t stv = 0u;
    if constexpr (D1)
    {
        if (has)
            stv = nfull == 0u ? (A.start0 != nullptr ? A.start0[j] : 0u) : A.in[pos - 1u];
    }
    uint32_t szv = 0u, pwv = 0u;
    uint64_t ov = 0ull;
    if constexpr (WRITE)
    {
        if (has)
        {
            pwv = A.plan[u];
            szv = A.sz[u];
            ov = A.off[u];
        }
    }
    uint32_t * img = imgs[WRITE ? wv : 0];
    if constexpr (WRITE)
    {
        for (uint32_t i = t; i < kLencTailImgU32; i += 64u)
            img[i] = 0u;
        wave_lds_sync();
    }
    const uint64_t out_base = reinterpret_cast<uint64_t>(A.out);
    // tail jj's elements t + 64q (zero past its count; nothing outside the list is read)
    auto load = [&](uint32_t jj, uint32_t v[4]) {
        const uint32_t * p = A.in + readlane_u64(pos, jj);
        const uint32_t c = rl32(cnt, jj);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            v[q] = t + 64u * q < c ? p[t + 64u * q] : 0u;
    };
    auto body = [&](uint32_t v[4], uint32_t jj) {
        const uint32_t c = rl32(cnt, jj);
        if constexpr (D1)
            delta_enc_g<uint32_t>(v, rl32(stv, jj), c, t);
        if constexpr (!WRITE)
        {
            const PlanG P = plan_block_g<Fmt::H32>(v, c, hist[wv], t);
            szv = t == jj ? P.size : szv;
            pwv = t == jj ? (P.b | (P.bx << 8) | (P.xn << 16) | (P.raw << 25)) : pwv;
        }
        else
        {
            const uint32_t size = rl32(szv, jj);
            const uint32_t pw = rl32(pwv, jj);
            const PlanG P{pw & 0xFFu, (pw >> 8) & 0xFFu, size, (pw >> 16) & 0x1FFu, (pw >> 25) & 1u};
            const uint64_t dst = out_base + readlane_u64(ov, jj);
            const uint32_t phase = static_cast<uint32_t>(dst & 3u);
            emit_block_g<Fmt::H32>(img, phase, P, v, c, t);
            wave_lds_sync();
            const uint64_t a0 = dst & ~3ull;
            const uint32_t end = phase + size;
            const uint32_t nd = (end + 3u) >> 2;
            typedef __attribute__((address_space(1))) uint32_t gu32;
            typedef __attribute__((address_space(1))) uint8_t gu8;
            for (uint32_t d = t; d < nd; d += 64u)
            {
                const uint64_t ga = a0 + 4u * d;
                const uint32_t w = img[d];
                const uint32_t lo = 4u * d, hi = lo + 4u;
                if (lo >= phase && hi <= end)
                    *(gu32 *)ga = w;
                else
                    for (uint32_t x = 0; x < 4; ++x)
                    {
                        const uint32_t bi = lo + x;
                        if (bi >= phase && bi < end)
                            *(gu8 *)(ga + x) = static_cast<uint8_t>(w >> (8u * x));
                    }
            }
            wave_lds_sync();
            for (uint32_t d = t; d < nd; d += 64u)
                img[d] = 0u;
            wave_lds_sync();
        }
    };
    // the next tail's values fly while one is encoded
    uint64_t m = hasmask;
    uint32_t jj = static_cast<uint32_t>(__builtin_ctzll(m));
    uint32_t va[4], vb[4]; // two tails rotate in registers (no copies of in-flight loads)
    load(jj, va);
    for (;;)
    {
        m &= m - 1ull;
        const uint32_t ja = jj;
        if (m != 0ull)
        {
            jj = static_cast<uint32_t>(__builtin_ctzll(m));
            load(jj, vb);
        }
        body(va, ja);
        if (m == 0ull)
            break;
        m &= m - 1ull;
        const uint32_t jb = jj;
        if (m != 0ull)
        {
            jj = static_cast<uint32_t>(__builtin_ctzll(m));
            load(jj, va);
        }
        body(vb, jb);
        if (m == 0ull)
            break;
    }
    if constexpr (!WRITE)
    {
        if (has)
        {
            A.sz[u] = szv;
            A.plan[u] = pwv;
        }
    }
}

// every list empty (nunits == 0): the stream is empty
__global__ void k_lenc_empty(const ListsEncHdr * __restrict hdr, uint64_t * __restrict off)
{
    if (threadIdx.x == 0 && lists_go(&hdr->h, 0u))
        off[0] = 0ull;
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
uint64_t lenc_runs(uint64_t nunits) { return (nunits + dev::kLencRun - 1u) / dev::kLencRun; }

// Workspace: header | run scan of the lists' unit counts | ubase (nlists + 1)
// | unit records | unit sizes | unit plan words (nunits each) | run scan of
// the kLencRun-unit runs' bytes, each 256-byte aligned.
struct ListsEncWs
{
    dev::ListsEncHdr * hdr;
    RunScanWs<uint64_t> lscan, uscan;
    uint32_t *ubase, *rec, *sz, *plan;
    size_t bytes;

    ListsEncWs(void * ws, uint64_t nunits, uint64_t nlists)
    {
        WsCarver c(ws);
        hdr = c.take<dev::ListsEncHdr>(1);
        lscan = c.scan<uint64_t>(nlists);
        ubase = c.take<uint32_t>(nlists + 1u);
        rec = c.take<uint32_t>(nunits);
        sz = c.take<uint32_t>(nunits);
        plan = c.take<uint32_t>(nunits);
        uscan = c.scan<uint64_t>(lenc_runs(nunits));
        bytes = c.used;
    }
};
} // namespace

size_t lists_enc_workspace(uint64_t nunits, uint64_t nlists) { return ListsEncWs(nullptr, nunits, nlists).bytes; }

namespace
{
// the passes after the structure: tails plan, full plan, run scan, full write, tails write
hipError_t lists_enc_passes(const dev::ListsEncArgs & A, const ListsEncWs & W, bool d1, hipStream_t s)
{
    hipError_t e;
    const uint64_t nunits = A.nunits;
    const uint32_t grid = wave_grid(nunits, dev::kLencRun), tgrid = wave_grid(A.nlists, dev::kLencTailRun);
    if ((e = launch_by(d1, [](auto D1) { return dev::k_lenc_tails<D1, false>; }, tgrid, 256, s, A)) != hipSuccess)
        return e;
    if ((e = launch_by(d1, [](auto D1) { return dev::k_lenc_plan<D1>; }, grid, 256, s, A)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64(W.uscan.tot, lenc_runs(nunits), W.uscan.pre, W.uscan.tile,
                                 reinterpret_cast<uint64_t *>(&W.hdr->bytes), s))
        != hipSuccess)
        return e;
    if ((e = launch_by(d1, [](auto D1) { return dev::k_lenc_write<D1>; }, grid, 256, s, A)) != hipSuccess)
        return e;
    return launch_by(d1, [](auto D1) { return dev::k_lenc_tails<D1, true>; }, tgrid, 256, s, A);
}

// the arguments over workspace W: `nunits` the unit count, or with devn its capacity
dev::ListsEncArgs lists_enc_args(const ListsEncWs & W, const uint32_t * in, const uint64_t * ptr, uint64_t nlists, const uint32_t * start0,
                                 uint64_t nunits, uint8_t * out, uint64_t out_cap, uint64_t * off, unsigned long long * err, uint32_t devn)
{
    return dev::ListsEncArgs{.in = in,
                             .ptr = ptr,
                             .nlists = nlists,
                             .start0 = start0,
                             .nunits = nunits,
                             .hdr = W.hdr,
                             .rec = W.rec,
                             .ubase = W.ubase,
                             .sz = W.sz,
                             .plan = W.plan,
                             .run_tot = W.uscan.tot,
                             .run_pre = W.uscan.pre,
                             .run_tile = W.uscan.tile,
                             .out = out,
                             .out_cap = out_cap,
                             .off = off,
                             .err = err,
                             .devn = devn};
}
} // namespace

// 11 launches whatever the lists: header reset, plan, 2 x run scan, heads
// (launch_lists_structure), tails plan, full plan, 2 x run scan, full write,
// tails write -- 12 with d_err's reset by the entry point.
hipError_t launch_lists_enc(const uint32_t * in, uint64_t in_values, const uint64_t * ptr, uint64_t nlists, bool d1,
                            const uint32_t * start0, uint8_t * out, uint64_t out_cap, uint64_t * off, uint64_t nunits, void * ws,
                            unsigned long long * err, hipStream_t s)
{
    if (nlists == 0)
        return off != nullptr ? fill_u32(off, 0u, 2, s) : hipSuccess;
    if (nunits > 0x7FFFFFFFull || nlists > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const ListsEncWs W(ws, nunits, nlists);
    hipError_t e = launch_lists_structure(ptr, nlists, in_values, nunits, &W.hdr->h, W.lscan, W.ubase, W.rec, err, s);
    if (e != hipSuccess)
        return e;
    if (nunits == 0)
        return launch(dev::k_lenc_empty, 1, 64, s, W.hdr, off);
    return lists_enc_passes(lists_enc_args(W, in, ptr, nlists, start0, nunits, out, out_cap, off, err, 0u), W, d1, s);
}

// The encode of lists whose structure a caller planned on the device (the
// append's staged lists): the caller fills the header (bad, total), ubase
// (nlists + 1) and the unit records of the view, units_cap (> 0) bounds the
// unit count, and nothing is reported through d_err.  6 launches.
ListsEncPlanView lists_enc_plan_view(void * ws, uint64_t units_cap, uint64_t nlists)
{
    const ListsEncWs W(ws, units_cap, nlists);
    return ListsEncPlanView{&W.hdr->h, W.ubase, W.rec};
}

hipError_t launch_lists_enc_planned(const uint32_t * in, const uint64_t * ptr, uint64_t nlists, bool d1, const uint32_t * start0,
                                    uint8_t * out, uint64_t out_cap, uint64_t * off, uint64_t units_cap, void * ws, hipStream_t s)
{
    const ListsEncWs W(ws, units_cap, nlists);
    return lists_enc_passes(lists_enc_args(W, in, ptr, nlists, start0, units_cap, out, out_cap, off, nullptr, 1u), W, d1, s);
}

} // namespace tpf
