// p4_lists_scan.hip -- tpf_lists_unit_offsets: the unit offsets of a lists
// stream that has none (an index written by the CPU library, or one saved
// without its 8 bytes per unit), from the lists' byte spans and the units'
// own headers (include/turbopfor_gpu.h).  The sequential
// definition is tpf_lists_scan_offsets (framing.cpp): the lengths below are
// one_block's for TPF_FMT_256V32 with n = 256 and TPF_FMT_32, refusals
// included.
//
// Passes: plan (one thread per list: the structure checks, its unit count) ->
// run scan of the unit counts (p4_scan.h) -> short (the verdict; one thread
// per list: the unit directory, and the one unit of a one-unit list, whose
// offset is its list's and whose length is only checked) -> walk (a wave per
// kScanRun lists; every list of two or more units is walked by the whole wave,
// a dependent chain of one step per unit).  No base payload is read: headers,
// exception bitmaps and vbyte markers only.
#include "p4_lists.h"

#include "p4_lists_dev.h"
#include "p4_lists_host.h"

namespace tpf::dev
{

constexpr uint32_t kScanRun = 16;       // lists per wave of the walk
constexpr uint32_t kScanWin = 1024;     // the walker's window: 64 lanes x 16 bytes of the stream in LDS
constexpr uint32_t kScanWinU32 = kScanWin / 4u + 20u; // + what lds_u32 and a 64-byte marker window may touch past a position
constexpr uint32_t kScanAvailCap = 1u << 20; // no unit is longer than 2 + 1024 + 5 * 255 + 255 bytes

struct ScanArgs
{
    const uint8_t * in;
    uint64_t in_bytes;
    const uint64_t * ptr;
    const uint64_t * lbyte;
    uint64_t nlists;
    uint64_t * off;
    uint64_t nunits;
    uint32_t * list_unit;      // optional
    const ListsHdr * hdr;
    const uint64_t * pre;      // run scan of the lists' unit counts
    const uint64_t * tile;
    unsigned long long * err;
};

// ---- the framing rules (framing.cpp one_block) -------------------------------
enum : uint32_t
{
    kUhBad = 0,
    kUhDone = 1,   // size: the unit's length
    kUhBitmap = 2, // size: its length without the exceptions (pad8(xn * bx) more, xn the bitmap's popcount)
    kUhVbyte = 3,  // size: where V starts (2 + base); xn values follow, then xn positions
};

struct UnitHead
{
    uint32_t kind, size, bx, xn;
};

// What the first two bytes decide.  h = in[0]; b1 = in[1], read only when
// avail >= 2; avail capped at kScanAvailCap; a full block is p4Enc256v32 of 256
// values, a tail p4Enc32 of n.
__device__ __forceinline__ UnitHead unit_head(uint32_t h, uint32_t b1, uint32_t avail, bool full, uint32_t n)
{
    UnitHead r{kUhBad, 0u, 0u, 0u};
    const auto base = [&](uint32_t b) { return full ? base_bytes<Fmt::V256>(256u, b) : base_bytes<Fmt::H32>(n, b); };
    if ((h & 0xC0u) == 0xC0u)
    {
        const uint32_t b = h & 0x3Fu;
        if (!full && b > 32u)
            return r;
        r.size = 1u + (b + 7u) / 8u;
        r.kind = r.size <= avail ? kUhDone : kUhBad;
        return r;
    }
    if ((h & 0x40u) == 0u)
    {
        const uint32_t b = h & 0x7Fu;
        uint32_t hdr = 1u;
        if ((h & 0x80u) != 0u)
        {
            if (avail < 2u)
                return r;
            r.bx = b1;
            hdr = 2u;
        }
        if (b > 32u || r.bx > 32u)
            return r;
        if (r.bx == 0u)
        {
            r.size = hdr + base(b);
            r.kind = r.size <= avail ? kUhDone : kUhBad;
            return r;
        }
        const uint32_t bm = pad8d(n);
        if (avail < 2u + bm)
            return r;
        r.size = 2u + bm + base(b);
        r.kind = kUhBitmap;
        return r;
    }
    const uint32_t b = h & 0x3Fu;
    if (b > 32u || avail < 2u)
        return r;
    r.xn = b1;
    r.size = 2u + base(b);
    r.kind = r.size < avail ? kUhVbyte : kUhBad; // V has at least one byte
    return r;
}

// the first `bits` (<= 32) bits of a bitmap word
__device__ __forceinline__ uint32_t bitmap_count(uint32_t w, uint32_t bits) { return __builtin_popcount(w & mask32(bits)); }

// One thread sizes the unit at g: byte loads, nothing at or past g + avail.
// 0: malformed, or longer than avail.
__device__ __forceinline__ uint32_t unit_size_serial(const uint8_t * __restrict g, uint64_t avail64, bool full, uint32_t n)
{
    const uint32_t avail = static_cast<uint32_t>(min_u64(avail64, kScanAvailCap));
    if (avail < 1u)
        return 0u;
    const UnitHead H = unit_head(g[0], avail >= 2u ? g[1] : 0u, avail, full, n);
    if (H.kind == kUhBad)
        return 0u;
    if (H.kind == kUhDone)
        return H.size;
    if (H.kind == kUhBitmap)
    {
        uint32_t xn = 0u;
        for (uint32_t i = 0; 8u * i < n; ++i)
            xn += bitmap_count(g[2u + i], n - 8u * i < 8u ? n - 8u * i : 8u);
        const uint32_t sz = H.size + pad8d(xn * H.bx);
        return sz <= avail ? sz : 0u;
    }
    uint32_t p = H.size;
    if (g[p] == 0xFFu)
        p += 1u + 4u * H.xn;
    else
        for (uint32_t k = 0; k < H.xn; ++k)
        {
            if (p >= avail)
                return 0u;
            p += vbyte_len<false>(g[p]);
        }
    p += H.xn;
    return p <= avail ? p : 0u;
}

// ---- the walker's window -----------------------------------------------------
// kScanWin bytes of the stream in LDS, from the 16-byte aligned address at or
// below in + pos: lane t loads one aligned 16-byte chunk, and only a chunk
// that starts below in + hi (the end of the list's span; the others read as
// zeros).  An aligned chunk that holds a byte of the stream lies in that
// byte's page.  wlo: the stream position of the window's first byte (up to 15
// below pos, so it may be negative).  (A second row in LDS with a third in
// flight into registers, so that a walk forwards never waits for a load, was
// measured and not kept: 0.67 us per step against 0.61 -- the chain is bound
// by its LDS and cross-lane round trips, not by the loads)
struct ScanWin
{
    uint32_t * w;
    const uint8_t * in;
    uint64_t hi;
    int64_t wlo;
    uint32_t t;

    __device__ __forceinline__ void load(uint64_t pos)
    {
        const uint64_t a = reinterpret_cast<uint64_t>(in) + pos;
        const uint64_t a0 = a & ~15ull;
        wlo = static_cast<int64_t>(pos) - static_cast<int64_t>(a - a0);
        const uint64_t c = a0 + 16u * t;
        u32x4 v{0u, 0u, 0u, 0u};
        if (c < reinterpret_cast<uint64_t>(in) + hi)
            v = *reinterpret_cast<const u32x4 *>(c);
        wave_lds_sync();
        reinterpret_cast<u32x4 *>(w)[t] = v;
        wave_lds_sync();
    }
    // the LDS byte offset of stream position pos, with [pos, pos + need) inside the window (need <= 80)
    __device__ __forceinline__ uint32_t at(uint64_t pos, uint32_t need)
    {
        const int64_t d = static_cast<int64_t>(pos) - wlo;
        if (d < 0 || d + need > static_cast<int64_t>(kScanWin))
            load(pos);
        return static_cast<uint32_t>(static_cast<int64_t>(pos) - wlo);
    }
};

// The whole wave sizes the unit at stream position p (every argument and the
// result wave-uniform): the bitmap's popcount across lanes, the marker walk by
// window_starts (p4_block32.h) over 64-byte windows of the LDS window.
__device__ __forceinline__ uint32_t unit_size_wave(ScanWin & W, uint64_t p, uint64_t avail64, bool full, uint32_t n)
{
    const uint32_t t = W.t;
    const uint32_t avail = static_cast<uint32_t>(min_u64(avail64, kScanAvailCap));
    if (avail < 1u)
        return 0u;
    const uint32_t o = W.at(p, 40u);
    const uint32_t hw = uni(lds_u32(W.w, o));
    const UnitHead H = unit_head(hw & 0xFFu, avail >= 2u ? (hw >> 8) & 0xFFu : 0u, avail, full, n);
    if (H.kind == kUhBad)
        return 0u;
    if (H.kind == kUhDone)
        return H.size;
    if (H.kind == kUhBitmap)
    {
        // lane t < 8: bits 32t .. 32t + 31 of the bitmap (at most 256)
        const uint32_t bits = 32u * t < n ? umin32(n - 32u * t, 32u) : 0u;
        const uint32_t xn = wave_sum(t < 8u ? bitmap_count(lds_u32(W.w, o + 2u + 4u * t), bits) : 0u);
        const uint32_t sz = H.size + pad8d(xn * H.bx);
        return sz <= avail ? sz : 0u;
    }
    const uint32_t xn = H.xn;
    const uint32_t m0 = uni(lds_byte(W.w, W.at(p + H.size, 1u)));
    uint32_t end = H.size; // of the values, from p
    if (m0 == 0xFFu)
        end += 1u + 4u * xn;
    else
    {
        uint64_t cpos = p + H.size;
        uint32_t sp = 0u, found = 0u;
        while (found < xn)
        {
            const uint32_t c = W.at(cpos, 64u);
            const uint32_t nxt = t + vbyte_len<false>(lds_byte(W.w, c + t));
            const uint32_t ps = window_starts(nxt, sp, t);
            const uint32_t m = static_cast<uint32_t>(__builtin_popcountll(__ballot(ps < 64u))); // >= 1: sp < 64
            const uint32_t cnt = umin32(m, xn - found);
            const uint32_t pn = bperm(nxt, ps); // every lane: bpermute reads 0 from inactive lanes
            const uint32_t pe = ps < 64u ? pn : ps;
            const uint32_t s_last = uni(__builtin_amdgcn_readlane(ps, cnt - 1u));
            const uint32_t e_last = uni(__builtin_amdgcn_readlane(pe, cnt - 1u));
            found += cnt;
            // every marker lies below avail: the starts ascend, and each is
            // decided by the markers before it alone
            if (cpos - p + s_last >= avail)
                return 0u;
            end = static_cast<uint32_t>(cpos - p) + e_last;
            sp = e_last >= 64u ? e_last - 64u : e_last;
            cpos += e_last >= 64u ? 64u : 0u;
        }
    }
    end += xn;
    return end <= avail ? end : 0u;
}

// ---- the passes --------------------------------------------------------------
// Plan: one thread per list -- the checks of everything the later passes index
// with, and its unit count for the run scan.
__global__ __launch_bounds__(256) void k_scan_plan(const uint64_t * __restrict ptr, const uint64_t * __restrict lbyte, uint64_t nlists,
                                                    uint64_t in_bytes, uint32_t * __restrict tot, ListsHdr * __restrict hdr)
{
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < nlists; j += gsz)
    {
        const uint64_t a = ptr[j], b = ptr[j + 1u];
        const uint64_t lo = lbyte[j], hi = lbyte[j + 1u];
        const bool bad = b < a || hi < lo || hi > in_bytes || (a == b && hi != lo);
        tot[j] = bad ? 0u : list_units(b - a);
        if (bad)
            atomicMin(&hdr->bad, static_cast<unsigned long long>(j));
    }
}

// Short: the verdict (d_err for a refused structure), then per list its entry
// of the unit directory and, for a list of one unit, that unit.
__global__ __launch_bounds__(256) void k_scan_short(const ScanArgs A)
{
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (!lists_go(A.hdr, A.nunits))
    {
        if (gid == 0 && A.err != nullptr)
            *A.err = A.hdr->bad != ~0ull ? A.nunits + A.hdr->bad : A.nunits + A.nlists;
        return;
    }
    const uint64_t gsz = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = gid; j < A.nlists; j += gsz)
    {
        const uint32_t ub = static_cast<uint32_t>(run_base(A.pre, A.tile, j)); // <= nunits < 2^31
        if (A.list_unit != nullptr)
            A.list_unit[j] = ub;
        const uint64_t n = A.ptr[j + 1u] - A.ptr[j];
        if (list_units(n) != 1u)
            continue;
        const uint64_t lo = A.lbyte[j], hi = A.lbyte[j + 1u];
        A.off[ub] = lo;
        const bool full = n == 256u;
        const uint32_t sz = unit_size_serial(A.in + lo, hi - lo, full, full ? 256u : static_cast<uint32_t>(n));
        if ((sz == 0u || sz != hi - lo) && A.err != nullptr) // the one unit ends its list's span
            atomicMin(A.err, static_cast<unsigned long long>(ub));
    }
    if (gid == 0)
    {
        A.off[A.nunits] = A.lbyte[A.nlists];
        if (A.list_unit != nullptr)
            A.list_unit[A.nlists] = static_cast<uint32_t>(A.nunits);
    }
}

// Walk: every wave owns kScanRun consecutive lists, lane t list first + t; the
// lists of two or more units are walked one after the other by the whole wave.
// Lane i % 64 keeps the offset of unit i until 64 are stored at once.  A bad
// unit ends its list: the units after it get the end of the span.
__global__ __launch_bounds__(256) void k_scan_walk(const ScanArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t wins[4][kScanWinU32];
    if (!lists_go(A.hdr, A.nunits))
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kScanRun;
    if (first >= A.nlists)
        return;
    const uint32_t nl = static_cast<uint32_t>(min_u64(kScanRun, A.nlists - first));
    const uint64_t j = first + t;
    const uint64_t n = t < nl ? A.ptr[j + 1u] - A.ptr[j] : 0ull;
    const uint32_t units = list_units(n);
    uint64_t walk = __ballot(units >= 2u);
    if (walk == 0ull)
        return;
    const uint64_t lo = units >= 2u ? A.lbyte[j] : 0ull;
    const uint64_t hi = units >= 2u ? A.lbyte[j + 1u] : 0ull;
    const uint32_t ub = units >= 2u ? static_cast<uint32_t>(run_base(A.pre, A.tile, j)) : 0u;
    ScanWin W{wins[wv], A.in, 0ull, 0, t};
    for (; walk != 0ull; walk &= walk - 1ull)
    {
        const uint32_t jj = static_cast<uint32_t>(__builtin_ctzll(walk));
        const uint32_t un = rl(units, jj), u0 = rl(ub, jj);
        const uint64_t nj = readlane_u64(n, jj);
        const uint32_t nfull = static_cast<uint32_t>(nj >> 8), rem = static_cast<uint32_t>(nj & 255u);
        const uint64_t end = readlane_u64(hi, jj);
        uint64_t p = readlane_u64(lo, jj);
        uint64_t mine = 0ull;
        W.hi = end;
        W.load(p);
        uint32_t i = 0u;
        bool bad = false;
        for (; i < un; ++i)
        {
            if ((i & 63u) == t)
                mine = p;
            const bool full = i < nfull;
            const uint32_t sz = unit_size_wave(W, p, end - p, full, full ? 256u : rem);
            bad = sz == 0u || (i + 1u == un && sz != end - p);
            if (bad)
                break;
            p += sz;
            if ((i & 63u) == 63u)
                A.off[u0 + (i - 63u) + t] = mine;
        }
        // what lanes still hold: units (i & ~63) .. i, or .. un - 1 of a clean list that did not end on a store
        const uint32_t held = bad ? (i & 63u) + 1u : (un & 63u);
        const uint32_t hbase = bad ? (i & ~63u) : (un & ~63u);
        if (t < held)
            A.off[u0 + hbase + t] = mine;
        if (bad)
        {
            if (t == 0 && A.err != nullptr)
                atomicMin(A.err, static_cast<unsigned long long>(u0 + i));
            for (uint32_t k = i + 1u + t; k < un; k += 64u)
                A.off[u0 + k] = end;
        }
    }
}

} // namespace tpf::dev

namespace tpf
{

namespace
{
// Workspace: header | run scan of the lists' unit counts, each 256-byte
// aligned.  Nothing in it is sized by the units.
struct ScanWs
{
    dev::ListsHdr * hdr;
    RunScanWs<uint64_t> scan;
    size_t bytes;

    ScanWs(void * ws, uint64_t nlists)
    {
        WsCarver c(ws);
        hdr = c.take<dev::ListsHdr>(1);
        scan = c.scan<uint64_t>(nlists);
        bytes = c.used;
    }
};
} // namespace

size_t lists_unit_offsets_workspace(uint64_t, uint64_t nlists) { return ScanWs(nullptr, nlists).bytes; }

hipError_t launch_lists_unit_offsets(const uint8_t * in, uint64_t in_bytes, const uint64_t * ptr, const uint64_t * lbyte, uint64_t nlists,
                                     uint64_t * off, uint64_t nunits, uint32_t * list_unit, void * ws, unsigned long long * err,
                                     hipStream_t s)
{
    if (nlists == 0)
        return fill_u32(off, 0u, 2, s);
    if (nunits > 0x7FFFFFFFull || nlists > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const ScanWs W(ws, nlists);
    hipError_t e = fill_u32(W.hdr, 0xFFFFFFFFu, 4, s);
    if (e != hipSuccess)
        return e;
    if ((e = launch(dev::k_scan_plan, flat_grid(nlists, s), 256, s, ptr, lbyte, nlists, in_bytes, W.scan.tot, W.hdr)) != hipSuccess)
        return e;
    if ((e = launch_run_scan_u64(W.scan.tot, nlists, W.scan.pre, W.scan.tile, reinterpret_cast<uint64_t *>(&W.hdr->total), s)) != hipSuccess)
        return e;
    const dev::ScanArgs A{.in = in,
                          .in_bytes = in_bytes,
                          .ptr = ptr,
                          .lbyte = lbyte,
                          .nlists = nlists,
                          .off = off,
                          .nunits = nunits,
                          .list_unit = list_unit,
                          .hdr = W.hdr,
                          .pre = W.scan.pre,
                          .tile = W.scan.tile,
                          .err = err};
    if ((e = launch(dev::k_scan_short, flat_grid(nlists, s), 256, s, A)) != hipSuccess)
        return e;
    return launch(dev::k_scan_walk, wave_grid(nlists, dev::kScanRun), 256, s, A);
}

} // namespace tpf
