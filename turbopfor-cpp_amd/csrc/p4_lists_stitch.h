// p4_lists_stitch.h -- the stitch pass the writers of a resident index share
// (tpf_lists_append, p4_lists_append.hip; tpf_lists_remove,
// p4_lists_remove.hip): every list of the new stream is a
// run of bytes kept from the old stream followed by a run of new bytes from a
// staged encode, and the output is cut into kListsAppendTile-byte tiles, a wave
// per tile.  Also the galloping search both calls use to go from a wave's
// first item to every lane's.  Device code only (internal).
#pragma once

#include "p4_lists_dev.h"

namespace tpf::dev
{

constexpr uint32_t kAppLaneBytes = 128; // the stitch pass: a list with no more bytes in the tile is moved by one lane

// The last j in [0, n) with tab[j] <= x, for tab[0] <= x < tab[n]: find_list (p4_lists_dev.h) for the wave's first item,
// then for one lane, from that j0 known to be at or before the answer, a galloping search -- one probe when the item
// lies in list j0 as most do.
template <class E>
__device__ __forceinline__ uint32_t gallop(const E * __restrict tab, uint32_t n, uint32_t j0, uint64_t x)
{
    uint32_t lo = j0, step = 1u;
    while (lo + step < n && tab[lo + step] <= x)
    {
        lo += step;
        step *= 2u;
    }
    uint32_t hi = umin32(lo + step, n); // tab[hi] > x (tab[n] > x)
    while (hi - lo > 1u)
    {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tab[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// dst[0 .. n) = src[0 .. n), a wave's work: 16-byte stores at the destination's
// 16-byte boundaries, each fed by aligned dword loads and v_alignbyte (k_copy16,
// host_copy.hip): a vector is moved that way only when every dword it reads
// holds a byte of src[0 .. n), the edges go byte by byte.
__device__ __forceinline__ void wave_move(uint8_t * dst, const uint8_t * src, uint32_t n, uint32_t t)
{
    const uint32_t head = umin32(n, (16u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src + head);
    const uint32_t sh = static_cast<uint32_t>(s0 & 3u);
    uint32_t nvec = (n - head) / 16u;
    // a shifted vector reads its last source bytes from a fifth dword, a
    // matching one reads four: both stay inside the source
    const uint32_t * w = reinterpret_cast<const uint32_t *>(s0 - sh);
    u32x4 * d = reinterpret_cast<u32x4 *>(dst + head);
    if (sh == 0u)
    {
        for (uint32_t i = t; i < nvec; i += 64u)
        {
            const uint32_t * q = w + 4u * i;
            const u32x4 v{q[0], q[1], q[2], q[3]};
            __builtin_nontemporal_store(v, d + i);
        }
    }
    else
    {
        for (uint32_t i = t; i < nvec; i += 64u)
        {
            const uint32_t * q = w + 4u * i;
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
            const u32x4 v{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                          __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh)};
            __builtin_nontemporal_store(v, d + i);
        }
    }
    const uint32_t tail0 = head + 16u * nvec; // n - tail0 < 16
    if (t < head)
        dst[t] = src[t];
    else if (t - head < n - tail0)
        dst[tail0 + (t - head)] = src[tail0 + (t - head)];
}

// A wave's tile of the output, n lists: lstart[j] (n + 1) is list j's first
// output byte; hdr->go and hdr->fit gate the pass.  Every list of the result is
// a run of kept bytes followed by a run of new ones, and `src` says where they
// come from: src(j, len, kb, ksrc, nsrc) is handed list j and its len output
// bytes and sets kb, its kept bytes, ksrc, their address, and nsrc, the address
// of the new bytes behind them.  NEW = false: no list has new bytes (kb = len)
// and nsrc is not read (tpf_lists_extract, p4_lists_extract.hip).
template <bool NEW, class Hdr, class Src>
__device__ __forceinline__ void stitch_tile(const Hdr * hdr, const uint64_t * lstart, uint64_t nlists_out, uint8_t * out, const Src & src)
{
    if (hdr->go == 0u || hdr->fit == 0u)
        return;
    const uint32_t t = threadIdx.x & 63u;
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t n = static_cast<uint32_t>(nlists_out);
    const uint64_t total = lstart[n];
    const uint64_t x0 = (static_cast<uint64_t>(blockIdx.x) * 4u + wv) * kListsAppendTile;
    if (x0 >= total)
        return;
    const uint64_t x1 = min_u64(x0 + kListsAppendTile, total);
    uint32_t jb = find_list(lstart, n, x0, t);
    for (;;)
    {
        // lane t: list jb + t, its bytes [s, e) of the output
        const uint32_t j = jb + t;
        const bool in = j < n;
        const uint64_t s = in ? lstart[j] : total;
        const uint64_t e = in ? lstart[j + 1u] : total;
        const bool act = in && s < x1 && e > x0 && e > s;
        uint64_t kb = 0ull, ksrc = 0ull, nsrc = 0ull;
        if (act)
            src(j, e - s, kb, ksrc, nsrc);
        // a list of at most kAppLaneBytes bytes inside the tile is moved by its own lane, 64 lists at a time: a tile of
        // thousands of one-value lists would otherwise pay one memory round trip per list
        const uint64_t c0 = s > x0 ? s : x0, c1 = min_u64(e, x1);
        const bool small = act && c1 - c0 <= kAppLaneBytes;
        if (small)
        {
            const uint64_t lk = s + kb;
            const uint64_t kp = ksrc - s, np = nsrc - lk; // + b: the source address of byte b of the output, kept / new
            for (uint64_t b0 = c0; b0 < c1; b0 += 8u)
            {
                uint8_t v[8];
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q)
                    v[q] = b0 + q < c1 ? *reinterpret_cast<const uint8_t *>((!NEW || b0 + q < lk ? kp : np) + b0 + q) : uint8_t(0);
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q)
                    if (b0 + q < c1)
                        out[b0 + q] = v[q];
            }
        }
        uint64_t mask = __ballot(act && !small);
        while (mask != 0ull)
        {
            const uint32_t l = static_cast<uint32_t>(__builtin_ctzll(mask));
            mask &= mask - 1ull;
            const uint64_t ls = readlane_u64(s, l), le = readlane_u64(e, l);
            const uint64_t lk = ls + readlane_u64(kb, l); // the kept bytes end, the new ones begin
            // the kept bytes, clipped to the tile
            uint64_t w0 = ls > x0 ? ls : x0, w1 = min_u64(lk, x1);
            if (w0 < w1)
                wave_move(out + w0, reinterpret_cast<const uint8_t *>(readlane_u64(ksrc, l)) + (w0 - ls), static_cast<uint32_t>(w1 - w0), t);
            w0 = lk > x0 ? lk : x0, w1 = min_u64(le, x1);
            if (NEW && w0 < w1)
                wave_move(out + w0, reinterpret_cast<const uint8_t *>(readlane_u64(nsrc, l)) + (w0 - lk), static_cast<uint32_t>(w1 - w0), t);
        }
        // the batch's end: past the tile, or the last list
        const uint64_t be = jb + 64u <= n ? lstart[jb + 64u] : total;
        if (jb + 64u >= n || be >= x1)
            break;
        jb += 64u;
    }
}

// The append's and the remove's lists: Args (AppArgs, RemArgs) names the old
// index ix and, per list j of the result, kbpre[j] (n + 1) the kept bytes of
// the lists before it, its kept bytes at ix.in + ix.off[ix.list_unit[j]], its
// new bytes at sbytes + noff[subase[j]].
template <class Args>
__device__ __forceinline__ void stitch_tile(const Args & A, uint64_t nlists_out)
{
    stitch_tile<true>(A.hdr, A.lstart, nlists_out, A.out, [&A](uint32_t j, uint64_t, uint64_t & kb, uint64_t & ksrc, uint64_t & nsrc) {
        kb = A.kbpre[j + 1u] - A.kbpre[j];
        if (kb != 0ull)
            ksrc = reinterpret_cast<uint64_t>(A.ix.in) + A.ix.off[A.ix.list_unit[j]];
        nsrc = reinterpret_cast<uint64_t>(A.sbytes) + A.noff[A.subase[j]];
    });
}

} // namespace tpf::dev
