// tpf_ws.h -- how every launcher lays out a device workspace (internal, host):
// arrays that start 256-byte aligned, handed out in order by one carver.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace tpf
{

inline size_t al256(size_t x) { return (x + 255u) & ~size_t(255); }

// workspace of the run scan (p4_scan.h): T prefixes over run totals of Tot
template <class T, class Tot = uint32_t>
struct RunScanWs;

// Hands out consecutive arrays of a workspace, each starting 256-byte aligned;
// `used` is the size of everything handed out so far (a null base: sizes only).
struct WsCarver
{
    uint8_t * base;
    size_t used = 0;

    explicit WsCarver(const void * ws) : base(static_cast<uint8_t *>(const_cast<void *>(ws))) {}

    template <class T>
    T * bytes(size_t nbytes)
    {
        T * r = reinterpret_cast<T *>(base + used);
        used += al256(nbytes);
        return r;
    }
    template <class T>
    T * take(uint64_t count)
    {
        return bytes<T>(sizeof(T) * count);
    }
    template <class T, class Tot = uint32_t>
    RunScanWs<T, Tot> scan(uint64_t nruns)
    {
        return RunScanWs<T, Tot>::carve(bytes<uint8_t>(RunScanWs<T, Tot>::bytes(nruns)), nruns);
    }
};

} // namespace tpf
