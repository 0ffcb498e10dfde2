// tpf_fmt.h -- facts about the format ids (TPF_FMT_*, include/turbopfor_gpu.h)
// that the host entry points share (internal; defined in capi.cpp).
#pragma once

#include <stddef.h>

namespace tpf
{

// (fmt, n) pairs the batch entry points accept (also checked by the host
// streams before they cut a batch into shards)
bool fmt_ok(int fmt, unsigned n);
// values a unit of n values occupies in a batch's value array (the vertical
// formats store whole units)
unsigned unit_values(int fmt, unsigned n);
// 64-bit values
bool wide_fmt(int fmt);

// bytes of one value and of one unit's values
struct UnitBytes
{
    size_t es, vbytes;
};
inline UnitBytes unit_bytes(int fmt, unsigned n)
{
    const size_t es = wide_fmt(fmt) ? 8 : 4;
    return {es, es * unit_values(fmt, n)};
}

} // namespace tpf
