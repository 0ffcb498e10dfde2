// capi.cpp -- extern "C" entry points of include/turbopfor_gpu.h.
// Argument checking, error reporting and launch sizing; the kernels live in
// the *.hip files.  There is deliberately no CPU fallback: without a HIP
// device every entry point fails with TPF_ENODEV.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>

#include "../../include/turbopfor_gpu.h"
#include "p4_lists.h"
#include "tpf_fmt.h"
#include "tpf_kernels.h"

#include <algorithm>

namespace
{
thread_local std::string g_err;

int fail(int code, const std::string & msg)
{
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char * where)
{
    return fail(TPF_EHIP, std::string(where) + ": " + hipGetErrorString(e));
}

int check_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(TPF_ENODEV, "no HIP device visible (turbopfor_amd has no CPU fallback)");
    return TPF_OK;
}

// d_err handling: init to UINT64_MAX before the kernel.
int prep_err(uint64_t * d_err, hipStream_t s)
{
    if (!d_err)
        return TPF_OK;
    hipError_t e = tpf::fill_u32(d_err, 0xFFFFFFFFu, 2, s);
    return e == hipSuccess ? TPF_OK : hip_fail(e, "init d_err");
}

// The stream of an entry point that resets d_err itself, opened by that reset.
int open_stream(void * stream, uint64_t * d_err, hipStream_t & s)
{
    s = static_cast<hipStream_t>(stream);
    return prep_err(d_err, s);
}

// The same for an entry point that judges its arguments before it looks for the device.
int open_device_stream(void * stream, uint64_t * d_err, hipStream_t & s)
{
    if (int rc = check_device())
        return rc;
    return open_stream(stream, d_err, s);
}

// d_err as the launchers take it.
unsigned long long * dev_err(uint64_t * d_err) { return reinterpret_cast<unsigned long long *>(d_err); }

// The epilogue of an entry point: its launcher's verdict as the return value.
int done(hipError_t e, const char * name) { return e == hipSuccess ? TPF_OK : hip_fail(e, name); }

// A count above the limit of the lists entry points, whose kernels index with
// 32 bits.  The refusal's message, which names the counts, stays with the caller.
bool over_limit(std::initializer_list<uint64_t> counts)
{
    for (uint64_t c : counts)
        if (c > 0x7FFFFFFFull)
            return true;
    return false;
}

// The resident index of an entry point, its arguments in the public order: a
// plain stream (d1 == 0) has neither starts nor a skip table, whatever the
// caller passed.
tpf::ListsIndex lists_index(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                            const uint32_t * d_list_unit, uint64_t nlists, int d1, const uint32_t * d_start0, const uint32_t * d_unit_last)
{
    return tpf::ListsIndex{.in = d_in,
                           .in_bytes = in_bytes,
                           .off = d_off,
                           .nunits = nunits,
                           .ptr = d_list_ptr,
                           .list_unit = d_list_unit,
                           .nlists = nlists,
                           .start0 = d1 ? d_start0 : nullptr,
                           .unit_last = d1 ? d_unit_last : nullptr};
}
} // namespace

namespace tpf
{
void set_last_error(const std::string & msg) { g_err = msg; }

uint64_t grid_cap(hipStream_t, uint32_t per_cu)
{
    static int cus[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64)
        dev = 0;
    if (cus[dev] == 0)
    {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        cus[dev] = n;
    }
    return static_cast<uint64_t>(cus[dev]) * per_cu;
}
} // namespace tpf

extern "C" {

const char * tpf_last_error(void) { return g_err.c_str(); }

int tpf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int tpf_p4dec256v32_batch(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nblocks, uint32_t * d_out,
                          uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (nblocks && (!d_in || !d_off || !d_out))
        return fail(TPF_EINVAL, "tpf_p4dec256v32_batch: null pointer");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_dec256v32(d_in, in_bytes, d_off, nblocks, d_out, nullptr, dev_err(d_err), s), "tpf_p4dec256v32_batch");
}

int tpf_p4d1dec256v32_batch(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nblocks, uint32_t * d_out,
                            const uint32_t * d_starts, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (nblocks && (!d_in || !d_off || !d_out || !d_starts))
        return fail(TPF_EINVAL, "tpf_p4d1dec256v32_batch: null pointer");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_dec256v32(d_in, in_bytes, d_off, nblocks, d_out, d_starts, dev_err(d_err), s), "tpf_p4d1dec256v32_batch");
}

size_t tpf_p4d1dec256v32_chain_workspace_size(uint64_t nblocks) { return tpf::d1chain_workspace(nblocks); }

int tpf_p4d1dec256v32_chain_sums(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nblocks, void * d_ws,
                                 size_t ws_bytes, uint32_t * d_total, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (nblocks && (!d_in || !d_off || !d_ws))
        return fail(TPF_EINVAL, "tpf_p4d1dec256v32_chain_sums: null pointer");
    if (ws_bytes < tpf_p4d1dec256v32_chain_workspace_size(nblocks))
        return fail(TPF_EINVAL, "tpf_p4d1dec256v32_chain_sums: workspace too small");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_d1chain_sums(d_in, in_bytes, d_off, nblocks, d_ws, ws_bytes, d_total, dev_err(d_err), s),
                "tpf_p4d1dec256v32_chain_sums");
}

int tpf_p4d1dec256v32_chain_decode(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nblocks, uint32_t * d_out,
                                   uint32_t base, const void * d_ws, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (nblocks && (!d_in || !d_off || !d_out || !d_ws))
        return fail(TPF_EINVAL, "tpf_p4d1dec256v32_chain_decode: null pointer");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_d1chain_decode(d_in, in_bytes, d_off, nblocks, d_out, d_ws, base, dev_err(d_err), s),
                "tpf_p4d1dec256v32_chain_decode");
}

int tpf_p4d1dec256v32_chained(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nblocks, uint32_t * d_out,
                              uint32_t start0, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    // Two phases (block sums + scan, then decode).  A one-launch variant
    // (per-run sum pass, decoupled look-back, decode pass) measured 335 vs
    // 580 G int32/s on C3 and was dropped.
    if (int rc = tpf_p4d1dec256v32_chain_sums(d_in, in_bytes, d_off, nblocks, d_ws, ws_bytes, nullptr, d_err, stream))
        return rc;
    // phase B re-checks lengths; keep the first error index from phase A
    return tpf_p4d1dec256v32_chain_decode(d_in, in_bytes, d_off, nblocks, d_out, start0, d_ws, nullptr, stream);
}

// ---- 64-bit chained delta-1 decode (128v64 / 256v64 units) ----------------
static int chain64_nb(int fmt) { return fmt == TPF_FMT_256V64 ? 2 : fmt == TPF_FMT_128V64 ? 1 : 0; }

size_t tpf_d1dec64_chain_workspace_size(uint64_t nunits) { return tpf::d1chain64_workspace(nunits); }

int tpf_d1dec64_chain_sums(int fmt, const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, void * d_ws,
                           size_t ws_bytes, uint64_t * d_total, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    const int nb = chain64_nb(fmt);
    if (!nb)
        return fail(TPF_EINVAL, "tpf_d1dec64_chain_sums: fmt must be TPF_FMT_128V64 or TPF_FMT_256V64");
    if (nunits && (!d_in || !d_off || !d_ws))
        return fail(TPF_EINVAL, "tpf_d1dec64_chain_sums: null pointer");
    if (ws_bytes < tpf_d1dec64_chain_workspace_size(nunits))
        return fail(TPF_EINVAL, "tpf_d1dec64_chain_sums: workspace too small");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_d1chain64_sums(static_cast<uint32_t>(nb), d_in, in_bytes, d_off, nunits, d_ws, ws_bytes, d_total,
                                           dev_err(d_err), s), "tpf_d1dec64_chain_sums");
}

int tpf_d1dec64_chain_decode(int fmt, const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, uint64_t * d_out,
                             uint64_t base, const void * d_ws, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    const int nb = chain64_nb(fmt);
    if (!nb)
        return fail(TPF_EINVAL, "tpf_d1dec64_chain_decode: fmt must be TPF_FMT_128V64 or TPF_FMT_256V64");
    if (nunits && (!d_in || !d_off || !d_out || !d_ws))
        return fail(TPF_EINVAL, "tpf_d1dec64_chain_decode: null pointer");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_d1chain64_decode(static_cast<uint32_t>(nb), d_in, in_bytes, d_off, nunits, d_out, d_ws, base, dev_err(d_err),
                                             s), "tpf_d1dec64_chain_decode");
}

int tpf_d1dec64_chained(int fmt, const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, uint64_t * d_out,
                        uint64_t start0, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (int rc = tpf_d1dec64_chain_sums(fmt, d_in, in_bytes, d_off, nunits, d_ws, ws_bytes, nullptr, d_err, stream))
        return rc;
    // phase B re-checks lengths; keep the first error index from phase A
    return tpf_d1dec64_chain_decode(fmt, d_in, in_bytes, d_off, nunits, d_out, start0, d_ws, nullptr, stream);
}

int tpf_p4d1dec256v64_chained(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, uint64_t * d_out,
                              uint64_t start0, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    return tpf_d1dec64_chained(TPF_FMT_256V64, d_in, in_bytes, d_off, nunits, d_out, start0, d_ws, ws_bytes, d_err, stream);
}

int tpf_p4d1dec128v64_chained(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, uint64_t * d_out,
                              uint64_t start0, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    return tpf_d1dec64_chained(TPF_FMT_128V64, d_in, in_bytes, d_off, nunits, d_out, start0, d_ws, ws_bytes, d_err, stream);
}

uint64_t tpf_p4enc256v32_bound(uint64_t nblocks) { return nblocks * 1800u + 64u; }

size_t tpf_p4enc256v32_workspace_size(uint64_t nblocks) { return tpf::enc256v32_workspace(nblocks); }

static int enc256v32_common(const uint32_t * d_in, uint64_t nblocks, const uint32_t * d_starts, uint32_t start0, bool d1,
                            uint8_t * d_out, uint64_t out_cap, uint64_t * d_off, void * d_ws, size_t ws_bytes, void * stream,
                            const char * name)
{
    if (int rc = check_device())
        return rc;
    if (!d_off || (nblocks && (!d_in || !d_out || !d_ws)))
        return fail(TPF_EINVAL, std::string(name) + ": null pointer");
    if (ws_bytes < tpf::enc256v32_workspace(nblocks))
        return fail(TPF_EINVAL, std::string(name) + ": workspace too small");
    // the encoded sizes are known only on the device: the caller's capacity
    // must cover the worst case, or a block could be cut off unreported
    if (nblocks && out_cap < tpf_p4enc256v32_bound(nblocks))
        return fail(TPF_EINVAL, std::string(name) + ": out_cap below tpf_p4enc256v32_bound(nblocks)");
    return done(tpf::launch_enc256v32(d_in, nblocks, d_starts, start0, d1, d_out, out_cap, d_off, d_ws, ws_bytes,
                                      static_cast<hipStream_t>(stream)), name);
}

int tpf_p4enc256v32_batch(const uint32_t * d_in, uint64_t nblocks, uint8_t * d_out, uint64_t out_cap, uint64_t * d_off, void * d_ws,
                          size_t ws_bytes, void * stream)
{
    return enc256v32_common(d_in, nblocks, nullptr, 0, false, d_out, out_cap, d_off, d_ws, ws_bytes, stream, "tpf_p4enc256v32_batch");
}

int tpf_p4d1enc256v32_batch(const uint32_t * d_in, uint64_t nblocks, const uint32_t * d_starts, uint32_t start0, uint8_t * d_out,
                            uint64_t out_cap, uint64_t * d_off, void * d_ws, size_t ws_bytes, void * stream)
{
    return enc256v32_common(d_in, nblocks, d_starts, start0, true, d_out, out_cap, d_off, d_ws, ws_bytes, stream,
                            "tpf_p4d1enc256v32_batch");
}

extern "C++" {
namespace tpf
{
// the format facts of tpf_fmt.h
bool fmt_ok(int fmt, unsigned n)
{
    switch (fmt)
    {
        case TPF_FMT_32:
        case TPF_FMT_64:
            return n >= 1 && n <= 256;
        case TPF_FMT_128V32:
            return n >= 1 && n <= 128;
        case TPF_FMT_256V32:
            return n >= 1 && n <= 256;
        case TPF_FMT_128V64: // n < 128: bitmap of pad8(n), exceptions over n values, full-width base
            return n >= 1 && n <= 128;
        case TPF_FMT_256V64: // batches of 256v64 units hold full units (the per-block API splits n < 256)
            return n == 256;
        default:
            return false;
    }
}
bool wide_fmt(int fmt) { return fmt == TPF_FMT_64 || fmt == TPF_FMT_128V64 || fmt == TPF_FMT_256V64; }

unsigned unit_values(int fmt, unsigned n)
{
    switch (fmt)
    {
        case TPF_FMT_128V32:
        case TPF_FMT_128V64:
            return 128;
        case TPF_FMT_256V32:
        case TPF_FMT_256V64:
            return 256;
        default:
            return n;
    }
}
} // namespace tpf
}
using tpf::fmt_ok;
using tpf::unit_values;

uint64_t tpf_enc_bound(int fmt, uint64_t nblocks, unsigned n)
{
    return nblocks * (64u + (tpf::wide_fmt(fmt) ? 18u : 8u) * unit_values(fmt, n)) + 64u;
}

size_t tpf_enc_workspace_size(int fmt, uint64_t nblocks, unsigned n)
{
    if (fmt == TPF_FMT_256V32 && n == 256)
        return tpf::enc256v32_workspace(nblocks);
    if ((fmt == TPF_FMT_128V64 && n == 128) || fmt == TPF_FMT_256V64)
        return tpf::enc128v64_workspace(nblocks);
    return tpf::generic_workspace(nblocks);
}

int tpf_dec_batch(int fmt, const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nblocks, unsigned n, void * d_vals,
                  const void * d_starts, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (!fmt_ok(fmt, n))
        return fail(TPF_EINVAL, "tpf_dec_batch: unsupported (fmt, n)");
    if (nblocks && (!d_in || !d_off || !d_vals))
        return fail(TPF_EINVAL, "tpf_dec_batch: null pointer");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    hipError_t e;
    if (fmt == TPF_FMT_256V32 && n == 256)
        e = tpf::launch_dec256v32(d_in, in_bytes, d_off, nblocks, static_cast<uint32_t *>(d_vals),
                                  static_cast<const uint32_t *>(d_starts), dev_err(d_err), s);
    else
        e = tpf::launch_dec_generic(fmt, d_in, in_bytes, d_off, nblocks, n, d_vals, d_starts,
                                    dev_err(d_err), s);
    return done(e, "tpf_dec_batch");
}

int tpf_enc_batch(int fmt, const void * d_vals, uint64_t nblocks, unsigned n, int d1, const void * d_starts, uint64_t start0,
                  uint8_t * d_out, uint64_t out_cap, uint64_t * d_off, void * d_ws, size_t ws_bytes, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (!fmt_ok(fmt, n))
        return fail(TPF_EINVAL, "tpf_enc_batch: unsupported (fmt, n)");
    if (!d_off || (nblocks && (!d_vals || !d_out || !d_ws)))
        return fail(TPF_EINVAL, "tpf_enc_batch: null pointer");
    if (ws_bytes < tpf_enc_workspace_size(fmt, nblocks, n))
        return fail(TPF_EINVAL, "tpf_enc_batch: workspace too small");
    if (nblocks && out_cap < tpf_enc_bound(fmt, nblocks, n))
        return fail(TPF_EINVAL, "tpf_enc_batch: out_cap below tpf_enc_bound(fmt, nblocks, n)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (fmt == TPF_FMT_256V32 && n == 256)
        e = tpf::launch_enc256v32(static_cast<const uint32_t *>(d_vals), nblocks, static_cast<const uint32_t *>(d_starts),
                                  static_cast<uint32_t>(start0), d1 != 0, d_out, out_cap, d_off, d_ws, ws_bytes, s);
    else if ((fmt == TPF_FMT_128V64 && n == 128) || fmt == TPF_FMT_256V64)
        e = tpf::launch_enc128v64(fmt == TPF_FMT_256V64 ? 2u : 1u, static_cast<const uint64_t *>(d_vals), nblocks, d1 != 0,
                                  static_cast<const uint64_t *>(d_starts), start0, d_out, out_cap, d_off, d_ws, ws_bytes, s);
    else
        e = tpf::launch_enc_generic(fmt, d_vals, nblocks, n, d1 != 0, d_starts, start0, d_out, out_cap, d_off, d_ws, ws_bytes, s);
    return done(e, "tpf_enc_batch");
}

// ---- n-variant streams: floor(n/256) 256v32 blocks + one
// p4Enc32 tail block.  Workspace: [0,256) scalars (tail start, tail error,
// tail offsets), then the tail's scratch image (encode), then the
// sub-call's own workspace.
static constexpr size_t kNHead = 256;

static size_t ntail_image(uint64_t) { return (tpf_enc_bound(TPF_FMT_32, 1, 256) + 255) & ~size_t(255); }

uint64_t tpf_p4nenc256v32_bound(uint64_t n) { return tpf_p4enc256v32_bound(n / 256) + tpf_enc_bound(TPF_FMT_32, 1, 256); }

size_t tpf_p4nenc256v32_workspace_size(uint64_t n)
{
    const size_t full = tpf::enc256v32_workspace(n / 256), tail = tpf_enc_workspace_size(TPF_FMT_32, 1, 256);
    return kNHead + ntail_image(n) + (full > tail ? full : tail);
}

int tpf_p4nenc256v32(const uint32_t * d_in, uint64_t n, int d1, uint32_t start0, uint8_t * d_out, uint64_t out_cap, uint64_t * d_off,
                     void * d_ws, size_t ws_bytes, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (!d_off || (n && (!d_in || !d_out || !d_ws)))
        return fail(TPF_EINVAL, "tpf_p4nenc256v32: null pointer");
    if (ws_bytes < tpf_p4nenc256v32_workspace_size(n))
        return fail(TPF_EINVAL, "tpf_p4nenc256v32: workspace too small");
    if (n && out_cap < tpf_p4nenc256v32_bound(n)) // the tail lands at an offset only the device knows
        return fail(TPF_EINVAL, "tpf_p4nenc256v32: out_cap below tpf_p4nenc256v32_bound(n)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nfull = n / 256;
    const unsigned tail = static_cast<unsigned>(n % 256);
    uint8_t * ws = static_cast<uint8_t *>(d_ws);
    uint8_t * sub_ws = ws + kNHead + ntail_image(n);
    const size_t sub_bytes = ws_bytes - kNHead - ntail_image(n);
    if (nfull || !tail)
        if (int rc = enc256v32_common(d_in, nfull, nullptr, start0, d1 != 0, d_out, out_cap, d_off, sub_ws, sub_bytes, stream,
                                      "tpf_p4nenc256v32"))
            return rc;
    if (!tail)
        return TPF_OK;
    // D1 tail: its start is the last value of the full blocks (device) or start0
    const uint32_t * starts = (d1 && nfull) ? d_in + nfull * 256 - 1 : nullptr;
    if (!nfull) // the whole stream is the tail block
        return tpf_enc_batch(TPF_FMT_32, d_in, 1, tail, d1, nullptr, start0, d_out, out_cap, d_off, sub_ws, sub_bytes, stream);
    uint64_t * tail_off = reinterpret_cast<uint64_t *>(ws + 16);
    uint8_t * img = ws + kNHead;
    if (int rc = tpf_enc_batch(TPF_FMT_32, d_in + nfull * 256, 1, tail, d1, starts, start0, img, ntail_image(n), tail_off, sub_ws,
                               sub_bytes, stream))
        return rc;
    return done(tpf::launch_append(d_out, img, d_off + nfull, tail_off + 1, d_off + nfull + 1, s), "tpf_p4nenc256v32");
}

size_t tpf_p4ndec256v32_workspace_size(uint64_t n) { return kNHead + tpf_p4d1dec256v32_chain_workspace_size(n / 256); }

int tpf_p4ndec256v32(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t n, int d1, uint32_t start0,
                     uint32_t * d_out, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (n && (!d_in || !d_off || !d_out || !d_ws))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32: null pointer");
    if (ws_bytes < tpf_p4ndec256v32_workspace_size(n))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nfull = n / 256;
    const unsigned tail = static_cast<unsigned>(n % 256);
    uint8_t * ws = static_cast<uint8_t *>(d_ws);
    if (nfull)
    {
        int rc = d1 ? tpf_p4d1dec256v32_chained(d_in, in_bytes, d_off, nfull, d_out, start0, ws + kNHead, ws_bytes - kNHead, d_err, stream)
                    : tpf_p4dec256v32_batch(d_in, in_bytes, d_off, nfull, d_out, d_err, stream);
        if (rc)
            return rc;
    }
    else if (int rc = prep_err(d_err, s))
        return rc;
    if (!tail)
        return TPF_OK;
    uint32_t * start = reinterpret_cast<uint32_t *>(ws);
    const uint32_t * starts = nullptr;
    if (d1)
    {
        if (nfull)
            starts = d_out + nfull * 256 - 1;
        else
        {
            hipError_t e = tpf::fill_u32(start, start0, 1, s);
            if (e != hipSuccess)
                return hip_fail(e, "tpf_p4ndec256v32");
            starts = start;
        }
    }
    uint64_t * tail_err = d_err ? reinterpret_cast<uint64_t *>(ws + 8) : nullptr;
    if (int rc = tpf_dec_batch(TPF_FMT_32, d_in, in_bytes, d_off + nfull, 1, tail, d_out + nfull * 256, starts, tail_err, stream))
        return rc;
    if (!d_err)
        return TPF_OK;
    return done(tpf::launch_err_merge(dev_err(d_err), reinterpret_cast<unsigned long long *>(tail_err), nfull, s), "tpf_p4ndec256v32");
}

// ---- many lists in one call: each list an n-variant stream, laid end to end
size_t tpf_p4ndec256v32_lists_workspace_size(uint64_t nunits, uint64_t nlists) { return tpf::lists_workspace(nunits, nlists); }

int tpf_p4ndec256v32_lists(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                           uint64_t nlists, int d1, const uint32_t * d_start0, uint32_t * d_out, uint64_t out_values, void * d_ws,
                           size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (nunits && nlists && (!d_in || !d_off || !d_list_ptr || !d_out || !d_ws))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists: null pointer");
    if (nunits && nlists && ws_bytes < tpf_p4ndec256v32_lists_workspace_size(nunits, nlists))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists: workspace too small");
    if (over_limit({nunits, nlists}))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists: nunits and nlists are limited to 0x7FFFFFFF");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, nullptr, nlists, d1, d_start0, nullptr);
    return done(tpf::launch_lists_dec(X, d1 != 0, d_out, out_values, d_ws, dev_err(d_err), s), "tpf_p4ndec256v32_lists");
}

// The per-unit bounds (1800 B per full block, tpf_enc_bound(TPF_FMT_32, 1, r)
// = 128 + 8 r per tail of r values) summed over the worst partition: a full
// block costs at most 8 B per value, so a stream of K full blocks and T tails
// is bounded by 8 nvalues - 248 K + 128 T; T <= min(nlists, nvalues) and the T
// tails hold at most 255 T values, so K >= (nvalues - 255 T) / 256, taken
// without rounding up ((x - 255) / 256 <= ceil(x / 256)) so that the bound
// never decreases with nvalues (the exact maximum does: one list of 255
// values is bounded by 2,168 B, of 256 by 1,800).
uint64_t tpf_p4nenc256v32_lists_bound(uint64_t nvalues, uint64_t nlists)
{
    const uint64_t T = std::min(nlists, nvalues);
    const uint64_t x = nvalues > 255u * T ? nvalues - 255u * T : 0u;
    const uint64_t k256 = x > 255u ? x - 255u : 0u; // 256 x the full blocks no partition can avoid
    return 8u * nvalues + 128u * T - (248u * k256) / 256u + 64u;
}

size_t tpf_p4nenc256v32_lists_workspace_size(uint64_t nunits, uint64_t nlists) { return tpf::lists_enc_workspace(nunits, nlists); }

int tpf_p4nenc256v32_lists(const uint32_t * d_in, uint64_t in_values, const uint64_t * d_list_ptr, uint64_t nlists, int d1,
                           const uint32_t * d_start0, uint8_t * d_out, uint64_t out_cap, uint64_t * d_off, uint64_t nunits, void * d_ws,
                           size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (nlists && (!d_list_ptr || !d_off || !d_ws))
        return fail(TPF_EINVAL, "tpf_p4nenc256v32_lists: null pointer");
    if (nlists && nunits && (!d_in || !d_out))
        return fail(TPF_EINVAL, "tpf_p4nenc256v32_lists: null pointer");
    if (over_limit({nunits, nlists}))
        return fail(TPF_EINVAL, "tpf_p4nenc256v32_lists: nunits and nlists are limited to 0x7FFFFFFF");
    if (nlists && ws_bytes < tpf_p4nenc256v32_lists_workspace_size(nunits, nlists))
        return fail(TPF_EINVAL, "tpf_p4nenc256v32_lists: workspace too small");
    hipStream_t s;
    if (int rc = open_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_lists_enc(d_in, in_values, d_list_ptr, nlists, d1 != 0, d1 ? d_start0 : nullptr, d_out, out_cap, d_off, nunits,
                                      d_ws, dev_err(d_err), s), "tpf_p4nenc256v32_lists");
}

// ---- the read side of a resident index: the unit directory and the decode of
// a selection of lists.  Arguments are judged before the device is looked for.
size_t tpf_lists_unit_base_workspace_size(uint64_t nlists) { return tpf::lists_unit_base_workspace(nlists); }

int tpf_lists_unit_base(const uint64_t * d_list_ptr, uint64_t nlists, uint32_t * d_list_unit, void * d_ws, size_t ws_bytes, uint64_t * d_err,
                        void * stream)
{
    if (over_limit({nlists}))
        return fail(TPF_EINVAL, "tpf_lists_unit_base: nlists is limited to 0x7FFFFFFF");
    if (!d_list_unit || (nlists && (!d_list_ptr || !d_ws)))
        return fail(TPF_EINVAL, "tpf_lists_unit_base: null pointer");
    if (nlists && ws_bytes < tpf_lists_unit_base_workspace_size(nlists))
        return fail(TPF_EINVAL, "tpf_lists_unit_base: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_lists_unit_base(d_list_ptr, nlists, d_list_unit, d_ws, dev_err(d_err), s), "tpf_lists_unit_base");
}

// ---- the way in for a stream without offsets: the unit offsets from the
// lists' byte spans and the units' headers.
size_t tpf_lists_unit_offsets_workspace_size(uint64_t nunits, uint64_t nlists) { return tpf::lists_unit_offsets_workspace(nunits, nlists); }

int tpf_lists_unit_offsets(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_list_ptr, const uint64_t * d_list_byte,
                           uint64_t nlists, uint64_t * d_off, uint64_t nunits, uint32_t * d_list_unit, void * d_ws, size_t ws_bytes,
                           uint64_t * d_err, void * stream)
{
    if (over_limit({nunits, nlists}))
        return fail(TPF_EINVAL, "tpf_lists_unit_offsets: nunits and nlists are limited to 0x7FFFFFFF");
    if (!d_off || (nlists && (!d_list_ptr || !d_list_byte || !d_ws)) || (nunits && !d_in))
        return fail(TPF_EINVAL, "tpf_lists_unit_offsets: null pointer");
    if (nlists && ws_bytes < tpf_lists_unit_offsets_workspace_size(nunits, nlists))
        return fail(TPF_EINVAL, "tpf_lists_unit_offsets: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_lists_unit_offsets(d_in, in_bytes, d_list_ptr, d_list_byte, nlists, d_off, nunits, d_list_unit, d_ws,
                                               dev_err(d_err), s), "tpf_lists_unit_offsets");
}

size_t tpf_p4ndec256v32_lists_select_workspace_size(uint64_t nsel, uint64_t out_values)
{
    return tpf::lists_select_workspace(nsel, out_values);
}

int tpf_p4ndec256v32_lists_select(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits,
                                  const uint64_t * d_list_ptr, const uint32_t * d_list_unit, uint64_t nlists, int d1,
                                  const uint32_t * d_start0, const uint32_t * d_sel, uint64_t nsel, uint32_t * d_out, uint64_t out_values,
                                  uint64_t * d_out_ptr, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (over_limit({nlists, nunits, nsel, nsel ? tpf::lists_select_unit_cap(nsel, out_values) : 0u}))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists_select: nlists, nunits, nsel and out_values / 256 + nsel are limited to 0x7FFFFFFF");
    if (nsel && (!d_sel || !d_out_ptr || !d_in || !d_off || !d_list_ptr || !d_list_unit || !d_out || !d_ws))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists_select: null pointer");
    if (nsel && ws_bytes < tpf_p4ndec256v32_lists_select_workspace_size(nsel, out_values))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists_select: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d1, d_start0, nullptr);
    return done(tpf::launch_lists_select(X, d1 != 0, d_sel, nsel, d_out, out_values, d_out_ptr, d_ws, dev_err(d_err), s),
                "tpf_p4ndec256v32_lists_select");
}

// ---- block-range reads of a resident index: the skip table, the range search
// and the decode of unit ranges.  Arguments are judged before the device is
// looked for.
size_t tpf_lists_unit_last_workspace_size(uint64_t nunits, uint64_t nlists) { return tpf::lists_unit_last_workspace(nunits, nlists); }

int tpf_lists_unit_last(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                        uint64_t nlists, const uint32_t * d_start0, uint32_t * d_unit_last, void * d_ws, size_t ws_bytes, uint64_t * d_err,
                        void * stream)
{
    if (over_limit({nunits, nlists}))
        return fail(TPF_EINVAL, "tpf_lists_unit_last: nunits and nlists are limited to 0x7FFFFFFF");
    if (nunits && nlists && (!d_in || !d_off || !d_list_ptr || !d_unit_last || !d_ws))
        return fail(TPF_EINVAL, "tpf_lists_unit_last: null pointer");
    if (nunits && nlists && ws_bytes < tpf_lists_unit_last_workspace_size(nunits, nlists))
        return fail(TPF_EINVAL, "tpf_lists_unit_last: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, nullptr, nlists, 1, d_start0, nullptr);
    return done(tpf::launch_lists_unit_last(X, d_unit_last, d_ws, dev_err(d_err), s), "tpf_lists_unit_last");
}

int tpf_lists_range_units(const uint32_t * d_list_unit, const uint32_t * d_unit_last, uint64_t nlists, uint64_t nunits,
                          const uint32_t * d_qlist, const uint32_t * d_qlo, const uint32_t * d_qhi, uint64_t nq, uint32_t * d_ufirst,
                          uint32_t * d_ucount, uint64_t * d_err, void * stream)
{
    if (over_limit({nlists, nunits, nq}))
        return fail(TPF_EINVAL, "tpf_lists_range_units: nlists, nunits and nq are limited to 0x7FFFFFFF");
    if (nq && (!d_list_unit || !d_unit_last || !d_qlist || !d_qlo || !d_qhi || !d_ufirst || !d_ucount))
        return fail(TPF_EINVAL, "tpf_lists_range_units: null pointer");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    return done(tpf::launch_lists_range_units(d_list_unit, d_unit_last, nlists, nunits, d_qlist, d_qlo, d_qhi, nq, d_ufirst, d_ucount,
                                              dev_err(d_err), s), "tpf_lists_range_units");
}

size_t tpf_p4ndec256v32_lists_units_workspace_size(uint64_t nsel, uint64_t out_values)
{
    return tpf::lists_units_workspace(nsel, out_values);
}

int tpf_p4ndec256v32_lists_units(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits,
                                 const uint64_t * d_list_ptr, const uint32_t * d_list_unit, uint64_t nlists, int d1,
                                 const uint32_t * d_start0, const uint32_t * d_unit_last, const uint32_t * d_sel,
                                 const uint32_t * d_ufirst, const uint32_t * d_ucount, uint64_t nsel, uint32_t * d_out, uint64_t out_values,
                                 uint64_t * d_out_ptr, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (over_limit({nlists, nunits, nsel, nsel ? tpf::lists_select_unit_cap(nsel, out_values) : 0u}))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists_units: nlists, nunits, nsel and out_values / 256 + nsel are limited to 0x7FFFFFFF");
    if (nsel && (!d_sel || !d_ufirst || !d_ucount || !d_out_ptr || !d_in || !d_off || !d_list_ptr || !d_list_unit || !d_out || !d_ws))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists_units: null pointer");
    if (nsel && d1 && !d_unit_last)
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists_units: null d_unit_last (delta-1 needs the skip table of tpf_lists_unit_last)");
    if (nsel && ws_bytes < tpf_p4ndec256v32_lists_units_workspace_size(nsel, out_values))
        return fail(TPF_EINVAL, "tpf_p4ndec256v32_lists_units: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d1, d_start0, d_unit_last);
    return done(tpf::launch_lists_units(X, d1 != 0, d_sel, d_ufirst, d_ucount, nsel, d_out, out_values, d_out_ptr, d_ws, dev_err(d_err), s),
                "tpf_p4ndec256v32_lists_units");
}

// ---- the probe calls on a resident index: intersection, union, difference.
// The three take the same arguments and judge them in the same order: one body,
// and per entry point its name, its launcher, its workspace size and the
// refusal of a count above its limits.  Only the union is sized by out_values.
size_t tpf_lists_intersect_workspace_size(uint64_t nq, uint64_t probe_values) { return tpf::lists_intersect_workspace(nq, probe_values); }

size_t tpf_lists_union_workspace_size(uint64_t nq, uint64_t probe_values, uint64_t out_values)
{
    return tpf::lists_union_workspace(nq, probe_values, out_values);
}

size_t tpf_lists_difference_workspace_size(uint64_t nq, uint64_t probe_values) { return tpf::lists_difference_workspace(nq, probe_values); }

enum ProbeOp { kIntersect, kUnion, kDifference };

static const struct
{
    const char * name;
    decltype(&tpf::launch_lists_intersect) launch;
    size_t (*ws_size)(uint64_t nq, uint64_t probe_values, uint64_t out_values);
    const char * limits;
} kProbeOps[] = {
    {"tpf_lists_intersect", tpf::launch_lists_intersect,
     [](uint64_t nq, uint64_t pv, uint64_t) { return tpf::lists_intersect_workspace(nq, pv); },
     "tpf_lists_intersect: nlists, nunits, nq and probe_values are limited to 0x7FFFFFFF"},
    {"tpf_lists_union", tpf::launch_lists_union, tpf::lists_union_workspace,
     "tpf_lists_union: nlists, nunits, nq, probe_values and out_values / 256 + nq are limited to 0x7FFFFFFF"},
    {"tpf_lists_difference", tpf::launch_lists_difference,
     [](uint64_t nq, uint64_t pv, uint64_t) { return tpf::lists_difference_workspace(nq, pv); },
     "tpf_lists_difference: nlists, nunits, nq and probe_values are limited to 0x7FFFFFFF"}};

static int lists_probe(ProbeOp op, const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits,
                       const uint64_t * d_list_ptr, const uint32_t * d_list_unit, uint64_t nlists, const uint32_t * d_start0,
                       const uint32_t * d_unit_last, const uint32_t * d_probe, uint64_t probe_values, const uint64_t * d_probe_ptr,
                       const uint32_t * d_qlist, uint64_t nq, uint32_t * d_out, uint64_t out_values, uint64_t * d_out_ptr,
                       uint32_t * d_out_pidx, uint32_t * d_out_tpos, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    const auto & O = kProbeOps[op];
    if (over_limit({nlists, nunits, nq, probe_values, op == kUnion ? tpf::lists_select_unit_cap(nq, out_values) : 0u}))
        return fail(TPF_EINVAL, O.limits);
    if (nq && (!d_in || !d_off || !d_list_ptr || !d_list_unit || !d_unit_last || !d_probe_ptr || !d_qlist || !d_out_ptr || !d_ws))
        return fail(TPF_EINVAL, std::string(O.name) + ": null pointer");
    if ((probe_values && !d_probe) || (out_values && !d_out))
        return fail(TPF_EINVAL, std::string(O.name) + ": null d_probe or d_out with a non-zero size");
    if (nq && ws_bytes < O.ws_size(nq, probe_values, out_values))
        return fail(TPF_EINVAL, std::string(O.name) + ": workspace too small");
    if (int rc = check_device())
        return rc;
    // d_err is reset by the launcher, together with its workspace header
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, 1, d_start0, d_unit_last);
    return done(O.launch(X, d_probe, probe_values, d_probe_ptr, d_qlist, nq, d_out, out_values, d_out_ptr, d_out_pidx, d_out_tpos, d_ws,
                         dev_err(d_err), static_cast<hipStream_t>(stream)),
                O.name);
}

int tpf_lists_intersect(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                        const uint32_t * d_list_unit, uint64_t nlists, const uint32_t * d_start0, const uint32_t * d_unit_last,
                        const uint32_t * d_probe, uint64_t probe_values, const uint64_t * d_probe_ptr, const uint32_t * d_qlist,
                        uint64_t nq, uint32_t * d_out, uint64_t out_values, uint64_t * d_out_ptr, uint32_t * d_out_pidx,
                        uint32_t * d_out_tpos, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    return lists_probe(kIntersect, d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d_start0, d_unit_last, d_probe,
                       probe_values, d_probe_ptr, d_qlist, nq, d_out, out_values, d_out_ptr, d_out_pidx, d_out_tpos, d_ws, ws_bytes, d_err,
                       stream);
}

int tpf_lists_union(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                    const uint32_t * d_list_unit, uint64_t nlists, const uint32_t * d_start0, const uint32_t * d_unit_last,
                    const uint32_t * d_probe, uint64_t probe_values, const uint64_t * d_probe_ptr, const uint32_t * d_qlist,
                    uint64_t nq, uint32_t * d_out, uint64_t out_values, uint64_t * d_out_ptr, uint32_t * d_out_pidx,
                    uint32_t * d_out_tpos, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    return lists_probe(kUnion, d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d_start0, d_unit_last, d_probe,
                       probe_values, d_probe_ptr, d_qlist, nq, d_out, out_values, d_out_ptr, d_out_pidx, d_out_tpos, d_ws, ws_bytes, d_err,
                       stream);
}

int tpf_lists_difference(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                         const uint32_t * d_list_unit, uint64_t nlists, const uint32_t * d_start0, const uint32_t * d_unit_last,
                         const uint32_t * d_probe, uint64_t probe_values, const uint64_t * d_probe_ptr, const uint32_t * d_qlist,
                         uint64_t nq, uint32_t * d_out, uint64_t out_values, uint64_t * d_out_ptr, uint32_t * d_out_pidx,
                         uint32_t * d_out_tpos, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    return lists_probe(kDifference, d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d_start0, d_unit_last, d_probe,
                       probe_values, d_probe_ptr, d_qlist, nq, d_out, out_values, d_out_ptr, d_out_pidx, d_out_tpos, d_ws, ws_bytes, d_err,
                       stream);
}

size_t tpf_lists_gather_workspace_size(uint64_t nq, uint64_t pos_values) { return tpf::lists_gather_workspace(nq, pos_values); }

int tpf_lists_gather(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                     const uint32_t * d_list_unit, uint64_t nlists, int d1, const uint32_t * d_start0, const uint32_t * d_unit_last,
                     const uint32_t * d_pos, uint64_t pos_values, const uint64_t * d_pos_ptr, const uint32_t * d_qlist, uint64_t nq,
                     uint32_t * d_out, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (over_limit({nlists, nunits, nq, pos_values}))
        return fail(TPF_EINVAL, "tpf_lists_gather: nlists, nunits, nq and pos_values are limited to 0x7FFFFFFF");
    if (nq && (!d_in || !d_off || !d_list_ptr || !d_list_unit || !d_pos_ptr || !d_qlist || !d_ws))
        return fail(TPF_EINVAL, "tpf_lists_gather: null pointer");
    if (nq && d1 && !d_unit_last)
        return fail(TPF_EINVAL, "tpf_lists_gather: null d_unit_last (delta-1 needs the skip table of tpf_lists_unit_last)");
    if (pos_values && (!d_pos || !d_out))
        return fail(TPF_EINVAL, "tpf_lists_gather: null d_pos or d_out with a non-zero pos_values");
    if (nq && ws_bytes < tpf_lists_gather_workspace_size(nq, pos_values))
        return fail(TPF_EINVAL, "tpf_lists_gather: workspace too small");
    if (int rc = check_device())
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // d_err is reset by the launcher, together with its workspace header
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d1, d_start0, d_unit_last);
    return done(tpf::launch_lists_gather(X, d1 != 0, d_pos, pos_values, d_pos_ptr, d_qlist, nq, d_out, d_ws, dev_err(d_err), s),
                "tpf_lists_gather");
}

// ---- postings appended to a resident index (p4_lists_append.hip)
// A null pointer of the output side, which tpf_lists_append, tpf_lists_remove and tpf_lists_extract share, for a result of n lists: the
// three directories written always; the workspace, and d_out when it has a capacity, once there are lists.
static bool index_out_null(uint64_t n, const uint8_t * d_out, uint64_t out_cap, const uint64_t * d_off_out, const uint64_t * d_list_ptr_out,
                           const uint32_t * d_list_unit_out, const void * d_ws)
{
    return !d_off_out || !d_list_ptr_out || !d_list_unit_out || (n && (!d_ws || (out_cap && !d_out)));
}

uint64_t tpf_lists_append_units_bound(uint64_t nunits, uint64_t nlists_out, uint64_t add_values)
{
    return nunits + add_values / 256u + std::min(nlists_out, add_values);
}

uint64_t tpf_lists_append_bound(uint64_t in_bytes, uint64_t nlists_out, uint64_t add_values)
{
    const uint64_t T = std::min(nlists_out, add_values);
    return in_bytes + tpf_p4nenc256v32_lists_bound(add_values + 255u * T, T);
}

size_t tpf_lists_append_workspace_size(uint64_t nunits, uint64_t nlists_out, uint64_t add_values)
{
    return tpf::lists_append_workspace(nunits, nlists_out, add_values);
}

int tpf_lists_append(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                     const uint32_t * d_list_unit, uint64_t nlists, int d1, const uint32_t * d_start0, const uint32_t * d_unit_last,
                     const uint32_t * d_add, uint64_t add_values, const uint64_t * d_add_ptr, uint64_t nlists_out, uint8_t * d_out,
                     uint64_t out_cap, uint64_t * d_off_out, uint64_t units_cap, uint64_t * d_list_ptr_out, uint32_t * d_list_unit_out,
                     uint32_t * d_unit_last_out, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (nlists_out < nlists)
        return fail(TPF_EINVAL, "tpf_lists_append: nlists_out is below nlists (lists are never removed)");
    if (over_limit({nunits, nlists_out, units_cap, add_values}))
        return fail(TPF_EINVAL, "tpf_lists_append: nunits, nlists_out, units_cap and add_values are limited to 0x7FFFFFFF");
    if (index_out_null(nlists_out, d_out, out_cap, d_off_out, d_list_ptr_out, d_list_unit_out, d_ws) || (nlists_out && !d_add_ptr))
        return fail(TPF_EINVAL, "tpf_lists_append: null pointer");
    if (nlists && nunits && (!d_in || !d_off || !d_list_ptr || !d_list_unit))
        return fail(TPF_EINVAL, "tpf_lists_append: null pointer (the old index)");
    if (nlists_out && d1 && (!d_unit_last_out || (nlists && nunits && !d_unit_last)))
        return fail(TPF_EINVAL,
                    "tpf_lists_append: null d_unit_last or d_unit_last_out (delta-1 needs the skip table of tpf_lists_unit_last)");
    if (add_values && !d_add)
        return fail(TPF_EINVAL, "tpf_lists_append: null d_add with a non-zero add_values");
    if (nlists_out && ws_bytes < tpf_lists_append_workspace_size(nunits, nlists_out, add_values))
        return fail(TPF_EINVAL, "tpf_lists_append: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d1, d_start0, d_unit_last);
    return done(tpf::launch_lists_append(X, d1 != 0, d_add, add_values, d_add_ptr, nlists_out, d_out, out_cap, d_off_out, units_cap,
                                         d_list_ptr_out, d_list_unit_out, d1 ? d_unit_last_out : nullptr, d_ws, dev_err(d_err), s),
                "tpf_lists_append");
}

// ---- postings deleted from a resident index (p4_lists_remove.hip)
uint64_t tpf_lists_remove_bound(uint64_t in_bytes, uint64_t nq, uint64_t stage_values)
{
    return in_bytes + tpf_p4nenc256v32_lists_bound(stage_values, nq);
}

size_t tpf_lists_remove_workspace_size(uint64_t nunits, uint64_t nlists, uint64_t nq, uint64_t pos_values, uint64_t stage_values)
{
    (void)nunits, (void)pos_values; // nothing of the workspace is sized by them
    return tpf::lists_remove_workspace(nlists, nq, stage_values);
}

int tpf_lists_remove(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                     const uint32_t * d_list_unit, uint64_t nlists, int d1, const uint32_t * d_start0, const uint32_t * d_unit_last,
                     const uint32_t * d_pos, uint64_t pos_values, const uint64_t * d_pos_ptr, const uint32_t * d_qlist, uint64_t nq,
                     uint64_t stage_values, uint8_t * d_out, uint64_t out_cap, uint64_t * d_off_out, uint64_t units_cap,
                     uint64_t * d_list_ptr_out, uint32_t * d_list_unit_out, uint32_t * d_unit_last_out, void * d_ws, size_t ws_bytes,
                     uint64_t * d_err, void * stream)
{
    if (over_limit({nunits, nlists, nq, pos_values, stage_values, units_cap, stage_values / 256u + nq + 1u}))
        return fail(TPF_EINVAL,
                    "tpf_lists_remove: nunits, nlists, nq, pos_values, stage_values, units_cap and stage_values / 256 + nq + 1 are "
                    "limited to 0x7FFFFFFF");
    if (index_out_null(nlists, d_out, out_cap, d_off_out, d_list_ptr_out, d_list_unit_out, d_ws)
        || (nlists && (!d_list_ptr || !d_list_unit)))
        return fail(TPF_EINVAL, "tpf_lists_remove: null pointer");
    if (nlists && nunits && (!d_in || !d_off))
        return fail(TPF_EINVAL, "tpf_lists_remove: null pointer (the old index)");
    if (nlists && d1 && (!d_unit_last_out || (nunits && !d_unit_last)))
        return fail(TPF_EINVAL,
                    "tpf_lists_remove: null d_unit_last or d_unit_last_out (delta-1 needs the skip table of tpf_lists_unit_last)");
    if (nlists && nq && (!d_pos_ptr || !d_qlist))
        return fail(TPF_EINVAL, "tpf_lists_remove: null d_pos_ptr or d_qlist with a non-zero nq");
    if (nlists && nq && pos_values && !d_pos)
        return fail(TPF_EINVAL, "tpf_lists_remove: null d_pos with a non-zero pos_values");
    if (nlists && ws_bytes < tpf_lists_remove_workspace_size(nunits, nlists, nq, pos_values, stage_values))
        return fail(TPF_EINVAL, "tpf_lists_remove: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d1, d_start0, d_unit_last);
    return done(tpf::launch_lists_remove(X, d1 != 0, d_pos, pos_values, d_pos_ptr, d_qlist, nlists ? nq : 0u, stage_values, d_out, out_cap,
                                         d_off_out, units_cap, d_list_ptr_out, d_list_unit_out, d1 ? d_unit_last_out : nullptr, d_ws,
                                         dev_err(d_err), s), "tpf_lists_remove");
}

// ---- a sub-index of a resident index (p4_lists_extract.hip)
size_t tpf_lists_extract_workspace_size(uint64_t nsel) { return tpf::lists_extract_workspace(nsel); }

int tpf_lists_extract(const uint8_t * d_in, uint64_t in_bytes, const uint64_t * d_off, uint64_t nunits, const uint64_t * d_list_ptr,
                      const uint32_t * d_list_unit, uint64_t nlists, int d1, const uint32_t * d_start0, const uint32_t * d_unit_last,
                      const uint32_t * d_sel, const uint32_t * d_ufirst, const uint32_t * d_ucount, uint64_t nsel, uint8_t * d_out,
                      uint64_t out_cap, uint64_t * d_off_out, uint64_t units_cap, uint64_t * d_list_ptr_out, uint32_t * d_list_unit_out,
                      uint32_t * d_start0_out, uint32_t * d_unit_last_out, void * d_ws, size_t ws_bytes, uint64_t * d_err, void * stream)
{
    if (over_limit({nunits, nlists, nsel, units_cap}))
        return fail(TPF_EINVAL, "tpf_lists_extract: nunits, nlists, nsel and units_cap are limited to 0x7FFFFFFF");
    if (index_out_null(nsel, d_out, out_cap, d_off_out, d_list_ptr_out, d_list_unit_out, d_ws)
        || (nsel && (!d_sel || !d_list_ptr || !d_list_unit)))
        return fail(TPF_EINVAL, "tpf_lists_extract: null pointer");
    if (nsel && nunits && (!d_in || !d_off))
        return fail(TPF_EINVAL, "tpf_lists_extract: null pointer (the index)");
    if (nsel && d_ufirst && !d_ucount)
        return fail(TPF_EINVAL, "tpf_lists_extract: null d_ucount with d_ufirst");
    if (nsel && d1 && !d_start0_out)
        return fail(TPF_EINVAL, "tpf_lists_extract: null d_start0_out (a delta-1 sub-index has starts of its own)");
    if (nsel && d1 && d_ufirst && !d_unit_last)
        return fail(TPF_EINVAL, "tpf_lists_extract: null d_unit_last (a delta-1 unit range starts from the skip table of tpf_lists_unit_last)");
    if (ws_bytes < tpf_lists_extract_workspace_size(nsel))
        return fail(TPF_EINVAL, "tpf_lists_extract: workspace too small");
    hipStream_t s;
    if (int rc = open_device_stream(stream, d_err, s))
        return rc;
    const tpf::ListsIndex X = lists_index(d_in, in_bytes, d_off, nunits, d_list_ptr, d_list_unit, nlists, d1, d_start0, d_unit_last);
    return done(tpf::launch_lists_extract(X, d1 != 0, d_sel, d_ufirst, d_ucount, nsel, d_out, out_cap, d_off_out, units_cap, d_list_ptr_out,
                                          d_list_unit_out, d1 ? d_start0_out : nullptr, d1 ? d_unit_last_out : nullptr, d_ws,
                                          dev_err(d_err), s),
                "tpf_lists_extract");
}

int tpf_copy_async(void * dst, const void * src, uint64_t bytes, void * stream)
{
    if (int rc = check_device())
        return rc;
    if (bytes && (!dst || !src))
        return fail(TPF_EINVAL, "tpf_copy_async: null pointer");
    return done(tpf::launch_copy(dst, src, bytes, static_cast<hipStream_t>(stream)), "tpf_copy_async");
}

} // extern "C"
