// gen_golden.cpp -- generates tests/golden/*.bin from the REFERENCE scalar
// codec (turbopfor::scalar::*, compiled from /root/reference/src by
// oracle/Makefile target `ref`).  Test infrastructure only.
//
// Inputs are produced by our own splitmix64 generator and STORED in the
// fixtures (std::uniform_int_distribution is implementation-defined, so the
// reference tests' seeds would not reproduce).  Patterns follow the
// reference tests: tests/test_helpers.h:90-155 (sequential, random, constant,
// fillWithExceptions), tests/test_p4dec_32.cpp:248-264, tests/test_d1enc.cpp:154
// (sorted, maxDelta 1/15/255/65535), tests/test_p4_64.cpp:587-611 (64-bit bit
// widths, 32/64-bit exceptions, 63->64 quirk) and benchmarks/ab_test.cpp:1610-1631
// (exception distribution).
//
// File format (little endian):
//   "TPFG" u32 version(1) u32 count
//   record: u32 flags  (bit0 = delta-1, bit1 = decode-only vector, bit2 = n
//                       below the layout width and the padding bits of enc
//                       follow the zero convention, see gen64_short)
//           u32 n      (values per call)
//           u64 start  (delta-1 start)
//           u32 esize  (4 or 8)
//           u32 enc_len
//           u8  values[n*esize]   (encoder input == expected decoder output)
//           u8  enc[enc_len]      (expected encoder output / decoder input)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cmath>

#include "turbopfor.h"
#include "scalar/p4_scalar.h"

namespace sc = turbopfor::scalar;

struct Rng
{
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) { }
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t range(uint64_t lo, uint64_t hi) // inclusive
    {
        uint64_t span = hi - lo + 1u;
        if (span == 0u)
            return next();
        return lo + next() % span;
    }
    double unit() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct Writer
{
    std::vector<uint8_t> buf;
    uint32_t count = 0;
    void put(const void * p, size_t n)
    {
        const uint8_t * b = static_cast<const uint8_t *>(p);
        buf.insert(buf.end(), b, b + n);
    }
    template <class T>
    void put(T v) { put(&v, sizeof(T)); }
    void record(uint32_t flags, uint32_t n, uint64_t start, uint32_t esize, const void * vals, const uint8_t * enc, uint32_t enc_len)
    {
        put(flags);
        put(n);
        put(start);
        put(esize);
        put(enc_len);
        put(vals, size_t(n) * esize);
        put(enc, enc_len);
        ++count;
    }
    void save(const std::string & path)
    {
        FILE * f = std::fopen(path.c_str(), "wb");
        if (!f)
        {
            std::perror(path.c_str());
            std::exit(1);
        }
        std::fwrite("TPFG", 1, 4, f);
        uint32_t ver = 1;
        std::fwrite(&ver, 4, 1, f);
        std::fwrite(&count, 4, 1, f);
        std::fwrite(buf.data(), 1, buf.size(), f);
        std::fclose(f);
        std::printf("%s: %u records, %zu bytes\n", path.c_str(), count, buf.size() + 12);
    }
};

static void die(const char * what, unsigned idx)
{
    std::fprintf(stderr, "reference self-check failed: %s (case %u)\n", what, idx);
    std::exit(2);
}

// ---------------------------------------------------------------- 32-bit
enum Fmt32
{
    F256V32,
    F128V32,
    FH32
};

static unsigned blockN(Fmt32 f, unsigned n) { return f == F256V32 ? 256u : f == F128V32 ? 128u : n; }

static void add32(Writer & w, Fmt32 f, std::vector<uint32_t> v, bool d1, uint32_t start)
{
    unsigned n = static_cast<unsigned>(v.size());
    std::vector<uint8_t> enc(n * 5 + 4096, 0);
    std::vector<uint32_t> in(std::max<size_t>(v.size(), 256) + 64, 0);
    std::copy(v.begin(), v.end(), in.begin());
    uint8_t * e = nullptr;
    if (f == F256V32)
        e = d1 ? sc::p4D1Enc256v32(in.data(), n, enc.data(), start) : sc::p4Enc256v32(in.data(), n, enc.data());
    else if (f == F128V32)
        e = d1 ? sc::p4D1Enc128v32(in.data(), n, enc.data(), start) : sc::p4Enc128v32(in.data(), n, enc.data());
    else
        e = d1 ? sc::p4D1Enc32(in.data(), n, enc.data(), start) : sc::p4Enc32(in.data(), n, enc.data());
    uint32_t len = static_cast<uint32_t>(e - enc.data());
    std::vector<uint32_t> dec(512 + 64, 0xDEADBEEFu);
    const uint8_t * r = nullptr;
    if (f == F256V32)
        r = d1 ? sc::p4D1Dec256v32(enc.data(), n, dec.data(), start) : sc::p4Dec256v32(enc.data(), n, dec.data());
    else if (f == F128V32)
        r = d1 ? sc::p4D1Dec128v32(enc.data(), n, dec.data(), start) : sc::p4Dec128v32(enc.data(), n, dec.data());
    else
        r = d1 ? sc::p4D1Dec32(enc.data(), n, dec.data(), start) : sc::p4Dec32(enc.data(), n, dec.data());
    if (r != e)
        die("decode end pointer", w.count);
    if (std::memcmp(dec.data(), v.data(), n * 4u) != 0)
        die("round trip", w.count);
    w.record(d1 ? 1u : 0u, n, start, 4u, v.data(), enc.data(), len);
}

static std::vector<uint32_t> sortedSeq(Rng & r, unsigned n, uint32_t max_delta, uint32_t & start_out)
{
    std::vector<uint32_t> v(n);
    uint32_t cur = static_cast<uint32_t>(r.range(0, 1000));
    start_out = cur;
    for (unsigned i = 0; i < n; ++i)
    {
        cur += static_cast<uint32_t>(r.range(1, max_delta));
        v[i] = cur;
    }
    return v;
}

// Zipf-ish posting-list gaps: 95% gaps from a bounded
// continuous Zipf(s=1.1) on [1,64], 5% gaps 64+U[0,2^16).
static uint32_t zipfGap(Rng & r)
{
    if (r.unit() < 0.05)
        return 64u + static_cast<uint32_t>(r.range(0, 65535));
    const double s = 1.1, a = 1.0, b = 65.0;
    double u = r.unit();
    double x = std::pow(std::pow(a, 1 - s) + u * (std::pow(b, 1 - s) - std::pow(a, 1 - s)), 1.0 / (1 - s));
    uint32_t g = static_cast<uint32_t>(std::floor(x));
    return g < 1u ? 1u : (g > 64u ? 64u : g);
}

static void gen32(Writer & w, Fmt32 f, uint64_t seed)
{
    Rng r(seed);
    std::vector<unsigned> ns;
    if (f == FH32)
        ns = {1, 2, 3, 5, 7, 8, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256};
    else
        ns = {blockN(f, 0)};
    for (unsigned n : ns)
    {
        std::vector<uint32_t> v(n);
        // sequential / zeros / constant 42 (test_p4dec_32.cpp:248-264)
        for (unsigned i = 0; i < n; ++i)
            v[i] = 1000u + i * 3u;
        add32(w, f, v, false, 0);
        std::fill(v.begin(), v.end(), 0u);
        add32(w, f, v, false, 0);
        std::fill(v.begin(), v.end(), 42u);
        add32(w, f, v, false, 0);
        // constant blocks of every bit width (constant payload = ceil(b/8) bytes)
        for (unsigned b = 1; b <= 32; b += (f == FH32 && n != 127 ? 7 : 1))
        {
            uint32_t c = (b == 32) ? 0xF0000001u : ((1u << (b - 1)) | static_cast<uint32_t>(r.range(0, (1u << (b - 1)) - 1)));
            std::fill(v.begin(), v.end(), c);
            add32(w, f, v, false, 0);
        }
        // random, every bit width
        unsigned reps = (f == FH32 && n != 127) ? 1u : 2u;
        for (unsigned b = 1; b <= 32; ++b)
            for (unsigned rep = 0; rep < reps; ++rep)
            {
                uint32_t mx = b == 32 ? 0xFFFFFFFFu : ((1u << b) - 1u);
                for (auto & x : v)
                    x = static_cast<uint32_t>(r.range(0, mx));
                add32(w, f, v, false, 0);
            }
        // fillWithExceptions(255, 100000, pct) (test_helpers.h:109-121)
        for (unsigned pct : {1u, 5u, 10u, 25u, 50u})
        {
            for (auto & x : v)
                x = (r.range(0, 99) < pct) ? 100000u : static_cast<uint32_t>(r.range(0, 255));
            add32(w, f, v, false, 0);
        }
        // ab_test distribution (ab_test.cpp:1610-1631): base U[0,2^bw), exc U[2^bw, 2^32)
        for (unsigned bw = 1; bw <= 28; bw += (f == FH32 && n != 127 ? 5 : 1))
            for (double pct : {0.0, 5.0, 10.0, 25.0})
            {
                for (auto & x : v)
                    x = (r.unit() * 100.0 < pct) ? static_cast<uint32_t>(r.range(1ull << bw, 0xFFFFFFFFull))
                                                 : static_cast<uint32_t>(r.range(0, (1ull << bw) - 1));
                add32(w, f, v, false, 0);
            }
        // mostly zero with a few large values (b = 0 with patches / vbyte at b = 0)
        for (unsigned k : {1u, 2u, 3u, 8u, 40u})
        {
            std::fill(v.begin(), v.end(), 0u);
            for (unsigned j = 0; j < k && j < n; ++j)
                v[r.range(0, n - 1)] = static_cast<uint32_t>(r.range(1, 0xFFFFFFFFull));
            add32(w, f, v, false, 0);
        }
        // small values + moderately sized exceptions: vbyte compressed vs raw escape
        for (unsigned k : {4u, 12u, 20u, 30u, 60u, 100u})
            for (uint32_t emax : {300u, 20000u, 3000000u, 0x7FFFFFFu})
            {
                for (auto & x : v)
                    x = static_cast<uint32_t>(r.range(0, 15));
                for (unsigned j = 0; j < k && j < n; ++j)
                    v[r.range(0, n - 1)] = static_cast<uint32_t>(r.range(16, emax));
                add32(w, f, v, false, 0);
            }
        // delta-1: sorted inputs (test_d1enc.cpp:154)
        for (uint32_t md : {1u, 15u, 255u, 65535u})
        {
            uint32_t st;
            auto s = sortedSeq(r, n, md, st);
            add32(w, f, s, true, st);
        }
        {
            // wrap-around start
            uint32_t st = 0xFFFFFF00u, cur = st;
            for (auto & x : v)
                x = (cur += static_cast<uint32_t>(r.range(1, 9)));
            add32(w, f, v, true, st);
        }
        for (unsigned rep = 0; rep < 6; ++rep)
        {
            uint32_t cur = static_cast<uint32_t>(r.range(0, 1u << 20)), st = cur;
            for (auto & x : v)
                x = (cur += zipfGap(r));
            add32(w, f, v, true, st);
        }
    }
}

// ---------------------------------------------------------------- 64-bit
static void add64(Writer & w, std::vector<uint64_t> v, bool d1, uint64_t start, bool v128)
{
    unsigned n = static_cast<unsigned>(v.size());
    std::vector<uint8_t> enc(n * 10 + 4096, 0);
    std::vector<uint64_t> in(256 + 64, 0);
    std::copy(v.begin(), v.end(), in.begin());
    uint8_t * e = v128 ? (d1 ? sc::p4D1Enc128v64(in.data(), n, enc.data(), start) : sc::p4Enc128v64(in.data(), n, enc.data()))
                       : (d1 ? sc::p4D1Enc256v64(in.data(), n, enc.data(), start) : sc::p4Enc256v64(in.data(), n, enc.data()));
    uint32_t len = static_cast<uint32_t>(e - enc.data());
    std::vector<uint64_t> dec(256 + 64, 0);
    const uint8_t * rp = v128 ? (d1 ? sc::p4D1Dec128v64(enc.data(), n, dec.data(), start) : sc::p4Dec128v64(enc.data(), n, dec.data()))
                              : (d1 ? sc::p4D1Dec256v64(enc.data(), n, dec.data(), start) : sc::p4Dec256v64(enc.data(), n, dec.data()));
    if (rp != e)
        die("64 decode end pointer", w.count);
    if (std::memcmp(dec.data(), v.data(), n * 8u) != 0)
        die("64 round trip", w.count);
    w.record(d1 ? 1u : 0u, n, start, 8u, v.data(), enc.data(), len);
}

static void gen64(Writer & w, uint64_t seed, bool v128)
{
    Rng r(seed);
    const unsigned n = v128 ? 128u : 256u;
    std::vector<uint64_t> v(n);
    for (unsigned i = 0; i < n; ++i)
        v[i] = 1000000ull + i * 7ull;
    add64(w, v, false, 0, v128);
    std::fill(v.begin(), v.end(), 0ull);
    add64(w, v, false, 0, v128);
    for (unsigned b : {1u, 8u, 31u, 32u, 33u, 40u, 56u, 63u, 64u})
    {
        uint64_t c = (b == 64) ? 0xF000000000000001ull : ((1ull << (b - 1)) | 1ull);
        std::fill(v.begin(), v.end(), c);
        add64(w, v, false, 0, v128);
    }
    // bit widths of test_p4_64.cpp:587-611
    for (unsigned b : {1u, 2u, 4u, 8u, 16u, 24u, 31u, 32u, 33u, 40u, 48u, 56u, 62u, 63u, 64u})
        for (unsigned rep = 0; rep < 3; ++rep)
        {
            uint64_t mx = b == 64 ? ~0ull : ((1ull << b) - 1ull);
            for (auto & x : v)
                x = r.range(0, mx);
            add64(w, v, false, 0, v128);
        }
    // exceptions above bit 32 and at bit 63/64
    for (unsigned bw : {4u, 8u, 16u, 20u, 31u, 32u, 40u})
        for (unsigned pct : {1u, 5u, 10u, 25u})
            for (unsigned hi : {33u, 48u, 63u, 64u})
            {
                for (auto & x : v)
                    x = (r.range(0, 99) < pct) ? r.range(1ull << (hi - 1), hi == 64 ? ~0ull : ((1ull << hi) - 1ull))
                                               : r.range(0, (1ull << bw) - 1ull);
                add64(w, v, false, 0, v128);
            }
    // vbyte-friendly: small base + a few moderately sized exceptions
    for (unsigned k : {3u, 10u, 20u, 40u})
        for (uint64_t emax : {300ull, 20000ull, 3000000ull, (1ull << 40), ~0ull})
        {
            for (auto & x : v)
                x = r.range(0, 15);
            for (unsigned j = 0; j < k; ++j)
                v[r.range(0, n - 1)] = r.range(16, emax);
            add64(w, v, false, 0, v128);
        }
    // 63->64 quirk: values whose width is exactly 63
    for (unsigned rep = 0; rep < 4; ++rep)
    {
        for (auto & x : v)
            x = r.range(1ull << 62, (1ull << 63) - 1ull);
        add64(w, v, false, 0, v128);
        for (auto & x : v)
            x = r.range(0, (1ull << 62) - 1ull);
        v[r.range(0, n - 1)] = (1ull << 62) | 5ull; // max width 63 with few at top
        add64(w, v, false, 0, v128);
    }
    // delta-1 (test_d1enc.cpp:300-339)
    for (uint64_t md : {1ull, 15ull, 255ull, 65535ull, (1ull << 40)})
        for (unsigned rep = 0; rep < 2; ++rep)
        {
            uint64_t cur = r.range(0, 100000), st = cur;
            for (auto & x : v)
                x = (cur += r.range(1, md));
            add64(w, v, true, st, v128);
        }
    {
        // 32-bit prefix overflow inside a 128 chunk (the simd::p4D1Dec256v64 bug of SURVEY a10)
        uint64_t cur = 0xFFFFF000ull, st = cur;
        for (auto & x : v)
            x = (cur += r.range(1 << 17, 1 << 22));
        add64(w, v, true, st, v128);
    }
}

// n below the layout width (128v64 n < 128, 256v64 n < 256).  The reference
// leaves the base slots past n of an exception block, and the delta slots
// past n of a D1 block, uninitialised (p4enc128v64_scalar.cpp:59,
// p4d1enc256v64_scalar.cpp:12): those payload bits are whatever its stack
// held.  Each vector is encoded after zero-filling the stack (the convention
// the oracle and the GPU path implement: padding slots are 0) and again after
// filling it with 0xA5; where the two differ the record carries flag 4
// ("padding bits follow the zero convention, not pinned by the reference").
__attribute__((noinline)) static void fill_stack(uint8_t v)
{
    volatile uint8_t junk[1 << 16];
    for (size_t i = 0; i < sizeof(junk); ++i)
        junk[i] = v;
    asm volatile("" ::"r"(junk) : "memory");
}

// p4Enc256v64 is a loop of p4Enc128v64 over 128-value chunks
// (p4enc256v64_scalar.cpp:15-30), so with `chunked` the 256v64 encoding is
// made chunk by chunk with the stack refilled before each call (the direct
// call's second chunk would see the first chunk's stale stack instead).
static uint32_t enc64_ref(const std::vector<uint64_t> & in, unsigned n, bool d1, uint64_t start, bool v128, uint8_t fill,
                          std::vector<uint8_t> & enc, bool chunked)
{
    std::vector<uint64_t> buf(in);
    std::fill(enc.begin(), enc.end(), 0);
    if (v128 || !chunked)
    {
        fill_stack(fill);
        uint8_t * e = v128 ? (d1 ? sc::p4D1Enc128v64(buf.data(), n, enc.data(), start) : sc::p4Enc128v64(buf.data(), n, enc.data()))
                           : (d1 ? sc::p4D1Enc256v64(buf.data(), n, enc.data(), start) : sc::p4Enc256v64(buf.data(), n, enc.data()));
        return static_cast<uint32_t>(e - enc.data());
    }
    uint8_t * e = enc.data();
    for (unsigned c0 = 0; c0 < n; c0 += 128u)
    {
        const unsigned c = std::min(n - c0, 128u);
        fill_stack(fill);
        e = d1 ? sc::p4D1Enc128v64(buf.data() + c0, c, e, c0 ? buf[c0 - 1] : start) : sc::p4Enc128v64(buf.data() + c0, c, e);
    }
    return static_cast<uint32_t>(e - enc.data());
}

static void add64_short(Writer & w, std::vector<uint64_t> v, bool d1, uint64_t start, bool v128)
{
    const unsigned n = static_cast<unsigned>(v.size());
    std::vector<uint64_t> in(256 + 64, 0);
    std::copy(v.begin(), v.end(), in.begin());
    std::vector<uint8_t> e0(n * 10 + 4096), e1(n * 10 + 4096), ed(n * 10 + 4096);
    const uint32_t len0 = enc64_ref(in, n, d1, start, v128, 0x00, e0, true);
    const uint32_t len1 = enc64_ref(in, n, d1, start, v128, 0xA5, e1, true);
    const uint32_t lend = enc64_ref(in, n, d1, start, v128, 0x00, ed, false);
    if (len0 != len1 || len0 != lend)
        die("64 short: length depends on stack contents", w.count);
    const bool unpinned = std::memcmp(e0.data(), e1.data(), len0) != 0 || std::memcmp(e0.data(), ed.data(), len0) != 0;
    std::vector<uint64_t> dec(256 + 64, 0);
    const uint8_t * rp = v128 ? (d1 ? sc::p4D1Dec128v64(e0.data(), n, dec.data(), start) : sc::p4Dec128v64(e0.data(), n, dec.data()))
                              : (d1 ? sc::p4D1Dec256v64(e0.data(), n, dec.data(), start) : sc::p4Dec256v64(e0.data(), n, dec.data()));
    if (rp != e0.data() + len0)
        die("64 short decode end pointer", w.count);
    if (std::memcmp(dec.data(), v.data(), n * 8u) != 0)
        die("64 short round trip", w.count);
    w.record((d1 ? 1u : 0u) | (unpinned ? 4u : 0u), n, start, 8u, v.data(), e0.data(), len0);
}

static void gen64_short(Writer & w, uint64_t seed, bool v128)
{
    Rng r(seed);
    const std::vector<unsigned> ns = v128 ? std::vector<unsigned>{1u, 7u, 64u, 100u, 127u}
                                          : std::vector<unsigned>{1u, 100u, 128u, 129u, 200u, 255u};
    for (unsigned n : ns)
    {
        std::vector<uint64_t> v(n);
        std::fill(v.begin(), v.end(), 0ull);
        add64_short(w, v, false, 0, v128);
        std::fill(v.begin(), v.end(), 0x123456789ull);
        add64_short(w, v, false, 0, v128); // constant
        for (unsigned b : {8u, 40u})
        {
            for (auto & x : v)
                x = r.range(0, (1ull << b) - 1ull);
            add64_short(w, v, false, 0, v128); // plain (or patched by chance)
        }
        for (unsigned pct : {10u, 30u})
            for (unsigned hi : {33u, 64u})
            {
                for (auto & x : v)
                    x = (r.range(0, 99) < pct) ? r.range(1ull << (hi - 1), hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) : r.range(0, 255);
                add64_short(w, v, false, 0, v128); // bitmap or vbyte exceptions
            }
        for (auto & x : v)
            x = r.range(0, 15);
        v[r.range(0, n - 1)] = r.range(1u << 20, 1u << 30);
        add64_short(w, v, false, 0, v128); // one exception: vbyte
        for (uint64_t md : {1ull, 255ull, (1ull << 40)})
        {
            uint64_t cur = r.range(0, 100000), st = cur;
            for (auto & x : v)
                x = (cur += r.range(1, md));
            add64_short(w, v, true, st, v128);
        }
    }
}

// ------------------------------------------------- horizontal 64-bit (p4Enc64)
// The base and the patch bits hold n values (any n <= 256), so n is swept
// over the bitmap-word and byte boundaries.  The encoder stores 8 bytes at a
// time (bitmap words, the constant): enc has slack behind the block.
static void add64h(Writer & w, const std::vector<uint64_t> & v, bool d1, uint64_t start)
{
    const unsigned n = static_cast<unsigned>(v.size());
    std::vector<uint8_t> enc(n * 10 + 4096, 0);
    std::vector<uint64_t> in(256 + 64, 0);
    std::copy(v.begin(), v.end(), in.begin());
    uint8_t * e = d1 ? sc::p4D1Enc64(in.data(), n, enc.data(), start) : sc::p4Enc64(in.data(), n, enc.data());
    const uint32_t len = static_cast<uint32_t>(e - enc.data());
    std::vector<uint64_t> dec(256 + 64, 0);
    const uint8_t * rp = d1 ? sc::p4D1Dec64(enc.data(), n, dec.data(), start) : sc::p4Dec64(enc.data(), n, dec.data());
    if (rp != e)
        die("64h decode end pointer", w.count);
    if (std::memcmp(dec.data(), v.data(), n * 8u) != 0)
        die("64h round trip", w.count);
    w.record(d1 ? 1u : 0u, n, start, 8u, v.data(), enc.data(), len);
}

static uint64_t ofWidth(Rng & r, unsigned b) // a value of width exactly b (b >= 1)
{
    return (1ull << (b - 1)) | (b > 1 ? r.range(0, (1ull << (b - 1)) - 1ull) : 0ull);
}

static void gen64h(Writer & w, uint64_t seed)
{
    Rng r(seed);
    const std::vector<unsigned> ns = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256};
    const std::vector<unsigned> wide_ns = {63, 64, 65, 127, 128, 129, 255, 256};
    unsigned rot = 0;
    auto next_n = [&] { return wide_ns[rot++ % wide_ns.size()]; };

    for (unsigned n : ns)
    {
        std::vector<uint64_t> v(n, 0ull);
        add64h(w, v, false, 0); // all zero: the header byte only
        // random of width <= b: every width at n = 256 and n <= 2, a thinner set between
        for (unsigned b = 1; b <= 64; ++b)
        {
            const bool thin = b == 1 || b == 7 || b == 8 || b == 31 || b == 32 || b == 33 || b == 57 || b == 63 || b == 64;
            if (n != 256 && n > 2 && !thin)
                continue;
            for (auto & x : v)
                x = r.range(0, b == 64 ? ~0ull : ((1ull << b) - 1ull));
            v[r.range(0, n - 1)] = ofWidth(r, b);
            add64h(w, v, false, 0);
        }
    }
    // constants: 8-byte store, advance ceil(b/8); header 63 stands for 63 and 64
    for (unsigned n : {1u, 2u, 65u, 256u})
        for (unsigned b : {1u, 8u, 32u, 33u, 56u, 57u, 63u, 64u})
        {
            std::vector<uint64_t> v(n, ofWidth(r, b));
            add64h(w, v, false, 0);
        }
    // exceptions reaching bit `hi` over a base of width bw
    for (unsigned bw : {0u, 3u, 8u, 20u, 31u, 32u, 33u, 40u})
        for (unsigned hi : {33u, 48u, 62u, 63u, 64u})
            for (unsigned pct : {2u, 10u, 30u})
            {
                if (hi <= bw)
                    continue;
                std::vector<uint64_t> v(next_n());
                bool any = false;
                for (auto & x : v)
                {
                    const bool ex = r.range(0, 99) < pct;
                    any |= ex;
                    x = ex ? r.range(1ull << (hi - 1), hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) : (bw ? r.range(0, (1ull << bw) - 1ull) : 0ull);
                }
                if (!any)
                    v[r.range(0, v.size() - 1)] = ofWidth(r, hi);
                add64h(w, v, false, 0);
            }
    // mixed exceptions: many one-byte vbyte markers and a few long forms, so the
    // compressed vbEnc64 stream is chosen and carries every marker length
    unsigned wstep = 0;
    for (unsigned rep = 0; rep < 32; ++rep)
    {
        const unsigned n = next_n();
        const unsigned b = static_cast<unsigned>(r.range(0, 11));
        std::vector<uint64_t> v(n);
        for (auto & x : v)
            x = b ? r.range(0, (1ull << b) - 1ull) : 0ull;
        const unsigned xn = static_cast<unsigned>(r.range((n + 7) / 8, n / 3));
        std::vector<unsigned> pos(n);
        for (unsigned i = 0; i < n; ++i)
            pos[i] = i;
        for (unsigned i = 0; i < xn; ++i)
            std::swap(pos[i], pos[i + r.range(0, n - 1 - i)]);
        for (unsigned i = 0; i < xn; ++i)
            v[pos[i]] |= r.range(1, 149) << b;
        const unsigned big = static_cast<unsigned>(r.range(1, 3));
        for (unsigned i = 0; i < big; ++i)
        {
            const unsigned span = 64u - (b + 8u) + 1u;
            v[pos[i]] = ofWidth(r, b + 8u + (wstep * 5u) % span);
            ++wstep;
        }
        add64h(w, v, false, 0);
    }
    // maximum width exactly 63: the plan turns b = 63 into 64 / bx = 0
    for (unsigned n : {65u, 256u})
    {
        std::vector<uint64_t> v(n);
        for (auto & x : v)
            x = r.range(1ull << 62, (1ull << 63) - 1ull);
        add64h(w, v, false, 0);
        for (auto & x : v)
            x = r.range(0, (1ull << 20) - 1ull);
        v[r.range(0, n - 1)] = (1ull << 62) | 5ull; // a single top value
        add64h(w, v, false, 0);
        for (auto & x : v)
            x = r.range(0, (1ull << 62) - 1ull);
        v[r.range(0, n - 1)] = (1ull << 62) | 5ull;
        add64h(w, v, false, 0);
    }
    // delta-1: gaps up to 2^62 (the sums wrap), starts 0, near 2^32 and wrapping 2^64
    for (uint64_t md : {1ull, 255ull, 65535ull, (1ull << 40), (1ull << 62)})
        for (uint64_t st : {0ull, 0xFFFFF000ull, ~0ull - 1000ull})
        {
            std::vector<uint64_t> v(md == 1ull ? 256u : next_n());
            uint64_t cur = st;
            for (auto & x : v)
                x = (cur += r.range(1, md));
            add64h(w, v, true, st);
        }
    for (unsigned n : {1u, 2u})
        for (uint64_t st : {0ull, ~0ull - 1000ull})
        {
            std::vector<uint64_t> v(n);
            uint64_t cur = st;
            for (auto & x : v)
                x = (cur += r.range(1, 1ull << 33));
            add64h(w, v, true, st);
        }
    // decode-only: header 0x80 | b with bx == 0 (p4dec64.cpp:95), b = 8 and 63 (= 64)
    for (unsigned b : {8u, 63u})
        for (unsigned n : {65u, 256u})
        {
            const unsigned bits = b == 63u ? 64u : b;
            std::vector<uint8_t> enc(2 + n * 8 + 64, 0);
            enc[0] = static_cast<uint8_t>(0x80u | b);
            enc[1] = 0;
            for (unsigned i = 0; i < (n * bits + 7u) / 8u; ++i)
                enc[2 + i] = static_cast<uint8_t>(r.next());
            std::vector<uint64_t> dec(256 + 64);
            const uint8_t * e = sc::p4Dec64(enc.data(), n, dec.data());
            if (e != enc.data() + 2 + (n * bits + 7u) / 8u)
                die("64h decode-only end pointer", w.count);
            w.record(2u, n, 0, 8u, dec.data(), enc.data(), static_cast<uint32_t>(e - enc.data()));
            const uint8_t * e1 = sc::p4D1Dec64(enc.data(), n, dec.data(), ~0ull - 77ull);
            w.record(3u, n, ~0ull - 77ull, 8u, dec.data(), enc.data(), static_cast<uint32_t>(e1 - enc.data()));
        }
}

// ------------------------------- 32-bit units with n below the layout width
// p4D1Enc128v32 / p4D1Enc256v32 delta-encode n values into an uninitialised
// stack array and hand it to the plain encoder (p4d1enc128v32_scalar.cpp:12),
// which packs the layout's full width when it picks the plain mode: those
// payload bits are whatever the stack held.  As add64_short: encoded after a
// 0x00 fill and after a 0xA5 fill of the stack, flag 4 where the bytes differ.
// The caller's slots past n are zero.
static uint32_t enc32_ref(Fmt32 f, const std::vector<uint32_t> & in, unsigned n, bool d1, uint32_t start, uint8_t fill,
                          std::vector<uint8_t> & enc)
{
    std::vector<uint32_t> buf(in);
    std::fill(enc.begin(), enc.end(), 0);
    fill_stack(fill);
    uint8_t * e = nullptr;
    if (f == F256V32)
        e = d1 ? sc::p4D1Enc256v32(buf.data(), n, enc.data(), start) : sc::p4Enc256v32(buf.data(), n, enc.data());
    else if (f == F128V32)
        e = d1 ? sc::p4D1Enc128v32(buf.data(), n, enc.data(), start) : sc::p4Enc128v32(buf.data(), n, enc.data());
    else
        e = d1 ? sc::p4D1Enc32(buf.data(), n, enc.data(), start) : sc::p4Enc32(buf.data(), n, enc.data());
    return static_cast<uint32_t>(e - enc.data());
}

static const uint8_t * dec32_ref(Fmt32 f, const uint8_t * enc, unsigned n, uint32_t * dec, bool d1, uint32_t start)
{
    uint8_t * e = const_cast<uint8_t *>(enc);
    if (f == F256V32)
        return d1 ? sc::p4D1Dec256v32(e, n, dec, start) : sc::p4Dec256v32(e, n, dec);
    if (f == F128V32)
        return d1 ? sc::p4D1Dec128v32(e, n, dec, start) : sc::p4Dec128v32(e, n, dec);
    return d1 ? sc::p4D1Dec32(e, n, dec, start) : sc::p4Dec32(e, n, dec);
}

static void add32_short(Writer & w, Fmt32 f, const std::vector<uint32_t> & v, bool d1, uint32_t start)
{
    const unsigned n = static_cast<unsigned>(v.size());
    std::vector<uint32_t> in(256 + 64, 0);
    std::copy(v.begin(), v.end(), in.begin());
    std::vector<uint8_t> e0(n * 5 + 4096), e1(n * 5 + 4096);
    const uint32_t len0 = enc32_ref(f, in, n, d1, start, 0x00, e0);
    const uint32_t len1 = enc32_ref(f, in, n, d1, start, 0xA5, e1);
    if (len0 != len1)
        die("32 short: length depends on stack contents", w.count);
    const bool unpinned = std::memcmp(e0.data(), e1.data(), len0) != 0;
    std::vector<uint32_t> dec(512 + 64, 0xDEADBEEFu);
    if (dec32_ref(f, e0.data(), n, dec.data(), d1, start) != e0.data() + len0)
        die("32 short decode end pointer", w.count);
    if (std::memcmp(dec.data(), v.data(), n * 4u) != 0)
        die("32 short round trip", w.count);
    w.record((d1 ? 1u : 0u) | (unpinned ? 4u : 0u), n, start, 4u, v.data(), e0.data(), len0);
}

static void gen32_short(Writer & w, Fmt32 f, uint64_t seed)
{
    Rng r(seed);
    const std::vector<unsigned> ns = f == F128V32 ? std::vector<unsigned>{1, 2, 7, 31, 32, 33, 63, 64, 65, 100, 127}
                                                  : std::vector<unsigned>{1, 63, 64, 65, 127, 128, 129, 200, 255};
    for (unsigned n : ns)
    {
        std::vector<uint32_t> v(n, 0u);
        add32_short(w, f, v, false, 0); // all zero
        std::fill(v.begin(), v.end(), 0x15u);
        add32_short(w, f, v, false, 0); // constant, b = 5
        std::fill(v.begin(), v.end(), 0xF0000001u);
        add32_short(w, f, v, false, 0); // constant, b = 32
        for (unsigned b : {1u, 8u, 17u, 32u})
        {
            const uint32_t mx = b == 32 ? 0xFFFFFFFFu : ((1u << b) - 1u);
            for (auto & x : v)
                x = static_cast<uint32_t>(r.range(0, mx));
            v[r.range(0, n - 1)] |= 1u << (b - 1); // width exactly b
            add32_short(w, f, v, false, 0);
        }
        // the exception mixes of gen32: fillWithExceptions, the ab_test distribution,
        // mostly zero with a few large values, small values + moderate exceptions
        for (unsigned pct : {5u, 25u})
        {
            for (auto & x : v)
                x = (r.range(0, 99) < pct) ? 100000u : static_cast<uint32_t>(r.range(0, 255));
            add32_short(w, f, v, false, 0);
        }
        for (unsigned bw : {4u, 12u, 20u})
            for (double pct : {5.0, 25.0})
            {
                for (auto & x : v)
                    x = (r.unit() * 100.0 < pct) ? static_cast<uint32_t>(r.range(1ull << bw, 0xFFFFFFFFull))
                                                 : static_cast<uint32_t>(r.range(0, (1ull << bw) - 1));
                add32_short(w, f, v, false, 0);
            }
        for (unsigned k : {1u, 3u})
        {
            std::fill(v.begin(), v.end(), 0u);
            for (unsigned j = 0; j < k && j < n; ++j)
                v[r.range(0, n - 1)] = static_cast<uint32_t>(r.range(1, 0xFFFFFFFFull));
            add32_short(w, f, v, false, 0);
        }
        for (unsigned k : {4u, 12u, 30u})
            for (uint32_t emax : {300u, 3000000u})
            {
                for (auto & x : v)
                    x = static_cast<uint32_t>(r.range(0, 15));
                for (unsigned j = 0; j < k && j < n; ++j)
                    v[r.range(0, n - 1)] = static_cast<uint32_t>(r.range(16, emax));
                add32_short(w, f, v, false, 0);
            }
        // delta-1 lists: sorted with bounded gaps, one wrapping 2^32, Zipf-ish gaps
        for (uint32_t md : {1u, 15u, 255u, 65535u})
        {
            uint32_t st;
            auto s = sortedSeq(r, n, md, st);
            add32_short(w, f, s, true, st);
        }
        {
            uint32_t st = 0xFFFFFF00u, cur = st;
            for (auto & x : v)
                x = (cur += static_cast<uint32_t>(r.range(1, 9)));
            add32_short(w, f, v, true, st);
        }
        for (unsigned rep = 0; rep < 2; ++rep)
        {
            uint32_t cur = static_cast<uint32_t>(r.range(0, 1u << 20)), st = cur;
            for (auto & x : v)
                x = (cur += zipfGap(r));
            add32_short(w, f, v, true, st);
        }
    }
}

// Compressed vbEnc32 streams with every marker length (1..5 bytes): a base of
// width 0..8, between n/8 and n/3 exceptions whose excess over the base is
// 1..149 (a one-byte marker), and one to three of them replaced by a value of
// width b+9..32 (the widths rotate, so that the 2-, 3-, 4- and 5-byte forms
// all occur).  The many short markers keep the compressed form 32 bytes under
// the raw one.  Plain and delta-1 (the values are then the list's gaps).
static void gen32_vbyte(Writer & w, Fmt32 f, uint64_t seed, const std::vector<unsigned> & ns, unsigned reps)
{
    Rng r(seed);
    unsigned wstep = 0;
    for (unsigned n : ns)
        for (unsigned d1 = 0; d1 < 2; ++d1)
            for (unsigned rep = 0; rep < reps; ++rep)
            {
                const unsigned b = static_cast<unsigned>(r.range(0, 8));
                std::vector<uint32_t> v(n);
                for (auto & x : v)
                    x = b ? static_cast<uint32_t>(r.range(0, (1u << b) - 1u)) : 0u;
                const unsigned xn = static_cast<unsigned>(r.range((n + 7) / 8, n / 3));
                std::vector<unsigned> pos(n);
                for (unsigned i = 0; i < n; ++i)
                    pos[i] = i;
                for (unsigned i = 0; i < xn; ++i)
                    std::swap(pos[i], pos[i + r.range(0, n - 1 - i)]);
                for (unsigned i = 0; i < xn; ++i)
                    v[pos[i]] |= static_cast<uint32_t>(r.range(1, 149)) << b;
                const unsigned big = static_cast<unsigned>(r.range(1, 3));
                for (unsigned i = 0; i < big; ++i)
                {
                    const unsigned span = 32u - (b + 9u) + 1u;
                    const unsigned wd = b + 9u + (wstep * 5u) % span;
                    ++wstep;
                    v[pos[i]] = (1u << (wd - 1)) | static_cast<uint32_t>(r.range(0, (1ull << (wd - 1)) - 1ull));
                }
                uint32_t st = 0;
                if (d1)
                {
                    uint32_t cur = st = static_cast<uint32_t>(r.next());
                    for (auto & x : v)
                        x = (cur += x + 1u);
                }
                add32_short(w, f, v, d1 != 0, st);
            }
}

// decode-only: header 0x80 | b with bx == 0 (p4dec128v32_scalar.cpp,
// p4dec32.cpp), which the encoder never emits
static void gen32_bx0(Writer & w, Fmt32 f, uint64_t seed, const std::vector<unsigned> & ns)
{
    Rng r(seed);
    for (unsigned n : ns)
        for (unsigned b : {8u, 32u})
        {
            const unsigned bb = f == F256V32 ? 32u * b : f == F128V32 ? 16u * b : (n * b + 7u) / 8u;
            std::vector<uint8_t> enc(2 + bb + 64, 0);
            enc[0] = static_cast<uint8_t>(0x80u | b);
            enc[1] = 0;
            for (unsigned i = 0; i < bb; ++i)
                enc[2 + i] = static_cast<uint8_t>(r.next());
            std::vector<uint32_t> dec(512 + 64, 0);
            if (dec32_ref(f, enc.data(), n, dec.data(), false, 0) != enc.data() + 2 + bb)
                die("32 decode-only end pointer", w.count);
            w.record(2u, n, 0, 4u, dec.data(), enc.data(), 2 + bb);
            if (dec32_ref(f, enc.data(), n, dec.data(), true, 0xFFFFFF00u) != enc.data() + 2 + bb)
                die("32 decode-only D1 end pointer", w.count);
            w.record(3u, n, 0xFFFFFF00u, 4u, dec.data(), enc.data(), 2 + bb);
        }
}

// ------------------- 128v64 / 256v64 at every n, mode and base layout
// One class of block per record: the mode (plain, bitmap patch, raw or
// compressed vbyte, constant, all zero) and the base width, which picks the
// base layout -- b = 0 (no base), 1..32 (the pair-swapped 128v32 layout),
// 33..62 (the horizontal 64-bit pack) -- with width 63 and 64 (header 63)
// for plain and constant.  A draw that the cost model encodes otherwise is
// drawn again.
enum Kind64
{
    K_ZERO,
    K_CONST,
    K_PLAIN,
    K_BITMAP,
    K_VBRAW,
    K_VBCOMP
};

struct Class64
{
    Kind64 kind;
    unsigned b; // base width wanted (K_CONST, K_PLAIN: the width, up to 64)
    bool wide_patch; // K_BITMAP: bx > 32
};

static bool isClass64(const uint8_t * enc, const Class64 & c)
{
    const unsigned h = enc[0], hb = h & 0x3Fu, want = c.b >= 63u ? 63u : c.b;
    // an exception block may settle on a neighbouring base width: the same layout counts
    const bool lay = c.b == 0u ? hb == 0u : c.b <= 32u ? (hb >= 1u && hb <= 32u) : (hb >= 33u && hb <= 62u);
    switch (c.kind)
    {
        case K_ZERO:
            return h == 0u;
        case K_CONST:
            return (h & 0xC0u) == 0xC0u && hb == want;
        case K_PLAIN:
            return (h & 0xC0u) == 0u && hb == want;
        case K_BITMAP:
            return (h & 0xC0u) == 0x80u && lay && (enc[1] > 32u) == c.wide_patch;
        default:
            return (h & 0xC0u) == 0x40u && lay && ((enc[2u + 16u * hb] == 0xFFu) == (c.kind == K_VBRAW));
    }
}

static std::vector<uint64_t> baseOf(Rng & r, unsigned n, unsigned b)
{
    std::vector<uint64_t> v(n, 0ull);
    if (b == 0u)
        return v;
    for (auto & x : v)
        x = r.range(0, b == 64u ? ~0ull : ((1ull << b) - 1ull));
    v[r.range(0, n - 1)] |= 1ull << (b - 1); // width exactly b
    return v;
}

static std::vector<unsigned> shuffled(Rng & r, unsigned n)
{
    std::vector<unsigned> pos(n);
    for (unsigned i = 0; i < n; ++i)
        pos[i] = i;
    for (unsigned i = 0; i + 1 < n; ++i)
        std::swap(pos[i], pos[i + r.range(0, n - 1 - i)]);
    return pos;
}

// One draw of the class (n values, the gaps of the list when delta-1).
// wstep rotates the widths of the long vbyte forms through b + 8 .. 64.
static std::vector<uint64_t> draw64(Rng & r, unsigned n, const Class64 & c, unsigned & wstep)
{
    const unsigned b = c.b;
    std::vector<uint64_t> v;
    switch (c.kind)
    {
        case K_ZERO:
            return std::vector<uint64_t>(n, 0ull);
        case K_CONST:
            return std::vector<uint64_t>(n, ofWidth(r, b));
        case K_PLAIN:
            return baseOf(r, n, b);
        case K_BITMAP:
        {
            // n/6 exceptions (at least one; fewer would go to vbyte) of one width: a patch of bx <= 32 or bx > 32 bits.
            // A few values over a horizontal base pay for the bitmap only over the
            // narrowest base and with the widest patch.
            const unsigned bb = (n < 16u && b > 32u) ? 33u : b;
            v = baseOf(r, n, bb);
            const unsigned hi = c.wide_patch ? 64u : std::min(64u, bb + 32u);
            const unsigned lo = n < 16u ? hi - 1u : c.wide_patch ? bb + 33u : bb + std::min(12u, 64u - bb);
            const unsigned w = static_cast<unsigned>(r.range(lo, hi));
            const auto pos = shuffled(r, n);
            for (unsigned i = 0; i < std::max(1u, n / 6u) && i + 1 < n; ++i)
                v[pos[i]] = ofWidth(r, w);
            return v;
        }
        case K_VBRAW:
        {
            // one to three values 8..24 bits over the base: fewer than 5 exceptions are never compressed
            v = baseOf(r, n, b);
            const auto pos = shuffled(r, n);
            if (n < 9u)
            {
                // the bitmap is one byte: vbyte pays only for one value 10..15 bits over a
                // narrow base beside one 62..64 bits wide (tests/v64_inputs.py VB_MIN_N64)
                v[pos[0]] = ofWidth(r, b + static_cast<unsigned>(r.range(10, 15)));
                v[pos[1]] = ofWidth(r, static_cast<unsigned>(r.range(62, 64)));
                return v;
            }
            const unsigned k = static_cast<unsigned>(r.range(1, 3));
            for (unsigned i = 0; i < k; ++i)
                v[pos[i]] = ofWidth(r, b + static_cast<unsigned>(r.range(8, std::min(24u, 64u - b))));
            return v;
        }
        default:
        {
            v = baseOf(r, n, b);
            const auto pos = shuffled(r, n);
            if (n < 40u)
            {
                // small n: 4 .. 12 exceptions (at most 2n/5) whose excess has exactly 7 bits and
                // one outlier 15 bits over the base (a 3-byte marker)
                const unsigned xn = static_cast<unsigned>(r.range(4, std::min(12u, 2u * n / 5u)));
                for (unsigned i = 0; i < xn; ++i)
                    v[pos[i]] = (v[pos[i]] & (b ? (1ull << b) - 1ull : 0ull)) | (r.range(64, 127) << b);
                v[pos[xn]] = ofWidth(r, b + 15u);
                return v;
            }
            // between n/8 and n/3 exceptions with a one-byte marker, one to three of them long
            const unsigned xn = static_cast<unsigned>(r.range((n + 7) / 8, n / 3));
            for (unsigned i = 0; i < xn; ++i)
                v[pos[i]] = (v[pos[i]] & (b ? (1ull << b) - 1ull : 0ull)) | (r.range(1, 149) << b);
            const unsigned big = static_cast<unsigned>(r.range(1, 3));
            for (unsigned i = 0; i < big; ++i)
            {
                const unsigned span = 64u - (b + 8u) + 1u;
                v[pos[i]] = ofWidth(r, b + 8u + (wstep * 5u) % span);
                ++wstep;
            }
            return v;
        }
    }
}

// A block of the class: drawn until the reference encodes it that way.
static std::vector<uint64_t> block64(Rng & r, unsigned n, const Class64 & c, unsigned & wstep, unsigned idx)
{
    std::vector<uint8_t> enc(128 * 10 + 4096);
    for (unsigned t = 0; t < 400; ++t)
    {
        std::vector<uint64_t> v = draw64(r, n, c, wstep);
        std::vector<uint64_t> in(128 + 64, 0ull);
        std::copy(v.begin(), v.end(), in.begin());
        std::fill(enc.begin(), enc.end(), 0);
        sc::p4Enc128v64(in.data(), n, enc.data());
        if (isClass64(enc.data(), c))
            return v;
    }
    std::fprintf(stderr, "class not reached: kind %d b %u n %u\n", int(c.kind), c.b, n);
    die("64 class", idx);
    return {};
}

// Which classes exist at n: one value is all zero or constant; vbyte needs
// n >= 5, over a horizontal base n >= 9, and compressed vbyte n >= 10
// (tests/v64_inputs.py).
static bool exists64(const Class64 & c, unsigned n)
{
    if (c.kind == K_ZERO || c.kind == K_CONST)
        return true;
    if (c.kind == K_VBRAW)
        return n >= (c.b > 32u ? 9u : 5u);
    if (c.kind == K_VBCOMP)
        return n >= 10u;
    return n >= 2u;
}

// The classes of one n; `rot` alternates the width of the header-63 records
// (63 / 64), the patch width of the bitmap records (bx <= 32 / bx > 32 where
// the base leaves room) and the horizontal base widths through 33..62.
static std::vector<Class64> classes64(unsigned rot)
{
    const unsigned top = 63u + (rot & 1u);
    const unsigned hb[4] = {33u, 40u, 62u, 35u};
    const unsigned h = hb[rot & 3u], hx = hb[(rot + 1u) & 3u];
    const bool wp = (rot & 1u) != 0u;
    return {
        {K_ZERO, 0, false},       {K_CONST, 5, false},         {K_CONST, top, false},      {K_PLAIN, (rot & 1u) ? 32u : 9u, false},
        {K_PLAIN, h, false},      {K_PLAIN, top, false},       {K_BITMAP, 0, wp},          {K_BITMAP, 7, !wp},
        {K_BITMAP, hx == 62u ? 50u : hx, false}, {K_VBRAW, 0, false}, {K_VBRAW, 6, false}, {K_VBRAW, hx == 62u ? 41u : hx, false},
        {K_VBCOMP, 0, false},     {K_VBCOMP, 3, false},        {K_VBCOMP, hx == 62u ? 36u : hx == 33u ? 38u : hx, false}, // (b = 33 loses to b + 7 by byte rounding at n = 10)
    };
}

static std::vector<uint64_t> asList(const std::vector<uint64_t> & gaps, uint64_t start)
{
    std::vector<uint64_t> v(gaps.size());
    uint64_t cur = start;
    for (size_t i = 0; i < gaps.size(); ++i)
        v[i] = (cur += gaps[i] + 1ull);
    return v;
}

static void gen64s_128(Writer & w, uint64_t seed)
{
    Rng r(seed);
    unsigned wstep = 0, rot = 0;
    for (unsigned n : {1u, 2u, 5u, 7u, 8u, 9u, 10u, 31u, 32u, 33u, 63u, 64u, 65u, 100u, 127u})
    {
        for (unsigned d1 = 0; d1 < 2; ++d1)
            for (const Class64 & c : classes64(rot + d1))
            {
                if (!exists64(c, n))
                    continue;
                std::vector<uint64_t> v = block64(r, n, c, wstep, w.count);
                // delta-1: the block's values are the list's gaps; one list per n wraps 2^64
                const uint64_t st = c.kind == K_PLAIN ? ~0ull - 1000ull : r.next() >> 1;
                add64_short(w, d1 ? asList(v, st) : v, d1 != 0, d1 ? st : 0ull, true);
            }
        ++rot;
    }
}

// decode-only: header 0x80 | b with bx == 0 (p4d1dec128v64_scalar.cpp:211,
// :298), which the encoder never emits: b = 8 (vertical base), 40
// (horizontal) and 63 (= 64)
static void gen64s_bx0(Writer & w, uint64_t seed)
{
    Rng r(seed);
    for (unsigned b : {8u, 40u, 63u})
        for (unsigned n : {128u, 100u, 7u})
        {
            const unsigned bb = 16u * (b == 63u ? 64u : b);
            std::vector<uint8_t> enc(2 + bb + 64, 0);
            enc[0] = static_cast<uint8_t>(0x80u | b);
            for (unsigned i = 0; i < bb; ++i)
                enc[2 + i] = static_cast<uint8_t>(r.next());
            std::vector<uint64_t> dec(256 + 64, 0);
            if (sc::p4Dec128v64(enc.data(), n, dec.data()) != enc.data() + 2 + bb)
                die("128v64 decode-only end pointer", w.count);
            w.record(2u, n, 0, 8u, dec.data(), enc.data(), 2 + bb);
            if (sc::p4D1Dec128v64(enc.data(), n, dec.data(), ~0ull - 77ull) != enc.data() + 2 + bb)
                die("128v64 decode-only D1 end pointer", w.count);
            w.record(3u, n, ~0ull - 77ull, 8u, dec.data(), enc.data(), 2 + bb);
        }
}

// 256v64 units of n values: a 128v64 block of min(n, 128) values and one of
// the rest, each of a class of its own, paired so that each half carries
// each base layout.
static void gen64s_256(Writer & w, uint64_t seed)
{
    Rng r(seed);
    unsigned wstep = 0;
    const Class64 Z{K_ZERO, 0, false}, C{K_CONST, 21, false}, C63{K_CONST, 63, false}, C64{K_CONST, 64, false};
    const Class64 PV{K_PLAIN, 17, false}, PH{K_PLAIN, 34, false}, P63{K_PLAIN, 63, false}, P64{K_PLAIN, 64, false};
    const Class64 B0{K_BITMAP, 0, true}, BV{K_BITMAP, 9, false}, BH{K_BITMAP, 37, false};
    const Class64 R0{K_VBRAW, 0, false}, RV{K_VBRAW, 4, false}, RH{K_VBRAW, 33, false};
    const Class64 V0{K_VBCOMP, 0, false}, VV{K_VBCOMP, 2, false}, VH{K_VBCOMP, 35, false};
    const std::vector<std::pair<Class64, Class64>> pairs = {{PV, PH}, {PH, PV}, {BV, BH}, {BH, BV}, {RV, RH},   {RH, RV}, {VV, VH},
                                                            {VH, VV}, {Z, P63},  {P64, C63}, {C, Z},  {C64, C}, {B0, R0}, {R0, V0},
                                                            {V0, B0}};
    // a class that does not exist at the block's n falls back: zero, constant, constant of width 64
    const Class64 small[3] = {Z, C, C64};
    for (unsigned n : {1u, 100u, 128u, 129u, 200u, 255u, 256u})
        for (unsigned d1 = 0; d1 < 2; ++d1)
            for (size_t p = 0; p < pairs.size(); ++p)
            {
                if (d1 && (p % 2u))
                    continue; // delta-1 twins: every other pair, one order of each layout pair
                std::vector<uint64_t> v;
                for (unsigned c0 = 0; c0 < n; c0 += 128u)
                {
                    const unsigned bn = std::min(n - c0, 128u);
                    Class64 c = c0 ? pairs[p].second : pairs[p].first;
                    if (!exists64(c, bn))
                        c = small[p % 3u];
                    const auto blk = block64(r, bn, c, wstep, w.count);
                    v.insert(v.end(), blk.begin(), blk.end());
                }
                const uint64_t st = p == 0 ? ~0ull - 1000ull : r.next() >> 1;
                add64_short(w, d1 ? asList(v, st) : v, d1 != 0, d1 ? st : 0ull, false);
            }
    // decode-only: the bx == 0 header in the first half, then in the second
    for (unsigned half = 0; half < 2; ++half)
    {
        std::vector<uint8_t> enc;
        for (unsigned k = 0; k < 2; ++k)
        {
            const unsigned b = k == half ? (half ? 40u : 8u) : (half ? 12u : 44u);
            if (k == half)
            {
                enc.push_back(static_cast<uint8_t>(0x80u | b));
                enc.push_back(0);
            }
            else
                enc.push_back(static_cast<uint8_t>(b));
            for (unsigned i = 0; i < 16u * b; ++i)
                enc.push_back(static_cast<uint8_t>(r.next()));
        }
        const uint32_t len = static_cast<uint32_t>(enc.size());
        enc.resize(enc.size() + 64, 0);
        std::vector<uint64_t> dec(256 + 64, 0);
        if (sc::p4Dec256v64(enc.data(), 256, dec.data()) != enc.data() + len)
            die("256v64 decode-only end pointer", w.count);
        w.record(2u, 256, 0, 8u, dec.data(), enc.data(), len);
        if (sc::p4D1Dec256v64(enc.data(), 256, dec.data(), ~0ull - 77ull) != enc.data() + len)
            die("256v64 decode-only D1 end pointer", w.count);
        w.record(3u, 256, ~0ull - 77ull, 8u, dec.data(), enc.data(), len);
    }
}

// Hand-made decode-only vectors: valid streams the encoder never emits.
static void genDecodeOnly(Writer & w)
{
    // header 0x88, bx = 0: "bitmap says no exceptions" (p4dec256v32_scalar.cpp:80-83)
    Rng r(7);
    std::vector<uint8_t> enc(2 + 256 + 64, 0);
    enc[0] = 0x80 | 8;
    enc[1] = 0;
    for (unsigned i = 0; i < 256; ++i)
        enc[2 + i] = static_cast<uint8_t>(r.next());
    std::vector<uint32_t> dec(256 + 64);
    const uint8_t * e = sc::p4Dec256v32(enc.data(), 256, dec.data());
    w.record(2u, 256, 0, 4u, dec.data(), enc.data(), static_cast<uint32_t>(e - enc.data()));
    const uint8_t * e1 = sc::p4D1Dec256v32(enc.data(), 256, dec.data(), 12345u);
    w.record(3u, 256, 12345u, 4u, dec.data(), enc.data(), static_cast<uint32_t>(e1 - enc.data()));
}

int main(int argc, char ** argv)
{
    std::string dir = argc > 1 ? argv[1] : "../tests/golden";
    {
        Writer w;
        gen32(w, F256V32, 0x256032);
        genDecodeOnly(w);
        w.save(dir + "/g256v32.bin");
    }
    {
        Writer w;
        gen32(w, F128V32, 0x128032);
        w.save(dir + "/g128v32.bin");
    }
    {
        Writer w;
        gen32(w, FH32, 0x32);
        w.save(dir + "/g32.bin");
    }
    {
        Writer w;
        gen64(w, 0x256064, false);
        gen64_short(w, 0x256065, false);
        w.save(dir + "/g256v64.bin");
    }
    {
        Writer w;
        gen64(w, 0x128064, true);
        gen64_short(w, 0x128065, true);
        w.save(dir + "/g128v64.bin");
    }
    {
        Writer w;
        gen64h(w, 0x64);
        w.save(dir + "/g64.bin");
    }
    {
        Writer w;
        gen32_short(w, F128V32, 0x128033);
        gen32_vbyte(w, F128V32, 0x128034, {128u, 100u}, 16u);
        gen32_bx0(w, F128V32, 0x128035, {128u, 100u, 7u});
        w.save(dir + "/g128v32s.bin");
    }
    {
        Writer w;
        gen32_short(w, F256V32, 0x256033);
        gen32_vbyte(w, F256V32, 0x256034, {256u, 200u}, 16u);
        gen32_bx0(w, F256V32, 0x256035, {200u, 65u});
        w.save(dir + "/g256v32s.bin");
    }
    {
        Writer w;
        gen32_vbyte(w, FH32, 0x33, {127u, 256u, 100u, 200u}, 16u);
        gen32_bx0(w, FH32, 0x34, {127u, 256u, 100u});
        w.save(dir + "/g32vb.bin");
    }
    {
        Writer w;
        gen64s_128(w, 0x128066);
        gen64s_bx0(w, 0x128067);
        w.save(dir + "/g128v64s.bin");
    }
    {
        Writer w;
        gen64s_256(w, 0x256066);
        w.save(dir + "/g256v64s.bin");
    }
    return 0;
}
