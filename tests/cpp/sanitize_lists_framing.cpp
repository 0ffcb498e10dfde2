// Host-side sanitizer driver of the lists framing (built with
// -fsanitize=address,undefined by tests/test_lists_scan_cpu.py):
// tpf_lists_scan_offsets (turbopfor-cpp_amd/csrc/framing.cpp) fed valid,
// corrupted, truncated and random lists streams, with and without per-list
// anchors.  Every stream sits in a heap buffer of exactly its size and every
// offsets array holds exactly nunits + 1 entries, so any access past either is
// an ASan error.  A valid stream must give back the offsets it was written
// with; whatever the bytes, the offsets of a call with anchors never decrease
// and end at list_byte[nlists].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/turbopfor_capi.h"
#include "../../oracle/tpf_oracle.h"

namespace
{

int fails = 0;
#define CHECK(c)                                                                                                                 \
    do                                                                                                                           \
    {                                                                                                                            \
        if (!(c))                                                                                                                \
        {                                                                                                                        \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c);                                          \
            ++fails;                                                                                                             \
        }                                                                                                                        \
    } while (0)

struct Index
{
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off, ptr, lbyte;
};

// lists of random lengths around the unit size, every block of a random width and exception rate
Index build(std::mt19937_64 & rng)
{
    Index X;
    const uint64_t nlists = 1 + rng() % 12;
    X.ptr.push_back(rng() % 1000);
    X.lbyte.push_back(0);
    std::vector<uint8_t> buf(256 * 9 + 64);
    for (uint64_t j = 0; j < nlists; ++j)
    {
        static const unsigned lens[] = {0, 0, 1, 7, 100, 255, 256, 257, 511, 512, 700, 256 * 5 + 3};
        const unsigned n = lens[rng() % 12];
        for (unsigned at = 0; at < n; at += 256)
        {
            const unsigned cnt = n - at < 256 ? n - at : 256;
            const unsigned bw = 1 + rng() % 32, pct = (rng() % 4) * 8;
            std::vector<uint32_t> v(cnt);
            for (auto & x : v)
            {
                x = static_cast<uint32_t>(rng() & ((1ull << bw) - 1));
                if (rng() % 100 < pct)
                    x = static_cast<uint32_t>(rng());
            }
            if (rng() % 9 == 0)
                std::fill(v.begin(), v.end(), v[0]);
            X.off.push_back(X.bytes.size());
            uint8_t * e = cnt == 256 ? orc_p4enc256v32(v.data(), 256, buf.data()) : orc_p4enc32(v.data(), cnt, buf.data());
            X.bytes.insert(X.bytes.end(), buf.data(), e);
        }
        X.ptr.push_back(X.ptr.back() + n);
        X.lbyte.push_back(X.bytes.size());
    }
    X.off.push_back(X.bytes.size());
    return X;
}

// One call on exactly-sized heap buffers.  -> the return value; *out the offsets
int64_t run(const uint8_t * bytes, uint64_t len, const Index & X, bool anchors, uint64_t nunits, std::vector<uint64_t> * out)
{
    uint8_t * buf = static_cast<uint8_t *>(std::malloc(len ? len : 1));
    std::memcpy(buf, bytes, len);
    uint64_t * off = static_cast<uint64_t *>(std::malloc(8 * (nunits + 1)));
    std::memset(off, 0x5A, 8 * (nunits + 1));
    const int64_t r = tpf_lists_scan_offsets(buf, len, X.ptr.data(), X.ptr.size() - 1, anchors ? X.lbyte.data() : nullptr, off, nunits);
    out->assign(off, off + nunits + 1);
    std::free(off);
    std::free(buf);
    return r;
}

void never_decreasing(const std::vector<uint64_t> & off, uint64_t end)
{
    for (size_t i = 0; i + 1 < off.size(); ++i)
        CHECK(off[i] <= off[i + 1]);
    CHECK(off.back() == end);
}

} // namespace

int main(int argc, char ** argv)
{
    const unsigned rounds = argc > 1 ? static_cast<unsigned>(std::atoi(argv[1])) : 40;
    std::mt19937_64 rng(4321);
    uint64_t units = 0;
    for (unsigned rd = 0; rd < rounds; ++rd)
    {
        const Index X = build(rng);
        const uint64_t nunits = X.off.size() - 1, len = X.bytes.size();
        std::vector<uint64_t> off;
        for (bool anchors : {false, true})
        {
            CHECK(run(X.bytes.data(), len, X, anchors, nunits, &off) == static_cast<int64_t>(len));
            CHECK(off == X.off);
            // a wrong unit count is refused before anything is read or written
            CHECK(run(X.bytes.data(), len, X, anchors, nunits + 1, &off) == -static_cast<int64_t>(nunits + 1 + X.ptr.size() - 1) - 1);
        }
        // corrupted: a few bytes flipped, headers included
        for (int rep = 0; rep < 8 && len; ++rep)
        {
            std::vector<uint8_t> bad(X.bytes);
            for (int k = 0; k < 1 + static_cast<int>(rng() % 4); ++k)
                bad[rng() % len] ^= static_cast<uint8_t>(1 + rng() % 255);
            const int64_t r = run(bad.data(), len, X, true, nunits, &off);
            CHECK(r == static_cast<int64_t>(len) || (r < 0 && static_cast<uint64_t>(-r - 1) < nunits));
            never_decreasing(off, len);
            (void)run(bad.data(), len, X, false, nunits, &off);
        }
        // truncated: the anchors now end past the stream (a structure refusal), the chained walk stops at a unit
        for (uint64_t cut = 0; cut < len && cut < 48; ++cut)
        {
            const uint64_t keep = rd % 2 ? cut : len - 1 - cut;
            CHECK(run(X.bytes.data(), keep, X, true, nunits, &off) <= -static_cast<int64_t>(nunits) - 1);
            const int64_t r = run(X.bytes.data(), keep, X, false, nunits, &off);
            CHECK(r < 0 && static_cast<uint64_t>(-r - 1) < nunits);
        }
        // random bytes under the same structure
        std::vector<uint8_t> junk(len);
        for (auto & x : junk)
            x = static_cast<uint8_t>(rng());
        (void)run(junk.data(), len, X, true, nunits, &off);
        if (nunits)
            never_decreasing(off, len);
        (void)run(junk.data(), len, X, false, nunits, &off);
        units += nunits;
    }
    std::printf("sanitize_lists_framing: %llu units, %d failures\n", static_cast<unsigned long long>(units), fails);
    return fails ? 1 : 0;
}
