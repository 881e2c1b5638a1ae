// Known answers of the folded draw (csrc/drt_fold.h, compiled here for the host) against the definition (include/drt_hip.h):
// combine_folded(fold16(h), fold16(k)) == drt_rng_combine(h, k), all 31 bits, for
//   h: the 65,536 words a << 16 | a (whose fold has a zero low half), 0, 0xFFFFFFFF, 0x80000000, 0x0000FFFF, 10^6 pseudo-random words;
//   k: 0, 1, 0xFFFF, 0x10000, 0xFFFFFFFF and 64 consecutive keys across a multiple of 2^16 (the key's carry into its high half).
#include "../../include/drt_hip.h"
#include "../../differentiable-renderer_amd/csrc/drt_fold.h"

#include <cstdio>
#include <vector>

int main()
{
    std::vector<uint32_t> hs, ks = {0u, 1u, 0xFFFFu, 0x10000u, 0xFFFFFFFFu};
    for (uint32_t i = 0; i < 64; ++i)
        ks.push_back(0x00030000u - 32u + i);
    for (uint32_t a = 0; a < 65536u; ++a)
        hs.push_back(a << 16 | a);
    for (uint32_t h : {0u, 0xFFFFFFFFu, 0x80000000u, 0x0000FFFFu})
        hs.push_back(h);
    uint32_t x = 2463534242u;                              // xorshift32: a generator that shares nothing with drt_mix32
    for (int i = 0; i < 1000000; ++i) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        hs.push_back(x);
    }
    unsigned long long n = 0, bad = 0;
    for (uint32_t h : hs) {
        const uint32_t hf = fold16(h);
        for (uint32_t k : ks) {
            const uint32_t want = drt_rng_combine(h, k), got = combine_folded(hf, fold16(k));
            ++n;
            if (got != want && bad++ < 5)
                std::printf("h = %08x k = %08x: folded %08x, drt_rng_combine %08x\n", h, k, got, want);
        }
    }
    // ... and through the whole draw, as the kernels write it: index hash, fold, combine
    for (uint32_t nidx = 0; nidx < 130; ++nidx)
        for (uint32_t k : ks) {
            const uint32_t stream = drt_rng_stream(1u + nidx, 0u);
            const drt_rng_key key = {stream, k};
            ++n;
            if (combine_folded(fold16(drt_rng_index_hash(stream, nidx)), fold16(k)) != drt_rng_draw(key, nidx) && bad++ < 5)
                std::printf("draw %u of key %08x differs\n", nidx, k);
        }
    std::printf("folded draw: %llu pairs of %zu index hashes and %zu keys, %llu differ\n", n, hs.size(), ks.size(), bad);
    if (bad == 0 && hs.size() == 65536u + 4u + 1000000u && ks.size() == 69u) { std::printf("ok\n"); return 0; }
    return 1;
}
