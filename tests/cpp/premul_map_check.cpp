// premul_map_check.cpp -- host check of the hoisted first twiddle product of the forward 64-bit ring 2^16 (csrc/
// contig_p4_map.hpp: namespace premul; no GPU, no library).
//   * Maps.  Every tile of the strided K = 6 pass of every polynomial of a batch is walked, thread by thread and register
//     by register, for mod_count 1 and 3: the positions the pass multiplies are exactly the ring positions with bit 9 set,
//     each once; the test "is this tile multiplied" is the same for all of a tile; the 16 table entries a wave reads
//     (one base index + the register number) are, entry for entry, the table slot the four-polynomial last pass reads
//     today for the first stage of that polynomial's segment -- the modulus slot of an RNS stack included.
//   * Ranges, in exact 128-bit integers, for the widest modulus of each family (31 q: the largest q with 31 q < 2^64,
//     hand-off cap 19; 16 q: the largest 60-bit q, cap 12): with U below cap q and T below 4 q, the new first stage
//     U' = U + T, V' = 2 U + 4 q - U' (mod 2^64) gives the exact values U + T and U - T + 4 q, both below LIMIT q and
//     below 2^64, at the corners U = cap q - 1 / 0 and T = 4 q - 1 / 0.
// contig_block / today_index are TRANSCRIPTIONS of merge_pass_lazy's P4 block map and of the one-polynomial twiddle
// index (device code); that the kernels compute the right words is what tests/test_gpu_premul.py establishes.
// Prints "OK <checks>" and returns 0, or the first mismatch and 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "contig_p4_map.hpp"

namespace p4 = gpuntt::kern::p4;
namespace premul = gpuntt::kern::premul;

static unsigned long long checks = 0;
#define REQUIRE(cond, ...)                                                                                               \
    do                                                                                                                   \
    {                                                                                                                    \
        checks++;                                                                                                        \
        if (!(cond))                                                                                                     \
        {                                                                                                                \
            std::printf("WRONG %s:%d %s: ", __FILE__, __LINE__, #cond);                                                  \
            std::printf(__VA_ARGS__);                                                                                    \
            std::printf("\n");                                                                                           \
            std::exit(1);                                                                                                \
        }                                                                                                                \
    } while (0)

// the one-polynomial tile's index of the butterfly of stage bit p >= 3 at ring position pos (load_twiddles)
static unsigned today_index(int n, unsigned pos, int p) { return (1u << (n - 1 - p)) + (pos >> (p + 1)); }

typedef unsigned __int128 u128;

static void range_check(const char* family, uint64_t q, unsigned cap, unsigned limit)
{
    const u128 two64 = static_cast<u128>(1) << 64;
    REQUIRE(static_cast<u128>(limit) * q < two64, "%s: LIMIT q does not fit the word", family);
    const uint64_t us[2] = {cap * q - 1, 0}, ts[2] = {4 * q - 1, 0};
    for (uint64_t U : us)
        for (uint64_t T : ts)
        {
            const uint64_t nu = U + T;                 // v_lshl_add_u64
            const uint64_t nv = (2 * U + 4 * q) - nu; // shl1_add, subtract: mod 2^64
            const u128 eu = static_cast<u128>(U) + T, ev = static_cast<u128>(U) + 4 * static_cast<u128>(q) - T;
            REQUIRE(eu < two64 && ev < two64, "%s: an output passes 2^64", family);
            REQUIRE(nu == static_cast<uint64_t>(eu) && nv == static_cast<uint64_t>(ev), "%s: wrapped", family);
            REQUIRE(eu < static_cast<u128>(limit) * q && ev < static_cast<u128>(limit) * q, "%s: an output passes LIMIT q", family);
            REQUIRE(eu <= static_cast<u128>(cap + 4) * q && ev <= static_cast<u128>(cap + 4) * q,
                    "%s: an output passes the bound the schedule continues from", family);
            REQUIRE(nu % q == static_cast<uint64_t>((static_cast<u128>(U % q) + T % q) % q), "%s: U' is not U + T", family);
            REQUIRE(nv % q == static_cast<uint64_t>((static_cast<u128>(U % q) + q - T % q) % q), "%s: V' is not U - T", family);
        }
}

int main()
{
    constexpr int N = 16, K = 6;
    constexpr unsigned NT = p4::NT, EPT = 1u << p4::RB, RING = 1u << N, TILES = RING >> p4::TLOG;
    for (unsigned mc : {1u, 3u})
    {
        const unsigned polys = 8 * mc; // two groups of four polynomials per modulus
        // the last pass today: (polynomial, segment) -> table slot of its first stage, block by block
        // (merge_pass_lazy<..., P4>: block -> segment, modulus, first polynomial; wave w = polynomial poly0 + w * mc)
        std::map<std::pair<unsigned, unsigned>, unsigned long long> contig;
        const int seg_log = N - p4::K;
        for (unsigned bx = 0; bx < (polys << seg_log) / 4; bx++)
        {
            const unsigned seg = bx & ((1u << seg_log) - 1u), pm = bx >> seg_log, mi = pm % mc;
            const unsigned poly0 = (pm / mc) * (4 * mc) + mi;
            for (unsigned w = 0; w < 4; w++)
            {
                const unsigned long long slot = (static_cast<unsigned long long>(mi) << N) + premul::tw_index_contig(N, seg);
                REQUIRE(contig.emplace(std::make_pair(poly0 + w * mc, seg), slot).second, "segment %u of polynomial %u twice", seg,
                        poly0 + w * mc);
            }
        }
        REQUIRE(contig.size() == static_cast<size_t>(polys) << seg_log, "the last pass does not cover the batch");

        for (unsigned poly = 0; poly < polys; poly++)
        {
            const unsigned mi = poly % mc; // merge_pass_lazy: polynomial index of the tile % mod_count
            std::vector<int> seen(RING, 0), multiplied(RING, 0);
            for (unsigned b = 0; b < TILES; b++)
                for (unsigned t = 0; t < NT; t++)
                {
                    // what the kernel computes once per wave: position of register 0 of the wave's first thread
                    const unsigned pos0 = premul::strided_ring_pos(N, K, b, premul::strided_elem(K, t & ~63u, 0));
                    const bool tile_mul = premul::premultiplied(pos0);
                    REQUIRE(tile_mul == premul::premultiplied(premul::strided_ring_pos(N, K, b, 0)), "the test differs inside tile %u", b);
                    for (unsigned j = 0; j < EPT; j++)
                    {
                        const unsigned e = premul::strided_elem(K, t, j);
                        REQUIRE(e < (1u << p4::TLOG), "element outside the tile");
                        const unsigned pos = premul::strided_ring_pos(N, K, b, e);
                        REQUIRE(pos < RING && seen[pos]++ == 0, "ring position %u twice", pos);
                        REQUIRE(premul::premultiplied(pos) == tile_mul, "bit 9 differs inside tile %u", b);
                        REQUIRE(premul::premultiplied(pos) == (((pos >> 9) & 1u) != 0u), "not bit 9");
                        if (!tile_mul)
                            continue;
                        multiplied[pos]++;
                        // the kernel: one base index per wave + the register number
                        const unsigned idx = premul::tw_index(N, pos0) + j;
                        REQUIRE(idx == premul::tw_index(N, pos), "register %u of thread %u does not follow the base index", j, t);
                        REQUIRE(idx == today_index(N, pos & ~(1u << premul::BIT), premul::BIT), "not the slot of stage bit 9");
                        REQUIRE(idx < RING, "index outside the table of the modulus");
                        const unsigned long long slot = (static_cast<unsigned long long>(mi) << N) + idx;
                        const auto it = contig.find(std::make_pair(poly, pos >> p4::K));
                        REQUIRE(it != contig.end() && it->second == slot, "polynomial %u position %u: slot %llu, the last pass reads %llu",
                                poly, pos, slot, it == contig.end() ? 0ull : it->second);
                    }
                }
            for (unsigned pos = 0; pos < RING; pos++)
            {
                REQUIRE(seen[pos] == 1, "ring position %u not covered", pos);
                REQUIRE(multiplied[pos] == static_cast<int>((pos >> 9) & 1u), "ring position %u multiplied %d times", pos, multiplied[pos]);
            }
        }
    }

    range_check("31 q", UINT64_MAX / 31, 19, 31);
    range_check("16 q", (1ull << 60) - 1, 12, 16);

    std::printf("OK %llu\n", checks);
    return 0;
}
