// contig_p4_map_check.cpp -- host check of csrc/contig_p4_map.hpp (no GPU, no library): the index maps of the
// four-polynomial tile of the forward 64-bit contiguous pass.
//   * every round's thread/register -> tile element map, and the store window, is a bijection on the 4096 elements;
//   * the partner of a butterfly of stage bit p is the element p bits away, in the same thread;
//   * LDS slots are distinct, inside the buffer, and additive in the way the kernel splits them (per-thread base +
//     compile-time register offset); rounds 1, 2 and the store window keep every element inside its wave;
//   * memory offsets are distinct and each store instruction of a wave covers one 512-byte run;
//   * for every lane, register and segment the twiddle index equals the index the one-polynomial tile map of
//     merge_lazy_kernels.hpp uses for the same ring position.
// today_index / today_elem below are TRANSCRIPTIONS of the one-polynomial map (load_twiddles and kern::elem_of are device
// code inside pass_body and cannot be called from here), so this program compares two readings of the same layout; that
// the kernel itself computes the right words is what the bit-exact GPU tests (tests/test_gpu_contig_p4.py) establish.
// Prints "OK <checks>" and returns 0, or the first mismatch and 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "contig_p4_map.hpp"

namespace p4 = gpuntt::kern::p4;

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

// the one-polynomial tile (merge_lazy_kernels.hpp: load_twiddles): prepared-table index of the butterfly of stage bit p
// whose lower element lies at ring position pos -- [tile][k][thread] for the distance-1/2/4 stages, plain above
static unsigned today_index(int n, unsigned pos, int p)
{
    const unsigned stage = 1u << (n - 1 - p);
    if (p <= 2)
        return stage + (pos >> 12) * ((8u >> p) * 256u) + ((pos & 15u) >> (p + 1)) * 256u + ((pos >> 4) & 255u);
    return stage + (pos >> (p + 1));
}
// register window of the one-polynomial tile (kern::elem_of)
static unsigned today_elem(int w, unsigned t, unsigned j) { return (t & ((1u << w) - 1u)) | (j << w) | ((t >> w) << (w + 4)); }

int main()
{
    constexpr unsigned TILE = 1u << p4::TLOG, NT = p4::NT, EPT = 1u << p4::RB;
    // stage bits of the rounds: 9, 8 | 7..4 | 3..0
    const int first_pos[3] = {9, 7, 3}, stages[3] = {2, 4, 4};

    for (int r = 0; r <= p4::ROUNDS; r++) // r == ROUNDS: the store window
    {
        std::vector<int> seen(TILE, 0), slot_seen(p4::LDS_ELEMS, 0);
        for (unsigned t = 0; t < NT; t++)
            for (unsigned j = 0; j < EPT; j++)
            {
                const unsigned e = r < p4::ROUNDS ? p4::elem(r, t, j) : p4::elem_out(t, j);
                REQUIRE(e < TILE, "round %d t %u j %u", r, t, j);
                REQUIRE(seen[e]++ == 0, "round %d: element %u twice", r, e);
                const unsigned s = p4::lds_slot(e);
                REQUIRE(s < static_cast<unsigned>(p4::LDS_ELEMS), "slot %u outside the buffer", s);
                REQUIRE(slot_seen[s]++ == 0, "round %d: slot %u twice", r, s);
                // per-thread base + register offset
                const unsigned e0 = r < p4::ROUNDS ? p4::elem(r, t, 0) : p4::elem_out(t, 0);
                const unsigned ej = r < p4::ROUNDS ? p4::elem(r, 0, j) : p4::elem_out(0, j);
                REQUIRE(e == (e0 | ej) && (e0 & ej) == 0, "round %d: element not split", r);
                REQUIRE(s == p4::lds_slot(e0) + p4::lds_slot(ej), "round %d: slot not additive", r);
                if (r < p4::ROUNDS)
                {
                    // the register offset is the one the other kernels use (kern::lds_joff<WL>)
                    const unsigned jw = j << p4::window(r);
                    REQUIRE(p4::lds_slot(ej) == jw + (jw >> 4), "round %d: register offset", r);
                }
                if (r == 0) // wave = polynomial
                    REQUIRE((e >> p4::K) == (t >> 6), "round 0: wave %u holds polynomial %u", t >> 6, e >> p4::K);
                else // wave = tile bits 8, 9: the exchanges behind the block barrier stay inside the wave
                    REQUIRE(((e >> 8) & 3u) == (t >> 6), "round %d: element %u outside wave %u", r, e, t >> 6);
                if (r == 1 || r == 2)
                    REQUIRE((e >> p4::K) == ((t >> 4) & 3u), "round %d: lane bits 4, 5 select the polynomial", r);
            }
    }

    // memory: distinct offsets; loads of round 0 and stores of the store window in 512-byte runs per wave instruction
    for (unsigned long long stride : {1ull << 16, 2ull << 16, 3ull << 16, 8ull << 16})
    {
        std::vector<unsigned long long> offs;
        for (unsigned e = 0; e < TILE; e++)
        {
            const unsigned long long o = p4::mem_offset(e, stride);
            REQUIRE(o == (e >> 10) * stride + (e & 1023u), "offset of %u", e);
            offs.push_back(o);
        }
        for (unsigned e = 1; e < TILE; e++)
            REQUIRE(offs[e] > offs[e - 1], "offsets not increasing at %u", e);
        for (unsigned t = 0; t < NT; t += 64)
            for (unsigned j = 0; j < EPT; j++)
                for (unsigned l = 1; l < 64; l++)
                {
                    REQUIRE(p4::mem_offset(p4::elem(0, t + l, j), stride) == p4::mem_offset(p4::elem(0, t, j), stride) + l,
                            "load run");
                    REQUIRE(p4::mem_offset(p4::elem_out(t + l, j), stride) == p4::mem_offset(p4::elem_out(t, j), stride) + l,
                            "store run");
                }
    }

    // twiddles: the index the kernel computes == the one-polynomial map's index for the same ring position
    for (int n : {16, 14, 18})
        for (unsigned seg = 0; seg < (1u << (n - p4::K)); seg += (n == 16 ? 1 : 5))
            for (int r = 0; r < p4::ROUNDS; r++)
                for (int s = 0; s < stages[r]; s++)
                {
                    const int p = first_pos[r] - s, jb = p - p4::window(r);
                    for (unsigned t = 0; t < NT; t++)
                        for (unsigned h = 0; h < EPT / 2; h++)
                        {
                            const unsigned j0 = (h & ((1u << jb) - 1u)) | ((h >> jb) << (jb + 1)), j1 = j0 | (1u << jb);
                            const unsigned kk = j0 >> (jb + 1);
                            const unsigned e0 = p4::elem(r, t, j0), e1 = p4::elem(r, t, j1);
                            REQUIRE(e1 == (e0 | (1u << p)) && (e0 & (1u << p)) == 0, "butterfly partner, stage %d", p);
                            const unsigned want = today_index(n, p4::ring_pos(seg, e0), p);
                            const unsigned got = r == 2   ? p4::tw_lane_index(n, seg, t, p, kk)
                                                 : r == 1 ? p4::tw_uniform_index(n, seg, t >> 6, p, kk)
                                                          : p4::tw_uniform_index(n, seg, 0, p, kk);
                            REQUIRE(got == want, "n %d seg %u stage %d t %u kk %u: %u, the one-polynomial map gives %u", n, seg, p,
                                    t, kk, got, want);
                            REQUIRE(got < (1u << n), "index outside the table");
                        }
                }

    // the one-polynomial tile's own windows give the same ring positions for the same (segment, polynomial) pair: tile
    // element e of polynomial 0 of segment seg is element ((seg & 3) << 10) | e of ring tile seg >> 2
    for (unsigned t = 0; t < NT; t++)
        for (unsigned j = 0; j < EPT; j++)
        {
            const unsigned e = today_elem(6, t, j); // wave = tile bits 10, 11 there
            REQUIRE(p4::ring_pos(t >> 6, p4::elem(0, (t & 63u), j)) == e, "round 0 window");
        }

    // round 2: the four 16-lane rows of a wave read the same addresses (256 bytes per load instruction)
    for (unsigned t = 0; t < NT; t++)
        for (int p = 0; p <= 3; p++)
        {
            REQUIRE(p4::tw_lane_index(16, 7, t, p, 0) == p4::tw_lane_index(16, 7, t & ~48u, p, 0), "rows differ");
            if ((t & 15u) != 0)
                REQUIRE(p4::tw_lane_index(16, 7, t, p, 0) == p4::tw_lane_index(16, 7, t - 1, p, 0) + 1, "lanes not consecutive");
        }

    std::printf("OK %llu\n", checks);
    return 0;
}
