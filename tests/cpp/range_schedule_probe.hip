// range_schedule_probe.hip -- prints, as compiled from the headers, the range-correction schedule (kern::PassSched) of
// every forward 64-bit pass shape lazy_launch_impl.hpp instantiates, and what the host's run-time twin
// (host::fwd_plan_bounds / fwd_bound_after) reports for the plans of the rings 2^13 .. 2^18.  Host code only: no HIP call.
// tests/test_range_schedule_host.py replays the tables with exact integer bounds.
//
//   S lim tile tlog contig k in cap last est limit tb final nrounds
//   R stages bin | jb ku[h = 0 .. 7] (per stage) | bout[0 .. 15]          one line per round of the S line above it
//   T lim tlog contig k in cap out                                        fwd_bound_after for the same shape (est only)
//   C lim cap10                                                           host::fwd_handoff_cap10
//   P lim n polys tl npass  /  Q contig k tlp first last in_b inst cap out one P line per plan, one Q line per pass
#include <cstdio>

#include "lazy_launch.hpp"

using namespace gpuntt;

template <int LIMSEL, int TLOG, bool CONTIG, int K, int IN, int CAP, bool LAST> static void sched(const char* tile)
{
    using M = lazy::Mod<uint64_t, LIMSEL>;
    constexpr bool EST = kern::plans_whole_pass<uint64_t, false, false, true>(M::LIMIT);
    using S = kern::PassSched<TLOG, false, CONTIG, K, IN, M::LIMIT, M::TB, 0, CAP, EST>;
    std::printf("S %d %s %d %d %d %d %d %d %d %d %d %d %d\n", LIMSEL, tile, TLOG, int(CONTIG), K, IN, CAP, int(LAST), int(EST),
                M::LIMIT, M::TB, S::d.final_bound, S::NR);
    for (int r = 0; r < S::NR; r++)
    {
        std::printf("R %d %d |", S::stages_of(r), S::d.bin[r]);
        for (int s = 0; s < S::stages_of(r); s++)
        {
            std::printf(" %d", S::first_pos(r) - s - S::wl_of(r));
            for (int h = 0; h < kern::EPT / 2; h++)
                std::printf(" %d", S::d.ku[r][s][h]);
            std::printf(" |");
        }
        for (int j = 0; j < kern::EPT; j++)
            std::printf(" %d", S::d.bout[r][j]);
        std::printf("\n");
    }
    if (EST)
        std::printf("T %d %d %d %d %d %d %d\n", LIMSEL, TLOG, int(CONTIG), K, IN, CAP, host::fwd_bound_after(IN, K, M::LIMIT, CAP));
}

// the shapes of dispatch_tl<uint64_t, TLOG, false, LIMSEL> (lazy_launch_impl.hpp), in its order
template <int LIMSEL> static void family()
{
    constexpr int LIM = lazy::Mod<uint64_t, LIMSEL>::LIMIT;
    constexpr bool CAPPED = LIM == 16 || LIM == 31;
#define ONE(CONTIG_, K_, IN_, LAST_) sched<LIMSEL, 12, CONTIG_, K_, IN_, 0, LAST_>("p1")
    ONE(true, 1, 1, true);
    ONE(true, 2, 1, true);
    ONE(true, 3, 1, true);
    ONE(true, 4, 1, true);
    ONE(true, 5, 1, true);
    ONE(true, 6, 1, true);
    ONE(true, 7, 1, true);
    ONE(true, 8, 1, true);
    ONE(true, 9, 1, true);
    ONE(true, 10, 1, true);
    ONE(true, 11, 1, true);
    ONE(true, 12, 1, true);
    ONE(true, 8, LIM, true);
    ONE(true, 9, LIM, true);
    ONE(true, 10, LIM, true);
    sched<LIMSEL, 12, true, 10, LIM, 0, true>("p4");
    ONE(true, 11, LIM, true);
    ONE(true, 12, LIM, true);
    if constexpr (CAPPED)
    {
        constexpr int CAP10 = host::FwdBounds<LIM>::CAP10;
        std::printf("C %d %d\n", LIMSEL, CAP10);
        sched<LIMSEL, 12, true, 10, CAP10, 0, true>("p1");
        sched<LIMSEL, 12, true, 10, CAP10, 0, true>("p4");
        sched<LIMSEL, 12, false, 4, 1, CAP10, false>("p1");
        sched<LIMSEL, 12, false, 6, 1, CAP10, false>("p1");
    }
#define BOTH(K_)                                                                                                               \
    ONE(false, K_, 1, false);                                                                                                  \
    ONE(false, K_, LIM, false);
    BOTH(1)
    BOTH(2)
    BOTH(3)
    BOTH(4)
    BOTH(5)
    BOTH(6)
    BOTH(7)
    BOTH(8)
#undef BOTH
#undef ONE
    if constexpr (LIMSEL == 0 || LIMSEL == 31)
    {
        sched<LIMSEL, 13, true, 13, 1, 0, true>("p1");
        sched<LIMSEL, 13, true, 13, LIM, 0, true>("p1");
        sched<LIMSEL, 14, true, 14, 1, 0, true>("p1");
        sched<LIMSEL, 14, true, 14, LIM, 0, true>("p1");
        sched<LIMSEL, 14, false, 9, 1, 0, false>("p1");
        sched<LIMSEL, 14, false, 10, 1, 0, false>("p1");
    }
    if constexpr (LIMSEL == 0)
        sched<LIMSEL, 14, true, 13, LIM, 0, true>("p1");
}

static void plans(int lim)
{
    const int limit = lim == 31 ? 31 : 16;
    for (int n = 13; n <= 18; n++)
        for (unsigned long long polys : {1ull, 3ull, 4ull, 255ull, 256ull, 1024ull})
        {
            const int tl = host::lazy_tile_log_merge<uint64_t>(n, false, polys);
            host::Plan pl = host::make_plan_tl(n, tl, tl == 12 ? host::lazy_contig_k_merge<uint64_t>(n, false) : tl, 8);
            int out[8] = {};
            // (fwd_plan_bounds, pass by pass: the hand-off of each pass is the bound the next one reads)
            const int fin = host::fwd_plan_bounds(pl, tl, false, limit);
            for (int i = 0; i < pl.count; i++)
                out[i] = i + 1 < pl.count ? pl.pass[i + 1].in_b : fin;
            std::printf("P %d %d %llu %d %d\n", lim, n, polys, tl, pl.count);
            for (int i = 0; i < pl.count; i++)
            {
                const host::Pass& p = pl.pass[i];
                const int tlp = host::fwd_pass_tile64(p, tl);
                std::printf("Q %d %d %d %d %d %d %d %d %d\n", int(p.contig), p.k, tlp, int(i == 0), int(i == pl.count - 1), p.in_b,
                            host::fwd_inst_bound(p, tlp, i == 0, i == pl.count - 1, limit), p.cap, out[i]);
            }
        }
}

int main()
{
    family<0>();
    family<31>();
    family<8>();
    family<4>();
    plans(0);
    plans(31);
    return 0;
}
