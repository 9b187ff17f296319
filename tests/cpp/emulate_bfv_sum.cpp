// emulate_bfv_sum.cpp -- bfv_tensor_sum on the CPU: the kernel's own text (the kern namespace of csrc/bfv_multiply_sum.hip,
// cut out by tests/bfv_sum_utils.py into kernel_extract.inc) compiled for the host against host_shim/hip/hip_runtime.h --
// one std::thread per lane -- under AddressSanitizer and UBSan.  It checks the index arithmetic, the bounds of every access
// (the operand region lies between guard bands), both loaders, the slot bytes of the kernel argument, the in-place output
// and the arithmetic at the edges of the word; it says nothing about waves or time.  A plain clang++ builds it (no hipcc,
// no GPU, nothing preloaded).  The fold constants are derived here, in exact integers, not by the library.
//   emulate_bfv_sum JOB RESULT   JOB: 64-bit words -- the number of cases, then per case W, n_power, M, count, slots, terms,
//                                off (words by which the region leaves 16-byte alignment), the M moduli, x_slot[terms],
//                                y_slot[terms], e[slots][2][count][M][N]
//                                RESULT: per case d[3][count][M][N], the first three planes of e after the launch
//                                one line per case, then "ALL OK" or "FAILED" (a guard band was touched, or a word of e
//                                behind the three planes changed)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

#include "bfv_multiply_sum_internal.hpp"
#include "inner_product_internal.hpp"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
std::barrier<>* g_block_barrier = nullptr;

namespace gpuntt
{
    namespace kern
    {
#include "kernel_extract.inc"
    } // namespace kern
} // namespace gpuntt

using namespace gpuntt;
using U64 = unsigned long long;
using U128 = unsigned __int128;

// kernel(): one lane's call, with the launch's arguments bound
template <typename Kernel> void launch(dim3 grid, unsigned nt, Kernel kernel)
{
    for (unsigned by = 0; by < grid.y; by++)
        for (unsigned bx = 0; bx < grid.x; bx++)
        {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; t++)
                th.emplace_back([&, t] {
                    threadIdx = dim3(t), blockIdx = dim3(bx, by), blockDim = dim3(nt), gridDim = grid;
                    kernel();
                });
            for (auto& x : th)
                x.join();
        }
}

// `w` words between two guard bands of 32 words, the first word `off` behind a 16-byte boundary
template <typename T> struct Guarded
{
    std::vector<T> store;
    size_t words, off;
    Guarded(size_t w, size_t o) : store(w + 64 + o + 4, T(0x5A)), words(w), off(o) {}
    T* data()
    {
        const size_t skew = (reinterpret_cast<uintptr_t>(store.data()) % 16) / sizeof(T);
        return store.data() + 32 + off + (skew ? 16 / sizeof(T) - skew : 0);
    }
    size_t touched()
    {
        size_t bad = 0;
        for (T* p = store.data(); p < data(); p++)
            bad += *p != T(0x5A);
        for (T* p = data() + words; p < store.data() + store.size(); p++)
            bad += *p != T(0x5A);
        return bad;
    }
};

static std::vector<U64> g_job;
static size_t g_at = 0;
static U64 next() { return g_job.at(g_at++); }

template <typename T> size_t run_case(int n, int M, int count, int slots, int terms, int off, std::FILE* res)
{
    constexpr int W = 8 * sizeof(T), VW = 16 / sizeof(T);
    const size_t N = size_t(1) << n, plane = size_t(count) * M * N;
    std::vector<U64> mods(M);
    for (auto& m : mods)
        m = next();
    kern::BfvSumArgs args{};
    args.terms = terms;
    for (int t = 0; t < terms; t++)
        args.x_slot[t] = static_cast<unsigned char>(next());
    for (int t = 0; t < terms; t++)
        args.y_slot[t] = static_cast<unsigned char>(next());
    Guarded<T> e(size_t(slots) * 2 * plane, off);
    for (size_t i = 0; i < e.words; i++)
        e.data()[i] = T(next());
    const std::vector<T> before(e.data(), e.data() + e.words);

    std::vector<T> fold(6 * size_t(M));
    auto shoup = [](U64 v, U64 m) { return T((U128(v) << W) / m); };
    for (int m = 0; m < M; m++)
    {
        const U64 q = mods[m], t1 = U64((U128(1) << W) % q), t2 = U64(U128(t1) * t1 % q);
        fold[m] = T(q), fold[M + m] = T(t1), fold[2 * M + m] = shoup(t1, q);
        fold[3 * M + m] = T(t2), fold[4 * M + m] = shoup(t2, q), fold[5 * M + m] = shoup(1, q);
    }

    const bool vec = host::relin_wide<T>(n, {e.data()});
    const host::RelinGrid g = host::relin_grid(n, vec ? VW : 1, count);
    const dim3 grid(g.blocks, M);
    if (vec)
        launch(grid, g.nt, [&] { kern::bfv_tensor_sum<T, VW>(e.data(), fold.data(), args, count, M, n, g.tiles); });
    else
        launch(grid, g.nt, [&] { kern::bfv_tensor_sum<T, 1>(e.data(), fold.data(), args, count, M, n, g.tiles); });

    size_t bad = e.touched();
    for (size_t i = 3 * plane; i < e.words; i++) // what lies behind d0, d1, d2 is nobody's output
        bad += e.data()[i] != before[i];
    for (size_t i = 0; i < 3 * plane; i++)
    {
        const U64 w = e.data()[i];
        std::fwrite(&w, sizeof(w), 1, res);
    }
    std::printf("W=%d n=%d M=%d count=%d slots=%d terms=%d off=%d vec=%d tiles=%u: %s (%zu)\n", W, n, M, count, slots,
                terms, off, vec, g.tiles, bad ? "TOUCHED" : "ok", bad);
    return bad;
}

int main(int argc, char** argv)
{
    if (argc != 3)
        return 2;
    std::FILE* job = std::fopen(argv[1], "rb");
    if (job == nullptr)
        return 2;
    U64 w;
    while (std::fread(&w, sizeof(w), 1, job) == 1)
        g_job.push_back(w);
    std::fclose(job);
    std::FILE* res = std::fopen(argv[2], "wb");
    if (res == nullptr)
        return 2;
    size_t bad = 0;
    const U64 cases = next();
    for (U64 c = 0; c < cases; c++)
    {
        const int W = int(next()), n = int(next()), M = int(next()), count = int(next()), slots = int(next()),
                  terms = int(next()), off = int(next());
        bad += W == 64 ? run_case<Data64>(n, M, count, slots, terms, off, res)
                       : run_case<Data32>(n, M, count, slots, terms, off, res);
    }
    std::fclose(res);
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
