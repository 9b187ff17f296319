// emulate_bfv_encode.cpp -- bfv_slot_permute, lift_centred and multiply_plain on the CPU: the kernels' own text (the kern
// namespaces of csrc/bfv_encode.hip and csrc/keygen.hip, cut out by tests/encode_utils.py into permute_extract.inc and
// kernel_extract.inc, over the accumulator and the fold of csrc/inner_product_internal.hpp) compiled for the host against
// host_shim/hip/hip_runtime.h -- one std::thread per lane -- under AddressSanitizer and UBSan.  It checks the index
// arithmetic, the bounds of every access (every buffer lies between guard bands), both loaders, the batch slices of the
// permutation and the in-place product; it says nothing about waves or time.  A plain clang++ builds it (no hipcc, no
// GPU, nothing preloaded).  The maps come from the public header's bfv_slot_position, the constants are derived here in
// exact integers; the expected words are tests/encode_exact.py's, compared by the test.
//   emulate_bfv_encode JOB RESULT  JOB: 64-bit words -- the number of cases, then per case W, n_power, L, K, count, off
//                                  (words by which every operand leaves 16-byte alignment), slices (the grid's y), t,
//                                  the M moduli, values[count][N], spectrum[count][N], words[count][N],
//                                  ct[2][count][L][N], pt[count][L][N]
//                                  RESULT: per case the permuted and reduced values[count][N] (encode before its
//                                  transform), the gathered spectrum[count][N] (decode after its transform),
//                                  lift_centred's out[count][M][N] and [count][L][N], multiply_plain's out
//                                  [2][count][L][N] with a shared plaintext, with one per ciphertext, and in place
//                                  one line per case, then "ALL OK" or "FAILED" (a guard band or an input was touched)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

#include "gpuntt/rns/bfv_encode.cuh"
#include "inner_product_internal.hpp"
#include "keygen_internal.hpp"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
std::barrier<>* g_block_barrier = nullptr;

namespace gpuntt
{
    namespace kern
    {
#include "kernel_extract.inc"
#include "permute_extract.inc"
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

static U64 mulmod(U64 a, U64 b, U64 m) { return U64(U128(a) * b % m); }

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

template <typename T> size_t run_case(int n, int L, int K, int count, int off, unsigned slices, U64 t, std::FILE* res)
{
    constexpr int W = 8 * sizeof(T), VW = 16 / sizeof(T);
    const int M = L + K;
    const size_t N = size_t(1) << n;
    std::vector<U64> mods(M);
    for (auto& m : mods)
        m = next();
    auto read = [&](size_t words) {
        Guarded<T> gd(words, off);
        for (size_t i = 0; i < words; i++)
            gd.data()[i] = T(next());
        return gd;
    };
    Guarded<T> values = read(size_t(count) * N), spectrum = read(size_t(count) * N), words = read(size_t(count) * N);
    Guarded<T> ct = read(size_t(2) * count * L * N), pt = read(size_t(count) * L * N);
    auto copy_of = [](Guarded<T>& gd) { return std::vector<T>(gd.data(), gd.data() + gd.words); };
    const std::vector<T> values0 = copy_of(values), spectrum0 = copy_of(spectrum), words0 = copy_of(words),
                         ct0 = copy_of(ct), pt0 = copy_of(pt);

    // the maps, from the public header (the plan keeps them 256-byte aligned: no offset here)
    Guarded<std::uint32_t> to_position(N, 0), to_slot(N, 0);
    for (std::uint32_t s = 0; s < N; s++)
    {
        const std::uint32_t p = bfv_slot_position(s, n);
        to_position.data()[s] = p, to_slot.data()[p] = s;
    }

    // the fold image of InnerProductPlan
    std::vector<T> fold(6 * size_t(M));
    auto shoup = [](U64 v, U64 m) { return T((U128(v) << W) / m); };
    for (int m = 0; m < M; m++)
    {
        const U64 q = mods[m], t1 = U64((U128(1) << W) % q), t2 = mulmod(t1, t1, q);
        fold[m] = T(q), fold[M + m] = T(t1), fold[2 * M + m] = shoup(t1, q);
        fold[3 * M + m] = T(t2), fold[4 * M + m] = shoup(t2, q), fold[5 * M + m] = shoup(1, q);
    }
    const T one_shoup_t = T((U128(1) << W) / t);

    size_t bad = 0;
    auto write = [&](Guarded<T>& gd) {
        bad += gd.touched();
        for (size_t i = 0; i < gd.words; i++)
        {
            const U64 w = gd.data()[i];
            std::fwrite(&w, sizeof(w), 1, res);
        }
    };

    // bfv_slot_permute, launched as the plan launches it: encode's direction (to_slot, reduced), decode's (to_position)
    bool pvec = false;
    for (int direction = 0; direction < 2; direction++)
    {
        Guarded<T> out(size_t(count) * N, off);
        const T* in = direction == 0 ? values.data() : spectrum.data();
        const std::uint32_t* map = direction == 0 ? to_slot.data() : to_position.data();
        pvec = host::relin_wide<T>(n, {out.data()});
        const host::RelinGrid g = host::relin_grid(n, pvec ? VW : 1, 1);
        const dim3 grid(g.tiles, std::min<unsigned>(slices, unsigned(count)));
        if (pvec)
            launch(grid, g.nt, [&] {
                kern::bfv_slot_permute<T, VW>(in, out.data(), map, count, n, direction == 0, T(t), one_shoup_t);
            });
        else
            launch(grid, g.nt, [&] {
                kern::bfv_slot_permute<T, 1>(in, out.data(), map, count, n, direction == 0, T(t), one_shoup_t);
            });
        write(out);
    }

    // lift_centred, launched as lift_centred_launch launches it: over the full base and over the q-base
    bool lvec = false;
    for (int B : {M, L})
    {
        Guarded<T> out(size_t(count) * B * N, off);
        lvec = host::relin_wide<T>(n, {words.data(), out.data()});
        const host::RelinGrid g = host::relin_grid(n, lvec ? VW : 1, U64(count));
        const T half_up = T((t + 1) >> 1);
        if (lvec)
            launch(dim3(g.blocks), g.nt, [&] {
                kern::lift_centred<T, VW>(words.data(), out.data(), fold.data(), T(t), one_shoup_t, half_up, B, M, n,
                                          g.tiles);
            });
        else
            launch(dim3(g.blocks), g.nt, [&] {
                kern::lift_centred<T, 1>(words.data(), out.data(), fold.data(), T(t), one_shoup_t, half_up, B, M, n,
                                         g.tiles);
            });
        write(out);
    }

    // multiply_plain, launched as multiply_plain_launch launches it: a shared plaintext, one per ciphertext, in place
    bool mvec = false;
    for (int form = 0; form < 3; form++)
    {
        Guarded<T> fresh(size_t(2) * count * L * N, off);
        if (form == 2)
            std::copy(ct0.begin(), ct0.end(), fresh.data());
        const T* in = form == 2 ? fresh.data() : ct.data();
        const U64 pt_stack = form == 0 ? 0 : U64(L) * N;
        mvec = host::relin_wide<T>(n, {in, pt.data(), fresh.data()});
        const host::RelinGrid g = host::relin_grid(n, mvec ? VW : 1, U64(count));
        const dim3 grid(g.blocks, L);
        if (mvec)
            launch(grid, g.nt, [&] {
                kern::multiply_plain<T, VW>(in, pt.data(), fresh.data(), fold.data(), pt_stack, count, L, M, n, g.tiles);
            });
        else
            launch(grid, g.nt, [&] {
                kern::multiply_plain<T, 1>(in, pt.data(), fresh.data(), fold.data(), pt_stack, count, L, M, n, g.tiles);
            });
        write(fresh);
    }

    bad += values.touched() + spectrum.touched() + words.touched() + ct.touched() + pt.touched() + to_position.touched() +
           to_slot.touched();
    bad += copy_of(values) != values0 || copy_of(spectrum) != spectrum0 || copy_of(words) != words0 ||
           copy_of(ct) != ct0 || copy_of(pt) != pt0;
    std::printf("W=%d n=%d L=%d K=%d count=%d off=%d slices=%u pvec=%d lvec=%d mvec=%d: %s (%zu)\n", W, n, L, K, count,
                off, slices, pvec, lvec, mvec, bad ? "GUARD TOUCHED" : "ok", bad);
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
        const int W = int(next()), n = int(next()), L = int(next()), K = int(next()), count = int(next()),
                  off = int(next());
        const unsigned slices = unsigned(next());
        const U64 t = next();
        bad += W == 64 ? run_case<Data64>(n, L, K, count, off, slices, t, res)
                       : run_case<Data32>(n, L, K, count, off, slices, t, res);
    }
    std::fclose(res);
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
