// emulate_keygen.cpp -- lift_small and keygen_combine on the CPU: the kernels' own text (the kern namespace of
// csrc/keygen.hip, cut out by tests/keygen_utils.py into kernel_extract.inc, over the accumulator and the fold of
// csrc/inner_product_internal.hpp) compiled for the host against host_shim/hip/hip_runtime.h -- one std::thread per lane
// -- under AddressSanitizer and UBSan.  It checks the index arithmetic, the bounds of every access (every buffer lies
// between guard bands), both loaders, the argument table of key pointers, the scalar branch on the digit and the signed
// lift at its extremes; it says nothing about waves or time.  A plain clang++ builds it (no hipcc, no GPU, nothing
// preloaded).  The constants are derived here, in exact integers, not by the library; the expected words are
// tests/keygen_exact.py's, compared by the test.
//   emulate_keygen JOB RESULT  JOB: 64-bit words -- the number of cases, then per case W, n_power, L, K, alpha, keys, off
//                              (words by which every operand leaves 16-byte alignment), the M moduli,
//                              errors[keys][D][N] (sign-extended), e[keys][D][M][N], s[M][N], s_from[keys][M][N],
//                              a[keys][D][M][N], ee[keys][L][N], ea[keys][L][N], msg[keys][L][N]
//                              RESULT: per case lift_small's out[keys * D][M][N] and [keys * D][L][N], keygen_combine's
//                              key0[keys][D][M][N], the ciphertexts' c0[keys][L][N] with the message and without
//                              one line per case, then "ALL OK" or "FAILED" (a guard band or an `a` plane was touched)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

#include "inner_product_internal.hpp"
#include "keygen_internal.hpp"

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

template <typename T> size_t run_case(int n, int L, int K, int alpha, int keys, int off, std::FILE* res)
{
    constexpr int W = 8 * sizeof(T), VW = 16 / sizeof(T);
    const int M = L + K, D = (L + alpha - 1) / alpha;
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
    Guarded<std::int32_t> errors(size_t(keys) * D * N, off);
    for (size_t i = 0; i < errors.words; i++)
        errors.data()[i] = std::int32_t(std::int64_t(next()));
    Guarded<T> e = read(size_t(keys) * D * M * N), s = read(size_t(M) * N), s_from = read(size_t(keys) * M * N);
    std::vector<std::unique_ptr<Guarded<T>>> key;
    std::vector<T> a_words(size_t(keys) * D * M * N);
    for (auto& w : a_words)
        w = T(next());
    for (int g = 0; g < keys; g++)
    {
        key.emplace_back(new Guarded<T>(size_t(D) * 2 * M * N, off));
        for (int d = 0; d < D; d++)
            for (size_t i = 0; i < size_t(M) * N; i++)
                key[g]->data()[(size_t(d) * 2 + 1) * M * N + i] = a_words[(size_t(g) * D + d) * M * N + i];
    }
    Guarded<T> ee = read(size_t(keys) * L * N), ea = read(size_t(keys) * L * N), msg = read(size_t(keys) * L * N);

    // the fold image of InnerProductPlan and P mod q_m
    std::vector<T> fold(6 * size_t(M));
    auto shoup = [](U64 v, U64 m) { return T((U128(v) << W) / m); };
    for (int m = 0; m < M; m++)
    {
        const U64 q = mods[m], t1 = U64((U128(1) << W) % q), t2 = mulmod(t1, t1, q);
        fold[m] = T(q), fold[M + m] = T(t1), fold[2 * M + m] = shoup(t1, q);
        fold[3 * M + m] = T(t2), fold[4 * M + m] = shoup(t2, q), fold[5 * M + m] = shoup(1, q);
    }

    size_t bad = 0;
    auto write = [&](Guarded<T>& gd) {
        bad += gd.touched();
        for (size_t i = 0; i < gd.words; i++)
        {
            const U64 w = gd.data()[i];
            std::fwrite(&w, sizeof(w), 1, res);
        }
    };

    // lift_small, launched as keygen_lift_launch launches it: over the full base and over the q-base
    bool lvec = false;
    for (int B : {M, L})
    {
        Guarded<T> out(size_t(keys) * D * B * N, off);
        lvec = host::relin_wide<T>(n, {errors.data(), out.data()});
        const host::RelinGrid g = host::relin_grid(n, lvec ? VW : 1, U64(keys) * D);
        if (lvec)
            launch(dim3(g.blocks), g.nt,
                   [&] { kern::lift_small<T, VW>(errors.data(), out.data(), fold.data(), B, M, n, g.tiles); });
        else
            launch(dim3(g.blocks), g.nt,
                   [&] { kern::lift_small<T, 1>(errors.data(), out.data(), fold.data(), B, M, n, g.tiles); });
        write(out);
    }

    // keygen_combine for keys, launched as keygen_combine_launch launches it
    bool cvec;
    {
        kern::KeygenArgs<T> args{};
        uintptr_t bits = reinterpret_cast<uintptr_t>(e.data()) | reinterpret_cast<uintptr_t>(s.data()) |
                         reinterpret_cast<uintptr_t>(s_from.data());
        for (int g = 0; g < keys; g++)
            args.group[g] = key[g]->data(), bits |= reinterpret_cast<uintptr_t>(args.group[g]);
        for (int m = 0; m < L; m++)
        {
            U64 pq = 1 % mods[m];
            for (int k = L; k < M; k++)
                pq = mulmod(pq, mods[k] % mods[m], mods[m]);
            args.mult[m] = T(pq);
        }
        const kern::KeygenShape shape{2 * M * N, M * N, M * N, 0, D, M, L, alpha > L ? L : alpha};
        cvec = host::relin_wide_bits<T>(n, bits);
        const host::RelinGrid g = host::relin_grid(n, cvec ? VW : 1, U64(keys) * D);
        const dim3 grid(g.blocks, M);
        if (cvec)
            launch(grid, g.nt, [&] {
                kern::keygen_combine<T, VW>(e.data(), s.data(), s_from.data(), args, shape, fold.data(), M, n, g.tiles);
            });
        else
            launch(grid, g.nt, [&] {
                kern::keygen_combine<T, 1>(e.data(), s.data(), s_from.data(), args, shape, fold.data(), M, n, g.tiles);
            });
        for (int g2 = 0; g2 < keys; g2++)
        {
            bad += key[g2]->touched();
            for (int d = 0; d < D; d++)
                for (size_t i = 0; i < size_t(M) * N; i++)
                {
                    const U64 w = key[g2]->data()[size_t(d) * 2 * M * N + i];
                    std::fwrite(&w, sizeof(w), 1, res);
                    // the `a` plane is as it was
                    bad += key[g2]->data()[(size_t(d) * 2 + 1) * M * N + i] != a_words[(size_t(g2) * D + d) * M * N + i];
                }
        }
    }

    // keygen_combine for ciphertexts: one group, a row per ciphertext, the q-base, with and without a message
    for (const T* message : {static_cast<const T*>(msg.data()), static_cast<const T*>(nullptr)})
    {
        const int count = keys;
        Guarded<T> out(size_t(2) * count * L * N, off);
        std::copy(ea.data(), ea.data() + ea.words, out.data() + size_t(count) * L * N);
        kern::KeygenArgs<T> args{};
        args.group[0] = out.data();
        for (int m = 0; m < L; m++)
            args.mult[m] = T(1);
        const kern::KeygenShape shape{L * N, size_t(count) * L * N, 0, L * N, count, L, L, 0};
        const bool vec = host::relin_wide<T>(n, {ee.data(), s.data(), message, out.data()});
        const host::RelinGrid g = host::relin_grid(n, vec ? VW : 1, U64(count));
        const dim3 grid(g.blocks, L);
        if (vec)
            launch(grid, g.nt, [&] {
                kern::keygen_combine<T, VW>(ee.data(), s.data(), message, args, shape, fold.data(), M, n, g.tiles);
            });
        else
            launch(grid, g.nt, [&] {
                kern::keygen_combine<T, 1>(ee.data(), s.data(), message, args, shape, fold.data(), M, n, g.tiles);
            });
        bad += out.touched();
        for (size_t i = 0; i < size_t(count) * L * N; i++)
        {
            const U64 w = out.data()[i];
            std::fwrite(&w, sizeof(w), 1, res);
            bad += out.data()[size_t(count) * L * N + i] != ea.data()[i];
        }
    }
    bad += errors.touched() + e.touched() + s.touched() + s_from.touched() + ee.touched() + ea.touched() + msg.touched();
    std::printf("W=%d n=%d L=%d K=%d alpha=%d keys=%d off=%d lvec=%d vec=%d: %s (%zu)\n", W, n, L, K, alpha, keys, off,
                lvec, cvec, bad ? "GUARD TOUCHED" : "ok", bad);
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
        const int W = int(next()), n = int(next()), L = int(next()), K = int(next()), alpha = int(next()),
                  keys = int(next()), off = int(next());
        bad += W == 64 ? run_case<Data64>(n, L, K, alpha, keys, off, res)
                       : run_case<Data32>(n, L, K, alpha, keys, off, res);
    }
    std::fclose(res);
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
