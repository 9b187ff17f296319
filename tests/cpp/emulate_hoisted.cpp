// emulate_hoisted.cpp -- inner_product_galois and inner_product_galois_sum on the CPU: the kernels' own text (the kern
// namespace of csrc/hoisted_rotation.hip, cut out by tests/hoisted_emulator.py into kernel_extract.inc) compiled for the
// host against host_shim/hip/hip_runtime.h -- one std::thread per lane, a std::barrier for __syncthreads -- under
// AddressSanitizer and UBSan, and compared word for word with the definitions in exact integers.  It checks the index
// arithmetic, the bounds of every access, both loaders, the arithmetic at the edges of the word and the barriers'
// placement as far as a thread schedule shows it; it says nothing about waves, LDS banks or time.  A plain clang++ builds
// it (no hipcc, no GPU, nothing preloaded).
//   emulate_hoisted [rotation | sum]     one line per case, then "ALL OK" or "FAILED"; both kernels without an argument
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <type_traits>
#include <vector>

#include "hoisted_rotation_internal.hpp"
#include "inner_product_internal.hpp"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
std::barrier<>* g_block_barrier = nullptr;

namespace gpuntt
{
    namespace kern
    {
        __attribute__((aligned(16))) unsigned char hoist_smem[65536];
#include "kernel_extract.inc"
    } // namespace kern
} // namespace gpuntt

using namespace gpuntt;
using U128 = unsigned __int128;

// kernel(): one lane's call, with the launch's arguments bound
template <typename Kernel> void launch(dim3 grid, unsigned nt, Kernel kernel)
{
    for (unsigned by = 0; by < grid.y; by++)
        for (unsigned bx = 0; bx < grid.x; bx++)
        {
            std::barrier<> bar(nt);
            g_block_barrier = &bar;
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

// the shape of one case.  top: the moduli lie below 2^(W-2), within an eighth of it -- all the kernels' bounds rest on is
// 3 q < 2^W -- otherwise below 2^(W-3), where no intermediate reaches 2^(W-1); ones: every word of a, c0, the keys and the
// weights is 2^W - 1, the largest sum the three-word accumulators can be given; off: every operand starts `off` words
// behind a 16-byte boundary
struct Shape
{
    int n, logc, D, L, K, count, G;
    bool with_c0, neg;
    int off;
    bool top = false, ones = false;
};

// what both kernels are given: moduli, the constants image, operands, the kernel arguments, guarded accumulators
template <typename T> struct Fixture
{
    static constexpr int W = 8 * sizeof(T);
    const Shape s;
    const int M, KM;
    const size_t N;
    std::mt19937_64 rng;
    std::vector<T> q, consts, a, c0, pq, acc;
    std::vector<std::vector<T>> keys;
    kern::HoistArgs<T> ha{};
    size_t acc_words = 0;

    std::vector<T> words(size_t w)
    {
        std::vector<T> v(w + s.off + 4);
        for (auto& x : v)
            x = static_cast<T>(rng());
        for (size_t i = 0; i < v.size(); i += 97)
            v[i] = (i % 2) ? T(~T(0)) : T(0);
        if (s.ones)
            for (auto& x : v)
                x = T(~T(0));
        return v;
    }

    explicit Fixture(const Shape& shape)
        : s(shape), M(s.L + s.K), KM(M + 1), N(size_t(1) << s.n),
          rng(s.n * 1000 + s.logc * 100 + s.D * 10 + s.G + s.off), q(M), consts(6 * M), pq(s.L)
    {
        for (int m = 0; m < M; m++)
        {
            // odd (not prime, not needed).  top: modulus 0 within 2000 of 2^(W-2), the others spread over the eighth below
            // it: right under a power of two 2^W mod q and 2^2W mod q are tiny, two of the fold's three terms carry all the
            // weight and the fold sum never passes 2 q -- only a modulus further down drives it into [2^(W-1), 3 q)
            const T away = s.top && m > 0 ? static_cast<T>(rng() % (T(1) << (W - 6))) : static_cast<T>(rng() % 1000);
            q[m] = static_cast<T>((T(1) << (s.top ? W - 2 : W - 3)) - 1 - 2 * away) | 1;
        }
        for (int m = 0; m < M; m++)
        {
            const U128 t1 = (U128(1) << W) % q[m], t2 = t1 * t1 % q[m];
            consts[m] = q[m], consts[M + m] = T(t1), consts[2 * M + m] = T((t1 << W) / q[m]);
            consts[3 * M + m] = T(t2), consts[4 * M + m] = T((t2 << W) / q[m]), consts[5 * M + m] = T((U128(1) << W) / q[m]);
        }
        // buffers 16-byte aligned by construction of std::vector<T> (operator new: 16), then shifted by `off` words
        a = words(size_t(s.D) * s.count * M * N), c0 = words(size_t(s.count) * s.L * N);
        ha.count = s.G;
        const std::uint32_t mask = s.neg ? (2u << s.n) - 1u : (1u << s.n) - 1u;
        for (int g = 0; g < s.G; g++)
        {
            keys.push_back(words(size_t(s.D) * 2 * KM * N));
            ha.key[g] = keys.back().data() + s.off;
            const std::uint32_t k = (static_cast<std::uint32_t>(rng()) | 1u) & mask;
            ha.elt[g] = g == 1 ? 1u : k, ha.inv[g] = galois_inverse(ha.elt[g]) & mask;
        }
        for (int m = 0; m < M; m++)
            ha.limb[m] = static_cast<unsigned char>(m < s.L ? m : m + 1); // the key has one limb more: skip limb L
        for (int m = 0; m < s.L; m++)
        {
            pq[m] = static_cast<T>(rng() % q[m]);
            ha.p_mod_q[m] = pq[m], ha.p_mod_q_shoup[m] = T((U128(pq[m]) << W) / q[m]);
        }
    }

    const T* pa() const { return a.data() + s.off; }
    const T* pc0() const { return s.with_c0 ? c0.data() + s.off : nullptr; }
    // the launchers' decision (hoist_dispatch)
    bool wide() const
    {
        return ((sizeof(T) << s.logc) % 16 == 0) &&
               ((reinterpret_cast<uintptr_t>(pa()) | reinterpret_cast<uintptr_t>(pc0())) & 15u) == 0;
    }
    // `groups` accumulators T[2][count][M][N] between two guard bands of 32 words
    T* out(int groups)
    {
        acc_words = size_t(groups) * 2 * s.count * M * N;
        acc.assign(acc_words + 64, T(0x5A));
        return acc.data() + 32;
    }
    size_t guards_touched() const
    {
        size_t bad = 0;
        for (int i = 0; i < 32; i++)
            bad += acc[i] != T(0x5A) || acc[32 + acc_words + i] != T(0x5A);
        return bad;
    }
    // one lane per slot, between a wave and the 256 lanes of a workgroup (hoist_dispatch)
    void run(bool vec, const auto& kernel_vec, const auto& kernel_plain) const
    {
        unsigned nt = 64;
        while (nt < 256u && nt < (1u << s.logc))
            nt *= 2;
        const dim3 grid(static_cast<unsigned>(s.count << (s.n - s.logc)), static_cast<unsigned>(M));
        if (vec)
            launch(grid, nt, kernel_vec);
        else
            launch(grid, nt, kernel_plain);
    }
    // u_g[c][r][m][j], the definition
    U128 term(int g, int c, int r, int m, size_t j) const
    {
        const size_t src = galois_ntt_source(static_cast<std::uint32_t>(j), ha.elt[g], s.n, s.neg);
        U128 u = 0;
        for (int d = 0; d < s.D; d++)
        {
            const U128 x = pa()[((size_t(d) * s.count + r) * M + m) * N + src] % q[m];
            const U128 k = ha.key[g][((size_t(d) * 2 + c) * KM + ha.limb[m]) * N + j] % q[m];
            u = (u + x * k) % q[m];
        }
        if (c == 0 && m < s.L && s.with_c0)
            u = (u + U128(pq[m]) * (pc0()[(size_t(r) * s.L + m) * N + src] % q[m])) % q[m];
        return u;
    }
    int report(const char* kernel, int nullw, size_t bad) const
    {
        std::printf("%s W=%d n=%d logc=%d D=%d L=%d K=%d count=%d G=%d c0=%d neg=%d off=%d nullw=%d top=%d ones=%d vec=%d: "
                    "%s (%zu)\n",
                    kernel, W, s.n, s.logc, s.D, s.L, s.K, s.count, s.G, s.with_c0, s.neg, s.off, nullw, s.top, s.ones,
                    wide(), bad ? "WRONG" : "ok", bad);
        return bad != 0;
    }
};

// inner_product_galois: acc[g][c][r][m][j] = u_g[c][r][m][j]
template <typename T> int rotation(const Shape& s)
{
    Fixture<T> f(s);
    T* acc = f.out(s.G);
    auto call = [&](auto vec) {
        return [&, vec] {
            kern::inner_product_galois<T, decltype(vec)::value>(f.pa(), f.pc0(), acc, f.consts.data(), f.ha, s.D, s.count, s.L,
                                                                f.M, f.KM, s.n, s.logc, s.neg);
        };
    };
    f.run(f.wide(), call(std::true_type{}), call(std::false_type{}));
    size_t bad = f.guards_touched();
    for (int g = 0; g < s.G; g++)
        for (int c = 0; c < 2; c++)
            for (int r = 0; r < s.count; r++)
                for (int m = 0; m < f.M; m++)
                    for (size_t j = 0; j < f.N; j++)
                        bad += acc[(((size_t(g) * 2 + c) * s.count + r) * f.M + m) * f.N + j] != T(f.term(g, c, r, m, j));
    return f.report("rotation", -1, bad);
}

// inner_product_galois_sum: acc[c][r][m][j] = ( sum_g w_g[m][j] * u_g[c][r][m][j] ) mod q_m; the weight of element g is
// null (1) when nullw < 0 or g % 3 == nullw
template <typename T> int sum(const Shape& s, int nullw)
{
    Fixture<T> f(s);
    std::vector<std::vector<T>> ws;
    kern::HoistSumArgs<T> ha{};
    ha.h = f.ha;
    for (int g = 0; g < s.G; g++)
    {
        ws.push_back(f.words(size_t(f.M) * f.N));
        ha.weight[g] = (nullw < 0 || g % 3 == nullw) ? nullptr : ws.back().data() + s.off;
    }
    T* acc = f.out(1);
    auto call = [&](auto vec) {
        return [&, vec] {
            kern::inner_product_galois_sum<T, decltype(vec)::value>(f.pa(), f.pc0(), acc, f.consts.data(), ha, s.D, s.count,
                                                                    s.L, f.M, f.KM, s.n, s.logc, s.neg);
        };
    };
    f.run(f.wide(), call(std::true_type{}), call(std::false_type{}));
    size_t bad = f.guards_touched();
    for (int c = 0; c < 2; c++)
        for (int r = 0; r < s.count; r++)
            for (int m = 0; m < f.M; m++)
                for (size_t j = 0; j < f.N; j++)
                {
                    U128 t = 0;
                    for (int g = 0; g < s.G; g++)
                    {
                        const U128 w = ha.weight[g] ? ha.weight[g][size_t(m) * f.N + j] % f.q[m] : 1;
                        t = (t + w * f.term(g, c, r, m, j)) % f.q[m];
                    }
                    bad += acc[((size_t(c) * s.count + r) * f.M + m) * f.N + j] != T(t);
                }
    return f.report("sum", nullw, bad);
}

template <typename T> int all_rotation()
{
    int bad = 0;
    for (const bool top : {false, true})
    {
        bad += rotation<T>({1, 1, 2, 2, 1, 2, 3, true, true, 0, top});
        bad += rotation<T>({2, 2, 2, 2, 1, 1, 1, false, true, 0, top});
        bad += rotation<T>({5, 5, 3, 3, 2, 2, 5, true, true, 0, top});
        bad += rotation<T>({6, 6, 2, 3, 2, 1, 4, true, false, 0, top});
        bad += rotation<T>({7, 6, 2, 3, 2, 3, 5, true, true, 0, top});
        bad += rotation<T>({7, 6, 2, 3, 2, 2, 5, false, true, 1, top});
        bad += rotation<T>({9, 7, 3, 2, 1, 1, 3, true, false, 1, top});
        bad += rotation<T>({9, 9, 2, 2, 1, 2, 3, true, true, 0, top}); // 512 slots on 256 lanes: two slots per lane
        // the largest sums: every operand word 2^W - 1, 64 elements and 64 digits
        bad += rotation<T>({6, 6, 2, 3, 2, 1, 64, true, true, 0, top, true});
        bad += rotation<T>({6, 6, 64, 1, 1, 1, 2, true, true, 0, top, true});
    }
    return bad;
}

template <typename T> int all_sum()
{
    int bad = 0;
    bad += sum<T>({1, 1, 2, 2, 1, 2, 3, true, true, 0}, 0);
    bad += sum<T>({2, 2, 2, 2, 1, 1, 1, false, true, 0}, -1);
    bad += sum<T>({5, 5, 3, 3, 2, 2, 5, true, true, 0}, 1);
    bad += sum<T>({6, 6, 2, 3, 2, 1, 4, true, false, 0}, 2);
    bad += sum<T>({7, 6, 2, 3, 2, 3, 5, true, true, 0}, 0);
    bad += sum<T>({7, 6, 2, 3, 2, 2, 5, false, true, 1}, 1);
    bad += sum<T>({9, 6, 3, 2, 1, 1, 3, true, true, 0}, 2);
    bad += sum<T>({9, 7, 3, 2, 1, 1, 3, true, false, 1}, 0);
    bad += sum<T>({9, 8, 2, 2, 1, 2, 6, true, true, 0}, 1);
    bad += sum<T>({5, 5, 1, 1, 1, 1, 64, true, true, 0}, 0);
    // moduli in the eighth below 2^(W-2); a dozen weighted elements, so that the carry word of the across-g
    // accumulator is not 0 and all three terms of the last fold count
    bad += sum<T>({5, 5, 3, 3, 2, 2, 12, true, true, 0, true}, 3);
    bad += sum<T>({7, 6, 2, 3, 2, 2, 9, false, true, 1, true}, 1);
    bad += sum<T>({9, 7, 3, 2, 1, 1, 3, true, false, 0, true}, -1);
    // the largest sums: every operand word 2^W - 1, 64 elements and 64 digits, at both widths of the moduli
    for (const bool top : {false, true})
    {
        bad += sum<T>({6, 6, 2, 3, 2, 1, 64, true, true, 0, top, true}, 3); // nullw = 3: no null weight
        bad += sum<T>({6, 6, 64, 1, 1, 1, 2, true, true, 0, top, true}, 3);
    }
    return bad;
}

int main(int argc, char** argv)
{
    const bool rot = argc < 2 || std::strcmp(argv[1], "rotation") == 0, sm = argc < 2 || std::strcmp(argv[1], "sum") == 0;
    if (!rot && !sm)
    {
        std::printf("usage: emulate_hoisted [rotation | sum]\n");
        return 2;
    }
    int bad = 0;
    if (rot)
        bad += all_rotation<Data64>() + all_rotation<Data32>();
    if (sm)
        bad += all_sum<Data64>() + all_sum<Data32>();
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
