// emulate_bsgs.cpp -- the three kernels of KeySwitchPlan::linear_transform_bsgs on the CPU: bsgs_scale_input,
// bsgs_weighted_sum and inner_product_galois_giant, the kernels' own text (the kern namespace of
// csrc/hoisted_rotation.hip, cut out by tests/bsgs_emulator.py into kernel_extract.inc) compiled for the host against
// host_shim/hip/hip_runtime.h -- one std::thread per lane, a std::barrier for __syncthreads -- under AddressSanitizer and
// UBSan, and compared word for word with their definitions in exact integers.  It checks the index arithmetic, the
// bounds of every access, both loaders and both group widths, the arithmetic at the edges of the word and the barriers'
// placement as far as a thread schedule shows it; it says nothing about waves, LDS banks or time.  A plain clang++
// builds it (no hipcc, no GPU, nothing preloaded).
//   emulate_bsgs [scale | sum | giant]     one line per case, then "ALL OK" or "FAILED"; all three without an argument
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
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

// the moduli (odd, not prime: not needed) with the constants image of InnerProductPlan, and the word makers.  top: the
// moduli lie in the eighth below 2^(W-2) -- all the kernels' bounds rest on is 3 q < 2^W -- otherwise below 2^(W-3);
// ones: every operand word is 2^W - 1, the largest sum the three-word accumulators can be given
template <typename T> struct Base
{
    static constexpr int W = 8 * sizeof(T);
    const int M;
    const bool ones;
    std::mt19937_64 rng;
    std::vector<T> q, consts;
    Base(int M_, bool top, bool ones_, unsigned seed) : M(M_), ones(ones_), rng(seed), q(M_), consts(6 * M_)
    {
        for (int m = 0; m < M; m++)
        {
            const T away = top && m > 0 ? static_cast<T>(rng() % (T(1) << (W - 6))) : static_cast<T>(rng() % 1000);
            q[m] = static_cast<T>((T(1) << (top ? W - 2 : W - 3)) - 1 - 2 * away) | 1;
            const U128 t1 = (U128(1) << W) % q[m], t2 = t1 * t1 % q[m];
            consts[m] = q[m], consts[M + m] = T(t1), consts[2 * M + m] = T((t1 << W) / q[m]);
            consts[3 * M + m] = T(t2), consts[4 * M + m] = T((t2 << W) / q[m]), consts[5 * M + m] = T((U128(1) << W) / q[m]);
        }
    }
    // w words behind `off` words of slack (std::vector<T>: 16-byte aligned by operator new) plus 4 more
    std::vector<T> words(size_t w, int off = 0)
    {
        std::vector<T> v(w + off + 4);
        for (auto& x : v)
            x = static_cast<T>(rng());
        for (size_t i = 0; i < v.size(); i += 97)
            v[i] = (i % 2) ? T(~T(0)) : T(0);
        if (ones)
            for (auto& x : v)
                x = T(~T(0));
        return v;
    }
};

// `words` output words between two guard bands of 32
template <typename T> struct Guarded
{
    std::vector<T> buf;
    size_t words;
    explicit Guarded(size_t w) : buf(w + 64, T(0x5A)), words(w) {}
    T* data() { return buf.data() + 32; }
    size_t touched() const
    {
        size_t bad = 0;
        for (int i = 0; i < 32; i++)
            bad += buf[i] != T(0x5A) || buf[32 + words + i] != T(0x5A);
        return bad;
    }
};

// bsgs_scale_input: u[b][c][r][m][j] = [m < L] pq_m * (c_c[r][m][j] mod q_m) mod q_m for first <= b < n1, c_0 = 0 if null
template <typename T> int scale(int n, int L, int K, int count, int first, int n1, bool with_c0, int off)
{
    constexpr int W = 8 * sizeof(T);
    const int M = L + K;
    const size_t N = size_t(1) << n;
    Base<T> f(M, true, false, n * 100 + L * 10 + count + off);
    std::vector<T> c0 = f.words(count * L * N, off), c1 = f.words(count * L * N, off);
    kern::HoistArgs<T> ha{};
    for (int m = 0; m < L; m++)
    {
        ha.p_mod_q[m] = static_cast<T>(f.rng() % f.q[m]);
        ha.p_mod_q_shoup[m] = T((U128(ha.p_mod_q[m]) << W) / f.q[m]);
    }
    const size_t S = size_t(count) * M * N;
    Guarded<T> u(size_t(n1) * 2 * S);
    for (size_t i = 0; i < u.words; i++)
        u.data()[i] = T(0x77); // what the steps with a key would have written: must survive below `first`
    const T* p0 = with_c0 ? c0.data() + off : nullptr;
    const T* p1 = c1.data() + off;
    const unsigned nt = 256;
    const dim3 grid(static_cast<unsigned>((N + nt - 1) / nt) * 2 * count, M);
    launch(grid, nt, [&] {
        kern::bsgs_scale_input<T>(p0, p1, u.data(), f.consts.data(), ha, first, n1, count, L, M, n);
    });
    size_t bad = u.touched();
    for (int b = 0; b < n1; b++)
        for (int c = 0; c < 2; c++)
            for (int r = 0; r < count; r++)
                for (int m = 0; m < M; m++)
                    for (size_t j = 0; j < N; j++)
                    {
                        const T* src = c == 0 ? p0 : p1;
                        U128 want = 0x77;
                        if (b >= first)
                            want = (m < L && src) ? U128(ha.p_mod_q[m]) * (src[(size_t(r) * L + m) * N + j] % f.q[m]) % f.q[m]
                                                  : 0;
                        bad += u.data()[(((size_t(b) * 2 + c) * count + r) * M + m) * N + j] != T(want);
                    }
    std::printf("scale W=%d n=%d L=%d K=%d count=%d first=%d n1=%d c0=%d off=%d: %s (%zu)\n", W, n, L, K, count, first, n1,
                with_c0, off, bad ? "WRONG" : "ok", bad);
    return bad != 0;
}

// the launcher's rule (host::bsgs_sum_shape), restated
static void sum_shape(size_t word_bytes, int n1, int n, bool aligned, int& V, unsigned& nt)
{
    const unsigned long long N = 1ull << n;
    V = static_cast<int>(16 / word_bytes);
    if (!aligned || N % V != 0 || size_t(n1) * 64 * 16 > 32768)
        V = 1;
    nt = 256;
    while (nt > 64 && (size_t(n1) * nt * V * word_bytes > 32768 || (unsigned long long) (nt / 2) * V >= N))
        nt /= 2;
}

// bsgs_weighted_sum: v[c][g][r][m][j] = (sum_{b: present} w_{g,b}[m][j] * u[b][c][r][m][j]) mod q_m; the weight (g, b) is
// absent when absent >= 0 and (g + b) % 3 == absent
template <typename T> int sum(int n, int M, int count, int n1, int n2, int off, int absent, bool top, bool ones)
{
    constexpr int W = 8 * sizeof(T);
    const size_t N = size_t(1) << n, S = size_t(count) * M * N;
    Base<T> f(M, top, ones, n * 1000 + n1 * 10 + n2 + off);
    std::vector<T> u = f.words(size_t(n1) * 2 * S);
    std::vector<std::vector<T>> ws;
    kern::BsgsWeights<T> wa{};
    wa.n1 = n1, wa.n2 = n2;
    for (int i = 0; i < n1 * n2; i++)
    {
        ws.push_back(f.words(size_t(M) * N, off));
        wa.w[i] = (absent >= 0 && (i / n1 + i % n1) % 3 == absent) ? nullptr : ws.back().data() + off;
    }
    // u and v are 16-byte aligned as the scratch is: 32 guard words are a multiple of 16 bytes at either width
    Guarded<T> v(size_t(n2) * 2 * S);
    int V;
    unsigned nt;
    sum_shape(sizeof(T), n1, n, off == 0, V, nt);
    const unsigned long long per = (unsigned long long) nt * V;
    const dim3 grid(static_cast<unsigned>((N + per - 1) / per) * 2 * count, M);
    if (V > 1)
        launch(grid, nt, [&] {
            kern::bsgs_weighted_sum<T, 16 / sizeof(T)>(u.data(), v.data(), f.consts.data(), wa, count, M, n);
        });
    else
        launch(grid, nt, [&] { kern::bsgs_weighted_sum<T, 1>(u.data(), v.data(), f.consts.data(), wa, count, M, n); });
    size_t bad = v.touched();
    for (int c = 0; c < 2; c++)
        for (int g = 0; g < n2; g++)
            for (int r = 0; r < count; r++)
                for (int m = 0; m < M; m++)
                    for (size_t j = 0; j < N; j++)
                    {
                        U128 t = 0;
                        for (int b = 0; b < n1; b++)
                            if (wa.w[g * n1 + b])
                                t = (t + U128(wa.w[g * n1 + b][size_t(m) * N + j] % f.q[m]) *
                                             (u[(((size_t(b) * 2 + c) * count + r) * M + m) * N + j] % f.q[m])) %
                                    f.q[m];
                        bad += v.data()[(((size_t(c) * n2 + g) * count + r) * M + m) * N + j] != T(t);
                    }
    std::printf("sum W=%d n=%d M=%d count=%d n1=%d n2=%d off=%d absent=%d top=%d ones=%d V=%d nt=%u: %s (%zu)\n", W, n, M,
                count, n1, n2, off, absent, top, ones, V, nt, bad ? "WRONG" : "ok", bad);
    return bad != 0;
}

// inner_product_galois_giant: acc[c][r][m][j] = (sum_{g < n2k} (sum_d a[d][g count + r][m][pi_g(j)] key_g[d][c][limb(m)][j]
// + [c = 0] v[0][g][r][m][pi_g(j)]) + sum_{n2k <= g < n2} v[c][g][r][m][j]) mod q_m
template <typename T> int giant(int n, int logc, int D, int M, int count, int n2, int n2k, bool neg, bool top, bool ones)
{
    constexpr int W = 8 * sizeof(T);
    const int KM = M + 1;
    const size_t N = size_t(1) << n, S = size_t(count) * M * N;
    Base<T> f(M, top, ones, n * 1000 + logc * 100 + D * 10 + n2);
    std::vector<T> a = f.words(size_t(D) * n2k * S), v = f.words(size_t(2) * n2 * S);
    std::vector<std::vector<T>> keys;
    kern::HoistArgs<T> ha{};
    ha.count = n2k;
    const std::uint32_t mask = neg ? (2u << n) - 1u : (1u << n) - 1u;
    for (int g = 0; g < n2k; g++)
    {
        keys.push_back(f.words(size_t(D) * 2 * KM * N, 1));
        ha.key[g] = keys.back().data() + 1; // the keys may lie anywhere: read one word at a time
        const std::uint32_t k = (static_cast<std::uint32_t>(f.rng()) | 1u) & mask;
        ha.elt[g] = g == 1 ? 1u : k, ha.inv[g] = galois_inverse(ha.elt[g]) & mask;
    }
    for (int m = 0; m < M; m++)
        ha.limb[m] = static_cast<unsigned char>(m < 2 ? m : m + 1); // the key has one limb more: skip limb 2
    Guarded<T> acc(2 * S);
    unsigned nt = 64;
    while (nt < 256u && nt < (1u << logc))
        nt *= 2;
    const dim3 grid(static_cast<unsigned>(count << (n - logc)), static_cast<unsigned>(M));
    const bool vec = (sizeof(T) << logc) % 16 == 0;
    if (vec)
        launch(grid, nt, [&] {
            kern::inner_product_galois_giant<T, true>(a.data(), v.data(), acc.data(), f.consts.data(), ha, n2, D, count, M,
                                                      KM, n, logc, neg);
        });
    else
        launch(grid, nt, [&] {
            kern::inner_product_galois_giant<T, false>(a.data(), v.data(), acc.data(), f.consts.data(), ha, n2, D, count, M,
                                                       KM, n, logc, neg);
        });
    size_t bad = acc.touched();
    for (int c = 0; c < 2; c++)
        for (int r = 0; r < count; r++)
            for (int m = 0; m < M; m++)
                for (size_t j = 0; j < N; j++)
                {
                    const U128 q = f.q[m];
                    U128 t = 0;
                    for (int g = 0; g < n2; g++)
                    {
                        if (g >= n2k)
                        {
                            t = (t + v[(((size_t(c) * n2 + g) * count + r) * M + m) * N + j] % q) % q;
                            continue;
                        }
                        const size_t src = galois_ntt_source(static_cast<std::uint32_t>(j), ha.elt[g], n, neg);
                        for (int d = 0; d < D; d++)
                        {
                            const U128 x = a[((size_t(d) * n2k * count + size_t(g) * count + r) * M + m) * N + src] % q;
                            const U128 k = ha.key[g][((size_t(d) * 2 + c) * KM + ha.limb[m]) * N + j] % q;
                            t = (t + x * k) % q;
                        }
                        if (c == 0)
                            t = (t + v[((size_t(g) * count + r) * M + m) * N + src] % q) % q;
                    }
                    bad += acc.data()[((size_t(c) * count + r) * M + m) * N + j] != T(t);
                }
    std::printf("giant W=%d n=%d logc=%d D=%d M=%d count=%d n2=%d n2k=%d neg=%d top=%d ones=%d vec=%d: %s (%zu)\n", W, n,
                logc, D, M, count, n2, n2k, neg, top, ones, vec, bad ? "WRONG" : "ok", bad);
    return bad != 0;
}

template <typename T> int all_scale()
{
    int bad = 0;
    bad += scale<T>(1, 2, 1, 2, 0, 1, true, 0);
    bad += scale<T>(5, 3, 2, 3, 2, 4, true, 1);
    bad += scale<T>(9, 2, 1, 1, 1, 2, false, 0); // 512 slots: two tiles
    bad += scale<T>(8, 1, 1, 2, 3, 4, true, 1);
    return bad;
}

template <typename T> int all_sum()
{
    int bad = 0;
    for (const bool top : {false, true})
    {
        bad += sum<T>(1, 3, 2, 3, 2, 0, 0, top, false); // a ring of 2 slots
        bad += sum<T>(2, 3, 1, 1, 1, 0, -1, top, false);
        bad += sum<T>(5, 4, 3, 3, 2, 0, 1, top, false);
        bad += sum<T>(6, 3, 1, 4, 1, 1, 2, top, false); // the weights one word off: one word per lane
        bad += sum<T>(7, 3, 2, 1, 3, 0, -1, top, false);
        bad += sum<T>(9, 2, 1, 5, 3, 0, 0, top, false); // 512 slots
        bad += sum<T>(9, 2, 1, 3, 2, 1, 1, top, false); // 512 slots, one word per lane: two tiles
        // n1 * n2 = 256 and the largest sums: every word 2^W - 1, 64 terms per output
        bad += sum<T>(5, 2, 1, 16, 16, 0, -1, top, true);
        bad += sum<T>(5, 2, 1, 64, 4, 0, -1, top, true);
        bad += sum<T>(5, 2, 1, 4, 64, 0, 2, top, false);
        bad += sum<T>(7, 2, 1, 32, 2, 0, 0, top, false); // the group width at its LDS limit
    }
    return bad;
}

template <typename T> int all_giant()
{
    int bad = 0;
    for (const bool top : {false, true})
    {
        bad += giant<T>(1, 1, 2, 3, 2, 3, 2, true, top, false);
        bad += giant<T>(2, 2, 2, 3, 1, 1, 1, true, top, false);
        bad += giant<T>(5, 5, 3, 5, 2, 3, 2, true, top, false);
        bad += giant<T>(6, 6, 2, 4, 1, 2, 2, false, top, false);
        bad += giant<T>(7, 6, 2, 4, 3, 3, 2, true, top, false);
        bad += giant<T>(7, 6, 2, 3, 2, 3, 0, true, top, false); // no giant step has a key: the plain sum
        bad += giant<T>(9, 6, 3, 3, 1, 2, 1, true, top, false);
        bad += giant<T>(9, 7, 3, 3, 1, 3, 3, false, top, false);
        bad += giant<T>(9, 8, 2, 3, 2, 4, 3, true, top, false);
        // the largest sums: every word 2^W - 1, 64 giant steps and 64 digits
        bad += giant<T>(6, 6, 2, 3, 1, 64, 64, true, top, true);
        bad += giant<T>(6, 6, 2, 3, 1, 64, 32, true, top, true);
        bad += giant<T>(6, 6, 64, 2, 1, 2, 2, true, top, true);
    }
    return bad;
}

int main(int argc, char** argv)
{
    const bool sc = argc < 2 || std::strcmp(argv[1], "scale") == 0, sm = argc < 2 || std::strcmp(argv[1], "sum") == 0;
    const bool gi = argc < 2 || std::strcmp(argv[1], "giant") == 0;
    if (!sc && !sm && !gi)
    {
        std::printf("usage: emulate_bsgs [scale | sum | giant]\n");
        return 2;
    }
    int bad = 0;
    if (sc)
        bad += all_scale<Data64>() + all_scale<Data32>();
    if (sm)
        bad += all_sum<Data64>() + all_sum<Data32>();
    if (gi)
        bad += all_giant<Data64>() + all_giant<Data32>();
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
