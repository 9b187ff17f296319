// emulate_hoisted_rotation.cpp -- inner_product_galois on the CPU: the kernel's own text (the kern namespace of
// csrc/hoisted_rotation.hip, cut out by tests/test_hoisted_rotation_host.py into kernel_extract.inc) compiled for the host
// against host_shim/hip/hip_runtime.h -- one std::thread per lane, a std::barrier for __syncthreads -- under
// AddressSanitizer and UBSan, and compared word for word with the definition in exact integers.  The sibling of
// emulate_hoisted_sum.cpp, with the same limits: index arithmetic, bounds, both loaders, the arithmetic at the edges of
// the word; nothing about waves, LDS banks or time.  A plain clang++ builds it; prints "ALL OK".
#include <hip/hip_runtime.h>

#include <cstdio>
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

template <typename T, bool VEC>
void launch(dim3 grid, unsigned nt, const T* a, const T* c0, T* acc, const T* consts, const kern::HoistArgs<T>& ha, int D,
            int count, int L, int M, int KM, int n, int logc, int neg)
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
                    kern::inner_product_galois<T, VEC>(a, c0, acc, consts, ha, D, count, L, M, KM, n, logc, neg);
                });
            for (auto& x : th)
                x.join();
        }
}

// top: the moduli lie below 2^(W-2), within an eighth of it -- all the kernel's bounds rest on is 3 q < 2^W -- otherwise
// below 2^(W-3), where no intermediate reaches 2^(W-1); ones: every word of a, c0 and the keys is 2^W - 1
template <typename T>
int run(int n, int logc, int D, int L, int K, int count, int G, bool with_c0, bool neg, int off, bool top = false,
        bool ones = false)
{
    constexpr int W = 8 * sizeof(T);
    const int M = L + K, KM = M + 1;
    const size_t N = size_t(1) << n;
    std::mt19937_64 rng(n * 1000 + logc * 100 + D * 10 + G + off);
    std::vector<T> q(M);
    for (int m = 0; m < M; m++)
    {
        // odd (not prime, not needed).  top: modulus 0 within 2000 of 2^(W-2), the others spread over the eighth below it:
        // right under a power of two 2^W mod q and 2^2W mod q are tiny, two of the fold's three terms carry all the
        // weight and the fold sum never passes 2 q -- only a modulus further down drives it into [2^(W-1), 3 q)
        const T away = top && m > 0 ? static_cast<T>(rng() % (T(1) << (W - 6))) : static_cast<T>(rng() % 1000);
        q[m] = static_cast<T>((T(1) << (top ? W - 2 : W - 3)) - 1 - 2 * away) | 1;
    }
    std::vector<T> consts(6 * M);
    for (int m = 0; m < M; m++)
    {
        const U128 t1 = (U128(1) << W) % q[m], t2 = t1 * t1 % q[m];
        consts[m] = q[m], consts[M + m] = T(t1), consts[2 * M + m] = T((t1 << W) / q[m]);
        consts[3 * M + m] = T(t2), consts[4 * M + m] = T((t2 << W) / q[m]), consts[5 * M + m] = T((U128(1) << W) / q[m]);
    }
    auto words = [&](size_t w) {
        std::vector<T> v(w + off + 4);
        for (auto& x : v)
            x = static_cast<T>(rng());
        for (size_t i = 0; i < v.size(); i += 97)
            v[i] = (i % 2) ? T(~T(0)) : T(0);
        if (ones)
            for (auto& x : v)
                x = T(~T(0));
        return v;
    };
    // buffers 16-byte aligned by construction of std::vector<T> (operator new: 16), then shifted by `off` words
    std::vector<T> a = words(size_t(D) * count * M * N), c0 = words(size_t(count) * L * N);
    std::vector<std::vector<T>> keys;
    kern::HoistArgs<T> ha{};
    ha.count = G;
    const std::uint32_t mask = neg ? (2u << n) - 1u : (1u << n) - 1u;
    for (int g = 0; g < G; g++)
    {
        keys.push_back(words(size_t(D) * 2 * KM * N));
        ha.key[g] = keys.back().data() + off;
        const std::uint32_t k = (static_cast<std::uint32_t>(rng()) | 1u) & mask;
        ha.elt[g] = g == 1 ? 1u : k, ha.inv[g] = galois_inverse(ha.elt[g]) & mask;
    }
    std::vector<T> pq(L);
    for (int m = 0; m < M; m++)
        ha.limb[m] = static_cast<unsigned char>(m < L ? m : m + 1); // the key has one limb more: skip limb L
    for (int m = 0; m < L; m++)
    {
        pq[m] = static_cast<T>(rng() % q[m]);
        ha.p_mod_q[m] = pq[m], ha.p_mod_q_shoup[m] = T((U128(pq[m]) << W) / q[m]);
    }
    const size_t acc_words = size_t(G) * 2 * count * M * N;
    std::vector<T> acc(acc_words + 64, T(0x5A));
    const T* pa = a.data() + off;
    const T* pc0 = with_c0 ? c0.data() + off : nullptr;
    unsigned nt = 64; // hoist_launch's rule
    while (nt < static_cast<unsigned>(kern::HOIST_NT) && nt < (1u << logc))
        nt *= 2;
    const dim3 grid(static_cast<unsigned>(count << (n - logc)), static_cast<unsigned>(M));
    const bool wide = ((sizeof(T) << logc) % 16 == 0) &&
                      ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pc0)) & 15u) == 0;
    if (wide)
        launch<T, true>(grid, nt, pa, pc0, acc.data() + 32, consts.data(), ha, D, count, L, M, KM, n, logc, neg);
    else
        launch<T, false>(grid, nt, pa, pc0, acc.data() + 32, consts.data(), ha, D, count, L, M, KM, n, logc, neg);
    // the definition
    size_t bad = 0;
    for (int g = 0; g < G; g++)
        for (int c = 0; c < 2; c++)
            for (int r = 0; r < count; r++)
                for (int m = 0; m < M; m++)
                    for (size_t j = 0; j < N; j++)
                    {
                        const size_t src = galois_ntt_source(static_cast<std::uint32_t>(j), ha.elt[g], n, neg);
                        U128 u = 0;
                        for (int d = 0; d < D; d++)
                        {
                            const U128 x = pa[((size_t(d) * count + r) * M + m) * N + src] % q[m];
                            const U128 k = ha.key[g][((size_t(d) * 2 + c) * KM + ha.limb[m]) * N + j] % q[m];
                            u = (u + x * k) % q[m];
                        }
                        if (c == 0 && m < L && with_c0)
                            u = (u + U128(pq[m]) * (pc0[(size_t(r) * L + m) * N + src] % q[m])) % q[m];
                        bad += acc[32 + (((size_t(g) * 2 + c) * count + r) * M + m) * N + j] != T(u);
                    }
    for (int i = 0; i < 32; i++)
        bad += acc[i] != T(0x5A) || acc[32 + acc_words + i] != T(0x5A);
    std::printf("W=%d n=%d logc=%d D=%d L=%d K=%d count=%d G=%d c0=%d neg=%d off=%d top=%d ones=%d vec=%d: %s (%zu)\n", W, n,
                logc, D, L, K, count, G, with_c0, neg, off, top, ones, wide, bad ? "WRONG" : "ok", bad);
    return bad != 0;
}

template <typename T> int all()
{
    int bad = 0;
    for (const bool top : {false, true})
    {
        bad += run<T>(1, 1, 2, 2, 1, 2, 3, true, true, 0, top);
        bad += run<T>(2, 2, 2, 2, 1, 1, 1, false, true, 0, top);
        bad += run<T>(5, 5, 3, 3, 2, 2, 5, true, true, 0, top);
        bad += run<T>(6, 6, 2, 3, 2, 1, 4, true, false, 0, top);
        bad += run<T>(7, 6, 2, 3, 2, 3, 5, true, true, 0, top);
        bad += run<T>(7, 6, 2, 3, 2, 2, 5, false, true, 1, top);
        bad += run<T>(9, 7, 3, 2, 1, 1, 3, true, false, 1, top);
        bad += run<T>(9, 9, 2, 2, 1, 2, 3, true, true, 0, top); // 512 slots on 256 lanes: two slots per lane
        // the largest sums: every operand word 2^W - 1, 64 elements and 64 digits
        bad += run<T>(6, 6, 2, 3, 2, 1, 64, true, true, 0, top, true);
        bad += run<T>(6, 6, 64, 1, 1, 1, 2, true, true, 0, top, true);
    }
    return bad;
}

int main()
{
    const int bad = all<Data64>() + all<Data32>();
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
