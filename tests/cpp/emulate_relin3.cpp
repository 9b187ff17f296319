// emulate_relin3.cpp -- inner_product_seeded and mod_down_add on the CPU: the kernels' own text (the kern namespace of
// csrc/relinearize.hip, cut out by tests/relin3_utils.py into kernel_extract.inc, over the digit loop of
// csrc/inner_product_internal.hpp; mod_down_add straight from csrc/base_conversion_internal.hpp) compiled for the host
// against host_shim/hip/hip_runtime.h -- one std::thread per lane -- under AddressSanitizer and UBSan.  It checks the index
// arithmetic, the bounds of every access (the outputs lie between guard bands), both loaders, the blocks of inputs with
// their ragged tails, the output split and the addend read in place; it says nothing about waves or time.  A plain
// clang++ builds it (no hipcc, no GPU, nothing preloaded).  The constants are derived here, in exact integers, not by the
// library; the expected words are tests/relin3_exact.py's, compared by the test.
//   emulate_relin3 JOB RESULT  JOB: 64-bit words -- the number of cases, then per case W, n_power, L, K, alpha, count,
//                              off (words by which every operand leaves 16-byte alignment), split (workgroups per
//                              column tile of mod_down_add), the M moduli, a[D][count][M][N], key[D][2][M + 1][N] (the
//                              plan skips key limb L), c01[2][count][L][N], x[2 count][M][N], addend[2 count][L][N]
//                              RESULT: per case inner_product_seeded's acc[2][count][M][N], mod_down_add's
//                              out[2 count][L][N], and the same with the addend given as out
//                              one line per case, then "ALL OK" or "FAILED" (a guard band was touched)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <thread>
#include <type_traits>
#include <vector>

#include "base_conversion_internal.hpp"
#include "inner_product_internal.hpp"
#include "relinearize_internal.hpp"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
std::barrier<>* g_block_barrier = nullptr;

namespace gpuntt
{
    namespace kern
    {
        __attribute__((aligned(16))) unsigned char bc_smem[65536];
#include "kernel_extract.inc"
    } // namespace kern
} // namespace gpuntt

using namespace gpuntt;
using U64 = unsigned long long;
using U128 = unsigned __int128;

// kernel(): one lane's call, with the launch's arguments bound.  The lanes of a workgroup share bc_smem, as on the device
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
// a^-1 mod m for gcd(a, m) = 1 (extended Euclid: the moduli need not be prime)
static U64 invmod(U64 a, U64 m)
{
    __int128 r0 = m, r1 = a % m, s0 = 0, s1 = 1;
    while (r1 != 0)
    {
        const __int128 q = r0 / r1, r2 = r0 - q * r1, s2 = s0 - q * s1;
        r0 = r1, r1 = r2, s0 = s1, s1 = s2;
    }
    return U64(((s0 % __int128(m)) + m) % m);
}

// the image of base_conversion_internal.hpp for {in} -> {out}
template <typename T> std::vector<T> image(kern::BcOffsets& o, const std::vector<U64>& in, const std::vector<U64>& out)
{
    constexpr int W = 8 * sizeof(T);
    const int L = int(in.size()), K = int(out.size()), KP = (K + kern::BC_KB - 1) / kern::BC_KB * kern::BC_KB;
    std::vector<T> run(5 * size_t(L) + size_t(L + 9) * KP, T(0));
    size_t at = 0;
    auto take = [&](size_t words) {
        const size_t first = at;
        at += words;
        return unsigned(first);
    };
    o.q = take(L), o.w = take(L), o.wp = take(L), o.recip = take(L), o.shift = take(L), o.matrix = take(size_t(L) * KP);
    o.p = take(KP), o.negq = take(KP), o.qinv = take(KP), o.qinvp = take(KP), o.t1 = take(KP), o.t1p = take(KP);
    o.t2 = take(KP), o.t2p = take(KP), o.onep = take(KP);
    auto hat = [&](int skip, U64 m) { // prod_{o != skip} in[o] mod m
        U64 r = 1 % m;
        for (int i = 0; i < L; i++)
            if (i != skip)
                r = mulmod(r, in[i] % m, m);
        return r;
    };
    auto shoup = [](U64 v, U64 m) { return T((U128(v) << W) / m); };
    for (int i = 0; i < L; i++)
    {
        const U64 q = in[i], w = invmod(hat(i, q), q);
        int b = 0;
        for (U64 v = q; v != 0; v >>= 1)
            b++;
        const U128 r = (U128(1) << (W - 1 + b)) / q;
        run[o.q + i] = T(q), run[o.w + i] = T(w), run[o.wp + i] = shoup(w, q);
        run[o.recip + i] = (r >> W) != 0 ? T(0) : T(r), run[o.shift + i] = T(b - 1);
        for (int j = 0; j < K; j++)
            run[o.matrix + size_t(i) * KP + j] = T(hat(i, out[j]));
    }
    for (int j = 0; j < K; j++)
    {
        const U64 p = out[j], Q = hat(-1, p), qi = invmod(Q, p), t1 = U64((U128(1) << W) % p), t2 = mulmod(t1, t1, p);
        run[o.p + j] = T(p), run[o.negq + j] = T(Q == 0 ? 0 : p - Q), run[o.qinv + j] = T(qi);
        run[o.qinvp + j] = shoup(qi, p), run[o.t1 + j] = T(t1), run[o.t1p + j] = shoup(t1, p), run[o.t2 + j] = T(t2);
        run[o.t2p + j] = shoup(t2, p), run[o.onep + j] = shoup(1, p);
    }
    return run;
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

template <typename T> size_t run_case(int n, int L, int K, int alpha, int count, int off, int split, std::FILE* res)
{
    constexpr int W = 8 * sizeof(T), VW = 16 / sizeof(T);
    const int M = L + K, KM = M + 1, D = (L + alpha - 1) / alpha, stacks = 2 * count;
    const size_t N = size_t(1) << n;
    std::vector<U64> mods(M);
    for (auto& m : mods)
        m = next();
    const std::vector<U64> qs(mods.begin(), mods.begin() + L), ps(mods.begin() + L, mods.end());
    auto read = [&](size_t words) {
        Guarded<T> gd(words, off);
        for (size_t i = 0; i < words; i++)
            gd.data()[i] = T(next());
        return gd;
    };
    Guarded<T> a = read(size_t(D) * count * M * N), key = read(size_t(D) * 2 * KM * N),
               c01 = read(size_t(2) * count * L * N), x = read(size_t(stacks) * M * N),
               addend = read(size_t(stacks) * L * N);

    // the fold image of InnerProductPlan and the kernel argument
    std::vector<T> fold(6 * size_t(M));
    auto shoup = [](U64 v, U64 m) { return T((U128(v) << W) / m); };
    for (int m = 0; m < M; m++)
    {
        const U64 q = mods[m], t1 = U64((U128(1) << W) % q), t2 = mulmod(t1, t1, q);
        fold[m] = T(q), fold[M + m] = T(t1), fold[2 * M + m] = shoup(t1, q);
        fold[3 * M + m] = T(t2), fold[4 * M + m] = shoup(t2, q), fold[5 * M + m] = shoup(1, q);
    }
    kern::RelinArgs<T> ra{};
    for (int m = 0; m < M; m++)
        ra.limbs.v[m] = static_cast<unsigned char>(m < L ? m : m + 1); // the key has one limb more: skip limb L
    for (int m = 0; m < L; m++)
    {
        U64 pq = 1 % qs[m];
        for (U64 p : ps)
            pq = mulmod(pq, p % qs[m], qs[m]);
        ra.p_mod_q[m] = T(pq), ra.p_mod_q_shoup[m] = shoup(pq, qs[m]);
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

    // inner_product_seeded, launched as relin_seeded_launch launches it
    bool vec;
    int rb;
    {
        Guarded<T> acc(size_t(2) * count * M * N, off);
        vec = host::relin_wide<T>(n, {a.data(), key.data(), acc.data(), c01.data()});
        rb = count >= 4 ? 4 : count >= 2 ? 2 : 1;
        const host::RelinGrid g = host::relin_grid(n, vec ? VW : 1, U64(count + rb - 1) / rb);
        const dim3 grid(g.blocks, M);
        auto call = [&](auto v, auto b) {
            return [&, v, b] {
                kern::inner_product_seeded<T, decltype(v)::value, decltype(b)::value>(
                    a.data(), key.data(), acc.data(), fold.data(), c01.data(), ra, D, count, L, M, KM, n, g.tiles);
            };
        };
        auto with_v = [&](auto v) {
            if (rb == 4)
                launch(grid, g.nt, call(v, std::integral_constant<int, 4>{}));
            else if (rb == 2)
                launch(grid, g.nt, call(v, std::integral_constant<int, 2>{}));
            else
                launch(grid, g.nt, call(v, std::integral_constant<int, 1>{}));
        };
        if (vec)
            with_v(std::integral_constant<int, VW>{});
        else
            with_v(std::integral_constant<int, 1>{});
        write(acc);
    }

    // mod_down_add, launched as KeySwitchPlan::mod_down_add launches it: the special limbs read in place
    kern::BcOffsets down{};
    const std::vector<T> img = image<T>(down, ps, qs);
    const int LP = (L + kern::BC_KB - 1) / kern::BC_KB * kern::BC_KB;
    const U64 total = U64(stacks) << n, full = U64(M) << n;
    const dim3 grid(unsigned((total + kern::BC_NT - 1) / kern::BC_NT), unsigned(split));
    const kern::BcStrides<true> strides{full, full, U64(L) << n};
    auto mod_down_add = [&](const T* add, T* o) {
        launch(grid, kern::BC_NT, [&] {
            kern::mod_down_add<T>(x.data() + L * N, x.data(), add, o, img.data(), down, K, L, LP, n, total, strides);
        });
    };
    {
        Guarded<T> o(size_t(stacks) * L * N, off);
        mod_down_add(addend.data(), o.data());
        write(o);
    }
    {
        Guarded<T> o(size_t(stacks) * L * N, off); // the addend exactly out
        std::copy(addend.data(), addend.data() + addend.words, o.data());
        mod_down_add(o.data(), o.data());
        write(o);
    }
    bad += a.touched() + key.touched() + c01.touched() + x.touched() + addend.touched();
    std::printf("W=%d n=%d L=%d K=%d alpha=%d count=%d off=%d split=%d vec=%d rb=%d: %s (%zu)\n", W, n, L, K, alpha, count,
                off, split, vec, rb, bad ? "GUARD TOUCHED" : "ok", bad);
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
                  count = int(next()), off = int(next()), split = int(next());
        bad += W == 64 ? run_case<Data64>(n, L, K, alpha, count, off, split, res)
                       : run_case<Data32>(n, L, K, alpha, count, off, split, res);
    }
    std::fclose(res);
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
