// emulate_bfv.cpp -- bfv_extend, bfv_scale_round and bfv_tensor on the CPU: the kernels' own text (the kern namespace of
// csrc/bfv_multiply.hip, cut out by tests/bfv_utils.py into kernel_extract.inc) compiled for the host against
// host_shim/hip/hip_runtime.h -- one std::thread per lane -- under AddressSanitizer and UBSan.  It checks the index
// arithmetic, the bounds of every access (the outputs lie between guard bands), both loaders of bfv_tensor and the
// arithmetic at the edges of the word; it says nothing about waves or time.  A plain clang++ builds it (no hipcc, no GPU,
// nothing preloaded).  The constants are derived here, in exact integers, not by the library.
//   emulate_bfv JOB RESULT    JOB: 64-bit words -- the number of cases, then per case W, n_power, L, K, stacks, count, t,
//                             off (words by which every operand leaves 16-byte alignment), the M moduli, in[stacks][L][N],
//                             full[stacks][M][N], xe[2][count][M][N], ye[2][count][M][N]
//                             RESULT: per case extend's full[stacks][M][N], scale_round's out[stacks][L][N], bfv_tensor's
//                             d[3][count][M][N] for (xe, ye) and d[3][count][M][N] for the squaring (xe, xe) written over xe
//                             one line per case, then "ALL OK" or "FAILED" (a guard band was touched)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

#include "bfv_multiply_internal.hpp"
#include "relinearize_internal.hpp"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
std::barrier<>* g_block_barrier = nullptr;

namespace gpuntt
{
    namespace kern
    {
        __attribute__((aligned(16))) unsigned char bfv_smem[65536];
#include "kernel_extract.inc"
    } // namespace kern
} // namespace gpuntt

using namespace gpuntt;
using U64 = unsigned long long;
using U128 = unsigned __int128;

// kernel(): one lane's call, with the launch's arguments bound.  The lanes of a workgroup share bfv_smem, as on the device
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

// the image of base_conversion_internal.hpp for {in} -> {out}, appended to `run`; every offset counts from run's start
template <typename T>
kern::BcOffsets image(std::vector<T>& run, const std::vector<U64>& in, const std::vector<U64>& out)
{
    constexpr int W = 8 * sizeof(T);
    const int L = int(in.size()), K = int(out.size()), KP = (K + kern::BC_KB - 1) / kern::BC_KB * kern::BC_KB;
    const size_t base = run.size();
    run.resize(base + 5 * size_t(L) + size_t(L + 9) * KP, T(0));
    size_t at = base;
    auto take = [&](size_t words) {
        const size_t first = at;
        at += words;
        return unsigned(first);
    };
    kern::BcOffsets o{};
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
    return o;
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

template <typename T> size_t run_case(int n, int L, int K, int stacks, int count, U64 t, int off, std::FILE* res)
{
    constexpr int W = 8 * sizeof(T), VW = 16 / sizeof(T);
    const int M = L + K, KP = (K + kern::BC_KB - 1) / kern::BC_KB * kern::BC_KB;
    const int LP = (L + kern::BC_KB - 1) / kern::BC_KB * kern::BC_KB;
    const size_t N = size_t(1) << n;
    std::vector<U64> mods(M);
    for (auto& m : mods)
        m = next();
    const std::vector<U64> qs(mods.begin(), mods.begin() + L), bs(mods.begin() + L, mods.end());
    auto read = [&](size_t words) {
        Guarded<T> gd(words, off);
        for (size_t i = 0; i < words; i++)
            gd.data()[i] = T(next());
        return gd;
    };
    Guarded<T> in = read(stacks * L * N), full = read(stacks * M * N), xe = read(2 * count * M * N),
               ye = read(2 * count * M * N);

    // the run of constants: a word of padding, the two images, the plan's own arrays, the fold image
    std::vector<T> run(1, T(0));
    const kern::BcOffsets up = image<T>(run, qs, bs), down = image<T>(run, bs, qs);
    kern::BfvOffsets ex{};
    auto shoup = [](U64 v, U64 m) { return T((U128(v) << W) / m); };
    ex.wt = unsigned(run.size()), ex.wtp = ex.wt + L, ex.onepq = ex.wtp + L, ex.tb = ex.onepq + L, ex.tbp = ex.tb + KP;
    run.resize(ex.tbp + KP, T(0));
    for (int i = 0; i < L; i++)
    {
        const U64 w = mulmod(t % qs[i], U64(run[up.w + i]), qs[i]);
        run[ex.wt + i] = T(w), run[ex.wtp + i] = shoup(w, qs[i]), run[ex.onepq + i] = shoup(1, qs[i]);
    }
    for (int j = 0; j < K; j++)
        run[ex.tb + j] = T(t % bs[j]), run[ex.tbp + j] = shoup(t % bs[j], bs[j]);
    const size_t fold = run.size();
    run.resize(fold + 6 * size_t(M));
    for (int m = 0; m < M; m++)
    {
        const U64 q = mods[m], t1 = U64((U128(1) << W) % q), t2 = mulmod(t1, t1, q);
        run[fold + m] = T(q), run[fold + M + m] = T(t1), run[fold + 2 * M + m] = shoup(t1, q);
        run[fold + 3 * M + m] = T(t2), run[fold + 4 * M + m] = shoup(t2, q), run[fold + 5 * M + m] = shoup(1, q);
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
    const U64 total = U64(stacks) << n;
    const dim3 grid(unsigned((total + kern::BC_NT - 1) / kern::BC_NT));
    {
        Guarded<T> o(stacks * M * N, off);
        launch(grid, kern::BC_NT,
               [&] { kern::bfv_extend<T>(in.data(), o.data(), run.data(), up, ex, L, K, KP, n, total); });
        write(o);
    }
    {
        Guarded<T> o(stacks * L * N, off);
        launch(grid, kern::BC_NT, [&] {
            kern::bfv_scale_round<T>(full.data(), o.data(), run.data(), up, down, ex, L, K, KP, LP, n, total);
        });
        write(o);
    }
    auto tensor = [&](const T* x, const T* y, T* d) {
        const bool vec = host::relin_wide<T>(n, {x, y, d});
        const host::RelinGrid g = host::relin_grid(n, vec ? VW : 1, count);
        const dim3 tg(g.blocks, M);
        if (vec)
            launch(tg, g.nt, [&] { kern::bfv_tensor<T, VW>(x, y, d, run.data() + fold, count, M, n, g.tiles); });
        else
            launch(tg, g.nt, [&] { kern::bfv_tensor<T, 1>(x, y, d, run.data() + fold, count, M, n, g.tiles); });
        return vec;
    };
    bool vec;
    {
        Guarded<T> o(3 * count * M * N, off);
        vec = tensor(xe.data(), ye.data(), o.data());
        write(o);
    }
    {
        // the squaring, in place: d over (x0, x1) and the N count M words behind them, as multiply lays its scratch out
        Guarded<T> o(3 * count * M * N, off);
        std::copy(xe.data(), xe.data() + 2 * count * M * N, o.data());
        tensor(o.data(), o.data(), o.data());
        write(o);
    }
    bad += in.touched() + full.touched() + xe.touched() + ye.touched();
    std::printf("W=%d n=%d L=%d K=%d stacks=%d count=%d off=%d vec=%d: %s (%zu)\n", W, n, L, K, stacks, count, off, vec,
                bad ? "GUARD TOUCHED" : "ok", bad);
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
        const int W = int(next()), n = int(next()), L = int(next()), K = int(next()), stacks = int(next()),
                  count = int(next());
        const U64 t = next();
        const int off = int(next());
        bad += W == 64 ? run_case<Data64>(n, L, K, stacks, count, t, off, res)
                       : run_case<Data32>(n, L, K, stacks, count, t, off, res);
    }
    std::fclose(res);
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
