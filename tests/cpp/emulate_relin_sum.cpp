// emulate_relin_sum.cpp -- tensor_top_sum and inner_product_tensor_sum on the CPU: the kernels' own text (the kern
// namespace of csrc/relinearize_sum.hip, cut out by tests/relin_sum_emulator.py into kernel_extract.inc, over the digit
// loop of csrc/inner_product_internal.hpp) compiled for the host against host_shim/hip/hip_runtime.h -- one std::thread
// per lane -- under AddressSanitizer and UBSan, and compared word for word with the definitions in exact integers.  It
// checks the index arithmetic, the bounds of every access, both loaders, every block of inputs with its ragged tail, the
// term loop and the arithmetic at the edges of the word (the largest carry count); it says nothing about waves or time.
// A plain clang++ builds it (no hipcc, no GPU, nothing preloaded).
//   emulate_relin_sum     one line per case, then "ALL OK" or "FAILED"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <thread>
#include <type_traits>
#include <vector>

#include "inner_product_internal.hpp"
#include "relinearize_sum_internal.hpp"

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

// the shape of one case.  terms: pairs summed; off: every operand starts `off` words behind a 16-byte boundary; one_off:
// only x of the last term does, which must switch the whole case to V = 1; dup: the last term's x is the first term's
// (one pointer in two terms); top: the moduli lie below
// 2^(W-2), within an eighth of it -- all the kernels' bounds rest on is 3 q < 2^W -- otherwise below 2^(W-3); ones: every
// word of x, y, a and the key is 2^W - 1, the largest sum the accumulators can be given; same: y[t] is x[t] (squares)
struct Shape
{
    int n, L, K, alpha, count, terms, off;
    bool top = false, ones = false, same = false, one_off = false, dup = false;
};

template <typename T> struct Fixture
{
    static constexpr int W = 8 * sizeof(T);
    static constexpr int VW = 16 / sizeof(T);
    const Shape s;
    const int M, KM, D;
    const size_t N;
    std::mt19937_64 rng;
    std::vector<T> q, consts, a, key, pq, out;
    std::vector<std::vector<T>> x, y;
    kern::RelinSumArgs<T> sa{};
    size_t out_words = 0;

    std::vector<T> words(size_t w)
    {
        std::vector<T> v(w + s.off + 1 + 4);
        for (auto& e : v)
            e = static_cast<T>(rng());
        for (size_t i = 0; i < v.size(); i += 97)
            v[i] = (i % 2) ? T(~T(0)) : T(0);
        if (s.ones)
            for (auto& e : v)
                e = T(~T(0));
        return v;
    }

    explicit Fixture(const Shape& shape)
        : s(shape), M(s.L + s.K), KM(M + 1), D((s.L + s.alpha - 1) / s.alpha), N(size_t(1) << s.n),
          rng(s.n * 1000 + s.L * 100 + s.count * 10 + s.off + 7 * s.terms), q(M), consts(6 * M), pq(s.L)
    {
        for (int m = 0; m < M; m++)
        {
            // odd (not prime, not needed).  top: modulus 0 within 2000 of 2^(W-2), the others spread over the eighth below
            // it, where the fold sum reaches [2^(W-1), 3 q)
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
        a = words(size_t(D) * s.count * M * N), key = words(size_t(D) * 2 * KM * N);
        for (int t = 0; t < s.terms; t++)
            x.push_back(words(size_t(2) * s.count * s.L * N)), y.push_back(words(size_t(2) * s.count * s.L * N));
        sa.terms = s.terms;
        for (int t = 0; t < s.terms; t++)
            sa.x[t] = px(t), sa.y[t] = py(t);
        kern::RelinArgs<T>& ra = sa.r;
        for (int m = 0; m < M; m++)
            ra.limbs.v[m] = static_cast<unsigned char>(m < s.L ? m : m + 1); // the key has one limb more: skip limb L
        for (int m = 0; m < s.L; m++)
        {
            pq[m] = static_cast<T>(rng() % q[m]);
            ra.p_mod_q[m] = pq[m], ra.p_mod_q_shoup[m] = T((U128(pq[m]) << W) / q[m]);
        }
    }

    const T* pa() const { return a.data() + s.off; }
    const T* pk() const { return key.data() + s.off; }
    const T* px(int t) const
    {
        if (s.dup && t == s.terms - 1)
            return px(0);
        return x[t].data() + s.off + (s.one_off && t == s.terms - 1 ? 1 : 0);
    }
    const T* py(int t) const { return s.same ? px(t) : y[t].data() + s.off; }
    // `w` words between two guard bands of 32 words, the first word `off` behind a 16-byte boundary
    T* guarded(size_t w)
    {
        out_words = w;
        out.assign(w + 64 + s.off, T(0x5A));
        return out.data() + 32 + s.off;
    }
    size_t guards_touched() const
    {
        size_t bad = 0;
        for (int i = 0; i < 32 + s.off; i++)
            bad += out[i] != T(0x5A);
        for (int i = 0; i < 32; i++)
            bad += out[32 + s.off + out_words + i] != T(0x5A);
        return bad;
    }
    // the launchers' decisions (relin_wide, relin_grid)
    bool wide(std::initializer_list<const void*> bases) const
    {
        uintptr_t bits = 0;
        for (const void* p : bases)
            bits |= reinterpret_cast<uintptr_t>(p);
        for (int t = 0; t < s.terms; t++)
            bits |= reinterpret_cast<uintptr_t>(px(t)) | reinterpret_cast<uintptr_t>(py(t));
        return s.n >= (sizeof(T) == 8 ? 1 : 2) && (bits & 15u) == 0;
    }
    void grid(int V, unsigned& nt, unsigned& tiles) const
    {
        const size_t lanes = N / V;
        nt = 64;
        while (nt < 256u && nt < lanes)
            nt *= 2;
        tiles = static_cast<unsigned>((lanes + nt - 1) / nt);
    }
    U128 word(const T* p, int c, int r, int m, size_t j) const
    {
        return p[((size_t(c) * s.count + r) * s.L + m) * N + j] % q[m];
    }
    int report(const char* kernel, bool vec, int rb, size_t bad) const
    {
        std::printf("%s W=%d n=%d L=%d K=%d alpha=%d count=%d terms=%d off=%d top=%d ones=%d same=%d one_off=%d dup=%d "
                    "vec=%d rb=%d: %s (%zu)\n",
                    kernel, W, s.n, s.L, s.K, s.alpha, s.count, s.terms, s.off, s.top, s.ones, s.same, s.one_off, s.dup, vec,
                    rb, bad ? "WRONG" : "ok", bad);
        return bad != 0;
    }
};

// tensor_top_sum: d2[r][m][j] = (sum_t x1_t y1_t) mod q_m
template <typename T> int top(const Shape& s)
{
    Fixture<T> f(s);
    const size_t comp = size_t(s.count) * s.L * f.N;
    T* d2 = f.guarded(comp);
    const bool vec = f.wide({d2});
    unsigned nt, tiles;
    f.grid(vec ? f.VW : 1, nt, tiles);
    const dim3 grid(tiles * s.count, s.L);
    if (vec)
        launch(grid, nt, [&] { kern::tensor_top_sum<T, f.VW>(d2, f.consts.data(), f.sa, s.count, s.L, f.M, s.n, tiles); });
    else
        launch(grid, nt, [&] { kern::tensor_top_sum<T, 1>(d2, f.consts.data(), f.sa, s.count, s.L, f.M, s.n, tiles); });
    size_t bad = f.guards_touched();
    for (int r = 0; r < s.count; r++)
        for (int m = 0; m < s.L; m++)
            for (size_t j = 0; j < f.N; j++)
            {
                U128 u = 0;
                for (int t = 0; t < s.terms; t++)
                    u = (u + f.word(f.px(t), 1, r, m, j) * f.word(f.py(t), 1, r, m, j)) % f.q[m];
                bad += d2[(size_t(r) * s.L + m) * f.N + j] != T(u);
            }
    return f.report("tensor_top_sum", vec, 0, bad);
}

// inner_product_tensor_sum: acc[c][r][m][j] = (sum_d a key + [m < L] (P mod q_m) d_c) mod q_m, d_c summed over the terms
template <typename T> int inner(const Shape& s)
{
    Fixture<T> f(s);
    T* acc = f.guarded(size_t(2) * s.count * f.M * f.N);
    const bool vec = f.wide({f.pa(), f.pk(), acc});
    static_assert(kern::RELIN_SUM_BLOCK == 2, "the blocks below are relin_sum_inner_v's");
    const int rb = s.count >= 2 ? 2 : 1;
    unsigned nt, tiles;
    f.grid(vec ? f.VW : 1, nt, tiles);
    const dim3 grid(tiles * ((s.count + rb - 1) / rb), f.M);
    auto call = [&](auto v, auto b) {
        return [&, v, b] {
            kern::inner_product_tensor_sum<T, decltype(v)::value, decltype(b)::value>(
                f.pa(), f.pk(), acc, f.consts.data(), f.sa, f.D, s.count, s.L, f.M, f.KM, s.n, tiles);
        };
    };
    auto with_v = [&](auto v) {
        if (rb == 2)
            launch(grid, nt, call(v, std::integral_constant<int, 2>{}));
        else
            launch(grid, nt, call(v, std::integral_constant<int, 1>{}));
    };
    if (vec)
        with_v(std::integral_constant<int, f.VW>{});
    else
        with_v(std::integral_constant<int, 1>{});
    size_t bad = f.guards_touched();
    for (int c = 0; c < 2; c++)
        for (int r = 0; r < s.count; r++)
            for (int m = 0; m < f.M; m++)
                for (size_t j = 0; j < f.N; j++)
                {
                    const U128 q = f.q[m];
                    U128 u = 0;
                    for (int d = 0; d < f.D; d++)
                    {
                        const U128 av = f.pa()[((size_t(d) * s.count + r) * f.M + m) * f.N + j] % q;
                        const U128 kv = f.pk()[((size_t(d) * 2 + c) * f.KM + f.sa.r.limbs.v[m]) * f.N + j] % q;
                        u = (u + av * kv) % q;
                    }
                    if (m < s.L)
                    {
                        U128 dc = 0;
                        for (int t = 0; t < s.terms; t++)
                        {
                            const U128 x0 = f.word(f.px(t), 0, r, m, j), x1 = f.word(f.px(t), 1, r, m, j);
                            const U128 y0 = f.word(f.py(t), 0, r, m, j), y1 = f.word(f.py(t), 1, r, m, j);
                            dc = (dc + (c == 0 ? x0 * y0 % q : (x0 * y1 % q + x1 * y0 % q) % q)) % q;
                        }
                        u = (u + U128(f.pq[m]) * dc) % q;
                    }
                    bad += acc[((size_t(c) * s.count + r) * f.M + m) * f.N + j] != T(u);
                }
    return f.report("inner_product_tensor_sum", vec, rb, bad);
}

template <typename T> int all()
{
    int bad = 0;
    const Shape shapes[] = {
        // {n, L, K, alpha, count, terms, off, top, ones, same, one_off, dup}
        // N = 2 .. 512; count 1 / 2 / 3 / 5: RB = 1, 2 (whole), 2 (ragged, two and three blocks); terms 1, 2, 3
        {1, 3, 2, 2, 1, 1, 0}, {1, 3, 2, 2, 3, 2, 0}, {1, 6, 2, 2, 5, 3, 1}, {2, 3, 2, 2, 2, 3, 0}, {2, 6, 2, 2, 5, 2, 0},
        {3, 3, 2, 2, 5, 1, 0}, {3, 6, 2, 2, 3, 3, 1}, {5, 6, 2, 2, 3, 2, 0}, {5, 3, 2, 2, 1, 3, 1}, {7, 6, 2, 2, 5, 3, 1},
        {7, 3, 2, 2, 2, 1, 0}, {9, 6, 2, 2, 1, 2, 0}, {9, 3, 2, 2, 5, 3, 0}, {9, 3, 2, 2, 2, 2, 1},
        // terms = 32
        {4, 3, 2, 2, 5, 32, 0}, {6, 6, 2, 2, 1, 32, 0}, {3, 3, 2, 2, 3, 32, 1}, {5, 3, 2, 2, 2, 32, 0, true},
        // D = 20
        {6, 20, 2, 1, 3, 3, 0}, {4, 20, 2, 1, 5, 2, 1}, {7, 20, 2, 1, 1, 3, 0}, {5, 20, 2, 1, 2, 1, 0, true},
        // moduli within an eighth below 2^(W-2)
        {7, 3, 2, 2, 2, 3, 0, true}, {9, 3, 2, 2, 5, 2, 0, true}, {5, 6, 2, 2, 3, 3, 1, true}, {2, 6, 2, 2, 1, 2, 0, true},
        // every operand word 2^W - 1 at terms = 32: the largest carry count
        {6, 3, 2, 2, 5, 32, 0, false, true}, {5, 6, 2, 2, 2, 32, 1, true, true}, {4, 20, 2, 1, 3, 32, 0, true, true},
        // y[t] = x[t]
        {5, 6, 2, 2, 3, 3, 0, false, false, true}, {8, 3, 2, 2, 1, 2, 0, true, false, true},
        {6, 3, 2, 2, 5, 32, 1, true, true, true},
        // one operand of one term one word off alignment: the whole case runs at V = 1
        {5, 3, 2, 2, 5, 3, 0, false, false, false, true}, {7, 6, 2, 2, 2, 2, 0, true, false, false, true},
        {4, 3, 2, 2, 1, 32, 0, false, false, false, true},
        // one pointer used in two terms
        {5, 3, 2, 2, 3, 3, 0, false, false, false, false, true}, {6, 6, 2, 2, 5, 2, 0, true, false, true, false, true}};
    for (const Shape& s : shapes)
        bad += top<T>(s) + inner<T>(s);
    return bad;
}

int main()
{
    const int bad = all<Data64>() + all<Data32>();
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
