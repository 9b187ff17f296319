// emulate_rescale.cpp -- rescale_gather and rescale_sub_scale on the CPU: the kernels' own text (the kern namespace of
// csrc/rescale.hip, cut out by tests/rescale_utils.py into kernel_extract.inc) compiled for the host against
// host_shim/hip/hip_runtime.h -- one std::thread per lane -- under AddressSanitizer and UBSan, and compared word for word
// with exact integers (unsigned __int128 and %).  It checks the index arithmetic, the bounds of every access, both loaders
// and the arithmetic at the edges of the word; it says nothing about waves or time.  A plain clang++ builds it (no hipcc,
// no GPU, nothing preloaded).
//   emulate_rescale     one line per case, then "ALL OK" or "FAILED"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "inner_product_internal.hpp"
#include "rescale_internal.hpp"

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

// off: every operand starts `off` words behind a 16-byte boundary; top: the moduli lie below 2^(W-2), within an eighth of
// it, otherwise below 2^(W-3) with one 20-bit modulus among them; ones: every word of x is 2^W - 1 and every word of out the
// largest canonical one, q - 1
struct Shape
{
    int n, L, R, stacks, off;
    bool top = false, ones = false;
};

template <typename T> struct Fixture
{
    static constexpr int W = 8 * sizeof(T);
    static constexpr int VW = 16 / sizeof(T);
    const Shape s;
    const int keep;
    const size_t N;
    std::mt19937_64 rng;
    std::vector<T> q, consts, x, out;
    kern::RsOffsets off{};
    kern::RsDropped<T> dropped_mods{};
    size_t out_words = 0;

    explicit Fixture(const Shape& shape)
        : s(shape), keep(s.L - s.R), N(size_t(1) << s.n), rng(s.n * 1000 + s.L * 100 + s.stacks * 10 + s.off), q(keep),
          consts(4 * keep + 3)
    {
        for (int j = 0; j < keep; j++)
        {
            const T away = s.top && j > 0 ? static_cast<T>(rng() % (T(1) << (W - 6))) : static_cast<T>(rng() % 1000);
            q[j] = static_cast<T>((T(1) << (s.top ? W - 2 : W - 3)) - 1 - 2 * away) | 1;
            if (!s.top && j == 1)
                q[j] = static_cast<T>((T(1) << 20) - 3); // a 64-bit word modulo a 20-bit q
        }
        // the four arrays 1, 0, 3 and 2 words apart, as pieces of a larger image are
        off = kern::RsOffsets{1u, unsigned(1 + keep), unsigned(1 + 2 * keep + 2), unsigned(3 + 3 * keep)};
        for (int j = 0; j < keep; j++)
        {
            const T w = static_cast<T>(rng() % q[j]);
            consts[off.q + j] = q[j], consts[off.onep + j] = T((U128(1) << W) / q[j]);
            consts[off.qinv + j] = w, consts[off.qinvp + j] = T((U128(w) << W) / q[j]);
        }
        for (int i = 0; i < s.R; i++)
        {
            const T away = static_cast<T>(rng() % (T(1) << (W - 6)));
            const T m = i == 1 ? static_cast<T>((T(1) << 20) - 5) : static_cast<T>((T(1) << (W - 2)) - 1 - 2 * away) | 1;
            dropped_mods.q[i] = m, dropped_mods.onep[i] = T((U128(1) << W) / m);
        }
        x.resize(size_t(s.stacks) * s.L * N + s.off + 4);
        for (auto& e : x)
            e = s.ones ? T(~T(0)) : static_cast<T>(rng());
        for (size_t i = 0; !s.ones && i < x.size(); i += 97)
            x[i] = (i % 2) ? T(~T(0)) : T(0);
    }

    const T* px() const { return x.data() + s.off; }
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
    bool wide(const void* a, const void* b) const { return host::relin_wide<T>(s.n, {a, b}); }
    int report(const char* kernel, bool vec, size_t bad) const
    {
        std::printf("%s W=%d n=%d L=%d R=%d stacks=%d off=%d top=%d ones=%d vec=%d: %s (%zu)\n", kernel, W, s.n, s.L, s.R,
                    s.stacks, s.off, s.top, s.ones, vec, bad ? "WRONG" : "ok", bad);
        return bad != 0;
    }
};

// rescale_gather: dropped[s][i] = x[s][L - R + i] mod its modulus
template <typename T> int gather(const Shape& s)
{
    Fixture<T> f(s);
    T* dropped = f.guarded(size_t(s.stacks) * s.R * f.N);
    const bool vec = f.wide(f.px(), dropped);
    const host::RelinGrid g = host::relin_grid(s.n, vec ? f.VW : 1, s.stacks);
    const dim3 grid(g.blocks, s.R);
    const kern::RsDropped<T>& mods = f.dropped_mods;
    if (vec)
        launch(grid, g.nt, [&] { kern::rescale_gather<T, f.VW>(f.px(), dropped, mods, s.L, s.R, s.n, g.tiles); });
    else
        launch(grid, g.nt, [&] { kern::rescale_gather<T, 1>(f.px(), dropped, mods, s.L, s.R, s.n, g.tiles); });
    size_t bad = f.guards_touched();
    for (int st = 0; st < s.stacks; st++)
        for (int i = 0; i < s.R; i++)
            for (size_t j = 0; j < f.N; j++)
                bad += dropped[(size_t(st) * s.R + i) * f.N + j] !=
                       f.px()[(size_t(st) * s.L + f.keep + i) * f.N + j] % f.dropped_mods.q[i];
    return f.report("rescale_gather", vec, bad);
}

// rescale_sub_scale: out[s][j] = ((x[s][j] mod q_j) - out[s][j]) w_j mod q_j
template <typename T> int sub_scale(const Shape& s)
{
    Fixture<T> f(s);
    const size_t words = size_t(s.stacks) * f.keep * f.N;
    T* out = f.guarded(words);
    std::vector<T> before(words);
    for (int st = 0; st < s.stacks; st++)
        for (int j = 0; j < f.keep; j++)
            for (size_t c = 0; c < f.N; c++)
            {
                const size_t at = (size_t(st) * f.keep + j) * f.N + c;
                before[at] = s.ones ? T(f.q[j] - 1) : (at % 53 == 0 ? T(0) : static_cast<T>(f.rng() % f.q[j]));
                out[at] = before[at];
            }
    const bool vec = f.wide(f.px(), out);
    const host::RelinGrid g = host::relin_grid(s.n, vec ? f.VW : 1, s.stacks);
    const dim3 grid(g.blocks, f.keep);
    if (vec)
        launch(grid, g.nt, [&] {
            kern::rescale_sub_scale<T, f.VW>(f.px(), out, f.consts.data(), f.off, s.L, f.keep, s.n, g.tiles);
        });
    else
        launch(grid, g.nt,
               [&] { kern::rescale_sub_scale<T, 1>(f.px(), out, f.consts.data(), f.off, s.L, f.keep, s.n, g.tiles); });
    size_t bad = f.guards_touched();
    for (int st = 0; st < s.stacks; st++)
        for (int j = 0; j < f.keep; j++)
            for (size_t c = 0; c < f.N; c++)
            {
                const size_t at = (size_t(st) * f.keep + j) * f.N + c;
                const U128 q = f.q[j];
                const U128 xw = f.px()[(size_t(st) * s.L + j) * f.N + c] % q;
                const U128 want = (xw + q - before[at]) % q * f.consts[f.off.qinv + j] % q;
                bad += out[at] != T(want);
            }
    return f.report("rescale_sub_scale", vec, bad);
}

template <typename T> int all()
{
    int bad = 0;
    const Shape shapes[] = {
        // N = 2 .. 512, aligned and one word off; (L, R) = (3, 1), (6, 2), (4, 3), (2, 1)
        {1, 3, 1, 1, 0}, {1, 6, 2, 3, 1}, {2, 3, 1, 2, 0}, {2, 4, 3, 3, 1}, {3, 6, 2, 3, 0}, {3, 2, 1, 1, 1},
        {4, 4, 3, 2, 0}, {5, 3, 1, 3, 0}, {5, 6, 2, 1, 1}, {6, 2, 1, 3, 0}, {7, 6, 2, 2, 1}, {7, 3, 1, 1, 0},
        {8, 4, 3, 1, 1}, {9, 6, 2, 3, 0}, {9, 3, 1, 2, 1},
        // moduli within an eighth below 2^(W-2)
        {1, 3, 1, 2, 0, true}, {5, 6, 2, 3, 1, true}, {9, 3, 1, 1, 0, true}, {6, 4, 3, 2, 0, true},
        // every word of x 2^W - 1, every word of out q - 1
        {2, 3, 1, 1, 0, false, true}, {6, 6, 2, 3, 1, true, true}, {9, 4, 3, 2, 0, true, true},
        {4, 2, 1, 3, 1, false, true}};
    for (const Shape& s : shapes)
        bad += gather<T>(s) + sub_scale<T>(s);
    return bad;
}

int main()
{
    const int bad = all<Data64>() + all<Data32>();
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
