// emulate_decrypt.cpp -- decrypt_phase, encrypt_public_combine, bfv_scale_message and bfv_decode on the CPU: the kernels'
// own text (the kern namespace of csrc/decrypt.hip, cut out by tests/decrypt_utils.py into kernel_extract.inc, over the
// accumulator and the fold of csrc/inner_product_internal.hpp and bc_z of csrc/base_conversion_internal.hpp) compiled
// for the host against host_shim/hip/hip_runtime.h -- one std::thread per lane, __syncthreads a std::barrier -- under
// AddressSanitizer and UBSan.  It checks the index arithmetic, the bounds of every access (every buffer lies between
// guard bands), both loaders, the workgroup reduction with lanes past the ring (the wave step is this program's own:
// dec_wave_max below), and the word arithmetic at its extremes; it says nothing about waves or time.  A plain clang++ builds it (no hipcc, no GPU, nothing preloaded).  The
// constants are derived here, in exact integers, not by the library; the expected words are tests/decrypt_exact.py's,
// compared by the test.
//   emulate_decrypt JOB RESULT  JOB: 64-bit words -- the number of cases, then per case W, n_power, L, count, off (words
//                               by which every operand leaves 16-byte alignment), t, the L moduli,
//                               ct[3][count][L][N], s[L][N], pk[2][L][N], lifted[3][count][L][N], msg[count][L][N],
//                               message[count][N], x[count][L][N]
//                               RESULT: per case decrypt_phase's out[count][L][N] for 2 and for 3 components, the third
//                               time written over ct's component 0 (3 components), encrypt_public_combine's
//                               out[2][count][L][N] with the message and without, bfv_scale_message's out[count][L][N],
//                               bfv_decode's message[count][N] and noise_max[count], the same two from the
//                               two-launch form (partial maxima, bfv_decode_merge), and message[count][N] once more
//                               from the call without noise_max
//                               one line per case, then "ALL OK" or "FAILED" (a guard band or an input was touched)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

#include "decrypt_internal.hpp"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
std::barrier<>* g_block_barrier = nullptr;

// the one atomic of the unit: a workgroup's lane 0 merges its maximum (workgroups run one after another here)
template <typename T> static T atomicMax(T* at, T v)
{
    const T old = *at;
    *at = std::max(old, v);
    return old;
}

namespace gpuntt
{
    namespace kern
    {
        __align__(16) unsigned char dec_smem[IP_NT * 8];
        // the wave primitive of the unit, over this program's threads: every lane of a "wave" of 64 threads gets the
        // maximum of the wave (the device exchanges lanes; here the words meet in an array between two barriers)
        constexpr unsigned DEC_WAVE = 64;
        static unsigned long long g_wave_words[IP_NT];
        template <typename T> T dec_wave_max(T v)
        {
            g_wave_words[threadIdx.x] = v;
            __syncthreads();
            const unsigned first = threadIdx.x / DEC_WAVE * DEC_WAVE;
            T best = 0;
            for (unsigned i = first; i < first + DEC_WAVE && i < blockDim.x; i++)
                best = std::max(best, static_cast<T>(g_wave_words[i]));
            __syncthreads();
            return best;
        }
#include "kernel_extract.inc"
    } // namespace kern
} // namespace gpuntt

using namespace gpuntt;
using U64 = unsigned long long;
using U128 = unsigned __int128;

// kernel(): one lane's call, with the launch's arguments bound; the lanes of a workgroup share a barrier
template <typename Kernel> void launch(dim3 grid, unsigned nt, Kernel kernel)
{
    for (unsigned by = 0; by < grid.y; by++)
        for (unsigned bx = 0; bx < grid.x; bx++)
        {
            std::barrier<> barrier(nt);
            g_block_barrier = &barrier;
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; t++)
                th.emplace_back([&, t] {
                    threadIdx = dim3(t), blockIdx = dim3(bx, by), blockDim = dim3(nt), gridDim = grid;
                    kernel();
                });
            for (auto& x : th)
                x.join();
            g_block_barrier = nullptr;
        }
}

static U64 mulmod(U64 a, U64 b, U64 m) { return U64(U128(a) * b % m); }
static U64 invmod(U64 a, U64 m) // a^-1 mod m, gcd(a, m) = 1
{
    __int128 r0 = m, r1 = a % m, c0 = 0, c1 = 1;
    while (r1 != 0)
    {
        const __int128 q = r0 / r1, r2 = r0 - q * r1, c2 = c0 - q * c1;
        r0 = r1, r1 = r2, c0 = c1, c1 = c2;
    }
    return U64(c0 < 0 ? c0 + m : c0);
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

template <typename T> size_t run_case(int n, int L, int count, int off, U64 t, std::FILE* res)
{
    constexpr int W = 8 * sizeof(T), VW = 16 / sizeof(T);
    const int M = L; // the fold image of the q-base alone
    const size_t N = size_t(1) << n;
    std::vector<U64> mods(L);
    for (auto& m : mods)
        m = next();
    auto read = [&](size_t words) {
        Guarded<T> gd(words, off);
        for (size_t i = 0; i < words; i++)
            gd.data()[i] = T(next());
        return gd;
    };
    const size_t stack = size_t(count) * L * N;
    Guarded<T> ct = read(3 * stack), s = read(size_t(L) * N), pk = read(size_t(2) * L * N), lifted = read(3 * stack);
    Guarded<T> msg = read(stack), message = read(size_t(count) * N), x = read(stack);
    const std::vector<T> ct0(ct.data(), ct.data() + ct.words), lifted0(lifted.data(), lifted.data() + lifted.words);

    // the fold image, the decode image (q, qhat^-1 and its companion, R, b - 1) and the constants of t
    auto shoup = [](U64 v, U64 m) { return T((U128(v) << W) / m); };
    std::vector<T> fold(6 * size_t(M)), image(5 * size_t(L));
    kern::BfvDecodeArgs<T> dargs{};
    kern::BfvScaleArgs<T> sargs{};
    U64 q_mod_t = 1 % t;
    for (int m = 0; m < L; m++)
    {
        const U64 q = mods[m], t1 = U64((U128(1) << W) % q), t2 = mulmod(t1, t1, q);
        fold[m] = T(q), fold[M + m] = T(t1), fold[2 * M + m] = shoup(t1, q);
        fold[3 * M + m] = T(t2), fold[4 * M + m] = shoup(t2, q), fold[5 * M + m] = shoup(1, q);
        U64 hat = 1 % q;
        for (int k = 0; k < L; k++)
            if (k != m)
                hat = mulmod(hat, mods[k] % q, q);
        const U64 w = invmod(hat, q);
        int b = 0;
        while ((q >> b) != 0)
            b++;
        const U128 R = (U128(1) << (W - 1 + b)) / q;
        image[m] = T(q), image[L + m] = T(w), image[2 * L + m] = shoup(w, q);
        image[3 * L + m] = T(R), image[4 * L + m] = T(b - 1); // a power of two: R = 2^W is stored as 0
        dargs.t_shoup[m] = shoup(t, q);
        const U64 ti = invmod(t, q);
        sargs.t_inv[m] = T(ti), sargs.t_inv_shoup[m] = shoup(ti, q);
        q_mod_t = mulmod(q_mod_t, q % t, t);
    }
    dargs.t = sargs.t = T(t), dargs.one_shoup_t = sargs.one_shoup_t = shoup(1, t);
    sargs.q_mod_t = T(q_mod_t), sargs.q_mod_t_shoup = shoup(q_mod_t, t), sargs.half = T(t / 2);
    kern::BcOffsets up{};
    up.q = 0, up.w = unsigned(L), up.wp = unsigned(2 * L), up.recip = unsigned(3 * L), up.shift = unsigned(4 * L);

    size_t bad = 0;
    auto write = [&](Guarded<T>& gd, size_t words) {
        bad += gd.touched();
        for (size_t i = 0; i < words; i++)
        {
            const U64 w = gd.data()[i];
            std::fwrite(&w, sizeof(w), 1, res);
        }
    };

    // decrypt_phase, launched as decrypt_phase_launch launches it: 2 and 3 components, then in place
    bool pvec = false;
    for (int pass = 0; pass < 3; pass++)
    {
        const int components = pass == 0 ? 2 : 3;
        Guarded<T> fresh(stack, off);
        T* out = pass == 2 ? ct.data() : fresh.data();
        pvec = host::relin_wide<T>(n, {ct.data(), s.data(), out});
        const host::RelinGrid g = host::relin_grid(n, pvec ? VW : 1, U64(count));
        const dim3 grid(g.blocks, L);
        if (pvec)
            launch(grid, g.nt, [&] {
                kern::decrypt_phase<T, VW>(ct.data(), s.data(), out, fold.data(), count, components, L, M, n, g.tiles);
            });
        else
            launch(grid, g.nt, [&] {
                kern::decrypt_phase<T, 1>(ct.data(), s.data(), out, fold.data(), count, components, L, M, n, g.tiles);
            });
        if (pass == 2)
        {
            write(ct, stack);
            for (size_t i = stack; i < 3 * stack; i++) // the other components are as they were
                bad += ct.data()[i] != ct0[i];
        }
        else
        {
            write(fresh, stack);
            for (size_t i = 0; i < 3 * stack; i++)
                bad += ct.data()[i] != ct0[i];
        }
    }

    // encrypt_public_combine with the message and without
    bool cvec = false;
    for (const T* mp : {static_cast<const T*>(msg.data()), static_cast<const T*>(nullptr)})
    {
        Guarded<T> out(2 * stack, off);
        cvec = host::relin_wide<T>(n, {pk.data(), lifted.data(), mp, out.data()});
        const host::RelinGrid g = host::relin_grid(n, cvec ? VW : 1, U64(count));
        const dim3 grid(g.blocks, L);
        if (cvec)
            launch(grid, g.nt, [&] {
                kern::encrypt_public_combine<T, VW>(pk.data(), lifted.data(), mp, out.data(), fold.data(), count, L, M, n,
                                                    g.tiles);
            });
        else
            launch(grid, g.nt, [&] {
                kern::encrypt_public_combine<T, 1>(pk.data(), lifted.data(), mp, out.data(), fold.data(), count, L, M, n,
                                                   g.tiles);
            });
        write(out, 2 * stack);
        for (size_t i = 0; i < 3 * stack; i++)
            bad += lifted.data()[i] != lifted0[i];
    }

    // bfv_scale_message
    bool svec;
    {
        Guarded<T> out(stack, off);
        svec = host::relin_wide<T>(n, {message.data(), out.data()});
        const host::RelinGrid g = host::relin_grid(n, svec ? VW : 1, U64(count));
        if (svec)
            launch(dim3(g.blocks), g.nt, [&] {
                kern::bfv_scale_message<T, VW>(message.data(), out.data(), fold.data(), sargs, L, n, g.tiles);
            });
        else
            launch(dim3(g.blocks), g.nt, [&] {
                kern::bfv_scale_message<T, 1>(message.data(), out.data(), fold.data(), sargs, L, n, g.tiles);
            });
        write(out, stack);
    }

    // bfv_decode with noise_max (zeroed, as the memset leaves it), with the partial maxima and bfv_decode_merge
    // (noise_max NOT zeroed: no memset precedes that form), and without noise_max
    bool dvec = false;
    for (int mode : {1, 2, 0})
    {
        const bool with_noise = mode != 0;
        Guarded<T> out(size_t(count) * N, off), worst(size_t(count), 0);
        Guarded<T> part(host::decode_partial_words(count, n), off);
        std::fill(worst.data(), worst.data() + count, mode == 2 ? T(0x77) : T(0));
        T* np = with_noise ? worst.data() : nullptr;
        T* pp = mode == 2 ? part.data() : nullptr;
        dvec = host::relin_wide<T>(n, {x.data(), out.data()});
        const host::RelinGrid g = host::relin_grid(n, dvec ? VW : 1, U64(count));
        if (dvec)
            launch(dim3(g.blocks), g.nt,
                   [&] { kern::bfv_decode<T, VW>(x.data(), out.data(), np, pp, image.data(), up, dargs, L, n, g.tiles); });
        else
            launch(dim3(g.blocks), g.nt,
                   [&] { kern::bfv_decode<T, 1>(x.data(), out.data(), np, pp, image.data(), up, dargs, L, n, g.tiles); });
        if (mode == 2)
            launch(dim3(unsigned(count)), kern::DEC_WAVE,
                   [&] { kern::bfv_decode_merge<T>(part.data(), worst.data(), g.tiles); });
        bad += part.touched();
        write(out, size_t(count) * N);
        if (with_noise)
            write(worst, size_t(count));
        else
            for (int i = 0; i < count; i++) // without noise_max nothing is written there
                bad += worst.data()[i] != T(0);
        bad += worst.touched();
    }
    bad += ct.touched() + s.touched() + pk.touched() + lifted.touched() + msg.touched() + message.touched() + x.touched();
    std::printf("W=%d n=%d L=%d count=%d off=%d t=%llu vec=%d%d%d%d: %s (%zu)\n", W, n, L, count, off, t, pvec, cvec, svec,
                dvec, bad ? "GUARD TOUCHED" : "ok", bad);
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
        const int W = int(next()), n = int(next()), L = int(next()), count = int(next()), off = int(next());
        const U64 t = next();
        bad += W == 64 ? run_case<Data64>(n, L, count, off, t, res) : run_case<Data32>(n, L, count, off, t, res);
    }
    std::fclose(res);
    std::printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad != 0;
}
