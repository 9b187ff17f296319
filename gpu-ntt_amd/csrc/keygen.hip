// keygen.hip -- the kernels of KeySwitchPlan<T>::lift_small, ::generate_keys and ::encrypt_symmetric
// (include/gpuntt/rns/key_switch.cuh, "Key material").
//
//   lift_small:      out[p][m][j] = small[p][j] mod q_m, canonical, m < B          -- int32 -> the RNS base
//   keygen_combine:  key[g][d][0][m][j] = ( E[g][d][m][j] - a[g][d][m][j] * s[m][j]
//                                           + [m in S_d] (P mod q_m) * s_from[g][m][j] ) mod q_m
//                    and, with other strides and multiplier 1, the first component of a symmetric encryption
//
// lift_small: a lane owns a 16-byte group of columns of one polynomial, reads its V signed values ONCE and walks the B
// limbs with them; |v| <= 2^31 is one word, rns_shoup(|v|, 1) is its canonical residue for any word, and a negative
// value takes q - r (0 stays 0).  The moduli come through the constant address space: scalar loads.
//
// keygen_combine: blockIdx.y is the limb, blockIdx.x = (g * rows + d) * tiles + tile, so limb, key and digit are
// workgroup-uniform: whether the gadget term is present is a scalar branch and the workgroups outside digit d load
// nothing of s_from.  The keys arrive through an argument table (KeygenArgs), as rotate_hoisted takes its keys.  Every
// word of E, a and s_from is read once; s (one stack, re-read by every key and digit) comes from the cache.  Arithmetic:
// the exact three-word accumulator of inner_product_internal.hpp seeded with E, ONE mac with (q - (a mod q)) * s -- a is
// made canonical by one Shoup product, s may be any word -- one mac with the gadget term, ONE fold: three terms, no new
// bound.
//
// Plaintext operands (KeySwitchPlan<T>::lift_centred and ::multiply_plain):
//   lift_centred:    out[p][m][j] = v mod q_m, v = w - t if w >= (t + 1) >> 1 else w, w = words[p][j] mod t
//   multiply_plain:  out[c][r][m][j] = (ct[c][r][m][j] * pt[r or 0][m][j]) mod q_m, c < 2
// lift_centred is lift_small with another head: the word is made canonical modulo t by one Shoup product by 1 (t and
// floor(2^W / t) are kernel arguments), centred, and sign and magnitude walk the limbs as there.  multiply_plain has
// decrypt_phase's grid (decrypt.hip); one mac into an empty accumulator and one fold per word -- the inner product's
// arithmetic with one term --, the plaintext word read once for both components; out may be ct, each word being
// written by the lane that read it.
//
// All kernels: V = 16 / sizeof(T) columns per lane, V = 1 for a base pointer that is not 16-byte aligned or N below a
// group; 64-bit indices.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "inner_product_internal.hpp"
#include "keygen_internal.hpp"
#include "launch.hpp"

namespace gpuntt
{
    namespace kern
    {
        // grid: x = p * tiles + tile; small: int32[polys][N], out: T[polys][B][N]; consts: the fold image (stride M)
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void lift_small(const std::int32_t* __restrict__ small, T* __restrict__ out,
                                                            const T* __restrict__ consts, int B, int M, int n_power,
                                                            unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            using CP = const T __attribute__((address_space(4)))*;
            const unsigned tile = blockIdx.x % tiles, p = blockIdx.x / tiles;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const IpVec<std::int32_t, V> sv =
                *reinterpret_cast<const IpVec<std::int32_t, V>*>(small + (static_cast<unsigned long long>(p) << n_power) + col);
            T mag[V];
            bool neg[V];
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                const long long x = sv.x[v]; // widened first: -INT32_MIN does not fit an int
                neg[v] = x < 0, mag[v] = static_cast<T>(x < 0 ? -x : x);
            }
            const CP k = (CP) (consts);
            T* po = out + ((static_cast<unsigned long long>(p) * static_cast<unsigned>(B)) << n_power) + col;
            for (int m = 0; m < B; m++)
            {
                const T q = k[m], onep = k[5 * M + m];
                Vec o;
#pragma unroll
                for (int v = 0; v < V; v++)
                {
                    const T r = rns_shoup<T>(mag[v], T(1), onep, q);
                    o.x[v] = neg[v] && r != 0 ? q - r : r;
                }
                *reinterpret_cast<Vec*>(po + (static_cast<unsigned long long>(m) << n_power)) = o;
            }
        }

        // grid: x = p * tiles + tile; words: T[polys][N], out: T[polys][B][N]; consts: the fold image (stride M);
        // t, one_shoup_t = floor(2^W / t), half_up = (t + 1) >> 1: the plaintext modulus, as kernel arguments
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void lift_centred(const T* __restrict__ words, T* __restrict__ out,
                                                              const T* __restrict__ consts, T t, T one_shoup_t,
                                                              T half_up, int B, int M, int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            using CP = const T __attribute__((address_space(4)))*;
            const unsigned tile = blockIdx.x % tiles, p = blockIdx.x / tiles;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const Vec wv = *reinterpret_cast<const Vec*>(words + (static_cast<unsigned long long>(p) << n_power) + col);
            T mag[V];
            bool neg[V];
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                const T m = rns_shoup<T>(wv.x[v], T(1), one_shoup_t, t); // the word modulo t
                neg[v] = m >= half_up, mag[v] = neg[v] ? t - m : m;       // |v| <= t / 2
            }
            const CP k = (CP) (consts);
            T* po = out + ((static_cast<unsigned long long>(p) * static_cast<unsigned>(B)) << n_power) + col;
            for (int m = 0; m < B; m++)
            {
                const T q = k[m], onep = k[5 * M + m];
                Vec o;
#pragma unroll
                for (int v = 0; v < V; v++)
                {
                    const T r = rns_shoup<T>(mag[v], T(1), onep, q); // t may pass q: any word enters
                    o.x[v] = neg[v] && r != 0 ? q - r : r;
                }
                *reinterpret_cast<Vec*>(po + (static_cast<unsigned long long>(m) << n_power)) = o;
            }
        }

        // grid: x = r * tiles + tile, y = m < L; ct: T[2][count][L][N], pt: T[plain_count][L][N] (pt_stack = L N words,
        // or 0 for a shared plaintext), out: T[2][count][L][N] (out may be ct: neither is __restrict__); consts: the fold
        // image (stride M).  Both components from one read of the plaintext word
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void multiply_plain(const T* ct, const T* __restrict__ pt, T* out,
                                                                const T* __restrict__ consts,
                                                                unsigned long long pt_stack, int count, int L, int M,
                                                                int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, r = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long limb = (static_cast<unsigned long long>(m) << n_power) + col;
            const unsigned long long at = ((static_cast<unsigned long long>(r) * static_cast<unsigned>(L)) << n_power) + limb;
            const unsigned long long comp =
                (static_cast<unsigned long long>(count) * static_cast<unsigned>(L)) << n_power;

            const Vec c0 = *reinterpret_cast<const Vec*>(ct + at);
            const Vec c1 = *reinterpret_cast<const Vec*>(ct + comp + at);
            const Vec pv = *reinterpret_cast<const Vec*>(pt + r * pt_stack + limb);

            const IpFold<T> fold(consts, M, m);
            Vec o0, o1;
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                IpAcc<T> a0{T(0), T(0), 0u}, a1{T(0), T(0), 0u};
                a0.mac(c0.x[v], pv.x[v]);
                a1.mac(c1.x[v], pv.x[v]);
                o0.x[v] = fold.reduce(fold.sum(a0)); // the sums are below 3 q < 2^W
                o1.x[v] = fold.reduce(fold.sum(a1));
            }
            *reinterpret_cast<Vec*>(out + at) = o0;
            *reinterpret_cast<Vec*>(out + comp + at) = o1;
        }

        // grid: x = (g * rows + d) * tiles + tile, y = m < B; the layouts: KeygenShape (keygen_internal.hpp)
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void keygen_combine(const T* __restrict__ e, const T* __restrict__ s,
                                                                const T* __restrict__ gadget, KeygenArgs<T> args,
                                                                KeygenShape sh, const T* __restrict__ consts, int M,
                                                                int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, grow = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned g = grow / static_cast<unsigned>(sh.rows), d = grow % static_cast<unsigned>(sh.rows);
            const unsigned long long limb = (static_cast<unsigned long long>(m) << n_power) + col;
            T* base = args.group[g] + d * sh.row + limb;
            const int lo = static_cast<int>(d) * sh.alpha, hi = ip_min(lo + sh.alpha, sh.L);
            const bool on =
                gadget != nullptr && (sh.alpha == 0 || (static_cast<int>(m) >= lo && static_cast<int>(m) < hi));

            const Vec ev = *reinterpret_cast<const Vec*>(
                e + ((static_cast<unsigned long long>(grow) * static_cast<unsigned>(sh.B) + m) << n_power) + col);
            const Vec av = *reinterpret_cast<const Vec*>(base + sh.a_at);
            const Vec sv = *reinterpret_cast<const Vec*>(s + limb);
            Vec gv{};
            if (on)
                gv = *reinterpret_cast<const Vec*>(gadget + g * sh.g_group + d * sh.g_row + limb);

            const IpFold<T> fold(consts, M, m);
            const T mult = args.mult[m];
            Vec o;
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                const T na = fold.q - rns_shoup<T>(av.x[v], T(1), fold.onep, fold.q); // -a mod q, in [1, q]
                IpAcc<T> acc{ev.x[v], T(0), 0u};
                acc.mac(na, sv.x[v]);
                if (on)
                    acc.mac(mult, gv.x[v]);
                o.x[v] = fold.reduce(fold.sum(acc)); // the sum is below 3 q < 2^W
            }
            *reinterpret_cast<Vec*>(base) = o;
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            template <typename T, int V>
            void lift_as(const std::int32_t* small, T* out, const T* consts, int polys, int B, int M, int n_power,
                         bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(polys));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::lift_small<T, V>), dim3(g.blocks), dim3(g.nt), 0, stream, small, out, consts, B, M,
                              n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V>
            void centred_as(const T* words, T* out, const T* consts, T t, int polys, int B, int M, int n_power,
                            bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(polys));
                if (!enqueue)
                    return;
                const T one_shoup_t = static_cast<T>((static_cast<unsigned __int128>(1) << (8 * sizeof(T))) / t);
                GPUNTT_LAUNCH((kern::lift_centred<T, V>), dim3(g.blocks), dim3(g.nt), 0, stream, words, out, consts, t,
                              one_shoup_t, static_cast<T>((t + 1) >> 1), B, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V>
            void plain_as(const T* ct, const T* pt, T* out, const T* consts, int count, int plain_count, int L, int M,
                          int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(count));
                if (!enqueue)
                    return;
                const unsigned long long pt_stack = plain_count == 1 ? 0ull : static_cast<unsigned long long>(L) << n_power;
                GPUNTT_LAUNCH((kern::multiply_plain<T, V>), dim3(g.blocks, static_cast<unsigned>(L)), dim3(g.nt), 0,
                              stream, ct, pt, out, consts, pt_stack, count, L, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V>
            void combine_as(const T* e, const T* s, const T* gadget, const kern::KeygenArgs<T>& args,
                            const kern::KeygenShape& shape, int groups, const T* consts, int M, int n_power, bool enqueue,
                            hipStream_t stream)
            {
                const RelinGrid g = relin_grid(
                    n_power, V, static_cast<unsigned long long>(groups) * static_cast<unsigned>(shape.rows));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::keygen_combine<T, V>), dim3(g.blocks, static_cast<unsigned>(shape.B)), dim3(g.nt), 0,
                              stream, e, s, gadget, args, shape, consts, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }
        } // namespace

        template <typename T>
        void keygen_lift_launch(const std::int32_t* small, T* out, const T* consts, int polys, int B, int M, int n_power,
                                bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {small, out}))
                lift_as<T, VW>(small, out, consts, polys, B, M, n_power, enqueue, stream);
            else
                lift_as<T, 1>(small, out, consts, polys, B, M, n_power, enqueue, stream);
        }

        template <typename T>
        void lift_centred_launch(const T* words, T* out, const T* consts, T t, int polys, int B, int M, int n_power,
                                 bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {words, out}))
                centred_as<T, VW>(words, out, consts, t, polys, B, M, n_power, enqueue, stream);
            else
                centred_as<T, 1>(words, out, consts, t, polys, B, M, n_power, enqueue, stream);
        }

        template <typename T>
        void multiply_plain_launch(const T* ct, const T* pt, T* out, const T* consts, int count, int plain_count, int L,
                                   int M, int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {ct, pt, out}))
                plain_as<T, VW>(ct, pt, out, consts, count, plain_count, L, M, n_power, enqueue, stream);
            else
                plain_as<T, 1>(ct, pt, out, consts, count, plain_count, L, M, n_power, enqueue, stream);
        }

        template <typename T>
        void keygen_combine_launch(const T* e, const T* s, const T* gadget, const kern::KeygenArgs<T>& args,
                                   const kern::KeygenShape& shape, int groups, const T* consts, int M, int n_power,
                                   bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            uintptr_t bits = reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(s) |
                             reinterpret_cast<uintptr_t>(gadget);
            for (int g = 0; g < groups; g++)
                bits |= reinterpret_cast<uintptr_t>(args.group[g]);
            if (relin_wide_bits<T>(n_power, bits))
                combine_as<T, VW>(e, s, gadget, args, shape, groups, consts, M, n_power, enqueue, stream);
            else
                combine_as<T, 1>(e, s, gadget, args, shape, groups, consts, M, n_power, enqueue, stream);
        }

        template void keygen_lift_launch<Data32>(const std::int32_t*, Data32*, const Data32*, int, int, int, int, bool,
                                                 hipStream_t);
        template void keygen_lift_launch<Data64>(const std::int32_t*, Data64*, const Data64*, int, int, int, int, bool,
                                                 hipStream_t);
        template void lift_centred_launch<Data32>(const Data32*, Data32*, const Data32*, Data32, int, int, int, int, bool,
                                                  hipStream_t);
        template void lift_centred_launch<Data64>(const Data64*, Data64*, const Data64*, Data64, int, int, int, int, bool,
                                                  hipStream_t);
        template void multiply_plain_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*, int, int, int,
                                                    int, int, bool, hipStream_t);
        template void multiply_plain_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*, int, int, int,
                                                    int, int, bool, hipStream_t);
        template void keygen_combine_launch<Data32>(const Data32*, const Data32*, const Data32*,
                                                    const kern::KeygenArgs<Data32>&, const kern::KeygenShape&, int,
                                                    const Data32*, int, int, bool, hipStream_t);
        template void keygen_combine_launch<Data64>(const Data64*, const Data64*, const Data64*,
                                                    const kern::KeygenArgs<Data64>&, const kern::KeygenShape&, int,
                                                    const Data64*, int, int, bool, hipStream_t);
    } // namespace host
} // namespace gpuntt
