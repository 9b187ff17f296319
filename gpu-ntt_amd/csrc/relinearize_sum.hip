// relinearize_sum.hip -- the two kernels of KeySwitchPlan<T>::multiply_relinearize_sum (include/gpuntt/rns/key_switch.cuh):
// sum_t x_t * y_t over `terms` pairs of ciphertexts with ONE key switch and ONE ModDown ("lazy relinearization").  The key
// switch is linear in the top term, so the three tensor terms are summed over t first:
//
//   tensor_top_sum:            d2[r][m][j] = (sum_t x1_t[r][m][j] * y1_t[r][m][j]) mod q_m,  m < L    -- what is decomposed
//   inner_product_tensor_sum:  acc[c][r][m][j] = ( sum_{d<D} a[d][r][m][j] * key[d][c][limb(m)][j]
//                                                  + [m < L] (P mod q_m) * d_c[r][m][j] ) mod q_m,  c < 2
//                              d_0 = sum_t x0_t y0_t,  d_1 = sum_t (x0_t y1_t + x1_t y0_t)
//
// They are relinearize.hip's tensor_top and inner_product_tensor with a run-time loop over t: the same grids, the same
// loaders, the same arithmetic (IpAcc, IpFold, rns_shoup, ip_digit_loop of inner_product_internal.hpp -- no copy of any).
// The 2 * terms operand pointers travel inside the kernel argument (RelinSumArgs) and are read at the wave-uniform t.
//
// The seed (IpSeedTensorSum).  Per term x0' = rns_shoup(x0, P mod q_m) and x1' = rns_shoup(x1, P mod q_m), canonical for
// ANY word, then IpSeedTensor's three exact macs: x0' y0 into c = 0, x0' y1 and x1' y0 into c = 1.  The term loop is NOT
// unrolled: the accumulators are live across it, and one term's 4 * RB loads are what is in flight.  RB = 1 or 2.
//
// Bound.  The accumulator is exact up to its 32-bit carry count and a mac carries at most once: D digits (D <= 64) and at
// most 3 macs per term (terms <= 32) are D + 3 * terms <= 160 carries.  The fold's product with the carry word is an
// exact Shoup product for any word, so no new bound is needed.  tensor_top_sum: `terms` macs, one fold.
//
// Both kernels: a lane owns a 16-byte group (V = 16 / sizeof(T) columns), V = 1 for the whole launch when ANY base pointer
// (a, key, acc, d2, every x_t and y_t) is not 16-byte aligned or N is below a group; constants through the constant
// address space; 64-bit indices.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "inner_product_internal.hpp"
#include "launch.hpp"
#include "relinearize_sum_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // How inner_product_tensor_sum seeds its accumulators: (P mod q_m) d_0 and (P mod q_m) d_1 for m < L, summed over
        // the terms before any reduction; zero for the special limbs, which load nothing of x or y.  An input past the
        // end of the last block re-reads the block's last one, as the digit loop does
        template <typename T> struct IpSeedTensorSum
        {
            const RelinSumArgs<T>& sa;
            T q, pq, pqs; // q_m, P mod q_m and its Shoup companion
            int L, count, n_power;
            bool on; // m < L
            template <int RB, int C, int V>
            __device__ __forceinline__ void operator()(IpAcc<T> (&acc)[RB][C][V], const IpPlace& p, const T*) const
            {
                static_assert(C == 2, "a product of two ciphertexts has two components after the switch");
                using Vec = IpVec<T, V>;
#pragma unroll
                for (int r = 0; r < RB; r++)
#pragma unroll
                    for (int c = 0; c < C; c++)
#pragma unroll
                        for (int v = 0; v < V; v++)
                            acc[r][c][v] = IpAcc<T>{T(0), T(0), 0u};
                if (!on)
                    return;
                const unsigned long long in_stack = static_cast<unsigned long long>(L) << n_power; // one input's limbs
                const unsigned long long in_comp = static_cast<unsigned long long>(count) * in_stack;
                const unsigned long long first =
                    static_cast<unsigned long long>(p.r0) * in_stack + (static_cast<unsigned long long>(p.m) << n_power) +
                    p.col;
                unsigned long long at[RB];
#pragma unroll
                for (int r = 0; r < RB; r++)
                    at[r] = first + static_cast<unsigned long long>(ip_min(r, p.nr - 1)) * in_stack;
#pragma unroll 1
                for (int t = 0; t < sa.terms; t++)
                {
                    const T* x = sa.x[t];
                    const T* y = sa.y[t];
#pragma unroll
                    for (int r = 0; r < RB; r++)
                    {
                        const Vec x0 = *reinterpret_cast<const Vec*>(x + at[r]);
                        const Vec x1 = *reinterpret_cast<const Vec*>(x + in_comp + at[r]);
                        const Vec y0 = *reinterpret_cast<const Vec*>(y + at[r]);
                        const Vec y1 = *reinterpret_cast<const Vec*>(y + in_comp + at[r]);
#pragma unroll
                        for (int v = 0; v < V; v++)
                        {
                            const T s0 = rns_shoup<T>(x0.x[v], pq, pqs, q), s1 = rns_shoup<T>(x1.x[v], pq, pqs, q);
                            acc[r][0][v].mac(s0, y0.x[v]);
                            acc[r][1][v].mac(s0, y1.x[v]);
                            acc[r][1][v].mac(s1, y0.x[v]);
                        }
                    }
                }
            }
        };

        // grid: x = rblock * tiles + tile, y = m < M; the mapping of inner_product
        template <typename T, int V, int RB>
        __global__ __launch_bounds__(IP_NT) void inner_product_tensor_sum(const T* __restrict__ a,
                                                                          const T* __restrict__ key, T* __restrict__ acc,
                                                                          const T* __restrict__ consts,
                                                                          RelinSumArgs<T> sa, int D, int count, int L,
                                                                          int M, int KM, int n_power, unsigned tiles)
        {
            using CP = const T __attribute__((address_space(4)))*;
            const unsigned m = blockIdx.y;
            const bool on = m < static_cast<unsigned>(L);
            const IpSeedTensorSum<T> seed{sa, ((CP) (consts))[m], sa.r.p_mod_q[m], sa.r.p_mod_q_shoup[m], L, count,
                                          n_power, on};
            ip_digit_loop<T, V, 2, RB>(a, key, acc, consts, sa.r.limbs, D, count, M, KM, n_power, tiles, seed);
        }

        // grid: x = r * tiles + tile, y = m < L; d2: T[count][L][N]; the second components of x_t, y_t: T[2][count][L][N]
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void tensor_top_sum(T* __restrict__ d2, const T* __restrict__ consts,
                                                                RelinSumArgs<T> sa, int count, int L, int M, int n_power,
                                                                unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, r = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long at =
                ((static_cast<unsigned long long>(r) * static_cast<unsigned>(L) + m) << n_power) + col;
            const unsigned long long top = // the lane's word of the second component
                ((static_cast<unsigned long long>(count) * static_cast<unsigned>(L)) << n_power) + at;
            IpAcc<T> s[V];
#pragma unroll
            for (int v = 0; v < V; v++)
                s[v] = IpAcc<T>{T(0), T(0), 0u};
#pragma unroll 1
            for (int t = 0; t < sa.terms; t++)
            {
                const Vec xv = *reinterpret_cast<const Vec*>(sa.x[t] + top);
                const Vec yv = *reinterpret_cast<const Vec*>(sa.y[t] + top);
#pragma unroll
                for (int v = 0; v < V; v++)
                    s[v].mac(xv.x[v], yv.x[v]);
            }
            const IpFold<T> fold(consts, M, m);
            Vec o;
#pragma unroll
            for (int v = 0; v < V; v++)
                o.x[v] = fold.reduce(fold.sum(s[v])); // the sum is below 3 q < 2^W
            *reinterpret_cast<Vec*>(d2 + at) = o;
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            // V = 1 for the whole launch when any base pointer is off 16 bytes
            template <typename T>
            bool relin_sum_wide(int n_power, const kern::RelinSumArgs<T>& args, std::initializer_list<const void*> bases)
            {
                uintptr_t bits = 0;
                for (const void* p : bases)
                    bits |= reinterpret_cast<uintptr_t>(p);
                for (int t = 0; t < args.terms; t++)
                    bits |= reinterpret_cast<uintptr_t>(args.x[t]) | reinterpret_cast<uintptr_t>(args.y[t]);
                return relin_wide_bits<T>(n_power, bits);
            }

            template <typename T, int V>
            void relin_sum_top_as(T* d2, const T* consts, const kern::RelinSumArgs<T>& args, int count, int L, int M,
                                  int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(count));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::tensor_top_sum<T, V>), dim3(g.blocks, static_cast<unsigned>(L)), dim3(g.nt), 0,
                              stream, d2, consts, args, count, L, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V, int RB>
            void relin_sum_inner_as(const T* a, const T* key, T* acc, const T* consts,
                                    const kern::RelinSumArgs<T>& args, int D, int count, int L, int M, int KM,
                                    int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, (static_cast<unsigned long long>(count) + RB - 1) / RB);
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::inner_product_tensor_sum<T, V, RB>), dim3(g.blocks, static_cast<unsigned>(M)),
                              dim3(g.nt), 0, stream, a, key, acc, consts, args, D, count, L, M, KM, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            // a block of RELIN_SUM_BLOCK = 2 inputs where count has them, one input per lane for count = 1
            template <typename T, int V>
            void relin_sum_inner_v(const T* a, const T* key, T* acc, const T* consts, const kern::RelinSumArgs<T>& args,
                                   int D, int count, int L, int M, int KM, int n_power, bool enqueue, hipStream_t stream)
            {
                constexpr int RB = kern::RELIN_SUM_BLOCK;
                if (count >= RB)
                    relin_sum_inner_as<T, V, RB>(a, key, acc, consts, args, D, count, L, M, KM, n_power, enqueue, stream);
                else
                    relin_sum_inner_as<T, V, 1>(a, key, acc, consts, args, D, count, L, M, KM, n_power, enqueue, stream);
            }
        } // namespace

        template <typename T>
        void relin_sum_top_launch(T* d2, const T* consts, const kern::RelinSumArgs<T>& args, int count, int L, int M,
                                  int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_sum_wide<T>(n_power, args, {d2}))
                relin_sum_top_as<T, VW>(d2, consts, args, count, L, M, n_power, enqueue, stream);
            else
                relin_sum_top_as<T, 1>(d2, consts, args, count, L, M, n_power, enqueue, stream);
        }

        template <typename T>
        void relin_sum_inner_launch(const T* a, const T* key, T* acc, const T* consts, const kern::RelinSumArgs<T>& args,
                                    int D, int count, int L, int M, int KM, int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_sum_wide<T>(n_power, args, {a, key, acc}))
                relin_sum_inner_v<T, VW>(a, key, acc, consts, args, D, count, L, M, KM, n_power, enqueue, stream);
            else
                relin_sum_inner_v<T, 1>(a, key, acc, consts, args, D, count, L, M, KM, n_power, enqueue, stream);
        }

        template void relin_sum_top_launch<Data32>(Data32*, const Data32*, const kern::RelinSumArgs<Data32>&, int, int, int,
                                                   int, bool, hipStream_t);
        template void relin_sum_top_launch<Data64>(Data64*, const Data64*, const kern::RelinSumArgs<Data64>&, int, int, int,
                                                   int, bool, hipStream_t);
        template void relin_sum_inner_launch<Data32>(const Data32*, const Data32*, Data32*, const Data32*,
                                                     const kern::RelinSumArgs<Data32>&, int, int, int, int, int, int, bool,
                                                     hipStream_t);
        template void relin_sum_inner_launch<Data64>(const Data64*, const Data64*, Data64*, const Data64*,
                                                     const kern::RelinSumArgs<Data64>&, int, int, int, int, int, int, bool,
                                                     hipStream_t);
    } // namespace host
} // namespace gpuntt
