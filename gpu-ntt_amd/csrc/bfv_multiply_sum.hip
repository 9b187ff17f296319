// bfv_multiply_sum.hip -- the kernel of BfvMultiplyPlan<T>::multiply_sum and multiply_relinearize_sum
// (include/gpuntt/rns/bfv_multiply.cuh): the tensor of `terms` pairs of extended ciphertexts, summed before anything is
// divided by Q ("lazy relinearization" for the scale-invariant product).
//
//   bfv_tensor_sum:  d0 = sum_t x0_t y0_t,  d1 = sum_t (x0_t y1_t + x1_t y0_t),  d2 = sum_t x1_t y1_t
//                    modulo every modulus of the full base
//
// It is bfv_tensor (bfv_multiply.hip) with tensor_top_sum's run-time loop over t (relinearize_sum.hip): the same grid, the
// same two loaders, the same arithmetic -- IpAcc::mac and IpFold of inner_product_internal.hpp, the ONE copy of it.  The
// carry bound is the one relinearize_sum.hip's header states: a mac carries at most once, so `terms` macs (d0, d2) and
// 2 * terms macs (d1), at most 64, stay far inside the 32-bit carry count; each sum is folded once.
//
// Operands.  The host has extended and transformed every DISTINCT operand once, into slot s of one region
// e = T[slots][2][count][M][N]; a term names its two slots by one byte each (BfvSumArgs, inside the kernel argument, read
// at the wave-uniform t).  A term whose two slots are equal is a squaring: its two extra loads are skipped, a wave-uniform
// branch.  The term loop is not unrolled: the accumulators are live across it and one term's four loads are what is in
// flight (an unroll by two was timed: DESIGN.md 3.21).
//
// Output, in place.  d0, d1, d2 go over planes (slot 0, c 0), (slot 0, c 1), (slot 1, c 0) of e: contiguous, the
// T[3][count][M][N] of the one inverse transform that follows.  INVARIANT: every access of a lane -- each load of every
// term and the three stores -- is at the lane's own offset `at` = (r, m, its columns) inside a plane, distinct lanes have
// distinct `at`, and the stores follow the lane's last load.  So a lane writes only offsets that no other lane ever reads,
// and a slot that appears in every term -- slot 0 and slot 1 included, read in the last term -- is safe to overwrite.
// e is therefore NOT __restrict__.
//
// A lane owns a 16-byte group (V = 16 / sizeof(T) columns), V = 1 for the whole launch when e is not 16-byte aligned or N
// is below a group; constants through IpFold; 64-bit indices.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "bfv_multiply_sum_internal.hpp"
#include "inner_product_internal.hpp"
#include "launch.hpp"

namespace gpuntt
{
    namespace kern
    {
        // grid: x = r * tiles + tile, y = m < M; e: T[slots][2][count][M][N], d = T[3][count][M][N] over its start; fold:
        // the six arrays of M words IpFold reads
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void bfv_tensor_sum(T* e, const T* __restrict__ fold_consts, BfvSumArgs sa,
                                                                int count, int M, int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, r = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long at =
                ((static_cast<unsigned long long>(r) * static_cast<unsigned>(M) + m) << n_power) + col;
            const unsigned long long comp = (static_cast<unsigned long long>(count) * static_cast<unsigned>(M)) << n_power;
            IpAcc<T> s0[V], s1[V], s2[V];
#pragma unroll
            for (int v = 0; v < V; v++)
                s0[v] = s1[v] = s2[v] = IpAcc<T>{T(0), T(0), 0u};
#pragma unroll 1
            for (int t = 0; t < sa.terms; t++)
            {
                const unsigned xs = sa.x_slot[t], ys = sa.y_slot[t]; // uniform over the grid
                const T* x = e + 2ull * xs * comp + at;
                const Vec x0 = *reinterpret_cast<const Vec*>(x);
                const Vec x1 = *reinterpret_cast<const Vec*>(x + comp);
                Vec y0 = x0, y1 = x1;
                if (ys != xs)
                {
                    const T* y = e + 2ull * ys * comp + at;
                    y0 = *reinterpret_cast<const Vec*>(y);
                    y1 = *reinterpret_cast<const Vec*>(y + comp);
                }
#pragma unroll
                for (int v = 0; v < V; v++)
                {
                    s0[v].mac(x0.x[v], y0.x[v]);
                    s1[v].mac(x0.x[v], y1.x[v]);
                    s1[v].mac(x1.x[v], y0.x[v]);
                    s2[v].mac(x1.x[v], y1.x[v]);
                }
            }
            const IpFold<T> fold(fold_consts, M, m);
            Vec o0, o1, o2;
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                o0.x[v] = fold.reduce(fold.sum(s0[v])); // each sum is below 3 q < 2^W
                o1.x[v] = fold.reduce(fold.sum(s1[v]));
                o2.x[v] = fold.reduce(fold.sum(s2[v]));
            }
            *reinterpret_cast<Vec*>(e + at) = o0;
            *reinterpret_cast<Vec*>(e + comp + at) = o1;
            *reinterpret_cast<Vec*>(e + 2 * comp + at) = o2;
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            template <typename T, int V>
            void bfv_tensor_sum_as(T* e, const T* fold, const kern::BfvSumArgs& args, int count, int M, int n_power,
                                   bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(count));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::bfv_tensor_sum<T, V>), dim3(g.blocks, static_cast<unsigned>(M)), dim3(g.nt), 0,
                              stream, e, fold, args, count, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }
        } // namespace

        template <typename T>
        void bfv_tensor_sum_launch(T* e, const T* fold, const kern::BfvSumArgs& args, int count, int M, int n_power,
                                   bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {e}))
                bfv_tensor_sum_as<T, VW>(e, fold, args, count, M, n_power, enqueue, stream);
            else
                bfv_tensor_sum_as<T, 1>(e, fold, args, count, M, n_power, enqueue, stream);
        }

        template void bfv_tensor_sum_launch<Data32>(Data32*, const Data32*, const kern::BfvSumArgs&, int, int, int, bool,
                                                    hipStream_t);
        template void bfv_tensor_sum_launch<Data64>(Data64*, const Data64*, const kern::BfvSumArgs&, int, int, int, bool,
                                                    hipStream_t);
    } // namespace host
} // namespace gpuntt
