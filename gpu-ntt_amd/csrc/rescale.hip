// rescale.hip -- the two kernels of KeySwitchPlan<T>::rescale with ntt_form = true (include/gpuntt/rns/key_switch.cuh):
// the division of an NTT-form ciphertext by its last R primes without inverse transforms of the limbs that stay.
//
//   rescale_gather:     dropped[s][i][col] = x[s][L - R + i][col] mod q_{L-R+i},  i < R      -- a strided copy that
//                       reduces: x holds any words, the inverse transform that follows is defined on residues
//   rescale_sub_scale:  out[s][j][col] = ((x[s][j][col] mod q_j) - out[s][j][col]) * Qinv_j mod q_j,  j < L' = L - R
//                       Qinv_j = (q_{L-R} ... q_{L-1})^-1 mod q_j;  out holds canonical residues on entry (the forward
//                       transform of the converted dropped limbs) and on exit
//
// Between the two the plan runs its own steps: the inverse transform of the R gathered limbs, the dense centred conversion
// into out and the forward transform of out over the L' kept moduli.
//
// Both kernels: grid x = stack * tiles + column tile, y = limb, so every constant is workgroup-uniform -- rescale_sub_scale
// reads its four through the constant address space, rescale_gather its two from a kernel argument: scalar loads either
// way; a lane owns a 16-byte group (V = 16 / sizeof(T) columns), V = 1 for a base
// pointer that is not 16-byte aligned or N below a group; 64-bit indices.  rescale_sub_scale per word: x is reduced with
// one Shoup product against the companion of 1 (a conditional subtraction does not reduce a 64-bit word modulo a 20-bit
// q), the difference is formed as a word congruent to it as base_convert forms c - conv, and the scaling is one Shoup
// product: rns_shoup of rns_arith.hpp, no copy of the arithmetic.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "inner_product_internal.hpp"
#include "launch.hpp"
#include "rescale_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // grid: x = s * tiles + tile, y = i < R; x: T[stacks][L][N], dropped: T[stacks][R][N]
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void rescale_gather(const T* __restrict__ x, T* __restrict__ dropped,
                                                                RsDropped<T> mods, int L, int R, int n_power,
                                                                unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, s = blockIdx.x / tiles;
            const unsigned i = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long from =
                ((static_cast<unsigned long long>(s) * static_cast<unsigned>(L) + static_cast<unsigned>(L - R) + i)
                 << n_power) + col;
            const unsigned long long to =
                ((static_cast<unsigned long long>(s) * static_cast<unsigned>(R) + i) << n_power) + col;
            const T q = mods.q[i], onep = mods.onep[i];
            Vec v = *reinterpret_cast<const Vec*>(x + from);
#pragma unroll
            for (int e = 0; e < V; e++)
                v.x[e] = rns_shoup<T>(v.x[e], T(1), onep, q);
            *reinterpret_cast<Vec*>(dropped + to) = v;
        }

        // grid: x = s * tiles + tile, y = j < keep; x: T[stacks][L][N], out: T[stacks][keep][N]
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void rescale_sub_scale(const T* __restrict__ x, T* __restrict__ out,
                                                                   const T* __restrict__ consts, RsOffsets off, int L,
                                                                   int keep, int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            using CP = const T __attribute__((address_space(4)))*;
            const unsigned tile = blockIdx.x % tiles, s = blockIdx.x / tiles;
            const unsigned j = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const CP k = (CP) (consts);
            const T q = k[off.q + j], onep = k[off.onep + j], w = k[off.qinv + j], wp = k[off.qinvp + j];
            const unsigned long long xat =
                ((static_cast<unsigned long long>(s) * static_cast<unsigned>(L) + j) << n_power) + col;
            const unsigned long long oat =
                ((static_cast<unsigned long long>(s) * static_cast<unsigned>(keep) + j) << n_power) + col;
            const Vec xv = *reinterpret_cast<const Vec*>(x + xat);
            Vec o = *reinterpret_cast<const Vec*>(out + oat);
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                const T c = rns_shoup<T>(xv.x[v], T(1), onep, q);
                const T r = o.x[v]; // canonical: what the forward transform wrote
                // c - r as a word that is congruent to it, below 2 q
                const T d = c >= r ? c - r : c + (q - r);
                o.x[v] = rns_shoup<T>(d, w, wp, q);
            }
            *reinterpret_cast<Vec*>(out + oat) = o;
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            template <typename T, int V>
            void rescale_gather_as(const T* x, T* dropped, const kern::RsDropped<T>& mods, int stacks, int L, int R,
                                   int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(stacks));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::rescale_gather<T, V>), dim3(g.blocks, static_cast<unsigned>(R)), dim3(g.nt), 0, stream,
                              x, dropped, mods, L, R, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V>
            void rescale_sub_scale_as(const T* x, T* out, const T* consts, const kern::RsOffsets& off, int stacks, int L,
                                      int keep, int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(stacks));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::rescale_sub_scale<T, V>), dim3(g.blocks, static_cast<unsigned>(keep)), dim3(g.nt), 0,
                              stream, x, out, consts, off, L, keep, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }
        } // namespace

        template <typename T>
        void rescale_gather_launch(const T* x, T* dropped, const kern::RsDropped<T>& mods, int stacks, int L, int R,
                                   int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {x, dropped}))
                rescale_gather_as<T, VW>(x, dropped, mods, stacks, L, R, n_power, enqueue, stream);
            else
                rescale_gather_as<T, 1>(x, dropped, mods, stacks, L, R, n_power, enqueue, stream);
        }

        template <typename T>
        void rescale_sub_scale_launch(const T* x, T* out, const T* consts, const kern::RsOffsets& off, int stacks, int L,
                                      int keep, int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {x, out}))
                rescale_sub_scale_as<T, VW>(x, out, consts, off, stacks, L, keep, n_power, enqueue, stream);
            else
                rescale_sub_scale_as<T, 1>(x, out, consts, off, stacks, L, keep, n_power, enqueue, stream);
        }

        template void rescale_gather_launch<Data32>(const Data32*, Data32*, const kern::RsDropped<Data32>&, int, int, int,
                                                    int, bool, hipStream_t);
        template void rescale_gather_launch<Data64>(const Data64*, Data64*, const kern::RsDropped<Data64>&, int, int, int,
                                                    int, bool, hipStream_t);
        template void rescale_sub_scale_launch<Data32>(const Data32*, Data32*, const Data32*, const kern::RsOffsets&, int,
                                                       int, int, int, bool, hipStream_t);
        template void rescale_sub_scale_launch<Data64>(const Data64*, Data64*, const Data64*, const kern::RsOffsets&, int,
                                                       int, int, int, bool, hipStream_t);
    } // namespace host
} // namespace gpuntt
