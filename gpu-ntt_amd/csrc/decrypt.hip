// decrypt.hip -- the kernels of KeySwitchPlan<T>::phase and ::encrypt_public (include/gpuntt/rns/key_switch.cuh,
// "Decryption and public-key encryption") and of BfvMultiplyPlan<T>::scale_message and ::decode
// (include/gpuntt/rns/bfv_multiply.cuh); DESIGN.md 3.23.
//
//   decrypt_phase:           out[r][m][j] = (c0 + c1 s[m][j] + c2 s[m][j]^2) mod q_m
//   encrypt_public_combine:  out[0][r][m][j] = (pk0[m][j] U[r][m][j] + E0[r][m][j] + message[r][m][j]) mod q_m
//                            out[1][r][m][j] = (pk1[m][j] U[r][m][j] + E1[r][m][j]) mod q_m
//   bfv_scale_message:       out[c][i][j] = floor((Q m + h) / t) mod q_i, m = message[c][j] mod t, h = floor(t / 2)
//   bfv_decode:              message[s][j] = round(t x / Q) mod t from the L residues of x, and max_j |noise word|
//
// decrypt_phase and encrypt_public_combine have keygen_combine's grid (keygen.hip): blockIdx.y is the limb, blockIdx.x =
// r * tiles + tile, so every constant is workgroup-uniform; a lane owns a 16-byte group of columns (V = 1 for a base
// pointer off 16-byte alignment or N below a group).  Arithmetic: the exact three-word accumulator of
// inner_product_internal.hpp seeded with the additive term, one mac per product, ONE fold per output word.  s^2 never
// reaches memory: s is made canonical by one Shoup product, its square is a two-word product whose carry word is zero,
// and the two products of the fold that remain give a word below 2 q congruent to s^2 -- any word may enter a mac.
// decrypt_phase may write out over component 0 of ct: every word is written by the lane that read it, after its loads.
//
// bfv_scale_message and bfv_decode: a lane owns V columns of one stack, blockIdx.x = stack * tiles + tile, and walks the
// L limbs; the moduli and the per-limb constants are read at wave-uniform indices through the constant address space
// (the plan's images) or from the kernel argument (the constants of t: decrypt_internal.hpp) -- scalar loads.
//   scale: Q m vanishes modulo q_i, so floor((Q m + h) / t) = (Q m + h - r) / t is ((h - r) t^-1) mod q_i with
//   r = ((Q mod t) m + h) mod t: two Shoup products modulo t per column, one modulo q_i per word.
//   decode: per limb y = x * qhat_i^-1 mod q_i, (a, r) = divmod(t y, q_i) by one Shoup quotient against
//   floor(t 2^W / q_i) with its correction (t < q_i, so a < t), z = bc_z(r): the conversion unit's term.  The sum of the a
//   is kept modulo t, the sum of the z in a 2W-bit word from 2^(W-1): its high word joins the message, its low word with
//   the top bit flipped is the signed noise word.  The per-stack maximum of |noise| is reduced inside every wave by
//   lane exchanges (dec_wave_max: no barrier; lanes past the ring take part with 0), one word per wave goes to LDS,
//   ONE barrier, and lane 0 merges the workgroup's maximum with ONE vector atomicMax -- only when noise_max is given;
//   without it the kernel has no barrier and no atomic.  With a partials buffer lane 0 stores the workgroup's maximum
//   at partials[stack][tile] instead, and bfv_decode_merge -- one wave per stack -- takes the maximum over the tiles and
//   stores noise_max[stack]: two launches, no memset, no atomic.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "decrypt_internal.hpp"
#include "launch.hpp"

namespace gpuntt
{
    namespace kern
    {
        // bfv_decode's reduction: one word per wave
        extern __shared__ __align__(16) unsigned char dec_smem[];
        constexpr unsigned DEC_WAVE = 64; // lanes per wave on gfx950; every workgroup of relin_grid is whole waves

        // the maximum over the lanes of a wave, in every lane: six exchanges, no barrier.  (The host emulator of
        // tests/cpp supplies its own, over its threads: this is the one device primitive of the unit beside the atomic)
        __device__ __forceinline__ Data32 dec_wave_max(Data32 v)
        {
            for (int off = DEC_WAVE / 2; off > 0; off /= 2)
            {
                const Data32 o = __shfl_xor(v, off, DEC_WAVE);
                v = o > v ? o : v;
            }
            return v;
        }
        __device__ __forceinline__ Data64 dec_wave_max(Data64 v)
        {
            for (int off = DEC_WAVE / 2; off > 0; off /= 2)
            {
                const unsigned long long o = __shfl_xor(static_cast<unsigned long long>(v), off, DEC_WAVE);
                v = o > v ? static_cast<Data64>(o) : v;
            }
            return v;
        }

        __device__ __forceinline__ void dec_atomic_max(Data32* at, Data32 v) { atomicMax(at, v); }
        __device__ __forceinline__ void dec_atomic_max(Data64* at, Data64 v)
        {
            atomicMax(reinterpret_cast<unsigned long long*>(at), static_cast<unsigned long long>(v));
        }

        // grid: x = r * tiles + tile, y = m < L; ct: T[components][count][L][N], s: T[>= L][N], out: T[count][L][N]
        // (out may be ct: neither is __restrict__); consts: the fold image (stride M)
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void decrypt_phase(const T* ct, const T* __restrict__ s, T* out,
                                                               const T* __restrict__ consts, int count, int components,
                                                               int L, int M, int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, r = blockIdx.x / tiles;
            const unsigned m = blockIdx.y;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long at =
                ((static_cast<unsigned long long>(r) * static_cast<unsigned>(L) + m) << n_power) + col;
            const unsigned long long comp =
                (static_cast<unsigned long long>(count) * static_cast<unsigned>(L)) << n_power;
            const bool top = components == 3;

            const Vec c0 = *reinterpret_cast<const Vec*>(ct + at);
            const Vec c1 = *reinterpret_cast<const Vec*>(ct + comp + at);
            const Vec sv = *reinterpret_cast<const Vec*>(s + (static_cast<unsigned long long>(m) << n_power) + col);
            Vec c2{};
            if (top)
                c2 = *reinterpret_cast<const Vec*>(ct + 2 * comp + at);

            const IpFold<T> fold(consts, M, m);
            Vec o;
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                IpAcc<T> acc{c0.x[v], T(0), 0u};
                acc.mac(c1.x[v], sv.x[v]);
                if (top)
                {
                    const T sc = rns_shoup<T>(sv.x[v], T(1), fold.onep, fold.q); // s mod q
                    IpAcc<T> sq{T(0), T(0), 0u};
                    sq.mac(sc, sc); // below 2^(2W-2): no carry word
                    const T s2 = rns_shoup<T>(sq.hi, fold.t1, fold.t1p, fold.q) +
                                 rns_shoup<T>(sq.lo, T(1), fold.onep, fold.q); // below 2 q, congruent to s^2
                    acc.mac(c2.x[v], s2);
                }
                o.x[v] = fold.reduce(fold.sum(acc)); // the sum is below 3 q < 2^W
            }
            *reinterpret_cast<Vec*>(out + at) = o;
        }

        // grid: x = r * tiles + tile, y = m < L; pk: T[2][L][N], lifted: T[3][count][L][N] = (U, E0, E1), message:
        // T[count][L][N] or nullptr, out: T[2][count][L][N]; consts: the fold image (stride M)
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void encrypt_public_combine(const T* __restrict__ pk,
                                                                        const T* __restrict__ lifted,
                                                                        const T* __restrict__ message,
                                                                        T* __restrict__ out,
                                                                        const T* __restrict__ consts, int count, int L,
                                                                        int M, int n_power, unsigned tiles)
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
            const bool on = message != nullptr;

            const Vec p0 = *reinterpret_cast<const Vec*>(pk + limb);
            const Vec p1 = *reinterpret_cast<const Vec*>(pk + (static_cast<unsigned long long>(L) << n_power) + limb);
            const Vec u = *reinterpret_cast<const Vec*>(lifted + at);
            const Vec e0 = *reinterpret_cast<const Vec*>(lifted + comp + at);
            const Vec e1 = *reinterpret_cast<const Vec*>(lifted + 2 * comp + at);
            Vec mv{};
            if (on)
                mv = *reinterpret_cast<const Vec*>(message + at);

            const IpFold<T> fold(consts, M, m);
            Vec o0, o1;
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                IpAcc<T> a0{e0.x[v], T(0), 0u}, a1{e1.x[v], T(0), 0u};
                a0.mac(p0.x[v], u.x[v]);
                if (on)
                    a0.mac(T(1), mv.x[v]);
                a1.mac(p1.x[v], u.x[v]);
                o0.x[v] = fold.reduce(fold.sum(a0)); // the sums are below 3 q < 2^W
                o1.x[v] = fold.reduce(fold.sum(a1));
            }
            *reinterpret_cast<Vec*>(out + at) = o0;
            *reinterpret_cast<Vec*>(out + comp + at) = o1;
        }

        // grid: x = c * tiles + tile; message: T[count][N], out: T[count][L][N]; consts: the fold image (q_i at i)
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void bfv_scale_message(const T* __restrict__ message, T* __restrict__ out,
                                                                   const T* __restrict__ consts, BfvScaleArgs<T> args,
                                                                   int L, int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            using CP = const T __attribute__((address_space(4)))*;
            const unsigned tile = blockIdx.x % tiles, c = blockIdx.x / tiles;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const Vec mv = *reinterpret_cast<const Vec*>(message + (static_cast<unsigned long long>(c) << n_power) + col);
            const T t = args.t, h = args.half;
            T mag[V];
            bool neg[V];
#pragma unroll
            for (int v = 0; v < V; v++)
            {
                const T m = rns_shoup<T>(mv.x[v], T(1), args.one_shoup_t, t); // the word modulo t
                T r = rns_shoup<T>(m, args.q_mod_t, args.q_mod_t_shoup, t) + h; // t < 2^(W-2): no carry
                r = r >= t ? r - t : r;
                neg[v] = r > h, mag[v] = r > h ? r - h : h - r; // |h - r| < t < q_i
            }
            const CP k = (CP) (consts);
            T* po = out + ((static_cast<unsigned long long>(c) * static_cast<unsigned>(L)) << n_power) + col;
            for (int i = 0; i < L; i++)
            {
                const T q = k[i], w = args.t_inv[i], wp = args.t_inv_shoup[i];
                Vec o;
#pragma unroll
                for (int v = 0; v < V; v++)
                {
                    const T x = rns_shoup<T>(mag[v], w, wp, q);
                    o.x[v] = neg[v] && x != 0 ? q - x : x;
                }
                *reinterpret_cast<Vec*>(po + (static_cast<unsigned long long>(i) << n_power)) = o;
            }
        }

        // grid: x = stack * tiles + tile; x: T[stacks][L][N], message: T[stacks][N], noise_max: T[stacks] or nullptr;
        // partials: T[stacks][tiles] or nullptr (then the atomic merge into noise_max, which the caller has zeroed);
        // consts / up: the plan's run of constants and the offsets of its {q} -> {b} image (q, qhat^-1, R, b - 1).
        // LDS: one word per wave when noise_max is given
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void bfv_decode(const T* __restrict__ x, T* __restrict__ message,
                                                            T* noise_max, T* __restrict__ partials,
                                                            const T* __restrict__ consts, BcOffsets up,
                                                            BfvDecodeArgs<T> args, int L, int n_power, unsigned tiles)
        {
            using Vec = IpVec<T, V>;
            using W2 = typename RnsWide<T>::type;
            constexpr int W = static_cast<int>(8 * sizeof(T));
            constexpr T TOP = T(1) << (W - 1);
            const BcConsts<T> k(consts, up);
            const unsigned tile = blockIdx.x % tiles, st = blockIdx.x / tiles;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            T worst = 0;
            if (col < (1ull << n_power)) // (a lane past the ring still joins the reduction below)
            {
                const T t = args.t;
                const T* px = x + ((static_cast<unsigned long long>(st) * static_cast<unsigned>(L)) << n_power) + col;
                W2 zsum[V];
                T asum[V];
#pragma unroll
                for (int v = 0; v < V; v++)
                    zsum[v] = static_cast<W2>(TOP), asum[v] = 0;
                for (int i = 0; i < L; i++)
                {
                    const T q = k.q[i], w = k.w[i], wp = k.wp[i], recip = k.recip[i], shift = k.shift[i];
                    const T tp = args.t_shoup[i];
                    const Vec xv = *reinterpret_cast<const Vec*>(px + (static_cast<unsigned long long>(i) << n_power));
#pragma unroll
                    for (int v = 0; v < V; v++)
                    {
                        const T y = rns_shoup<T>(xv.x[v], w, wp, q);
                        T a = rns_mulhi(y, tp); // floor(t y / q) or one less
                        T r = t * y - a * q;    // in [0, 2 q)
                        if (r >= q)
                            r -= q, a += 1;
                        asum[v] += a; // both below t < 2^(W-2)
                        asum[v] = asum[v] >= t ? asum[v] - t : asum[v];
                        zsum[v] += bc_z<T>(r, recip, shift);
                    }
                }
                Vec o;
#pragma unroll
                for (int v = 0; v < V; v++)
                {
                    const T hi = static_cast<T>(zsum[v] >> W), lo = static_cast<T>(zsum[v]); // hi <= L
                    T m = asum[v] + rns_shoup<T>(hi, T(1), args.one_shoup_t, t);
                    o.x[v] = m >= t ? m - t : m;
                    const T nw = lo ^ TOP;                                  // lo - 2^(W-1): the signed noise word
                    const T mag = (nw & TOP) != 0 ? static_cast<T>(T(0) - nw) : nw; // |.|; 2^(W-1) for the most negative
                    worst = mag > worst ? mag : worst;
                }
                *reinterpret_cast<Vec*>(message + (static_cast<unsigned long long>(st) << n_power) + col) = o;
            }
            if (noise_max != nullptr) // workgroup-uniform
            {
                T* red = reinterpret_cast<T*>(dec_smem);
                const T best = dec_wave_max(worst);
                if (threadIdx.x % DEC_WAVE == 0)
                    red[threadIdx.x / DEC_WAVE] = best;
                __syncthreads();
                if (threadIdx.x == 0)
                {
                    T all = red[0];
                    for (unsigned w = 1; w < blockDim.x / DEC_WAVE; w++)
                        all = red[w] > all ? red[w] : all;
                    if (partials != nullptr)
                        partials[static_cast<unsigned long long>(st) * tiles + tile] = all;
                    else
                        dec_atomic_max(noise_max + st, all);
                }
            }
        }

        // grid: x = stack, ONE wave; partials: T[stacks][tiles] -> noise_max[stack] = the maximum over the tiles
        template <typename T>
        __global__ __launch_bounds__(DEC_WAVE) void bfv_decode_merge(const T* __restrict__ partials,
                                                                     T* __restrict__ noise_max, unsigned tiles)
        {
            const T* row = partials + static_cast<unsigned long long>(blockIdx.x) * tiles;
            T worst = 0;
            for (unsigned i = threadIdx.x; i < tiles; i += DEC_WAVE)
                worst = row[i] > worst ? row[i] : worst;
            const T best = dec_wave_max(worst);
            if (threadIdx.x == 0)
                noise_max[blockIdx.x] = best;
        }
    } // namespace kern

    namespace host
    {
        namespace
        {
            template <typename T, int V>
            void phase_as(const T* ct, const T* s, T* out, const T* consts, int count, int components, int L, int M,
                          int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(count));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::decrypt_phase<T, V>), dim3(g.blocks, static_cast<unsigned>(L)), dim3(g.nt), 0, stream,
                              ct, s, out, consts, count, components, L, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V>
            void public_as(const T* pk, const T* lifted, const T* message, T* out, const T* consts, int count, int L,
                           int M, int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(count));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::encrypt_public_combine<T, V>), dim3(g.blocks, static_cast<unsigned>(L)), dim3(g.nt),
                              0, stream, pk, lifted, message, out, consts, count, L, M, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V>
            void scale_as(const T* message, T* out, const T* consts, const kern::BfvScaleArgs<T>& args, int count, int L,
                          int n_power, bool enqueue, hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(count));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::bfv_scale_message<T, V>), dim3(g.blocks), dim3(g.nt), 0, stream, message, out,
                              consts, args, L, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
            }

            template <typename T, int V>
            void decode_as(const T* x, T* message, T* noise_max, T* partials, const T* consts, const kern::BcOffsets& up,
                           const kern::BfvDecodeArgs<T>& args, int stacks, int L, int n_power, bool enqueue,
                           hipStream_t stream)
            {
                const RelinGrid g = relin_grid(n_power, V, static_cast<unsigned long long>(stacks));
                if (!enqueue)
                    return;
                GPUNTT_LAUNCH((kern::bfv_decode<T, V>), dim3(g.blocks), dim3(g.nt),
                              (g.nt / kern::DEC_WAVE) * sizeof(T), stream, x, message, noise_max,
                              noise_max != nullptr ? partials : nullptr, consts, up, args, L, n_power, g.tiles);
                GPUNTT_HIP_CHECK(hipGetLastError());
                if (noise_max != nullptr && partials != nullptr)
                {
                    GPUNTT_LAUNCH((kern::bfv_decode_merge<T>), dim3(static_cast<unsigned>(stacks)), dim3(kern::DEC_WAVE), 0,
                                  stream, partials, noise_max, g.tiles);
                    GPUNTT_HIP_CHECK(hipGetLastError());
                }
            }
        } // namespace

        template <typename T>
        void decrypt_phase_launch(const T* ct, const T* s, T* out, const T* consts, int count, int components, int L,
                                  int M, int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {ct, s, out}))
                phase_as<T, VW>(ct, s, out, consts, count, components, L, M, n_power, enqueue, stream);
            else
                phase_as<T, 1>(ct, s, out, consts, count, components, L, M, n_power, enqueue, stream);
        }

        template <typename T>
        void encrypt_public_combine_launch(const T* pk, const T* lifted, const T* message, T* out, const T* consts,
                                           int count, int L, int M, int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {pk, lifted, message, out}))
                public_as<T, VW>(pk, lifted, message, out, consts, count, L, M, n_power, enqueue, stream);
            else
                public_as<T, 1>(pk, lifted, message, out, consts, count, L, M, n_power, enqueue, stream);
        }

        template <typename T>
        void bfv_scale_message_launch(const T* message, T* out, const T* consts, const kern::BfvScaleArgs<T>& args,
                                      int count, int L, int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {message, out}))
                scale_as<T, VW>(message, out, consts, args, count, L, n_power, enqueue, stream);
            else
                scale_as<T, 1>(message, out, consts, args, count, L, n_power, enqueue, stream);
        }

        template <typename T>
        void bfv_decode_launch(const T* x, T* message, T* noise_max, T* partials, const T* consts,
                               const kern::BcOffsets& up, const kern::BfvDecodeArgs<T>& args, int stacks, int L,
                               int n_power, bool enqueue, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (relin_wide<T>(n_power, {x, message}))
                decode_as<T, VW>(x, message, noise_max, partials, consts, up, args, stacks, L, n_power, enqueue, stream);
            else
                decode_as<T, 1>(x, message, noise_max, partials, consts, up, args, stacks, L, n_power, enqueue, stream);
        }

#define GPUNTT_DECRYPT_INSTANCES(T)                                                                                      \
    template void decrypt_phase_launch<T>(const T*, const T*, T*, const T*, int, int, int, int, int, bool, hipStream_t);  \
    template void encrypt_public_combine_launch<T>(const T*, const T*, const T*, T*, const T*, int, int, int, int, bool, \
                                                   hipStream_t);                                                         \
    template void bfv_scale_message_launch<T>(const T*, T*, const T*, const kern::BfvScaleArgs<T>&, int, int, int, bool, \
                                              hipStream_t);                                                              \
    template void bfv_decode_launch<T>(const T*, T*, T*, T*, const T*, const kern::BcOffsets&,                           \
                                       const kern::BfvDecodeArgs<T>&, int, int, int, bool, hipStream_t);
        GPUNTT_DECRYPT_INSTANCES(Data32)
        GPUNTT_DECRYPT_INSTANCES(Data64)
#undef GPUNTT_DECRYPT_INSTANCES
    } // namespace host
} // namespace gpuntt
