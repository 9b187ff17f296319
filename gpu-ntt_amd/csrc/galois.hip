// galois.hip -- Galois automorphisms sigma_k: a(X) -> a(X^k) (extension, include/gpuntt/ntt_merge/galois.cuh).
//
// NTT domain (the hot path).  Take the top s bits of an output slot i: they depend only on the top s bits of its
// source slot j.  Bit reversal turns top bits into low bits, and the low bits of k * e mod 2^(n+1) depend only on the
// low bits of e, so every chunk of C = N / 2^s consecutive output slots is filled from exactly ONE chunk of C
// consecutive input slots.  One workgroup per (polynomial, source chunk) loads its chunk with 16-byte loads into LDS
// and, for each of the G elements of the call, writes that element's destination chunk with consecutive stores,
// reading LDS in permuted order.  Traffic: (1 + G) * N * sizeof(T) per polynomial.  Within one wave the 64
// consecutive output slots read a permutation of 64 consecutive LDS words (the slot's low 6 bits become the source's
// low 6 bits), so the permuted side costs no more LDS cycles than a linear read would.
//
// Coefficient domain.  Rings up to the LDS tile: one workgroup per tile (one polynomial, or several small ones),
// loaded coalesced, then written in order, gathered from LDS at the odd stride k^-1 (an odd stride hits every bank
// once per 32 lanes).  Larger rings: j = k^-1 * i mod 2N scatters every chunk over the whole polynomial, so each
// workgroup owns a contiguous output range and gathers from global memory; the workgroups of one polynomial are
// launched next to each other, so its source stays in L2 / the Infinity Cache while they run.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "gpuntt/ntt_merge/galois.cuh"
#include "launch.hpp"

namespace gpuntt
{
    namespace kern
    {
        // the call's Galois elements as kernel arguments: elt[g] = k (reduced), inv[g] = k^-1 (same modulus)
        struct GaloisArgs
        {
            std::uint32_t elt[GALOIS_MAX_COUNT];
            std::uint32_t inv[GALOIS_MAX_COUNT];
            int count;
        };

        constexpr int GALOIS_NT = 256;

        // one workgroup loads `len` consecutive words of `in` into `tile` (16-byte loads when VEC)
        template <typename T, bool VEC>
        __device__ __forceinline__ void galois_load_tile(T* tile, const T* __restrict__ in, unsigned len)
        {
            if constexpr (VEC)
            {
                constexpr unsigned V = 16 / sizeof(T);
                struct alignas(16) Vec
                {
                    T x[V];
                };
                const unsigned nv = len / V;
                for (unsigned v = threadIdx.x; v < nv; v += GALOIS_NT)
                    reinterpret_cast<Vec*>(tile)[v] = reinterpret_cast<const Vec*>(in)[v];
                for (unsigned t = nv * V + threadIdx.x; t < len; t += GALOIS_NT)
                    tile[t] = in[t];
            }
            else
            {
                for (unsigned t = threadIdx.x; t < len; t += GALOIS_NT)
                    tile[t] = in[t];
            }
            __syncthreads();
        }

        // NTT domain.  n >= LOGC: block = (polynomial, source chunk of 2^LOGC slots); n < LOGC: block = up to 2^(LOGC-n)
        // whole polynomials.
        template <typename T, int LOGC, bool VEC>
        __global__ __launch_bounds__(GALOIS_NT) void automorphism_ntt(const T* __restrict__ in, T* __restrict__ out,
                                                                      GaloisArgs ga, int n, int negacyclic,
                                                                      unsigned batch)
        {
            constexpr unsigned C = 1u << LOGC;
            __shared__ T tile[C];
            const bool neg = negacyclic != 0;
            const unsigned long long plane = static_cast<unsigned long long>(batch) << n; // words per element's output
            if (n >= LOGC)
            {
                const int s = n - LOGC;
                const unsigned poly = blockIdx.x >> s, c = blockIdx.x & ((1u << s) - 1u);
                const unsigned long long base = (static_cast<unsigned long long>(poly) << n);
                galois_load_tile<T, VEC>(tile, in + base + (static_cast<unsigned long long>(c) << LOGC), C);
                for (int g = 0; g < ga.count; g++)
                {
                    const std::uint32_t k = ga.elt[g];
                    // the chunk this source chunk lands in: where its first slot goes under sigma_k, i.e. the source
                    // of that slot under sigma_k^-1
                    const unsigned d = galois_ntt_source(c << LOGC, ga.inv[g], n, neg) >> LOGC;
                    T* dst = out + g * plane + base + (static_cast<unsigned long long>(d) << LOGC);
#pragma unroll 4
                    for (unsigned l = threadIdx.x; l < C; l += GALOIS_NT)
                    {
                        const std::uint32_t j = galois_ntt_source((d << LOGC) | l, k, n, neg);
                        dst[l] = tile[j & (C - 1u)];
                    }
                }
            }
            else
            {
                const unsigned per = 1u << (LOGC - n);
                const unsigned first = blockIdx.x * per;
                const unsigned polys = min(per, batch - first);
                const unsigned len = polys << n, nmask = (1u << n) - 1u;
                const unsigned long long base = static_cast<unsigned long long>(first) << n;
                galois_load_tile<T, VEC>(tile, in + base, len);
                for (int g = 0; g < ga.count; g++)
                {
                    const std::uint32_t k = ga.elt[g];
                    T* dst = out + g * plane + base;
                    for (unsigned t = threadIdx.x; t < len; t += GALOIS_NT)
                        dst[t] = tile[(t & ~nmask) | galois_ntt_source(t & nmask, k, n, neg)];
                }
            }
        }

        template <typename T> __device__ __forceinline__ T galois_negate(T x, T q) { return x == 0 ? T(0) : q - x; }

        // coefficient domain, n <= LOGC: block = up to 2^(LOGC-n) whole polynomials staged in LDS
        template <typename T, int LOGC, bool VEC>
        __global__ __launch_bounds__(GALOIS_NT) void automorphism_coeff_tile(const T* __restrict__ in,
                                                                             T* __restrict__ out, GaloisArgs ga,
                                                                             const Modulus<T>* __restrict__ mods,
                                                                             T q, int mod_count, int n,
                                                                             int negacyclic, unsigned batch)
        {
            constexpr unsigned C = 1u << LOGC;
            __shared__ T tile[C];
            const bool neg = negacyclic != 0;
            const unsigned long long plane = static_cast<unsigned long long>(batch) << n;
            const unsigned per = 1u << (LOGC - n);
            const unsigned first = blockIdx.x * per;
            const unsigned polys = min(per, batch - first);
            const unsigned len = polys << n, nmask = (1u << n) - 1u;
            const unsigned long long base = static_cast<unsigned long long>(first) << n;
            galois_load_tile<T, VEC>(tile, in + base, len);
            for (int g = 0; g < ga.count; g++)
            {
                const std::uint32_t kinv = ga.inv[g];
                T* dst = out + g * plane + base;
                for (unsigned t = threadIdx.x; t < len; t += GALOIS_NT)
                {
                    const std::uint32_t j = galois_coeff_source(t & nmask, kinv, n, neg);
                    T v = tile[(t & ~nmask) | (j & nmask)];
                    if (j > nmask)
                        v = galois_negate(v, mods ? mods[(first + (t >> n)) % static_cast<unsigned>(mod_count)].value : q);
                    dst[t] = v;
                }
            }
        }

        // coefficient domain, n > LOGC: block = (polynomial, element, output range of 2^LOGC coefficients), gathered
        // from global
        template <typename T, int LOGC>
        __global__ __launch_bounds__(GALOIS_NT) void automorphism_coeff_gather(const T* __restrict__ in,
                                                                               T* __restrict__ out, GaloisArgs ga,
                                                                               const Modulus<T>* __restrict__ mods,
                                                                               T q, int mod_count, int n,
                                                                               int negacyclic, unsigned batch)
        {
            constexpr unsigned C = 1u << LOGC;
            const bool neg = negacyclic != 0;
            const unsigned long long plane = static_cast<unsigned long long>(batch) << n;
            const int s = n - LOGC;
            // block = ((poly * count + g) << s) + r: every workgroup that reads one polynomial runs next to the others
            const unsigned r = blockIdx.x & ((1u << s) - 1u), pg = blockIdx.x >> s;
            const unsigned poly = pg / static_cast<unsigned>(ga.count), g = pg % static_cast<unsigned>(ga.count);
            const unsigned nmask = (1u << n) - 1u;
            const unsigned long long base = static_cast<unsigned long long>(poly) << n;
            const T* src = in + base;
            const T qp = mods ? mods[poly % static_cast<unsigned>(mod_count)].value : q;
            const std::uint32_t kinv = ga.inv[g];
            T* dst = out + g * plane + base + (static_cast<unsigned long long>(r) << LOGC);
#pragma unroll 4
            for (unsigned l = threadIdx.x; l < C; l += GALOIS_NT)
            {
                const std::uint32_t j = galois_coeff_source((r << LOGC) | l, kinv, n, neg);
                const T v = src[j & nmask];
                dst[l] = (j > nmask) ? galois_negate(v, qp) : v;
            }
        }
    } // namespace kern

    namespace
    {
        // 32 KiB chunks and tiles (4096 u64 / 8192 u32 words: five workgroups per CU by LDS).  64 KiB coefficient tiles
        // (two workgroups per CU) were slower than the L2-served gather at u32 2^14 x 8192 (2.0 x the time of a copy)
        template <typename T> constexpr int ntt_chunk_log() { return sizeof(T) == 8 ? 12 : 13; }
        template <typename T> constexpr int coeff_tile_log() { return ntt_chunk_log<T>(); }

        template <typename T>
        kern::GaloisArgs galois_args(const T* in, const T* out, const std::uint32_t* elts, int count, int n_power,
                                     ReductionPolynomial poly, int batch_size)
        {
            if (n_power <= 0 || n_power >= 29)
                throw std::invalid_argument("Invalid n_power range!");
            if (poly != ReductionPolynomial::X_N_plus && poly != ReductionPolynomial::X_N_minus)
                throw std::invalid_argument("Invalid reduction_poly!");
            if (count < 1 || count > GALOIS_MAX_COUNT)
                throw std::invalid_argument("Invalid galois_count!");
            if (elts == nullptr || in == nullptr || out == nullptr)
                throw std::invalid_argument("null pointer argument");
            if (batch_size < 0)
                throw std::invalid_argument("Invalid batch_size!");
            const unsigned long long words = static_cast<unsigned long long>(batch_size) << n_power;
            const auto in_lo = reinterpret_cast<uintptr_t>(in), out_lo = reinterpret_cast<uintptr_t>(out);
            const auto in_hi = in_lo + words * sizeof(T), out_hi = out_lo + words * count * sizeof(T);
            if (in_lo == out_lo || (words != 0 && in_lo < out_hi && out_lo < in_hi))
                throw std::invalid_argument("Automorphism input and output overlap!");
            const std::uint32_t mask =
                (poly == ReductionPolynomial::X_N_plus) ? (2u << n_power) - 1u : (1u << n_power) - 1u;
            kern::GaloisArgs ga{};
            ga.count = count;
            for (int g = 0; g < count; g++)
            {
                const std::uint32_t k = elts[g] & mask;
                if ((k & 1u) == 0u)
                    throw std::invalid_argument("Invalid Galois element (must be odd)!");
                ga.elt[g] = k;
                ga.inv[g] = galois_inverse(k) & mask;
            }
            return ga;
        }

        bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

        // HIP caps a launch at gridDim.x * blockDim.x <= 2^32 - 1 work-items (2^24 - 1 blocks of GALOIS_NT)
        void check_grid(unsigned long long blocks)
        {
            if (blocks * kern::GALOIS_NT > 0xFFFFFFFFull)
                throw std::invalid_argument("Invalid batch_size!");
        }

        template <typename T>
        void coeff_launch(const T* in, T* out, const std::uint32_t* elts, int count, const Modulus<T>* mods, T q,
                          int mod_count, int n_power, ReductionPolynomial poly, int batch_size, hipStream_t stream)
        {
            const kern::GaloisArgs ga = galois_args<T>(in, out, elts, count, n_power, poly, batch_size);
            if (batch_size == 0)
                return;
            constexpr int L = coeff_tile_log<T>();
            const int neg = poly == ReductionPolynomial::X_N_plus ? 1 : 0;
            const unsigned batch = static_cast<unsigned>(batch_size);
            if (n_power <= L)
            {
                const unsigned per = 1u << (L - n_power);
                const dim3 grid((batch + per - 1u) / per);
                if (aligned16(in))
                    GPUNTT_LAUNCH((kern::automorphism_coeff_tile<T, L, true>), grid, dim3(kern::GALOIS_NT), 0, stream,
                                  in, out, ga, mods, q, mod_count, n_power, neg, batch);
                else
                    GPUNTT_LAUNCH((kern::automorphism_coeff_tile<T, L, false>), grid, dim3(kern::GALOIS_NT), 0, stream,
                                  in, out, ga, mods, q, mod_count, n_power, neg, batch);
            }
            else
            {
                const unsigned long long blocks = (static_cast<unsigned long long>(batch) * count) << (n_power - L);
                check_grid(blocks);
                GPUNTT_LAUNCH((kern::automorphism_coeff_gather<T, L>), dim3(static_cast<unsigned>(blocks)),
                              dim3(kern::GALOIS_NT), 0, stream, in, out, ga, mods, q, mod_count, n_power, neg, batch);
            }
            GPUNTT_HIP_CHECK(hipGetLastError());
        }
    } // namespace

    std::uint32_t GaloisElementForRotation(int steps, int n_power)
    {
        if (n_power <= 0 || n_power >= 29)
            throw std::invalid_argument("Invalid n_power range!");
        const std::uint32_t mask = (2u << n_power) - 1u;
        // 5 generates a cyclic subgroup of order N/2 of (Z/2N)^*: reduce the exponent into [0, N/2)
        const long long order = (n_power >= 2) ? (1ll << (n_power - 1)) : 1ll;
        long long e = steps % order;
        if (e < 0)
            e += order;
        std::uint32_t r = 1u, b = 5u & mask;
        for (; e != 0; e >>= 1)
        {
            if (e & 1)
                r = (r * b) & mask;
            b = (b * b) & mask;
        }
        return r;
    }

    std::uint32_t GaloisElementForConjugation(int n_power)
    {
        if (n_power <= 0 || n_power >= 29)
            throw std::invalid_argument("Invalid n_power range!");
        return (2u << n_power) - 1u;
    }

    template <typename T>
    __host__ void GPU_Automorphism_NTT(const T* device_in, T* device_out, const std::uint32_t* galois_elts_host,
                                       int galois_count, int n_power, ReductionPolynomial reduction_poly,
                                       int batch_size, stream_t stream)
    {
        const kern::GaloisArgs ga =
            galois_args<T>(device_in, device_out, galois_elts_host, galois_count, n_power, reduction_poly, batch_size);
        if (batch_size == 0)
            return;
        constexpr int L = ntt_chunk_log<T>();
        const int neg = reduction_poly == ReductionPolynomial::X_N_plus ? 1 : 0;
        const unsigned batch = static_cast<unsigned>(batch_size);
        unsigned long long blocks;
        if (n_power >= L)
            blocks = static_cast<unsigned long long>(batch) << (n_power - L);
        else
        {
            const unsigned per = 1u << (L - n_power);
            blocks = (batch + per - 1u) / per;
        }
        check_grid(blocks);
        if (aligned16(device_in))
            GPUNTT_LAUNCH((kern::automorphism_ntt<T, L, true>), dim3(static_cast<unsigned>(blocks)),
                          dim3(kern::GALOIS_NT), 0, stream, device_in, device_out, ga, n_power, neg, batch);
        else
            GPUNTT_LAUNCH((kern::automorphism_ntt<T, L, false>), dim3(static_cast<unsigned>(blocks)),
                          dim3(kern::GALOIS_NT), 0, stream, device_in, device_out, ga, n_power, neg, batch);
        GPUNTT_HIP_CHECK(hipGetLastError());
    }

    template <typename T>
    __host__ void GPU_Automorphism(const T* device_in, T* device_out, const std::uint32_t* galois_elts_host,
                                   int galois_count, Modulus<T> modulus, int n_power,
                                   ReductionPolynomial reduction_poly, int batch_size, stream_t stream)
    {
        coeff_launch<T>(device_in, device_out, galois_elts_host, galois_count, nullptr, modulus.value, 1, n_power,
                        reduction_poly, batch_size, stream);
    }

    template <typename T>
    __host__ void GPU_Automorphism(const T* device_in, T* device_out, const std::uint32_t* galois_elts_host,
                                   int galois_count, const Modulus<T>* modulus_device, int mod_count, int n_power,
                                   ReductionPolynomial reduction_poly, int batch_size, stream_t stream)
    {
        if (mod_count <= 0 || modulus_device == nullptr)
            throw std::invalid_argument("Invalid mod_count!");
        coeff_launch<T>(device_in, device_out, galois_elts_host, galois_count, modulus_device, T(0), mod_count,
                        n_power, reduction_poly, batch_size, stream);
    }

#define GPUNTT_INST_GALOIS(T)                                                                                        \
    template __host__ void GPU_Automorphism_NTT<T>(const T*, T*, const std::uint32_t*, int, int, ReductionPolynomial,  \
                                                   int, stream_t);                                                     \
    template __host__ void GPU_Automorphism<T>(const T*, T*, const std::uint32_t*, int, Modulus<T>, int,              \
                                               ReductionPolynomial, int, stream_t);                                    \
    template __host__ void GPU_Automorphism<T>(const T*, T*, const std::uint32_t*, int, const Modulus<T>*, int, int,  \
                                               ReductionPolynomial, int, stream_t);
    GPUNTT_INST_GALOIS(Data32)
    GPUNTT_INST_GALOIS(Data64)
#undef GPUNTT_INST_GALOIS
} // namespace gpuntt
