// sampling.hip -- the kernels and host references of include/gpuntt/rns/sampling.cuh: counter-based uniform and small
// samplers.  Every word is sample_uniform_word / sample_small_word of the header, a pure function of (seed, stream, word
// index), so the launch shape below is free: a lane owns a 16-byte group of one polynomial (V = 1 for a base pointer or
// a stride that is not 16-byte aligned, or N below a group) and stores it once.  blockIdx.x = row * tiles + tile with
// row = s * mod_count + m, so the limb is workgroup-uniform: q comes from the kernel argument by a scalar load and the
// mask stays in scalar registers.  The candidate loop is bounded by SAMPLE_MAX_CANDIDATES.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "gpuntt/rns/sampling.cuh"
#include "launch.hpp"
#include "relinearize_internal.hpp"
#include "rns_host.hpp"

namespace gpuntt
{
    namespace kern
    {
        // the moduli of one call, as a kernel argument (2 KiB for u64: inside the 4 KiB argument segment)
        template <typename T> struct SampleModuli
        {
            T q[SAMPLE_MAX_MODULI];
        };
        static_assert(sizeof(SampleModuli<Data64>) == 2048, "SampleModuli has to stay inside the argument segment");

        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void sample_uniform_words(T* __restrict__ out, SampleModuli<T> mods,
                                                                      int mod_count, int n_power, unsigned tiles,
                                                                      unsigned long long stride, unsigned long long seed,
                                                                      unsigned stream_id)
        {
            using Vec = IpVec<T, V>;
            const unsigned tile = blockIdx.x % tiles, row = blockIdx.x / tiles;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned s = row / static_cast<unsigned>(mod_count), m = row % static_cast<unsigned>(mod_count);
            const T q = mods.q[m], mask = sample_mask<T>(q);
            const unsigned long long w = (static_cast<unsigned long long>(row) << n_power) + col; // the dense index
            Vec o;
#pragma unroll
            for (int v = 0; v < V; v++)
                o.x[v] = sample_uniform_word<T>(w + v, q, mask, seed, stream_id, SAMPLE_MAX_CANDIDATES);
            *reinterpret_cast<Vec*>(out + s * stride + (static_cast<unsigned long long>(m) << n_power) + col) = o;
        }

        template <int V>
        __global__ __launch_bounds__(IP_NT) void sample_small_words(std::int32_t* __restrict__ out, int n_power,
                                                                    unsigned tiles, int distribution,
                                                                    unsigned long long seed, unsigned stream_id)
        {
            using Vec = IpVec<std::int32_t, V>;
            const unsigned tile = blockIdx.x % tiles, p = blockIdx.x / tiles;
            const unsigned long long col = (static_cast<unsigned long long>(tile) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const unsigned long long w = (static_cast<unsigned long long>(p) << n_power) + col;
            Vec o;
#pragma unroll
            for (int v = 0; v < V; v++)
                o.x[v] = sample_small_word(w + v, static_cast<SmallDistribution>(distribution), seed, stream_id);
            *reinterpret_cast<Vec*>(out + w) = o;
        }
    } // namespace kern

    namespace
    {
        template <typename T>
        void check_uniform(const T* out, const T* moduli, int mod_count, int n_power, int stacks, std::uint64_t stride)
        {
            host::rns_check_n_power(n_power);
            if (out == nullptr || moduli == nullptr)
                throw std::invalid_argument("null pointer argument");
            if (mod_count < 1 || mod_count > SAMPLE_MAX_MODULI)
                throw std::invalid_argument("Invalid mod_count!");
            if (stacks < 0)
                throw std::invalid_argument("Invalid stacks!");
            for (int m = 0; m < mod_count; m++)
                if (moduli[m] == 0)
                    throw std::invalid_argument("Invalid modulus!");
            if (stride < (static_cast<std::uint64_t>(mod_count) << n_power))
                throw std::invalid_argument("Invalid stack stride!");
        }
        void check_small(const std::int32_t* out, int polys, int n_power, SmallDistribution distribution)
        {
            host::rns_check_n_power(n_power);
            if (out == nullptr)
                throw std::invalid_argument("null pointer argument");
            if (polys < 0)
                throw std::invalid_argument("Invalid polys!");
            if (distribution != SmallDistribution::ternary && distribution != SmallDistribution::cbd21)
                throw std::invalid_argument("Invalid distribution!");
        }

        template <typename T, int V>
        void uniform_as(T* out, const kern::SampleModuli<T>& mods, int mod_count, int n_power, int stacks,
                        std::uint64_t stride, std::uint64_t seed, std::uint32_t stream_id, hipStream_t stream)
        {
            const host::RelinGrid g =
                host::relin_grid(n_power, V, static_cast<unsigned long long>(stacks) * static_cast<unsigned>(mod_count));
            GPUNTT_LAUNCH((kern::sample_uniform_words<T, V>), dim3(g.blocks), dim3(g.nt), 0, stream, out, mods, mod_count,
                          n_power, g.tiles, static_cast<unsigned long long>(stride), static_cast<unsigned long long>(seed),
                          stream_id);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        template <int V>
        void small_as(std::int32_t* out, int polys, int n_power, SmallDistribution distribution, std::uint64_t seed,
                      std::uint32_t stream_id, hipStream_t stream)
        {
            const host::RelinGrid g = host::relin_grid(n_power, V, static_cast<unsigned long long>(polys));
            GPUNTT_LAUNCH((kern::sample_small_words<V>), dim3(g.blocks), dim3(g.nt), 0, stream, out, n_power, g.tiles,
                          static_cast<int>(distribution), static_cast<unsigned long long>(seed), stream_id);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }
    } // namespace

    template <typename T>
    void sample_uniform(T* device_out, const T* moduli_host, int mod_count, int n_power, int stacks,
                        std::uint64_t stack_stride_words, std::uint64_t seed, std::uint32_t stream_id, stream_t stream)
    {
        check_uniform<T>(device_out, moduli_host, mod_count, n_power, stacks, stack_stride_words);
        if (stacks == 0)
            return;
        kern::SampleModuli<T> mods{};
        for (int m = 0; m < mod_count; m++)
            mods.q[m] = moduli_host[m];
        constexpr int VW = 16 / sizeof(T);
        const bool wide = n_power >= (sizeof(T) == 8 ? 1 : 2) && reinterpret_cast<uintptr_t>(device_out) % 16 == 0 &&
                          stack_stride_words % VW == 0;
        if (wide)
            uniform_as<T, VW>(device_out, mods, mod_count, n_power, stacks, stack_stride_words, seed, stream_id, stream);
        else
            uniform_as<T, 1>(device_out, mods, mod_count, n_power, stacks, stack_stride_words, seed, stream_id, stream);
    }

    void sample_small(std::int32_t* device_out, int polys, int n_power, SmallDistribution distribution,
                      std::uint64_t seed, std::uint32_t stream_id, stream_t stream)
    {
        check_small(device_out, polys, n_power, distribution);
        if (polys == 0)
            return;
        if (n_power >= 2 && reinterpret_cast<uintptr_t>(device_out) % 16 == 0)
            small_as<4>(device_out, polys, n_power, distribution, seed, stream_id, stream);
        else
            small_as<1>(device_out, polys, n_power, distribution, seed, stream_id, stream);
    }

    void reference_philox(const std::uint32_t ctr[4], const std::uint32_t key[2], std::uint32_t out[4])
    {
        if (ctr == nullptr || key == nullptr || out == nullptr)
            throw std::invalid_argument("null pointer argument");
        const std::uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
        const PhiloxBlock b = philox4x32_10(c, k);
        for (int i = 0; i < 4; i++)
            out[i] = b.v[i];
    }

    template <typename T>
    void reference_sample_uniform(T* out_host, const T* moduli_host, int mod_count, int n_power, int stacks,
                                  std::uint64_t stack_stride_words, std::uint64_t seed, std::uint32_t stream_id,
                                  int max_candidates)
    {
        check_uniform<T>(out_host, moduli_host, mod_count, n_power, stacks, stack_stride_words);
        if (max_candidates < 1)
            throw std::invalid_argument("Invalid max_candidates!");
        const std::uint64_t n = 1ull << n_power;
        for (std::uint64_t s = 0; s < static_cast<std::uint64_t>(stacks); s++)
            for (std::uint64_t m = 0; m < static_cast<std::uint64_t>(mod_count); m++)
            {
                const T q = moduli_host[m], mask = sample_mask<T>(q);
                for (std::uint64_t j = 0; j < n; j++)
                    out_host[s * stack_stride_words + m * n + j] = sample_uniform_word<T>(
                        (s * mod_count + m) * n + j, q, mask, seed, stream_id, max_candidates);
            }
    }

    void reference_sample_small(std::int32_t* out_host, int polys, int n_power, SmallDistribution distribution,
                                std::uint64_t seed, std::uint32_t stream_id)
    {
        check_small(out_host, polys, n_power, distribution);
        const std::uint64_t total = static_cast<std::uint64_t>(polys) << n_power;
        for (std::uint64_t w = 0; w < total; w++)
            out_host[w] = sample_small_word(w, distribution, seed, stream_id);
    }

    template void sample_uniform<Data32>(Data32*, const Data32*, int, int, int, std::uint64_t, std::uint64_t,
                                         std::uint32_t, stream_t);
    template void sample_uniform<Data64>(Data64*, const Data64*, int, int, int, std::uint64_t, std::uint64_t,
                                         std::uint32_t, stream_t);
    template void reference_sample_uniform<Data32>(Data32*, const Data32*, int, int, int, std::uint64_t, std::uint64_t,
                                                   std::uint32_t, int);
    template void reference_sample_uniform<Data64>(Data64*, const Data64*, int, int, int, std::uint64_t, std::uint64_t,
                                                   std::uint32_t, int);
} // namespace gpuntt
