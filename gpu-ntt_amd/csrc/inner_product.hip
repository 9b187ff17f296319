// inner_product.hip -- RNS inner product (extension, include/gpuntt/rns/inner_product.cuh).
//
// HBM-bound: per lane and digit one 16-byte group of `a` per input, C groups of the key, and one full product plus a
// three-word add per word pair.  A lane owns 16 contiguous bytes (V = 16 / sizeof(T) columns) of one modulus m of a
// BLOCK of RB inputs; it walks d = 0 .. D-1 once with all RB * C * V accumulators live, so every word of `a` is read
// once per call (not once per component) and every word of the key once per block of inputs (not once per input).
// blockIdx.y is m: q_m, the folding constants and the key limb are wave-uniform and come through the scalar cache
// (the constants) and the kernel-argument segment (the limb table).
//
// The accumulator is the three-word one of base_conversion.hip: S = c 2^2W + h 2^W + l, exact for 64 products of
// ARBITRARY words plus one word (< 2^(2W+7)); the operands are arbitrary, so unlike there no group of terms is known to
// fit 2W bits and the carry is taken on every term, from the add's own carry-out.  S leaves as
// (h * [2^W]_q + c * [2^2W]_q + l) mod q: three exact Shoup products (each canonical, their sum below 3 q < 2^W) and two
// conditional subtractions.  Nothing is pre-reduced and Modulus<T>::mu is not used.
//
// N below the 16-byte group or a buffer that is not 16-byte aligned: the same kernel with V = 1.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <vector>

#include "gpuntt/rns/inner_product.cuh"
#include "inner_product_internal.hpp"
#include "launch.hpp"
#include "rns_host.hpp"

namespace gpuntt
{
    namespace kern
    {
        // IP_NT, ip_block, IpLimbs, ip_addc, IpAcc, IpFold: inner_product_internal.hpp; RnsWide, rns_shoup: rns_arith.hpp

        // the plan's constants in the workspace: six arrays of M words (q, 2^W mod q and its Shoup companion, 2^2W mod q
        // and its companion, the companion of 1), read through the CONSTANT address space -- nothing writes the workspace
        // while a call runs, and a load from that address space at a wave-uniform address is a scalar load
        template <typename T, int V, int C, int RB>
        __global__ __launch_bounds__(IP_NT) void inner_product(const T* __restrict__ a, const T* __restrict__ key,
                                                               T* __restrict__ out, const T* __restrict__ consts,
                                                               IpLimbs limbs, int D, int count, int M, int KM,
                                                               int n_power, unsigned tiles, int accumulate)
        {
            ip_digit_loop<T, V, C, RB>(a, key, out, consts, limbs, D, count, M, KM, n_power, tiles,
                                       IpSeedOut<T>{accumulate});
        }
    } // namespace kern

    namespace
    {
        using U128 = unsigned __int128;

        template <typename T> std::uint64_t ip_checked_value(const Modulus<T>& m)
        {
            if (m.value < 2)
                throw std::invalid_argument("Invalid modulus!");
            const Modulus<T> ref(m.value); // throws for a modulus outside the library's domain
            if (ref.bit != m.bit || ref.mu != m.mu)
                throw std::invalid_argument("Invalid modulus!");
            return static_cast<std::uint64_t>(m.value);
        }

        // the constants in exact integers (64-bit words for both widths)
        struct IpHostConsts
        {
            std::vector<std::uint64_t> q, t1, t1p, t2, t2p, onep;
        };

        template <typename T> IpHostConsts ip_derive(const Modulus<T>* mods, int M)
        {
            constexpr int W = static_cast<int>(8 * sizeof(T));
            if (M < 1 || M > INNERPROD_MAX_MODULI)
                throw std::invalid_argument("Invalid mod_count!");
            if (mods == nullptr)
                throw std::invalid_argument("null pointer argument");
            IpHostConsts h;
            for (int i = 0; i < M; i++)
            {
                const std::uint64_t q = ip_checked_value(mods[i]);
                const host::RnsFoldConsts f = host::rns_fold_consts(q, W);
                h.q.push_back(q);
                h.t1.push_back(f.t1), h.t1p.push_back(f.t1p), h.t2.push_back(f.t2), h.t2p.push_back(f.t2p);
                h.onep.push_back(f.onep);
            }
            return h;
        }

        // the argument checks of one call (device or host arrays alike); fills the limb table
        template <typename T>
        void ip_check_call(int M, const T* a, const T* key, const T* out, int n_power, int D, int C, int count, int KM,
                           const int* key_limbs, unsigned char limbs[INNERPROD_MAX_MODULI])
        {
            host::rns_check_n_power(n_power);
            if (D < 1 || D > INNERPROD_MAX_DIGITS)
                throw std::invalid_argument("Invalid digits!");
            if (C < 1 || C > INNERPROD_MAX_COMPONENTS)
                throw std::invalid_argument("Invalid components!");
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (KM < M || KM > INNERPROD_MAX_KEY_MODULI)
                throw std::invalid_argument("Invalid key_mod_count!");
            for (int m = 0; m < M; m++)
            {
                const int l = key_limbs != nullptr ? key_limbs[m] : m;
                if (l < 0 || l >= KM)
                    throw std::invalid_argument("Invalid key_limbs!");
                limbs[m] = static_cast<unsigned char>(l);
            }
            if (a == nullptr || key == nullptr || out == nullptr)
                throw std::invalid_argument("null pointer argument");
            const std::uint64_t stack = (static_cast<std::uint64_t>(count) * M) << n_power;
            const std::uint64_t out_bytes = C * stack * sizeof(T);
            const std::uint64_t key_bytes = ((static_cast<std::uint64_t>(D) * C * KM) << n_power) * sizeof(T);
            if (host::rns_overlap(a, D * stack * sizeof(T), out, out_bytes) ||
                host::rns_overlap(key, key_bytes, out, out_bytes))
                throw std::invalid_argument("Inner product output overlaps an input!");
        }
    } // namespace

    template <typename T> struct InnerProductPlan<T>::Impl
    {
        int M = 0;
        void* ws = nullptr;
        bool owns = false;

        template <int V, int C, int RB>
        void launch_as(const T* a, const T* key, T* out, const kern::IpLimbs& limbs, int n_power, int D, int count,
                       int KM, bool accumulate, hipStream_t stream) const
        {
            const unsigned long long lanes = (1ull << n_power) / V; // per polynomial
            unsigned nt = 64;
            while (nt < kern::IP_NT && nt < lanes)
                nt *= 2;
            const unsigned long long tiles = (lanes + nt - 1) / nt;
            const unsigned long long blocks = tiles * ((static_cast<unsigned long long>(count) + RB - 1) / RB);
            if (blocks * nt > 0xFFFFFFFFull) // HIP caps a launch at 2^32 - 1 work-items per dimension
                throw std::invalid_argument("Invalid count!");
            GPUNTT_LAUNCH((kern::inner_product<T, V, C, RB>), dim3(static_cast<unsigned>(blocks), M), dim3(nt), 0, stream,
                          a, key, out, static_cast<const T*>(ws), limbs, D, count, M, KM, n_power,
                          static_cast<unsigned>(tiles), accumulate ? 1 : 0);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        // a block of 4 inputs where the registers allow it and count has them, of 2 for count = 2 or 3 (a block past
        // the end of count multiplies for nothing), one input per lane for count = 1
        template <int V, int C> void launch_c(const T* a, const T* key, T* out, const kern::IpLimbs& limbs, int n_power,
                                              int D, int count, int KM, bool accumulate, hipStream_t stream) const
        {
            if (count >= 4 && kern::ip_block(C) == 4)
                launch_as<V, C, kern::ip_block(C)>(a, key, out, limbs, n_power, D, count, KM, accumulate, stream);
            else if (count >= 2)
                launch_as<V, C, 2>(a, key, out, limbs, n_power, D, count, KM, accumulate, stream);
            else
                launch_as<V, C, 1>(a, key, out, limbs, n_power, D, count, KM, accumulate, stream);
        }

        template <int V> void launch_v(const T* a, const T* key, T* out, const kern::IpLimbs& limbs, int n_power, int D,
                                       int C, int count, int KM, bool accumulate, hipStream_t stream) const
        {
            switch (C)
            {
            case 1: return launch_c<V, 1>(a, key, out, limbs, n_power, D, count, KM, accumulate, stream);
            case 2: return launch_c<V, 2>(a, key, out, limbs, n_power, D, count, KM, accumulate, stream);
            case 3: return launch_c<V, 3>(a, key, out, limbs, n_power, D, count, KM, accumulate, stream);
            default: return launch_c<V, 4>(a, key, out, limbs, n_power, D, count, KM, accumulate, stream);
            }
        }

        void launch(const T* a, const T* key, T* out, int n_power, int D, int C, int count, bool accumulate, int KM,
                    const int* key_limbs, hipStream_t stream) const
        {
            kern::IpLimbs limbs{};
            ip_check_call<T>(M, a, key, out, n_power, D, C, count, KM, key_limbs, limbs.v);
            if (count == 0)
                return;
            constexpr int VW = 16 / sizeof(T);
            // a 16-byte group must stay inside one polynomial and be aligned (every stride is a multiple of N words)
            const bool wide = (n_power >= (sizeof(T) == 8 ? 1 : 2)) &&
                              ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(key) |
                                reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
            if (wide)
                launch_v<VW>(a, key, out, limbs, n_power, D, C, count, KM, accumulate, stream);
            else
                launch_v<1>(a, key, out, limbs, n_power, D, C, count, KM, accumulate, stream);
        }
    };

    template <typename T> size_t InnerProductPlan<T>::workspace_bytes(int mod_count)
    {
        if (mod_count < 1 || mod_count > INNERPROD_MAX_MODULI)
            throw std::invalid_argument("Invalid mod_count!");
        return host::rns_align(6 * static_cast<size_t>(mod_count) * sizeof(T));
    }

    template <typename T>
    InnerProductPlan<T>::InnerProductPlan(const Modulus<T>* moduli_host, int mod_count, stream_t stream,
                                          void* workspace_device)
        : p_(nullptr)
    {
        const IpHostConsts h = ip_derive<T>(moduli_host, mod_count);
        const int M = mod_count;
        std::vector<T> img;
        for (const std::vector<std::uint64_t>* v : {&h.q, &h.t1, &h.t1p, &h.t2, &h.t2p, &h.onep})
            for (std::uint64_t w : *v)
                img.push_back(static_cast<T>(w));

        Impl* p = new Impl;
        p->M = M;
        try
        {
            if (workspace_device != nullptr)
                p->ws = workspace_device;
            else
            {
                GPUNTT_HIP_CHECK(hipMalloc(&p->ws, workspace_bytes(M)));
                p->owns = true;
            }
            GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws, img.data(), img.size() * sizeof(T), hipMemcpyHostToDevice, stream));
            GPUNTT_HIP_CHECK(hipStreamSynchronize(stream)); // `img` dies with this scope
        }
        catch (...)
        {
            if (p->owns)
                (void) hipFree(p->ws);
            delete p;
            throw;
        }
        p_ = p;
    }

    template <typename T> InnerProductPlan<T>::~InnerProductPlan()
    {
        if (p_ != nullptr && p_->owns)
            (void) hipFree(p_->ws);
        delete p_;
    }

    template <typename T>
    void InnerProductPlan<T>::multiply_accumulate(const T* device_a, const T* device_key, T* device_out, int n_power,
                                                  int digits, int components, int count, bool accumulate,
                                                  int key_mod_count, const int* key_limbs_host, stream_t stream) const
    {
        p_->launch(device_a, device_key, device_out, n_power, digits, components, count, accumulate, key_mod_count,
                   key_limbs_host, stream);
    }

    template <typename T> int InnerProductPlan<T>::mod_count() const { return p_->M; }
    template <typename T> bool InnerProductPlan<T>::owns_workspace() const { return p_->owns; }

    template <typename T>
    void InnerProductPlan<T>::constants(const Modulus<T>* moduli_host, int mod_count,
                                        const InnerProductConstants<T>& out)
    {
        const IpHostConsts h = ip_derive<T>(moduli_host, mod_count);
        auto copy = [](const std::vector<std::uint64_t>& v, T* dst) {
            if (dst == nullptr)
                throw std::invalid_argument("null pointer argument");
            for (size_t i = 0; i < v.size(); i++)
                dst[i] = static_cast<T>(v[i]);
        };
        copy(h.t1, out.pow_w);
        copy(h.t1p, out.pow_w_shoup);
        copy(h.t2, out.pow_2w);
        copy(h.t2p, out.pow_2w_shoup);
        copy(h.onep, out.one_shoup);
    }

    template <typename T>
    void InnerProductPlan<T>::reference(const Modulus<T>* moduli_host, int mod_count, const T* a_host,
                                        const T* key_host, T* out_host, int n_power, int digits, int components,
                                        int count, bool accumulate, int key_mod_count, const int* key_limbs_host)
    {
        const IpHostConsts h = ip_derive<T>(moduli_host, mod_count);
        const int M = mod_count, D = digits, C = components, KM = key_mod_count;
        unsigned char limbs[INNERPROD_MAX_MODULI];
        ip_check_call<T>(M, a_host, key_host, out_host, n_power, D, C, count, KM, key_limbs_host, limbs);
        const size_t n = size_t(1) << n_power;
        for (int c = 0; c < C; c++)
            for (int r = 0; r < count; r++)
                for (int m = 0; m < M; m++)
                {
                    const U128 q = h.q[m];
                    T* o = out_host + ((static_cast<size_t>(c) * count + r) * M + m) * n;
                    for (size_t j = 0; j < n; j++)
                    {
                        U128 s = accumulate ? static_cast<U128>(o[j]) % q : 0;
                        for (int d = 0; d < D; d++)
                        {
                            const U128 x = a_host[((static_cast<size_t>(d) * count + r) * M + m) * n + j];
                            const U128 y = key_host[((static_cast<size_t>(d) * C + c) * KM + limbs[m]) * n + j];
                            s = (s + (x % q) * (y % q)) % q;
                        }
                        o[j] = static_cast<T>(s);
                    }
                }
    }

    template class InnerProductPlan<Data32>;
    template class InnerProductPlan<Data64>;
} // namespace gpuntt
