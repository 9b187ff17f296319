// c_api.cpp -- extern "C" boundary (include/gpuntt_c.h) over the C++ template API.
#include <algorithm>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpuntt/ntt_4step/ntt_4step.cuh"
#include "gpuntt/ntt_merge/galois.cuh"
#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/base_conversion.cuh"
#include "gpuntt/rns/bfv_encode.cuh"
#include "gpuntt/rns/bfv_multiply.cuh"
#include "gpuntt/rns/inner_product.cuh"
#include "gpuntt/rns/key_switch.cuh"
#include "gpuntt/rns/sampling.cuh"
#include "gpuntt_c.h"
#include "hoisted_rotation_internal.hpp"
#include "test_hooks.h"

namespace gpuntt
{
    namespace host
    {
        // prep.hip (diagnostic): the preparation kernels' normalised reciprocal of every q[i]
        template <typename T> void debug_recip_norm(const T* q, T* out, unsigned long long count, hipStream_t stream);
        // prep.hip: test hooks (csrc/test_hooks.h)
        bool set_test_hook(const char* name, const char* value);
        void launch_log_start();
        size_t launch_log_take(std::string& out, size_t capacity);
        unsigned long long alloc_count();
        void scratch_stats(unsigned long long out[6]);
        unsigned long long contig_p4_launches();
        unsigned long long premul_launches();
    } // namespace host
} // namespace gpuntt

using namespace gpuntt;

namespace
{
    thread_local std::string g_last_error;

    template <typename F> int guarded(F&& f)
    {
        try
        {
            f();
            return GPUNTT_OK;
        }
        catch (const std::invalid_argument& e)
        {
            g_last_error = e.what();
            return GPUNTT_ERR_INVALID_ARGUMENT;
        }
        catch (const HipException& e)
        {
            g_last_error = e.what();
            return GPUNTT_ERR_HIP;
        }
        catch (const std::exception& e)
        {
            g_last_error = e.what();
            return GPUNTT_ERR_UNKNOWN;
        }
    }

    // device / host pointer arguments of the C entry points must not be NULL (the C++ templates,
    // like the reference's, do not check)
    inline int need(std::initializer_list<const void*> ptrs)
    {
        for (const void* p : ptrs)
            if (p == nullptr)
            {
                g_last_error = "null pointer argument";
                return GPUNTT_ERR_INVALID_ARGUMENT;
            }
        return GPUNTT_OK;
    }
#define GPUNTT_NEED(...)                                                                          \
    if (int rc_ = need({__VA_ARGS__}))                                                            \
        return rc_;

    template <typename T, typename CM> Modulus<T> to_mod(const CM& m)
    {
        Modulus<T> r;
        r.value = m.value;
        r.bit = m.bit;
        r.mu = m.mu;
        return r;
    }

    template <typename T, typename CM>
    int ntt_single(const void* in, T* out, const T* roots, CM modulus, int n_power, int layout,
                   int poly, int input_signed, void* stream, int batch)
    {
        using S = typename std::make_signed<T>::type;
        return guarded([&] {
            ntt_configuration<T> cfg = {n_power,
                                        FORWARD,
                                        static_cast<NTTLayout>(layout),
                                        static_cast<ReductionPolynomial>(poly),
                                        false,
                                        0,
                                        static_cast<hipStream_t>(stream)};
            if (input_signed)
                GPU_NTT<S>(static_cast<S*>(const_cast<void*>(in)), out, const_cast<T*>(roots),
                           to_mod<T>(modulus), cfg, batch);
            else
                GPU_NTT<T>(static_cast<T*>(const_cast<void*>(in)), out, const_cast<T*>(roots),
                           to_mod<T>(modulus), cfg, batch);
        });
    }

    template <typename T, typename CM>
    int intt_single(const T* in, void* out, const T* roots, CM modulus, int n_power, int layout,
                    int poly, T mod_inverse, int output_signed, void* stream, int batch)
    {
        using S = typename std::make_signed<T>::type;
        return guarded([&] {
            ntt_configuration<T> cfg = {n_power,
                                        INVERSE,
                                        static_cast<NTTLayout>(layout),
                                        static_cast<ReductionPolynomial>(poly),
                                        false,
                                        mod_inverse,
                                        static_cast<hipStream_t>(stream)};
            if (output_signed)
                GPU_INTT<S>(const_cast<T*>(in), static_cast<S*>(out), const_cast<T*>(roots),
                            to_mod<T>(modulus), cfg, batch);
            else
                GPU_INTT<T>(const_cast<T*>(in), static_cast<T*>(out), const_cast<T*>(roots),
                            to_mod<T>(modulus), cfg, batch);
        });
    }

    template <typename T, typename CM>
    int ntt_rns(const void* in, T* out, const T* roots, const CM* modulus, int n_power, int layout,
                int poly, int input_signed, void* stream, int batch, int mod_count)
    {
        using S = typename std::make_signed<T>::type;
        static_assert(sizeof(CM) == sizeof(Modulus<T>), "C and C++ modulus layouts differ");
        return guarded([&] {
            ntt_rns_configuration<T> cfg = {n_power,
                                            FORWARD,
                                            static_cast<NTTLayout>(layout),
                                            static_cast<ReductionPolynomial>(poly),
                                            false,
                                            nullptr,
                                            static_cast<hipStream_t>(stream)};
            auto* mods = reinterpret_cast<Modulus<T>*>(const_cast<CM*>(modulus));
            if (input_signed)
                GPU_NTT<S>(static_cast<S*>(const_cast<void*>(in)), out, const_cast<T*>(roots), mods,
                           cfg, batch, mod_count);
            else
                GPU_NTT<T>(static_cast<T*>(const_cast<void*>(in)), out, const_cast<T*>(roots), mods,
                           cfg, batch, mod_count);
        });
    }

    template <typename T, typename CM>
    int intt_rns(const T* in, void* out, const T* roots, const CM* modulus, int n_power, int layout,
                 int poly, const T* mod_inverse, int output_signed, void* stream, int batch,
                 int mod_count)
    {
        using S = typename std::make_signed<T>::type;
        return guarded([&] {
            ntt_rns_configuration<T> cfg = {n_power,
                                            INVERSE,
                                            static_cast<NTTLayout>(layout),
                                            static_cast<ReductionPolynomial>(poly),
                                            false,
                                            const_cast<T*>(mod_inverse),
                                            static_cast<hipStream_t>(stream)};
            auto* mods = reinterpret_cast<Modulus<T>*>(const_cast<CM*>(modulus));
            if (output_signed)
                GPU_INTT<S>(const_cast<T*>(in), static_cast<S*>(out), const_cast<T*>(roots), mods,
                            cfg, batch, mod_count);
            else
                GPU_INTT<T>(const_cast<T*>(in), static_cast<T*>(out), const_cast<T*>(roots), mods,
                            cfg, batch, mod_count);
        });
    }

    template <typename T, typename CM>
    int polymul_single(T* a, T* b, T* out, const T* fwd, const T* inv, CM modulus, int n_power,
                       int reduction_poly, T mod_inverse, void* stream, int batch)
    {
        return guarded([&] {
            ntt_configuration<T> cfg = {n_power, FORWARD, PerPolynomial,
                                        static_cast<ReductionPolynomial>(reduction_poly), false, mod_inverse,
                                        static_cast<hipStream_t>(stream)};
            GPU_PolyMul<T>(a, b, out, const_cast<T*>(fwd), const_cast<T*>(inv), to_mod<T>(modulus), cfg, batch);
        });
    }
    template <typename T, typename CM>
    int polymul_rns(T* a, T* b, T* out, const T* fwd, const T* inv, const CM* modulus, int n_power,
                    int reduction_poly, const T* mod_inverse, void* stream, int batch, int mod_count)
    {
        return guarded([&] {
            ntt_rns_configuration<T> cfg = {n_power, FORWARD, PerPolynomial,
                                            static_cast<ReductionPolynomial>(reduction_poly), false,
                                            const_cast<T*>(mod_inverse), static_cast<hipStream_t>(stream)};
            GPU_PolyMul<T>(a, b, out, const_cast<T*>(fwd), const_cast<T*>(inv),
                           reinterpret_cast<Modulus<T>*>(const_cast<CM*>(modulus)), cfg, batch, mod_count);
        });
    }

    template <typename T>
    int automorphism_ntt(const T* in, T* out, const uint32_t* elts, int count, int n_power, int reduction_poly,
                         void* stream, int batch)
    {
        return guarded([&] {
            GPU_Automorphism_NTT<T>(in, out, elts, count, n_power, static_cast<ReductionPolynomial>(reduction_poly),
                                    batch, static_cast<hipStream_t>(stream));
        });
    }
    template <typename T, typename CM>
    int automorphism_single(const T* in, T* out, const uint32_t* elts, int count, CM modulus, int n_power,
                            int reduction_poly, void* stream, int batch)
    {
        return guarded([&] {
            GPU_Automorphism<T>(in, out, elts, count, to_mod<T>(modulus), n_power,
                                static_cast<ReductionPolynomial>(reduction_poly), batch,
                                static_cast<hipStream_t>(stream));
        });
    }
    template <typename T, typename CM>
    int automorphism_rns(const T* in, T* out, const uint32_t* elts, int count, const CM* modulus, int n_power,
                         int reduction_poly, void* stream, int batch, int mod_count)
    {
        return guarded([&] {
            GPU_Automorphism<T>(in, out, elts, count, reinterpret_cast<const Modulus<T>*>(modulus), mod_count, n_power,
                                static_cast<ReductionPolynomial>(reduction_poly), batch,
                                static_cast<hipStream_t>(stream));
        });
    }

    template <typename T, typename CM>
    int fourstep_single(const T* in, T* out, const T* t1, const T* t2, const T* w, CM modulus,
                        int n_power, int ntt_type, T mod_inverse, void* stream, int batch)
    {
        return guarded([&] {
            ntt4step_configuration<T> cfg = {n_power, static_cast<type>(ntt_type), mod_inverse,
                                             static_cast<hipStream_t>(stream)};
            GPU_4STEP_NTT<T>(const_cast<T*>(in), out, const_cast<T*>(t1), const_cast<T*>(t2),
                             const_cast<T*>(w), to_mod<T>(modulus), cfg, batch);
        });
    }

    template <typename T, typename CM>
    int fourstep_natural(T* in, T* out, const T* t1, const T* t2, const T* w, CM modulus, int n_power,
                         int ntt_type, T mod_inverse, void* stream, int batch)
    {
        return guarded([&] {
            ntt4step_configuration<T> cfg = {n_power, static_cast<type>(ntt_type), mod_inverse,
                                             static_cast<hipStream_t>(stream)};
            GPU_4STEP_NTT_NaturalOrder<T>(in, out, const_cast<T*>(t1), const_cast<T*>(t2), const_cast<T*>(w),
                                          to_mod<T>(modulus), cfg, batch);
        });
    }

    template <typename T, typename CM>
    int fourstep_rns(const T* in, T* out, const T* t1, const T* t2, const T* w, const CM* modulus,
                     int n_power, int ntt_type, const T* mod_inverse, void* stream, int batch,
                     int mod_count)
    {
        return guarded([&] {
            ntt4step_rns_configuration<T> cfg = {n_power, static_cast<type>(ntt_type),
                                                 const_cast<T*>(mod_inverse),
                                                 static_cast<hipStream_t>(stream)};
            GPU_4STEP_NTT<T>(const_cast<T*>(in), out, const_cast<T*>(t1), const_cast<T*>(t2),
                             const_cast<T*>(w),
                             reinterpret_cast<Modulus<T>*>(const_cast<CM*>(modulus)), cfg, batch,
                             mod_count);
        });
    }

    template <typename T, typename CM>
    int ordered(bool poly_ordered, const T* in, T* out, const T* roots, const CM* modulus, int n_power,
                int ntt_type, int poly, const T* mod_inverse, void* stream, int batch, int mod_count,
                const int* order)
    {
        return guarded([&] {
            ntt_rns_configuration<T> cfg = {n_power,
                                            static_cast<type>(ntt_type),
                                            PerPolynomial,
                                            static_cast<ReductionPolynomial>(poly),
                                            false,
                                            const_cast<T*>(mod_inverse),
                                            static_cast<hipStream_t>(stream)};
            auto* mods = reinterpret_cast<Modulus<T>*>(const_cast<CM*>(modulus));
            if (poly_ordered)
                GPU_NTT_Poly_Ordered<T>(const_cast<T*>(in), out, const_cast<T*>(roots), mods, cfg, batch,
                                        mod_count, const_cast<int*>(order));
            else
                GPU_NTT_Modulus_Ordered<T>(const_cast<T*>(in), out, const_cast<T*>(roots), mods, cfg, batch,
                                           mod_count, const_cast<int*>(order));
        });
    }

    template <typename T>
    int merge_params(int logn, int poly, const T* factors, uint64_t* info, T* fwd, T* inv)
    {
        return guarded([&] {
            if (poly != GPUNTT_X_N_PLUS && poly != GPUNTT_X_N_MINUS)
                throw std::invalid_argument("Invalid reduction_poly!");
            const auto rp = static_cast<ReductionPolynomial>(poly);
            NTTParameters<T> p = factors ? NTTParameters<T>(logn,
                                                            NTTFactors<T>(Modulus<T>(factors[0]),
                                                                          factors[1], factors[2]),
                                                            rp)
                                         : NTTParameters<T>(logn, rp);
            if (info)
            {
                info[0] = p.modulus.value;
                info[1] = p.modulus.bit;
                info[2] = p.modulus.mu;
                info[3] = p.omega;
                info[4] = p.psi;
                info[5] = p.n_inv;
                info[6] = p.root_of_unity_size;
                info[7] = p.n;
            }
            if (fwd)
            {
                auto t = p.gpu_root_of_unity_table_generator(p.forward_root_of_unity_table);
                std::memcpy(fwd, t.data(), t.size() * sizeof(T));
            }
            if (inv)
            {
                auto t = p.gpu_root_of_unity_table_generator(p.inverse_root_of_unity_table);
                std::memcpy(inv, t.data(), t.size() * sizeof(T));
            }
        });
    }

    template <typename T>
    int fourstep_params(int logn, int inverse, uint64_t* info, T* t1, T* t2, T* w)
    {
        return guarded([&] {
            NTTParameters4Step<T> p(logn, ReductionPolynomial::X_N_minus);
            if (info)
            {
                info[0] = p.modulus.value;
                info[1] = p.modulus.bit;
                info[2] = p.modulus.mu;
                info[3] = p.omega;
                info[4] = p.psi;
                info[5] = p.n_inv;
                info[6] = p.n1;
                info[7] = p.n2;
                info[8] = p.n;
            }
            if (t1)
            {
                auto t = p.gpu_root_of_unity_table_generator(
                    inverse ? p.n1_based_inverse_root_of_unity_table : p.n1_based_root_of_unity_table);
                std::memcpy(t1, t.data(), t.size() * sizeof(T));
            }
            if (t2)
            {
                auto t = p.gpu_root_of_unity_table_generator(
                    inverse ? p.n2_based_inverse_root_of_unity_table : p.n2_based_root_of_unity_table);
                std::memcpy(t2, t.data(), t.size() * sizeof(T));
            }
            if (w)
            {
                const auto& t = inverse ? p.W_inverse_root_of_unity_table : p.W_root_of_unity_table;
                std::memcpy(w, t.data(), t.size() * sizeof(T));
            }
        });
    }
} // namespace

namespace
{
    // OPERATOR_GPU<T> applied elementwise (diagnostic entry point: the public device class on real hardware)
    template <typename T>
    __global__ __launch_bounds__(256) void operator_gpu_apply(int op, const T* a, const T* b, T* out, Modulus<T> m,
                                                              unsigned long long count)
    {
        using S = typename std::make_signed<T>::type;
        for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < count;
             i += static_cast<unsigned long long>(gridDim.x) * 256ull)
        {
            const T x = a[i];
            const T y = (b != nullptr) ? b[i] : T(0);
            T r = 0;
            switch (op)
            {
                case 0: r = OPERATOR_GPU<T>::add(x, y, m); break;
                case 1: r = OPERATOR_GPU<T>::sub(x, y, m); break;
                case 2: r = OPERATOR_GPU<T>::mult(x, y, m); break;
                case 3: r = OPERATOR_GPU<T>::reduce(x, m); break;
                case 4: r = OPERATOR_GPU<T>::reduce(static_cast<S>(x), m); break;
                default: r = static_cast<T>(OPERATOR_GPU<T>::centered_reduction(x, m)); break;
            }
            out[i] = r;
        }
    }
    template <typename T, typename CM>
    int operator_gpu(int op, const T* a, const T* b, T* out, const CM& cm, uint64_t count, void* stream)
    {
        return guarded([&] {
            if (op < 0 || op > 5)
                throw std::invalid_argument("Invalid operator!");
            if (count == 0)
                return;
            unsigned long long blocks = (count + 255) / 256;
            if (blocks > 65536)
                blocks = 65536;
            hipLaunchKernelGGL((operator_gpu_apply<T>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                               static_cast<hipStream_t>(stream), op, a, b, out, to_mod<T>(cm), count);
            GPUNTT_HIP_CHECK(hipGetLastError());
        });
    }

    // the public device butterflies CooleyTukeyUnit / GentlemanSandeUnit (gpuntt/ntt_merge/ntt.cuh) applied pairwise
    template <typename T>
    __global__ __launch_bounds__(256) void butterfly_unit_apply(int gs, T* u, T* v, const T* roots, Modulus<T> m,
                                                                unsigned long long count)
    {
        for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < count;
             i += static_cast<unsigned long long>(gridDim.x) * 256ull)
        {
            T U = u[i], V = v[i];
            if (gs)
                GentlemanSandeUnit<T>(U, V, roots[i], m);
            else
                CooleyTukeyUnit<T>(U, V, roots[i], m);
            u[i] = U;
            v[i] = V;
        }
    }
    template <typename T, typename CM>
    int butterfly_unit(int gs, T* u, T* v, const T* roots, const CM& cm, uint64_t count, void* stream)
    {
        return guarded([&] {
            if (count == 0)
                return;
            unsigned long long blocks = (count + 255) / 256;
            if (blocks > 65536)
                blocks = 65536;
            hipLaunchKernelGGL((butterfly_unit_apply<T>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                               static_cast<hipStream_t>(stream), gs, u, v, roots, to_mod<T>(cm), count);
            GPUNTT_HIP_CHECK(hipGetLastError());
        });
    }

    template <typename T, typename CM>
    int plan_create(gpuntt_plan** plan, const T* table, const CM* moduli, int mod_count, int n_power, int poly,
                    int ntt_type, const T* ninv, int batch_hint, void* ws, void* stream)
    {
        return guarded([&] {
            if (plan == nullptr || moduli == nullptr || mod_count <= 0)
                throw std::invalid_argument("Invalid mod_count!");
            std::vector<Modulus<T>> ms;
            for (int i = 0; i < mod_count; i++)
                ms.push_back(to_mod<T>(moduli[i]));
            auto* p = new NTTPlan<T>(table, ms.data(), mod_count, n_power, static_cast<ReductionPolynomial>(poly),
                                     static_cast<type>(ntt_type), ninv, batch_hint,
                                     static_cast<hipStream_t>(stream), ws);
            *plan = reinterpret_cast<gpuntt_plan*>(p);
        });
    }

    template <typename T, typename CM> std::vector<Modulus<T>> to_mods(const CM* moduli, int count, const char* what)
    {
        if (moduli == nullptr || count < 1 || count > BASECONV_MAX_COUNT)
            throw std::invalid_argument(what);
        std::vector<Modulus<T>> ms;
        for (int i = 0; i < count; i++)
            ms.push_back(to_mod<T>(moduli[i]));
        return ms;
    }
} // namespace

extern "C"
{
    const char* gpuntt_last_error(void) { return g_last_error.c_str(); }
    int gpuntt_release_workspaces(void)
    {
        return guarded([] { GPU_NTT_ReleaseWorkspaces(); });
    }
    int gpuntt_set_option(const char* name, const char* value)
    {
        return guarded([&] {
            if (!GPU_NTT_SetOption(name, value))
                throw std::invalid_argument("Unknown option or value!");
        });
    }
    int gpuntt_version(void) { return 101; }

    // ---- test hooks (csrc/test_hooks.h; not declared by the public headers) ----------------------------------------
    int gpuntt_test_set_hook(const char* name, const char* value)
    {
        return guarded([&] {
            if (!host::set_test_hook(name, value))
                throw std::invalid_argument("Unknown option or value!");
        });
    }
    int gpuntt_test_launch_log_start(void)
    {
        return guarded([] { host::launch_log_start(); });
    }
    int gpuntt_test_launch_log_take(char* buf, int capacity)
    {
        // never a cut list: a buffer too small for the names and their terminator gets an empty string, and the log is
        // kept for a second take with the capacity returned here
        std::string s;
        const size_t room = (buf != nullptr && capacity > 0) ? static_cast<size_t>(capacity - 1) : 0;
        const size_t need = host::launch_log_take(s, room);
        if (buf != nullptr && capacity > 0)
        {
            std::memcpy(buf, s.data(), s.size());
            buf[s.size()] = '\0';
        }
        return static_cast<int>(need) + 1;
    }
    unsigned long long gpuntt_test_alloc_count(void) { return host::alloc_count(); }

    int gpuntt_test_scratch_stats(unsigned long long out[6])
    {
        return guarded([&] { host::scratch_stats(out); });
    }
    unsigned long long gpuntt_test_contig_p4_launches(void) { return host::contig_p4_launches(); }
    unsigned long long gpuntt_test_premul_launches(void) { return host::premul_launches(); }
    int gpuntt_test_keyswitch_hoist_chunk(int word_bytes, int digits, int n_power)
    {
        if ((word_bytes != 4 && word_bytes != 8) || digits < 1 || digits > INNERPROD_MAX_DIGITS || n_power < 1 ||
            n_power > 28)
            return -1;
        return host::hoist_chunk_log(static_cast<size_t>(word_bytes), digits, n_power, host::HOIST_LOG_MAX);
    }
    int gpuntt_test_keyswitch_hoist_sum_chunk(int word_bytes, int digits, int n_power)
    {
        if ((word_bytes != 4 && word_bytes != 8) || digits < 1 || digits > INNERPROD_MAX_DIGITS || n_power < 1 ||
            n_power > 28)
            return -1;
        return host::hoist_chunk_log(static_cast<size_t>(word_bytes), digits, n_power, host::HOIST_SUM_LOG_MAX);
    }
    int gpuntt_test_bsgs_sum_shape(int word_bytes, int n1, int n_power, int aligned, int* V, unsigned* nt)
    {
        if ((word_bytes != 4 && word_bytes != 8) || n1 < 1 || n1 > KEYSWITCH_MAX_STEPS || n_power < 1 || n_power > 28 ||
            V == nullptr || nt == nullptr)
            return -1;
        host::bsgs_sum_shape(static_cast<size_t>(word_bytes), n1, n_power, aligned != 0, *V, *nt);
        return 0;
    }

    int gpuntt_philox4x32_10(const uint32_t* ctr4_host, const uint32_t* key2_host, uint32_t* out4_host)
    {
        GPUNTT_NEED(ctr4_host, key2_host, out4_host)
        return guarded([&] { reference_philox(ctr4_host, key2_host, out4_host); });
    }
    int gpuntt_sample_small(int32_t* out, int polys, int n_power, int distribution, uint64_t seed, uint32_t stream_id,
                            void* stream)
    {
        GPUNTT_NEED(out)
        return guarded([&] {
            sample_small(out, polys, n_power, static_cast<SmallDistribution>(distribution), seed, stream_id,
                         static_cast<hipStream_t>(stream));
        });
    }
    int gpuntt_sample_reference_small(int32_t* out_host, int polys, int n_power, int distribution, uint64_t seed,
                                      uint32_t stream_id)
    {
        GPUNTT_NEED(out_host)
        return guarded([&] {
            reference_sample_small(out_host, polys, n_power, static_cast<SmallDistribution>(distribution), seed,
                                   stream_id);
        });
    }
    int gpuntt_galois_element_u32(int steps, int n_power, int conjugation, uint32_t* elt_host)
    {
        GPUNTT_NEED(elt_host)
        return guarded([&] {
            *elt_host = conjugation ? GaloisElementForConjugation(n_power) : GaloisElementForRotation(steps, n_power);
        });
    }
    int gpuntt_automorphism_index_map(int n_power, uint32_t galois_elt, int reduction_poly, int domain,
                                      uint32_t* map_host)
    {
        GPUNTT_NEED(map_host)
        return guarded([&] {
            if (n_power <= 0 || n_power >= 29)
                throw std::invalid_argument("Invalid n_power range!");
            if (reduction_poly != GPUNTT_X_N_PLUS && reduction_poly != GPUNTT_X_N_MINUS)
                throw std::invalid_argument("Invalid reduction_poly!");
            if (domain != GPUNTT_DOMAIN_NTT && domain != GPUNTT_DOMAIN_COEFFICIENT)
                throw std::invalid_argument("Invalid domain!");
            const bool neg = reduction_poly == GPUNTT_X_N_PLUS;
            const uint32_t mask = neg ? (2u << n_power) - 1u : (1u << n_power) - 1u;
            const uint32_t k = galois_elt & mask;
            if ((k & 1u) == 0u)
                throw std::invalid_argument("Invalid Galois element (must be odd)!");
            const uint32_t n = 1u << n_power;
            if (domain == GPUNTT_DOMAIN_NTT)
                for (uint32_t i = 0; i < n; i++)
                    map_host[i] = galois_ntt_source(i, k, n_power, neg);
            else
                for (uint32_t i = 0; i < n; i++)
                    map_host[i] = galois_coeff_source(i, galois_inverse(k) & mask, n_power, neg);
        });
    }

    int gpuntt_bfv_slot_maps(int n_power, uint32_t* to_position_host, uint32_t* to_slot_host)
    {
        return guarded([&] { bfv_slot_maps(n_power, to_position_host, to_slot_host); });
    }

    int gpuntt_modulus_u32(uint32_t q, gpuntt_modulus32* out)
    {
        return guarded([&] {
            if (!out || q < 2)
                throw std::invalid_argument("Invalid modulus!");
            Modulus<Data32> m(q);
            out->value = m.value;
            out->bit = m.bit;
            out->mu = m.mu;
        });
    }
    int gpuntt_modulus_u64(uint64_t q, gpuntt_modulus64* out)
    {
        return guarded([&] {
            if (!out || q < 2)
                throw std::invalid_argument("Invalid modulus!");
            Modulus<Data64> m(q);
            out->value = m.value;
            out->bit = m.bit;
            out->mu = m.mu;
        });
    }

#define GPUNTT_C_API(S, T, CM)                                                                    \
    int gpuntt_ntt_##S(const void* in, T* out, const T* roots, CM modulus, int n_power,           \
                       int ntt_layout, int reduction_poly, int input_signed, void* stream,        \
                       int batch_size)                                                            \
    {                                                                                             \
        GPUNTT_NEED(in, out, roots)                                                                      \
        return ntt_single<T>(in, out, roots, modulus, n_power, ntt_layout, reduction_poly,        \
                             input_signed, stream, batch_size);                                   \
    }                                                                                             \
    int gpuntt_intt_##S(const T* in, void* out, const T* inverse_roots, CM modulus, int n_power,  \
                        int ntt_layout, int reduction_poly, T mod_inverse, int output_signed,     \
                        void* stream, int batch_size)                                             \
    {                                                                                             \
        GPUNTT_NEED(in, out, inverse_roots)                                                              \
        return intt_single<T>(in, out, inverse_roots, modulus, n_power, ntt_layout,               \
                              reduction_poly, mod_inverse, output_signed, stream, batch_size);    \
    }                                                                                             \
    int gpuntt_ntt_rns_##S(const void* in, T* out, const T* roots, const CM* modulus,             \
                           int n_power, int ntt_layout, int reduction_poly, int input_signed,     \
                           void* stream, int batch_size, int mod_count)                           \
    {                                                                                             \
        GPUNTT_NEED(in, out, roots, modulus)                                                             \
        return ntt_rns<T>(in, out, roots, modulus, n_power, ntt_layout, reduction_poly,           \
                          input_signed, stream, batch_size, mod_count);                           \
    }                                                                                             \
    int gpuntt_intt_rns_##S(const T* in, void* out, const T* inverse_roots, const CM* modulus,    \
                            int n_power, int ntt_layout, int reduction_poly,                      \
                            const T* mod_inverse, int output_signed, void* stream,                \
                            int batch_size, int mod_count)                                        \
    {                                                                                             \
        GPUNTT_NEED(in, out, inverse_roots, modulus, mod_inverse)                                        \
        return intt_rns<T>(in, out, inverse_roots, modulus, n_power, ntt_layout, reduction_poly,  \
                           mod_inverse, output_signed, stream, batch_size, mod_count);            \
    }                                                                                             \
    int gpuntt_ntt_modulus_ordered_##S(const T* in, T* out, const T* roots, const CM* modulus,    \
                                       int n_power, int ntt_type, int reduction_poly,             \
                                       const T* mod_inverse, void* stream, int batch_size,        \
                                       int mod_count, const int* order)                           \
    {                                                                                             \
        GPUNTT_NEED(in, out, roots, modulus, order)                                                      \
        return ordered<T>(false, in, out, roots, modulus, n_power, ntt_type, reduction_poly,      \
                          mod_inverse, stream, batch_size, mod_count, order);                     \
    }                                                                                             \
    int gpuntt_ntt_poly_ordered_##S(const T* in, T* out, const T* roots, const CM* modulus,       \
                                    int n_power, int ntt_type, int reduction_poly,                \
                                    const T* mod_inverse, void* stream, int batch_size,           \
                                    int mod_count, const int* order)                              \
    {                                                                                             \
        GPUNTT_NEED(in, out, roots, modulus, order)                                                      \
        return ordered<T>(true, in, out, roots, modulus, n_power, ntt_type, reduction_poly,       \
                          mod_inverse, stream, batch_size, mod_count, order);                     \
    }                                                                                             \
    int gpuntt_4step_##S(const T* in, T* out, const T* n1_table, const T* n2_table,               \
                         const T* w_table, CM modulus, int n_power, int ntt_type, T mod_inverse,  \
                         void* stream, int batch_size)                                            \
    {                                                                                             \
        GPUNTT_NEED(in, out, n1_table, n2_table, w_table)                                                \
        return fourstep_single<T>(in, out, n1_table, n2_table, w_table, modulus, n_power,         \
                                  ntt_type, mod_inverse, stream, batch_size);                     \
    }                                                                                             \
    int gpuntt_polymul_##S(T* a, T* b, T* out, const T* forward_table, const T* inverse_table,     \
                           CM modulus, int n_power, int reduction_poly, T mod_inverse, void* stream, \
                           int batch_size)                                                          \
    {                                                                                             \
        GPUNTT_NEED(a, b, out, forward_table, inverse_table)                                             \
        return polymul_single<T>(a, b, out, forward_table, inverse_table, modulus, n_power,        \
                                 reduction_poly, mod_inverse, stream, batch_size);                \
    }                                                                                             \
    int gpuntt_polymul_rns_##S(T* a, T* b, T* out, const T* forward_table, const T* inverse_table, \
                               const CM* modulus, int n_power, int reduction_poly,                 \
                               const T* mod_inverse, void* stream, int batch_size, int mod_count)  \
    {                                                                                             \
        GPUNTT_NEED(a, b, out, forward_table, inverse_table, modulus, mod_inverse)                       \
        return polymul_rns<T>(a, b, out, forward_table, inverse_table, modulus, n_power,           \
                              reduction_poly, mod_inverse, stream, batch_size, mod_count);        \
    }                                                                                             \
    int gpuntt_automorphism_ntt_##S(const T* in, T* out, const uint32_t* galois_elts_host, int galois_count,      \
                                    int n_power, int reduction_poly, void* stream, int batch_size)                \
    {                                                                                             \
        GPUNTT_NEED(in, out, galois_elts_host)                                                    \
        return automorphism_ntt<T>(in, out, galois_elts_host, galois_count, n_power, reduction_poly, stream,      \
                                   batch_size);                                                   \
    }                                                                                             \
    int gpuntt_automorphism_##S(const T* in, T* out, const uint32_t* galois_elts_host, int galois_count,          \
                                CM modulus, int n_power, int reduction_poly, void* stream, int batch_size)        \
    {                                                                                             \
        GPUNTT_NEED(in, out, galois_elts_host)                                                    \
        return automorphism_single<T>(in, out, galois_elts_host, galois_count, modulus, n_power, reduction_poly,  \
                                      stream, batch_size);                                        \
    }                                                                                             \
    int gpuntt_automorphism_rns_##S(const T* in, T* out, const uint32_t* galois_elts_host, int galois_count,      \
                                    const CM* modulus, int n_power, int reduction_poly, void* stream,             \
                                    int batch_size, int mod_count)                                \
    {                                                                                             \
        GPUNTT_NEED(in, out, galois_elts_host, modulus)                                           \
        return automorphism_rns<T>(in, out, galois_elts_host, galois_count, modulus, n_power, reduction_poly,     \
                                   stream, batch_size, mod_count);                                \
    }                                                                                             \
    int gpuntt_4step_natural_##S(T* in_scratch, T* out, const T* n1_table, const T* n2_table,      \
                                 const T* w_table, CM modulus, int n_power, int ntt_type,          \
                                 T mod_inverse, void* stream, int batch_size)                      \
    {                                                                                             \
        GPUNTT_NEED(in_scratch, out, n1_table, n2_table, w_table)                                        \
        return fourstep_natural<T>(in_scratch, out, n1_table, n2_table, w_table, modulus, n_power, \
                                   ntt_type, mod_inverse, stream, batch_size);                    \
    }                                                                                             \
    int gpuntt_4step_rns_##S(const T* in, T* out, const T* n1_table, const T* n2_table,           \
                             const T* w_table, const CM* modulus, int n_power, int ntt_type,      \
                             const T* mod_inverse, void* stream, int batch_size, int mod_count)   \
    {                                                                                             \
        GPUNTT_NEED(in, out, n1_table, n2_table, w_table, modulus)                                       \
        return fourstep_rns<T>(in, out, n1_table, n2_table, w_table, modulus, n_power, ntt_type,  \
                               mod_inverse, stream, batch_size, mod_count);                       \
    }                                                                                             \
    int gpuntt_transpose_##S(const T* in, T* out, int row, int col, int n_power, int batch_size)  \
    {                                                                                             \
        GPUNTT_NEED(in, out)                                                                             \
        return guarded(                                                                           \
            [&] { GPU_Transpose<T>(const_cast<T*>(in), out, row, col, n_power, batch_size); });   \
    }                                                                                             \
    int gpuntt_merge_params_##S(int logn, int reduction_poly, const T* factors_host,              \
                                uint64_t* info_host, T* forward_table_host,                       \
                                T* inverse_table_host)                                            \
    {                                                                                             \
        return merge_params<T>(logn, reduction_poly, factors_host, info_host,                     \
                               forward_table_host, inverse_table_host);                           \
    }                                                                                             \
    int gpuntt_4step_params_##S(int logn, int inverse, uint64_t* info_host, T* n1_table_host,     \
                                T* n2_table_host, T* w_table_host)                                \
    {                                                                                             \
        return fourstep_params<T>(logn, inverse, info_host, n1_table_host, n2_table_host,         \
                                  w_table_host);                                                  \
    }                                                                                             \
    int gpuntt_plan_workspace_bytes_##S(int n_power, int mod_count, uint64_t* bytes_host)         \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] { *bytes_host = NTTPlan<T>::workspace_bytes(n_power, mod_count); });    \
    }                                                                                             \
    int gpuntt_plan_create_##S(gpuntt_plan** plan_host, const T* table, const CM* moduli_host,    \
                               int mod_count, int n_power, int reduction_poly, int ntt_type,      \
                               const T* mod_inverse_host, int batch_hint, void* workspace_device, \
                               void* stream)                                                      \
    {                                                                                             \
        GPUNTT_NEED(plan_host, table, moduli_host)                                                \
        return plan_create<T>(plan_host, table, moduli_host, mod_count, n_power, reduction_poly,  \
                              ntt_type, mod_inverse_host, batch_hint, workspace_device, stream);  \
    }                                                                                             \
    int gpuntt_plan_execute_##S(const gpuntt_plan* plan, const void* in, void* out,               \
                                int batch_size, int io_signed, void* stream)                      \
    {                                                                                             \
        GPUNTT_NEED(plan, in, out)                                                                \
        return guarded([&] {                                                                      \
            reinterpret_cast<const NTTPlan<T>*>(plan)->execute(in, out, batch_size,               \
                                                               static_cast<hipStream_t>(stream),  \
                                                               io_signed != 0);                   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_plan_fast_path_##S(const gpuntt_plan* plan)                                        \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const NTTPlan<T>*>(plan)->fast_path() ? 1 : 0;                    \
    }                                                                                             \
    int gpuntt_plan_destroy_##S(gpuntt_plan* plan)                                                \
    {                                                                                             \
        return guarded([&] { delete reinterpret_cast<NTTPlan<T>*>(plan); });                      \
    }                                                                                             \
    int gpuntt_baseconv_plan_workspace_bytes_##S(int in_count, int out_count, uint64_t* bytes_host)               \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] { *bytes_host = BaseConvPlan<T>::workspace_bytes(in_count, out_count); });             \
    }                                                                                             \
    int gpuntt_baseconv_plan_create_##S(gpuntt_baseconv_plan** plan_host, const CM* in_moduli_host, int in_count,  \
                                        const CM* out_moduli_host, int out_count, void* workspace_device,         \
                                        void* stream)                                             \
    {                                                                                             \
        GPUNTT_NEED(plan_host)                                                                    \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(in_moduli_host, in_count, "Invalid in_count!");             \
            const auto ps = to_mods<T>(out_moduli_host, out_count, "Invalid out_count!");          \
            *plan_host = reinterpret_cast<gpuntt_baseconv_plan*>(new BaseConvPlan<T>(             \
                qs.data(), in_count, ps.data(), out_count, static_cast<hipStream_t>(stream), workspace_device));  \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_baseconv_plan_convert_##S(const gpuntt_baseconv_plan* plan, const T* in, T* out, int n_power,       \
                                         int count, int mode, void* stream)                       \
    {                                                                                             \
        GPUNTT_NEED(plan, in, out)                                                                \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BaseConvPlan<T>*>(plan)->convert(in, out, n_power, count,       \
                                                                    static_cast<BaseConvMode>(mode),              \
                                                                    static_cast<hipStream_t>(stream));            \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_baseconv_plan_convert_and_divide_##S(const gpuntt_baseconv_plan* plan, const T* in, const T* c,     \
                                                    T* out, int n_power, int count, int mode, void* stream)       \
    {                                                                                             \
        GPUNTT_NEED(plan, in, c, out)                                                             \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BaseConvPlan<T>*>(plan)->convert_and_divide(                   \
                in, c, out, n_power, count, static_cast<BaseConvMode>(mode), static_cast<hipStream_t>(stream));   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_baseconv_plan_owns_workspace_##S(const gpuntt_baseconv_plan* plan)                 \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const BaseConvPlan<T>*>(plan)->owns_workspace() ? 1 : 0;          \
    }                                                                                             \
    int gpuntt_baseconv_plan_destroy_##S(gpuntt_baseconv_plan* plan)                              \
    {                                                                                             \
        return guarded([&] { delete reinterpret_cast<BaseConvPlan<T>*>(plan); });                 \
    }                                                                                             \
    int gpuntt_baseconv_constants_##S(const CM* in_moduli_host, int in_count, const CM* out_moduli_host,          \
                                      int out_count, T* qhat_inv, T* qhat_inv_shoup, T* matrix, T* q_mod_p,       \
                                      T* q_inv_mod_p, T* recip, T* bit_length)                    \
    {                                                                                             \
        GPUNTT_NEED(qhat_inv, qhat_inv_shoup, matrix, q_mod_p, q_inv_mod_p, recip, bit_length)    \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(in_moduli_host, in_count, "Invalid in_count!");             \
            const auto ps = to_mods<T>(out_moduli_host, out_count, "Invalid out_count!");          \
            BaseConvPlan<T>::constants(qs.data(), in_count, ps.data(), out_count,                 \
                                       BaseConvConstants<T>{qhat_inv, qhat_inv_shoup, matrix, q_mod_p,            \
                                                            q_inv_mod_p, recip, bit_length});     \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_innerprod_plan_workspace_bytes_##S(int mod_count, uint64_t* bytes_host)            \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] { *bytes_host = InnerProductPlan<T>::workspace_bytes(mod_count); });    \
    }                                                                                             \
    int gpuntt_innerprod_plan_create_##S(gpuntt_innerprod_plan** plan_host, const CM* moduli_host, int mod_count,  \
                                         void* workspace_device, void* stream)                    \
    {                                                                                             \
        GPUNTT_NEED(plan_host)                                                                    \
        return guarded([&] {                                                                      \
            const auto ms = to_mods<T>(moduli_host, mod_count, "Invalid mod_count!");              \
            *plan_host = reinterpret_cast<gpuntt_innerprod_plan*>(new InnerProductPlan<T>(        \
                ms.data(), mod_count, static_cast<hipStream_t>(stream), workspace_device));       \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_innerprod_plan_execute_##S(const gpuntt_innerprod_plan* plan, const T* a, const T* key, T* out,     \
                                          int n_power, int digits, int components, int count, int accumulate,     \
                                          int key_mod_count, const int* key_limbs_host, void* stream)             \
    {                                                                                             \
        GPUNTT_NEED(plan, a, key, out)                                                            \
        return guarded([&] {                                                                      \
            reinterpret_cast<const InnerProductPlan<T>*>(plan)->multiply_accumulate(              \
                a, key, out, n_power, digits, components, count, accumulate != 0, key_mod_count, key_limbs_host,  \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_innerprod_plan_owns_workspace_##S(const gpuntt_innerprod_plan* plan)               \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const InnerProductPlan<T>*>(plan)->owns_workspace() ? 1 : 0;      \
    }                                                                                             \
    int gpuntt_innerprod_plan_destroy_##S(gpuntt_innerprod_plan* plan)                            \
    {                                                                                             \
        return guarded([&] { delete reinterpret_cast<InnerProductPlan<T>*>(plan); });             \
    }                                                                                             \
    int gpuntt_innerprod_constants_##S(const CM* moduli_host, int mod_count, T* pow_w, T* pow_w_shoup, T* pow_2w,  \
                                       T* pow_2w_shoup, T* one_shoup)                             \
    {                                                                                             \
        GPUNTT_NEED(pow_w, pow_w_shoup, pow_2w, pow_2w_shoup, one_shoup)                          \
        return guarded([&] {                                                                      \
            const auto ms = to_mods<T>(moduli_host, mod_count, "Invalid mod_count!");              \
            InnerProductPlan<T>::constants(                                                       \
                ms.data(), mod_count,                                                             \
                InnerProductConstants<T>{pow_w, pow_w_shoup, pow_2w, pow_2w_shoup, one_shoup});   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_innerprod_reference_##S(const CM* moduli_host, int mod_count, const T* a_host, const T* key_host,   \
                                       T* out_host, int n_power, int digits, int components, int count,           \
                                       int accumulate, int key_mod_count, const int* key_limbs_host)              \
    {                                                                                             \
        GPUNTT_NEED(a_host, key_host, out_host)                                                   \
        return guarded([&] {                                                                      \
            const auto ms = to_mods<T>(moduli_host, mod_count, "Invalid mod_count!");              \
            InnerProductPlan<T>::reference(ms.data(), mod_count, a_host, key_host, out_host, n_power, digits,     \
                                           components, count, accumulate != 0, key_mod_count, key_limbs_host);    \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_workspace_bytes_##S(int q_count, int p_count, int alpha, int n_power,               \
                                                  uint64_t* bytes_host)                           \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded(                                                                           \
            [&] { *bytes_host = KeySwitchPlan<T>::workspace_bytes(q_count, p_count, alpha, n_power); });          \
    }                                                                                             \
    int gpuntt_keyswitch_plan_scratch_bytes_##S(int q_count, int p_count, int alpha, int n_power, int count,      \
                                                int components, uint64_t* bytes_host)             \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] {                                                                      \
            *bytes_host = KeySwitchPlan<T>::scratch_bytes(q_count, p_count, alpha, n_power, count, components);   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_create_##S(gpuntt_keyswitch_plan** plan_host, const CM* q_moduli_host, int q_count, \
                                         const CM* p_moduli_host, int p_count, int alpha, int n_power,            \
                                         const T* forward_table, const T* inverse_table,          \
                                         const T* mod_inverse_host, int reduction_poly, int batch_hint,           \
                                         int key_mod_count, const int* key_limbs_host, void* workspace_device,    \
                                         void* stream)                                            \
    {                                                                                             \
        GPUNTT_NEED(plan_host)                                                                    \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto ps = to_mods<T>(p_moduli_host, p_count, "Invalid p_count!");                \
            if (reduction_poly != GPUNTT_X_N_PLUS && reduction_poly != GPUNTT_X_N_MINUS)          \
                throw std::invalid_argument("Invalid reduction_poly!");                           \
            *plan_host = reinterpret_cast<gpuntt_keyswitch_plan*>(new KeySwitchPlan<T>(           \
                qs.data(), q_count, ps.data(), p_count, alpha, n_power, forward_table, inverse_table,             \
                mod_inverse_host, static_cast<ReductionPolynomial>(reduction_poly), batch_hint, key_mod_count,    \
                key_limbs_host, static_cast<hipStream_t>(stream), workspace_device));             \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_mod_up_##S(const gpuntt_keyswitch_plan* plan, const T* in, T* a, int count,          \
                                         int mode, void* stream)                                  \
    {                                                                                             \
        GPUNTT_NEED(plan, in, a)                                                                  \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->mod_up(in, a, count, static_cast<BaseConvMode>(mode), \
                                                                    static_cast<hipStream_t>(stream));            \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_mod_down_##S(const gpuntt_keyswitch_plan* plan, const T* x, T* out, int stacks,      \
                                           void* stream)                                          \
    {                                                                                             \
        GPUNTT_NEED(plan, x, out)                                                                 \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->mod_down(x, out, stacks,              \
                                                                      static_cast<hipStream_t>(stream));          \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_mod_down_add_##S(const gpuntt_keyswitch_plan* plan, const T* x, const T* addend, \
                                               T* out, int stacks, void* stream)                  \
    {                                                                                             \
        GPUNTT_NEED(plan, x, addend, out)                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->mod_down_add(x, addend, out, stacks, \
                                                                          static_cast<hipStream_t>(stream)); \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_relinearize_##S(const gpuntt_keyswitch_plan* plan, const T* c01, const T* c2, \
                                              const T* key, T* out, int count, int input_ntt, int output_ntt, \
                                              void* scratch, void* stream)                        \
    {                                                                                             \
        GPUNTT_NEED(plan, c01, c2, key, out, scratch)                                             \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->relinearize(                         \
                c01, c2, key, out, count, input_ntt != 0, output_ntt != 0, scratch,               \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_decompose_##S(const gpuntt_keyswitch_plan* plan, const T* c_in, T* a, int count,     \
                                            int input_ntt, void* scratch, void* stream)           \
    {                                                                                             \
        GPUNTT_NEED(plan, c_in, a)                                                                \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->decompose(c_in, a, count, input_ntt != 0, scratch,   \
                                                                       static_cast<hipStream_t>(stream));         \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_switch_digits_##S(const gpuntt_keyswitch_plan* plan, const T* a, const T* key,       \
                                                T* out, int count, int components, int output_ntt, void* scratch,  \
                                                void* stream)                                     \
    {                                                                                             \
        GPUNTT_NEED(plan, a, key, out, scratch)                                                   \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->switch_digits(                       \
                a, key, out, count, components, output_ntt != 0, scratch, static_cast<hipStream_t>(stream));      \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_apply_##S(const gpuntt_keyswitch_plan* plan, const T* c_in, const T* key, T* out,    \
                                        int count, int components, int input_ntt, int output_ntt, void* scratch,  \
                                        void* stream)                                             \
    {                                                                                             \
        GPUNTT_NEED(plan, c_in, key, out, scratch)                                                \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->apply(c_in, key, out, count, components,              \
                                                                   input_ntt != 0, output_ntt != 0, scratch,      \
                                                                   static_cast<hipStream_t>(stream));             \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_hoisted_scratch_bytes_##S(int q_count, int p_count, int alpha, int n_power,         \
                                                        int count, int elements, uint64_t* bytes_host)            \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] {                                                                      \
            *bytes_host =                                                                         \
                KeySwitchPlan<T>::hoisted_scratch_bytes(q_count, p_count, alpha, n_power, count, elements);       \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_rotate_hoisted_##S(const gpuntt_keyswitch_plan* plan, const T* a, const T* c0,       \
                                                 const T* const* keys_host,                       \
                                                 const uint32_t* galois_elements_host, int elements, T* out,      \
                                                 int count, int output_ntt, void* scratch, void* stream)          \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->rotate_hoisted(                      \
                a, c0, keys_host, galois_elements_host, elements, out, count, output_ntt != 0, scratch,           \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_hoisted_sum_scratch_bytes_##S(int q_count, int p_count, int alpha, int n_power,     \
                                                            int count, uint64_t* bytes_host)       \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] {                                                                      \
            *bytes_host = KeySwitchPlan<T>::hoisted_sum_scratch_bytes(q_count, p_count, alpha, n_power, count);   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_rotate_hoisted_sum_##S(const gpuntt_keyswitch_plan* plan, const T* a, const T* c0,   \
                                                     const T* const* keys_host,                   \
                                                     const uint32_t* galois_elements_host,        \
                                                     const T* const* weights_host, int elements, T* out,          \
                                                     int count, int output_ntt, void* scratch, void* stream)      \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->rotate_hoisted_sum(                  \
                a, c0, keys_host, galois_elements_host, weights_host, elements, out, count, output_ntt != 0,      \
                scratch, static_cast<hipStream_t>(stream));                                       \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_multiply_relinearize_##S(const gpuntt_keyswitch_plan* plan, const T* x, const T* y,  \
                                                       const T* key, T* out, int count, int output_ntt,           \
                                                       void* scratch, void* stream)               \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->multiply_relinearize(                \
                x, y, key, out, count, output_ntt != 0, scratch, static_cast<hipStream_t>(stream));               \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_multiply_relinearize_sum_##S(const gpuntt_keyswitch_plan* plan,      \
                                                           const T* const* x_host, const T* const* y_host,        \
                                                           int terms, const T* key, T* out, int count,            \
                                                           int output_ntt, void* scratch, void* stream)           \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->multiply_relinearize_sum(            \
                x_host, y_host, terms, key, out, count, output_ntt != 0, scratch,                 \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_owns_workspace_##S(const gpuntt_keyswitch_plan* plan)               \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const KeySwitchPlan<T>*>(plan)->owns_workspace() ? 1 : 0;         \
    }                                                                                             \
    int gpuntt_sample_uniform_##S(T* out, const T* moduli_host, int mod_count, int n_power, int stacks,\
                                  uint64_t stack_stride_words, uint64_t seed, uint32_t stream_id, void* stream)\
    {                                                                                             \
        GPUNTT_NEED(out, moduli_host)                                                             \
        return guarded([&] {                                                                      \
            sample_uniform<T>(out, moduli_host, mod_count, n_power, stacks, stack_stride_words, seed, stream_id,\
                              static_cast<hipStream_t>(stream));                                  \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_sample_reference_uniform_##S(T* out_host, const T* moduli_host, int mod_count, int n_power,\
                                            int stacks, uint64_t stack_stride_words, uint64_t seed,\
                                            uint32_t stream_id, int max_candidates)               \
    {                                                                                             \
        GPUNTT_NEED(out_host, moduli_host)                                                        \
        return guarded([&] {                                                                      \
            reference_sample_uniform<T>(out_host, moduli_host, mod_count, n_power, stacks, stack_stride_words,\
                                        seed, stream_id, max_candidates);                         \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_lift_small_##S(const gpuntt_keyswitch_plan* plan, const int32_t* small, T* out,\
                                             int polys, int full_base, int to_ntt, void* stream)  \
    {                                                                                             \
        GPUNTT_NEED(plan, small, out)                                                             \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->lift_small(                          \
                small, out, polys, full_base != 0, to_ntt != 0, static_cast<hipStream_t>(stream));\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_keygen_scratch_bytes_##S(const gpuntt_keyswitch_plan* plan, int keys,\
                                                       uint64_t* bytes_host)                      \
    {                                                                                             \
        GPUNTT_NEED(plan, bytes_host)                                                             \
        return guarded([&] {                                                                      \
            *bytes_host = reinterpret_cast<const KeySwitchPlan<T>*>(plan)->keygen_scratch_bytes(keys);\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_encrypt_scratch_bytes_##S(const gpuntt_keyswitch_plan* plan, int count,\
                                                        uint64_t* bytes_host)                     \
    {                                                                                             \
        GPUNTT_NEED(plan, bytes_host)                                                             \
        return guarded([&] {                                                                      \
            *bytes_host = reinterpret_cast<const KeySwitchPlan<T>*>(plan)->encrypt_scratch_bytes(count);\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_generate_keys_##S(const gpuntt_keyswitch_plan* plan, const T* s, const T* s_from,\
                                                const int32_t* errors, T* const* keys_host, int keys,\
                                                void* scratch, void* stream)                      \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->generate_keys(                       \
                s, s_from, errors, keys_host, keys, scratch, static_cast<hipStream_t>(stream));   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_encrypt_symmetric_##S(const gpuntt_keyswitch_plan* plan, const T* s,\
                                                    const int32_t* errors, const T* message, T* out, int count,\
                                                    void* scratch, void* stream)                  \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->encrypt_symmetric(                   \
                s, errors, message, out, count, scratch, static_cast<hipStream_t>(stream));       \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_phase_scratch_bytes_##S(const gpuntt_keyswitch_plan* plan, int count, int components,\
                                                      int input_ntt, uint64_t* bytes_host)        \
    {                                                                                             \
        GPUNTT_NEED(plan, bytes_host)                                                             \
        return guarded([&] {                                                                      \
            *bytes_host = reinterpret_cast<const KeySwitchPlan<T>*>(plan)->phase_scratch_bytes(   \
                count, components, input_ntt != 0);                                               \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_phase_##S(const gpuntt_keyswitch_plan* plan, const T* ct, const T* s, T* out,\
                                        int count, int components, int input_ntt, int output_ntt, \
                                        void* scratch, void* stream)                              \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->phase(                               \
                ct, s, out, count, components, input_ntt != 0, output_ntt != 0, scratch,          \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_encrypt_public_scratch_bytes_##S(const gpuntt_keyswitch_plan* plan, int count,\
                                                               uint64_t* bytes_host)              \
    {                                                                                             \
        GPUNTT_NEED(plan, bytes_host)                                                             \
        return guarded([&] {                                                                      \
            *bytes_host = reinterpret_cast<const KeySwitchPlan<T>*>(plan)->encrypt_public_scratch_bytes(count);\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_encrypt_public_##S(const gpuntt_keyswitch_plan* plan, const T* pk,  \
                                                 const int32_t* small, const T* message, T* out, int count,\
                                                 void* scratch, void* stream)                     \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->encrypt_public(                      \
                pk, small, message, out, count, scratch, static_cast<hipStream_t>(stream));       \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_lift_centred_##S(const gpuntt_keyswitch_plan* plan, const T* words, T plain_modulus,\
                                               T* out, int polys, int full_base, int to_ntt, void* stream)\
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->lift_centred(                        \
                words, plain_modulus, out, polys, full_base != 0, to_ntt != 0, static_cast<hipStream_t>(stream));\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_multiply_plain_##S(const gpuntt_keyswitch_plan* plan, const T* ct, const T* pt,\
                                                 T* out, int count, int plain_count, void* stream)\
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->multiply_plain(                      \
                ct, pt, out, count, plain_count, static_cast<hipStream_t>(stream));               \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_encoder_workspace_bytes_##S(int n_power, uint64_t* bytes_host)                 \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] { *bytes_host = BfvBatchEncoder<T>::workspace_bytes(n_power); });       \
    }                                                                                             \
    int gpuntt_bfv_encoder_scratch_bytes_##S(int n_power, int count, uint64_t* bytes_host)        \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] { *bytes_host = BfvBatchEncoder<T>::scratch_bytes(n_power, count); });  \
    }                                                                                             \
    int gpuntt_bfv_encoder_create_##S(gpuntt_bfv_encoder** encoder_host, CM plain_modulus, int n_power,\
                                      const T* forward_table, const T* inverse_table, T n_inverse,\
                                      int batch_hint, void* workspace_device, void* stream)       \
    {                                                                                             \
        GPUNTT_NEED(encoder_host)                                                                 \
        return guarded([&] {                                                                      \
            *encoder_host = reinterpret_cast<gpuntt_bfv_encoder*>(new BfvBatchEncoder<T>(         \
                to_mod<T>(plain_modulus), n_power, forward_table, inverse_table, n_inverse, batch_hint,\
                static_cast<hipStream_t>(stream), workspace_device));                             \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_encoder_encode_##S(const gpuntt_bfv_encoder* encoder, const T* values, T* plain, int count,\
                                      void* stream)                                               \
    {                                                                                             \
        GPUNTT_NEED(encoder)                                                                      \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvBatchEncoder<T>*>(encoder)->encode(values, plain, count,    \
                                                                         static_cast<hipStream_t>(stream));\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_encoder_decode_##S(const gpuntt_bfv_encoder* encoder, const T* plain, T* values, int count,\
                                      void* scratch, void* stream)                                \
    {                                                                                             \
        GPUNTT_NEED(encoder)                                                                      \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvBatchEncoder<T>*>(encoder)->decode(plain, values, count, scratch,\
                                                                         static_cast<hipStream_t>(stream));\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_encoder_owns_workspace_##S(const gpuntt_bfv_encoder* encoder)                  \
    {                                                                                             \
        GPUNTT_NEED(encoder)                                                                      \
        return reinterpret_cast<const BfvBatchEncoder<T>*>(encoder)->owns_workspace() ? 1 : 0;    \
    }                                                                                             \
    int gpuntt_bfv_encoder_destroy_##S(gpuntt_bfv_encoder* encoder)                               \
    {                                                                                             \
        return guarded([&] { delete reinterpret_cast<BfvBatchEncoder<T>*>(encoder); });           \
    }                                                                                             \
    int gpuntt_bfv_plan_scale_message_##S(const gpuntt_bfv_plan* plan, const T* message, T* out, int count,\
                                          int to_ntt, void* stream)                               \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->scale_message(                     \
                message, out, count, to_ntt != 0, static_cast<hipStream_t>(stream));              \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_decode_##S(const gpuntt_bfv_plan* plan, const T* x, T* message_out, T* noise_max,\
                                   int stacks, void* stream)                                      \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->decode(                            \
                x, message_out, noise_max, stacks, static_cast<hipStream_t>(stream));             \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_decode_partials_bytes_##S(const gpuntt_bfv_plan* plan, int stacks, uint64_t* bytes_host)\
    {                                                                                             \
        GPUNTT_NEED(plan, bytes_host)                                                             \
        return guarded([&] {                                                                      \
            *bytes_host = reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->decode_partials_bytes(stacks);\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_decode_two_launch_##S(const gpuntt_bfv_plan* plan, const T* x, T* message_out,\
                                              T* noise_max, int stacks, void* partials, void* stream)\
    {                                                                                             \
        GPUNTT_NEED(plan, partials)                                                               \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->decode(                            \
                x, message_out, noise_max, stacks, static_cast<hipStream_t>(stream), partials);   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_decrypt_scratch_bytes_##S(const gpuntt_bfv_plan* plan, int count, uint64_t* bytes_host)\
    {                                                                                             \
        GPUNTT_NEED(plan, bytes_host)                                                             \
        return guarded([&] {                                                                      \
            *bytes_host = reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->decrypt_scratch_bytes(count);\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_decrypt_##S(const gpuntt_bfv_plan* plan, const T* ct,                     \
                                    const gpuntt_keyswitch_plan* key_switch, const T* s, T* message_out,\
                                    T* noise_max, int count, int components, int input_ntt, void* scratch,\
                                    void* key_switch_scratch, void* stream)                       \
    {                                                                                             \
        GPUNTT_NEED(plan, key_switch)                                                             \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->decrypt(                           \
                ct, *reinterpret_cast<const KeySwitchPlan<T>*>(key_switch), s, message_out, noise_max, count,\
                components, input_ntt != 0, scratch, key_switch_scratch, static_cast<hipStream_t>(stream));\
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_noise_budget_bits_##S(T noise_max, int q_count)                                \
    {                                                                                             \
        return noise_budget_bits<T>(noise_max, q_count);                                          \
    }                                                                                             \
    int gpuntt_keyswitch_plan_destroy_##S(gpuntt_keyswitch_plan* plan)                            \
    {                                                                                             \
        return guarded([&] { delete reinterpret_cast<KeySwitchPlan<T>*>(plan); });                \
    }                                                                                             \
    int gpuntt_keyswitch_constants_##S(const CM* q_moduli_host, int q_count, const CM* p_moduli_host, int p_count, \
                                       int alpha, T* const* arrays_host)                          \
    {                                                                                             \
        GPUNTT_NEED(arrays_host)                                                                  \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto ps = to_mods<T>(p_moduli_host, p_count, "Invalid p_count!");                \
            T* const* v = arrays_host;                                                            \
            KeySwitchPlan<T>::constants(qs.data(), q_count, ps.data(), p_count, alpha,            \
                                        KeySwitchConstants<T>{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], \
                                                              v[9], v[10], v[11], v[12], v[13], v[14], v[15],     \
                                                              v[16], v[17]});                     \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_reference_mod_up_##S(const CM* q_moduli_host, int q_count, const CM* p_moduli_host,       \
                                              int p_count, int alpha, const T* in_host, T* a_host, int n_power,   \
                                              int count, int mode)                                \
    {                                                                                             \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto ps = to_mods<T>(p_moduli_host, p_count, "Invalid p_count!");                \
            KeySwitchPlan<T>::reference_mod_up(qs.data(), q_count, ps.data(), p_count, alpha, in_host, a_host,    \
                                               n_power, count, static_cast<BaseConvMode>(mode));  \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_reference_mod_down_##S(const CM* q_moduli_host, int q_count, const CM* p_moduli_host,     \
                                                int p_count, const T* x_host, T* out_host, int n_power,           \
                                                int stacks)                                       \
    {                                                                                             \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto ps = to_mods<T>(p_moduli_host, p_count, "Invalid p_count!");                \
            KeySwitchPlan<T>::reference_mod_down(qs.data(), q_count, ps.data(), p_count, x_host, out_host,        \
                                                 n_power, stacks);                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_workspace_bytes_rescale_##S(int q_count, int p_count, int alpha, int n_power,       \
                                                          int rescale_limbs, uint64_t* bytes_host) \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] {                                                                      \
            *bytes_host = KeySwitchPlan<T>::workspace_bytes(q_count, p_count, alpha, n_power, rescale_limbs);     \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_create_rescale_##S(                                                 \
        gpuntt_keyswitch_plan** plan_host, const CM* q_moduli_host, int q_count, const CM* p_moduli_host,         \
        int p_count, int alpha, int n_power, const T* forward_table, const T* inverse_table,      \
        const T* mod_inverse_host, int reduction_poly, int batch_hint, int key_mod_count,         \
        const int* key_limbs_host, int rescale_limbs, void* workspace_device, void* stream)       \
    {                                                                                             \
        GPUNTT_NEED(plan_host)                                                                    \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto ps = to_mods<T>(p_moduli_host, p_count, "Invalid p_count!");                \
            if (reduction_poly != GPUNTT_X_N_PLUS && reduction_poly != GPUNTT_X_N_MINUS)          \
                throw std::invalid_argument("Invalid reduction_poly!");                           \
            *plan_host = reinterpret_cast<gpuntt_keyswitch_plan*>(new KeySwitchPlan<T>(           \
                qs.data(), q_count, ps.data(), p_count, alpha, n_power, forward_table, inverse_table,             \
                mod_inverse_host, static_cast<ReductionPolynomial>(reduction_poly), batch_hint, key_mod_count,    \
                key_limbs_host, static_cast<hipStream_t>(stream), workspace_device, rescale_limbs));              \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_rescale_limbs_##S(const gpuntt_keyswitch_plan* plan)                \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const KeySwitchPlan<T>*>(plan)->rescale_limbs();                  \
    }                                                                                             \
    int gpuntt_keyswitch_plan_rescale_scratch_bytes_##S(const gpuntt_keyswitch_plan* plan, int stacks,            \
                                                        uint64_t* bytes_host)                     \
    {                                                                                             \
        GPUNTT_NEED(plan, bytes_host)                                                             \
        return guarded([&] {                                                                      \
            *bytes_host = reinterpret_cast<const KeySwitchPlan<T>*>(plan)->rescale_scratch_bytes(stacks);         \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_mod_down_rescale_##S(const gpuntt_keyswitch_plan* plan, const T* x, T* out,          \
                                                   int stacks, void* stream)                      \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->mod_down_rescale(x, out, stacks,      \
                                                                              static_cast<hipStream_t>(stream));  \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_rescale_##S(const gpuntt_keyswitch_plan* plan, const T* x, T* out, int stacks,       \
                                          int ntt_form, void* scratch, void* stream)              \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->rescale(x, out, stacks, ntt_form != 0, scratch,      \
                                                                     static_cast<hipStream_t>(stream));           \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_multiply_relinearize_rescale_##S(const gpuntt_keyswitch_plan* plan, const T* x,      \
                                                               const T* y, const T* key, T* out, int count,       \
                                                               int output_ntt, void* scratch, void* stream)       \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->multiply_relinearize_rescale(        \
                x, y, key, out, count, output_ntt != 0, scratch, static_cast<hipStream_t>(stream));               \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_multiply_relinearize_sum_rescale_##S(                               \
        const gpuntt_keyswitch_plan* plan, const T* const* x_host, const T* const* y_host, int terms,             \
        const T* key, T* out, int count, int output_ntt, void* scratch, void* stream)             \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->multiply_relinearize_sum_rescale(    \
                x_host, y_host, terms, key, out, count, output_ntt != 0, scratch,                 \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_rotate_hoisted_sum_rescale_##S(                                     \
        const gpuntt_keyswitch_plan* plan, const T* a, const T* c0, const T* const* keys_host,    \
        const uint32_t* galois_elements_host, const T* const* weights_host, int elements, T* out, int count,      \
        int output_ntt, void* scratch, void* stream)                                              \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->rotate_hoisted_sum_rescale(          \
                a, c0, keys_host, galois_elements_host, weights_host, elements, out, count, output_ntt != 0,      \
                scratch, static_cast<hipStream_t>(stream));                                       \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_bsgs_scratch_bytes_##S(int q_count, int p_count, int alpha, int n_power, int count,  \
                                                     int n1, int n2, uint64_t* bytes_host)        \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] {                                                                      \
            *bytes_host = KeySwitchPlan<T>::bsgs_scratch_bytes(q_count, p_count, alpha, n_power, count, n1, n2);  \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_linear_transform_bsgs_##S(                                          \
        const gpuntt_keyswitch_plan* plan, const T* a, const T* c0, const T* c1, const T* const* baby_keys_host,  \
        const uint32_t* baby_elements_host, int n1, const T* const* giant_keys_host,              \
        const uint32_t* giant_elements_host, int n2, const T* const* weights_host, T* out, int count,             \
        int output_ntt, void* scratch, void* stream)                                              \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->linear_transform_bsgs(               \
                a, c0, c1, baby_keys_host, baby_elements_host, n1, giant_keys_host, giant_elements_host, n2,      \
                weights_host, out, count, output_ntt != 0, scratch, static_cast<hipStream_t>(stream));            \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_plan_linear_transform_bsgs_rescale_##S(                                  \
        const gpuntt_keyswitch_plan* plan, const T* a, const T* c0, const T* c1, const T* const* baby_keys_host,  \
        const uint32_t* baby_elements_host, int n1, const T* const* giant_keys_host,              \
        const uint32_t* giant_elements_host, int n2, const T* const* weights_host, T* out, int count,             \
        int output_ntt, void* scratch, void* stream)                                              \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const KeySwitchPlan<T>*>(plan)->linear_transform_bsgs_rescale(       \
                a, c0, c1, baby_keys_host, baby_elements_host, n1, giant_keys_host, giant_elements_host, n2,      \
                weights_host, out, count, output_ntt != 0, scratch, static_cast<hipStream_t>(stream));            \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_reference_mod_down_rescale_##S(const CM* q_moduli_host, int q_count,     \
                                                        const CM* p_moduli_host, int p_count, int rescale_limbs,  \
                                                        const T* x_host, T* out_host, int n_power, int stacks)    \
    {                                                                                             \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto ps = to_mods<T>(p_moduli_host, p_count, "Invalid p_count!");                \
            KeySwitchPlan<T>::reference_mod_down_rescale(qs.data(), q_count, ps.data(), p_count, rescale_limbs,   \
                                                         x_host, out_host, n_power, stacks);      \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_keyswitch_reference_rescale_##S(const CM* q_moduli_host, int q_count, int rescale_limbs,           \
                                               const T* x_host, T* out_host, int n_power, int stacks)             \
    {                                                                                             \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            KeySwitchPlan<T>::reference_rescale(qs.data(), q_count, rescale_limbs, x_host, out_host, n_power,     \
                                                stacks);                                          \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_workspace_bytes_##S(int q_count, int b_count, int n_power, uint64_t* bytes_host)          \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] { *bytes_host = BfvMultiplyPlan<T>::workspace_bytes(q_count, b_count, n_power); });    \
    }                                                                                             \
    int gpuntt_bfv_plan_scratch_bytes_##S(int q_count, int b_count, int n_power, int count, uint64_t* bytes_host) \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded(                                                                           \
            [&] { *bytes_host = BfvMultiplyPlan<T>::scratch_bytes(q_count, b_count, n_power, count); });          \
    }                                                                                             \
    int gpuntt_bfv_plan_create_##S(gpuntt_bfv_plan** plan_host, const CM* q_moduli_host, int q_count,             \
                                   const CM* b_moduli_host, int b_count, T plain_modulus, int n_power,            \
                                   const T* forward_table, const T* inverse_table, const T* mod_inverse_host,     \
                                   int reduction_poly, int batch_hint, void* workspace_device, void* stream)      \
    {                                                                                             \
        GPUNTT_NEED(plan_host)                                                                    \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto bs = to_mods<T>(b_moduli_host, b_count, "Invalid b_count!");                \
            if (reduction_poly != GPUNTT_X_N_PLUS && reduction_poly != GPUNTT_X_N_MINUS)          \
                throw std::invalid_argument("Invalid reduction_poly!");                           \
            *plan_host = reinterpret_cast<gpuntt_bfv_plan*>(new BfvMultiplyPlan<T>(               \
                qs.data(), q_count, bs.data(), b_count, plain_modulus, n_power, forward_table, inverse_table,     \
                mod_inverse_host, static_cast<ReductionPolynomial>(reduction_poly), batch_hint,   \
                static_cast<hipStream_t>(stream), workspace_device));                             \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_extend_##S(const gpuntt_bfv_plan* plan, const T* in, T* full, int stacks, void* stream)   \
    {                                                                                             \
        GPUNTT_NEED(plan, in, full)                                                               \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->extend(in, full, stacks,            \
                                                                      static_cast<hipStream_t>(stream));          \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_scale_round_##S(const gpuntt_bfv_plan* plan, const T* full, T* out, int stacks,           \
                                        void* stream)                                             \
    {                                                                                             \
        GPUNTT_NEED(plan, full, out)                                                              \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->scale_round(full, out, stacks,      \
                                                                           static_cast<hipStream_t>(stream));     \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_multiply_##S(const gpuntt_bfv_plan* plan, const T* x, const T* y, T* out, int count,      \
                                     int input_ntt, int output_ntt, void* scratch, void* stream)  \
    {                                                                                             \
        GPUNTT_NEED(plan, x, y, out, scratch)                                                     \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->multiply(                          \
                x, y, out, count, input_ntt != 0, output_ntt != 0, scratch, static_cast<hipStream_t>(stream));    \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_multiply_relinearize_##S(const gpuntt_bfv_plan* plan, const T* x, const T* y, \
                                                 const gpuntt_keyswitch_plan* key_switch, const T* key, T* out, \
                                                 int count, int input_ntt, int output_ntt, void* scratch, \
                                                 void* key_switch_scratch, void* stream)          \
    {                                                                                             \
        GPUNTT_NEED(plan, x, y, key_switch, key, out, scratch, key_switch_scratch)                \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->multiply_relinearize(              \
                x, y, *reinterpret_cast<const KeySwitchPlan<T>*>(key_switch), key, out, count, input_ntt != 0, \
                output_ntt != 0, scratch, key_switch_scratch, static_cast<hipStream_t>(stream));  \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_max_terms_##S(const gpuntt_bfv_plan* plan)                                \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->max_terms();                    \
    }                                                                                             \
    int gpuntt_bfv_max_terms_##S(const CM* q_moduli_host, int q_count, const CM* b_moduli_host, int b_count,      \
                                 T plain_modulus, int n_power, int* terms_host)                   \
    {                                                                                             \
        GPUNTT_NEED(terms_host)                                                                   \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto bs = to_mods<T>(b_moduli_host, b_count, "Invalid b_count!");                \
            *terms_host = BfvMultiplyPlan<T>::max_terms(qs.data(), q_count, bs.data(), b_count, plain_modulus,    \
                                                        n_power);                                 \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_sum_scratch_bytes_##S(int q_count, int b_count, int n_power, int count, int operands,     \
                                              uint64_t* bytes_host)                               \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] {                                                                      \
            *bytes_host = BfvMultiplyPlan<T>::sum_scratch_bytes(q_count, b_count, n_power, count, operands);      \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_multiply_sum_##S(const gpuntt_bfv_plan* plan, const T* const* x_host,     \
                                         const T* const* y_host, int terms, T* out, int count, int input_ntt,     \
                                         int output_ntt, void* scratch, void* stream)             \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->multiply_sum(                      \
                x_host, y_host, terms, out, count, input_ntt != 0, output_ntt != 0, scratch,      \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_multiply_relinearize_sum_##S(                                             \
        const gpuntt_bfv_plan* plan, const T* const* x_host, const T* const* y_host, int terms,   \
        const gpuntt_keyswitch_plan* key_switch, const T* key, T* out, int count, int input_ntt, int output_ntt,  \
        void* scratch, void* key_switch_scratch, void* stream)                                    \
    {                                                                                             \
        GPUNTT_NEED(plan, key_switch)                                                             \
        return guarded([&] {                                                                      \
            reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->multiply_relinearize_sum(          \
                x_host, y_host, terms, *reinterpret_cast<const KeySwitchPlan<T>*>(key_switch), key, out, count,   \
                input_ntt != 0, output_ntt != 0, scratch, key_switch_scratch,                     \
                static_cast<hipStream_t>(stream));                                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_plan_owns_workspace_##S(const gpuntt_bfv_plan* plan)                           \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const BfvMultiplyPlan<T>*>(plan)->owns_workspace() ? 1 : 0;       \
    }                                                                                             \
    int gpuntt_bfv_plan_destroy_##S(gpuntt_bfv_plan* plan)                                        \
    {                                                                                             \
        return guarded([&] { delete reinterpret_cast<BfvMultiplyPlan<T>*>(plan); });              \
    }                                                                                             \
    int gpuntt_bfv_constants_##S(const CM* q_moduli_host, int q_count, const CM* b_moduli_host, int b_count,      \
                                 T plain_modulus, int n_power, T* const* arrays_host)             \
    {                                                                                             \
        GPUNTT_NEED(arrays_host)                                                                  \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto bs = to_mods<T>(b_moduli_host, b_count, "Invalid b_count!");                \
            T* const* v = arrays_host;                                                            \
            BfvMultiplyPlan<T>::constants(                                                        \
                qs.data(), q_count, bs.data(), b_count, plain_modulus, n_power,                   \
                BfvConstants<T>{BaseConvConstants<T>{v[0], v[1], v[2], v[3], v[4], v[5], v[6]},   \
                                BaseConvConstants<T>{v[7], v[8], v[9], v[10], v[11], v[12], v[13]}, v[14], v[15], \
                                v[16], v[17]});                                                   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_reference_extend_##S(const CM* q_moduli_host, int q_count, const CM* b_moduli_host,            \
                                        int b_count, const T* in_host, T* full_host, int n_power, int stacks)     \
    {                                                                                             \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto bs = to_mods<T>(b_moduli_host, b_count, "Invalid b_count!");                \
            BfvMultiplyPlan<T>::reference_extend(qs.data(), q_count, bs.data(), b_count, in_host, full_host,      \
                                                 n_power, stacks);                                \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_bfv_reference_scale_round_##S(const CM* q_moduli_host, int q_count, const CM* b_moduli_host,       \
                                             int b_count, T plain_modulus, const T* full_host, T* out_host,       \
                                             int n_power, int stacks)                             \
    {                                                                                             \
        return guarded([&] {                                                                      \
            const auto qs = to_mods<T>(q_moduli_host, q_count, "Invalid q_count!");                \
            const auto bs = to_mods<T>(b_moduli_host, b_count, "Invalid b_count!");                \
            BfvMultiplyPlan<T>::reference_scale_round(qs.data(), q_count, bs.data(), b_count, plain_modulus,      \
                                                      full_host, out_host, n_power, stacks);      \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_4step_plan_workspace_bytes_##S(int n_power, uint64_t* bytes_host)                  \
    {                                                                                             \
        GPUNTT_NEED(bytes_host)                                                                   \
        return guarded([&] { *bytes_host = FourStepPlan<T>::workspace_bytes(n_power); });          \
    }                                                                                             \
    int gpuntt_4step_plan_create_##S(gpuntt_4step_plan** plan_host, const T* n1_table,            \
                                     const T* n2_table, const T* w_table, CM modulus, int n_power, \
                                     int ntt_type, T mod_inverse, int natural_order,              \
                                     int batch_hint, void* workspace_device, void* stream)        \
    {                                                                                             \
        GPUNTT_NEED(plan_host, n1_table, n2_table, w_table)                                       \
        return guarded([&] {                                                                      \
            ntt4step_configuration<T> cfg = {n_power, static_cast<type>(ntt_type), mod_inverse,   \
                                             static_cast<hipStream_t>(stream)};                   \
            *plan_host = reinterpret_cast<gpuntt_4step_plan*>(new FourStepPlan<T>(                \
                const_cast<T*>(n1_table), const_cast<T*>(n2_table), const_cast<T*>(w_table),      \
                to_mod<T>(modulus), cfg, natural_order != 0, batch_hint, workspace_device));      \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_4step_plan_execute_##S(const gpuntt_4step_plan* plan, T* in, T* out,               \
                                      int batch_size, void* stream)                               \
    {                                                                                             \
        GPUNTT_NEED(plan, in, out)                                                                \
        return guarded([&] {                                                                      \
            reinterpret_cast<const FourStepPlan<T>*>(plan)->execute(in, out, batch_size,          \
                                                                    static_cast<hipStream_t>(stream)); \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_4step_plan_fast_path_##S(const gpuntt_4step_plan* plan)                            \
    {                                                                                             \
        GPUNTT_NEED(plan)                                                                         \
        return reinterpret_cast<const FourStepPlan<T>*>(plan)->fast_path() ? 1 : 0;               \
    }                                                                                             \
    int gpuntt_4step_plan_destroy_##S(gpuntt_4step_plan* plan)                                    \
    {                                                                                             \
        return guarded([&] { delete reinterpret_cast<FourStepPlan<T>*>(plan); });                 \
    }                                                                                             \
    int gpuntt_generate_power_table_##S(T* out, T base, CM modulus, int log_count,                \
                                        int bit_reversed, void* stream)                           \
    {                                                                                             \
        GPUNTT_NEED(out)                                                                          \
        return guarded([&] {                                                                      \
            GPU_GeneratePowerTable<T>(out, base, to_mod<T>(modulus), log_count, bit_reversed != 0, \
                                      static_cast<hipStream_t>(stream));                          \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_generate_4step_w_##S(T* out, T root, CM modulus, int n_power, int ntt_type,        \
                                    void* stream)                                                 \
    {                                                                                             \
        GPUNTT_NEED(out)                                                                          \
        return guarded([&] {                                                                      \
            GPU_Generate4StepW<T>(out, root, to_mod<T>(modulus), n_power,                         \
                                  static_cast<type>(ntt_type), static_cast<hipStream_t>(stream)); \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_operator_gpu_##S(int op, const T* a, const T* b, T* out, CM modulus,               \
                                uint64_t count, void* stream)                                     \
    {                                                                                             \
        GPUNTT_NEED(a, out)                                                                       \
        return operator_gpu<T>(op, a, b, out, modulus, count, stream);                            \
    }                                                                                             \
    int gpuntt_debug_recip_norm_##S(const T* q, T* out, uint64_t count, void* stream)              \
    {                                                                                             \
        GPUNTT_NEED(q, out)                                                                       \
        return guarded([&] {                                                                      \
            gpuntt::host::debug_recip_norm<T>(q, out, count, static_cast<hipStream_t>(stream));   \
        });                                                                                       \
    }                                                                                             \
    int gpuntt_butterfly_unit_##S(int gentleman_sande, T* u, T* v, const T* roots, CM modulus,    \
                                  uint64_t count, void* stream)                                   \
    {                                                                                             \
        GPUNTT_NEED(u, v)                                                                         \
        GPUNTT_NEED(roots, roots)                                                                 \
        return butterfly_unit<T>(gentleman_sande, u, v, roots, modulus, count, stream);           \
    }

    GPUNTT_C_API(u32, uint32_t, gpuntt_modulus32)
    GPUNTT_C_API(u64, uint64_t, gpuntt_modulus64)
#undef GPUNTT_C_API
}
