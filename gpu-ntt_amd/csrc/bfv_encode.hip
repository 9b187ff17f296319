// bfv_encode.hip -- BfvBatchEncoder<T> (include/gpuntt/rns/bfv_encode.cuh): the slot <-> coefficient
// map of a BFV plaintext, a permutation into GPU_NTT's output order and a transform modulo t.
//
//   bfv_slot_permute:  out[p][i] = in[p][map[i]] [mod t],  p < count, i < N                  -- gather form
//
// One kernel serves both directions; the map (to_slot for encode, to_position for decode) and whether the words are
// reduced modulo t (encode: values may be any word) are the switches.  A lane owns a 16-byte group of OUTPUT words
// (V = 1 for an output off 16-byte alignment or N below a group), loads its V map entries once and walks the
// polynomials of its batch slice: blockIdx.x is the column tile, blockIdx.y the first polynomial, gridDim.y the step.
// The writes are contiguous vector stores; the reads are scattered single words -- inherent in the 5^c order -- inside
// one polynomial of at most 512 KiB at 2^16, which the caches hold.  No LDS, no barrier; 64-bit indices.  The reduction
// is the canonical Shoup product by 1 (rns_arith.hpp) against floor(2^W / t): any word in, a residue out.
#include <hip/hip_runtime.h>

#include <memory>
#include <stdexcept>
#include <vector>

#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/bfv_encode.cuh"
#include "inner_product_internal.hpp"
#include "launch.hpp"
#include "relinearize_internal.hpp"
#include "rns_call.hpp"

namespace gpuntt
{
    namespace kern
    {
        // grid: x = column tile, y = batch slice; in, out: T[count][N]; map: uint32[N], every entry below N
        template <typename T, int V>
        __global__ __launch_bounds__(IP_NT) void bfv_slot_permute(const T* __restrict__ in, T* __restrict__ out,
                                                                  const std::uint32_t* __restrict__ map, int count,
                                                                  int n_power, int reduce, T t, T one_shoup_t)
        {
            using Vec = IpVec<T, V>;
            const unsigned long long col = (static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x) * V;
            if (col >= (1ull << n_power))
                return;
            const IpVec<std::uint32_t, V> mv = *reinterpret_cast<const IpVec<std::uint32_t, V>*>(map + col);
            for (unsigned p = blockIdx.y; p < static_cast<unsigned>(count); p += gridDim.y)
            {
                const T* pi = in + (static_cast<unsigned long long>(p) << n_power);
                Vec o;
#pragma unroll
                for (int v = 0; v < V; v++)
                {
                    const T w = pi[mv.x[v]];
                    o.x[v] = reduce != 0 ? rns_shoup<T>(w, T(1), one_shoup_t, t) : w;
                }
                *reinterpret_cast<Vec*>(out + (static_cast<unsigned long long>(p) << n_power) + col) = o;
            }
        }
    } // namespace kern

    void bfv_slot_maps(int n_power, std::uint32_t* to_position_host, std::uint32_t* to_slot_host)
    {
        host::rns_check_n_power(n_power);
        host::need_pointers(to_position_host, to_slot_host);
        const std::uint32_t n = 1u << n_power, half = n >> 1, mask = 2u * n - 1u;
        std::uint32_t e = 1u; // 5^c mod 2N
        for (std::uint32_t c = 0; c < half; c++)
        {
            const std::uint32_t top = galois_brev((e - 1u) >> 1, n_power);
            const std::uint32_t bottom = galois_brev((((mask + 1u - e) & mask) - 1u) >> 1, n_power);
            to_position_host[c] = top, to_position_host[half + c] = bottom;
            to_slot_host[top] = c, to_slot_host[bottom] = half + c;
            e = (e * 5u) & mask;
        }
    }

    namespace
    {
        // slices of the batch: a lane keeps its map entries over count / slices polynomials; small calls are spread
        // over about four workgroups per CU (an estimate, as rns_split's)
        unsigned permute_slices(unsigned tiles, int count)
        {
            unsigned s = 1;
            while (s < 1024u && tiles * s < 1024u)
                s *= 2;
            return s < static_cast<unsigned>(count) ? s : static_cast<unsigned>(count);
        }

        template <typename T, int V>
        void permute_as(const T* in, T* out, const std::uint32_t* map, int count, int n_power, bool reduce, T t,
                        T one_shoup_t, hipStream_t stream)
        {
            const host::RelinGrid g = host::relin_grid(n_power, V, 1);
            GPUNTT_LAUNCH((kern::bfv_slot_permute<T, V>), dim3(g.tiles, permute_slices(g.tiles, count)), dim3(g.nt), 0,
                          stream, in, out, map, count, n_power, reduce ? 1 : 0, t, one_shoup_t);
            GPUNTT_HIP_CHECK(hipGetLastError());
        }

        template <typename T>
        void permute(const T* in, T* out, const std::uint32_t* map, int count, int n_power, bool reduce, T t,
                     T one_shoup_t, hipStream_t stream)
        {
            constexpr int VW = 16 / sizeof(T);
            if (host::relin_wide<T>(n_power, {out})) // the map lies 256-byte aligned in the workspace
                permute_as<T, VW>(in, out, map, count, n_power, reduce, t, one_shoup_t, stream);
            else
                permute_as<T, 1>(in, out, map, count, n_power, reduce, t, one_shoup_t, stream);
        }
    } // namespace

    template <typename T> struct BfvBatchEncoder<T>::Impl
    {
        int n = 0;
        Modulus<T> mod;
        T one_shoup = 0; // floor(2^W / t)
        char* ws = nullptr;
        bool owns = false;
        size_t at_slot = 0, at_fwd = 0, at_inv = 0;
        std::unique_ptr<NTTPlan<T>> fwd, inv;

        const std::uint32_t* to_position() const { return reinterpret_cast<const std::uint32_t*>(ws); }
        const std::uint32_t* to_slot() const { return reinterpret_cast<const std::uint32_t*>(ws + at_slot); }
        std::uint64_t bytes(int count) const { return (static_cast<std::uint64_t>(count) << n) * sizeof(T); }

        static void check_count(int count)
        {
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
        }

        void encode(const T* values, T* plain, int count, hipStream_t stream) const
        {
            check_count(count);
            host::need_pointers(values, plain);
            if (count == 0)
                return;
            host::refuse_overlap({{plain, bytes(count)}}, {{values, bytes(count)}}, "encode input and output overlap!");
            permute<T>(values, plain, to_slot(), count, n, true, mod.value, one_shoup, stream);
            inv->execute(plain, plain, count, stream);
        }

        void decode(const T* plain, T* values, int count, void* scratch, hipStream_t stream) const
        {
            check_count(count);
            host::need_pointers(plain, values, scratch);
            host::need_aligned_scratch(scratch);
            if (count == 0)
                return;
            host::refuse_overlap({{values, bytes(count)}}, {{plain, bytes(count)}}, "decode input and output overlap!");
            host::refuse_overlap({{scratch, host::rns_align(bytes(count))}}, {{plain, bytes(count)}, {values, bytes(count)}},
                                 "The scratch overlaps an operand!");
            T* w = static_cast<T*>(scratch);
            fwd->execute(plain, w, count, stream);
            permute<T>(w, values, to_position(), count, n, false, mod.value, one_shoup, stream);
        }
    };

    namespace
    {
        struct EncLayout
        {
            size_t slot, fwd, inv, total;
        };
        template <typename T> EncLayout enc_layout(int n_power)
        {
            host::rns_check_n_power(n_power);
            EncLayout l{};
            const size_t map = host::rns_align((static_cast<size_t>(1) << n_power) * sizeof(std::uint32_t));
            const size_t plan = host::rns_align(NTTPlan<T>::workspace_bytes(n_power, 1));
            l.slot = map, l.fwd = 2 * map, l.inv = 2 * map + plan, l.total = 2 * map + 2 * plan;
            return l;
        }
    } // namespace

    template <typename T> size_t BfvBatchEncoder<T>::workspace_bytes(int n_power) { return enc_layout<T>(n_power).total; }

    template <typename T> size_t BfvBatchEncoder<T>::scratch_bytes(int n_power, int count)
    {
        host::rns_check_n_power(n_power);
        if (count < 0)
            throw std::invalid_argument("Invalid count!");
        return host::rns_align((static_cast<size_t>(count) << n_power) * sizeof(T));
    }

    template <typename T>
    BfvBatchEncoder<T>::BfvBatchEncoder(Modulus<T> plain_modulus, int n_power, const Root<T>* forward_table_device,
                                        const Root<T>* inverse_table_device, Ninverse<T> n_inverse_host, int batch_hint,
                                        stream_t stream, void* workspace_device)
        : p_(nullptr)
    {
        constexpr int W = static_cast<int>(8 * sizeof(T));
        const EncLayout lay = enc_layout<T>(n_power); // checks n_power
        if (plain_modulus.value < 2)
            throw std::invalid_argument("Invalid modulus!");
        const Modulus<T> ref(plain_modulus.value); // throws for a modulus outside the library's domain
        if (ref.bit != plain_modulus.bit || ref.mu != plain_modulus.mu)
            throw std::invalid_argument("Invalid modulus!");
        const std::uint64_t t = plain_modulus.value;
        if ((t - 1) % (2ull << n_power) != 0)
            throw std::invalid_argument("Plaintext modulus does not support batching!");
        if (forward_table_device == nullptr || inverse_table_device == nullptr)
            throw std::invalid_argument("null pointer argument");

        const size_t n = static_cast<size_t>(1) << n_power;
        std::vector<std::uint32_t> to_position(n), to_slot(n);
        bfv_slot_maps(n_power, to_position.data(), to_slot.data());

        std::unique_ptr<Impl> p(new Impl);
        p->n = n_power, p->mod = plain_modulus;
        p->one_shoup = static_cast<T>((static_cast<unsigned __int128>(1) << W) / t);
        p->at_slot = lay.slot, p->at_fwd = lay.fwd, p->at_inv = lay.inv;
        void* raw = workspace_device;
        if (raw == nullptr)
        {
            GPUNTT_HIP_CHECK(hipMalloc(&raw, lay.total));
            p->owns = true;
        }
        p->ws = static_cast<char*>(raw);
        try
        {
            GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws, to_position.data(), n * sizeof(std::uint32_t), hipMemcpyHostToDevice,
                                            stream));
            GPUNTT_HIP_CHECK(hipMemcpyAsync(p->ws + lay.slot, to_slot.data(), n * sizeof(std::uint32_t),
                                            hipMemcpyHostToDevice, stream));
            GPUNTT_HIP_CHECK(hipStreamSynchronize(stream)); // the maps die with this scope
            p->fwd.reset(new NTTPlan<T>(forward_table_device, &plain_modulus, 1, n_power, ReductionPolynomial::X_N_plus,
                                        FORWARD, nullptr, batch_hint, stream, p->ws + lay.fwd));
            p->inv.reset(new NTTPlan<T>(inverse_table_device, &plain_modulus, 1, n_power, ReductionPolynomial::X_N_plus,
                                        INVERSE, &n_inverse_host, batch_hint, stream, p->ws + lay.inv));
        }
        catch (...)
        {
            p->fwd.reset(), p->inv.reset();
            if (p->owns)
                (void) hipFree(p->ws);
            throw;
        }
        p_ = p.release();
    }

    template <typename T> BfvBatchEncoder<T>::~BfvBatchEncoder()
    {
        if (p_ == nullptr)
            return;
        p_->fwd.reset(), p_->inv.reset();
        if (p_->owns)
            (void) hipFree(p_->ws);
        delete p_;
    }

    template <typename T>
    void BfvBatchEncoder<T>::encode(const T* device_values, T* device_plain, int count, stream_t stream) const
    {
        p_->encode(device_values, device_plain, count, stream);
    }
    template <typename T>
    void BfvBatchEncoder<T>::decode(const T* device_plain, T* device_values, int count, void* scratch_device,
                                    stream_t stream) const
    {
        p_->decode(device_plain, device_values, count, scratch_device, stream);
    }
    template <typename T> size_t BfvBatchEncoder<T>::scratch_bytes(int count) const { return scratch_bytes(p_->n, count); }
    template <typename T> int BfvBatchEncoder<T>::n_power() const { return p_->n; }
    template <typename T> Modulus<T> BfvBatchEncoder<T>::plain_modulus() const { return p_->mod; }
    template <typename T> bool BfvBatchEncoder<T>::owns_workspace() const { return p_->owns; }

    template class BfvBatchEncoder<Data32>;
    template class BfvBatchEncoder<Data64>;
} // namespace gpuntt
