// base_conversion.hip -- RNS fast base conversion (extension, include/gpuntt/rns/base_conversion.cuh).
//
// One lane owns one coefficient column of one ring element: it reads its L input words (coalesced: consecutive lanes,
// consecutive columns), turns each into y_i with one exact Shoup product and parks the y_i in LDS -- at word
// [i][lane], so a lane only ever reads what it wrote itself: no barrier, and consecutive lanes hit consecutive banks.
// The K outputs are then produced BC_KB at a time: for a block of outputs the lane walks i = 0 .. L-1 once, reads y_i
// back from LDS and multiply-accumulates it into BC_KB three-word accumulators, which leave through the three-product
// fold -- the conversion unit of base_conversion_internal.hpp (bc_z, bc_block_mac, bc_fold), where the bounds are
// proved.  Every constant -- the Shoup pair of qhat_i^-1, the matrix row, the folding constants -- is indexed by
// wave-uniform values only, so it travels through the scalar cache.
//
// Small count * N: the grid's second dimension splits the blocks of BC_KB outputs over several workgroups, each of
// which re-reads the column (from L2) and recomputes the y_i -- see host::bc_ksplit().
#include <hip/hip_runtime.h>

#include <atomic>
#include <stdexcept>
#include <vector>

#include "base_conversion_internal.hpp"
#include "gpuntt/rns/base_conversion.cuh"
#include "launch.hpp"

namespace gpuntt
{
    // kern::base_convert and what it is made of: base_conversion_internal.hpp (key_switch.hip launches its strided form)

    namespace host
    {
        namespace
        {
            std::atomic<int> g_bc_ksplit{0}; // test hook baseconv_ksplit: 0 = rns_split(), n = n workgroups per column tile
        }
        void baseconv_set_ksplit(int v) { g_bc_ksplit.store(v, std::memory_order_relaxed); }
    } // namespace host

    namespace
    {
        using U128 = unsigned __int128;

        std::uint64_t bc_gcd(std::uint64_t a, std::uint64_t b)
        {
            while (b != 0)
            {
                const std::uint64_t r = a % b;
                a = b;
                b = r;
            }
            return a;
        }
        std::uint64_t bc_mulmod(std::uint64_t a, std::uint64_t b, std::uint64_t m)
        {
            return static_cast<std::uint64_t>(static_cast<U128>(a) * b % m);
        }
        // a^-1 mod m for gcd(a, m) = 1, m >= 2 (extended Euclid)
        std::uint64_t bc_modinv(std::uint64_t a, std::uint64_t m)
        {
            __int128 r0 = m, r1 = a % m, s0 = 0, s1 = 1;
            while (r1 != 0)
            {
                const __int128 qt = r0 / r1;
                const __int128 r2 = r0 - qt * r1, s2 = s0 - qt * s1;
                r0 = r1, r1 = r2, s0 = s1, s1 = s2;
            }
            if (s0 < 0)
                s0 += m;
            return static_cast<std::uint64_t>(s0 % static_cast<__int128>(m));
        }
        int bc_bit_length(std::uint64_t v)
        {
            int b = 0;
            for (; v != 0; v >>= 1)
                b++;
            return b;
        }

        using HostConsts = host::BcHostConsts; // the constants in exact integers (64-bit words for both widths)

        template <typename T> std::uint64_t checked_value(const Modulus<T>& m)
        {
            if (m.value < 2)
                throw std::invalid_argument("Invalid modulus!");
            const Modulus<T> ref(m.value); // throws for a modulus outside the library's domain
            if (ref.bit != m.bit || ref.mu != m.mu)
                throw std::invalid_argument("Invalid modulus!");
            return static_cast<std::uint64_t>(m.value);
        }

        template <typename T> HostConsts derive(const Modulus<T>* qm, int L, const Modulus<T>* pm, int K)
        {
            constexpr int W = static_cast<int>(8 * sizeof(T));
            if (L < 1 || L > BASECONV_MAX_COUNT)
                throw std::invalid_argument("Invalid in_count!");
            if (K < 1 || K > BASECONV_MAX_COUNT)
                throw std::invalid_argument("Invalid out_count!");
            if (qm == nullptr || pm == nullptr)
                throw std::invalid_argument("null pointer argument");
            HostConsts h;
            h.L = L, h.K = K;
            for (int i = 0; i < L; i++)
                h.q.push_back(checked_value(qm[i]));
            for (int j = 0; j < K; j++)
                h.p.push_back(checked_value(pm[j]));
            for (int i = 0; i < L; i++)
            {
                for (int o = i + 1; o < L; o++)
                    if (bc_gcd(h.q[i], h.q[o]) != 1)
                        throw std::invalid_argument("Input base moduli are not pairwise coprime!");
                for (int j = 0; j < K; j++)
                    if (bc_gcd(h.q[i], h.p[j]) != 1)
                        throw std::invalid_argument("An output modulus is not coprime to the input base!");
            }
            auto shoup = [](std::uint64_t v, std::uint64_t m) {
                return static_cast<std::uint64_t>((static_cast<U128>(v) << W) / m);
            };
            // qhat_i mod m: the product of the other q's
            auto qhat_mod = [&](int i, std::uint64_t m) {
                std::uint64_t r = 1 % m;
                for (int o = 0; o < L; o++)
                    if (o != i)
                        r = bc_mulmod(r, h.q[o] % m, m);
                return r;
            };
            h.matrix.assign(static_cast<size_t>(L) * K, 0);
            for (int i = 0; i < L; i++)
            {
                const std::uint64_t q = h.q[i];
                const std::uint64_t w = bc_modinv(qhat_mod(i, q), q);
                h.w.push_back(w);
                h.wp.push_back(shoup(w, q));
                const int b = bc_bit_length(q);
                const U128 r = (static_cast<U128>(1) << (W - 1 + b)) / q;
                h.recip.push_back((r >> W) != 0 ? 0 : static_cast<std::uint64_t>(r));
                h.blen.push_back(static_cast<std::uint64_t>(b));
                for (int j = 0; j < K; j++)
                    h.matrix[static_cast<size_t>(i) * K + j] = qhat_mod(i, h.p[j]);
            }
            for (int j = 0; j < K; j++)
            {
                const std::uint64_t p = h.p[j];
                const std::uint64_t qm_p = qhat_mod(-1, p);
                const std::uint64_t qi = bc_modinv(qm_p, p);
                const host::RnsFoldConsts f = host::rns_fold_consts(p, W);
                h.qmod.push_back(qm_p);
                h.negq.push_back(qm_p == 0 ? 0 : p - qm_p);
                h.qinv.push_back(qi);
                h.qinvp.push_back(shoup(qi, p));
                h.t1.push_back(f.t1), h.t1p.push_back(f.t1p), h.t2.push_back(f.t2), h.t2p.push_back(f.t2p);
                h.onep.push_back(f.onep);
            }
            return h;
        }

        using host::bc_padded;
        size_t ws_words(int L, int K) { return 5 * static_cast<size_t>(L) + static_cast<size_t>(L + 9) * bc_padded(K); }
    } // namespace

    template <typename T> struct BaseConvPlan<T>::Impl
    {
        int L = 0, K = 0, KP = 0;
        void* ws = nullptr;
        bool owns = false;
        kern::BcOffsets off{};

        void launch(const T* in, const T* c, T* out, int n_power, int count, BaseConvMode mode, bool divide,
                    hipStream_t stream) const
        {
            host::rns_check_n_power(n_power);
            if (mode != BaseConvMode::approximate && mode != BaseConvMode::centred)
                throw std::invalid_argument("Invalid mode!");
            if (count < 0)
                throw std::invalid_argument("Invalid count!");
            if (in == nullptr || out == nullptr || (divide && c == nullptr))
                throw std::invalid_argument("null pointer argument");
            if (count == 0)
                return;
            const unsigned long long total = static_cast<unsigned long long>(count) << n_power;
            const unsigned long long tiles = host::column_tiles(total, kern::BC_NT, "Invalid count!");
            if (host::rns_overlap(in, total * L * sizeof(T), out, total * K * sizeof(T)))
                throw std::invalid_argument("Base conversion input and output overlap!");
            const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(host::bc_ksplit(tiles, K)));
            const size_t lds = static_cast<size_t>(L) * kern::BC_NT * sizeof(T);
            const bool cen = mode == BaseConvMode::centred;
#define GPUNTT_BC_LAUNCH(CEN, DIV)                                                                                     \
    GPUNTT_LAUNCH((kern::base_convert<T, CEN, DIV>), grid, dim3(kern::BC_NT), lds, stream, in, c, out,                 \
                  static_cast<const T*>(ws), off, L, K, KP, n_power, total, kern::BcStrides<false>{})
            if (cen && divide)
                GPUNTT_BC_LAUNCH(true, true);
            else if (cen)
                GPUNTT_BC_LAUNCH(true, false);
            else if (divide)
                GPUNTT_BC_LAUNCH(false, true);
            else
                GPUNTT_BC_LAUNCH(false, false);
#undef GPUNTT_BC_LAUNCH
            GPUNTT_HIP_CHECK(hipGetLastError());
        }
    };

    namespace host
    {
        template <typename T> std::uint64_t bc_checked_value(const Modulus<T>& m) { return checked_value<T>(m); }
        template <typename T> BcHostConsts bc_derive(const Modulus<T>* qm, int L, const Modulus<T>* pm, int K)
        {
            return derive<T>(qm, L, pm, K);
        }
        size_t bc_image_words(int L, int K) { return ws_words(L, K); }

        template <typename T> std::vector<T> bc_image(const BcHostConsts& h, kern::BcOffsets& off)
        {
            const int L = h.L, K = h.K, KP = bc_padded(K);
            std::vector<T> img(ws_words(L, K), T(0));
            size_t at = 0;
            auto put = [&](const std::vector<std::uint64_t>& v, size_t slots) {
                const size_t first = at;
                for (size_t i = 0; i < v.size(); i++)
                    img[at + i] = static_cast<T>(v[i]);
                at += slots;
                return first;
            };
            std::vector<std::uint64_t> shift(L), mat(static_cast<size_t>(L) * KP, 0), ppad(h.p);
            for (int i = 0; i < L; i++)
            {
                shift[i] = h.blen[i] - 1;
                for (int j = 0; j < K; j++)
                    mat[static_cast<size_t>(i) * KP + j] = h.matrix[static_cast<size_t>(i) * K + j];
            }
            const size_t o_q = put(h.q, L), o_w = put(h.w, L), o_wp = put(h.wp, L), o_r = put(h.recip, L),
                         o_sh = put(shift, L), o_m = put(mat, static_cast<size_t>(L) * KP), o_p = put(ppad, KP),
                         o_nq = put(h.negq, KP), o_qi = put(h.qinv, KP), o_qip = put(h.qinvp, KP), o_t1 = put(h.t1, KP),
                         o_t1p = put(h.t1p, KP), o_t2 = put(h.t2, KP), o_t2p = put(h.t2p, KP), o_one = put(h.onep, KP);
            auto u = [](size_t v) { return static_cast<unsigned>(v); };
            off = kern::BcOffsets{u(o_q),  u(o_w),   u(o_wp), u(o_r),   u(o_sh), u(o_m),  u(o_p),  u(o_nq),
                                  u(o_qi), u(o_qip), u(o_t1), u(o_t1p), u(o_t2), u(o_t2p), u(o_one)};
            return img;
        }

        int bc_ksplit(unsigned long long tiles, int K)
        {
            return rns_split(tiles, bc_padded(K) / kern::BC_KB, g_bc_ksplit.load(std::memory_order_relaxed));
        }

        template <typename T>
        void bc_ref_convert(const BcHostConsts& c, const std::uint64_t* x, bool centred, std::uint64_t* conv)
        {
            constexpr int W = static_cast<int>(8 * sizeof(T));
            std::uint64_t y[BASECONV_MAX_COUNT];
            U128 zsum = static_cast<U128>(1) << (W - 1);
            for (int i = 0; i < c.L; i++)
            {
                y[i] = static_cast<std::uint64_t>(static_cast<U128>(x[i] % c.q[i]) * c.w[i] % c.q[i]);
                const int sh = static_cast<int>(c.blen[i]) - 1;
                const U128 z = c.recip[i] != 0 ? (static_cast<U128>(y[i]) * c.recip[i]) >> sh
                                               : static_cast<U128>(y[i]) << (W - sh);
                zsum += static_cast<T>(z);
            }
            const std::uint64_t v = centred ? static_cast<std::uint64_t>(static_cast<T>(zsum >> W)) : 0;
            for (int j = 0; j < c.K; j++)
            {
                const U128 p = c.p[j];
                U128 s = static_cast<U128>(v % c.p[j]) * c.negq[j] % p;
                for (int i = 0; i < c.L; i++)
                    s = (s + static_cast<U128>(y[i] % c.p[j]) * c.matrix[static_cast<size_t>(i) * c.K + j]) % p;
                conv[j] = static_cast<std::uint64_t>(s);
            }
        }

#define GPUNTT_BC_INTERNAL(T)                                                                                          \
    template std::uint64_t bc_checked_value<T>(const Modulus<T>&);                                                     \
    template BcHostConsts bc_derive<T>(const Modulus<T>*, int, const Modulus<T>*, int);                                \
    template std::vector<T> bc_image<T>(const BcHostConsts&, kern::BcOffsets&);                                        \
    template void bc_ref_convert<T>(const BcHostConsts&, const std::uint64_t*, bool, std::uint64_t*);
        GPUNTT_BC_INTERNAL(Data32)
        GPUNTT_BC_INTERNAL(Data64)
#undef GPUNTT_BC_INTERNAL
    } // namespace host

    template <typename T> size_t BaseConvPlan<T>::workspace_bytes(int in_count, int out_count)
    {
        if (in_count < 1 || in_count > BASECONV_MAX_COUNT)
            throw std::invalid_argument("Invalid in_count!");
        if (out_count < 1 || out_count > BASECONV_MAX_COUNT)
            throw std::invalid_argument("Invalid out_count!");
        return host::rns_align(ws_words(in_count, out_count) * sizeof(T));
    }

    template <typename T>
    BaseConvPlan<T>::BaseConvPlan(const Modulus<T>* in_moduli_host, int in_count, const Modulus<T>* out_moduli_host,
                                  int out_count, stream_t stream, void* workspace_device)
        : p_(nullptr)
    {
        const HostConsts h = derive<T>(in_moduli_host, in_count, out_moduli_host, out_count);
        const int L = h.L, K = h.K, KP = bc_padded(K);
        kern::BcOffsets off{};
        const std::vector<T> img = host::bc_image<T>(h, off);

        Impl* p = new Impl;
        p->L = L, p->K = K, p->KP = KP;
        try
        {
            if (workspace_device != nullptr)
                p->ws = workspace_device;
            else
            {
                GPUNTT_HIP_CHECK(hipMalloc(&p->ws, workspace_bytes(L, K)));
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
        p->off = off;
        p_ = p;
    }

    template <typename T> BaseConvPlan<T>::~BaseConvPlan()
    {
        if (p_ != nullptr && p_->owns)
            (void) hipFree(p_->ws);
        delete p_;
    }

    template <typename T>
    void BaseConvPlan<T>::convert(const T* device_in, T* device_out, int n_power, int count, BaseConvMode mode,
                                  stream_t stream) const
    {
        p_->launch(device_in, nullptr, device_out, n_power, count, mode, false, stream);
    }

    template <typename T>
    void BaseConvPlan<T>::convert_and_divide(const T* device_in, const T* device_c, T* device_out, int n_power,
                                             int count, BaseConvMode mode, stream_t stream) const
    {
        p_->launch(device_in, device_c, device_out, n_power, count, mode, true, stream);
    }

    template <typename T> int BaseConvPlan<T>::in_count() const { return p_->L; }
    template <typename T> int BaseConvPlan<T>::out_count() const { return p_->K; }
    template <typename T> bool BaseConvPlan<T>::owns_workspace() const { return p_->owns; }

    template <typename T>
    void BaseConvPlan<T>::constants(const Modulus<T>* in_moduli_host, int in_count, const Modulus<T>* out_moduli_host,
                                    int out_count, const BaseConvConstants<T>& out)
    {
        const HostConsts h = derive<T>(in_moduli_host, in_count, out_moduli_host, out_count);
        auto copy = [](const std::vector<std::uint64_t>& v, T* dst) {
            if (dst == nullptr)
                throw std::invalid_argument("null pointer argument");
            for (size_t i = 0; i < v.size(); i++)
                dst[i] = static_cast<T>(v[i]);
        };
        copy(h.w, out.qhat_inv);
        copy(h.wp, out.qhat_inv_shoup);
        copy(h.matrix, out.matrix);
        copy(h.qmod, out.q_mod_p);
        copy(h.qinv, out.q_inv_mod_p);
        copy(h.recip, out.recip);
        copy(h.blen, out.bit_length);
    }

    template class BaseConvPlan<Data32>;
    template class BaseConvPlan<Data64>;
} // namespace gpuntt
