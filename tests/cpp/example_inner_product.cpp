// example_inner_product.cpp -- a C++ caller of gpuntt/rns/inner_product.cuh: the data path of a hybrid key switch, every
// step a call of the library.
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3); one digit per q-prime (D = 2); a switching
//   key of C = 2 components.  For `count` polynomials c in coefficient form, base q:
//     ModUp      digit d is the limb [c]_{q_d}; BaseConvPlan {q_d} -> the other two primes extends it to the full base
//     GPU_NTT    one RNS call over the D * count * M polynomials of a = T[D][count][M][N]
//     inner      out[c][r][m] = sum_d a[d][r][m] * key[d][c][m]   (one launch; checked against reference())
//     GPU_INTT   one RNS call over the C * count * M polynomials of out = T[C][count][M][N]
//     ModDown    BaseConvPlan {p0} -> {q0, q1}, convert_and_divide: (x - [x]_p0) / p0 in the base q
//   The key is random (a real one encrypts the old secret under the new one; the data path is the same), so what is
//   checked is the inner product, word for word, and that the ModDown of its output is what host integers give.
//
//   ./example_inner_product <LOGN <= 14> <COUNT> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/base_conversion.cuh"
#include "gpuntt/rns/inner_product.cuh"

using U128 = unsigned __int128;

template <typename T> T mulmod(T a, T b, T m) { return static_cast<T>(static_cast<U128>(a) * b % m); }
template <typename T> T powmod(T a, std::uint64_t e, T m)
{
    T r = 1;
    for (; e != 0; e >>= 1, a = mulmod(a, a, m))
        if (e & 1)
            r = mulmod(r, a, m);
    return r;
}

template <typename T> struct Prime
{
    T q, psi; // psi: a primitive 2^(max_logn + 1)-th root of unity
};

template <typename T> int run(int logn, int count, const Prime<T> (&primes)[3], int max_logn)
{
    using namespace gpuntt;
    constexpr int M = 3, D = 2, C = 2;
    const size_t n = size_t(1) << logn;
    const auto poly = ReductionPolynomial::X_N_plus;

    std::vector<Modulus<T>> mods;
    std::vector<Root<T>> fwd(M * n), inv(M * n);
    std::vector<Ninverse<T>> ninv;
    for (int m = 0; m < M; m++)
    {
        const T q = primes[m].q, psi = powmod<T>(primes[m].psi, std::uint64_t(1) << (max_logn - logn), q);
        NTTParameters<T> prm(logn, NTTFactors<T>(Modulus<T>(q), mulmod(psi, psi, q), psi), poly);
        const auto f = prm.gpu_root_of_unity_table_generator(prm.forward_root_of_unity_table);
        const auto b = prm.gpu_root_of_unity_table_generator(prm.inverse_root_of_unity_table);
        std::copy(f.begin(), f.end(), fwd.begin() + m * n); // the table of modulus m starts at m << n_power
        std::copy(b.begin(), b.end(), inv.begin() + m * n);
        mods.push_back(prm.modulus);
        ninv.push_back(prm.n_inv);
    }

    std::mt19937_64 rng(11);
    std::vector<T> c_q(count * 2 * n), key(size_t(D) * C * M * n);
    for (size_t i = 0; i < c_q.size(); i++)
        c_q[i] = static_cast<T>(rng() % primes[(i / n) % 2].q);
    for (size_t i = 0; i < key.size(); i++)
        key[i] = static_cast<T>(rng() % primes[(i / n) % M].q);

    const size_t a_words = size_t(D) * count * M * n, out_words = size_t(C) * count * M * n;
    T *d_c = nullptr, *d_digit = nullptr, *d_up = nullptr, *d_a = nullptr, *d_key = nullptr, *d_out = nullptr,
      *d_res = nullptr;
    Root<T>*d_fwd = nullptr, *d_inv = nullptr;
    Modulus<T>* d_mods = nullptr;
    Ninverse<T>* d_ninv = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_c, c_q.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_digit, count * n * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_up, count * 2 * n * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_a, a_words * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_key, key.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_out, out_words * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_res, size_t(C) * count * 2 * n * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_fwd, fwd.size() * sizeof(Root<T>)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_inv, inv.size() * sizeof(Root<T>)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_mods, M * sizeof(Modulus<T>)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_ninv, M * sizeof(Ninverse<T>)));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_c, c_q.data(), c_q.size() * sizeof(T), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_key, key.data(), key.size() * sizeof(T), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_fwd, fwd.data(), fwd.size() * sizeof(Root<T>), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_inv, inv.data(), inv.size() * sizeof(Root<T>), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_mods, mods.data(), M * sizeof(Modulus<T>), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_ninv, ninv.data(), M * sizeof(Ninverse<T>), hipMemcpyHostToDevice));
    auto copy_poly = [&](T* dst, const T* src) {
        GPUNTT_CUDA_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, 0));
    };

    bool ok = true;
    {
        // ---- ModUp: digit d from {q_d} to the other two primes of the full base, then into its stack a[d]
        for (int d = 0; d < D; d++)
        {
            const int others[2] = {1 - d, 2};
            const Modulus<T> from[1] = {mods[d]}, to[2] = {mods[others[0]], mods[others[1]]};
            BaseConvPlan<T> up(from, 1, to, 2, 0);
            for (int r = 0; r < count; r++)
                copy_poly(d_digit + r * n, d_c + (r * 2 + d) * n);
            up.convert(d_digit, d_up, logn, count, BaseConvMode::centred, 0);
            for (int r = 0; r < count; r++)
            {
                T* stack = d_a + (size_t(d) * count + r) * M * n;
                copy_poly(stack + d * n, d_digit + r * n);
                copy_poly(stack + others[0] * n, d_up + (r * 2 + 0) * n);
                copy_poly(stack + others[1] * n, d_up + (r * 2 + 1) * n);
            }
            GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // `up` goes out of scope
        }
        // ---- one forward transform over all D * count * M polynomials
        ntt_rns_configuration<T> cfg_f = {.n_power = logn, .ntt_type = FORWARD, .ntt_layout = PerPolynomial,
                                          .reduction_poly = poly, .zero_padding = false, .stream = 0};
        GPU_NTT_Inplace(d_a, d_fwd, d_mods, cfg_f, D * count * M, M);
        // ---- the inner product, in a caller-owned workspace
        void* d_ws = nullptr;
        GPUNTT_CUDA_CHECK(hipMalloc(&d_ws, InnerProductPlan<T>::workspace_bytes(M)));
        {
            InnerProductPlan<T> ip(mods.data(), M, 0, d_ws);
            ok = ok && !ip.owns_workspace();
            ip.multiply_accumulate(d_a, d_key, d_out, logn, D, C, count, false, M, nullptr, 0);
            std::vector<T> a(a_words), got(out_words), want(out_words);
            GPUNTT_CUDA_CHECK(hipMemcpy(a.data(), d_a, a_words * sizeof(T), hipMemcpyDeviceToHost));
            GPUNTT_CUDA_CHECK(hipMemcpy(got.data(), d_out, out_words * sizeof(T), hipMemcpyDeviceToHost));
            InnerProductPlan<T>::reference(mods.data(), M, a.data(), key.data(), want.data(), logn, D, C, count, false,
                                           M, nullptr);
            ok = ok && got == want;
            // out overlapping an input is refused
            try
            {
                ip.multiply_accumulate(d_a, d_key, d_a, logn, D, C, count, false, M, nullptr, 0);
                ok = false;
            }
            catch (const std::invalid_argument&)
            {
            }
        }
        (void) hipFree(d_ws);
        // ---- one inverse transform over all C * count * M polynomials
        ntt_rns_configuration<T> cfg_i = {.n_power = logn, .ntt_type = INVERSE, .ntt_layout = PerPolynomial,
                                          .reduction_poly = poly, .zero_padding = false, .mod_inverse = d_ninv,
                                          .stream = 0};
        GPU_INTT_Inplace(d_out, d_inv, d_mods, cfg_i, C * count * M, M);
        // ---- ModDown: every stack is {q0, q1, p0}: the p0 limb converted to the base q, subtracted and divided
        const Modulus<T> from[1] = {mods[2]}, to[2] = {mods[0], mods[1]};
        BaseConvPlan<T> down(from, 1, to, 2, 0);
        for (int s = 0; s < C * count; s++)
            down.convert_and_divide(d_out + (size_t(s) * M + 2) * n, d_out + size_t(s) * M * n, d_res + size_t(s) * 2 * n,
                                    logn, 1, BaseConvMode::centred, 0);
        std::vector<T> x(out_words), got(size_t(C) * count * 2 * n);
        GPUNTT_CUDA_CHECK(hipMemcpy(x.data(), d_out, out_words * sizeof(T), hipMemcpyDeviceToHost));
        GPUNTT_CUDA_CHECK(hipMemcpy(got.data(), d_res, got.size() * sizeof(T), hipMemcpyDeviceToHost));
        // host: r = the representative of [x]_p0 in [-p0/2, p0/2) (random data keeps clear of the rounding band),
        // result_j = ([x]_qj - r) * p0^-1 mod q_j
        const T p0 = primes[2].q;
        for (int s = 0; s < C * count && ok; s++)
            for (int j = 0; j < 2 && ok; j++)
            {
                const T q = primes[j].q, pinv = powmod<T>(p0 % q, q - 2, q);
                for (size_t i = 0; i < n && ok; i++)
                {
                    const T xp = x[(size_t(s) * M + 2) * n + i], xq = x[(size_t(s) * M + j) * n + i];
                    const bool neg = xp >= p0 - p0 / 2; // r = xp - p0
                    const T rq = neg ? (q - (p0 - xp) % q) % q : xp % q;
                    ok = got[(size_t(s) * 2 + j) * n + i] == mulmod<T>((xq + q - rq) % q, pinv, q);
                }
            }
    }
    for (void* p : {(void*) d_c, (void*) d_digit, (void*) d_up, (void*) d_a, (void*) d_key, (void*) d_out, (void*) d_res,
                    (void*) d_fwd, (void*) d_inv, (void*) d_mods, (void*) d_ninv})
        (void) hipFree(p);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 3) ? std::atoi(argv[1]) : 12;
    const int count = (argc >= 3) ? std::atoi(argv[2]) : 1;
    const bool u32 = (argc >= 4) && std::string(argv[3]) == "u32";
    if (logn < 1 || logn > 14 || count < 1)
        return EXIT_FAILURE;
    if (u32)
        return run<Data32>(logn, count, {{536641537u, 167028958u}, {536608769u, 417302965u}, {1073643521u, 269685106u}},
                           14);
    return run<Data64>(logn, count,
                       {{576460752300015617ull, 296969298802020438ull},
                        {576460752298835969ull, 132309083155986965ull},
                        {1152921504598720513ull, 560939867933173424ull}},
                       16);
}
