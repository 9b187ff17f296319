// example_key_switch.cpp -- a C++ caller of gpuntt/rns/key_switch.cuh: the hybrid key switch of example_inner_product.cpp
// on ONE plan.
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3), digit size alpha = 1 (D = 2), a switching key
//   of C = 2 components.  For `count` polynomials c in coefficient form, base q, KeySwitchPlan::apply runs
//     mod_up (all digits, one launch) -> forward NTT over D * count * M -> inner product -> inverse NTT over C * count * M
//     -> mod_down (all stacks, one launch, the special limb read in place)
//   with the digit stacks and the accumulators in a caller-owned scratch and every constant in a caller-owned workspace.
//   Checked: mod_up and mod_down word for word against the plan's host references, apply against decompose +
//   switch_digits, and apply against the host chain reference_mod_down(INTT(InnerProductPlan::reference(NTT(a)))) with the
//   transforms taken from the GPU.  The key is random (a real one encrypts the old secret under the new one; the data path
//   is the same).
//
//   ./example_key_switch <LOGN <= 14> <COUNT> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/key_switch.cuh"

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

template <typename T> std::vector<T> download(const T* d, size_t words)
{
    std::vector<T> h(words);
    GPUNTT_CUDA_CHECK(hipMemcpy(h.data(), d, words * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}

template <typename T> int run(int logn, int count, const Prime<T> (&primes)[3], int max_logn)
{
    using namespace gpuntt;
    constexpr int L = 2, K = 1, M = 3, ALPHA = 1, C = 2;
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
    const int D = KeySwitchPlan<T>::digits(L, ALPHA);

    std::mt19937_64 rng(11);
    std::vector<T> c_q(count * L * n), key(size_t(D) * C * M * n);
    for (size_t i = 0; i < c_q.size(); i++)
        c_q[i] = static_cast<T>(rng() % primes[(i / n) % L].q);
    for (size_t i = 0; i < key.size(); i++)
        key[i] = static_cast<T>(rng() % primes[(i / n) % M].q);

    const size_t a_words = size_t(D) * count * M * n, acc_words = size_t(C) * count * M * n,
                 out_words = size_t(C) * count * L * n;
    T *d_c = nullptr, *d_a = nullptr, *d_acc = nullptr, *d_key = nullptr, *d_out = nullptr, *d_out2 = nullptr;
    Root<T>*d_fwd = nullptr, *d_inv = nullptr;
    void *d_ws = nullptr, *d_scratch = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_c, c_q.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_a, a_words * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_acc, acc_words * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_key, key.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_out, out_words * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_out2, out_words * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_fwd, fwd.size() * sizeof(Root<T>)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_inv, inv.size() * sizeof(Root<T>)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_ws, KeySwitchPlan<T>::workspace_bytes(L, K, ALPHA, logn)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, KeySwitchPlan<T>::scratch_bytes(L, K, ALPHA, logn, count, C)));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_c, c_q.data(), c_q.size() * sizeof(T), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_key, key.data(), key.size() * sizeof(T), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_fwd, fwd.data(), fwd.size() * sizeof(Root<T>), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_inv, inv.data(), inv.size() * sizeof(Root<T>), hipMemcpyHostToDevice));

    bool ok = true;
    {
        KeySwitchPlan<T> ks(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                            D * count * M, M, nullptr, 0, d_ws);
        ok = ok && !ks.owns_workspace() && ks.digits() == D;

        // ---- ModUp of both digits: one launch, against the host reference
        ks.mod_up(d_c, d_a, count, BaseConvMode::centred, 0);
        std::vector<T> want_a(a_words);
        KeySwitchPlan<T>::reference_mod_up(mods.data(), L, mods.data() + L, K, ALPHA, c_q.data(), want_a.data(), logn,
                                           count, BaseConvMode::centred);
        ok = ok && download(d_a, a_words) == want_a;

        // ---- the whole switch in one call, and as the two halves a hoisting caller uses
        ks.apply(d_c, d_key, d_out, count, C, false, false, d_scratch, 0);
        ks.decompose(d_c, d_a, count, false, d_scratch, 0);
        const std::vector<T> a_ntt = download(d_a, a_words); // NTT form, digit-major
        ks.switch_digits(d_a, d_key, d_out2, count, C, false, d_scratch, 0);
        const std::vector<T> got = download(d_out, out_words);
        ok = ok && got == download(d_out2, out_words);

        // ---- the host chain: inner product reference on the GPU's NTT of a, the GPU's inverse NTT of that, then the
        // ModDown reference
        std::vector<T> acc(acc_words), want(out_words);
        InnerProductPlan<T>::reference(mods.data(), M, a_ntt.data(), key.data(), acc.data(), logn, D, C, count, false, M,
                                       nullptr);
        GPUNTT_CUDA_CHECK(hipMemcpy(d_acc, acc.data(), acc_words * sizeof(T), hipMemcpyHostToDevice));
        NTTPlan<T> intt(d_inv, mods.data(), M, logn, poly, INVERSE, ninv.data(), C * count * M, 0);
        intt.execute(d_acc, d_acc, C * count * M, 0);
        KeySwitchPlan<T>::reference_mod_down(mods.data(), L, mods.data() + L, K, download(d_acc, acc_words).data(),
                                             want.data(), logn, C * count);
        ok = ok && got == want;

        // ---- ModDown on its own: all stacks in one launch
        ks.mod_down(d_acc, d_out2, C * count, 0);
        ok = ok && download(d_out2, out_words) == want;

        // overlapping buffers are refused
        try
        {
            ks.mod_down(d_acc, d_acc, C * count, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (void* p : {(void*) d_c, (void*) d_a, (void*) d_acc, (void*) d_key, (void*) d_out, (void*) d_out2, (void*) d_fwd,
                    (void*) d_inv, d_ws, d_scratch})
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
