// example_multiply_rescale.cpp -- a C++ caller of the rescaling calls of KeySwitchPlan<T> (gpuntt/rns/key_switch.cuh): two
// pairs of ciphertexts multiplied, relinearized and rescaled, the rescale inside the product's own ModDown.
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3), digit size alpha = 1 (D = 2), rescale_limbs = 1:
//   the calls drop q1 and leave a ciphertext over {q0}.
//     two steps:  multiply_relinearize(x, y, key), then rescale of its result
//                   -- in coefficient form compared word for word with reference_rescale on the host,
//                   -- in NTT form (only the dropped limb is inverse-transformed) compared with the same words after an
//                      inverse transform over q0
//     one call:   multiply_relinearize_rescale(x, y, key): ONE rounding, by p0 q1, where the two steps round twice; the
//                 two results differ by at most 1 per coefficient (key_switch.cuh), which is what is checked, in
//                 coefficient and in NTT form
//   A plan built without rescale_limbs refuses the call.  The key is random (a real key encrypts s^2; the data path is the
//   same).
//
//   ./example_multiply_rescale <LOGN <= 14> [u32]
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

template <typename T> T* upload(const std::vector<T>& h)
{
    T* d = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d, h.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T> T* device_words(size_t words)
{
    T* d = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d, words * sizeof(T)));
    return d;
}
template <typename T> std::vector<T> download(const T* d, size_t words)
{
    std::vector<T> h(words);
    GPUNTT_CUDA_CHECK(hipMemcpy(h.data(), d, words * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}

// a and b canonical modulo q: is a - b in {-1, 0, 1} modulo q?
template <typename T> bool within_one(T a, T b, T q)
{
    const T d = a >= b ? a - b : a + (q - b);
    return d == 0 || d == 1 || d == q - 1;
}

template <typename T> int run(int logn, const Prime<T> (&primes)[3], int max_logn)
{
    using namespace gpuntt;
    constexpr int L = 2, K = 1, M = 3, ALPHA = 1, R = 1, KEEP = L - R, count = 2, stacks = 2 * count;
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

    std::mt19937_64 rng(41);
    const size_t ct_words = size_t(stacks) * L * n, out_words = size_t(stacks) * KEEP * n, key_words = size_t(D) * 2 * M * n;
    std::vector<T> x(ct_words), y(ct_words), key(key_words);
    for (size_t i = 0; i < ct_words; i++)
    {
        x[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // T[2][count][L][N], NTT form
        y[i] = static_cast<T>(rng() % primes[(i / n) % L].q);
    }
    for (size_t i = 0; i < key_words; i++)
        key[i] = static_cast<T>(rng() % primes[(i / n) % M].q);
    T *d_x = upload(x), *d_y = upload(y), *d_key = upload(key), *d_full = device_words<T>(ct_words),
      *d_out = device_words<T>(out_words), *d_fused = device_words<T>(out_words);
    Root<T>*d_fwd = upload(fwd), *d_inv = upload(inv);
    void *d_scratch = nullptr, *d_rescale_scratch = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, KeySwitchPlan<T>::scratch_bytes(L, K, ALPHA, logn, count, 2)));

    bool ok = true;
    {
        KeySwitchPlan<T> ks(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                            D * count * M, M, nullptr, 0, nullptr, R);
        NTTPlan<T> intt_keep(d_inv, mods.data(), KEEP, logn, poly, INVERSE, ninv.data(), stacks * KEEP, 0);
        ok = ok && ks.rescale_limbs() == R;
        const size_t old_bytes = KeySwitchPlan<T>::workspace_bytes(L, K, ALPHA, logn); // R = 0 is the plan as it was
        ok = ok && KeySwitchPlan<T>::workspace_bytes(L, K, ALPHA, logn, 0) == old_bytes;
        ok = ok && KeySwitchPlan<T>::workspace_bytes(L, K, ALPHA, logn, R) > old_bytes;
        GPUNTT_CUDA_CHECK(hipMalloc(&d_rescale_scratch, ks.rescale_scratch_bytes(stacks)));

        // two steps, coefficient form: the product, then rescale -- one launch, word for word the host reference
        ks.multiply_relinearize(d_x, d_y, d_key, d_full, count, false, d_scratch, 0);
        ks.rescale(d_full, d_out, stacks, false, nullptr, 0);
        const std::vector<T> product = download(d_full, ct_words);
        std::vector<T> two_steps(out_words);
        KeySwitchPlan<T>::reference_rescale(mods.data(), L, R, product.data(), two_steps.data(), logn, stacks);
        ok = ok && download(d_out, out_words) == two_steps;

        // two steps, NTT form: the same words after an inverse transform over the kept limb
        ks.multiply_relinearize(d_x, d_y, d_key, d_full, count, true, d_scratch, 0);
        ks.rescale(d_full, d_out, stacks, true, d_rescale_scratch, 0);
        intt_keep.execute(d_out, d_out, stacks * KEEP, 0);
        ok = ok && download(d_out, out_words) == two_steps;

        // one call: the rescale inside the product's ModDown, ONE rounding -- within 1 of the two steps, both forms
        ks.multiply_relinearize_rescale(d_x, d_y, d_key, d_fused, count, false, d_scratch, 0);
        const std::vector<T> fused = download(d_fused, out_words);
        size_t differ = 0;
        for (size_t i = 0; i < out_words; i++)
        {
            ok = ok && within_one(fused[i], two_steps[i], primes[0].q);
            differ += fused[i] != two_steps[i];
        }
        std::cout << differ << " of " << out_words << " coefficients differ (by one) from the two-step result" << std::endl;
        ks.multiply_relinearize_rescale(d_x, d_y, d_key, d_fused, count, true, d_scratch, 0);
        intt_keep.execute(d_fused, d_fused, stacks * KEEP, 0);
        ok = ok && download(d_fused, out_words) == fused;

        // a plan without rescale_limbs refuses the call before anything is launched
        KeySwitchPlan<T> plain(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                               D * count * M, M, nullptr, 0);
        try
        {
            plain.multiply_relinearize_rescale(d_x, d_y, d_key, d_fused, count, false, d_scratch, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (void* p : {(void*) d_x, (void*) d_y, (void*) d_key, (void*) d_full, (void*) d_out, (void*) d_fused, (void*) d_fwd,
                    (void*) d_inv, d_scratch, d_rescale_scratch})
        (void) hipFree(p);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 2) ? std::atoi(argv[1]) : 12;
    const bool u32 = (argc >= 3) && std::string(argv[2]) == "u32";
    if (logn < 1 || logn > 14)
        return EXIT_FAILURE;
    if (u32)
        return run<Data32>(logn, {{536641537u, 167028958u}, {536608769u, 417302965u}, {1073643521u, 269685106u}}, 14);
    return run<Data64>(logn,
                       {{576460752300015617ull, 296969298802020438ull},
                        {576460752298835969ull, 132309083155986965ull},
                        {1152921504598720513ull, 560939867933173424ull}},
                       16);
}
