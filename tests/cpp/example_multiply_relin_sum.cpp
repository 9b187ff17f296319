// example_multiply_relin_sum.cpp -- a C++ caller of KeySwitchPlan<T>::multiply_relinearize_sum
// (gpuntt/rns/key_switch.cuh): sum_t x_t * y_t over three pairs of ciphertext batches, in ONE key switch and ONE ModDown
// ("lazy relinearization": an encrypted dot product of length three).
//
//   base q = {q0, q1}, special prime p0, full base {q0, q1, p0} (M = 3), digit size alpha = 1 (D = 2), T = 3 terms.
//     one call:     multiply_relinearize_sum({x_t}, {y_t}, T, key)
//     composition:  per input the three summed tensor terms d0 = sum_t x0 y0, d1 = sum_t x0 y1 + x1 y0, d2 = sum_t x1 y1
//                   through a q-base InnerProductPlan::multiply_accumulate over gathered polynomials (D = T, 2 T, T; the
//                   polynomials of y in the key's place), apply(d2, key, components = 2, input_ntt), and the two
//                   additions on the host -- with the q-base INTT of d0 and d1 first when the output is in coefficient
//                   form                                                                          -- the definition
//   and every output word of the two is compared, in coefficient and in NTT form; then with one term against
//   multiply_relinearize, and squares written over one of their operands.  The result is NOT word for word the sum of
//   three multiply_relinearize calls (that rounds three times); only the decrypted values agree.
//   The key is random (a real key encrypts s^2; the data path is the same).
//
//   ./example_multiply_relin_sum <LOGN <= 14> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/inner_product.cuh"
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

template <typename T> int run(int logn, const Prime<T> (&primes)[3], int max_logn)
{
    using namespace gpuntt;
    constexpr int L = 2, K = 1, M = 3, ALPHA = 1, count = 2, TERMS = 3;
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

    std::mt19937_64 rng(37);
    const size_t stack = size_t(L) * n, comp = count * stack, ct_words = 2 * comp, key_words = size_t(D) * 2 * M * n;
    std::vector<T> key(key_words);
    std::vector<T*> d_x(TERMS), d_y(TERMS);
    for (int t = 0; t < TERMS; t++)
    {
        std::vector<T> x(ct_words), y(ct_words);
        for (size_t i = 0; i < ct_words; i++)
        {
            x[i] = static_cast<T>(rng() % primes[(i / n) % L].q); // T[2][count][L][N], NTT form
            y[i] = static_cast<T>(rng() % primes[(i / n) % L].q);
        }
        d_x[t] = upload(x), d_y[t] = upload(y);
    }
    for (size_t i = 0; i < key_words; i++)
        key[i] = static_cast<T>(rng() % primes[(i / n) % M].q);
    T *d_key = upload(key), *d_out = device_words<T>(ct_words), *d_one = device_words<T>(ct_words),
      *d_d = device_words<T>(3 * comp), *d_k = device_words<T>(ct_words), *d_ga = device_words<T>(2 * TERMS * stack),
      *d_gk = device_words<T>(2 * TERMS * stack);
    Root<T>*d_fwd = upload(fwd), *d_inv = upload(inv);
    void *d_scratch = nullptr, *d_scratch2 = nullptr;
    const size_t sbytes = KeySwitchPlan<T>::scratch_bytes(L, K, ALPHA, logn, count, 2);
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, sbytes));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch2, sbytes));
    // digit `slot` of a gathered operand: one input's L limbs
    auto gather = [&](T* dst, int slot, const T* src) {
        GPUNTT_CUDA_CHECK(hipMemcpy(dst + slot * stack, src, stack * sizeof(T), hipMemcpyDeviceToDevice));
    };

    bool ok = true;
    {
        KeySwitchPlan<T> ks(mods.data(), L, mods.data() + L, K, ALPHA, logn, d_fwd, d_inv, ninv.data(), poly,
                            D * count * M, M, nullptr, 0);
        InnerProductPlan<T> inner_q(mods.data(), L, 0);
        NTTPlan<T> intt_q(d_inv, mods.data(), L, logn, poly, INVERSE, ninv.data(), 2 * count * L, 0);
        ok = ok && ks.scratch_bytes(count, 2) == sbytes;

        // the definition of sum_t x_t * y_t, for both output forms
        auto composition = [&](const std::vector<const T*>& px, const std::vector<const T*>& py, bool output_ntt) {
            const int terms = static_cast<int>(px.size());
            for (int r = 0; r < count; r++)
            {
                // per term: (x0, y0) in slot t and (x1, y1) in slot terms + t -- d0 reads the first half, d2 the second
                for (int t = 0; t < terms; t++)
                {
                    gather(d_ga, t, px[t] + r * stack), gather(d_ga, terms + t, px[t] + comp + r * stack);
                    gather(d_gk, t, py[t] + r * stack), gather(d_gk, terms + t, py[t] + comp + r * stack);
                }
                inner_q.multiply_accumulate(d_ga, d_gk, d_d + r * stack, logn, terms, 1, 1, false, L, nullptr, 0);
                inner_q.multiply_accumulate(d_ga + terms * stack, d_gk + terms * stack, d_d + 2 * comp + r * stack, logn,
                                            terms, 1, 1, false, L, nullptr, 0);
                GPUNTT_CUDA_CHECK(hipStreamSynchronize(0));
                // the cross term: the "key" is y1 of every term, then y0 of every term
                for (int t = 0; t < terms; t++)
                    gather(d_gk, t, py[t] + comp + r * stack), gather(d_gk, terms + t, py[t] + r * stack);
                inner_q.multiply_accumulate(d_ga, d_gk, d_d + comp + r * stack, logn, 2 * terms, 1, 1, false, L, nullptr,
                                            0);
                GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the gathers are reused by the next input
            }
            ks.apply(d_d + 2 * comp, d_key, d_k, count, 2, true, output_ntt, d_scratch2, 0);
            if (!output_ntt)
                intt_q.execute(d_d, d_d, 2 * count * L, 0);
            std::vector<T> want = download(d_k, ct_words);
            const std::vector<T> low = download(d_d, ct_words);
            for (size_t i = 0; i < ct_words; i++)
                want[i] = static_cast<T>((static_cast<U128>(want[i]) + low[i]) % primes[(i / n) % L].q);
            return want;
        };

        const std::vector<const T*> xs(d_x.begin(), d_x.end()), ys(d_y.begin(), d_y.end());
        for (const bool output_ntt : {false, true})
        {
            ks.multiply_relinearize_sum(xs.data(), ys.data(), TERMS, d_key, d_out, count, output_ntt, d_scratch, 0);
            ok = ok && download(d_out, ct_words) == composition(xs, ys, output_ntt);
            // one term: multiply_relinearize's words
            ks.multiply_relinearize_sum(xs.data(), ys.data(), 1, d_key, d_out, count, output_ntt, d_scratch, 0);
            ks.multiply_relinearize(d_x[0], d_y[0], d_key, d_one, count, output_ntt, d_scratch, 0);
            ok = ok && download(d_out, ct_words) == download(d_one, ct_words);
        }
        // a sum of squares, written over one of its operands: out may be exactly any x[t] or y[t]
        const std::vector<T> squares = composition(xs, xs, true);
        ks.multiply_relinearize_sum(xs.data(), xs.data(), TERMS, d_key, d_x[1], count, true, d_scratch, 0);
        ok = ok && download(d_x[1], ct_words) == squares;

        // an output that overlaps an operand without being exactly it, and more terms than the call takes, are refused
        // before anything is launched
        try
        {
            ks.multiply_relinearize_sum(xs.data(), ys.data(), TERMS, d_key, d_y[2] + n, count, false, d_scratch, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        try
        {
            ks.multiply_relinearize_sum(xs.data(), ys.data(), KEYSWITCH_MAX_TERMS + 1, d_key, d_out, count, false, d_scratch,
                                        0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (T* p : d_x)
        (void) hipFree(p);
    for (T* p : d_y)
        (void) hipFree(p);
    for (void* p : {(void*) d_key, (void*) d_out, (void*) d_one, (void*) d_d, (void*) d_k, (void*) d_ga, (void*) d_gk,
                    (void*) d_fwd, (void*) d_inv, d_scratch, d_scratch2})
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
