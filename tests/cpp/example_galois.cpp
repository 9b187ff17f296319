// example_galois.cpp -- a C++ caller of gpuntt/ntt_merge/galois.cuh: rotates NTT-form polynomials with
// GPU_Automorphism_NTT (one call, two elements: a slot rotation and the conjugation) and checks every word against
// NTTCPU<T>::ntt of the rotated coefficients, computed on the host from the definition a(X) -> a(X^k).
//
//   ./example_galois <LOGN> <BATCH> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/galois.cuh"

template <typename T> int run(int logn, int batch)
{
    using namespace gpuntt;
    NTTParameters<T> prm(logn, ReductionPolynomial::X_N_plus);
    NTTCPU<T> cpu(prm);
    const size_t n = prm.n;
    const T q = prm.modulus.value;
    const std::vector<std::uint32_t> elts = {GaloisElementForRotation(1, logn), GaloisElementForConjugation(logn)};

    std::mt19937 rng(1);
    std::uniform_int_distribution<std::uint64_t> below_q(0, q - 1);
    std::vector<T> coeffs(batch * n);
    for (T& c : coeffs)
        c = static_cast<T>(below_q(rng));

    // expected: NTT(sigma_k(a)) with sigma_k(a) = sum a_j X^(k j), X^N = -1
    std::vector<T> expected(elts.size() * batch * n);
    for (size_t g = 0; g < elts.size(); g++)
        for (int p = 0; p < batch; p++)
        {
            std::vector<T> rotated(n);
            for (size_t j = 0; j < n; j++)
            {
                const std::uint64_t e = (static_cast<std::uint64_t>(elts[g]) * j) % (2 * n);
                const T a = coeffs[p * n + j];
                rotated[e % n] = (e < n) ? a : (a == 0 ? T(0) : q - a);
            }
            const std::vector<T> f = cpu.ntt(rotated);
            std::copy(f.begin(), f.end(), expected.begin() + (g * batch + p) * n);
        }

    T *d_in = nullptr, *d_out = nullptr;
    Root<T>* d_table = nullptr;
    const std::vector<Root<T>> table = prm.gpu_root_of_unity_table_generator(prm.forward_root_of_unity_table);
    GPUNTT_CUDA_CHECK(hipMalloc(&d_in, coeffs.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_out, expected.size() * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_table, table.size() * sizeof(Root<T>)));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_in, coeffs.data(), coeffs.size() * sizeof(T), hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_table, table.data(), table.size() * sizeof(Root<T>), hipMemcpyHostToDevice));

    ntt_configuration<T> cfg = {.n_power = logn,
                                .ntt_type = FORWARD,
                                .ntt_layout = PerPolynomial,
                                .reduction_poly = ReductionPolynomial::X_N_plus,
                                .zero_padding = false,
                                .stream = 0};
    GPU_NTT_Inplace(d_in, d_table, prm.modulus, cfg, batch);
    GPU_Automorphism_NTT(d_in, d_out, elts.data(), static_cast<int>(elts.size()), logn, ReductionPolynomial::X_N_plus,
                         batch, 0);
    std::vector<T> got(expected.size());
    GPUNTT_CUDA_CHECK(hipMemcpy(got.data(), d_out, got.size() * sizeof(T), hipMemcpyDeviceToHost));

    bool ok = got == expected;
    // an even element is refused before anything is launched
    try
    {
        const std::uint32_t even = 2;
        GPU_Automorphism_NTT(d_in, d_out, &even, 1, logn, ReductionPolynomial::X_N_plus, batch, 0);
        ok = false;
    }
    catch (const std::invalid_argument&)
    {
    }
    (void) hipFree(d_in);
    (void) hipFree(d_out);
    (void) hipFree(d_table);
    if (ok)
        std::cout << "All Correct." << std::endl;
    else
        std::cout << "WRONG" << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 3) ? std::atoi(argv[1]) : 12;
    const int batch = (argc >= 3) ? std::atoi(argv[2]) : 1;
    const bool u32 = (argc >= 4) && std::string(argv[3]) == "u32";
    return u32 ? run<Data32>(logn, batch) : run<Data64>(logn, batch);
}
