// example_baseconv.cpp -- a C++ caller of gpuntt/rns/base_conversion.cuh: a ModUp and the ModDown back.
//
//   ModUp    integers a with |a| < Q/2, given by their residues in the base q = {q0, q1}, are converted (centred) to
//            the base p = {p0, p1}: every word must be a mod p_j
//   ModDown  C = a P + r with |r| < P/2 lives in the base q u p; converting its p-part back to the base q and dividing
//            ((C - r) / P) must return the residues of a the ModUp started from
// Every word is checked against host integers (__int128: L = 2).
//
//   ./example_baseconv <LOGN> <COUNT> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/rns/base_conversion.cuh"

using I128 = __int128;

template <typename T> T residue(I128 v, T m)
{
    const I128 r = v % static_cast<I128>(m);
    return static_cast<T>(r < 0 ? r + m : r);
}

template <typename T> int run(int logn, int count, const T (&qv)[2], const T (&pv)[2])
{
    using namespace gpuntt;
    const size_t n = size_t(1) << logn;
    const Modulus<T> q[2] = {Modulus<T>(qv[0]), Modulus<T>(qv[1])}, p[2] = {Modulus<T>(pv[0]), Modulus<T>(pv[1])};
    const I128 Q = static_cast<I128>(qv[0]) * qv[1], P = static_cast<I128>(pv[0]) * pv[1];

    std::mt19937_64 rng(7);
    auto centred_below = [&](I128 m) { // uniform in (-(m/2 - m/2^20), m/2 - m/2^20)
        const I128 bound = m / 2 - (m >> 20);
        const I128 v = ((static_cast<I128>(rng()) << 64) | rng()) & ((static_cast<I128>(1) << 126) - 1);
        return v % (2 * bound - 1) - (bound - 1);
    };
    std::vector<I128> a(count * n), r(count * n);
    for (size_t i = 0; i < a.size(); i++)
        a[i] = centred_below(Q), r[i] = centred_below(P);

    // layout T[count][2][N]
    std::vector<T> a_q(count * 2 * n), a_p(count * 2 * n), c_q(count * 2 * n), c_p(count * 2 * n);
    for (int e = 0; e < count; e++)
        for (int j = 0; j < 2; j++)
            for (size_t i = 0; i < n; i++)
            {
                const I128 av = a[e * n + i], rv = r[e * n + i];
                const size_t at = (e * 2 + j) * n + i;
                a_q[at] = residue<T>(av, qv[j]);
                a_p[at] = residue<T>(av, pv[j]);
                // C = a P + r:  mod q_j from the residues (C itself has ~240 bits), mod p_j it is r
                const I128 aq = residue<T>(av, qv[j]), pq = residue<T>(P, qv[j]);
                c_q[at] = residue<T>(aq * pq % qv[j] + residue<T>(rv, qv[j]), qv[j]);
                c_p[at] = residue<T>(rv, pv[j]);
            }

    const size_t bytes = a_q.size() * sizeof(T);
    T *d_aq = nullptr, *d_up = nullptr, *d_cq = nullptr, *d_cp = nullptr;
    void* d_ws = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_aq, bytes));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_up, bytes));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_cq, bytes));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_cp, bytes));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_ws, BaseConvPlan<T>::workspace_bytes(2, 2)));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_aq, a_q.data(), bytes, hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_cq, c_q.data(), bytes, hipMemcpyHostToDevice));
    GPUNTT_CUDA_CHECK(hipMemcpy(d_cp, c_p.data(), bytes, hipMemcpyHostToDevice));

    bool ok = true;
    {
        BaseConvPlan<T> up(q, 2, p, 2, 0, d_ws); // caller-owned workspace
        BaseConvPlan<T> down(p, 2, q, 2, 0);     // the plan's own
        ok = ok && !up.owns_workspace() && down.owns_workspace();
        up.convert(d_aq, d_up, logn, count, BaseConvMode::centred, 0);
        down.convert_and_divide(d_cp, d_cq, d_cq, logn, count, BaseConvMode::centred, 0); // out aliases c
        std::vector<T> got_up(a_p.size()), got_down(a_q.size());
        GPUNTT_CUDA_CHECK(hipMemcpy(got_up.data(), d_up, bytes, hipMemcpyDeviceToHost));
        GPUNTT_CUDA_CHECK(hipMemcpy(got_down.data(), d_cq, bytes, hipMemcpyDeviceToHost));
        ok = ok && got_up == a_p && got_down == a_q;
        // a repeated modulus is refused
        try
        {
            const Modulus<T> twice[2] = {q[0], q[0]};
            BaseConvPlan<T> bad(twice, 2, p, 2, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
    }
    (void) hipFree(d_aq);
    (void) hipFree(d_up);
    (void) hipFree(d_cq);
    (void) hipFree(d_cp);
    (void) hipFree(d_ws);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 3) ? std::atoi(argv[1]) : 12;
    const int count = (argc >= 3) ? std::atoi(argv[2]) : 1;
    const bool u32 = (argc >= 4) && std::string(argv[3]) == "u32";
    if (u32)
        return run<Data32>(logn, count, {536870849u, 536870657u}, {268435361u, 268435313u});
    return run<Data64>(logn, count, {576460752302898689ull, 576460752302898433ull},
                       {288230376151449521ull, 288230376151449409ull});
}
