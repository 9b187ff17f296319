// example_bfv_multiply.cpp -- a C++ caller of BfvMultiplyPlan<T> (gpuntt/rns/bfv_multiply.cuh): two messages encrypted on
// the host, multiplied on the GPU at constant scale, decrypted on the host.
//
//   base q = {q0} (Q = q0), auxiliary base {b0, b1}, full base {q0, b0, b1} (M = 3); plaintext modulus t, Delta = Q / t.
//     encrypt:  ct = (Delta m + e - a s, a) mod Q, s ternary, e in {-1, 0, 1}, a uniform            -- on the host
//     multiply: out = round(t (ct1 (x) ct2) / Q), three components                                  -- ONE call
//     decrypt:  round(t (out0 + out1 s + out2 s^2) / Q) mod t  =  m1 m2 mod (t, X^N + 1)            -- on the host
//   in coefficient form and through the NTT-form entry (input_ntt / output_ntt) of the same call; extend and scale_round
//   are compared with the plan's host references on the way.
//
//   ./example_bfv_multiply <LOGN <= 12 (u32: 5)> [u32]
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "gpuntt/ntt_merge/ntt.cuh"
#include "gpuntt/rns/bfv_multiply.cuh"

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
template <typename T> std::vector<T> download(const T* d, size_t words)
{
    std::vector<T> h(words);
    GPUNTT_CUDA_CHECK(hipMemcpy(h.data(), d, words * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}

// a * b in Z_q[X] / (X^N + 1), canonical words
template <typename T> std::vector<T> negacyclic(const std::vector<T>& a, const std::vector<T>& b, T q)
{
    const size_t n = a.size();
    std::vector<T> out(n, 0);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++)
        {
            const T p = mulmod(a[i], b[j], q);
            T& o = out[(i + j) % n];
            o = (i + j < n) ? static_cast<T>((static_cast<U128>(o) + p) % q) : static_cast<T>((static_cast<U128>(o) + q - p) % q);
        }
    return out;
}

template <typename T> int run(int logn, const Prime<T> (&primes)[3], int max_logn, T t)
{
    using namespace gpuntt;
    constexpr int L = 1, K = 2, M = 3, count = 1;
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
    const T Q = primes[0].q, delta = Q / t;

    std::mt19937_64 rng(41);
    std::vector<T> s(n), s2;
    for (auto& v : s)
        v = static_cast<T>((rng() % 3 + Q - 1) % Q); // -1, 0, 1 modulo Q
    s2 = negacyclic(s, s, Q);
    auto encrypt = [&](const std::vector<T>& m) { // T[2][count][L][N]
        std::vector<T> a(n), ct(2 * n);
        for (auto& v : a)
            v = static_cast<T>(rng() % Q);
        const std::vector<T> as = negacyclic(a, s, Q);
        for (size_t i = 0; i < n; i++)
        {
            const T e = static_cast<T>((rng() % 3 + Q - 1) % Q);
            ct[i] = static_cast<T>((static_cast<U128>(mulmod(delta, m[i], Q)) + e + Q - as[i]) % Q);
            ct[n + i] = a[i];
        }
        return ct;
    };
    auto decrypt = [&](const std::vector<T>& out) { // T[3][count][L][N]
        const std::vector<T> c0(out.begin(), out.begin() + n), c1(out.begin() + n, out.begin() + 2 * n),
            c2(out.begin() + 2 * n, out.end());
        const std::vector<T> p1 = negacyclic(c1, s, Q), p2 = negacyclic(c2, s2, Q);
        std::vector<T> m(n);
        for (size_t i = 0; i < n; i++)
        {
            const T v = static_cast<T>((static_cast<U128>(c0[i]) + p1[i] + p2[i]) % Q);
            // round(t v / Q) mod t of the centred v: for v >= Q / 2 the centred value is v - Q, and t (v - Q) / Q = t v / Q - t
            m[i] = static_cast<T>(((static_cast<U128>(v) * t * 2 + Q) / (2 * static_cast<U128>(Q))) % t);
        }
        return m;
    };
    std::vector<T> m1(n), m2(n);
    for (size_t i = 0; i < n; i++)
        m1[i] = static_cast<T>(rng() % t), m2[i] = static_cast<T>(rng() % t);
    std::vector<T> want = negacyclic(m1, m2, Q); // below N t^2 < Q: the product over the integers, reduced modulo t next
    for (size_t i = 0; i < n; i++)
    {
        // a coefficient of m1 m2 over Z lies in (-N t^2, N t^2); negacyclic() returned it modulo Q
        const T w = want[i];
        want[i] = w > Q / 2 ? static_cast<T>((t - (Q - w) % t) % t) : static_cast<T>(w % t);
    }
    const std::vector<T> x = encrypt(m1), y = encrypt(m2);

    T *d_x = upload(x), *d_y = upload(y), *d_out = nullptr, *d_full = nullptr;
    Root<T>*d_fwd = upload(fwd), *d_inv = upload(inv);
    GPUNTT_CUDA_CHECK(hipMalloc(&d_out, 3 * n * sizeof(T)));
    GPUNTT_CUDA_CHECK(hipMalloc(&d_full, 2 * M * n * sizeof(T)));
    void* d_scratch = nullptr;
    GPUNTT_CUDA_CHECK(hipMalloc(&d_scratch, BfvMultiplyPlan<T>::scratch_bytes(L, K, logn, count)));

    bool ok = true;
    {
        BfvMultiplyPlan<T> bfv(mods.data(), L, mods.data() + L, K, t, logn, d_fwd, d_inv, ninv.data(), poly,
                               4 * count * M, 0);
        NTTPlan<T> ntt_q(d_fwd, mods.data(), L, logn, poly, FORWARD, nullptr, 2 * count * L, 0);
        NTTPlan<T> intt_q(d_inv, mods.data(), L, logn, poly, INVERSE, ninv.data(), 3 * count * L, 0);
        ok = ok && bfv.scratch_bytes(count) == BfvMultiplyPlan<T>::scratch_bytes(L, K, logn, count);

        // the two conversions alone, against the plan's host references
        std::vector<T> full_ref(2 * M * n), out_ref(2 * L * n);
        bfv.extend(d_x, d_full, 2, 0);
        BfvMultiplyPlan<T>::reference_extend(mods.data(), L, mods.data() + L, K, x.data(), full_ref.data(), logn, 2);
        ok = ok && download(d_full, 2 * M * n) == full_ref;
        bfv.scale_round(d_full, d_out, 2, 0);
        BfvMultiplyPlan<T>::reference_scale_round(mods.data(), L, mods.data() + L, K, t, full_ref.data(), out_ref.data(),
                                                  logn, 2);
        ok = ok && download(d_out, 2 * L * n) == out_ref;

        // coefficient form in, coefficient form out
        bfv.multiply(d_x, d_y, d_out, count, false, false, d_scratch, 0);
        const std::vector<T> coeff = download(d_out, 3 * n);
        ok = ok && decrypt(coeff) == want;

        // NTT form in, NTT form out: the same three components, transformed
        ntt_q.execute(d_x, d_x, 2 * count * L, 0);
        ntt_q.execute(d_y, d_y, 2 * count * L, 0);
        bfv.multiply(d_x, d_y, d_out, count, true, true, d_scratch, 0);
        intt_q.execute(d_out, d_out, 3 * count * L, 0);
        ok = ok && download(d_out, 3 * n) == coeff;

        // an auxiliary base that cannot hold the product is refused
        try
        {
            BfvMultiplyPlan<T> small(mods.data(), L, mods.data() + L, 1, t, logn, nullptr, nullptr, nullptr, poly, 1, 0);
            ok = false;
        }
        catch (const std::invalid_argument&)
        {
        }
        GPUNTT_CUDA_CHECK(hipStreamSynchronize(0)); // the plans go out of scope
    }
    for (void* p : {(void*) d_x, (void*) d_y, (void*) d_out, (void*) d_full, (void*) d_fwd, (void*) d_inv, d_scratch})
        (void) hipFree(p);
    std::cout << (ok ? "All Correct." : "WRONG") << std::endl;
    return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    gpuntt::CudaDevice();
    const int logn = (argc >= 2) ? std::atoi(argv[1]) : 10;
    const bool u32 = (argc >= 3) && std::string(argv[2]) == "u32";
    // one q-prime is all the noise budget there is: t and N stay small (N t^2 and t^2 N^2 far below Q / t)
    if (logn < 1 || logn > (u32 ? 5 : 12))
        return EXIT_FAILURE;
    if (u32)
        return run<Data32>(logn, {{536641537u, 167028958u}, {536608769u, 417302965u}, {1073643521u, 269685106u}}, 14, 17u);
    return run<Data64>(logn,
                       {{576460752300015617ull, 296969298802020438ull},
                        {576460752298835969ull, 132309083155986965ull},
                        {1152921504598720513ull, 560939867933173424ull}},
                       16, 257ull);
}
