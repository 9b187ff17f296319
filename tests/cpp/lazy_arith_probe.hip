// lazy_arith_probe.hip -- runs every primitive of gpu-ntt_amd/csrc/lazy.hpp on a file of operands and writes the raw
// result words, so that tests/test_gpu_lazy_arith.py can compare each one with exact integers (tests/lazy_model.py).
// The arithmetic is the header's own: nothing of it is restated here.
//
//   lazy_arith_probe run CASES OUT     one family's case file -> one record of result words per primitive (GPU)
//   lazy_arith_probe norm LIST         lines "W q bit"            -> "q bit sh c M hi"   (host only, no HIP call)
//   lazy_arith_probe plan LIST         lines "bu bv limit tb"     -> "ct ku out gs ku kv c ko out_u" (host only)
//
// Case file (little endian): 8 x u64 header {MAGIC, family, ncase, nuni, 0, 0, 0, 0}, then arrays of the family's word
// (u64 or u32): per case x, acc, q, bit, w, wp; per block of 64 cases qb, bitb, wu, wpu.  One block is one wave:
//   * families with a wave-uniform modulus read q / bit from qb / bitb at blockIdx.x (scalar registers), the per-lane
//     moduli (VQ) families from q / bit at the case index (vector registers);
//   * the UNI forms of the products read the twiddle {wu, wpu} at blockIdx.x (scalar registers) and run on the first
//     `nuni` cases only (in a VQ family the blocks behind them mix moduli, and a twiddle's quotient belongs to ONE);
//     the other forms read {w, wp} per lane.
// Output file: 4 x u64 header {MAGIC, family, ncase, nrec}, then nrec records {char name[16]; word result[ncase]}.
#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../gpu-ntt_amd/csrc/lazy.hpp"

using namespace gpuntt::lazy;

namespace
{
    constexpr uint64_t MAGIC = 0x424f52505a414c4cull; // the bytes "LAZPROB" behind an 'L'
    constexpr int WAVE = 64;
    constexpr unsigned long long MAX_CASES = 1ull << 18;

#define HIP_CHECK(expr)                                                                                        \
    do                                                                                                         \
    {                                                                                                          \
        const hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                                  \
        {                                                                                                      \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e_));         \
            std::exit(3);                                                                                      \
        }                                                                                                      \
    } while (0)

    template <typename T> struct Args
    {
        const T *x, *acc, *q, *bit, *w, *wp; // per case
        const T *qb, *bitb, *wu, *wpu;       // per block
        const NormConst *ncl, *ncb;          // per case / per block, from the header's norm_const_of on the host
        unsigned n;                          // cases this launch covers (a multiple of WAVE)
    };

    // ---- one struct per primitive: run(m, a, i) is the call a kernel makes -------------------------------------
    template <typename T> __device__ __forceinline__ Tw<T> tw_uni(const Args<T>& a) { return Tw<T>{a.wu[blockIdx.x], a.wpu[blockIdx.x]}; }
    template <typename T> __device__ __forceinline__ Tw<T> tw_lane(const Args<T>& a, unsigned i) { return Tw<T>{a.w[i], a.wp[i]}; }
    template <bool UNI, typename T> __device__ __forceinline__ Tw<T> tw_of(const Args<T>& a, unsigned i)
    {
        if constexpr (UNI)
            return tw_uni(a);
        else
            return tw_lane(a, i);
    }

    template <bool UNI> struct OpMul
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return m.template mul<UNI>(a.x[i], tw_of<UNI>(a, i));
        }
    };
    template <bool UNI, bool ZERO> struct OpMulAcc
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return m.template mul_acc<UNI, ZERO>(a.x[i], tw_of<UNI>(a, i), a.acc[i]);
        }
    };
    template <bool UNI> struct OpMulAccRaw // 64-bit only
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return m.template mul_acc_raw<UNI, false>(a.x[i], tw_of<UNI>(a, i), a.acc[i]);
        }
    };
    template <bool UNI> struct OpMulc // 32-bit only: the twiddle arrives negated
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            const Tw<T> t = tw_of<UNI>(a, i);
            return m.template mulc<UNI>(a.x[i], static_cast<T>(0u - t.w), t.wp);
        }
    };
    template <int K> struct OpCsub
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return m.template csub<K>(a.x[i]);
        }
    };
    template <int K> struct OpCsubC // 32-bit only: handed the COMPLEMENT of x, so that its edges are x = K q - 1 / K q too
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return m.template csub_c<K>(static_cast<T>(~a.x[i]));
        }
    };
    template <bool VQ> struct OpShl1Add // k: any word; wave-uniform unless VQ
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return m.shl1_add(a.x[i], VQ ? a.acc[i] : a.wpu[blockIdx.x]);
        }
    };
    template <bool HI> struct OpReduce2q
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return m.template reduce_2q<HI>(a.x[i]);
        }
    };
    template <int B, bool HI> struct OpNormalize
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M& m, const Args<T>& a, unsigned i)
        {
            return normalize<B, HI>(m, a.x[i]);
        }
    };
    struct OpXadNot // 32-bit only
    {
        template <typename M, typename T> static __device__ __forceinline__ T run(const M&, const Args<T>& a, unsigned i)
        {
            return xad_not(a.x[i], a.acc[i]);
        }
    };

    template <typename OP> struct needs_hi : std::false_type
    {
    };
    template <> struct needs_hi<OpReduce2q<true>> : std::true_type
    {
    };
    template <int B> struct needs_hi<OpNormalize<B, true>> : std::true_type
    {
    };

    // one wave per block: the 512-VGPR budget holds the fixed pair v[126:127] of Mod64::mul_acc_raw
    template <typename M, typename T, bool VQ, typename OP> __global__ __launch_bounds__(WAVE) void probe_kernel(Args<T> a, T* out)
    {
        const unsigned i = blockIdx.x * WAVE + threadIdx.x;
        if (i >= a.n)
            return;
        const NormConst nc = VQ ? a.ncl[i] : a.ncb[blockIdx.x];
        // the HI forms (quotient estimate from the high word) are for moduli with nc.hi set: the other words stay 0
        if constexpr (needs_hi<OP>::value)
            if (nc.hi == 0u)
                return;
        M m;
        if constexpr (VQ)
            m.set(a.q[i], nc);
        else
            m.set(a.qb[blockIdx.x], nc);
        out[i] = OP::template run<M, T>(m, a, i);
    }

    template <typename T> struct Run
    {
        Args<T> a{};
        unsigned ncase = 0, nuni = 0;
        T* d_out = nullptr;
        std::vector<T> h_out;
        std::FILE* fo = nullptr;
        uint64_t nrec = 0;

        template <typename M, bool VQ, typename OP> void rec(const char* name, bool uni = false)
        {
            const unsigned n = uni ? nuni : ncase;
            HIP_CHECK(hipMemset(d_out, 0, sizeof(T) * ncase));
            if (n != 0)
            {
                Args<T> b = a;
                b.n = n;
                probe_kernel<M, T, VQ, OP><<<dim3(n / WAVE), dim3(WAVE)>>>(b, d_out);
                HIP_CHECK(hipGetLastError());
            }
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(h_out.data(), d_out, sizeof(T) * ncase, hipMemcpyDeviceToHost));
            char tag[16] = {0};
            std::strncpy(tag, name, sizeof(tag) - 1);
            if (std::fwrite(tag, 1, sizeof(tag), fo) != sizeof(tag) || std::fwrite(h_out.data(), sizeof(T), ncase, fo) != ncase)
            {
                std::fprintf(stderr, "short write\n");
                std::exit(4);
            }
            ++nrec;
        }
    };

    // every member a kernel calls, for one 64-bit family
    template <int LIM, bool VQ> void family64(Run<uint64_t>& r)
    {
        using M = Mod64<LIM, VQ>;
        r.template rec<M, VQ, OpMul<true>>("mul_u", true);
        r.template rec<M, VQ, OpMul<false>>("mul_v");
        r.template rec<M, VQ, OpMulAcc<true, false>>("macc_u", true);
        r.template rec<M, VQ, OpMulAcc<false, false>>("macc_v");
        r.template rec<M, VQ, OpMulAcc<true, true>>("maccz_u", true);
        r.template rec<M, VQ, OpMulAcc<false, true>>("maccz_v");
        if constexpr (LIM == 4) // elsewhere mul_acc IS mul_acc_raw
        {
            r.template rec<M, VQ, OpMulAccRaw<true>>("raw_u", true);
            r.template rec<M, VQ, OpMulAccRaw<false>>("raw_v");
        }
        r.template rec<M, VQ, OpCsub<1>>("csub1");
        r.template rec<M, VQ, OpCsub<2>>("csub2");
        r.template rec<M, VQ, OpCsub<4>>("csub4");
        if constexpr (LIM >= 8)
            r.template rec<M, VQ, OpCsub<8>>("csub8");
        if constexpr (LIM >= 16)
            r.template rec<M, VQ, OpCsub<16>>("csub16");
        r.template rec<M, VQ, OpShl1Add<VQ>>("shl1");
        r.template rec<M, VQ, OpReduce2q<false>>("red2q");
        r.template rec<M, VQ, OpReduce2q<true>>("red2q_hi");
        r.template rec<M, VQ, OpNormalize<2, false>>("norm2");
        r.template rec<M, VQ, OpNormalize<4, false>>("norm4");
        if constexpr (LIM >= 8)
        {
            r.template rec<M, VQ, OpNormalize<8, false>>("norm8");
            r.template rec<M, VQ, OpNormalize<8, true>>("norm8_hi");
        }
        if constexpr (LIM >= 16)
        {
            r.template rec<M, VQ, OpNormalize<16, false>>("norm16");
            r.template rec<M, VQ, OpNormalize<16, true>>("norm16_hi");
        }
        if constexpr (LIM >= 31)
        {
            r.template rec<M, VQ, OpNormalize<31, false>>("norm31");
            r.template rec<M, VQ, OpNormalize<31, true>>("norm31_hi");
            // one past the family's range: the stated domain of reduce_2q itself (x < 32 q)
            r.template rec<M, VQ, OpNormalize<32, false>>("norm32");
            r.template rec<M, VQ, OpNormalize<32, true>>("norm32_hi");
        }
    }

    template <int LIM, bool VQ> void family32(Run<uint32_t>& r)
    {
        using M = Mod32<LIM, VQ>;
        r.template rec<M, VQ, OpMul<true>>("mul_u", true);
        r.template rec<M, VQ, OpMul<false>>("mul_v");
        r.template rec<M, VQ, OpMulAcc<true, false>>("macc_u", true);
        r.template rec<M, VQ, OpMulAcc<false, false>>("macc_v");
        r.template rec<M, VQ, OpMulAcc<true, true>>("maccz_u", true);
        r.template rec<M, VQ, OpMulAcc<false, true>>("maccz_v");
        r.template rec<M, VQ, OpMulc<true>>("mulc_u", true);
        r.template rec<M, VQ, OpMulc<false>>("mulc_v");
        r.template rec<M, VQ, OpCsub<1>>("csub1");
        r.template rec<M, VQ, OpCsub<2>>("csub2");
        r.template rec<M, VQ, OpCsub<4>>("csub4");
        r.template rec<M, VQ, OpCsubC<1>>("csubc1");
        r.template rec<M, VQ, OpCsubC<2>>("csubc2");
        r.template rec<M, VQ, OpCsubC<4>>("csubc4");
        if constexpr (LIM >= 8)
        {
            r.template rec<M, VQ, OpCsub<8>>("csub8");
            r.template rec<M, VQ, OpCsubC<8>>("csubc8");
        }
        r.template rec<M, VQ, OpShl1Add<VQ>>("shl1");
        r.template rec<M, VQ, OpReduce2q<false>>("red2q");
        r.template rec<M, VQ, OpNormalize<2, false>>("norm2");
        r.template rec<M, VQ, OpNormalize<4, false>>("norm4");
        if constexpr (LIM >= 8)
            r.template rec<M, VQ, OpNormalize<8, false>>("norm8");
        r.template rec<M, VQ, OpXadNot>("xad_not");
    }

    // family ids of the case file: the Mod<...> specialisations of lazy.hpp
    enum Family : uint64_t
    {
        M64_16 = 0,
        M64_31 = 1,
        M64_8 = 2,
        M64_4 = 3,
        M64_4V = 4,
        M64_16V = 5,
        M64_8V = 6,
        M32_4 = 7,
        M32_4V = 8,
        M32_8 = 9,
        FAMILIES = 10
    };

    std::vector<void*> g_allocs;
    template <typename T> T* upload(const std::vector<T>& h)
    {
        T* d = nullptr;
        HIP_CHECK(hipMalloc(&d, sizeof(T) * (h.empty() ? 1 : h.size())));
        g_allocs.push_back(d);
        if (!h.empty())
            HIP_CHECK(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
        return d;
    }

    template <typename T> int run_family(uint64_t family, unsigned ncase, unsigned nuni, std::FILE* fi, const char* out_path)
    {
        const unsigned nblk = ncase / WAVE;
        std::vector<T> lane[6], blk[4];
        for (auto& v : lane)
        {
            v.resize(ncase);
            if (std::fread(v.data(), sizeof(T), ncase, fi) != ncase)
            {
                std::fprintf(stderr, "case file too short\n");
                return 2;
            }
        }
        for (auto& v : blk)
        {
            v.resize(nblk);
            if (std::fread(v.data(), sizeof(T), nblk, fi) != nblk)
            {
                std::fprintf(stderr, "case file too short\n");
                return 2;
            }
        }
        if (std::fgetc(fi) != EOF)
        {
            std::fprintf(stderr, "case file too long\n");
            return 2;
        }
        // the constants of the final normalisation: the header's own host function on the `bit` the file carries
        std::vector<NormConst> ncl(ncase), ncb(nblk);
        for (unsigned i = 0; i < ncase; i++)
            ncl[i] = norm_const_of<T>(lane[2][i], lane[3][i]);
        for (unsigned b = 0; b < nblk; b++)
            ncb[b] = norm_const_of<T>(blk[0][b], blk[1][b]);

        Run<T> r;
        r.ncase = ncase;
        r.nuni = nuni;
        r.h_out.resize(ncase);
        r.a.x = upload(lane[0]);
        r.a.acc = upload(lane[1]);
        r.a.q = upload(lane[2]);
        r.a.bit = upload(lane[3]);
        r.a.w = upload(lane[4]);
        r.a.wp = upload(lane[5]);
        r.a.qb = upload(blk[0]);
        r.a.bitb = upload(blk[1]);
        r.a.wu = upload(blk[2]);
        r.a.wpu = upload(blk[3]);
        r.a.ncl = upload(ncl);
        r.a.ncb = upload(ncb);
        HIP_CHECK(hipMalloc(&r.d_out, sizeof(T) * ncase));
        r.fo = std::fopen(out_path, "wb");
        if (r.fo == nullptr)
        {
            std::perror(out_path);
            return 2;
        }
        const uint64_t head[4] = {MAGIC, family, ncase, 0};
        if (std::fwrite(head, sizeof(head), 1, r.fo) != 1)
            return 4;
        if constexpr (sizeof(T) == 8)
        {
            switch (family)
            {
            case M64_16: family64<16, false>(r); break;
            case M64_31: family64<31, false>(r); break;
            case M64_8: family64<8, false>(r); break;
            case M64_4: family64<4, false>(r); break;
            case M64_4V: family64<4, true>(r); break;
            case M64_16V: family64<16, true>(r); break;
            case M64_8V: family64<8, true>(r); break;
            default: return 2;
            }
        }
        else
        {
            switch (family)
            {
            case M32_4: family32<4, false>(r); break;
            case M32_4V: family32<4, true>(r); break;
            case M32_8: family32<8, false>(r); break;
            default: return 2;
            }
        }
        const uint64_t full[4] = {MAGIC, family, ncase, r.nrec};
        if (std::fseek(r.fo, 0, SEEK_SET) != 0 || std::fwrite(full, sizeof(full), 1, r.fo) != 1 || std::fclose(r.fo) != 0)
        {
            std::fprintf(stderr, "cannot finish %s\n", out_path);
            return 4;
        }
        HIP_CHECK(hipFree(r.d_out));
        for (void* p : g_allocs)
            HIP_CHECK(hipFree(p));
        g_allocs.clear();
        std::printf("family %" PRIu64 ": %u cases (%u with a wave-uniform twiddle), %" PRIu64 " records\n", family, ncase, nuni,
                    r.nrec);
        return 0;
    }

    int run_mode(const char* in_path, const char* out_path)
    {
        std::FILE* fi = std::fopen(in_path, "rb");
        if (fi == nullptr)
        {
            std::perror(in_path);
            return 2;
        }
        uint64_t head[8];
        if (std::fread(head, sizeof(head), 1, fi) != 1 || head[0] != MAGIC || head[1] >= FAMILIES || head[2] == 0 ||
            head[2] > MAX_CASES || head[2] % WAVE != 0 || head[3] > head[2] || head[3] % WAVE != 0)
        {
            std::fprintf(stderr, "%s: bad header\n", in_path);
            return 2;
        }
        const unsigned ncase = static_cast<unsigned>(head[2]), nuni = static_cast<unsigned>(head[3]);
        const int rc = head[1] >= M32_4 ? run_family<uint32_t>(head[1], ncase, nuni, fi, out_path)
                                        : run_family<uint64_t>(head[1], ncase, nuni, fi, out_path);
        std::fclose(fi);
        return rc;
    }

    // ---- host-only modes: the header's constexpr / __host__ functions, no HIP call ------------------------------
    int norm_mode(const char* path)
    {
        std::FILE* fi = std::fopen(path, "r");
        if (fi == nullptr)
        {
            std::perror(path);
            return 2;
        }
        unsigned w;
        uint64_t q, bit;
        while (std::fscanf(fi, "%u %" SCNu64 " %" SCNu64, &w, &q, &bit) == 3)
        {
            const NormConst n = (w == 32) ? norm_const_of<uint32_t>(static_cast<uint32_t>(q), static_cast<uint32_t>(bit))
                                          : norm_const_of<uint64_t>(q, bit);
            std::printf("%u %" PRIu64 " %" PRIu64 " %u %u %u %u\n", w, q, bit, n.sh, n.c, n.M, n.hi);
        }
        std::fclose(fi);
        return 0;
    }

    int plan_mode(const char* path)
    {
        std::FILE* fi = std::fopen(path, "r");
        if (fi == nullptr)
        {
            std::perror(path);
            return 2;
        }
        int bu, bv, limit, tb;
        while (std::fscanf(fi, "%d %d %d %d", &bu, &bv, &limit, &tb) == 4)
        {
            const CtPlan c = ct_plan(bu, limit, tb);
            const GsPlan g = gs_plan(bu, bv, limit);
            std::printf("%d %d %d %d ct %d %d gs %d %d %d %d %d\n", bu, bv, limit, tb, c.ku, c.out, g.ku, g.kv, g.c, g.ko, g.out_u);
        }
        std::fclose(fi);
        return 0;
    }
} // namespace

int main(int argc, char** argv)
{
    if (argc == 4 && std::strcmp(argv[1], "run") == 0)
        return run_mode(argv[2], argv[3]);
    if (argc == 3 && std::strcmp(argv[1], "norm") == 0)
        return norm_mode(argv[2]);
    if (argc == 3 && std::strcmp(argv[1], "plan") == 0)
        return plan_mode(argv[2]);
    std::fprintf(stderr, "usage: %s run CASES OUT | norm LIST | plan LIST\n", argv[0]);
    return 2;
}
