// rescale_internal.hpp -- what key_switch.hip needs of rescale.hip: where the constants of rescale_sub_scale lie and the
// launchers of the two kernels behind KeySwitchPlan<T>::rescale(ntt_form = true).  The grid and the choice of the loader
// are relin_grid and relin_wide of relinearize_internal.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "relinearize_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // Four arrays of the constants image of the conversion {dropped q} -> {kept q} (bc_image), in words behind its
        // start, each indexed by the kept limb j: BcOffsets' p, onep, qinv and qinvp
        struct RsOffsets
        {
            unsigned q;     // [L'] q_j
            unsigned onep;  // [L'] floor(2^W / q_j): the Shoup companion of 1
            unsigned qinv;  // [L'] (q_{L-R} ... q_{L-1})^-1 mod q_j
            unsigned qinvp; // [L'] its Shoup companion
        };

        // The dropped moduli travel as ONE kernel argument (as RelinArgs does): read at blockIdx.y, a scalar load.  1 KiB
        // for u64, inside the 4 KiB argument segment
        template <typename T> struct RsDropped
        {
            T q[INNERPROD_MAX_MODULI];    // q_{L-R+i}, i < R ...
            T onep[INNERPROD_MAX_MODULI]; // ... and floor(2^W / q_{L-R+i}): the Shoup companion of 1
        };
        static_assert(sizeof(RsDropped<Data64>) == 1024 && sizeof(RsDropped<Data32>) == 512,
                      "RsDropped has to stay inside the 4 KiB argument segment");
    } // namespace kern

    namespace host
    {
        // x: T[stacks][L][N] (any words); dropped: T[stacks][R][N] = limbs L - R .. L - 1 of every stack, each word
        // reduced modulo its q (the transform that follows is defined on residues).  One launch.  enqueue false: only the
        // checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void rescale_gather_launch(const T* x, T* dropped, const kern::RsDropped<T>& mods, int stacks, int L, int R,
                                   int n_power, bool enqueue, hipStream_t stream);

        // x: T[stacks][L][N] (any words), out: T[stacks][keep][N] holding canonical residues, rewritten in place:
        // out[s][j] = ((x[s][j] mod q_j) - out[s][j]) * qinv_j mod q_j.  consts: the image `off` points into.  One
        // launch.  enqueue false: only the checks.  Throws std::invalid_argument beyond the grid limits
        template <typename T>
        void rescale_sub_scale_launch(const T* x, T* out, const T* consts, const kern::RsOffsets& off, int stacks, int L,
                                      int keep, int n_power, bool enqueue, hipStream_t stream);
    } // namespace host
} // namespace gpuntt
