// bfv_multiply_internal.hpp -- what bfv_multiply.hip's kernels and its host side share, and what the host emulator
// (tests/cpp/emulate_bfv.cpp) needs to call the kernels: where the plan's own constants lie beside the two base
// conversion images.  Not a public header.
#pragma once

#include <hip/hip_runtime.h>

#include "base_conversion_internal.hpp"
#include "inner_product_internal.hpp"

namespace gpuntt
{
    namespace kern
    {
        // The constants of a BfvMultiplyPlan are ONE run of words: the image of {q} -> {b} (bc_image), the image of
        // {b} -> {q}, the arrays below and the fold image of bfv_tensor (InnerProductPlan's six arrays of M words).  Every
        // offset -- those of the two BcOffsets included -- counts words from the start of that run, so the kernels take
        // one pointer.  KP = K rounded up to BC_KB
        struct BfvOffsets
        {
            unsigned wt;    // [L]  (t * qhat_i^-1) mod q_i
            unsigned wtp;   // [L]  its Shoup companion
            unsigned onepq; // [L]  floor(2^W / q_i): the Shoup companion of 1
            unsigned tb;    // [KP] t mod b_j
            unsigned tbp;   // [KP] its Shoup companion
        };
    } // namespace kern
} // namespace gpuntt
