/* test_hooks.h -- C entry points for the TESTS of this repository (tests/, tools/).  NOT part of the drop-in boundary: the
 * public headers (include/gpuntt_c.h, include/gpuntt/...) do not declare them and a GPU-NTT user has no use for them.
 *
 *   gpuntt_test_set_hook(name, value)   everything gpuntt_set_option takes, plus the hooks
 *       path = fast-strict       a call the fast kernels cannot take throws; no generic launch behind any call
 *       path = generic-capped    the generic kernels of an RNS call on the capped grid they use behind a go-flag
 *       no_scratch = 0 | 1       the drop-in calls behave as if their twiddle scratch could not be allocated
 *       rns_force_fallback = 0|1 the preparation kernel's own fall-back serves every drop-in RNS Merge call
 *       u32_e32 = mask           32-bit Merge rings 2^12 .. 2^15 on the 32-coefficients-per-lane kernels (bit n = ring 2^n;
 *                                bit 16: the full-tile contiguous pass of larger rings)
 *       contig_p4 = 0 | 1        forward 64-bit Merge transforms of the ring 2^16: the 10-stage last pass on tiles of four
 *                                polynomials x one 1024-coefficient segment (1), or on the one-polynomial tile (0)
 *       premul = 0 | 1           the same calls, 16 q / 31 q ranges, when they take the four-polynomial tile: the strided pass
 *                                multiplies the bit-9 half of the ring by the last pass's first-stage twiddles and the last pass
 *                                starts from the products (1), or both passes as before (0)
 *       two_sweep_big = 0 | 1    experiment: 64-bit rings 2^23 / 2^24 forward in two sweeps on 16384-coefficient tiles
 *       baseconv_ksplit = 0..16  base conversion: workgroups per column tile that share its outputs (0: the library's choice)
 *       keyswitch_split = 0..64  key switching: workgroups per column tile that share the (digit, block) pairs of the ModUp
 *       keyswitch_hoist_chunk = 0 | 6..13  rotate_hoisted / rotate_hoisted_sum: log2 of the slots of a chunk of the two kernels
 *                                of hoisted_rotation.hip (0: the LDS budget rule; a forced chunk is still capped at N, at what
 *                                LDS can hold and, for inner_product_galois_sum, at 256 slots)
 *       reset_predictions = 1    the family prediction of the RNS overloads forgets every stack it has seen
 *   gpuntt_test_launch_log_start()      start recording the kernel of every launch the library enqueues (all threads)
 *   gpuntt_test_launch_log_take(buf, n) stop; the kernels since start, space-separated ("prep_twiddles merge_pass_lazy:31 ..."),
 *                                       fast kernels with their lazy range behind a colon; returns the capacity needed
 *                                       (terminator included).  Never a cut list: when n is smaller than that, buf gets an
 *                                       empty string and the log is KEPT -- take again with the returned capacity
 *   gpuntt_test_alloc_count()           hipMalloc / hipHostMalloc / hipFree / hipHostFree calls the scratch chains and the
 *                                       family prediction's pool of host-mapped words (prep.hip) have made since the
 *                                       library was loaded: a steady-state call makes none
 *   gpuntt_test_scratch_stats(out[6])   the twiddle scratch of captured calls, which their graph owns (prep.hip): buffers handed to
 *                                       a graph, of those reported dead by their graph, buffers pooled now, buffers re-used from
 *                                       the pool, chains erased, chains alive
 *   gpuntt_test_contig_p4_launches()    launches of the four-polynomial tile of the forward 64-bit contiguous pass since the
 *                                       library was loaded (hook contig_p4): the launch log shows them under the name of the
 *                                       one-polynomial tile
 *   gpuntt_test_premul_launches()       calls since the library was loaded whose strided pass did the last pass's first twiddle
 *                                       product (hook premul); the launch log shows both kernels under their usual names
 *   gpuntt_test_keyswitch_hoist_chunk(word_bytes, digits, n_power)  host only: log2 of the chunk inner_product_galois takes
 *                                       for this word size, D and ring under the hook's current value; -1: bad argument
 *   gpuntt_test_keyswitch_hoist_sum_chunk(word_bytes, digits, n_power)  the same for the destination chunk of
 *                                       inner_product_galois_sum (rotate_hoisted_sum): the same rule capped at one slot per
 *                                       lane, 256 slots, which the hook keyswitch_hoist_chunk forces as well, inside that cap
 *   gpuntt_test_bsgs_sum_shape(word_bytes, n1, n_power, aligned, V, nt)  host only: the launch shape bsgs_weighted_sum
 *                                       (linear_transform_bsgs) takes for this word size, n1 baby steps and ring -- V words
 *                                       per lane (a 16-byte group, or 1) and nt lanes per workgroup; aligned: every base
 *                                       pointer of the launch is 16-byte aligned; -1: bad argument
 * Options are snapshot once per API call (prep.hip), so a hook set while another thread's call is in flight does not change
 * that call. */
#ifndef GPUNTT_TEST_HOOKS_H
#define GPUNTT_TEST_HOOKS_H
#ifdef __cplusplus
extern "C"
{
#endif
    int gpuntt_test_set_hook(const char* name, const char* value);
    int gpuntt_test_launch_log_start(void);
    int gpuntt_test_launch_log_take(char* buf, int capacity);
    int gpuntt_test_scratch_stats(unsigned long long out[6]);
    unsigned long long gpuntt_test_contig_p4_launches(void);
    unsigned long long gpuntt_test_premul_launches(void);
    unsigned long long gpuntt_test_alloc_count(void);
    int gpuntt_test_keyswitch_hoist_chunk(int word_bytes, int digits, int n_power);
    int gpuntt_test_keyswitch_hoist_sum_chunk(int word_bytes, int digits, int n_power);
    int gpuntt_test_bsgs_sum_shape(int word_bytes, int n1, int n_power, int aligned, int* V, unsigned* nt);
#ifdef __cplusplus
}
#endif
#endif
