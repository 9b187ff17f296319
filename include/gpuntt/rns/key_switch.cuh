// gpuntt/rns/key_switch.cuh -- hybrid (RNS-digit) key switching (extension: no counterpart in the reference).
//
// The operation the three pieces before it were built for -- Galois automorphisms (ntt_merge/galois.cuh), fast base
// conversion (rns/base_conversion.cuh) and the RNS inner product (rns/inner_product.cuh) -- as ONE plan that owns the
// constants, the digit partition and the sequence.  All integers, W = 8 * sizeof(T).
//
// Bases.  q-primes q_0 .. q_{L-1}, special primes p_0 .. p_{K-1}; the FULL base is {q_0 .. q_{L-1}, p_0 .. p_{K-1}} in
// that order, M = L + K limbs, modulus m of the full base is q_m for m < L and p_{m-L} otherwise.  A digit size
// alpha >= 1 cuts the q-base into D = ceil(L / alpha) digits: digit d owns the limbs S_d = [d alpha, min((d+1) alpha, L))
// (the last digit may be shorter), Q_d = prod_{i in S_d} q_i, P = prod_k p_k.
//
//   mod_up(in, a, count, mode):  in = T[count][L][N] (coefficient form), a = T[D][count][M][N] -- the digit-major
//     layout InnerProductPlan reads.  For every d < D, r < count, m < M:
//       m in S_d:   a[d][r][m] = in[r][m] mod q_m                 canonical; ANY input word is accepted
//       otherwise:  a[d][r][m] = WORD FOR WORD what BaseConvPlan gives for the input base {q_i : i in S_d} (in that
//                   order), an output base that contains modulus m and the same BaseConvMode, on the limbs in[r][i],
//                   i in S_d.  The formulas of base_conversion.cuh ARE the definition (y_i, approximate / centred, R_i,
//                   b_i, v); nothing is restated here
//     ONE kernel launch for all digits: every input word is read from memory once, every word of a is written once --
//     unless count * N is too small to fill the part: then the (digit, output block) pairs of a column tile are split
//     over up to 8 workgroups, each of which re-reads the tile's input (the threshold is an estimate).
//     `in` must not overlap `a`
//   mod_down(x, out, stacks):  x = T[stacks][M][N] (coefficient form, full base), out = T[stacks][L][N]:
//       out[s][j] = what BaseConvPlan({p_k} -> {q_j})::convert_and_divide gives in centred mode with in = limbs
//                   L .. M-1 of stack s and c = limbs 0 .. L-1 of stack s: round(x / P) in the base q outside that
//                   header's rounding band
//     ONE kernel launch for all stacks, the special limbs read in place.  out must NOT overlap x: stacks of x are M N
//     words apart and those of out L N, so out[s] lies over limbs of earlier stacks that other workgroups may not have
//     read yet -- in-place operation cannot be made safe without a second pass and is refused
//   mod_down_add(x, addend, out, stacks):  mod_down with an addend.  x as for mod_down; addend = T[stacks][L][N], ANY word
//     (read modulo q_j); out = T[stacks][L][N].  DEFINITION, word for word:
//       out[s][j] = (mod_down(x)[s][j] + (addend[s][j] mod q_j)) mod q_j, canonical
//     ONE launch (mod_down_add: mod_down's kernel with an addend epilogue behind a compile-time switch, the same output
//     split); allocates nothing, never synchronises; stacks = 0 launches nothing.  addend may be exactly out: each word is
//     read and then written by the same lane.  out must not overlap x (mod_down's rule); any other overlap of addend with
//     out or x is refused.  Refusals: mod_down's, plus a null addend
//   decompose(c_in, a, count, input_ntt, scratch):
//       [input_ntt: INTT over the count * L polynomials of c_in (q-base) into scratch]  mod_up (centred)  forward NTT in
//       place over the D * count * M polynomials of a
//   switch_digits(a, key, out, count, components, output_ntt, scratch):
//       InnerProductPlan::multiply_accumulate(a, key) with D digits, C = components, accumulate = false and the plan's
//       key_mod_count / key_limbs into scratch T[C][count][M][N]; INTT over C * count * M; mod_down into
//       out = T[C][count][L][N]; [output_ntt: forward NTT over C * count * L in place]
//   apply(c_in, key, out, count, components, input_ntt, output_ntt, scratch) = decompose, then switch_digits, a in scratch
//     The split is there to hoist: decompose once, then rotate_hoisted -- many rotation keys applied to one decomposition.
//     key = T[D_key][C][key_mod_count][N] in NTT form, exactly InnerProductPlan's.
//   rotate_hoisted(a, c0, keys, galois_elements, G, out, count, output_ntt, scratch):  G rotations (or any Galois
//     automorphisms) of the count ciphertexts whose second components were decomposed into a = T[D][count][M][N] (what
//     decompose writes), each with its own switching key; c0 = T[count][L][N] in NTT form, the first components, or
//     nullptr; keys = a HOST array of G device pointers, each T[D_key][2][key_mod_count][N], read through the plan's
//     key_mod_count / key_limbs; galois_elements = a HOST array of G odd elements k_g, reduced mod 2N (X_N_plus) or mod N
//     (X_N_minus) as GPU_Automorphism_NTT reduces them, 1 <= G <= 64, duplicates and the identity allowed;
//     out = T[G][2][count][L][N].  DEFINITION, word for word: out[g] is what the existing public calls give --
//       1. GPU_Automorphism_NTT(a, k_g) over the D * count * M polynomials of a,
//       2. switch_digits(that, keys[g], components = 2, output_ntt),
//       3. c0 != nullptr: component 0 plus GPU_Automorphism_NTT(c0, k_g), added mod q_m; with output_ntt false the
//          NTT-form operand is inverse-transformed before the addition.
//     What runs instead, each step ONE launch over the whole batch (plus the transforms' own):
//       inner_product_galois: acc[g][c][r][m][j] = (sum_d a[d][r][m][pi_g(j)] * keys[g][d][c][limb(m)][j]
//                             + [c = 0, m < L, c0 != nullptr] (P mod q_m) * c0[r][m][pi_g(j)]) mod q_m into the scratch,
//                             pi_g = galois_ntt_source(., k_g), the permutation of GPU_Automorphism_NTT -- the permuted
//                             digits are never written to memory, every word of a and c0 is read once per call;
//       the full-base INTT over G * 2 * count * M polynomials; mod_down with stacks = G * 2 * count into out;
//       [output_ntt: the q-base forward NTT over G * 2 * count * L polynomials].
//     Folding c0 in as P * c0 BEFORE the ModDown is exact, not approximate.  sigma_k and the transforms are linear, so the
//     q-limbs of the stack that reaches mod_down hold c_j + P y (mod q_j), with c the accumulators of step 2 and
//     y = sigma_k(c0) in coefficient form, while the special limbs are untouched (P = 0 mod p_k): the conversion term
//     conv_j of mod_down is computed from the special limbs only and is identical.  Then
//       (c_j + P y - conv_j) P^-1 = y + (c_j - conv_j) P^-1  (mod q_j),
//     the right side is step 3's sum, and both sides are canonical residues, so they are the same word.  With output_ntt
//     the forward NTT is linear and its outputs canonical, so the words agree there too.
//     Every input word of a and c0 may hold any value (it is read modulo q_m); the keys are read the same way.
//     Allocates nothing, never synchronises: one stream, capturable into a hipGraph as it is.  count = 0: nothing is
//     launched.  The scratch is hoisted_scratch_bytes(count, G) bytes (the accumulators T[G][2][count][M][N]), 256-byte
//     aligned; out and the scratch must not overlap a, c0, any key or each other.  std::invalid_argument, before anything
//     is launched: G outside [1, 64], count < 0, an even element, a null a / out / key pointer / scratch, a scratch that
//     is not 256-byte aligned, an overlap, a plan built without transforms
//   rotate_hoisted_sum(a, c0, keys, galois_elements, weights, G, out, count, output_ntt, scratch):  the weighted sum of
//     those G rotations, sum_g pt_g (.) sigma_{k_g}(ct) -- a linear transform (a matrix diagonal per rotation, a
//     baby-step/giant-step product, CoeffToSlot) -- taken in the extended base P Q BEFORE the ModDown ("double hoisting").
//     a, c0, keys, galois_elements and G are exactly rotate_hoisted's (1 <= G <= 64, duplicates and the identity allowed,
//     elements reduced as GPU_Automorphism_NTT reduces them, key_mod_count / key_limbs from the plan).
//     weights = a HOST array of G device pointers, or nullptr (every weight is 1: the plain sum of the rotations);
//     weights[g] = T[M][N], the plaintext diagonal pt_g in NTT form over the FULL base, limb m under modulus m of the
//     plan's full base -- any word is accepted, it is read modulo q_m -- or nullptr (weight 1).
//     out = T[2][count][L][N].  DEFINITION, with pi_g = galois_ntt_source(., k_g) and w_g[m][j] = weights[g][m][j] mod q_m
//     (1 where the pointer is null):
//       u_g[c][r][m][j] = (sum_d a[d][r][m][pi_g(j)] * keys[g][d][c][limb(m)][j]
//                          + [c = 0, m < L, c0 != nullptr] (P mod q_m) * c0[r][m][pi_g(j)]) mod q_m  -- rotate_hoisted's acc
//       acc[c][r][m][j] = (sum_g w_g[m][j] * u_g[c][r][m][j]) mod q_m                               -- canonical
//     into the scratch (inner_product_galois_sum, ONE launch), then the plan's own steps, each ONE launch over the whole
//     batch plus the transforms' own: the full-base INTT over 2 * count * M polynomials; mod_down with stacks = 2 * count
//     into out; [output_ntt: the q-base forward NTT over 2 * count * L polynomials].  One INTT, one mod_down and one NTT
//     over 2 * count stacks whatever G is, where rotate_hoisted runs them over G * 2 * count.
//     NOT word for word sum_g pt_g (.) rotate_hoisted(...)[g]: that expression rounds G times, this one once.  With U_g
//     the coefficient-form stack of u_g (full base, the value X_g = CRT(U_g) taken mod P Q) and pt_g the weight as a
//     polynomial, rotate_hoisted returns r_g = (X_g - [X_g]_P) / P (mod Q), [.]_P the centred residue mod P that
//     mod_down converts -- round(X_g / P) outside base_conversion.cuh's rounding band -- while this call returns
//     (S - [S]_P) / P (mod Q) for S = sum_g pt_g X_g mod P Q.  Both sides are exact in the q-limbs, so
//       out - sum_g pt_g r_g = (sum_g pt_g [X_g]_P - [S]_P) / P  (mod Q),
//     a multiple of P divided by P: an integer polynomial of infinity norm at most (1 + sum_g |pt_g|_1) / 2 (plus the
//     rounding band of each conversion).  That difference is the rounding noise the G-fold expression carries and this
//     one does not: here the error against the exact sum_g pt_g X_g / P is that of ONE mod_down, whatever G and pt_g are.
//     The c0 term is exact as above (P c0 is 0 mod P and leaves [.]_P alone); the weight applies to it too.
//     Contract as for rotate_hoisted: allocates nothing, never synchronises, one stream, capturable as it is; count = 0
//     launches nothing.  The scratch is hoisted_sum_scratch_bytes(count) bytes (the accumulators T[2][count][M][N] --
//     it does not grow with G), 256-byte aligned; out and the scratch must not overlap a, c0, any key, any non-null weight
//     or each other.  std::invalid_argument, before anything is launched: G outside [1, 64], count < 0, an even element
//     (also one that is even once reduced), a null a / out / key pointer / scratch, a scratch that is not 256-byte aligned,
//     an overlap, a count beyond the grid and batch limits rotate_hoisted checks, a plan built without transforms
//   multiply_relinearize(x, y, key, out, count, output_ntt, scratch):  the product of `count` pairs of two-component
//     ciphertexts, relinearized: ct x ct in ONE key switch.  x, y = T[2][count][L][N], the component-major layout every
//     plan call writes (so results chain), in NTT form over the q-base; every word may hold any value and is read modulo
//     q_m.  y may equal x (a squaring).  key = T[D_key][2][key_mod_count][N], the relinearization key (s^2 -> s), read
//     through the plan's key_mod_count / key_limbs exactly as apply reads it.  out = T[2][count][L][N].
//     DEFINITION, word for word, through the calls that exist beside it:
//       1. for every r, m < L and column j the canonical residues
//            d0 = x0 y0 mod q_m,   d1 = (x0 y1 + x1 y0) mod q_m,   d2 = x1 y1 mod q_m
//          -- each what a q-base InnerProductPlan::multiply_accumulate gives for that one input (D = 1 for d0 and d2,
//          D = 2 for d1, C = 1, the polynomials of y in the key's place),
//       2. k = apply(d2, key, count, components = 2, input_ntt = true, output_ntt),
//       3. out[c] = (k[c] + d_c) mod q_m; with output_ntt false d_c is inverse-transformed over the q-base before the
//          addition.
//     What runs instead, each step ONE launch over the whole batch (plus the transforms' own):
//       tensor_top: d2[r][m][j] = x1 y1 mod q_m into the scratch's c_coeff region (one exact mac, the fold);
//       the plan's own decompose steps on that region: the q-base INTT in place, mod_up (centred) into the `a` region,
//       the full-base NTT over D * count * M polynomials;
//       inner_product_tensor: acc[c][r][m][j] = (sum_d a[d][r][m][j] * key[d][c][limb(m)][j]
//                             + [m < L] (P mod q_m) * d_c[r][m][j]) mod q_m into the inner_out region -- d0 and d1 are
//                             formed on the fly from the four input words and never written to memory; the K special
//                             limbs load nothing of x or y;
//       finish over 2 * count stacks: the full-base INTT, mod_down, [output_ntt: the q-base NTT].
//     Folding d_c in as P * d_c BEFORE the ModDown is exact: it is rotate_hoisted's c0 argument applied to both
//     components.  The transforms are linear, so the q-limbs of the stack that reaches mod_down hold c_j + P d (mod q_j),
//     c the accumulators of step 2 and d = d_c in coefficient form, while the special limbs are untouched (P d vanishes
//     mod p_k): conv_j is computed from the special limbs only and is unchanged.  Then
//       (c_j + P d - conv_j) P^-1 = d + (c_j - conv_j) P^-1  (mod q_j),
//     the right side is step 3's sum and both sides are canonical residues, so they are the same word; with output_ntt
//     the forward NTT is linear and its outputs canonical, so the words agree there too.
//     Allocates nothing, never synchronises: one stream, capturable as it is.  count = 0: nothing is launched.  The
//     scratch is the existing scratch_bytes(count, 2) bytes, 256-byte aligned.  out may be exactly x or exactly y: on the
//     stream the last read of both (inner_product_tensor) precedes mod_down's first write.  std::invalid_argument, before
//     anything is launched: any other overlap of out or the scratch with an operand or with each other, a null pointer, a
//     scratch that is not 256-byte aligned, count < 0, a count beyond the grid and batch limits rotate_hoisted checks, a
//     plan built without transforms
//   relinearize(c01, c2, key, out, count, input_ntt, output_ntt, scratch):  the key switch of `count` THREE-component
//     ciphertexts, whatever formed them -- a BFV product (rns/bfv_multiply.cuh), a hand-accumulated sum of tensors, a
//     scheme with a step between the tensor and the key switch.  c01 = T[2][count][L][N], the two low components, any
//     word, read modulo q_m; c2 = T[count][L][N], the top component: any word in coefficient form, residues in NTT form,
//     as apply takes them.  A contiguous T[3][count][L][N] is c2 = c01 + 2 * count * L * N.  key, out = T[2][count][L][N]
//     and the scratch (the existing scratch_bytes(count, 2), 256-byte aligned) are multiply_relinearize's.
//     DEFINITION, word for word, through the calls that exist beside it:
//       1. k = apply(c2, key, count, components = 2, input_ntt, output_ntt),
//       2. out[c] = (k[c] + c01[c]) mod q_m, c01 reduced and -- when input_ntt != output_ntt -- brought to the output's
//          form by the q-base transform first.
//     What runs, no step's launch count growing with count, and c01 never transformed on its own:
//       input_ntt true:   the plan's decompose steps on c2 (the q-base INTT into the scratch, mod_up, the full-base NTT);
//                         inner_product_seeded: acc[c][r][m][j] = (sum_d a[d][r][m][j] * key[d][c][limb(m)][j]
//                         + [m < L] (P mod q_m) * c01[c][r][m][j]) mod q_m, one exact mac per seed word, the K special
//                         limbs load nothing of c01; finish over 2 * count stacks.
//       input_ntt false:  mod_up (centred) straight from c2; the full-base NTT; the plan's inner_product; the full-base
//                         INTT; mod_down_add with c01 as the addend; [output_ntt: the q-base NTT over 2 * count * L].
//     Both equal the definition.  input_ntt true: folding c01 in as P * c01 before the ModDown is multiply_relinearize's
//     argument above with d_c = c01[c] -- (c_j + P d - conv_j) P^-1 = d + (c_j - conv_j) P^-1 (mod q_j), canonical on both
//     sides, and the same after the linear, canonical forward NTT; with output_ntt false the fold goes through the
//     full-base INTT, which on the q-limbs is the q-base INTT of c01.  input_ntt false: mod_down_add adds the reduced
//     coefficient-form c01 to the coefficient-form k, which is the definition for output_ntt false; for output_ntt true
//     NTT(k + c) = NTT(k) + NTT(c) (mod q_m), and both sides are canonical, so they are the same word.
//     With input_ntt and a c01 that holds the d_0, d_1 of multiply_relinearize's step 1, the call returns that call's
//     words.  Allocates nothing, never synchronises: one stream, capturable as it is.  count = 0: nothing is launched.
//     out may be exactly c01.  std::invalid_argument, before anything is launched: every other overlap among out, the
//     scratch, c01, c2 and key; a null pointer; a scratch that is not 256-byte aligned; count < 0 or beyond the grid and
//     int limits multiply_relinearize checks; a plan built without transforms.
//     There is no relinearize_rescale: on the coefficient path P * c01 would have to be added to the DROPPED q-limbs
//     before the conversion reads them (they are part of X, see "Rescaling"), which the epilogue of mod_down_add, after
//     the division, cannot do -- a different change to the kernel
//   multiply_relinearize_sum(x, y, terms, key, out, count, output_ntt, scratch):  sum_t x_t * y_t over `terms` pairs of
//     two-component ciphertexts with ONE key switch and ONE ModDown ("lazy relinearization"): an encrypted dot product, a
//     matrix-vector product, a convolution, the power-basis terms of a polynomial evaluation.  x, y = HOST arrays of
//     `terms` device pointers (as rotate_hoisted takes its keys), 1 <= terms <= KEYSWITCH_MAX_TERMS = 32; each pointer a
//     batch T[2][count][L][N] in NTT form over the q-base, every word any value, read modulo q_m.  y[t] may be x[t] (a
//     square) and the same pointer may appear in several terms.  key, out, count, output_ntt and the scratch are exactly
//     multiply_relinearize's; the scratch is the existing scratch_bytes(count, 2).
//     DEFINITION, word for word, through the calls that exist beside it:
//       1. for every r, m < L and column j the canonical residues
//            d0 = (sum_t x0_t y0_t) mod q_m,   d1 = (sum_t x0_t y1_t + x1_t y0_t) mod q_m,   d2 = (sum_t x1_t y1_t) mod q_m
//          -- each what a q-base InnerProductPlan::multiply_accumulate gives (D = terms for d0 and d2, D = 2 * terms for
//          d1 -- the cap on terms keeps that inside INNERPROD_MAX_DIGITS -- C = 1, the polynomials of y in the key's
//          place),
//       2. k = apply(d2, key, count, components = 2, input_ntt = true, output_ntt),
//       3. out[c] = (k[c] + d_c) mod q_m; with output_ntt false d_c is inverse-transformed over the q-base before the
//          addition.
//     With terms = 1 this is multiply_relinearize's definition, and the two calls return the same words.
//     What runs instead is multiply_relinearize's sequence with the two kernels that loop over t (relinearize_sum.hip):
//       tensor_top_sum: d2 into the scratch's c_coeff region (one exact mac per term, ONE fold);
//       the q-base INTT in place, mod_up (centred), the full-base NTT over D * count * M polynomials;
//       inner_product_tensor_sum: acc[c][r][m][j] = (sum_d a[d][r][m][j] * key[d][c][limb(m)][j]
//                                 + [m < L] (P mod q_m) * d_c[r][m][j]) mod q_m -- d0 and d1 summed over t on the fly in
//                                 the exact accumulator (at most one carry per mac, D + 3 * terms <= 160 of them), never
//                                 written to memory; the K special limbs load nothing of x or y;
//       finish over 2 * count stacks.
//     The key switch (INTT, ModUp, NTT over D * M, inner product, INTT over M, ModDown, NTT) does not grow with terms;
//     6 * terms + 1 passes over count * L * N words remain.
//     NOT word for word sum_t multiply_relinearize(x_t, y_t): that expression decomposes `terms` top terms and rounds
//     `terms` times, this one decomposes their sum and rounds once.  ModUp is not additive, so with an arbitrary key the
//     two are unrelated words and no bound on their difference is promised; only the decrypted values agree, and this
//     call carries the noise of one key switch and one ModDown instead of `terms`.
//     Exactness of the fold is multiply_relinearize's argument, unchanged by the sum: P d_c vanishes in the special
//     limbs, so mod_down's conv_j is what it is for step 2's accumulators alone, and
//       (c_j + P d - conv_j) P^-1 = d + (c_j - conv_j) P^-1  (mod q_j),
//     the right side is step 3's sum and both sides are canonical residues: the same word, also after the linear,
//     canonical forward NTT.
//     Allocates nothing, never synchronises: one stream, capturable as it is.  count = 0: nothing is launched.  out may
//     be exactly any one of the x[t] or y[t]: every read of them (the two kernels above) precedes mod_down's first write
//     on the stream.  std::invalid_argument, before anything is launched: terms outside [1, 32], a null array, a null
//     entry, a null key / out / scratch, a scratch that is not 256-byte aligned, count < 0, a count beyond the limits
//     multiply_relinearize checks, any other overlap of out or the scratch with an operand or with each other, a plan
//     built without transforms
//   linear_transform_bsgs(a, c0, c1, baby_keys, baby_elements, n1, giant_keys, giant_elements, n2, weights, out, count,
//     output_ntt, scratch):  a baby-step/giant-step linear transform, double hoisted (Bossuat et al.): everything stays in
//     the extended base P Q until ONE final ModDown, with n1 + n2 switching keys for n1 * n2 diagonals.
//     CONVENTION: out = sum_g sigma_{k_g}( sum_b pt_{g,b} (.) sigma_{k_b}(ct) ).  The diagonal is applied BEFORE the giant
//     rotation, so a caller pre-rotates its diagonals by the inverse giant step, as every BSGS does.
//     a = T[D][count][M][N], what decompose writes for the second components.  c0, c1 = T[count][L][N] in NTT form, any
//     word, read modulo q_m; c0 may be nullptr ("no first component", as in rotate_hoisted); c1 is required only if some
//     baby key is nullptr.  baby_elements / giant_elements: odd once reduced as GPU_Automorphism_NTT reduces them;
//     duplicates and the identity are allowed.  Keys = T[D_key][2][key_mod_count][N], read through the plan's
//     key_mod_count / key_limbs; every key word may hold any value, it is read modulo q_m, as rotate_hoisted reads its
//     keys.  **A nullptr key means "no key switch for this step" and is accepted only where the
//     reduced element is 1**: the usual b = 0 and g = 0 steps need no identity key.
//     weights = a HOST array of n2 * n1 device pointers, row-major [g][b]; weights[g * n1 + b] = T[M][N], the diagonal
//     pt_{g,b} in NTT form over the FULL base, any word.  **A nullptr entry means the term is ABSENT (weight 0) -- unlike
//     rotate_hoisted_sum, where nullptr means 1.**  The array itself must not be nullptr and every giant row g must have
//     at least one present weight.  Limits: 1 <= n1 <= 64, 1 <= n2 <= 64, n1 * n2 <= KEYSWITCH_MAX_DIAGONALS = 256.
//     out = T[2][count][L][N].
//     DEFINITION, word for word, through the calls that exist beside it; every residue canonical, pi = galois_ntt_source:
//       1. baby accumulators u_b, b < n1.  With a key, rotate_hoisted's acc:
//            u_b[c][r][m][j] = (sum_d a[d][r][m][pi_b(j)] * key_b[d][c][limb(m)][j]
//                               + [c = 0, m < L, c0 != nullptr] (P mod q_m) * c0[r][m][pi_b(j)]) mod q_m;
//          with a nullptr key: u_b[c][r][m][j] = [m < L] (P mod q_m) * (c_c[r][m][j] mod q_m) mod q_m, c_0 = c0 (0 if
//          nullptr), c_1 = c1.
//       2. v_g[c][r][m][j] = (sum_{b: present} (w_{g,b}[m][j] mod q_m) * u_b[c][r][m][j]) mod q_m -- a full-base
//          InnerProductPlan::multiply_accumulate with the n1 stacks as digits, the weights as the key (absent = zero
//          limbs), C = 1, over 2 * count inputs.
//       3. giant step g with a key: t_g = mod_down(full-base GPU_INTT(v_g[1]), stacks = count); a'_g = decompose(t_g,
//          count, input_ntt = false);
//            s_g[c][r][m][j] = (sum_d a'_g[d][r][m][pi_g(j)] * gkey_g[d][c][limb(m)][j] + [c = 0] v_g[0][r][m][pi_g(j)])
//                              mod q_m for ALL m < M, with multiplier 1
//          -- GPU_Automorphism_NTT + multiply_accumulate + GPU_Automorphism_NTT(v_g[0]) added mod q_m.  With a nullptr
//          key: s_g = v_g.  Multiplier 1 is right because v_g already lives at scale P (step 1 folded c0 in as P c0) and
//          so do the key-switch accumulators of decompose(mod_down(V1)).
//       4. acc[c][r][m][j] = (sum_g s_g[c][r][m][j]) mod q_m, then finish over 2 * count stacks: the full-base INTT,
//          mod_down, [output_ntt: the q-base NTT].
//     The fused path computes canonical residues of the same exact sums, so every word equals this composition; the
//     order of summation and the reordering of steps inside the scratch (keyed steps first) cannot change a word.  With
//     n2 = 1, a nullptr giant key, every baby key and every weight present, the call returns EXACTLY rotate_hoisted_sum's
//     words for the same operands.
//     What runs, no step's launch count growing with count, n1 or n2: inner_product_galois over the
//     keyed baby steps and bsgs_scale_input over the others (each only if there is such a step); bsgs_weighted_sum;
//     if a giant step has a key, the full-base INTT, mod_down, mod_up (centred) and the full-base NTT over all keyed
//     giant steps at once; inner_product_galois_giant; finish.
//     Contract as for rotate_hoisted_sum: allocates nothing, never synchronises, one stream, capturable as it is; count =
//     0 launches nothing.  The scratch is bsgs_scratch_bytes(count, n1, n2) bytes, 256-byte aligned; out and the scratch
//     must not overlap a, c0, c1, any key, any present weight or each other.  std::invalid_argument, before anything is
//     launched: n1, n2 or their product out of range; count < 0 or beyond the grid / int limits of the transforms, mod_up
//     and mod_down at (n2 * count, D * n2 * count * M) stacks; an even element; a nullptr key at an element != 1; a
//     nullptr c1 while some baby key is nullptr; a nullptr weights array; a giant row with no present weight; a nullptr
//     a / out / array / scratch; a misaligned scratch; an overlap; a plan without transforms
//   linear_transform_bsgs_rescale:  the same on a plan built with rescale_limbs = R > 0: out = T[2][count][L'][N], step 4
//     ends in mod_down_rescale and the NTT over the L' kept moduli, exactly as rotate_hoisted_sum_rescale relates to
//     rotate_hoisted_sum; std::invalid_argument on a plan with R = 0
//
// Rescaling.  A plan built with rescale_limbs = R, 1 <= R <= L - 1, also divides by the last R q-primes -- the rescale that
// follows every CKKS product (R = 1; R = 2 on 32-bit rings).  L' = L - R limbs are kept, Q_R = q_{L-R} ... q_{L-1},
// D_R = P Q_R.  Every call below throws std::invalid_argument on a plan with R = 0.
//   mod_down_rescale(x, out, stacks):  x = T[stacks][M][N] (coefficient form, full base), out = T[stacks][L'][N]:
//       out[s][j] = what BaseConvPlan({q_{L-R} .. q_{L-1}, p_0 .. p_{K-1}} -> {q_0 .. q_{L'-1}})::convert_and_divide gives
//                   in centred mode with in = limbs L' .. M-1 of stack s and c = limbs 0 .. L'-1 of stack s:
//                   round(x / D_R) in the kept base outside that header's rounding band
//     ONE launch of the strided kernel mod_down launches, with a second constants image: the R dropped q-limbs and the K
//     special limbs are one contiguous run of the stack, L' N words behind its start, and are read in place (in = x + L' N,
//     strides {M N, M N, L' N}; K + R <= 63 inputs, so the LDS stays below 64 KiB).  Checks and overlap rule: mod_down's,
//     with the new sizes
//   rescale(x, out, stacks, ntt_form, scratch):  x = T[stacks][L][N] over the q-base, every word any value, read modulo its
//     q; out = T[stacks][L'][N].  For a ciphertext that has not passed a key switch: a ct x pt product, a sum.
//     ntt_form = false, DEFINITION, word for word: convert_and_divide of BaseConvPlan({q_{L-R} .. q_{L-1}} ->
//       {q_0 .. q_{L'-1}}), centred, with in = the dropped limbs of stack s and c = the kept limbs.  ONE launch of the
//       strided kernel with a third image; no scratch (nullptr)
//     ntt_form = true, DEFINITION: the q-base inverse transform of x, then that conversion, then the forward transform over
//       the L' kept moduli.  What runs instead, no step's launch count growing with stacks:
//         1. rescale_gather: the dropped limbs, each word reduced modulo its q, into the scratch T[stacks][R][N];
//         2. the inverse transform over R * stacks polynomials in the scratch (the R dropped moduli only);
//         3. the dense centred conversion (no division) from the scratch into out: conv_j in coefficient form;
//         4. the forward transform over L' * stacks polynomials in place on out;
//         5. rescale_sub_scale: out[s][j] = ((x[s][j] mod q_j) - out[s][j]) * Q_R^-1 mod q_j, canonical.
//       R + L' transforms per stack instead of L + L'.  This equals the definition word for word: with c the coefficient
//       form of x, the definition is NTT_j((c_j - conv_j) Q_R^-1 mod q_j); the forward transform is linear modulo q_j, so
//       that is (NTT_j(c_j) - NTT_j(conv_j)) Q_R^-1 mod q_j, NTT_j(c_j) is x_j as a residue and NTT_j(conv_j) is what step 4
//       leaves in out; both sides are canonical residues, hence the same word
//     The scratch is rescale_scratch_bytes(stacks) bytes, 256-byte aligned; out must not overlap x or the scratch, nor the
//     scratch x.  Allocates nothing, never synchronises, capturable as it is; stacks = 0 launches nothing.  A plan without
//     transforms supports ntt_form = false only
//   multiply_relinearize_rescale, multiply_relinearize_sum_rescale, rotate_hoisted_sum_rescale:  arguments, refusals,
//     scratch sizes and the rule "out may be exactly an operand" are those of the call without the suffix; out =
//     T[2][count][L'][N].  DEFINITION, through the existing calls: the accumulators of the call without the suffix as its
//     own description gives them -- for the two products, the full-base multiply_accumulate of decompose(d2) with the key;
//     for the rotations, acc of rotate_hoisted_sum without its c0 term -- taken to coefficient form by the full-base
//     inverse transform; P d_c (P c0, rotated and weighted) in coefficient form added to their q-limbs modulo q_m; then
//     mod_down_rescale over 2 * count stacks and, with output_ntt, the forward transform over the L' kept moduli.  What
//     runs is the existing sequence up to the accumulators in the scratch (the P d fold in the NTT domain, equal by
//     linearity), then finish with the rescale flag: the full-base INTT, mod_down_rescale, [the NTT over L' * stacks].
//     NOT word for word "the call without the suffix, then rescale": that expression rounds twice, this one once.  With X
//     the integer in the full-base stack, the two steps return round(round(X / P) / Q_R), this call round(X / (P Q_R)).
//     The two differ by at most 1 per coefficient outside the rounding bands: round(X / P) = X / P + e with |e| <= 1/2
//     moves the argument of the outer round by at most 1 / (2 Q_R), so the two-step value lies within 1/2 + 1 / (2 Q_R)
//     of X / (P Q_R) and the fused one within 1/2 -- two integers less than 2 apart.
//     The P d fold stays exact: P d vanishes modulo the p_k, and modulo the dropped q-limbs it is simply part of X -- the
//     conversion now reads those limbs, and they hold c_j + P d as the definition says.
//     switch_digits, apply and rotate_hoisted get no rescale variant: a key switch or a rotation alone does not change the
//     scale
//   workspace and waits with R > 0: two more constants images (bc_image of {q_{L-R} .., p} -> {q_0 ..} and of {q_{L-R} ..}
//     -> {q_0 ..}) and, when the plan has transforms, two more NTTPlans -- forward over the first L' moduli (the same table
//     pointer), inverse over the R dropped moduli (table pointer, moduli and n^-1 values L' slots on) -- which wait for the
//     stream once each: up to eight host waits per plan, none afterwards.  With R = 0 workspace_bytes, the waits and every
//     launch are those of a plan built without the argument
//
// Key material.  THE KEY CONVENTION, stated once: a switching key from the secret s_from to the secret s is
//   key = T[D][2][M][N] in NTT form over the full base,  key[d] = (-a_d s + e_d + P g_d s_from,  a_d),
//   g_d = (Q / Q_d) [(Q / Q_d)^-1 mod Q_d]  -- so P g_d is (P mod q_m) on the limbs m of digit d and 0 on every other
//   limb, the special limbs included --, a_d uniform, e_d small.  A relinearization key has s_from = s^2 (a pointwise
//   product in NTT form), the key of the automorphism k has s_from = sigma_k(s) (GPU_Automorphism_NTT).  A ciphertext is
//   (c0, c1) with c0 + c1 s = m + e.  The three calls below make such keys and ciphertexts on the device; their
//   randomness comes in as buffers (rns/sampling.cuh fills them for tests and benchmarks; a production caller uses its
//   own generator).
//   lift_small(small, out, polys, full_base, to_ntt):  small = int32[polys][N], any value; out = T[polys][B][N] with
//     B = M (full_base) or L.  out[p][m][j] = the canonical residue of the signed value small[p][j] modulo modulus m;
//     with to_ntt the plan's forward transform over that base follows in place (polys * B polynomials).  This is how a
//     caller obtains s in the form the calls below read.  ONE launch (lift_small) plus the transform's own; no scratch;
//     allocates nothing, never synchronises; polys = 0 launches nothing.  std::invalid_argument: polys < 0 or
//     polys * B beyond an int, a null pointer, small overlapping out, to_ntt on a plan without transforms
//   generate_keys(s_ntt, s_from_ntt, errors, keys_host, keys, scratch):  0 <= keys <= KEYGEN_MAX_KEYS = 64.
//     s_ntt = T[M][N], the target secret over the full base in NTT form, any word, read modulo modulus m;
//     s_from_ntt = T[keys][M][N], the source secrets, likewise; errors = int32[keys][D][N]; keys_host = a HOST array of
//     `keys` device pointers, each T[D][2][M][N]: component 1 holds a on entry (any word) and is left untouched,
//     component 0 is written.  DEFINITION, word for word, with E = the full-base GPU_NTT of lift_small(errors):
//       key[g][d][0][m][j] = (E[g][d][m][j] - a[g][d][m][j] s[m][j] + [m in S_d] (P mod q_m) s_from[g][m][j]) mod m_m,
//     canonical; the gadget term is absent on every limb outside digit d and on the special limbs.
//     What runs: lift_small into the scratch T[keys][D][M][N], ONE full-base NTT over keys * D * M polynomials, ONE
//     launch of keygen_combine over all keys (the key pointers travel in the kernel argument, as rotate_hoisted's do).
//     Allocates nothing, never synchronises, capturable as it is; keys = 0 launches nothing.  The scratch is
//     keygen_scratch_bytes(keys) bytes, 256-byte aligned.  std::invalid_argument, before anything is launched: keys
//     outside [0, 64]; a null pointer or a null entry; an overlap among the scratch, the keys, the secrets and the
//     errors; a misaligned scratch; a plan without transforms; a plan whose key_mod_count != M or whose key_limbs is not
//     the identity -- keys are generated by the plan of the level they are laid out for, lower-level plans read them
//     through key_limbs
//   encrypt_symmetric(s_ntt, errors, message_ntt, out, count, scratch):  out = T[2][count][L][N] with out[1] = a on
//     entry (any word), untouched; errors = int32[count][N]; message_ntt = T[count][L][N] in NTT form over the q-base
//     (any word) or nullptr -- an encryption of zero, which is also how a public key is made.  Only the first L limbs of
//     s_ntt are read.  DEFINITION, with E = the q-base GPU_NTT of lift_small(errors):
//       out[0][r][m][j] = (E[r][m][j] - a[r][m][j] s[m][j] + message[r][m][j]) mod q_m, canonical.
//     The same kernel over the first L limbs, one row per ciphertext, the message in the gadget term's place with
//     multiplier 1.  The scratch is encrypt_scratch_bytes(count) bytes (T[count][L][N]), 256-byte aligned; refusals as
//     for generate_keys (count < 0 in the place of keys).  Public-key encryption: encrypt_public below.  Not here:
//     coefficient-form output, fixed-Hamming-weight secrets, BGV error scaling, a sampler fused into the combine kernel
//     
//
// Decryption and public-key encryption (the kernels are in decrypt.hip).
//   phase(ct, s_ntt, out, count, components, input_ntt, output_ntt, scratch):  c0 + c1 s [+ c2 s^2], what CKKS and BFV both
//     decrypt from.  components in {2, 3}; ct = T[components][count][L][N]; s_ntt = T[M][N] as encrypt_symmetric takes it
//     (any word, read modulo its limb; only the first L limbs are read); out = T[count][L][N].  DEFINITION, word for word:
//       1. [input_ntt false: the q-base GPU_NTT of ct into the scratch, components * count * L polynomials; canonical
//          words are required, as for any transform]
//       2. out[r][m][j] = (c0[r][m][j] + c1[r][m][j] s[m][j] + c2[r][m][j] s[m][j]^2) mod q_m, canonical, from ANY input
//          words (c2 = 0 with two components)
//       3. [output_ntt false: the q-base GPU_INTT of out in place, count * L polynomials]
//     What runs: [the NTT,] ONE launch of decrypt_phase -- the exact accumulator of the inner product seeded with c0, one
//     mac per product, one fold per output word; with three components s^2 is formed in registers at three more Shoup
//     products per word (one makes s canonical, two are the partial fold of s * s) -- [the INTT].  phase_scratch_bytes(count,
//     components, input_ntt) is 0 for NTT-form input (the scratch may then be nullptr) and T[components][count][L][N]
//     otherwise, 256-byte aligned.  out may be exactly ct (component 0's place) in NTT form.  Allocates nothing, never
//     synchronises, capturable as it is; count = 0 launches nothing.  std::invalid_argument, before anything is
//     launched: components outside {2, 3} ("Invalid components!"), count < 0 or components * count * L beyond an int, a
//     null pointer, out overlapping ct (other than being exactly ct in NTT form) or s, the scratch overlapping ct, s or
//     out, a misaligned scratch, a transform on a plan without transforms
//   encrypt_public(pk, small, message_ntt, out, count, scratch):  pk = T[2][L][N] in NTT form, any word -- what
//     encrypt_symmetric(count = 1, message = nullptr) leaves in out: pk0 + pk1 s = e_pk; small = int32[3][count][N] holding
//     (u, e0, e1), any value; message_ntt = T[count][L][N] in NTT form (any word) or nullptr; out = T[2][count][L][N].
//     DEFINITION, with U, E0, E1 = the q-base GPU_NTT of lift_small(small):
//       out[0][r][m][j] = (pk[0][m][j] U[r][m][j] + E0[r][m][j] + message[r][m][j]) mod q_m
//       out[1][r][m][j] = (pk[1][m][j] U[r][m][j] + E1[r][m][j]) mod q_m,
//     both canonical: out0 + out1 s = m + e_pk u + e0 + e1 s.  What runs: ONE lift_small over 3 * count polynomials into
//     the scratch T[3][count][L][N] (encrypt_public_scratch_bytes(count) bytes, 256-byte aligned), ONE q-base NTT over
//     3 * count * L polynomials, ONE launch of encrypt_public_combine, which writes both components from one read of U
//     (keygen_combine's accumulator and fold).  Refusals as for encrypt_symmetric.  Not here: a sampler fused into the
//     kernel, coefficient-form output, BGV error scaling
//
// Plaintext operands (the kernels are in keygen.hip).  How a plaintext modulo a word-sized t -- what
// BfvBatchEncoder::encode (rns/bfv_encode.cuh) writes -- becomes an operand of a ciphertext, on the device.
//   lift_centred(words, t, out, polys, full_base, to_ntt):  a sibling of lift_small.  words = T[polys][N], any word;
//     out = T[polys][B][N] with B = M (full_base) or L.  DEFINITION, in integers: m = word mod t, v = m - t if
//     m >= (t + 1) >> 1, else m; out[p][i][j] = v mod modulus_i, canonical; with to_ntt the plan's forward transform
//     over that base follows in place.  The centred lift multiplies the noise by |pt| <= t / 2 and not by t.  ONE launch
//     (lift_centred) plus the transform's own; no scratch.  t is any value Modulus<T> accepts, from 2 on; it may exceed
//     a limb's modulus.  This is how a plaintext operand of multiply_plain (q-base, NTT form) or a diagonal for
//     rotate_hoisted_sum / linear_transform_bsgs (full base, NTT form) is made.  Refusals are lift_small's, and
//     "Invalid plaintext modulus!" for a t outside that range
//   multiply_plain(ct, pt_ntt, out, count, plain_count):  ct = T[2][count][L][N] and pt_ntt = T[plain_count][L][N], both in
//     NTT form and both holding any word; plain_count in {1, count}: 1 means the plaintext is shared (otherwise
//     "Invalid plain_count!").  out[c][r][i][j] = (ct[c][r][i][j] * pt[r or 0][i][j]) mod q_i, canonical.  ONE launch of
//     multiply_plain, which writes both components from one read of the plaintext word: the inner product's mac and
//     fold with one term, no new arithmetic.  out may be exactly ct; any other overlap of out with an operand is
//     refused ("out overlaps an operand!").  Works on a plan without transforms.  Allocates nothing, never synchronises,
//     capturable as it is; count = 0 launches nothing.  Not here: add_plain (one modular addition of scale_message's
//     output to component 0), three-component inputs, a coefficient-form path
//
//   * ranges: 1 <= L, 1 <= K, M = L + K <= 64, alpha >= 1, 1 <= components <= 4, count >= 0 and stacks >= 0 (0: nothing
//     happens), n_power in [1, 28], M <= key_mod_count <= 256.  A plan is built for ONE level (one L) and one ring; a
//     caller at a lower level builds another plan and points it at the full-level key through key_mod_count /
//     key_limbs_host (limb of the key for every modulus of THIS plan's full base; nullptr: limb m)
//   * transforms: the plan builds four NTTPlan<T> (forward and inverse over the full base, inverse and forward over the
//     q-base) from ONE caller table pair -- forward_table_device / inverse_table_device as for GPU_NTT / GPU_INTT, slot i
//     at i << n_power in full-base order, so the q-base is the first L slots -- plus the M host n^-1 values, the
//     reduction polynomial and a batch_hint.  The tables must outlive the plan (NTTPlan).  Both table pointers nullptr: a
//     plan without transforms -- mod_up and mod_down work for any moduli Modulus<T> accepts (not necessarily prime), the
//     pipeline methods throw
//   * workspace: every constant and every NTTPlan lives in workspace_bytes(L, K, alpha, n_power) bytes of device memory
//     (nullptr = the plan allocates and owns it; owns_workspace()).  The constructor waits for `stream`: once for its own
//     constants and once in each plan it builds (the inner product's and the four NTTPlans) -- up to six host waits per
//     plan, none afterwards.  rescale_limbs = R > 0: workspace_bytes(L, K, alpha, n_power, R) bytes and two more waits
//     ("Rescaling" above); R outside [0, L - 1]: std::invalid_argument ("Invalid rescale_limbs!")
//   * scratch: scratch_bytes(L, K, alpha, n_power, count, components) bytes owned by the CALLER, 256-byte aligned; the
//     pipeline methods allocate nothing and never synchronise, so apply can be captured on one stream as it is.
//     mod_up and mod_down allocate nothing, never synchronise and launch exactly one kernel
//   * std::invalid_argument: the moduli of the full base are not pairwise coprime, a modulus is not the Modulus<T> of its
//     value ("Invalid modulus!"), n_power outside [1, 28] ("Invalid n_power range!"), a count outside the ranges above,
//     alpha < 1, a null pointer, buffers that overlap where the contract forbids it, a pipeline call on a plan
//     without transforms
#pragma once

#include <cstddef>
#include <cstdint>

#include "gpuntt/common/common.cuh"
#include "gpuntt/common/modular_arith.cuh"
#include "gpuntt/common/nttparameters.cuh"
#include "gpuntt/rns/base_conversion.cuh"
#include "gpuntt/rns/inner_product.cuh"

namespace gpuntt
{
    constexpr int KEYSWITCH_MAX_TERMS = 32; // multiply_relinearize_sum: pairs of ciphertexts per call
    constexpr int KEYSWITCH_MAX_DIAGONALS = 256; // linear_transform_bsgs: n1 * n2, the weight pointers of one call
    constexpr int KEYSWITCH_MAX_STEPS = 64;      // linear_transform_bsgs: n1 and n2 each
    constexpr int KEYGEN_MAX_KEYS = 64;          // generate_keys: switching keys per call

    // The plan's constants as the host derived them (KeySwitchPlan::constants, gpuntt_keyswitch_constants_*): every
    // pointer is a caller array of the stated length.  d(i) = i / alpha is the digit of q-limb i.
    template <typename T> struct KeySwitchConstants
    {
        // ModUp, per digit: BaseConvPlan::constants({q_i : i in S_d} -> the other M - |S_d| moduli in full-base order)
        T* up_qhat_inv;       // [L]    (Q_d(i) / q_i)^-1 mod q_i
        T* up_qhat_inv_shoup; // [L]    its Shoup companion
        T* up_matrix;         // [L][M] (Q_d(i) / q_i) mod modulus m; 0 where m is in S_d(i) (never used)
        T* up_q_mod;          // [D][M] Q_d mod modulus m (0 where m is in S_d)
        T* up_recip;          // [L]    R_i mod 2^W
        T* up_bit_length;     // [L]    b_i
        // ModDown: BaseConvPlan::constants({p_k} -> {q_j})
        T* down_qhat_inv;       // [K]
        T* down_qhat_inv_shoup; // [K]
        T* down_matrix;         // [K][L]
        T* down_p_mod_q;        // [L] P mod q_j
        T* down_p_inv_mod_q;    // [L] P^-1 mod q_j
        T* down_recip;          // [K]
        T* down_bit_length;     // [K]
        // the folding constants of the final reductions, per modulus of the full base: InnerProductPlan::constants
        T* pow_w;        // [M]
        T* pow_w_shoup;  // [M]
        T* pow_2w;       // [M]
        T* pow_2w_shoup; // [M]
        T* one_shoup;    // [M]
    };

    template <typename T> class KeySwitchPlan
    {
      public:
        static size_t workspace_bytes(int q_count, int p_count, int alpha, int n_power, int rescale_limbs = 0);
        static size_t scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count, int components);
        static size_t hoisted_scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count, int elements);
        static size_t hoisted_sum_scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count);
        static size_t bsgs_scratch_bytes(int q_count, int p_count, int alpha, int n_power, int count, int n1, int n2);
        static int digits(int q_count, int alpha); // D

        KeySwitchPlan(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* p_moduli_host, int p_count,
                      int alpha, int n_power, const Root<T>* forward_table_device, const Root<T>* inverse_table_device,
                      const Ninverse<T>* mod_inverse_host, ReductionPolynomial reduction_poly, int batch_hint,
                      int key_mod_count, const int* key_limbs_host, stream_t stream, void* workspace_device = nullptr,
                      int rescale_limbs = 0);
        ~KeySwitchPlan();
        KeySwitchPlan(const KeySwitchPlan&) = delete;
        KeySwitchPlan& operator=(const KeySwitchPlan&) = delete;

        void mod_up(const T* device_in, T* device_a, int count, BaseConvMode mode, stream_t stream) const;
        void mod_down(const T* device_x, T* device_out, int stacks, stream_t stream) const;
        void mod_down_add(const T* device_x, const T* device_addend, T* device_out, int stacks, stream_t stream) const;
        void decompose(const T* device_c_in, T* device_a, int count, bool input_ntt, void* scratch_device,
                       stream_t stream) const;
        void switch_digits(const T* device_a, const T* device_key, T* device_out, int count, int components,
                           bool output_ntt, void* scratch_device, stream_t stream) const;
        void apply(const T* device_c_in, const T* device_key, T* device_out, int count, int components, bool input_ntt,
                   bool output_ntt, void* scratch_device, stream_t stream) const;
        void rotate_hoisted(const T* device_a, const T* device_c0, const T* const* device_keys_host,
                            const std::uint32_t* galois_elements_host, int elements, T* device_out, int count,
                            bool output_ntt, void* scratch_device, stream_t stream) const;
        void rotate_hoisted_sum(const T* device_a, const T* device_c0, const T* const* device_keys_host,
                                const std::uint32_t* galois_elements_host, const T* const* device_weights_host,
                                int elements, T* device_out, int count, bool output_ntt, void* scratch_device,
                                stream_t stream) const;

        void multiply_relinearize(const T* device_x, const T* device_y, const T* device_key, T* device_out, int count,
                                  bool output_ntt, void* scratch_device, stream_t stream) const;
        void multiply_relinearize_sum(const T* const* device_x_host, const T* const* device_y_host, int terms,
                                      const T* device_key, T* device_out, int count, bool output_ntt,
                                      void* scratch_device, stream_t stream) const;

        void relinearize(const T* device_c01, const T* device_c2, const T* device_key, T* device_out, int count,
                         bool input_ntt, bool output_ntt, void* scratch_device, stream_t stream) const;

        // rescaling: a plan built with rescale_limbs = R > 0; every one of them throws on a plan with R = 0
        void mod_down_rescale(const T* device_x, T* device_out, int stacks, stream_t stream) const;
        void rescale(const T* device_x, T* device_out, int stacks, bool ntt_form, void* scratch_device,
                     stream_t stream) const;
        size_t rescale_scratch_bytes(int stacks) const; // the scratch of rescale(ntt_form = true): T[stacks][R][N]
        void multiply_relinearize_rescale(const T* device_x, const T* device_y, const T* device_key, T* device_out,
                                          int count, bool output_ntt, void* scratch_device, stream_t stream) const;
        void multiply_relinearize_sum_rescale(const T* const* device_x_host, const T* const* device_y_host, int terms,
                                              const T* device_key, T* device_out, int count, bool output_ntt,
                                              void* scratch_device, stream_t stream) const;
        void rotate_hoisted_sum_rescale(const T* device_a, const T* device_c0, const T* const* device_keys_host,
                                        const std::uint32_t* galois_elements_host, const T* const* device_weights_host,
                                        int elements, T* device_out, int count, bool output_ntt, void* scratch_device,
                                        stream_t stream) const;

        // the double-hoisted baby-step/giant-step linear transform ("linear_transform_bsgs" above); _rescale: R > 0
        void linear_transform_bsgs(const T* device_a, const T* device_c0, const T* device_c1,
                                   const T* const* baby_keys_host, const std::uint32_t* baby_elements_host, int n1,
                                   const T* const* giant_keys_host, const std::uint32_t* giant_elements_host, int n2,
                                   const T* const* weights_host, T* device_out, int count, bool output_ntt,
                                   void* scratch_device, stream_t stream) const;
        void linear_transform_bsgs_rescale(const T* device_a, const T* device_c0, const T* device_c1,
                                           const T* const* baby_keys_host, const std::uint32_t* baby_elements_host, int n1,
                                           const T* const* giant_keys_host, const std::uint32_t* giant_elements_host,
                                           int n2, const T* const* weights_host, T* device_out, int count,
                                           bool output_ntt, void* scratch_device, stream_t stream) const;
        size_t bsgs_scratch_bytes(int count, int n1, int n2) const;

        // key material ("Key material" above)
        void lift_small(const std::int32_t* device_small, T* device_out, int polys, bool full_base, bool to_ntt,
                        stream_t stream) const;
        size_t keygen_scratch_bytes(int keys) const;   // T[keys][D][M][N]
        size_t encrypt_scratch_bytes(int count) const; // T[count][L][N]
        void generate_keys(const T* device_s_ntt, const T* device_s_from_ntt, const std::int32_t* device_errors,
                           T* const* device_keys_host, int keys, void* scratch_device, stream_t stream) const;
        void encrypt_symmetric(const T* device_s_ntt, const std::int32_t* device_errors, const T* device_message_ntt,
                               T* device_out, int count, void* scratch_device, stream_t stream) const;

        // plaintext operands ("Plaintext operands" above)
        void lift_centred(const T* device_words, T plain_modulus, T* device_out, int polys, bool full_base, bool to_ntt,
                          stream_t stream) const;
        void multiply_plain(const T* device_ct, const T* device_pt_ntt, T* device_out, int count, int plain_count,
                            stream_t stream) const;

        // decryption and public-key encryption ("Decryption and public-key encryption" above)
        size_t phase_scratch_bytes(int count, int components, bool input_ntt) const; // 0 for NTT-form input
        void phase(const T* device_ct, const T* device_s_ntt, T* device_out, int count, int components, bool input_ntt,
                   bool output_ntt, void* scratch_device, stream_t stream) const;
        size_t encrypt_public_scratch_bytes(int count) const; // T[3][count][L][N]
        void encrypt_public(const T* device_pk, const std::int32_t* device_small, const T* device_message_ntt,
                            T* device_out, int count, void* scratch_device, stream_t stream) const;

        int q_count() const;
        int rescale_limbs() const; // R
        int p_count() const;
        int key_mod_count() const;
        int alpha() const;
        int digits() const;
        int n_power() const;
        bool has_transforms() const;
        Modulus<T> modulus(int m) const;            // modulus m < M of the full base, as the constructor took it
        ReductionPolynomial reduction_poly() const; // as the constructor took it
        bool owns_workspace() const; // false: the plan lives in the caller's workspace and has allocated nothing
        size_t scratch_bytes(int count, int components) const;
        size_t hoisted_scratch_bytes(int count, int elements) const;
        size_t hoisted_sum_scratch_bytes(int count) const;

        // host only (no GPU): the constants of these bases, with the checks of the constructor
        static void constants(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* p_moduli_host, int p_count,
                              int alpha, const KeySwitchConstants<T>& out);
        // host only (no GPU): mod_up / mod_down on HOST arrays, with unsigned __int128 and %, after the same argument
        // checks.  What tests and examples compare the kernels with; never a GPU fall-back
        static void reference_mod_up(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* p_moduli_host,
                                     int p_count, int alpha, const T* in_host, T* a_host, int n_power, int count,
                                     BaseConvMode mode);
        static void reference_mod_down(const Modulus<T>* q_moduli_host, int q_count, const Modulus<T>* p_moduli_host,
                                       int p_count, const T* x_host, T* out_host, int n_power, int stacks);
        // host only (no GPU): mod_down_rescale and rescale(ntt_form = false) on HOST arrays, in the same manner.
        // rescale_limbs outside [1, q_count - 1] throws ("Invalid rescale_limbs!")
        static void reference_mod_down_rescale(const Modulus<T>* q_moduli_host, int q_count,
                                               const Modulus<T>* p_moduli_host, int p_count, int rescale_limbs,
                                               const T* x_host, T* out_host, int n_power, int stacks);
        static void reference_rescale(const Modulus<T>* q_moduli_host, int q_count, int rescale_limbs, const T* x_host,
                                      T* out_host, int n_power, int stacks);

      private:
        struct Impl;
        Impl* p_;
    };
} // namespace gpuntt
