/*
 * include/binius_amd_host.h -- C entry points of libbinius_amd_host.so, the COMPILED HOST MIRROR.
 *
 * This is NOT the drop-in boundary (that is include/binius_amd.h, which the reference's Rust host
 * binds directly).  The reference's callers of the HAL are Rust generics over ComputeLayer; with no
 * Rust toolchain in the build image they are mirrored in C++ (binius_amd/host/compute_layer.hpp,
 * sumcheck.hpp) and driven through these few calls, so that tests and bench.py run the prover loops
 * at compiled-host speed over the same C ABI:
 *
 *   bnh_bivariate_sumcheck_prove   BivariateSumcheckProver  execute/fold/finish loop
 *                                  crates/core/src/protocols/sumcheck/v3/bivariate_product.rs:27-254
 *                                  (+ the multi-GPU variants of DESIGN.md section 6)
 *   bnh_bivariate_mlecheck_prove   BivariateMLEcheckProver   v3/bivariate_mlecheck.rs:27-372
 *   bnh_shm_*                      intra-node exchange of the per-round partials (host shared memory)
 *   bnh_rccl_*                     the same exchange through one ncclAllGather per round (librccl is
 *                                  bound at run time from the process's own copy)
 *
 * All functions return 0 on success or a BN_ERR_* code; bnh_last_error() describes the last failure
 * of the calling thread's library instance.
 */
#ifndef BINIUS_AMD_HOST_H
#define BINIUS_AMD_HOST_H

#include "binius_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *bnh_last_error(void);

/* combine callback of the generic sharded variant: XOR the rank partials left in d_partial (2
 * elements: y_1, y_inf) across ranks into evals[2]; 0 on success */
typedef int (*bnh_round_reduce_fn)(void *user, const void *d_partial, bn_f128 *evals);

/* One complete prove.  d_multilins[m]: 2^n_vars elements each, never modified; d_scratch: device
 * memory for the folded copies (m * 2^(n_vars-1) elements, + 64 with tail_rounds); comp_indices:
 * n_comps pairs; sums[n_comps]; challenges[n_vars (+ log2 world with tail_rounds)];
 * round_coeffs_out[3 * rounds]; final_evals_out[m].
 * Single GPU: reduce = NULL, rccl_comm = NULL, shm = NULL.
 * Sharded (rank holds the elements with index = rank mod world): exactly one of
 *   shm        handle from bnh_shm_open: partials combined in host shared memory; with tail_rounds != 0
 *              the residual log2(world) rounds run in the same call
 *   rccl_comm  communicator from bnh_rccl_init, d_partial (2 elements) and d_gathered (2 * world
 *              elements) device buffers: one ncclAllGather per round on the context's stream
 *   reduce     caller-supplied combine of d_partial */
int bnh_bivariate_sumcheck_prove(bn_ctx *ctx, uint32_t n_vars, uint32_t m, const void *const *d_multilins, void *d_scratch,
                                 uint64_t scratch_elems, uint32_t n_comps, const uint32_t *comp_indices, const bn_f128 *sums,
                                 const bn_f128 *batch_coeff, const bn_f128 *challenges, bn_f128 *round_coeffs_out,
                                 bn_f128 *final_evals_out, bnh_round_reduce_fn reduce, void *reduce_user, void *d_partial,
                                 void *rccl_comm, int world, void *d_gathered, void *shm, int tail_rounds);

/* d_eq_ind: 2^(n_vars-1) elements = tensor expansion of eq_ind_challenges[0 .. n_vars-1);
 * round_coeffs_out[4 * n_vars] (degree-3 round polynomials); final_evals_out[m + 1] (the last one is
 * eq_ind_prefix_eval); d_scratch: (m + 1) * 2^(n_vars-1) elements (the weighted prover needs 2^n_vars per weighted
 * multilinear and 2^(n_vars-1) per other one, and is not used when the scratch is smaller than that) */
int bnh_bivariate_mlecheck_prove(bn_ctx *ctx, uint32_t n_vars, uint32_t m, const void *const *d_multilins, const void *d_eq_ind,
                                 const bn_f128 *eq_ind_challenges, void *d_scratch, uint64_t scratch_elems, uint32_t n_comps,
                                 const uint32_t *comp_indices, const bn_f128 *sums, const bn_f128 *batch_coeff,
                                 const bn_f128 *challenges, bn_f128 *round_coeffs_out, bn_f128 *final_evals_out);

/* The same prover behind a handle, one call per SumcheckProver method (prove/batch_sumcheck.rs:38-70): for hosts whose
 * challenges come out of a transcript round by round -- what the Rust shim's Mi355xMLEcheckProver binds
 * (crates/binius_mi355x/src/mlecheck.rs).  execute: coeffs_out[4]; finish: final_evals_out[m + 1]. */
typedef struct bnh_mlecheck bnh_mlecheck;
int bnh_mlecheck_new(bn_ctx *ctx, uint32_t n_vars, uint32_t m, const void *const *d_multilins, const void *d_eq_ind,
                     const bn_f128 *eq_ind_challenges, void *d_scratch, uint64_t scratch_elems, uint32_t n_comps,
                     const uint32_t *comp_indices, const bn_f128 *sums, bnh_mlecheck **out);
int bnh_mlecheck_execute(bnh_mlecheck *prover, const bn_f128 *batch_coeff, bn_f128 *coeffs_out);
int bnh_mlecheck_fold(bnh_mlecheck *prover, const bn_f128 *challenge);
int bnh_mlecheck_finish(bnh_mlecheck *prover, bn_f128 *final_evals_out);
void bnh_mlecheck_free(bnh_mlecheck *prover);

/* which prover the calling thread's last bnh_mlecheck_new / bnh_bivariate_mlecheck_prove chose: 1 = WeightedMLEcheckProver (the indicator
 * carried inside one factor of every composition; plain bivariate rounds on the matrix cores), 0 = the literal mirror
 * BivariateMLEcheckProver (no proper 2-colouring of the compositions, an indicator coordinate equal to 0 or 1, too
 * little scratch, n_vars < 2, a table that is not the expansion of the coordinates, or BN_MLECHECK=eager), -1 = none yet */
int bnh_mlecheck_last_mode(void);

/* FRI commit phase (commit_interleaved, crates/core/src/protocols/fri/prove.rs:88-198), every fold round
 * (FRIFolder::execute_fold_round, :307-432) and finalize (:444-482) through the C++ mirror
 * binius_amd/host/fri.hpp, codewords and Merkle trees resident on the device.
 * d_message: 2^(log_dim + log_batch_size) elements; d_scratch: 2 * 2^(log_dim + log_batch_size + log_inv_rate) elements are always enough (codeword + folded codewords + trees)
 * ; challenges[log_dim + log_batch_size]; roots_out[(n_arities + 1) * 32]: the commitment, then one
 * root per committed oracle; terminate_out: 2^(log_inv_rate + n_final_challenges) elements or NULL;
 * phase_ms_out[2]: wall-clock ms of the commit and of the fold phase, or NULL. */
int bnh_fri_commit_fold(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                        uint32_t n_arities, uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems,
                        const bn_f128 *challenges, uint8_t *roots_out, bn_f128 *terminate_out, double *phase_ms_out);
/* The same with the query phase: FRIFolder::finish_proof (fri/prove.rs:483-507) in place of finalize, the indices
 * transcript.sample_bits(index_bits) would have returned handed in like the challenges (query_indices[n_test_queries], each below
 * 2^index_bits with index_bits = log_dim + log_inv_rate + log_batch_size - fold_arities[0], 0 without arities).  advice_out receives the
 * decommitment in transcript byte order (bn_fri_query_openings, one launch): terminate codeword, the layer of every opened oracle at
 * its optimal depth, then per query and oracle the coset and its branch; *n_advice_elems_out: its length in field elements.
 * BN_ERR_INPUT_VALIDATION when max_advice_elems is smaller than that.  phase_ms_out[3]: commit, fold, query phase, or NULL. */
int bnh_fri_prove(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                  uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems, const bn_f128 *challenges, uint8_t *roots_out,
                  const uint64_t *query_indices, bn_f128 *advice_out, uint64_t max_advice_elems, uint64_t *n_advice_elems_out, double *phase_ms_out);

/* diagnostic (tools/bench_fri_query.py): one commit and fold, then the query phase timed warmup + runs times two ways on the same
 * resident codewords and trees, alternating -- FRIFolder::finish_proof (one launch) into new_ms_out[runs], and finalize's copy plus one
 * FRIQueryProver::prove_query per index (a copy and a gather per opening) into old_ms_out[runs]; wall clock between two
 * synchronisations.  *advice_elems_out: the length of the advice; *equal_out: both routes returned the same bytes. */
int bnh_fri_query_phase_bench(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                              uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems, const bn_f128 *challenges,
                              const uint64_t *query_indices, uint32_t warmup, uint32_t runs, double *new_ms_out, double *old_ms_out, uint64_t *advice_elems_out,
                              uint32_t *equal_out);

/* The front-loaded batch prover (SumcheckBatchProver = protocols/sumcheck/prove/front_loaded.rs:33-203, BatchProver::run with the
 * transcript's samples handed in) over p BivariateSumcheckProvers on ONE layer, ascending by number of variables: per round
 * execute() on every live prover, one challenge, fold() on every live prover; a prover finishes in the round that equals its
 * number of variables.  prover_desc[3 i ..] = (n_vars, m, n_comps); d_multilins / comp_indices / sums: the provers' lists
 * concatenated; batch_coeffs[n_provers]; challenges[max n_vars]; d_scratch: sum over provers of m * 2^(n_vars - 1) elements.
 * round_proofs_out[2 * rounds]: the truncated round polynomials (RoundCoeffs::truncate, common.rs:101-105; missing coefficients
 * zero); final_evals_out[sum m]: the final evaluations in finishing order. */
int bnh_batch_sumcheck_prove(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const void *const *d_multilins, const uint32_t *comp_indices,
                             const bn_f128 *sums, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *challenges,
                             bn_f128 *round_proofs_out, bn_f128 *final_evals_out);

/* piop::prove (crates/core/src/piop/prove.rs:148-395) through the C++ mirror binius_amd/host/piop.hpp: commit_interleaved of the
 * merged message (fri.hpp), one BivariateSumcheckProver per number of variables that has a committed multilinear, the
 * front-loaded batch prover interleaved with the FRI folder (prove_interleaved_fri_sumcheck, :306-395).
 *   committed_n_vars[n_committed] ascending, d_committed[i]: 2^n_vars elements (the packed committed multilinears, on the device)
 *   transparent_n_vars[n_transparent] ascending, d_transparent[i] likewise
 *   claims[3 i ..] = (n_vars, committed index, transparent index), claim_sums[i]          (PIOPSumcheckClaim, piop/verify.rs)
 *   d_message: 2^(log_dim + log_batch_size) elements = merge_multilins of the committed multilinears (piop/prove.rs:66-104);
 *              log_dim + log_batch_size must equal CommitMeta::total_vars
 *   d_scratch: codeword, folded codewords, Merkle trees and folded multilinears
 *   batch_coeffs: one per prover (sizes with a committed multilinear, ascending); challenges[total_vars]
 * The transcript comes back in writing order: items_out[2 i] = kind (0 round proof, 1 final evaluations of a finished prover,
 * 2 FRI round commitment, 3 FRI terminate codeword), items_out[2 i + 1] = its scalars (kinds 0, 1, 3: taken from scalars_out
 * in order) or 1 (kind 2: one 32-byte digest from digests_out).  phase_ms_out[2]: commit, prove (wall clock), or NULL. */
int bnh_piop_prove(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                   const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims, const bn_f128 *claim_sums,
                   uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities, uint32_t n_test_queries,
                   const void *d_message, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs,
                   const bn_f128 *challenges, uint32_t n_challenges, uint8_t *commitment_out, uint32_t *items_out, uint32_t max_items, uint32_t *n_items_out,
                   bn_f128 *scalars_out, uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out, uint32_t max_digests, uint32_t *n_digests_out,
                   double *phase_ms_out);

/* piop::commit (crates/core/src/piop/prove.rs:120-165) apart from piop::prove, for a caller with a live transcript: the commitment
 * is written before the first challenge of any phase is sampled (constraint_system/prove.rs:232-234), the codeword and its Merkle
 * tree are kept until piop::prove at the very end.
 * bnh_piop_message_layout: pure host arithmetic, no context.  offsets_out[i]: where multilinear i starts in the message of
 * merge_multilins (the sum of the lengths of the multilinears after it); *total_vars_out: CommitMeta::total_vars.  n_vars ascending
 * ("CommittedsNotSorted" otherwise), each below 48.
 * bnh_piop_commit_elems: the field elements the caller provides for the codeword, 2^(log_dim + log_batch_size + log_inv_rate), and
 * for the flattened tree, 2 * (2 * leaves - 1) with one leaf per coset of 2^fold_arities[0] elements (of the whole message when
 * n_arities = 0).
 * bnh_piop_commit: merge_multilins of the committed multilinears (on the device, ascending) straight into d_codeword with all
 * 2^log_inv_rate copies (bn_merge_multilins), the batched NTT, the tree into d_tree in the layout of BinaryMerkleTree{log_len,
 * nodes}: flattened layers, leaves first, root last (= commitment_out[32]).  codeword_elems and tree_elems must be what
 * bnh_piop_commit_elems states, total_vars must equal log_dim + log_batch_size; BN_ERR_INPUT_VALIDATION otherwise.
 * phase_ms_out[3]: merge, encode, Merkle (wall clock, a synchronisation after each), or NULL.
 * bnh_piop_prove_committed: bnh_piop_prove from that codeword and tree, which it only reads (any number of proves may follow one
 * commit); no d_message, no commitment_out; phase_ms_out[1]: the prove, or NULL. */
int bnh_piop_message_layout(uint32_t n, const uint32_t *n_vars, uint64_t *offsets_out, uint32_t *total_vars_out);
int bnh_piop_commit_elems(uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                          uint64_t *codeword_elems_out, uint64_t *tree_elems_out);
int bnh_piop_commit(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t log_dim, uint32_t log_inv_rate,
                    uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities, uint32_t n_test_queries, void *d_codeword, uint64_t codeword_elems,
                    void *d_tree, uint64_t tree_elems, uint8_t *commitment_out, double *phase_ms_out);
/* diagnostic: wall-clock ms of this thread's last bnh_piop_commit between the synchronisations around its commit (the quantity
 * bnh_piop_prove and bnh_fri_commit_fold report as their commit phase); with phase_ms_out NULL nothing synchronises in between */
double bnh_piop_commit_last_ms(void);
int bnh_piop_prove_committed(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                             const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims,
                             const bn_f128 *claim_sums, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                             uint32_t n_arities, uint32_t n_test_queries, const void *d_codeword, const void *d_tree, void *d_scratch, uint64_t scratch_elems,
                             const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs, const bn_f128 *challenges, uint32_t n_challenges, uint32_t *items_out,
                             uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out, uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out,
                             uint32_t max_digests, uint32_t *n_digests_out, double *phase_ms_out);
/* bnh_piop_prove_committed with the FRI query phase (prove_interleaved_fri_sumcheck ending in FRIFolder::finish_proof): the same
 * arguments and the same item list, then query_indices[n_test_queries] and the advice buffer of bnh_fri_prove.  The advice comes back
 * in its own buffer; the terminate item of the list is filled from the same block.  BN_ERR_INPUT_VALIDATION when max_advice_elems is
 * too small. */
int bnh_piop_prove_committed_open(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                                  const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims,
                                  const bn_f128 *claim_sums, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                                  uint32_t n_arities, uint32_t n_test_queries, const void *d_codeword, const void *d_tree, void *d_scratch, uint64_t scratch_elems,
                                  const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs, const bn_f128 *challenges, uint32_t n_challenges, uint32_t *items_out,
                                  uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out, uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out,
                                  uint32_t max_digests, uint32_t *n_digests_out, double *phase_ms_out, const uint64_t *query_indices, bn_f128 *advice_out,
                                  uint64_t max_advice_elems, uint64_t *n_advice_elems_out);

/* EqIndSumcheckProver (crates/core/src/protocols/sumcheck/prove/eq_ind.rs:378-644) through the C++ mirror binius_amd/host/eq_ind.hpp,
 * over the old HAL (binius_hal::ComputationBackend: bn_hal_round_evals + the ComputeLayer's folds), evaluation order High-to-Low,
 * compositions of degree 1 .. 8 (degrees[c]; NULL: all 2; evaluation points 1 ..= degree: 1, infinity, the points 2, 3, ... of the default
 * interpolation domain, eq_ind.rs:664-668, math/src/univariate.rs:60-99): the zerocheck of a constraint set -- ONE composition per
 * constraint over ALL multilinears of the table (core/src/constraint_system/prove.rs:431-505).
 *   d_multilins[n_mls]: 2^n_vars elements each, FOLDED IN PLACE;  steps / steps_inf: the compositions and their leading forms
 *   (ArithCircuit::leading_term), concatenated, n_steps[c] / n_steps_inf[c] steps each;  sums[n_comps]: the claimed sums
 *   eq_ind_challenges[n_vars];  d_eq_ind: >= 2^(n_vars - 1) elements of scratch (the indicator's partial evaluations)
 *   round_coeffs_out[(D + 2) * n_vars], D = max(2, largest degree): the batched round polynomials (degree D + 1; the tables'
 *   constraints: D = 2, four coefficients per round);  final_evals_out[n_mls + 1]: the multilinears'
 *   evaluations at the challenges, then the indicator's prefix evaluation (eq_ind.rs:639-643) */
int bnh_eqind_sumcheck_prove(bn_ctx *ctx, uint32_t n_vars, uint32_t n_mls, void *const *d_multilins, uint32_t n_comps, const bn_step *steps,
                             const uint32_t *n_steps, const bn_step *steps_inf, const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *sums,
                             const bn_f128 *eq_ind_challenges, void *d_eq_ind, uint64_t eq_ind_elems, const bn_f128 *batch_coeff, const bn_f128 *challenges,
                             bn_f128 *round_coeffs_out, bn_f128 *final_evals_out);

/* The batched univariate-skip zerocheck prover, sumcheck::prove::batch_zerocheck::batch_prove (crates/core/src/protocols/sumcheck/prove/
 * batch_zerocheck.rs:166-293) over ZerocheckProverImpl (prove/zerocheck.rs:121-516), for the domain field B8 (the 0..=3 arm of core/src/
 * constraint_system/prove.rs:484), through the C++ mirror binius_amd/host/zerocheck.hpp.  The transcript's samples are handed in.
 *   n_tables provers (tables) in ascending n_vars[p]; k = skip_rounds, 1 <= k <= 8, k <= the largest n_vars (= max_n)
 *   d_cols / tower_levels: the tables' columns, concatenated, n_cols[p] each: device, TRANSPARENT (packed as bn_hal_multilinear says), level 0
 *     or 3; only read.  A table of n_vars < k is padded high by repetition to k variables on the host (prove/zerocheck.rs:79-119)
 *   steps / steps_inf / n_steps / n_steps_inf / degrees: the tables' compositions, concatenated, n_comps[p] each, as bnh_eqind_sumcheck_prove
 *     takes them.  The constants lie in B8: the same steps are the B8 form of the univariate round and the B128 form of the multilinear
 *     rounds.  1 <= degree and degree 2^k <= 256
 *   zerocheck_challenges[max_n - k] (table p takes the suffix of length max(n_p, k) - k, constraint_system/prove.rs:470), batch_coeffs[n_tables]
 *     (pre-sampled, batch_zerocheck.rs:198-206; front_loaded::BatchProver::new_prebatched), univariate_challenge, sumcheck_challenges[max_n - k],
 *     reduction_batch_coeff, reduction_challenges[k]
 *   d_scratch: at least bnh_zerocheck_batch_scratch_elems(n_tables, k, n_vars, n_cols) elements of device memory
 * Steps: per table one bn_zerocheck_univariate_evals; the Lagrange coefficients and the claimed sums on the host (prove/univariate.rs:139-193);
 * ONE bn_univariate_fold_batch over the columns of all tables; one EqIndSumcheckProver per table over max(n, k) - k variables, all started in
 * round 0 (a table without remaining rounds finishes at once); ONE bn_partial_eval_high_batch per table for project_to_skipped_variables
 * (prove/zerocheck.rs:472-516); the univariatizing reduction (batch_zerocheck.rs:115-154) as host arithmetic.
 * Outputs, in the transcript's writing order:
 *   message_out[D - 2^k], D = (largest degree of the batch) 2^k: the univariate round's message (may be NULL when D = 2^k)
 *   round_coeffs_out[(max_n - k) (Dmax + 2)], Dmax = max(2, largest degree of the batch): the round polynomials of the multilinear rounds with
 *     ALL their coefficients (the transcript carries the truncated form), padded to the widest degree of the batch as
 *     bnh_eqind_sumcheck_prove pads
 *   final_evals_out[sum (n_cols[p] + 1)]: per table in finishing (= input) order its columns' evaluations, then the indicator's
 *   reduction_round_coeffs_out[3 k], reduction_final_evals_out[sum n_cols + 1]: every column's evaluation, then the Lagrange multilinear's
 *   skipped_challenges_out[k], unskipped_challenges_out[max_n - k], concat_multilinear_evals_out[sum n_cols]: BatchZerocheckOutput
 *     (zerocheck.rs:140-150), what the evalcheck phase starts from
 *   phase_ms_out[5] / phase_calls_out[5] (or NULL): wall time and device-op calls of the univariate round, the fold, the multilinear rounds
 *     (time only), the projection, the reduction (host only)
 * Claims out of order, k > max_n, a level other than 0 or 3, a degree out of range and a short scratch are BN_ERR_INPUT_VALIDATION before
 * anything is launched. */
uint64_t bnh_zerocheck_batch_scratch_elems(uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols);
int bnh_zerocheck_batch_prove(bn_ctx *ctx, uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const void *const *d_cols,
                              const uint32_t *tower_levels, const uint32_t *n_comps, const bn_step *steps, const uint32_t *n_steps, const bn_step *steps_inf,
                              const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *zerocheck_challenges, const bn_f128 *batch_coeffs,
                              const bn_f128 *univariate_challenge, const bn_f128 *sumcheck_challenges, const bn_f128 *reduction_batch_coeff,
                              const bn_f128 *reduction_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *message_out, bn_f128 *round_coeffs_out,
                              bn_f128 *final_evals_out, bn_f128 *reduction_round_coeffs_out, bn_f128 *reduction_final_evals_out, bn_f128 *skipped_challenges_out,
                              bn_f128 *unskipped_challenges_out, bn_f128 *concat_multilinear_evals_out, double *phase_ms_out, uint64_t *phase_calls_out);
/* The same prover for every arm of core/src/constraint_system/prove.rs:483-490 (0..=3 => B8, 4 => B16, 5 => B32, 6 => B64, 7 => B128), with
 * the argument list of bnh_zerocheck_batch_prove.  tower_levels: 0 or 3 .. 7 (little-endian values of 2^(level - 3) bytes); the constants of
 * the compositions anywhere in B128.  A table's arm is the largest of its column levels and of the levels of its compositions' constants,
 * at least 3 (:458-467): its univariate round is bn_zerocheck_univariate_evals at 3 and bn_zerocheck_univariate_evals_base above.  The
 * columns of level 0 / 3 of ALL tables stay in the ONE bn_univariate_fold_batch; a wider column takes one bn_fold_right with the 2^k
 * Lagrange coefficients (uploaded once per proof), which phase_calls_out[1] counts beside the batched call.  The projection is the one
 * bn_partial_eval_high_batch per table.  Padding (n_vars < k) and the columns of less than one 16-byte element are done on the host at
 * every level.
 *   d_scratch: at least bnh_zerocheck_batch_scratch_elems_tower(n_tables, k, n_vars, n_cols, tower_levels) elements: the formula above with
 *   column_elems(k, level) = max(1, 2^(k + level - 7)) elements per padded column (a level-7 column at k = 7: 128) and 2^k elements of
 *   coefficients when some column lies above level 3.  0: an argument out of range.
 * bnh_zerocheck_batch_prove and its scratch formula are unchanged: it still rejects level 4. */
uint64_t bnh_zerocheck_batch_scratch_elems_tower(uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const uint32_t *tower_levels);
int bnh_zerocheck_batch_prove_tower(bn_ctx *ctx, uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const void *const *d_cols,
                                    const uint32_t *tower_levels, const uint32_t *n_comps, const bn_step *steps, const uint32_t *n_steps, const bn_step *steps_inf,
                                    const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *zerocheck_challenges, const bn_f128 *batch_coeffs,
                                    const bn_f128 *univariate_challenge, const bn_f128 *sumcheck_challenges, const bn_f128 *reduction_batch_coeff,
                                    const bn_f128 *reduction_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *message_out, bn_f128 *round_coeffs_out,
                                    bn_f128 *final_evals_out, bn_f128 *reduction_round_coeffs_out, bn_f128 *reduction_final_evals_out, bn_f128 *skipped_challenges_out,
                                    bn_f128 *unskipped_challenges_out, bn_f128 *concat_multilinear_evals_out, double *phase_ms_out, uint64_t *phase_calls_out);

/* gkr_gpa::batch_prove (crates/core/src/protocols/gkr_gpa/prove.rs:33-296) through the C++ mirror binius_amd/host/gkr_gpa.hpp: the GKR
 * grand-product argument over n_claims witnesses, which the constraint system runs for every flush and non-zero oracle
 * (core/src/constraint_system/prove.rs:285-412), High-to-Low.  The witnesses' layers come from ONE bn_product_tree_layers; step
 * j = 0, 1, ... first lets the claims with n_vars = j leave, then runs one EqIndSumcheckProver over j variables for the others as a
 * front-loaded batch of one prover.
 *   n_vars[t] in 0 .. 28; d_inputs[t]: input_lens[t] <= 2^n_vars[t] elements, only read (the absent tail counts as ONE)
 *   d_arenas[t]: 2^n_vars[t] elements, the tree's layers in heap order -- CONSUMED by the sumchecks (NULL allowed for n_vars = 0)
 *   d_scratch: at least sum_{n_vars[t] >= 1} 2^n_vars[t] + 2^(max n_vars - 1) elements: the ONE-padded copies of the inputs that each
 *     tree's last step folds, and the indicator's table
 *   batch_coeffs[max n_vars]: one per step (step 0 has no rounds: its coefficient is sampled and unused)
 *   sumcheck_challenges: step j's j challenges, steps concatenated (max (max - 1) / 2);  gpa_challenges[max n_vars]
 *   products_out[n_claims];  round_proofs_out: 3 coefficients per round, steps concatenated;
 *   layer_evals_out: per step the 2 * active evaluations (claims in the sorted order: n_vars descending, stable) then the
 *     indicator's prefix evaluation
 *   final_points_out: claim t's evaluation point (n_vars[t] coordinates), claims concatenated in the callers' order -- a claim that
 *     leaves at step j has the point of step j - 1 (its reversed challenges, then its layer challenge), which is NOT a prefix of a
 *     longer claim's point, so every claim gets its own
 *   final_evals_out[n_claims]: the callers' order (unsort, prove.rs:140);  step_ms_out[max n_vars]: wall time per step, or NULL */
int bnh_gkr_gpa_prove(bn_ctx *ctx, uint32_t n_claims, const uint32_t *n_vars, const void *const *d_inputs, const uint64_t *input_lens, void *const *d_arenas,
                      void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *sumcheck_challenges, const bn_f128 *gpa_challenges,
                      bn_f128 *products_out, bn_f128 *round_proofs_out, bn_f128 *layer_evals_out, bn_f128 *final_points_out, bn_f128 *final_evals_out,
                      double *step_ms_out);

/* gkr_exp::batch_prove (crates/core/src/protocols/gkr_exp/batch_prove.rs:46-315; provers.rs:20-385, compositions.rs:43-61, utils.rs:5-10)
 * through the C++ mirror binius_amd/host/gkr_exp.hpp: the GKR exponentiation argument over n_claims claims, which the constraint system runs
 * for every Exp of its tables (core/src/constraint_system/prove.rs:236-274), High-to-Low.  The witnesses' layers come from ONE
 * bn_exp_circuit_layers, made here.  Layer L = 0 .. max width - 1 groups the consecutive active provers with equal evaluation points
 * (batch_prove.rs:123-196), runs one EqIndSumcheckProver per group that has a claim, batched by sumcheck::batch_prove
 * (prove/batch_sumcheck.rs:102-199), emits the LayerClaims (batch_prove.rs:254-291) and retires the provers whose last layer it was (:112).
 *   n_witnesses must equal n_claims (MismatchedWitnessClaimLength, :63-65); the claims sorted by n_vars descending (ClaimsOutOfOrder, :73-76)
 *   widths / kinds / d_exponent_bits / static_bases / d_bases: as bn_exp_circuit_layers takes them; all only read
 *   d_arenas[t]: widths[t] * 2^n_vars[t] elements -- filled, then CONSUMED by the sumchecks
 *   eval_points: claim t's n_vars[t] coordinates, claims concatenated;  evals[n_claims]: the claimed evaluations of the result layers
 *   d_scratch: at least sum_t ((kind_t dynamic ? 2 : 1) * 2^n_vars[t] + (n_vars[t] >= 1 ? 2^(n_vars[t] - 1) : 0)) elements: per layer the
 *     bit columns as B128 multilinears, the copies of the dynamic bases, the indicators' tables (reused layer by layer)
 *   batch_coeffs[max_width * n_claims]: [L * n_claims + g] = the coefficient of the g-th sumcheck prover of layer L (the groups that yield
 *     a prover, in order; other slots ignored);  challenges[max_width * max_n_vars]: [L * max_n_vars + r] = round r of layer L
 * Outputs (counts explicit; M = max_width, N = max(1, max_n_vars), K = n_claims):
 *   *n_layers_out = M;  rounds_per_layer_out[M];  coeffs_per_round_out[M * N]: [L * N + r] = coefficients of round r of layer L (3, or 5
 *     once a dynamic prover below its last layer is active);  round_proofs_out[<= 5 * M * N]: the coefficients, rounds and layers concatenated
 *   provers_per_layer_out[M] (0: the layer had no sumcheck);  evals_per_prover_out[M * K]: [L * K + g];  multilinear_evals_out[<= 4 * M * K]: as
 *     written to the transcript, the indicator's evaluation last in every prover's list
 *   claims_per_layer_out[M];  claim_n_vars_out[M * 2 * K]: [L * 2 * K + i] = coordinates of claim i of layer L;  claim_points_out
 *     [<= 2 * M * K * N] and claim_evals_out[<= 2 * M * K]: concatenated, in the reference's order (per prover the bit claim, then for a
 *     dynamic base the base claim)
 *   layer_ms_out[M]: wall time per layer, or NULL */
int bnh_gkr_exp_prove(bn_ctx *ctx, uint32_t n_witnesses, const uint32_t *widths, const uint32_t *kinds, const void *const *d_exponent_bits,
                      const bn_f128 *static_bases, const void *const *d_bases, void *const *d_arenas, uint32_t n_claims, const uint32_t *n_vars,
                      const bn_f128 *eval_points, const bn_f128 *evals, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs,
                      const bn_f128 *challenges, uint32_t *n_layers_out, uint32_t *rounds_per_layer_out, uint32_t *coeffs_per_round_out,
                      bn_f128 *round_proofs_out, uint32_t *provers_per_layer_out, uint32_t *evals_per_prover_out, bn_f128 *multilinear_evals_out,
                      uint32_t *claims_per_layer_out, uint32_t *claim_n_vars_out, bn_f128 *claim_points_out, bn_f128 *claim_evals_out, double *layer_ms_out);

/* The product-check phase of the constraint-system prover (core/src/constraint_system/prove.rs:276-428) through the C++ mirror
 * binius_amd/host/flush.hpp: the flush witnesses made on the device by ONE bn_flush_witness_batch (make_masked_flush_witnesses, :671-881),
 * the non-zero columns widened by ONE bn_partial_eval_high_batch at query_vars = 0, gkr_gpa::batch_prove over chain(flush witnesses with their
 * prefix lengths, non-zero witnesses) (:386-400, as bnh_gkr_gpa_prove runs it), and reduce_flush_evalcheck_claims (:1017-1117): the claim on a
 * flush without selectors (a linear combination) is passed through; the claims on the others (composite oracles 1 + S * L,
 * constraint_system/verify.rs:519-571) are grouped by equal evaluation point in order of first appearance -- flushes of equal n_vars leave the
 * grand-product argument with the same point --, and per group ONE EqIndSumcheckProver runs at that point over the sorted, de-duplicated
 * union of the group's oracle ids (oracle/constraint.rs:114-129) as a front-loaded batch of one (evalcheck/subclaims.rs:589-633).
 *   Flushes in the caller's order (sorted by channel, :333).  Per flush f: channel_ids[f] < n_channels, flush_n_vars[f] in 0 .. 28,
 *     n_selectors[f] in 0 .. 7, n_entries[f].  selector_ids / d_selectors: the selectors (caller's oracle id, packed B1 column), flushes
 *     concatenated.  entry_kinds / entry_ids / d_entry_columns / entry_levels / entry_consts: the entries in order, flushes concatenated:
 *     BNH_FLUSH_ORACLE (id, column of tower level 0 or 3 .. 7 packed into F) or BNH_FLUSH_CONST (base = entry_consts[i]; the rest ignored).
 *     Entry k of a flush carries the mixing power alpha^k whatever its kind (:744-771).  A flush needs an ORACLE entry (EmptyFlushOracles);
 *     a composite flush reads at most 16 distinct oracles.  Equal ids must name equal columns.
 *   Non-zero oracles: nonzero_ids / d_nonzero_columns / nonzero_levels / nonzero_n_vars.  A zero product among them is the reference's
 *     Error::Zeros (:311-316): BN_ERR_INPUT_VALIDATION with a bnh_last_error text that starts with "Zeros", before any flush work runs.
 *   mixing_challenge; permutation_challenges[n_channels].
 *   d_scratch: at least flush_prodcheck_scratch_elems elements = 1 + sum over all witnesses of 2^n_vars (+ 2^n_vars more for n_vars >= 1: the
 *     arena) + the grand-product prover's scratch (bnh_gkr_gpa_prove) + the largest m * 2^n + 2^(n - 1) over the groups (m multilinears).
 *   gpa_batch_coeffs / gpa_sumcheck_challenges / gpa_challenges: as bnh_gkr_gpa_prove takes them, N = the largest n_vars of all witnesses.
 *   red_batch_coeffs[g], red_challenges: per group one batch coefficient and its n_vars challenges, groups concatenated.
 * Outputs: prefix_lens_out[n_flushes]; products_out / gpa_final_evals_out [n_flushes + n_nonzero] and gpa_round_proofs_out /
 *   gpa_layer_evals_out / gpa_final_points_out as bnh_gkr_gpa_prove lays them out, claims in the order flushes, non-zero oracles.
 *   *n_checks_out groups; check_desc_out[3 g ..] = (n_vars, multilinears m, coefficients per round: max(2, largest n_selectors + 1) + 1);
 *   check_ids_out: each group's m ids; check_round_proofs_out: its n_vars rounds of truncated coefficients; check_final_evals_out: its m
 *   evaluations then the indicator's -- all groups concatenated.  The new claim on id i of a group is (id, the group's challenges reversed,
 *   its evaluation); the indicator's evaluation is written and dropped (subclaims.rs:619-630).
 *   *n_linear_out, linear_flushes_out: the flushes whose claims (their gpa final point and evaluation) pass through unchanged.
 *   phase_ms_out[4]: witnesses, grand-product argument, reductions, total (wall time), or NULL.
 * The caller's columns are only read. */
enum { BNH_FLUSH_ORACLE = 0, BNH_FLUSH_CONST = 1 };
int bnh_flush_prodcheck_prove(bn_ctx *ctx, uint32_t n_flushes, const uint32_t *channel_ids, const uint32_t *flush_n_vars, const uint32_t *n_selectors,
                              const uint32_t *selector_ids, const void *const *d_selectors, const uint32_t *n_entries, const uint32_t *entry_kinds,
                              const uint32_t *entry_ids, const void *const *d_entry_columns, const uint32_t *entry_levels, const bn_f128 *entry_consts,
                              uint32_t n_nonzero, const uint32_t *nonzero_ids, const void *const *d_nonzero_columns, const uint32_t *nonzero_levels,
                              const uint32_t *nonzero_n_vars, const bn_f128 *mixing_challenge, const bn_f128 *permutation_challenges, uint32_t n_channels,
                              void *d_scratch, uint64_t scratch_elems, const bn_f128 *gpa_batch_coeffs, const bn_f128 *gpa_sumcheck_challenges,
                              const bn_f128 *gpa_challenges, const bn_f128 *red_batch_coeffs, const bn_f128 *red_challenges, uint64_t *prefix_lens_out,
                              bn_f128 *products_out, bn_f128 *gpa_round_proofs_out, bn_f128 *gpa_layer_evals_out, bn_f128 *gpa_final_points_out,
                              bn_f128 *gpa_final_evals_out, uint32_t *n_checks_out, uint32_t *check_desc_out, uint32_t *check_ids_out,
                              bn_f128 *check_round_proofs_out, bn_f128 *check_final_evals_out, uint32_t *n_linear_out, uint32_t *linear_flushes_out,
                              double *phase_ms_out);

/* One round of evalcheck's bivariate sumchecks: one call of prove_bivariate_sumchecks_with_switchover (core/src/protocols/evalcheck/
 * subclaims.rs:549-586) with the witness construction in front of it (process_shifted_sumcheck, process_packed_sumcheck :52-145,
 * collect_projected_mles :356-439) through the C++ mirror binius_amd/host/evalcheck.hpp.  The caller hands in explicit multilinear lists;
 * the greedy loop and EvalcheckProver's oracle bookkeeping stay with it.
 *   prover_desc[3 * i] = (b, m, n_claims) of prover i, ascending by its number of variables b <= 12; its m multilinears in the order its
 *     constraint set holds them (= the order of its final evaluations in the transcript)
 *   ml_desc[BNH_EC_DESC_WORDS * j], multilinears of prover 0, then of prover 1, ...:
 *     BNH_EC_PROJECTION : (kind, tower_level, n_vars, suffix_off, suffix_len) -- the inner column d_columns[j] (2^n_vars values packed into F,
 *       only read, n_vars = b + suffix_len) evaluated at the high coordinates point_pool[suffix_off .. + suffix_len): evaluate_partial_high.
 *       Distinct suffixes (slices of the pool) are tensor-expanded once each, all projections of one suffix are ONE
 *       bn_partial_eval_high_batch, identical (column, suffix) pairs are projected once; an empty suffix is the column widened to B128
 *     BNH_EC_SHIFT_IND  : (kind, block_size, shift_offset, variant, r_off, r_len) -- ShiftIndPartialEval::multilinear_extension (transparent/
 *       shift_ind.rs:117-161, 276-366) at the prefix point_pool[r_off .. + r_len): table[x] = eq(r)[y(x)], y = x + o mod 2^b (circular left),
 *       x + o or zero outside the block (logical left), x - o or zero when negative (logical right); block_size = r_len = b,
 *       0 < shift_offset < 2^b (assert_valid_shift_ind_args, :218-235)
 *     BNH_EC_TOWER_BASIS: (kind, k, iota) -- table[i] = TowerField::basis(iota, i) (transparent/tower_basis.rs:54-70), k = b, iota + k <= 7
 *     d_columns[j] is ignored for the transparent kinds
 *   comp_indices / sums: per prover its claims as index pairs into its multilinears with their sums, concatenated
 *   d_scratch: at least the sum of 2^|suffix| per distinct suffix, 2^b per distinct (column, suffix) and per transparent multilinear, and
 *     m * 2^(b-1) per prover (EvalcheckPlan.scratch_elems / evalcheck_scratch_elems)
 *   batch_coeffs[n_provers], challenges[max b]: the transcript's samples, as for bnh_batch_sumcheck_prove
 * Outputs, as for bnh_batch_sumcheck_prove: round_proofs_out[2 * max b] the truncated round polynomials; final_evals_out: the provers'
 * final evaluations concatenated in finishing (= input) order.  A PROJECTION's final evaluation v is the evaluation of its table at the
 * reversed challenges r' (r'[i] = the challenge of round b - 1 - i): the new evalcheck claim (r' || suffix, v) on the inner column.
 * The caller's columns are only read. */
enum { BNH_EC_PROJECTION = 0, BNH_EC_SHIFT_IND = 1, BNH_EC_TOWER_BASIS = 2, BNH_EC_LINCOMB = 3 };
enum { BNH_SHIFT_CIRCULAR_LEFT = 0, BNH_SHIFT_LOGICAL_LEFT = 1, BNH_SHIFT_LOGICAL_RIGHT = 2 };
#define BNH_EC_DESC_WORDS 6
int bnh_evalcheck_bivariate_prove(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const uint32_t *ml_desc, const void *const *d_columns,
                                  const bn_f128 *point_pool, uint32_t pool_len, const uint32_t *comp_indices, const bn_f128 *sums, void *d_scratch,
                                  uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *challenges, bn_f128 *round_proofs_out,
                                  bn_f128 *final_evals_out);
/* The same round with inner columns that are LINEAR COMBINATIONS of columns (try_build_partial_eval, evalcheck/subclaims.rs:305-346; keccak's
 * c[x] under its shift): bnh_evalcheck_bivariate_prove's arguments and one more kind, which bnh_evalcheck_bivariate_prove rejects,
 *     BNH_EC_LINCOMB    : (kind, n_vars, suffix_off, suffix_len, first_term, n_terms) -- ml_offsets[j] + the sum over the terms
 *       [first_term, first_term + n_terms) of term_coeffs[t] * the column d_term_columns[t] (2^n_vars values of tower level term_levels[t],
 *       packed into F, only read), n_vars = b + suffix_len, projected at point_pool[suffix_off .. + suffix_len) from its constituents: the
 *       combination is never materialised.  Nested combinations are flattened by the caller (coefficients multiplied through).
 *   term_levels / d_term_columns / term_coeffs: the n_terms terms of the call; ml_offsets: one offset per multilinear, read for kind 3 only
 *     (all four may be null when no multilinear is of kind 3); d_columns[j] is ignored for kind 3
 * All BNH_EC_LINCOMB multilinears of one distinct suffix are ONE bn_partial_eval_high_lincomb_batch, beside the one
 * bn_partial_eval_high_batch of that suffix's plain projections; the suffix expansion is shared; an identical (term range, offset, suffix) is
 * projected once and counts 2^b elements of scratch once.  A call without kind 3 makes exactly bnh_evalcheck_bivariate_prove's calls.  A
 * BNH_EC_LINCOMB's final evaluation v is the new evalcheck claim (r' || suffix, v) on the linear-combination oracle itself. */
int bnh_evalcheck_bivariate_prove_lc(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const uint32_t *ml_desc, const void *const *d_columns,
                                     uint32_t n_terms, const uint32_t *term_levels, const void *const *d_term_columns, const bn_f128 *term_coeffs,
                                     const bn_f128 *ml_offsets, const bn_f128 *point_pool, uint32_t pool_len, const uint32_t *comp_indices, const bn_f128 *sums,
                                     void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *challenges, bn_f128 *round_proofs_out,
                                     bn_f128 *final_evals_out);

/* The evaluations in front of every evalcheck round: EvalcheckProver::prove evaluates the materialised witness of every leaf oracle whose
 * value is not yet known at its whole claim point ("MLE Fold Full", core/src/protocols/evalcheck/prove.rs:191-275, make_new_eval_claim
 * :812-879: evaluate_partial_high at the suffix of the point, then evaluate at its prefix) through the C++ mirror binius_amd/host/
 * evalcheck.hpp (evalcheck_evaluate_claims).  Which oracles are leaves and which values are known (collect_subclaims_for_memoization,
 * :350-467) stays with the caller.
 *   claim_desc[4 * i] = (tower_level, n_vars, point_off, point_len): claim i is the column d_columns[i] (2^n_vars values of tower level 0 or
 *     3..7 packed into F as bn_mle_evaluate_batch takes them, only read) at the point point_pool[point_off .. + point_len), point_len == n_vars
 * Every point is split at lo = min(point_len / 2, BNH_EVALCHECK_LO_SPLIT); every distinct prefix slice [off, off + lo) and every distinct
 * suffix slice [off + lo, off + len) of the pool is tensor-expanded once (memoize_query_par, evalcheck/subclaims.rs:489-508); a repeated
 * (column, level, point) is evaluated once (visited_claims); ONE bn_mle_evaluate_batch serves everything; evals_out[i] is the value of
 * claim i.  The arithmetic is exact, so the values do not depend on the split: the mirror reproduces neither the reference's middle
 * split nor its reuse of an already memoised suffix (prove.rs:211-221).
 *   d_scratch: at least bnh_evalcheck_evaluate_scratch_elems elements (the formula is exact): 2^len per distinct prefix slice and per
 *     distinct suffix slice.  lo_split: the bound of the split to plan for, at most BN_ME_MAX_LO_VARS; 0 = BNH_EVALCHECK_LO_SPLIT, the one
 *     bnh_evalcheck_evaluate uses.  Returns 0 for a null list or a lo_split out of range.
 * A short scratch, point_len != n_vars, a slice outside the pool and a tower level of 1 or 2 are BN_ERR_INPUT_VALIDATION before anything is
 * launched.  phase_ms_out[2] (may be null): wall milliseconds of the expansions and of the evaluation call. */
#define BNH_EVALCHECK_LO_SPLIT 8
uint64_t bnh_evalcheck_evaluate_scratch_elems(uint32_t n_claims, const uint32_t *claim_desc, uint32_t lo_split);
int bnh_evalcheck_evaluate(bn_ctx *ctx, uint32_t n_claims, const uint32_t *claim_desc, const void *const *d_columns, const bn_f128 *point_pool,
                           uint32_t pool_len, void *d_scratch, uint64_t scratch_elems, bn_f128 *evals_out, double *phase_ms_out);

/* The ring-switching reduction: ring_switch::prove (core/src/ring_switch/prove.rs:42-144) through the C++ mirror binius_amd/host/
 * ring_switch.hpp.  The caller has done the oracle-set bookkeeping of EvalClaimSystem::new (ring_switch/common.rs:72-205).
 *   d_columns[c], column_desc[2 * c] = (tower_level, n_vars): the committed columns, 2^n_vars values packed into F as bn_partial_eval_high_batch
 *     takes them (n_vars + tower_level >= 7), only read
 *   point_pool / suffix_desc[3 * s] = (off, len, kappa): the suffix descriptors, suffix s = point_pool[off .. off + len)
 *   prefix_kappas[p]: kappa of prefix descriptor p
 *   claim_desc[3 * i] = (committed_idx, suffix_desc_idx, prefix_desc_idx), in the order the reference sorts the claims; kappa of the
 *     suffix = 7 - tower_level of the column = kappa of the prefix (else the reference's TowerLevelMismatch), len = n_vars - kappa
 *   mixing_challenges[ceil(log2 n_claims)], row_batch_challenges[max kappa]: the transcript's two sample_vec calls (prove.rs:68-69, 97)
 *   d_scratch: at least bnh_ring_switch_scratch_elems elements (the formula is exact): 2^len per distinct suffix (slice of the pool), 2^kappa per distinct
 *     (column, suffix), 2^len per claim
 * Distinct suffixes are tensor-expanded once each; the partial evaluations of the distinct columns of one suffix are ONE
 * bn_partial_eval_high_batch and one copy to the host; scaling, mixing per prefix and the row-batched evaluations run on the host; the
 * transparents of ALL claims are ONE bn_ring_switch_eq_ind_batch over the same suffix tables.
 * Outputs, in transcript order: mixed_tensor_elems_out -- per prefix its 2^kappa vertical elements, concatenated (prove.rs:90-94);
 * row_batched_evals_out[n_claims] (prove.rs:104).  d_transparents_out[i]: the transparent of claim i (2^len elements inside d_scratch);
 * the PIOP sumcheck claim of claim i is (n_vars = len, committed_idx, transparent = i, sum = row_batched_evals_out[i]) (prove.rs:127-138).
 * phase_ms_out[3] (may be null): wall milliseconds of partial_evals, tensor_algebra, eq_inds. */
uint64_t bnh_ring_switch_scratch_elems(uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_claims, const uint32_t *claim_desc);
int bnh_ring_switch_prove(bn_ctx *ctx, uint32_t n_columns, const void *const *d_columns, const uint32_t *column_desc, const bn_f128 *point_pool, uint32_t pool_len,
                          uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_prefixes, const uint32_t *prefix_kappas, uint32_t n_claims,
                          const uint32_t *claim_desc, const bn_f128 *mixing_challenges, uint32_t n_mixing_challenges, const bn_f128 *row_batch_challenges,
                          uint32_t n_row_batch_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *mixed_tensor_elems_out, bn_f128 *row_batched_evals_out,
                          void **d_transparents_out, double *phase_ms_out);

/* ---- Against a live transcript ------------------------------------------------------------------------------------------------------
 * Every entry point above takes the transcript's samples as arrays, drawn before the call.  In a proof, round r's challenge is a hash
 * of round r's message, so a prover with a Fiat-Shamir transcript drives the `_live` forms below instead: the library hands each
 * message to the caller at the moment the reference writes it and asks the caller for each sample at the moment the reference draws
 * it.  The transcript itself stays with the caller (ProverTranscript<Challenger>, crates/core/src/transcript/mod.rs).
 *   write        TranscriptWriter: channel BNH_TR_MESSAGE is transcript.message() (observed by the challenger), BNH_TR_DECOMMITMENT is
 *                transcript.decommitment() (not observed).  `bytes` are in transcript byte order: a scalar is its 16-byte little-endian
 *                canonical-tower element (the layout of bn_f128), a digest its 32 bytes.  Only the concatenation of the bytes between
 *                two samples is specified, not how it is cut into calls.
 *   sample       n x transcript.sample() of B128, in order, into out[n]
 *   sample_bits  n x transcript.sample_bits(bits), in order, into out[n]
 * A callback returns 0, or non-zero to end the proof: the call returns BN_ERR_CALLBACK after the unwinding that any error inside a
 * mirror takes, and the context stays usable.  Callbacks run on the calling thread, inside the call; they MUST NOT re-enter the
 * library on the same context.  A null table, or a null member that the entry point needs (write and sample always; sample_bits
 * where indices are drawn), is BN_ERR_INPUT_VALIDATION before anything is launched.
 * A `_live` form keeps its array form's argument list but for the sample arrays, which go, and the `const bnh_transcript *`, which
 * stands where the first of them stood.  The output arrays stay: a `_live` call that drew the samples S fills every output array
 * exactly as the array form fed S (both run the same mirror code over a TranscriptSource, binius_amd/host/transcript.hpp).  Work
 * computed ahead (armed kernels, the first execute() carrying other provers' claims, the host tail) depends only on past challenges
 * and is untouched. */
enum { BNH_TR_MESSAGE = 0, BNH_TR_DECOMMITMENT = 1 }; /* TranscriptWriter: message() is observed, decommitment() is not */
typedef struct bnh_transcript {
	void *user;
	int (*write)(void *user, uint32_t channel, const void *bytes, uint64_t len);  /* transcript byte order */
	int (*sample)(void *user, bn_f128 *out, uint32_t n);                          /* n x transcript.sample() of B128 */
	int (*sample_bits)(void *user, uint32_t bits, uint32_t n, uint64_t *out);     /* n x sample_bits(bits) */
} bnh_transcript;

/* The schedules.  W(k): k scalars written to BNH_TR_MESSAGE; S(k): k samples drawn; "batch run": front_loaded::BatchProver::run
 * (sumcheck/prove/front_loaded.rs:122-197) -- per round r the final evaluations of every prover whose number of variables is r (m
 * scalars each, :109-120), the TRUNCATED round polynomial (RoundCoeffs::truncate: all coefficients but the last), S(1); after the last
 * round the evaluations of the provers that finish then.
 *
 * bnh_batch_sumcheck_prove_live (front_loaded.rs:51-59, 175-197): S(n_provers) batch coefficients; batch run with W(2) per round.
 * bnh_eqind_sumcheck_prove_live (eq_ind.rs:378-644 as a front-loaded batch of one): S(1) the batch coefficient; n_vars rounds of
 *   W(D + 1), S(1) -- the prover's polynomial TIMES the batch coefficient, without its last coefficient (front_loaded.rs:128-135),
 *   while round_coeffs_out keeps the prover's own D + 2 coefficients; W(n_mls + 1).
 * bnh_zerocheck_batch_prove_tower_live (constraint_system/prove.rs:470; batch_zerocheck.rs:193-272), the superset of the B8 form:
 *   S(max_n - k) zerocheck challenges; S(n_tables) batch coefficients; W(D - 2^k) the univariate round's message; S(1) the univariate
 *   challenge; batch run over the tables with max(n_p, k) - k variables each, the round polynomial truncated to the live tables'
 *   largest degree + 1 coefficients (round_coeffs_out keeps all, padded); S(1) the reduction's batch coefficient; k rounds of W(2),
 *   S(1); W(sum n_cols + 1).
 * bnh_gkr_gpa_prove_live (gkr_gpa/prove.rs:67-126): step j = 0 .. max n_vars - 1: S(1) the batch coefficient; j rounds of W(3), S(1);
 *   W(2 * active + 1) the layer evaluations and the indicator's; S(1) the layer challenge, drawn after them (:113-114).
 * bnh_gkr_exp_prove_live (gkr_exp/batch_prove.rs:101 = sumcheck::batch_prove, prove/batch_sumcheck.rs:138-187): per layer with a
 *   prover: per round first S(1) for every prover that joins in it (:143-151), then W(truncated round polynomial: 3, or 5 once a
 *   degree-4 composition is live -- the eq-ind polynomial of a degree-d composition has d + 2 coefficients, d + 1 are written), S(1); after the last round S(1) per zero-variable prover (:173-177); then every prover's evaluations,
 *   in order.  A layer without a prover writes and draws nothing.
 * bnh_flush_prodcheck_prove_live (constraint_system/prove.rs:309-425): W(n_nonzero) the non-zero products (:318-320); S(1) the mixing
 *   challenge; S(n_channels) the permutation challenges (:329-330) -- these two draws are made even when there is neither a flush nor a
 *   non-zero oracle, and are then all the call does; W(n_flushes) the flush products (:378-380); the schedule of
 *   bnh_gkr_gpa_prove_live over chain(flushes, non-zero oracles); per MLE-check g: S(1), n_vars rounds of W(check_desc_out[3 g + 2]),
 *   S(1), then W(m + 1) (evalcheck/subclaims.rs:589-633).
 * bnh_evalcheck_bivariate_prove_lc_live (evalcheck/subclaims.rs:549-586), the superset of bnh_evalcheck_bivariate_prove: S(n_provers);
 *   batch run with W(2) per round.
 * bnh_ring_switch_prove_live (ring_switch/prove.rs:68-104): S(ceil(log2 n_claims)) mixing challenges; W(sum over prefixes of 2^kappa)
 *   the mixed tensor elements; S(max kappa) row-batch challenges; W(n_claims) the row-batched evaluations.
 * bnh_fri_prove_live (fri/prove.rs:88-198, 307-432, 483-507): the commitment (32 bytes, MESSAGE); per fold round S(1), then the
 *   round's commitment (32 bytes) when the folder commits in it; the terminate codeword on BNH_TR_DECOMMITMENT; sample_bits(index_bits)
 *   n_test_queries times; the layers and every query's openings on BNH_TR_DECOMMITMENT (the decommitment is not observed, so the
 *   openings of all queries follow the last index; the byte string is the reference's, and equals advice_out).
 * bnh_piop_prove_committed_open_live (piop/prove.rs:306-395): S(provers) batch coefficients; per round: finished provers' evaluations,
 *   W(2) (W(0) in the rounds after the largest prover has finished), S(1), the FRI round's commitment (32 bytes) when there is one -- the item list of bnh_piop_prove in order, up to its
 *   terminate item; then the query phase as in bnh_fri_prove_live.  items_out still ends with the terminate item. */
int bnh_batch_sumcheck_prove_live(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const void *const *d_multilins, const uint32_t *comp_indices,
                                  const bn_f128 *sums, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, bn_f128 *round_proofs_out,
                                  bn_f128 *final_evals_out);
int bnh_eqind_sumcheck_prove_live(bn_ctx *ctx, uint32_t n_vars, uint32_t n_mls, void *const *d_multilins, uint32_t n_comps, const bn_step *steps,
                                  const uint32_t *n_steps, const bn_step *steps_inf, const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *sums,
                                  const bn_f128 *eq_ind_challenges, void *d_eq_ind, uint64_t eq_ind_elems, const bnh_transcript *transcript,
                                  bn_f128 *round_coeffs_out, bn_f128 *final_evals_out);
int bnh_zerocheck_batch_prove_tower_live(bn_ctx *ctx, uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const void *const *d_cols,
                                         const uint32_t *tower_levels, const uint32_t *n_comps, const bn_step *steps, const uint32_t *n_steps, const bn_step *steps_inf,
                                         const uint32_t *n_steps_inf, const uint32_t *degrees, const bnh_transcript *transcript, void *d_scratch, uint64_t scratch_elems,
                                         bn_f128 *message_out, bn_f128 *round_coeffs_out, bn_f128 *final_evals_out, bn_f128 *reduction_round_coeffs_out,
                                         bn_f128 *reduction_final_evals_out, bn_f128 *skipped_challenges_out, bn_f128 *unskipped_challenges_out,
                                         bn_f128 *concat_multilinear_evals_out, double *phase_ms_out, uint64_t *phase_calls_out);
int bnh_gkr_gpa_prove_live(bn_ctx *ctx, uint32_t n_claims, const uint32_t *n_vars, const void *const *d_inputs, const uint64_t *input_lens, void *const *d_arenas,
                           void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, bn_f128 *products_out, bn_f128 *round_proofs_out,
                           bn_f128 *layer_evals_out, bn_f128 *final_points_out, bn_f128 *final_evals_out, double *step_ms_out);
int bnh_gkr_exp_prove_live(bn_ctx *ctx, uint32_t n_witnesses, const uint32_t *widths, const uint32_t *kinds, const void *const *d_exponent_bits,
                           const bn_f128 *static_bases, const void *const *d_bases, void *const *d_arenas, uint32_t n_claims, const uint32_t *n_vars,
                           const bn_f128 *eval_points, const bn_f128 *evals, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript,
                           uint32_t *n_layers_out, uint32_t *rounds_per_layer_out, uint32_t *coeffs_per_round_out, bn_f128 *round_proofs_out,
                           uint32_t *provers_per_layer_out, uint32_t *evals_per_prover_out, bn_f128 *multilinear_evals_out, uint32_t *claims_per_layer_out,
                           uint32_t *claim_n_vars_out, bn_f128 *claim_points_out, bn_f128 *claim_evals_out, double *layer_ms_out);
int bnh_flush_prodcheck_prove_live(bn_ctx *ctx, uint32_t n_flushes, const uint32_t *channel_ids, const uint32_t *flush_n_vars, const uint32_t *n_selectors,
                                   const uint32_t *selector_ids, const void *const *d_selectors, const uint32_t *n_entries, const uint32_t *entry_kinds,
                                   const uint32_t *entry_ids, const void *const *d_entry_columns, const uint32_t *entry_levels, const bn_f128 *entry_consts,
                                   uint32_t n_nonzero, const uint32_t *nonzero_ids, const void *const *d_nonzero_columns, const uint32_t *nonzero_levels,
                                   const uint32_t *nonzero_n_vars, uint32_t n_channels, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript,
                                   uint64_t *prefix_lens_out, bn_f128 *products_out, bn_f128 *gpa_round_proofs_out, bn_f128 *gpa_layer_evals_out,
                                   bn_f128 *gpa_final_points_out, bn_f128 *gpa_final_evals_out, uint32_t *n_checks_out, uint32_t *check_desc_out, uint32_t *check_ids_out,
                                   bn_f128 *check_round_proofs_out, bn_f128 *check_final_evals_out, uint32_t *n_linear_out, uint32_t *linear_flushes_out,
                                   double *phase_ms_out);
int bnh_evalcheck_bivariate_prove_lc_live(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const uint32_t *ml_desc, const void *const *d_columns,
                                          uint32_t n_terms, const uint32_t *term_levels, const void *const *d_term_columns, const bn_f128 *term_coeffs,
                                          const bn_f128 *ml_offsets, const bn_f128 *point_pool, uint32_t pool_len, const uint32_t *comp_indices, const bn_f128 *sums,
                                          void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, bn_f128 *round_proofs_out, bn_f128 *final_evals_out);
int bnh_ring_switch_prove_live(bn_ctx *ctx, uint32_t n_columns, const void *const *d_columns, const uint32_t *column_desc, const bn_f128 *point_pool, uint32_t pool_len,
                               uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_prefixes, const uint32_t *prefix_kappas, uint32_t n_claims,
                               const uint32_t *claim_desc, const bnh_transcript *transcript, void *d_scratch, uint64_t scratch_elems, bn_f128 *mixed_tensor_elems_out,
                               bn_f128 *row_batched_evals_out, void **d_transparents_out, double *phase_ms_out);
int bnh_fri_prove_live(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                       uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, uint8_t *roots_out,
                       bn_f128 *advice_out, uint64_t max_advice_elems, uint64_t *n_advice_elems_out, double *phase_ms_out);
int bnh_piop_prove_committed_open_live(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                                       const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims,
                                       const bn_f128 *claim_sums, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                                       uint32_t n_arities, uint32_t n_test_queries, const void *d_codeword, const void *d_tree, void *d_scratch, uint64_t scratch_elems,
                                       const bnh_transcript *transcript, uint32_t *items_out, uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out,
                                       uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out, uint32_t max_digests, uint32_t *n_digests_out,
                                       double *phase_ms_out, bn_f128 *advice_out, uint64_t max_advice_elems, uint64_t *n_advice_elems_out);

/* The virtual columns of a constraint system derived on the device (binius_amd/host/witness.hpp): the witness-side reading of a
 * MultilinearOracleSet (core/src/oracle/multilinear.rs).  The n_columns columns come in oracle-id order; column i is
 * col_desc[4 i .. 4 i + 4) = (kind, a, b, c), with col_args[i] and lc_offsets[i] (both [n_columns]; 0 where unused):
 *   BNH_WIT_GIVEN        a = tower level, b = n_vars; d_given[i] = the column on the device (d_given[i] of other kinds is not read)
 *   BNH_WIT_SHIFTED      a = inner, b = block_size, c = BN_SHIFT_* variant, col_args[i] = shift_offset        (add_shifted)
 *   BNH_WIT_REPEATING    a = inner, b = log_count                                                             (add_repeating)
 *   BNH_WIT_ZERO_PADDED  a = inner, b = n_pad_vars, c = start_index, col_args[i] = nonzero_index              (add_zero_padded)
 *   BNH_WIT_PACKED       a = inner, b = log_degree                                                            (add_packed)
 *   BNH_WIT_LINCOMB      a = first term, b = number of terms (<= BN_PEL_MAX_TERMS) in lc_terms / lc_coeffs [n_lc_terms], c = n_vars,
 *                        lc_offsets[i] = the offset                                       (add_linear_combination_with_offset)
 * An inner index (and a term) is smaller than the column's own index, as OracleIds are.  Levels follow multilinear.rs:91-266: shifted,
 * repeating and padded columns keep the inner's; packed is inner + log_degree with n_vars - log_degree; a combination has the maximum of
 * its terms' levels and the minimal levels of its coefficients and offset.  How the plan runs:
 *   - Packed is an alias: the inner's pointer, no launch.
 *   - A column's wave is one more than its deepest inner (given: 0; an alias adds nothing).  ONE bn_derive_columns_batch per wave
 *     serves its shifted, repeating and padded columns and the combinations in XOR form (all coefficients ONE, every term at the
 *     combination's level).
 *   - The B128 combinations outside the XOR form share, per wave, ONE bn_partial_eval_high_lincomb_batch at query_vars = 0, its
 *     one-element query ONE in scratch.
 *   - A combination that is neither is BN_ERR_INPUT_VALIDATION.  Projected, transparent and structured polynomials are NOT taken HERE
 *     (bnh_witness_build below takes those that its kinds name), Composite and the other subfield combinations by neither
 *     (bnh_witness_compute further below takes both): list them as given columns.
 *   - Columns of less than one 16-byte element are host work (one element read, one written) and make no launch.
 * d_columns_out / tower_levels_out / n_vars_out [n_columns]: every column's pointer (a given column's own, an alias's inner's, a derived
 * column's place in d_scratch), level and n_vars; *n_waves_out: the largest wave; *n_launches_out: the op calls made (either may be null).
 * bnh_witness_derive_scratch_elems is exact: every derived column at its packed size (one element below 2^7 bits), plus one element
 * when a combination goes to the lincomb op; 0 for a plan that bnh_witness_derive would reject.  Everything is checked before the first
 * device call. */
enum { BNH_WIT_GIVEN = 0, BNH_WIT_SHIFTED = 1, BNH_WIT_REPEATING = 2, BNH_WIT_ZERO_PADDED = 3, BNH_WIT_PACKED = 4, BNH_WIT_LINCOMB = 5 };
uint64_t bnh_witness_derive_scratch_elems(uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const uint32_t *lc_terms, const bn_f128 *lc_coeffs,
                                          uint32_t n_lc_terms, const bn_f128 *lc_offsets);
int bnh_witness_derive(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                       const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                       uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out);

/* bnh_witness_derive with the columns that a few integers, one field element or a 0/1 projection determine generated on the device as
 * well (bn_generate_columns_batch): with it a caller uploads the committed columns and nothing else for the column kinds m3 emits.
 * Arguments, encoding, outputs and the kinds 0 .. 5 are bnh_witness_derive's; lc_offsets[i] also carries a constant's value or a
 * power's base.  The further kinds:
 *   BNH_WIT_PROJECTED_BITS  a = inner, b = start_index, c = query_size, col_args[i] = query_bits: add_projected / add_selected at query
 *                           values ZERO / ONE, bit k of query_bits the k-th; the inner's level, n_vars = inner - query_size
 *   BNH_WIT_CONSTANT        a = tower level, b = n_vars, lc_offsets[i] = the value                              (transparent/constant.rs)
 *   BNH_WIT_STEP_DOWN       a = 0 (the level), b = n_vars, col_args[i] = index <= 2^n_vars                      (step_down.rs)
 *   BNH_WIT_STEP_UP         the same                                                                            (step_up.rs)
 *   BNH_WIT_SELECT_ROW      a = 0, b = n_vars, col_args[i] = index < 2^n_vars                                   (select_row.rs)
 *   BNH_WIT_INCREMENTING    a = tower level, b = n_vars <= 2^level                              (add_structured(Incrementing))
 *   BNH_WIT_POWERS          a = tower level 3 .. 7, b = n_vars, lc_offsets[i] = the base                        (powers.rs)
 * with the bounds of bn_generate_columns_batch.  A generated column without an inner is wave 0, a projection one more than its inner;
 * every wave that has such columns makes ONE bn_generate_columns_batch beside its derive and lincomb calls (wave 0 makes no other
 * call).  Columns below one 16-byte element stay host work (a projection's inner is read back whole).  The scratch formula stays
 * exact: every derived or generated column at its packed size, plus the lincomb op's one element.  bnh_witness_derive itself rejects
 * these kinds as before.  NOT taken: Projected at other query values, general circuit transparents and StructuredFixedSize,
 * TowerBasis, EqIndPartialEval, ShiftIndPartialEval, DisjointProduct: list them as given columns; Composite and subfield combinations
 * outside the XOR form (m3's add_computed): bnh_witness_compute below. */
enum { BNH_WIT_PROJECTED_BITS = 6, BNH_WIT_CONSTANT = 7, BNH_WIT_STEP_DOWN = 8, BNH_WIT_STEP_UP = 9, BNH_WIT_SELECT_ROW = 10, BNH_WIT_INCREMENTING = 11, BNH_WIT_POWERS = 12 };
uint64_t bnh_witness_build_scratch_elems(uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const uint32_t *lc_terms, const bn_f128 *lc_coeffs,
                                         uint32_t n_lc_terms, const bn_f128 *lc_offsets);
int bnh_witness_build(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                      const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                      uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out);

/* bnh_witness_build with the columns of m3's add_computed computed on the device as well (m3/src/builder/constraint_system.rs:515-540),
 * each by ONE bn_compute_composite with a tower-typed expression (bn_expr_compile_tower, include/binius_amd.h): the last kind of witness
 * column that crossed PCIe at column size.  The arguments of bnh_witness_build, then the expressions: expression e is
 * steps[step_off[e] .. step_off[e + 1]) over the columns expr_inputs[expr_input_off[e] .. expr_input_off[e + 1]) (variable v of the steps
 * is the v-th of them); step_off and expr_input_off hold n_exprs + 1 entries.
 *   BNH_WIT_COMPUTED  a = expression index, b = n_vars, c = the column's tower level (0 or 3 .. 7): add_computed -> composite_mle, e.g.
 *                     prod_high[bit] + x_is_negative * (prod_high[bit] + zout[bit]) at B1 (m3/src/gadgets/mul.rs:466-489).  The inputs are
 *                     column indices smaller than the column's own, all of n_vars = b; levels follow bn_expr_compile_tower (no step above c).
 *   BNH_WIT_LINCOMB   widened: the XOR form and the B128 form run as in bnh_witness_derive; every other combination -- pack_fp / pack_b8:
 *                     sum of bit_i * beta_i with B1 terms and coefficients in B8 / B32 / B64 -- becomes the expression sum of coeff * term +
 *                     offset, left-deep, at the reference's level: the maximum of the terms' levels and the minimal levels of coefficients
 *                     and offset.  A level of 1 or 2 cannot be packed: BN_ERR_INPUT_VALIDATION.
 * Such a column's wave is one more than its deepest input's; each is one bn_compute_composite call of its wave, counted in
 * *n_launches_out (bnh_witness_compute_batched below serves a wave in one launch: the counter shows the difference).  Below one 16-byte
 * element it is host work like the other kinds: its inputs' single elements read back, evaluated value by value with bn_scalar_mul, one
 * element written.  bnh_witness_compute_scratch_elems is exact -- every derived, generated or computed column at its packed size, plus the
 * lincomb op's one element -- and 0 for a plan that bnh_witness_compute would reject.  bnh_witness_derive and bnh_witness_build keep
 * rejecting kind 13 and the combinations they rejected. */
enum { BNH_WIT_COMPUTED = 13 };
uint64_t bnh_witness_compute_scratch_elems(uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const uint32_t *lc_terms, const bn_f128 *lc_coeffs,
                                           uint32_t n_lc_terms, const bn_f128 *lc_offsets, const bn_step *steps, const uint32_t *step_off, const uint32_t *expr_inputs,
                                           const uint32_t *expr_input_off, uint32_t n_exprs);
int bnh_witness_compute(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                        const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                        uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out, const bn_step *steps, const uint32_t *step_off,
                        const uint32_t *expr_inputs, const uint32_t *expr_input_off, uint32_t n_exprs);
/* bnh_witness_compute with the expression columns of a wave in ONE launch: per wave every distinct (steps, input levels, output level) is
 * compiled once, one batch is built (bn_expr_compile_tower_batch, include/binius_amd.h) whose arena is the plan's scratch and whose
 * out_offset is each column's place in it, one bn_compute_composite serves it, the handles are freed.  *n_launches_out counts one per
 * wave that has expression columns.  Same parameters, same columns, same bytes, same rejections; bnh_witness_compute_scratch_elems serves
 * both.  Columns below one element stay host work. */
int bnh_witness_compute_batched(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                                const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                                uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out, const bn_step *steps, const uint32_t *step_off,
                                const uint32_t *expr_inputs, const uint32_t *expr_input_off, uint32_t n_exprs);

/* An array-backed transcript, for C callers, benchmarks and tests: it serves samples[n_samples] to `sample` and
 * bit_samples[n_bit_samples] (masked to `bits`) to `sample_bits`, in order, returns non-zero when they run out, and records every
 * write.  Pure host code, no context.
 * bnh_transcript_replay_table: the table to hand to a `_live` entry point; valid until bnh_transcript_replay_free.
 * bnh_transcript_replay_written: the bytes written to `channel` so far, concatenated; *len_out is set even when buf (max bytes) is too
 *   small, which is BN_ERR_INPUT_VALIDATION.
 * bnh_transcript_replay_events: the alternation log.  kinds_out[i] is a BNH_TR_EVENT_*; counts_out[i] its bytes (writes) or its
 *   samples (draws).  Neighbouring events of one kind are one event: the log does not depend on how writes or draws were cut into
 *   calls.  *n_events_out is set even when max_events is too small, which is BN_ERR_INPUT_VALIDATION. */
enum { BNH_TR_EVENT_WRITE_MESSAGE = 0, BNH_TR_EVENT_WRITE_DECOMMITMENT = 1, BNH_TR_EVENT_SAMPLE = 2, BNH_TR_EVENT_SAMPLE_BITS = 3 };
typedef struct bnh_transcript_replay bnh_transcript_replay;
int bnh_transcript_replay_new(const bn_f128 *samples, uint64_t n_samples, const uint64_t *bit_samples, uint64_t n_bit_samples, bnh_transcript_replay **handle_out);
const bnh_transcript *bnh_transcript_replay_table(bnh_transcript_replay *handle);
int bnh_transcript_replay_written(bnh_transcript_replay *handle, uint32_t channel, uint8_t *buf, uint64_t max, uint64_t *len_out);
int bnh_transcript_replay_events(bnh_transcript_replay *handle, uint32_t *kinds_out, uint64_t *counts_out, uint64_t max_events, uint64_t *n_events_out);
void bnh_transcript_replay_free(bnh_transcript_replay *handle);

/* shared-memory exchange: rank 0 creates the segment `name` ("/..."), the others open it afterwards */
int bnh_shm_open(const char *name, int world, int rank, int create, void **handle_out);
int bnh_shm_close(void *handle);
/* every rank contributes n_words (<= 7) 64-bit words; out[world * n_words], rank-major */
int bnh_shm_allgather(void *handle, const uint64_t *in, uint32_t n_words, uint64_t *out);

/* RCCL, bound with dlopen from `librccl_path` (the librccl.so the process already uses) */
int bnh_rccl_open(const char *librccl_path);
int bnh_rccl_unique_id(void *out128);
int bnh_rccl_init(const void *id128, int world, int rank, void **comm_out);
int bnh_rccl_destroy(void *comm);

#ifdef __cplusplus
}
#endif
#endif
