/*
 * binius_amd.h -- C ABI of the MI355X (gfx950) compute backend for the Binius prover hot path.
 *
 * Drop-in boundary: these entry points are what an implementation of the reference's HAL traits
 *   binius_compute::ComputeLayer          crates/compute/src/layer.rs:22
 *   binius_compute::ComputeLayerExecutor  crates/compute/src/layer.rs:100
 *   binius_compute::KernelExecutor        crates/compute/src/layer.rs:518
 *   binius_ntt::AdditiveNTT               crates/ntt/src/additive_ntt.rs:58
 * binds over FFI (INTEGRATION.md shows the Rust `extern "C"` block and the trait impl).
 * Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - F = BinaryField128b = one little-endian u128 = bn_f128 {lo, hi}
 *     (crates/field/src/binary_field.rs:747); element i of a slice is at byte offset 16*i.
 *   - Pointers named d_* are device pointers (16-byte aligned); h_* are host pointers.
 *     All lengths are in field elements unless stated otherwise.
 *   - Every function returns a bn_status.  Non-zero mirrors binius_compute::Error
 *     (crates/compute/src/layer.rs:706-716); bn_last_error() gives the message for the calling
 *     thread.  Precondition violations the reference reports as Error::InputValidation are
 *     reported as BN_ERR_INPUT_VALIDATION with nothing launched.
 *   - Ownership: the caller owns every buffer; the library owns its context (stream, scratch).
 *   - Ordering: work is enqueued on the context's HIP stream in call order, which gives the
 *     store-to-load ordering the executor contract asks for (layer.rs:92-95).  Functions that
 *     return scalars to the host synchronise the stream.
 */
#ifndef BINIUS_AMD_H
#define BINIUS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
	uint64_t lo, hi;
} bn_f128;

typedef enum {
	BN_OK = 0,
	BN_ERR_INPUT_VALIDATION = 1, /* Error::InputValidation */
	BN_ERR_ALLOC = 2,            /* Error::Alloc(OutOfMemory) */
	BN_ERR_DEVICE = 3,           /* Error::DeviceError (hipError_t) */
	BN_ERR_CORE_LIB = 4,         /* Error::CoreLibError */
	BN_ERR_CALLBACK = 5          /* a caller's transcript callback returned non-zero (include/binius_amd_host.h, bnh_transcript) */
} bn_status;

typedef struct bn_ctx bn_ctx;
typedef struct bn_expr bn_expr;

const char *bn_last_error(void);
/* "gfx950" build tag + ABI version, for the loader to check */
const char *bn_version(void);

/* ---- context = ComputeHolder (layer.rs:732-776; FastCpuLayerHolder::new(host, dev),
 *      crates/fast_compute/src/layer.rs:905).  arena_elems may be 0 (caller brings its own device
 *      memory, e.g. a torch allocation); otherwise one arena of arena_elems F is hipMalloc'ed and
 *      the host side bump-allocates from it (crates/compute/src/alloc.rs:31). */
int bn_ctx_create(int device, uint64_t arena_elems, bn_ctx **out);
int bn_ctx_destroy(bn_ctx *ctx);
int bn_arena_base(bn_ctx *ctx, void **d_base, uint64_t *elems);
/* Stream contract.  Work is enqueued on the context's stream in call order, with ONE exception: on the
 * context's OWN stream (the default) bn_extrapolate_line[_batch] and bn_copy_d2d may be deferred to the
 * next bn_* call (which either launches them first or fuses them into its own kernel) -- invisible to
 * every bn_* call, host read-back included.  Anything the caller enqueues on that stream itself must
 * come after bn_ctx_get_stream or bn_sync: both flush deferred work first.
 * bn_ctx_set_stream(s != NULL) runs the context on a caller-owned hipStream_t (e.g.
 * torch.cuda.Stream().cuda_stream) and turns the deferral OFF (strict call order, no fold +
 * evaluation fusion) unless BN_LAZY_ON_SHARED_STREAM=1 accepts the rule above; NULL = back to an own
 * stream with the behaviour the context was created with.  Handle 0 IS NULL: the default (null) stream,
 * torch's default stream included, selects the own stream and is never adopted.  Every entry point makes
 * the context's device current on the calling thread. */
int bn_ctx_set_stream(bn_ctx *ctx, void *hip_stream);
int bn_sync(bn_ctx *ctx);
/* the hipStream_t the context enqueues on, after flushing deferred work (so a caller can put an RCCL
 * collective in the same order) */
int bn_ctx_get_stream(bn_ctx *ctx, void **hip_stream);

/* ---- ComputeLayer (layer.rs:36-87) ---- */
int bn_copy_h2d(bn_ctx *ctx, const bn_f128 *h_src, uint64_t src_len, void *d_dst, uint64_t dst_len);
int bn_copy_d2h(bn_ctx *ctx, const void *d_src, uint64_t src_len, bn_f128 *h_dst, uint64_t dst_len);
int bn_copy_d2d(bn_ctx *ctx, const void *d_src, uint64_t src_len, void *d_dst, uint64_t dst_len);
int bn_fill(bn_ctx *ctx, void *d_dst, uint64_t n, const bn_f128 *value);

/* compile_expr (layer.rs:57): ArithCircuitStep list, crates/math/src/arith_expr.rs:200-206 */
enum { BN_STEP_ADD = 0, BN_STEP_MUL = 1, BN_STEP_POW = 2, BN_STEP_CONST = 3, BN_STEP_VAR = 4 };
typedef struct {
	uint32_t kind;
	uint32_t a;   /* Add/Mul: left step; Pow: base step; Var: variable index */
	uint64_t b;   /* Add/Mul: right step; Pow: exponent */
	bn_f128 cst;  /* Const */
} bn_step;
int bn_expr_compile(bn_ctx *ctx, const bn_step *steps, uint64_t n_steps, bn_expr **out);
int bn_expr_free(bn_expr *expr);
int bn_expr_n_vars(const bn_expr *expr, uint32_t *n_vars);
/* Extension (not a trait method): a TOWER-TYPED expression, for bn_compute_composite on packed subfield columns -- the computed
 * columns of m3's add_computed (m3/src/builder/constraint_system.rs:515-540): pack_fp / pack_b8 (sum of bit_i * beta_i: B1 terms,
 * coefficients and output in B8 / B32 / B64) and composites such as prod_high[bit] + x_is_negative * (prod_high[bit] + zout[bit]) at B1
 * (m3/src/gadgets/mul.rs:466-489).  Steps as for bn_expr_compile: topological order, the last step is the result.  input_levels[v]
 * (variable v) and out_level are packable tower levels, 0 or 3 .. 7.  Every step has a level: VAR its input's; CONST the smallest l
 * in 0 .. 7 with cst < 2^(2^l) (1 and 2 are fine for a constant); ADD / MUL the maximum of its operands'; POW its base's; none may
 * exceed out_level.  A value of a lower level is zero-extended (the tower embedding is the identity on the low bits), so the result
 * equals evaluating in B128 and truncating to 2^out_level bits.
 * VAR and CONST steps hold no slot; an ADD / MUL / POW result holds one from its step to its last use, and at most
 * BN_TOWER_EXPR_MAX_LIVE may be live at once (the kernel's LDS: 16 slots x 16 B x 256 threads = 64 KiB).  Steps that do not feed the
 * result are dropped first.
 * BN_ERR_INPUT_VALIDATION with nothing allocated: null arguments, n_steps = 0 or above BN_TOWER_EXPR_MAX_STEPS, n_inputs above
 * BN_TOWER_EXPR_MAX_INPUTS, an operand that is not an earlier step, a VAR index >= n_inputs, an unknown kind, level 1, 2 or > 7 for an
 * input or the output, a step above out_level, too many live slots.
 * bn_expr_n_vars answers n_inputs; bn_expr_free frees it.  ONLY bn_compute_composite takes such an expression: every other consumer
 * of a bn_expr (bn_kernel_launch, bn_hal_round_evals) answers BN_ERR_INPUT_VALIDATION before it launches anything. */
#define BN_TOWER_EXPR_MAX_STEPS 1024
#define BN_TOWER_EXPR_MAX_INPUTS 256
#define BN_TOWER_EXPR_MAX_LIVE 16
int bn_expr_compile_tower(bn_ctx *ctx, const bn_step *steps, uint64_t n_steps, const uint32_t *input_levels, uint32_t n_inputs,
                          uint32_t out_level, bn_expr **out);

/* ---- ComputeLayerExecutor ---- */
/* extrapolate_line (layer.rs:421): evals_0[i] += (evals_1[i] - evals_0[i]) * z */
int bn_extrapolate_line(bn_ctx *ctx, void *d_evals_0, uint64_t n0, const void *d_evals_1, uint64_t n1,
                        const bn_f128 *z);
/* `count` extrapolate_line calls with the same z and length issued inside one executor `map` scope
 * (ComputeLayerExecutor::map, layer.rs:126; the fold of all multilinears of a round,
 * v3/bivariate_product.rs:217-228) as one call.  count <= BN_FOLD_CALL_MAX per call: a BivariateSumcheckProver of the PCS
 * prover holds every committed multilinear of one size and its transparents (piop/prove.rs:262-287: >= 100 for keccak), and
 * the backend defers the whole fold as one batch whose arrays the next round evaluation's launch folds on the way. */
#define BN_FOLD_CALL_MAX 256
int bn_extrapolate_line_batch(bn_ctx *ctx, void *const *d_evals_0, const void *const *d_evals_1, uint32_t count, uint64_t n,
                              const bn_f128 *z);
/* Extension (not a trait method): the same batch fold, after which the UPPER half of every folded array i with bit i of
 * scale_mask set is multiplied by *hi_scale (n even).  Deferred and fused with the next round evaluation exactly like
 * bn_extrapolate_line_batch.  It lets a prover keep a multilinear pre-multiplied by the equality indicator across
 * rounds (the weighted MLE-check prover of binius_amd/host/sumcheck.hpp): when the variable that
 * splits the folded array becomes the round variable, its two halves carry the factors (1 - zeta) and zeta of that
 * variable's indicator coordinate; multiplying the upper half by (1 - zeta) / zeta levels them. */
int bn_extrapolate_line_batch_scaled(bn_ctx *ctx, void *const *d_evals_0, const void *const *d_evals_1, uint32_t count, uint64_t n,
                                     const bn_f128 *z, uint32_t scale_mask, const bn_f128 *hi_scale);
/* tensor_expand (layer.rs:291): data[..2^(log_n+k)] = data[..2^log_n] (x) (1-r_0,r_0) (x) ...
 * The upper half of every pass is OVERWRITTEN (y = prod), as in FastCpuLayer and
 * math/src/tensor_prod_eq_ind.rs:35-77.  The scalar CpuLayer ACCUMULATES into it instead (*y += prod,
 * cpu/layer.rs:298); the two agree whenever data[2^log_n ..] is zero on entry, which is what every
 * caller in crates/core guarantees (they allocate and zero-fill first).  A caller that relies on the
 * accumulate form with a non-zero tail must add the old tail itself. */
int bn_tensor_expand(bn_ctx *ctx, void *d_data, uint64_t data_len, uint32_t log_n, const bn_f128 *h_coords,
                     uint32_t k);
/* inner_product (layer.rs:263): a is a SubfieldSlice{slice, tower_level} (memory.rs:257-281) */
int bn_inner_product(bn_ctx *ctx, const void *d_a, uint64_t a_len, uint32_t tower_level, const void *d_b,
                     uint64_t b_len, bn_f128 *h_out);
/* fold_left / fold_right (layer.rs:321, 351) */
int bn_fold_left(bn_ctx *ctx, const void *d_mat, uint64_t mat_len, uint32_t tower_level, const void *d_vec,
                 uint64_t vec_len, void *d_out, uint64_t out_len);
int bn_fold_right(bn_ctx *ctx, const void *d_mat, uint64_t mat_len, uint32_t tower_level, const void *d_vec,
                  uint64_t vec_len, void *d_out, uint64_t out_len);
/* fri_fold (layer.rs:389).  The NTT object is passed as its on-the-fly twiddle basis:
 * h_s_evals[i*BN_NTT_MAX_DIM + b] = s_evals[i][b] of OnTheFlyTwiddleAccess
 * (crates/ntt/src/twiddle.rs:93-124), elements of T_tw_level in the low bits of a u64. */
#define BN_NTT_MAX_DIM 64
int bn_fri_fold(bn_ctx *ctx, const uint64_t *h_s_evals, uint32_t tw_level, uint32_t log_domain, uint32_t log_len,
                uint32_t log_batch_size, const bn_f128 *h_challenges, uint32_t n_challenges, const void *d_in,
                uint64_t in_len, void *d_out, uint64_t out_len);
/* compute_composite (layer.rs:459)
 * With an expression of bn_expr_compile_tower the rows are PACKED SUBFIELD columns: row_len = out_len = the number of VALUES, a power of
 * two with row_len * 2^out_level >= 128; d_rows[v] is input v packed at input_levels[v] as bn_hal_multilinear says (a row below one
 * element: the low bits of one 16-byte element); d_out receives exactly row_len * 2^out_level / 128 elements, out[i] = expr(in_0[i], ...)
 * in T_out_level.  Bit-exact, overwritten; inputs are only read; d_out overlaps no row; pointers 16-byte aligned; n_inputs <= n_rows.
 * Everything else is BN_ERR_INPUT_VALIDATION with nothing launched and no counter moved.  ONE launch per call (kernels_compose_tower.hip):
 * a thread owns whole output elements, level 0 is bitwise on the whole element, a product walks the bits of its operand of lower level. */
int bn_compute_composite(bn_ctx *ctx, const void *const *d_rows, uint32_t n_rows, uint64_t row_len, void *d_out,
                         uint64_t out_len, const bn_expr *expr);
/* Read-only, per context (not part of the reference interface): accepted bn_compute_composite calls with a tower-typed expression, the
 * launches they made, how many of them ran at level 0 (bitwise) and at levels 3 .. 7 (per value).  A rejected call counts nowhere. */
enum { BN_CC_TOWER_CALLS = 0, BN_CC_TOWER_LAUNCHES = 1, BN_CC_TOWER_BITWISE = 2, BN_CC_TOWER_VALUES = 3, BN_CC_N = 4 };
int bn_compute_composite_counters(bn_ctx *ctx, uint64_t *counters /*[BN_CC_N]*/);
/* Extension (not a trait method): a BATCH of tower-typed expressions -- the expression columns of one wave of a witness plan in ONE
 * launch, as bn_derive_columns_batch, bn_generate_columns_batch and bn_partial_eval_high_lincomb_batch serve theirs.  exprs[] are handles of
 * bn_expr_compile_tower; the batch COPIES their compiled programs (duplicates are dropped), so the members may be freed right after.  The
 * result is a bn_expr of a third kind that owns no device memory: its tables travel with each call.  bn_expr_free frees it; bn_expr_n_vars
 * answers the number of rows a call must pass, the maximum over jobs of first_row + the job expression's input count; bn_kernel_launch
 * and bn_hal_round_evals reject it as they reject a tower-typed expression.
 * bn_compute_composite with such a batch: d_rows[0 .. n_rows) are the input columns of ALL jobs -- job j's input v is
 * d_rows[first_row_j + v], 2^n_vars_j values packed at that input's level (below one element: the low bits of one element); the
 * batch's row count is <= n_rows.  d_out is the base of an output ARENA of out_len 16-byte elements and row_len = out_len; job j writes
 * exactly 2^(n_vars_j + L_j - 7) elements at d_out + 16 * out_offset_j, inside the arena.  Rows may lie inside the arena (a wave's inputs are
 * an earlier wave's outputs in the same scratch), but no job's output overlaps any row of any job, each row at its own packed size.
 * Bit-exact, overwritten, inputs only read, pointers 16-byte aligned.  One upload and ONE launch per call (k_compose_tower_batch: a
 * workgroup finds its job by bisection over the job table; the dynamic LDS is the maximum over the jobs).
 * BN_ERR_INPUT_VALIDATION at compile time with nothing allocated: null arguments, n_jobs = 0 or above BN_COMPOSE_BATCH_MAX_JOBS, expr >=
 * n_exprs, a member that is no tower expression or belongs to another device, reserved != 0, n_vars > BN_PE_MAX_VARS, n_vars + out_level
 * < 7, two jobs' output ranges overlapping, units (1024 output elements each, rounded up per job) that leave 31 bits.  At the call, with
 * nothing launched or written and no counter moved: every violation of the paragraph above. */
typedef struct {
	uint32_t expr;       /* index into exprs[]: several jobs may share one */
	uint32_t first_row;  /* the job's input v is the call's d_rows[first_row + v] */
	uint32_t n_vars;     /* the job computes 2^n_vars values */
	uint32_t reserved;   /* 0 */
	uint64_t out_offset; /* where the job's output starts, in 16-byte elements from the call's d_out */
} bn_compose_job;
#define BN_COMPOSE_BATCH_MAX_JOBS 4096
/* The job table crosses this interface as two arrays of integers, as the column tables of bnh_witness_* do: job j is
 * job_desc[4 j .. 4 j + 4) = { expr, first_row, n_vars, reserved } and out_offsets[j] -- the fields of bn_compose_job, which is what the
 * planner (csrc/compose_batch.hpp) and the C++ and Rust wrappers take. */
#define BN_COMPOSE_JOB_DESC_WORDS 4
int bn_expr_compile_tower_batch(bn_ctx *ctx, const bn_expr *const *exprs, uint32_t n_exprs, const uint32_t *job_desc, const uint64_t *out_offsets,
                                uint32_t n_jobs, bn_expr **out);
/* Read-only, per context: accepted bn_compute_composite calls with a batch, the launches they made, the jobs they served and the
 * programs they uploaded (distinct ones, after dropping duplicates).  A batch call moves none of BN_CC_TOWER_*; a rejected call counts
 * nowhere. */
enum { BN_CCB_CALLS = 0, BN_CCB_LAUNCHES = 1, BN_CCB_JOBS = 2, BN_CCB_PROGRAMS = 3, BN_CCB_N = 4 };
int bn_compute_composite_batch_counters(bn_ctx *ctx, uint64_t *counters /*[BN_CCB_N]*/);
/* pairwise_product_reduce (layer.rs:505) */
int bn_pairwise_product_reduce(bn_ctx *ctx, const void *d_in, uint64_t n, void *const *d_round_outs,
                               const uint64_t *round_lens, uint32_t n_rounds);
/* Every layer of a batch of halves-product trees: the witness of the GKR grand-product argument (GrandProductWitness::new,
 * core/src/protocols/gkr_gpa/gkr_gpa.rs:38-90; the same layers as ProductCircuitLayers::compute, prodcheck/prove.rs:24-77),
 *   layer_j[i] = layer_{j+1}[i] * layer_{j+1}[i + 2^j],  0 <= i < 2^j,  layer_{n_vars} = the input.
 * Tree t has n_vars[t] in 0 .. 28 variables; d_inputs[t] holds input_lens[t] <= 2^n_vars[t] B128 elements, the absent tail counts
 * as ONE (the truncated witness, gkr_gpa.rs:34-37, 70-73; input_lens[t] = 0 is legal, d_inputs[t] may then be NULL).  d_layers[t]
 * is an arena of 2^n_vars[t] elements in heap order: on return arena[2^j + i] = element i of layer j for 0 <= j < n_vars (arena[1]
 * is the product), arena[0] is not touched, every layer is written in full.  The two multilinears of layer j's sumcheck are the
 * contiguous halves arena[2^(j+1) ..] and arena[2^(j+1) + 2^j ..].  Inputs are only read; an arena must not overlap its input.
 * products_out[t] = layer 0 (n_vars = 0: the input element, or ONE; d_layers[t] is not used).  All trees share the launches
 * of the largest one.  Returns when the products are on the host. */
#define BN_PRODUCT_TREE_MAX_VARS 28
int bn_product_tree_layers(bn_ctx *ctx, uint32_t n_trees, const uint32_t *n_vars, const void *const *d_inputs,
                           const uint64_t *input_lens, void *const *d_layers, bn_f128 *products_out);
/* d_dsts[t][i] = i < src_lens[t] ? d_srcs[t][i] : ONE for i < 2^log_lens[t], all n arrays in one launch: the full-length copies
 * of truncated inputs that the grand-product prover folds (its sumcheck consumes what it works on).  Synchronises the stream. */
int bn_pad_with_ones(bn_ctx *ctx, uint32_t n, const uint32_t *log_lens, const void *const *d_srcs, const uint64_t *src_lens,
                     void *const *d_dsts);
/* Every layer of a batch of exponentiation circuits: the witness of the GKR exponentiation argument (core/src/protocols/gkr_exp/
 * witness.rs:31-110 the static base, :139-156, 258-284 the dynamic base; built at constraint_system/prove.rs:186-195).  Witness t
 * has n_vars[t] in 0 .. 28 variables (2^n_vars rows), an exponent of widths[t] in 1 .. 128 bit columns e_0 (least significant)
 * .. e_{w-1}, and kinds[t]: BN_EXP_STATIC with the constant base g = static_bases[t], or BN_EXP_DYNAMIC with the column
 * d_bases[t] of 2^n_vars B128 elements (the entry of the other kind is ignored).  Its w layers of 2^n_vars B128 elements are
 *   static :  V_0[i] = e_0[i] ? g : 1              V_k[i] = V_{k-1}[i]   * (e_k[i] ? g^(2^k) : 1)
 *   dynamic:  V_0[i] = e_{w-1}[i] ? base[i] : 1    V_k[i] = V_{k-1}[i]^2 * (e_{w-1-k}[i] ? base[i] : 1)
 * (note the opposite bit orders); V_{w-1} is the exponentiation result.  All in B128: a base of a subfield is passed embedded,
 * which is the identity on the low bits.  d_exponent_bits is a HOST array of sum(widths) device pointers, witness after witness,
 * e_0 first.  A bit column is a B1 multilinear packed into F as bn_hal_multilinear describes for tower level 0: bit i of the
 * column is bit i & 127 of 16-byte element i >> 7, little-endian; for n_vars < 7 the low 2^n_vars bits of one element.
 * d_layers[t] is an arena of widths[t] * 2^n_vars[t] elements, layer k at offset k * 2^n_vars.  Inputs are only read, every layer
 * is written in full, an arena must not overlap its witness's inputs; pointers are 16-byte aligned.  The whole batch is ONE
 * launch whatever the widths and the number of witnesses.  Returns when the layers are complete. */
enum { BN_EXP_STATIC = 0, BN_EXP_DYNAMIC = 1 };
#define BN_EXP_MAX_VARS 28
#define BN_EXP_MAX_WIDTH 128
int bn_exp_circuit_layers(bn_ctx *ctx, uint32_t n_witnesses, const uint32_t *n_vars, const uint32_t *widths, const uint32_t *kinds,
                          const void *const *d_exponent_bits, const bn_f128 *static_bases, const void *const *d_bases,
                          void *const *d_layers);
/* d_dsts[t][i] = bit i of d_srcs[t] ? ONE : ZERO for i < 2^log_lens[t] (bits packed as above), all n arrays in one launch: the bit
 * columns as the B128 multilinears that the exponentiation prover folds.  Synchronises the stream. */
int bn_bits_to_b128(bn_ctx *ctx, uint32_t n, const uint32_t *log_lens, const void *const *d_srcs, void *const *d_dsts);
/* Read-only, per context (not part of the reference interface): accepted bn_exp_circuit_layers calls, the kernel launches they
 * made, and the launches of bn_bits_to_b128.  A rejected call counts nowhere. */
enum { BN_EXP_CALLS = 0, BN_EXP_LAUNCHES = 1, BN_EXP_BITS_LAUNCHES = 2, BN_EXP_N = 3 };
int bn_exp_counters(bn_ctx *ctx, uint64_t *counters /*[BN_EXP_N]*/);
/* The masked witnesses of a batch of channel flushes: make_masked_flush_witnesses (core/src/constraint_system/prove.rs:671-881), the
 * input of the grand-product argument over every flush oracle (prove.rs:386-400).  Flush f has n_vars[f] in 0 .. 28 variables
 * (2^n_vars rows), n_selectors[f] in 0 .. 8 selectors and n_columns[f] in 1 .. 64 columns (none is the reference's
 * EmptyFlushOracles: BN_ERR_INPUT_VALIDATION).  d_selectors, d_columns, tower_levels and coeffs are HOST arrays, concatenated flush
 * after flush; the first two hold device pointers.  A selector is a B1 column, a column holds values of tower level 0 or 3 .. 7
 * (levels may be mixed inside a flush), both packed into F as bn_hal_multilinear describes: bit i & 127 of 16-byte element i >> 7
 * is the level-0 value of row i; a column with n_vars + level < 7 occupies the low 2^(n_vars + level) bits of one element.  A
 * subfield value embeds into B128 as the identity on the low bits.
 *   p_s           = 128 * (1 + index of the last non-zero 16-byte element of selector s), 0 if there is none, clipped to 2^n_vars
 *                   (count_zero_suffixes, prove.rs:883-902, at a 128-bit underlier)
 *   prefix_len[f] = min_s p_s, or 2^n_vars without selectors
 *   d_outs[f][i]  = (every selector has bit i set) ? const_terms[f] + sum_j coeffs[f, j] * col_{f, j}[i] : ONE    for i < prefix_len[f]
 * bit-exact; the caller passes const_terms[f] = r_channel + sum over the flush's constant entries of base * alpha^k and the mixing
 * powers alpha^k of its column entries as coeffs (prove.rs:744-771).  Elements at and beyond prefix_len[f] are NOT written:
 * bn_product_tree_layers takes prefix_lens_out[f] as input_lens and counts the tail as ONE.  The result does not depend on which
 * coefficients equal ONE (prove.rs:836-844 special-cases the first mixing power; so does the kernel).  Inputs are only read; an
 * output must not overlap an input or another output of the call; pointers are 16-byte aligned; n_flushes = 0 is a no-op; a
 * rejected call launches nothing.  The whole batch is ONE launch, behind ONE launch that finds the selectors' prefixes when the
 * call has a selector, whatever the number of flushes, their sizes and levels.  Returns when the witnesses are complete and
 * prefix_lens_out is filled in. */
#define BN_FLUSH_MAX_VARS 28
#define BN_FLUSH_MAX_SELECTORS 8
#define BN_FLUSH_MAX_COLUMNS 64
int bn_flush_witness_batch(bn_ctx *ctx, uint32_t n_flushes, const uint32_t *n_vars, const uint32_t *n_selectors,
                           const void *const *d_selectors, const uint32_t *n_columns, const void *const *d_columns,
                           const uint32_t *tower_levels, const bn_f128 *coeffs, const bn_f128 *const_terms, void *const *d_outs,
                           uint64_t *prefix_lens_out);
/* Read-only, per context (not part of the reference interface): accepted bn_flush_witness_batch calls, the kernel launches they
 * made, the flushes they served, and how many of those needed more than one pass of nibble tables.  A rejected call counts
 * nowhere. */
enum { BN_FLUSH_CALLS = 0, BN_FLUSH_LAUNCHES = 1, BN_FLUSH_SERVED = 2, BN_FLUSH_MULTIPASS = 3, BN_FLUSH_N = 4 };
int bn_flush_counters(bn_ctx *ctx, uint64_t *counters /*[BN_FLUSH_N]*/);
/* A batch of columns evaluated at the high coordinates of one point: evaluate_partial_high (math/src/multilinear_extension.rs:
 * 253-300) of the inner column of every shifted or packed virtual column of an evalcheck round (collect_projected_mles,
 * core/src/protocols/evalcheck/subclaims.rs:356-439), where every claim of a table shares the point.  Column c holds 2^n_vars
 * values of tower level 0 or 3 .. 7 packed into F as bn_fold_left takes them (at least one 16-byte element: n_vars + tower_level
 * >= 7); d_tensor_query is the tensor expansion of the query_vars <= n_vars high coordinates (2^query_vars B128 elements, shared
 * by all columns).  d_outs[c] receives exactly what
 *   bn_fold_left(d_evals, 2^(n_vars - 7 + tower_level), tower_level, d_tensor_query, 2^query_vars, d_outs[c], 2^(n_vars - query_vars))
 * writes: out[i] = sum_j query[j] * column[j * out_len + i], bit-exact, overwritten not accumulated.  query_vars = 0 widens the
 * column to B128; n_vars = query_vars is one inner product.  cols and d_outs are HOST arrays; pointers are 16-byte aligned; inputs
 * are only read; an output must not overlap its column.  Columns with at most 1024 outputs share TWO launches whatever their
 * number, levels and sizes (the reduction of a column is split across workgroups, the query chunk of a workgroup serves several
 * columns); a column with more outputs runs on the bn_fold_left kernels inside the same call.  n_cols = 0 is a no-op.
 * bn_fold_left itself takes this route as a one-column job for out_len <= 1024 and vec_len >= 4096. */
typedef struct {
	const void *d_evals;
	uint32_t tower_level;
	uint32_t n_vars;
} bn_pe_column;
#define BN_PE_MAX_VARS 40
/* (cols points to n_cols bn_pe_column; the prototype spells it as untyped memory so that the checked FFI declarations, which know a
 * closed set of type names, carry it unchanged.) */
int bn_partial_eval_high_batch(bn_ctx *ctx, const void *cols, uint32_t n_cols, const void *d_tensor_query, uint32_t query_vars,
                               void *const *d_outs);
/* Read-only, per context (not part of the reference interface): accepted bn_partial_eval_high_batch calls; kernel launches of
 * the partial-evaluation kernels (routed bn_fold_left calls included); columns they served; columns that went to the fold_left
 * kernels; the largest number of workgroups that shared one column in the last call; bn_fold_left calls routed here.  A rejected
 * call counts nowhere. */
enum { BN_PE_CALLS = 0, BN_PE_LAUNCHES = 1, BN_PE_COLS_KERNEL = 2, BN_PE_COLS_FALLBACK = 3, BN_PE_MAX_SHARE = 4, BN_PE_FOLD_LEFT_ROUTED = 5, BN_PE_N = 6 };
int bn_partial_eval_counters(bn_ctx *ctx, uint64_t *counters /*[BN_PE_N]*/);
/* The same projection for inner columns that are LINEAR COMBINATIONS of columns and are never materialised (try_build_partial_eval,
 * core/src/protocols/evalcheck/subclaims.rs:305-346; keccak's c[x], the sum of five state columns, under its shift).  Job j has n_vars
 * variables and the terms terms[first_term .. first_term + n_terms), n_terms <= BN_PEL_MAX_TERMS; a term is a column of 2^n_vars values
 * of its own tower level (0 or 3 .. 7, levels may differ inside a job), packed as bn_partial_eval_high_batch takes columns (n_vars +
 * tower_level >= 7), with a B128 coefficient.  A column may appear in several jobs and more than once in one.  With out_len =
 * 2^(n_vars - query_vars):
 *   d_outs[j][i] = offset + sum_t coeff_t * sum_{q < 2^query_vars} query[q] * column_t[q * out_len + i]
 * bit-exact, overwritten not accumulated, exactly out_len elements.  The offset is added once, unscaled (the tensor expansion of a point
 * sums to one; the op does not check the query).  n_terms = 0 gives the offset; a zero coefficient contributes nothing; nested
 * combinations are flattened by the caller.  jobs, terms and d_outs are HOST arrays; pointers are 16-byte aligned; every reserved
 * field is 0; inputs are only read; an output overlaps no column, not the query and no other output.  Inside a job the terms of equal
 * (tower level, coefficient) are XOR-ed as packed words when they are loaded and cost ONE pass over the rows; the sums of such a class
 * are multiplied by the coefficient once per workgroup (never for ONE).  TWO launches serve all jobs of at most 1024 outputs whatever
 * their number, terms, levels and sizes (neither is made when the call has no such job); jobs with more outputs share ONE further
 * launch of a one-thread-per-output form.  n_jobs = 0 is a no-op.  The work runs on the context's stream; the outputs are complete when the
 * call returns. */
typedef struct {
	const void *d_evals;
	uint32_t tower_level;
	uint32_t reserved;
	bn_f128 coeff;
} bn_pel_term;
typedef struct {
	uint32_t n_vars;
	uint32_t first_term;
	uint32_t n_terms;
	uint32_t reserved;
	bn_f128 offset;
} bn_pel_job;
#define BN_PEL_MAX_TERMS 64
/* (jobs points to n_jobs bn_pel_job, terms to n_terms_total bn_pel_term; untyped in the prototype for the same reason as
 * bn_partial_eval_high_batch's cols.) */
int bn_partial_eval_high_lincomb_batch(bn_ctx *ctx, const void *jobs, uint32_t n_jobs, const void *terms, uint32_t n_terms_total,
                                       const void *d_tensor_query, uint32_t query_vars, void *const *d_outs);
/* Read-only, per context: accepted bn_partial_eval_high_lincomb_batch calls; the kernel launches they made; jobs; terms; classes (row
 * loops planned, summed over the jobs); jobs served by the one-thread-per-output form; the largest number of workgroups that shared one
 * job in the last call.  A rejected call counts nowhere; the BN_PE_* counters do not move. */
enum { BN_PEL_CALLS = 0, BN_PEL_LAUNCHES = 1, BN_PEL_JOBS = 2, BN_PEL_TERMS = 3, BN_PEL_CLASSES = 4, BN_PEL_JOBS_FALLBACK = 5, BN_PEL_MAX_SHARE = 6, BN_PEL_N = 7 };
int bn_partial_eval_lincomb_counters(bn_ctx *ctx, uint64_t *counters /*[BN_PEL_N]*/);
/* The fold of the univariate round of the univariate-skip zerocheck, for every column of a call: ZerocheckProverImpl::
 * fold_univariate_round (core/src/protocols/sumcheck/prove/zerocheck.rs:384-434), which is evaluate_partial_low (math/src/
 * multilinear_extension.rs:302-341) at a query whose expansion is overwritten with the Lagrange coefficients of the univariate
 * challenge (prove/univariate.rs:139-193).  k = skip_rounds, 1 <= k <= 8; h_coeffs: the 2^k coefficients in B128, on the HOST, shared by
 * all columns.  Column c (cols[c], the layout of bn_pe_column) is TRANSPARENT with n_vars in k .. BN_PE_MAX_VARS variables at tower
 * level 0 (B1) or 3 (B8) -- the levels bn_zerocheck_univariate_evals accepts --, packed into F as bn_hal_multilinear says (a column of
 * n_vars + tower_level < 7 occupies the low bits of one 16-byte element); sizes and levels may differ inside a call.  d_outs[c]
 * receives exactly what
 *   bn_fold_right(d_evals, 2^(n_vars - 7 + tower_level), tower_level, coeffs, 2^k, d_outs[c], 2^(n_vars - k))
 * writes with the coefficients on the device (a column of at least one element): out[x] = sum_{u < 2^k} coeffs[u] * column[u + 2^k x], bit-exact, overwritten not
 * accumulated, nothing written beyond 2^(n_vars - k) elements.  cols and d_outs are HOST arrays; pointers are 16-byte aligned; inputs
 * are only read; an output must not overlap its column.  Another level, k = 0, k > 8, k > n_vars, a misaligned or null pointer and an
 * overlapping output are BN_ERR_INPUT_VALIDATION with nothing launched; n_cols = 0 is a no-op.  The whole call is ONE launch whatever
 * the number of columns, their sizes and levels: the nibble tables of the coefficients are built once per workgroup and serve every
 * column.  Returns when the outputs are complete. */
#define BN_UNIVARIATE_FOLD_MAX_SKIP 8
int bn_univariate_fold_batch(bn_ctx *ctx, const void *cols, uint32_t n_cols, uint32_t skip_rounds, const bn_f128 *h_coeffs,
                             void *const *d_outs);
/* Read-only, per context (not part of the reference interface): accepted bn_univariate_fold_batch calls, the kernel launches they
 * made, the columns they served.  A rejected call counts nowhere. */
enum { BN_UF_CALLS = 0, BN_UF_LAUNCHES = 1, BN_UF_COLS = 2, BN_UF_N = 3 };
int bn_univariate_fold_counters(bn_ctx *ctx, uint64_t *counters /*[BN_UF_N]*/);
/* Every ring-switch equality indicator of a call: RingSwitchEqInd::multilinear_extension (core/src/ring_switch/eq_ind.rs:81-147),
 * one per claim of ring_switch::prove (core/src/ring_switch/prove.rs:116-124).  Job j (jobs[j], a HOST array of bn_rs_job) has d_query,
 * the tensor expansion of its suffix -- 2^n_vars B128 elements on the device, the table bn_partial_eval_high_batch takes as
 * d_tensor_query, shared by every job of that suffix and only read --, n_vars in 0 .. BN_PE_MAX_VARS, kappa in {0, 1, 2, 3, 4, 7} (the
 * packed tower level is 7 - kappa) and its mixing coefficient.  h_row_batch_coeffs: n_coeffs coefficients on the HOST that serve all
 * jobs, n_coeffs a power of two and at least 2^kappa for every job; a job uses the first 2^kappa.  d_outs[j] (2^n_vars elements)
 * receives exactly what
 *   bn_fill(evals, 0); evals[0] = mixing_coeff; bn_tensor_expand(evals, 0, suffix);
 *   bn_fold_right(evals, 2^n_vars, 7 - kappa, coeffs, 2^kappa, out, 2^n_vars)
 * writes: out[x] = sum_{i < 2^kappa} coeffs[i] * limb_i(mixing_coeff * query[x]), bit-exact, overwritten not accumulated, nothing
 * written beyond 2^n_vars elements.  A null or misaligned pointer, an output that overlaps a query or another output, kappa of 5 or 6
 * or above 7, n_vars out of range and too few coefficients are BN_ERR_INPUT_VALIDATION with nothing launched; n_jobs = 0 is a no-op.
 * The whole call is ONE launch whatever the number of jobs, queries and sizes: the jobs are sorted by query, a workgroup loads a
 * tile of a query once and takes it through the nibble tables of up to eight of the query's jobs.  Returns when the outputs are
 * complete. */
typedef struct {
	const void *d_query;
	uint32_t n_vars;
	uint32_t kappa;
	bn_f128 mixing_coeff;
} bn_rs_job;
/* (jobs points to n_jobs bn_rs_job; untyped in the prototype for the same reason as bn_partial_eval_high_batch's cols.) */
int bn_ring_switch_eq_ind_batch(bn_ctx *ctx, const void *jobs, uint32_t n_jobs, const bn_f128 *h_row_batch_coeffs, uint32_t n_coeffs,
                                void *const *d_outs);
/* Read-only, per context (not part of the reference interface): accepted bn_ring_switch_eq_ind_batch calls, the kernel launches
 * they made, the jobs they served, the distinct query pointers among those jobs (summed over calls).  A rejected call counts
 * nowhere. */
enum { BN_RS_CALLS = 0, BN_RS_LAUNCHES = 1, BN_RS_JOBS = 2, BN_RS_QUERIES = 3, BN_RS_N = 4 };
int bn_ring_switch_counters(bn_ctx *ctx, uint64_t *counters /*[BN_RS_N]*/);
/* A batch of columns evaluated at their whole claim points: the first step of every EvalcheckProver::prove call ("MLE Fold Full",
 * core/src/protocols/evalcheck/prove.rs:191-275, make_new_eval_claim evalcheck/prove.rs:812-879), which splits the point into a prefix
 * and a suffix, takes evaluate_partial_high of the column at the suffix and evaluate of the result at the prefix
 * (math/src/multilinear_extension.rs evaluate / evaluate_partial_high).  Point p (points[p], a HOST array of bn_me_point) has d_lo,
 * the 2^lo_vars B128 elements of the tensor expansion of its first lo_vars coordinates, lo_vars <= BN_ME_MAX_LO_VARS, and d_hi, the
 * 2^hi_vars elements of the expansion of the rest (the reference's memoised prefix and suffix query), both on the device.  Job j
 * (jobs[j], a HOST array of bn_me_job) names a column of 2^n_vars values of tower level 0 or 3..7 packed into F as
 * bn_partial_eval_high_batch takes them (n_vars + tower_level >= 7) and a point with lo_vars + hi_vars == n_vars; reserved is 0.
 *   h_out[j] = sum_h hi[h] * sum_l lo[l] * col[h * 2^lo_vars + l],
 * bit-exact, valid when the call returns (published through pinned memory and the sequence word, as bn_inner_product and
 * bn_xor_reduce publish theirs).  lo_vars = 0 and hi_vars = 0 are legal: a plain inner product with one table.  Columns and tables
 * are only read; pointers are 16-byte aligned; the work is issued on the context's stream.  n_jobs = 0 is a no-op.  A null or
 * misaligned pointer, lo_vars above BN_ME_MAX_LO_VARS, lo_vars + hi_vars != n_vars, tower level 1 or 2 or above 7, a column of less
 * than one 128-bit element, a point index outside the table, reserved != 0 and more than BN_ME_MAX_JOBS jobs are
 * BN_ERR_INPUT_VALIDATION: nothing is launched and nothing is counted.
 * TWO launches per call whatever the number of jobs, their levels, sizes and points: the evaluation kernel (a workgroup takes a
 * chunk of the high rows of up to eight jobs of one point and level, keeps their 2^lo_vars partial sums in LDS, multiplies them by
 * lo once and XOR-combines one element per job) and the kernel that publishes the results. */
typedef struct {
	const void *d_lo;
	const void *d_hi;
	uint32_t lo_vars;
	uint32_t hi_vars;
} bn_me_point;
typedef struct {
	const void *d_evals;
	uint32_t tower_level;
	uint32_t n_vars;
	uint32_t point;
	uint32_t reserved;
} bn_me_job;
#define BN_ME_MAX_LO_VARS 10
#define BN_ME_MAX_JOBS 4096 /* the pinned result area of a context holds this many evaluations */
/* (jobs points to n_jobs bn_me_job, points to n_points bn_me_point; untyped in the prototype for the same reason as
 * bn_partial_eval_high_batch's cols.) */
int bn_mle_evaluate_batch(bn_ctx *ctx, const void *jobs, uint32_t n_jobs, const void *points, uint32_t n_points, bn_f128 *h_out /*[n_jobs]*/);
/* Read-only, per context (not part of the reference interface): accepted bn_mle_evaluate_batch calls, the kernel launches they made,
 * the jobs they served, the largest number of workgroups that shared one job in the last call.  A rejected call counts nowhere; the
 * BN_PE_* counters do not move. */
enum { BN_ME_CALLS = 0, BN_ME_LAUNCHES = 1, BN_ME_JOBS = 2, BN_ME_MAX_SHARE = 3, BN_ME_N = 4 };
int bn_mle_evaluate_counters(bn_ctx *ctx, uint64_t *counters /*[BN_ME_N]*/);
/* merge_multilins (crates/core/src/piop/prove.rs:78-118, P = F) for multilinears resident on the device: the FRI message that
 * piop::commit encodes.  n_vars (HOST array, ascending) and d_multilins name n multilinears of 2^n_vars[i] B128 elements; with
 * off_i = sum_{j > i} 2^n_vars[j] (the last, largest multilinear comes first), for every r < 2^log_repeats and x < 2^n_vars[i]
 *   message[r * 2^total_vars + off_i + bitrev(x, n_vars[i])] = multilins[i][x],
 * every other element of message[0 .. 2^(total_vars + log_repeats)) is zero, nothing outside that range is written and the
 * multilinears are only read.  log_repeats > 0 writes the copies ReedSolomonCode::encode_ext_batch_inplace makes before its NTT, so a
 * commit can merge straight into the codeword buffer.  The op does not depend on the tower level: packed committed multilinears are
 * B128 elements already.  n = 0 is a zero fill; the same multilinear may appear twice.  A null or misaligned pointer, n_vars not
 * ascending (the error text starts "CommittedsNotSorted"), an n_vars[i] >= 48, total_vars + log_repeats >= 48, more than 2^total_vars
 * elements in all and a multilinear that overlaps the message range are BN_ERR_INPUT_VALIDATION: nothing is launched, nothing is
 * counted.  Like every op it first brings up to date what it reads (a fold deferred by bn_extrapolate_line_batch on a multilinear is
 * visible to the merge); the message is complete when the call returns.
 * ONE launch per call: a multilinear of at least 2 * BN_MERGE_TILE_LOG2 variables is a tiled job (a workgroup transposes a
 * 2^t x 2^t tile through LDS: both sides of memory see runs of 2^t elements), a smaller one a small job, the zero tail of every repeat
 * one more job.  (A call whose jobs or workgroups exceed what one launch holds -- 4096 jobs, 2^30 workgroups -- makes further
 * launches.) */
#define BN_MERGE_TILE_LOG2 6
int bn_merge_multilins(bn_ctx *ctx, uint32_t n, const uint32_t *n_vars, const void *const *d_multilins, void *d_message, uint32_t total_vars,
                       uint32_t log_repeats);
/* Read-only, per context (not part of the reference interface): accepted bn_merge_multilins calls, the kernel launches they made,
 * the jobs they served (multilinears and zero tails), and of the multilinears the tiled and the small ones.  A rejected call counts
 * nowhere. */
enum { BN_MERGE_CALLS = 0, BN_MERGE_LAUNCHES = 1, BN_MERGE_JOBS = 2, BN_MERGE_JOBS_TILED = 3, BN_MERGE_JOBS_SMALL = 4, BN_MERGE_N = 5 };
int bn_merge_counters(bn_ctx *ctx, uint64_t *counters /*[BN_MERGE_N]*/);
/* The virtual columns of a constraint system that are pure functions of columns already on the device, built there at their own
 * tower level: MultilinearPolyVariant::{Shifted, Repeating, ZeroPadded} and a LinearCombination whose coefficients are all ONE
 * (core/src/oracle/multilinear.rs), value by value as validate_witness defines them (core/src/constraint_system/validate.rs:151-279;
 * zero_pad: math/src/fold.rs:27-77).  u32_add's cin = cout << 1, keccak's rotations and c[x] sums and every repeated constant are of
 * these forms; a caller no longer fills them on the host and uploads them.
 * Job j (jobs[j], a HOST array of bn_derive_job) writes the column d_out of 2^n_vars values at tower_level (0 or 3 .. 7), n_vars <=
 * BN_PE_MAX_VARS, packed as bn_hal_multilinear says, at least one element (n_vars + tower_level >= 7): exactly 2^(n_vars + tower_level - 7)
 * elements are overwritten.  Indices below are value indices.
 *   BN_DERIVE_SHIFTED          d_inner has the output's level and n_vars.  block_size <= n_vars, 1 <= shift_offset < 2^block_size
 *                              (Shifted::new, multilinear.rs:805-816).  Inside every aligned block of B = 2^block_size values, with
 *                              s = shift_offset and o the index inside the block (validate.rs:177-238):
 *                                BN_SHIFT_CIRCULAR_LEFT   out[o] = in[(o + B - s) mod B]
 *                                BN_SHIFT_LOGICAL_LEFT    out[o] = in[o - s] for o >= s, else 0
 *                                BN_SHIFT_LOGICAL_RIGHT   out[o] = in[o + s] for o < B - s, else 0
 *   BN_DERIVE_REPEATING        d_inner has the output's level and inner_n_vars <= n_vars variables (it may be less than one element:
 *                              the low bits of one 16-byte element).  out[i] = in[i mod 2^inner_n_vars]  (validate.rs:167-176)
 *   BN_DERIVE_ZERO_PADDED      d_inner has the output's level and inner_n_vars <= n_vars variables, n_pad_vars = n_vars - inner_n_vars,
 *                              start_index <= inner_n_vars, nonzero_index < 2^n_pad_vars (the strict bound of
 *                              MultilinearExtension::zero_pad, not the `>` of ZeroPadded::new).  With col = i mod 2^(start_index +
 *                              n_pad_vars), row = i div 2^(start_index + n_pad_vars) and z = nonzero_index 2^start_index:
 *                              out[i] = in[row 2^start_index + col - z] for z <= col < z + 2^start_index, else 0  (fold.rs:52-75)
 *   BN_DERIVE_XOR_COMBINATION  out[i] = offset + sum of d_terms[first_term + t][i], t < n_terms <= BN_PEL_MAX_TERMS: the terms are
 *                              columns of the output's own level and n_vars from the call's term list (a HOST array of n_terms_total
 *                              device pointers), the offset a value of the output's level (below 2^(2^tower_level)).  A column may
 *                              appear in several jobs and more than once in one (twice cancels); n_terms = 0 is the constant column.
 * Fields a kind does not use are ignored; reserved is 0.  Everything is bit-exact; inner columns and terms are only read; pointers are
 * 16-byte aligned.  An output overlaps no inner column or term of ANY job of the call and no other output: a call holds no dependency
 * between its jobs (a column derived from a derived column goes into the next call).  Like every op it first brings up to date what it
 * reads; the outputs are complete when the call returns.  n_jobs = 0 is a no-op that counts nowhere.
 * ONE launch per call whatever the number, kinds, sizes and levels of the jobs: a streaming kernel over a job table, a workgroup
 * 4096 contiguous output elements of one job (1024 at a time), in bit coordinates (a value is 2^tower_level bits) so that one code
 * path serves every level (kernels_derive.hip).
 * BN_ERR_INPUT_VALIDATION with nothing launched and no counter moved: an unknown kind or shift variant, tower level 1 or 2 or above 7,
 * a null or misaligned pointer, a forbidden overlap, an output below one element, n_vars above BN_PE_MAX_VARS, reserved != 0, a job's
 * terms outside the term list, an offset outside the level's field and every bound stated above.
 * NOT taken here: any other LinearCombination (a B128 one with arbitrary coefficients is bn_partial_eval_high_lincomb_batch at
 * query_vars = 0), Projected (at ZERO / ONE query values and the transparent and structured columns that a few parameters determine:
 * bn_generate_columns_batch below; at other query values: bn_partial_eval_high_batch / bn_fold_right), Packed (the same bytes: an alias),
 * general circuit transparents.  A subfield LinearCombination with other coefficients (pack_fp: B1 terms, B32 coefficients) and Composite
 * at the column's own level are bn_compute_composite with an expression of bn_expr_compile_tower (the plan: bnh_witness_compute). */
enum { BN_DERIVE_SHIFTED = 0, BN_DERIVE_REPEATING = 1, BN_DERIVE_ZERO_PADDED = 2, BN_DERIVE_XOR_COMBINATION = 3 };
enum { BN_SHIFT_CIRCULAR_LEFT = 0, BN_SHIFT_LOGICAL_LEFT = 1, BN_SHIFT_LOGICAL_RIGHT = 2 }; /* ShiftVariant, multilinear.rs */
typedef struct {
	uint32_t kind;
	uint32_t tower_level;
	uint32_t n_vars;
	uint32_t inner_n_vars;
	const void *d_inner;
	void *d_out;
	uint32_t block_size;
	uint32_t shift_variant;
	uint64_t shift_offset;
	uint32_t start_index;
	uint32_t reserved;
	uint64_t nonzero_index;
	uint32_t first_term;
	uint32_t n_terms;
	bn_f128 offset;
} bn_derive_job;
/* (jobs points to n_jobs bn_derive_job; untyped in the prototype for the same reason as bn_partial_eval_high_batch's cols.) */
int bn_derive_columns_batch(bn_ctx *ctx, const void *jobs, uint32_t n_jobs, const void *const *d_terms, uint32_t n_terms_total);
/* Read-only, per context (not part of the reference interface): accepted bn_derive_columns_batch calls, the kernel launches they made,
 * the jobs they served.  A rejected call counts nowhere. */
enum { BN_DERIVE_CALLS = 0, BN_DERIVE_LAUNCHES = 1, BN_DERIVE_JOBS = 2, BN_DERIVE_N = 3 };
int bn_derive_counters(bn_ctx *ctx, uint64_t *counters /*[BN_DERIVE_N]*/);
/* The columns of a constraint system that a few integers, one field element or a 0/1 projection of a column on the device determine,
 * generated there at their own tower level.  It replaces filling them on the host and uploading them at column size: the Projected
 * oracles of m3's add_selected / add_projected (m3/src/builder/constraint_system.rs:445-483), whose query values are only ever ZERO or
 * ONE, the StepDown selector of every table whose size is not a power of two (core/src/constraint_system/prove.rs:653-), the
 * incrementing column of add_structured (m3/src/builder/structured.rs:64-81) and the transparents of core/src/transparent/ that are
 * determined by such parameters.  (bn_partial_eval_high_batch is no substitute for the projection: it returns B128 values.)
 * Job j (jobs[j], a HOST array of bn_generate_job) writes the column d_out of 2^n_vars values at tower_level (0 or 3 .. 7), n_vars <=
 * BN_PE_MAX_VARS, packed as bn_hal_multilinear says, at least one element (n_vars + tower_level >= 7): exactly 2^(n_vars + tower_level - 7)
 * elements are overwritten.  Indices below are value indices.
 *   BN_GEN_PROJECTED_BITS  d_inner has the output's level and inner_n_vars = n_vars + query_size variables; query_size >= 1, query_bits <
 *                          2^query_size, start_index + query_size <= inner_n_vars.  With s = start_index, lo = i mod 2^s, hi = i div 2^s:
 *                          out[i] = in[lo + query_bits 2^s + hi 2^(s + query_size)]: Projected, which is MultilinearExtension::
 *                          evaluate_partial at the hypercube vertex whose coordinates are the bits of query_bits, lowest first
 *                          (math/src/multilinear_extension.rs:193-237, validate.rs:239-254).  d_inner is only read and overlaps no output.
 *   BN_GEN_CONSTANT        out[i] = value, below 2^(2^tower_level)                                      (transparent/constant.rs)
 *   BN_GEN_STEP_DOWN       level 0: out[i] = 1 for i < index, else 0; index <= 2^n_vars                 (step_down.rs:38-70)
 *   BN_GEN_STEP_UP         level 0: out[i] = 0 for i < index, else 1; index <= 2^n_vars                 (step_up.rs:39-66)
 *   BN_GEN_SELECT_ROW      level 0: out[i] = 1 at i = index, else 0; index < 2^n_vars                   (select_row.rs:37)
 *   BN_GEN_INCREMENTING    out[i] = the value whose bit b is bit b of i (the integer i in the tower basis); n_vars <= 2^tower_level
 *                          (incrementing_expr, structured.rs:73-81)
 *   BN_GEN_POWERS          level 3 .. 7: out[i] = value^i in the level's field, out[0] = 1 also for value = 0; value (the base) below
 *                          2^(2^tower_level)                                                            (powers.rs:35-57)
 * Fields a kind does not use are ignored; reserved is 0.  Everything is bit-exact; pointers are 16-byte aligned; no output overlaps
 * another output or an inner column of ANY job of the call.  Like every op it first brings up to date what it reads; the outputs are
 * complete when the call returns.  n_jobs = 0 is a no-op that counts nowhere.
 * ONE launch per call whatever the number, kinds, sizes and levels of the jobs (kernels_generate.hip): the frame of
 * bn_derive_columns_batch.  A projection whose runs are whole elements is a strided copy; below that an output element is put together
 * from one piece per input element; the other kinds load nothing.  The powers base^(2^b) come from the host in a table of the call.
 * BN_ERR_INPUT_VALIDATION with nothing launched and no counter moved: an unknown kind, tower level 1 or 2 or above 7 (or not the
 * kind's), a null or misaligned pointer, a forbidden overlap, an output below one element, n_vars above BN_PE_MAX_VARS, reserved != 0
 * and every bound stated above.
 * NOT taken here: Projected at query values other than ZERO and ONE (bn_partial_eval_high_batch / bn_fold_right), Composite
 * (bn_compute_composite with an expression of bn_expr_compile_tower: bnh_witness_compute), general circuit transparents and StructuredFixedSize, TowerBasis, EqIndPartialEval (bn_tensor_expand),
 * ShiftIndPartialEval, DisjointProduct. */
enum {
	BN_GEN_PROJECTED_BITS = 0,
	BN_GEN_CONSTANT = 1,
	BN_GEN_STEP_DOWN = 2,
	BN_GEN_STEP_UP = 3,
	BN_GEN_SELECT_ROW = 4,
	BN_GEN_INCREMENTING = 5,
	BN_GEN_POWERS = 6
};
typedef struct {
	uint32_t kind;
	uint32_t tower_level;
	uint32_t n_vars;
	uint32_t start_index;
	const void *d_inner;
	void *d_out;
	uint32_t query_size;
	uint32_t reserved;
	uint64_t query_bits;
	uint64_t index;
	bn_f128 value;
} bn_generate_job;
/* (jobs points to n_jobs bn_generate_job; untyped in the prototype for the same reason as bn_partial_eval_high_batch's cols.) */
int bn_generate_columns_batch(bn_ctx *ctx, const void *jobs, uint32_t n_jobs);
/* Read-only, per context (not part of the reference interface): accepted bn_generate_columns_batch calls, the kernel launches they
 * made, the jobs they served.  A rejected call counts nowhere. */
enum { BN_GENERATE_CALLS = 0, BN_GENERATE_LAUNCHES = 1, BN_GENERATE_JOBS = 2, BN_GENERATE_N = 3 };
int bn_generate_counters(bn_ctx *ctx, uint64_t *counters /*[BN_GENERATE_N]*/);
/* The FRI query phase: everything FRIFolder::finish_proof (crates/core/src/protocols/fri/prove.rs:483-507) writes to the
 * decommitment, from codewords and Merkle trees resident on the device.  The indices are the caller's, as every challenge is: the
 * decommitment is not observed by the challenger (transcript/mod.rs:182-195), so all of them can be sampled before any opening is made.
 * Oracle i (oracles[i], a HOST array of bn_fri_oracle) names a committed codeword of 2^(log_n_cosets + log_coset_size) B128 elements,
 * the flattened tree over its 2^log_n_cosets cosets as bn_merkle_build writes it (2 * (2^(log_n_cosets + 1) - 1) elements: layers
 * concatenated, leaves first, root last; a digest is two elements), the depth of the layer the verifier receives
 * (FRIParams optimal layer depths, common.rs:174-190) and index_shift, the sum of the arities after the first up to this oracle: the
 * coset of query q in oracle i is indices[q] >> index_shift.  h_out receives, in transcript byte order,
 *   d_terminate[0 .. terminate_elems)                                             the terminate codeword
 *   for each oracle i: the 2^layer_depth digests of its layer                     (vcs_optimal_layers, prove.rs:597-610)
 *   for each query q, for each oracle i:                                          (prove_query, prove.rs:545-595)
 *       the 2^log_coset_size elements of the coset, then log_n_cosets - layer_depth digests, leaf sibling first
 * so the header and every query's record have the lengths bn_fri_query_proof_elems states (a pure host function: it reads the sizes
 * of the descriptors only, pointers may be null).  n_queries = 0 or n_oracles = 0 still copies the header; layer_depth = log_n_cosets
 * is an empty branch.  Like every op it first brings up to date what it reads (a fold deferred on a codeword is visible); everything
 * is only read; h_out is complete when the call returns.  ONE launch and one synchronisation per call whatever the number of queries
 * and oracles: a wave serves one (query, oracle), computing the coset offset and the branch node ids on the device, further
 * workgroups copy the header; the block comes back through pinned, device-mapped staging that grows on demand.
 * BN_ERR_INPUT_VALIDATION, with nothing launched and nothing counted: a null or misaligned pointer, an index >= 2^index_bits,
 * index_shift > index_bits or index_bits - index_shift > log_n_cosets (the shifted index would not be a coset of the oracle),
 * layer_depth > log_n_cosets, out_elems different from the layout's total, more than BN_FRI_QUERY_MAX_ORACLES oracles (the
 * descriptor table travels in the kernel arguments; FRI over 2^47 elements with arities of 2 or more has at most 23), a codeword of
 * 2^48 elements or more, and a total above 2^26 elements (bn_gather_d2h's limit for one call). */
typedef struct {
	const void *d_codeword;
	const void *d_nodes;
	uint32_t log_n_cosets;
	uint32_t log_coset_size;
	uint32_t layer_depth;
	uint32_t index_shift;
} bn_fri_oracle;
#define BN_FRI_QUERY_MAX_ORACLES 32
/* (oracles points to n_oracles bn_fri_oracle; untyped in the prototype for the same reason as bn_partial_eval_high_batch's cols.) */
int bn_fri_query_proof_elems(const void *oracles, uint32_t n_oracles, uint64_t terminate_elems, uint64_t n_queries, uint64_t *header_elems_out,
                             uint64_t *record_elems_out, uint64_t *total_elems_out);
int bn_fri_query_openings(bn_ctx *ctx, const void *oracles, uint32_t n_oracles, const void *d_terminate, uint64_t terminate_elems,
                          const uint64_t *indices /*[n_queries]*/, uint64_t n_queries, uint32_t index_bits, bn_f128 *h_out, uint64_t out_elems);
/* Read-only, per context (not part of the reference interface): accepted bn_fri_query_openings calls, the kernel launches they made,
 * the (query, oracle) openings they served.  A rejected call counts nowhere. */
enum { BN_FQ_CALLS = 0, BN_FQ_LAUNCHES = 1, BN_FQ_OPENINGS = 2, BN_FQ_N = 3 };
int bn_fri_query_counters(bn_ctx *ctx, uint64_t *counters /*[BN_FQ_N]*/);

/* ---- accumulate_kernels / map_kernels (layer.rs:183, 236) + KernelExecutor (layer.rs:518-590).
 * The kernel-spec closure cannot cross an FFI: the host shim runs it ONCE against a recording
 * KernelExecutor (the trait allows re-invocation, layer.rs:171-177) and passes the recorded op
 * list here.  Slices are chunk-relative views of the mapped buffers. */
enum { BN_MAP_CHUNKED = 0, BN_MAP_CHUNKED_MUT = 1, BN_MAP_LOCAL = 2 }; /* KernelMemMap, layer.rs:595-612 */
typedef struct {
	uint32_t kind;
	uint32_t log_min_chunk_size;
	void *d_data;     /* Chunked / ChunkedMut */
	uint64_t len;
	uint32_t log_size; /* Local: total size over all chunks */
} bn_memmap;

typedef struct {
	uint32_t buf;       /* index into the memmap list */
	uint64_t off, len;  /* within the chunk */
} bn_kslice;

enum { BN_KOP_DECL_VALUE = 0, BN_KOP_SUM_COMPOSITION = 1, BN_KOP_ADD = 2, BN_KOP_ADD_ASSIGN = 3 };
typedef struct {
	uint32_t kind;
	uint32_t value;          /* DECL_VALUE: id declared; SUM_COMPOSITION: accumulator id */
	bn_f128 scalar;          /* DECL_VALUE: init; SUM_COMPOSITION: batch_coeff */
	const bn_expr *expr;     /* SUM_COMPOSITION */
	uint32_t n_rows;
	const bn_kslice *rows;   /* SUM_COMPOSITION inputs */
	bn_kslice src1, src2, dst; /* ADD: dst = src1 + src2; ADD_ASSIGN: dst += src1 */
} bn_kop;

/* KernelMemMap::log_chunks_range (layer.rs:617-644), ComputeMemory::ALIGNMENT = 1. Host only. */
int bn_log_chunks_range(const bn_memmap *maps, uint32_t n_maps, uint32_t *start, uint32_t *end);
/* log_chunks this backend wants the closure recorded with (host only; deterministic). */
int bn_pick_log_chunks(const bn_memmap *maps, uint32_t n_maps, uint32_t *log_chunks);
/* Launch.  ops were recorded for `log_chunks`.  n_ret == 0 is map_kernels.  The n_ret returned
 * values (ids in ret_values) are XOR-accumulated over chunks (cpu/layer.rs:178-188) and written
 * to h_out (stream is synchronised) and/or left in d_out (n_ret elements, no sync) -- the latter
 * lets a multi-GPU caller feed them straight into an RCCL collective. */
int bn_kernel_launch(bn_ctx *ctx, const bn_memmap *maps, uint32_t n_maps, const bn_kop *ops, uint32_t n_ops,
                     const uint32_t *ret_values, uint32_t n_ret, uint32_t log_chunks, bn_f128 *h_out, void *d_out);

/* ---- AdditiveNTT (crates/ntt/src/additive_ntt.rs:102, 128): data is 2^(log_x+log_y+log_z)
 * elements of T_elem_level (elem_level 5 = BinaryField32b ... 7 = BinaryField128b), transform along
 * y; twiddles in T_tw_level given as the on-the-fly basis (see bn_fri_fold). */
/* ---- the OLD hardware abstraction layer: binius_hal::ComputationBackend (crates/hal/src/backend.rs:35-84), which the
 * v2 provers (zerocheck, evalcheck, RegularSumcheckProver) still run on, for device-resident multilinears.
 *   tensor_product_full_query   = bn_fill(1 element) + bn_tensor_expand            (cpu.rs:36-41)
 *   evaluate_partial_high       = bn_fold_left, evaluate_partial_low = bn_fold_right (multilinear_extension.rs:253-341)
 *   sumcheck_compute_round_evals = bn_hal_round_evals                               (sumcheck_round_calculation.rs:45-330)
 *   sumcheck_fold_multilinears   = bn_hal_fold_multilinear per multilinear           (sumcheck_folding.rs:16-237)
 * The trait takes its evaluators as trait objects; what crosses the boundary instead is their content: the
 * composition and its leading term as compiled circuits, the range of evaluation point indices, and the optional
 * equality-indicator table (RegularSumcheckEvaluator, regular_sumcheck.rs:219-282; eq_ind Evaluator, eq_ind.rs:646-735).
 * The switchover bookkeeping (switchover_round countdown, Transparent -> Folded) stays with the host-side state, as
 * in the reference (sumcheck_multilinear.rs:8-76).  Constant evaluation suffixes of EVALUATORS are not supported
 * (const_eval_suffix must be 0); constant suffixes of Folded multilinears are. */
enum { BN_ORDER_LOW_TO_HIGH = 0, BN_ORDER_HIGH_TO_LOW = 1 };  /* binius_math::EvaluationOrder */
enum { BN_HAL_ML_FOLDED = 0, BN_HAL_ML_TRANSPARENT = 1 };     /* SumcheckMultilinear */
typedef struct {
	uint32_t kind;
	uint32_t tower_level;  /* TRANSPARENT: level of the packed subfield values (0, 3..7) */
	const void *d_evals;   /* FOLDED: `len` evaluations; TRANSPARENT: the 2^n_vars_ml subfield values, packed into F */
	uint64_t len;          /* FOLDED: stored evaluations (the rest of the 2^n_vars cube equals suffix_eval); TRANSPARENT: F elements */
	bn_f128 suffix_eval;   /* FOLDED */
	uint32_t n_vars_ml;    /* TRANSPARENT: variables of the multilinear = n_vars + query_vars */
} bn_hal_multilinear;
typedef struct {
	const bn_expr *composition;
	const bn_expr *composition_at_infinity;     /* ArithCircuit::leading_term */
	uint32_t eval_point_start, eval_point_end;  /* SumcheckEvaluator::eval_point_indices: 0 -> X=0, 1 -> X=1, 2 -> infinity, 3+k -> point k */
	const void *d_eq_ind;                       /* NULL, or 2^(n_vars-1) factors (eq_ind partial evaluations) */
} bn_hal_evaluator;
/* h_out: evaluator by evaluator, one value per evaluation point index of its range.  d_tensor_query: the query
 * EXPANSION (2^query_vars elements) that TRANSPARENT multilinears are partially evaluated at (low variables for
 * BN_ORDER_LOW_TO_HIGH, high variables for BN_ORDER_HIGH_TO_LOW); NULL when query_vars == 0. */
int bn_hal_round_evals(bn_ctx *ctx, uint32_t order, uint32_t n_vars, const void *d_tensor_query, uint32_t query_vars,
                       const bn_hal_multilinear *mls, uint32_t n_mls, const bn_hal_evaluator *evaluators, uint32_t n_evaluators,
                       const bn_f128 *h_nontrivial_points, uint32_t n_points, bn_f128 *h_out);
/* FOLDED: single-variable lerp fold in the given order (d_out may be d_evals for BN_ORDER_HIGH_TO_LOW, must not overlap it
 * for BN_ORDER_LOW_TO_HIGH).  TRANSPARENT, at its switchover round: partial evaluation at the query, which already holds
 * this round's challenge (n_vars_ml = n_vars - 1 + query_vars).  *out_len evaluations are written. */
int bn_hal_fold_multilinear(bn_ctx *ctx, uint32_t order, uint32_t n_vars, const bn_hal_multilinear *ml, const bn_f128 *challenge,
                            const void *d_tensor_query, uint32_t query_vars, void *d_out, uint64_t out_cap, uint64_t *out_len);
/* The univariate round of the univariate-skip zerocheck: zerocheck_univariate_evals (prove/univariate.rs:235-507) with
 * extrapolate_round_evals (:571-640), for the domain field B8 (core/src/constraint_system/prove.rs:484, the 0..=3 arm).
 * k = skip_rounds (1 <= k <= n_vars), index i = u + 2^k x (u < 2^k), omega_j = the B8 element whose tower bits are j, L_u the
 * Lagrange basis over omega_0 .. omega_{2^k - 1}, Mhat_i(omega, x) = sum_u L_u(omega) M_i(u + 2^k x), eq = the tensor expansion
 * of the n_vars - k zerocheck challenges (d_eq, eq_len = 2^(n_vars - k) elements, challenge t on bit t of x).
 *   mls[n_mls]: the columns, TRANSPARENT, tower level 0 (B1) or 3 (B8), n_vars_ml = n_vars, packed as bn_hal_multilinear says
 *   steps / step_offsets[n_comps + 1] / degrees[n_comps]: composition c = steps[step_offsets[c] .. step_offsets[c + 1]) over B8
 *   (at most 64 steps, constants in B8), of degree d_c with d_c 2^k <= 256;  max_domain_size D: max_c d_c 2^k <= D <= 256.
 * P_c = the polynomial of degree < d_c 2^k that is zero on omega_0 .. omega_{2^k - 1} and equals
 * R_c(omega_j) = sum_x eq(x) C_c(Mhat_1(omega_j, x), ...) on omega_{2^k} .. omega_{d_c 2^k - 1} (P_c = 0 for d_c = 1).
 * h_out: P_c(omega_j) for 2^k <= j < D, composition by composition (n_comps (D - 2^k) values), or with h_batch_coeff = alpha
 * only sum_c alpha^c P_c (D - 2^k values; prove/zerocheck.rs:354-370).  A column at another level, a constant outside B8,
 * d_c 2^k > 256, k > n_vars and k = 0 are BN_ERR_INPUT_VALIDATION with nothing launched.  Synchronises the stream. */
int bn_zerocheck_univariate_evals(bn_ctx *ctx, uint32_t n_vars, uint32_t skip_rounds, const bn_hal_multilinear *mls, uint32_t n_mls,
                                  const bn_step *steps, const uint32_t *step_offsets, const uint32_t *degrees, uint32_t n_comps,
                                  const void *d_eq, uint64_t eq_len, uint32_t max_domain_size, const bn_f128 *h_batch_coeff, bn_f128 *h_out);
/* The same round for every arm of core/src/constraint_system/prove.rs:483-490: base_level = 3 .. 7 mirrors constructor.create::<FBase>()
 * with FBase = B8, B16, B32, B64, B128 (the table's arm: the largest column level and the compositions' binary_tower_level(), :458-467).
 * The domain and the Lagrange coefficients stay in B8; Mhat_i(omega_j, x) is a B8 x FBase product (the B8 scalar acts on each byte
 * coordinate), the composition is evaluated in FBase, eq(x) * v is a B128 x FBase product.  base_level 3 forwards to
 * bn_zerocheck_univariate_evals unchanged.  Above it:
 *   mls: TRANSPARENT, tower level 0 or 3 .. base_level, mixed freely, packed as bn_hal_multilinear says (little-endian values of
 *   2^(level - 3) bytes); constants of the compositions in the base field (below 2^(2^base_level)); every other limit, the
 *   outputs and the h_batch_coeff form as above (kernels_univariate_base.hip).
 * base_level outside 3 .. 7, a column at level 1, 2 or above base_level and a constant outside the base field are
 * BN_ERR_INPUT_VALIDATION with nothing launched. */
int bn_zerocheck_univariate_evals_base(bn_ctx *ctx, uint32_t base_level, uint32_t n_vars, uint32_t skip_rounds, const bn_hal_multilinear *mls,
                                       uint32_t n_mls, const bn_step *steps, const uint32_t *step_offsets, const uint32_t *degrees, uint32_t n_comps,
                                       const void *d_eq, uint64_t eq_len, uint32_t max_domain_size, const bn_f128 *h_batch_coeff, bn_f128 *h_out);

int bn_ntt_forward(bn_ctx *ctx, void *d_data, uint32_t elem_level, uint32_t tw_level, const uint64_t *h_s_evals,
                   uint32_t log_domain, uint32_t log_x, uint32_t log_y, uint32_t log_z, uint64_t coset,
                   uint32_t coset_bits, uint32_t skip_rounds);
int bn_ntt_inverse(bn_ctx *ctx, void *d_data, uint32_t elem_level, uint32_t tw_level, const uint64_t *h_s_evals,
                   uint32_t log_domain, uint32_t log_x, uint32_t log_y, uint32_t log_z, uint64_t coset,
                   uint32_t coset_bits, uint32_t skip_rounds);
/* OnTheFlyTwiddleAccess::generate for the canonical subspace (twiddle.rs:107-124, 244-306). Host only. */
int bn_ntt_s_evals(uint32_t tw_level, uint32_t log_domain, uint64_t *h_s_evals);

/* ---- host-only scalar helpers for the O(1)-per-round protocol scalars the host keeps
 * (evaluate_univariate of the round polynomial, powers of the batch coefficient:
 * crates/core/src/protocols/sumcheck/v3/bivariate_product.rs:150-156, 339-341).  Same arithmetic
 * as the kernels (gf128.hpp); never used on hypercube-sized data. */
int bn_scalar_mul(const bn_f128 *a, const bn_f128 *b, bn_f128 *out);
int bn_scalar_invert(const bn_f128 *a, bn_f128 *out);

/* ---- measurement plumbing: time the launches enqueued between begin and end with hipEvents on
 * the context's stream.  Not part of the reference interface. */
int bn_timer_begin(bn_ctx *ctx);
int bn_timer_end_ms(bn_ctx *ctx, float *ms);
/* 32 elements of fine-grained pinned host memory, readable by kernels through *d_ptr: a handful of
 * elements can be handed to the device without an upload.  Not part of the reference interface. */
int bn_host_scratch(bn_ctx *ctx, void **h_ptr, void **d_ptr, uint64_t *elems);
/* NUMA node of the host the device hangs off (its PCI function's numa_node in sysfs), -1 if the platform does not say.
 * A small round is a host -> device -> host round trip (the armed kernels of csrc/arm.hpp poll pinned host memory and
 * answer into it): from a core of the other socket every such trip crosses the socket interconnect as well -- measured
 * 15.0 against 17.1 us per two-round launch on a 2-socket host -- so the thread that drives a context should run on this
 * node.  The library never changes an affinity itself.  Not part of the reference interface. */
int bn_device_numa_node(int device, int *node);

/* out[i] = XOR over g < n_groups of d_vals[g * group_len + i], i < group_len <= 64, returned to the
 * host.  Not part of the reference interface: the combine step behind the per-round all_gather of
 * the multi-GPU prover (RCCL has no XOR reduction). */
int bn_xor_reduce(bn_ctx *ctx, const void *d_vals, uint32_t n_groups, uint32_t group_len, bn_f128 *h_out);

/* ---- Cross-rank reduction of round evaluations inside the kernel's finalize step (one process
 * per GPU, the hypercube sharded on the last-bound variables; the only exchange of a sumcheck round is one partial
 * (y_1, y_inf) per rank -- crates/core/src/protocols/sumcheck/v3/bivariate_product.rs:303-408 is a sum over hypercube
 * points, so the shards' sums add).  Not part of the reference interface.
 *   bn_peer_create   allocates this rank's mailbox (BN_PEER_MAILBOX_BYTES of fine-grained device memory) and returns
 *                    its hipIpc handle (BN_PEER_HANDLE_BYTES) for the caller to hand to the other ranks of the node
 *   bn_peer_connect  maps every rank's mailbox (handles[world][BN_PEER_HANDLE_BYTES], rank-major; the own entry is
 *                    ignored) -- same-device peers on a one-GPU box, xGMI peers on a node
 *   bn_peer_set_active(1)  from now on every bn_kernel_launch that returns values to the host (h_out)
 *                    returns the XOR over all ranks of the values it would have returned alone: the finalizing workgroup
 *                    stores its values into every peer's mailbox, waits for the world's, XORs (csrc/finalize.hpp
 *                    peer_exchange).  All ranks must issue the same sequence of such launches.  Values declared with a
 *                    non-zero initial value are XORed in once per rank.  (0): back to local results (e.g. for the residual
 *                    rounds every rank runs identically).
 *   bn_peer_stats    stats[0] = reduced launches so far */
enum { BN_PEER_HANDLE_BYTES = 64, BN_PEER_MAX_WORLD = 16, BN_PEER_MAILBOX_BYTES = 2 * 16 * 24 * 8 };
int bn_peer_create(bn_ctx *ctx, uint32_t world, uint32_t rank, uint8_t *handle_out /*[BN_PEER_HANDLE_BYTES]*/);
int bn_peer_connect(bn_ctx *ctx, const uint8_t *handles /*[world][BN_PEER_HANDLE_BYTES]*/);
int bn_peer_set_active(bn_ctx *ctx, int on);
int bn_peer_stats(bn_ctx *ctx, uint64_t *stats /*[2]*/);
/* The host tail under a peer exchange (sharded sumcheck): once the arrays of a shard are down to <= 2^12 (2^8) elements the library
 * takes the remaining rounds onto the host (BN_ARM_HT_*), where the ranks' partial sums cannot meet on the devices any more.
 * A caller that exchanges the partials of those rounds ITSELF (host shared memory: binius_amd/host/host_capi.cpp) says so with
 * bn_host_tail_allow_peer(ctx, 1); after every reduced launch it asks bn_host_tail_active, and from the launch that answers 1 on
 * it switches the peer exchange off (bn_peer_set_active(ctx, 0): no flush while the tail is active) and combines what
 * bn_kernel_launch returns -- this rank's LOCAL sums -- across the ranks.  Without the permission a context with an active peer
 * exchange never starts a host tail. */
int bn_host_tail_allow_peer(bn_ctx *ctx, int on);
int bn_host_tail_active(bn_ctx *ctx, int *active);
int bn_peer_destroy(bn_ctx *ctx);

/* ---- Merkle commitment of a BinaryField128b vector with Groestl-256.
 * BinaryMerkleTreeProver::commit (crates/core/src/merkle_tree/prover.rs:47-62) =
 * binary_merkle_tree::build (binary_merkle_tree.rs:27-101) with H = Groestl256
 * (crates/hash/src/groestl/digest.rs:30-87) and C = Groestl256ByteCompression
 * (crates/hash/src/groestl/compression.rs:21-36), which the FRI prover runs on the host copy of every
 * folded codeword (crates/core/src/protocols/fri/prove.rs:395-420).
 * Leaf i = Groestl-256 of the canonical serialization (16 little-endian bytes per element,
 * crates/utils/src/serialization.rs:94-104) of elements [i * batch_size, (i + 1) * batch_size).
 * d_nodes receives the flattened tree, (2 * n_leaves - 1) digests of 32 bytes = 2 * (2 * n_leaves - 1)
 * arena elements, leaves first, root last (binary_merkle_tree.rs:22-25).  No synchronisation.
 * Errors as the reference: n_elems % batch_size != 0 -> "IncorrectBatchSize", leaf count not a power
 * of two -> "PowerOfTwoLengthRequired" (both BN_ERR_INPUT_VALIDATION). */
int bn_merkle_build(bn_ctx *ctx, const void *d_elems, uint64_t n_elems, uint64_t batch_size, void *d_nodes);
/* hash_interleaved alone (binary_merkle_tree.rs:175-211): d_digests[i] = Groestl-256(batch i), 32 B each. */
int bn_groestl256_leaves(bn_ctx *ctx, const void *d_elems, uint64_t n_elems, uint64_t batch_size, void *d_digests);
/* compress_layer alone (binary_merkle_tree.rs:158-168): d_next[i] = C(d_prev[2i], d_prev[2i+1]), i < n_out. */
int bn_groestl256_compress_layer(bn_ctx *ctx, const void *d_prev, uint64_t n_out, void *d_next);

/* Openings of a committed vector: h_out[i * item_elems + e] = d_src[h_offsets[i] + e] (offsets and
 * lengths in 16-byte elements), e < item_elems, i < n_items, in one kernel and one synchronisation.
 * Not part of the reference interface: the reference reads branches and cosets out of host copies
 * (binary_merkle_tree.rs:121-141, fri/prove.rs:631-661); here the tree and the codewords stay on the
 * device and only what a query opens is read back. */
int bn_gather_d2h(bn_ctx *ctx, const void *d_src, const uint64_t *h_offsets, uint64_t n_items, uint64_t item_elems, bn_f128 *h_out);

/* Per-kernel-class timing without perturbing the stream: while profiling is on, every launch of a
 * hot kernel is bracketed by two hipEvents recorded on the context's stream (no synchronisation);
 * bn_prof_end synchronises once and sums the elapsed times per class. */
enum { BN_PROF_ROUND_EVAL = 0, BN_PROF_FOLD = 1, BN_PROF_TENSOR_EXPAND = 2, BN_PROF_NTT = 3, BN_PROF_OTHER = 4, BN_PROF_FOLD_EVAL = 5, BN_PROF_TAIL = 6, BN_PROF_FOLD_EVAL_SMALL = 7, BN_PROF_FOLD_EVAL_MFMA = 8, BN_PROF_ROUND_EVAL_MFMA = 9, BN_PROF_FOLD_EVAL8 = 10, BN_PROF_N = 11 };
int bn_prof_begin(bn_ctx *ctx);
int bn_prof_end(bn_ctx *ctx, double *ms_by_class /*[BN_PROF_N]*/, uint64_t *launches_by_class /*[BN_PROF_N]*/);

/* Armed rounds (binius_amd/csrc/arm.hpp): behind the fused fold + evaluation kernel of a small sumcheck round the
 * dispatcher enqueues the kernel of the NEXT round, which waits on the device for its challenge; the caller's next
 * extrapolate_line + accumulate_kernels pair then costs a write to pinned memory instead of a launch.  Purely an
 * execution detail of bn_extrapolate_line_batch + bn_kernel_launch (the results are those of the unarmed path; BN_ARM=0
 * turns it off).  Counters since context creation: rounds served by an armed kernel, armed kernels that were cancelled
 * because the next call was something else, armed kernels that gave up waiting; host nanoseconds between handing over
 * a challenge and seeing the round's result, the part of that spent enqueueing the next armed kernel, and the time from
 * the entry of bn_kernel_launch to handing the challenge over (validation + recognising the round).
 * BN_ARM_HT_*: the host tail -- once the arrays of a bivariate sumcheck are down to <= 2^12 (2^8) elements the two-round kernel
 * hands them to the host and the remaining evaluations and folds are host arithmetic (PCLMULQDQ in an isomorphic power
 * basis), the device catching up with one launch; instances taken over, evaluations answered, catch-up launches, and (not a
 * counter) the largest array the host takes over: 2^12 elements when the host has VPCLMULQDQ (four products per instruction),
 * else 2^8; 0 when the host tail is off.  BN_HOST_TAIL=0 turns it off.  Like arming, an execution detail of the unchanged call
 * sequence. */
enum { BN_ARM_HITS = 0, BN_ARM_CANCELS = 1, BN_ARM_EXPIRED = 2, BN_ARM_NS_WAIT = 3, BN_ARM_NS_LAUNCH = 4, BN_ARM_NS_PARSE = 5, BN_ARM_HOSTED = 6, BN_ARM_TWO_ROUND = 7, BN_ARM_SHADOW_CREATED = 8, BN_ARM_SHADOW_ROUNDS = 9, BN_ARM_SHADOW_DROPPED = 10, BN_ARM_HT_STARTED = 11, BN_ARM_HT_ROUNDS = 12, BN_ARM_HT_FLUSHED = 13, BN_ARM_HT_MAX = 14, BN_ARM_N = 15 };
int bn_arm_counters(bn_ctx *ctx, uint64_t *counters /*[BN_ARM_N]*/);
/* Claim groups (not part of the reference interface: counters of how the backend ran the call shape of piop::prove --
 * k product claims over m multilinears per BivariateSumcheckProver, several provers front-loaded on one layer,
 * core/src/piop/prove.rs:271-287, protocols/sumcheck/prove/front_loaded.rs:122-155).  LAUNCHES: launches of the group kernel
 * (each answers one execute() and computes ahead for the other waiting provers); JOBS_FUSED / JOBS_EVAL: claims evaluated
 * together with the fold of their two arrays / on arrays folded by a plain launch (shared arrays, round 0); PREFOLDS: those
 * plain fold launches; SPEC_JOBS: claims of OTHER provers carried by a launch; SPEC_HITS: execute() calls answered from sums
 * computed ahead, without a launch; EVALS: execute() calls answered on this path; FLUSHED_FOLDS: deferred fold batches that a
 * foreign call forced out as plain launches. */
/* HOSTED_*: provers whose arrays were small enough to finish on the host (started), execute() / fold() calls performed
 * there, write-backs of the host's folded copies launched.  JOBS_FOLD: fold-only jobs of the group launches (arrays shared by
 * several claims or in none, folded inside the launch); CHAINS: groups of jobs run by one set of workgroups one after the other
 * (folds first, then the evaluations that read them back). */
enum { BN_GROUP_LAUNCHES = 0, BN_GROUP_JOBS_FUSED = 1, BN_GROUP_JOBS_EVAL = 2, BN_GROUP_PREFOLDS = 3, BN_GROUP_SPEC_JOBS = 4, BN_GROUP_SPEC_HITS = 5, BN_GROUP_EVALS = 6, BN_GROUP_FLUSHED_FOLDS = 7, BN_GROUP_HOSTED_STARTED = 8, BN_GROUP_HOSTED_EVALS = 9, BN_GROUP_HOSTED_FOLDS = 10, BN_GROUP_HOSTED_WRITEBACKS = 11, BN_GROUP_JOBS_FOLD = 12, BN_GROUP_CHAINS = 13, BN_GROUP_N = 14 };
int bn_group_counters(bn_ctx *ctx, uint64_t *counters /*[BN_GROUP_N]*/);
/* The wave-specialised FP4 kernels keep sums of GF(2) products as counts in f32 accumulators, exact while a workgroup sees at
 * most 2^14 tiles (2^22 points) per launch; their launchers refuse a grid beyond that bound (also one asked for through the test
 * switches BN_FP4_WS_GRID / BN_FE_FP4_GRID).  Read-only, process-wide: how the LAST FP4 round evaluation and the LAST fused FP4
 * fold + evaluation were launched -- workgroups, the largest number of tiles a workgroup took, and for the round evaluation which
 * form ran (1: stager / Gram waves, 0: three workgroups per CU); *_MAX_TILES: the largest share of a workgroup in any such launch
 * of the process so far; zeros before the first such launch. */
enum { BN_FP4_RE_GRID = 0, BN_FP4_RE_TILES = 1, BN_FP4_RE_WS = 2, BN_FP4_FE_GRID = 3, BN_FP4_FE_TILES = 4, BN_FP4_RE_MAX_TILES = 5, BN_FP4_FE_MAX_TILES = 6, BN_FP4_N = 7 };
int bn_fp4_last_grids(bn_ctx *ctx, uint64_t *grids /*[BN_FP4_N]*/);
/* Which kernel family served the bn_ntt_forward / bn_ntt_inverse calls of this context since it was created: the bit-sliced
 * kernels (B32 twiddles, log_y >= 14), the LDS-tiled kernel (B8 .. B32 twiddles, B16 .. B128 elements, 2^12 elements and more) or the
 * per-layer kernel (everything else).  Read-only; a call that is rejected, or an accepted no-op (log_y == 0, skip_rounds == log_y),
 * counts nowhere. */
enum { BN_NTT_CALLS_BS = 0, BN_NTT_CALLS_TILED = 1, BN_NTT_CALLS_LAYER = 2, BN_NTT_N = 3 };
int bn_ntt_counters(bn_ctx *ctx, uint64_t *counters /*[BN_NTT_N]*/);
/* The passes that the bn_fri_fold calls of this context have launched since it was created, by form: one challenge per pass
 * (PASS_ONE), two or three interleave challenges in one pass (PASS_INTER2 / PASS_INTER3), two challenges in one pass of which at least
 * one is a fold round with its butterfly (PASS_NTT2: B8 .. B32 twiddles, 2^14 elements and more), three such (PASS_NTT3: a measurement
 * form that the normal build never launches), and the calls with no challenge at all, which are one copy (COPIES).  Read-only; a
 * rejected call counts nowhere. */
enum { BN_FRI_PASS_ONE = 0, BN_FRI_PASS_INTER2 = 1, BN_FRI_PASS_INTER3 = 2, BN_FRI_PASS_NTT2 = 3, BN_FRI_PASS_NTT3 = 4, BN_FRI_COPIES = 5, BN_FRI_N = 6 };
int bn_fri_counters(bn_ctx *ctx, uint64_t *counters /*[BN_FRI_N]*/);
/* Which kernel answered the bn_fold_right / bn_fold_left calls of this context since it was created: fold_right on the matrix cores
 * (RIGHT_MFMA: rows of 512 / 1024 / 2048 bits, 4096 outputs and more), by the nibble-table kernel (RIGHT_TAB: B8 .. B32 entries, 1024
 * outputs and more) or by the scalar kernel (RIGHT_SCALAR); fold_left handed to the partial-evaluation kernel (LEFT_PE: at most 1024
 * outputs under a vector of 4096 elements and more; bn_partial_eval_counters counts the same calls as FOLD_LEFT_ROUTED), on the matrix
 * cores (LEFT_MFMA: B32 entries, 16 / 32 / 64 vector elements, 4096 outputs and more), by the nibble-table kernel (LEFT_TAB) or by
 * the scalar kernel (LEFT_SCALAR).  Every accepted call counts in exactly one of the seven.  RING2 / RING4 / RING8 and RING_LEFT2 /
 * RING_LEFT4 / RING_LEFT8 split the matrix-core calls by the kernel's row width in 256-bit units; LAST_GRID and LAST_PREP are the
 * workgroups of the last matrix-core launch and the tower level of its table preparation (0 before the first); N_CU is the number of
 * compute units of the context's device, which the launchers size their grids by (a matrix-core fold: at most two workgroups per unit,
 * the scalar kernel: at most eight).  Read-only; a rejected call moves nothing. */
enum {
	BN_FOLD_RIGHT_MFMA = 0, BN_FOLD_RIGHT_TAB = 1, BN_FOLD_RIGHT_SCALAR = 2, BN_FOLD_LEFT_PE = 3, BN_FOLD_LEFT_MFMA = 4, BN_FOLD_LEFT_TAB = 5,
	BN_FOLD_LEFT_SCALAR = 6, BN_FOLD_RING2 = 7, BN_FOLD_RING4 = 8, BN_FOLD_RING8 = 9, BN_FOLD_RING_LEFT2 = 10, BN_FOLD_RING_LEFT4 = 11,
	BN_FOLD_RING_LEFT8 = 12, BN_FOLD_LAST_GRID = 13, BN_FOLD_LAST_PREP = 14, BN_FOLD_N_CU = 15, BN_FOLD_N = 16
};
int bn_fold_counters(bn_ctx *ctx, uint64_t *counters /*[BN_FOLD_N]*/);
/* Which kernel answered the bn_inner_product calls of this context: the F x F split sum on the matrix cores (MFMA_SPLIT: level 7, even
 * length, at least one 256-point tile per CU in each half), the 9-lane split kernel (SPLIT9: level 7, every other even length), the
 * bit-sliced B32 kernel (IP32: level 5, 8192 elements and more, a multiple of 512) or the scalar kernel (SCALAR: everything else).
 * Read-only; a rejected call counts nowhere. */
enum { BN_IP_MFMA_SPLIT = 0, BN_IP_SPLIT9 = 1, BN_IP_IP32 = 2, BN_IP_SCALAR = 3, BN_IP_N = 4 };
int bn_inner_product_counters(bn_ctx *ctx, uint64_t *counters /*[BN_IP_N]*/);
/* Which route answered the bn_hal_round_evals calls of this context, and which branches ran inside it.  One counter per route -- COEF
 * (the coefficient form), EQ_SET (a constraint set's two launches), IN_PARTS (a wide request dealt out; every part comes back through
 * the entry point and counts under the route that answered it), MONOMIALS (one product-sum pass per distinct monomial), ROWS_BATCHED /
 * ROWS_PER_POINT (rows + compiled circuits, the points side by side up to 2^19 points a row / point by point above), INTERPRETER --:
 * requests the route answered with BN_OK; a request that asks for no value counts nowhere.  The jobs of the monomial route by kind:
 * MONO_STRIDED (Low-to-High pairs read with an element stride of two by the matrix-core kernel), MONO_PRODUCT2 / MONO_PRODUCT3 (the
 * product-sum kernels over two / three factors, the indicator and the all-ones table counted), MONO_XOR_SUM (launches of the streaming
 * sum of a lone column from 2^18 points: one, or three where a form at infinity holds the column), MONO_CONST (constants without an
 * indicator: no pass).  ROWS_LAUNCHES / ROWS_WRITTEN: launches of the rows kernel and the rows they wrote (at most 24 a launch);
 * ROWS_IN_PLACE: halves of full multilinears read where they lie.  TRANSPARENT: Transparent multilinears partially evaluated into
 * scratch.  N_CU: the compute units of the device, by which the launchers size their grids and the matrix-core threshold is set.
 * Counted on the host where the route is decided; read-only; a call that returns an error moves nothing. */
enum {
	BN_HALCNT_COEF = 0, BN_HALCNT_EQ_SET = 1, BN_HALCNT_IN_PARTS = 2, BN_HALCNT_MONOMIALS = 3, BN_HALCNT_ROWS_BATCHED = 4,
	BN_HALCNT_ROWS_PER_POINT = 5, BN_HALCNT_INTERPRETER = 6, BN_HALCNT_MONO_STRIDED = 7, BN_HALCNT_MONO_PRODUCT2 = 8, BN_HALCNT_MONO_PRODUCT3 = 9,
	BN_HALCNT_MONO_XOR_SUM = 10, BN_HALCNT_MONO_CONST = 11, BN_HALCNT_ROWS_LAUNCHES = 12, BN_HALCNT_ROWS_WRITTEN = 13, BN_HALCNT_ROWS_IN_PLACE = 14,
	BN_HALCNT_TRANSPARENT = 15, BN_HALCNT_N_CU = 16, BN_HALCNT_N = 17
};
int bn_hal_counters(bn_ctx *ctx, uint64_t *counters /*[BN_HALCNT_N]*/);

#ifdef __cplusplus
}
#endif
#endif /* BINIUS_AMD_H */
