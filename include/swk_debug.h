/*
 * swk_debug.h -- A/B switches, profiling hooks and diagnostics of libswk.so.
 *
 * Nothing in here belongs to the drop-in boundary (swk.h): a maintainer who binds the reference's call surface never calls these.
 * They exist for the measurements (bench.py, tools/), for the cross-checks of the GPU tests (every IALM pass variant and both
 * small-matrix solvers against the CPU restatement of the reference) and for the counters the bench line reports.  Results never depend on a switch: each one
 * selects between implementations that the tests hold to the same outputs.
 */
#ifndef SWK_DEBUG_H
#define SWK_DEBUG_H
#include "swk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement hooks -----------------------------------------------------------
 * With profiling on, every kernel launch of swk_batch_run is bracketed by HIP events on
 * the context's stream; swk_prof_get returns accumulated device time and launch count per
 * kernel family since the last swk_prof_reset (swk_yuv420_to_bgr's and swk_yuv_to_bgr's kernels count as SWK_K_GRAY, the colour conversions).  Family ids: */
enum {
    SWK_K_GRAY = 0, SWK_K_IALM_STATS = 1, SWK_K_IALM_PASS = 2, SWK_K_IALM_SMALL = 3,
    SWK_K_FILTER = 4, SWK_K_CCL = 5, SWK_K_PROPS = 6, SWK_K_COPY = 7, SWK_K_COUNT = 8
};
int32_t swk_prof_enable(swk_ctx *ctx, int32_t on);
int32_t swk_prof_reset(swk_ctx *ctx);
int32_t swk_prof_get(swk_ctx *ctx, int32_t family, double *ms_total, int64_t *launches);
/* Total IALM pass launches x windows still active, i.e. window-iterations streamed. */
int32_t swk_prof_window_iters(swk_ctx *ctx, int64_t *window_iters);
/* Select the IALM pass kernel: 0 = auto (4, or 2 when A / E are requested, 6 above 64 frames), 1 = LDS/VALU kernel with one wave per
 * 64-pixel tile, 6 = the same kernel with four waves per tile (and the small-matrix step of long windows), accepted for any n: the
 * tests compare it with 1, 2 = MFMA f64 kernel carrying A and Y, 4 = MFMA f64 kernel carrying M alone (21-22 instead of 34 B per element and
 * iteration; produces the sparse u8 image and the iteration count, not A / E), instantiated per 4-frame k-step with a
 * software-pipelined tile loop, 5 = 4 without the pipeline (its cross-check).  3 (round 1's M-state kernel, one instantiation
 * per 16-frame block) is gone: SWK_ERR_ARG.  For A/B measurements and cross-checks only. */
int32_t swk_set_ialm_variant(swk_ctx *ctx, int32_t variant);
/* k-step-templated M-state pass (variants 4 / 5): bit 0 = the wave in the odd hardware slot of each SIMD runs at raised
 * priority (breaks the lockstep of the two co-resident waves), bit 1 = it also starts late.  A/B knob; results never
 * depend on it. */
int32_t swk_set_pass_tuning(swk_ctx *ctx, int32_t flags);
/* M-state pass only: the per-iteration stores of the sparse u8 image start once ||Z||_F < factor * tol * ||X||_F
 * (default 16; <= 0 = every pass).  A window that stops although the pass before its last iteration skipped the
 * stores makes the library run the batch again without the speculation, so results never depend on the factor;
 * swk_prof_redo_batches counts those reruns. */
int32_t swk_set_sparse_speculation(swk_ctx *ctx, double factor);
/* M-state pass only: while the last formed ||Z||_F is >= factor * tol * ||X||_F (default 256; <= 0 = never) the
 * stopping norm is formed every other iteration only (the f16 copy of Y/mu is neither written nor read in between).
 * In between, the norm over frames 0..3 is still formed: a lower bound that proves the skipped iteration did not
 * stop; a window where it cannot is rerun like above.  After a rerun the guess that failed stays off for the next
 * 64 batches of the context (the windows of one video behave alike). */
int32_t swk_set_norm_speculation(swk_ctx *ctx, double factor);
/* M-state pass only: the stopping test ||Z||_F < tol ||X||_F (image_filtering.py:297) is made on a float32 sum over a binary16 copy
 * of Y/mu (relative error about 1e-6).  A window whose ratio ||Z|| / (tol ||X||) comes within `rel` of 1 (default 1e-3; 0 = off) is
 * not decided on that number: it is run again, alone, by the A/Y-state pass, whose norm is formed in float64 like the reference's.
 * swk_prof_guard_windows counts those windows. */
int32_t swk_set_norm_guard(swk_ctx *ctx, double rel);
int32_t swk_prof_guard_windows(swk_ctx *ctx, int64_t *windows);
/* Diagnostic of the same decision: for every window of the last swk_batch_run / swk_ialm (up to cap) the ratio ||Z||_F / ||X||_F of its
 * LAST stopping test (image_filtering.py:297) and, for the M-state pass, the bound on that number's relative error the band is held
 * against (float32 sum over a binary16 copy of Y/mu: csrc/ialm_small_dev.h; the effective band is max(rel, 4 x bound) per window).
 * Returns the number of windows of that batch (negative: error).  The A/Y-state pass forms the norm in float64: bound 0. */
int32_t swk_last_stopping_norms(swk_ctx *ctx, double *ratio, double *err_bound, int32_t cap);
/* Pass variants 1, 2, 4 and 5 (variant 6 always takes the f64 start pass): 1 (default) = statistics and the first iteration's
 * Gram matrix come from one read of X on the integer matrix cores wherever the first shrinkage provably removes nothing;
 * 0 = always the f64 start pass. */
int32_t swk_set_integer_start(swk_ctx *ctx, int32_t on);
/* Windows of the last swk_batch_run / swk_ialm whose start came from the integer kernel (the others ran the f64 start pass). */
int32_t swk_last_integer_start_windows(swk_ctx *ctx, int32_t *windows);
/* Diagnostic: the start of the IALM alone, on nwin host windows X[nwin][n][P] (u8), staged like swk_ialm's window and run with the
 * context's current switches (swk_set_ialm_variant, swk_set_integer_start): statistics and, where it may run, the integer Gram
 * kernel; the start choice; the start pass of the selected variant; the chip-wide slab sum when a window has more than 4 slabs.
 * Returns what the first small-matrix step would read, per window:
 *   G[nwin][n][n]   the Gram slabs summed in that step's order, frame-block pairs below the diagonal mirrored, UNSCALED: the exact
 *                   integer X^T X where int_gram is 1, M_1^T M_1 of the f64 start pass otherwise (zeros for an all-zero window,
 *                   which is done before it starts);
 *   sumsq, maxv     exact sum of squares and maximum of the window;
 *   int_gram        1 = the window starts from the integer kernel's matrix;
 *   scal[nwin][4]   dual_norm, mu_0, thr_0 = lmbda / mu_0, dnorm (image_filtering.py:271-276);
 *   *nblk_out       Gram slabs per window of this batch, *gram8_ran = 1 when the integer kernel ran for the batch.
 * Every output but G may be NULL.  No IALM iteration runs; the counters of the context do not move. */
int32_t swk_debug_ialm_start(swk_ctx *ctx, const uint8_t *X, int32_t nwin, int32_t n, int32_t P, double lmbda, double *G,
                             uint64_t *sumsq, uint32_t *maxv, int32_t *int_gram, double *scal, int32_t *nblk_out, int32_t *gram8_ran);
/* Diagnostic: the start and the first step of the IALM alone, on nwin host windows X[nwin][n][P] (u8), staged and checked like
 * swk_debug_ialm_start's and run with the context's current switches (swk_set_ialm_variant, swk_set_integer_start, swk_set_eig_method,
 * swk_set_start_refine): the start, then what the chain runs next through the same helper -- the chip-wide slab sum when a window has
 * more than 4 slabs, the small-matrix step of k = 0 (k_ialm_small, or k_ialm_small_wide above 64 frames and under variant 6) and, with
 * the refinement on, the accurate first iteration of the windows that step flagged (csrc/ialm_refine.hip).  Per window:
 *   B_fin[nwin][n][n]  B_1 = I - W / mu_0 as iteration 1's pass reads it: A_1 = M_1 B_1 with M_1 pixels x frames, B_1 row-major (NOT
 *                      symmetric where the window was refined);
 *   B_std[nwin][n][n]  the same matrix as the small-matrix step left it, copied before the refinement is launched;
 *   refine             0 = not asked for, 2 = refined, 3 = given up (rank deficient or not converged), 4 = over the work cap of the
 *                      double-double Gram matrix from the pixels;
 *   cond_sum           the step's estimate ||G_1||_F sum_i 1 / lambda_i (0 from k_ialm_small_wide, which makes none);
 *   sweeps             solver steps of k = 0: Newton-Schulz iterations, or 100 + Jacobi sweeps;
 *   int_gram, scal[nwin][4]   as swk_debug_ialm_start returns them.
 * Every output but B_fin may be NULL.  No pass of an iteration runs; the counters of the context do not move. */
int32_t swk_debug_ialm_first_step(swk_ctx *ctx, const uint8_t *X, int32_t nwin, int32_t n, int32_t P, double lmbda, double *B_fin,
                                  double *B_std, int32_t *refine, double *cond_sum, int32_t *sweeps, int32_t *int_gram, double *scal);
/* Diagnostic: how each group of the last swk_batch_run / swk_batch_run_groups reached the device, one value per group (up to cap):
 * 0 = one copy of a packed ROI, 1 = the whole buffer as it lies, read at (x0, y0) with the caller's strides, 2 = one copy per frame
 * (full-width rows), 3 = one 2-D copy per frame; -1 = a device group, read in place.  Returns the number of groups of that call (0 before
 * the first; a refused call leaves the previous call's values; negative: error). */
int32_t swk_last_host_stage(swk_ctx *ctx, int32_t *kinds, int32_t cap);
/* Diagnostic: iterations the G^(-1/2) solver took in the LAST small-matrix step of the last batch, maximum over its
 * windows: Newton-Schulz iterations, or 100 + Jacobi sweeps where that solver ran. */
int32_t swk_last_eig_sweeps(swk_ctx *ctx, int32_t *sweeps);
int32_t swk_prof_redo_batches(swk_ctx *ctx, int64_t *batches);
/* ... and the windows that were run again for it (only the windows whose guess failed run again, together, with the guesses off). */
int32_t swk_prof_redo_windows(swk_ctx *ctx, int64_t *windows);
/* M-state pass: algorithmic bytes per matrix element moved by all its launches since swk_prof_reset, summed over
 * windows (each window-iteration counts X 1 + M 8 (+8 read) + U 2 or 1/8 each way + 1 when the sparse image is
 * stored); multiply by n*P for bytes.  Meaningful for the M-state pass only. */
int32_t swk_prof_pass_bytes_per_element(swk_ctx *ctx, double *bytes);
/* G^(-1/2) of the n x n Gram matrix: 0 = coupled Newton-Schulz on the f64 matrix cores (default; falls back
 * to Jacobi by itself if it does not converge), 1 = cyclic Jacobi eigen-solve. */
int32_t swk_set_eig_method(swk_ctx *ctx, int32_t method);

/* Accurate first iteration of ill-conditioned windows (csrc/ialm_refine.hip).  The Gram-matrix route squares cond(M); in iteration 1
 * (M_1 = c X, 1/mu largest) that costs about eps * cond(G_1) / mu_0 in A, and windows of few pixels and many frames carry that error
 * to the end.  A window whose estimate eps * ||G_1||_F sum_i 1/lambda_i / mu_0 exceeds `tau` (default 1e-5; <= 0 = never) gets B_1
 * from a double-double Cholesky factor of the exact integer X^T X (of a double-double M_1^T M_1 where the first shrinkage clips)
 * instead.  swk_prof_refined_windows: windows refined / wanted but given up (rank deficient, or too large for one workgroup's
 * double-double Gram matrix) since the context was made. */
int32_t swk_set_start_refine(swk_ctx *ctx, double tau);
int32_t swk_prof_refined_windows(swk_ctx *ctx, int64_t *refined, int64_t *unrefined);

/* Diagnostic: the resize tables the classifier-input kernels form on the device (Pillow's antialiased bilinear coefficients for 24 output
 * samples, 22-bit fixed point) for the input sizes first .. first + count - 1:
 *   bounds[count][24][2]    first input sample and number of coefficients of each output sample;
 *   coeffs[count][24][343]  the coefficients, zeros behind each sample's last.
 * route 1 = as the large-crop kernel of swk_segment_inputs forms them (weights summed in one sweep, formed again in a second; sizes 1..4096),
 * route 0 = as the kernels of crops up to 512 pixels form them (sizes 1..512).  The tests hold both to the float64 restatement of
 * Pillow, integer for integer: a fused multiply-add or another summation order in the device code would show here. */
int32_t swk_debug_resize_table(swk_ctx *ctx, int32_t first, int32_t count, int32_t route, int32_t *bounds, int32_t *coeffs);

/* Diagnostic: the fused filter kernel of the batch calls (csrc/filters.hip, k_filter_fused<GEOM, R>: bilateral filter, to-zero
 * threshold, 3 x 3 grey opening) alone, on u8 planes the CALLER chooses -- in a batch call it only ever reads what the RPCA left.  The
 * planes go to the device and through the launcher swk_batch_run takes (planes == NULL: count planes of H x W pixels, densely packed,
 * src and every output count * H * W bytes) or the one swk_batch_run_groups takes (planes[count] = size of every plane and its byte
 * offset in src, a buffer of `total` bytes; the outputs are `total` bytes with the same layout, bytes that belong to no plane come back
 * 0), with p's bil_d, bil_sigma_color, bil_sigma_space, bil_fma and thresh.  bilateral and thresh may be NULL: the launcher is then
 * handed a null pointer for that stage, as in a batch call that does not ask for it.  Before the launch every device output and
 * SWK_DEBUG_GUARD_BYTES behind it are filled with SWK_DEBUG_FILL; guard (may be NULL) receives 3 x SWK_DEBUG_GUARD_BYTES: the bytes
 * behind the opened, the bilateral and the thresholded planes as the launch left them (SWK_DEBUG_FILL where the output is NULL).
 * SWK_ERR_ARG, before any buffer or launch, by the batch calls' own rules: a plane below 4 x 4, a radius above 4, an opening window
 * other than (3, 3), planes that overlap or leave the buffer. */
#define SWK_DEBUG_GUARD_BYTES 64
#define SWK_DEBUG_FILL 0xA5
typedef struct swk_debug_plane { int32_t H, W; int64_t off; } swk_debug_plane;
int32_t swk_debug_filter_fused(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, const swk_debug_plane *planes,
                               int64_t total, const swk_params *p, uint8_t *bilateral, uint8_t *thresh, uint8_t *opened, uint8_t *guard);
/* Diagnostic: the one-workgroup-per-frame labeller with region records (csrc/ccl.hip, k_ccl_frame<VEC, true>) alone, on count opened
 * planes of H x W pixels the caller chooses, through the launcher swk_batch_run takes: labels [count][H][W] (u8, label & 255),
 * segs [count][seg_cap] (zeros behind a frame's last record), nseg [count] (every live label value, also above seg_cap).
 * SWK_ERR_ARG for a frame size the kernel does not take (no fall-back to the multi-kernel path), connectivity other than 4 or 8,
 * seg_cap outside 1..255. */
int32_t swk_debug_ccl_frame_props(swk_ctx *ctx, const uint8_t *opened, int32_t count, int32_t H, int32_t W, int32_t connectivity,
                                  int32_t label_order, int32_t seg_cap, uint8_t *labels, swk_segment *segs, int32_t *nseg);

/* Labelling route of swk_ccl_u8, swk_batch_run and swk_batch_run_groups: on = every frame size takes the multi-kernel labeller
 * (csrc/ccl.hip: k_ccl_init / union / flatten / wordprefix / label through launch_ccl, and k_props* through launch_regionprops where a
 * batch call wants records), which otherwise only runs for frames the one-workgroup kernel does not take; 0 (default) = each frame size's
 * own route.  swk_debug_ccl_frame_props is unaffected.  Results never depend on it: the tests run the small pattern frames and more
 * than 32768 frames through the path that way. */
int32_t swk_debug_force_ccl_multi_kernel(swk_ctx *ctx, int32_t on);
/* The largest window count of one IALM (sub-)batch that the context's device takes (swk.h, "Windows per call"): its grid y extent,
 * hipDeviceAttributeMaxGridDimY, read once when the context is made.  Negative: error. */
int32_t swk_debug_max_windows(swk_ctx *ctx);

/* White-box hook of the window tracker's tests: after skip_frames more frames, the next frame that swk_track_window steps takes
 * col4row[n] (n = its previous plus its current segments, each entry in [0, n)) instead of the solver's assignment -- the one way to an
 * assignment that leaves a current segment without a status (SWK_ERR_TRACK_STATUS), which no optimal solver returns.  Used up by that
 * frame; SWK_ERR_ARG from swk_track_window when n is not that frame's size. */
int32_t swk_debug_tracker_force_assignment(swk_tracker *t, int32_t skip_frames, const int32_t *col4row, int32_t n);

/* ---- classifier kernels: A/B switches ---- */
/* Measurement knobs of the classifier kernels (A/B runs).  knob 0: workgroup layout of the 1 x 1 kernel (0 = 16-wave workgroups, the
 * default; 1 = 8 waves with the deepest activation ring that fits; results do not depend on it).  knob 1, the Fire modules' expand1x1
 * shapes: 0 = the float32 kernel; 1 = the split-bf16 kernel with its weights in LDS (float32 products as six bf16 MFMA products of
 * three-way split operands: float32-accurate, another summation order than the float32 kernel's); 2 = the split-bf16 kernel with its
 * weights in registers (the same results as 1, bit for bit); 3 = the default: each shape's own choice of these, the same at every batch
 * size (today 2 for all four shapes).  knob 2: workgroup layout of the split-bf16 Winograd 3 x 3 expands (results do
 * not depend on it, bit for bit): 0 = each shape's default, 1 = one column block and two tile groups of 32 tiles per wave for every
 * shape, 2 = two waves per column block sharing one filter slice (48 -> 192 as 12 waves, 64 -> 256 as 16, 32 -> 128 as 8 waves over 128
 * tiles) for every shape that has such a layout.  knob 4, conv1 and the wide plain squeezes (256 -> 48, 384 -> 48, 384 -> 64): 0 = the float32
 * kernel; 1 = the default: each shape's own choice, the same at every batch size (today the split-bf16 kernel with its weights in LDS
 * for conv1 and all three squeezes: float32-accurate, another summation order; environment default SWK_SQUEEZE_SPLIT_BF16, beside SWK_EXPAND_SPLIT_BF16
 * for knob 1).  Any other knob (3 included) or value: SWK_ERR_ARG. */
int32_t swk_set_cnn_tuning(int32_t knob, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* SWK_DEBUG_H */
