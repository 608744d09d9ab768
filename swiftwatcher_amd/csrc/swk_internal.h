// Internal declarations shared by the HIP translation units of libswk.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "swk.h"
#include "swk_debug.h"
#include "batch_plan.h"
#include "review_plan.h"

namespace swk {

constexpr int kMaxN = 64;          // frames per window supported by the matrix-core IALM kernels
// kMaxNWide = 128 (batch_plan.h, where the batch plan refuses more): ... and by the plain f64 kernels that take over above kMaxN

// Kernels that take more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize, and the attribute
// belongs to the (kernel, device) pair: `mask` (one static per kernel instantiation) keeps a bit per device it has been
// set on, so a second context on another device of the same process gets it too.  A failure is parked in
// g_launch_error (one atomic for the process: launchers do not know a context) and surfaces at the next sync() of a context.
extern std::atomic<int> g_launch_error;
inline bool ensure_dyn_lds(const void *fn, size_t bytes, unsigned long long &mask)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev < 64 && ((mask >> dev) & 1ull)) return true;
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { g_launch_error = (int)e; return false; }
    if (dev < 64) mask |= 1ull << dev;
    return true;
}
inline void note_launch() { hipError_t e = hipGetLastError(); if (e != hipSuccess) g_launch_error = (int)e; }

// Division of a 31-bit dividend by a launch-invariant divisor as one multiply-high and a shift (a 64-bit integer division is some
// 150 vector instructions on gfx950, a 32-bit one 30 -- and in the matrix kernels every vector instruction is paid in MFMA time).
// For n < 2^31 and d >= 1: l = ceil(log2 d), mul = floor(2^(31+l) / d) + 1, n / d = umulhi(n, mul) >> (l - 1); d = 1 is the identity.
struct FastDiv {
    unsigned mul, shift, d;
    FastDiv() : mul(0), shift(0), d(1) {}
    explicit FastDiv(unsigned div) : mul(0), shift(0), d(div)
    {
        if (div > 1) {
            unsigned l = 0;
            while ((1ull << l) < div) ++l;
            mul = (unsigned)(((1ull << (31 + l)) / div) + 1);
            shift = l - 1;
        }
    }
    __host__ __device__ unsigned div(unsigned n) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return d == 1 ? n : __umulhi(n, mul) >> shift;
#else
        return n / d;
#endif
    }
};

// Per-window scalar state of the IALM loop (device resident).
struct IalmScal { double mu, inv_mu, thr; };
struct IalmWin {
    IalmScal cur;                  // mu of the iteration being finished (image_filtering.py:282-294)
    IalmScal nxt;                  // mu of the iteration being started  (:295)
    double dual_norm;              // :271
    double dnorm;                  // :275
    unsigned long long sumsq;      // exact sum of squares of the u8 window
    unsigned int maxv;
    int iter;                      // iterations completed
    int done;
    int sweeps;                    // Jacobi sweeps used by the last eigen solve (diagnostic)
    int ws, ws_prev;               // M-state pass: did / does the pass of this (the previous) iteration write the sparse image
    int redo;                      // the window has to be run again: bit 0 = the last iteration's sparse image was not
                                   // written, bit 1 = a partial norm could not rule out that an iteration was the last,
                                   // bit 2 = the float32 stopping norm fell inside the guard band around the tolerance: this
                                   // window alone is run again by the A/Y-state pass (float64 norm, like the reference)
    int ru, wu;                    // M-state pass: this pass reads / writes ALL of U (else frames 0..3 only)
    double last_ratio;             // last full ||Z||_F / ||X||_F that was formed
    int int_gram;                  // the Gram matrix of the first iteration came from k_gram_u8 (unscaled X^T X)
    unsigned long long pass_b16;   // algorithmic bytes per element moved by the passes 1..iter of this window, in 1/16 B
    double zf2;                    // ||(G/s)^(-1/2)||_F^2 of the last Newton-Schulz solve (0: none yet): where the next solve's bound starts
    double norm_err;               // M-state pass: bound on the relative error of the float32 / binary16 stopping norm at the last test
    double cond_sum;               // ||G_1||_F sum_i 1 / lambda_i(G_1) of the first solve (>= cond(G_1)): the ill-conditioning estimate
    int refine;                    // accurate first iteration (ialm_refine.hip): 0 not needed, 1 asked for by k_ialm_small (k = 0),
                                   // 2 done, 3 given up (rank deficient: the standard route's defined result stands),
                                   // 4 wanted but not done (a window without an integer start that is too large for one workgroup's
                                   // double-double Gram matrix)
};

struct IalmBuffers {
    const uint8_t *X;              // [nwin][n][P]
    double *A, *Y;                 // [nwin][n][P]
    uint8_t *S;                    // [nwin][n][P]
    uint8_t *Salt;                 // M-state pass: second sparse-image buffer (iteration parity), else null
    uint16_t *U;                   // M-state pass: Y/mu as binary16 (x 1/128) for the stopping norm, planes like A; b.A holds M
    double *E;                     // optional [nwin][n][P]
    double *Bm;                    // [nwin][n][n]   I - W/mu
    double *Vprev;                 // [nwin][n][n]   eigenvectors of the previous solve (warm start)
    double *gpart;                 // [nwin][nblk][n][n]
    double *zzpart;                // [nwin][nblk] partial sums of z^2; the M-state pass appends [nwin][nblk] largest |U_{k-1}| per block
    IalmWin *win;                  // [nwin]
    int *active;                   // device counter of windows not yet converged
    int nwin, n, P, nblk;
    double spec;                   // M-state pass: sparse image written only once ||Z|| < spec * tol * ||X|| (<= 0: always)
    int use_gram8;                 // k_gram_u8 ran: k_ialm_init decides per window whether its result stands
    double nspec;                  // M-state pass: ||Z|| formed every other iteration while above nspec * tol * ||X|| (<= 0: always)
    double guard;                  // M-state pass: relative half-width of the band around tol in which the float32 norm does
                                   // not decide (<= 0: off; the A/Y-state pass forms the norm in float64 and needs none)
    double refine;                 // a window whose estimated first-iteration error eps * cond_sum / mu_0 exceeds this gets the accurate
                                   // first iteration of ialm_refine.hip (<= 0: never)
    int nred;                      // Gram slabs the small-matrix kernel still has to sum (1 after k_gram_reduce)
    int fpad;                      // planes allocated per window in A, Y, E: n rounded up to 16
    int64_t pstride;               // plane pitch (elements) of A, Y, E: P rounded up to 16 -> 128-B aligned rows
    const PnWin *wpix;             // optional [nwin]: window w holds wpix[w].P real pixels, the rest of its P is zero padding
                                   // (swk_batch_run_groups); null: every window holds P
};

// ialm.hip
void launch_ialm_stats(hipStream_t s, const IalmBuffers &b);
void launch_ialm_init(hipStream_t s, const IalmBuffers &b, double lmbda);
// k = iteration number of the pass (0 = Gram-only start pass); variants 4 / 5 = M-state pass (no A/E outputs)
void launch_ialm_pass(hipStream_t s, const IalmBuffers &b, int mode, int variant, int k, int tune = 0);
// ialm_mstate.hip: the M-state pass instantiated per k-step count
void launch_ialm_pass_m(hipStream_t s, const IalmBuffers &b, int mode, int k, int tune, bool pipe);
int  ialm_mstate_fpad(int n);
void launch_select_sparse(hipStream_t s, const IalmBuffers &b);
// method: 0 = Newton-Schulz on the f64 matrix cores (Jacobi only as fallback), 1 = cyclic Jacobi
void launch_ialm_small(hipStream_t s, const IalmBuffers &b, int k, double lmbda, double tol, int maxiter, int method);
// windows of 65 .. 128 frames: cyclic Jacobi with its matrices in global memory (work: 3 (n + 2)^2 doubles per window)
void launch_ialm_small_wide(hipStream_t s, const IalmBuffers &b, int k, double lmbda, double tol, int maxiter, double *work);
size_t ialm_small_wide_doubles(int n);
// ialm_refine.hip: accurate first iteration (B_1) of the windows k_ialm_small flagged at k = 0; one launch after that step
void launch_ialm_refine_start(hipStream_t s, const IalmBuffers &b);
// sums the nblk Gram partial slabs of every live window into slab 0, in fixed order, chip-wide
void launch_gram_reduce(hipStream_t s, const IalmBuffers &b);
// ialm_gram8.hip: exact X^T X, sum of squares and max of every window on the i8 matrix cores
bool gram_u8_supported(const IalmBuffers &b);
void launch_gram_u8(hipStream_t s, const IalmBuffers &b);
void launch_planes_to_pn(hipStream_t s, const double *planes, double *out, int nwin, int n, int P, int64_t pstride, int fpad);
void launch_rpca_epilogue(hipStream_t s, const double *E, int64_t count, uint8_t *S);
int  ialm_pass_nblk(int variant, int n, int P, int nwin);

// filters.hip
struct BilateralTables {           // device copies of the weight tables
    float *color_w;                // [256]
    float *space_w;                // [maxk]
    int8_t *tap_dr, *tap_dc;       // [maxk]
    int maxk, radius;
};
void launch_gray(hipStream_t s, const uint8_t *frames, int channels, int64_t frame_stride, int64_t row_stride,
                 int x0, int y0, int F, int H, int W, int gray_mode, uint8_t *out);
void launch_bilateral(hipStream_t s, const uint8_t *src, int F, int H, int W, const BilateralTables &t,
                      int use_fma, uint8_t *dst);
void launch_thresh(hipStream_t s, const uint8_t *src, int64_t count, int thresh, uint8_t *dst);
void launch_open3x3(hipStream_t s, const uint8_t *src, int F, int H, int W, uint8_t *dst);
// any window (scipy's placement of even ones); tmp: F x H x W bytes for the eroded image
void launch_grey_open(hipStream_t s, const uint8_t *src, int F, int H, int W, int kh, int kw, uint8_t *tmp, uint8_t *dst);
// cv2.resize INTER_LINEAR on 8-bit pixels; per-axis index / weight tables made by the host
void launch_resize_linear(hipStream_t s, const uint8_t *src, int F, int H, int W, int ch, int dH, int dW, const int *xi, const short *xw,
                          const int *yi, const short *yw, uint8_t *dst);
// fused bilateral (t.radius = 1..4) + to-zero threshold + 3x3 opening; optional intermediates
void launch_filter_fused(hipStream_t s, const uint8_t *src, int F, int H, int W, const BilateralTables &t,
                         int use_fma, int thresh, uint8_t *bil_out, uint8_t *thr_out, uint8_t *open_out);

// yuv.hip: the rectangle [y0, y0 + Hr) x [x0, x0 + Wr) of F 4:2:0 frames (layout SWK_YUV_I420 / SWK_YUV_NV12; strides in bytes)
// -> dense BGR [F][Hr][Wr][3]
void launch_yuv420_to_bgr(hipStream_t s, int layout, const uint8_t *y, const uint8_t *u, const uint8_t *v, int64_t y_fs, int64_t y_rs,
                          int64_t c_fs, int64_t c_rs, int x0, int y0, int F, int Hr, int Wr, uint8_t *out);
// the same for any swk_yuv format (layout SWK_YUV_PLANAR / _SEMIPLANAR / _MONO, chroma shifts sx 0..2 and sy 0..1, bits 8..16)
void launch_yuv_to_bgr(hipStream_t s, int layout, int sx, int sy, int bits, int msb_aligned, int full_range, const uint8_t *y,
                       const uint8_t *u, const uint8_t *v, int64_t y_fs, int64_t y_rs, int64_t c_fs, int64_t c_rs, int x0, int y0, int F,
                       int Hr, int Wr, uint8_t *out);

// deinterlace.hip: one component plane of `count` interlaced frames -> the rectangle [py0, py0 + ph) x [px0, px0 + pw) of that plane
// in nout deinterlaced pictures, dense [nout][ph][pw] LSB-aligned samples (swk_yuv_deinterlace, include/swk.h).  Device memory.
// (tests/deinterlace_host.py mirrors both structs in ctypes and checks its copy against swk_deint_layout of the host-check build:
//  a member added here is added there and in that function.)
struct DeintPlane {
    const uint8_t *src;            // the sample at row oy, column ox of the plane in the first described frame
    int64_t fs, rs;                // frame and row stride in bytes
    int step;                      // samples from one sample of a row to the next (2: interleaved chroma)
    int oy, ox;                    // (a staged copy of a host source starts inside the plane; 0, 0 for the plane itself)
    int PH, PW;                    // the plane's size: its borders are the picture's borders
    int py0, px0, ph, pw;
    int parity0;                   // parity, in the picture, of the plane's row 0
    int msb;                       // 16 - bits for MSB-aligned words, else 0
    uint8_t *dst;
};
struct DeintJob {
    int count;                     // described frames
    int first;                     // the first frame that gives output (has_prev)
    int nout;                      // pictures made: rate x frames that give output
    int rate, tff, temporal;
};
void launch_deint_plane(hipStream_t s, const DeintPlane &p, const DeintJob &j, int wide);

// review.hip: F source frames' ROI (frame f at src + f * fs, ROI pixel (r, c) at + (y0 + r) * rs + (x0 + c) * channels; device memory)
// composed with the review overlay and converted to 8-bit 4:2:0 in device memory (include/swk.h, swk_render_review).  The host
// resolves styles: boxes [nboxes][6] = (r0, c0, r1, c1, colour b | g << 8 | r << 16, fill alpha | line alpha << 16) with
// box_start [F + 1] the first box of every frame, marks [nmarks][4] = (r, c, colour, line alpha) with mark_start [F + 1],
// frame_border [F][2] = (colour, line alpha or -1 for none) or null.  draw = false: the conversion alone (nothing but the source, the
// geometry and the destination is read).  text (with draw; null = no labels): labels [nlabels][16] = (r, c, scale, len, ink colour,
// ink alpha, plate colour, plate alpha, 8 words of text as font indices = byte - kReviewFontFirst) with label_start [F + 1]; an alpha
// of 0 stands for style 0 / plate 0 (the blend is then the identity).  The host builds all of these in one block (plan_review,
// review_plan.h, where kReviewFontFirst, kReviewFontCount and the host's copy of the font, review_font, live).
struct ReviewArgs {
    const uint8_t *src;
    int64_t fs, rs;
    int x0, y0, Hc, Wc, channels, layout;
    uint8_t *y, *u, *v;
    int64_t y_fs, y_rs, c_fs, c_rs;
    const uint8_t *mask;               // [Hc][Wc] or null
    uint32_t mask_colour; int mask_alpha;
    const int32_t *boxes, *box_start, *marks, *mark_start, *frame_border;
    int mark_arm, border;
};
// the labels go to the kernel as an argument of their own, which only the instantiation with text has: the others keep their arguments
struct ReviewLabels { const int32_t *labels, *label_start; };
void launch_review(hipStream_t s, const ReviewArgs &a, int F, bool draw, const ReviewLabels *text = nullptr);
// The stage panels of a mosaic (swk_render_review_panels): a's destination describes the mosaic, ncells = rows * cols cells of
// Hp x Wp luma pixels (Hc, Wc made even), cell k at ((k / cols) * Hp, (k % cols) * Wp).  launch_review draws cell 0 (it writes the
// ROI's pixels at the mosaic's strides); launch_review_panels writes the rest in one launch per 32768 frames: cell k = 1..npanels from
// panel[k - 1] (device memory; frame f, pixel (r, c) at plane + f * fs + r * rs + c) with the layers of a whose bit is set and label
// record captions[k - 1] (16 words as in ReviewLabels; len 0 = none), Y = 16 and U = V = 128 in the cells after them and in every
// cell's pad row / column.  palette [256] = b | g << 8 | r << 16 (device; read only where a panel is SWK_PANEL_LABELS; the host's
// review_label_palette and kReviewMaxPanels = 15 are in review_plan.h).
struct ReviewPanel { const uint8_t *plane; int64_t fs, rs; int kind, gain, layers, pad_; };
struct ReviewPanels {
    ReviewPanel panel[kReviewMaxPanels];
    const int32_t *captions;
    const uint32_t *palette;
    int npanels, ncells, cols;
};
void launch_review_panels(hipStream_t s, const ReviewArgs &a, int F, const ReviewPanels &q);

// classify_input.hip
void launch_classifier_input(hipStream_t s, const uint8_t *crops, const int64_t *offsets, const int32_t *hw, int nseg,
                             uint8_t *patches, float *net, int pad, bool nhwc, const float *mean, const float *sd);

void launch_segment_prefix(hipStream_t s, const int32_t *nseg, int F, int seg_cap, int32_t *offsets);
void launch_segment_inputs(hipStream_t s, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, int frame_h, int frame_w,
                           int x0, int y0, const swk_segment *segs, const int32_t *offsets, int F, int seg_cap, int min_h, int min_w,
                           int first, int count, float *net, int32_t *seg_frame, int pad, bool nhwc, const float *mean, const float *sd,
                           int32_t *oversize, int32_t *large);
// Boxes with a side of 513..4096: launch_segment_inputs / _groups append them to `large` ([0] = how many, then 6 ints each: row of net,
// frame, r0, c0, h, w; room for `count` boxes) and leave their rows of net alone; this writes those rows.  fr: the groups call's frames.
void launch_segment_inputs_large(hipStream_t s, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const struct SegFrame *fr,
                                 const int32_t *large, int nlarge, float *net, int pad, bool nhwc, const float *mean, const float *sd);
// diagnostic: Pillow coefficient tables of input sizes first .. first + count - 1; bounds [count][24][2], coeffs [count][24][343]
void launch_resize_table(hipStream_t s, int first, int count, int route, int32_t *bounds, int32_t *coeffs);

// ccl.hip
struct CclBuffers {
    int32_t *parent;               // [F][Pp] in the id space chosen by label_order
    uint32_t *rootbits;            // [F][words]
    int32_t *wordprefix;           // [F][words]
    int32_t *ncomp;                // [F]
    int32_t *table;                // [F][256][8] region accumulators (ints)
    unsigned long long *sums;      // [F][256][2] sum_r, sum_c
    int words;                     // per frame
    int Pp;                        // padded id-space size per frame
};
void launch_ccl(hipStream_t s, const uint8_t *src, int F, int H, int W, int connectivity, int order,
                const CclBuffers &b, int32_t *labels32 /*optional*/, uint8_t *labels8 /*optional*/);
void launch_regionprops(hipStream_t s, const uint8_t *labels8, int F, int H, int W, const CclBuffers &b,
                        int seg_cap, swk_segment *segs, int32_t *nseg);
// one-workgroup-per-frame fused labelling (+ region properties); needs the frame's bitmap in LDS
bool ccl_frame_supported(int H, int W);
void launch_ccl_frame(hipStream_t s, const uint8_t *src, int F, int H, int W, int connectivity, int order, const CclBuffers &b,
                      int32_t *labels32, uint8_t *labels8, bool props, int seg_cap, swk_segment *segs, int32_t *nseg);
size_t ccl_words(int H, int W);
size_t ccl_padded(int H, int W);

// shape_props.hip: the shape sums of every label value of F u8 planes (device memory; frame f, pixel (r, c) at labels + f * fs +
// r * rs + c) as ascending-label records; table: shape_table_bytes(F) bytes of scratch; shapes [F][seg_cap] and nseg [F] on the device
size_t shape_table_bytes(int F);
void launch_segment_shapes(hipStream_t s, const uint8_t *labels, int F, int H, int W, int64_t fs, int64_t rs, void *table, int seg_cap,
                           swk_segment_shape *shapes, int32_t *nseg);

// stabilize.hip: the shift search of swk_stabilize_u8 over F device frames (frame f, pixel (r, c) at frames + f * fs + r * rs + 3 c);
// anchor [Ho][Wo] dense; scratch: plane (stabilize_plane_bytes), nonzero [F], table (stabilize_table_bytes; what sad_table gets);
// shifts [F] and out [F][Ho][Wo][3] on the device
size_t stabilize_plane_bytes(int F, int Hs, int Ws);
size_t stabilize_table_bytes(int F, int S);
void launch_stabilize(hipStream_t s, const uint8_t *frames, int64_t fs, int64_t rs, int F, int Hs, int Ws, int y0, int x0, int Ho, int Wo,
                      int S, const uint8_t *anchor, int gray_mode, uint8_t *plane, uint32_t *nonzero, void *table, swk_shift *shifts,
                      uint8_t *out);
// the same search, then the quarter-pixel stage of swk_stabilize_subpel_u8: sub_table (stabilize_sub_table_bytes; what sub_table gets)
// and recs [F] on the device; shifts [F] is stage 1's scratch; out is resampled at the chosen phase
size_t stabilize_sub_table_bytes(int F);
void launch_stabilize_subpel(hipStream_t s, const uint8_t *frames, int64_t fs, int64_t rs, int F, int Hs, int Ws, int y0, int x0, int Ho,
                             int Wo, int S, const uint8_t *anchor, int gray_mode, uint8_t *plane, uint32_t *nonzero, void *table,
                             swk_shift *shifts, void *sub_table, swk_subshift *recs, uint8_t *out);

// ---- several groups of windows in one call ---------------------------------------------------------------
// swk_batch_run and swk_batch_run_groups share one driver (run_batch, swk_api.hip) and one host-only plan (batch_plan.h, which
// also holds the descriptor records GroupWin, FrameGeom, SegFrame and PnWin).  A call of one group takes the uniform launchers
// above; a call of several takes these: a group's windows keep their own geometry, the image stages address every frame through
// a descriptor, and the IALM runs over planes zero-padded to the call's largest ROI (groups.hip, DESIGN section "Several videos
// in one call").
void launch_gray_groups(hipStream_t s, const GroupWin *wins, int F, int n, int Pmax, int gray_mode, uint8_t *X);
void launch_planes_to_pn_groups(hipStream_t s, const double *planes, const PnWin *wins, int nwin, int n, int Pmax, int64_t pstride,
                                int fpad);
// fused filter with per-frame geometry; grid sized by the largest frame; outputs [total] pre-cleared here
void launch_filter_fused_geom(hipStream_t s, const uint8_t *src, int F, int Hmax, int Wmax, const FrameGeom *geom, size_t total,
                              const BilateralTables &t, int use_fma, int thresh, uint8_t *bil_out, uint8_t *thr_out, uint8_t *open_out);
// one-workgroup-per-frame labelling + region properties with per-frame geometry (frames with H = 0 are skipped);
// lds = the largest ccl_frame_lds_bytes of the frames, vec = word width every frame's size and offset allow (4, 2, 1)
size_t ccl_frame_lds_bytes(int H, int W);
void launch_ccl_frame_geom(hipStream_t s, const uint8_t *src, int F, const FrameGeom *geom, size_t lds, int vec, int connectivity,
                           int order, const CclBuffers &b, uint8_t *labels8, int seg_cap, swk_segment *segs, int32_t *nseg);
void launch_segment_prefix_groups(hipStream_t s, const int32_t *nseg, const SegFrame *fr, int F, int32_t *offsets);
void launch_segment_inputs_groups(hipStream_t s, const SegFrame *fr, const swk_segment *segs, int seg_stride, const int32_t *offsets,
                                  int F, int min_h, int min_w, int first, int count, float *net, int32_t *seg_frame, int pad, bool nhwc,
                                  const float *mean, const float *sd, int32_t *oversize, int32_t *large);

}  // namespace swk
