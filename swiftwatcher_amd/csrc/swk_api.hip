// C ABI of libswk.so (include/swk.h): context, workspaces, stage orchestration.
// Host side only; every kernel lives in ialm*.hip / filters.hip / ccl.hip.
#include "swk_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <string>
#include <algorithm>
#include <array>
#include <vector>

using namespace swk;

namespace swk { std::atomic<int> g_launch_error{0}; }

namespace {

std::string g_create_error;

enum Slot {
    SL_ROI = 0, SL_X, SL_S, SL_BIL, SL_THR, SL_OPEN, SL_LAB8, SL_LAB32, SL_A, SL_Y, SL_E, SL_PN,
    SL_BM, SL_VPREV, SL_GPART, SL_ZZPART, SL_WIN, SL_ACTIVE, SL_PARENT, SL_ROOTBITS, SL_WORDPREFIX,
    SL_NCOMP, SL_TABLE, SL_SUMS, SL_SEGS, SL_NSEG, SL_TMP_IN, SL_TMP_OUT, SL_TMP_AUX, SL_COLORW, SL_SPACEW,
    SL_TAPDR, SL_TAPDC, SL_SALT, SL_WIDE, SL_REDO_X, SL_REDO_S, SL_REDO_P, SL_SEGOFFS, SL_SEGLARGE, SL_CL_CROPS, SL_CL_OFFS, SL_CL_HW, SL_CL_PATCH, SL_CL_NET, SL_GRP, SL_REVIEW, SL_SHAPE_TAB, SL_SHAPE_REC, SL_SHAPE_NSEG,
    SL_STAB_PLANE, SL_STAB_TAB, SL_STAB_REC, SL_SUBPEL_PLANE, SL_SUBPEL_TAB, SL_SUBPEL_REC, SL_SUBPEL_SUBTAB, SL_COUNT
};

struct EventPair { hipEvent_t a, b; int fam; };

}  // namespace

struct swk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    void *slot[SL_COUNT] = {nullptr};
    size_t slot_bytes[SL_COUNT] = {0};
    int *h_active = nullptr;             // pinned
    // bilateral tables currently on the device
    int bil_d = -1; double bil_sc = -1, bil_ss = -1;
    BilateralTables bil{};
    // profiling
    bool prof_on = false;
    std::vector<EventPair> pending;
    std::vector<hipEvent_t> pool;
    double prof_ms[SWK_K_COUNT] = {0};
    int64_t prof_n[SWK_K_COUNT] = {0};
    int64_t window_iters = 0;
    int ialm_variant = 0;
    int pass_tune = 0;             // k-step-templated pass: bit 0 priority, bit 1 stagger for the odd hardware wave slot
    double sparse_spec = 16.0;     // M-state pass: sparse image stores start at 16 x tol (<= 0: every pass)
    double norm_guard = 1e-3;      // M-state pass: |ratio / tol - 1| below this does not decide (the window is rerun with the f64 norm)
    int64_t guard_windows = 0;     // windows rerun for that reason
    double start_refine = 1e-5;    // estimated first-iteration error above which a window gets the accurate start (ialm_refine.hip)
    int64_t refined_windows = 0, unrefined_windows = 0;
    int64_t redo_batches = 0;      // batches in which a guess of the M-state pass failed ...
    int64_t redo_windows = 0;      // ... and the windows that were run again for it
    int last_eig_sweeps = 0;       // largest IalmWin::sweeps of the last batch (Newton-Schulz iterations, or 100 + Jacobi sweeps)
    int last_int_start = 0;        // windows of the last batch whose first Gram matrix came from the integer matrix cores
    int use_gram8 = 1;             // M-state pass: first Gram matrix from k_gram_u8 (A/B knob)
    unsigned long long pass_b16 = 0;   // sum over windows of IalmWin::pass_b16 since the last swk_prof_reset
    double norm_spec = 256.0;      // M-state pass: ||Z|| every other iteration while above 256 x tol (<= 0: every iteration)
    int sparse_backoff = 0, norm_backoff = 0;   // batches for which a guess stays off after it failed (same video, same behaviour)
    int eig_method = 0;                  // 0 Newton-Schulz (MFMA), 1 Jacobi
    int max_grid_y = 65535;              // hipDeviceAttributeMaxGridDimY of the device: the IALM kernels put the window in blockIdx.y, unsplit
    bool force_ccl_multi = false;        // swk_debug_force_ccl_multi_kernel: every frame size takes launch_ccl (+ launch_regionprops)
    hipEvent_t ev_poll[2] = {nullptr, nullptr};   // the host polls convergence two iterations late (ialm_chain)
    std::vector<int32_t> last_stage;     // staging route of each group of the last batch call (host_stage_plan's kind; -1: a device group)
    std::vector<IalmWin> last_hw;        // host copy of the last batch's per-window IALM state (account_iters): diagnostics
    // what the last batch call left on the device for swk_segment_inputs_last: its frames (SL_ROI copy of a host input,
    // or the caller's device frames) and region records; valid until a call reuses those buffers
    struct LastBatch {
        bool valid = false;
        const uint8_t *frames = nullptr;
        int64_t fs = 0, rs = 0;
        int nwin = 0, n = 0, Hc = 0, Wc = 0, x0 = 0, y0 = 0, frame_h = 0, frame_w = 0, cap = 0;
        int total = -1;          // segments of the batch (regions beyond cap not counted), when nseg was copied to the host
        const swk_segment *segs = nullptr;
        const int32_t *nseg = nullptr;
        const SegFrame *fr = nullptr;   // swk_batch_run_groups: per-frame frames and geometry (device table), nwin * n frames
    } last;
};

namespace {

#define HIPCHK(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            char buf_[512];                                                                    \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            (ctx)->err = buf_;                                                                 \
            return SWK_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

int fail(swk_ctx *ctx, int code, const char *msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

// The IALM kernels put the window in blockIdx.y and do not split it (include/swk.h, "Windows per call"): a call with more windows in
// one IALM (sub-)batch than the device's grid y extent is refused before anything is allocated, copied or launched.
int check_windows(swk_ctx *ctx, int64_t nwin)
{
    if (nwin <= ctx->max_grid_y) return SWK_OK;
    char buf[160];
    snprintf(buf, sizeof buf, "too many windows in one call: %lld, the device takes %d at most (grid y extent; windows are not chunked)",
             (long long)nwin, ctx->max_grid_y);
    ctx->err = buf;
    return SWK_ERR_CAPACITY;
}

int need(swk_ctx *ctx, Slot s, size_t bytes, void **out)
{
    if (bytes == 0) bytes = 16;
    if (ctx->slot_bytes[s] < bytes) {
        if (ctx->slot[s]) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->slot[s])); }
        ctx->slot[s] = nullptr;
        ctx->slot_bytes[s] = 0;
        hipError_t e = hipMalloc(&ctx->slot[s], bytes);
        if (e != hipSuccess) {
            char buf[256];
            snprintf(buf, sizeof buf, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
            ctx->err = buf;
            return SWK_ERR_NOMEM;
        }
        ctx->slot_bytes[s] = bytes;
    }
    *out = ctx->slot[s];
    return SWK_OK;
}

#define NEED(ctx, slot, bytes, ptr)                                          \
    do { void *p_; int rc_ = need(ctx, slot, bytes, &p_); if (rc_) return rc_; ptr = (decltype(ptr))p_; } while (0)

// ---- profiling --------------------------------------------------------------------
hipEvent_t take_event(swk_ctx *ctx)
{
    if (!ctx->pool.empty()) { hipEvent_t e = ctx->pool.back(); ctx->pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct Timed {
    swk_ctx *ctx; int fam; hipStream_t st; hipEvent_t a{}, b{};
    Timed(swk_ctx *c, int f, hipStream_t stream = nullptr) : ctx(c), fam(f), st(stream ? stream : c->stream)
    {
        if (ctx->prof_on) { a = take_event(ctx); b = take_event(ctx); (void)hipEventRecord(a, st); }
    }
    ~Timed()
    {
        if (ctx->prof_on) { (void)hipEventRecord(b, st); ctx->pending.push_back({a, b, fam}); }
    }
};

int ensure_poll_events(swk_ctx *ctx)
{
    for (int i = 0; i < 2; ++i)
        if (!ctx->ev_poll[i]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_poll[i], hipEventDisableTiming));
    return SWK_OK;
}

void drain_prof(swk_ctx *ctx)
{
    for (auto &p : ctx->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { ctx->prof_ms[p.fam] += ms; ctx->prof_n[p.fam] += 1; }
        ctx->pool.push_back(p.a);
        ctx->pool.push_back(p.b);
    }
    ctx->pending.clear();
}

int sync(swk_ctx *ctx)
{
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    if (const int le = g_launch_error.exchange(0)) {          // a launcher could not set a kernel attribute or start a kernel
        HIPCHK(ctx, (hipError_t)le);
    }
    drain_prof(ctx);
    return SWK_OK;
}

// ---- bilateral weight tables (OpenCV 4.1.0 bilateralFilter_8u set-up, host side) ----
// radius of a diameter: d <= 0 derives it from sigma_space; at least 1
int bilateral_radius(int d, double sigma_space)
{
    const double ss = sigma_space <= 0 ? 1 : sigma_space;
    const int radius = d <= 0 ? (int)lrint(ss * 1.5) : d / 2;
    return radius < 1 ? 1 : radius;
}

int ensure_bilateral(swk_ctx *ctx, int d, double sigma_color, double sigma_space)
{
    if (ctx->bil_d == d && ctx->bil_sc == sigma_color && ctx->bil_ss == sigma_space) return SWK_OK;
    double sc = sigma_color <= 0 ? 1 : sigma_color, ss = sigma_space <= 0 ? 1 : sigma_space;
    const double gc = -0.5 / (sc * sc), gs = -0.5 / (ss * ss);
    const int radius = bilateral_radius(d, sigma_space);
    if (radius > 4) return fail(ctx, SWK_ERR_ARG, "bilateral diameter > 9 is not supported");
    float cw[256], sw[81];
    int8_t dr[81], dc[81];
    for (int i = 0; i < 256; ++i) cw[i] = (float)exp((double)(i * i) * gc);
    int k = 0;
    for (int i = -radius; i <= radius; ++i)
        for (int j = -radius; j <= radius; ++j) {
            const double r = sqrt((double)i * i + (double)j * j);
            if (r > radius) continue;
            sw[k] = (float)exp(r * r * gs);
            dr[k] = (int8_t)i; dc[k] = (int8_t)j;
            ++k;
        }
    NEED(ctx, SL_COLORW, sizeof cw, ctx->bil.color_w);
    NEED(ctx, SL_SPACEW, sizeof sw, ctx->bil.space_w);
    NEED(ctx, SL_TAPDR, sizeof dr, ctx->bil.tap_dr);
    NEED(ctx, SL_TAPDC, sizeof dc, ctx->bil.tap_dc);
    HIPCHK(ctx, hipMemcpyAsync(ctx->bil.color_w, cw, sizeof cw, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->bil.space_w, sw, sizeof(float) * k, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->bil.tap_dr, dr, k, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->bil.tap_dc, dc, k, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // cw/sw live on this stack frame
    ctx->bil.maxk = k;
    ctx->bil.radius = radius;
    ctx->bil_d = d; ctx->bil_sc = sigma_color; ctx->bil_ss = sigma_space;
    return SWK_OK;
}

int ensure_ccl(swk_ctx *ctx, int F, int H, int W, CclBuffers *b)
{
    b->Pp = (int)ccl_padded(H, W);
    b->words = (int)ccl_words(H, W);
    NEED(ctx, SL_PARENT, (size_t)F * b->Pp * 4, b->parent);
    NEED(ctx, SL_ROOTBITS, (size_t)F * b->words * 4, b->rootbits);
    NEED(ctx, SL_WORDPREFIX, (size_t)F * b->words * 4, b->wordprefix);
    NEED(ctx, SL_NCOMP, (size_t)F * 4, b->ncomp);
    NEED(ctx, SL_TABLE, (size_t)F * 256 * 8 * 4, b->table);
    NEED(ctx, SL_SUMS, (size_t)F * 256 * 2 * 8, b->sums);
    return SWK_OK;
}

// ---- host input -> device (the copy strategy comes from host_stage_plan, batch_plan.h) ----
// Copies `in` to roi and says where the kernels find it there: frame 0 at *dframes, strides *fs / *rs, ROI origin (*x0, *y0).
int host_stage_copy(swk_ctx *ctx, const swk_input *in, const HostStage &st, uint8_t *roi, const uint8_t **dframes, int64_t *fs_out,
                    int64_t *rs_out, int *x0_out, int *y0_out)
{
    hipStream_t s = ctx->stream;
    const int F = in->nwin * in->n, H = in->Hc, W = in->Wc, P = H * W;
    const size_t plane = (size_t)F * P;
    const int64_t fs = in->frame_stride, rs = in->row_stride, afs = fs < 0 ? -fs : fs;
    const int x0 = in->x0, y0 = in->y0;
    const size_t rowb = (size_t)W * in->channels;
    if (st.kind == ST_DENSE) {
        // pre-cropped, densely packed ROI frames: one copy for the whole batch
        HIPCHK(ctx, hipMemcpyAsync(roi, in->frames + (int64_t)y0 * rs, plane * in->channels, hipMemcpyHostToDevice, s));
    } else if (st.kind == ST_WHOLE) {
        // ROI frames with a margin around them (FrameQueue stages the crop plus the half minimum segment size, so that
        // segment boxes can grow into it like they grow into the full frame, image_filtering.py:338-369): the whole
        // buffer in one copy; the kernels read the ROI at (x0, y0) of the device copy.  A NEGATIVE frame stride (queue
        // position 0 = the LAST frame in memory: a reader's block in file order) is copied as it lies and read backwards.
        const uint8_t *lowest = fs < 0 ? in->frames + (int64_t)(F - 1) * fs : in->frames;
        HIPCHK(ctx, hipMemcpyAsync(roi, lowest, (size_t)F * (size_t)afs, hipMemcpyHostToDevice, s));
        *dframes = fs < 0 ? roi + (int64_t)(F - 1) * afs : roi;
        *fs_out = fs; *rs_out = rs; *x0_out = x0; *y0_out = y0;
        return SWK_OK;
    } else if (st.kind == ST_ROWS) {
        for (int f = 0; f < F; ++f)                    // full-width rows: one contiguous block per frame
            HIPCHK(ctx, hipMemcpyAsync(roi + (size_t)f * P * in->channels, in->frames + (int64_t)f * fs + (int64_t)y0 * rs,
                                       (size_t)P * in->channels, hipMemcpyHostToDevice, s));
    } else {
        for (int f = 0; f < F; ++f)
            HIPCHK(ctx, hipMemcpy2DAsync(roi + (size_t)f * P * in->channels, rowb,
                                         in->frames + (int64_t)f * fs + (int64_t)y0 * rs + (int64_t)x0 * in->channels, (size_t)rs,
                                         rowb, H, hipMemcpyHostToDevice, s));
    }
    *dframes = roi;
    *fs_out = (int64_t)P * in->channels; *rs_out = (int64_t)rowb; *x0_out = 0; *y0_out = 0;
    return SWK_OK;
}

// ---- IALM driver ----------------------------------------------------------------------
// Planes per window in the A / Y / E workspaces (the M-state pass pads n to its k-step, the others to 16) and their pitch: P rounded
// up to whole groups of 8 tiles.  A window's planes must stay below 2^28 elements.
int ialm_fpad(bool mstate, int n) { return mstate ? ialm_mstate_fpad(n) : (n + 15) & ~15; }
int64_t ialm_pstride(int64_t P) { return (P + 127) & ~(int64_t)127; }

// What one IALM chain runs, decided once from the call and the context's switches.
struct IalmPlan {
    int variant;           // pass kernel (launch_ialm_pass): 1, 2, 4, 5 or 6
    bool mstate;           // the M-state pass (variants 4 / 5): no A / E; guesses and the guard band, so windows may run again
    int fpad;              // planes per window in A, Y, E
    int64_t pstride;       // plane pitch (elements) of A, Y, E
    int nblk;              // blocks per window of every pass
    bool gram8;            // the integer start may run (where gram_u8_supported allows it for the buffers)
    double refine;         // threshold of the accurate first iteration (ialm_refine.hip); 0 = never
    bool small_wide;       // the small-matrix step of long windows (k_ialm_small_wide) instead of k_ialm_small
};

IalmPlan plan_ialm(const swk_ctx *ctx, int n, int P, int nwin, bool want_AE, int force_variant)
{
    // auto: the M-state pass (k-step-templated, 21 B/element) unless the caller wants the f64 low-rank / sparse matrices,
    // which only the A/Y-state pass (v2, 34 B/element) materialises; 65 .. 128 frames: the plain f64 kernels (A/Y state, Jacobi in
    // global memory)
    int variant = force_variant ? force_variant : ctx->ialm_variant;
    if (variant == 0) variant = 4;
    if (variant >= 4 && variant != 6 && want_AE) variant = 2;
    if (n > kMaxN) variant = 6;
    IalmPlan pl{};
    pl.variant = variant;
    pl.mstate = variant == 4 || variant == 5;
    pl.fpad = ialm_fpad(pl.mstate, n);
    pl.pstride = ialm_pstride(P);
    pl.nblk = ialm_pass_nblk(variant, n, P, nwin);
    pl.gram8 = (pl.mstate || variant == 2 || variant == 1) && ctx->use_gram8;
    pl.refine = n > kMaxN ? 0.0 : ctx->start_refine;          // (by the window length: a forced variant 6 below 65 frames refines)
    pl.small_wide = variant == 6;
    return pl;
}

// One IALM call's windows: nwin windows of n frames x P pixels side by side in X; their sparse images go to S.
struct IalmJob {
    const uint8_t *X;
    uint8_t *S;
    int nwin, n, P;
    const PnWin *wpix;          // each window's true pixel count (several groups: the rest of its P is zero padding); null: P
    double lmbda, tol;
    int maxiter;
};

// What run_ialm leaves on the device for its caller: the final per-window state and the A / E workspaces (when asked for).
struct IalmRun {
    IalmWin *win;
    int nwin;
    int64_t pstride;
    int fpad;
    const double *A, *E;
};

// Copies the per-window IALM state of nwin windows to the host (waits for it).
int copy_windows(swk_ctx *ctx, const IalmWin *win, int nwin, IalmWin *dst)
{
    // (on the context's own, non-blocking stream: a copy on the null stream would wait for every blocking stream of the process, and
    //  fails outright while another thread captures a HIP graph on one -- the classifier does, segment_classification.py)
    HIPCHK(ctx, hipMemcpyAsync(dst, win, (size_t)nwin * sizeof(IalmWin), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SWK_OK;
}

// The start of a chain (ialm_chain, and swk_debug_ialm_start, which stops after it): the chain's buffers, then window statistics,
// start choice and the first iteration's Gram slabs -- k_gram_u8 or k_ialm_stats, k_ialm_init, the MODE 0 pass of the plan's variant.
// speculate: the M-state pass may guess (ialm_chain).  *bp describes the buffers; *wide_work_out is the workspace of k_ialm_small_wide
// (null unless the plan uses it).
int ialm_start(swk_ctx *ctx, const IalmJob &job, const IalmPlan &plan, bool want_E, bool speculate, IalmBuffers *bp, double **wide_work_out)
{
    const int nwin = job.nwin, n = job.n, P = job.P;
    IalmBuffers &b = *bp;
    b = IalmBuffers{};
    b.X = job.X; b.S = job.S; b.nwin = nwin; b.n = n; b.P = P; b.wpix = job.wpix;
    b.nblk = plan.nblk;
    b.nred = b.nblk > 4 ? 1 : b.nblk;       // several slabs: reduce them chip-wide first (k_gram_reduce)
    b.pstride = plan.pstride;
    b.fpad = plan.fpad;
    if ((int64_t)b.fpad * b.pstride >= (1ll << 28)) return fail(ctx, SWK_ERR_ARG, "window too large: frames x ROI pixels must stay below 2^28");
    const size_t elems = (size_t)nwin * n * P;
    const size_t felems = (size_t)nwin * b.fpad * b.pstride;
    NEED(ctx, SL_A, felems * 8, b.A);
    NEED(ctx, SL_Y, felems * 8, b.Y);
    if (plan.mstate) {
        b.U = (uint16_t *)b.Y;               // binary16 planes in the Y slot
        b.spec = (speculate && ctx->sparse_backoff == 0) ? ctx->sparse_spec : 0.0;
        b.nspec = (speculate && ctx->norm_backoff == 0) ? ctx->norm_spec : 0.0;
        b.guard = ctx->norm_guard;
        if (speculate) {
            if (ctx->sparse_backoff > 0) ctx->sparse_backoff -= 1;
            if (ctx->norm_backoff > 0) ctx->norm_backoff -= 1;
        }
        NEED(ctx, SL_SALT, elems, b.Salt);
    }
    if (want_E) NEED(ctx, SL_E, felems * 8, b.E);
    NEED(ctx, SL_BM, (size_t)nwin * n * n * 8, b.Bm);
    NEED(ctx, SL_VPREV, (size_t)nwin * n * n * 8, b.Vprev);
    NEED(ctx, SL_GPART, (size_t)nwin * b.nblk * n * n * 8, b.gpart);
    NEED(ctx, SL_ZZPART, (size_t)2 * nwin * b.nblk * 8, b.zzpart);          // [nwin][nblk] sums of z^2, then [nwin][nblk] max |U| (M-state pass)
    NEED(ctx, SL_WIN, (size_t)nwin * sizeof(IalmWin), b.win);
    NEED(ctx, SL_ACTIVE, 16 * sizeof(int), b.active);
    double *wide_work = nullptr;
    if (plan.small_wide) NEED(ctx, SL_WIDE, (size_t)nwin * ialm_small_wide_doubles(n) * sizeof(double), wide_work);
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(b.win, 0, (size_t)nwin * sizeof(IalmWin), s));
    HIPCHK(ctx, hipMemsetAsync(b.active, 0, 16 * sizeof(int), s));
    HIPCHK(ctx, hipMemsetAsync(b.S, 0, elems, s));
    if (plan.mstate) {
        HIPCHK(ctx, hipMemsetAsync(b.Salt, 0, elems, s));
    } else {
        // a window that stops before writing A (all-zero input) must still read back zeros
        HIPCHK(ctx, hipMemsetAsync(b.A, 0, felems * 8, s));
        // padded frame planes (n..fpad-1) of Y are read by the MFMA pass and must contribute zeros
        if (b.fpad != n) HIPCHK(ctx, hipMemsetAsync(b.Y, 0, felems * 8, s));
    }
    if (want_E) HIPCHK(ctx, hipMemsetAsync(b.E, 0, felems * 8, s));

    // window statistics (||X||_F, max) and, for the M-state pass, the first Gram matrix in the same read of X
    // on the integer matrix cores; windows it does not cover get the f64 start pass below
    b.use_gram8 = (plan.gram8 && gram_u8_supported(b)) ? 1 : 0;
    b.refine = plan.refine;
    { Timed t(ctx, SWK_K_IALM_STATS);
      if (b.use_gram8) launch_gram_u8(s, b); else launch_ialm_stats(s, b);
      launch_ialm_init(s, b, job.lmbda); }
    // the Gram-only start pass reads X alone (1 B/element): booked with the statistics family so
    // SWK_K_IALM_PASS times only the full streaming passes
    { Timed t(ctx, SWK_K_IALM_STATS); launch_ialm_pass(s, b, 0, plan.variant, 0, ctx->pass_tune); }
    *wide_work_out = wide_work;
    return SWK_OK;
}

// The small-matrix step of iteration k over the chain's windows: the chip-wide slab sum where a window has more than 4 slabs, then the
// step's kernel (k_ialm_small_wide above 64 frames or under pass variant 6, k_ialm_small under the context's solver otherwise).
void ialm_small_step(swk_ctx *ctx, const IalmJob &job, const IalmPlan &plan, const IalmBuffers &b, int k, double *wide_work)
{
    hipStream_t s = ctx->stream;
    Timed t(ctx, SWK_K_IALM_SMALL);
    if (b.nblk > 4) launch_gram_reduce(s, b);
    if (plan.small_wide) launch_ialm_small_wide(s, b, k, job.lmbda, job.tol, job.maxiter, wide_work);
    else launch_ialm_small(s, b, k, job.lmbda, job.tol, job.maxiter, ctx->eig_method);
}

// The first step after the start (ialm_chain, and swk_debug_ialm_first_step, which stops after it): the small-matrix step of k = 0,
// then the windows that step found ill-conditioned get their first iteration's matrix B_1 again, from a double-double Cholesky factor
// of the exact integer X^T X -- of a double-double M_1^T M_1 where the window had no integer start -- (one workgroup per flagged
// window; the others leave at the first branch).  B_std (optional, host, [nwin][n][n]): the step's own B_1, copied out in stream
// order before the refinement is launched.
int ialm_first_step(swk_ctx *ctx, const IalmJob &job, const IalmPlan &plan, const IalmBuffers &b, double *wide_work, double *B_std)
{
    hipStream_t s = ctx->stream;
    ialm_small_step(ctx, job, plan, b, 0, wide_work);
    if (B_std) HIPCHK(ctx, hipMemcpyAsync(B_std, b.Bm, (size_t)b.nwin * b.n * b.n * 8, hipMemcpyDeviceToHost, s));
    if (b.refine > 0.0) { Timed t(ctx, SWK_K_IALM_SMALL); launch_ialm_refine_start(s, b); }
    return SWK_OK;
}

// One chain over the job's windows on the context's stream: start, first step, then per iteration pass -> (slab sum) -> small-matrix
// step, until every window has stopped.  speculate: the M-state pass may guess (sparse-image stores and stopping norms skipped far
// from the tolerance).  *bp describes the buffers the chain worked in.
int ialm_chain(swk_ctx *ctx, const IalmJob &job, const IalmPlan &plan, bool want_A, bool want_E, bool speculate, IalmBuffers *bp)
{
    int rc = ensure_poll_events(ctx);
    if (rc) return rc;
    double *wide_work = nullptr;
    if ((rc = ialm_start(ctx, job, plan, want_E, speculate, bp, &wide_work))) return rc;
    IalmBuffers &b = *bp;
    hipStream_t s = ctx->stream;
    const int check_from = 6;     // no window converges earlier (mu grows 1.5x per iteration)
    const int maxiter = job.maxiter;
    if ((rc = ialm_first_step(ctx, job, plan, b, wide_work, nullptr))) return rc;
    for (int k = 1; k <= maxiter + 2; ++k) {
        // convergence is polled two iterations late so the host never stalls the queue; the launches made
        // meanwhile for an already finished batch return at their first branch
        const int kc = k - 2;
        if (kc >= check_from) {
            HIPCHK(ctx, hipEventSynchronize(ctx->ev_poll[kc & 1]));
            if (ctx->h_active[kc & 1] <= 0) break;
        }
        if (k > maxiter) break;
        { Timed t(ctx, SWK_K_IALM_PASS); launch_ialm_pass(s, b, k == 1 ? 1 : 2, plan.variant, k, ctx->pass_tune); }
        ialm_small_step(ctx, job, plan, b, k, wide_work);
        if (k >= check_from) {
            HIPCHK(ctx, hipMemcpyAsync(&ctx->h_active[k & 1], b.active, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipEventRecord(ctx->ev_poll[k & 1], s));
        }
    }
    if (plan.mstate) { Timed t(ctx, SWK_K_IALM_STATS); launch_select_sparse(s, b); }
    return SWK_OK;
}

// Runs the job's windows `list` again, side by side as a chain of their own through `variant`, with the guesses off: their pixels
// (and pixel counts) gathered into the rerun slots, their sparse images scattered back into the job's S, their final state into
// hw[list[i]] (pass_b16 keeps counting the abandoned passes).  band (optional): the windows of `list` that chain sent to the guard band.
int rerun_windows(swk_ctx *ctx, const IalmJob &job, const std::vector<int> &list, int variant, std::vector<IalmWin> &hw,
                  std::vector<int> *band)
{
    hipStream_t s = ctx->stream;
    const int cnt = (int)list.size();
    const size_t wbytes = (size_t)job.n * job.P;
    IalmJob sub = job;
    sub.nwin = cnt;
    uint8_t *gx, *gs;
    NEED(ctx, SL_REDO_X, (size_t)cnt * wbytes + 4, gx);
    NEED(ctx, SL_REDO_S, (size_t)cnt * wbytes, gs);
    for (int i = 0; i < cnt; ++i)
        HIPCHK(ctx, hipMemcpyAsync(gx + (size_t)i * wbytes, job.X + (size_t)list[i] * wbytes, wbytes, hipMemcpyDeviceToDevice, s));
    PnWin *gp = nullptr;
    if (job.wpix) {
        NEED(ctx, SL_REDO_P, (size_t)cnt * sizeof(PnWin), gp);
        for (int i = 0; i < cnt; ++i)
            HIPCHK(ctx, hipMemcpyAsync(gp + i, job.wpix + list[i], sizeof(PnWin), hipMemcpyDeviceToDevice, s));
    }
    sub.X = gx; sub.S = gs; sub.wpix = gp;
    IalmBuffers b;
    int rc = ialm_chain(ctx, sub, plan_ialm(ctx, job.n, job.P, cnt, false, variant), false, false, false, &b);
    if (rc) return rc;
    for (int i = 0; i < cnt; ++i)
        HIPCHK(ctx, hipMemcpyAsync(job.S + (size_t)list[i] * wbytes, gs + (size_t)i * wbytes, wbytes, hipMemcpyDeviceToDevice, s));
    std::vector<IalmWin> sw(cnt);
    if ((rc = copy_windows(ctx, b.win, cnt, sw.data()))) return rc;
    if (band) band->clear();
    for (int i = 0; i < cnt; ++i) {
        if (band && (sw[i].redo & 4)) band->push_back(list[i]);
        sw[i].pass_b16 += hw[list[i]].pass_b16;          // the roofline books every pass a window ran, the abandoned ones included
        hw[list[i]] = sw[i];
    }
    return SWK_OK;
}

// The IALM over the job's windows: one chain, then the chains that finish the windows the M-state pass could not finish on its own
// terms (IalmWin::redo): bits 0 / 1 = a guess failed (the window stopped right after a pass that had its sparse-image stores
// switched off, or a partial norm could not rule out that an iteration was the last); bit 2 = the float32 stopping norm fell inside
// the guard band around the tolerance.  Only those windows run again, in this order, each list as a chain of its own (the batch size
// sets nblk and with it the summation order, so the lists are not merged):
//   1. the windows whose guess failed, with the guesses off (the guard band stays);
//   2. those of them that this rerun sent to the guard band, through the A/Y-state pass (norm in float64, statement by statement the
//      reference's :293-297);
//   3. the windows the first chain sent to the guard band, the same way.
// A rerun makes no guesses, so it cannot set bits 0 / 1, and the A/Y-state pass has no guard band: no rerun needs one of its own.
// The reruns' sparse images, iteration counts and diagnostics replace the windows' entries.
int run_ialm(swk_ctx *ctx, const IalmJob &job, bool want_A, bool want_E, IalmRun *run)
{
    const int nwin = job.nwin;
    if (job.n < 1 || job.n > kMaxNWide) return fail(ctx, SWK_ERR_ARG, "frames per window must be in 1..128");
    const IalmPlan plan = plan_ialm(ctx, job.n, job.P, nwin, want_A || want_E, 0);
    IalmBuffers b;
    int rc = ialm_chain(ctx, job, plan, want_A, want_E, true, &b);
    if (rc) return rc;
    *run = IalmRun{b.win, nwin, b.pstride, b.fpad, want_A ? b.A : nullptr, b.E};          // (reruns follow M-state chains: no A / E)
    if (!plan.mstate || !(b.spec > 0.0 || b.nspec > 0.0 || b.guard > 0.0)) return SWK_OK;
    std::vector<IalmWin> hw(nwin);
    if ((rc = copy_windows(ctx, b.win, nwin, hw.data()))) return rc;
    std::vector<int> guess, band, guess_band;
    int redo = 0;
    for (int w = 0; w < nwin; ++w) {
        redo |= hw[w].redo;
        if (hw[w].redo & 3) guess.push_back(w);
        else if (hw[w].redo & 4) band.push_back(w);
    }
    if (redo & 3) {
        // windows of one video behave alike: a guess that failed stays off for the next batches
        ctx->redo_batches += 1;
        ctx->redo_windows += (int64_t)guess.size();
        if (redo & 1) ctx->sparse_backoff = 64;
        if (redo & 2) ctx->norm_backoff = 64;
    }
    ctx->guard_windows += (int64_t)band.size();
    if (!guess.empty() && (rc = rerun_windows(ctx, job, guess, plan.variant, hw, &guess_band))) return rc;
    ctx->guard_windows += (int64_t)guess_band.size();
    if (!guess_band.empty() && (rc = rerun_windows(ctx, job, guess_band, 2, hw, nullptr))) return rc;
    if (!band.empty() && (rc = rerun_windows(ctx, job, band, 2, hw, nullptr))) return rc;
    if (!guess.empty() || !band.empty()) {
        // the reruns used the window-state slot for their own (smaller) batches: this batch's entries go back
        NEED(ctx, SL_WIN, (size_t)nwin * sizeof(IalmWin), run->win);
        HIPCHK(ctx, hipMemcpyAsync(run->win, hw.data(), (size_t)nwin * sizeof(IalmWin), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SWK_OK;
}

// Appends the per-window IALM state of a run to hw (waits for it).
int read_windows(swk_ctx *ctx, const IalmRun &run, std::vector<IalmWin> &hw)
{
    const size_t w0 = hw.size();
    hw.resize(w0 + run.nwin);
    return copy_windows(ctx, run.win, run.nwin, hw.data() + w0);
}

// Books the per-window IALM state of a call (counters, diagnostics) and hands out its iteration counts (host, optional).
void account_iters(swk_ctx *ctx, const std::vector<IalmWin> &hw, int32_t *iters)
{
    ctx->last_hw = hw;
    ctx->last_int_start = 0;
    ctx->last_eig_sweeps = 0;
    for (size_t w = 0; w < hw.size(); ++w) {
        if (iters) iters[w] = hw[w].iter;
        ctx->window_iters += hw[w].iter; ctx->pass_b16 += hw[w].pass_b16;
        ctx->last_int_start += hw[w].int_gram ? 1 : 0;
        if (hw[w].refine == 2) ctx->refined_windows += 1;
        else if (hw[w].refine != 0) ctx->unrefined_windows += 1;
        if (hw[w].sweeps > ctx->last_eig_sweeps) ctx->last_eig_sweeps = hw[w].sweeps;
    }
}

int segment_inputs_impl(swk_ctx *ctx, const uint8_t *frames, int64_t fs, int64_t rs, int F, int x0, int y0, int frame_h, int frame_w,
                        const swk_segment *segs, const int32_t *nseg, int seg_cap, int min_h, int min_w, const float *mean,
                        const float *std_, int pad, bool nhwc, int first, int net_cap, float *net, int32_t *seg_frame, int32_t *total,
                        int32_t *skipped, int known_total = -1, const SegFrame *fr = nullptr)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int32_t *doffs;
    NEED(ctx, SL_SEGOFFS, ((size_t)F + 2) * 4, doffs);           // [F+1] prefix sums, then the skipped-box counter
    int32_t *dskip = doffs + F + 1;
    HIPCHK(ctx, hipMemsetAsync(dskip, 0, 4, s));
    if (fr) launch_segment_prefix_groups(s, nseg, fr, F, doffs);          // (seg_cap = the records' stride; caps per frame in fr)
    else launch_segment_prefix(s, nseg, F, seg_cap, doffs);
    int32_t tot = known_total;
    if (tot < 0) {          // the caller does not know how many segments the batch holds: one round trip
        HIPCHK(ctx, hipMemcpyAsync(&tot, doffs + F, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    *total = tot;
    if (skipped) *skipped = 0;
    int count = tot - first;
    if (count > net_cap) count = net_cap;
    if (count < 1) return SWK_OK;
    int32_t *dlarge;          // boxes with a side of 513..4096: [0] = how many, then 6 ints each
    NEED(ctx, SL_SEGLARGE, ((size_t)count * 6 + 1) * 4, dlarge);
    HIPCHK(ctx, hipMemsetAsync(dlarge, 0, 4, s));
    if (fr)
        launch_segment_inputs_groups(s, fr, segs, seg_cap, doffs, F, min_h, min_w, first, count, net, seg_frame, pad, nhwc, mean, std_, dskip, dlarge);
    else
        launch_segment_inputs(s, frames, fs, rs, frame_h, frame_w, x0, y0, segs, doffs, F, seg_cap,
                              min_h, min_w, first, count, net, seg_frame, pad, nhwc, mean, std_, dskip, dlarge);
    int32_t sk = 0, nlarge = 0;
    HIPCHK(ctx, hipMemcpyAsync(&sk, dskip, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(&nlarge, dlarge, 4, hipMemcpyDeviceToHost, s));
    int rc = sync(ctx);
    if (rc) return rc;
    if (skipped) *skipped = sk;
    if (nlarge > 0) {          // rare: the rows of net those boxes own are written by a second kernel
        launch_segment_inputs_large(s, fr ? nullptr : frames, fs, rs, fr, dlarge, nlarge > count ? count : nlarge, net, pad, nhwc, mean, std_);
        return sync(ctx);
    }
    return SWK_OK;
}

// rows x width bytes from src (rows spitch apart) to dst (dpitch apart): nothing when dst is src (an output written in place),
// one plain copy when both sides are dense
int copy_out(swk_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind)
{
    if (!dst || dst == src) return SWK_OK;
    if (dpitch == width && spitch == width) HIPCHK(ctx, hipMemcpyAsync(dst, src, width * rows, kind, ctx->stream));
    else HIPCHK(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, ctx->stream));
    return SWK_OK;
}

// ---- the batch driver of swk_batch_run (one group) and swk_batch_run_groups (G groups) ----------------
// plan_batch (batch_plan.h) turns (groups, outs) into a BatchPlan on the host: sub-batches, placement, staging, record flags and the
// layout of the descriptor tables.  run_batch refuses what the parameters, the plan or the device rule out, reserves every buffer
// (batch_buffers), then runs the stages below once, in order.  Each stage owns its fork -- one group: the uniform kernels, in the
// caller's device buffers where it may; several groups: the per-frame geometry kernels, driven by the descriptor tables, on library
// buffers -- and its profiling family.
std::array<uint8_t *, 6> out_planes(const swk_output &o) { return {o.gray, o.rpca, o.bilateral, o.thresh, o.opened, o.labels}; }

// What the batch path's filter (and, with `labels`, its labeller) cannot run, by the parameters alone: the message, or null
const char *params_refusal(const swk_params *p, bool labels)
{
    if (p->open_kh != 3 || p->open_kw != 3) return "only the (3,3) opening window is implemented";
    if (labels && p->connectivity != 4 && p->connectivity != 8) return "connectivity must be 4 or 8";
    // the fused filter kernel has one instantiation per radius 1..4 (ensure_bilateral's own check comes after the buffers)
    if (bilateral_radius(p->bil_d, p->bil_sigma_space) > 4) return "bilateral diameter > 9 is not supported";
    return nullptr;
}

struct BatchBuffers {
    uint8_t *roi = nullptr;                          // host groups' staged frames
    uint8_t *pl[6] = {};                             // stage planes: gray (X), sparse image (S), bilateral, threshold, opened, labels
    double *pn = nullptr;                            // host outputs' A / E staging, (pixels, frames) layout
    swk_segment *dsegs = nullptr; int32_t *dnseg = nullptr;
    CclBuffers cb{};
    size_t lds = 0;                                  // the largest ccl_frame_lds_bytes of the fused groups (0: none is)
    std::vector<char> fused;                         // per group: its frames take the one-workgroup labeller
    uint8_t *tmp_in = nullptr, *tmp_out = nullptr;   // several groups: dense copy of an unfused group's opened / label planes
    uint8_t *dtab = nullptr;                         // several groups: the descriptor tables
};

// Every buffer of a batch call, before its first launch: a later NEED may not move one a queued kernel uses, so no stage calls NEED.
int batch_buffers(swk_ctx *ctx, const BatchPlan &plan, const swk_input *groups, const swk_output *outs, BatchBuffers *buf)
{
    const int G = (int)plan.grp.size(), n = plan.n, F = plan.F;
    const bool single = plan.single;
    if (plan.roi_bytes) NEED(ctx, SL_ROI, plan.roi_bytes, buf->roi);
    // One group works in the caller's device buffers (mem = SWK_MEM_DEVICE or planes_on_device) -- but a gray plane whose size is not
    // a whole number of dwords stays in the library's padded buffer: k_gram_u8 reads it in dwords; the caller's copy is made at the end
    const bool in_place = single && (outs[0].mem == SWK_MEM_DEVICE || outs[0].planes_on_device != 0);
    const Slot plane_slot[6] = {SL_X, SL_S, SL_BIL, SL_THR, SL_OPEN, SL_LAB8};
    for (int i = 0; i < 6; ++i) {
        bool wanted = i != 2 && i != 3;          // the filter writes the bilateral and threshold images only when asked for
        for (int g = 0; g < G; ++g) wanted = wanted || out_planes(outs[g])[i];
        if (!wanted) continue;
        uint8_t *mine = in_place ? out_planes(outs[0])[i] : nullptr;
        if (i == 0 && ((size_t)F * groups[0].Hc * groups[0].Wc) % 4) mine = nullptr;
        if (!mine) NEED(ctx, plane_slot[i], plan.total + (i == 0 ? 4 : 0), mine);
        buf->pl[i] = mine;
    }
    if (plan.pn_bytes) NEED(ctx, SL_PN, plan.pn_bytes, buf->pn);
    if (plan.want_props) {
        const bool rec_in_place = single && outs[0].mem == SWK_MEM_DEVICE;          // one group's device records are written in place
        if (rec_in_place && outs[0].segs) buf->dsegs = outs[0].segs;
        else NEED(ctx, SL_SEGS, (size_t)F * plan.capmax * sizeof(swk_segment), buf->dsegs);
        if (rec_in_place && outs[0].nseg) buf->dnseg = outs[0].nseg; else NEED(ctx, SL_NSEG, (size_t)F * 4, buf->dnseg);
    }
    // labelling: the one-workgroup-per-frame kernel for every group that fits it, the multi-kernel path for the others (several
    // groups: on a dense copy of the group's planes)
    size_t Pp = 1, words = 1, ccl_F = 1, ccl_Pp = 1, ccl_words_ = 1, tmp_bytes = 16;
    buf->fused.resize(G);
    for (int g = 0; g < G; ++g) {
        const int H = groups[g].Hc, W = groups[g].Wc, Fg = groups[g].nwin * n;
        buf->fused[g] = !ctx->force_ccl_multi && ccl_frame_supported(H, W);
        Pp = std::max(Pp, ccl_padded(H, W));
        words = std::max(words, ccl_words(H, W));
        if (buf->fused[g]) buf->lds = std::max(buf->lds, ccl_frame_lds_bytes(H, W));
        else {
            ccl_F = std::max(ccl_F, (size_t)Fg);
            ccl_Pp = std::max(ccl_Pp, ccl_padded(H, W));
            ccl_words_ = std::max(ccl_words_, ccl_words(H, W));
            if (!single) tmp_bytes = std::max(tmp_bytes, (size_t)Fg * H * W);
        }
    }
    CclBuffers &cb = buf->cb;
    cb.Pp = (int)Pp;
    cb.words = (int)words;          // (the geometry kernel takes each frame's own)
    NEED(ctx, SL_PARENT, std::max((size_t)F * Pp, ccl_F * ccl_Pp) * 4, cb.parent);
    NEED(ctx, SL_ROOTBITS, ccl_F * ccl_words_ * 4, cb.rootbits);
    NEED(ctx, SL_WORDPREFIX, ccl_F * ccl_words_ * 4, cb.wordprefix);
    NEED(ctx, SL_NCOMP, (size_t)F * 4, cb.ncomp);
    NEED(ctx, SL_TABLE, ccl_F * 256 * 8 * 4, cb.table);
    NEED(ctx, SL_SUMS, ccl_F * 256 * 2 * 8, cb.sums);
    if (tmp_bytes > 16) { NEED(ctx, SL_TMP_IN, tmp_bytes, buf->tmp_in); NEED(ctx, SL_TMP_OUT, tmp_bytes, buf->tmp_out); }
    if (!single) NEED(ctx, SL_GRP, plan.tab_bytes, buf->dtab);
    return SWK_OK;
}

// One batch call: its arguments, plan and buffers, and what a stage leaves for a later one.
struct Batch {
    swk_ctx *ctx; const swk_input *groups; int G; const swk_params *p; swk_output *outs;
    BatchPlan plan;
    BatchBuffers buf;
    std::vector<BatchView> view;          // where the kernels find each group's frames
    std::vector<uint8_t> tab;             // host image of the descriptor tables (uploaded asynchronously: lives until the call's final sync)
    std::vector<IalmWin> hw_sub;          // window state, sub-batch order
    IalmRun run{};                        // the last sub-batch's IALM
};

// A or E of group g, (pixels, frames) layout: the caller's device buffer, or the group's part of the host outputs' staging buffer
double *ae_dst(const Batch &b, int g, int which)
{
    double *dst = which == 0 ? b.outs[g].A : b.outs[g].E;
    return dst && b.outs[g].mem == SWK_MEM_HOST ? b.buf.pn + b.plan.grp[g].pn_off / 8 : dst;
}

// inputs: host groups staged one after the other into the ROI buffer
int batch_inputs(Batch &b)
{
    b.view.resize(b.G);
    for (int g = 0; g < b.G; ++g) {
        const swk_input *in = &b.groups[g];
        BatchView &v = b.view[g];
        v = {in->frames, in->frame_stride, in->row_stride, in->x0, in->y0};
        if (in->mem == SWK_MEM_HOST) {
            Timed t(b.ctx, SWK_K_COPY);
            const int rc = host_stage_copy(b.ctx, in, b.plan.grp[g].stage, b.buf.roi + b.plan.grp[g].roi_off, &v.frames, &v.fs, &v.rs, &v.x0, &v.y0);
            if (rc) return rc;
        }
    }
    return SWK_OK;
}

// several groups: the descriptor tables, one upload
int batch_tables(Batch &b)
{
    if (b.plan.single) return SWK_OK;
    std::vector<BatchAE> ae(b.G);
    for (int g = 0; g < b.G; ++g) ae[g] = {ae_dst(b, g, 0), ae_dst(b, g, 1)};
    b.tab.assign(b.plan.tab_bytes, 0);
    fill_batch_tables(b.plan, b.groups, b.outs, b.view.data(), ae.data(), b.buf.fused.data(), b.tab.data());
    HIPCHK(b.ctx, hipMemcpyAsync(b.buf.dtab, b.tab.data(), b.plan.tab_bytes, hipMemcpyHostToDevice, b.ctx->stream));
    return SWK_OK;
}

// gray + ROI gather into the (padded) X planes
void batch_gray(Batch &b)
{
    const BatchPlan &pl = b.plan;
    const swk_input &in = b.groups[0];
    const BatchView &v = b.view[0];
    Timed t(b.ctx, SWK_K_GRAY);
    if (pl.single) launch_gray(b.ctx->stream, v.frames, in.channels, v.fs, v.rs, v.x0, v.y0, pl.F, in.Hc, in.Wc, b.p->gray_mode, b.buf.pl[0]);
    else launch_gray_groups(b.ctx->stream, (const GroupWin *)(b.buf.dtab + pl.o_win), pl.F, pl.n, pl.Pmax, b.p->gray_mode, b.buf.pl[0]);
}

// IALM per sub-batch; its float64 factors leave before the next sub-batch reuses the workspaces
int batch_ialm(Batch &b)
{
    swk_ctx *ctx = b.ctx;
    const BatchPlan &pl = b.plan;
    const swk_params *p = b.p;
    hipStream_t s = ctx->stream;
    const int n = pl.n;
    for (size_t k = 0; k < pl.subs.size(); ++k) {
        const BatchSub &sb = pl.subs[k];
        // (several groups: each window's own pixel count, from the scatter table, bounds the accurate first iteration's work)
        const IalmJob job{b.buf.pl[0] + sb.off, b.buf.pl[1] + sb.off, sb.nwin, n, sb.P,
                          pl.single ? nullptr : (const PnWin *)(b.buf.dtab + pl.o_pa) + sb.w0, p->lmbda, p->tol, p->maxiter};
        int rc = run_ialm(ctx, job, sb.A, sb.E, &b.run);
        if (rc) return rc;
        for (int which = 0; which < 2; ++which) {
            if (!(which == 0 ? sb.A : sb.E)) continue;
            const double *planes = which == 0 ? b.run.A : b.run.E;
            {
                Timed t(ctx, SWK_K_COPY);
                if (pl.single) launch_planes_to_pn(s, planes, ae_dst(b, 0, which), sb.nwin, n, sb.P, b.run.pstride, b.run.fpad);
                else launch_planes_to_pn_groups(s, planes, (const PnWin *)(b.buf.dtab + (which == 0 ? pl.o_pa : pl.o_pe)) + sb.w0, sb.nwin, n,
                                                sb.P, b.run.pstride, b.run.fpad);
            }
            for (int g : sb.gs) {
                double *dst = which == 0 ? b.outs[g].A : b.outs[g].E;
                if (dst && b.outs[g].mem == SWK_MEM_HOST)
                    HIPCHK(ctx, hipMemcpyAsync(dst, ae_dst(b, g, which), (size_t)b.groups[g].nwin * n * b.groups[g].Hc * b.groups[g].Wc * 8,
                                               hipMemcpyDeviceToHost, s));
            }
        }
        // the next sub-batch reuses the window-state slot: this one's state is read now (the last one's after the final sync)
        if (k + 1 < pl.subs.size() && (rc = read_windows(ctx, b.run, b.hw_sub))) return rc;
    }
    return SWK_OK;
}

// bilateral + threshold + opening
void batch_filter(Batch &b)
{
    swk_ctx *ctx = b.ctx;
    const BatchPlan &pl = b.plan;
    uint8_t *const *d = b.buf.pl;
    Timed t(ctx, SWK_K_FILTER);
    if (pl.single) launch_filter_fused(ctx->stream, d[1], pl.F, b.groups[0].Hc, b.groups[0].Wc, ctx->bil, b.p->bil_fma, b.p->thresh, d[2], d[3], d[4]);
    else launch_filter_fused_geom(ctx->stream, d[1], pl.F, pl.Hmax, pl.Wmax, (const FrameGeom *)(b.buf.dtab + pl.o_gf), pl.total, ctx->bil,
                                  b.p->bil_fma, b.p->thresh, d[2], d[3], d[4]);
}

// labels + region properties: one launch for the fused groups, the multi-kernel path for every other group
int batch_labels(Batch &b)
{
    swk_ctx *ctx = b.ctx;
    const BatchPlan &pl = b.plan;
    const BatchBuffers &buf = b.buf;
    const swk_params *p = b.p;
    hipStream_t s = ctx->stream;
    const bool single = pl.single;
    const int n = pl.n, F = pl.F, capmax = pl.capmax;
    uint8_t *const dOpen = buf.pl[4], *const dLab = buf.pl[5];
    if (pl.want_props) HIPCHK(ctx, hipMemsetAsync(buf.dsegs, 0, (size_t)F * capmax * sizeof(swk_segment), s));
    if (buf.lds) {
        Timed t(ctx, SWK_K_CCL);
        if (single) launch_ccl_frame(s, dOpen, F, b.groups[0].Hc, b.groups[0].Wc, p->connectivity, p->label_order, buf.cb, nullptr, dLab,
                                     pl.want_props, capmax, buf.dsegs, buf.dnseg);
        else launch_ccl_frame_geom(s, dOpen, F, (const FrameGeom *)(buf.dtab + pl.o_gc), buf.lds, pl.vec, p->connectivity, p->label_order,
                                   buf.cb, dLab, capmax, buf.dsegs, buf.dnseg);
    }
    for (int g = 0; g < b.G; ++g) {
        if (buf.fused[g]) continue;
        const BatchGroup &bg = pl.grp[g];
        const int H = b.groups[g].Hc, W = b.groups[g].Wc, P = H * W, Fg = b.groups[g].nwin * n, pitch = bg.pitch;
        const int f0 = bg.win0 * n;
        CclBuffers gb = buf.cb;
        gb.Pp = (int)ccl_padded(H, W);
        gb.words = (int)ccl_words(H, W);
        gb.ncomp = buf.cb.ncomp + f0;
        uint8_t *src = single ? dOpen : buf.tmp_in, *lab = single ? dLab : buf.tmp_out;
        if (!single) HIPCHK(ctx, hipMemcpy2DAsync(buf.tmp_in, P, dOpen + bg.goff, pitch, P, Fg, hipMemcpyDeviceToDevice, s));
        { Timed t(ctx, SWK_K_CCL); launch_ccl(s, src, Fg, H, W, p->connectivity, p->label_order, gb, nullptr, lab); }
        if (pl.want_props) {
            Timed t(ctx, SWK_K_PROPS);
            launch_regionprops(s, lab, Fg, H, W, gb, capmax, buf.dsegs + (size_t)f0 * capmax, buf.dnseg + f0);
        }
        if (!single) HIPCHK(ctx, hipMemcpy2DAsync(dLab + bg.goff, pitch, buf.tmp_out, P, P, Fg, hipMemcpyDeviceToDevice, s));
    }
    return SWK_OK;
}

// outputs, group by group, in swk_batch_run's layouts (what was written in place is not copied)
int batch_outputs(Batch &b)
{
    swk_ctx *ctx = b.ctx;
    const BatchPlan &pl = b.plan;
    const size_t capmax = pl.capmax;
    int rc;
    Timed t(ctx, SWK_K_COPY);
    for (int g = 0; g < b.G; ++g) {
        const swk_output *out = &b.outs[g];
        const BatchGroup &bg = pl.grp[g];
        const size_t P = (size_t)b.groups[g].Hc * b.groups[g].Wc, Fg = (size_t)b.groups[g].nwin * pl.n, pitch = bg.pitch;
        const size_t f0 = (size_t)bg.win0 * pl.n;
        const bool dev_planes = out->mem == SWK_MEM_DEVICE || out->planes_on_device != 0;
        const hipMemcpyKind pk = dev_planes ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        const hipMemcpyKind ok = out->mem == SWK_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        const std::array<uint8_t *, 6> dst = out_planes(*out);
        for (int i = 0; i < 6; ++i)
            if (dst[i] && (rc = copy_out(ctx, dst[i], P, b.buf.pl[i] + bg.goff, pitch, P, Fg, pk))) return rc;
        const size_t rec = sizeof(swk_segment);
        if (out->segs && (rc = copy_out(ctx, out->segs, out->seg_cap * rec, b.buf.dsegs + f0 * capmax, capmax * rec, out->seg_cap * rec, Fg, ok)))
            return rc;
        if (out->nseg && (rc = copy_out(ctx, out->nseg, Fg * 4, b.buf.dnseg + f0, Fg * 4, Fg * 4, 1, ok))) return rc;
    }
    return SWK_OK;
}

// after the call's final sync: iteration counts (sub-batch order -> call order) and the record swk_segment_inputs_last reads
int batch_epilogue(Batch &b)
{
    swk_ctx *ctx = b.ctx;
    const BatchPlan &pl = b.plan;
    const int G = b.G, n = pl.n;
    int rc = read_windows(ctx, b.run, b.hw_sub);
    if (rc) return rc;
    std::vector<IalmWin> hw(pl.nwin);
    for (int g = 0; g < G; ++g)
        for (int wl = 0; wl < b.groups[g].nwin; ++wl) hw[pl.grp[g].win0 + wl] = b.hw_sub[pl.grp[g].swin0 + wl];
    std::vector<int32_t> it(pl.nwin);
    account_iters(ctx, hw, it.data());
    bool uploaded = false;
    for (int g = 0; g < G; ++g) {
        const swk_output &out = b.outs[g];
        const int32_t *mine = it.data() + pl.grp[g].win0;
        if (!out.iters) continue;
        if (out.mem == SWK_MEM_DEVICE) {
            HIPCHK(ctx, hipMemcpyAsync(out.iters, mine, (size_t)b.groups[g].nwin * 4, hipMemcpyHostToDevice, ctx->stream));
            uploaded = true;
        } else memcpy(out.iters, mine, (size_t)b.groups[g].nwin * 4);
    }
    if (uploaded) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // `it` is a local
    if (!pl.seg_last) return SWK_OK;
    swk_ctx::LastBatch &lb = ctx->last;
    lb = swk_ctx::LastBatch{};
    lb.nwin = pl.nwin; lb.n = n;
    lb.segs = b.buf.dsegs; lb.nseg = b.buf.dnseg; lb.cap = pl.capmax;
    if (pl.single) {          // one geometry: k_segment_inputs
        const BatchView &v = b.view[0];
        lb.frames = v.frames; lb.fs = v.fs; lb.rs = v.rs;
        lb.Hc = b.groups[0].Hc; lb.Wc = b.groups[0].Wc; lb.x0 = v.x0; lb.y0 = v.y0; lb.frame_h = v.frame_h(); lb.frame_w = v.frame_w();
    } else {
        lb.fr = (const SegFrame *)(b.buf.dtab + pl.o_sf);          // per-frame frames and geometry: k_segment_inputs_groups
    }
    if (pl.host_total) {
        lb.total = 0;
        for (int g = 0; g < G; ++g)
            for (int f = 0; f < b.groups[g].nwin * n; ++f) lb.total += std::min(b.outs[g].nseg[f], b.outs[g].seg_cap);
    }
    lb.valid = true;
    return SWK_OK;
}

int run_batch(swk_ctx *ctx, const swk_input *groups, int G, const swk_params *p, swk_output *outs)
{
    if (const char *msg = params_refusal(p, true)) return fail(ctx, SWK_ERR_ARG, msg);
    Batch b{ctx, groups, G, p, outs};
    const BatchPlan &pl = b.plan;
    const char *why = nullptr;
    int rc = plan_batch(groups, G, outs, &b.plan, &why);
    if (rc) return fail(ctx, rc, why);
    // capacity, checked here so that a refused call launches nothing: the grid's y extent, and run_ialm's limit on the padded plane
    // (at the wider fpad of the two pass families: its reruns may take the other)
    const int fpad_max = std::max(ialm_fpad(true, pl.n), ialm_fpad(false, pl.n));
    for (const BatchSub &sb : pl.subs) {
        if ((rc = check_windows(ctx, sb.nwin))) return rc;
        if ((int64_t)fpad_max * ialm_pstride(sb.P) >= (1ll << 28))
            return fail(ctx, SWK_ERR_ARG, "window too large: frames x padded ROI pixels must stay below 2^28");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->last.valid = false;
    ctx->last_stage.resize(G);
    for (int g = 0; g < G; ++g) ctx->last_stage[g] = pl.grp[g].stage.kind;
    if ((rc = batch_buffers(ctx, pl, groups, outs, &b.buf))) return rc;
    if ((rc = ensure_bilateral(ctx, p->bil_d, p->bil_sigma_color, p->bil_sigma_space))) return rc;          // (slots of its own)
    if ((rc = batch_inputs(b))) return rc;
    if ((rc = batch_tables(b))) return rc;
    batch_gray(b);
    if ((rc = batch_ialm(b))) return rc;
    batch_filter(b);
    if ((rc = batch_labels(b))) return rc;
    if ((rc = batch_outputs(b))) return rc;
    if ((rc = sync(ctx))) return rc;
    return batch_epilogue(b);
}

}  // namespace

// =====================================================================================
#pragma GCC visibility push(default)
extern "C" {

int32_t swk_abi_version(void) { return SWK_ABI_VERSION; }

void swk_params_default(swk_params *p)
{
    memset(p, 0, sizeof *p);
    p->lmbda = 0.01; p->tol = 0.001; p->maxiter = 100;
    p->bil_d = 7; p->bil_sigma_color = 15.0; p->bil_sigma_space = 1.0; p->bil_fma = 0;
    p->thresh = 15; p->open_kh = 3; p->open_kw = 3;
    p->connectivity = 8; p->label_order = SWK_ORDER_BLOCK2X2; p->gray_mode = SWK_GRAY_Q14;
}

const char *swk_last_error(const swk_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int32_t swk_ctx_create(int32_t device, int32_t max_windows, int32_t max_n, int32_t max_Hc, int32_t max_Wc, swk_ctx **out)
{
    if (!out) return SWK_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        g_create_error = "no HIP device visible: libswk has no CPU fallback";
        return SWK_ERR_NOGPU;
    }
    if (device < 0 || device >= count) { g_create_error = "device index out of range"; return SWK_ERR_ARG; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return SWK_ERR_HIP; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName + ", libswk is built for gfx950 (MI355X) only";
        return SWK_ERR_NOGPU;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return SWK_ERR_HIP; }
    int grid_y = 0;
    if (hipDeviceGetAttribute(&grid_y, hipDeviceAttributeMaxGridDimY, device) != hipSuccess || grid_y < 1) {
        g_create_error = "hipDeviceGetAttribute(hipDeviceAttributeMaxGridDimY) failed";
        return SWK_ERR_HIP;
    }
    swk_ctx *ctx = new swk_ctx();
    ctx->device = device;
    ctx->max_grid_y = grid_y;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&ctx->h_active, 256, hipHostMallocDefault) != hipSuccess) {
        g_create_error = "stream / pinned memory creation failed";
        delete ctx;
        return SWK_ERR_HIP;
    }
    // pre-size the big workspaces so the first batch does not pay for hipMalloc
    if (max_windows > 0 && max_n > 0 && max_Hc > 0 && max_Wc > 0) {
        const size_t elems = (size_t)max_windows * max_n * max_Hc * max_Wc;
        void *p;
        int rc = 0;
        rc = rc ? rc : need(ctx, SL_X, elems + 4, &p);
        rc = rc ? rc : need(ctx, SL_S, elems, &p);
        rc = rc ? rc : need(ctx, SL_OPEN, elems, &p);
        rc = rc ? rc : need(ctx, SL_LAB8, elems, &p);
        const size_t felems = (size_t)max_windows * ialm_fpad(false, max_n) * ialm_pstride((int64_t)max_Hc * max_Wc);
        rc = rc ? rc : need(ctx, SL_A, felems * 8, &p);
        rc = rc ? rc : need(ctx, SL_Y, felems * 8, &p);
        if (rc) { g_create_error = ctx->err; swk_ctx_destroy(ctx); return rc; }
    }
    *out = ctx;
    return SWK_OK;
}

void swk_ctx_destroy(swk_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    drain_prof(ctx);
    for (auto e : ctx->pool) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i)
        if (ctx->ev_poll[i]) (void)hipEventDestroy(ctx->ev_poll[i]);
    for (int i = 0; i < SL_COUNT; ++i)
        if (ctx->slot[i]) (void)hipFree(ctx->slot[i]);
    if (ctx->h_active) (void)hipHostFree(ctx->h_active);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int64_t swk_ctx_device_bytes(const swk_ctx *ctx)
{
    int64_t t = 0;
    if (ctx) for (int i = 0; i < SL_COUNT; ++i) t += (int64_t)ctx->slot_bytes[i];
    return t;
}

int32_t swk_prof_enable(swk_ctx *ctx, int32_t on) { if (!ctx) return SWK_ERR_ARG; ctx->prof_on = on != 0; return SWK_OK; }
int32_t swk_prof_reset(swk_ctx *ctx)
{
    if (!ctx) return SWK_ERR_ARG;
    memset(ctx->prof_ms, 0, sizeof ctx->prof_ms);
    memset(ctx->prof_n, 0, sizeof ctx->prof_n);
    ctx->window_iters = 0;
    ctx->pass_b16 = 0;
    return SWK_OK;
}
int32_t swk_prof_get(swk_ctx *ctx, int32_t family, double *ms_total, int64_t *launches)
{
    if (!ctx || family < 0 || family >= SWK_K_COUNT) return SWK_ERR_ARG;
    if (ms_total) *ms_total = ctx->prof_ms[family];
    if (launches) *launches = ctx->prof_n[family];
    return SWK_OK;
}
int32_t swk_prof_window_iters(swk_ctx *ctx, int64_t *window_iters)
{
    if (!ctx || !window_iters) return SWK_ERR_ARG;
    *window_iters = ctx->window_iters;
    return SWK_OK;
}
int32_t swk_set_ialm_variant(swk_ctx *ctx, int32_t variant)
{
    if (!ctx || variant < 0 || variant > 6 || variant == 3) return SWK_ERR_ARG;          // 3 was round 1's M-state kernel (removed)
    ctx->ialm_variant = variant;
    return SWK_OK;
}

// Page-locked host memory for the caller's staging buffers: a host -> device copy out of it is one DMA instead of a
// driver-side staging copy plus a DMA (the FrameQueue drop-in stacks a window's crops into such a buffer).
int32_t swk_pinned_alloc(int32_t device, int64_t bytes, void **out)
{
    if (!out || bytes < 1 || device < 0) return SWK_ERR_ARG;
    *out = nullptr;
    // on the GPU the buffer feeds (a thread that has not chosen a device would otherwise open a context on GPU 0); portable: every
    // context of the process may copy out of it
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return SWK_ERR_ARG; }
    if (hipHostMalloc(out, (size_t)bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return SWK_ERR_NOMEM; }
    return SWK_OK;
}

int32_t swk_pinned_free(void *p)
{
    if (!p) return SWK_OK;
    return hipHostFree(p) == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

int32_t swk_device_alloc(swk_ctx *ctx, int64_t bytes, void **out)
{
    if (!ctx || !out || bytes < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (hipMalloc(out, (size_t)bytes) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return fail(ctx, SWK_ERR_NOMEM, "hipMalloc failed"); }
    return SWK_OK;
}

int32_t swk_device_free(swk_ctx *ctx, void *p)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!p) return SWK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipFree(p));
    return SWK_OK;
}

int32_t swk_device_read(swk_ctx *ctx, const void *src_device, void *dst_host, int64_t bytes)
{
    if (!ctx || !src_device || !dst_host || bytes < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(dst_host, src_device, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SWK_OK;
}

int32_t swk_set_pass_tuning(swk_ctx *ctx, int32_t flags)
{
    if (!ctx || flags < 0 || flags > 3) return SWK_ERR_ARG;
    ctx->pass_tune = flags;
    return SWK_OK;
}

int32_t swk_set_sparse_speculation(swk_ctx *ctx, double factor)
{
    if (!ctx) return SWK_ERR_ARG;
    ctx->sparse_spec = factor;
    return SWK_OK;
}
int32_t swk_set_integer_start(swk_ctx *ctx, int32_t on)
{
    if (!ctx) return SWK_ERR_ARG;
    ctx->use_gram8 = on ? 1 : 0;
    return SWK_OK;
}
int32_t swk_set_norm_guard(swk_ctx *ctx, double rel)
{
    if (!ctx || !(rel >= 0.0) || rel >= 1.0) return SWK_ERR_ARG;
    ctx->norm_guard = rel;
    return SWK_OK;
}
int32_t swk_prof_guard_windows(swk_ctx *ctx, int64_t *windows)
{
    if (!ctx || !windows) return SWK_ERR_ARG;
    *windows = ctx->guard_windows;
    return SWK_OK;
}
int32_t swk_set_norm_speculation(swk_ctx *ctx, double factor)
{
    if (!ctx) return SWK_ERR_ARG;
    ctx->norm_spec = factor;
    return SWK_OK;
}
int32_t swk_prof_pass_bytes_per_element(swk_ctx *ctx, double *bytes)
{
    if (!ctx || !bytes) return SWK_ERR_ARG;
    *bytes = (double)ctx->pass_b16 / 16.0;
    return SWK_OK;
}
int32_t swk_last_eig_sweeps(swk_ctx *ctx, int32_t *sweeps)
{
    if (!ctx || !sweeps) return SWK_ERR_ARG;
    *sweeps = ctx->last_eig_sweeps;
    return SWK_OK;
}
int32_t swk_last_integer_start_windows(swk_ctx *ctx, int32_t *windows)
{
    if (!ctx || !windows) return SWK_ERR_ARG;
    *windows = ctx->last_int_start;
    return SWK_OK;
}
int32_t swk_last_host_stage(swk_ctx *ctx, int32_t *kinds, int32_t cap)
{
    if (!ctx || (!kinds && cap > 0)) return SWK_ERR_ARG;
    const int32_t G = (int32_t)ctx->last_stage.size();
    for (int32_t g = 0; g < G && g < cap; ++g) kinds[g] = ctx->last_stage[g];
    return G;
}
int32_t swk_prof_redo_batches(swk_ctx *ctx, int64_t *batches)
{
    if (!ctx || !batches) return SWK_ERR_ARG;
    *batches = ctx->redo_batches;
    return SWK_OK;
}

int32_t swk_set_start_refine(swk_ctx *ctx, double tau)
{
    if (!ctx) return SWK_ERR_ARG;
    ctx->start_refine = tau;
    return SWK_OK;
}
int32_t swk_prof_refined_windows(swk_ctx *ctx, int64_t *refined, int64_t *unrefined)
{
    if (!ctx) return SWK_ERR_ARG;
    if (refined) *refined = ctx->refined_windows;
    if (unrefined) *unrefined = ctx->unrefined_windows;
    return SWK_OK;
}

int32_t swk_last_stopping_norms(swk_ctx *ctx, double *ratio, double *err_bound, int32_t cap)
{
    if (!ctx || cap < 0) return SWK_ERR_ARG;
    const int n = (int)ctx->last_hw.size();
    for (int w = 0; w < n && w < cap; ++w) {
        if (ratio) ratio[w] = ctx->last_hw[w].last_ratio;
        if (err_bound) err_bound[w] = ctx->last_hw[w].norm_err;
    }
    return n;
}

int32_t swk_prof_redo_windows(swk_ctx *ctx, int64_t *windows)
{
    if (!ctx || !windows) return SWK_ERR_ARG;
    *windows = ctx->redo_windows;
    return SWK_OK;
}

int32_t swk_debug_force_ccl_multi_kernel(swk_ctx *ctx, int32_t on)
{
    if (!ctx) return SWK_ERR_ARG;
    ctx->force_ccl_multi = on != 0;
    return SWK_OK;
}

int32_t swk_debug_max_windows(swk_ctx *ctx) { return ctx ? ctx->max_grid_y : SWK_ERR_ARG; }

int32_t swk_set_eig_method(swk_ctx *ctx, int32_t method)
{
    if (!ctx || method < 0 || method > 1) return SWK_ERR_ARG;
    ctx->eig_method = method;
    return SWK_OK;
}

// -------------------------------------------------------------------------------------
int32_t swk_batch_run(swk_ctx *ctx, const swk_input *in, const swk_params *p, swk_output *out)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!in || !p || !out) return fail(ctx, SWK_ERR_ARG, "null argument");
    return run_batch(ctx, in, 1, p, out);
}

// Several groups of windows (one video's windows each, every one with its own geometry and memory) in ONE call (run_batch).
int32_t swk_batch_run_groups(swk_ctx *ctx, const swk_input *groups, int32_t ngroups, const swk_params *p, swk_output *outs)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!groups || !p || !outs || ngroups < 1) return fail(ctx, SWK_ERR_ARG, "null argument");
    return run_batch(ctx, groups, ngroups, p, outs);
}

// ---- stage-level entry points (host buffers) ----------------------------------------
int32_t swk_bgr2gray(swk_ctx *ctx, const uint8_t *bgr, int32_t count, int32_t H, int32_t W, int32_t gray_mode, uint8_t *gray)
{
    if (!ctx || !bgr || !gray || count < 1 || H < 1 || W < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)count * H * W;
    uint8_t *din, *dout;
    NEED(ctx, SL_TMP_IN, px * 3, din);
    NEED(ctx, SL_TMP_OUT, px, dout);
    HIPCHK(ctx, hipMemcpyAsync(din, bgr, px * 3, hipMemcpyHostToDevice, ctx->stream));
    launch_gray(ctx->stream, din, 3, (int64_t)H * W * 3, (int64_t)W * 3, 0, 0, count, H, W, gray_mode, dout);
    HIPCHK(ctx, hipMemcpyAsync(gray, dout, px, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

// rows x width bytes of each of `count` frames between a host plane (first byte host, rows rs apart, frames fs apart) and its dense
// copy on the device (dev), up = host to device.  ((size_t)rs == width implies rs > 0: width >= 1.)
static int copy_rects(swk_ctx *ctx, uint8_t *dev, const uint8_t *host, int64_t rs, int64_t fs, size_t width, size_t rows, int count, bool up)
{
    const size_t per = width * rows;
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    uint8_t *h = const_cast<uint8_t *>(host);                         // (written only on the way down)
    const bool rows_dense = (size_t)rs == width;
    const bool one = rows_dense && (count == 1 || fs == (int64_t)per);                // the frames are dense too: one copy for all
    const int copies = one ? 1 : count;
    const size_t bytes = one ? per * count : per;
    for (int f = 0; f < copies; ++f) {
        uint8_t *d = dev + (size_t)f * per, *s = h + (int64_t)f * fs;
        if (rows_dense) HIPCHK(ctx, hipMemcpyAsync(up ? d : s, up ? s : d, bytes, kind, ctx->stream));
        else HIPCHK(ctx, hipMemcpy2DAsync(up ? d : s, up ? width : (size_t)rs, up ? s : d, up ? (size_t)rs : width, width, rows, kind, ctx->stream));
    }
    return SWK_OK;
}

// what swk_yuv_to_bgr and swk_yuv_deinterlace refuse alike, after their null and layout checks (bgr_mem: where the BGR result goes)
static int yuv_refusal(swk_ctx *ctx, const swk_yuv *src, int32_t count, int32_t x0, int32_t y0, int32_t Hr, int32_t Wr, int32_t bgr_mem)
{
    const bool semi = src->layout == SWK_YUV_SEMIPLANAR, mono = src->layout == SWK_YUV_MONO;
    if (src->bits < 8 || src->bits > 16) return fail(ctx, SWK_ERR_ARG, "bits must be in 8..16");
    const int sx = mono ? 0 : src->sx, sy = mono ? 0 : src->sy;
    if (sx < 0 || sx > 2 || sy < 0 || sy > 1) return fail(ctx, SWK_ERR_ARG, "chroma subsampling shifts must be sx 0..2 and sy 0..1");
    if (!src->y || (!mono && !src->u) || (!mono && !semi && !src->v)) return fail(ctx, SWK_ERR_ARG, "null YUV plane");
    if (count < 1 || count > (1 << 24)) return fail(ctx, SWK_ERR_ARG, "count must be in 1..2^24");
    if ((src->mem != SWK_MEM_HOST && src->mem != SWK_MEM_DEVICE) || (bgr_mem != SWK_MEM_HOST && bgr_mem != SWK_MEM_DEVICE))
        return fail(ctx, SWK_ERR_ARG, "mem must be SWK_MEM_HOST or SWK_MEM_DEVICE");
    const int H = src->H, W = src->W;
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return fail(ctx, SWK_ERR_ARG, "frame size must be 1..32768 on each side");
    if (x0 < 0 || y0 < 0 || Hr < 1 || Wr < 1 || (int64_t)x0 + Wr > W || (int64_t)y0 + Hr > H)
        return fail(ctx, SWK_ERR_ARG, "rectangle outside the frame");
    const int B = src->bits > 8 ? 2 : 1;                              // bytes per sample
    const int cbytes = semi ? 2 * B : B;                              // bytes per chroma sample position in a chroma row
    const int cwf = ((W - 1) >> sx) + 1;                              // chroma samples in a row of the frame
    if (src->y_row_stride < (int64_t)W * B || (!mono && src->c_row_stride < (int64_t)cwf * cbytes))
        return fail(ctx, SWK_ERR_ARG, "row stride smaller than a row");
    if (B == 2) {
        const bool frames = count > 1;
        if ((src->y_row_stride & 1) || (frames && (src->y_frame_stride & 1)) ||
            (!mono && ((src->c_row_stride & 1) || (frames && (src->c_frame_stride & 1)))))
            return fail(ctx, SWK_ERR_ARG, "odd stride with 2-byte samples");
        if (((uintptr_t)src->y & 1) || (!mono && ((uintptr_t)src->u & 1)) || (!mono && !semi && ((uintptr_t)src->v & 1)))
            return fail(ctx, SWK_ERR_ARG, "odd plane address with 2-byte samples");
    }
    return SWK_OK;
}

// swk_yuv_to_bgr after its null and layout checks; yuv420: swk_yuv420_to_bgr's view of its argument (sx = sy = 1, bits = 8, where
// the checks of bits, shifts and 2-byte samples cannot fire), which takes its own launcher
static int yuv_call(swk_ctx *ctx, const swk_yuv *src, bool yuv420, int32_t count, int32_t x0, int32_t y0, int32_t Hr, int32_t Wr, uint8_t *bgr,
                    int32_t bgr_mem)
{
    const int refused = yuv_refusal(ctx, src, count, x0, y0, Hr, Wr, bgr_mem);
    if (refused) return refused;
    const bool semi = src->layout == SWK_YUV_SEMIPLANAR, mono = src->layout == SWK_YUV_MONO;
    const int sx = mono ? 0 : src->sx, sy = mono ? 0 : src->sy;
    const int B = src->bits > 8 ? 2 : 1;                              // bytes per sample
    const int cbytes = semi ? 2 * B : B;                              // bytes per chroma sample position in a chroma row
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t out_b = (size_t)count * Hr * Wr * 3;
    const uint8_t *dy = src->y, *du = mono ? nullptr : src->u, *dv = mono || semi ? nullptr : src->v;
    int64_t y_rs = src->y_row_stride, y_fs = src->y_frame_stride, c_rs = mono ? 0 : src->c_row_stride, c_fs = mono ? 0 : src->c_frame_stride;
    int kx0 = x0, ky0 = y0;
    if (src->mem == SWK_MEM_HOST) {
        // only the chroma cells that cover the rectangle, and the luma samples of those cells (the rectangle grown to origins that
        // are multiples of 2^sx and 2^sy: at 4:2:0 at most one more row and column), go to the device, densely; the kernel then
        // sees a frame whose origin is the rectangle's first chroma cell, and the rectangle starts at its origin's remainder
        const int cy0 = y0 >> sy, ch = ((y0 + Hr - 1) >> sy) - cy0 + 1, cx0 = x0 >> sx, cw = ((x0 + Wr - 1) >> sx) - cx0 + 1;
        const int ly0 = cy0 << sy, lx0 = cx0 << sx, lh = y0 + Hr - ly0, lw = x0 + Wr - lx0;
        const size_t yb = ((size_t)count * lh * lw * B + 15) & ~(size_t)15;
        const size_t cb = mono ? 0 : ((size_t)count * ch * cw * cbytes + 15) & ~(size_t)15;
        uint8_t *din;
        NEED(ctx, SL_TMP_IN, yb + cb * (semi ? 1 : 2), din);
        int rc = copy_rects(ctx, din, src->y + (int64_t)ly0 * y_rs + (int64_t)lx0 * B, y_rs, y_fs, (size_t)lw * B, (size_t)lh, count, true);
        if (rc) return rc;
        if (!mono) {
            const int64_t coff = (int64_t)cy0 * c_rs + (int64_t)cx0 * cbytes;
            rc = copy_rects(ctx, din + yb, src->u + coff, c_rs, c_fs, (size_t)cw * cbytes, (size_t)ch, count, true);
            if (rc) return rc;
            if (!semi) {
                rc = copy_rects(ctx, din + yb + cb, src->v + coff, c_rs, c_fs, (size_t)cw * cbytes, (size_t)ch, count, true);
                if (rc) return rc;
            }
            du = din + yb; dv = semi ? nullptr : din + yb + cb;
            c_rs = (int64_t)cw * cbytes; c_fs = (int64_t)ch * c_rs;
        }
        dy = din;
        y_rs = (int64_t)lw * B; y_fs = (int64_t)lh * y_rs;
        kx0 = x0 - lx0; ky0 = y0 - ly0;
    }
    uint8_t *dout = bgr;
    if (bgr_mem == SWK_MEM_HOST) NEED(ctx, SL_TMP_OUT, out_b, dout);
    {
        Timed t(ctx, SWK_K_GRAY);
        // (launch_yuv420_to_bgr hands its NV12 kernel a null v whatever it is given)
        if (yuv420) launch_yuv420_to_bgr(ctx->stream, src->layout, dy, du, dv, y_fs, y_rs, c_fs, c_rs, kx0, ky0, count, Hr, Wr, dout);
        else launch_yuv_to_bgr(ctx->stream, src->layout, sx, sy, src->bits, src->msb_aligned, src->full_range, dy, du, dv, y_fs, y_rs, c_fs, c_rs,
                               kx0, ky0, count, Hr, Wr, dout);
    }
    if (bgr_mem == SWK_MEM_HOST) HIPCHK(ctx, hipMemcpyAsync(bgr, dout, out_b, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_yuv420_to_bgr(swk_ctx *ctx, const swk_yuv420 *src, int32_t count, int32_t x0, int32_t y0, int32_t Hr, int32_t Wr,
                          uint8_t *bgr, int32_t bgr_mem)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!src || !bgr) return fail(ctx, SWK_ERR_ARG, "null argument");
    if (src->layout != SWK_YUV_I420 && src->layout != SWK_YUV_NV12) return fail(ctx, SWK_ERR_ARG, "unknown YUV layout (SWK_YUV_I420 or SWK_YUV_NV12)");
    static_assert(SWK_YUV_I420 == SWK_YUV_PLANAR && SWK_YUV_NV12 == SWK_YUV_SEMIPLANAR, "swk_yuv420's layouts are swk_yuv's at 4:2:0");
    swk_yuv view{};
    view.y = src->y; view.u = src->u; view.v = src->v; view.mem = src->mem; view.layout = src->layout; view.H = src->H; view.W = src->W;
    view.y_row_stride = src->y_row_stride; view.y_frame_stride = src->y_frame_stride;
    view.c_row_stride = src->c_row_stride; view.c_frame_stride = src->c_frame_stride;
    view.sx = view.sy = 1; view.bits = 8;
    return yuv_call(ctx, &view, true, count, x0, y0, Hr, Wr, bgr, bgr_mem);
}

int32_t swk_yuv_to_bgr(swk_ctx *ctx, const swk_yuv *src, int32_t count, int32_t x0, int32_t y0, int32_t Hr, int32_t Wr, uint8_t *bgr,
                       int32_t bgr_mem)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!src || !bgr) return fail(ctx, SWK_ERR_ARG, "null argument");
    if (src->layout != SWK_YUV_PLANAR && src->layout != SWK_YUV_SEMIPLANAR && src->layout != SWK_YUV_MONO)
        return fail(ctx, SWK_ERR_ARG, "unknown YUV layout (SWK_YUV_PLANAR, SWK_YUV_SEMIPLANAR or SWK_YUV_MONO)");
    return yuv_call(ctx, src, false, count, x0, y0, Hr, Wr, bgr, bgr_mem);
}

// ---- deinterlacing (deinterlace.hip): every field of interlaced frames as a whole picture ----------------------------------------
int32_t swk_yuv_deinterlace(swk_ctx *ctx, const swk_yuv *src, const swk_deinterlace *d, int32_t count, int32_t x0, int32_t y0, int32_t Hr,
                            int32_t Wr, uint8_t *bgr, int32_t bgr_mem, void *planes, int32_t planes_mem)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!src || !d) return fail(ctx, SWK_ERR_ARG, "null argument");
    if (!bgr && !planes) return fail(ctx, SWK_ERR_ARG, "no output asked for: bgr and planes are both null");
    if (src->layout != SWK_YUV_PLANAR && src->layout != SWK_YUV_SEMIPLANAR && src->layout != SWK_YUV_MONO)
        return fail(ctx, SWK_ERR_ARG, "unknown YUV layout (SWK_YUV_PLANAR, SWK_YUV_SEMIPLANAR or SWK_YUV_MONO)");
    const int refused = yuv_refusal(ctx, src, count, x0, y0, Hr, Wr, bgr ? bgr_mem : (int32_t)SWK_MEM_HOST);
    if (refused) return refused;
    if (planes && planes_mem != SWK_MEM_HOST && planes_mem != SWK_MEM_DEVICE) return fail(ctx, SWK_ERR_ARG, "mem must be SWK_MEM_HOST or SWK_MEM_DEVICE");
    if (d->rate != 1 && d->rate != 2) return fail(ctx, SWK_ERR_ARG, "rate must be 1 (first fields) or 2 (both fields)");
    const int hp = d->has_prev != 0, hn = d->has_next != 0;
    if (count - hp - hn < 1) return fail(ctx, SWK_ERR_ARG, "no frame is left between the context frames");
    const bool semi = src->layout == SWK_YUV_SEMIPLANAR, mono = src->layout == SWK_YUV_MONO;
    const int sx = mono ? 0 : src->sx, sy = mono ? 0 : src->sy;
    const int B = src->bits > 8 ? 2 : 1;
    if (B == 2 && planes && planes_mem == SWK_MEM_DEVICE && ((uintptr_t)planes & 1))
        return fail(ctx, SWK_ERR_ARG, "odd plane address with 2-byte samples");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DeintJob job{count, hp, d->rate * (count - hp - hn), d->rate, d->tff != 0, d->temporal != 0};
    // the rectangle in each plane, and the plane's own size
    const int H = src->H, W = src->W, CH = ((H - 1) >> sy) + 1, CW = ((W - 1) >> sx) + 1;
    const int cy0 = y0 >> sy, ch = ((y0 + Hr - 1) >> sy) - cy0 + 1, cx0 = x0 >> sx, cw = ((x0 + Wr - 1) >> sx) - cx0 + 1;
    const size_t yb = (size_t)job.nout * Hr * Wr * B, cb = mono ? 0 : (size_t)job.nout * ch * cw * B;
    const int msb = B == 2 && src->msb_aligned ? 16 - src->bits : 0;
    DeintPlane pl[3];
    pl[0] = DeintPlane{src->y, src->y_frame_stride, src->y_row_stride, 1, 0, 0, H, W, y0, x0, Hr, Wr, d->y_parity0 & 1, msb, nullptr};
    if (!mono) {
        pl[1] = DeintPlane{src->u, src->c_frame_stride, src->c_row_stride, semi ? 2 : 1, 0, 0, CH, CW, cy0, cx0, ch, cw, d->c_parity0 & 1, msb, nullptr};
        pl[2] = pl[1];
        pl[2].src = semi ? src->u + B : src->v;
    }
    const int np = mono ? 1 : 3;
    if (src->mem == SWK_MEM_HOST) {
        // of each plane only the rectangle grown by the definition's footprint, one row and three columns on every side, clipped to
        // the plane, goes to the device, densely (interleaved chroma as it lies: one copy serves U and V)
        size_t at[3] = {0, 0, 0}, total = 0;
        int ry0[3], rx0[3], rh[3], rw[3];
        const int ncopy = mono ? 1 : (semi ? 2 : 3);
        for (int k = 0; k < ncopy; ++k) {
            const DeintPlane &p = pl[k];
            ry0[k] = p.py0 > 0 ? p.py0 - 1 : 0; rx0[k] = p.px0 > 3 ? p.px0 - 3 : 0;
            rh[k] = (p.py0 + p.ph + 1 < p.PH ? p.py0 + p.ph + 1 : p.PH) - ry0[k];
            rw[k] = (p.px0 + p.pw + 3 < p.PW ? p.px0 + p.pw + 3 : p.PW) - rx0[k];
            at[k] = total;
            total += ((size_t)count * rh[k] * rw[k] * p.step * B + 15) & ~(size_t)15;
        }
        uint8_t *din;
        NEED(ctx, SL_TMP_IN, total, din);
        for (int k = 0; k < ncopy; ++k) {
            DeintPlane &p = pl[k];
            const size_t width = (size_t)rw[k] * p.step * B;
            const int rc = copy_rects(ctx, din + at[k], p.src + (int64_t)ry0[k] * p.rs + (int64_t)rx0[k] * p.step * B, p.rs, p.fs, width,
                                      (size_t)rh[k], count, true);
            if (rc) return rc;
            p.src = din + at[k]; p.rs = (int64_t)width; p.fs = (int64_t)rh[k] * p.rs; p.oy = ry0[k]; p.ox = rx0[k];
        }
        if (semi) { pl[2] = pl[1]; pl[2].src = pl[1].src + B; }
    }
    // the scratch planar picture stack, laid out as `planes` is: a device `planes` is the stack itself
    uint8_t *dpl = (uint8_t *)planes;
    if (!planes || planes_mem == SWK_MEM_HOST) NEED(ctx, SL_TMP_AUX, yb + 2 * cb, dpl);
    pl[0].dst = dpl;
    if (!mono) { pl[1].dst = dpl + yb; pl[2].dst = dpl + yb + cb; }
    const size_t out_b = (size_t)job.nout * Hr * Wr * 3;
    uint8_t *dout = bgr;
    if (bgr && bgr_mem == SWK_MEM_HOST) NEED(ctx, SL_TMP_OUT, out_b, dout);
    {
        Timed t(ctx, SWK_K_GRAY);
        for (int k = 0; k < np; ++k) launch_deint_plane(ctx->stream, pl[k], job, B == 2);
        if (bgr) {
            // the stack as frames whose origin is the rectangle's first chroma cell: the rectangle starts at its origin's remainder
            // (ky0, kx0), and the luma base is moved back by that much -- the kernel reads no sample in front of the rectangle
            const int ky0 = y0 - (cy0 << sy), kx0 = x0 - (cx0 << sx);
            const int64_t y_rs = (int64_t)Wr * B, c_rs = (int64_t)cw * B;
            const uintptr_t ybase = (uintptr_t)dpl - (uintptr_t)(ky0 * y_rs + (int64_t)kx0 * B);
            launch_yuv_to_bgr(ctx->stream, mono ? SWK_YUV_MONO : SWK_YUV_PLANAR, sx, sy, src->bits, 0, src->full_range, (const uint8_t *)ybase,
                              mono ? nullptr : dpl + yb, mono ? nullptr : dpl + yb + cb, (int64_t)Hr * y_rs, y_rs, (int64_t)ch * c_rs, c_rs, kx0, ky0,
                              job.nout, Hr, Wr, dout);
        }
    }
    if (bgr && bgr_mem == SWK_MEM_HOST) HIPCHK(ctx, hipMemcpyAsync(bgr, dout, out_b, hipMemcpyDeviceToHost, ctx->stream));
    if (planes && planes_mem == SWK_MEM_HOST) HIPCHK(ctx, hipMemcpyAsync(planes, dpl, yb + 2 * cb, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

// ---- review video (review.hip): the ROI of a call's frames, composed with the overlay, as 8-bit 4:2:0 -----------------------------
namespace {

// plan_review (review_plan.h) refuses the call or derives its geometry, staging sizes and the kernels' table on the host; what is
// left here reserves, copies and launches.  cols == 0: the ROI's frames alone (dst holds Hc x Wc frames); cols >= 1:
// swk_render_review_panels' mosaic
int review_call(swk_ctx *ctx, const swk_input *in, const swk_review *rv, const swk_review_label *labels, int nlabels, swk_yuv420_dst *dst,
                const swk_review_panel *panels = nullptr, int npanels = 0, int cols = 0)
{
    // ---- every refusal comes before anything is copied or launched
    ReviewPlan pl;
    const char *why = nullptr;
    if (const int rc = plan_review(in, rv, labels, nlabels, dst, panels, npanels, cols, &pl, &why)) return fail(ctx, rc, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int F = pl.F, Hc = pl.Hc, Wc = pl.Wc;
    ReviewArgs a{};
    ReviewLabels text{};
    a.src = in->frames; a.fs = in->frame_stride; a.rs = in->row_stride; a.x0 = in->x0; a.y0 = in->y0;
    a.Hc = Hc; a.Wc = Wc; a.channels = in->channels; a.layout = dst->layout;
    if (in->mem == SWK_MEM_HOST) {
        // the ROI alone, densely
        uint8_t *din;
        NEED(ctx, SL_TMP_IN, pl.src_bytes, din);
        const int rc = copy_rects(ctx, din, in->frames + (int64_t)in->y0 * in->row_stride + (int64_t)in->x0 * in->channels, in->row_stride,
                                  in->frame_stride, pl.rowb, (size_t)Hc, F, true);
        if (rc) return rc;
        a.src = din; a.fs = (int64_t)Hc * pl.rowb; a.rs = (int64_t)pl.rowb; a.x0 = a.y0 = 0;
    }
    ReviewPanels q{};
    q.npanels = npanels; q.ncells = pl.rows * pl.cols; q.cols = pl.cols;
    // device planes are read where they lie; host planes go up densely, one after the other
    uint8_t *dpl = nullptr;
    if (pl.host_panels) NEED(ctx, SL_TMP_AUX, pl.host_panels * pl.per, dpl);
    for (int k = 0; k < npanels; ++k) {
        const swk_review_panel &p = panels[k];
        q.panel[k] = ReviewPanel{p.plane, p.frame_stride, p.row_stride, p.kind, p.gain, p.layers, 0};
        if (p.mem == SWK_MEM_HOST) {
            const int rc = copy_rects(ctx, dpl, p.plane, p.row_stride, p.frame_stride, (size_t)Wc, (size_t)Hc, F, true);
            if (rc) return rc;
            q.panel[k].plane = dpl; q.panel[k].fs = (int64_t)Hc * Wc; q.panel[k].rs = Wc;
            dpl += pl.per;
        }
    }
    if (dst->mem == SWK_MEM_HOST) {
        uint8_t *dout;
        NEED(ctx, SL_TMP_OUT, pl.yb + pl.cb * (pl.nv12 ? 1 : 2), dout);
        a.y = dout; a.u = dout + pl.yb; a.v = pl.nv12 ? nullptr : dout + pl.yb + pl.cb;
        a.y_rs = pl.Wd; a.y_fs = (int64_t)pl.Hd * pl.Wd; a.c_rs = (int64_t)pl.cw * pl.cbytes; a.c_fs = (int64_t)pl.ch * a.c_rs;
    } else {
        a.y = dst->y; a.u = dst->u; a.v = pl.nv12 ? nullptr : dst->v;
        a.y_rs = dst->y_row_stride; a.y_fs = dst->y_frame_stride; a.c_rs = dst->c_row_stride; a.c_fs = dst->c_frame_stride;
    }
    if (rv) {
        int32_t *dmeta;
        NEED(ctx, SL_REVIEW, pl.meta.size() * 4, dmeta);
        if (!pl.meta.empty()) HIPCHK(ctx, hipMemcpyAsync(dmeta, pl.meta.data(), pl.meta.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        a.boxes = dmeta + pl.o_boxes; a.box_start = dmeta + pl.o_bstart; a.marks = dmeta + pl.o_marks; a.mark_start = dmeta + pl.o_mstart;
        a.frame_border = pl.has_border ? dmeta + pl.o_border : nullptr;
        a.mask = pl.mask_alpha ? (const uint8_t *)(dmeta + pl.o_mask) : nullptr;
        a.mask_colour = pl.mask_colour; a.mask_alpha = pl.mask_alpha;
        a.mark_arm = rv->mark_arm; a.border = rv->border;
        if (nlabels > 0) { text.labels = dmeta + pl.o_labels; text.label_start = dmeta + pl.o_lstart; }
        if (npanels > 0) { q.captions = dmeta + pl.o_captions; q.palette = (const uint32_t *)(dmeta + pl.o_palette); }
    }
    {
        Timed t(ctx, SWK_K_GRAY);
        launch_review(ctx->stream, a, F, rv != nullptr, rv != nullptr && nlabels > 0 ? &text : nullptr);
        if (pl.mosaic) launch_review_panels(ctx->stream, a, F, q);
    }
    if (dst->mem == SWK_MEM_HOST) {
        int rc = copy_rects(ctx, a.y, dst->y, dst->y_row_stride, dst->y_frame_stride, (size_t)pl.Wd, (size_t)pl.Hd, F, false);
        if (rc) return rc;
        rc = copy_rects(ctx, a.u, dst->u, dst->c_row_stride, dst->c_frame_stride, (size_t)pl.cw * pl.cbytes, (size_t)pl.ch, F, false);
        if (rc) return rc;
        if (!pl.nv12) {
            rc = copy_rects(ctx, a.v, dst->v, dst->c_row_stride, dst->c_frame_stride, (size_t)pl.cw, (size_t)pl.ch, F, false);
            if (rc) return rc;
        }
    }
    return sync(ctx);            // (the table lives in pl, on this stack frame)
}

}  // namespace

int32_t swk_bgr_to_yuv420(swk_ctx *ctx, const swk_input *in, swk_yuv420_dst *dst)
{
    if (!ctx) return SWK_ERR_ARG;
    return review_call(ctx, in, nullptr, nullptr, 0, dst);
}

int32_t swk_render_review(swk_ctx *ctx, const swk_input *in, const swk_review *rv, swk_yuv420_dst *dst)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!rv) return fail(ctx, SWK_ERR_ARG, "null argument");
    return review_call(ctx, in, rv, nullptr, 0, dst);
}

int32_t swk_render_review_labels(swk_ctx *ctx, const swk_input *in, const swk_review *rv, const swk_review_label *labels, int32_t nlabels,
                                 swk_yuv420_dst *dst)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!rv) return fail(ctx, SWK_ERR_ARG, "null argument");
    return review_call(ctx, in, rv, labels, nlabels, dst);
}

void swk_review_font(uint8_t out[128][8])
{
    if (out) swk::review_font(out);
}

int32_t swk_render_review_panels(swk_ctx *ctx, const swk_input *in, const swk_review *rv, const swk_review_label *labels, int32_t nlabels,
                                 const swk_review_panel *panels, int32_t npanels, int32_t cols, swk_yuv420_dst *dst)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!rv) return fail(ctx, SWK_ERR_ARG, "null argument");
    if (cols < 1) return fail(ctx, SWK_ERR_ARG, "npanels outside 0..15 or cols outside 1..16");
    return review_call(ctx, in, rv, labels, nlabels, dst, panels, npanels, cols);
}

void swk_review_label_palette(uint8_t out[256][3])
{
    if (out) swk::review_label_palette(out);
}

int32_t swk_ialm(swk_ctx *ctx, const uint8_t *planes, int32_t n, int32_t P, double lmbda, double tol, int32_t maxiter,
                 double *A, double *E, int32_t *iters)
{
    if (!ctx || !planes || n < 1 || P < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t elems = (size_t)n * P;
    uint8_t *dX, *dS;
    NEED(ctx, SL_X, elems + 4, dX);
    NEED(ctx, SL_S, elems, dS);
    HIPCHK(ctx, hipMemcpyAsync(dX, planes, elems, hipMemcpyHostToDevice, ctx->stream));
    IalmRun run{};
    int rc = run_ialm(ctx, IalmJob{dX, dS, 1, n, P, nullptr, lmbda, tol, maxiter}, A != nullptr, E != nullptr, &run);
    if (rc) return rc;
    for (int which = 0; which < 2; ++which) {
        double *dst = which == 0 ? A : E;
        if (!dst) continue;
        double *pn;
        NEED(ctx, SL_PN, elems * 8, pn);
        launch_planes_to_pn(ctx->stream, which == 0 ? run.A : run.E, pn, 1, n, P, run.pstride, run.fpad);
        HIPCHK(ctx, hipMemcpyAsync(dst, pn, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    rc = sync(ctx);
    if (rc) return rc;
    std::vector<IalmWin> hw;
    rc = read_windows(ctx, run, hw);
    if (rc) return rc;
    account_iters(ctx, hw, iters);
    return SWK_OK;
}

// The diagnostics below stage nwin host windows X[nwin][n][P] like swk_ialm's window -- the library's own allocation, padded to whole
// dwords past the last pixel (k_gram_u8) -- and run the chain's start on them under the context's switches.
static int debug_stage_and_start(swk_ctx *ctx, const uint8_t *X, int nwin, int n, int P, double lmbda, IalmJob *job, IalmPlan *plan,
                                 IalmBuffers *b, double **wide_work)
{
    if (!ctx || !X || nwin < 1 || n < 1 || n > kMaxNWide || P < 1 || !(lmbda > 0.0)) return fail(ctx, SWK_ERR_ARG, "bad argument");
    if ((int64_t)nwin * n * P >= (1ll << 31)) return fail(ctx, SWK_ERR_ARG, "too many pixels in one call");
    if (int rcw = check_windows(ctx, nwin)) return rcw;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t elems = (size_t)nwin * n * P;
    uint8_t *dX, *dS;
    NEED(ctx, SL_X, elems + 4, dX);
    NEED(ctx, SL_S, elems, dS);
    HIPCHK(ctx, hipMemcpyAsync(dX, X, elems, hipMemcpyHostToDevice, ctx->stream));
    *plan = plan_ialm(ctx, n, P, nwin, false, 0);
    *job = IalmJob{dX, dS, nwin, n, P, nullptr, lmbda, 1e-3, 100};
    return ialm_start(ctx, *job, *plan, false, false, b, wide_work);
}

// Diagnostic (swk_debug.h): the start of ialm_chain on host windows, and what it left for the first small-matrix step.
int32_t swk_debug_ialm_start(swk_ctx *ctx, const uint8_t *X, int32_t nwin, int32_t n, int32_t P, double lmbda, double *G,
                             uint64_t *sumsq, uint32_t *maxv, int32_t *int_gram, double *scal, int32_t *nblk_out, int32_t *gram8_ran)
{
    if (!G) return fail(ctx, SWK_ERR_ARG, "bad argument");
    IalmJob job;
    IalmPlan plan;
    IalmBuffers b;
    double *wide_work = nullptr;
    int rc = debug_stage_and_start(ctx, X, nwin, n, P, lmbda, &job, &plan, &b, &wide_work);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (b.nblk > 4) launch_gram_reduce(s, b);          // as the first small-matrix step does (ialm_chain)
    // the slabs that step would sum: the first nred of every window
    const size_t nn = (size_t)n * n;
    std::vector<double> slabs((size_t)nwin * b.nred * nn);
    HIPCHK(ctx, hipMemcpy2DAsync(slabs.data(), b.nred * nn * 8, b.gpart, (size_t)b.nblk * nn * 8, b.nred * nn * 8, nwin,
                                 hipMemcpyDeviceToHost, s));
    std::vector<IalmWin> hw(nwin);
    HIPCHK(ctx, hipMemcpyAsync(hw.data(), b.win, (size_t)nwin * sizeof(IalmWin), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    for (int w = 0; w < nwin; ++w) {
        const IalmWin &st = hw[w];
        // gram_reduce's read (ialm_small_dev.h) without its scale: slabs in order, frame-block pairs ib > jb from their mirror
        const double *gp = slabs.data() + (size_t)w * b.nred * nn;
        for (int idx = 0; idx < (int)nn; ++idx) {
            const int i = idx / n, j = idx - i * n;
            const int src = (i >> 4) <= (j >> 4) ? idx : j * n + i;
            double acc = 0.0;
            for (int bk = 0; bk < b.nred && !st.done; ++bk) acc += gp[(size_t)bk * nn + src];
            G[(size_t)w * nn + idx] = acc;
        }
        if (sumsq) sumsq[w] = st.sumsq;
        if (maxv) maxv[w] = st.maxv;
        if (int_gram) int_gram[w] = st.int_gram;
        if (scal) { scal[4 * w] = st.dual_norm; scal[4 * w + 1] = st.cur.mu; scal[4 * w + 2] = st.cur.thr; scal[4 * w + 3] = st.dnorm; }
    }
    if (nblk_out) *nblk_out = b.nblk;
    if (gram8_ran) *gram8_ran = b.use_gram8;
    return SWK_OK;
}

// Diagnostic (swk_debug.h): the start and the first step of ialm_chain on host windows, and the matrix B_1 they leave for iteration 1's pass.
int32_t swk_debug_ialm_first_step(swk_ctx *ctx, const uint8_t *X, int32_t nwin, int32_t n, int32_t P, double lmbda, double *B_fin,
                                  double *B_std, int32_t *refine, double *cond_sum, int32_t *sweeps, int32_t *int_gram, double *scal)
{
    if (!B_fin) return fail(ctx, SWK_ERR_ARG, "bad argument");
    IalmJob job;
    IalmPlan plan;
    IalmBuffers b;
    double *wide_work = nullptr;
    int rc = debug_stage_and_start(ctx, X, nwin, n, P, lmbda, &job, &plan, &b, &wide_work);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if ((rc = ialm_first_step(ctx, job, plan, b, wide_work, B_std))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(B_fin, b.Bm, (size_t)nwin * n * n * 8, hipMemcpyDeviceToHost, s));
    std::vector<IalmWin> hw(nwin);
    HIPCHK(ctx, hipMemcpyAsync(hw.data(), b.win, (size_t)nwin * sizeof(IalmWin), hipMemcpyDeviceToHost, s));
    if ((rc = sync(ctx))) return rc;
    for (int w = 0; w < nwin; ++w) {
        const IalmWin &st = hw[w];
        if (refine) refine[w] = st.refine;
        if (cond_sum) cond_sum[w] = st.cond_sum;
        if (sweeps) sweeps[w] = st.sweeps;
        if (int_gram) int_gram[w] = st.int_gram;
        if (scal) { scal[4 * w] = st.dual_norm; scal[4 * w + 1] = st.cur.mu; scal[4 * w + 2] = st.cur.thr; scal[4 * w + 3] = st.dnorm; }
    }
    return SWK_OK;
}

int32_t swk_rpca_epilogue(swk_ctx *ctx, const double *E, int64_t count, uint8_t *S)
{
    if (!ctx || !E || !S || count < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double *din; uint8_t *dout;
    NEED(ctx, SL_PN, (size_t)count * 8, din);
    NEED(ctx, SL_TMP_OUT, (size_t)count, dout);
    HIPCHK(ctx, hipMemcpyAsync(din, E, (size_t)count * 8, hipMemcpyHostToDevice, ctx->stream));
    launch_rpca_epilogue(ctx->stream, din, count, dout);
    HIPCHK(ctx, hipMemcpyAsync(S, dout, (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_bilateral_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, int32_t d,
                         double sigma_color, double sigma_space, int32_t use_fma, uint8_t *dst)
{
    if (!ctx || !src || !dst || count < 1 || H < 2 || W < 2) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_bilateral(ctx, d, sigma_color, sigma_space);
    if (rc) return rc;
    const size_t px = (size_t)count * H * W;
    uint8_t *din, *dout;
    NEED(ctx, SL_TMP_IN, px, din);
    NEED(ctx, SL_TMP_OUT, px, dout);
    HIPCHK(ctx, hipMemcpyAsync(din, src, px, hipMemcpyHostToDevice, ctx->stream));
    launch_bilateral(ctx->stream, din, count, H, W, ctx->bil, use_fma, dout);
    HIPCHK(ctx, hipMemcpyAsync(dst, dout, px, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_thresh_tozero_u8(swk_ctx *ctx, const uint8_t *src, int64_t count, int32_t thresh, uint8_t *dst)
{
    if (!ctx || !src || !dst || count < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint8_t *din, *dout;
    NEED(ctx, SL_TMP_IN, (size_t)count, din);
    NEED(ctx, SL_TMP_OUT, (size_t)count, dout);
    HIPCHK(ctx, hipMemcpyAsync(din, src, (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    launch_thresh(ctx->stream, din, count, thresh, dout);
    HIPCHK(ctx, hipMemcpyAsync(dst, dout, (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_grey_open3x3_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, uint8_t *dst)
{
    if (!ctx || !src || !dst || count < 1 || H < 1 || W < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)count * H * W;
    uint8_t *din, *dout;
    NEED(ctx, SL_TMP_IN, px, din);
    NEED(ctx, SL_TMP_OUT, px, dout);
    HIPCHK(ctx, hipMemcpyAsync(din, src, px, hipMemcpyHostToDevice, ctx->stream));
    launch_open3x3(ctx->stream, din, count, H, W, dout);
    HIPCHK(ctx, hipMemcpyAsync(dst, dout, px, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_grey_open_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, int32_t kh, int32_t kw, uint8_t *dst)
{
    if (!ctx || !src || !dst || count < 1 || H < 1 || W < 1 || kh < 1 || kw < 1 || kh > 255 || kw > 255) return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)count * H * W;
    uint8_t *din, *dout, *dtmp;
    NEED(ctx, SL_TMP_IN, px, din);
    NEED(ctx, SL_TMP_OUT, px, dout);
    NEED(ctx, SL_TMP_AUX, px, dtmp);
    HIPCHK(ctx, hipMemcpyAsync(din, src, px, hipMemcpyHostToDevice, ctx->stream));
    launch_grey_open(ctx->stream, din, count, H, W, kh, kw, dtmp, dout);
    HIPCHK(ctx, hipMemcpyAsync(dst, dout, px, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_resize_linear_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, int32_t channels, int32_t dH, int32_t dW,
                             uint8_t *dst)
{
    if (!ctx || !src || !dst || count < 1 || H < 1 || W < 1 || dH < 1 || dW < 1 || channels < 1 || channels > 4)
        return fail(ctx, SWK_ERR_ARG, "bad argument");
    // (k_resize_linear_u8 puts the frame in the grid's z extent and does not split it)
    if (count > 65535) return fail(ctx, SWK_ERR_CAPACITY, "too many frames in one call (65535 at most)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // per-axis tables (OpenCV 4.1.0 resizeGeneric_ for INTER_LINEAR, 8u: float32 coordinates, 11-bit weights)
    std::vector<int> idx((size_t)dW + dH);
    std::vector<short> wts(2 * ((size_t)dW + dH));
    auto axis = [](int srcn, int dstn, int *ix, short *w) {
        const double scale = (double)srcn / dstn;
        for (int d = 0; d < dstn; ++d) {
            float f = (float)((d + 0.5) * scale - 0.5);
            int s0 = (int)floorf(f);
            f -= s0;
            if (s0 < 0) { s0 = 0; f = 0.f; }
            if (s0 >= srcn - 1) { s0 = srcn - 1; f = 0.f; }
            ix[d] = s0;
            w[2 * d] = (short)lrintf((1.f - f) * 2048.f);
            w[2 * d + 1] = (short)lrintf(f * 2048.f);
        }
    };
    axis(W, dW, idx.data(), wts.data());
    axis(H, dH, idx.data() + dW, wts.data() + 2 * dW);
    const size_t in_b = (size_t)count * H * W * channels, out_b = (size_t)count * dH * dW * channels;
    uint8_t *din, *dout;
    int *dix; short *dw;
    NEED(ctx, SL_TMP_IN, in_b, din);
    NEED(ctx, SL_TMP_OUT, out_b, dout);
    NEED(ctx, SL_TMP_AUX, idx.size() * 4 + wts.size() * 2, dix);
    dw = (short *)(dix + idx.size());
    HIPCHK(ctx, hipMemcpyAsync(din, src, in_b, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dix, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dw, wts.data(), wts.size() * 2, hipMemcpyHostToDevice, ctx->stream));
    launch_resize_linear(ctx->stream, din, count, H, W, channels, dH, dW, dix, dw, dix + dW, dw + 2 * dW, dout);
    HIPCHK(ctx, hipMemcpyAsync(dst, dout, out_b, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);          // (synchronous: idx / wts live on this stack frame)
}

int32_t swk_ccl_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, int32_t connectivity,
                   int32_t label_order, int32_t *labels, int32_t *ncomp)
{
    if (!ctx || !src || count < 1 || H < 1 || W < 1) return fail(ctx, SWK_ERR_ARG, "bad argument");
    if (connectivity != 4 && connectivity != 8) return fail(ctx, SWK_ERR_ARG, "connectivity must be 4 or 8");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)count * H * W;
    uint8_t *din; int32_t *dlab;
    NEED(ctx, SL_TMP_IN, px, din);
    NEED(ctx, SL_LAB32, px * 4, dlab);
    CclBuffers cb{};
    int rc = ensure_ccl(ctx, count, H, W, &cb);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(din, src, px, hipMemcpyHostToDevice, ctx->stream));
    if (!ctx->force_ccl_multi && ccl_frame_supported(H, W))
        launch_ccl_frame(ctx->stream, din, count, H, W, connectivity, label_order, cb, dlab, nullptr, false, 1, nullptr, nullptr);
    else
        launch_ccl(ctx->stream, din, count, H, W, connectivity, label_order, cb, dlab, nullptr);
    if (labels) HIPCHK(ctx, hipMemcpyAsync(labels, dlab, px * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (ncomp) HIPCHK(ctx, hipMemcpyAsync(ncomp, cb.ncomp, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_regionprops_u8(swk_ctx *ctx, const uint8_t *labels, int32_t count, int32_t H, int32_t W, int32_t seg_cap,
                           swk_segment *segs, int32_t *nseg)
{
    if (!ctx || !labels || !segs || !nseg || count < 1 || H < 1 || W < 1 || seg_cap < 1 || seg_cap > 255)
        return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->last.valid = false;          // SL_SEGS / SL_NSEG are about to be reused
    const size_t px = (size_t)count * H * W;
    uint8_t *din; swk_segment *dsegs; int32_t *dnseg;
    NEED(ctx, SL_TMP_IN, px, din);
    NEED(ctx, SL_SEGS, (size_t)count * seg_cap * sizeof(swk_segment), dsegs);
    NEED(ctx, SL_NSEG, (size_t)count * 4, dnseg);
    CclBuffers cb{};
    int rc = ensure_ccl(ctx, count, H, W, &cb);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(din, labels, px, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dsegs, 0, (size_t)count * seg_cap * sizeof(swk_segment), ctx->stream));
    launch_regionprops(ctx->stream, din, count, H, W, cb, seg_cap, dsegs, dnseg);
    HIPCHK(ctx, hipMemcpyAsync(segs, dsegs, (size_t)count * seg_cap * sizeof(swk_segment), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(nseg, dnseg, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_segment_shapes_u8(swk_ctx *ctx, const uint8_t *labels, int32_t mem, int32_t count, int32_t H, int32_t W, int64_t frame_stride,
                              int64_t row_stride, int32_t seg_cap, swk_segment_shape *shapes, int32_t *nseg)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!labels || !shapes || !nseg) return fail(ctx, SWK_ERR_ARG, "null argument");
    if (count < 1) return fail(ctx, SWK_ERR_ARG, "count must be at least 1");
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return fail(ctx, SWK_ERR_ARG, "plane size must be 1..32768 on each side");
    if (seg_cap < 1 || seg_cap > 255) return fail(ctx, SWK_ERR_ARG, "seg_cap must be in 1..255");
    if (row_stride < W) return fail(ctx, SWK_ERR_ARG, "row stride smaller than a row");
    if (mem != SWK_MEM_HOST && mem != SWK_MEM_DEVICE) return fail(ctx, SWK_ERR_ARG, "mem must be SWK_MEM_HOST or SWK_MEM_DEVICE");
    {
        const unsigned __int128 side = (unsigned)((H > W ? H : W) - 1);
        if ((unsigned __int128)H * (unsigned)W * side * side * side >= ((unsigned __int128)1 << 63))
            return fail(ctx, SWK_ERR_ARG, "plane too large: H * W * max(H - 1, W - 1)^3 must stay below 2^63");
    }
    if (count > (1 << 24)) return fail(ctx, SWK_ERR_CAPACITY, "too many frames in one call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t *planes = labels;
    int64_t fs = frame_stride, rs = row_stride;
    if (mem == SWK_MEM_HOST) {
        uint8_t *din;
        NEED(ctx, SL_TMP_IN, (size_t)count * H * W, din);
        const int rc = copy_rects(ctx, din, labels, row_stride, frame_stride, (size_t)W, (size_t)H, count, true);
        if (rc) return rc;
        planes = din; fs = (int64_t)H * W; rs = W;
    }
    void *table; swk_segment_shape *drec; int32_t *dnseg;
    const size_t rec_b = (size_t)count * seg_cap * sizeof(swk_segment_shape);
    NEED(ctx, SL_SHAPE_TAB, shape_table_bytes(count), table);
    NEED(ctx, SL_SHAPE_REC, rec_b, drec);
    NEED(ctx, SL_SHAPE_NSEG, (size_t)count * 4, dnseg);
    launch_segment_shapes(ctx->stream, planes, count, H, W, fs, rs, table, seg_cap, drec, dnseg);
    HIPCHK(ctx, hipMemcpyAsync(shapes, drec, rec_b, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(nseg, dnseg, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

// the refusals that swk_stabilize_u8 and swk_stabilize_subpel_u8 share (shifts: either call's record array)
static int32_t stabilize_refusal(swk_ctx *ctx, const uint8_t *frames, int32_t mem, int32_t count, int32_t Hs, int32_t Ws, int64_t row_stride,
                                 int32_t y0, int32_t x0, int32_t Ho, int32_t Wo, int32_t search, const uint8_t *anchor, int32_t anchor_mem,
                                 int64_t anchor_bytes, int32_t gray_mode, const void *shifts, const uint8_t *out, int32_t out_mem)
{
    if (!ctx) return SWK_ERR_ARG;
    if (!frames || !anchor || !shifts || !out) return fail(ctx, SWK_ERR_ARG, "null argument");
    if (count < 1) return fail(ctx, SWK_ERR_ARG, "count must be at least 1");
    if (Hs < 1 || Ws < 1 || Hs > 32768 || Ws > 32768) return fail(ctx, SWK_ERR_ARG, "frame size must be 1..32768 on each side");
    if (search < 0 || search > 16) return fail(ctx, SWK_ERR_ARG, "search must be in 0..16");
    if (Ho < 1 || Wo < 1 || y0 < 0 || x0 < 0 || (int64_t)y0 + Ho > Hs || (int64_t)x0 + Wo > Ws)
        return fail(ctx, SWK_ERR_ARG, "the nominal rectangle leaves the source frame");
    if (anchor_bytes != (int64_t)Ho * Wo) return fail(ctx, SWK_ERR_ARG, "the anchor must hold Ho x Wo bytes");
    if (row_stride < (int64_t)Ws * 3) return fail(ctx, SWK_ERR_ARG, "row stride smaller than a row");
    if (gray_mode != SWK_GRAY_Q14 && gray_mode != SWK_GRAY_Q15) return fail(ctx, SWK_ERR_ARG, "gray_mode must be SWK_GRAY_Q14 or SWK_GRAY_Q15");
    for (int32_t m : {mem, anchor_mem, out_mem})
        if (m != SWK_MEM_HOST && m != SWK_MEM_DEVICE) return fail(ctx, SWK_ERR_ARG, "mem must be SWK_MEM_HOST or SWK_MEM_DEVICE");
    if (count > (1 << 24)) return fail(ctx, SWK_ERR_CAPACITY, "too many frames in one call");
    return SWK_OK;
}

int32_t swk_stabilize_u8(swk_ctx *ctx, const uint8_t *frames, int32_t mem, int32_t count, int32_t Hs, int32_t Ws, int64_t frame_stride,
                         int64_t row_stride, int32_t y0, int32_t x0, int32_t Ho, int32_t Wo, int32_t search, const uint8_t *anchor,
                         int32_t anchor_mem, int64_t anchor_bytes, int32_t gray_mode, swk_shift *shifts, uint64_t *sad_table, uint8_t *out,
                         int32_t out_mem)
{
    const int32_t refused = stabilize_refusal(ctx, frames, mem, count, Hs, Ws, row_stride, y0, x0, Ho, Wo, search, anchor, anchor_mem,
                                              anchor_bytes, gray_mode, shifts, out, out_mem);
    if (refused) return refused;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t *src = frames, *danchor = anchor;
    int64_t fs = frame_stride, rs = row_stride;
    const size_t out_b = (size_t)count * Ho * Wo * 3, tab_b = stabilize_table_bytes(count, search);
    if (mem == SWK_MEM_HOST) {
        uint8_t *din;
        NEED(ctx, SL_TMP_IN, (size_t)count * Hs * Ws * 3, din);
        const int rc = copy_rects(ctx, din, frames, row_stride, frame_stride, (size_t)Ws * 3, (size_t)Hs, count, true);
        if (rc) return rc;
        src = din; rs = (int64_t)Ws * 3; fs = (int64_t)Hs * rs;
    }
    if (anchor_mem == SWK_MEM_HOST) {
        uint8_t *da;
        NEED(ctx, SL_TMP_AUX, (size_t)anchor_bytes, da);
        HIPCHK(ctx, hipMemcpyAsync(da, anchor, (size_t)anchor_bytes, hipMemcpyHostToDevice, ctx->stream));
        danchor = da;
    }
    uint8_t *dout = out, *plane, *rec;
    void *table;
    if (out_mem == SWK_MEM_HOST) NEED(ctx, SL_TMP_OUT, out_b, dout);
    NEED(ctx, SL_STAB_PLANE, stabilize_plane_bytes(count, Hs, Ws), plane);
    NEED(ctx, SL_STAB_TAB, tab_b, table);
    NEED(ctx, SL_STAB_REC, (size_t)count * (sizeof(swk_shift) + 4), rec);          // the records, then the frames' non-zero flags
    swk_shift *dshifts = (swk_shift *)rec;
    launch_stabilize(ctx->stream, src, fs, rs, count, Hs, Ws, y0, x0, Ho, Wo, search, danchor, gray_mode, plane,
                     (uint32_t *)(rec + (size_t)count * sizeof(swk_shift)), table, dshifts, dout);
    HIPCHK(ctx, hipMemcpyAsync(shifts, dshifts, (size_t)count * sizeof(swk_shift), hipMemcpyDeviceToHost, ctx->stream));
    if (sad_table) HIPCHK(ctx, hipMemcpyAsync(sad_table, table, tab_b, hipMemcpyDeviceToHost, ctx->stream));
    if (out_mem == SWK_MEM_HOST) HIPCHK(ctx, hipMemcpyAsync(out, dout, out_b, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_stabilize_subpel_u8(swk_ctx *ctx, const uint8_t *frames, int32_t mem, int32_t count, int32_t Hs, int32_t Ws,
                                int64_t frame_stride, int64_t row_stride, int32_t y0, int32_t x0, int32_t Ho, int32_t Wo, int32_t search,
                                const uint8_t *anchor, int32_t anchor_mem, int64_t anchor_bytes, int32_t gray_mode, swk_subshift *shifts,
                                uint64_t *sad_table, uint64_t *sub_table, uint8_t *out, int32_t out_mem)
{
    const int32_t refused = stabilize_refusal(ctx, frames, mem, count, Hs, Ws, row_stride, y0, x0, Ho, Wo, search, anchor, anchor_mem,
                                              anchor_bytes, gray_mode, shifts, out, out_mem);
    if (refused) return refused;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t *src = frames, *danchor = anchor;
    int64_t fs = frame_stride, rs = row_stride;
    const size_t out_b = (size_t)count * Ho * Wo * 3, tab_b = stabilize_table_bytes(count, search), sub_b = stabilize_sub_table_bytes(count);
    if (mem == SWK_MEM_HOST) {
        uint8_t *din;
        NEED(ctx, SL_TMP_IN, (size_t)count * Hs * Ws * 3, din);
        const int rc = copy_rects(ctx, din, frames, row_stride, frame_stride, (size_t)Ws * 3, (size_t)Hs, count, true);
        if (rc) return rc;
        src = din; rs = (int64_t)Ws * 3; fs = (int64_t)Hs * rs;
    }
    if (anchor_mem == SWK_MEM_HOST) {
        uint8_t *da;
        NEED(ctx, SL_TMP_AUX, (size_t)anchor_bytes, da);
        HIPCHK(ctx, hipMemcpyAsync(da, anchor, (size_t)anchor_bytes, hipMemcpyHostToDevice, ctx->stream));
        danchor = da;
    }
    uint8_t *dout = out, *plane, *rec;
    void *table, *sub;
    if (out_mem == SWK_MEM_HOST) NEED(ctx, SL_TMP_OUT, out_b, dout);
    NEED(ctx, SL_SUBPEL_PLANE, stabilize_plane_bytes(count, Hs, Ws), plane);
    NEED(ctx, SL_SUBPEL_TAB, tab_b, table);
    NEED(ctx, SL_SUBPEL_SUBTAB, sub_b, sub);
    // the records, then stage 1's records, then the frames' non-zero flags
    NEED(ctx, SL_SUBPEL_REC, (size_t)count * (sizeof(swk_subshift) + sizeof(swk_shift) + 4), rec);
    swk_subshift *drecs = (swk_subshift *)rec;
    swk_shift *dfirst = (swk_shift *)(rec + (size_t)count * sizeof(swk_subshift));
    launch_stabilize_subpel(ctx->stream, src, fs, rs, count, Hs, Ws, y0, x0, Ho, Wo, search, danchor, gray_mode, plane,
                            (uint32_t *)(rec + (size_t)count * (sizeof(swk_subshift) + sizeof(swk_shift))), table, dfirst, sub, drecs, dout);
    HIPCHK(ctx, hipMemcpyAsync(shifts, drecs, (size_t)count * sizeof(swk_subshift), hipMemcpyDeviceToHost, ctx->stream));
    if (sad_table) HIPCHK(ctx, hipMemcpyAsync(sad_table, table, tab_b, hipMemcpyDeviceToHost, ctx->stream));
    if (sub_table) HIPCHK(ctx, hipMemcpyAsync(sub_table, sub, sub_b, hipMemcpyDeviceToHost, ctx->stream));
    if (out_mem == SWK_MEM_HOST) HIPCHK(ctx, hipMemcpyAsync(out, dout, out_b, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_debug_filter_fused(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, const swk_debug_plane *planes,
                               int64_t total, const swk_params *p, uint8_t *bilateral, uint8_t *thresh, uint8_t *opened, uint8_t *guard)
{
    if (!ctx || !src || !p || !opened || count < 1 || count > (1 << 24)) return fail(ctx, SWK_ERR_ARG, "bad argument");
    // the batch path's rules for its filter, before any buffer or launch
    if (const char *msg = params_refusal(p, false)) return fail(ctx, SWK_ERR_ARG, msg);
    std::vector<FrameGeom> hg;
    int Hmax = 0, Wmax = 0;
    if (planes) {
        if (total < 1 || total >= (1ll << 40)) return fail(ctx, SWK_ERR_ARG, "bad buffer size");
        hg.resize(count);
        std::vector<std::pair<int64_t, int64_t>> span(count);          // [first, end) of every plane
        for (int f = 0; f < count; ++f) {
            if (planes[f].H < 4 || planes[f].W < 4 || planes[f].H > 32768 || planes[f].W > 32768)
                return fail(ctx, SWK_ERR_ARG, "plane sides must be in 4..32768");
            const int64_t px = (int64_t)planes[f].H * planes[f].W;
            if (planes[f].off < 0 || planes[f].off > total - px) return fail(ctx, SWK_ERR_ARG, "a plane leaves the buffer");
            hg[f] = {planes[f].H, planes[f].W, planes[f].off};
            span[f] = {planes[f].off, planes[f].off + px};
            Hmax = std::max(Hmax, planes[f].H);
            Wmax = std::max(Wmax, planes[f].W);
        }
        std::sort(span.begin(), span.end());
        for (int f = 1; f < count; ++f)
            if (span[f].first < span[f - 1].second) return fail(ctx, SWK_ERR_ARG, "planes overlap");
    } else {
        if (H < 4 || W < 4 || H > 32768 || W > 32768) return fail(ctx, SWK_ERR_ARG, "plane sides must be in 4..32768");
        total = (int64_t)count * H * W;
        if (total >= (1ll << 40)) return fail(ctx, SWK_ERR_ARG, "bad buffer size");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nb = (size_t)total, gb = SWK_DEBUG_GUARD_BYTES;
    uint8_t *din, *dout[3] = {nullptr, nullptr, nullptr};          // opened, bilateral, thresholded
    uint8_t *const host[3] = {opened, bilateral, thresh};
    const Slot slot[3] = {SL_OPEN, SL_BIL, SL_THR};
    FrameGeom *dgeom = nullptr;
    NEED(ctx, SL_TMP_IN, nb, din);
    for (int i = 0; i < 3; ++i)
        if (host[i]) NEED(ctx, slot[i], nb + gb, dout[i]);
    if (planes) NEED(ctx, SL_TMP_AUX, hg.size() * sizeof(FrameGeom), dgeom);
    int rc = ensure_bilateral(ctx, p->bil_d, p->bil_sigma_color, p->bil_sigma_space);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(din, src, nb, hipMemcpyHostToDevice, s));
    if (planes) HIPCHK(ctx, hipMemcpyAsync(dgeom, hg.data(), hg.size() * sizeof(FrameGeom), hipMemcpyHostToDevice, s));
    // outputs and the guard behind them start from a non-zero byte: the launcher's clear is part of what is tested
    for (int i = 0; i < 3; ++i)
        if (dout[i]) HIPCHK(ctx, hipMemsetAsync(dout[i], SWK_DEBUG_FILL, nb + gb, s));
    if (planes) launch_filter_fused_geom(s, din, count, Hmax, Wmax, dgeom, nb, ctx->bil, p->bil_fma, p->thresh, dout[1], dout[2], dout[0]);
    else launch_filter_fused(s, din, count, H, W, ctx->bil, p->bil_fma, p->thresh, dout[1], dout[2], dout[0]);
    for (int i = 0; i < 3; ++i) {
        if (dout[i]) {
            HIPCHK(ctx, hipMemcpyAsync(host[i], dout[i], nb, hipMemcpyDeviceToHost, s));
            if (guard) HIPCHK(ctx, hipMemcpyAsync(guard + i * gb, dout[i] + nb, gb, hipMemcpyDeviceToHost, s));
        } else if (guard) {
            memset(guard + i * gb, SWK_DEBUG_FILL, gb);
        }
    }
    return sync(ctx);          // (synchronous: hg lives on this stack frame)
}

int32_t swk_debug_ccl_frame_props(swk_ctx *ctx, const uint8_t *opened, int32_t count, int32_t H, int32_t W, int32_t connectivity,
                                  int32_t label_order, int32_t seg_cap, uint8_t *labels, swk_segment *segs, int32_t *nseg)
{
    if (!ctx || !opened || !labels || !segs || !nseg || count < 1 || count > (1 << 24) || H < 1 || W < 1 || seg_cap < 1 || seg_cap > 255)
        return fail(ctx, SWK_ERR_ARG, "bad argument");
    if (connectivity != 4 && connectivity != 8) return fail(ctx, SWK_ERR_ARG, "connectivity must be 4 or 8");
    if (!ccl_frame_supported(H, W)) return fail(ctx, SWK_ERR_ARG, "the one-workgroup labeller does not take this frame size");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->last.valid = false;          // SL_SEGS / SL_NSEG are about to be reused
    const size_t px = (size_t)count * H * W, rec = (size_t)count * seg_cap * sizeof(swk_segment);
    uint8_t *din, *dlab; swk_segment *dsegs; int32_t *dnseg;
    NEED(ctx, SL_TMP_IN, px, din);
    NEED(ctx, SL_LAB8, px, dlab);
    NEED(ctx, SL_SEGS, rec, dsegs);
    NEED(ctx, SL_NSEG, (size_t)count * 4, dnseg);
    CclBuffers cb{};
    int rc = ensure_ccl(ctx, count, H, W, &cb);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(din, opened, px, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dsegs, 0, rec, ctx->stream));
    launch_ccl_frame(ctx->stream, din, count, H, W, connectivity, label_order, cb, nullptr, dlab, true, seg_cap, dsegs, dnseg);
    HIPCHK(ctx, hipMemcpyAsync(labels, dlab, px, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(segs, dsegs, rec, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(nseg, dnseg, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_classifier_input_window(swk_ctx *ctx, const uint8_t *crops, int64_t crops_bytes, const int64_t *offsets,
                                    const int32_t *hw, int32_t nseg, const float mean[3], const float std_[3],
                                    int32_t pad, int32_t channels_last, uint8_t *patches, float *net, int32_t net_mem)
{
    if (!ctx || !crops || !offsets || !hw || !mean || !std_ || nseg < 1 || crops_bytes < 1 || (!patches && !net) ||
        pad < 0 || pad > 100 || (channels_last != 0 && channels_last != 1))
        return fail(ctx, SWK_ERR_ARG, "bad argument");
    for (int i = 0; i < nseg; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        if (h < 1 || w < 1 || h > 512 || w > 512) return fail(ctx, SWK_ERR_ARG, "segment crops must be 1..512 pixels on each side");
        if (offsets[i] < 0 || offsets[i] + (int64_t)h * w * 3 > crops_bytes) return fail(ctx, SWK_ERR_ARG, "crop outside the packed buffer");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    uint8_t *dcrops, *dpatch = nullptr; int64_t *doffs; int32_t *dhw; float *dnet = nullptr;
    NEED(ctx, SL_CL_CROPS, (size_t)crops_bytes, dcrops);
    NEED(ctx, SL_CL_OFFS, (size_t)nseg * 8, doffs);
    NEED(ctx, SL_CL_HW, (size_t)nseg * 8, dhw);
    HIPCHK(ctx, hipMemcpyAsync(dcrops, crops, (size_t)crops_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(doffs, offsets, (size_t)nseg * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(dhw, hw, (size_t)nseg * 8, hipMemcpyHostToDevice, s));
    if (patches) NEED(ctx, SL_CL_PATCH, (size_t)nseg * 24 * 24 * 3, dpatch);
    const size_t side = 24 + 2 * (size_t)pad;
    const size_t net_bytes = (size_t)nseg * 3 * side * side * sizeof(float);
    if (net) { if (net_mem == SWK_MEM_DEVICE) dnet = net; else NEED(ctx, SL_CL_NET, net_bytes, dnet); }
    launch_classifier_input(s, dcrops, doffs, dhw, nseg, dpatch, dnet, pad, channels_last != 0, mean, std_);
    if (patches) HIPCHK(ctx, hipMemcpyAsync(patches, dpatch, (size_t)nseg * 24 * 24 * 3, hipMemcpyDeviceToHost, s));
    if (net && net_mem != SWK_MEM_DEVICE) HIPCHK(ctx, hipMemcpyAsync(net, dnet, net_bytes, hipMemcpyDeviceToHost, s));
    return sync(ctx);
}

int32_t swk_segment_inputs(swk_ctx *ctx, const swk_input *in, int32_t frame_h, int32_t frame_w,
                           const swk_segment *segs, const int32_t *nseg, int32_t seg_cap, int32_t min_h, int32_t min_w,
                           const float mean[3], const float std_[3], int32_t pad, int32_t channels_last, int32_t first, int32_t net_cap,
                           float *net, int32_t *seg_frame, int32_t *total, int32_t *skipped)
{
    if (!ctx || !in || !in->frames || !segs || !nseg || !mean || !std_ || !net || !total)
        return fail(ctx, SWK_ERR_ARG, "bad argument");
    if (in->mem != SWK_MEM_DEVICE || in->channels != 3) return fail(ctx, SWK_ERR_ARG, "segment inputs are cut from device-resident BGR frames");
    const int64_t F64 = (int64_t)in->nwin * in->n;
    if (in->nwin < 1 || in->n < 1 || F64 > (1 << 24) || seg_cap < 1 || pad < 0 || pad > 100 || first < 0 || net_cap < 1 ||
        (channels_last != 0 && channels_last != 1) ||
        frame_h < 1 || frame_w < 1 || min_h < 1 || min_w < 1 || min_h > 512 || min_w > 512 ||
        in->x0 < 0 || in->y0 < 0 || in->x0 + in->Wc > frame_w || in->y0 + in->Hc > frame_h ||
        in->row_stride < (int64_t)frame_w * 3 || (in->frame_stride < 0 ? -in->frame_stride : in->frame_stride) < in->row_stride * frame_h)
        return fail(ctx, SWK_ERR_ARG, "bad geometry");
    return segment_inputs_impl(ctx, in->frames, in->frame_stride, in->row_stride, (int)F64, in->x0, in->y0, frame_h, frame_w, segs, nseg,
                               seg_cap, min_h, min_w, mean, std_, pad, channels_last != 0, first, net_cap, net, seg_frame, total, skipped);
}

int32_t swk_segment_inputs_last(swk_ctx *ctx, int32_t min_h, int32_t min_w, const float mean[3], const float std_[3], int32_t pad,
                                int32_t channels_last, int32_t first, int32_t net_cap, float *net, int32_t *seg_frame, int32_t *total,
                                int32_t *skipped)
{
    if (!ctx || !mean || !std_ || !net || !total || pad < 0 || pad > 100 || first < 0 || net_cap < 1 ||
        (channels_last != 0 && channels_last != 1) || min_h < 1 || min_w < 1 || min_h > 512 || min_w > 512)
        return fail(ctx, SWK_ERR_ARG, "bad argument");
    const swk_ctx::LastBatch &lb = ctx->last;
    if (!lb.valid) return fail(ctx, SWK_ERR_STALE, "no batch with BGR frames and region records is held by the context any more");
    const int known = *total >= 0 && lb.total >= 0 ? lb.total : -1;          // the batch's own count, when its nseg went to the host
    if (known >= 0 && *total != known) return fail(ctx, SWK_ERR_ARG, "*total does not match the batch");
    return segment_inputs_impl(ctx, lb.frames, lb.fs, lb.rs, lb.nwin * lb.n, lb.x0, lb.y0, lb.frame_h, lb.frame_w, lb.segs, lb.nseg, lb.cap,
                               min_h, min_w, mean, std_, pad, channels_last != 0, first, net_cap, net, seg_frame, total, skipped, known, lb.fr);
}

int32_t swk_debug_resize_table(swk_ctx *ctx, int32_t first, int32_t count, int32_t route, int32_t *bounds, int32_t *coeffs)
{
    if (!ctx || !bounds || !coeffs || first < 1 || count < 1 || (route != 0 && route != 1) ||
        (int64_t)first + count - 1 > (route == 0 ? 512 : 4096))
        return fail(ctx, SWK_ERR_ARG, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)count * 24 * 2, nk = (size_t)count * 24 * 343;
    int32_t *d;
    NEED(ctx, SL_TMP_OUT, (nb + nk) * 4, d);
    launch_resize_table(ctx->stream, first, count, route, d, d + nb);
    HIPCHK(ctx, hipMemcpyAsync(bounds, d, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(coeffs, d + nb, nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int32_t swk_classifier_input(swk_ctx *ctx, const uint8_t *crops, int64_t crops_bytes, const int64_t *offsets,
                             const int32_t *hw, int32_t nseg, const float mean[3], const float std_[3],
                             uint8_t *patches, float *net, int32_t net_mem)
{
    return swk_classifier_input_window(ctx, crops, crops_bytes, offsets, hw, nseg, mean, std_, 100, 0, patches, net, net_mem);
}

}  // extern "C"
#pragma GCC visibility pop
