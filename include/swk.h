/*
 * swk.h -- C ABI of libswk.so, the MI355X (gfx950) implementation of
 * swiftwatcher's per-frame segmentation hot path.
 *
 * The reference (joshuacwnewton/swiftwatcher) is pure Python and has no FFI of its
 * own; the boundary it offers is its Python call surface
 * (swiftwatcher/data_structures.py:116-217 FrameQueue.preprocess_queue/segment_queue,
 * swiftwatcher/image_filtering.py:188-369 free functions).  Each entry point below
 * names the reference function it replaces.  The ctypes binding a maintainer would add
 * is shown in INTEGRATION.md and shipped in swiftwatcher_amd/_lib.py.
 *
 * Conventions
 *   - every function returns int32 status: 0 = SWK_OK, negative = error;
 *     swk_last_error(ctx) gives the text of the last failure on that context.
 *   - plain pointers and sizes only.  Buffers are caller-allocated and C-contiguous;
 *     the library never frees or retains a caller pointer after the call returns.
 *   - "mem" fields say where a caller buffer lives: SWK_MEM_HOST (pageable or pinned
 *     host memory; the library copies) or SWK_MEM_DEVICE (a HIP device pointer on the
 *     context's GPU, e.g. torch.Tensor.data_ptr()).
 *   - one swk_ctx per process per GPU; a context is not thread-safe (serialise the calls on it: the Python layer holds one
 *     lock per context); calls are synchronous (work runs on the context's own non-blocking HIP stream and is waited for;
 *     the library issues nothing on the null stream, so it can run beside a thread that captures a HIP graph in
 *     thread-local capture mode).
 *   - there is NO CPU fallback: without a usable gfx950 device swk_ctx_create fails
 *     with SWK_ERR_NOGPU and nothing else can be called.
 */
#ifndef SWK_H
#define SWK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWK_ABI_VERSION 2

enum {
    SWK_OK = 0,
    SWK_ERR_ARG = -1,       /* bad argument / unsupported parameter value   */
    SWK_ERR_HIP = -2,       /* a HIP runtime call failed                    */
    SWK_ERR_NOGPU = -3,     /* no usable gfx950 device                      */
    SWK_ERR_CAPACITY = -4,  /* request exceeds what the context was sized for */
    SWK_ERR_NOMEM = -5,
    SWK_ERR_STALE = -6,     /* the batch a call refers to is no longer held by the context */
    SWK_ERR_TRACK_STATUS = -7 /* swk_track_window: a segment without a status, the reference's TypeError */
};

enum { SWK_MEM_HOST = 0, SWK_MEM_DEVICE = 1 };

/* component numbering of cc_labeling (see swk_ccl_u8) */
enum { SWK_ORDER_RASTER = 0, SWK_ORDER_BLOCK2X2 = 1 };

/* BGR->gray fixed-point weights (see swk_bgr2gray) */
enum { SWK_GRAY_Q14 = 0, SWK_GRAY_Q15 = 1 };

typedef struct swk_ctx swk_ctx;

/* Algorithm constants.  The reference hard-codes all of them; swk_params_default()
 * fills in exactly those literals (file:line next to each field). */
typedef struct swk_params {
    double  lmbda;            /* IALM lambda = 0.01          image_filtering.py:256 */
    double  tol;              /* IALM tolerance = 0.001      image_filtering.py:256 */
    int32_t maxiter;          /* IALM max iterations = 100   image_filtering.py:257 */
    int32_t bil_d;            /* bilateral diameter = 7      data_structures.py:194.  The batch calls and swk_bilateral_u8 run
                                 radius bil_d / 2 = 1..4 (bil_d 2..9); bil_d <= 0: radius lrint(1.5 * bil_sigma_space), at
                                 least 1, as OpenCV derives it.  A radius above 4 is SWK_ERR_ARG. */
    double  bil_sigma_color;  /* = 15                        data_structures.py:194 */
    double  bil_sigma_space;  /* = 1                         data_structures.py:194 */
    int32_t bil_fma;          /* 0: sum += v*w (mul, add); 1: fused multiply-add.
                                 OpenCV builds differ; unpinned, default 0          */
    int32_t thresh;           /* THRESH_TOZERO level = 15    data_structures.py:198 */
    int32_t open_kh, open_kw; /* grey opening window = 3,3   data_structures.py:202 */
    int32_t connectivity;     /* 8: what cv2.connectedComponents(frame, 4) really runs
                                 (the 4 lands in the `labels` slot, image_filtering.py:327);
                                 4 also supported                                    */
    int32_t label_order;      /* SWK_ORDER_BLOCK2X2 (OpenCV 8-way default, BBDT) or
                                 SWK_ORDER_RASTER (SAUF; always used for 4-way)      */
    int32_t gray_mode;        /* SWK_GRAY_Q14 = OpenCV 4.1.0 (requirements.txt:8)    */
    int32_t reserved_;
} swk_params;

/* One region of one frame: what get_segment_properties()/regionprops yields that
 * the rest of swiftwatcher reads (image_filtering.py:332-335, data_structures.py:16-30).
 * bbox = (r0, c0, r1, c1) half-open; centroid = (sum_r/area, sum_c/area) -- the caller
 * divides in float64, which is bit-identical to skimage's coords.mean(axis=0). */
typedef struct swk_segment {
    int32_t label;
    int32_t r0, c0, r1, c1;
    int32_t reserved_;
    int64_t area;
    int64_t sum_r, sum_c;
} swk_segment;

/* A batch of RPCA windows taken from a stream of frames.
 * Window w, queue position j (0 = newest, data_structures.py:134) is the frame at
 *   frames + (w*n + j)*frame_stride, pixel (r, c) of its ROI at
 *   + (y0 + r)*row_stride + (x0 + c)*channels.
 * Passing whole 1080p frames with (x0, y0, Hc, Wc) = crop_region reproduces
 * crop_frame() (image_filtering.py:199-203); passing pre-cropped ROIs uses x0=y0=0.
 * frame_stride may be negative: `frames` is then the LAST frame in memory (a window that lies in the order it was read,
 * oldest first, is handed over without reversing it: queue position 0 = the newest = the last one read). */
typedef struct swk_input {
    const uint8_t *frames;
    int32_t mem;            /* SWK_MEM_HOST / SWK_MEM_DEVICE */
    int32_t channels;       /* 3 = BGR (convert_grayscale runs), 1 = already gray (passes
                               through, image_filtering.py:193-194) */
    int32_t nwin;           /* windows in this batch */
    int32_t n;              /* frames per window = FrameQueue queue_size (21 default); up to 128 (65 .. 128 run on plain
                               float64 kernels: correct, not fast) */
    int32_t Hc, Wc;         /* ROI rows, cols */
    int32_t x0, y0;         /* ROI origin inside each frame */
    int64_t frame_stride;   /* bytes */
    int64_t row_stride;     /* bytes */
} swk_input;

/* Every pointer is optional (NULL = not wanted).  Planes are u8 [nwin*n][Hc][Wc] in the
 * same frame order as the input; they are the per-stage images FrameQueue stores under
 * "grayscale", "RPCA", "bilateral", "thresh_15", "opened", "cc_labeling"
 * (data_structures.py:183-208). */
typedef struct swk_output {
    int32_t mem;            /* where ALL non-NULL buffers below live */
    int32_t seg_cap;        /* capacity of segs per frame (<= 255; labels are u8) */
    uint8_t *gray, *rpca, *bilateral, *thresh, *opened, *labels;
    double  *A, *E;         /* [nwin][Hc*Wc][n] float64, the reference's (pixels, frames)
                               layout (image_filtering.py:235-237); E costs an extra
                               8 B/element/iteration of HBM traffic when requested */
    int32_t *iters;         /* [nwin] IALM iterations executed */
    int32_t *nseg;          /* [nwin*n] regions found per frame (may exceed seg_cap) */
    swk_segment *segs;      /* [nwin*n][seg_cap], ascending label */
    int32_t planes_on_device; /* nonzero: the six u8 planes above are DEVICE pointers even when mem = SWK_MEM_HOST
                               (FrameQueue keeps the stage images on the GPU and copies one only when somebody reads
                               it, data_structures.py:183-208 stores them but the counting loop never looks) */
    int32_t reserved_;
} swk_output;

/* ---- lifecycle ---------------------------------------------------------------- */
int32_t swk_abi_version(void);
void    swk_params_default(swk_params *p);
/* Sizes device workspaces for batches up to max_windows x max_n frames of max_Hc x max_Wc. */
int32_t swk_ctx_create(int32_t device, int32_t max_windows, int32_t max_n,
                       int32_t max_Hc, int32_t max_Wc, swk_ctx **out);
void    swk_ctx_destroy(swk_ctx *ctx);
const char *swk_last_error(const swk_ctx *ctx);   /* ctx may be NULL: last create error */
/* Bytes of device memory the context holds (for sizing against 288 GB HBM). */
int64_t swk_ctx_device_bytes(const swk_ctx *ctx);

/* Page-locked host memory for staging buffers the caller fills and then passes as swk_input.frames (SWK_MEM_HOST): the
 * copy to the device is then a single DMA.  Allocated on `device` (the GPU the buffer will be copied to; a thread that never
 * chose a device would otherwise create a context on GPU 0), usable from any; no swk_ctx needed; free with swk_pinned_free. */
int32_t swk_pinned_alloc(int32_t device, int64_t bytes, void **out);
int32_t swk_pinned_free(void *p);
/* Host-side staging (no GPU, no context): rows [y0, y0 + rows) x bytes [x_bytes, x_bytes + row_bytes) of each of `count` frames
 * (frames[f] = address of frame f's first byte, row_stride bytes per row) copied densely into dst [count][rows][row_bytes] --
 * the stack FrameQueue.segment_queue hands to swk_batch_run, i.e. crop_frame (image_filtering.py:199-203) for a whole window.
 * threads > 1: the frames are split over a small persistent pool (video frames are cold in the caches; one core copies a
 * 21-frame 1080p window's ROI in about half a millisecond). */
int32_t swk_stage_frames(const uint8_t *const *frames, int32_t count, int64_t row_stride, int32_t y0, int32_t rows, int64_t x_bytes,
                         int64_t row_bytes, uint8_t *dst, int32_t threads);
/* Host side, no context: `count` boxes cut out of a window's frames in one call -- box i = rows [boxes[4i], boxes[4i+1]) x columns
 * [boxes[4i+2], boxes[4i+3]) of frame frame_of[i] (frames[f] = first byte of frame f, row_stride bytes per row, pixel_bytes per
 * pixel), copied densely to out + offsets[i].  The segment images of extract_segment_images (image_filtering.py:338-369) for
 * frames whose memory is reused (the ROI-stream reader's blocks): the segments then hold their crops, not the frames. */
int32_t swk_cut_boxes(const uint8_t *const *frames, int32_t nframes, int64_t row_stride, int32_t pixel_bytes, int32_t count,
                      const int32_t *frame_of, const int32_t *boxes, const int64_t *offsets, uint8_t *out);
/* Device memory on the context's GPU for outputs the caller wants to keep there (swk_output with planes_on_device, or
 * mem = SWK_MEM_DEVICE), and a synchronous copy of a piece of it to host memory.  The library never frees such a buffer
 * by itself; swk_device_free waits for the context's stream first. */
int32_t swk_device_alloc(swk_ctx *ctx, int64_t bytes, void **out);
int32_t swk_device_free(swk_ctx *ctx, void *p);
int32_t swk_device_read(swk_ctx *ctx, const void *src_device, void *dst_host, int64_t bytes);

/* ---- the hot path --------------------------------------------------------------
 * Replaces, for a batch of windows, FrameQueue.preprocess_queue + segment_queue
 * (data_structures.py:171-217): crop -> gray -> RPCA/IALM -> bilateral -> to-zero
 * threshold -> 3x3 grey opening -> connected components -> region properties.
 * Windows are independent (no state is carried between them).
 * Frames per call: nwin * n <= 2^24 over all groups (SWK_ERR_ARG above); the image stages split the frames into launches of 32768.
 * Windows per call: the IALM kernels put the window in the grid's y extent and do not split it, so the windows of one IALM
 * (sub-)batch -- all windows of swk_batch_run; in a groups call the groups whose ROI has at least n pixels together, and each group
 * below that alone -- may number at most hipDeviceAttributeMaxGridDimY of the context's device (65536 on the MI355X; read once when the
 * context is made, swk_debug_max_windows in swk_debug.h reports it).  A call above it returns SWK_ERR_CAPACITY before anything is
 * allocated, copied or launched, names the limit in swk_last_error, and leaves the context usable.  (A device that reported 2^24 or
 * more would make the rule unreachable behind the frame rule.) */
int32_t swk_batch_run(swk_ctx *ctx, const swk_input *in, const swk_params *p, swk_output *out);
/* Several groups of windows in ONE call.  A group is what one swk_batch_run call takes: one video's windows with its own frames
 * pointer, mem, channels, nwin, Hc, Wc, x0, y0, frame_stride and row_stride.  Every group has the same n.  outs[g] receives group
 * g's results with exactly the layout and meaning swk_batch_run gives them.  The IALM runs over all groups at once on planes
 * zero-padded to the largest ROI (exact: the padding leaves X^T X, ||X||_F and max|X| unchanged); a group whose ROI has fewer
 * pixels than n runs as a sub-batch of its own.  Errors as swk_batch_run, checked per group before anything is launched, and
 * SWK_ERR_ARG when the groups' n differ.  swk_segment_inputs_last then serves every group's segments, in group order, then
 * frame order. */
int32_t swk_batch_run_groups(swk_ctx *ctx, const swk_input *groups, int32_t ngroups, const swk_params *p, swk_output *outs);

/* ---- decoder hand-over: 8-bit 4:2:0 YUV -> BGR ------------------------------------------------------------
 * The reference reads BGR frames from cv2.VideoCapture (io_video.py:85-125); every decoder delivers 4:2:0 YUV.  This is
 * the conversion a reference user would have applied to raw YUV, cv2.cvtColor(yuv, COLOR_YUV2BGR_I420 / _NV12) of OpenCV
 * 4.1.0 (requirements.txt:8), restated.  PARITY UNPINNED (ITU-R BT.601, limited range, 20-bit fixed point, all in int32,
 * arithmetic shift, sat8 = clamp to 0..255):
 *   y = max(0, Y - 16) * 1220542;  uu = U - 128;  vv = V - 128;  h = 1 << 19
 *   R = sat8((y + h + 1673527 * vv) >> 20)
 *   G = sat8((y + h - 852492 * vv - 409993 * uu) >> 20)
 *   B = sat8((y + h + 2116026 * uu) >> 20)
 * Chroma is not interpolated: pixel (r, c) uses chroma sample (r >> 1, c >> 1); the chroma planes hold ceil(H / 2) x
 * ceil(W / 2) samples, so an odd last row or column has a sample of its own. */
enum { SWK_YUV_I420 = 0,   /* three planes: Y, then U and V of ceil(H/2) x ceil(W/2) bytes each */
       SWK_YUV_NV12 = 1 }; /* two planes: Y, then ceil(H/2) rows of ceil(W/2) interleaved (U, V) byte pairs */

/* `count` frames of H x W pixels.  Pixel (r, c) of frame f has its luma at y + f * y_frame_stride + r * y_row_stride + c and
 * its chroma at u (and v) + f * c_frame_stride + (r >> 1) * c_row_stride + (c >> 1) for I420, at u + f * c_frame_stride +
 * (r >> 1) * c_row_stride + 2 * (c >> 1) (U) and + 1 (V) for NV12 (v is not read).  Strides are bytes; row strides may exceed
 * the width (decoder surfaces), luma and chroma frame strides are independent (planes of a frame need not be adjacent). */
typedef struct swk_yuv420 {
    const uint8_t *y, *u, *v;
    int32_t mem;            /* SWK_MEM_HOST / SWK_MEM_DEVICE: where all planes live */
    int32_t layout;         /* SWK_YUV_I420 / SWK_YUV_NV12 */
    int32_t H, W;           /* frame size in pixels (each 1..32768, odd sizes allowed) */
    int64_t y_row_stride, y_frame_stride;
    int64_t c_row_stride, c_frame_stride;
} swk_yuv420;

/* The rectangle [y0, y0 + Hr) x [x0, x0 + Wr) of every frame, converted to dense BGR: bgr [count][Hr][Wr][3] in host
 * (bgr_mem = SWK_MEM_HOST) or device memory.  Any origin parity and odd Hr / Wr are fine (a chroma sample is then shared
 * across the rectangle's edge).  Of a host source only the chroma samples that cover the rectangle and their luma pixels are copied to the
 * device.  The device result is what swk_input.frames takes (channels = 3, SWK_MEM_DEVICE): the hook for a hardware decoder
 * whose NV12 surfaces are in device memory already.  SWK_ERR_ARG: a null plane, a rectangle outside the frame, an unknown
 * layout, count < 1, a row stride below the row's bytes. */
int32_t swk_yuv420_to_bgr(swk_ctx *ctx, const swk_yuv420 *src, int32_t count, int32_t x0, int32_t y0, int32_t Hr, int32_t Wr,
                          uint8_t *bgr, int32_t bgr_mem);

/* ---- decoder hand-over, every format: planar / semiplanar / mono YUV, 8..16 bits, limited or full range -> BGR ----
 * What cameras and decoders deliver besides 8-bit 4:2:0: full-range 4:2:0 (yuvj420p), 10-bit (P010 surfaces, C420p10
 * files), 4:2:2 and 4:4:4, 4:1:1, luma-only thermal video.  One definition in exact integers (PARITY UNPINNED, like
 * swk_yuv420_to_bgr: cv2.VideoCapture hands BGR over whatever the file holds, and this restates the BT.601 matrix it
 * applies at every resolution).  bits = d in 8..16, k = d - 8; chroma is subsampled by shifts sx in {0, 1, 2} and sy in
 * {0, 1} (4:4:4 = (0,0), 4:2:2 = (1,0), 4:2:0 = (1,1), 4:1:1 = (2,0)); the chroma planes hold ceil(H / 2^sy) x
 * ceil(W / 2^sx) samples and pixel (r, c) uses chroma sample (r >> sy, c >> sx), not interpolated.  Mono behaves as
 * U = V = 128 << k.
 *   limited range: Yt = max(Y - (16 << k), 0); (CY, CUB, CUG, CVG, CVR) = (1220542, 2116026, -409993, -852492, 1673527)
 *   full range:    Yt = Y;                     (CY, CUB, CUG, CVG, CVR) = (1048576, 1858077, -360853, -748826, 1470104)
 *   uu = U - (128 << k);  vv = V - (128 << k);  h = 1 << (19 + k);  s = 20 + k
 *   B = sat8((CY * Yt + CUB * uu + h) >> s)
 *   G = sat8((CY * Yt + CUG * uu + CVG * vv + h) >> s)
 *   R = sat8((CY * Yt + CVR * vv + h) >> s)
 * with an arithmetic shift and exact integers (64-bit for d > 8).  The full-range constants are floor(x * 2^20 + 1/2) of
 * 2 (1 - Kb), -2 Kb (1 - Kb) / Kg, -2 Kr (1 - Kr) / Kg, 2 (1 - Kr) with Kr = 0.299, Kb = 0.114, Kg = 0.587.  Samples are
 * taken as stored: a value above 2^d - 1 is not masked.  At d = 8, limited range, (sx, sy) = (1, 1) this is
 * swk_yuv420_to_bgr bit for bit; a d-bit picture whose samples are 8-bit samples << k converts to the 8-bit picture's bytes. */
enum { SWK_YUV_PLANAR = 0,       /* three planes: Y, U, V (= SWK_YUV_I420 at (1,1)) */
       SWK_YUV_SEMIPLANAR = 1,   /* two planes: Y, then rows of interleaved (U, V) samples: NV12, NV16, NV24, P010, P016, P210 */
       SWK_YUV_MONO = 2 };       /* Y only; u and v are ignored and may be null */

/* swk_yuv420 with the format spelled out.  Samples are bytes at bits = 8 and little-endian 16-bit words above; all strides
 * stay in bytes.  Pixel (r, c) of frame f has its luma sample at y + f * y_frame_stride + r * y_row_stride + c * B (B bytes
 * per sample) and its chroma at u (and v) + f * c_frame_stride + (r >> sy) * c_row_stride + (c >> sx) * B (planar), at
 * u + ... + (c >> sx) * 2 B (U) and + B (V) for semiplanar (v is not read). */
typedef struct swk_yuv {
    const uint8_t *y, *u, *v;
    int32_t mem;            /* SWK_MEM_HOST / SWK_MEM_DEVICE: where all planes live */
    int32_t layout;         /* SWK_YUV_PLANAR / SWK_YUV_SEMIPLANAR / SWK_YUV_MONO */
    int32_t H, W;           /* frame size in pixels (each 1..32768, odd sizes allowed) */
    int64_t y_row_stride, y_frame_stride;
    int64_t c_row_stride, c_frame_stride;
    int32_t sx, sy;         /* chroma shifts: 0..2 and 0..1 (ignored for mono) */
    int32_t bits;           /* 8..16 */
    int32_t msb_aligned;    /* bits > 8: the sample is word >> (16 - bits), as P010 / P016 surfaces store it; planar
                               high-bit-depth files are LSB-aligned (0) */
    int32_t full_range;     /* 0 = limited (16..235 << k), 1 = full */
    int32_t reserved_;
} swk_yuv;

/* As swk_yuv420_to_bgr: the rectangle [y0, y0 + Hr) x [x0, x0 + Wr) of every frame as dense BGR [count][Hr][Wr][3] in host or
 * device memory; host or device planes; of a host source only the samples that cover the rectangle (grown to multiples of
 * 2^sx and 2^sy) are copied up; the device result is what swk_input.frames takes.  SWK_ERR_ARG: bits outside 8..16, sx > 2 or
 * sy > 1, an unknown layout, a null plane that the layout needs, a rectangle outside the frame, count < 1, a row stride below
 * the row's bytes, an odd stride or plane address with 2-byte samples. */
int32_t swk_yuv_to_bgr(swk_ctx *ctx, const swk_yuv *src, int32_t count, int32_t x0, int32_t y0, int32_t Hr, int32_t Wr,
                       uint8_t *bgr, int32_t bgr_mem);

/* ---- interlaced video: every field as a whole picture (motion-adaptive, edge-directed, exact integers) ----------
 * Camcorder footage (1080i) stores two fields, taken 1/50 or 1/59.94 s apart, in the even and odd rows of one frame.
 * cv2.VideoCapture hands the reference the woven frame, in which a moving bird is two combed half-birds; doubling each
 * field's rows moves every still edge up and down at field rate.  This is this project's own definition (no other
 * deinterlacer is claimed to be equalled): where nothing moves it reproduces the stored picture exactly, and it
 * interpolates only where something moves.
 *
 * A plane is the H x W sample array of one component (Y, U or V) of stored frame t: P_t, with d-bit unsigned sample values
 * (for MSB-aligned sources the value is word >> (16 - d)).  Every plane is processed on its own, by the same rule.
 * Row y of a plane belongs to the top field if (y + parity0) is even, otherwise to the bottom field; parity0 is the parity,
 * in the picture, of the described plane's row 0: 0 for whole pictures, and luma and chroma have their own (y_parity0,
 * c_parity0).  With sy = 1 chroma row j belongs to field j & 1, the convention of interlaced 4:2:0.
 * tff = 1: a frame's top field is earlier in time (It); tff = 0: the bottom field is (Ib).  Stored frame t gives output
 * picture 2t (its first field in time) and output picture 2t + 1 (its second field).
 *
 * The output picture for (frame t, kept parity p) keeps the rows of P_t that have parity p.  Every other row y is computed
 * per column x, all in int32:
 *   up = y - 1 if that row exists, else y + 1;  dn = y + 1 if it exists, else y - 1;  a one-row plane: out = P_t[y][x].
 *   c = P_t[up][x],  e = P_t[dn][x],  xl = max(x - 1, 0),  xr = min(x + 1, W - 1)
 *   score = |P_t[up][xl] - P_t[dn][xl]| + |c - e| + |P_t[up][xr] - P_t[dn][xr]| - 1;   pred = (c + e) >> 1
 *   direction j in {-2, -1, 1, 2} is admissible iff x - 1 - |j| >= 0 and x + 1 + |j| <= W - 1, and then
 *     score_j = sum over k = -1..1 of |P_t[up][x + k + j] - P_t[dn][x + k - j]|,  pred_j = (P_t[up][x + j] + P_t[dn][x - j]) >> 1
 *   search: j = -1 is taken (score, pred = score_j, pred_j) if admissible and score_j < score, strictly; only if it was
 *   taken j = -2 is tried the same way; then j = +1 against the current score; only if it was taken, j = +2.
 *   temporal = 0: out = pred.  temporal = 1: Pv = P_(t-1), Nx = P_(t+1), a frame that does not exist replaced by P_t;
 *     for the frame's first field in time Bf = Pv, Af = P_t, otherwise Bf = P_t, Af = Nx;
 *     b = Bf[y][x],  a = Af[y][x],  dm = (b + a) >> 1,  td0 = |b - a|
 *     td1 = (|Pv[up][x] - c| + |Pv[dn][x] - e|) >> 1,  td2 = (|Nx[up][x] - c| + |Nx[dn][x] - e|) >> 1
 *     diff = max(td0 >> 1, td1, td2);   out = min(max(pred, dm - diff), dm + diff)
 * Consequences: the result lies in 0 .. 2^d - 1 (pred and dm are means of two samples, and the clamp only moves pred towards dm); a sample
 * depends only on frames t - 1, t, t + 1 at rows y - 1 .. y + 1 and columns x - 3 .. x + 3; where those three frames agree
 * on that footprint, out = P_t[y][x] (diff = 0 and dm = P_t[y][x]): a still scene comes out as it was stored; at d = 16 every
 * sum fits int32 (the largest is 3 * 65535).
 * Limits: no inverse telecine, no streams of mixed field order, no per-frame field flags; the chroma of 4:2:0 is
 * deinterlaced per plane and not re-sited. */
typedef struct swk_deinterlace {
    int32_t tff, rate /* 1: first field of each frame only, 2: both */, temporal;
    int32_t has_prev, has_next;    /* the first / last described frame is context only: it gives no output */
    int32_t y_parity0, c_parity0, reserved_;
} swk_deinterlace;

/* src is read exactly as swk_yuv_to_bgr reads it (host or device memory; planar, semiplanar and mono; 8..16 bits; every
 * (sx, sy)).  nout = rate * (count - has_prev - has_next) pictures come out, in temporal order.  bgr, if not null, receives
 * dense [nout][Hr][Wr][3]: swk_yuv_to_bgr's formula applied to the deinterlaced samples, so a source whose three neighbouring
 * frames are equal gives swk_yuv_to_bgr's bytes.  planes, if not null, receives the deinterlaced samples themselves:
 * Y [nout][Hr][Wr], then U and V [nout][ch][cw] over chroma rows (y0 >> sy) .. ((y0 + Hr - 1) >> sy) and the matching
 * columns; bytes at 8 bits, otherwise LSB-aligned little-endian 16-bit words.  The rectangle is a crop of the picture-wide
 * definition: the footprint outside it is read from the described planes, and the planes' borders are the picture's
 * borders.  Of a host source only the samples the footprint needs go to the device.  SWK_ERR_ARG: everything
 * swk_yuv_to_bgr refuses, rate outside {1, 2}, count - has_prev - has_next < 1, both outputs null, an odd device address
 * of planes with 2-byte samples. */
int32_t swk_yuv_deinterlace(swk_ctx *ctx, const swk_yuv *src, const swk_deinterlace *d, int32_t count,
                            int32_t x0, int32_t y0, int32_t Hr, int32_t Wr,
                            uint8_t *bgr, int32_t bgr_mem, void *planes, int32_t planes_mem);

/* ---- review video: BGR -> 8-bit 4:2:0 YUV, with the overlay of a count drawn in ---------------------------------
 * The reference shows what it counted with `--export`: one overlay PNG per segment (data_structures.py:65-113).  Here the
 * ROI frames of a call leave as 4:2:0 video frames (what Y4MWriter stores and ffmpeg / mpv open) with the segments, the
 * rejected segments, the events and the ROI mask drawn in; the overlay is this project's own definition.
 *
 * Source frames: `in` names them exactly as swk_batch_run reads them -- frame f = w * n + j at frames + f * frame_stride (may be
 * negative), ROI pixel (r, c) at + (y0 + r) * row_stride + (x0 + c) * channels, host or device memory, channels 3 (BGR) or 1
 * (gray, taken as B = G = R); of a host source only the ROI's rows and columns are copied to the device.  The `frame` fields
 * of boxes and marks and the index of frame_style are this f.
 *
 * Composition, per pixel of frame f, in exact integers, with blend(p, col, a) = (p * (256 - a) + col * a + 128) >> 8 per channel;
 * the layers apply in this order (the blends do not commute):
 *   1. mask: where mask[r][c] != 0, blend with the colour and fill_alpha of style mask_style.
 *   2. boxes of this frame, in array order: a pixel with r0 <= r < r1 and c0 <= c < c1 is blended once, with line_alpha if
 *      r == r0 || r == r1 - 1 || c == c0 || c == c1 - 1, else with fill_alpha.  Boxes may leave the frame (they are clipped by the
 *      pixel test alone: an edge outside the frame is not drawn); empty boxes draw nothing.
 *   3. marks of this frame, in array order: the pixels (r + d, c) and (r, c + d), |d| <= mark_arm, that lie in the frame are
 *      blended once each (the centre once) with line_alpha.
 *   4. border: if frame_style[f] != 0, pixels with r < border || r >= Hc - border || c < border || c >= Wc - border are blended
 *      with that style's line_alpha.
 * Style k is styles[k - 1]; style 0 draws nothing.
 *
 * Conversion: cv2.cvtColor(bgr, COLOR_BGR2YUV_I420) of OpenCV 4.1.0 (requirements.txt:8) restated.  PARITY UNPINNED, like its
 * inverse swk_yuv420_to_bgr (ITU-R BT.601, limited range, 20-bit fixed point, all in int32, arithmetic shift):
 *   Y = ( 269484 R + 528482 G + 102760 B + (1 << 19) + (16  << 20)) >> 20
 *   U = (-155188 R - 305135 G + 460324 B + (1 << 19) + (128 << 20)) >> 20
 *   V = ( 460324 R - 385875 G -  74448 B + (1 << 19) + (128 << 20)) >> 20
 * Y comes from every composed pixel; U and V of chroma cell (i, j) from the composed pixel (2 i, 2 j) alone, the cell's top-left
 * pixel as 4.1.0 samples it (no averaging).  The chroma planes hold ceil(Hc / 2) x ceil(Wc / 2) samples, so odd sizes work and
 * the sampled pixel always exists.  Over all 2^24 colours Y stays in 16..235 and U, V in 16..240: nothing saturates; converting
 * back with swk_yuv420_to_bgr is off by at most 2 in B and R and 1 in G. */
typedef struct swk_yuv420_dst {           /* 8-bit 4:2:0 destination of Hc x Wc pixel frames (in->Hc, in->Wc) */
    uint8_t *y, *u, *v;                   /* NV12: u is the interleaved plane, v is not used */
    int32_t mem;                          /* SWK_MEM_HOST / SWK_MEM_DEVICE */
    int32_t layout;                       /* SWK_YUV_I420 / SWK_YUV_NV12 */
    int64_t y_row_stride, y_frame_stride, c_row_stride, c_frame_stride;   /* bytes, row strides may exceed the row */
} swk_yuv420_dst;

typedef struct swk_review_style { uint8_t b, g, r, reserved_; int32_t fill_alpha, line_alpha; } swk_review_style;  /* alphas 0..256 */
typedef struct swk_review_box   { int32_t frame, r0, c0, r1, c1, style; } swk_review_box;    /* half-open, like swk_segment */
typedef struct swk_review_mark  { int32_t frame, r, c, style; } swk_review_mark;

typedef struct swk_review {
    const uint8_t *mask; int32_t mask_style;          /* host u8 [Hc][Wc] or NULL; pixels != 0 are tinted */
    const swk_review_box *boxes;   int32_t nboxes;    /* ascending .frame */
    const swk_review_mark *marks;  int32_t nmarks;    /* ascending .frame */
    int32_t mark_arm;                                 /* plus sign: centre +- mark_arm pixels */
    const int32_t *frame_style;    int32_t border;    /* [frames] or NULL; border thickness in pixels */
    const swk_review_style *styles; int32_t nstyles;  /* style k = styles[k - 1]; style 0 draws nothing */
} swk_review;

/* The ROI of every frame of `in` as 4:2:0 frames in dst, converted (swk_bgr_to_yuv420) or composed with the overlay and then
 * converted (swk_render_review; the former is the latter without drawing: one kernel).  rv, boxes, marks, styles, mask and
 * frame_style are host memory.  SWK_ERR_ARG, before anything is launched and with dst untouched: a null plane the layout needs, a
 * row stride below the row's bytes, an unknown layout or mem, an alpha outside 0..256, a style index outside 0..nstyles, a box or
 * mark `frame` outside 0 .. nwin * n - 1, boxes or marks not in ascending `frame`, negative mark_arm or border, channels other
 * than 1 or 3, an empty batch, a negative ROI origin.  SWK_ERR_CAPACITY: more than 2^24 frames, or an ROI side above 32768. */
int32_t swk_bgr_to_yuv420(swk_ctx *ctx, const swk_input *in, swk_yuv420_dst *dst);
int32_t swk_render_review(swk_ctx *ctx, const swk_input *in, const swk_review *rv, swk_yuv420_dst *dst);

/* ---- review video, layer 5: labels (short strings in a built-in bitmap font) -----------------------------------
 * Font: glyphs 5 wide and 7 high, one byte per glyph row, bit 4 the leftmost column; the table is written by hand in
 * csrc/review.hip.  Character set: space, 0-9, A-Z and # : . - + / = %; every other byte is refused.  swk_review_font (host
 * only, no context) copies the table out: out[ch][0..6] the glyph's rows, out[ch][7] = 1 for a byte of the set, else 0 (and
 * rows of zeros).
 *
 * A label: (r, c) is the top-left ink pixel position of the first glyph (may be negative or outside the frame), scale 1..8,
 * len 0..32 bytes of text; `style` gives the ink's colour and line_alpha (style 0 draws no ink: ink pixels stay as they are),
 * `plate` is a style index whose colour and fill_alpha give the background plate (0: no plate).
 *
 * Pixels, with s = scale: the label's rectangle is rows [r - s, r + 8 s) and columns [c - s, c + 6 s len) -- a character cell
 * is 6 x 8 units with the ink in its top-left 5 x 7, and one unit of margin lies on every side.  For a pixel (y, x) inside
 * the rectangle and inside the frame let v = y - r, u = x - c.  The pixel is ink if v >= 0, u >= 0, v / s < 7,
 * (u / s) % 6 < 5 and bit 4 - (u / s) % 6 of font[text[u / (6 s)]][v / s] is set; an ink pixel is blended once with the colour
 * and line_alpha of `style`; every other pixel of the rectangle is blended once with the colour and fill_alpha of `plate`, if
 * plate != 0.  The blend is blend(p, col, a) above.  Labels are layer 5: after the border, in array order within a frame (later
 * labels lie over earlier ones); conversion and chroma sampling as above.  A len of 0 draws nothing. */
typedef struct swk_review_label { int32_t frame, r, c, style, plate, scale, len, reserved_; uint8_t text[32]; } swk_review_label;

void swk_review_font(uint8_t out[128][8]);

/* swk_render_review with labels (host memory, ascending .frame).  rv must not be null; nlabels == 0 equals swk_render_review
 * bit for bit.  SWK_ERR_ARG, before anything is copied or launched and with dst untouched, besides swk_render_review's list: a
 * null array with a non-zero count, or a negative count; a label's frame outside 0 .. nwin * n - 1; labels not in ascending
 * `frame`; scale outside 1..8; len outside 0..32; style or plate outside 0..nstyles; a byte of text[0..len) outside the set. */
int32_t swk_render_review_labels(swk_ctx *ctx, const swk_input *in, const swk_review *rv, const swk_review_label *labels,
                                 int32_t nlabels, swk_yuv420_dst *dst);

/* ---- review video, stage images: a mosaic of panels beside the composed frame -------------------------------------
 * A review frame shows what was counted; a stage image (swk_output's gray, rpca, bilateral, thresh, opened, labels: u8 planes)
 * shows why.  swk_render_review_panels writes both into one 4:2:0 frame, a grid of equal cells.
 *
 * Geometry: Hp = Hc + (Hc & 1), Wp = Wc + (Wc & 1), cells = 1 + npanels, rows = ceil(cells / cols).  dst describes frames of
 * rows * Hp by cols * Wp luma pixels, their chroma planes exactly half of that per side.  Cell k has its origin at luma
 * ((k / cols) * Hp, (k % cols) * Wp): always even, so no chroma sample belongs to two cells.
 *
 * Cell 0 holds what swk_render_review_labels(ctx, in, rv, labels, nlabels, ...) writes for an Hc x Wc destination.  Cell k >= 1
 * holds what swk_render_review_labels would write for a 3-channel source whose pixel (r, c) of frame f is the mapped value v of
 * panels[k - 1]'s plane: SWK_PANEL_GRAY B = G = R = min(255, v * gain); SWK_PANEL_LABELS (B, G, R) = palette[v].  It is composed
 * with those of rv's layers 1..4 (mask, boxes, marks, border) whose bit (0..3) is set in `layers`, frame indices being the same f,
 * and with the panel's caption as its only label (layer 5; .frame is ignored, it is drawn on every frame; len 0: none).  Same
 * blend, same conversion, same top-left chroma sampling.  Every other luma sample is 16 and every other chroma sample 128: the pad
 * row / column of an odd Hc / Wc in every cell (cell 0's too) and the cells of the last row after `cells`.  Bytes of dst outside
 * the mosaic (row strides above the row) are not written.
 *
 * The palette is the library's own (csrc/review.hip): palette[0] = (0, 0, 0); for v >= 1 hue (v - 1) % 12 of
 *   (0,0,255) (0,255,0) (255,0,0) (0,255,255) (255,0,255) (255,255,0) (0,128,255) (128,255,0) (255,0,128) (255,128,0) (128,0,255)
 *   (0,255,128)                                                                                       (B, G, R)
 * with every channel scaled (x * s) >> 8, s = 256, 176, 112 for ((v - 1) / 12) % 3 = 0, 1, 2: no entry above 0 is black and
 * palette[v] != palette[v + 1].  swk_review_label_palette (host only, no context) copies it out. */
#define SWK_PANEL_GRAY   0   /* B = G = R = min(255, v * gain) */
#define SWK_PANEL_LABELS 1   /* B, G, R = palette[v]; palette[0] = black */
typedef struct swk_review_panel {
    const uint8_t *plane;            /* u8; frame f, pixel (r, c) at plane + f * frame_stride + r * row_stride + c */
    int32_t mem, kind;               /* SWK_MEM_HOST / SWK_MEM_DEVICE; SWK_PANEL_* */
    int64_t frame_stride, row_stride;/* bytes; frame_stride may be negative (as swk_input), row_stride >= Wc */
    int32_t gain;                    /* GRAY: 1..255; LABELS: ignored */
    int32_t layers;                  /* bit 0..3: layers 1..4 of swk_render_review (mask, boxes, marks, border) drawn on this panel */
    swk_review_label caption;        /* .frame ignored; len 0: none; drawn on every frame of the panel as its only label */
} swk_review_panel;

void swk_review_label_palette(uint8_t out[256][3]);   /* host only, no context: B, G, R per label value */

/* rv must not be null.  Device planes are read where they lie; of a host plane the Hc x Wc pixels of every frame are copied up.
 * With npanels == 0, cols == 1 and even Hc and Wc the call equals swk_render_review_labels bit for bit.  SWK_ERR_ARG, before
 * anything is copied or launched and with dst untouched, besides swk_render_review_labels' list: npanels outside 0..15, cols
 * outside 1..16, null panels with npanels > 0, a null plane, an unknown kind or mem, gain outside 1..255 on a GRAY panel,
 * row_stride < Wc, layers outside 0..15, a caption that swk_render_review_labels would refuse (scale, len, style, plate, a byte
 * outside the font's set), a dst row stride below the mosaic's row.  SWK_ERR_CAPACITY: a mosaic side above 32768. */
int32_t swk_render_review_panels(swk_ctx *ctx, const swk_input *in, const swk_review *rv, const swk_review_label *labels,
                                 int32_t nlabels, const swk_review_panel *panels, int32_t npanels, int32_t cols,
                                 swk_yuv420_dst *dst);

/* ---- stage-level entry points (host buffers; used by the parity tests and by the
 *      image_filtering.* drop-in functions) ------------------------------------- */
/* convert_grayscale (image_filtering.py:188-196): [count][H][W][3] -> [count][H][W] */
int32_t swk_bgr2gray(swk_ctx *ctx, const uint8_t *bgr, int32_t count, int32_t H, int32_t W,
                     int32_t gray_mode, uint8_t *gray);
/* inexact_augmented_lagrange_multiplier (image_filtering.py:256-301) on one window.
 * planes: u8 [n][P] (frame j = column j of the reference's X); A, E: float64 [P][n]. */
int32_t swk_ialm(swk_ctx *ctx, const uint8_t *planes, int32_t n, int32_t P,
                 double lmbda, double tol, int32_t maxiter,
                 double *A, double *E, int32_t *iters);
/* rpca() tail (image_filtering.py:244-245): S = clip(-E, 0, 255).astype(uint8) */
int32_t swk_rpca_epilogue(swk_ctx *ctx, const double *E, int64_t count, uint8_t *S);
/* bilateral_blur (image_filtering.py:304-307): [count][H][W] u8 */
int32_t swk_bilateral_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W,
                         int32_t d, double sigma_color, double sigma_space, int32_t use_fma,
                         uint8_t *dst);
/* thresh_to_zero (image_filtering.py:310-316) */
int32_t swk_thresh_tozero_u8(swk_ctx *ctx, const uint8_t *src, int64_t count, int32_t thresh,
                             uint8_t *dst);
/* grayscale_opening with SE (3,3) (image_filtering.py:319-322): [count][H][W] u8 */
int32_t swk_grey_open3x3_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W,
                            uint8_t *dst);
/* grayscale_opening with any SE (kh, kw) (image_filtering.py:319-322: scipy.ndimage.grey_opening(size=SE), border mode 'reflect',
 * scipy's placement of even windows).  The reference's loop only asks for (3, 3) (data_structures.py:202: swk_batch_run's fused
 * filter kernel and swk_grey_open3x3_u8); this is the stage function's general case. */
int32_t swk_grey_open_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, int32_t kh, int32_t kw, uint8_t *dst);
/* resize_frame (image_filtering.py:206-212): cv2.resize(frame, (dW, dH)) = INTER_LINEAR on 8-bit pixels, [count][H][W][channels] ->
 * [count][dH][dW][channels].  PARITY UNPINNED (OpenCV 4.1.0's generic 8u arithmetic restated); dead code in the reference (both call
 * sites are commented out, data_structures.py:179-181), kept for the completeness of the module's surface.  SWK_ERR_CAPACITY: more than
 * 65535 frames in one call (the kernel does not split them). */
int32_t swk_resize_linear_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W, int32_t channels, int32_t dH, int32_t dW,
                             uint8_t *dst);
/* cc_labeling (image_filtering.py:325-329) before the uint8 cast: int32 labels, and the
 * component count per plane. */
int32_t swk_ccl_u8(swk_ctx *ctx, const uint8_t *src, int32_t count, int32_t H, int32_t W,
                   int32_t connectivity, int32_t label_order, int32_t *labels, int32_t *ncomp);
/* get_segment_properties (image_filtering.py:332-335) on u8 label planes. */
int32_t swk_regionprops_u8(swk_ctx *ctx, const uint8_t *labels, int32_t count, int32_t H, int32_t W,
                           int32_t seg_cap, swk_segment *segs, int32_t *nseg);

/* ---- shape sums of regions ---------------------------------------------------------------------------------
 * The integer sums every other regionprops attribute (central, normalized and Hu moments, inertia tensor, axis lengths,
 * eccentricity, orientation, perimeter, Euler number) is a function of; the floats are derived on the host
 * (swiftwatcher_amd/image_filtering.py, ShapeMeasures).  All sums are integers, so a record does not depend on scheduling. */
typedef struct swk_segment_shape {
    int32_t label, reserved_;
    int64_t m[10];     /* sum of r^p c^q over the region's pixels, ABSOLUTE plane coordinates, (p,q) in the order
                          (0,0) (1,0) (0,1) (2,0) (1,1) (0,2) (3,0) (2,1) (1,2) (0,3) */
    int64_t border;    /* border pixels: pixels of the region with a 4-neighbour that is not of the region (outside the plane counts) */
    int64_t perim[3];  /* border pixels by skimage's perimeter weight: 1, sqrt(2), (1 + sqrt(2)) / 2 */
    int64_t quads[3];  /* 2x2 windows of the zero-padded plane with exactly one, exactly three, and two diagonal pixels of the region */
} swk_segment_shape;

/* labels: u8 planes, frame f, pixel (r, c) at labels + f * frame_stride + r * row_stride + c (bytes; row_stride >= W, frame_stride
 * of either sign).  mem = SWK_MEM_DEVICE: read where they lie; SWK_MEM_HOST: the H x W pixels of every frame are copied up.
 * A region is the set of pixels with one non-zero value, as in swk_regionprops_u8: record k of frame f describes the same region
 * as its segs[f][k] (ascending value), m[0], m[1], m[2] = that record's area, sum_r, sum_c.  nseg[f] = values present (may exceed
 * seg_cap); slots past it are zero.  shapes: host [count][seg_cap]; nseg: host [count].
 * Perimeter classes (skimage.measure.perimeter(image, 4) of scikit-image 0.15.0 restated): for a border pixel of value v, with
 * a / b = how many of its four edge / four diagonal neighbours are border pixels of v, code = 1 + 2 a + 10 b; codes 5 7 15 17 25 27
 * count in perim[0], 21 33 in perim[1], 13 23 in perim[2], every other code in border alone.
 * 8-connected Euler number = (quads[0] - quads[1] - 2 * quads[2]) / 4; a window holding several values counts once for each.
 * SWK_ERR_ARG, before anything is copied or launched and with the outputs untouched: a null pointer, count < 1, H or W outside
 * 1..32768, seg_cap outside 1..255, row_stride < W, an unknown mem, H * W * max(H - 1, W - 1)^3 >= 2^63 (below it no degree-3
 * sum overflows; 4096 x 4096 passes).  SWK_ERR_CAPACITY: more than 2^24 frames. */
int32_t swk_segment_shapes_u8(swk_ctx *ctx, const uint8_t *labels, int32_t mem, int32_t count, int32_t H, int32_t W,
                              int64_t frame_stride, int64_t row_stride, int32_t seg_cap, swk_segment_shape *shapes, int32_t *nseg);

/* ---- stabilization: per-frame integer shift search against an anchor image ------------------------------------
 * No counterpart in the reference, which assumes a camera that does not move.  For each of `count` BGR frames of Hs x Ws pixels
 * (frame f, pixel (r, c) at frames + f * frame_stride + r * row_stride + 3 c; strides in bytes, row_stride >= 3 Ws, frame_stride of
 * either sign; mem = SWK_MEM_DEVICE: read where they lie, SWK_MEM_HOST: copied up) every integer shift (dy, dx), |dy|, |dx| <=
 * search, whose rectangle [y0 + dy, y0 + dy + Ho) x [x0 + dx, x0 + dx + Wo) lies inside the frame is a candidate; the others are
 * excluded (no reflected pixels).  The score of a candidate is the sum over the rectangle of
 * |anchor[r][c] - gray(frame)[y0 + dy + r][x0 + dx + c]|, gray as swk_bgr2gray's for gray_mode, bit for bit; an exact integer.
 * The smallest score is chosen; ties go to the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx.
 * A frame whose Hs x Ws x 3 bytes are all zero (a reader's null frame) is not matched: dy = dx = 0 and sad = sad_unshifted.
 *   anchor     [Ho][Wo] u8 grey, dense, anchor_bytes = Ho * Wo (anchor_mem: host or device)
 *   shifts     host [count]
 *   sad_table  optional, host [count][(2 search + 1)^2], entry (dy + search) * (2 search + 1) + dx + search; UINT64_MAX where the
 *              candidate is excluded
 *   out        [count][Ho][Wo][3] dense (out_mem: host or device): each frame's chosen rectangle
 * SWK_ERR_ARG, before anything is copied or launched and with the outputs untouched: a null pointer (sad_table may be null),
 * count < 1, a frame side outside 1..32768, search outside 0..16, a nominal rectangle that leaves the frame, anchor_bytes other
 * than Ho * Wo, row_stride < 3 Ws, an unknown gray_mode or mem.  SWK_ERR_CAPACITY: more than 2^24 frames. */
typedef struct swk_shift {
    int32_t dy, dx;
    uint64_t sad;             /* the chosen candidate's score */
    uint64_t sad_unshifted;   /* the score of (0, 0) */
} swk_shift;
int32_t swk_stabilize_u8(swk_ctx *ctx, const uint8_t *frames, int32_t mem, int32_t count, int32_t Hs, int32_t Ws, int64_t frame_stride,
                         int64_t row_stride, int32_t y0, int32_t x0, int32_t Ho, int32_t Wo, int32_t search, const uint8_t *anchor,
                         int32_t anchor_mem, int64_t anchor_bytes, int32_t gray_mode, swk_shift *shifts, uint64_t *sad_table,
                         uint8_t *out, int32_t out_mem);

/* ---- stabilization to a quarter pixel: swk_stabilize_u8's search, then 25 quarter-pixel candidates around its winner -------
 * The arguments of swk_stabilize_u8; `shifts` takes swk_subshift records and there is one more optional table.  All integers.
 * Stage 1 is swk_stabilize_u8's search bit for bit (candidates, scores, tie rule, null frames, sad_table); its winner is (dy, dx).
 * Stage 2: the candidates are the total shifts in quarter pixels (Qy, Qx) = (4 dy + qy, 4 dx + qx), qy, qx in -2..2.  Per axis
 * i = floor(Q / 4) and the phase p = Q mod 4 in 0..3.  The resampled value at anchor pixel (r, c) is separable with one rounding:
 *     h[r'][c] = sum_k T[px][k] * g[r'][x0 + ix + c - 1 + k]                    k = 0..3
 *     v[r][c]  = sum_k T[py][k] * h[y0 + iy + r - 1 + k][c]
 *     R[r][c]  = clamp((v + 8192) >> 14, 0, 255)                                (>> of a negative value rounds down)
 * with T Catmull-Rom in units of 1/128: T[0] = {0, 128, 0, 0}, T[1] = {-9, 111, 29, -3}, T[2] = {-8, 72, 72, -8},
 * T[3] = {-3, 29, 111, -9} (every row sums to 128; g >= 0, so |v| <= (144 * 144 + 16 * 16) * 255 < 2^23: int32 holds it).  Phase (0, 0) reproduces the pixel.  For the
 * score g is the grey of the source frame, swk_bgr2gray's for gray_mode.  A candidate is admissible if on an axis with phase 0 the
 * rectangle [o + i, o + i + size) and on an axis with another phase the footprint [o + i - 1, o + i + size + 2) lies inside the
 * frame (o = y0 or x0); the others are excluded (no reflected pixels); q = (0, 0) is always admissible.
 * Score = sum |anchor[r][c] - R[r][c]|; the smallest is chosen, ties go to the smallest Qy^2 + Qx^2, then Qy, then Qx.  A null
 * frame (all bytes zero) gets Q = (0, 0).
 *   shifts     host [count]
 *   sad_table  optional, as swk_stabilize_u8's
 *   sub_table  optional, host [count][25], entry (qy + 2) * 5 + qx + 2; UINT64_MAX where the candidate is excluded
 *   out        [count][Ho][Wo][3] dense: the frame's B, G and R, each resampled by the formula at the chosen (Qy, Qx); a frame
 *              left at q = (0, 0) is byte for byte what swk_stabilize_u8 writes
 * SWK_ERR_ARG and SWK_ERR_CAPACITY exactly as swk_stabilize_u8 (sub_table may be null). */
typedef struct swk_subshift {
    int32_t dy, dx;             /* stage 1's winner, pixels */
    int32_t qy_total, qx_total; /* the chosen total shift (Qy, Qx), quarter pixels */
    uint64_t sad;               /* the chosen candidate's score */
    uint64_t sad_int;           /* stage 1's score: that of q = (0, 0) */
    uint64_t sad_unshifted;     /* the score of the shift (0, 0) */
} swk_subshift;
int32_t swk_stabilize_subpel_u8(swk_ctx *ctx, const uint8_t *frames, int32_t mem, int32_t count, int32_t Hs, int32_t Ws,
                                int64_t frame_stride, int64_t row_stride, int32_t y0, int32_t x0, int32_t Ho, int32_t Wo, int32_t search,
                                const uint8_t *anchor, int32_t anchor_mem, int64_t anchor_bytes, int32_t gray_mode, swk_subshift *shifts,
                                uint64_t *sad_table, uint64_t *sub_table, uint8_t *out, int32_t out_mem);

/* ---- classifier input(segment_classification.py:18-24) -------------------------------------------------
 * ToPILImage -> Resize((24,24)) (Pillow's antialiased bilinear resampling, 8-bit fixed point, restated
 * exactly) -> Pad(100) -> ToTensor -> Normalize(mean, std) for nseg segment crops.
 *   crops    packed uint8 H x W x 3 images (host), crop i at byte offsets[i] with hw[2i] rows, hw[2i+1] columns
 *            (each side 1..512)
 *   patches  optional uint8 [nseg][24][24][3] (host): the resized crops
 *   net      optional float32 [nseg][3][224][224]; net_mem says whether it is a host or a device pointer
 *            (a torch tensor's data_ptr() feeds the network without another copy) */
int32_t swk_classifier_input(swk_ctx *ctx, const uint8_t *crops, int64_t crops_bytes, const int64_t *offsets,
                             const int32_t *hw, int32_t nseg, const float mean[3], const float std_[3],
                             uint8_t *patches, float *net, int32_t net_mem);
/* Same, writing only the centred (24 + 2 pad)^2 window of each 224x224 input: net is [nseg][3][24+2pad][24+2pad].
 * pad = 100 is swk_classifier_input; pad = 8 (rows/cols 92..131) is all the receptive-field cropped network of
 * swiftwatcher_amd/segment_classification.py reads. */
int32_t swk_classifier_input_window(swk_ctx *ctx, const uint8_t *crops, int64_t crops_bytes, const int64_t *offsets,
                                    const int32_t *hw, int32_t nseg, const float mean[3], const float std_[3],
                                    int32_t pad, int32_t channels_last, uint8_t *patches, float *net, int32_t net_mem);
/* channels_last: memory order of the float32 network input: 0 = planes [3][side][side] per segment (an NCHW tensor),
 * 1 = [side][side][3] (what the library's convolution kernels read; a torch tensor of shape (n, 3, side, side) in
 * torch.channels_last memory format).  swk_classifier_input writes planes. */

/* Classifier inputs cut on the device from the frames and region records of a swk_batch_run with device buffers
 * (in->mem = SWK_MEM_DEVICE, BGR; segs / nseg / net / seg_frame are device pointers): segment k of the batch is
 * region i of frame f in frame order.  Its crop box is extract_segment_images' (image_filtering.py:338-369): bbox
 * grown to at least min_h x min_w (floor / ceil split), translated by (x0, y0), sliced out of the full frame_h x
 * frame_w frame -- intersected with the frame where the reference's unchecked slice would leave it.  Segments
 * [first, first + net_cap) get their (24 + 2 pad)^2 network inputs written to net; seg_frame (optional) receives
 * the frame index of each.  *total = segments in the batch (regions beyond seg_cap per frame do not count);
 * *skipped = boxes that were empty or had a side above 4096 (their input is the blank image).  Boxes with a side of 513..4096
 * are resampled by a second kernel, launched only when the batch holds one; the result is Pillow's horizontal-pass-first resize,
 * like every smaller box's. */
int32_t swk_segment_inputs(swk_ctx *ctx, const swk_input *in, int32_t frame_h, int32_t frame_w,
                           const swk_segment *segs, const int32_t *nseg, int32_t seg_cap, int32_t min_h, int32_t min_w,
                           const float mean[3], const float std_[3], int32_t pad, int32_t channels_last, int32_t first,
                           int32_t net_cap, float *net, int32_t *seg_frame, int32_t *total, int32_t *skipped);
/* The same for the LAST swk_batch_run of the context, from what that call left on the device: its frames (the copy the
 * library made of a SWK_MEM_HOST input, or the caller's device frames, which must still be alive) and its region records.
 * A host input that carries a margin around the ROI (x0, y0 > 0 in a densely packed buffer: the library then uploads the
 * whole buffer) lets boxes grow into that margin like extract_segment_images grows them into the full frame
 * (image_filtering.py:338-369): with a margin of min_seg_size / 2 (or up to the frame's edge) every crop equals the
 * reference's.  This is how SegmentClassifier scores all segments of a FrameQueue window in one batch at the window's
 * first classifier call (__main__.py:84-85).  SWK_ERR_STALE when another call has reused the buffers since.
 * *total is read as well: >= 0 = the caller's own count of the batch's segments (sum of min(nseg, seg_cap) of that batch_run's
 * host output; checked, and it saves the round trip that fetches the count from the device), -1 = not known. */
int32_t swk_segment_inputs_last(swk_ctx *ctx, int32_t min_h, int32_t min_w, const float mean[3], const float std_[3],
                                int32_t pad, int32_t channels_last, int32_t first, int32_t net_cap, float *net,
                                int32_t *seg_frame, int32_t *total, int32_t *skipped);

/* Glue of the receptive-field cropped classifier, launched on the CALLER's HIP stream (PyTorch's current stream;
 * no context): channels-last dense float32 tensors, (n, c, h, w) = memory [n][h][w][c], c multiple of 4.
 * bias_relu_place: dst[n][off_y+y][off_x+x][c_off+ch] = max(src[n][crop_y+y][crop_x+x][ch] + bias[ch], 0), the three
 * passes PyTorch makes between two convolutions (bias add, ReLU, copy into the next layer's tile) as one.
 * maxpool3s2: nn.MaxPool2d(3, 2) without padding, output [n][(h-3)/2+1][(w-3)/2+1][c]. */
int32_t swk_nhwc_bias_relu_place(void *stream, const float *src, int32_t n, int32_t sh, int32_t sw, int32_t c, int32_t crop_y,
                                 int32_t crop_x, int32_t h, int32_t w, const float *bias, float *dst, int32_t dH, int32_t dW,
                                 int32_t dC, int32_t off_y, int32_t off_x, int32_t c_off);
int32_t swk_nhwc_maxpool3s2(void *stream, const float *src, int32_t n, int32_t h, int32_t w, int32_t c, float *dst);
/* head2_relu_mean: the classifier's two-class head (Conv2d(c, 2, 1), ReLU, AdaptiveAvgPool2d(1); the reference re-heads torchvision's
 * SqueezeNet this way, segment_classification.py:47-67) over the px live positions of the last Fire's output, x [n][px][c]:
 *   out[n][k] = (sum_p max(sum_ch x[n][p][ch] w[k][ch] + bias[k], 0) + ring[k]) / n_pos
 * ring[k] = the head's sum over the positions that do not depend on the segment, n_pos = all positions.  c in {256, 512, 768, 1024}.
 * Fixed summation order: a segment's scores do not depend on the batch it is in. */
int32_t swk_nhwc_head2_relu_mean(void *stream, const float *x, int32_t n, int32_t px, int32_t c, const float *w, const float *bias,
                                 const float *ring, float n_pos, float *out);
/* head2_dropout_relu_mean: the same head with the reference's Dropout(0.5) LIVE in front of it (the reference never puts its model into
 * eval mode, segment_classification.py:47-67: every decision it publishes is one draw), `samples` realisations per segment in one launch:
 *   out[n][s][k] = (sum_{p < n_pos} max(sum_ch 2 m(n, s, p, ch) f(n, p, ch) w[k][ch] + bias[k], 0)) / n_pos,     s < samples, k = 0, 1
 * x [n][px][c]: the px live positions of the last Fire's output; pos [px] (device, int32): the position 0 <= pos[j] < n_pos of live
 * pixel j in the full map, raster order, all distinct; bg [n_pos][c]: the last Fire's output for the blank image.  f(n, p, ch) =
 * x[n][j][ch] where pos[j] == p, bg[p][ch] at every other position (only those rows of bg are read; bg may be NULL when px == n_pos).
 * The factor 2 = 1 / (1 - 0.5) is nn.Dropout's scaling.  keys [n] (device, uint64): one key per segment; seed: one per run.
 * The mask m(n, s, p, ch) in {0, 1} is a pure function of (seed, keys[n], s, p, ch) -- not of the row n, the batch size, the launch or
 * the stream:
 *   Philox4x32-10 with the standard constants (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds)
 *   key      = (seed & 0xffffffff, seed >> 32)
 *   counter  = (p * (c / 4) + ch / 4,  s >> 5,  keys[n] & 0xffffffff,  keys[n] >> 32)
 *   m        = bit (s & 31) of output word (ch & 3);  the value is KEPT when the bit is 1.
 * (One generator call serves four channels for 32 samples.)  It is this library's own stream of bits, not torch's: one draw cannot be
 * matched against a run of the reference, the distribution can.
 * c in {256, 512, 768, 1024}, 1 <= samples <= 256, px <= n_pos <= 8192; x, w and bg 16-byte aligned.  Fixed summation order (a function
 * of c, px, n_pos and samples alone): a segment's samples x 2 scores are bit-identical whatever batch it is scored in. */
int32_t swk_nhwc_head2_dropout_relu_mean(void *stream, const float *x, int32_t n, int32_t px, int32_t c, const int32_t *pos, const float *bg,
                                         int32_t n_pos, const float *w, const float *bias, const uint64_t *keys, uint64_t seed,
                                         int32_t samples, float *out);
/* conv7x7s2_bias_relu: the network's first convolution (Conv2d(3, 96, 7, stride 2), no padding) with bias and ReLU on the f32 matrix
 * cores, for the m x m outputs starting at output (lo, lo) of a side x side channels-last input:
 *   dst[n][y][x][co] = max(sum src[n][2 (lo + y) + dy][2 (lo + x) + dx][c] * weight[co][c][dy][dx] + bias[co], 0)
 * src [n][side][side][3] (side even, 2 (lo + m - 1) + 8 <= side: a zero-weighted eighth patch row is read), weight the Conv2d weight
 * [96][3][7][7] in plain (contiguous) layout, dst [n][m][m][96]. */
int32_t swk_nhwc_conv7x7s2_bias_relu(void *stream, const float *src, int32_t n, int32_t side, int32_t lo, int32_t m, const float *weight,
                                     const float *bias, int32_t cout, float *dst);
/* conv1x1_bias_relu_place: a 1 x 1 convolution fused with everything up to the next layer's tile (the squeeze and expand1x1
 * convolutions of a Fire module), on the f32 matrix cores:
 *   dst[n][off_y+y][off_x+x][c_off+co] = max(sum_ci src[n][crop_y+y][crop_x+x][ci] * weight[co][ci] + bias[co], 0)
 * src [n][sh][sw][cin] (cin a multiple of 16), weight [cout][cin] (a Conv2d weight with a 1 x 1 kernel), cout <= 256,
 * dst [n][dH][dW][dC]; cout, dC and c_off multiples of 4 (the kernel stores four channels at a time), src and dst 16-byte
 * aligned. */
int32_t swk_nhwc_conv1x1_bias_relu_place(void *stream, const float *src, int32_t n, int32_t sh, int32_t sw, int32_t cin, int32_t crop_y,
                                         int32_t crop_x, int32_t h, int32_t w, const float *weight, const float *bias, int32_t cout,
                                         float *dst, int32_t dH, int32_t dW, int32_t dC, int32_t off_y, int32_t off_x, int32_t c_off);

/* maxpool3s2 + conv1x1_bias_relu_place as ONE kernel (a MaxPool2d(3, 2) followed by a Fire module's squeeze: the pooled tensor never
 * goes to memory): src [n][t][t][cin] (cin a multiple of 32), pooled size p = (t - 3) / 2 + 1 (p * p <= 96), weight [cout][cin] with
 * cout <= 64 a multiple of 4;  dst[n][off_y + y][off_x + x][co] = max(sum_ci weight[co][ci] max_{3x3, stride 2} src + bias[co], 0).
 * ring (or NULL): ONE tile [t][t][cin] whose pixels outside the square [live_lo, live_lo + live_n)^2 equal those of every tile of src
 * (the receptive-field cropped network's tiles carry a ring of segment-independent values): those pixels are then read from it, so
 * that the ring of n tiles is not fetched n times. */
int32_t swk_nhwc_maxpool3s2_conv1x1_bias_relu_place(void *stream, const float *src, int32_t n, int32_t t, int32_t cin, const float *weight,
                                                    const float *bias, int32_t cout, float *dst, int32_t dH, int32_t dW, int32_t dC,
                                                    int32_t off_y, int32_t off_x, const float *ring, int32_t live_lo, int32_t live_n);


/* conv3x3_bias_relu_place: the 3 x 3 expand convolution of a Fire module as a VALID convolution over the t x t squeeze tile
 * (the tile carries the halo), fused with bias, ReLU and the placement behind the expand1x1 channels:
 *   dst[n][off_y+y][off_x+x][c_off+co] = max(sum src[n][y+dy][x+dx][ci] * W[co][ci][dy][dx] + bias[co], 0),  y, x < t - 2
 * src [n][t][t][cin] (cin a multiple of 16); weight_t = the Conv2d weight re-laid as [dy][dx][ci][co]; cout <= 256. */
int32_t swk_nhwc_conv3x3_bias_relu_place(void *stream, const float *src, int32_t n, int32_t t, int32_t cin, const float *weight_t,
                                         const float *bias, int32_t cout, float *dst, int32_t dH, int32_t dW, int32_t dC, int32_t off_y,
                                         int32_t off_x, int32_t c_off);

/* The same convolution by Winograd's F(2x2, 3x3) on the f32 matrix cores (2.25 x fewer multiplies; csrc/cnn_wino3x3.hip) for
 * the Fire shapes cin = cout / 4 in {32, 48, 64}; other shapes are refused (SWK_ERR_ARG) and take the direct kernel above.
 * weight_w = the filter transform G g G^T in the kernel's operand layout, made once per layer by
 * swk_winograd_f2x2_3x3_weights (host code, float64 then rounded) from the Conv2d weight [cout][cin][3][3] into
 * out[16 * cin * 32 * ceil(cout / 32)].  Results differ from the direct kernel by float32 rounding of the transform
 * (<= 1e-5 of the output scale, tests/test_classifier.py).  cout, dC, c_off multiples of 4; src, dst, weight_w 16-byte aligned. */
int32_t swk_winograd_f2x2_3x3_weights(const float *weight, int32_t cout, int32_t cin, float *out);
int32_t swk_nhwc_conv3x3_winograd_bias_relu_place(void *stream, const float *src, int32_t n, int32_t t, int32_t cin, const float *weight_w,
                                                  const float *bias, int32_t cout, float *dst, int32_t dH, int32_t dW, int32_t dC,
                                                  int32_t off_y, int32_t off_x, int32_t c_off);

/* The same F(2x2, 3x3) convolution with every float32 product formed as six bf16 x bf16 matrix-core products of three-way split
 * operands (float32-accurate; csrc/cnn_wino3x3_bf16s.hip), for the Fire shapes cin = cout / 4 in {16, 32, 48, 64}; other shapes are
 * refused (SWK_ERR_ARG).  Same arguments and contract as swk_nhwc_conv3x3_winograd_bias_relu_place, but weight_s = the split filter
 * transform made by swk_winograd_f2x2_3x3_weights_bf16s (host code): U = G g G^T in float64, rounded to float32 (the values
 * swk_winograd_f2x2_3x3_weights makes), each split exactly into u1 + u2 + u3 of three round-to-nearest-even bf16 parts, into
 * out[3 * 16 * cin * 32 * ceil(cout / 32)] bf16 bit patterns laid out as the matrix cores' A operands.  weight_s 16-byte aligned. */
int32_t swk_winograd_f2x2_3x3_weights_bf16s(const float *weight, int32_t cout, int32_t cin, uint16_t *out);
int32_t swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place(void *stream, const float *src, int32_t n, int32_t t, int32_t cin,
                                                        const uint16_t *weight_s, const float *bias, int32_t cout, float *dst, int32_t dH,
                                                        int32_t dW, int32_t dC, int32_t off_y, int32_t off_x, int32_t c_off);

/* ---- host-side tracker kernels (no GPU, no context): SURVEY section 8f rank 1 -----------------------
 * Cost matrix of SegmentTracker.formulate_cost_matrix (segment_tracking.py:46-102, 179-254): square, size
 * n_prev + n_curr, row-major.  Centroids are (row, col) float64 pairs; prev_hist0 = centroid of the first
 * segment in each previous segment's history (ignored where prev_has_hist is 0). */
int32_t swk_track_costs(const double *prev_c, const double *prev_hist0, const uint8_t *prev_has_hist,
                        const double *curr_c, int32_t n_prev, int32_t n_curr, double *cost);
/* apply_hungarian_algorithm (segment_tracking.py:257-263): scipy.optimize.linear_sum_assignment's algorithm
 * with its tie rule; col4row[i] = column assigned to row i (n_rows <= n_cols). */
int32_t swk_lsap(const double *cost, int32_t n_rows, int32_t n_cols, int32_t *col4row);

/* ---- the tracker, a whole window of frames per call (host, no GPU, no context) -----------------------
 * A swk_tracker carries what SegmentTracker carries between frames (segment_tracking.py:17-44): the ROI mask (copied at creation,
 * [H][W] uint8) and the cached frame's segments.  Segments are named by ORDINALS: a running int64 count since creation, in frame
 * order and then segment order; the caller keeps whatever else belongs to a segment under that number.  Per live segment (a segment
 * of the last frame) the handle keeps its centroid, its chain (the ordinals of its segment_history, oldest first -- the reference
 * shares ONE list along a chain of matches, :149-152, so a chain has one owner here) and the centroid of the chain's first member,
 * the only history value a cost reads (:225-227).
 * A handle is NOT thread-safe: serialise the calls on it.  Different handles are independent. */
typedef struct swk_tracker swk_tracker;
int32_t swk_tracker_create(const uint8_t *roi_mask, int32_t H, int32_t W, swk_tracker **out);
void swk_tracker_destroy(swk_tracker *t);

/* SegmentTracker.step (:46-176: cost matrix, assignment, statuses, history take-over, events, caching) for `nframes` consecutive frames,
 * in order, against the state in `t`.  nseg[nframes] = segments per frame (0 is valid, and so is nframes = 0); centroids = the
 * (row, col) float64 pairs of all of them, frame after frame.  The frames' segments get the ordinals *first_ordinal,
 * *first_ordinal + 1, ...  Per frame exactly what the per-frame path does: swk_track_costs and swk_lsap themselves (the same libm
 * calls in the same order, the same tie-breaking); a previous segment becomes matched or disappeared, a current one appeared only on
 * its own diagonal cell (store_assignments :104-131); a matched segment takes over its predecessor's chain and appends the
 * predecessor (:133-152); then, over the previous frame's segments in their order, a disappeared one with
 * roi_mask[int(row), int(col)] == 255 (numpy's indexing: truncation towards zero, negative indices count from the end) and a chain
 * of at least one member is an EVENT (:154-176), its path the chain plus the segment itself.
 * Events of this window, in detection order, in CSR form: event e is event_ordinals[event_offsets[e] .. event_offsets[e + 1]).
 * event_offsets holds event_capacity + 1 entries, event_ordinals ordinal_capacity.  *n_events / *n_ordinals = what the window
 * needs; when either exceeds its capacity the call returns SWK_ERR_CAPACITY and has changed NOTHING in `t`: call again with larger
 * buffers.  *frames_done = frames applied (nframes unless SWK_ERR_TRACK_STATUS).  *min_live (optional) = the smallest ordinal a live
 * segment or its chain still names: nothing below it can appear in a later event (= the next ordinal when nothing is live).
 * SWK_ERR_TRACK_STATUS: at frame *frames_done a current segment is neither matched nor on its diagonal, where the reference's
 * link_matching_segments raises TypeError (:139; only an assignment no optimal solver returns gets there).  The frames before it are
 * applied and their events returned; that frame and those behind it are not.
 * SWK_ERR_ARG: a null pointer with a non-zero count, a negative count, or a disappeared segment whose centroid lies outside the mask
 * (numpy would raise); `t` is unchanged then. */
int32_t swk_track_window(swk_tracker *t, int32_t nframes, const int32_t *nseg, const double *centroids,
                         int32_t event_capacity, int64_t ordinal_capacity, int64_t *event_offsets, int64_t *event_ordinals,
                         int32_t *n_events, int64_t *n_ordinals, int32_t *frames_done, int64_t *first_ordinal,
                         int64_t *min_live);

/* The live state, out and in: for a caller that moves between this path and SegmentTracker's per-frame methods.
 * swk_tracker_export: per live segment its centroid, its ordinal and its chain (CSR: chain_offsets[n + 1], chain_ordinals);
 * *n_segments / *n_chain_ordinals = what is needed, SWK_ERR_CAPACITY when a buffer is smaller (chain_offsets holds
 * segment_capacity + 1 entries).  `t` is not changed.
 * swk_tracker_import: replaces the live state by n_segments segments with the given centroids; chain_lengths[k] = members of segment
 * k's chain, chain_first[k] = (row, col) of its first member (ignored for an empty chain).  The imported segments are numbered like
 * a frame's: from *first_ordinal (the handle's next ordinal) the chain members of segment 0 oldest first, those of segment 1, ...,
 * then the n_segments segments themselves. */
int32_t swk_tracker_export(swk_tracker *t, int32_t segment_capacity, int64_t ordinal_capacity, double *centroids,
                           int64_t *ordinals, int64_t *chain_offsets, int64_t *chain_ordinals, int32_t *n_segments,
                           int64_t *n_chain_ordinals);
int32_t swk_tracker_import(swk_tracker *t, int32_t n_segments, const double *centroids, const int64_t *chain_lengths,
                           const double *chain_first, int64_t *first_ordinal);

/* ---- ROI mask of a video (host side, no GPU, no context): SURVEY section 8f rank 3 -----------------------
 * image_filtering.py:99-180, run once per video on its first frame.  PARITY UNPINNED (OpenCV 4.1.0 semantics restated:
 * exact integer rules, see csrc/roi_mask.cpp).  Stage-level pieces first: */
/* cv2.medianBlur (image_filtering.py:125-131): ksize x ksize per channel, BORDER_REPLICATE; src/dst [H][W][channels] */
int32_t swk_median_blur_u8(const uint8_t *src, int32_t H, int32_t W, int32_t channels, int32_t ksize, uint8_t *dst);
/* cv2.threshold(image, 0, 255, THRESH_BINARY + THRESH_OTSU) (image_filtering.py:143-151): dst (optional) = src > t ? 255 : 0,
 * *thresh (optional) = Otsu's threshold t */
int32_t swk_otsu_threshold_u8(const uint8_t *src, int64_t count, uint8_t *dst, int32_t *thresh);
/* cv2.Canny(image, low, high) (image_filtering.py:154-159), aperture 3, L1 gradient */
int32_t swk_canny_u8(const uint8_t *src, int32_t H, int32_t W, int32_t low, int32_t high, uint8_t *dst);
/* cv2.dilate(image, ones((N, 1)), anchor=(0, 0)) (image_filtering.py:162-170): edges grow upwards by N - 1 rows */
int32_t swk_dilate_up_u8(const uint8_t *src, int32_t H, int32_t W, int32_t N, uint8_t *dst);
/* generate_regions (image_filtering.py:20-28): frame = first BGR frame [H][W][3] with row_stride bytes per row,
 * corners = {x1, y1, x2, y2} of the chimney's top edge.  Writes crop_region = {x0, y0, x1, y1} (generate_crop_region)
 * and the ROI mask, uint8 0 / 255, [y1 - y0][x1 - x0] (mask_capacity bytes available).  SWK_ERR_ARG when a region
 * leaves the frame. */
int32_t swk_roi_mask(const uint8_t *frame, int32_t H, int32_t W, int64_t row_stride, const int32_t corners[4],
                     int32_t crop_region[4], uint8_t *mask, int64_t mask_capacity);

/* A/B switches, profiling hooks and diagnostics of the library are declared in swk_debug.h: nothing a caller of the boundary above needs. */

#ifdef __cplusplus
}
#endif
#endif /* SWK_H */
