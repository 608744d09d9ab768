// Review video on gfx950: BGR (or gray) ROI frames -> 8-bit 4:2:0 YUV, with the overlay of a count drawn in on the way
// (swk_render_review, swk_bgr_to_yuv420; include/swk.h has the definition).
//
// Composition per pixel, exact integers, blend(p, col, a) = (p * (256 - a) + col * a + 128) >> 8 per channel, in this order:
// ROI mask tint, the frame's boxes in array order (edge pixels with the style's line alpha, inner pixels with its fill alpha),
// the frame's marks in array order (plus signs, line alpha), the frame's border (line alpha).  Then BGR -> YUV, OpenCV 4.1.0's
// COLOR_BGR2YUV_I420 restated (BT.601 limited range, 20-bit fixed point, int32; PARITY UNPINNED like its inverse in yuv.hip):
//   Y = ( 269484 R + 528482 G + 102760 B + (1 << 19) + (16  << 20)) >> 20
//   U = (-155188 R - 305135 G + 460324 B + (1 << 19) + (128 << 20)) >> 20
//   V = ( 460324 R - 385875 G -  74448 B + (1 << 19) + (128 << 20)) >> 20
// Y of every composed pixel; U and V of chroma cell (i, j) from the composed pixel (2 i, 2 j) alone (no averaging); no value
// leaves 16..235 / 16..240, so nothing saturates.
//
// A byte-streaming kernel: 3 B read and 1.5 B written per pixel.  One thread owns a strip of 8 x 2 pixels (four whole 2 x 2
// cells): two 24-byte runs of source pixels in, two 8-byte luma runs and four chroma samples per plane (I420) or four (U, V) pairs
// (NV12) out, each run as the widest accesses its address allows (8, 4, 2 bytes, else bytes), so consecutive lanes stay on
// consecutive addresses whatever the ROI's origin, the strides and the sizes' parity.  blockIdx.y is the frame: a workgroup reads
// its frame's boxes and marks, style already resolved by the host, into LDS in chunks of kChunk, so a frame may carry any number;
// a strip tests a box's rectangle once and walks its 16 pixels only where they meet.
//
// Labels (layer 5, swk_render_review_labels) are a further template flag, so the instantiations without text keep their registers,
// LDS and kernel arguments (the label tables are an argument that only the instantiation with text has): the records (16 words:
// geometry, resolved ink and plate, 32 bytes of text as font indices) are staged through the same LDS words in chunks of kLabelChunk,
// the font's rows sit in 512 bytes of LDS beside them, and a strip tests a label's rectangle in 64 bits before it walks its pixels
// in 32-bit offsets from the label's origin.
#include <string.h>

#include <type_traits>

#include "swk_internal.h"

namespace swk {

namespace {

constexpr int kChunk = 128;
constexpr int kLabelChunk = kChunk * 6 / 16;          // 48 labels of 16 words: the LDS words of a chunk of boxes

// the font's rows for draw_labels (review_font.h; the host's copy is review_font, review_plan.cpp)
#include "review_font.h"
__constant__ uint8_t d_font[kReviewFontCount][8] = SWK_REVIEW_FONT_ROWS;
#undef SWK_REVIEW_FONT_ROWS
#undef NONE
#undef G
constexpr int kYR = 269484, kYG = 528482, kYB = 102760, kUR = -155188, kUG = -305135, kUB = 460324, kVR = 460324, kVG = -385875,
              kVB = -74448;

__device__ __forceinline__ int blend1(int p, int col, int a) { return (p * (256 - a) + col * a + 128) >> 8; }

__device__ __forceinline__ void blend3(int (&px)[3], uint32_t colour, int a)
{
    px[0] = blend1(px[0], (int)(colour & 255u), a);
    px[1] = blend1(px[1], (int)((colour >> 8) & 255u), a);
    px[2] = blend1(px[2], (int)((colour >> 16) & 255u), a);
}

// n <= 8 bytes of w (w[0] = bytes 0..3) to p, with the widest stores the address allows
__device__ __forceinline__ void store_run8(uint8_t *p, uint32_t w0, uint32_t w1, int n)
{
    if (n == 8) {
        const uintptr_t a = (uintptr_t)p;
        if ((a & 7) == 0) { *(uint2 *)p = make_uint2(w0, w1); return; }
        if ((a & 3) == 0) { ((uint32_t *)p)[0] = w0; ((uint32_t *)p)[1] = w1; return; }
        if ((a & 1) == 0) {
            uint16_t *q = (uint16_t *)p;
            q[0] = (uint16_t)w0; q[1] = (uint16_t)(w0 >> 16); q[2] = (uint16_t)w1; q[3] = (uint16_t)(w1 >> 16);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < n) p[k] = (uint8_t)((k < 4 ? w0 >> (8 * k) : w1 >> (8 * (k - 4))) & 255u);
}

__device__ __forceinline__ void store_run4(uint8_t *p, uint32_t w, int n)
{
    if (n == 4) {
        const uintptr_t a = (uintptr_t)p;
        if ((a & 3) == 0) { *(uint32_t *)p = w; return; }
        if ((a & 1) == 0) { ((uint16_t *)p)[0] = (uint16_t)w; ((uint16_t *)p)[1] = (uint16_t)(w >> 16); return; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) p[k] = (uint8_t)((w >> (8 * k)) & 255u);
}

// ---- k_review's layers and stores of one strip as functions, for k_review_panels: r0, c0 the strip's first pixel, nrow x ncol the pixels
// of it that exist, px its 16 pixels (B, G, R).  The text is k_review's; k_review keeps its own, inline: built from these functions
// hipcc unrolls the loops that fill LDS and k_review<true, .> takes 112 and 114 vector registers where it has 94 and 96 (a wave per SIMD
// less); with that unrolling forbidden, as here, still 96 and 100.  Every workgroup thread calls the layers that stage records through
// LDS (they hold barriers); a thread without a strip has live = false.

// 1. the ROI mask
__device__ __forceinline__ void draw_mask(int (&px)[16][3], const ReviewArgs &a, int r0, int c0, int nrow, int ncol)
{
    if (a.mask && a.mask_alpha != 0) {
#pragma unroll
        for (int dr = 0; dr < 2; ++dr) {
            if (dr < nrow) {
                const uint8_t *m = a.mask + (int64_t)(r0 + dr) * a.Wc + c0;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < ncol && m[k] != 0) blend3(px[8 * dr + k], a.mask_colour, a.mask_alpha);
            }
        }
    }
}

// 2. frame f's boxes, in array order: LDS entries (r0, c0, r1, c1, colour, fill alpha | line alpha << 16)
__device__ __forceinline__ void draw_boxes(int (&px)[16][3], int32_t *lds, const ReviewArgs &a, int f, bool live, int r0, int c0, int nrow, int ncol)
{
    const int b_begin = a.box_start[f], b_end = a.box_start[f + 1];
    for (int base = b_begin; base < b_end; base += kChunk) {
        const int cnt = b_end - base < kChunk ? b_end - base : kChunk;
        __syncthreads();
#pragma nounroll
        for (int k = threadIdx.x; k < cnt * 6; k += blockDim.x) lds[k] = a.boxes[(int64_t)base * 6 + k];
        __syncthreads();
        for (int b = 0; b < cnt; ++b) {
            const int br0 = lds[6 * b], bc0 = lds[6 * b + 1], br1 = lds[6 * b + 2], bc1 = lds[6 * b + 3];
            if (!live || br0 >= r0 + nrow || br1 <= r0 || bc0 >= c0 + ncol || bc1 <= c0) continue;
            const uint32_t colour = (uint32_t)lds[6 * b + 4];
            const int fill = lds[6 * b + 5] & 0xffff, line = lds[6 * b + 5] >> 16;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int r = r0 + (k >> 3), c = c0 + (k & 7);
                if (r >= br0 && r < br1 && c >= bc0 && c < bc1) {
                    const bool edge = r == br0 || r == br1 - 1 || c == bc0 || c == bc1 - 1;
                    blend3(px[k], colour, edge ? line : fill);
                }
            }
        }
    }
}

// 3. frame f's marks, in array order: LDS entries (r, c, colour, line alpha)
__device__ __forceinline__ void draw_marks(int (&px)[16][3], int32_t *lds, const ReviewArgs &a, int f, bool live, int r0, int c0, int nrow, int ncol)
{
    const int m_begin = a.mark_start[f], m_end = a.mark_start[f + 1];
    for (int base = m_begin; base < m_end; base += kChunk) {
        const int cnt = m_end - base < kChunk ? m_end - base : kChunk;
        __syncthreads();
#pragma nounroll
        for (int k = threadIdx.x; k < cnt * 4; k += blockDim.x) lds[k] = a.marks[(int64_t)base * 4 + k];
        __syncthreads();
        for (int m = 0; m < cnt; ++m) {
            const int64_t mr = lds[4 * m], mc = lds[4 * m + 1], arm = a.mark_arm;
            // the strip meets the vertical or the horizontal bar?
            const bool vbar = mc >= c0 && mc < c0 + ncol && mr + arm >= r0 && mr - arm < r0 + nrow;
            const bool hbar = mr >= r0 && mr < r0 + nrow && mc + arm >= c0 && mc - arm < c0 + ncol;
            if (!live || (!vbar && !hbar)) continue;
            const uint32_t colour = (uint32_t)lds[4 * m + 2];
            const int line = lds[4 * m + 3];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int64_t r = r0 + (k >> 3), c = c0 + (k & 7);
                const int64_t dr = r > mr ? r - mr : mr - r, dc = c > mc ? c - mc : mc - c;
                if ((c == mc && dr <= arm) || (r == mr && dc <= arm)) blend3(px[k], colour, line);
            }
        }
    }
}

// 4. frame f's border: (colour, line alpha) per frame, alpha < 0 = none
__device__ __forceinline__ void draw_border(int (&px)[16][3], const ReviewArgs &a, int f, int r0, int c0)
{
    if (a.frame_border) {
        const uint32_t colour = (uint32_t)a.frame_border[2 * (int64_t)f];
        const int line = a.frame_border[2 * (int64_t)f + 1];
        if (line >= 0 && a.border > 0) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int r = r0 + (k >> 3), c = c0 + (k & 7);
                if (r < a.border || r >= a.Hc - a.border || c < a.border || c >= a.Wc - a.border) blend3(px[k], colour, line);
            }
        }
    }
}

// 5. the labels [l_begin, l_end) of `labels`, in array order: LDS entries (r, c, scale, len, ink colour, ink alpha, plate colour, plate
// alpha, 8 words of font indices); font: 64 x 8 bytes of LDS that this fills
__device__ __forceinline__ void draw_labels(int (&px)[16][3], int32_t *lds, uint8_t *font, const int32_t *labels, int l_begin, int l_end, bool live,
                                            int r0, int c0, int nrow, int ncol)
{
    for (int k = threadIdx.x; k < 64 * 8; k += blockDim.x) font[k] = k < kReviewFontCount * 8 ? (&d_font[0][0])[k] : (uint8_t)0;
    for (int base = l_begin; base < l_end; base += kLabelChunk) {
        const int cnt = l_end - base < kLabelChunk ? l_end - base : kLabelChunk;
        __syncthreads();
#pragma nounroll
        for (int k = threadIdx.x; k < cnt * 16; k += blockDim.x) lds[k] = labels[(int64_t)base * 16 + k];
        __syncthreads();
        for (int l = 0; l < cnt; ++l) {
            const int32_t *e = &lds[16 * l];
            const int64_t lr = e[0], lc = e[1];
            const int s = e[2], len = e[3];
            const int64_t top = lr - s, bottom = lr + 8 * s, left = lc - s, right = lc + (int64_t)6 * s * len;
            if (!live || len <= 0 || top >= r0 + nrow || bottom <= r0 || left >= c0 + ncol || right <= c0) continue;
            const uint32_t ink_colour = (uint32_t)e[4], plate_colour = (uint32_t)e[6];
            const int ink_alpha = e[5], plate_alpha = e[7];
            // x / s as (x * inv) >> 16, inv = ceil(2^16 / s): exact for x < 2048 and s <= 8 (the error x (inv - 2^16 / s) / 2^16 is
            // below 1 / 32, the fraction of x / s at most 1 - 1 / 8); here x < 8 s <= 64 and x < 6 s len <= 1536
            const uint32_t inv = (65536u + (uint32_t)s - 1u) / (uint32_t)s;
            // the strip meets the rectangle, so its first pixel lies within 16 pixels of it: 32 bits from here on
            const int v0 = (int)(r0 - lr), u0 = (int)(c0 - lc), tall = 8 * s, wide = 6 * s * len;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int v = v0 + (k >> 3), u = u0 + (k & 7);
                if (v < -s || v >= tall || u < -s || u >= wide) continue;          // outside rows [r - s, r + 8 s) or columns [c - s, c + 6 s len)
                bool ink = false;
                if (v >= 0 && u >= 0) {
                    const uint32_t vs = ((uint32_t)v * inv) >> 16, cell = ((uint32_t)u * inv) >> 16, ci = cell / 6u, col = cell - 6u * ci;
                    if (vs < 7u && col < 5u) {
                        const uint32_t ch = ((uint32_t)e[8 + (ci >> 2)] >> (8 * (ci & 3u))) & 63u;          // ci < len <= 32
                        ink = ((font[8 * ch + vs] >> (4u - col)) & 1u) != 0;
                    }
                }
                blend3(px[k], ink ? ink_colour : plate_colour, ink ? ink_alpha : plate_alpha);
            }
        }
    }
}

// conversion and stores: strip (sr, sc) of a picture whose first luma sample is at y and whose first chroma samples are at u (and v) + cbase;
// nrow rows of ncol pixels leave
__device__ __forceinline__ void store_strip(const int (&px)[16][3], uint8_t *y, uint8_t *u, uint8_t *v, int64_t cbase, int64_t y_rs, int64_t c_rs,
                                            int layout, int sr, int sc, int nrow, int ncol)
{
    constexpr int h = 1 << 19;
    const int r0 = 2 * sr, c0 = 8 * sc;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr) {
        if (dr < nrow) {
            uint32_t w[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int *p = px[8 * dr + k];
                const int Y = (kYR * p[2] + kYG * p[1] + kYB * p[0] + h + (16 << 20)) >> 20;
                w[k >> 2] |= (uint32_t)Y << (8 * (k & 3));
            }
            store_run8(y + (int64_t)(r0 + dr) * y_rs + c0, w[0], w[1], ncol);
        }
    }
    const int ncell = (ncol + 1) >> 1;
    uint32_t uw = 0u, vw = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int *p = px[2 * k];                                        // pixel (2 i, 2 j): the cell's top-left
        const int U = (kUR * p[2] + kUG * p[1] + kUB * p[0] + h + (128 << 20)) >> 20;
        const int V = (kVR * p[2] + kVG * p[1] + kVB * p[0] + h + (128 << 20)) >> 20;
        uw |= (uint32_t)U << (8 * k);
        vw |= (uint32_t)V << (8 * k);
    }
    const int64_t crow = cbase + (int64_t)sr * c_rs;
    if (layout == SWK_YUV_I420) {
        store_run4(u + crow + 4 * sc, uw, ncell);
        store_run4(v + crow + 4 * sc, vw, ncell);
    } else {
        const uint32_t lo = (uw & 255u) | ((vw & 255u) << 8) | (((uw >> 8) & 255u) << 16) | (((vw >> 8) & 255u) << 24);
        const uint32_t hi = ((uw >> 16) & 255u) | (((vw >> 16) & 255u) << 8) | ((uw >> 24) << 16) | ((vw >> 24) << 24);
        store_run8(u + crow + 8 * sc, lo, hi, 2 * ncell);
    }
}

}  // namespace

struct NoLabels {};

template <bool DRAW, bool TEXT>
__global__ __launch_bounds__(256) void k_review(ReviewArgs a, int f0, typename std::conditional<TEXT, ReviewLabels, NoLabels>::type t)
{
    __shared__ int32_t lds[kChunk * 6];
    const int f = f0 + (int)blockIdx.y;
    const int sw = (a.Wc + 7) >> 3, sh = (a.Hc + 1) >> 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < sw * sh;
    const int sr = live ? idx / sw : 0, sc = live ? idx - sr * sw : 0;
    const int r0 = 2 * sr, c0 = 8 * sc;                                  // the strip's first pixel: even row, column a multiple of 8
    const int ncol = !live ? 0 : (a.Wc - c0 < 8 ? a.Wc - c0 : 8);
    const int nrow = !live ? 0 : (a.Hc - r0 < 2 ? a.Hc - r0 : 2);

    // ---- source pixels: two runs of ncol pixels
    int px[16][3];
#pragma unroll
    for (int dr = 0; dr < 2; ++dr) {
        const uint8_t *s = a.src + (int64_t)f * a.fs + (int64_t)(a.y0 + r0 + dr) * a.rs + (int64_t)(a.x0 + c0) * a.channels;
        if (dr >= nrow) {
#pragma unroll
            for (int k = 0; k < 8; ++k) px[8 * dr + k][0] = px[8 * dr + k][1] = px[8 * dr + k][2] = 0;
        } else if (a.channels == 3) {
            if (ncol == 8 && ((uintptr_t)s & 3) == 0) {
                uint32_t w[6];
                if (((uintptr_t)s & 7) == 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) { const uint2 q = ((const uint2 *)s)[k]; w[2 * k] = q.x; w[2 * k + 1] = q.y; }
                } else {
#pragma unroll
                    for (int k = 0; k < 6; ++k) w[k] = ((const uint32_t *)s)[k];
                }
#pragma unroll
                for (int k = 0; k < 24; ++k) px[8 * dr + k / 3][k % 3] = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
            } else {
#pragma unroll
                for (int k = 0; k < 24; ++k) px[8 * dr + k / 3][k % 3] = k / 3 < ncol ? (int)s[k] : 0;
            }
        } else {
            if (ncol == 8 && ((uintptr_t)s & 3) == 0) {
                const uint32_t w0 = ((const uint32_t *)s)[0], w1 = ((const uint32_t *)s)[1];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    px[8 * dr + k][0] = px[8 * dr + k][1] = px[8 * dr + k][2] = (int)(((k < 4 ? w0 : w1) >> (8 * (k & 3))) & 255u);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) px[8 * dr + k][0] = px[8 * dr + k][1] = px[8 * dr + k][2] = k < ncol ? (int)s[k] : 0;
            }
        }
    }

    if (DRAW) {
        // ---- 1. the ROI mask
        if (a.mask && a.mask_alpha != 0) {
#pragma unroll
            for (int dr = 0; dr < 2; ++dr) {
                if (dr < nrow) {
                    const uint8_t *m = a.mask + (int64_t)(r0 + dr) * a.Wc + c0;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < ncol && m[k] != 0) blend3(px[8 * dr + k], a.mask_colour, a.mask_alpha);
                }
            }
        }
        // ---- 2. the frame's boxes, in array order: LDS entries (r0, c0, r1, c1, colour, fill alpha | line alpha << 16)
        const int b_begin = a.box_start[f], b_end = a.box_start[f + 1];
        for (int base = b_begin; base < b_end; base += kChunk) {
            const int cnt = b_end - base < kChunk ? b_end - base : kChunk;
            __syncthreads();
            for (int k = threadIdx.x; k < cnt * 6; k += blockDim.x) lds[k] = a.boxes[(int64_t)base * 6 + k];
            __syncthreads();
            for (int b = 0; b < cnt; ++b) {
                const int br0 = lds[6 * b], bc0 = lds[6 * b + 1], br1 = lds[6 * b + 2], bc1 = lds[6 * b + 3];
                if (!live || br0 >= r0 + nrow || br1 <= r0 || bc0 >= c0 + ncol || bc1 <= c0) continue;
                const uint32_t colour = (uint32_t)lds[6 * b + 4];
                const int fill = lds[6 * b + 5] & 0xffff, line = lds[6 * b + 5] >> 16;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int r = r0 + (k >> 3), c = c0 + (k & 7);
                    if (r >= br0 && r < br1 && c >= bc0 && c < bc1) {
                        const bool edge = r == br0 || r == br1 - 1 || c == bc0 || c == bc1 - 1;
                        blend3(px[k], colour, edge ? line : fill);
                    }
                }
            }
        }
        // ---- 3. the frame's marks, in array order: LDS entries (r, c, colour, line alpha)
        const int m_begin = a.mark_start[f], m_end = a.mark_start[f + 1];
        for (int base = m_begin; base < m_end; base += kChunk) {
            const int cnt = m_end - base < kChunk ? m_end - base : kChunk;
            __syncthreads();
            for (int k = threadIdx.x; k < cnt * 4; k += blockDim.x) lds[k] = a.marks[(int64_t)base * 4 + k];
            __syncthreads();
            for (int m = 0; m < cnt; ++m) {
                const int64_t mr = lds[4 * m], mc = lds[4 * m + 1], arm = a.mark_arm;
                // the strip meets the vertical or the horizontal bar?
                const bool vbar = mc >= c0 && mc < c0 + ncol && mr + arm >= r0 && mr - arm < r0 + nrow;
                const bool hbar = mr >= r0 && mr < r0 + nrow && mc + arm >= c0 && mc - arm < c0 + ncol;
                if (!live || (!vbar && !hbar)) continue;
                const uint32_t colour = (uint32_t)lds[4 * m + 2];
                const int line = lds[4 * m + 3];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int64_t r = r0 + (k >> 3), c = c0 + (k & 7);
                    const int64_t dr = r > mr ? r - mr : mr - r, dc = c > mc ? c - mc : mc - c;
                    if ((c == mc && dr <= arm) || (r == mr && dc <= arm)) blend3(px[k], colour, line);
                }
            }
        }
        // ---- 4. the frame's border: (colour, line alpha) per frame, alpha < 0 = none
        if (a.frame_border) {
            const uint32_t colour = (uint32_t)a.frame_border[2 * (int64_t)f];
            const int line = a.frame_border[2 * (int64_t)f + 1];
            if (line >= 0 && a.border > 0) {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int r = r0 + (k >> 3), c = c0 + (k & 7);
                    if (r < a.border || r >= a.Hc - a.border || c < a.border || c >= a.Wc - a.border) blend3(px[k], colour, line);
                }
            }
        }
        // ---- 5. the frame's labels, in array order: LDS entries (r, c, scale, len, ink colour, ink alpha, plate colour, plate alpha,
        // 8 words of font indices)
        if constexpr (TEXT) {
            __shared__ uint8_t font[64 * 8];                             // (a font index is taken & 63: no index leaves the table)
            for (int k = threadIdx.x; k < 64 * 8; k += blockDim.x) font[k] = k < kReviewFontCount * 8 ? (&d_font[0][0])[k] : (uint8_t)0;
            const int l_begin = t.label_start[f], l_end = t.label_start[f + 1];
            for (int base = l_begin; base < l_end; base += kLabelChunk) {
                const int cnt = l_end - base < kLabelChunk ? l_end - base : kLabelChunk;
                __syncthreads();
                for (int k = threadIdx.x; k < cnt * 16; k += blockDim.x) lds[k] = t.labels[(int64_t)base * 16 + k];
                __syncthreads();
                for (int l = 0; l < cnt; ++l) {
                    const int32_t *e = &lds[16 * l];
                    const int64_t lr = e[0], lc = e[1];
                    const int s = e[2], len = e[3];
                    const int64_t top = lr - s, bottom = lr + 8 * s, left = lc - s, right = lc + (int64_t)6 * s * len;
                    if (!live || len <= 0 || top >= r0 + nrow || bottom <= r0 || left >= c0 + ncol || right <= c0) continue;
                    const uint32_t ink_colour = (uint32_t)e[4], plate_colour = (uint32_t)e[6];
                    const int ink_alpha = e[5], plate_alpha = e[7];
                    // x / s as (x * inv) >> 16, inv = ceil(2^16 / s): exact for x < 2048 and s <= 8 (the error x (inv - 2^16 / s) / 2^16 is
                    // below 1 / 32, the fraction of x / s at most 1 - 1 / 8); here x < 8 s <= 64 and x < 6 s len <= 1536
                    const uint32_t inv = (65536u + (uint32_t)s - 1u) / (uint32_t)s;
                    // the strip meets the rectangle, so its first pixel lies within 16 pixels of it: 32 bits from here on
                    const int v0 = (int)(r0 - lr), u0 = (int)(c0 - lc), tall = 8 * s, wide = 6 * s * len;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int v = v0 + (k >> 3), u = u0 + (k & 7);
                        if (v < -s || v >= tall || u < -s || u >= wide) continue;          // outside rows [r - s, r + 8 s) or columns [c - s, c + 6 s len)
                        bool ink = false;
                        if (v >= 0 && u >= 0) {
                            const uint32_t vs = ((uint32_t)v * inv) >> 16, cell = ((uint32_t)u * inv) >> 16, ci = cell / 6u, col = cell - 6u * ci;
                            if (vs < 7u && col < 5u) {
                                const uint32_t ch = ((uint32_t)e[8 + (ci >> 2)] >> (8 * (ci & 3u))) & 63u;          // ci < len <= 32
                                ink = ((font[8 * ch + vs] >> (4u - col)) & 1u) != 0;
                            }
                        }
                        blend3(px[k], ink ? ink_colour : plate_colour, ink ? ink_alpha : plate_alpha);
                    }
                }
            }
        }
    }
    if (!live) return;

    // ---- conversion and stores
    constexpr int h = 1 << 19;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr) {
        if (dr < nrow) {
            uint32_t w[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int *p = px[8 * dr + k];
                const int Y = (kYR * p[2] + kYG * p[1] + kYB * p[0] + h + (16 << 20)) >> 20;
                w[k >> 2] |= (uint32_t)Y << (8 * (k & 3));
            }
            store_run8(a.y + (int64_t)f * a.y_fs + (int64_t)(r0 + dr) * a.y_rs + c0, w[0], w[1], ncol);
        }
    }
    const int ncell = (ncol + 1) >> 1;
    uint32_t uw = 0u, vw = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int *p = px[2 * k];                                        // pixel (2 i, 2 j): the cell's top-left
        const int U = (kUR * p[2] + kUG * p[1] + kUB * p[0] + h + (128 << 20)) >> 20;
        const int V = (kVR * p[2] + kVG * p[1] + kVB * p[0] + h + (128 << 20)) >> 20;
        uw |= (uint32_t)U << (8 * k);
        vw |= (uint32_t)V << (8 * k);
    }
    const int64_t crow = (int64_t)f * a.c_fs + (int64_t)sr * a.c_rs;
    if (a.layout == SWK_YUV_I420) {
        store_run4(a.u + crow + 4 * sc, uw, ncell);
        store_run4(a.v + crow + 4 * sc, vw, ncell);
    } else {
        const uint32_t lo = (uw & 255u) | ((vw & 255u) << 8) | (((uw >> 8) & 255u) << 16) | (((vw >> 8) & 255u) << 24);
        const uint32_t hi = ((uw >> 16) & 255u) | (((vw >> 16) & 255u) << 8) | ((uw >> 24) << 16) | ((vw >> 24) << 24);
        store_run8(a.u + crow + 8 * sc, lo, hi, 2 * ncell);
    }
}

// The stage panels of a mosaic (swk_render_review_panels): blockIdx.z + 1 is the cell, blockIdx.y the frame, and a thread owns a strip of
// 8 x 2 pixels of the cell's Hp x Wp (the ROI's size made even), so a window's panels, pads and empty cells are one launch beside
// k_review's, which writes cell 0 at the mosaic's strides.  A panel's pixel is read as one byte where the plane lies, mapped (gain, or the
// palette held in 1 KB of LDS), composed with the chosen layers and the caption exactly as k_review composes and converts; the pixels of
// a strip that lie beyond the ROI (an odd size's pad row / column) and every pixel of a cell past the panels are black before the
// conversion, which gives Y = 16, U = V = 128.  blockIdx.z == gridDim.z - 1 is cell 0 where the ROI's size is odd: only its pad luma
// bytes are written (k_review owns the rest of it).
__global__ __launch_bounds__(256) void k_review_panels(ReviewArgs a, int f0, ReviewPanels q)
{
    __shared__ int32_t lds[kChunk * 6];
    __shared__ uint8_t font[64 * 8];
    __shared__ uint32_t pal[256];
    const int f = f0 + (int)blockIdx.y;
    const int Hp = a.Hc + (a.Hc & 1), Wp = a.Wc + (a.Wc & 1);
    const int cell = (int)blockIdx.z + 1 < q.ncells ? (int)blockIdx.z + 1 : 0;          // (the grid has a slice past the cells only for cell 0's pads)
    const int sw = (Wp + 7) >> 3, sh = Hp >> 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < sw * sh;
    const int sr = live ? idx / sw : 0, sc = live ? idx - sr * sw : 0;
    const int r0 = 2 * sr, c0 = 8 * sc;
    const int ncol = !live ? 0 : (Wp - c0 < 8 ? Wp - c0 : 8);                            // the pixels that leave: even, rows always 2
    const int vcol = !live ? 0 : (a.Wc - c0 < 8 ? (a.Wc - c0 < 0 ? 0 : a.Wc - c0) : 8);  // the pixels of the ROI among them
    const int vrow = !live ? 0 : (a.Hc - r0 < 2 ? a.Hc - r0 : 2);
    const int oy = (cell / q.cols) * Hp, ox = (cell % q.cols) * Wp;                      // the cell's origin: even
    uint8_t *y = a.y + (int64_t)f * a.y_fs + (int64_t)oy * a.y_rs + ox;
    if (cell == 0) {
        if (!live) return;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int r = r0 + (k >> 3), c = c0 + (k & 7);
            if (c < Wp && (r >= a.Hc || c >= a.Wc)) y[(int64_t)r * a.y_rs + c] = (uint8_t)16;
        }
        return;
    }
    int px[16][3];
#pragma unroll
    for (int k = 0; k < 16; ++k) px[k][0] = px[k][1] = px[k][2] = 0;
    if (cell <= q.npanels) {
        const ReviewPanel &p = q.panel[cell - 1];
        if (p.kind == SWK_PANEL_LABELS) {
            for (int k = threadIdx.x; k < 256; k += blockDim.x) pal[k] = q.palette[k];
            __syncthreads();
        }
        // ---- source pixels: two runs of vcol bytes, mapped
#pragma unroll
        for (int dr = 0; dr < 2; ++dr) {
            if (dr < vrow) {
                const uint8_t *s = p.plane + (int64_t)f * p.fs + (int64_t)(r0 + dr) * p.rs + c0;
                uint32_t w0 = 0u, w1 = 0u;
                if (vcol == 8 && ((uintptr_t)s & 7) == 0) { const uint2 t = *(const uint2 *)s; w0 = t.x; w1 = t.y; }
                else if (vcol == 8 && ((uintptr_t)s & 3) == 0) { w0 = ((const uint32_t *)s)[0]; w1 = ((const uint32_t *)s)[1]; }
                else {
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < vcol) { if (k < 4) w0 |= (uint32_t)s[k] << (8 * k); else w1 |= (uint32_t)s[k] << (8 * (k - 4)); }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t v = ((k < 4 ? w0 : w1) >> (8 * (k & 3))) & 255u;
                    uint32_t bgr;
                    if (p.kind == SWK_PANEL_LABELS) bgr = pal[v];
                    else { const uint32_t g = v * (uint32_t)p.gain; bgr = (g > 255u ? 255u : g) * 0x010101u; }
                    px[8 * dr + k][0] = (int)(bgr & 255u); px[8 * dr + k][1] = (int)((bgr >> 8) & 255u); px[8 * dr + k][2] = (int)(bgr >> 16);
                }
            }
        }
        if (p.layers & 1) draw_mask(px, a, r0, c0, vrow, vcol);
        if (p.layers & 2) draw_boxes(px, lds, a, f, live, r0, c0, vrow, vcol);
        if (p.layers & 4) draw_marks(px, lds, a, f, live, r0, c0, vrow, vcol);
        if (p.layers & 8) draw_border(px, a, f, r0, c0);
        draw_labels(px, lds, font, q.captions, cell - 1, cell, live, r0, c0, vrow, vcol);
        // what was drawn beyond the ROI (boxes and labels may leave it) is not part of the picture
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((k >> 3) >= vrow || (k & 7) >= vcol) px[k][0] = px[k][1] = px[k][2] = 0;
    }
    if (!live) return;
    const int cbytes = a.layout == SWK_YUV_I420 ? 1 : 2;
    const int64_t coff = (int64_t)f * a.c_fs + (int64_t)(oy >> 1) * a.c_rs + (ox >> 1) * cbytes;
    store_strip(px, y, a.u, a.v, coff, a.y_rs, a.c_rs, a.layout, sr, sc, 2, ncol);
}

void launch_review_panels(hipStream_t s, const ReviewArgs &a, int F, const ReviewPanels &q)
{
    const int Hp = a.Hc + (a.Hc & 1), Wp = a.Wc + (a.Wc & 1);
    const int strips = ((Wp + 7) >> 3) * (Hp >> 1);
    const int slices = q.ncells - 1 + (Hp != a.Hc || Wp != a.Wc ? 1 : 0);          // the cells after cell 0, then cell 0's pads
    if (slices == 0) return;
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        hipLaunchKernelGGL(k_review_panels, dim3((strips + 255) / 256, fc, slices), dim3(256), 0, s, a, f0, q);
        note_launch();
    }
}

void launch_review(hipStream_t s, const ReviewArgs &a, int F, bool draw, const ReviewLabels *text)
{
    const int strips = ((a.Wc + 7) >> 3) * ((a.Hc + 1) >> 1);
    // grid.y is limited to 65535: split the frame range
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        const dim3 grid((strips + 255) / 256, fc);
        if (draw && text) hipLaunchKernelGGL((k_review<true, true>), grid, dim3(256), 0, s, a, f0, *text);
        else if (draw) hipLaunchKernelGGL((k_review<true, false>), grid, dim3(256), 0, s, a, f0, NoLabels{});
        else hipLaunchKernelGGL((k_review<false, false>), grid, dim3(256), 0, s, a, f0, NoLabels{});
        note_launch();
    }
}

}  // namespace swk
