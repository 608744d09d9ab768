// What the classifier's convolution kernels (cnn_*.hip) share: the placement arguments and their host check, the fused
// bias + ReLU + float4 epilogue, the three-way bf16 split (device and host), the Winograd filter transform and the LDS-DMA copy.
#pragma once
#include "swk_internal.h"

#include <cstring>

namespace swk {

typedef float f16v __attribute__((ext_vector_type(16)));          // accumulator of a 32 x 32 MFMA
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));        // A / B operand of v_mfma_f32_32x32x16_bf16

// Where a kernel puts its output: the h x w x c block of segment n goes to dst[n][off_y ..][off_x ..][c_off ..] of the next layer's
// tile, dst being [n][dH][dW][dC] channels-last.
struct Place {
    float *dst;
    int dH, dW, dC, off_y, off_x, c_off;
};
// Where a 1x1 kernel reads its input: the h x w window at (crop_y, crop_x) of src, [n][sh][sw][channels].
struct Crop {
    int sh, sw, crop_y, crop_x;
};

// The host check of every placement entry point: the h x w x c block lies inside dst (and the window inside src).  quads: the kernel
// stores float4s of four consecutive channels, so c, dC and c_off are multiples of four and dst is 16-byte aligned.
inline bool place_ok(const Place &p, int h, int w, int c, bool quads, const Crop *crop = nullptr)
{
    if (!p.dst || c < 1 || p.off_y < 0 || p.off_x < 0 || p.off_y + h > p.dH || p.off_x + w > p.dW || p.c_off < 0 || p.c_off + c > p.dC) return false;
    if (quads && ((c & 3) || (p.dC & 3) || (p.c_off & 3) || ((uintptr_t)p.dst & 15))) return false;
    return !crop || (crop->crop_y >= 0 && crop->crop_x >= 0 && crop->crop_y + h <= crop->sh && crop->crop_x + w <= crop->sw);
}

// expand1x1 of the Fire shapes with float32 products formed from split bf16 operands (cnn_expand_bf16.hip); SWK_ERR_ARG for other shapes
int launch_expand1x1_split_bf16(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int cin, int h, int w, const float *wgt,
                                const float *bias, int cout, const Place &pl);
// the same products, bit for bit, with the split weights held in registers and the split activations shared through LDS
int launch_expand1x1_split_bf16_ws(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int cin, int h, int w, const float *wgt,
                                   const float *bias, int cout, const Place &pl);
// A/B switch (swk_set_cnn_tuning knob 1) for the expand1x1 shapes: 0 = the float32 kernel, 1 = the split-bf16 kernel with its weights in
// LDS, 2 = the split-bf16 kernel with its weights in registers, 3 = each shape's default (swk_nhwc_conv1x1_bias_relu_place)
extern int g_expand_split_bf16;
// the wide plain squeezes (256 -> 48, 384 -> 48, 384 -> 64) on split-bf16 products (cnn_squeeze_bf16.hip); SWK_ERR_ARG for other shapes
int launch_squeeze1x1_split_bf16(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int cin, int h, int w, const float *wgt,
                                 const float *bias, int cout, const Place &pl);
extern int g_squeeze_split_bf16;         // A/B switch (swk_set_cnn_tuning knob 4), conv1 and the wide squeezes: 0 = the float32 kernels, 1 = each shape's default
extern int g_wino_bf16s_layout;         // A/B switch (swk_set_cnn_tuning knob 2): workgroup layout of the split-bf16 Winograd expands

// The fused epilogue: register quad g of an accumulator = four consecutive output channels of the lane's pixel; bias, ReLU, one
// float4 store.  An add, then a max (the library is built without contraction).
__device__ __forceinline__ void store_bias_relu(float *q, const f16v &acc, int g, const float4 b)
{
    float4 v;
    v.x = fmaxf(acc[4 * g] + b.x, 0.0f);
    v.y = fmaxf(acc[4 * g + 1] + b.y, 0.0f);
    v.z = fmaxf(acc[4 * g + 2] + b.z, 0.0f);
    v.w = fmaxf(acc[4 * g + 3] + b.w, 0.0f);
    *(float4 *)q = v;
}

// x = a + b + c, each part bf16 (round to nearest even), the remainders exact in float32: 3 x 8 bits cover float32's 24.
// The split kernels are float32-accurate only if the device form (activations, 1x1 weights) and the host form (Winograd filters,
// finite values) round alike.
__device__ __forceinline__ void split3(float x, __bf16 &a, __bf16 &b, __bf16 &c)
{
    a = (__bf16)x;
    const float r = x - (float)a;
    b = (__bf16)r;
    c = (__bf16)(r - (float)b);
}
// eight consecutive channels (two float4s) into the three operands of a k-step of v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ void split3(const float4 lo, const float4 hi, bf16x8 &p1, bf16x8 &p2, bf16x8 &p3)
{
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __bf16 a, b, c;
        split3(v[j], a, b, c);
        p1[j] = a; p2[j] = b; p3[j] = c;
    }
}
inline void split3_host(float x, uint16_t part[3])
{
    for (int i = 0; i < 3; ++i) {
        uint32_t u;
        float back;
        memcpy(&u, &x, 4);
        u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
        memcpy(&back, &u, 4);
        part[i] = (uint16_t)(u >> 16);
        x -= back;
    }
}

// Winograd F(2x2, 3x3) filter transform U = G g G^T of one 3 x 3 filter, in float64 (the weight layouts round it to float32).
inline void winograd_U(const float g[9], double U[4][4])
{
    static const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
    double tmp[4][3];
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 3; ++c) tmp[a][c] = G[a][0] * g[c] + G[a][1] * g[3 + c] + G[a][2] * g[6 + c];
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) U[a][c] = tmp[a][0] * G[c][0] + tmp[a][1] * G[c][1] + tmp[a][2] * G[c][2];
}

// LDS-DMA: N consecutive 1 KB pieces (16 bytes per lane) from g to the LDS address lds (both wave-uniform), the lane's place in a
// piece given by voff; the pieces are addressed by the instruction offset, which advances the global and the LDS address alike.
// Written as an asm statement: through __builtin_amdgcn_global_load_lds the compiler treats the copy as an LDS store that
// every later ds_read may alias and waits for it (s_waitcnt vmcnt(0)) before the very next operand read -- the copy is then
// no longer asynchronous.  The waits are placed by hand instead: lds_dma_wait<KEEP>() retires the copies and leaves the KEEP
// vector-memory loads issued after them in flight (the kernel counts them).
template <int N>
__device__ __forceinline__ void lds_dma_copy(unsigned lds, const void *g, unsigned voff)
{
    static_assert(N >= 1 && N <= 3, "1 KB pieces per statement");
    unsigned keep;
#define SWK_LDS_DMA(pieces)                                                                                                 \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t" pieces "s_mov_b32 m0, %0" : "=&s"(keep) : "v"(voff), "s"(lds), "s"(g) : "memory")
#define SWK_LDS_DMA_PIECE(offset) "global_load_lds_dwordx4 %1, %3" offset "\n\t"
    if constexpr (N == 1) SWK_LDS_DMA(SWK_LDS_DMA_PIECE(""));
    else if constexpr (N == 2) SWK_LDS_DMA(SWK_LDS_DMA_PIECE("") SWK_LDS_DMA_PIECE(" offset:1024"));
    else SWK_LDS_DMA(SWK_LDS_DMA_PIECE("") SWK_LDS_DMA_PIECE(" offset:1024") SWK_LDS_DMA_PIECE(" offset:2048"));
#undef SWK_LDS_DMA_PIECE
#undef SWK_LDS_DMA
}
template <int KEEP>
__device__ __forceinline__ void lds_dma_wait()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KEEP) : "memory");
}

}  // namespace swk
