// The wide plain squeezes of the Fire modules (256 -> 48, 384 -> 48, 384 -> 64; segment_classification.py of the reference :14-67 via
// torchvision's SqueezeNet-1.0) with every float32 product formed as a sum of six bfloat16 products of three-way split operands, as
// cnn_expand_bf16.hip forms them (same split3, same six products per k-step, smallest first, same epilogue).
//
// The hypothesis this kernel was built on, and what became of it: with N padded to 64 v_mfma_f32_32x32x2_f32 caps a 1x1 convolution at
// 4.9 TB/s of input, k_conv1x1_relu_place held these three layers at 3.3-3.5 TB/s, so they were taken to be pipe-bound in a
// memory-shaped layer, and split products cost 6 x 32 cycles per 16 channels and column block where float32 costs
// 8 x 64.  REFUTED in part: with the matrix time cut to a quarter the layers stream at about 4 TB/s in every workgroup layout tried (last
// bullet below) -- they are held by memory short of the 6.3 TB/s other kernels reach.  What the kernel gains (12-14 %
// per layer) comes from the shorter matrix time at the ends of a launch and from the finer split of the row tiles over the waves.
//
// k_squeeze1x1_bf16s generalises k_expand1x1_bf16s (split weights in LDS) to large K and N <= 64:
//   * operand roles as there: weights = A (i = output channel), pixels = B (j = pixel), an accumulator quad = four consecutive output
//     channels of the lane's own pixel; a wave owns a row tile of 32 pixels and both column blocks (32 accumulator registers).
//   * K = 256 or 384 does not fit in registers for a whole tile beside the next one: a ring of D activation chunks as in
//     k_conv1x1_relu_place, a chunk = 32 channels = one whole 128-byte line per pixel (lane (pixel r, half h) loads channels
//     32 c + 16 h .. + 15), the ring running on into the wave's next row tile.  A chunk is two k-steps: step i multiplies channels
//     32 c + 16 h + 8 i .. + 7 of half h -- a permuted k order, matched by the weight layout.  A chunk's registers are split right
//     before their products and, once both k-steps are split, refilled with the chunk that takes the slot next.
//   * split weights in LDS, [K / 16][2 column blocks][3 parts][2 halves][32 output channels][8 bf16]: an operand read is one
//     ds_read_b128 per lane, conflict-free; 96 KB at K = 256, 144 KB at K = 384 (one workgroup per CU), split once per persistent
//     workgroup while they are staged.  Output channels past cout (48 -> 64) are zero weights.
//   * operands are read from LDS one (k-step, column block) ahead of the products; the last read of a tile is the first of the next.
//   * FOUR waves per workgroup, one per SIMD, and a deep ring (half a tile at K = 384, a whole one at K = 256; up to 272 registers) at
//     every size.  Measured at 4,096 segments: with 16 waves and a ring of two chunks (124 registers) the three
//     layers ran 3 % faster than the float32 kernel, with 8 waves and four or six chunks 9 %, with four waves 13 % -- the time follows
//     the largest number of row tiles any wave gets (7 of 6.1, 13 of 12.25, 25 of 24.5), not the bytes in flight or the waves that
//     could cover the split: the kernel waits on memory at about 4 TB/s in every layout, well short of the matrix pipe.
// The result of a pixel does not depend on the number of workgroups: the kernel is chosen per shape, never per size.
// Launched on the CALLER's stream.
#include "cnn_common.h"

namespace swk {

// KS = cin / 16 k-steps; D = chunks in the ring; NWV waves per workgroup (one per SIMD), each with row tiles of its own.
template <int KS, int D>
__global__ __launch_bounds__(256) void k_squeeze1x1_bf16s(const float *__restrict__ src, int64_t rows, int sh, int sw, int crop_y, int crop_x,
                                                          int h, int w, const float *__restrict__ wgt, const float *__restrict__ bias, int cout,
                                                          float *__restrict__ dst, int dH, int dW, int dC, int off_y, int off_x, int c_off,
                                                          FastDiv fhw, FastDiv fw)
{
    constexpr int CIN = 16 * KS, NC = CIN / 32, NWV = 4, NT = 64 * NWV, ITEMS = KS * 128, OPS = 2 * KS;
    static_assert(KS % 2 == 0 && NC % D == 0, "whole chunks, whole rings");
    extern __shared__ uint4 lds_q[];               // split weights: [KS][2][3][2][32] x 16 bytes, then the bias padded to 64
    float *lbias = (float *)(lds_q + KS * 2 * 3 * 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int hw = h * w;
    const int64_t ntiles = (rows + 31) >> 5, stride = (int64_t)gridDim.x * NWV;
    int64_t tile = (int64_t)blockIdx.x * NWV + wave;

    // source pointer of this lane's pixel in a row tile (rows past the end repeat the last one)
    auto locate = [&](int64_t t) -> const float * {
        const unsigned m = (unsigned)t * 32u + (unsigned)r;          // rows < 2^31 (checked by the launcher)
        const unsigned mm = m < (unsigned)rows ? m : (unsigned)rows - 1u;
        const unsigned b = fhw.div(mm), rem = mm - b * (unsigned)hw;
        const unsigned y = fw.div(rem), x = rem - y * (unsigned)w;
        return src + (((int64_t)b * sh + crop_y + y) * sw + crop_x + x) * (int64_t)CIN + 16 * hh;
    };
    float4 a[D][4];
    const float *p = src, *pn = src;
    if (tile < ntiles) {           // the first chunks leave before the weights are staged
        p = locate(tile);
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int v = 0; v < 4; ++v) a[d][v] = *(const float4 *)(p + 32 * d + 4 * v);
    }
    // ---- weights: item = (k-step, column block, half, output channel): the eight floats W[co][32 (s / 2) + 16 half + 8 (s % 2) ..], split,
    //      three 16-byte stores.  Four items' loads leave before the first is split ----
    for (int i0 = tid; i0 < ITEMS; i0 += 4 * NT) {
        float4 lo[4], hi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * NT, m = i & 31, kg = (i >> 5) & 1, nb = (i >> 6) & 1, s = i >> 7, co = 32 * nb + m;
            lo[u] = make_float4(0.f, 0.f, 0.f, 0.f); hi[u] = lo[u];
            if (i < ITEMS && co < cout) {
                const float *q = wgt + (int64_t)co * CIN + 32 * (s >> 1) + 16 * kg + 8 * (s & 1);
                lo[u] = *(const float4 *)q; hi[u] = *(const float4 *)(q + 4);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * NT;
            if (i < ITEMS) {
                bf16x8 w1, w2, w3;
                split3(lo[u], hi[u], w1, w2, w3);
                uint4 *d = lds_q + (i >> 6) * 192 + (i & 63);
                d[0] = __builtin_bit_cast(uint4, w1); d[64] = __builtin_bit_cast(uint4, w2); d[128] = __builtin_bit_cast(uint4, w3);
            }
        }
    }
    for (int i = tid; i < 64; i += NT) lbias[i] = i < cout ? bias[i] : 0.0f;
    __syncthreads();

    // operand reads run one (k-step, column block) ahead of the products (two register sets, scheduling fences, as in k_expand1x1_bf16s)
    bf16x8 wq[2][3];
    auto read_w = [&](int op, int set) {
        const uint4 *q = lds_q + op * 192 + lane;
        wq[set][0] = __builtin_bit_cast(bf16x8, q[0]); wq[set][1] = __builtin_bit_cast(bf16x8, q[64]); wq[set][2] = __builtin_bit_cast(bf16x8, q[128]);
    };
    read_w(0, 0);
    for (; tile < ntiles; tile += stride) {
        const bool more = tile + stride < ntiles;
        if (more) pn = locate(tile + stride);
        f16v acc[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nb][e] = 0.0f;
#pragma unroll 1
        for (int c0 = 0; c0 < NC; c0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int c = c0 + d, kn = 32 * (c + D);          // kn: the chunk that takes this ring slot next
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    bf16x8 x1, x2, x3;
                    split3(a[d][2 * i], a[d][2 * i + 1], x1, x2, x3);
                    if (i == 1) {          // past the last tile pn still points at loadable pixels: no branch among the products
                        const float *q = kn < CIN ? p + kn : pn + (kn - CIN);
                        // fenced: left alone the scheduler moves every refill to the end of the loop body, right before its use
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int v = 0; v < 4; ++v) a[d][v] = *(const float4 *)(q + 4 * v);
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        const int op = 2 * (2 * c + i) + nb, set = (2 * i + nb) & 1;
                        read_w(op + 1 < OPS ? op + 1 : 0, set ^ 1);
                        // smallest terms first
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][0], x3, acc[nb], 0, 0, 0);
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][1], x2, acc[nb], 0, 0, 0);
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][2], x1, acc[nb], 0, 0, 0);
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][0], x2, acc[nb], 0, 0, 0);
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][1], x1, acc[nb], 0, 0, 0);
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][0], x1, acc[nb], 0, 0, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100 /* DS read */, 3, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008 /* MFMA */, 6, 0);
                    }
                }
            }
        }
        // ---- bias + ReLU + placement: register quads = four consecutive output channels of the lane's pixel (located anew: a
        //      destination offset kept through the products costs the registers the ring needs) ----
        const unsigned m = (unsigned)tile * 32u + (unsigned)r;
        if (m < (unsigned)rows) {
            const unsigned b = fhw.div(m), rem = m - b * (unsigned)hw;
            const unsigned y = fw.div(rem), x = rem - y * (unsigned)w;
            float *o = dst + (((int64_t)b * dH + off_y + y) * dW + off_x + x) * (int64_t)dC + c_off + 4 * hh;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = nb * 32 + 8 * g;
                    if (c + 4 * hh < cout) store_bias_relu(o + c, acc[nb], g, *(const float4 *)(lbias + c + 4 * hh));
                }
        }
        p = pn;
    }
}

template <int KS, int D>
static int launch_squeeze_bf16s(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int h, int w, const float *wgt, const float *bias,
                                int cout, const Place &pl)
{
    constexpr size_t lds = (size_t)KS * 2 * 3 * 64 * 16 + 64 * sizeof(float);
    static_assert(lds <= 160 * 1024 - 256, "the split weights fit the LDS");
    static unsigned long long attr_mask = 0;
    if (!ensure_dyn_lds((const void *)k_squeeze1x1_bf16s<KS, D>, 160 * 1024 - 256, attr_mask)) return SWK_ERR_HIP;
    if (rows > (int64_t)0x7fffff00) return SWK_ERR_CAPACITY;
    // persistent over the row tiles: one 4-wave workgroup per CU (the split weights take more than half of the LDS) at every size
    const int64_t ntiles = (rows + 31) / 32;
    int64_t blocks = (ntiles + 3) / 4;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL((k_squeeze1x1_bf16s<KS, D>), dim3((unsigned)blocks), dim3(256), lds, s, src, rows, cr.sh, cr.sw, cr.crop_y, cr.crop_x,
                       h, w, wgt, bias, cout, pl.dst, pl.dH, pl.dW, pl.dC, pl.off_y, pl.off_x, pl.c_off, FastDiv((unsigned)(h * w)), FastDiv((unsigned)w));
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

// the wide plain squeezes: SWK_ERR_ARG for anything else (the caller then takes the float32 kernel)
int launch_squeeze1x1_split_bf16(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int cin, int h, int w, const float *wgt,
                                 const float *bias, int cout, const Place &pl)
{
    if (cin == 256 && cout == 48) return launch_squeeze_bf16s<16, 8>(s, src, rows, cr, h, w, wgt, bias, cout, pl);
    if (cin == 384 && (cout == 48 || cout == 64)) return launch_squeeze_bf16s<24, 6>(s, src, rows, cr, h, w, wgt, bias, cout, pl);
    return SWK_ERR_ARG;
}

}  // namespace swk
