// Glue kernels of the receptive-field cropped classifier (swiftwatcher_amd/segment_classification.py): what is left between
// the convolution kernels (cnn_conv1x1.hip, cnn_conv3x3.hip, cnn_wino3x3.hip, which carry bias, ReLU and placement
// themselves) -- bias + ReLU + crop behind conv1 (MIOpen), and the three max-pools (PyTorch's NHWC max-pool kernel runs far
// below the memory rate).  Plain streaming jobs, launched on the CALLER's stream (PyTorch's current stream).
// Layout: channels-last dense float32, tensor (n, c, h, w) = memory [n][h][w][c].
#include "cnn_common.h"

namespace swk {

// dst[n][off_y + y][off_x + x][c_off + ch] = max(src[n][crop_y + y][crop_x + x][ch] + bias[ch], 0)
// for y < h, x < w, ch < c;  src is [n][sh][sw][c], dst is [n][dH][dW][dC].  c, dC, c_off multiples of 4.
__global__ __launch_bounds__(256) void k_bias_relu_place(const float4 *__restrict__ src, int sh, int sw, int c4, int crop_y, int crop_x,
                                                         int h, int w, const float4 *__restrict__ bias, float4 *__restrict__ dst,
                                                         int dH, int dW, int dC4, int off_y, int off_x, int c_off4, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % c4);
    int64_t r = i / c4;
    const int x = (int)(r % w); r /= w;
    const int y = (int)(r % h);
    const int64_t n = r / h;
    const float4 v = src[((n * sh + crop_y + y) * sw + crop_x + x) * c4 + ch];
    const float4 b = bias[ch];
    float4 o;
    o.x = fmaxf(v.x + b.x, 0.0f); o.y = fmaxf(v.y + b.y, 0.0f); o.z = fmaxf(v.z + b.z, 0.0f); o.w = fmaxf(v.w + b.w, 0.0f);
    dst[((n * dH + off_y + y) * dW + off_x + x) * dC4 + c_off4 + ch] = o;
}

// MaxPool2d(3, stride 2) without padding over [n][h][w][c] -> [n][oh][ow][c], oh = (h - 3) / 2 + 1.
// One thread = one output ROW of one channel quad: it walks the row's columns once, keeping the maximum of the column it shares
// with the next window (6 loads per output instead of 9; lanes = consecutive channel quads, every load 1 KB per wave).
__global__ __launch_bounds__(256) void k_maxpool3s2(const float4 *__restrict__ src, int h, int w, int c4, float4 *__restrict__ dst,
                                                    int oh, int ow, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % c4);
    int64_t r = i / c4;
    const int oy = (int)(r % oh);
    const int64_t n = r / oh;
    const float4 *p = src + ((n * h + 2 * oy) * w) * c4 + ch;
    const int64_t rs = (int64_t)w * c4;
    auto colmax = [&](int x) {
        const float4 a = p[(int64_t)x * c4], b = p[rs + (int64_t)x * c4], c = p[2 * rs + (int64_t)x * c4];
        float4 m;
        m.x = fmaxf(fmaxf(a.x, b.x), c.x); m.y = fmaxf(fmaxf(a.y, b.y), c.y);
        m.z = fmaxf(fmaxf(a.z, b.z), c.z); m.w = fmaxf(fmaxf(a.w, b.w), c.w);
        return m;
    };
    float4 prev = colmax(0);
    float4 *q = dst + ((n * oh + oy) * ow) * (int64_t)c4 + ch;
#pragma unroll 3
    for (int ox = 0; ox < ow; ++ox) {
        const float4 c1 = colmax(2 * ox + 1), c2 = colmax(2 * ox + 2);
        float4 m;
        m.x = fmaxf(fmaxf(prev.x, c1.x), c2.x); m.y = fmaxf(fmaxf(prev.y, c1.y), c2.y);
        m.z = fmaxf(fmaxf(prev.z, c1.z), c2.z); m.w = fmaxf(fmaxf(prev.w, c1.w), c2.w);
        q[(int64_t)ox * c4] = m;
        prev = c2;
    }
}

// The classifier's head (Dropout is the identity in eval mode, then Conv2d(512, 2, 1), ReLU, AdaptiveAvgPool2d(1): torchvision's
// SqueezeNet classifier as segment_classification.py:47-67 of the reference re-heads it) over the live square of the last Fire's
// output, [n][px][c] channels-last:
//     out[n][k] = (sum_p max(sum_ch x[n][p][ch] w[k][ch] + bias[k], 0) + ring[k]) / n_pos,       k = 0, 1
// (ring: the sum over the positions outside the square, which do not depend on the segment).  One workgroup per segment, four waves;
// a wave takes pixels wave, wave + 4, ...: lane l holds the weights of channels 256 j + 4 l .. + 3, multiplies its float4s, the two
// sums cross the wave as a butterfly, pixels add up in order, the four waves in order: the summation order is a function of the
// shapes alone, so a segment's score does not depend on the batch it is scored in (the library product this replaces picked its
// kernel, and with it the last bit, by the row count).  Memory-bound: 4 c bytes per pixel read once.
template <int CJ>
__global__ __launch_bounds__(256) void k_head2_relu_mean(const float *__restrict__ x, int px, const float *__restrict__ w,
                                                         const float *__restrict__ bias, const float *__restrict__ ring, float inv_pos,
                                                         float *__restrict__ out)
{
    constexpr int C = 256 * CJ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *xp = x + (int64_t)blockIdx.x * px * C + 4 * lane;
    float4 w0[CJ], w1[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
        w0[j] = *(const float4 *)(w + 256 * j + 4 * lane);
        w1[j] = *(const float4 *)(w + C + 256 * j + 4 * lane);
    }
    const float b0 = bias[0], b1 = bias[1];
    float s0 = 0.0f, s1 = 0.0f;
    auto dot = [&](const float4 (&v)[CJ], float &d0, float &d1) {
        d0 = 0.0f; d1 = 0.0f;
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            d0 = fmaf(v[j].x, w0[j].x, d0); d0 = fmaf(v[j].y, w0[j].y, d0); d0 = fmaf(v[j].z, w0[j].z, d0); d0 = fmaf(v[j].w, w0[j].w, d0);
            d1 = fmaf(v[j].x, w1[j].x, d1); d1 = fmaf(v[j].y, w1[j].y, d1); d1 = fmaf(v[j].z, w1[j].z, d1); d1 = fmaf(v[j].w, w1[j].w, d1);
        }
    };
    auto across = [&](float v) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        return v;
    };
    // two pixels per trip: their loads leave together
    int p = wave;
    for (; p + 4 < px; p += 8) {
        float4 va[CJ], vb[CJ];
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            va[j] = *(const float4 *)(xp + (int64_t)p * C + 256 * j);
            vb[j] = *(const float4 *)(xp + (int64_t)(p + 4) * C + 256 * j);
        }
        float a0, a1, c0, c1;
        dot(va, a0, a1);
        dot(vb, c0, c1);
        s0 += fmaxf(across(a0) + b0, 0.0f); s1 += fmaxf(across(a1) + b1, 0.0f);
        s0 += fmaxf(across(c0) + b0, 0.0f); s1 += fmaxf(across(c1) + b1, 0.0f);
    }
    if (p < px) {
        float4 va[CJ];
#pragma unroll
        for (int j = 0; j < CJ; ++j) va[j] = *(const float4 *)(xp + (int64_t)p * C + 256 * j);
        float a0, a1;
        dot(va, a0, a1);
        s0 += fmaxf(across(a0) + b0, 0.0f); s1 += fmaxf(across(a1) + b1, 0.0f);
    }
    __shared__ float part[4][2];
    if (lane == 0) { part[wave][0] = s0; part[wave][1] = s1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        const float t = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
        out[(int64_t)blockIdx.x * 2 + k] = (t + ring[k]) * inv_pos;
    }
}

// Philox4x32-10 (Salmon et al., SC'11; the constants of Random123): counter (c0..c3), key (k0, k1) -> four 32-bit words.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// The same head with the reference's LIVE Dropout(0.5) in front of it (the reference never leaves train mode), S realisations per
// segment in one launch:
//     out[n][s][k] = (sum_{p < n_pos} max(sum_ch 2 m(n, s, p, ch) f(n, p, ch) w[k][ch] + bias[k], 0)) / n_pos
// f = x[n][j] where pos[j] == p, bg[p] at the other positions (the ring is dropped per segment and sample like everything else, so it
// cannot be a constant here).  The mask m is defined in swk.h: Philox4x32-10 keyed by the seed, counter (p c/4 + ch/4, s >> 5, segment
// key): ONE generator call gives a lane the bits of its four channels for 32 samples.
// One workgroup per segment, four waves, a wave takes positions wave, wave + 4, ... of the full map; lane l holds (twice) the weights
// of channels 256 j + 4 l .. + 3 and reads its float4s ONCE per position.  Per block of 32 samples a lane keeps 64 partial sums
// (value v = 32 k + s); they cross the wave as a transposing butterfly -- at distance h a lane hands over the half of its values whose
// bit h differs from its own lane bit and adds what it receives to the half it keeps: 63 exchanges instead of 64 x 6, and lane l ends
// with the complete sum of value l.  (A block of at most four samples takes a plain butterfly per value instead: same sums, fewer exchanges.)  Bias, ReLU and the sum over positions then run on all 64 lanes (one value each, in LDS per wave
// and block of samples); the four waves add up in order.  Summation order: a function of (c, px, n_pos, S) alone.
template <int CJ>
__global__ __launch_bounds__(256) void k_head2_dropout_relu_mean(const float *__restrict__ x, int px, const int32_t *__restrict__ pos,
                                                                 const float *__restrict__ bg, int n_pos, const float *__restrict__ w,
                                                                 const float *__restrict__ bias, const uint64_t *__restrict__ keys,
                                                                 uint64_t seed, int S, float inv_pos, float *__restrict__ out)
{
    constexpr int C = 256 * CJ;
    extern __shared__ int32_t live_of[];          // [n_pos]: row of x that holds position p, or -1 (bg)
    __shared__ float part[4][8][64];               // [wave][block of 32 samples][value]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < n_pos; i += 256) live_of[i] = -1;
    for (int i = threadIdx.x; i < 4 * 8 * 64; i += 256) (&part[0][0][0])[i] = 0.0f;
    __syncthreads();
    for (int j = threadIdx.x; j < px; j += 256) {
        const int q = pos[j];
        if ((unsigned)q < (unsigned)n_pos) live_of[q] = j;
    }
    __syncthreads();
    const float *xs = x + (int64_t)blockIdx.x * px * C + 4 * lane;
    float4 w0[CJ], w1[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
        w0[j] = *(const float4 *)(w + 256 * j + 4 * lane);
        w1[j] = *(const float4 *)(w + C + 256 * j + 4 * lane);
        // nn.Dropout scales what it keeps by 1 / (1 - 0.5): exact
        w0[j].x *= 2.0f; w0[j].y *= 2.0f; w0[j].z *= 2.0f; w0[j].w *= 2.0f;
        w1[j].x *= 2.0f; w1[j].y *= 2.0f; w1[j].z *= 2.0f; w1[j].w *= 2.0f;
    }
    const float b = bias[lane >> 5];
    const uint64_t key = keys[blockIdx.x];
    const uint32_t key_lo = (uint32_t)key, key_hi = (uint32_t)(key >> 32), seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
    const int nblk = (S + 31) >> 5;
    for (int p = wave; p < n_pos; p += 4) {
        const int row = live_of[p];
        float4 f[CJ];
        if (row >= 0) {
#pragma unroll
            for (int j = 0; j < CJ; ++j) f[j] = *(const float4 *)(xs + (int64_t)row * C + 256 * j);
        } else if (bg) {
#pragma unroll
            for (int j = 0; j < CJ; ++j) f[j] = *(const float4 *)(bg + (int64_t)p * C + 256 * j + 4 * lane);
        } else {
#pragma unroll
            for (int j = 0; j < CJ; ++j) f[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        for (int blk = 0; blk < nblk; ++blk) {
            const int ns = min(32, S - 32 * blk);
            float a[64];
#pragma unroll
            for (int v = 0; v < 64; ++v) a[v] = 0.0f;
#pragma unroll
            for (int j = 0; j < CJ; ++j) {
                uint32_t m[4];
                philox4x32_10((uint32_t)(p * (C / 4) + 64 * j + lane), (uint32_t)blk, key_lo, key_hi, seed_lo, seed_hi, m);
                const float fv[4] = {f[j].x, f[j].y, f[j].z, f[j].w};
                const float u0[4] = {w0[j].x, w0[j].y, w0[j].z, w0[j].w};
                const float u1[4] = {w1[j].x, w1[j].y, w1[j].z, w1[j].w};
#pragma unroll
                for (int s = 0; s < 32; ++s) {
                    if (s < ns) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const bool keep = (m[q] >> s) & 1u;
                            a[s] = keep ? fmaf(fv[q], u0[q], a[s]) : a[s];
                            a[32 + s] = keep ? fmaf(fv[q], u1[q], a[32 + s]) : a[32 + s];
                        }
                    }
                }
            }
            if (ns <= 4) {
                // a few samples (S = 1 is how a counting loop decides): a plain butterfly per value, 12 ns exchanges instead of 63.  Lane
                // v of a plain butterfly adds the same pairs in the same order as the transposing one below (a + b = b + a bit for
                // bit), so a sample's score does not depend on which path its block takes.
                float mine = 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (s < ns) {
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            float t = a[32 * k + s];
#pragma unroll
                            for (int h = 32; h >= 1; h >>= 1) t += __shfl_xor(t, h, 64);
                            mine = lane == 32 * k + s ? t : mine;
                        }
                    }
                }
                a[0] = mine;
            } else {
#pragma unroll
                for (int half = 32; half >= 1; half >>= 1) {
                    const bool up = lane & half;
#pragma unroll
                    for (int v = 0; v < half; ++v) {
                        const float send = up ? a[v] : a[v + half];
                        const float keep = up ? a[v + half] : a[v];
                        a[v] = keep + __shfl_xor(send, half, 64);
                    }
                }
            }
            part[wave][blk][lane] += fmaxf(a[0] + b, 0.0f);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nblk * 64; i += 256) {
        const int blk = i >> 6, v = i & 63, s = 32 * blk + (v & 31);
        const float t = ((part[0][blk][v] + part[1][blk][v]) + part[2][blk][v]) + part[3][blk][v];
        if (s < S) out[((int64_t)blockIdx.x * S + s) * 2 + (v >> 5)] = t * inv_pos;
    }
}

}  // namespace swk

#pragma GCC visibility push(default)
extern "C" {

int32_t swk_nhwc_bias_relu_place(void *stream, const float *src, int32_t n, int32_t sh, int32_t sw, int32_t c, int32_t crop_y,
                                 int32_t crop_x, int32_t h, int32_t w, const float *bias, float *dst, int32_t dH, int32_t dW,
                                 int32_t dC, int32_t off_y, int32_t off_x, int32_t c_off)
{
    const swk::Place pl{dst, dH, dW, dC, off_y, off_x, c_off};
    const swk::Crop cr{sh, sw, crop_y, crop_x};
    // beyond the placement: float4 loads of src and bias (16-byte aligned)
    if (!src || !bias || n < 1 || h < 1 || w < 1 || !swk::place_ok(pl, h, w, c, true, &cr) || (((uintptr_t)src | (uintptr_t)bias) & 15))
        return SWK_ERR_ARG;
    const int64_t total = (int64_t)n * h * w * (c / 4);
    hipLaunchKernelGGL(swk::k_bias_relu_place, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)src, sh, sw, c / 4, crop_y, crop_x, h, w, (const float4 *)bias, (float4 *)dst, dH, dW, dC / 4,
                       off_y, off_x, c_off / 4, total);
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

int32_t swk_nhwc_maxpool3s2(void *stream, const float *src, int32_t n, int32_t h, int32_t w, int32_t c, float *dst)
{
    if (!src || !dst || n < 1 || h < 3 || w < 3 || c < 4 || (c & 3) || (((uintptr_t)src | (uintptr_t)dst) & 15)) return SWK_ERR_ARG;
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    const int64_t total = (int64_t)n * oh * (c / 4);
    hipLaunchKernelGGL(swk::k_maxpool3s2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)src, h, w, c / 4, (float4 *)dst, oh, ow, total);
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

int32_t swk_nhwc_head2_relu_mean(void *stream, const float *x, int32_t n, int32_t px, int32_t c, const float *w, const float *bias,
                                 const float *ring, float n_pos, float *out)
{
    if (!x || !w || !bias || !ring || !out || n < 1 || px < 1 || !(n_pos > 0.0f) || (((uintptr_t)x | (uintptr_t)w) & 15)) return SWK_ERR_ARG;
    if (c != 256 && c != 512 && c != 768 && c != 1024) return SWK_ERR_ARG;
    const dim3 grid((unsigned)n), block(256);
    hipStream_t st = (hipStream_t)stream;
    const float inv = 1.0f / n_pos;
    switch (c / 256) {
    case 1: hipLaunchKernelGGL(swk::k_head2_relu_mean<1>, grid, block, 0, st, x, px, w, bias, ring, inv, out); break;
    case 2: hipLaunchKernelGGL(swk::k_head2_relu_mean<2>, grid, block, 0, st, x, px, w, bias, ring, inv, out); break;
    case 3: hipLaunchKernelGGL(swk::k_head2_relu_mean<3>, grid, block, 0, st, x, px, w, bias, ring, inv, out); break;
    default: hipLaunchKernelGGL(swk::k_head2_relu_mean<4>, grid, block, 0, st, x, px, w, bias, ring, inv, out); break;
    }
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

int32_t swk_nhwc_head2_dropout_relu_mean(void *stream, const float *x, int32_t n, int32_t px, int32_t c, const int32_t *pos, const float *bg,
                                         int32_t n_pos, const float *w, const float *bias, const uint64_t *keys, uint64_t seed,
                                         int32_t samples, float *out)
{
    // bg may be NULL only when every position is live
    if (!x || !pos || !w || !bias || !keys || !out || n < 1 || px < 1 || n_pos < 1 || n_pos > 8192 || px > n_pos || (!bg && px != n_pos))
        return SWK_ERR_ARG;
    if (samples < 1 || samples > 256 || (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bg) & 15) || ((uintptr_t)keys & 7)) return SWK_ERR_ARG;
    if (c != 256 && c != 512 && c != 768 && c != 1024) return SWK_ERR_ARG;
    const dim3 grid((unsigned)n), block(256);
    hipStream_t st = (hipStream_t)stream;
    const float inv = 1.0f / (float)n_pos;
    const size_t lds = (size_t)n_pos * sizeof(int32_t);
    switch (c / 256) {
    case 1: hipLaunchKernelGGL(swk::k_head2_dropout_relu_mean<1>, grid, block, lds, st, x, px, pos, bg, n_pos, w, bias, keys, seed, samples, inv, out); break;
    case 2: hipLaunchKernelGGL(swk::k_head2_dropout_relu_mean<2>, grid, block, lds, st, x, px, pos, bg, n_pos, w, bias, keys, seed, samples, inv, out); break;
    case 3: hipLaunchKernelGGL(swk::k_head2_dropout_relu_mean<3>, grid, block, lds, st, x, px, pos, bg, n_pos, w, bias, keys, seed, samples, inv, out); break;
    default: hipLaunchKernelGGL(swk::k_head2_dropout_relu_mean<4>, grid, block, lds, st, x, px, pos, bg, n_pos, w, bias, keys, seed, samples, inv, out); break;
    }
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

}  // extern "C"
#pragma GCC visibility pop
