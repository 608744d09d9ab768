// 4:2:0 YUV -> BGR on gfx950: the hand-over point of a video decoder (planar I420 from a software decoder or a .y4m file,
// NV12 surfaces from a hardware one) to the segment path, which takes BGR frames.
//
// The arithmetic is OpenCV 4.1.0's cv2.cvtColor(yuv, COLOR_YUV2BGR_I420 / _NV12) restated (ITU-R BT.601, limited range, 20-bit
// fixed point; PARITY UNPINNED like BGR2GRAY):
//   y = max(0, Y - 16) * 1220542;  uu = U - 128;  vv = V - 128;  h = 1 << 19
//   R = sat8((y + h + 1673527 vv) >> 20)
//   G = sat8((y + h -  852492 vv - 409993 uu) >> 20)
//   B = sat8((y + h + 2116026 uu) >> 20)
// with an arithmetic shift; every intermediate fits int32 (largest magnitude 5.7e8).  Chroma is not interpolated: pixel (r, c)
// uses chroma sample (r >> 1, c >> 1); the chroma planes are ceil(H / 2) x ceil(W / 2).
//
// A byte-streaming kernel: 1.5 B read and 3 B written per pixel.  One thread converts four consecutive pixels of a row of the
// rectangle: the luma quad is one dword when its address allows it, the two or three chroma samples that cover it are one
// 2-byte (I420, per plane) or 4-byte (NV12) access when theirs does, and the twelve output bytes leave as three dwords, six
// 16-bit words or bytes, whichever the output address allows (k_gray4g's way, filters.hip): consecutive lanes stay on
// consecutive addresses whatever the rectangle's origin and width.
#include "swk_internal.h"

namespace swk {

namespace {

constexpr int kCY = 1220542, kCUB = 2116026, kCUG = -409993, kCVG = -852492, kCVR = 1673527, kShift = 20;

__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

}  // namespace

template <int LAYOUT>
__global__ __launch_bounds__(256) void k_yuv420_to_bgr(const uint8_t *__restrict__ yp, const uint8_t *__restrict__ up,
                                                       const uint8_t *__restrict__ vp, int64_t y_fs, int64_t y_rs, int64_t c_fs,
                                                       int64_t c_rs, int x0, int y0, int Hr, int Wr, uint8_t *__restrict__ out)
{
    const int f = blockIdx.y;
    const int wq = (Wr + 3) >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Hr * wq) return;
    const int r = idx / wq, c = (idx - r * wq) << 2;
    const int npx = Wr - c < 4 ? Wr - c : 4;
    const int yy = y0 + r, xx = x0 + c;

    // luma: pixels xx .. xx + npx - 1 of row yy
    const uint8_t *ys = yp + (int64_t)f * y_fs + (int64_t)yy * y_rs + xx;
    uint32_t lum[4];
    if (npx == 4 && ((uintptr_t)ys & 3) == 0) {
        const uint32_t w = *(const uint32_t *)ys;
#pragma unroll
        for (int k = 0; k < 4; ++k) lum[k] = (w >> (8 * k)) & 255u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) lum[k] = k < npx ? ys[k] : 16u;
    }

    // chroma: samples cx .. cx + ns - 1 of chroma row yy >> 1 cover the quad (ns = 1 .. 3; 3 only when xx is odd)
    const int cx = xx >> 1;
    const int ns = ((xx + npx - 1) >> 1) - cx + 1;
    uint32_t cu[3], cv[3];
    if (LAYOUT == SWK_YUV_I420) {
        const int64_t off = (int64_t)f * c_fs + (int64_t)(yy >> 1) * c_rs + cx;
        const uint8_t *us = up + off, *vs = vp + off;
        if (ns >= 2 && ((uintptr_t)us & 1) == 0) {
            const uint32_t w = *(const uint16_t *)us;
            cu[0] = w & 255u; cu[1] = w >> 8; cu[2] = ns == 3 ? us[2] : 128u;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) cu[k] = k < ns ? us[k] : 128u;
        }
        if (ns >= 2 && ((uintptr_t)vs & 1) == 0) {
            const uint32_t w = *(const uint16_t *)vs;
            cv[0] = w & 255u; cv[1] = w >> 8; cv[2] = ns == 3 ? vs[2] : 128u;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) cv[k] = k < ns ? vs[k] : 128u;
        }
    } else {
        const uint8_t *uv = up + (int64_t)f * c_fs + (int64_t)(yy >> 1) * c_rs + 2 * (int64_t)cx;
        if (ns >= 2 && ((uintptr_t)uv & 3) == 0) {
            const uint32_t w = *(const uint32_t *)uv;
            cu[0] = w & 255u; cv[0] = (w >> 8) & 255u; cu[1] = (w >> 16) & 255u; cv[1] = w >> 24;
            const uint32_t w2 = ns == 3 ? (uint32_t)*(const uint16_t *)(uv + 4) : 0x8080u;
            cu[2] = w2 & 255u; cv[2] = w2 >> 8;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { cu[k] = k < ns ? uv[2 * k] : 128u; cv[k] = k < ns ? uv[2 * k + 1] : 128u; }
        }
    }
    int ruv[3], guv[3], buv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int uu = (int)cu[k] - 128, vv = (int)cv[k] - 128;
        ruv[k] = (1 << (kShift - 1)) + kCVR * vv;
        guv[k] = (1 << (kShift - 1)) + kCVG * vv + kCUG * uu;
        buv[k] = (1 << (kShift - 1)) + kCUB * uu;
    }

    const int odd = xx & 1;
    uint32_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = (k + odd) >> 1;                                   // sample of pixel xx + k, relative to cx
        const int l = (int)lum[k] - 16;
        const int y = (l < 0 ? 0 : l) * kCY;
        // (s is 0 .. 2; selected without indexing the arrays by a runtime value, which would put them in scratch memory)
        const int rr = s == 0 ? ruv[0] : (s == 1 ? ruv[1] : ruv[2]);
        const int gg = s == 0 ? guv[0] : (s == 1 ? guv[1] : guv[2]);
        const int bb = s == 0 ? buv[0] : (s == 1 ? buv[1] : buv[2]);
        b[3 * k] = sat8((y + bb) >> kShift);
        b[3 * k + 1] = sat8((y + gg) >> kShift);
        b[3 * k + 2] = sat8((y + rr) >> kShift);
    }

    uint8_t *dst = out + (((int64_t)f * Hr + r) * Wr + c) * 3;
    if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
        uint32_t *d32 = (uint32_t *)dst;
#pragma unroll
        for (int k = 0; k < 3; ++k) d32[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
    } else if (npx == 4 && ((uintptr_t)dst & 1) == 0) {
        uint16_t *d16 = (uint16_t *)dst;
#pragma unroll
        for (int k = 0; k < 6; ++k) d16[k] = (uint16_t)(b[2 * k] | (b[2 * k + 1] << 8));
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * npx) dst[k] = (uint8_t)b[k];
    }
}

void launch_yuv420_to_bgr(hipStream_t s, int layout, const uint8_t *y, const uint8_t *u, const uint8_t *v, int64_t y_fs, int64_t y_rs,
                          int64_t c_fs, int64_t c_rs, int x0, int y0, int F, int Hr, int Wr, uint8_t *out)
{
    const int groups = Hr * ((Wr + 3) >> 2);
    // grid.y is limited to 65535: split the frame range
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        const dim3 grid((groups + 255) / 256, fc);
        uint8_t *o = out + (int64_t)f0 * Hr * Wr * 3;
        if (layout == SWK_YUV_I420)
            hipLaunchKernelGGL(k_yuv420_to_bgr<SWK_YUV_I420>, grid, dim3(256), 0, s, y + (int64_t)f0 * y_fs, u + (int64_t)f0 * c_fs,
                               v + (int64_t)f0 * c_fs, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, o);
        else
            hipLaunchKernelGGL(k_yuv420_to_bgr<SWK_YUV_NV12>, grid, dim3(256), 0, s, y + (int64_t)f0 * y_fs, u + (int64_t)f0 * c_fs,
                               (const uint8_t *)nullptr, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, o);
        note_launch();
    }
}

}  // namespace swk
