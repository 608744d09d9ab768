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
//
// k_yuv_to_bgr further down is the same kernel for every other format (4:2:2, 4:4:4, 4:1:1, mono, 9 .. 16 bits, full range,
// interleaved chroma at any subsampling); k_yuv420_to_bgr stays the route of 8-bit 4:2:0 limited range.
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

// ---- every planar / semiplanar / mono format, 8 .. 16 bits, limited or full range (swk_yuv_to_bgr, include/swk.h) -----------------
// The same byte-streaming design with what changes the addressing and the unrolling as template parameters: BPS bytes per sample
// (1, 2), SX the horizontal chroma shift (0, 1, 2: a quad of pixels is covered by up to 4, 3, 2 chroma samples), SEMI interleaved
// (U, V) samples in one plane.  The vertical shift, the range's constants, k = bits - 8, the shift of MSB-aligned words and "mono"
// are wave-uniform arguments.  One-byte samples stay in int32 (full range: largest magnitude 5.1e8); two-byte samples use 64-bit
// multiply-adds, the kernel is bound by bytes.
struct YuvConv {
    int cy, cub, cug, cvg, cvr;          // 20-bit fixed point
    int yoff;                            // 16 << k (limited range) or 0
    int k;                               // bits - 8: the final shift is 20 + k
    int msb;                             // 16 - bits for MSB-aligned two-byte samples, else 0
    int sy;                              // vertical chroma shift
    int mono;                            // no chroma planes: U = V = 128 << k
};

namespace {

template <int BPS> struct YuvT;
template <> struct YuvT<1> { using sample = uint8_t; using pair = uint16_t; using acc = int; };
template <> struct YuvT<2> { using sample = uint16_t; using pair = uint32_t; using acc = int64_t; };

template <typename T> __device__ __forceinline__ void unpack_words(const uint32_t *w, int first, int count, uint32_t *e)
{
    // `count` samples of T out of consecutive dwords w[0 ..] into e[first ..] (constant indices after unrolling)
    constexpr int PER = 4 / (int)sizeof(T);
    constexpr uint32_t MASK = sizeof(T) == 1 ? 255u : 65535u;
#pragma unroll
    for (int i = 0; i < count; ++i) e[first + i] = (w[i / PER] >> (8 * (int)sizeof(T) * (i % PER))) & MASK;
}

// e[K0 .. N) from p[K0 .. n) two samples at a time where the pair's address allows one access, else sample by sample; `fill` past n
template <typename T, int N, int K0> __device__ __forceinline__ void load_pairs(const T *p, int n, uint32_t fill, uint32_t (&e)[N])
{
    using P = typename YuvT<sizeof(T)>::pair;
    // (the alignment is tested per pair although all pairs of a run share it: with one test around the whole run planar 4:2:0 at
    //  an odd origin took 1.14 x k_yuv420_to_bgr's time instead of 1.03 x, and 4:1:1 1.79 ms instead of 1.33 ms)
#pragma unroll
    for (int k = K0; k < N; k += 2) {
        if (k + 1 < N && k + 1 < n && ((uintptr_t)(p + k) & (2 * sizeof(T) - 1)) == 0) {
            const uint32_t w = *(const P *)(p + k);
            unpack_words<T>(&w, k, 2, e);
        } else {
            e[k] = k < n ? (uint32_t)p[k] : fill;
            if (k + 1 < N) e[k + 1] = k + 1 < n ? (uint32_t)p[k + 1] : fill;
        }
    }
}

// e[0 .. N) = p[0 .. n), `fill` past n, with the widest accesses the address allows; reads nothing past p[n - 1]
template <typename T, int N> __device__ __forceinline__ void load_run(const T *p, int n, uint32_t fill, uint32_t (&e)[N])
{
    constexpr int B = sizeof(T);
    if constexpr ((N * B) % 4 == 0) {
        if (n == N && ((uintptr_t)p & 3) == 0) {
            constexpr int D = N * B / 4;
            uint32_t w[D];
            bool done = false;
            if constexpr (D == 4) {
                if (((uintptr_t)p & 15) == 0) {
                    const uint4 q = *(const uint4 *)p;
                    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
                    done = true;
                }
            }
            if constexpr (D % 2 == 0) {
                if (!done && ((uintptr_t)p & 7) == 0) {
#pragma unroll
                    for (int i = 0; i < D / 2; ++i) {
                        const uint2 q = ((const uint2 *)p)[i];
                        w[2 * i] = q.x; w[2 * i + 1] = q.y;
                    }
                    done = true;
                }
            }
            if (!done) {
#pragma unroll
                for (int i = 0; i < D; ++i) w[i] = ((const uint32_t *)p)[i];
            }
            unpack_words<T>(w, 0, N, e);
            return;
        }
    }
    if constexpr (N > 4) {
        // a run of six samples (4:2:2 interleaved), or a longer one cut short by the rectangle's edge: four at once, then pairs
        if (n >= 4 && ((uintptr_t)p & (4 * B - 1)) == 0) {
            uint32_t w[2];
            if constexpr (B == 1) w[0] = *(const uint32_t *)p;
            else { const uint2 q = *(const uint2 *)p; w[0] = q.x; w[1] = q.y; }
            unpack_words<T>(w, 0, 4, e);
            load_pairs<T, N, 4>(p, n, fill, e);
            return;
        }
    }
    load_pairs<T, N, 0>(p, n, fill, e);
}

}  // namespace

template <int BPS, int SX, bool SEMI>
__global__ __launch_bounds__(256) void k_yuv_to_bgr(const uint8_t *__restrict__ yp, const uint8_t *__restrict__ up,
                                                    const uint8_t *__restrict__ vp, int64_t y_fs, int64_t y_rs, int64_t c_fs, int64_t c_rs,
                                                    int x0, int y0, int Hr, int Wr, YuvConv cv, uint8_t *__restrict__ out)
{
    using T = typename YuvT<BPS>::sample;
    using acc = typename YuvT<BPS>::acc;
    constexpr int NS = SX == 0 ? 4 : (SX == 1 ? 3 : 2);          // chroma samples that can cover four consecutive pixels
    const int f = blockIdx.y;
    const int wq = (Wr + 3) >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Hr * wq) return;
    const int r = idx / wq, c = (idx - r * wq) << 2;
    const int npx = Wr - c < 4 ? Wr - c : 4;
    const int yy = y0 + r, xx = x0 + c;
    const uint32_t mid = 128u << cv.k;

    // luma: pixels xx .. xx + npx - 1 of row yy
    uint32_t lum[4];
    load_run<T, 4>((const T *)(yp + (int64_t)f * y_fs + (int64_t)yy * y_rs) + xx, npx, 0u, lum);

    // chroma: samples cx .. cx + ns - 1 of chroma row yy >> sy cover the quad
    const int cx = xx >> SX;
    const int ns = ((xx + npx - 1) >> SX) - cx + 1;
    uint32_t cu[NS], cw[NS];
    if (cv.mono) {
#pragma unroll
        for (int k = 0; k < NS; ++k) cu[k] = cw[k] = mid;
    } else {
        const int64_t row = (int64_t)f * c_fs + (int64_t)(yy >> cv.sy) * c_rs;
        if (SEMI) {
            uint32_t uv[2 * NS];
            load_run<T, 2 * NS>((const T *)(up + row) + 2 * (int64_t)cx, 2 * ns, 0u, uv);
#pragma unroll
            for (int k = 0; k < NS; ++k) { cu[k] = uv[2 * k]; cw[k] = uv[2 * k + 1]; }
        } else {
            load_run<T, NS>((const T *)(up + row) + cx, ns, 0u, cu);
            load_run<T, NS>((const T *)(vp + row) + cx, ns, 0u, cw);
        }
    }
    if (BPS == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) lum[k] >>= cv.msb;
        if (!cv.mono) {
#pragma unroll
            for (int k = 0; k < NS; ++k) { cu[k] >>= cv.msb; cw[k] >>= cv.msb; }
        }
    }
    const acc h = (acc)1 << (kShift - 1 + cv.k);
    acc ruv[NS], guv[NS], buv[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const acc uu = (acc)cu[k] - (acc)mid, vv = (acc)cw[k] - (acc)mid;
        ruv[k] = h + (acc)cv.cvr * vv;
        guv[k] = h + (acc)cv.cvg * vv + (acc)cv.cug * uu;
        buv[k] = h + (acc)cv.cub * uu;
    }

    const int sh = kShift + cv.k;
    const int ph = xx & ((1 << SX) - 1);                                // the quad's phase inside its first chroma cell
    uint32_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = (k + ph) >> SX;                                   // sample of pixel xx + k, relative to cx (k itself at SX = 0)
        const acc l = (acc)lum[k] - (acc)cv.yoff;
        const acc y = (l < 0 ? 0 : l) * (acc)cv.cy;
        // (selected without indexing the arrays by a runtime value, which would put them in scratch memory)
        acc rr = ruv[0], gg = guv[0], bb = buv[0];
#pragma unroll
        for (int j = 1; j < NS; ++j)
            if (s == j) { rr = ruv[j]; gg = guv[j]; bb = buv[j]; }
        const acc vb = (y + bb) >> sh, vg = (y + gg) >> sh, vr = (y + rr) >> sh;
        b[3 * k] = (uint32_t)(vb < 0 ? 0 : (vb > 255 ? 255 : vb));
        b[3 * k + 1] = (uint32_t)(vg < 0 ? 0 : (vg > 255 ? 255 : vg));
        b[3 * k + 2] = (uint32_t)(vr < 0 ? 0 : (vr > 255 ? 255 : vr));
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

namespace {

template <int BPS, int SX, bool SEMI>
void launch_yuv_one(hipStream_t s, dim3 grid, const uint8_t *y, const uint8_t *u, const uint8_t *v, int64_t y_fs, int64_t y_rs, int64_t c_fs,
                    int64_t c_rs, int x0, int y0, int Hr, int Wr, const YuvConv &cv, uint8_t *out)
{
    hipLaunchKernelGGL((k_yuv_to_bgr<BPS, SX, SEMI>), grid, dim3(256), 0, s, y, u, v, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, out);
}

template <int BPS, bool SEMI>
void launch_yuv_sx(hipStream_t s, int sx, dim3 grid, const uint8_t *y, const uint8_t *u, const uint8_t *v, int64_t y_fs, int64_t y_rs,
                   int64_t c_fs, int64_t c_rs, int x0, int y0, int Hr, int Wr, const YuvConv &cv, uint8_t *out)
{
    if (sx == 0) launch_yuv_one<BPS, 0, SEMI>(s, grid, y, u, v, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, out);
    else if (sx == 1) launch_yuv_one<BPS, 1, SEMI>(s, grid, y, u, v, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, out);
    else launch_yuv_one<BPS, 2, SEMI>(s, grid, y, u, v, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, out);
}

}  // namespace

void launch_yuv_to_bgr(hipStream_t s, int layout, int sx, int sy, int bits, int msb_aligned, int full_range, const uint8_t *y,
                       const uint8_t *u, const uint8_t *v, int64_t y_fs, int64_t y_rs, int64_t c_fs, int64_t c_rs, int x0, int y0, int F,
                       int Hr, int Wr, uint8_t *out)
{
    const int k = bits - 8;
    const bool mono = layout == SWK_YUV_MONO, semi = layout == SWK_YUV_SEMIPLANAR, wide = bits > 8;
    YuvConv cv;
    if (full_range) cv = YuvConv{1048576, 1858077, -360853, -748826, 1470104, 0, k, 0, sy, mono};
    else cv = YuvConv{kCY, kCUB, kCUG, kCVG, kCVR, 16 << k, k, 0, sy, mono};
    cv.msb = wide && msb_aligned ? 16 - bits : 0;
    if (mono) { sx = 2; u = v = nullptr; c_fs = c_rs = 0; }          // (no chroma is read: the instantiation with the fewest samples)
    const int groups = Hr * ((Wr + 3) >> 2);
    // grid.y is limited to 65535: split the frame range
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        const dim3 grid((groups + 255) / 256, fc);
        uint8_t *o = out + (int64_t)f0 * Hr * Wr * 3;
        const uint8_t *yf = y + (int64_t)f0 * y_fs, *uf = u ? u + (int64_t)f0 * c_fs : nullptr, *vf = v && !semi ? v + (int64_t)f0 * c_fs : nullptr;
        if (!wide && !semi) launch_yuv_sx<1, false>(s, sx, grid, yf, uf, vf, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, o);
        else if (!wide) launch_yuv_sx<1, true>(s, sx, grid, yf, uf, vf, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, o);
        else if (!semi) launch_yuv_sx<2, false>(s, sx, grid, yf, uf, vf, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, o);
        else launch_yuv_sx<2, true>(s, sx, grid, yf, uf, vf, y_fs, y_rs, c_fs, c_rs, x0, y0, Hr, Wr, cv, o);
        note_launch();
    }
}

}  // namespace swk
