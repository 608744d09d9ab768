// Kernels that only swk_batch_run_groups uses: the gather of several groups' windows into one zero-padded X, and the
// scatter of the float64 factors back to each window's own (pixels, frames) layout.
//   crop + BGR2GRAY (image_filtering.py:199-203, 188-196) with the arithmetic of k_gray / k_gray4 (same Q14 / Q15 weights)
//   A / E in the reference's layout (image_filtering.py:235-237), as k_planes_to_pn, for a window's own pixel count
#include "swk_internal.h"

namespace swk {

// One thread per pixel of the padded plane: frame f = blockIdx.y (+ f0) is queue position j of window f / n.
__global__ __launch_bounds__(256) void k_gray_groups(const GroupWin *__restrict__ wins, int f0, int n, int mode, uint8_t *__restrict__ X)
{
    const int f = f0 + blockIdx.y;
    const int w = f / n, j = f - w * n;
    const GroupWin d = wins[w];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.pitch) return;
    uint8_t *out = X + d.off + (int64_t)j * d.pitch + p;
    if (p >= d.H * d.W) { *out = 0; return; }          // padding: zero pixel rows leave X^T X, ||X||_F and max|X| unchanged
    const int r = p / d.W, c = p - r * d.W;
    const uint8_t *src = d.src + (int64_t)j * d.fs + (int64_t)(d.y0 + r) * d.rs + (int64_t)(d.x0 + c) * d.channels;
    int y;
    if (d.channels == 1) {
        y = src[0];
    } else {
        const int bb = src[0], gg = src[1], rr = src[2];
        if (mode == SWK_GRAY_Q14) y = (bb * 1868 + gg * 9617 + rr * 4899 + (1 << 13)) >> 14;
        else y = (bb * 3735 + gg * 19235 + rr * 9798 + (1 << 14)) >> 15;
    }
    *out = (uint8_t)y;
}

void launch_gray_groups(hipStream_t s, const GroupWin *wins, int F, int n, int Pmax, int gray_mode, uint8_t *X)
{
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        hipLaunchKernelGGL(k_gray_groups, dim3((Pmax + 255) / 256, fc), dim3(256), 0, s, wins, f0, n, gray_mode, X);
    }
}

// planes [nwin][fpad][pstride] (padded pixel count) -> window w's [P_w][n] at wins[w].dst
__global__ void k_planes_to_pn_groups(const double *__restrict__ planes, const PnWin *__restrict__ wins, int n, int64_t ps, int fpad)
{
    const int w = blockIdx.y;
    const PnWin d = wins[w];
    const int64_t total = (int64_t)n * d.P;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!d.dst || i >= total) return;
    const int p = (int)(i / n), j = (int)(i % n);
    d.dst[i] = planes[(int64_t)w * fpad * ps + (int64_t)j * ps + p];
}

void launch_planes_to_pn_groups(hipStream_t s, const double *planes, const PnWin *wins, int nwin, int n, int Pmax, int64_t pstride,
                                int fpad)
{
    const int64_t total = (int64_t)n * Pmax;
    hipLaunchKernelGGL(k_planes_to_pn_groups, dim3((unsigned)((total + 255) / 256), nwin), dim3(256), 0, s, planes, wins, n, pstride, fpad);
}

}  // namespace swk
