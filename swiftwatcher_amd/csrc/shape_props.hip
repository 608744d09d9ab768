// Shape sums of the regions of u8 label planes (include/swk.h, swk_segment_shapes_u8): per label value 1..255 the ten
// coordinate power sums up to degree 3, the border pixel count, skimage's three perimeter classes and the three bit-quad
// counts of the 8-connected Euler number.  Everything is an integer sum, so the records do not depend on scheduling: bit-exact.
//
// Workgroup = one tile of kShapeRows x kShapeCols pixels of one frame, held in LDS with a halo (zero outside the plane):
//   * the power sums are accumulated per horizontal run of one value inside the tile, from closed-form power sums of the run's
//     columns (sum c^3 up to c = 32767 is below 2^58): one set of 64-bit LDS atomics per run, not per pixel;
//   * a pixel is a border pixel when one of its four edge neighbours has another value; its perimeter class needs the border
//     flag of its eight neighbours, which depends on THEIR four neighbours: a 5x5 footprint, two halo rows and columns.  The
//     flags of the tile plus one ring are made first, in a second LDS plane;
//   * every 2x2 window of the zero-padded plane belongs to its top-left pixel; the windows that start in row / column -1
//     belong to the pixels of row / column 0.  A window counts once for every value in it, on that value's own mask.
// A 256-entry table of 17 sums in LDS (34 KB), then one 64-bit global atomic per non-zero sum and value; a compaction kernel
// writes the records in ascending label order (as k_props_compact does for swk_segment).
#include "swk_internal.h"

namespace swk {

constexpr int kShapeRows = 16, kShapeCols = 256, kShapeThreads = 256;
constexpr int kShapePadL = 4;                                   // LDS column 0 = plane column c0 - 4: words stay aligned
constexpr int kShapePitch = kShapeCols + 2 * kShapePadL;        // 264
constexpr int kShapeTileRows = kShapeRows + 4;                  // two halo rows on each side
constexpr int kShapeSums = 17;                                  // m[10], border, perim[3], quads[3]
enum { SH_BORDER = 10, SH_PERIM = 11, SH_QUADS = 14 };

typedef unsigned long long u64;

// sum of k, k^2, k^3 over k = 0..x (x >= -1)
__device__ __forceinline__ u64 pow1(int64_t x) { return (u64)(x * (x + 1) / 2); }
__device__ __forceinline__ u64 pow2(int64_t x) { return (u64)(x * (x + 1) * (2 * x + 1) / 6); }
__device__ __forceinline__ u64 pow3(int64_t x) { const u64 s = pow1(x); return s * s; }

// one 2x2 window (a b / c d): every value in it counts on its own mask
__device__ __forceinline__ void count_quad(u64 (*tab)[256], int a, int b, int c, int d)
{
    if (a == b && b == c && c == d) return;
    const int v[4] = {a, b, c, d};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = v[i];
        if (!x) continue;
        bool first = true;
#pragma unroll
        for (int j = 0; j < i; ++j) first = first && v[j] != x;
        if (!first) continue;
        const int n = (a == x) + (b == x) + (c == x) + (d == x);
        if (n == 1) atomicAdd(&tab[SH_QUADS][x], 1ull);
        else if (n == 3) atomicAdd(&tab[SH_QUADS + 1][x], 1ull);
        else if (n == 2 && ((a == x && d == x) || (b == x && c == x))) atomicAdd(&tab[SH_QUADS + 2][x], 1ull);
    }
}

// lab: frame f, pixel (r, c) at lab + f * fs + r * rs + c.  VEC: every row start and c0 - 4 are multiples of VEC bytes.
template <int VEC>
__global__ __launch_bounds__(kShapeThreads) void k_shape_sums(const uint8_t *__restrict__ lab, int H, int W, int64_t fs, int64_t rs,
                                                              u64 *__restrict__ gtab)
{
    __shared__ u64 s_tab[kShapeSums][256];
    __shared__ __attribute__((aligned(4))) uint8_t s_px[kShapeTileRows][kShapePitch];
    __shared__ uint8_t s_bd[kShapeTileRows][kShapePitch];
    const int t = threadIdx.x, f = blockIdx.z;
    const int r0 = blockIdx.y * kShapeRows, c0 = blockIdx.x * kShapeCols;
    const uint8_t *img = lab + (int64_t)f * fs;
    for (int k = 0; k < kShapeSums; ++k) s_tab[k][t] = 0;
    // ---- the tile and its halo: rows r0 - 2 .. r0 + kShapeRows + 1, columns c0 - 4 .. c0 + kShapeCols + 3 ----
    constexpr int kWordsRow = kShapePitch / VEC;
    for (int i = t; i < kShapeTileRows * kWordsRow; i += kShapeThreads) {
        const int lr = i / kWordsRow, lw = i - lr * kWordsRow;
        const int r = r0 - 2 + lr, c = c0 - kShapePadL + lw * VEC;
        uint32_t word = 0;
        if (r >= 0 && r < H && c + VEC > 0 && c < W) {
            const uint8_t *row = img + (int64_t)r * rs;
            if (c >= 0 && c + VEC <= W) {
                if (VEC == 4) word = *(const uint32_t *)(row + c);
                else if (VEC == 2) word = *(const uint16_t *)(row + c);
                else word = row[c];
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    if (c + k >= 0 && c + k < W) word |= (uint32_t)row[c + k] << (8 * k);
            }
        }
        if (VEC == 4) *(uint32_t *)&s_px[lr][lw * 4] = word;
        else if (VEC == 2) *(uint16_t *)&s_px[lr][lw * 2] = (uint16_t)word;
        else s_px[lr][lw] = (uint8_t)word;
    }
    __syncthreads();
    // ---- border flags of the tile plus one ring (a pixel outside the plane is 0 and never a border pixel) ----
    constexpr int kRingCols = kShapeCols + 2;
    for (int i = t; i < (kShapeRows + 2) * kRingCols; i += kShapeThreads) {
        const int lr = 1 + i / kRingCols, lc = kShapePadL - 1 + i % kRingCols;
        const int v = s_px[lr][lc];
        s_bd[lr][lc] = v && (s_px[lr - 1][lc] != v || s_px[lr + 1][lc] != v || s_px[lr][lc - 1] != v || s_px[lr][lc + 1] != v);
    }
    __syncthreads();
    const int nr = H - r0 < kShapeRows ? H - r0 : kShapeRows;            // the tile's own pixels
    const int nc = W - c0 < kShapeCols ? W - c0 : kShapeCols;
    for (int i = t; i < nr * kShapeCols; i += kShapeThreads) {
        const int pr = i / kShapeCols, pc = i % kShapeCols;
        if (pc >= nc) continue;
        const int lr = pr + 2, lc = pc + kShapePadL;
        const int v = s_px[lr][lc];
        const int r = r0 + pr, c = c0 + pc;
        // ---- bit quads ----
        const int e = s_px[lr][lc + 1], s = s_px[lr + 1][lc], se = s_px[lr + 1][lc + 1];
        count_quad(s_tab, v, e, s, se);
        if (r == 0) count_quad(s_tab, 0, 0, v, e);
        if (c == 0) count_quad(s_tab, 0, v, 0, s);
        if (r == 0 && c == 0) count_quad(s_tab, 0, 0, 0, v);
        if (!v) continue;
        // ---- power sums: the run that starts here ----
        if (pc == 0 || s_px[lr][lc - 1] != v) {
            int pe = pc;
            while (pe + 1 < nc && s_px[lr][lc + (pe + 1 - pc)] == v) ++pe;
            const int64_t cs = c, ce = c0 + pe;
            const u64 n = (u64)(ce - cs + 1), rr = (u64)r;
            const u64 s1 = pow1(ce) - pow1(cs - 1), s2 = pow2(ce) - pow2(cs - 1), s3 = pow3(ce) - pow3(cs - 1);
            atomicAdd(&s_tab[0][v], n);
            atomicAdd(&s_tab[1][v], rr * n);
            atomicAdd(&s_tab[2][v], s1);
            atomicAdd(&s_tab[3][v], rr * rr * n);
            atomicAdd(&s_tab[4][v], rr * s1);
            atomicAdd(&s_tab[5][v], s2);
            atomicAdd(&s_tab[6][v], rr * rr * rr * n);
            atomicAdd(&s_tab[7][v], rr * rr * s1);
            atomicAdd(&s_tab[8][v], rr * s2);
            atomicAdd(&s_tab[9][v], s3);
        }
        // ---- border pixel and its perimeter class (code = 1 + 2 a + 10 b) ----
        if (s_bd[lr][lc]) {
            auto bd = [&](int dr, int dc) -> int { return s_bd[lr + dr][lc + dc] && s_px[lr + dr][lc + dc] == v; };
            const int a = bd(-1, 0) + bd(1, 0) + bd(0, -1) + bd(0, 1);
            const int b = bd(-1, -1) + bd(-1, 1) + bd(1, -1) + bd(1, 1);
            const int code = 1 + 2 * a + 10 * b;
            atomicAdd(&s_tab[SH_BORDER][v], 1ull);
            if (code == 5 || code == 7 || code == 15 || code == 17 || code == 25 || code == 27) atomicAdd(&s_tab[SH_PERIM][v], 1ull);
            else if (code == 21 || code == 33) atomicAdd(&s_tab[SH_PERIM + 1][v], 1ull);
            else if (code == 13 || code == 23) atomicAdd(&s_tab[SH_PERIM + 2][v], 1ull);
        }
    }
    __syncthreads();
    if (t > 0) {
        u64 *g = gtab + ((int64_t)f * 256 + t) * kShapeSums;
        for (int k = 0; k < kShapeSums; ++k) {
            const u64 x = s_tab[k][t];
            if (x) atomicAdd(&g[k], x);
        }
    }
}

// compact the 255 table rows of a frame into its ascending-label record list (slots past the count stay as they were: zero)
__global__ __launch_bounds__(256) void k_shape_compact(const u64 *__restrict__ gtab, int seg_cap, swk_segment_shape *__restrict__ shapes,
                                                       int32_t *__restrict__ nseg)
{
    __shared__ int s_wave[4];
    const int f = blockIdx.x, t = threadIdx.x;
    const u64 *g = gtab + ((int64_t)f * 256 + t) * kShapeSums;
    const bool live = t > 0 && g[0] > 0;
    const unsigned long long mask = __ballot(live);
    const int lane = t & 63, wv = t >> 6;
    if (lane == 0) s_wave[wv] = __popcll(mask);
    __syncthreads();
    int base = 0;
    for (int i = 0; i < wv; ++i) base += s_wave[i];
    const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (live && pos < seg_cap) {
        swk_segment_shape sh;
        sh.label = t; sh.reserved_ = 0;
        for (int k = 0; k < 10; ++k) sh.m[k] = (int64_t)g[k];
        sh.border = (int64_t)g[SH_BORDER];
        for (int k = 0; k < 3; ++k) { sh.perim[k] = (int64_t)g[SH_PERIM + k]; sh.quads[k] = (int64_t)g[SH_QUADS + k]; }
        shapes[(int64_t)f * seg_cap + pos] = sh;
    }
    if (t == 0) nseg[f] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

size_t shape_table_bytes(int F) { return (size_t)F * 256 * kShapeSums * sizeof(u64); }

void launch_segment_shapes(hipStream_t s, const uint8_t *labels, int F, int H, int W, int64_t fs, int64_t rs, void *table, int seg_cap,
                           swk_segment_shape *shapes, int32_t *nseg)
{
    u64 *gtab = (u64 *)table;
    hipError_t me = hipMemsetAsync(gtab, 0, shape_table_bytes(F), s);
    if (me == hipSuccess) me = hipMemsetAsync(shapes, 0, (size_t)F * seg_cap * sizeof(swk_segment_shape), s);
    if (me != hipSuccess) { g_launch_error = (int)me; return; }          // surfaces at the context's next sync()
    const uintptr_t align = (uintptr_t)labels | (uintptr_t)(fs < 0 ? -fs : fs) | (uintptr_t)rs;
    const int vec = align % 4 == 0 ? 4 : align % 2 == 0 ? 2 : 1;
    const dim3 blk(kShapeThreads);
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        const dim3 grid((W + kShapeCols - 1) / kShapeCols, (H + kShapeRows - 1) / kShapeRows, fc);
        const uint8_t *lp = labels + (int64_t)f0 * fs;
        u64 *gp = gtab + (int64_t)f0 * 256 * kShapeSums;
        if (vec == 4) hipLaunchKernelGGL(k_shape_sums<4>, grid, blk, 0, s, lp, H, W, fs, rs, gp);
        else if (vec == 2) hipLaunchKernelGGL(k_shape_sums<2>, grid, blk, 0, s, lp, H, W, fs, rs, gp);
        else hipLaunchKernelGGL(k_shape_sums<1>, grid, blk, 0, s, lp, H, W, fs, rs, gp);
        note_launch();
    }
    hipLaunchKernelGGL(k_shape_compact, dim3(F), dim3(256), 0, s, gtab, seg_cap, shapes, nseg);
    note_launch();
}

}  // namespace swk
