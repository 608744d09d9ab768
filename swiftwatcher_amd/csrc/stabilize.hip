// Per-frame integer shift search against an anchor image (include/swk.h, swk_stabilize_u8): for every candidate shift (dy, dx),
// |dy|, |dx| <= S, whose rectangle lies inside the source frame, the sum of absolute differences between the anchor and the grey
// of the frame's rectangle at that shift; the smallest score wins (ties: smallest dy^2 + dx^2, then dy, then dx), and the chosen
// BGR rectangle is copied out.  Every sum is an integer, so the table does not depend on scheduling: bit-exact.
//
//   k_stab_gray    BGR -> grey of the whole source frame into a scratch plane whose rows are padded to 4 bytes (pad bytes 0), with
//                  the arithmetic of k_gray (filters.hip) bit for bit; a frame with any non-zero byte sets its flag (a frame
//                  without one is a null frame of the reader and is not matched).
//   k_stab_sad     workgroup = (frame, tile of kStabRows anchor rows x kStabCols columns).  The anchor tile and the grey tile with
//                  its S-pixel halo sit in LDS as dwords.  A thread owns one candidate (looping where (2S + 1)^2 > 256) and walks
//                  the tile in dwords: the anchor dword is an LDS broadcast (every lane reads one address), the shifted grey dword
//                  is v_alignbyte of two neighbouring dwords, of which one is carried over from the previous step -- all four byte
//                  alignments of x0 + dx are one code path -- and v_sad_u8 accumulates four pixels per instruction into a 32-bit
//                  register (255 * 16 * 256 < 2^21).  One 64-bit atomic add per candidate and workgroup.
//                  LDS: 16 x 256 B anchor + 48 rows x 77 dwords grey = 18.9 KB, eight workgroups per CU; a grey row pitch of 77 dwords
//                  (13 mod 32) puts the three or four rows the 32 lanes of a ds_read_b32 group touch on disjoint banks.
//   k_stab_pick    one workgroup per frame: the minimum by the rule above, the record, UINT64_MAX into the excluded table entries.
//   k_stab_copy    the chosen rectangle's BGR bytes, four per thread.
//
// The quarter-pixel stage (swk_stabilize_subpel_u8) runs after k_stab_gray, k_stab_sad and k_stab_pick, which it leaves as they are:
// the 25 total shifts (4 dy + qy, 4 dx + qx), qy, qx = -2..2, around stage 1's winner, each scored by the summed absolute difference
// between the anchor and the grey plane resampled with the 4-tap Catmull-Rom filter in units of 1/128 (one rounding, exact integers).
//   k_stab_sub_sad   workgroup = (frame, tile of kSubRows anchor rows x kSubCols columns); it reads its frame's stage-1 record.  The
//                    anchor tile and the grey tile at the winner's offset with a halo of 2 pixels on every side sit in LDS (floor(Q / 4)
//                    is d - 1 or d and the taps are -1..+2: rows and columns d - 2 .. d + 2 of a pixel).  A thread owns one column and
//                    kSubRowsPerThread rows of it and keeps the 25 sums in registers: walking down, it filters one new grey row
//                    horizontally for the five qx (five bytes, 16 multiply-adds without the zero taps) into a window of five such rows
//                    that lives in registers, and combines the window vertically for the five qy (25 x 4 multiply-adds), so a row
//                    is filtered once for the five vertical offsets it serves.  q = -2, -1 read rows d - 2 .. d + 1 at phases 2, 3,
//                    q = 0, 1, 2 rows d - 1 .. d + 2 at phases 0, 1, 2: one 5 x 5 weight matrix, constant after unrolling.  Pixels
//                    outside the anchor are skipped by predicate and the tile's grey outside the plane is staged as zero (only taps of
//                    weight zero or of excluded candidates meet it).  Sums: DPP/shuffle within a wave, LDS across the four waves, then one
//                    64-bit atomic add per admissible candidate and workgroup.
//                    LDS: 32 x 64 B anchor + 36 rows x 19 dwords grey + 25 sums = 4.9 KB (4,884 B); 125 VGPRs as compiled (25 sums,
//                    25 window values, the grey bytes and filtered values of the unrolled steps in flight): 4 waves per SIMD by
//                    registers, so 4 workgroups of 4 waves per CU, registers and not LDS (32 workgroups' worth) being the limit.
//   k_stab_sub_pick  one wave per frame: UINT64_MAX into the excluded entries, the minimum by (score, Qy^2 + Qx^2, Qy, Qx), the record;
//                    a null frame keeps Q = (0, 0).
//   k_stab_resample  in k_stab_copy's place: four output bytes per thread, every byte the 16-tap sum of its channel at the chosen
//                    phases (taps of weight zero are not read, so a phase-0 axis touches no pixel outside the rectangle); at phase
//                    (0, 0), which includes every null frame, it is k_stab_copy's copy.
#include "swk_internal.h"

namespace swk {

constexpr int kStabRows = 16, kStabCols = 256, kStabThreads = 256;
constexpr int kStabMaxS = 16;
constexpr int kStabAnchorDw = kStabCols / 4;                          // 64
constexpr int kStabGreyRows = kStabRows + 2 * kStabMaxS;              // 48
constexpr int kStabGreyDw = 77;                                       // >= 64 + (2 S + 3) / 4 + 1 = 73
static_assert(kStabGreyDw >= kStabAnchorDw + (2 * kStabMaxS + 3) / 4 + 1, "grey tile too narrow");

typedef unsigned long long u64;

// frames: frame f, pixel (r, c) at frames + f * fs + r * rs + 3 c.  plane: [F][Hs][pitch], pitch a multiple of 4.
__global__ __launch_bounds__(256) void k_stab_gray(const uint8_t *__restrict__ frames, int64_t fs, int64_t rs, int Hs, int Ws, int pitch,
                                                   int mode, uint8_t *__restrict__ plane, uint32_t *__restrict__ nonzero)
{
    const int f = blockIdx.y;
    const int wq = pitch >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t any = 0;
    if (idx < Hs * wq) {
        const int r = idx / wq, c = (idx - r * wq) << 2;
        const int npx = Ws - c < 4 ? Ws - c : 4;                      // 1..4: pitch - Ws < 4
        const uint8_t *src = frames + (int64_t)f * fs + (int64_t)r * rs + (int64_t)c * 3;
        uint32_t b[12];
        if (npx == 4 && ((uintptr_t)src & 3) == 0) {
            const uint32_t *s32 = (const uint32_t *)src;
            const uint32_t w0 = s32[0], w1 = s32[1], w2 = s32[2];
#pragma unroll
            for (int k = 0; k < 4; ++k) { b[k] = (w0 >> (8 * k)) & 255u; b[4 + k] = (w1 >> (8 * k)) & 255u; b[8 + k] = (w2 >> (8 * k)) & 255u; }
            any = w0 | w1 | w2;
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) { b[k] = k < 3 * npx ? src[k] : 0u; any |= b[k]; }
        }
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t y = mode == SWK_GRAY_Q14 ? (b[3 * k] * 1868u + b[3 * k + 1] * 9617u + b[3 * k + 2] * 4899u + (1u << 13)) >> 14
                                                    : (b[3 * k] * 3735u + b[3 * k + 1] * 19235u + b[3 * k + 2] * 9798u + (1u << 14)) >> 15;
            if (k < npx) packed |= y << (8 * k);
        }
        *(uint32_t *)(plane + ((int64_t)f * Hs + r) * pitch + c) = packed;
    }
    if (__any(any != 0) && (threadIdx.x & 63) == 0) atomicOr(&nonzero[f], 1u);
}

// anchor: dense [Ho][Wo]; plane as k_stab_gray wrote it; table [F][(2 S + 1)^2], zero before the launch
__global__ __launch_bounds__(kStabThreads) void k_stab_sad(const uint8_t *__restrict__ anchor, const uint8_t *__restrict__ plane, int Hs,
                                                           int Ws, int pitch, int y0, int x0, int Ho, int Wo, int S,
                                                           u64 *__restrict__ table)
{
    __shared__ uint32_t s_a[kStabRows][kStabAnchorDw];
    __shared__ uint32_t s_g[kStabGreyRows][kStabGreyDw];
    const int t = threadIdx.x, f = blockIdx.z;
    const int r0 = blockIdx.y * kStabRows, c0 = blockIdx.x * kStabCols;
    const int nr = Ho - r0 < kStabRows ? Ho - r0 : kStabRows;         // the tile's own anchor pixels
    const int nc = Wo - c0 < kStabCols ? Wo - c0 : kStabCols;
    // ---- anchor tile: bytes outside the anchor are zero (and masked below) ----
    for (int i = t; i < kStabRows * kStabAnchorDw; i += kStabThreads) {
        const int lr = i / kStabAnchorDw, lw = i - lr * kStabAnchorDw;
        uint32_t word = 0;
        if (lr < nr) {
            const uint8_t *row = anchor + (int64_t)(r0 + lr) * Wo + c0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * lw + k < nc) word |= (uint32_t)row[4 * lw + k] << (8 * k);
        }
        s_a[lr][lw] = word;
    }
    // ---- grey tile with its halo: LDS row lr = plane row y0 + r0 - S + lr, LDS dword lw = plane bytes cb + 4 lw .. + 3 ----
    const int cb = (x0 + c0 - S) & ~3;                                // (floor to a multiple of 4, also below zero)
    const int grows = nr + 2 * S;
    const uint8_t *img = plane + (int64_t)f * Hs * pitch;
    for (int i = t; i < grows * kStabGreyDw; i += kStabThreads) {
        const int lr = i / kStabGreyDw, lw = i - lr * kStabGreyDw;
        const int gy = y0 + r0 - S + lr, gx = cb + 4 * lw;
        uint32_t word = 0;
        if (gy >= 0 && gy < Hs && gx >= 0 && gx + 4 <= pitch) word = *(const uint32_t *)(img + (int64_t)gy * pitch + gx);
        s_g[lr][lw] = word;
    }
    __syncthreads();
    const int side = 2 * S + 1, ncand = side * side;
    const int nwf = nc >> 2;                                          // full dwords of an anchor row
    const uint32_t tail = (nc & 3) ? (1u << (8 * (nc & 3))) - 1u : 0u;
    for (int cand = t; cand < ncand; cand += kStabThreads) {
        const int dy = cand / side - S, dx = cand - (dy + S) * side - S;
        if (y0 + dy < 0 || y0 + dy + Ho > Hs || x0 + dx < 0 || x0 + dx + Wo > Ws) continue;          // excluded: k_stab_pick marks it
        const int o = x0 + c0 + dx - cb;                              // 0 .. 2 S + 3: byte offset of the shifted tile in an LDS row
        const int d0 = o >> 2;
        const uint32_t sh = (uint32_t)(o & 3);
        uint32_t acc = 0;
        for (int r = 0; r < nr; ++r) {
            const uint32_t *g = &s_g[r + dy + S][d0];
            const uint32_t *a = s_a[r];
            uint32_t lo = g[0];
            for (int w = 0; w < nwf; ++w) {
                const uint32_t hi = g[w + 1];
                acc = __builtin_amdgcn_sad_u8(a[w], __builtin_amdgcn_alignbyte(hi, lo, sh), acc);
                lo = hi;
            }
            if (tail) acc = __builtin_amdgcn_sad_u8(a[nwf], __builtin_amdgcn_alignbyte(g[nwf + 1], lo, sh) & tail, acc);
        }
        atomicAdd(&table[(int64_t)f * ncand + cand], (u64)acc);
    }
}

// smaller (score, dy^2 + dx^2, dy, dx)
struct StabKey { u64 sad; int norm, dy, dx; };
__device__ __forceinline__ bool stab_less(const StabKey &a, const StabKey &b)
{
    if (a.sad != b.sad) return a.sad < b.sad;
    if (a.norm != b.norm) return a.norm < b.norm;
    if (a.dy != b.dy) return a.dy < b.dy;
    return a.dx < b.dx;
}

__global__ __launch_bounds__(256) void k_stab_pick(u64 *__restrict__ table, const uint32_t *__restrict__ nonzero, int Hs, int Ws, int y0,
                                                   int x0, int Ho, int Wo, int S, swk_shift *__restrict__ shifts)
{
    __shared__ StabKey s_key[256];
    const int f = blockIdx.x, t = threadIdx.x;
    const int side = 2 * S + 1, ncand = side * side;
    u64 *tab = table + (int64_t)f * ncand;
    StabKey best{~0ull, 0x7fffffff, 0, 0};
    for (int cand = t; cand < ncand; cand += 256) {
        const int dy = cand / side - S, dx = cand - (dy + S) * side - S;
        if (y0 + dy < 0 || y0 + dy + Ho > Hs || x0 + dx < 0 || x0 + dx + Wo > Ws) { tab[cand] = ~0ull; continue; }
        const StabKey k{tab[cand], dy * dy + dx * dx, dy, dx};
        if (stab_less(k, best)) best = k;
    }
    s_key[t] = best;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (t < half && stab_less(s_key[t + half], s_key[t])) s_key[t] = s_key[t + half];
        __syncthreads();
    }
    if (t == 0) {
        const u64 unshifted = tab[S * side + S];                      // (0, 0) is always a candidate
        swk_shift sh;
        if (nonzero[f]) { sh.dy = s_key[0].dy; sh.dx = s_key[0].dx; sh.sad = s_key[0].sad; }
        else { sh.dy = 0; sh.dx = 0; sh.sad = unshifted; }            // a null frame is not matched
        sh.sad_unshifted = unshifted;
        shifts[f] = sh;
    }
}

// out [F][Ho][Wo][3] dense; four bytes of a row per thread
__global__ __launch_bounds__(256) void k_stab_copy(const uint8_t *__restrict__ frames, int64_t fs, int64_t rs, int y0, int x0, int Ho, int Wo,
                                                   const swk_shift *__restrict__ shifts, uint8_t *__restrict__ out)
{
    const int f = blockIdx.y;
    const int rowb = Wo * 3, wq = (rowb + 3) >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Ho * wq) return;
    const int r = idx / wq, c = (idx - r * wq) << 2;
    const int nb = rowb - c < 4 ? rowb - c : 4;
    const uint8_t *src = frames + (int64_t)f * fs + (int64_t)(y0 + shifts[f].dy + r) * rs + (int64_t)(x0 + shifts[f].dx) * 3 + c;
    uint8_t *dst = out + ((int64_t)f * Ho + r) * rowb + c;
    uint32_t word = 0;
    for (int k = 0; k < nb; ++k) word |= (uint32_t)src[k] << (8 * k);
    if (nb == 4 && ((uintptr_t)dst & 3) == 0) *(uint32_t *)dst = word;
    else for (int k = 0; k < nb; ++k) dst[k] = (uint8_t)(word >> (8 * k));
}

int stabilize_pitch(int Ws) { return (Ws + 3) & ~3; }
size_t stabilize_plane_bytes(int F, int Hs, int Ws) { return (size_t)F * Hs * stabilize_pitch(Ws); }
size_t stabilize_table_bytes(int F, int S) { return (size_t)F * (2 * S + 1) * (2 * S + 1) * sizeof(u64); }

void launch_stabilize(hipStream_t s, const uint8_t *frames, int64_t fs, int64_t rs, int F, int Hs, int Ws, int y0, int x0, int Ho, int Wo,
                      int S, const uint8_t *anchor, int gray_mode, uint8_t *plane, uint32_t *nonzero, void *table, swk_shift *shifts,
                      uint8_t *out)
{
    u64 *tab = (u64 *)table;
    const int pitch = stabilize_pitch(Ws), ncand = (2 * S + 1) * (2 * S + 1);
    hipError_t me = hipMemsetAsync(tab, 0, stabilize_table_bytes(F, S), s);
    if (me == hipSuccess) me = hipMemsetAsync(nonzero, 0, (size_t)F * 4, s);
    if (me != hipSuccess) { g_launch_error = (int)me; return; }          // surfaces at the context's next sync()
    const int gq = Hs * (pitch >> 2), cq = Ho * ((Wo * 3 + 3) >> 2);
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        const uint8_t *fp = frames + (int64_t)f0 * fs;
        uint8_t *pp = plane + (int64_t)f0 * Hs * pitch;
        hipLaunchKernelGGL(k_stab_gray, dim3((gq + 255) / 256, fc), dim3(256), 0, s, fp, fs, rs, Hs, Ws, pitch, gray_mode, pp, nonzero + f0);
        note_launch();
        const dim3 grid((Wo + kStabCols - 1) / kStabCols, (Ho + kStabRows - 1) / kStabRows, fc);
        hipLaunchKernelGGL(k_stab_sad, grid, dim3(kStabThreads), 0, s, anchor, pp, Hs, Ws, pitch, y0, x0, Ho, Wo, S, tab + (int64_t)f0 * ncand);
        note_launch();
        hipLaunchKernelGGL(k_stab_pick, dim3(fc), dim3(256), 0, s, tab + (int64_t)f0 * ncand, nonzero + f0, Hs, Ws, y0, x0, Ho, Wo, S,
                           shifts + f0);
        note_launch();
        hipLaunchKernelGGL(k_stab_copy, dim3((cq + 255) / 256, fc), dim3(256), 0, s, fp, fs, rs, y0, x0, Ho, Wo, shifts + f0,
                           out + (int64_t)f0 * Ho * Wo * 3);
        note_launch();
    }
}

// ---- the quarter-pixel stage ------------------------------------------------------------------------------------------------------
constexpr int kSubRows = 32, kSubCols = 64, kSubThreads = 256;
constexpr int kSubRowsPerThread = kSubRows / (kSubThreads / kSubCols);          // 8
constexpr int kSubHalo = 2;
constexpr int kSubGreyRows = kSubRows + 2 * kSubHalo;                            // 36
constexpr int kSubGreyDw = 19;                                                   // 3 bytes of alignment + 64 + 4 of halo = 71 bytes
static_assert(kSubGreyDw * 4 >= 3 + kSubCols + 2 * kSubHalo, "grey tile too narrow");
static_assert(kSubCols == 64 && kSubThreads == 4 * kSubCols, "a wave takes a band of rows, a lane a column");

// Catmull-Rom at phase p / 4, units of 1/128
__device__ __constant__ int kSubTap[4][4] = {{0, 128, 0, 0}, {-9, 111, 29, -3}, {-8, 72, 72, -8}, {-3, 29, 111, -9}};

// The weight of sample d - 2 + w (w = 0..4) for the candidate q = j - 2: q < 0 is phase q + 4 at floor(Q / 4) = d - 1 (samples
// d - 2 .. d + 1), q >= 0 phase q at d (samples d - 1 .. d + 2).
__device__ __forceinline__ constexpr int sub_weight(int j, int w)
{
    constexpr int T[4][4] = {{0, 128, 0, 0}, {-9, 111, 29, -3}, {-8, 72, 72, -8}, {-3, 29, 111, -9}};
    const int q = j - 2, p = q < 0 ? q + 4 : q, k = q < 0 ? w : w - 1;
    return k < 0 || k > 3 ? 0 : T[p][k];
}

// one axis of a candidate's admissibility: o = y0 or x0, size = Ho or Wo, lim = Hs or Ws, Q the total shift in quarter pixels
__device__ __forceinline__ bool sub_axis_inside(int o, int size, int lim, int Q)
{
    const int i = Q >> 2;                                                         // floor
    return (Q & 3) ? (o + i - 1 >= 0 && o + i + size + 2 <= lim) : (o + i >= 0 && o + i + size <= lim);
}

// sub [F][25], zero before the launch; shifts: stage 1's records
__global__ __launch_bounds__(kSubThreads) void k_stab_sub_sad(const uint8_t *__restrict__ anchor, const uint8_t *__restrict__ plane, int Hs,
                                                              int Ws, int pitch, int y0, int x0, int Ho, int Wo,
                                                              const swk_shift *__restrict__ shifts, u64 *__restrict__ sub)
{
    __shared__ uint32_t s_a[kSubRows][kSubCols / 4];
    __shared__ uint32_t s_g[kSubGreyRows][kSubGreyDw];
    __shared__ uint32_t s_sum[25];
    const int t = threadIdx.x, f = blockIdx.z;
    const int r0 = blockIdx.y * kSubRows, c0 = blockIdx.x * kSubCols;
    const int nr = Ho - r0 < kSubRows ? Ho - r0 : kSubRows;
    const int nc = Wo - c0 < kSubCols ? Wo - c0 : kSubCols;
    const int dy = shifts[f].dy, dx = shifts[f].dx;
    if (t < 25) s_sum[t] = 0;
    // ---- anchor tile: bytes outside the anchor are zero (and skipped below) ----
    for (int i = t; i < kSubRows * (kSubCols / 4); i += kSubThreads) {
        const int lr = i / (kSubCols / 4), lw = i - lr * (kSubCols / 4);
        uint32_t word = 0;
        if (lr < nr) {
            const uint8_t *row = anchor + (int64_t)(r0 + lr) * Wo + c0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * lw + k < nc) word |= (uint32_t)row[4 * lw + k] << (8 * k);
        }
        s_a[lr][lw] = word;
    }
    // ---- grey tile with its halo: LDS row lr = plane row y0 + dy + r0 - 2 + lr, LDS dword lw = plane bytes cb + 4 lw .. + 3 ----
    const int gx0 = x0 + dx + c0 - kSubHalo, gy0 = y0 + dy + r0 - kSubHalo;
    const int cb = gx0 & ~3, off = gx0 - cb;                          // (floor to a multiple of 4, also below zero)
    const uint8_t *img = plane + (int64_t)f * Hs * pitch;
    for (int i = t; i < kSubGreyRows * kSubGreyDw; i += kSubThreads) {
        const int lr = i / kSubGreyDw, lw = i - lr * kSubGreyDw;
        const int gy = gy0 + lr, gx = cb + 4 * lw;
        uint32_t word = 0;
        if (lr < nr + 2 * kSubHalo && gy >= 0 && gy < Hs && gx >= 0 && gx + 4 <= pitch) word = *(const uint32_t *)(img + (int64_t)gy * pitch + gx);
        s_g[lr][lw] = word;
    }
    __syncthreads();
    const int tc = t & (kSubCols - 1), rb = (t / kSubCols) * kSubRowsPerThread;
    uint32_t acc[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) acc[k] = 0;
    if (rb < nr) {                                                    // (wave-uniform)
        const uint8_t *gcol = (const uint8_t *)&s_g[0][0] + off + tc;
        const uint8_t *acol = (const uint8_t *)&s_a[0][0] + tc;
        int win[5][5];                                                // win[w][jx]: the filtered row d - 2 + w of the current pixel
#pragma unroll
        for (int w = 0; w < 5; ++w)
#pragma unroll
            for (int j = 0; j < 5; ++j) win[w][j] = 0;
#pragma unroll
        for (int step = 0; step < kSubRowsPerThread + 2 * kSubHalo; ++step) {
            const uint8_t *row = gcol + (rb + step) * (kSubGreyDw * 4);
            int g[5];
#pragma unroll
            for (int w = 0; w < 5; ++w) g[w] = row[w];
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int j = 0; j < 5; ++j) win[w][j] = win[w + 1][j];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                int h = 0;
#pragma unroll
                for (int w = 0; w < 5; ++w)
                    if (sub_weight(j, w) != 0) h += sub_weight(j, w) * g[w];
                win[4][j] = h;
            }
            if (step < 2 * kSubHalo) continue;
            const int pr = rb + step - 2 * kSubHalo;                  // the anchor row whose five filtered rows the window now holds
            if (pr < nr && tc < nc) {
                const uint32_t a = acol[pr * kSubCols];
#pragma unroll
                for (int jy = 0; jy < 5; ++jy)
#pragma unroll
                    for (int jx = 0; jx < 5; ++jx) {
                        int v = 8192;
#pragma unroll
                        for (int w = 0; w < 5; ++w)
                            if (sub_weight(jy, w) != 0) v += sub_weight(jy, w) * win[w][jx];
                        v >>= 14;
                        v = v < 0 ? 0 : v > 255 ? 255 : v;
                        acc[jy * 5 + jx] = __builtin_amdgcn_sad_u8(a, (uint32_t)v, acc[jy * 5 + jx]);
                    }
            }
        }
    }
    // ---- the workgroup's 25 sums (at most 32 * 64 * 255 each), then one atomic per admissible candidate ----
#pragma unroll
    for (int k = 0; k < 25; ++k) {
        uint32_t s = acc[k];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
        if ((t & 63) == 0 && s) atomicAdd(&s_sum[k], s);
    }
    __syncthreads();
    if (t < 25) {
        const int Qy = 4 * dy + t / 5 - 2, Qx = 4 * dx + t % 5 - 2;
        if (sub_axis_inside(y0, Ho, Hs, Qy) && sub_axis_inside(x0, Wo, Ws, Qx))      // excluded: k_stab_sub_pick marks it
            atomicAdd(&sub[(int64_t)f * 25 + t], (u64)s_sum[t]);
    }
}

__global__ __launch_bounds__(64) void k_stab_sub_pick(u64 *__restrict__ sub, const swk_shift *__restrict__ shifts,
                                                      const uint32_t *__restrict__ nonzero, int Hs, int Ws, int y0, int x0, int Ho, int Wo,
                                                      swk_subshift *__restrict__ recs)
{
    __shared__ u64 s_score[25];
    const int f = blockIdx.x, t = threadIdx.x;
    const swk_shift first = shifts[f];
    u64 *tab = sub + (int64_t)f * 25;
    if (t < 25) {
        const int Qy = 4 * first.dy + t / 5 - 2, Qx = 4 * first.dx + t % 5 - 2;
        const bool inside = sub_axis_inside(y0, Ho, Hs, Qy) && sub_axis_inside(x0, Wo, Ws, Qx);
        if (!inside) tab[t] = ~0ull;
        s_score[t] = inside ? tab[t] : ~0ull;                         // (no score reaches UINT64_MAX)
    }
    __syncthreads();
    if (t == 0) {
        StabKey best{s_score[12], 16 * (first.dy * first.dy + first.dx * first.dx), 4 * first.dy, 4 * first.dx};      // q = (0, 0): always a candidate
        if (nonzero[f])                                               // a null frame is not matched
            for (int k = 0; k < 25; ++k) {
                if (s_score[k] == ~0ull) continue;
                const int Qy = 4 * first.dy + k / 5 - 2, Qx = 4 * first.dx + k % 5 - 2;
                const StabKey key{s_score[k], Qy * Qy + Qx * Qx, Qy, Qx};
                if (stab_less(key, best)) best = key;
            }
        swk_subshift rec;
        rec.dy = first.dy; rec.dx = first.dx; rec.qy_total = best.dy; rec.qx_total = best.dx;
        rec.sad = best.sad; rec.sad_int = first.sad; rec.sad_unshifted = first.sad_unshifted;
        recs[f] = rec;
    }
}

// out [F][Ho][Wo][3] dense; four bytes of a row per thread
__global__ __launch_bounds__(256) void k_stab_resample(const uint8_t *__restrict__ frames, int64_t fs, int64_t rs, int y0, int x0, int Ho,
                                                       int Wo, const swk_subshift *__restrict__ recs, uint8_t *__restrict__ out)
{
    const int f = blockIdx.y;
    const int rowb = Wo * 3, wq = (rowb + 3) >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Ho * wq) return;
    const int r = idx / wq, c = (idx - r * wq) << 2;
    const int nb = rowb - c < 4 ? rowb - c : 4;
    const int Qy = recs[f].qy_total, Qx = recs[f].qx_total;
    const int py = Qy & 3, px = Qx & 3;
    // byte c of row r at phase (0, 0); the taps reach rows -1..+2 and pixels -1..+2 (3 bytes each) around it
    const uint8_t *src = frames + (int64_t)f * fs + (int64_t)(y0 + (Qy >> 2) + r) * rs + (int64_t)(x0 + (Qx >> 2)) * 3 + c;
    uint8_t *dst = out + ((int64_t)f * Ho + r) * rowb + c;
    uint32_t word = 0;
    if (py == 0 && px == 0) {
        for (int k = 0; k < nb; ++k) word |= (uint32_t)src[k] << (8 * k);
    } else {
        for (int k = 0; k < nb; ++k) {
            int v = 8192;
            for (int ky = 0; ky < 4; ++ky) {
                const int wy = kSubTap[py][ky];
                if (wy == 0) continue;                                // (not read: it may lie outside the frame)
                const uint8_t *row = src + (int64_t)(ky - 1) * rs + k;
                int h = 0;
                for (int kx = 0; kx < 4; ++kx) {
                    const int wx = kSubTap[px][kx];
                    if (wx != 0) h += wx * (int)row[3 * (kx - 1)];
                }
                v += wy * h;
            }
            v >>= 14;
            word |= (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << (8 * k);
        }
    }
    if (nb == 4 && ((uintptr_t)dst & 3) == 0) *(uint32_t *)dst = word;
    else for (int k = 0; k < nb; ++k) dst[k] = (uint8_t)(word >> (8 * k));
}

size_t stabilize_sub_table_bytes(int F) { return (size_t)F * 25 * sizeof(u64); }

void launch_stabilize_subpel(hipStream_t s, const uint8_t *frames, int64_t fs, int64_t rs, int F, int Hs, int Ws, int y0, int x0, int Ho,
                             int Wo, int S, const uint8_t *anchor, int gray_mode, uint8_t *plane, uint32_t *nonzero, void *table,
                             swk_shift *shifts, void *sub_table, swk_subshift *recs, uint8_t *out)
{
    u64 *tab = (u64 *)table, *sub = (u64 *)sub_table;
    const int pitch = stabilize_pitch(Ws), ncand = (2 * S + 1) * (2 * S + 1);
    hipError_t me = hipMemsetAsync(tab, 0, stabilize_table_bytes(F, S), s);
    if (me == hipSuccess) me = hipMemsetAsync(sub, 0, stabilize_sub_table_bytes(F), s);
    if (me == hipSuccess) me = hipMemsetAsync(nonzero, 0, (size_t)F * 4, s);
    if (me != hipSuccess) { g_launch_error = (int)me; return; }          // surfaces at the context's next sync()
    const int gq = Hs * (pitch >> 2), cq = Ho * ((Wo * 3 + 3) >> 2);
    for (int f0 = 0; f0 < F; f0 += 32768) {
        const int fc = F - f0 < 32768 ? F - f0 : 32768;
        const uint8_t *fp = frames + (int64_t)f0 * fs;
        uint8_t *pp = plane + (int64_t)f0 * Hs * pitch;
        hipLaunchKernelGGL(k_stab_gray, dim3((gq + 255) / 256, fc), dim3(256), 0, s, fp, fs, rs, Hs, Ws, pitch, gray_mode, pp, nonzero + f0);
        note_launch();
        const dim3 grid((Wo + kStabCols - 1) / kStabCols, (Ho + kStabRows - 1) / kStabRows, fc);
        hipLaunchKernelGGL(k_stab_sad, grid, dim3(kStabThreads), 0, s, anchor, pp, Hs, Ws, pitch, y0, x0, Ho, Wo, S, tab + (int64_t)f0 * ncand);
        note_launch();
        hipLaunchKernelGGL(k_stab_pick, dim3(fc), dim3(256), 0, s, tab + (int64_t)f0 * ncand, nonzero + f0, Hs, Ws, y0, x0, Ho, Wo, S,
                           shifts + f0);
        note_launch();
        const dim3 sgrid((Wo + kSubCols - 1) / kSubCols, (Ho + kSubRows - 1) / kSubRows, fc);
        hipLaunchKernelGGL(k_stab_sub_sad, sgrid, dim3(kSubThreads), 0, s, anchor, pp, Hs, Ws, pitch, y0, x0, Ho, Wo, shifts + f0,
                           sub + (int64_t)f0 * 25);
        note_launch();
        hipLaunchKernelGGL(k_stab_sub_pick, dim3(fc), dim3(64), 0, s, sub + (int64_t)f0 * 25, shifts + f0, nonzero + f0, Hs, Ws, y0, x0, Ho,
                           Wo, recs + f0);
        note_launch();
        hipLaunchKernelGGL(k_stab_resample, dim3((cq + 255) / 256, fc), dim3(256), 0, s, fp, fs, rs, y0, x0, Ho, Wo, recs + f0,
                           out + (int64_t)f0 * Ho * Wo * 3);
        note_launch();
    }
}

}  // namespace swk
