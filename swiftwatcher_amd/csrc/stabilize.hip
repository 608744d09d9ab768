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

}  // namespace swk
