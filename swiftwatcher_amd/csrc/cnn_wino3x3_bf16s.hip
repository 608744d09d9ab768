// The Winograd F(2x2, 3x3) expands of cnn_wino3x3.hip with every float32 product formed as SIX bf16 x bf16 products of three-way split
// operands (the arithmetic of cnn_expand_bf16.hip):
//
//     U = u1 + u2 + u3,  V = v1 + v2 + v3  (each part bf16, the remainders exact: 3 x 8 bits cover float32's 24)
//     U V  ~  u1 v3 + u2 v2 + u3 v1 + u1 v2 + u2 v1 + u1 v1          (smallest first; the three terms below 2^-24 |U V| are dropped)
//
// v_mfma_f32_32x32x16_bf16 accumulates in float32 at 16 times the rate of v_mfma_f32_32x32x2_f32: the six products cost 6 x 32 cycles per
// 16 channels x 32 x 32 outputs where the float32 kernel pays 8 x 64, and the bf16 MFMA holds vector issue for 8 of its 32 cycles, so the
// transforms, splits and output updates (which the float32 MFMA shares one execution unit with) run beside it.  Float32-grade results
// (tests/test_wino_bf16s.py: at most the float32 kernel's error against float64).
//
// Kept from the float32 kernel: positions in sequence through ONE accumulator M per tile group, Y_ij += c M after each position, V_p formed
// once per task by the workgroup (a signed sum of four patch pixels), double buffered in LDS, the filter operands streamed into LDS by
// LDS-DMA with hand-placed counted waits (asm: see cnn_wino3x3.hip), the fused bias + ReLU + placement epilogue.
// Changed:
//   * a wave owns ONE column block of 32 output channels and TWO tile groups of 32 tiles: a workgroup = cout / 32 waves over 64 tiles, so
//     each filter operand read from LDS feeds two tile groups, and the filter bytes streamed per output tile are 0.75 of the float32
//     kernel's (1.5 x the bytes per value, over twice the tiles).  Y = 2 x 2 x 2 x 16 + M 2 x 16 accumulator registers: two waves per SIMD.
//   * the filter slices are private to their wave ([phase][column block][SPP k-steps][part][lane][8 bf16], host-made by
//     swk_winograd_f2x2_3x3_weights_bf16s): its own vmcnt tells a wave that they have landed, and the workgroup meets once per POSITION
//     (for V), not once per phase.  SPP k-steps per phase: every k-step of a position where LDS allows, two of four for 64 -> 256.
//   * V is split right after the signed sum and stored as three bf16 B operands [part][k / 8][tile (+ pad)][8]: one ds_read_b128 per part
//     and tile group per k-step, 512 contiguous bytes per half wave; the pad makes the staging stores conflict-free.
// Where it stands (MI355X, batch 4,096, tools/bench_convs.py, against the float32 kernel in the same call): 64 -> 256 on 16 x 16 outputs
// 987 us against 1,303, on 11 x 11 533 against 714; 48 -> 192 430 / 612 against 499 / 714; 32 -> 128 281 / 153 against 329 / 168 --
// the Winograd total of a forward 3.17 against 3.89 ms.  16 -> 64 measured slower (77 / 101 against 73 / 93 us) and stays on the float32
// kernel in the classifier.  The matrix pipe is no longer the wall: the six products put 64 -> 256 near 0.33 ms of MFMA time, a third of
// what it takes.  What remains is the filter stream (0.75 of the float32 kernel's bytes per tile, from L2 by LDS-DMA, one phase ahead),
// the per-position V staging (patch loads, transform and split per thread, then a workgroup barrier) and LDS bank conflicts
// (0.6-1.1 conflict cycles per LDS instruction, profiles/wino_bf16s_pmc_counters.txt); the counters do not separate these further.
// The staging loads every patch pixel once per ROW of positions: the four positions (xi, 0..3) combine the column pairs (0,2) (1,2)
// (2,1) (1,3) of the same two patch rows, so (xi, 0) loads four pixels, (xi, 1) and (xi, 3) two and (xi, 2) none -- 32 pixel loads
// per item and task where 64 were issued, the same values into the same expressions (bit-identical outputs).  nu is unrolled for it,
// so that the registers and their roles are fixed in the code.  The 16-wave 64 -> 256 layout cannot hold pixels through a position's
// products at 128 registers: it loads the four pixels of (xi, 1), stores V(xi, 1) and, after the barrier, V(xi, 2) from the same
// registers into the buffer that barrier has freed (the compiler further keeps column 1 for (xi, 3): 40 loads, no scratch).
// Measured: DESIGN section 6, "Patch pixels once per row of positions".
// Twice the tiles per filter byte would need 128 x 256 outputs in one CU's registers (Y alone fills the register file) or V formed
// twice; see DESIGN section 10.
// Two kernels: k_wino3x3_bf16s_relu_place as described above (32 -> 128, and every shape under swk_set_cnn_tuning(2, 1)), and
// k_wino3x3_bf16s_shared_relu_place further down, in which two waves share a column block's filter slice (48 -> 192 on 12 waves: 378 / 531
// against 430 / 612 us; 64 -> 256 on 16 waves: 941 / 510 against 978 / 535; 32 -> 128 over 128 tiles measured slower, 295 / 162 against
// 287 / 155, and is reached by the knob only).  Bit-identical outputs; DESIGN sections 6 and 10.
// Launched on the CALLER's stream.
#include "cnn_common.h"

#include <type_traits>

namespace swk {

// k-steps (16 input channels) per filter phase of a shape: the host layout depends on it
static int wino_bf16s_spp(int cin, int cout) { return cin == 64 && cout == 256 ? 2 : cin / 16; }

// tile pad of a V row: 16 / (8-channel groups) tiles, so that a 16-lane pass of staging stores spreads over all banks
template <int KG> struct WinoVPad { static constexpr int value = KG == 6 ? 3 : 16 / KG; };

template <int NBLK, int SPP>
__global__ __launch_bounds__(64 * NBLK, 2) void k_wino3x3_bf16s_relu_place(const float *__restrict__ src, int nseg, int t, int T,
                                                                          const uint16_t *__restrict__ wu, const float *__restrict__ bias,
                                                                          int cout, float *__restrict__ dst, int dH, int dW, int dC, int off_y,
                                                                          int off_x, int c_off, FastDiv fTT, FastDiv fT)
{
    // NBLK column blocks = waves = 8-channel groups of the input (cout = 4 cin); S k-steps per position, PHS phases of SPP of them
    constexpr int NW = NBLK, NT = 64 * NW, KG = NBLK, CIN = 8 * KG, S = CIN / 16, PHS = S / SPP, SLOTS = 64, NP = 32 * NBLK;
    constexpr int VT = SLOTS + WinoVPad<KG>::value;          // 16-byte rows of a V part
    constexpr int WPB = SPP * 3 * 1024;                       // bytes of a wave's filter slice of one phase
    static_assert(S % SPP == 0 && NT == SLOTS * KG, "one staging item per thread");
    extern __shared__ uint4 lds_w[];          // W[2][NW][WPB], V[2][3][KG][VT] x 16 B, the bias padded to NP
    char *const Wl = (char *)lds_w;
    uint4 *const V0 = (uint4 *)(Wl + 2 * NW * WPB), *const V1 = V0 + 3 * KG * VT;
    float *const lbias = (float *)(V1 + 3 * KG * VT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int o = t - 2, TT = T * T;
    const int64_t ntiles = (int64_t)nseg * TT, src_floats = (int64_t)nseg * t * t * CIN;
    const int64_t ntasks = (ntiles + SLOTS - 1) / SLOTS;
    for (int i = tid; i < NP; i += NT) lbias[i] = i < cout ? bias[i] : 0.0f;

    // ---- the staging item of this thread: (tile slot, 8-channel group), channel group fastest (a wave reads whole pixels) ----
    const int sg = tid % KG, sslot = tid / KG;
    unsigned sbase;          // byte offset of the item's patch origin in src
    int slim;                // largest byte offset a patch load of the item may add (the last 32 bytes of src)
    const char *const srcb = (const char *)src;
    auto stage_setup = [&](int64_t task) {
        int ti = tid;
        asm volatile("" : "+v"(ti));          // opaque: the next task's origin is formed at its last position, not held through all sixteen
        const int item = ti;
        int64_t m = task * SLOTS + item / KG;
        if (m >= ntiles) m = ntiles - 1;
        const unsigned bu = fTT.div((unsigned)m), rem = (unsigned)m - bu * (unsigned)TT, ty = fT.div(rem), tx = rem - ty * (unsigned)T;
        const int64_t b = bu;
        const int64_t base = (((b * t + 2 * ty) * t + 2 * tx) * (int64_t)CIN + 8 * (item % KG)) * 4;
        const int64_t lim = src_floats * 4 - 32 - base;          // a patch may reach one row / column past an odd-sized tile
        sbase = (unsigned)base;
        slim = (int)(lim < (1 << 30) ? lim : (1 << 30));
    };
    float4 st[4][2];
    // patch rows (columns) position xi (nu) combines, as in cnn_wino3x3.hip: first row {0,1,2,1}, second {2,2,1,3}, sign {-,+,-,-}.
    // Along a row of positions the column pairs are (0,2) (1,2) (2,1) (1,3): st[0], st[2] hold the pixels of column 0, then 1, and
    // st[1], st[3] those of column 2, then 3 -- nu = 0 loads all four, nu = 1 and 3 one column each, nu = 2 none (nu is a constant
    // of the unrolled code: the slots and their roles cost nothing at run time).  Nothing is kept from one xi to the next.
    auto stage_issue = [&](int xi, int nu) {
        const int ra[2] = {(0x1210 >> (4 * xi)) & 15, (0x3122 >> (4 * xi)) & 15};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = (i & 1) ? (nu == 3 ? 3 : 2) : (nu == 0 ? 0 : 1);
            if ((i & 1) ? (nu == 0 || nu == 3) : nu < 2) {
                const int os = (ra[i >> 1] * t + col) * (CIN * 4);
                const char *q = srcb + (sbase + (unsigned)(os < slim ? os : slim));
                st[i][0] = *(const float4 *)q;
                st[i][1] = *(const float4 *)(q + 16);
            }
        }
    };
    // V = (d00 + sn d01) + sx (d10 + sn d11), split three ways, stored as the parts' B operands; nu = 2 takes the columns (2,1) from
    // the slots of (1,2)
    auto stage_store = [&](int xi, int nu, uint4 *Vn) {
        const float sx = xi == 1 ? 1.0f : -1.0f, sn = nu == 1 ? 1.0f : -1.0f;
        const int ia = nu == 2 ? 1 : 0, ib = 1 - ia;
        bf16x8 v1, v2, v3;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float a[4] = {st[ia][h].x, st[ia][h].y, st[ia][h].z, st[ia][h].w}, b[4] = {st[ib][h].x, st[ib][h].y, st[ib][h].z, st[ib][h].w},
                        c[4] = {st[2 + ia][h].x, st[2 + ia][h].y, st[2 + ia][h].z, st[2 + ia][h].w},
                        d[4] = {st[2 + ib][h].x, st[2 + ib][h].y, st[2 + ib][h].z, st[2 + ib][h].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = __builtin_fmaf(__builtin_fmaf(d[e], sn, c[e]), sx, __builtin_fmaf(b[e], sn, a[e]));
                __bf16 x1, x2, x3;
                split3(v, x1, x2, x3);
                v1[4 * h + e] = x1; v2[4 * h + e] = x2; v3[4 * h + e] = x3;
            }
        }
        uint4 *q = Vn + sg * VT + sslot;
        q[0] = __builtin_bit_cast(uint4, v1);
        q[KG * VT] = __builtin_bit_cast(uint4, v2);
        q[2 * KG * VT] = __builtin_bit_cast(uint4, v3);
    };

    // ---- this wave's filter slice of phase g: WPB contiguous bytes of wu, copied as they lie by LDS-DMA (cnn_common.h), three 1 KB
    //      pieces (the parts) per k-step ----
    const unsigned wvoff = (unsigned)(lane * 16);
    auto w_issue = [&](int g, int buf) {
        const char *gp = (const char *)wu + ((int64_t)g * NW + __builtin_amdgcn_readfirstlane(wave)) * WPB;          // uniform
        const unsigned l = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(Wl + (buf * NW + wave) * WPB));
#pragma unroll
        for (int sub = 0; sub < SPP; ++sub) lds_dma_copy<3>(l + sub * 3072u, gp + sub * 3072, wvoff);
    };
    // the copies of a phase are issued BEFORE the patch loads: where a position has two phases, lds_dma_wait<N>() retires them and leaves
    // the N patch loads of the next position (eight, four or none) in flight

    int64_t task = blockIdx.x;
    if (task < ntasks) {
        stage_setup(task);
        stage_issue(0, 0);
        stage_store(0, 0, V0);
        w_issue(0, 0);
    }
    lds_dma_wait<0>();
    __syncthreads();
    for (; task < ntasks; task += gridDim.x) {
        const bool more = task + gridDim.x < ntasks;
        f16v Y[2][2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int tg = 0; tg < 2; ++tg)
#pragma unroll
                    for (int e = 0; e < 16; ++e) Y[i][j][tg][e] = 0.0f;
        // one phase = SPP k-steps of this wave's column block: 6 SPP dependent MFMAs per tile group
        auto phase = [&](const char *Wb, const uint4 *Vc, int s0, f16v *M) {
            const uint4 *wq = (const uint4 *)Wb + lane;
#pragma unroll
            for (int sub = 0; sub < SPP; ++sub) {
                const int s = s0 + sub;
                const bf16x8 u1 = __builtin_bit_cast(bf16x8, wq[(3 * sub) * 64]), u2 = __builtin_bit_cast(bf16x8, wq[(3 * sub + 1) * 64]),
                             u3 = __builtin_bit_cast(bf16x8, wq[(3 * sub + 2) * 64]);
#pragma unroll
                for (int tg = 0; tg < 2; ++tg) {
                    const uint4 *vq = Vc + (2 * s + hh) * VT + 32 * tg + r;
                    const bf16x8 x1 = __builtin_bit_cast(bf16x8, vq[0]), x2 = __builtin_bit_cast(bf16x8, vq[KG * VT]),
                                 x3 = __builtin_bit_cast(bf16x8, vq[2 * KG * VT]);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, x3, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u2, x2, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u3, x1, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, x2, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u2, x1, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, x1, M[tg], 0, 0, 0);
                }
            }
        };
        // positions p = 4 xi + nu in their natural order, the four of a row unrolled (and no more than those)
#pragma unroll 1
        for (int xi = 0; xi < 4; ++xi)
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
            const int p = 4 * xi + nu;
            const uint4 *Vc = (nu & 1) ? V1 : V0;
            uint4 *Vn = (nu & 1) ? V0 : V1;
            const int xin = nu == 3 ? (xi + 1) & 3 : xi, nun = (nu + 1) & 3;          // the next position
            if (nu == 3 && xi == 3 && more) stage_setup(task + gridDim.x);
            // Y_ij += A^T[i][xi] A^T[j][nu] M_p,   A^T = [1 1 1 0; 0 1 -1 -1]
            const float ax[2] = {xi < 3 ? 1.0f : 0.0f, xi == 0 ? 0.0f : xi == 1 ? 1.0f : -1.0f};
            const float an[2] = {nu < 3 ? 1.0f : 0.0f, nu == 0 ? 0.0f : nu == 1 ? 1.0f : -1.0f};
            f16v M[2];
#pragma unroll
            for (int tg = 0; tg < 2; ++tg)
#pragma unroll
                for (int e = 0; e < 16; ++e) M[tg][e] = 0.0f;
#pragma unroll
            for (int h = 0; h < PHS; ++h) {
                // the next phase's filter slice travels while this one multiplies; the next position's new patch pixels during the whole
                // position (after a workgroup's last position they fetch position 0 of the same tiles again, unused: see cnn_wino3x3.hip)
                const int g = p * PHS + h, gn = g + 1 == 16 * PHS ? 0 : g + 1;
                // No barrier lies between the phases of a position, so nothing but this wait keeps the copy below from overwriting the
                // buffer the phase before read while its last operand reads are still on their way: where the next position has no patch
                // pixels to fetch, the compiler puts the reads of the last parts (u2, u3 of the second k-step) right in front of the copy,
                // and in a few tasks of a hundred they returned the next phase's bytes
                if (h > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                w_issue(gn, (g + 1) & 1);
                if (h == 0) stage_issue(xin, nun);
                phase(Wl + ((g & 1) * NW + wave) * WPB, Vc, h * SPP, M);
                if (h == PHS - 1) {
                    stage_store(xin, nun, Vn);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const float c = ax[i] * an[j];
                            if (c != 0.0f) {          // uniform; 36 of the 64 (position, pair) combinations
#pragma unroll
                                for (int tg = 0; tg < 2; ++tg)
#pragma unroll
                                    for (int e = 0; e < 16; ++e) Y[i][j][tg][e] = __builtin_fmaf(M[tg][e], c, Y[i][j][tg][e]);
                            }
                        }
                }
                // this wave's slice of the next phase has landed (patch loads issued in a first phase of several stay in flight)
                if (h == 0 && PHS > 1 && nun == 0) lds_dma_wait<8>();
                else if (h == 0 && PHS > 1 && nun != 2) lds_dma_wait<4>();
                else lds_dma_wait<0>();
                // the next position's V is complete, this one's buffer is free
                if (h == PHS - 1) __syncthreads();
            }
        }
        // ---- this lane's two tiles as the matrix cores see them: destinations of their 2 x 2 outputs (formed here, not before the
        //      positions: nothing of it occupies a register meanwhile) ----
        int te = tid;
        asm volatile("" : "+v"(te));          // opaque: what follows from it is formed here every task and not kept through the positions
        const int re = te & 31, he = (te >> 5) & 1, we = te >> 6;
        int64_t ro[2];
        bool valid[2], vy1[2], vx1[2];
#pragma unroll
        for (int tg = 0; tg < 2; ++tg) {
            const int64_t m = task * SLOTS + tg * 32 + re;
            valid[tg] = m < ntiles;
            const int64_t mm = valid[tg] ? m : ntiles - 1;
            const unsigned bu = fTT.div((unsigned)mm), rem = (unsigned)mm - bu * (unsigned)TT;
            const int ty = (int)fT.div(rem), tx = (int)(rem - (unsigned)ty * (unsigned)T);
            const int64_t b = bu;
            ro[tg] = ((b * dH + off_y + 2 * ty) * dW + off_x + 2 * tx) * (int64_t)dC + c_off + 32 * we + 4 * he;
            vy1[tg] = 2 * ty + 1 < o;
            vx1[tg] = 2 * tx + 1 < o;
        }
        // ---- bias + ReLU + placement: register quads = four consecutive output channels of the lane's tile ----
#pragma unroll
        for (int tg = 0; tg < 2; ++tg) {
            if (!valid[tg]) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if ((i == 1 && !vy1[tg]) || (j == 1 && !vx1[tg])) continue;
                    float *q = dst + ro[tg] + ((int64_t)i * dW + j) * dC;
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const int c = 32 * we + 8 * gq + 4 * he;
                        if (c < cout) store_bias_relu(q + 8 * gq, Y[i][j][tg], gq, *(const float4 *)(lbias + c));
                    }
                }
        }
    }
}

template <int NBLK, int SPP>
static int launch_wino3x3_bf16s(hipStream_t s, const float *src, int n, int t, const uint16_t *wu, const float *bias, int cout, const Place &pl)
{
    constexpr int NW = NBLK, KG = NBLK, CIN = 8 * NBLK, VT = 64 + WinoVPad<KG>::value;
    const size_t lds = (size_t)2 * NW * SPP * 3 * 1024 + (size_t)2 * 3 * KG * VT * 16 + 32 * NBLK * sizeof(float);
    static_assert((size_t)2 * NW * SPP * 3 * 1024 + (size_t)2 * 3 * KG * VT * 16 + 32 * NBLK * 4 <= 160 * 1024 - 256, "LDS of one workgroup");
    static unsigned long long attr_mask = 0;
    if (!ensure_dyn_lds((const void *)k_wino3x3_bf16s_relu_place<NBLK, SPP>, 160 * 1024 - 256, attr_mask)) return SWK_ERR_HIP;
    if ((int64_t)n * t * t * CIN * 4 >= ((int64_t)1 << 32)) return SWK_ERR_CAPACITY;          // 32-bit byte offsets into src (and tile indices)
    const int T = (t - 2 + 1) / 2;
    const int64_t ntiles = (int64_t)n * T * T;
    int64_t blocks = (ntiles + 63) / 64;
    // persistent workgroups, two waves per SIMD: as many per CU as eight waves and the LDS allow
    const int64_t by_lds = (int64_t)((160 * 1024 - 256) / lds), by_waves = 8 / NW;
    const int64_t per_cu = by_waves < 1 ? 1 : (by_lds < by_waves ? by_lds : by_waves);
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    hipLaunchKernelGGL((k_wino3x3_bf16s_relu_place<NBLK, SPP>), dim3((unsigned)blocks), dim3(64 * NW), lds, s, src, n, t, T, wu, bias, cout, pl.dst,
                       pl.dH, pl.dW, pl.dC, pl.off_y, pl.off_x, pl.c_off, FastDiv((unsigned)(T * T)), FastDiv((unsigned)T));
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

// ---- the shared-filter layouts: WCB waves per column block, TGW tile groups (32 tiles) per wave ----
// A task is SLOTS = 32 TGW WCB tiles and a workgroup NBLK WCB waves: wave (cb, j) owns column block cb and tile groups j TGW .. j TGW + TGW - 1.
// What differs from k_wino3x3_bf16s_relu_place, which is <TGW 2, WCB 1> (the arithmetic and its order are the same: outputs are bit-identical,
// tests/test_wino_bf16s_layouts_gpu.py):
//   * the WCB waves of a column block read ONE filter slice per phase (the host layout, the LDS bytes and the bytes streamed per 64 tiles
//     are unchanged).  They divide its 1 KB pieces between them, each waits on its own vmcnt, and the workgroup barrier shows a wave its
//     partner's pieces: with one phase per position that is the barrier which ends the position anyway, with two (64 -> 256) every phase
//     ends in one -- it also keeps a partner's operand reads ahead of the copy that overwrites them.
//   * TGW 1: twice the threads for the 64 KG staging items.  A thread takes four channels of an item, neighbouring lanes the two halves
//     (a wave's float4 loads stay contiguous): 4 loads and three 8-byte LDS stores.  TGW 2: one item per thread over 128 slots.
//   * WPS waves per SIMD, WPS x 4 / (NBLK WCB) workgroups per CU: 48 -> 192 as 12 waves (3 on every SIMD, where six waves of two tile
//     groups leave two SIMDs half empty), 32 -> 128 as 8 waves over 128 tiles (half the filter bytes, copies and barriers per tile).
// The staging stores meet the LDS in groups of 16 lanes x 8 bytes or 8 lanes x 16 bytes, eight consecutive items over 32 banks, so the rows
// (16 bytes) of the items of a group have to differ mod 8: VT = 2 mod 8 for four channel groups, odd for eight; six admit no such pad
// (one pair of the eight collides).  The operand reads are contiguous per half wave whatever the pad.
template <int KG> struct WinoVPadW { static constexpr int value = KG == 4 ? 2 : KG == 6 ? 3 : 1; };

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

template <int NBLK, int SPP, int TGW, int WCB, int WPS>
__global__ __launch_bounds__(64 * NBLK * WCB, WPS) void k_wino3x3_bf16s_shared_relu_place(const float *__restrict__ src, int nseg, int t, int T,
                                                                                         const uint16_t *__restrict__ wu,
                                                                                         const float *__restrict__ bias, int cout,
                                                                                         float *__restrict__ dst, int dH, int dW, int dC, int off_y,
                                                                                         int off_x, int c_off, FastDiv fTT, FastDiv fT)
{
    constexpr int NW = NBLK * WCB, NT = 64 * NW, KG = NBLK, CIN = 8 * KG, S = CIN / 16, PHS = S / SPP, SLOTS = 32 * TGW * WCB, NP = 32 * NBLK;
    constexpr bool LATE = WPS == 4;                           // at 128 registers the patch pixels are fetched after a position's products
    constexpr int NH = TGW;                                   // 4-channel halves of a staging item per thread
    constexpr int VT = SLOTS + WinoVPadW<KG>::value;          // 16-byte rows of a V part
    constexpr int WPB = SPP * 3 * 1024;                       // bytes of a column block's filter slice of one phase
    constexpr int PC = 3 * SPP, PC0 = (PC + WCB - 1) / WCB;   // its 1 KB pieces; those of a column block's first wave
    static_assert(S % SPP == 0 && NT * NH == 2 * SLOTS * KG && (TGW == 1 || TGW == 2) && (WCB == 1 || WCB == 2), "staging items and waves");
    extern __shared__ uint4 lds_w[];          // W[2][NBLK][WPB], V[2][3][KG][VT] x 16 B, the bias padded to NP
    char *const Wl = (char *)lds_w;
    uint4 *const V0 = (uint4 *)(Wl + 2 * NBLK * WPB), *const V1 = V0 + 3 * KG * VT;
    float *const lbias = (float *)(V1 + 3 * KG * VT);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), cb = wv % NBLK, wj = wv / NBLK, tg0 = wj * TGW;
    const int o = t - 2, TT = T * T;
    const int64_t ntiles = (int64_t)nseg * TT, src_floats = (int64_t)nseg * t * t * CIN;
    const int64_t ntasks = (ntiles + SLOTS - 1) / SLOTS;
    for (int i = tid; i < NP; i += NT) lbias[i] = i < cout ? bias[i] : 0.0f;

    // ---- the staging item of this thread: (tile slot, 8-channel group), channel group fastest (a wave reads whole pixels); with two
    //      threads per item the half is faster still ----
    const int item = NH == 2 ? tid : tid >> 1, shalf = NH == 2 ? 0 : tid & 1;
    const int sg = item % KG, sslot = item / KG;
    unsigned sbase;          // byte offset of the thread's part of the patch origin in src
    int slim;                // largest byte offset a patch load of the thread may add (the last 16 NH bytes of src)
    const char *const srcb = (const char *)src;
    auto stage_setup = [&](int64_t task) {
        int ti = tid;
        asm volatile("" : "+v"(ti));          // opaque: the next task's origin is formed at its last position, not held through all sixteen
        const int item = NH == 2 ? ti : ti >> 1;
        int64_t m = task * SLOTS + item / KG;
        if (m >= ntiles) m = ntiles - 1;
        const unsigned bu = fTT.div((unsigned)m), rem = (unsigned)m - bu * (unsigned)TT, ty = fT.div(rem), tx = rem - ty * (unsigned)T;
        const int64_t b = bu;
        const int64_t base = (((b * t + 2 * ty) * t + 2 * tx) * (int64_t)CIN + 8 * (item % KG) + 4 * (NH == 2 ? 0 : ti & 1)) * 4;
        const int64_t lim = src_floats * 4 - 16 * NH - base;          // a patch may reach one row / column past an odd-sized tile
        sbase = (unsigned)base;
        slim = (int)(lim < (1 << 30) ? lim : (1 << 30));
    };
    float4 st[4][NH];
    // the slots as in k_wino3x3_bf16s_relu_place: st[0], st[2] hold column 0, then 1, st[1], st[3] column 2, then 3.  Where st lives
    // through a position (!LATE) a position loads only the columns its row of positions has not loaded yet: all four pixels for nu = 0,
    // one column for nu = 1 and 3, nothing for nu = 2.  LATE keeps nothing through the products: `both` loads the position's two columns.
    auto stage_issue = [&](int xi, int nu, bool both) {
        const int ra[2] = {(0x1210 >> (4 * xi)) & 15, (0x3122 >> (4 * xi)) & 15};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = (i & 1) ? (nu == 3 ? 3 : 2) : (nu == 0 ? 0 : 1);
            if (nu != 2 && (both || ((i & 1) ? (nu == 0 || nu == 3) : nu < 2))) {
                const int os = (ra[i >> 1] * t + col) * (CIN * 4);
                const char *q = srcb + (sbase + (unsigned)(os < slim ? os : slim));
#pragma unroll
                for (int h = 0; h < NH; ++h) st[i][h] = *(const float4 *)(q + 16 * h);
            }
        }
    };
    // V = (d00 + sn d01) + sx (d10 + sn d11), split three ways, stored as the parts' B operands; nu = 2 takes the columns (2,1) from
    // the slots of (1,2)
    auto stage_store = [&](int xi, int nu, uint4 *Vn) {
        const float sx = xi == 1 ? 1.0f : -1.0f, sn = nu == 1 ? 1.0f : -1.0f;
        const int ia = nu == 2 ? 1 : 0, ib = 1 - ia;
        bf16x4 v1[NH], v2[NH], v3[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const float a[4] = {st[ia][h].x, st[ia][h].y, st[ia][h].z, st[ia][h].w}, b[4] = {st[ib][h].x, st[ib][h].y, st[ib][h].z, st[ib][h].w},
                        c[4] = {st[2 + ia][h].x, st[2 + ia][h].y, st[2 + ia][h].z, st[2 + ia][h].w},
                        d[4] = {st[2 + ib][h].x, st[2 + ib][h].y, st[2 + ib][h].z, st[2 + ib][h].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = __builtin_fmaf(__builtin_fmaf(d[e], sn, c[e]), sx, __builtin_fmaf(b[e], sn, a[e]));
                __bf16 x1, x2, x3;
                split3(v, x1, x2, x3);
                v1[h][e] = x1; v2[h][e] = x2; v3[h][e] = x3;
            }
        }
        uint4 *q = Vn + sg * VT + sslot;
        if constexpr (NH == 2) {
            const uint2 a1 = __builtin_bit_cast(uint2, v1[0]), b1 = __builtin_bit_cast(uint2, v1[NH - 1]), a2 = __builtin_bit_cast(uint2, v2[0]),
                        b2 = __builtin_bit_cast(uint2, v2[NH - 1]), a3 = __builtin_bit_cast(uint2, v3[0]), b3 = __builtin_bit_cast(uint2, v3[NH - 1]);
            q[0] = make_uint4(a1.x, a1.y, b1.x, b1.y);
            q[KG * VT] = make_uint4(a2.x, a2.y, b2.x, b2.y);
            q[2 * KG * VT] = make_uint4(a3.x, a3.y, b3.x, b3.y);
        } else {
            ((uint2 *)q)[shalf] = __builtin_bit_cast(uint2, v1[0]);
            ((uint2 *)(q + KG * VT))[shalf] = __builtin_bit_cast(uint2, v2[0]);
            ((uint2 *)(q + 2 * KG * VT))[shalf] = __builtin_bit_cast(uint2, v3[0]);
        }
    };

    // ---- this wave's pieces of its column block's filter slice of phase g (WPB contiguous bytes of wu, copied as they lie) ----
    const unsigned wvoff = (unsigned)(lane * 16);
    auto w_pieces = [&](auto first, auto count, unsigned l, const char *gp) {
        constexpr int F = decltype(first)::value, N = decltype(count)::value;
#pragma unroll
        for (int i = 0; i + 3 <= N; i += 3) lds_dma_copy<3>(l + (F + i) * 1024u, gp + (F + i) * 1024, wvoff);
        if constexpr (N % 3 != 0) lds_dma_copy<N % 3>(l + (F + N - N % 3) * 1024u, gp + (F + N - N % 3) * 1024, wvoff);
    };
    auto w_issue = [&](int g, int buf) {
        const char *gp = (const char *)wu + ((int64_t)g * NBLK + cb) * WPB;          // uniform
        const unsigned l = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(Wl + (buf * NBLK + cb) * WPB));
        if (WCB == 1 || wj == 0) w_pieces(std::integral_constant<int, 0>(), std::integral_constant<int, PC0>(), l, gp);
        else w_pieces(std::integral_constant<int, PC0>(), std::integral_constant<int, PC - PC0>(), l, gp);
    };
    // the copies of a phase are issued BEFORE the patch loads: lds_dma_wait<N>() retires them and leaves the N patch loads of the next
    // position (4 NH, 2 NH or none) in flight

    int64_t task = blockIdx.x;
    if (task < ntasks) {
        stage_setup(task);
        stage_issue(0, 0, true);
        stage_store(0, 0, V0);
        w_issue(0, 0);
    }
    lds_dma_wait<0>();
    __syncthreads();
    for (; task < ntasks; task += gridDim.x) {
        const bool more = task + gridDim.x < ntasks;
        f16v Y[2][2][TGW];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int tg = 0; tg < TGW; ++tg)
#pragma unroll
                    for (int e = 0; e < 16; ++e) Y[i][j][tg][e] = 0.0f;
        // one phase = SPP k-steps of this wave's column block: 6 SPP dependent MFMAs per tile group
        auto phase = [&](const char *Wb, const uint4 *Vc, int s0, f16v *M) {
            const uint4 *wq = (const uint4 *)Wb + lane;
#pragma unroll
            for (int sub = 0; sub < SPP; ++sub) {
                const int s = s0 + sub;
                const bf16x8 u1 = __builtin_bit_cast(bf16x8, wq[(3 * sub) * 64]), u2 = __builtin_bit_cast(bf16x8, wq[(3 * sub + 1) * 64]),
                             u3 = __builtin_bit_cast(bf16x8, wq[(3 * sub + 2) * 64]);
#pragma unroll
                for (int tg = 0; tg < TGW; ++tg) {
                    const uint4 *vq = Vc + (2 * s + hh) * VT + 32 * (tg0 + tg) + r;
                    const bf16x8 x1 = __builtin_bit_cast(bf16x8, vq[0]), x2 = __builtin_bit_cast(bf16x8, vq[KG * VT]),
                                 x3 = __builtin_bit_cast(bf16x8, vq[2 * KG * VT]);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, x3, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u2, x2, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u3, x1, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, x2, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u2, x1, M[tg], 0, 0, 0);
                    M[tg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, x1, M[tg], 0, 0, 0);
                }
                // at 128 registers the operands of one k-step at a time: nothing is scheduled across
                if constexpr (WPS == 4) __builtin_amdgcn_sched_barrier(0);
            }
        };
        // positions p = 4 xi + nu in their natural order, the four of a row unrolled (and no more than those)
#pragma unroll 1
        for (int xi = 0; xi < 4; ++xi)
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
            const int p = 4 * xi + nu;
            uint4 *const Vc = (nu & 1) ? V1 : V0, *const Vn = (nu & 1) ? V0 : V1;
            const int xin = nu == 3 ? (xi + 1) & 3 : xi, nun = (nu + 1) & 3;          // the next position
            if (nu == 3 && xi == 3 && more) stage_setup(task + gridDim.x);
            // Y_ij += A^T[i][xi] A^T[j][nu] M_p,   A^T = [1 1 1 0; 0 1 -1 -1]
            const float ax[2] = {xi < 3 ? 1.0f : 0.0f, xi == 0 ? 0.0f : xi == 1 ? 1.0f : -1.0f};
            const float an[2] = {nu < 3 ? 1.0f : 0.0f, nu == 0 ? 0.0f : nu == 1 ? 1.0f : -1.0f};
            f16v M[TGW];
#pragma unroll
            for (int tg = 0; tg < TGW; ++tg)
#pragma unroll
                for (int e = 0; e < 16; ++e) M[tg][e] = 0.0f;
#pragma unroll
            for (int h = 0; h < PHS; ++h) {
                // the next phase's filter slice travels while this one multiplies (into the buffer the phase before this one read: a barrier
                // lies between), the next position's new patch pixels during the whole position
                const int g = p * PHS + h, gn = g + 1 == 16 * PHS ? 0 : g + 1;
                // where no barrier ends a phase, the wave's own operand reads of the buffer the copy overwrites (k_wino3x3_bf16s_relu_place)
                if (h > 0 && WCB == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                w_issue(gn, (g + 1) & 1);
                if (h == 0 && !LATE) stage_issue(xin, nun, false);
                phase(Wl + ((g & 1) * NBLK + cb) * WPB, Vc, h * SPP, M);
                if (h == PHS - 1) {
                    // LATE: V(xi, 2) was stored at the start of (xi, 1), below: nothing to fetch or to store at its end
                    if (LATE) stage_issue(xin, nun, true);
                    if (!LATE || nun != 2) stage_store(xin, nun, Vn);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const float c = ax[i] * an[j];
                            if (c != 0.0f) {          // uniform; 36 of the 64 (position, pair) combinations
#pragma unroll
                                for (int tg = 0; tg < TGW; ++tg)
#pragma unroll
                                    for (int e = 0; e < 16; ++e) Y[i][j][tg][e] = __builtin_fmaf(M[tg][e], c, Y[i][j][tg][e]);
                            }
                        }
                }
                // this wave's pieces of the next phase have landed (patch loads issued in a first phase of several stay in flight) ...
                if (h == 0 && PHS > 1 && !LATE && nun == 0) lds_dma_wait<4 * NH>();
                else if (h == 0 && PHS > 1 && !LATE && nun != 2) lds_dma_wait<2 * NH>();
                else lds_dma_wait<0>();
                // ... and the barrier shows them to its partner; after the last phase the next position's V is complete, this one's buffer free
                if (h == PHS - 1 || WCB > 1) __syncthreads();
            }
            // LATE: the pixels of (xi, 1) are those of (xi, 2).  Its V goes into the buffer the barrier has just freed, before the products
            // of (xi, 1) need the registers, and is read two barriers later
            if (LATE && nu == 0) {
                stage_store(xi, 2, Vc);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- this lane's tiles as the matrix cores see them: destinations of their 2 x 2 outputs (formed here, not
        //      before the positions: nothing of it occupies a register meanwhile) ----
        int le = tid & 63;
        asm volatile("" : "+v"(le));          // opaque: what follows from it is formed here every task and not kept through the positions
        const int re = le & 31, he = le >> 5;
        int64_t ro[TGW];
        bool valid[TGW], vy1[TGW], vx1[TGW];
#pragma unroll
        for (int tg = 0; tg < TGW; ++tg) {
            const int64_t m = task * SLOTS + (tg0 + tg) * 32 + re;
            valid[tg] = m < ntiles;
            const int64_t mm = valid[tg] ? m : ntiles - 1;
            const unsigned bu = fTT.div((unsigned)mm), rem = (unsigned)mm - bu * (unsigned)TT;
            const int ty = (int)fT.div(rem), tx = (int)(rem - (unsigned)ty * (unsigned)T);
            const int64_t b = bu;
            ro[tg] = ((b * dH + off_y + 2 * ty) * dW + off_x + 2 * tx) * (int64_t)dC + c_off + 32 * cb + 4 * he;
            vy1[tg] = 2 * ty + 1 < o;
            vx1[tg] = 2 * tx + 1 < o;
        }
        // ---- bias + ReLU + placement: register quads = four consecutive output channels of the lane's tile ----
#pragma unroll
        for (int tg = 0; tg < TGW; ++tg) {
            if (!valid[tg]) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if ((i == 1 && !vy1[tg]) || (j == 1 && !vx1[tg])) continue;
                    float *q = dst + ro[tg] + ((int64_t)i * dW + j) * dC;
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const int c = 32 * cb + 8 * gq + 4 * he;
                        if (c < cout) store_bias_relu(q + 8 * gq, Y[i][j][tg], gq, *(const float4 *)(lbias + c));
                    }
                }
        }
    }
}

template <int NBLK, int SPP, int TGW, int WCB, int WPS>
static int launch_wino3x3_bf16s_shared(hipStream_t s, const float *src, int n, int t, const uint16_t *wu, const float *bias, int cout,
                                       const Place &pl)
{
    constexpr int KG = NBLK, CIN = 8 * NBLK, SLOTS = 32 * TGW * WCB, VT = SLOTS + WinoVPadW<KG>::value;
    constexpr size_t lds = (size_t)2 * NBLK * SPP * 3 * 1024 + (size_t)2 * 3 * KG * VT * 16 + 32 * NBLK * sizeof(float);
    constexpr int per_cu = 4 * WPS / (NBLK * WCB);          // whole workgroups at WPS waves on every SIMD
    static_assert(per_cu >= 1 && per_cu * lds <= 160 * 1024 - 256, "LDS of a CU's workgroups");
    static unsigned long long attr_mask = 0;
    if (!ensure_dyn_lds((const void *)k_wino3x3_bf16s_shared_relu_place<NBLK, SPP, TGW, WCB, WPS>, 160 * 1024 - 256, attr_mask)) return SWK_ERR_HIP;
    if ((int64_t)n * t * t * CIN * 4 >= ((int64_t)1 << 32)) return SWK_ERR_CAPACITY;          // 32-bit byte offsets into src (and tile indices)
    const int T = (t - 2 + 1) / 2;
    const int64_t ntiles = (int64_t)n * T * T;
    int64_t blocks = (ntiles + SLOTS - 1) / SLOTS;
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;          // persistent workgroups
    hipLaunchKernelGGL((k_wino3x3_bf16s_shared_relu_place<NBLK, SPP, TGW, WCB, WPS>), dim3((unsigned)blocks), dim3(64 * NBLK * WCB), lds, s, src, n, t,
                       T, wu, bias, cout, pl.dst, pl.dH, pl.dW, pl.dC, pl.off_y, pl.off_x, pl.c_off, FastDiv((unsigned)(T * T)),
                       FastDiv((unsigned)T));
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

// A/B switch of the layouts (swk_set_cnn_tuning knob 2): 0 = the per-shape default, 1 = k_wino3x3_bf16s_relu_place for every shape,
// 2 = the shared-filter layout wherever one is built (32 -> 128 on 128-tile tasks, 48 -> 192 and 64 -> 256 on 64; 16 -> 64 has none)
int g_wino_bf16s_layout = 0;

}  // namespace swk

#pragma GCC visibility push(default)
extern "C" {

int32_t swk_winograd_f2x2_3x3_weights_bf16s(const float *weight, int32_t cout, int32_t cin, uint16_t *out)
{
    if (!weight || !out || cout < 1 || cin < 16 || (cin & 15)) return SWK_ERR_ARG;
    // A operands of v_mfma_f32_32x32x16_bf16 (lane l: output channel 32 cb + (l & 31), input channels 16 s + 8 (l >> 5) .. + 7), output
    // channels padded to whole column blocks: [p][phase][cb][k-step of the phase][part][lane][8], a wave's slice of a phase contiguous
    const int spp = swk::wino_bf16s_spp(cin, cout), S = cin / 16, PHS = S / spp, CG = (cout + 31) / 32;
    if (S % spp) return SWK_ERR_ARG;
    for (int64_t i = 0, e = (int64_t)16 * cin * CG * 32 * 3; i < e; ++i) out[i] = 0;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            double U[4][4];          // rounded to float32 as in swk_winograd_f2x2_3x3_weights, then split
            swk::winograd_U(weight + ((int64_t)co * cin + ci) * 9, U);
            const int s = ci >> 4, ph = s / spp, sub = s % spp, lane = ((ci >> 3) & 1) * 32 + (co & 31), j = ci & 7, cb = co >> 5;
            for (int p = 0; p < 16; ++p) {
                uint16_t part[3];
                swk::split3_host((float)U[p >> 2][p & 3], part);
                const int64_t blk = (((int64_t)p * PHS + ph) * CG + cb) * spp + sub;
                for (int k = 0; k < 3; ++k) out[((blk * 3 + k) * 64 + lane) * 8 + j] = part[k];
            }
        }
    return SWK_OK;
}

int32_t swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place(void *stream, const float *src, int32_t n, int32_t t, int32_t cin,
                                                        const uint16_t *weight_s, const float *bias, int32_t cout, float *dst, int32_t dH,
                                                        int32_t dW, int32_t dC, int32_t off_y, int32_t off_x, int32_t c_off)
{
    const swk::Place pl{dst, dH, dW, dC, off_y, off_x, c_off};
    // beyond the placement: float4 patch loads and LDS-DMA filter copies (src, weight_s 16-byte aligned)
    if (!src || !weight_s || !bias || n < 1 || t < 3 || !swk::place_ok(pl, t - 2, t - 2, cout, true) || (((uintptr_t)src | (uintptr_t)weight_s) & 15))
        return SWK_ERR_ARG;
    using namespace swk;
    hipStream_t s = (hipStream_t)stream;
    // the layout of a shape: the knob's, or the shape's default (what measured faster)
    const int knob = g_wino_bf16s_layout;
    if (cin == 16 && cout == 64) return launch_wino3x3_bf16s<2, 1>(s, src, n, t, weight_s, bias, cout, pl);
    if (cin == 32 && cout == 128) {
        const int lay = knob ? knob : 1;
        if (lay == 2) return launch_wino3x3_bf16s_shared<4, 2, 2, 2, 2>(s, src, n, t, weight_s, bias, cout, pl);
        return launch_wino3x3_bf16s<4, 2>(s, src, n, t, weight_s, bias, cout, pl);
    }
    if (cin == 48 && cout == 192) {
        const int lay = knob ? knob : 2;
        if (lay == 2) return launch_wino3x3_bf16s_shared<6, 3, 1, 2, 3>(s, src, n, t, weight_s, bias, cout, pl);
        return launch_wino3x3_bf16s<6, 3>(s, src, n, t, weight_s, bias, cout, pl);
    }
    if (cin == 64 && cout == 256) {
        const int lay = knob ? knob : 2;
        if (lay == 2) return launch_wino3x3_bf16s_shared<8, 2, 1, 2, 4>(s, src, n, t, weight_s, bias, cout, pl);
        return launch_wino3x3_bf16s<8, 2>(s, src, n, t, weight_s, bias, cout, pl);
    }
    return SWK_ERR_ARG;
}

}  // extern "C"
#pragma GCC visibility pop
