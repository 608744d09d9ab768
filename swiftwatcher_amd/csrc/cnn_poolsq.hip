// Max-pool + the squeeze convolution behind it as ONE kernel (the three MaxPool2d(3, 2) of SqueezeNet-1.0 are each followed by a Fire
// module's 1x1 squeeze: features 2 -> 3, 6 -> 7, 11 -> 12 of torchvision's network, segment_classification.py of the reference :47-67):
//
//     dst[n][off_y + y][off_x + x][co] = max(sum_ci W[co][ci] * max_{dy,dx < 3} src[n][2 y + dy][2 x + dx][ci] + bias[co], 0)
//
// Separately the pooled tensor made one round trip through HBM (written by k_maxpool3s2, read back by k_conv1x1_relu_place): 332 KB of
// the 1.07 MB the pair moves per segment at pool3 + fire9.  Two kernels, chosen by the number of row tiles (pool_squeeze_by_row_tiles):
// k_pool_squeeze for the large forwards, k_pool_squeeze_seg (a workgroup per segment, described where it stands) for the small ones.
// In k_pool_squeeze the pool is the LOAD STAGE of a persistent 1x1 kernel built like k_conv1x1_relu_place (cnn_conv1x1.hip).
//   * rows are the pooled pixels flattened over the batch (n P^2 of them); a wave owns a tile of 32 rows and all output channels of it
//     (one or two 32-channel column blocks).  No pixel is pooled twice, an 81-pixel map pads nothing, and there is no barrier in the
//     main loop: a wave works alone.
//   * the whole weight matrix sits transposed in LDS, [ci][co] with pitch 32 NBLK + 1, next to the padded bias, staged once per
//     workgroup; the workgroup is persistent over the row tiles.
//   * a tile is pooled 32 channels at a time.  Eight consecutive lanes load the eight float4 of ONE pixel's 128-byte line, so a load
//     instruction covers eight whole lines: the L1 looks lines up one per clock, and with the MFMA's own operand layout (a lane = a
//     pixel, its float4 a quarter of a line) nine taps per pixel ran at that lookup rate, a quarter slower than the kernel before
//     this one.  A lane (quad q, pixel row pl) pools the four pixels 8 u + pl of the tile: nine taps of four float4, loaded one tap
//     ROW (12 float4) at a time, ahead of use: row 0 of the NEXT chunk leaves before the current chunk's MFMAs, rows 1 and 2 are
//     folded in and issued between thirds of the MFMAs, and the pipeline runs on into the wave's next row tile.
//   * the pooled chunk crosses to the MFMA's layout through 4.25 KB of LDS that belong to the wave alone, [channel][pixel] with pitch
//     34 (writes and operand reads are free of bank conflicts): LDS instructions of one wave execute in order, so no barrier and no
//     second buffer are needed: the chunk is written after the last operand read of the previous one.
//   * what does not depend on the chunk is computed once per row tile (locate): each pixel's window in its segment's tile and in the
//     ring tile, and a nine-bit mask of the taps inside the live square.  A tap outside it is LOADED from the ring tile: the choice
//     is made on the address, so a value from the wrong source never exists in a register, let alone enters a maximum.
//   * the arithmetic is that of k_maxpool3s2 followed by k_conv1x1_relu_place at cin % 32 == 0, value for value: an exact maximum
//     (taps in the order (dy, dx) ascending), then the k-ordered chain of v_mfma_f32_32x32x2_f32: chunks ascending, step i of a chunk
//     multiplies channels {kb + i, kb + 16 + i}, one accumulator per column block.
//
// Addresses.  A pooled pixel (py, px) has py, px <= P - 1 and P = (T - 3) / 2 + 1, so its taps touch rows and columns 2 py + d <=
// 2 P <= T - 1 (T - 2 when T is even: row and column T - 1 are never read), channels kb + 4 q .. + 3 <= C - 1 with kb <= C - 32:
// every offset lies inside one T x T x C tile.  The tile is segment `seg` of src with seg <= n - 1 (rows past the end repeat row
// n P^2 - 1) or the ring tile.  A run-ahead load reads a chunk c + 1 < nchunk of the same row tile or chunk 0 of a row tile below
// ntiles (the wave's next one; after its last tile, that tile's own chunk 0 once more): no address is formed beyond these.
// Launched on the CALLER's stream (PyTorch's current stream), like the other classifier kernels.
#include "cnn_common.h"

namespace swk {

constexpr int POOLSQ_XP = 34;                               // pitch of a wave's pooled chunk [32 channels][32 pixels] in LDS
constexpr int POOLSQ_XFLOATS = 32 * POOLSQ_XP;              // 4,352 bytes per wave

// NBLK = 32-channel column blocks (1 or 2), NWV = waves per workgroup.  Three waves per SIMD: 168 registers.
template <int NBLK, int NWV>
__global__ __launch_bounds__(64 * NWV, 3) void k_pool_squeeze(const float *__restrict__ src, int64_t rows, int T, int C, const float *__restrict__ wgt,
                                                              const float *__restrict__ bias, int S, float *__restrict__ dst, int dH, int dW, int dC,
                                                              int off_y, int off_x, const float *__restrict__ ring, int live_lo, int live_n,
                                                              FastDiv fpp, FastDiv fp)
{
    constexpr int NP = 32 * NBLK, PITCH = NP + 1, NT = 64 * NWV, KC = 32, XP = POOLSQ_XP;
    extern __shared__ float lds[];                 // weights [C][PITCH], the bias padded to NP, then a pooled chunk per wave
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5, q = lane & 7, pl = lane >> 3;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform for the compiler too: scalar loop control
    float *lbias = lds + ((C * PITCH + 3) & ~3);
    float *xw = lbias + NP + wave * POOLSQ_XFLOATS + (4 * q) * XP + pl;           // where the lane writes its pooled values
    const float *xr = lbias + NP + wave * POOLSQ_XFLOATS + (16 * hh) * XP + r;    // where it reads its pixel operand
    const int P = (int)fp.d, nchunk = C / KC;
    const int rs = T * C;                          // floats per source row (a tile is far below 2^31 floats: C is bounded by the LDS)
    const int64_t ntiles = (rows + 31) >> 5, stride = (int64_t)gridDim.x * NWV;
    int64_t tile = (int64_t)blockIdx.x * NWV + wave;

    // the loader's state, per pixel 8 u + pl of the tile being loaded: where this lane's quad of the pixel's window starts in its
    // segment's tile and in the ring tile, and which of the nine taps (bit 3 dy + dx) lie in the live square; lk = the chunk's
    // first channel
    const float *lsrc[4];
    int lwin[4];
    unsigned lmask[4];
    int lk = 0;
    // row j of a row tile (rows past the end repeat the last one): segment and pooled pixel.
    // The tile number goes through an empty asm statement: the compiler then computes this where it is written, at a tile's last
    // chunk and in its epilogue, instead of ahead of the chunk loop, where the results would occupy registers through all of it.
    auto pixel = [&](unsigned t32, int j, unsigned &seg, unsigned &py, unsigned &px) -> bool {
        asm volatile("" : "+s"(t32));
        const unsigned m = t32 * 32u + (unsigned)j;          // rows < 2^31 (checked by the launcher): invariant-divisor division
        const bool valid = m < (unsigned)rows;
        const unsigned mm = valid ? m : (unsigned)rows - 1u;
        seg = fpp.div(mm);
        const unsigned p = mm - seg * fpp.d;
        py = fp.div(p);
        px = p - py * (unsigned)P;
        return valid;
    };
    auto locate = [&](int64_t t) {
        int l = threadIdx.x & 63;     // like the tile number: the lane's place in the load layout is worked out here
        asm volatile("" : "+v"(l));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned seg, py, px;
            pixel((unsigned)t, 8 * u + (l >> 3), seg, py, px);
            lwin[u] = (int)(2 * py) * rs + (int)(2 * px) * C + 4 * (l & 7);
            lsrc[u] = src + (int64_t)seg * T * rs + lwin[u];
            unsigned iny = 0, inx = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                iny |= (unsigned)((unsigned)(2 * py + d - live_lo) < (unsigned)live_n) << d;
                inx |= (unsigned)((unsigned)(2 * px + d - live_lo) < (unsigned)live_n) << d;
            }
            lmask[u] = ((iny & 1u) ? inx : 0u) | ((iny & 2u) ? inx << 3 : 0u) | ((iny & 4u) ? inx << 6 : 0u);
        }
    };
    float4 L[3][4];                // one tap row in flight: [dx][pixel u]
    float4 m[4];                   // the running maximum of the chunk being loaded, per pixel u
    auto issue = [&](int dy) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
                L[dx][u] = *(const float4 *)((((lmask[u] >> (3 * dy + dx)) & 1u) ? lsrc[u] : ring + lwin[u]) + (lk + dy * rs + dx * C));
    };
    auto max4 = [](const float4 a, const float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); };
    auto fold = [&](bool first) {
#pragma unroll
        for (int u = 0; u < 4; ++u) m[u] = max4(max4(first ? L[0][u] : max4(m[u], L[0][u]), L[1][u]), L[2][u]);
    };

    // the first tap row leaves before the weights are staged (a wave without a tile loads the last one's and drops it: every load
    // below is unconditional, so the tap row lives in one set of registers)
    locate(tile < ntiles ? tile : ntiles - 1);
    issue(0);
    // ---- weights, transposed: W[co][ci] read along ci as float4s (16 lanes = 64 channels of one output channel), [ci][co] in LDS ----
    for (int co = tid >> 4; co < NP; co += NT / 16)
        for (int c4 = (tid & 15) * 4; c4 < C; c4 += 64) {
            const float4 wv = co < S ? *(const float4 *)(wgt + (int64_t)co * C + c4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float *w = lds + c4 * PITCH + co;
            w[0] = wv.x; w[PITCH] = wv.y; w[2 * PITCH] = wv.z; w[3 * PITCH] = wv.w;
        }
    for (int i = tid; i < NP; i += NT) lbias[i] = i < S ? bias[i] : 0.0f;
    fold(true);
    issue(1);
    fold(false);
    issue(2);
    __syncthreads();

    const float *wrow0 = lds + (16 * hh) * PITCH + r, *wrow = wrow0;
    float bw[2][NBLK], bx[2];

    // steps I0 .. I1 - 1 of a chunk: the operands of step i + 1 (weights, and the lane's pixel from the wave's pooled chunk) are read
    // from LDS while step i multiplies (two register sets, scheduling fences, as in k_conv1x1_relu_place)
#define SWK_PS_STEPS(I0, I1)                                                                                                          \
    _Pragma("unroll") for (int i = I0; i < I1; ++i) {                                                                                 \
        if (i < 15) {                                                                                                                 \
            _Pragma("unroll") for (int nb = 0; nb < NBLK; ++nb) bw[(i + 1) & 1][nb] = wrow[(i + 1) * PITCH + 32 * nb];                \
            bx[(i + 1) & 1] = xr[(i + 1) * XP];                                                                                       \
        }                                                                                                                             \
        _Pragma("unroll") for (int nb = 0; nb < NBLK; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(bw[i & 1][nb], bx[i & 1], acc[nb], 0, 0, 0); \
        if (i < 15) __builtin_amdgcn_sched_group_barrier(0x100 /* DS read */, NBLK + 1, 0);                                           \
        __builtin_amdgcn_sched_group_barrier(0x008 /* MFMA */, NBLK, 0);                                                              \
    }

    for (; tile < ntiles; tile += stride) {
        const bool more = tile + stride < ntiles;
        f16v acc[NBLK];
#pragma unroll
        for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nb][e] = 0.0f;
        for (int c = 0; c < nchunk; ++c) {
            // tap row 2 completes this chunk's pooled values; they cross to the MFMA's layout through the wave's own LDS (in-order
            // within a wave: the previous chunk's operand reads are done, the reads below see these writes)
            fold(false);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xw[8 * u] = m[u].x; xw[XP + 8 * u] = m[u].y; xw[2 * XP + 8 * u] = m[u].z; xw[3 * XP + 8 * u] = m[u].w;
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int nb = 0; nb < NBLK; ++nb) bw[0][nb] = wrow[32 * nb];
            bx[0] = xr[0];
            // the chunk that is loaded while this one multiplies: the next of this tile, or the first of the wave's next tile (after
            // its last tile a wave loads that tile's first chunk once more and drops it)
            const bool last = c + 1 == nchunk;
            if (!last) lk += KC;
            else { lk = 0; locate(more ? tile + stride : tile); }
            __builtin_amdgcn_sched_barrier(0);          // the loads stay behind the fold: one tap row of registers, not two
            issue(0);
            __builtin_amdgcn_sched_barrier(0);
            SWK_PS_STEPS(0, 5)
            __builtin_amdgcn_sched_barrier(0);
            fold(true);
            issue(1);
            __builtin_amdgcn_sched_barrier(0);
            SWK_PS_STEPS(5, 10)
            __builtin_amdgcn_sched_barrier(0);
            fold(false);
            issue(2);
            __builtin_amdgcn_sched_barrier(0);
            SWK_PS_STEPS(10, 16)
            __builtin_amdgcn_sched_barrier(0);
            wrow = last ? wrow0 : wrow + KC * PITCH;
        }
        // ---- bias + ReLU + placement: register quads = four consecutive output channels of the lane's pixel ----
        unsigned seg, py, px;
        int h4 = lane;                 // 4 hh, through an empty asm statement like the tile number: nothing of the epilogue's
        asm volatile("" : "+v"(h4));   // addressing is kept in registers through the chunk loop
        const int rr = h4 & 31;
        h4 = (h4 >> 5) * 4;
        if (pixel((unsigned)tile, rr, seg, py, px)) {
            float *o = dst + (((int64_t)seg * dH + off_y + py) * dW + off_x + px) * (int64_t)dC + h4;
#pragma unroll
            for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = nb * 32 + 8 * g;
                    if (co + h4 < S) store_bias_relu(o + co, acc[nb], g, *(const float4 *)(lbias + co + h4));
                }
        }
    }
#undef SWK_PS_STEPS
}

// bytes of LDS of a workgroup of nwv waves: the weights [C][32 nblk + 1] rounded up to four floats, the padded bias, a pooled chunk per wave
static size_t pool_squeeze_lds(int C, int nblk, int nwv)
{
    return (size_t)(((C * (32 * nblk + 1) + 3) & ~3) + 32 * nblk + nwv * POOLSQ_XFLOATS) * sizeof(float);
}

template <int NBLK, int NWV>
static int launch_pool_squeeze_w(hipStream_t s, const float *src, int64_t rows, int T, int C, int P, const float *wgt, const float *bias, int S,
                                 const Place &pl, const float *ring, int live_lo, int live_n)
{
    const size_t lds = pool_squeeze_lds(C, NBLK, NWV);
    static unsigned long long attr_mask = 0;          // lds <= 160 KB - 256 and rows < 2^31: pool_squeeze_by_row_tiles
    if (!ensure_dyn_lds((const void *)k_pool_squeeze<NBLK, NWV>, 160 * 1024 - 256, attr_mask)) return SWK_ERR_HIP;
    const int64_t ntiles = (rows + 31) / 32;
    int64_t blocks = (ntiles + NWV - 1) / NWV;
    // persistent over the row tiles: as many workgroups per CU as three waves per SIMD (the kernel's registers) and the LDS allow
    const int64_t by_lds = (int64_t)((160 * 1024 - 256) / lds), by_waves = 12 / NWV;
    const int64_t cap = 256 * (by_lds < by_waves ? by_lds : by_waves);
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((k_pool_squeeze<NBLK, NWV>), dim3((unsigned)blocks), dim3(64 * NWV), lds, s, src, rows, T, C, wgt, bias, S, pl.dst, pl.dH, pl.dW,
                       pl.dC, pl.off_y, pl.off_x, ring, live_lo, live_n, FastDiv((unsigned)(P * P)), FastDiv((unsigned)P));
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

// ---- fewer row tiles than two rounds of the resident waves: a workgroup per segment ----
// The kernel this file had before the row-tile kernel.  A workgroup owns a segment: its P x P pooled pixels (at most 96) are formed 32
// channels at a time in LDS (item = (pooled pixel, channel quad): nine float4 loads, eight lanes per 128-byte line), the chunk's weights
// are read along ci and transposed into LDS beside them, wave (pt, nb) multiplies 32 pixels x 32 output channels with the same k-ordered
// chain; double-buffered, one barrier per chunk.  Every wave of the row-tile kernel walks its tiles alone, three dependent load round
// trips per chunk, so a launch that gives a wave one or two tiles is as long as its slowest wave: measured against this kernel
// (profiles/poolsq_cnn_layers_summary.txt) the row tiles lose 10-46 % on the 8 x 8 maps at 1,024 and 2,048 rows (2,048 and 4,096 row
// tiles against 3,072 resident waves) and 3-6 % on 512 -> 64 at 256 and 512 rows, and win 5-18 % from two rounds on.
template <int PT, int NB>
__global__ __launch_bounds__(64 * PT * NB) void k_pool_squeeze_seg(const float *__restrict__ src, int n, int T, int C, int P, const float *__restrict__ wgt,
                                                                   const float *__restrict__ bias, int S, float *__restrict__ dst, int dH, int dW, int dC,
                                                                   int off_y, int off_x, const float *__restrict__ ring, int live_lo, int live_n)
{
    constexpr int NW = PT * NB, NT = 64 * NW, PP = 32 * PT + 1, SP = 32 * NB + 1, KC = 32;
    __shared__ float sB[2][KC * PP];          // pooled pixels of a chunk: [channel k][pixel]
    __shared__ float sA[2][KC * SP];          // the chunk's weights: [channel k][output channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int pt = wave % PT, nb = wave / PT;
    const int npix = P * P, nchunk = C / KC;
    const int64_t rs = (int64_t)T * C;          // floats per source row

    auto stage = [&](int seg, int c, int buf) {
        const int kb = c * KC;
        // ---- weights: (co, quad of k) items, float4 along ci ----
        for (int i = tid; i < 32 * NB * 8; i += NT) {
            const int co = i >> 3, q = i & 7;
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < S) w = *(const float4 *)(wgt + (int64_t)co * C + kb + 4 * q);
            float *a = &sA[buf][(4 * q) * SP + co];
            a[0] = w.x; a[SP] = w.y; a[2 * SP] = w.z; a[3 * SP] = w.w;
        }
        // ---- pooled pixels: (pixel, quad of k) items ----
        // pixels outside the live square [live_lo, live_lo + live_n)^2 hold the same values in every segment's tile (the ring the
        // tiles were created with): they are read from ONE tile (`ring`, cache-resident) instead of the segment's own -- at pool2 /
        // pool3 half of a tile's bytes.  ring == src's first tile and live = the whole tile when the caller has no ring.
        const float *base = src + (int64_t)seg * T * rs + kb, *rbase = ring + kb;
        for (int i = tid; i < 32 * PT * 8; i += NT) {
            const int p = i >> 3, q = i & 7;
            float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < npix) {
                const int py = p / P, px = p - py * P;
                const int64_t o0 = (int64_t)(2 * py) * rs + (int64_t)(2 * px) * C + 4 * q;
                bool iny[3], inx[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    iny[d] = (unsigned)(2 * py + d - live_lo) < (unsigned)live_n;
                    inx[d] = (unsigned)(2 * px + d - live_lo) < (unsigned)live_n;
                }
                m = *(const float4 *)((iny[0] && inx[0] ? base : rbase) + o0);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        if (dy == 0 && dx == 0) continue;
                        const float4 v = *(const float4 *)((iny[dy] && inx[dx] ? base : rbase) + o0 + dy * rs + dx * C);
                        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
                    }
            }
            float *b = &sB[buf][(4 * q) * PP + p];
            b[0] = m.x; b[PP] = m.y; b[2 * PP] = m.z; b[3 * PP] = m.w;
        }
    };

    for (int seg = blockIdx.x; seg < n; seg += gridDim.x) {
        f16v acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        stage(seg, 0, 0);
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const int buf = c & 1;
            if (c + 1 < nchunk) stage(seg, c + 1, buf ^ 1);
            const float *a = &sA[buf][(16 * hh) * SP + 32 * nb + r];
            const float *b = &sB[buf][(16 * hh) * PP + 32 * pt + r];
#pragma unroll
            for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i * SP], b[i * PP], acc, 0, 0, 0);
            __syncthreads();
        }
        // ---- bias + ReLU + placement: register quad g = output channels 32 nb + 8 g + 4 hh .. + 3 of pixel 32 pt + r ----
        const int p = 32 * pt + r;
        if (p < npix) {
            const int py = p / P, px = p - py * P;
            float *o = dst + (((int64_t)seg * dH + off_y + py) * dW + off_x + px) * dC + 32 * nb + 4 * hh;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = 32 * nb + 8 * g + 4 * hh;
                if (co < S) store_bias_relu(o + 8 * g, acc, g, *(const float4 *)(bias + co));
            }
        }
    }
}

template <int PT, int NB>
static int launch_pool_squeeze_seg(hipStream_t s, const float *src, int n, int T, int C, int P, const float *wgt, const float *bias, int S, const Place &pl,
                                   const float *ring, int live_lo, int live_n)
{
    int blocks = n < 256 * 8 ? n : 256 * 8;          // persistent over the segments beyond a few workgroups per CU
    hipLaunchKernelGGL((k_pool_squeeze_seg<PT, NB>), dim3((unsigned)blocks), dim3(64 * PT * NB), 0, s, src, n, T, C, P, wgt, bias, S, pl.dst, pl.dH, pl.dW,
                       pl.dC, pl.off_y, pl.off_x, ring, live_lo, live_n);
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}


// The row-tile kernel from two rounds of its resident waves on (256 CUs x the waves per workgroup that fit beside the weights: twelve,
// six next to 512 x 65 floats), the segment kernel below that, for a weight matrix that leaves no room for three waves' pooled chunks
// and for 2^31 rows or more.  Measured crossovers: between 4,096 and 8,192 row tiles on the 8 x 8 maps (rule: 6,144), between 1,296
// and 2,592 on 512 -> 64 (rule: 3,072).
static bool pool_squeeze_by_row_tiles(int n, int P, int C, int nblk, int &nwv)
{
    const int64_t rows = (int64_t)n * P * P, ntiles = (rows + 31) / 32;
    nwv = 12;
    while (nwv > 3 && pool_squeeze_lds(C, nblk, nwv) > 160 * 1024 - 256) nwv /= 2;
    return pool_squeeze_lds(C, nblk, nwv) <= 160 * 1024 - 256 && rows <= (int64_t)0x7fffff00 && ntiles >= 2 * 256 * nwv;
}

template <int NBLK>
static int launch_pool_squeeze(hipStream_t s, const float *src, int n, int T, int C, int P, int nwv, const float *wgt, const float *bias, int S,
                               const Place &pl, const float *ring, int live_lo, int live_n)
{
    const int64_t rows = (int64_t)n * P * P;
    if (nwv == 12) return launch_pool_squeeze_w<NBLK, 12>(s, src, rows, T, C, P, wgt, bias, S, pl, ring, live_lo, live_n);
    if (nwv == 6) return launch_pool_squeeze_w<NBLK, 6>(s, src, rows, T, C, P, wgt, bias, S, pl, ring, live_lo, live_n);
    return launch_pool_squeeze_w<NBLK, 3>(s, src, rows, T, C, P, wgt, bias, S, pl, ring, live_lo, live_n);
}

}  // namespace swk

#pragma GCC visibility push(default)
extern "C" {

int32_t swk_nhwc_maxpool3s2_conv1x1_bias_relu_place(void *stream, const float *src, int32_t n, int32_t t, int32_t cin, const float *weight,
                                                    const float *bias, int32_t cout, float *dst, int32_t dH, int32_t dW, int32_t dC,
                                                    int32_t off_y, int32_t off_x, const float *ring, int32_t live_lo, int32_t live_n)
{
    const int P = (t - 3) / 2 + 1;
    const swk::Place pl{dst, dH, dW, dC, off_y, off_x, 0};          // no c_off: the squeeze output starts at channel 0
    // beyond the placement: the shapes the kernel is built for (32-channel chunks, at most 96 pooled pixels and 64 outputs per
    // segment), float4 loads of src, weight and bias
    if (!src || !weight || !bias || n < 1 || t < 3 || cin < 32 || (cin & 31) || cout > 64 || P * P > 96 || !swk::place_ok(pl, P, P, cout, true) ||
        (((uintptr_t)src | (uintptr_t)weight | (uintptr_t)bias) & 15))
        return SWK_ERR_ARG;
    if (!ring) { ring = src; live_lo = 0; live_n = t; }
    if (live_lo < 0 || live_n < 0 || live_lo + live_n > t || ((uintptr_t)ring & 15)) return SWK_ERR_ARG;
    using namespace swk;
    hipStream_t s = (hipStream_t)stream;
    const int PT = (P * P + 31) / 32, NB = (cout + 31) / 32;
    int nwv;
    if (pool_squeeze_by_row_tiles(n, P, cin, NB, nwv)) {
        if (NB == 1) return launch_pool_squeeze<1>(s, src, n, t, cin, P, nwv, weight, bias, cout, pl, ring, live_lo, live_n);
        return launch_pool_squeeze<2>(s, src, n, t, cin, P, nwv, weight, bias, cout, pl, ring, live_lo, live_n);
    }
    if (PT == 1 && NB == 1) return launch_pool_squeeze_seg<1, 1>(s, src, n, t, cin, P, weight, bias, cout, pl, ring, live_lo, live_n);
    if (PT == 2 && NB == 1) return launch_pool_squeeze_seg<2, 1>(s, src, n, t, cin, P, weight, bias, cout, pl, ring, live_lo, live_n);
    if (PT == 3 && NB == 1) return launch_pool_squeeze_seg<3, 1>(s, src, n, t, cin, P, weight, bias, cout, pl, ring, live_lo, live_n);
    if (PT == 1 && NB == 2) return launch_pool_squeeze_seg<1, 2>(s, src, n, t, cin, P, weight, bias, cout, pl, ring, live_lo, live_n);
    if (PT == 2 && NB == 2) return launch_pool_squeeze_seg<2, 2>(s, src, n, t, cin, P, weight, bias, cout, pl, ring, live_lo, live_n);
    if (PT == 3 && NB == 2) return launch_pool_squeeze_seg<3, 2>(s, src, n, t, cin, P, weight, bias, cout, pl, ring, live_lo, live_n);
    return SWK_ERR_ARG;
}

}  // extern "C"
#pragma GCC visibility pop
