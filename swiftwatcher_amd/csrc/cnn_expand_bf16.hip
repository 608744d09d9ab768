// expand1x1 of the Fire modules (16 -> 64, 32 -> 128, 48 -> 192, 64 -> 256; segment_classification.py of the reference :14-67 via torchvision's
// SqueezeNet-1.0) with every float32 product formed as a SUM OF bfloat16 PRODUCTS OF SPLIT OPERANDS:
//
//     x = x1 + x2 + x3,  x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)          (the remainders are exact in float32: 3 x 8 = 24 bits)
//     w x  ~  w1 x3 + w2 x2 + w3 x1 + w1 x2 + w2 x1 + w1 x1                                  (the three terms below 2^-24 |w x| are dropped)
//
// A bf16 x bf16 product is exact in float32 and v_mfma_f32_32x32x16_bf16 accumulates in float32: the sum carries the error of a float32
// multiply-add chain (measured against float64: 2-4e-7 of the output scale, the chain of k_conv1x1_relu_place 6e-7; tools/r4/
// bf16_split_accuracy.py, test_split_bf16_expand_kernel_is_float32_accurate) -- at six MFMAs of 32 cycles per 16 channels and 32 x 32
// outputs instead of eight of 64.  Why here: in exact float32 the matrix pipe gives 157 TFLOP/s against 6 TB/s of memory, a ridge at 26
// flop per byte, and these layers write four bytes per 8-32 flop of their own: the float32 kernel holds them at 2.8-3.7 TB/s with the pipe
// half busy; the split products take the pipe out of the way.  The split itself is vector work (47 instructions per
// eight activations); the weights are split once per workgroup while they are staged.
//
// STATUS: two kernels, the same bits.  k_expand1x1_bf16s (round 4; swk_set_cnn_tuning knob 1 = 1 or SWK_EXPAND_SPLIT_BF16=1) keeps the
// split weights in LDS: per 4,096 rows (profiles/r4_cnn_split_bf16_expand.txt) 16 -> 64 33 us against the float32 kernel's 38, 32 -> 128 80
// against 98, 48 -> 192 102 / 125 against 119 / 147 -- and 64 -> 256 430 / 187 against 349 / 143: its split weights take 96 KB of LDS, one
// 8-wave workgroup per CU at 168 registers, too few waves to cover the stores.  It stayed off.
// k_expand1x1_bf16s_ws (knob 1 = 2, and every Fire shape's DEFAULT, knob 1 = 3) keeps them in registers instead: with K <= 64 a wave that
// owns one 32-channel column block needs 12 KS registers for all its split weights (12 .. 48), loads and splits them once for its
// persistent lifetime, and nothing but the activations is left in LDS -- a row tile is loaded once per workgroup with whole lines, split
// once and read as B operands by the waves of all column blocks.  At most 96 registers, no scratch (tests/test_expand_ws_codegen.py),
// 12-20 waves per CU.  Per 4,096 rows (profiles/expand_ws_cnn_layers.txt, medians of four, parent = the float32 kernel): 16 -> 64 19 / 27 us
// against 21 / 35, 32 -> 128 94 / 38 against 108 / 38, 48 -> 192 89 / 108 against 115 / 147, 64 -> 256 206 / 95 against 354 / 145; the eight
// launches 0.68 ms against 0.96 (byte floor at 6.3 TB/s: 0.50), the forward -3.8 %, as two chains -2.6 %, the headline +2.0-2.5 %
// (DESIGN section 6).  The outputs equal k_expand1x1_bf16s's bit for bit (tests/test_expand_ws_gpu.py).
//
// Layout as in k_conv1x1_relu_place: weights = A operand (i = output channel), pixels = B operand (j = pixel), so that an accumulator
// register quad holds four consecutive output channels of the lane's own pixel.  v_mfma_f32_32x32x16_bf16: lane l supplies
// A[i = l & 31][k = 8 (l >> 5) .. + 7] and B[k = 8 (l >> 5) .. + 7][j = l & 31]: a lane (pixel r, half h) loads the eight consecutive
// channels 16 s + 8 h .. + 7 of its pixel for k-step s (two float4s), all steps of a tile at once (K <= 64: at most eight float4s), and
// the next tile's while this one multiplies.  LDS: the split weights [step][column block][part][half][output channel][8] -- an operand
// read is one ds_read_b128 per lane, conflict-free.  Launched on the CALLER's stream.
#include "cnn_common.h"

namespace swk {

// NBLK column blocks of 32 output channels; KS = cin / 16 k-steps; CS waves share a row tile (each NBLK / CS column blocks); NWV waves.
template <int NBLK, int KS, int CS, int NWV>
__global__ __launch_bounds__(64 * NWV) void k_expand1x1_bf16s(const float *__restrict__ src, int64_t rows, int sh, int sw, int crop_y, int crop_x,
                                                         int h, int w, const float *__restrict__ wgt, const float *__restrict__ bias, int cout,
                                                         float *__restrict__ dst, int dH, int dW, int dC, int off_y, int off_x, int c_off,
                                                         FastDiv fhw, FastDiv fw)
{
    constexpr int CIN = 16 * KS, NP = 32 * NBLK, NB = NBLK / CS, NT = 64 * NWV, SLOTS = NWV / CS;
    static_assert(NBLK % CS == 0 && NWV % CS == 0, "column splits");
    extern __shared__ uint4 lds_e[];               // split weights: [KS][NBLK][3][2][32] x 16 bytes, then the bias padded to NP
    float *lbias = (float *)(lds_e + KS * NBLK * 3 * 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int hw = h * w, cs = wave % CS;
    const int64_t ntiles = (rows + 31) >> 5, stride = (int64_t)gridDim.x * SLOTS;
    int64_t tile = (int64_t)blockIdx.x * SLOTS + wave / CS;

    auto locate = [&](int64_t t, int64_t &ro) -> const float * {
        const unsigned m = (unsigned)t * 32u + (unsigned)r;
        const bool valid = m < (unsigned)rows;
        const unsigned mm = valid ? m : (unsigned)rows - 1u;
        const unsigned b = fhw.div(mm), rem = mm - b * (unsigned)hw;
        const unsigned y = fw.div(rem), x = rem - y * (unsigned)w;
        ro = valid ? (((int64_t)b * dH + off_y + y) * dW + off_x + x) * (int64_t)dC + c_off + 32 * NB * cs : -1;
        return src + (((int64_t)b * sh + crop_y + y) * sw + crop_x + x) * (int64_t)CIN + 8 * hh;
    };
    float4 raw[KS][2];
    int64_t ro = -1, ro_next = -1;
    const float *p = src;
    if (tile < ntiles) {           // the first tile's pixels leave before the weights are staged
        p = locate(tile, ro);
#pragma unroll
        for (int s = 0; s < KS; ++s) { raw[s][0] = *(const float4 *)(p + 16 * s); raw[s][1] = *(const float4 *)(p + 16 * s + 4); }
    }
    // ---- weights: item = (k-step, column block, half, output channel): eight floats of W[co][16 s + 8 half ..], split, three 16-byte stores ----
    for (int i = tid; i < KS * NBLK * 64; i += NT) {
        const int m = i & 31, kg = (i >> 5) & 1, nb = (i >> 6) % NBLK, s = (i >> 6) / NBLK, co = 32 * nb + m;
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (co < cout) {
            const float *q = wgt + (int64_t)co * CIN + 16 * s + 8 * kg;
            lo = *(const float4 *)q; hi = *(const float4 *)(q + 4);
        }
        bf16x8 w1, w2, w3;
        split3(lo, hi, w1, w2, w3);
        uint4 *d = lds_e + ((s * NBLK + nb) * 3) * 64 + kg * 32 + m;
        d[0] = __builtin_bit_cast(uint4, w1); d[64] = __builtin_bit_cast(uint4, w2); d[128] = __builtin_bit_cast(uint4, w3);
    }
    for (int i = tid; i < NP; i += NT) lbias[i] = i < cout ? bias[i] : 0.0f;
    __syncthreads();

    for (; tile < ntiles; tile += stride) {
        const bool more = tile + stride < ntiles;
        if (more) p = locate(tile + stride, ro_next);
        f16v acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nb][e] = 0.0f;
        // operand reads run one (k-step, column block) ahead of the products (two register sets, scheduling fences: left alone the
        // compiler reads every operand of the tile first -- 190 registers -- or each right before its MFMAs)
        bf16x8 wq[2][3];
        auto read_w = [&](int s, int nb, int set) {
            const uint4 *a = lds_e + ((s * NBLK + NB * cs + nb) * 3) * 64 + lane;
            wq[set][0] = __builtin_bit_cast(bf16x8, a[0]); wq[set][1] = __builtin_bit_cast(bf16x8, a[64]); wq[set][2] = __builtin_bit_cast(bf16x8, a[128]);
        };
        read_w(0, 0, 0);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            // this k-step's activations, split; the registers they came in take the next tile's
            bf16x8 x1, x2, x3;
            split3(raw[s][0], raw[s][1], x1, x2, x3);
            if (more) { raw[s][0] = *(const float4 *)(p + 16 * s); raw[s][1] = *(const float4 *)(p + 16 * s + 4); }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int i = s * NB + nb, set = i & 1;
                if (i + 1 < KS * NB) read_w((i + 1) / NB, (i + 1) % NB, set ^ 1);
                // smallest terms first
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][0], x3, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][1], x2, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][2], x1, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][0], x2, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][1], x1, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[set][0], x1, acc[nb], 0, 0, 0);
                if (i + 1 < KS * NB) __builtin_amdgcn_sched_group_barrier(0x100 /* DS read */, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x008 /* MFMA */, 6, 0);
            }
        }
        // ---- bias + ReLU + placement: register quads = four consecutive output channels of the lane's pixel ----
        if (ro >= 0) {
            float *o = dst + ro + 4 * hh;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = nb * 32 + 8 * g;
                    if (32 * NB * cs + c + 4 * hh < cout) store_bias_relu(o + c, acc[nb], g, *(const float4 *)(lbias + 32 * NB * cs + c + 4 * hh));
                }
        }
        ro = ro_next;
    }
}

template <int NBLK, int KS, int CS, int NWV>
static int launch_expand_bf16s(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int h, int w, const float *wgt, const float *bias,
                               int cout, const Place &pl)
{
    const size_t lds = (size_t)KS * NBLK * 3 * 64 * 16 + 32 * NBLK * sizeof(float);
    static unsigned long long attr_mask = 0;
    if (!ensure_dyn_lds((const void *)k_expand1x1_bf16s<NBLK, KS, CS, NWV>, 160 * 1024 - 256, attr_mask)) return SWK_ERR_HIP;
    if (lds > 160 * 1024 - 256 || rows > (int64_t)0x7fffff00) return SWK_ERR_CAPACITY;
    constexpr int SLOTS = NWV / CS;
    const int64_t ntiles = (rows + 31) / 32;
    int64_t blocks = (ntiles + SLOTS - 1) / SLOTS;
    const int64_t by_lds = (int64_t)((160 * 1024 - 256) / lds), by_waves = 16 / NWV;
    const int64_t per_cu = by_lds < 1 ? 1 : (by_lds < by_waves ? by_lds : by_waves);
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    hipLaunchKernelGGL((k_expand1x1_bf16s<NBLK, KS, CS, NWV>), dim3((unsigned)blocks), dim3(64 * NWV), lds, s, src, rows, cr.sh, cr.sw, cr.crop_y,
                       cr.crop_x, h, w, wgt, bias, cout, pl.dst, pl.dH, pl.dW, pl.dC, pl.off_y, pl.off_x, pl.c_off, FastDiv((unsigned)(h * w)), FastDiv((unsigned)w));
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

// ---- the weight-stationary kernel: split weights in registers, split activations handed round through LDS ----
// Row pitch (16-byte units) of an LDS operand row of 32 pixels.  A staging thread stores the three parts of (pixel, item), item = one
// (k-step, half), 2 KS per pixel, at 3 PITCH item + PITCH part + pixel; consecutive threads take consecutive items of a pixel (they
// load whole 128-byte lines).  ds_write_b128 goes by eight consecutive lanes over 32 banks = eight units: 3 PITCH = 4 (KS 1: four pixels
// x two items), 6 (KS 2: two pixels x four items) or odd (KS 4: one pixel) mod 8 keeps the eight apart; with KS 3 (six items per pixel)
// no pitch does, an odd one leaves two lanes of some groups on one bank, which the store's own 13 cycles cover.  An operand read
// (ds_read_b128, sixteen lanes over 64 banks) takes consecutive pixels of one row: conflict-free at any pitch.
template <int KS>
struct ExpandWsPitch {
    static constexpr int value = KS == 1 ? 36 : KS == 2 ? 34 : 33;
};

// NBLK column blocks x TG tile groups = the waves of a workgroup: wave (cb, j) keeps the split weights of column block cb in registers
// (12 KS of them) for its lifetime and multiplies the row tiles j TPW .. + TPW - 1 of every stage; a stage = TG TPW row tiles of 32
// pixels, loaded, split and stored once by all threads (one item of eight channels per thread and TPW / 2), two buffers, one barrier.
// Per accumulator the products are issued exactly as in k_expand1x1_bf16s: the outputs are the same bit for bit.
template <int NBLK, int KS, int TG, int TPW>
__global__ __launch_bounds__(64 * NBLK * TG, 5) void k_expand1x1_bf16s_ws(
    const float *__restrict__ src, int64_t rows, int sh, int sw, int crop_y, int crop_x, int h, int w, const float *__restrict__ wgt,
    const float *__restrict__ bias, int cout, float *__restrict__ dst, int dH, int dW, int dC, int off_y, int off_x, int c_off, FastDiv fhw,
    FastDiv fw)
{
    constexpr int CIN = 16 * KS, NT = 64 * NBLK * TG, TILES = TG * TPW, SP = 32 * TILES, IT = 2 * KS, IPT = SP * IT / NT;
    constexpr int PITCH = ExpandWsPitch<KS>::value, TILE_U = IT * 3 * PITCH, BUF_U = TILES * TILE_U;
    static_assert(SP * IT % NT == 0 && NT % IT == 0, "whole items per thread");
    extern __shared__ uint4 lds_ws[];              // split activations [2][TILES][IT][3][PITCH] x 16 bytes, then the bias padded to 32 NBLK
    float *lbias = (float *)(lds_ws + 2 * BUF_U);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int cb = wave % NBLK, tg = wave / NBLK, hw = h * w;
    const int px0 = tid / IT, it = tid % IT;          // staging: pixel px0 + u NT / IT of the stage, channels 8 it .. + 7
    const int64_t nstages = (rows + SP - 1) / SP, stride = gridDim.x;
    int64_t st = blockIdx.x;

    float4 raw[IPT][2];
    auto load_stage = [&](int64_t s_) {          // rows past the end repeat the last one
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            const unsigned m = (unsigned)s_ * (unsigned)SP + (unsigned)(px0 + u * (NT / IT));
            const unsigned mm = m < (unsigned)rows ? m : (unsigned)rows - 1u;
            const unsigned b = fhw.div(mm), rem = mm - b * (unsigned)hw;
            const unsigned y = fw.div(rem), x = rem - y * (unsigned)w;
            const float *p = src + (((int64_t)b * sh + crop_y + y) * sw + crop_x + x) * (int64_t)CIN + 8 * it;
            raw[u][0] = *(const float4 *)p; raw[u][1] = *(const float4 *)(p + 4);
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            const int px = px0 + u * (NT / IT);
            bf16x8 x1, x2, x3;
            split3(raw[u][0], raw[u][1], x1, x2, x3);
            uint4 *d = lds_ws + buf * BUF_U + (px >> 5) * TILE_U + it * 3 * PITCH + (px & 31);
            d[0] = __builtin_bit_cast(uint4, x1); d[PITCH] = __builtin_bit_cast(uint4, x2); d[2 * PITCH] = __builtin_bit_cast(uint4, x3);
        }
    };
    load_stage(st);          // the first stage's pixels leave before the weights (the grid has no more workgroups than stages)
    // ---- weights: the A operands of this wave's column block, all k-steps, split once (output channels past cout are zeros) ----
    bf16x8 wq[KS][3];
    {
        const int co = 32 * cb + r;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
            if (co < cout) {
                const float *q = wgt + (int64_t)co * CIN + 16 * s + 8 * hh;
                lo = *(const float4 *)q; hi = *(const float4 *)(q + 4);
            }
            split3(lo, hi, wq[s][0], wq[s][1], wq[s][2]);
        }
    }
    for (int i = tid; i < 32 * NBLK; i += NT) lbias[i] = i < cout ? bias[i] : 0.0f;
    store_stage(0);
    if (st + stride < nstages) load_stage(st + stride);
    __syncthreads();

    for (int buf = 0; st < nstages; st += stride, buf ^= 1) {
        // the next stage: split and stored into the buffer the stage before this one was read from (the barrier below lies between);
        // then the loads of the stage after it, a whole stage ahead of their use
        if (st + stride < nstages) {
            store_stage(buf ^ 1);
            if (st + 2 * stride < nstages) load_stage(st + 2 * stride);
        }
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const int tile = tg * TPW + u;
            const uint4 *xb = lds_ws + buf * BUF_U + tile * TILE_U + hh * 3 * PITCH + r;
            f16v acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 x1 = __builtin_bit_cast(bf16x8, xb[(2 * s) * 3 * PITCH]), x2 = __builtin_bit_cast(bf16x8, xb[(2 * s) * 3 * PITCH + PITCH]),
                             x3 = __builtin_bit_cast(bf16x8, xb[(2 * s) * 3 * PITCH + 2 * PITCH]);
                // smallest terms first
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s][0], x3, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s][1], x2, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s][2], x1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s][0], x2, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s][1], x1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s][0], x1, acc, 0, 0, 0);
            }
            // ---- bias + ReLU + placement: register quads = four consecutive output channels of the lane's pixel ----
            const unsigned m = (unsigned)st * (unsigned)SP + (unsigned)(32 * tile + r);
            if (m < (unsigned)rows) {
                const unsigned b = fhw.div(m), rem = m - b * (unsigned)hw;
                const unsigned y = fw.div(rem), x = rem - y * (unsigned)w;
                float *o = dst + (((int64_t)b * dH + off_y + y) * dW + off_x + x) * (int64_t)dC + c_off + 32 * cb + 4 * hh;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (32 * cb + 8 * g + 4 * hh < cout) store_bias_relu(o + 8 * g, acc, g, *(const float4 *)(lbias + 32 * cb + 8 * g + 4 * hh));
            }
        }
        __syncthreads();
    }
}

template <int NBLK, int KS, int TG, int TPW>
static int launch_expand_bf16s_ws(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int h, int w, const float *wgt, const float *bias,
                                  int cout, const Place &pl)
{
    constexpr int NWV = NBLK * TG, SP = 32 * TG * TPW;
    constexpr size_t lds = (size_t)2 * TG * TPW * 2 * KS * 3 * ExpandWsPitch<KS>::value * 16 + 32 * NBLK * sizeof(float);
    static_assert(lds <= 160 * 1024 - 256, "two stage buffers fit the LDS");
    static unsigned long long attr_mask = 0;
    if (!ensure_dyn_lds((const void *)k_expand1x1_bf16s_ws<NBLK, KS, TG, TPW>, 160 * 1024 - 256, attr_mask)) return SWK_ERR_HIP;
    if (rows > (int64_t)0x7fffff00) return SWK_ERR_CAPACITY;
    // persistent over the stages: as many workgroups per CU as their waves (five per SIMD: at most 96 registers, tests/
    // test_expand_ws_codegen.py) and their LDS allow
    const int64_t by_lds = (int64_t)((160 * 1024 - 256) / lds), by_waves = 20 / NWV;
    const int64_t cap = 256 * (by_lds < by_waves ? by_lds : by_waves);
    int64_t blocks = (rows + SP - 1) / SP;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((k_expand1x1_bf16s_ws<NBLK, KS, TG, TPW>), dim3((unsigned)blocks), dim3(64 * NWV), lds, s, src, rows, cr.sh, cr.sw, cr.crop_y,
                       cr.crop_x, h, w, wgt, bias, cout, pl.dst, pl.dH, pl.dW, pl.dC, pl.off_y, pl.off_x, pl.c_off, FastDiv((unsigned)(h * w)), FastDiv((unsigned)w));
    return hipGetLastError() == hipSuccess ? SWK_OK : SWK_ERR_HIP;
}

// the Fire shapes on the weight-stationary kernel.  From 65,536 rows (about a thousand segments) a workgroup takes several tile groups:
// 16 waves and one workgroup per CU (12 waves for 48 -> 192: three per SIMD; two workgroups of 8 for 16 -> 64), measured against the
// narrower layouts in DESIGN section 6 -- at 48 -> 192 three 6-wave workgroups per CU, which fill the SIMDs unevenly, ran no faster than
// the float32 kernel.  Below that one tile group per workgroup (stages of 64 pixels), which spreads a small launch over more CUs.
int launch_expand1x1_split_bf16_ws(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int cin, int h, int w, const float *wgt,
                                   const float *bias, int cout, const Place &pl)
{
    const bool small = rows < 65536;
#define SWK_WS(NBLK, KS, TG) (small ? launch_expand_bf16s_ws<NBLK, KS, 1, 2>(s, src, rows, cr, h, w, wgt, bias, cout, pl) \
                                    : launch_expand_bf16s_ws<NBLK, KS, TG, 2>(s, src, rows, cr, h, w, wgt, bias, cout, pl))
    if (cin == 16 && cout == 64) return SWK_WS(2, 1, 4);
    if (cin == 32 && cout == 128) return SWK_WS(4, 2, 4);
    if (cin == 48 && cout == 192) return SWK_WS(6, 3, 2);
    if (cin == 64 && cout == 256) return SWK_WS(8, 4, 2);
#undef SWK_WS
    return SWK_ERR_ARG;
}

// the Fire shapes (cout = 4 cin): SWK_ERR_ARG for anything else (the caller then takes the float32 kernel)
int launch_expand1x1_split_bf16(hipStream_t s, const float *src, int64_t rows, const Crop &cr, int cin, int h, int w, const float *wgt,
                                const float *bias, int cout, const Place &pl)
{
    if (cin == 16 && cout == 64) return launch_expand_bf16s<2, 1, 1, 8>(s, src, rows, cr, h, w, wgt, bias, cout, pl);
    if (cin == 32 && cout == 128) return launch_expand_bf16s<4, 2, 1, 8>(s, src, rows, cr, h, w, wgt, bias, cout, pl);
    if (cin == 48 && cout == 192) return launch_expand_bf16s<6, 3, 2, 8>(s, src, rows, cr, h, w, wgt, bias, cout, pl);
    if (cin == 64 && cout == 256) return launch_expand_bf16s<8, 4, 2, 8>(s, src, rows, cr, h, w, wgt, bias, cout, pl);
    return SWK_ERR_ARG;
}

}  // namespace swk
