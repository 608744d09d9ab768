// Deinterlacing on gfx950: one field of an interlaced frame -> a whole picture (swk_yuv_deinterlace, include/swk.h).  Every component
// plane (Y, U, V) is processed on its own: the rows of the kept field are copied, every other row is an edge-directed average of the
// rows above and below it in the same frame (five directions, exact integers), clamped around the temporal mean by the largest
// change the neighbouring frames show, so that a still scene comes out as it was stored.
//
// k_deint_plane<T> makes one plane of a scratch planar picture stack [nout][ph][pw] of LSB-aligned samples, which launch_yuv_to_bgr
// (yuv.hip) then converts.  A byte-streaming kernel without reuse inside a thread beyond its own footprint: one thread makes four
// adjacent samples of one row.  Of a kept row it moves one dword (uint8_t) or two (uint16_t) where the addresses allow it.  Of a
// missing row it reads the ten samples x - 3 .. x + 6 of the rows above and below -- from the aligned dwords that hold them, shifted
// into place with v_alignbyte_b32 -- and, for the temporal clamp, the four samples of the same three rows in the neighbouring frames;
// neighbouring threads read overlapping spans, which the caches serve, so no LDS is used.  Next to a plane border, in the ragged
// last group of a row and for interleaved chroma (sample step 2) the samples are read one by one with clamped column numbers.
//
// Pictures do not meet a grid's y or z extent: the 1-D grid holds (groups of one picture) x (as many pictures as keep it below
// 2^22 blocks), and every block strides over the pictures from there with 64-bit offsets.
#include "swk_internal.h"

namespace swk {

#if defined(SWK_DEINT_HOST_CHECK)
std::atomic<int> g_launch_error{0};          // (swk_api.hip's, which the host check is built without)
#endif

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#else
inline uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * sh)); }
#endif

__host__ __device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// samples x .. x + 3 of a row (n of them exist and are read), all inside the plane
template <typename T> __host__ __device__ __forceinline__ void load4(const T *row, int x, int n, int step, int msb, int (&e)[4])
{
    const T *p = row + (int64_t)x * step;
    if (step == 1 && n == 4 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t w = *(const uint32_t *)p;
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = (int)((w >> (8 * k)) & 255u);
        } else {
            const uint2 w = *(const uint2 *)p;
            e[0] = (int)(w.x & 65535u) >> msb; e[1] = (int)(w.x >> 16) >> msb;
            e[2] = (int)(w.y & 65535u) >> msb; e[3] = (int)(w.y >> 16) >> msb;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = k < n ? (int)p[(int64_t)k * step] >> msb : 0;
    }
}

// e[i] = sample min(max(x - 3 + i, 0), hi) of a row, i = 0 .. 9 (`row` points at the plane's column 0; hi <= the last column that may
// be read).  Where all ten columns exist and lie side by side: the aligned dwords that hold them, shifted into place.  The first
// and the last of those dwords may begin up to 3 bytes before the first sample and end up to 3 bytes after the last one: bytes
// outside the described plane where its rows are not dword-aligned.  They are read and shifted out, never used.  The read cannot
// fault, because each dword also holds a sample of the plane and an aligned dword never crosses a page; it is a read outside the
// caller's object all the same, which is why the host check (below) hands this code buffers with four spare bytes on either side.
template <typename T> __host__ __device__ __forceinline__ void load10(const T *row, int x, int hi, int step, int msb, int (&e)[10])
{
    if (step == 1 && x >= 3 && x + 6 <= hi) {
        constexpr int NB = 10 * (int)sizeof(T), ND = (NB + 3) / 4;           // bytes wanted, dwords that hold them once aligned
        const uintptr_t a = (uintptr_t)(row + (x - 3));
        const uint32_t off = (uint32_t)(a & 3);
        const uint32_t *wp = (const uint32_t *)(a - off);
        uint32_t w[ND + 1], d[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) w[i] = wp[i];
        w[ND] = off + NB > 4 * ND ? wp[ND] : 0u;                             // (the ten samples reach into one more dword)
#pragma unroll
        for (int i = 0; i < ND; ++i) d[i] = align_bytes(w[i + 1], w[i], off);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            if constexpr (sizeof(T) == 1) e[i] = (int)((d[i >> 2] >> (8 * (i & 3))) & 255u);
            else e[i] = (int)((d[i >> 1] >> (16 * (i & 1))) & 65535u) >> msb;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            int c = x - 3 + i;
            c = c < 0 ? 0 : (c > hi ? hi : c);
            e[i] = (int)row[(int64_t)c * step] >> msb;
        }
    }
}

template <typename T> __host__ __device__ __forceinline__ void store4(T *p, int n, const int (&v)[4])
{
    if (n == 4 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 1) {
            *(uint32_t *)p = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
            uint2 w;
            w.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16);
            w.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
            *(uint2 *)p = w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = (T)v[k];
    }
}

}  // namespace

// Samples c .. c + 3 (n of them) of row r of the rectangle, in output picture o: the definition of include/swk.h, restated.
template <typename T> __host__ __device__ __forceinline__ void deint_quad(const DeintPlane &p, const DeintJob &j, int o, int r, int c, int n)
{
    const int t = j.first + (j.rate == 2 ? o >> 1 : o);                     // the stored frame, among the `count` described ones
    const int second = j.rate == 2 ? o & 1 : 0;                             // the frame's second field in time
    const int keep = j.tff ? second : 1 - second;                           // the parity of the rows this picture keeps
    const int y = p.py0 + r, x = p.px0 + c;
    const uint8_t *cur = p.src + (int64_t)t * p.fs;
    // (row yy of a frame, from the plane's column 0; the described or staged samples start at row oy, column ox)
    auto rowp = [&](const uint8_t *frame, int yy) { return (const T *)(frame + (int64_t)(yy - p.oy) * p.rs) - (int64_t)p.ox * p.step; };
    int out[4];
    if (p.PH == 1 || ((y + p.parity0) & 1) == keep) {
        load4<T>(rowp(cur, y), x, n, p.step, p.msb, out);
    } else {
        const int up = y > 0 ? y - 1 : y + 1, dn = y < p.PH - 1 ? y + 1 : y - 1;
        const int last = p.PW - 1;
        const int hi = x + n + 2 < last ? x + n + 2 : last;                 // the last column the footprint of these n samples holds
        int U[10], D[10];
        load10<T>(rowp(cur, up), x, hi, p.step, p.msb, U);
        load10<T>(rowp(cur, dn), x, hi, p.step, p.msb, D);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = k + 3, xx = x + k;                                // U[i], D[i]: column xx
            const int cc = U[i], ee = D[i];
            int score = iabs(U[i - 1] - D[i - 1]) + iabs(cc - ee) + iabs(U[i + 1] - D[i + 1]) - 1;
            int pred = (cc + ee) >> 1;
            const bool adm1 = xx - 2 >= 0 && xx + 2 <= last, adm2 = xx - 3 >= 0 && xx + 3 <= last;
            // direction j pairs column xx + j above with column xx - j below
            const int sm1 = iabs(U[i - 2] - D[i]) + iabs(U[i - 1] - D[i + 1]) + iabs(U[i] - D[i + 2]);
            if (adm1 && sm1 < score) {
                score = sm1; pred = (U[i - 1] + D[i + 1]) >> 1;
                const int sm2 = iabs(U[i - 3] - D[i + 1]) + iabs(U[i - 2] - D[i + 2]) + iabs(U[i - 1] - D[i + 3]);
                if (adm2 && sm2 < score) { score = sm2; pred = (U[i - 2] + D[i + 2]) >> 1; }
            }
            const int sp1 = iabs(U[i] - D[i - 2]) + iabs(U[i + 1] - D[i - 1]) + iabs(U[i + 2] - D[i]);
            if (adm1 && sp1 < score) {
                score = sp1; pred = (U[i + 1] + D[i - 1]) >> 1;
                const int sp2 = iabs(U[i + 1] - D[i - 3]) + iabs(U[i + 2] - D[i - 2]) + iabs(U[i + 3] - D[i - 1]);
                if (adm2 && sp2 < score) { score = sp2; pred = (U[i + 2] + D[i - 2]) >> 1; }
            }
            out[k] = pred;
        }
        if (j.temporal) {
            const uint8_t *pv = p.src + (int64_t)(t > 0 ? t - 1 : t) * p.fs, *nx = p.src + (int64_t)(t < j.count - 1 ? t + 1 : t) * p.fs;
            int bq[4], aq[4], pu[4], pd[4], nu[4], nd[4];
            load4<T>(rowp(second ? cur : pv, y), x, n, p.step, p.msb, bq);
            load4<T>(rowp(second ? nx : cur, y), x, n, p.step, p.msb, aq);
            load4<T>(rowp(pv, up), x, n, p.step, p.msb, pu);
            load4<T>(rowp(pv, dn), x, n, p.step, p.msb, pd);
            load4<T>(rowp(nx, up), x, n, p.step, p.msb, nu);
            load4<T>(rowp(nx, dn), x, n, p.step, p.msb, nd);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cc = U[k + 3], ee = D[k + 3];
                const int dm = (bq[k] + aq[k]) >> 1;
                const int td0 = iabs(bq[k] - aq[k]) >> 1;
                const int td1 = (iabs(pu[k] - cc) + iabs(pd[k] - ee)) >> 1;
                const int td2 = (iabs(nu[k] - cc) + iabs(nd[k] - ee)) >> 1;
                int diff = td0 > td1 ? td0 : td1;
                diff = diff > td2 ? diff : td2;
                const int lo = dm - diff, hh = dm + diff;
                int v = out[k] > lo ? out[k] : lo;
                out[k] = v < hh ? v : hh;
            }
        }
    }
    store4<T>((T *)p.dst + ((int64_t)o * p.ph + r) * p.pw + c, n, out);
}

template <typename T> __global__ __launch_bounds__(256) void k_deint_plane(DeintPlane p, DeintJob j, int gblocks)
{
    const int wq = (p.pw + 3) >> 2;
    const int o0 = blockIdx.x / gblocks, opar = gridDim.x / gblocks;        // (wave-uniform)
    const int g = (blockIdx.x - o0 * gblocks) * 256 + threadIdx.x;
    if (g >= p.ph * wq) return;
    const int r = g / wq, c = (g - r * wq) << 2;
    const int n = p.pw - c < 4 ? p.pw - c : 4;
    for (int o = o0; o < j.nout; o += opar) deint_quad<T>(p, j, o, r, c, n);
}

void launch_deint_plane(hipStream_t s, const DeintPlane &p, const DeintJob &j, int wide)
{
    const int groups = p.ph * ((p.pw + 3) >> 2);                            // <= 32768 * 8192 = 2^28
    const int gblocks = (groups + 255) / 256;                               // <= 2^20
    int opar = (1 << 22) / gblocks;                                         // pictures side by side in the grid; the rest by stride
    opar = opar < 1 ? 1 : (opar > j.nout ? j.nout : opar);
    const dim3 grid((unsigned)gblocks * (unsigned)opar);
    if (wide) hipLaunchKernelGGL(k_deint_plane<uint16_t>, grid, dim3(256), 0, s, p, j, gblocks);
    else hipLaunchKernelGGL(k_deint_plane<uint8_t>, grid, dim3(256), 0, s, p, j, gblocks);
    note_launch();
}

#if defined(SWK_DEINT_HOST_CHECK)
// The layout of DeintPlane and DeintJob as compiled: sizes, then the offset of every member in declaration order.  The test mirrors
// both structs in ctypes (tests/deinterlace_host.py) and compares before it calls anything.  Returns the number of entries.
extern "C" __attribute__((visibility("default"))) int swk_deint_layout(int *out, int cap)
{
    const int v[] = {(int)sizeof(DeintPlane), (int)sizeof(DeintJob),
                     (int)offsetof(DeintPlane, src), (int)offsetof(DeintPlane, fs), (int)offsetof(DeintPlane, rs), (int)offsetof(DeintPlane, step),
                     (int)offsetof(DeintPlane, oy), (int)offsetof(DeintPlane, ox), (int)offsetof(DeintPlane, PH), (int)offsetof(DeintPlane, PW),
                     (int)offsetof(DeintPlane, py0), (int)offsetof(DeintPlane, px0), (int)offsetof(DeintPlane, ph), (int)offsetof(DeintPlane, pw),
                     (int)offsetof(DeintPlane, parity0), (int)offsetof(DeintPlane, msb), (int)offsetof(DeintPlane, dst),
                     (int)offsetof(DeintJob, count), (int)offsetof(DeintJob, first), (int)offsetof(DeintJob, nout), (int)offsetof(DeintJob, rate),
                     (int)offsetof(DeintJob, tff), (int)offsetof(DeintJob, temporal)};
    const int n = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

// The same code on the host, sample group by sample group (tests build this file alone with the macro set).
extern "C" __attribute__((visibility("default"))) void swk_deint_plane_host(const DeintPlane *p, const DeintJob *j, int wide)
{
    const int wq = (p->pw + 3) >> 2;
    for (int o = 0; o < j->nout; ++o)
        for (int r = 0; r < p->ph; ++r)
            for (int q = 0; q < wq; ++q) {
                const int c = q << 2, n = p->pw - c < 4 ? p->pw - c : 4;
                if (wide) deint_quad<uint16_t>(*p, *j, o, r, c, n);
                else deint_quad<uint8_t>(*p, *j, o, r, c, n);
            }
}
#endif

}  // namespace swk
