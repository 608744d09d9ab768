// Stand-alone checker of the batch plan (swiftwatcher_amd/csrc/batch_plan.{h,cpp}): plan_batch and fill_batch_tables on designed and
// seeded random group mixes, held to invariants recomputed here the slow way -- no recorded numbers.  Built and run by
// tests/test_batch_plan_cpu.py with the address and undefined-behaviour sanitizers; exit status 0 = every invariant held.
// No pointer handed to the plan is ever dereferenced by it: frames and destinations are made-up addresses.
#include "batch_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <utility>
#include <vector>

using namespace swk;

namespace {

int g_failed = 0;
long g_cases = 0;
const char *g_case = "";

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            if (++g_failed <= 20) fprintf(stderr, "%s: line %d: %s\n", g_case, __LINE__, #cond);      \
        }                                                                                             \
    } while (0)

struct Spec {
    int H, W, nwin;
    int channels = 3;
    bool host_in = false, host_out = true;
    bool A = false, E = false;
    int cap = 7;              // 0: no segs
    bool nseg = true;
    int layout = 0;           // 0 dense, 1 margins (whole frames), 2 cropped rows, 3 wide frames (2-D copy), 4 margins, frames backwards
    bool fused = true;
};

uint8_t *fake(uint64_t a) { return (uint8_t *)(uintptr_t)a; }

swk_input make_input(const Spec &s, int n, int g)
{
    swk_input in{};
    in.frames = fake(0x100000000000ull + ((uint64_t)g << 36));
    in.mem = s.host_in ? SWK_MEM_HOST : SWK_MEM_DEVICE;
    in.channels = s.channels; in.nwin = s.nwin; in.n = n; in.Hc = s.H; in.Wc = s.W;
    const int64_t ch = s.channels;
    switch (s.layout) {
    case 0: in.row_stride = s.W * ch; in.frame_stride = s.H * in.row_stride; break;
    case 1: case 4:
        in.x0 = 3; in.y0 = 2; in.row_stride = (s.W + 5) * ch; in.frame_stride = (s.H + 4) * in.row_stride;
        if (s.layout == 4) { in.frames += (int64_t)(s.nwin * n - 1) * in.frame_stride; in.frame_stride = -in.frame_stride; }
        break;
    case 2: in.y0 = 5; in.row_stride = s.W * ch; in.frame_stride = (s.H + 40) * in.row_stride; break;
    default: in.x0 = 7; in.y0 = 1; in.row_stride = (4 * s.W + 64) * ch; in.frame_stride = (4 * s.H + 9) * in.row_stride; break;
    }
    return in;
}

swk_output make_output(const Spec &s, int g)
{
    swk_output o{};
    o.mem = s.host_out ? SWK_MEM_HOST : SWK_MEM_DEVICE;
    o.seg_cap = s.cap;
    const uint64_t base = 0x200000000000ull + ((uint64_t)g << 36);
    if (s.A) o.A = (double *)fake(base);
    if (s.E) o.E = (double *)fake(base + (1ull << 34));
    if (s.cap) o.segs = (swk_segment *)fake(base + (2ull << 34));
    if (s.nseg) o.nseg = (int32_t *)fake(base + (3ull << 34));
    return o;
}

// [first, end) intervals are pairwise disjoint
bool disjoint(std::vector<std::pair<uint64_t, uint64_t>> v)
{
    std::sort(v.begin(), v.end());
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i].first < v[i - 1].second) return false;
    return true;
}

void check_case(const char *name, int n, const std::vector<Spec> &specs)
{
    g_case = name;
    g_cases += 1;
    const int G = (int)specs.size();
    std::vector<swk_input> in(G);
    std::vector<swk_output> out(G);
    for (int g = 0; g < G; ++g) { in[g] = make_input(specs[g], n, g); out[g] = make_output(specs[g], g); }
    BatchPlan pl;
    const char *why = nullptr;
    const int rc = plan_batch(in.data(), G, out.data(), &pl, &why);
    CHECK(rc == SWK_OK && why == nullptr);
    if (rc != SWK_OK) return;

    // ---- sizes ----
    int nwin = 0, Pmax = 0, Hmax = 0, Wmax = 0;
    for (const Spec &s : specs) {
        nwin += s.nwin; Pmax = std::max(Pmax, s.H * s.W); Hmax = std::max(Hmax, s.H); Wmax = std::max(Wmax, s.W);
    }
    CHECK(pl.n == n && pl.nwin == nwin && pl.F == nwin * n && pl.single == (G == 1));
    CHECK(pl.Pmax == Pmax && pl.Hmax == Hmax && pl.Wmax == Wmax);
    CHECK((int)pl.grp.size() == G);
    if ((int)pl.grp.size() != G) return;

    // ---- sub-batch membership: every group in exactly one; all with P >= n share the first at the largest P; P < n alone at its own P ----
    std::vector<int> seen(G, 0);
    int big_max = 0, nbig = 0;
    for (const Spec &s : specs)
        if (s.H * s.W >= n) { big_max = std::max(big_max, s.H * s.W); nbig += 1; }
    CHECK(pl.subs.size() == (size_t)(nbig ? 1 : 0) + (size_t)(G - nbig));
    for (size_t k = 0; k < pl.subs.size(); ++k) {
        const BatchSub &sb = pl.subs[k];
        CHECK(!sb.gs.empty());
        int wins = 0;
        bool A = false, E = false;
        for (int g : sb.gs) {
            CHECK(g >= 0 && g < G);
            if (g < 0 || g >= G) return;
            seen[g] += 1;
            CHECK(pl.grp[g].sub == (int)k && pl.grp[g].pitch == sb.P);
            wins += specs[g].nwin;
            A = A || specs[g].A; E = E || specs[g].E;
            const int P = specs[g].H * specs[g].W;
            if (P >= n) CHECK(k == 0 && sb.P == big_max);
            else CHECK(sb.gs.size() == 1 && sb.P == P && (k > 0 || nbig == 0));
        }
        CHECK(std::is_sorted(sb.gs.begin(), sb.gs.end()));
        CHECK(sb.nwin == wins && sb.A == A && sb.E == E);
    }
    for (int g = 0; g < G; ++g) CHECK(seen[g] == 1);

    // ---- sub-batch offsets: multiples of 256, ascending, total = the end of the last; windows contiguous in sub-batch order ----
    int64_t end = 0;
    int w_next = 0;
    for (const BatchSub &sb : pl.subs) {
        CHECK(sb.off % 256 == 0 && sb.off >= end);
        CHECK(sb.off - end < 256);
        end = sb.off + (int64_t)sb.nwin * n * sb.P;
        CHECK(sb.w0 == w_next);
        w_next += sb.nwin;
    }
    CHECK(pl.total >= (size_t)end && pl.total - (size_t)end < 256 && pl.total % 256 == 0);
    CHECK(w_next == nwin);

    // ---- plane spans inside their sub-batch, pairwise disjoint; window order ----
    std::vector<std::pair<uint64_t, uint64_t>> spans, wspans;
    int win0 = 0;
    for (int g = 0; g < G; ++g) {
        const BatchGroup &bg = pl.grp[g];
        const BatchSub &sb = pl.subs[bg.sub];
        const int64_t len = (int64_t)specs[g].nwin * n * bg.pitch;
        CHECK(bg.goff >= sb.off && bg.goff + len <= sb.off + (int64_t)sb.nwin * n * sb.P);
        CHECK((bg.goff - sb.off) % ((int64_t)n * sb.P) == 0);
        spans.push_back({(uint64_t)bg.goff, (uint64_t)(bg.goff + len)});
        CHECK(bg.win0 == win0);
        win0 += specs[g].nwin;
        CHECK(bg.swin0 >= sb.w0 && bg.swin0 + specs[g].nwin <= sb.w0 + sb.nwin);
        CHECK(bg.goff == sb.off + (int64_t)(bg.swin0 - sb.w0) * n * sb.P);
        wspans.push_back({(uint64_t)bg.swin0, (uint64_t)(bg.swin0 + specs[g].nwin)});
    }
    CHECK(disjoint(spans));
    CHECK(disjoint(wspans));          // with w_next == nwin above: one-to-one onto 0 .. nwin - 1
    for (const BatchSub &sb : pl.subs)          // members keep the call's order inside their sub-batch
        for (size_t i = 1; i < sb.gs.size(); ++i) CHECK(pl.grp[sb.gs[i]].swin0 == pl.grp[sb.gs[i - 1]].swin0 + specs[sb.gs[i - 1]].nwin);

    // ---- vec: the widest of 4, 2, 1 that divides every group's P, pitch and goff ----
    int vec = 1;
    for (int v : {2, 4}) {
        bool all = true;
        for (int g = 0; g < G; ++g) all = all && (specs[g].H * specs[g].W) % v == 0 && pl.grp[g].pitch % v == 0 && pl.grp[g].goff % v == 0;
        if (all) vec = v;
    }
    CHECK(pl.vec == vec);

    // ---- staging offsets ----
    std::vector<std::pair<uint64_t, uint64_t>> rspans, pspans;
    for (int g = 0; g < G; ++g) {
        const BatchGroup &bg = pl.grp[g];
        const size_t dense = (size_t)specs[g].nwin * n * specs[g].H * specs[g].W * specs[g].channels;
        if (specs[g].host_in) {
            const int kind = bg.stage.kind;
            // make_input's layouts: whole frames are copied where they are at most twice the ROI's bytes (3: never)
            const int64_t afs = in[g].frame_stride < 0 ? -in[g].frame_stride : in[g].frame_stride;
            const size_t whole_bytes = (size_t)specs[g].nwin * n * (size_t)afs;
            const int lay = specs[g].layout;
            const bool whole = lay != 0 && lay != 3 && whole_bytes <= 2 * dense;
            CHECK(kind == (lay == 0 ? ST_DENSE : whole ? ST_WHOLE : lay == 2 ? ST_ROWS : ST_2D));
            CHECK(bg.stage.bytes == (kind == ST_WHOLE ? whole_bytes : dense));
            CHECK(bg.stage.bytes >= dense);
            CHECK(bg.roi_off % 256 == 0 && bg.roi_off + bg.stage.bytes <= pl.roi_bytes);
            rspans.push_back({bg.roi_off, bg.roi_off + bg.stage.bytes});
        } else CHECK(bg.stage.kind == -1);
        if ((specs[g].A || specs[g].E) && specs[g].host_out) {
            const size_t bytes = dense / specs[g].channels * 8;
            CHECK(bg.pn_off % 8 == 0 && bg.pn_off + bytes <= pl.pn_bytes);
            pspans.push_back({bg.pn_off, bg.pn_off + bytes});
        }
    }
    CHECK(disjoint(rspans) && disjoint(pspans));
    if (rspans.empty()) CHECK(pl.roi_bytes == 0);
    if (pspans.empty()) CHECK(pl.pn_bytes == 0);

    // ---- record flags, by their definitions ----
    int capmax = 1;
    bool want_props = false, seg_last = true, host_total = true;
    for (const Spec &s : specs) {
        if (s.cap || s.nseg) want_props = true;
        if (s.cap > capmax) capmax = s.cap;
        if (!s.cap || s.channels != 3) seg_last = false;
        if (!s.host_out || !s.nseg) host_total = false;
    }
    CHECK(pl.capmax == capmax && pl.want_props == want_props && pl.seg_last == seg_last && pl.host_total == host_total);

    // ---- tables: no one overlaps the next; tab_bytes is the end of the last ----
    const size_t F = (size_t)nwin * n;
    CHECK(pl.o_win == 0 && pl.o_win + (size_t)nwin * sizeof(GroupWin) <= pl.o_gf);
    CHECK(pl.o_gf + F * sizeof(FrameGeom) <= pl.o_gc && pl.o_gc + F * sizeof(FrameGeom) <= pl.o_sf);
    CHECK(pl.o_sf + F * sizeof(SegFrame) <= pl.o_pa && pl.o_pa + (size_t)nwin * sizeof(PnWin) <= pl.o_pe);
    CHECK(pl.tab_bytes == pl.o_pe + (size_t)nwin * sizeof(PnWin));
    CHECK(pl.o_gf % 8 == 0 && pl.o_gc % 8 == 0 && pl.o_sf % 8 == 0 && pl.o_pa % 8 == 0 && pl.o_pe % 8 == 0);

    // ---- the tables' contents: device views (a host group: dense in its part of the ROI buffer), destinations, labeller flags ----
    std::vector<BatchView> view(G);
    std::vector<BatchAE> ae(G);
    std::vector<char> fused(G);
    for (int g = 0; g < G; ++g) {
        view[g] = {in[g].frames, in[g].frame_stride, in[g].row_stride, in[g].x0, in[g].y0};
        if (specs[g].host_in) {
            const int64_t rs = (int64_t)specs[g].W * specs[g].channels;
            view[g] = {fake(0x300000000000ull + pl.grp[g].roi_off), specs[g].H * rs, rs, 0, 0};
        }
        double *pn = (double *)fake(0x400000000000ull + pl.grp[g].pn_off);
        ae[g].A = !specs[g].A ? nullptr : specs[g].host_out ? pn : out[g].A;
        ae[g].E = !specs[g].E ? nullptr : specs[g].host_out ? pn : out[g].E;
        fused[g] = specs[g].fused;
    }
    std::vector<uint8_t> tab(pl.tab_bytes, 0);          // (exactly tab_bytes: a write past the end is the sanitizer's)
    fill_batch_tables(pl, in.data(), out.data(), view.data(), ae.data(), fused.data(), tab.data());
    std::vector<GroupWin> hwin(nwin);
    std::vector<FrameGeom> hgf(F), hgc(F);
    std::vector<SegFrame> hsf(F);
    std::vector<PnWin> hpa(nwin), hpe(nwin);
    memcpy(hwin.data(), tab.data() + pl.o_win, nwin * sizeof(GroupWin));
    memcpy(hgf.data(), tab.data() + pl.o_gf, F * sizeof(FrameGeom));
    memcpy(hgc.data(), tab.data() + pl.o_gc, F * sizeof(FrameGeom));
    memcpy(hsf.data(), tab.data() + pl.o_sf, F * sizeof(SegFrame));
    memcpy(hpa.data(), tab.data() + pl.o_pa, nwin * sizeof(PnWin));
    memcpy(hpe.data(), tab.data() + pl.o_pe, nwin * sizeof(PnWin));
    for (int g = 0; g < G; ++g) {
        const BatchGroup &bg = pl.grp[g];
        const BatchView &v = view[g];
        const int H = specs[g].H, W = specs[g].W, P = H * W;
        const int64_t afs = v.fs < 0 ? -v.fs : v.fs;
        for (int wl = 0; wl < specs[g].nwin; ++wl) {
            const int w = bg.win0 + wl, ws = bg.swin0 + wl;
            const GroupWin &d = hwin[w];
            CHECK(d.src == v.frames + (int64_t)wl * n * v.fs && d.fs == v.fs && d.rs == v.rs && d.x0 == v.x0 && d.y0 == v.y0);
            CHECK(d.H == H && d.W == W && d.channels == specs[g].channels && d.pitch == bg.pitch);
            CHECK(d.off == bg.goff + (int64_t)wl * n * bg.pitch);
            CHECK(d.off == hgf[(size_t)w * n].off);
            CHECK(hpa[ws].P == P && hpe[ws].P == P);
            CHECK(hpa[ws].dst == (ae[g].A ? ae[g].A + (size_t)wl * n * P : nullptr));
            CHECK(hpe[ws].dst == (ae[g].E ? ae[g].E + (size_t)wl * n * P : nullptr));
            for (int j = 0; j < n; ++j) {
                const size_t f = (size_t)w * n + j;
                CHECK(hgf[f].H == H && hgf[f].W == W && hgf[f].off == d.off + (int64_t)j * bg.pitch);
                if (specs[g].fused) CHECK(hgc[f].H == H && hgc[f].W == W && hgc[f].off == hgf[f].off);
                else CHECK(hgc[f].H == 0 && hgc[f].W == 0 && hgc[f].off == 0);
                const SegFrame &sf = hsf[f];
                CHECK(sf.frame == v.frames + ((int64_t)wl * n + j) * v.fs && sf.rs == v.rs && sf.x0 == v.x0 && sf.y0 == v.y0);
                CHECK(sf.frame_h == (int)(afs / v.rs) && sf.frame_w == (int)(v.rs / 3));
                CHECK(sf.cap == (specs[g].cap ? specs[g].cap : 1));
            }
        }
    }
}

// ---- refusals: code and exact message, the first one that applies in the order plan_batch lists them ----
void check_refusal(const char *name, int n, std::vector<Spec> specs, void (*spoil)(std::vector<swk_input> &, std::vector<swk_output> &),
                   const char *message)
{
    g_case = name;
    g_cases += 1;
    const int G = (int)specs.size();
    std::vector<swk_input> in(G);
    std::vector<swk_output> out(G);
    for (int g = 0; g < G; ++g) { in[g] = make_input(specs[g], n, g); out[g] = make_output(specs[g], g); }
    spoil(in, out);
    BatchPlan pl;
    const char *why = nullptr;
    const int rc = plan_batch(in.data(), G, out.data(), &pl, &why);
    CHECK(rc == SWK_ERR_ARG);
    CHECK(why && !strcmp(why, message));
}

Spec spec(int H, int W, int nwin) { Spec s{}; s.H = H; s.W = W; s.nwin = nwin; return s; }

void designed()
{
    // the labeller's word width, as the GPU tests' ids say (n = 21)
    { std::vector<Spec> m = {spec(64, 96, 1), spec(32, 40, 2), spec(48, 64, 1)};
      check_case("vec4", 21, m);
      BatchPlan pl; const char *why; std::vector<swk_input> in; std::vector<swk_output> out;
      for (int g = 0; g < 3; ++g) { in.push_back(make_input(m[g], 21, g)); out.push_back(make_output(m[g], g)); }
      g_case = "vec4 value";
      CHECK(plan_batch(in.data(), 3, out.data(), &pl, &why) == SWK_OK && pl.vec == 4); }
    { std::vector<Spec> m = {spec(64, 96, 1), spec(33, 47, 2)};
      check_case("vec1", 21, m);
      BatchPlan pl; const char *why; std::vector<swk_input> in; std::vector<swk_output> out;
      for (int g = 0; g < 2; ++g) { in.push_back(make_input(m[g], 21, g)); out.push_back(make_output(m[g], g)); }
      g_case = "vec1 value";
      CHECK(plan_batch(in.data(), 2, out.data(), &pl, &why) == SWK_OK && pl.vec == 1); }
    // the boundary P = n and the groups below it
    check_case("P = n at 64", 64, {spec(64, 96, 1), spec(8, 8, 2), spec(7, 9, 1), spec(32, 40, 3)});
    check_case("below n first", 64, {spec(7, 9, 2), spec(8, 8, 1)});
    check_case("all below n", 21, {spec(4, 4, 1), spec(4, 5, 2)});
    check_case("three below n", 21, {spec(4, 5, 3), spec(4, 4, 1), spec(5, 4, 2)});
    check_case("below n between", 21, {spec(33, 47, 1), spec(4, 4, 2), spec(64, 96, 1), spec(4, 5, 1), spec(32, 40, 2)});
    check_case("wide window", 128, {spec(64, 96, 1), spec(8, 8, 1), spec(33, 47, 2)});
    check_case("short window", 7, {spec(4, 4, 3), spec(33, 47, 1)});
    // one group: the degenerate plan
    for (int n : {7, 21, 64, 128})
        for (int nw = 1; nw <= 3; ++nw) {
            check_case("one group", n, {spec(33, 47, nw)});
            check_case("one small group", n, {spec(4, 4, nw)});
        }
    // memory kinds, channels, staging routes, records and A / E mixed
    { std::vector<Spec> m = {spec(64, 96, 2), spec(32, 40, 1), spec(4, 5, 3), spec(33, 47, 1), spec(8, 8, 2)};
      m[0].host_in = true; m[0].layout = 1; m[0].A = true;
      m[1].host_in = true; m[1].layout = 3; m[1].E = true; m[1].host_out = false; m[1].cap = 255;
      m[2].host_in = true; m[2].layout = 2; m[2].A = m[2].E = true; m[2].channels = 1; m[2].cap = 1;
      m[3].layout = 4; m[3].cap = 0; m[3].nseg = false; m[3].fused = false;
      m[4].host_in = true; m[4].layout = 4; m[4].E = true; m[4].fused = false;
      check_case("mixed", 21, m);
      check_case("mixed at 64", 64, m); }
}

void random_cases(unsigned seed, int count)
{
    std::mt19937 rng(seed);
    auto pick = [&](int k) { return (int)(rng() % (unsigned)k); };
    const int ns[4] = {7, 21, 64, 128};
    const int rois[8][2] = {{64, 96}, {32, 40}, {33, 47}, {8, 8}, {7, 9}, {4, 5}, {4, 4}, {48, 64}};
    const int caps[4] = {0, 1, 7, 255};
    char name[64];
    for (int c = 0; c < count; ++c) {
        const int n = ns[pick(4)], G = 1 + pick(6);
        std::vector<Spec> m;
        for (int g = 0; g < G; ++g) {
            const int *r = rois[pick(8)];
            Spec s = spec(r[0], r[1], 1 + pick(3));
            s.channels = pick(4) ? 3 : 1;
            s.host_in = pick(2); s.host_out = pick(2);
            s.A = pick(3) == 0; s.E = pick(3) == 0;
            s.cap = caps[pick(4)]; s.nseg = pick(4) != 0;
            s.layout = pick(5);
            s.fused = pick(3) != 0;
            m.push_back(s);
        }
        snprintf(name, sizeof name, "random %u/%d", seed, c);
        check_case(name, n, m);
    }
}

void refusals()
{
    const std::vector<Spec> two = {spec(64, 96, 1), spec(32, 40, 2)};
    using In = std::vector<swk_input>; using Out = std::vector<swk_output>;
    check_refusal("null frames", 21, two, [](In &i, Out &) { i[1].frames = nullptr; }, "null frames");
    check_refusal("no windows", 21, two, [](In &i, Out &) { i[1].nwin = 0; }, "empty batch");
    check_refusal("no frames", 21, two, [](In &i, Out &) { i[0].n = 0; i[1].n = 0; }, "empty batch");
    check_refusal("no rows", 21, two, [](In &i, Out &) { i[0].Hc = 0; }, "empty batch");
    check_refusal("differing n", 21, two, [](In &i, Out &) { i[1].n = 22; }, "every group must have the same frames per window");
    check_refusal("two channels", 21, two, [](In &i, Out &) { i[1].channels = 2; }, "channels must be 1 or 3");
    check_refusal("129 frames", 129, two, [](In &, Out &) {}, "frames per window must be <= 128");
    check_refusal("cap 0", 21, two, [](In &, Out &o) { o[1].seg_cap = 0; }, "seg_cap must be in 1..255");
    check_refusal("cap 256", 21, two, [](In &, Out &o) { o[0].seg_cap = 256; }, "seg_cap must be in 1..255");
    check_refusal("3 x 96", 21, two, [](In &i, Out &) { i[1].Hc = 3; }, "ROI must be at least 4x4");
    check_refusal("64 x 3", 21, two, [](In &i, Out &) { i[0].Wc = 3; }, "ROI must be at least 4x4");
    check_refusal("2^24 frames + 1 window", 128, two, [](In &i, Out &) { i[0].nwin = (1 << 17) - 1; }, "too many frames in one call");
    // a cap nobody reads is not refused; 2^24 frames exactly pass
    g_case = "unread cap";
    { In i = {make_input(two[0], 21, 0)}; Out o = {make_output(two[0], 0)};
      o[0].segs = nullptr; o[0].seg_cap = 0;
      BatchPlan pl; const char *why = nullptr;
      CHECK(plan_batch(i.data(), 1, o.data(), &pl, &why) == SWK_OK && pl.capmax == 1); }
    g_case = "2^24 frames";
    { In i = {make_input(spec(4, 4, 1 << 17), 128, 0)}; Out o = {make_output(two[0], 0)};
      BatchPlan pl; const char *why = nullptr;
      CHECK(plan_batch(i.data(), 1, o.data(), &pl, &why) == SWK_OK && pl.F == 1 << 24); }
}

}  // namespace

int main()
{
    designed();
    refusals();
    for (unsigned seed = 1; seed <= 4; ++seed) random_cases(seed, 750);
    if (g_failed) { fprintf(stderr, "batch_plan_check: %d checks failed in %ld cases\n", g_failed, g_cases); return 1; }
    printf("batch_plan_check: %ld cases passed\n", g_cases);
    return 0;
}
