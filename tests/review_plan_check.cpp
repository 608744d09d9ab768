// Stand-alone checker of the review plan (swiftwatcher_amd/csrc/review_plan.{h,cpp}): plan_review on designed and seeded random calls,
// held to what include/swk.h and swk_internal.h say a plan and its table must hold, restated here the slow way -- no recorded
// numbers, and no expectation made by calling the plan.  Built and run by tests/test_review_plan_cpu.py with the address and
// undefined-behaviour sanitizers; it stops with exit status 1 at the first invariant that does not hold.
// Source frames, panel planes and destination planes are one poisoned byte each: the plan may test these pointers, never follow them.
#include "review_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <random>
#include <string>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

using namespace swk;

namespace {

std::string g_case;
long g_cases = 0;

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "%s: line %d: %s\n", g_case.c_str(), __LINE__, #cond);           \
            exit(1);                                                                         \
        }                                                                                    \
    } while (0)

uint8_t *forbidden()
{
    uint8_t *p = (uint8_t *)malloc(1);
    ASAN_POISON_MEMORY_REGION(p, 1);
    return p;
}
uint8_t *const g_frames = forbidden(), *const g_plane = forbidden(), *const g_y = forbidden(), *const g_u = forbidden(),
               *const g_v = forbidden();

// A call with its own storage (Call); wire() makes the arguments of it, pointers set the way a caller would.
struct Args {
    swk_input in; swk_review rv; swk_yuv420_dst dst;
    const swk_input *pin; const swk_review *prv; const swk_review_label *labels; int nlabels; const swk_yuv420_dst *pdst;
    const swk_review_panel *panels; int npanels, cols;
};
struct Call {
    swk_input in{};
    swk_yuv420_dst dst{};
    bool has_rv = true, has_fstyle = false, has_mask = false;
    int mask_style = 0, mark_arm = 2, border = 1;
    std::vector<swk_review_style> styles;
    std::vector<swk_review_box> boxes;
    std::vector<swk_review_mark> marks;
    std::vector<int32_t> fstyle;
    std::vector<uint8_t> mask;
    std::vector<swk_review_label> labels;
    std::vector<swk_review_panel> panels;
    int cols = 0;
    int F() const { return in.nwin * in.n; }
};

template <class T> const T *data_or_null(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

// `a` must stay where it is while the plan runs: it points into itself
void wire(const Call &c, Args &a)
{
    a.in = c.in; a.dst = c.dst;
    a.rv = swk_review{};
    a.rv.mask = c.has_mask ? c.mask.data() : nullptr; a.rv.mask_style = c.mask_style;
    a.rv.boxes = data_or_null(c.boxes); a.rv.nboxes = (int)c.boxes.size();
    a.rv.marks = data_or_null(c.marks); a.rv.nmarks = (int)c.marks.size();
    a.rv.mark_arm = c.mark_arm; a.rv.border = c.border;
    a.rv.frame_style = c.has_fstyle ? c.fstyle.data() : nullptr;
    a.rv.styles = data_or_null(c.styles); a.rv.nstyles = (int)c.styles.size();
    a.pin = &a.in; a.prv = c.has_rv ? &a.rv : nullptr; a.pdst = &a.dst;
    a.labels = data_or_null(c.labels); a.nlabels = (int)c.labels.size();
    a.panels = data_or_null(c.panels); a.npanels = (int)c.panels.size(); a.cols = c.cols;
}

int run(const Args &a, ReviewPlan *pl, const char **why)
{
    return plan_review(a.pin, a.prv, a.labels, a.nlabels, a.pdst, a.panels, a.npanels, a.cols, pl, why);
}

int even(int x) { return x % 2 ? x + 1 : x; }
int half_up(int x) { return x / 2 + x % 2; }
// b is the smallest multiple of 16 that holds `bytes`
bool is_round16(size_t b, size_t bytes) { return b % 16 == 0 && b >= bytes && b - bytes < 16; }

swk_review_label make_label(int frame, int r, int c, int style, int plate, int scale, const char *text)
{
    swk_review_label l{};
    l.frame = frame; l.r = r; l.c = c; l.style = style; l.plate = plate; l.scale = scale; l.len = (int)strlen(text);
    memset(l.text, 0xEE, sizeof l.text);                  // bytes past len are not the plan's business
    memcpy(l.text, text, (size_t)l.len);
    return l;
}

swk_review_panel make_panel(int kind, int gain, int layers, int Wc, bool host, const swk_review_label &caption)
{
    swk_review_panel p{};
    p.plane = g_plane; p.mem = host ? SWK_MEM_HOST : SWK_MEM_DEVICE; p.kind = kind; p.gain = gain; p.layers = layers;
    p.row_stride = Wc; p.frame_stride = -1000; p.caption = caption;
    return p;
}

// a dense destination for the call's geometry (include/swk.h: rows = ceil((1 + npanels) / cols) cells of Hp x Wp)
void fit_dst(Call &c, int layout, bool host)
{
    int Wd = c.in.Wc;
    if (c.cols) Wd = c.cols * even(c.in.Wc);
    c.dst = swk_yuv420_dst{};
    c.dst.y = g_y; c.dst.u = g_u; c.dst.v = layout == SWK_YUV_I420 ? g_v : nullptr;
    c.dst.mem = host ? SWK_MEM_HOST : SWK_MEM_DEVICE; c.dst.layout = layout;
    c.dst.y_row_stride = Wd; c.dst.c_row_stride = half_up(Wd) * (layout == SWK_YUV_NV12 ? 2 : 1);
    c.dst.y_frame_stride = 123456; c.dst.c_frame_stride = 7890;
}

void fit_src(Call &c, int nwin, int n, int Hc, int Wc, int channels, int x0, int y0, bool host)
{
    c.in = swk_input{};
    c.in.frames = g_frames; c.in.mem = host ? SWK_MEM_HOST : SWK_MEM_DEVICE; c.in.channels = channels;
    c.in.nwin = nwin; c.in.n = n; c.in.Hc = Hc; c.in.Wc = Wc; c.in.x0 = x0; c.in.y0 = y0;
    c.in.row_stride = (int64_t)(x0 + Wc) * channels; c.in.frame_stride = -c.in.row_stride * (y0 + Hc);
}

// ---- geometry and staging sizes of an accepted plan, from the header's definitions -----------------------------------------------
void check_geometry(const Call &c, const ReviewPlan &pl)
{
    const int F = c.F(), Hc = c.in.Hc, Wc = c.in.Wc, npanels = (int)c.panels.size();
    CHECK(pl.F == F && pl.Hc == Hc && pl.Wc == Wc);
    CHECK(pl.mosaic == (c.cols != 0));
    CHECK(pl.Hp == even(Hc) && pl.Wp == even(Wc));
    int rows = 1, cols = 1;
    if (c.cols) {
        cols = c.cols;
        while (rows * cols < 1 + npanels) ++rows;             // the fewest rows that hold the composed frame and every panel
    }
    CHECK(pl.rows == rows && pl.cols == cols);
    const int Hd = c.cols ? rows * even(Hc) : Hc, Wd = c.cols ? cols * even(Wc) : Wc;
    CHECK(pl.Hd == Hd && pl.Wd == Wd);
    CHECK(pl.ch == half_up(Hd) && pl.cw == half_up(Wd));
    CHECK(pl.nv12 == (c.dst.layout == SWK_YUV_NV12) && pl.cbytes == (pl.nv12 ? 2 : 1));
    CHECK(pl.rowb == (size_t)Wc * c.in.channels && pl.src_bytes == (size_t)F * Hc * Wc * c.in.channels);
    CHECK(is_round16(pl.per, (size_t)F * Hc * Wc));
    size_t host_panels = 0;
    for (const swk_review_panel &p : c.panels) host_panels += p.mem == SWK_MEM_HOST ? 1 : 0;
    CHECK(pl.host_panels == host_panels);
    CHECK(is_round16(pl.yb, (size_t)F * Hd * Wd));
    CHECK(is_round16(pl.cb, (size_t)F * half_up(Hd) * half_up(Wd) * (pl.nv12 ? 2 : 1)));
}

// ---- the table (swk_internal.h: launch_review, launch_review_panels) -------------------------------------------------------------
uint32_t style_colour(const swk_review_style &s) { return (uint32_t)s.b + 256u * s.g + 65536u * s.r; }

// the header's palette: black, then twelve hues at three strengths
void header_palette(uint32_t out[256])
{
    static const int hue[12][3] = {{0, 0, 255},   {0, 255, 0},   {255, 0, 0},   {0, 255, 255}, {255, 0, 255}, {255, 255, 0},
                                   {0, 128, 255}, {128, 255, 0}, {255, 0, 128}, {255, 128, 0}, {128, 0, 255}, {0, 255, 128}};
    static const int s[3] = {256, 176, 112};
    out[0] = 0;
    for (int v = 1; v < 256; ++v) {
        const int *h = hue[(v - 1) % 12], k = s[((v - 1) / 12) % 3];
        out[v] = (uint32_t)(h[0] * k / 256) + 256u * (uint32_t)(h[1] * k / 256) + 65536u * (uint32_t)(h[2] * k / 256);
    }
}

void check_label_record(const Call &c, const swk_review_label &l, const int32_t *e)
{
    CHECK(e[0] == l.r && e[1] == l.c && e[2] == l.scale && e[3] == l.len);
    if (l.style) CHECK((uint32_t)e[4] == style_colour(c.styles[l.style - 1]) && e[5] == c.styles[l.style - 1].line_alpha);
    else CHECK(e[5] == 0);
    if (l.plate) CHECK((uint32_t)e[6] == style_colour(c.styles[l.plate - 1]) && e[7] == c.styles[l.plate - 1].fill_alpha);
    else CHECK(e[7] == 0);
    // 32 font indices, little-endian in 8 words; those past len are zero
    uint8_t idx[32] = {0};
    for (int j = 0; j < l.len; ++j) idx[j] = (uint8_t)(l.text[j] - 32);
    for (int w = 0; w < 8; ++w) {
        const uint32_t want = idx[4 * w] | (uint32_t)idx[4 * w + 1] << 8 | (uint32_t)idx[4 * w + 2] << 16 | (uint32_t)idx[4 * w + 3] << 24;
        CHECK((uint32_t)e[8 + w] == want);
    }
}

// start [F + 1] at meta[o]: frame f's records are [start[f], start[f + 1])
template <class Rec> void check_starts(const ReviewPlan &pl, size_t o, int F, const std::vector<Rec> &recs)
{
    CHECK(pl.meta[o] == 0);
    for (int f = 0; f < F; ++f) {
        int on_frame = 0;
        for (const Rec &r : recs) on_frame += r.frame == f ? 1 : 0;
        CHECK(pl.meta[o + f + 1] - pl.meta[o + f] == on_frame);
    }
    CHECK(pl.meta[o + F] == (int)recs.size());
}

void check_tables(const Call &c, const ReviewPlan &pl)
{
    if (!c.has_rv) { CHECK(pl.meta.empty() && pl.mask_alpha == 0 && !pl.has_border); return; }
    const int F = c.F();
    const std::vector<int32_t> &m = pl.meta;
    size_t at = 0;                                            // the blocks follow one another in the documented order
    auto take = [&](size_t off, size_t words) { CHECK(off == at); at += words; CHECK(at <= m.size()); };
    take(pl.o_boxes, c.boxes.size() * 6);
    for (size_t k = 0; k < c.boxes.size(); ++k) {
        const swk_review_box &b = c.boxes[k];
        const int32_t *e = &m[pl.o_boxes + 6 * k];
        CHECK(e[0] == b.r0 && e[1] == b.c0 && e[3] == b.c1);
        if (b.style == 0) { CHECK(e[2] == e[0]); continue; }                  // empty: nothing is drawn
        const swk_review_style &s = c.styles[b.style - 1];
        CHECK(e[2] == b.r1 && (uint32_t)e[4] == style_colour(s));
        CHECK((e[5] & 0xFFFF) == s.fill_alpha && (e[5] >> 16) == s.line_alpha);
    }
    take(pl.o_bstart, (size_t)F + 1);
    check_starts(pl, pl.o_bstart, F, c.boxes);
    take(pl.o_marks, c.marks.size() * 4);
    for (size_t k = 0; k < c.marks.size(); ++k) {
        const swk_review_mark &mk = c.marks[k];
        const int32_t *e = &m[pl.o_marks + 4 * k];
        CHECK(e[0] == mk.r && e[1] == mk.c);
        if (mk.style) CHECK((uint32_t)e[2] == style_colour(c.styles[mk.style - 1]) && e[3] == c.styles[mk.style - 1].line_alpha);
        else CHECK(e[3] == 0);
    }
    take(pl.o_mstart, (size_t)F + 1);
    check_starts(pl, pl.o_mstart, F, c.marks);
    CHECK(pl.has_border == c.has_fstyle);
    if (c.has_fstyle) {
        take(pl.o_border, (size_t)F * 2);
        for (int f = 0; f < F; ++f) {
            const int st = c.fstyle[f];
            if (st) CHECK((uint32_t)m[pl.o_border + 2 * f] == style_colour(c.styles[st - 1]) && m[pl.o_border + 2 * f + 1] == c.styles[st - 1].line_alpha);
            else CHECK(m[pl.o_border + 2 * f] == 0 && m[pl.o_border + 2 * f + 1] == -1);
        }
    }
    if (c.has_mask && c.mask_style) {
        const size_t px = (size_t)c.in.Hc * c.in.Wc;
        take(pl.o_mask, (px + 3) / 4);
        const uint8_t *bytes = (const uint8_t *)&m[pl.o_mask];
        for (size_t i = 0; i < (px + 3) / 4 * 4; ++i) CHECK(bytes[i] == (i < px ? c.mask[i] : 0));
        CHECK(pl.mask_colour == style_colour(c.styles[c.mask_style - 1]) && pl.mask_alpha == c.styles[c.mask_style - 1].fill_alpha);
    } else {
        CHECK(pl.mask_alpha == 0);
    }
    if (!c.panels.empty()) {
        take(pl.o_captions, c.panels.size() * 16);
        for (size_t k = 0; k < c.panels.size(); ++k) check_label_record(c, c.panels[k].caption, &m[pl.o_captions + 16 * k]);
        take(pl.o_palette, 256);
        uint32_t want[256];
        header_palette(want);
        uint8_t lib[256][3];
        review_label_palette(lib);
        for (int v = 0; v < 256; ++v) {
            CHECK((uint32_t)m[pl.o_palette + v] == want[v]);
            CHECK(want[v] == (uint32_t)lib[v][0] + 256u * lib[v][1] + 65536u * lib[v][2]);
        }
    }
    if (!c.labels.empty()) {
        take(pl.o_labels, c.labels.size() * 16);
        for (size_t k = 0; k < c.labels.size(); ++k) check_label_record(c, c.labels[k], &m[pl.o_labels + 16 * k]);
        take(pl.o_lstart, (size_t)F + 1);
        check_starts(pl, pl.o_lstart, F, c.labels);
    }
    CHECK(at == m.size());                                    // and nothing else is in the table
}

void accept(const std::string &name, const Call &c)
{
    g_case = name;
    g_cases += 1;
    Args a;
    wire(c, a);
    ReviewPlan pl;
    const char *why = nullptr;
    const int rc = run(a, &pl, &why);
    if (rc) fprintf(stderr, "%s: refused: %s\n", name.c_str(), why ? why : "(null)");
    CHECK(rc == SWK_OK);
    check_geometry(c, pl);
    check_tables(c, pl);
}

// ---- refusals ----------------------------------------------------------------------------------------------------------------
// the call every refusal case starts from: a mosaic of two panels with every layer and two labels
Call base_call()
{
    Call c;
    fit_src(c, 2, 3, 5, 7, 3, 2, 1, true);
    c.cols = 2;
    fit_dst(c, SWK_YUV_I420, true);
    c.styles = {{1, 2, 3, 0, 256, 255}, {200, 100, 50, 0, 0, 128}};
    c.boxes = {{0, 1, 1, 4, 5, 1}, {2, -3, -3, 9, 9, 2}, {2, 0, 0, 2, 2, 0}};
    c.marks = {{1, 2, 3, 1}, {5, 0, 0, 0}};
    c.has_fstyle = true; c.fstyle = {0, 1, 2, 0, 0, 1};
    c.has_mask = true; c.mask.assign(35, 0); c.mask[3] = 1; c.mask[34] = 255; c.mask_style = 2;
    c.labels = {make_label(0, 1, 1, 1, 2, 1, "SWIFT 12"), make_label(4, -5, 100, 0, 0, 8, "")};
    c.panels = {make_panel(SWK_PANEL_GRAY, 3, 15, 7, true, make_label(99, 0, 0, 1, 0, 2, "AB")),
                make_panel(SWK_PANEL_LABELS, 0, 0, 7, false, make_label(-1, 0, 0, 0, 0, 1, ""))};
    return c;
}

using EditCall = std::function<void(Call &)>;
using EditArgs = std::function<void(Args &)>;

// the base call with the faults applied must be refused with (code, msg), and the plan handed in must be left as it was
void refuse(const char *name, int code, const char *msg, const EditCall &edit, const EditArgs &late = nullptr)
{
    g_case = std::string("refusal: ") + name;
    g_cases += 1;
    Call c = base_call();
    if (edit) edit(c);
    Args a;
    wire(c, a);
    if (late) late(a);
    ReviewPlan pl;
    pl.F = -77; pl.yb = 4242; pl.meta = {1, 2, 3};
    const char *why = nullptr;
    const int rc = run(a, &pl, &why);
    if (rc != code || !why || strcmp(why, msg)) fprintf(stderr, "%s: got %d '%s', want %d '%s'\n", name, rc, why ? why : "(null)", code, msg);
    CHECK(rc == code && why && !strcmp(why, msg));
    CHECK(pl.F == -77 && pl.yb == 4242 && pl.meta == std::vector<int32_t>({1, 2, 3}) && pl.Hc == 0 && pl.o_lstart == 0);
}

const char *const kNullArg = "null argument", *const kNullFrames = "null frames", *const kEmpty = "empty batch",
                 *const kChannels = "channels must be 1 or 3", *const kMem = "mem must be SWK_MEM_HOST or SWK_MEM_DEVICE",
                 *const kOrigin = "negative ROI origin", *const kFrames = "too many frames in one call (2^24 at most)",
                 *const kSide = "ROI side above 32768", *const kCells = "npanels outside 0..15 or cols outside 1..16",
                 *const kNullPanels = "null panels with a non-zero count", *const kMosaic = "mosaic side above 32768",
                 *const kSrcStride = "source row stride smaller than the ROI's row",
                 *const kLayout = "unknown YUV layout (SWK_YUV_I420 or SWK_YUV_NV12)", *const kNullPlane = "null YUV plane",
                 *const kDstStride = "row stride smaller than a row", *const kPanelPlane = "a panel's plane is null",
                 *const kPanelMem = "a panel's mem must be SWK_MEM_HOST or SWK_MEM_DEVICE",
                 *const kPanelKind = "a panel's kind is SWK_PANEL_GRAY or SWK_PANEL_LABELS", *const kGain = "a gray panel's gain outside 1..255",
                 *const kPanelStride = "a panel's row stride smaller than the ROI's row", *const kLayers = "a panel's layers outside 0..15",
                 *const kStyles = "styles", *const kArrays = "a null array with a non-zero count, or a negative count",
                 *const kArm = "negative mark_arm or border", *const kAlpha = "an alpha outside 0..256",
                 *const kMaskStyle = "mask style outside 0..nstyles", *const kBoxFrame = "a box's frame outside the call's frames",
                 *const kBoxOrder = "boxes not in ascending frame order", *const kBoxStyle = "a box's style outside 0..nstyles",
                 *const kMarkFrame = "a mark's frame outside the call's frames", *const kMarkOrder = "marks not in ascending frame order",
                 *const kMarkStyle = "a mark's style outside 0..nstyles", *const kBorderStyle = "a frame's border style outside 0..nstyles",
                 *const kLabelArray = "a null label array with a non-zero count, or a negative count",
                 *const kLabelFrame = "a label's frame outside the call's frames", *const kLabelOrder = "labels not in ascending frame order",
                 *const kScale = "a label's scale outside 1..8", *const kLen = "a label's len outside 0..32",
                 *const kLabelStyle = "a label's style or plate outside 0..nstyles",
                 *const kText = "a label's text holds a byte outside the character set";

// one fault per name: reused alone (every refusal) and in pairs (the earlier one wins)
struct Fault { const char *name; int code; const char *msg; EditCall edit; EditArgs late; };

std::vector<Fault> faults_in_order()
{
    const int A = SWK_ERR_ARG, C = SWK_ERR_CAPACITY;
    std::vector<Fault> v;
    auto call = [&](const char *name, int code, const char *msg, EditCall e) { v.push_back({name, code, msg, e, nullptr}); };
    auto late = [&](const char *name, int code, const char *msg, EditArgs e) { v.push_back({name, code, msg, nullptr, e}); };
    // in the order the call meets them
    late("null in", A, kNullArg, [](Args &a) { a.pin = nullptr; });
    late("null dst", A, kNullArg, [](Args &a) { a.pdst = nullptr; });
    call("null frames", A, kNullFrames, [](Call &c) { c.in.frames = nullptr; });
    call("nwin 0", A, kEmpty, [](Call &c) { c.in.nwin = 0; });
    call("n 0", A, kEmpty, [](Call &c) { c.in.n = 0; });
    call("Hc 0", A, kEmpty, [](Call &c) { c.in.Hc = 0; });
    call("Wc -1", A, kEmpty, [](Call &c) { c.in.Wc = -1; });
    call("channels 2", A, kChannels, [](Call &c) { c.in.channels = 2; });
    call("channels 4", A, kChannels, [](Call &c) { c.in.channels = 4; });
    call("source mem", A, kMem, [](Call &c) { c.in.mem = 2; });
    call("dst mem", A, kMem, [](Call &c) { c.dst.mem = -1; });
    call("x0 -1", A, kOrigin, [](Call &c) { c.in.x0 = -1; });
    call("y0 -1", A, kOrigin, [](Call &c) { c.in.y0 = -1; });
    call("2^24 + 1 frames", C, kFrames, [](Call &c) { c.in.nwin = (1 << 24) + 1; c.in.n = 1; });
    call("2^31 frames", C, kFrames, [](Call &c) { c.in.nwin = 1 << 16; c.in.n = 1 << 15; });
    call("Hc 32769", C, kSide, [](Call &c) { c.in.Hc = 32769; });
    call("Wc 32769", C, kSide, [](Call &c) { c.in.Wc = 32769; });
    late("npanels -1", A, kCells, [](Args &a) { a.npanels = -1; });
    late("npanels 16", A, kCells, [](Args &a) { a.npanels = 16; });
    call("cols 17", A, kCells, [](Call &c) { c.cols = 17; });
    call("cols -1", A, kCells, [](Call &c) { c.cols = -1; });
    late("null panels", A, kNullPanels, [](Args &a) { a.panels = nullptr; });
    call("mosaic rows", C, kMosaic, [](Call &c) { c.in.Hc = 16385; c.cols = 2; });           // 2 rows of 16386
    call("mosaic cols", C, kMosaic, [](Call &c) { c.in.Wc = 16385; c.cols = 2; });
    call("source row stride", A, kSrcStride, [](Call &c) { c.in.row_stride -= 1; });
    call("dst layout", A, kLayout, [](Call &c) { c.dst.layout = 2; });
    call("null y", A, kNullPlane, [](Call &c) { c.dst.y = nullptr; });
    call("null u", A, kNullPlane, [](Call &c) { c.dst.u = nullptr; });
    call("null v of I420", A, kNullPlane, [](Call &c) { c.dst.v = nullptr; });
    call("dst luma stride", A, kDstStride, [](Call &c) { c.dst.y_row_stride = 15; });          // the mosaic's row is 16
    call("dst chroma stride", A, kDstStride, [](Call &c) { c.dst.c_row_stride = 7; });
    call("NV12 chroma stride", A, kDstStride, [](Call &c) { c.dst.layout = SWK_YUV_NV12; c.dst.c_row_stride = 15; });
    call("panel plane", A, kPanelPlane, [](Call &c) { c.panels[0].plane = nullptr; });
    call("panel mem", A, kPanelMem, [](Call &c) { c.panels[0].mem = 7; });
    call("panel kind", A, kPanelKind, [](Call &c) { c.panels[0].kind = 2; });
    call("gain 0", A, kGain, [](Call &c) { c.panels[0].gain = 0; });
    call("gain 256", A, kGain, [](Call &c) { c.panels[0].gain = 256; });
    call("panel row stride", A, kPanelStride, [](Call &c) { c.panels[0].row_stride = 6; });
    call("layers 16", A, kLayers, [](Call &c) { c.panels[0].layers = 16; });
    call("layers -1", A, kLayers, [](Call &c) { c.panels[1].layers = -1; });
    late("nstyles -1", A, kStyles, [](Args &a) { a.rv.nstyles = -1; });
    late("null styles", A, kStyles, [](Args &a) { a.rv.styles = nullptr; });
    late("nboxes -1", A, kArrays, [](Args &a) { a.rv.nboxes = -1; });
    late("nmarks -1", A, kArrays, [](Args &a) { a.rv.nmarks = -1; });
    late("null boxes", A, kArrays, [](Args &a) { a.rv.boxes = nullptr; });
    late("null marks", A, kArrays, [](Args &a) { a.rv.marks = nullptr; });
    call("mark_arm -1", A, kArm, [](Call &c) { c.mark_arm = -1; });
    call("border -1", A, kArm, [](Call &c) { c.border = -1; });
    call("fill alpha -1", A, kAlpha, [](Call &c) { c.styles[0].fill_alpha = -1; });
    call("fill alpha 257", A, kAlpha, [](Call &c) { c.styles[1].fill_alpha = 257; });
    call("line alpha -1", A, kAlpha, [](Call &c) { c.styles[1].line_alpha = -1; });
    call("line alpha 257", A, kAlpha, [](Call &c) { c.styles[0].line_alpha = 257; });
    call("mask style 3", A, kMaskStyle, [](Call &c) { c.mask_style = 3; });
    call("mask style -1", A, kMaskStyle, [](Call &c) { c.mask_style = -1; });
    call("box frame -1", A, kBoxFrame, [](Call &c) { c.boxes[0].frame = -1; });
    call("box frame F", A, kBoxFrame, [](Call &c) { c.boxes[2].frame = 6; });
    call("boxes order", A, kBoxOrder, [](Call &c) { c.boxes[2].frame = 1; });
    call("box style", A, kBoxStyle, [](Call &c) { c.boxes[1].style = 3; });
    call("mark frame -1", A, kMarkFrame, [](Call &c) { c.marks[0].frame = -1; });
    call("mark frame F", A, kMarkFrame, [](Call &c) { c.marks[1].frame = 6; });
    call("marks order", A, kMarkOrder, [](Call &c) { c.marks[1].frame = 0; });
    call("mark style", A, kMarkStyle, [](Call &c) { c.marks[1].style = -1; });
    call("border style", A, kBorderStyle, [](Call &c) { c.fstyle[5] = 3; });
    late("nlabels -1", A, kLabelArray, [](Args &a) { a.nlabels = -1; });
    late("null labels", A, kLabelArray, [](Args &a) { a.labels = nullptr; });
    call("label frame -1", A, kLabelFrame, [](Call &c) { c.labels[0].frame = -1; });
    call("label frame F", A, kLabelFrame, [](Call &c) { c.labels[1].frame = 6; });
    call("labels order", A, kLabelOrder, [](Call &c) { c.labels[0].frame = 5; });
    call("scale 0", A, kScale, [](Call &c) { c.labels[0].scale = 0; });
    call("scale 9", A, kScale, [](Call &c) { c.labels[1].scale = 9; });
    call("len -1", A, kLen, [](Call &c) { c.labels[1].len = -1; });
    call("len 33", A, kLen, [](Call &c) { c.labels[0].len = 33; });
    call("label style", A, kLabelStyle, [](Call &c) { c.labels[0].style = 3; });
    call("label plate", A, kLabelStyle, [](Call &c) { c.labels[0].plate = -1; });
    call("lower case", A, kText, [](Call &c) { c.labels[0].text[2] = 'a'; });
    call("byte 200", A, kText, [](Call &c) { c.labels[0].text[7] = 200; });
    call("byte inside the table, no glyph", A, kText, [](Call &c) { c.labels[0].text[0] = '!'; });
    call("caption scale", A, kScale, [](Call &c) { c.panels[1].caption.scale = 0; });
    call("caption len", A, kLen, [](Call &c) { c.panels[0].caption.len = 33; });
    call("caption plate", A, kLabelStyle, [](Call &c) { c.panels[0].caption.plate = 3; });
    call("caption text", A, kText, [](Call &c) { c.panels[0].caption.text[1] = '['; });
    return v;
}

void check_refusals()
{
    const std::vector<Fault> faults = faults_in_order();
    for (const Fault &f : faults) refuse(f.name, f.code, f.msg, f.edit, f.late);
    // two faults in one call: the one met first is reported.  Every fault against a later one with another message, where the
    // two edits do not touch the same field
    auto find = [&](const char *name) {
        for (const Fault &f : faults)
            if (!strcmp(f.name, name)) return f;
        fprintf(stderr, "no fault named %s\n", name);
        exit(1);
    };
    const char *pairs[][2] = {
        {"null frames", "Hc 0"}, {"n 0", "channels 2"}, {"channels 4", "dst mem"}, {"source mem", "x0 -1"}, {"y0 -1", "2^24 + 1 frames"},
        {"2^31 frames", "Hc 32769"}, {"Wc 32769", "cols 17"}, {"npanels 16", "null panels"}, {"null panels", "source row stride"},
        {"mosaic cols", "source row stride"}, {"source row stride", "dst layout"}, {"dst layout", "null y"}, {"null u", "dst luma stride"},
        {"dst chroma stride", "panel plane"}, {"panel plane", "panel mem"}, {"panel mem", "panel kind"}, {"panel kind", "gain 0"},
        {"gain 256", "panel row stride"}, {"panel row stride", "layers 16"}, {"gain 0", "layers -1"}, {"layers -1", "nstyles -1"},
        {"layers 16", "caption text"}, {"null styles", "nboxes -1"}, {"null marks", "border -1"}, {"mark_arm -1", "fill alpha 257"},
        {"line alpha -1", "mask style 3"}, {"mask style -1", "box frame -1"}, {"box frame -1", "box style"}, {"box style", "boxes order"},
        {"boxes order", "mark frame -1"}, {"mark frame -1", "mark style"}, {"mark style", "border style"}, {"border style", "nlabels -1"},
        {"null labels", "caption scale"}, {"label frame -1", "scale 0"}, {"scale 0", "label frame F"}, {"lower case", "labels order"},
        {"scale 0", "len 33"},
        {"len 33", "label plate"}, {"label style", "byte 200"}, {"lower case", "caption scale"}, {"scale 9", "caption len"},
    };
    for (const auto &p : pairs) {
        const Fault first = find(p[0]), second = find(p[1]);
        CHECK(strcmp(first.msg, second.msg) != 0);
        const std::string name = std::string(p[0]) + " before " + p[1];
        refuse(name.c_str(), first.code, first.msg,
               [&](Call &c) { if (first.edit) first.edit(c); if (second.edit) second.edit(c); },
               [&](Args &a) { if (first.late) first.late(a); if (second.late) second.late(a); });
    }
    // records are checked one after the other, each against all its rules ("box style" on box 1 before "boxes order" on box 2,
    // "scale 0" on label 0 before "label frame F" on label 1): an earlier record's last rule comes before a later record's first
    refuse("panel 0's last rule before panel 1's first", SWK_ERR_ARG, kLayers, [](Call &c) { c.panels[0].layers = 16; c.panels[1].plane = nullptr; });
    refuse("caption of panel 0 before panel 1", SWK_ERR_ARG, kLen, [](Call &c) { c.panels[0].caption.len = 33; c.panels[1].caption.scale = 0; });
    // without rv none of rv's, the labels' or the captions' rules is applied (swk_bgr_to_yuv420), the others are
    {
        Call c = base_call();
        c.has_rv = false;
        c.labels[0].scale = 0; c.panels[0].caption.len = 33; c.mask_style = 9;
        accept("no rv: labels and captions are not looked at", c);
        refuse("no rv: a panel's own fields still count", SWK_ERR_ARG, kGain, [](Call &k) { k.has_rv = false; k.panels[0].gain = 0; });
    }
    // what is allowed: a LABELS panel's gain is ignored, an NV12 destination needs no v, equal frames are ascending
    {
        Call c = base_call();
        c.panels[1].gain = -5;
        c.dst.layout = SWK_YUV_NV12; c.dst.v = nullptr; c.dst.c_row_stride = 16;
        c.boxes[0].frame = 2;
        accept("allowed", c);
    }
}

// ---- the font, against the header's character set --------------------------------------------------------------------------
void check_font()
{
    g_case = "font";
    uint8_t font[128][8];
    review_font(font);
    const char *set = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#:.-+/=%";
    for (int ch = 0; ch < 128; ++ch) {
        const bool in_set = ch != 0 && strchr(set, ch) != nullptr;
        CHECK(font[ch][7] == (in_set ? 1 : 0));
        int ink = 0;
        for (int r = 0; r < 7; ++r) { CHECK(font[ch][r] < 32); ink += font[ch][r]; }
        CHECK((ink != 0) == (in_set && ch != ' '));
        CHECK(!in_set || (ch >= kReviewFontFirst && ch < kReviewFontFirst + kReviewFontCount));
    }
    CHECK(kReviewMaxPanels == 15);
}

// ---- geometry on the listed sizes ------------------------------------------------------------------------------------------
void check_geometries()
{
    const int sizes[] = {1, 2, 3, 8, 9}, colss[] = {0, 1, 2, 16}, counts[] = {0, 1, 15};
    for (int Hc : sizes)
        for (int Wc : sizes)
            for (int layout : {SWK_YUV_I420, SWK_YUV_NV12})
                for (int cols : colss)
                    for (int np : counts) {
                        if (cols == 0 && np) continue;             // (no entry point hands panels over without a mosaic)
                        Call c;
                        const int channels = (Hc + Wc + np) % 2 ? 3 : 1;
                        fit_src(c, 3, 5 + cols % 3, Hc, Wc, channels, Wc % 3, Hc % 2, np % 2 == 0);
                        c.cols = cols;
                        fit_dst(c, layout, true);
                        c.has_rv = (Hc + cols) % 2 == 0;
                        for (int k = 0; k < np; ++k)
                            c.panels.push_back(make_panel(k % 2, 1 + k, k, Wc + k, k % 3 != 0, make_label(0, k, k, 0, 0, 1 + k % 8, "P")));
                        char name[96];
                        snprintf(name, sizeof name, "geometry %dx%d layout %d cols %d npanels %d", Hc, Wc, layout, cols, np);
                        accept(name, c);
                    }
    // the 32768 limits from the side that is accepted (the other side: "Hc 32769", "Wc 32769", "mosaic rows", "mosaic cols")
    for (int which = 0; which < 4; ++which) {
        Call c;
        if (which == 0) fit_src(c, 1, 2, 32768, 4, 1, 0, 0, false);
        if (which == 1) fit_src(c, 1, 2, 4, 32768, 3, 0, 0, false);
        if (which == 2) fit_src(c, 1, 1, 16384, 4, 1, 0, 0, false);       // 2 rows of 16384
        if (which == 3) fit_src(c, 1, 1, 4, 2047, 1, 0, 0, false);        // 16 cells of 2048 columns
        if (which >= 2) {
            c.cols = which == 2 ? 1 : 16;
            c.panels.assign(which == 2 ? 1 : 15, make_panel(SWK_PANEL_LABELS, 0, 0, c.in.Wc, false, make_label(0, 0, 0, 0, 0, 1, "")));
        }
        fit_dst(c, which % 2 ? SWK_YUV_NV12 : SWK_YUV_I420, false);
        c.has_rv = false;
        accept("a side of 32768, case " + std::to_string(which), c);
    }
    {
        Call c;                                                    // exactly 2^24 frames are taken
        fit_src(c, 1 << 12, 1 << 12, 1, 1, 3, 0, 0, false);
        fit_dst(c, SWK_YUV_I420, false);
        c.has_rv = false;
        accept("2^24 frames", c);
    }
}

// ---- overlays ------------------------------------------------------------------------------------------------------------------
void check_designed_overlays()
{
    accept("the base call", base_call());
    {
        // known numbers, spelled out: style 1 = (b 1, g 2, r 3, fill 256, line 255)
        Call c = base_call();
        Args a;
        wire(c, a);
        ReviewPlan pl;
        const char *why = nullptr;
        g_case = "the base call's words";
        CHECK(run(a, &pl, &why) == SWK_OK);
        const int32_t *box0 = &pl.meta[pl.o_boxes];
        CHECK(box0[0] == 1 && box0[1] == 1 && box0[2] == 4 && box0[3] == 5 && box0[4] == 0x030201 && box0[5] == (256 | 255 << 16));
        const int32_t *box2 = &pl.meta[pl.o_boxes + 12];
        CHECK(box2[2] == box2[0] && box2[5] == 0);
        const int32_t bstart[7] = {0, 1, 1, 3, 3, 3, 3};
        CHECK(!memcmp(&pl.meta[pl.o_bstart], bstart, sizeof bstart));
        const int32_t mstart[7] = {0, 0, 1, 1, 1, 1, 2};
        CHECK(!memcmp(&pl.meta[pl.o_mstart], mstart, sizeof mstart));
        CHECK(pl.meta[pl.o_border] == 0 && pl.meta[pl.o_border + 1] == -1 && pl.meta[pl.o_border + 2] == 0x030201 && pl.meta[pl.o_border + 3] == 255);
        CHECK(pl.mask_colour == (200u | 100u << 8 | 50u << 16) && pl.mask_alpha == 0);        // style 2's fill alpha is 0
        const int32_t *lab = &pl.meta[pl.o_labels];                 // "SWIF" "T 12"
        CHECK(lab[8] == (('S' - 32) | ('W' - 32) << 8 | ('I' - 32) << 16 | ('F' - 32) << 24) && lab[9] == (('T' - 32) | 0 << 8 | ('1' - 32) << 16 | ('2' - 32) << 24));
        CHECK(lab[10] == 0 && lab[15] == 0 && lab[5] == 255 && lab[7] == 0 && lab[6] == (200 | 100 << 8 | 50 << 16));
        CHECK(pl.rows == 2 && pl.Hd == 12 && pl.Wd == 16 && pl.ch == 6 && pl.cw == 8 && pl.yb == 6 * 12 * 16 && pl.cb == 6 * 6 * 8);
        CHECK(pl.per == 224 && pl.host_panels == 1 && pl.src_bytes == 6 * 5 * 21);            // 6 x 35 = 210 bytes -> 224
    }
    {
        Call c = base_call();                                       // an overlay with nothing in it: two prefix tables of zeros
        c.boxes.clear(); c.marks.clear(); c.labels.clear(); c.panels.clear(); c.has_fstyle = false; c.has_mask = false; c.styles.clear();
        c.mask_style = 0; c.cols = 0;
        fit_dst(c, SWK_YUV_NV12, false);
        accept("empty overlay", c);
    }
    {
        Call c = base_call();                                       // everything on the last frame, everything style 0
        for (auto &b : c.boxes) { b.frame = 5; b.style = 0; }
        for (auto &m : c.marks) { m.frame = 5; m.style = 0; }
        for (auto &l : c.labels) { l.frame = 5; l.style = 0; l.plate = 0; }
        c.fstyle.assign(6, 0);
        c.mask_style = 0;
        accept("last frame, style 0", c);
    }
    {
        Call c = base_call();                                       // a mask without a pad byte, and a full-length text
        fit_src(c, 1, 4, 2, 6, 1, 0, 0, false);
        fit_dst(c, SWK_YUV_I420, true);
        c.mask.assign(12, 7); c.mask_style = 1;
        c.boxes.clear(); c.marks.clear(); c.fstyle.assign(4, 2);
        c.labels = {make_label(3, 0, 0, 2, 1, 3, "0123456789ABCDEFGHIJKLMNOPQRSTUV")};
        for (auto &p : c.panels) p.row_stride = 6;
        accept("whole words", c);
    }
}

void check_random_overlays()
{
    std::mt19937 rng(20261021);
    auto upto = [&](int hi) { return (int)(rng() % (uint32_t)(hi + 1)); };          // 0..hi
    const char *set = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#:.-+/=%";
    const int nset = (int)strlen(set);
    for (int it = 0; it < 3000; ++it) {
        Call c;
        const int nwin = 1 + upto(4), n = 1 + upto(7), F = nwin * n, Hc = 1 + upto(11), Wc = 1 + upto(11);
        fit_src(c, nwin, n, Hc, Wc, upto(1) ? 3 : 1, upto(3), upto(3), upto(1) == 1);
        c.has_rv = upto(9) != 0;
        c.cols = upto(2) == 0 ? 0 : 1 + upto(15);
        const int ns = upto(5);
        auto alpha = [&]() { const int k = upto(5); return k == 0 ? 0 : k == 1 ? 256 : upto(256); };
        for (int k = 0; k < ns; ++k) c.styles.push_back({(uint8_t)upto(255), (uint8_t)upto(255), (uint8_t)upto(255), (uint8_t)upto(255), alpha(), alpha()});
        auto coord = [&]() { return upto(60) - 20; };
        auto frames = [&](int count) {                             // ascending, with runs and gaps
            std::vector<int> f(count);
            for (int &x : f) x = upto(F - 1);
            std::sort(f.begin(), f.end());
            return f;
        };
        auto count = [&]() { const int k = upto(3); return k == 0 ? 0 : k == 1 ? upto(5) : upto(200); };
        auto label = [&](int frame) {
            char text[33] = {0};
            const int len = upto(3) == 0 ? 32 * upto(1) : upto(32);
            for (int j = 0; j < len; ++j) text[j] = set[upto(nset - 1)];
            return make_label(frame, coord(), coord(), upto(ns), upto(ns), 1 + upto(7), text);
        };
        if (c.has_rv) {
            for (int f : frames(count())) c.boxes.push_back({f, coord(), coord(), coord(), coord(), upto(ns)});
            for (int f : frames(count())) c.marks.push_back({f, coord(), coord(), upto(ns)});
            for (int f : frames(count())) c.labels.push_back(label(f));
            c.has_fstyle = upto(1) == 1;
            if (c.has_fstyle) for (int f = 0; f < F; ++f) c.fstyle.push_back(upto(ns));
            c.has_mask = upto(1) == 1;
            if (c.has_mask) for (int i = 0; i < Hc * Wc; ++i) c.mask.push_back((uint8_t)upto(255));
            c.mask_style = upto(ns);
            c.mark_arm = upto(9); c.border = upto(9);
        }
        if (c.cols)
            for (int k = upto(15); k > 0; --k)
                c.panels.push_back(make_panel(upto(1), 1 + upto(254), upto(15), Wc + upto(5), upto(1) == 1, label(upto(1000) - 500)));
        fit_dst(c, upto(1), upto(1) == 1);
        c.dst.y_row_stride += upto(1) * upto(40); c.dst.c_row_stride += upto(1) * upto(40);
        accept("random overlay " + std::to_string(it), c);
    }
}

}  // namespace

int main()
{
    check_font();
    check_refusals();
    check_geometries();
    check_designed_overlays();
    check_random_overlays();
    printf("review_plan_check: %ld cases passed\n", g_cases);
    return 0;
}
