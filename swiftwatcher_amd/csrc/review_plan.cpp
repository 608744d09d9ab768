// The host-only plan of a review call (review_plan.h): refusals, geometry and the kernels' table.  Integer arithmetic on include/swk.h.
#include "review_plan.h"

#include <string.h>

#include <utility>

namespace swk {

namespace {

#include "review_font.h"
const uint8_t h_font[kReviewFontCount][8] = SWK_REVIEW_FONT_ROWS;
#undef SWK_REVIEW_FONT_ROWS
#undef NONE
#undef G

// a label's own fields, as swk_render_review_labels and a panel's caption are held to them; null = fine
const char *label_fault(const swk_review_label &l, int nstyles, const uint8_t (*font)[8])
{
    if (l.scale < 1 || l.scale > 8) return "a label's scale outside 1..8";
    if (l.len < 0 || l.len > 32) return "a label's len outside 0..32";
    if (l.style < 0 || l.style > nstyles || l.plate < 0 || l.plate > nstyles) return "a label's style or plate outside 0..nstyles";
    for (int j = 0; j < l.len; ++j)
        if (l.text[j] > 127 || !font[l.text[j]][7]) return "a label's text holds a byte outside the character set";
    return nullptr;
}

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

void review_font(uint8_t out[128][8])
{
    memset(out, 0, 128 * 8);
    memcpy(out[kReviewFontFirst], h_font, sizeof(h_font));
}

void review_label_palette(uint8_t out[256][3])
{
    // twelve hues drawn by hand, each at three strengths: label v >= 1 takes hue (v - 1) % 12 at strength ((v - 1) / 12) % 3, so
    // neighbouring label values never share a colour and none is black
    static const uint8_t hue[12][3] = {{0, 0, 255},   {0, 255, 0},   {255, 0, 0},   {0, 255, 255}, {255, 0, 255}, {255, 255, 0},
                                       {0, 128, 255}, {128, 255, 0}, {255, 0, 128}, {255, 128, 0}, {128, 0, 255}, {0, 255, 128}};
    static const int strength[3] = {256, 176, 112};
    out[0][0] = out[0][1] = out[0][2] = 0;
    for (int v = 1; v < 256; ++v)
        for (int c = 0; c < 3; ++c) out[v][c] = (uint8_t)((hue[(v - 1) % 12][c] * strength[((v - 1) / 12) % 3]) >> 8);
}

// ---- the refusals, in the order that is part of the contract; they leave the plan alone ----------------------------------------
static int review_refusal(const swk_input *in, const swk_review *rv, const swk_review_label *labels, int nlabels, const swk_yuv420_dst *dst,
                          const swk_review_panel *panels, int npanels, int cols, const char **why)
{
    auto refuse = [&](int code, const char *msg) { *why = msg; return code; };
    if (!in || !dst) return refuse(SWK_ERR_ARG, "null argument");
    if (!in->frames) return refuse(SWK_ERR_ARG, "null frames");
    if (in->nwin < 1 || in->n < 1 || in->Hc < 1 || in->Wc < 1) return refuse(SWK_ERR_ARG, "empty batch");
    if (in->channels != 1 && in->channels != 3) return refuse(SWK_ERR_ARG, "channels must be 1 or 3");
    if ((in->mem != SWK_MEM_HOST && in->mem != SWK_MEM_DEVICE) || (dst->mem != SWK_MEM_HOST && dst->mem != SWK_MEM_DEVICE))
        return refuse(SWK_ERR_ARG, "mem must be SWK_MEM_HOST or SWK_MEM_DEVICE");
    if (in->x0 < 0 || in->y0 < 0) return refuse(SWK_ERR_ARG, "negative ROI origin");
    if ((int64_t)in->nwin * in->n > (1 << 24)) return refuse(SWK_ERR_CAPACITY, "too many frames in one call (2^24 at most)");
    if (in->Hc > 32768 || in->Wc > 32768) return refuse(SWK_ERR_CAPACITY, "ROI side above 32768");
    const int F = in->nwin * in->n, Hc = in->Hc, Wc = in->Wc;
    const bool mosaic = cols != 0;
    if (mosaic && (npanels < 0 || npanels > kReviewMaxPanels || cols < 1 || cols > 16))
        return refuse(SWK_ERR_ARG, "npanels outside 0..15 or cols outside 1..16");
    if (mosaic && npanels > 0 && !panels) return refuse(SWK_ERR_ARG, "null panels with a non-zero count");
    const int Hp = Hc + (Hc & 1), Wp = Wc + (Wc & 1), rows = mosaic ? (1 + npanels + cols - 1) / cols : 1;
    if (mosaic && ((int64_t)rows * Hp > 32768 || (int64_t)cols * Wp > 32768)) return refuse(SWK_ERR_CAPACITY, "mosaic side above 32768");
    const int Wd = mosaic ? cols * Wp : Wc, cw = (Wd + 1) / 2;
    if (in->row_stride < ((int64_t)in->x0 + Wc) * in->channels) return refuse(SWK_ERR_ARG, "source row stride smaller than the ROI's row");
    if (dst->layout != SWK_YUV_I420 && dst->layout != SWK_YUV_NV12) return refuse(SWK_ERR_ARG, "unknown YUV layout (SWK_YUV_I420 or SWK_YUV_NV12)");
    const bool nv12 = dst->layout == SWK_YUV_NV12;
    if (!dst->y || !dst->u || (!nv12 && !dst->v)) return refuse(SWK_ERR_ARG, "null YUV plane");
    if (dst->y_row_stride < Wd || dst->c_row_stride < (int64_t)cw * (nv12 ? 2 : 1)) return refuse(SWK_ERR_ARG, "row stride smaller than a row");
    for (int k = 0; k < npanels; ++k) {
        const swk_review_panel &p = panels[k];
        if (!p.plane) return refuse(SWK_ERR_ARG, "a panel's plane is null");
        if (p.mem != SWK_MEM_HOST && p.mem != SWK_MEM_DEVICE) return refuse(SWK_ERR_ARG, "a panel's mem must be SWK_MEM_HOST or SWK_MEM_DEVICE");
        if (p.kind != SWK_PANEL_GRAY && p.kind != SWK_PANEL_LABELS) return refuse(SWK_ERR_ARG, "a panel's kind is SWK_PANEL_GRAY or SWK_PANEL_LABELS");
        if (p.kind == SWK_PANEL_GRAY && (p.gain < 1 || p.gain > 255)) return refuse(SWK_ERR_ARG, "a gray panel's gain outside 1..255");
        if (p.row_stride < Wc) return refuse(SWK_ERR_ARG, "a panel's row stride smaller than the ROI's row");
        if (p.layers < 0 || p.layers > 15) return refuse(SWK_ERR_ARG, "a panel's layers outside 0..15");
    }
    if (!rv) return SWK_OK;
    if (rv->nstyles < 0 || (rv->nstyles > 0 && !rv->styles)) return refuse(SWK_ERR_ARG, "styles");
    if (rv->nboxes < 0 || rv->nmarks < 0 || (rv->nboxes > 0 && !rv->boxes) || (rv->nmarks > 0 && !rv->marks))
        return refuse(SWK_ERR_ARG, "a null array with a non-zero count, or a negative count");
    if (rv->mark_arm < 0 || rv->border < 0) return refuse(SWK_ERR_ARG, "negative mark_arm or border");
    for (int k = 0; k < rv->nstyles; ++k)
        if (rv->styles[k].fill_alpha < 0 || rv->styles[k].fill_alpha > 256 || rv->styles[k].line_alpha < 0 || rv->styles[k].line_alpha > 256)
            return refuse(SWK_ERR_ARG, "an alpha outside 0..256");
    auto bad_style = [&](int st) { return st < 0 || st > rv->nstyles; };
    if (bad_style(rv->mask_style)) return refuse(SWK_ERR_ARG, "mask style outside 0..nstyles");
    int prev = 0;
    for (int k = 0; k < rv->nboxes; ++k) {
        const swk_review_box &b = rv->boxes[k];
        if (b.frame < 0 || b.frame >= F) return refuse(SWK_ERR_ARG, "a box's frame outside the call's frames");
        if (b.frame < prev) return refuse(SWK_ERR_ARG, "boxes not in ascending frame order");
        if (bad_style(b.style)) return refuse(SWK_ERR_ARG, "a box's style outside 0..nstyles");
        prev = b.frame;
    }
    prev = 0;
    for (int k = 0; k < rv->nmarks; ++k) {
        const swk_review_mark &m = rv->marks[k];
        if (m.frame < 0 || m.frame >= F) return refuse(SWK_ERR_ARG, "a mark's frame outside the call's frames");
        if (m.frame < prev) return refuse(SWK_ERR_ARG, "marks not in ascending frame order");
        if (bad_style(m.style)) return refuse(SWK_ERR_ARG, "a mark's style outside 0..nstyles");
        prev = m.frame;
    }
    if (rv->frame_style)
        for (int f = 0; f < F; ++f)
            if (bad_style(rv->frame_style[f])) return refuse(SWK_ERR_ARG, "a frame's border style outside 0..nstyles");
    if (nlabels < 0 || (nlabels > 0 && !labels)) return refuse(SWK_ERR_ARG, "a null label array with a non-zero count, or a negative count");
    uint8_t font[128][8];
    review_font(font);
    prev = 0;
    for (int k = 0; k < nlabels; ++k) {
        const swk_review_label &l = labels[k];
        if (l.frame < 0 || l.frame >= F) return refuse(SWK_ERR_ARG, "a label's frame outside the call's frames");
        if (l.frame < prev) return refuse(SWK_ERR_ARG, "labels not in ascending frame order");
        if (const char *fault = label_fault(l, rv->nstyles, font)) return refuse(SWK_ERR_ARG, fault);
        prev = l.frame;
    }
    for (int k = 0; k < npanels; ++k)
        if (const char *fault = label_fault(panels[k].caption, rv->nstyles, font)) return refuse(SWK_ERR_ARG, fault);
    return SWK_OK;
}

// ---- the kernels' tables of a call that passed, styles resolved ------------------------------------------------------------------
static void review_tables(const swk_review *rv, const swk_review_label *labels, int nlabels, const swk_review_panel *panels, int npanels,
                          ReviewPlan &pl)
{
    const int F = pl.F;
    std::vector<int32_t> &meta = pl.meta;
    auto colour = [&](int st) { const swk_review_style &y = rv->styles[st - 1]; return (uint32_t)y.b | ((uint32_t)y.g << 8) | ((uint32_t)y.r << 16); };
    // a block of n words appended to the table; its offset
    auto block = [&](size_t n) { const size_t o = meta.size(); meta.resize(o + n, 0); return o; };
    // first record of every frame, [F + 1], from the records' ascending frames
    auto starts = [&](int count, auto frame_of) {
        const size_t o = block((size_t)F + 1);
        for (int k = 0; k < count; ++k) meta[o + frame_of(k) + 1] += 1;
        for (int f = 0; f < F; ++f) meta[o + f + 1] += meta[o + f];
        return o;
    };
    pl.o_boxes = block((size_t)rv->nboxes * 6);
    for (int k = 0; k < rv->nboxes; ++k) {
        const swk_review_box &b = rv->boxes[k];
        int32_t *e = &meta[pl.o_boxes + (size_t)k * 6];
        e[0] = b.r0; e[1] = b.c0; e[2] = b.r1; e[3] = b.c1;
        if (b.style == 0) { e[2] = b.r0; continue; }                  // style 0 draws nothing: an empty box
        e[4] = (int32_t)colour(b.style);
        e[5] = rv->styles[b.style - 1].fill_alpha | (rv->styles[b.style - 1].line_alpha << 16);
    }
    pl.o_bstart = starts(rv->nboxes, [&](int k) { return rv->boxes[k].frame; });
    pl.o_marks = block((size_t)rv->nmarks * 4);
    for (int k = 0; k < rv->nmarks; ++k) {
        const swk_review_mark &m = rv->marks[k];
        int32_t *e = &meta[pl.o_marks + (size_t)k * 4];
        e[0] = m.r; e[1] = m.c;
        e[2] = m.style ? (int32_t)colour(m.style) : 0;
        e[3] = m.style ? rv->styles[m.style - 1].line_alpha : 0;   // (alpha 0 is the identity)
    }
    pl.o_mstart = starts(rv->nmarks, [&](int k) { return rv->marks[k].frame; });
    pl.has_border = rv->frame_style != nullptr;
    pl.o_border = block(pl.has_border ? (size_t)F * 2 : 0);
    for (int f = 0; f < F && pl.has_border; ++f) {
        const int st = rv->frame_style[f];
        meta[pl.o_border + 2 * (size_t)f] = st ? (int32_t)colour(st) : 0;
        meta[pl.o_border + 2 * (size_t)f + 1] = st ? rv->styles[st - 1].line_alpha : -1;
    }
    pl.o_mask = meta.size();
    if (rv->mask && rv->mask_style) {
        block(((size_t)pl.Hc * pl.Wc + 3) / 4);
        memcpy(&meta[pl.o_mask], rv->mask, (size_t)pl.Hc * pl.Wc);
        pl.mask_colour = colour(rv->mask_style);
        pl.mask_alpha = rv->styles[rv->mask_style - 1].fill_alpha;
    }
    auto label_record = [&](const swk_review_label &l, int32_t *e) {
        e[0] = l.r; e[1] = l.c; e[2] = l.scale; e[3] = l.len;
        e[4] = l.style ? (int32_t)colour(l.style) : 0;
        e[5] = l.style ? rv->styles[l.style - 1].line_alpha : 0;          // (alpha 0 is the identity)
        e[6] = l.plate ? (int32_t)colour(l.plate) : 0;
        e[7] = l.plate ? rv->styles[l.plate - 1].fill_alpha : 0;
        for (int j = 0; j < l.len; ++j) e[8 + (j >> 2)] |= (int32_t)((uint32_t)(l.text[j] - kReviewFontFirst) << (8 * (j & 3)));
    };
    if (npanels > 0) {
        // the panels' captions, then the palette as b | g << 8 | r << 16
        pl.o_captions = block((size_t)npanels * 16);
        for (int k = 0; k < npanels; ++k) label_record(panels[k].caption, &meta[pl.o_captions + (size_t)k * 16]);
        pl.o_palette = block(256);
        uint8_t pal[256][3];
        review_label_palette(pal);
        for (int v = 0; v < 256; ++v) meta[pl.o_palette + v] = (int32_t)((uint32_t)pal[v][0] | ((uint32_t)pal[v][1] << 8) | ((uint32_t)pal[v][2] << 16));
    }
    if (nlabels > 0) {
        pl.o_labels = block((size_t)nlabels * 16);
        for (int k = 0; k < nlabels; ++k) label_record(labels[k], &meta[pl.o_labels + (size_t)k * 16]);
        pl.o_lstart = starts(nlabels, [&](int k) { return labels[k].frame; });
    }
}

int plan_review(const swk_input *in, const swk_review *rv, const swk_review_label *labels, int nlabels, const swk_yuv420_dst *dst,
                const swk_review_panel *panels, int npanels, int cols, ReviewPlan *plan, const char **why)
{
    if (const int rc = review_refusal(in, rv, labels, nlabels, dst, panels, npanels, cols, why)) return rc;
    ReviewPlan pl;
    const int F = pl.F = in->nwin * in->n, Hc = pl.Hc = in->Hc, Wc = pl.Wc = in->Wc;
    pl.mosaic = cols != 0;
    pl.Hp = Hc + (Hc & 1); pl.Wp = Wc + (Wc & 1);
    pl.cols = pl.mosaic ? cols : 1;
    pl.rows = pl.mosaic ? (1 + npanels + cols - 1) / cols : 1;
    pl.Hd = pl.mosaic ? pl.rows * pl.Hp : Hc; pl.Wd = pl.mosaic ? pl.cols * pl.Wp : Wc;
    pl.ch = (pl.Hd + 1) / 2; pl.cw = (pl.Wd + 1) / 2;
    pl.nv12 = dst->layout == SWK_YUV_NV12;
    pl.cbytes = pl.nv12 ? 2 : 1;
    pl.rowb = (size_t)Wc * in->channels;
    pl.src_bytes = (size_t)F * Hc * pl.rowb;
    pl.per = round16((size_t)F * Hc * Wc);
    for (int k = 0; k < npanels; ++k) pl.host_panels += panels[k].mem == SWK_MEM_HOST;
    pl.yb = round16((size_t)F * pl.Hd * pl.Wd); pl.cb = round16((size_t)F * pl.ch * pl.cw * pl.cbytes);
    if (rv) review_tables(rv, labels, nlabels, panels, npanels, pl);
    *plan = std::move(pl);
    return SWK_OK;
}

}  // namespace swk
