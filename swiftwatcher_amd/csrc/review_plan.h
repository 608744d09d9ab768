// The host-only plan of a review call (swk_bgr_to_yuv420, swk_render_review, swk_render_review_labels, swk_render_review_panels):
// everything the driver (review_call, swk_api.hip) derives from its arguments before it touches the device -- the refusals, the
// destination's geometry, the staging sizes and the kernels' int32 table with styles resolved.
// Plain C++ on include/swk.h: no HIP header, no device, no context -- tests/review_plan_check.cpp drives it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "swk.h"

namespace swk {

constexpr int kReviewFontFirst = 32, kReviewFontCount = 59;          // the font table covers bytes 32 (space) .. 90 ('Z')
constexpr int kReviewMaxPanels = 15;

// the font's rows of byte ch (0..127): rows[0..6], rows[7] = 1 where ch is in the character set
void review_font(uint8_t out[128][8]);
// (b, g, r) of label value v in a SWK_PANEL_LABELS panel (include/swk.h has the definition)
void review_label_palette(uint8_t out[256][3]);

struct ReviewPlan {
    int F = 0, Hc = 0, Wc = 0;         // frames of the call, ROI
    // the destination's frames: the ROI (mosaic false: rows = cols = 1), or rows x cols cells of Hp x Wp (Hc, Wc made even)
    bool mosaic = false;
    int rows = 1, cols = 1, Hp = 0, Wp = 0;
    int Hd = 0, Wd = 0, ch = 0, cw = 0;    // luma and chroma samples per side of a destination frame
    bool nv12 = false;
    int cbytes = 1;                    // bytes per chroma sample position in a chroma row
    // dense staging: a host source's ROI (rowb bytes a row); `per` bytes for each of host_panels host planes; a host destination's
    // luma plane and each of its chroma planes (per, yb, cb: multiples of 16)
    size_t rowb = 0, src_bytes = 0, per = 0, host_panels = 0, yb = 0, cb = 0;
    // the kernels' tables in one block of int32, in this order (word layouts: launch_review, launch_review_panels, swk_internal.h);
    // empty without rv.  boxes [nboxes][6], box_start [F + 1], marks [nmarks][4], mark_start [F + 1], border [F][2] (has_border),
    // mask bytes (mask_alpha != 0), captions [npanels][16] and palette [256] (npanels > 0), labels [nlabels][16] and
    // label_start [F + 1] (nlabels > 0).  An offset whose block is absent is not to be used.
    std::vector<int32_t> meta;
    size_t o_boxes = 0, o_bstart = 0, o_marks = 0, o_mstart = 0, o_border = 0, o_mask = 0, o_captions = 0, o_palette = 0, o_labels = 0,
           o_lstart = 0;
    bool has_border = false;
    uint32_t mask_colour = 0;
    int mask_alpha = 0;
};

// Refuses a call (SWK_ERR_ARG / SWK_ERR_CAPACITY, *why = the message, *plan untouched) or fills *plan.  cols == 0: the ROI's frames
// alone; cols >= 1: the mosaic.  rv null: the conversion alone (labels, captions and rv's own checks are skipped).  Reads rv's arrays,
// labels and the panel records; never what in->frames, a panel's plane or a dst plane point to.
int plan_review(const swk_input *in, const swk_review *rv, const swk_review_label *labels, int nlabels, const swk_yuv420_dst *dst,
                const swk_review_panel *panels, int npanels, int cols, ReviewPlan *plan, const char **why);

}  // namespace swk
