// The host-only plan of a batch call (swk_batch_run: one group, swk_batch_run_groups: G groups): everything the driver (run_batch,
// swk_api.hip) derives from (groups, outs) before it touches the device, and the descriptor tables of a call of several groups.
// Plain C++ on include/swk.h: no HIP header, no device, no context -- tests/batch_plan_check.cpp drives it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "swk.h"

namespace swk {

constexpr int kMaxNWide = 128;     // frames per window the plain f64 IALM kernels take (k_ialm_pass_lds<4>, k_ialm_small_wide)

// ---- descriptor records of a call of several groups (read by the kernels of groups.hip, filters.hip, ccl.hip, classify_input.hip) ----
// Gather source of one window: queue position j is the frame at src + j * fs, its ROI pixel (r, c) at
// + (y0 + r) * rs + (x0 + c) * channels; frame j's X plane starts at off + j * pitch, pixels p >= H * W of it are zero.
struct GroupWin {
    const uint8_t *src;
    int64_t fs, rs, off;
    int x0, y0, H, W, channels, pitch;
};
// Geometry of one frame's u8 stage planes: H x W dense pixels starting at element `off` (H = 0: the kernel skips the frame)
struct FrameGeom { int H, W; int64_t off; };
// Classifier-input cut of one frame: its device BGR frame, row stride, frame size, ROI origin, and its region-record cap
struct SegFrame { const uint8_t *frame; int64_t rs; int frame_h, frame_w, x0, y0, cap, pad_; };
// (pixels, frames) scatter of one window: P pixels written to dst (null: not wanted)
struct PnWin { double *dst; int P, pad_; };

// ---- host input -> device: the copy strategy of one host group and the bytes it takes in the ROI buffer ----
struct HostStage { int kind; size_t bytes; };
enum { ST_DENSE = 0, ST_WHOLE, ST_ROWS, ST_2D };
HostStage host_stage_plan(const swk_input *in);

// ---- the plan ----
// A group is one video's windows, with its own frames, memory, ROI and strides.  Every frame's u8 stage planes start at an offset
// of their own and hold its H x W pixels.  The IALM runs once over all groups whose ROI has at least n pixels, on X planes zero-padded
// to the largest of those ROIs: zero pixel rows change neither X^T X nor ||X||_F nor max|X|, and their rows of A, E, Y and S stay
// zero.  A group with fewer pixels than frames runs as a sub-batch of its own at its true P (there svp = min(P, n),
// image_filtering.py:285, so padding would change the result).  One group is the degenerate case: one sub-batch, pitch = P, offset 0.
struct BatchSub {
    std::vector<int> gs;           // member groups, call order
    int P = 0;                     // plane pitch: the largest Hc * Wc of the members
    int nwin = 0, w0 = 0;          // windows, and the first of them in sub-batch order
    int64_t off = 0;               // first stage-plane byte (a multiple of 256)
    bool A = false, E = false;     // a member wants the low-rank / sparse matrices
};
struct BatchGroup {
    int sub, pitch;                // its sub-batch and that one's P
    int win0, swin0;               // first window in call order / in sub-batch order
    int64_t goff;                  // stage-plane offset of its first frame: its planes are [goff, goff + nwin * n * pitch)
    HostStage stage;               // a host group's staging, at roi_off of the ROI buffer (kind -1: a device group)
    size_t roi_off;
    size_t pn_off;                 // a host output's A / E staging, bytes into the (pixels, frames) staging buffer
};
struct BatchPlan {
    int n = 0, nwin = 0, F = 0;
    bool single = true;            // one group: the uniform kernels, no tables
    int Pmax = 0, Hmax = 0, Wmax = 0;
    std::vector<BatchSub> subs;    // [0] = every group with P >= n (when there is one); then one per group with P < n
    size_t total = 0;              // stage-plane bytes: the sub-batches one after the other
    std::vector<BatchGroup> grp;
    size_t roi_bytes = 0, pn_bytes = 0;
    // region records: one stride for the call (the largest cap); records wanted at all; every group leaves what
    // swk_segment_inputs_last needs (records and BGR frames); every group's counts reach the host
    int capmax = 1;
    bool want_props = false, seg_last = true, host_total = true;
    int vec = 4;                   // word width every group's P, pitch and goff allow the one-workgroup labeller (4, 2, 1)
    // descriptor tables, one upload: windows (gather), frames (filter), frames (labelling), frames (classifier inputs), windows in
    // sub-batch order (A, then E)
    size_t o_win = 0, o_gf = 0, o_gc = 0, o_sf = 0, o_pa = 0, o_pe = 0, tab_bytes = 0;
};

// Refuses a call no kernel could serve (SWK_ERR_ARG, *why = the message) or fills *plan.  Launches and allocates nothing.
int plan_batch(const swk_input *groups, int G, const swk_output *outs, BatchPlan *plan, const char **why);

// Where the kernels find a group's frames on the device: frame 0, strides, ROI origin (a host group: in its staged copy).
struct BatchView {
    const uint8_t *frames; int64_t fs, rs; int x0, y0;
    int frame_h() const { return (int)((fs < 0 ? -fs : fs) / rs); }
    int frame_w() const { return (int)(rs / 3); }
};
// A or E of a group, (pixels, frames) layout, on the device (null: not wanted)
struct BatchAE { double *A, *E; };

// Writes the host image of the descriptor tables (plan.tab_bytes bytes at tab, zeroed by the caller) of a call of several groups.
// fused[g]: the group's frames take the one-workgroup labeller (their row of the labelling table is {0, 0, 0} otherwise).
void fill_batch_tables(const BatchPlan &plan, const swk_input *groups, const swk_output *outs, const BatchView *view, const BatchAE *ae,
                       const char *fused, uint8_t *tab);

}  // namespace swk
