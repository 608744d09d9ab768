// The host-only plan of a batch call and its descriptor tables (batch_plan.h).  Integer arithmetic on swk_input / swk_output.
#include "batch_plan.h"

#include <algorithm>

namespace swk {

// swk_batch_run's copy strategies; swk_batch_run_groups stages its host groups the same way
HostStage host_stage_plan(const swk_input *in)
{
    const int F = in->nwin * in->n, H = in->Hc, W = in->Wc;
    const size_t plane = (size_t)F * H * W;
    const int64_t fs = in->frame_stride, rs = in->row_stride, afs = fs < 0 ? -fs : fs;
    const int x0 = in->x0, y0 = in->y0;
    const size_t rowb = (size_t)W * in->channels;
    if (x0 == 0 && (size_t)rs == rowb && fs == (int64_t)H * rs) return {ST_DENSE, plane * in->channels};
    if (rs >= (int64_t)(x0 + W) * in->channels && rs % in->channels == 0 && afs % rs == 0 && afs >= (int64_t)(y0 + H) * rs &&
        (size_t)F * (size_t)afs <= 2 * plane * in->channels) {
        const size_t whole = (size_t)F * (size_t)afs;
        return {ST_WHOLE, whole > plane * in->channels ? whole : plane * in->channels};
    }
    if (x0 == 0 && (size_t)rs == rowb) return {ST_ROWS, plane * in->channels};
    return {ST_2D, plane * in->channels};
}

int plan_batch(const swk_input *groups, int G, const swk_output *outs, BatchPlan *plan, const char **why)
{
    auto refuse = [&](const char *msg) { *why = msg; return (int)SWK_ERR_ARG; };
    BatchPlan &pl = *plan;
    pl = BatchPlan{};
    const int n = groups[0].n;
    int64_t nwin64 = 0;
    for (int g = 0; g < G; ++g) {
        const swk_input *in = &groups[g];
        const swk_output *out = &outs[g];
        if (!in->frames) return refuse("null frames");
        if (in->nwin < 1 || in->n < 1 || in->Hc < 1 || in->Wc < 1) return refuse("empty batch");
        if (in->n != n) return refuse("every group must have the same frames per window");
        if (in->channels != 1 && in->channels != 3) return refuse("channels must be 1 or 3");
        if (in->n > kMaxNWide) return refuse("frames per window must be <= 128");
        if (out->segs && (out->seg_cap < 1 || out->seg_cap > 255)) return refuse("seg_cap must be in 1..255");
        if (in->Hc < 4 || in->Wc < 4) return refuse("ROI must be at least 4x4");
        nwin64 += in->nwin;
    }
    if (nwin64 * n > (1 << 24)) return refuse("too many frames in one call");
    pl.n = n; pl.nwin = (int)nwin64; pl.F = pl.nwin * n;
    pl.single = G == 1;

    // sub-batches of the IALM, and the region-record flags
    pl.subs.resize(1);
    for (int g = 0; g < G; ++g) {
        const int P = groups[g].Hc * groups[g].Wc;
        pl.Hmax = std::max(pl.Hmax, groups[g].Hc);
        pl.Wmax = std::max(pl.Wmax, groups[g].Wc);
        pl.Pmax = std::max(pl.Pmax, P);
        BatchSub *sb = &pl.subs[0];
        if (P < n) { pl.subs.emplace_back(); sb = &pl.subs.back(); }
        sb->gs.push_back(g);
        sb->P = std::max(sb->P, P);
        sb->nwin += groups[g].nwin;
        sb->A = sb->A || outs[g].A; sb->E = sb->E || outs[g].E;
        pl.want_props = pl.want_props || outs[g].segs || outs[g].nseg;
        if (outs[g].segs && outs[g].seg_cap > pl.capmax) pl.capmax = outs[g].seg_cap;
        pl.seg_last = pl.seg_last && outs[g].segs && groups[g].channels == 3;
        pl.host_total = pl.host_total && outs[g].mem == SWK_MEM_HOST && outs[g].nseg;
    }
    if (pl.subs[0].gs.empty()) pl.subs.erase(pl.subs.begin());
    int sub_first = 0;                    // windows in sub-batch order
    for (BatchSub &sb : pl.subs) {        // stage planes: each sub-batch 256-byte aligned
        sb.off = (int64_t)pl.total;
        pl.total += ((size_t)sb.nwin * n * sb.P + 255) & ~(size_t)255;
        sb.w0 = sub_first;
        sub_first += sb.nwin;
    }

    // groups: placement in their sub-batch, host staging of inputs and of A / E
    pl.grp.resize(G);
    for (size_t k = 0; k < pl.subs.size(); ++k)
        for (int g : pl.subs[k].gs) pl.grp[g].sub = (int)k;
    std::vector<int> fill(pl.subs.size(), 0);     // windows of each sub-batch placed so far
    int win0 = 0;
    for (int g = 0; g < G; ++g) {
        BatchGroup &bg = pl.grp[g];
        const BatchSub &sb = pl.subs[bg.sub];
        const int P = groups[g].Hc * groups[g].Wc;
        bg.pitch = sb.P;
        bg.win0 = win0;
        bg.swin0 = sb.w0 + fill[bg.sub];
        bg.goff = sb.off + (int64_t)fill[bg.sub] * n * sb.P;
        win0 += groups[g].nwin;
        fill[bg.sub] += groups[g].nwin;
        if (P % 4 || bg.pitch % 4 || bg.goff % 4) pl.vec = std::min(pl.vec, (P % 2 || bg.pitch % 2 || bg.goff % 2) ? 1 : 2);
        bg.stage = {-1, 0};
        bg.roi_off = bg.pn_off = 0;
        if (groups[g].mem == SWK_MEM_HOST) {
            bg.stage = host_stage_plan(&groups[g]);
            bg.roi_off = pl.roi_bytes;
            pl.roi_bytes += (bg.stage.bytes + 255) & ~(size_t)255;
        }
        if ((outs[g].A || outs[g].E) && outs[g].mem == SWK_MEM_HOST) {
            bg.pn_off = pl.pn_bytes;
            pl.pn_bytes += (size_t)groups[g].nwin * n * P * 8;
        }
    }

    pl.o_win = 0;
    pl.o_gf = pl.o_win + (((size_t)pl.nwin * sizeof(GroupWin) + 15) & ~(size_t)15);
    pl.o_gc = pl.o_gf + (size_t)pl.F * sizeof(FrameGeom);
    pl.o_sf = pl.o_gc + (size_t)pl.F * sizeof(FrameGeom);
    pl.o_pa = pl.o_sf + (size_t)pl.F * sizeof(SegFrame);
    pl.o_pe = pl.o_pa + (size_t)pl.nwin * sizeof(PnWin);
    pl.tab_bytes = pl.o_pe + (size_t)pl.nwin * sizeof(PnWin);
    return SWK_OK;
}

void fill_batch_tables(const BatchPlan &plan, const swk_input *groups, const swk_output *outs, const BatchView *view, const BatchAE *ae,
                       const char *fused, uint8_t *tab)
{
    GroupWin *hwin = (GroupWin *)(tab + plan.o_win);
    FrameGeom *hgf = (FrameGeom *)(tab + plan.o_gf), *hgc = (FrameGeom *)(tab + plan.o_gc);
    SegFrame *hsf = (SegFrame *)(tab + plan.o_sf);
    PnWin *hpa = (PnWin *)(tab + plan.o_pa), *hpe = (PnWin *)(tab + plan.o_pe);
    const int n = plan.n;
    for (size_t g = 0; g < plan.grp.size(); ++g) {
        const swk_input *in = &groups[g];
        const BatchGroup &bg = plan.grp[g];
        const BatchView &v = view[g];
        const int H = in->Hc, W = in->Wc, P = H * W, pitch = bg.pitch;
        for (int wl = 0; wl < in->nwin; ++wl) {
            const int w = bg.win0 + wl;
            GroupWin &d = hwin[w];
            d.src = v.frames + (int64_t)wl * n * v.fs;
            d.fs = v.fs; d.rs = v.rs; d.off = bg.goff + (int64_t)wl * n * pitch;
            d.x0 = v.x0; d.y0 = v.y0; d.H = H; d.W = W; d.channels = in->channels; d.pitch = pitch;
            const int ws = bg.swin0 + wl;
            const size_t wb = (size_t)wl * n * P;
            hpa[ws].P = hpe[ws].P = P;
            if (ae[g].A) hpa[ws].dst = ae[g].A + wb;
            if (ae[g].E) hpe[ws].dst = ae[g].E + wb;
            for (int j = 0; j < n; ++j) {
                const int f = w * n + j;
                hgf[f] = {H, W, d.off + (int64_t)j * pitch};
                hgc[f] = fused[g] ? hgf[f] : FrameGeom{0, 0, 0};
                hsf[f].frame = v.frames + ((int64_t)wl * n + j) * v.fs;
                hsf[f].rs = v.rs;
                hsf[f].frame_h = v.frame_h();
                hsf[f].frame_w = v.frame_w();
                hsf[f].x0 = v.x0; hsf[f].y0 = v.y0;
                hsf[f].cap = outs[g].segs ? outs[g].seg_cap : 1;
            }
        }
    }
}

}  // namespace swk
