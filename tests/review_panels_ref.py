"""Test-side restatement of the review video's stage panels (include/swk.h, swk_render_review_panels) on top of review_ref and
review_text_ref: a panel's plane mapped to BGR, composed with its selected layers and its caption, converted, and the cells pasted
into the mosaic by _lib.panel_layout over Y = 16, U = V = 128.  Written from the definition's text, not from the kernel; the palette
and the font come in as arguments (the library's tables), so they are defined in one place."""
import numpy as np

import review_text_ref as tref


def panel_bgr(plane, kind, gain, palette):
    """(F, H, W, 3) int64: SWK_PANEL_GRAY B = G = R = min(255, v * gain); SWK_PANEL_LABELS palette[v]."""
    v = np.asarray(plane).astype(np.int64)
    if kind == "labels":
        return np.asarray(palette).astype(np.int64)[v]
    return np.repeat(np.minimum(255, v * gain)[..., None], 3, axis=-1)


def panel_cell(plane, kind, gain, layers, caption, overlay, font, palette):
    """(y, u, v) of one stage cell: the mapped plane under those of the overlay's layers 1..4 whose bit is set in `layers` (overlay:
    review_ref.compose's keyword arguments), then the caption (r, c, style, plate, scale, text) or None on every frame."""
    src = panel_bgr(plane, kind, gain, palette)
    kw = dict(styles=overlay["styles"], mark_arm=overlay.get("mark_arm", 0), border=overlay.get("border", 0))
    if layers & 1:
        kw.update(mask=overlay.get("mask"), mask_style=overlay.get("mask_style", 0))
    if layers & 2:
        kw.update(boxes=overlay.get("boxes", ()))
    if layers & 4:
        kw.update(marks=overlay.get("marks", ()))
    if layers & 8:
        kw.update(frame_style=overlay.get("frame_style"))
    labels = [(f,) + tuple(caption) for f in range(src.shape[0])] if caption is not None else []
    return tref.render(src, labels=labels, font=font, **kw)


def paste(cells, Hc, Wc, cols):
    """The mosaic (y, u, v) of the cells' (y, u, v): pasted at panel_layout's origins over Y = 16, U = V = 128."""
    from swiftwatcher_amd._lib import panel_layout
    height, width, origins = panel_layout(Hc, Wc, len(cells), cols)
    F = cells[0][0].shape[0]
    Y = np.full((F, height, width), 16, np.uint8)
    U, V = (np.full((F, height // 2, width // 2), 128, np.uint8) for _ in range(2))
    hc, wc = (Hc + 1) // 2, (Wc + 1) // 2
    for (r, c), (y, u, v) in zip(origins, cells):
        assert y.shape == (F, Hc, Wc) and u.shape == v.shape == (F, hc, wc)
        Y[:, r:r + Hc, c:c + Wc] = y
        U[:, r // 2:r // 2 + hc, c // 2:c // 2 + wc] = u
        V[:, r // 2:r // 2 + hc, c // 2:c // 2 + wc] = v
    return Y, U, V
