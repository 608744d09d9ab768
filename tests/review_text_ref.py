"""Test-side restatement of the review video's fifth layer, labels (include/swk.h, swk_render_review_labels), on top of
review_ref.compose.  Written from the definition's text, not from the kernel: Python integers, one loop per label and pixel.

    rectangle of a label, s = scale: rows [r - s, r + 8 s), columns [c - s, c + 6 s len)
    pixel (y, x) of it inside the frame, v = y - r, u = x - c:
        ink    if v >= 0, u >= 0, v // s < 7, (u // s) % 6 < 5 and bit 4 - (u // s) % 6 of font[text[u // (6 s)]][v // s] is set:
               blend with the colour and line_alpha of `style` (style 0: nothing)
        else   blend with the colour and fill_alpha of `plate` (plate 0: nothing)
    after the border, in array order; len 0 draws nothing.

The glyph shapes come in as an argument (the library's swk_review_font table), so they are defined in one place."""
import numpy as np

import review_ref as ref

CHARSET = b" 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#:.-+/=%"


def _text(text):
    return text.encode("ascii") if isinstance(text, str) else bytes(text)


def draw_labels(img, labels, frame, styles, font):
    """Layer 5 of frame `frame` onto img (H, W, 3) int64, in place.  labels: tuples (frame, r, c, style, plate, scale, text)."""
    H, W = img.shape[:2]
    for lf, r, c, style, plate, s, text in labels:
        text = _text(text)
        n = len(text)
        if lf != frame or n == 0:
            continue
        r, c, s = int(r), int(c), int(s)
        ink, rest = np.zeros((H, W), bool), np.zeros((H, W), bool)          # the label's ink pixels, and the rectangle's other pixels
        for y in range(max(r - s, 0), min(r + 8 * s, H)):
            for x in range(max(c - s, 0), min(c + 6 * s * n, W)):
                v, u = y - r, x - c
                if v >= 0 and u >= 0 and v // s < 7 and (u // s) % 6 < 5 and (int(font[text[u // (6 * s)]][v // s]) >> (4 - (u // s) % 6)) & 1:
                    ink[y, x] = True
                else:
                    rest[y, x] = True
        if style:                                                           # every pixel is blended once: the two sets are disjoint
            col, _, line = ref._style(styles, style)
            img[ink] = ref.blend(img[ink], col, line)
        if plate:
            col, fill, _ = ref._style(styles, plate)
            img[rest] = ref.blend(img[rest], col, fill)


def compose(frames, labels=(), font=None, **kw):
    """review_ref.compose's four layers, then the labels: (F, H, W, 3) int64."""
    out = ref.compose(frames, **kw)
    for f in range(out.shape[0]):
        draw_labels(out[f], labels, f, kw.get("styles", ()), font)
    return out


def render(frames, labels=(), font=None, **kw):
    """(y, u, v) uint8 of the composed frames."""
    return ref.yuv420(compose(frames, labels=labels, font=font, **kw))
