"""Writes tests/golden/pil_resize_large.npz: Pillow's own 24 x 24 x 3 bilinear resize of the formula images of tests/pil_resize_ref.py
at shapes where a crop side exceeds 512 pixels.  Run it with a Pillow that runs the horizontal pass first at every shape, like the
reference's pinned 8.1.1 (8.4.0 does; 12.2 runs the vertical pass first on some tall, narrow images and must not be used):

    python3.9 tools/make_pil_resize_goldens.py

Imports numpy and Pillow only; the formula is restated here so that the fixture does not depend on the code it checks."""
import os

import numpy as np
import PIL
from PIL import Image

# rows x columns
SHAPES = [(4096, 25), (3000, 25), (4096, 40), (8000, 30), (30, 4096), (2160, 3840), (513, 24), (24, 513), (3500, 25), (4097, 25),
          (4096, 47), (513, 513), (4096, 600)]


def formula_image(rows, cols, offset=0):
    r = np.arange(rows, dtype=np.int64)[:, None, None]
    c = np.arange(cols, dtype=np.int64)[None, :, None]
    ch = np.arange(3, dtype=np.int64)[None, None, :]
    return ((131 * r + 71 * c + 37 * ch + (r * c) % 251 + offset) % 256).astype(np.uint8)


def main():
    major = int(PIL.__version__.split(".")[0])
    if major >= 10:
        raise SystemExit("Pillow %s may run the vertical pass first on tall images; use a Pillow 8 (the reference pins 8.1.1)" % PIL.__version__)
    bil = getattr(Image, "Resampling", Image).BILINEAR
    patches = np.stack([np.asarray(Image.fromarray(formula_image(h, w)).resize((24, 24), bil)) for h, w in SHAPES])
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "pil_resize_large.npz")
    np.savez_compressed(out, shapes=np.array(SHAPES, np.int32), patches=patches, pillow_version=np.array(PIL.__version__))
    print("wrote", out, patches.shape, "Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
