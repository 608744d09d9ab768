"""Cases and inputs shared by tests/test_squeeze_bf16s_cpu.py and tests/test_squeeze_bf16s_gpu.py: the wide plain squeezes on
k_squeeze1x1_bf16s (csrc/cnn_squeeze_bf16.hip; swk_set_cnn_tuning knob 4).  No GPU here.

The random inputs are seeded per (case, family) from SEED.  SEED was chosen on the CPU (test_squeeze_bf16s_cpu.py): with it the
simulated intact kernel meets the 3 x criterion of tests/cnn_refs.py on every case and family below, and the simulated kernel that
drops the products i + j >= 2 does not."""
import numpy as np
import torch

import cnn_refs as R

SEED = 3
SHAPES = [(256, 48), (384, 48), (384, 64)]
# cin, cout, n, h, w, source h, source w, crop_y, crop_x, dH, dW, off_y, off_x, dC, c_off
CASES = [(cin, cout, 2, 5, 5, 5, 5, 0, 0, 5, 5, 0, 0, cout, 0) for cin, cout in SHAPES] + [          # 50 rows: a whole row tile and a ragged one
    (384, 48, 1, 3, 11, 3, 11, 0, 0, 3, 11, 0, 0, 48, 0),                                           # 33 rows
    (256, 48, 2, 5, 6, 8, 9, 2, 1, 7, 9, 1, 2, 72, 20),                                             # crop, placement offset, c_off, wider destination
]
IDS = ["%dto%d-%dx%dx%d%s" % (c[0], c[1], c[2], c[3], c[4], "-placed" if c[14] else "") for c in CASES]


def with_segments(case, n):
    return case[:2] + (n,) + case[3:]


def window(x, case):
    cin, cout, n, h, w, sh, sw, cy, cx = case[:9]
    return x[:, :, cy:cy + h, cx:cx + w]


def random_inputs(case, family):
    """x (n, cin, sh, sw), w (cout, cin, 1, 1), b (cout,) as float32 numpy arrays; zero_segment needs a middle segment: n >= 3."""
    cin, cout, n, h, w, sh, sw = case[:7]
    g = torch.Generator(device="cpu").manual_seed(SEED * 100003 + CASES_KEY[(case[:2], case[3:])] * 101 + R.FAMILIES.index(family))
    return tuple(t.numpy() for t in R.random_case(g, family, (n, cin, sh, sw), cout, 1))


CASES_KEY = {(c[:2], c[3:]): i for i, c in enumerate(CASES)}


def kernel_k_order(cin):
    """The reduction order of k_squeeze1x1_bf16s: chunks of 32 channels ascending; k-step i of chunk c multiplies the channels
    32 c + 8 i .. + 7 (lanes 0-31) and 32 c + 16 + 8 i .. + 7 (lanes 32-63)."""
    return np.array([32 * c + 16 * half + 8 * i + j for c in range(cin // 32) for i in range(2) for half in range(2) for j in range(8)])


def rows_of(x, case):
    """The window's pixels as matrix rows (n h w, cin), in the order of the placed block flattened as (n, h, w)."""
    xw = window(x, case)
    return np.ascontiguousarray(xw.transpose(0, 2, 3, 1)).reshape(-1, xw.shape[1])
