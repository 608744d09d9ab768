"""ctypes binding of libswk.so (include/swk.h; the A/B switches and counters of include/swk_debug.h).  No torch, no numpy arithmetic: this module
only marshals pointers.  There is no CPU fallback -- if the HIP library is missing or no
gfx950 device is usable, importing is fine but creating a Context raises SwkError."""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWK_LIB", os.path.join(_HERE, "libswk.so"))     # SWK_LIB: A/B another build of the same ABI

ABI_VERSION = 2
MEM_HOST, MEM_DEVICE = 0, 1
ERR_STALE = -6
STAGE_DENSE, STAGE_WHOLE, STAGE_ROWS, STAGE_2D, STAGE_DEVICE = 0, 1, 2, 3, -1          # swk_last_host_stage
STAGES = ("gray", "rpca", "bilateral", "thresh", "opened", "labels")
ORDER_RASTER, ORDER_BLOCK2X2 = 0, 1
GRAY_Q14, GRAY_Q15 = 0, 1
YUV_I420, YUV_NV12 = 0, 1
YUV_PLANAR, YUV_SEMIPLANAR, YUV_MONO = 0, 1, 2
K_GRAY, K_IALM_STATS, K_IALM_PASS, K_IALM_SMALL, K_FILTER, K_CCL, K_PROPS, K_COPY = range(8)
KERNEL_FAMILIES = ["gray", "ialm_stats", "ialm_pass", "ialm_small", "filter", "ccl", "props", "copy"]

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_f64p = ctypes.POINTER(ctypes.c_double)
c_i32p = ctypes.POINTER(ctypes.c_int32)


class SwkError(RuntimeError):
    pass


class StaleBatch(SwkError):
    """What a batch left on the device has been overwritten by a later call on the same context."""


class Params(ctypes.Structure):
    _fields_ = [("lmbda", ctypes.c_double), ("tol", ctypes.c_double), ("maxiter", ctypes.c_int32),
                ("bil_d", ctypes.c_int32), ("bil_sigma_color", ctypes.c_double),
                ("bil_sigma_space", ctypes.c_double), ("bil_fma", ctypes.c_int32),
                ("thresh", ctypes.c_int32), ("open_kh", ctypes.c_int32), ("open_kw", ctypes.c_int32),
                ("connectivity", ctypes.c_int32), ("label_order", ctypes.c_int32),
                ("gray_mode", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class Segment(ctypes.Structure):
    _fields_ = [("label", ctypes.c_int32), ("r0", ctypes.c_int32), ("c0", ctypes.c_int32),
                ("r1", ctypes.c_int32), ("c1", ctypes.c_int32), ("reserved_", ctypes.c_int32),
                ("area", ctypes.c_int64), ("sum_r", ctypes.c_int64), ("sum_c", ctypes.c_int64)]


SEGMENT_DTYPE = np.dtype([("label", "<i4"), ("r0", "<i4"), ("c0", "<i4"), ("r1", "<i4"), ("c1", "<i4"),
                          ("reserved_", "<i4"), ("area", "<i8"), ("sum_r", "<i8"), ("sum_c", "<i8")])
assert SEGMENT_DTYPE.itemsize == ctypes.sizeof(Segment) == 48
# swk_segment_shape: m = sums of r^p c^q in the order of SHAPE_MOMENT_ORDER
SHAPE_DTYPE = np.dtype([("label", "<i4"), ("reserved_", "<i4"), ("m", "<i8", (10,)), ("border", "<i8"), ("perim", "<i8", (3,)),
                        ("quads", "<i8", (3,))])
assert SHAPE_DTYPE.itemsize == 144
# swk_shift
SHIFT_DTYPE = np.dtype([("dy", "<i4"), ("dx", "<i4"), ("sad", "<u8"), ("sad_unshifted", "<u8")])
assert SHIFT_DTYPE.itemsize == 24
SUBSHIFT_DTYPE = np.dtype([("dy", "<i4"), ("dx", "<i4"), ("qy_total", "<i4"), ("qx_total", "<i4"), ("sad", "<u8"), ("sad_int", "<u8"),
                           ("sad_unshifted", "<u8")])          # swk_subshift
assert SUBSHIFT_DTYPE.itemsize == 40
STABILIZE_SUBPEL_TILE = (32, 64)          # kSubRows, kSubCols of csrc/stabilize.hip: the anchor tile of a workgroup of the quarter-pixel score kernel
SHAPE_MOMENT_ORDER = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))
DEBUG_GUARD_BYTES, DEBUG_FILL = 64, 0xA5          # swk_debug_filter_fused (include/swk_debug.h)
DEBUG_PLANE_DTYPE = np.dtype([("H", "<i4"), ("W", "<i4"), ("off", "<i8")])


class Input(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_void_p), ("mem", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("nwin", ctypes.c_int32), ("n", ctypes.c_int32), ("Hc", ctypes.c_int32), ("Wc", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32),
                ("frame_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64)]


class Output(ctypes.Structure):
    _fields_ = [("mem", ctypes.c_int32), ("seg_cap", ctypes.c_int32),
                ("gray", ctypes.c_void_p), ("rpca", ctypes.c_void_p), ("bilateral", ctypes.c_void_p),
                ("thresh", ctypes.c_void_p), ("opened", ctypes.c_void_p), ("labels", ctypes.c_void_p),
                ("A", ctypes.c_void_p), ("E", ctypes.c_void_p),
                ("iters", ctypes.c_void_p), ("nseg", ctypes.c_void_p), ("segs", ctypes.c_void_p),
                ("planes_on_device", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class Yuv420(ctypes.Structure):
    _fields_ = [("y", ctypes.c_void_p), ("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("mem", ctypes.c_int32),
                ("layout", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("y_row_stride", ctypes.c_int64), ("y_frame_stride", ctypes.c_int64),
                ("c_row_stride", ctypes.c_int64), ("c_frame_stride", ctypes.c_int64)]


class Yuv(ctypes.Structure):
    _fields_ = Yuv420._fields_ + [("sx", ctypes.c_int32), ("sy", ctypes.c_int32), ("bits", ctypes.c_int32),
                                  ("msb_aligned", ctypes.c_int32), ("full_range", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class Deinterlace(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("tff", "rate", "temporal", "has_prev", "has_next", "y_parity0", "c_parity0", "reserved_")]


class Yuv420Dst(ctypes.Structure):
    _fields_ = [("y", ctypes.c_void_p), ("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("mem", ctypes.c_int32),
                ("layout", ctypes.c_int32), ("y_row_stride", ctypes.c_int64), ("y_frame_stride", ctypes.c_int64),
                ("c_row_stride", ctypes.c_int64), ("c_frame_stride", ctypes.c_int64)]


class ReviewStyle(ctypes.Structure):
    _fields_ = [("b", ctypes.c_uint8), ("g", ctypes.c_uint8), ("r", ctypes.c_uint8), ("reserved_", ctypes.c_uint8),
                ("fill_alpha", ctypes.c_int32), ("line_alpha", ctypes.c_int32)]


class Review(ctypes.Structure):
    _fields_ = [("mask", ctypes.c_void_p), ("mask_style", ctypes.c_int32),
                ("boxes", ctypes.c_void_p), ("nboxes", ctypes.c_int32),
                ("marks", ctypes.c_void_p), ("nmarks", ctypes.c_int32), ("mark_arm", ctypes.c_int32),
                ("frame_style", ctypes.c_void_p), ("border", ctypes.c_int32),
                ("styles", ctypes.c_void_p), ("nstyles", ctypes.c_int32)]


REVIEW_BOX_DTYPE = np.dtype([("frame", "<i4"), ("r0", "<i4"), ("c0", "<i4"), ("r1", "<i4"), ("c1", "<i4"), ("style", "<i4")])
REVIEW_MARK_DTYPE = np.dtype([("frame", "<i4"), ("r", "<i4"), ("c", "<i4"), ("style", "<i4")])
REVIEW_STYLE_DTYPE = np.dtype([("b", "u1"), ("g", "u1"), ("r", "u1"), ("reserved_", "u1"), ("fill_alpha", "<i4"), ("line_alpha", "<i4")])
assert REVIEW_STYLE_DTYPE.itemsize == ctypes.sizeof(ReviewStyle) == 12 and REVIEW_BOX_DTYPE.itemsize == 24 and REVIEW_MARK_DTYPE.itemsize == 16
REVIEW_LABEL_DTYPE = np.dtype([("frame", "<i4"), ("r", "<i4"), ("c", "<i4"), ("style", "<i4"), ("plate", "<i4"), ("scale", "<i4"), ("len", "<i4"),
                               ("reserved_", "<i4"), ("text", "u1", (32,))])
assert REVIEW_LABEL_DTYPE.itemsize == 64


class ReviewLabel(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in ("frame", "r", "c", "style", "plate", "scale", "len", "reserved_")] + [("text", ctypes.c_uint8 * 32)]


class ReviewPanel(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_void_p), ("mem", ctypes.c_int32), ("kind", ctypes.c_int32), ("frame_stride", ctypes.c_int64),
                ("row_stride", ctypes.c_int64), ("gain", ctypes.c_int32), ("layers", ctypes.c_int32), ("caption", ReviewLabel)]


assert ctypes.sizeof(ReviewLabel) == 64 and ctypes.sizeof(ReviewPanel) == 104
PANEL_GRAY, PANEL_LABELS = 0, 1
MAX_PANELS, MAX_PANEL_COLS = 15, 16


def panel_layout(Hc, Wc, cells, cols):
    """The mosaic of swk_render_review_panels: (height, width, origins) -- `cells` cells of Hp x Wp luma pixels (Hc, Wc made even) in
    rows of `cols`; origins[k] = (row, column) of cell k's first luma pixel, always even."""
    if Hc < 1 or Wc < 1 or cells < 1 or cols < 1:
        raise ValueError("a mosaic has at least one cell of at least one pixel, in at least one column")
    Hp, Wp = Hc + (Hc & 1), Wc + (Wc & 1)
    rows = (cells + cols - 1) // cols
    return rows * Hp, cols * Wp, [((k // cols) * Hp, (k % cols) * Wp) for k in range(cells)]


def label_records(labels):
    """REVIEW_LABEL_DTYPE records of tuples (frame, r, c, style, plate, scale, text), text a str (ASCII) or bytes of at most 32 bytes;
    records pass through."""
    if isinstance(labels, np.ndarray) and labels.dtype == REVIEW_LABEL_DTYPE:
        return np.ascontiguousarray(labels)
    labels = list(labels)
    out = np.zeros(len(labels), REVIEW_LABEL_DTYPE)
    if not labels:
        return out
    texts = [lab[6].encode("ascii") if isinstance(lab[6], str) else bytes(lab[6]) for lab in labels]
    if max(len(raw) for raw in texts) > 32:
        raise ValueError("a label holds at most 32 bytes")
    rows = np.array([lab[:6] for lab in labels], dtype=np.int64).reshape(-1, 6)
    for k, name in enumerate(("frame", "r", "c", "style", "plate", "scale")):
        out[name] = rows[:, k]
    out["len"] = [len(raw) for raw in texts]
    out["text"] = np.frombuffer(b"".join(raw.ljust(32, b"\0") for raw in texts), np.uint8).reshape(-1, 32)
    return out


def review_label_palette():
    """swk_review_label_palette: uint8 (256, 3) -- (b, g, r) of label value v in a SWK_PANEL_LABELS panel; row 0 is black."""
    out = np.zeros((256, 3), np.uint8)
    load().swk_review_label_palette(out.ctypes.data)
    return out


def review_font():
    """swk_review_font: uint8 (128, 8) -- rows 0..6 of byte ch's 5 x 7 glyph (bit 4 = the leftmost column), [ch, 7] = 1 where ch is in
    the labels' character set."""
    out = np.zeros((128, 8), np.uint8)
    load().swk_review_font(out.ctypes.data)
    return out


_lib = None
_lib_lock = threading.Lock()

_SIGS = {
    "swk_abi_version": (ctypes.c_int32, []),
    "swk_params_default": (None, [ctypes.POINTER(Params)]),
    "swk_ctx_create": (ctypes.c_int32, [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_void_p)]),
    "swk_ctx_destroy": (None, [ctypes.c_void_p]),
    "swk_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "swk_ctx_device_bytes": (ctypes.c_int64, [ctypes.c_void_p]),
    "swk_batch_run": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Input), ctypes.POINTER(Params), ctypes.POINTER(Output)]),
    "swk_batch_run_groups": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Input), ctypes.c_int32, ctypes.POINTER(Params), ctypes.POINTER(Output)]),
    "swk_yuv420_to_bgr": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Yuv420)] + [ctypes.c_int32] * 5 + [ctypes.c_void_p, ctypes.c_int32]),
    "swk_yuv_to_bgr": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Yuv)] + [ctypes.c_int32] * 5 + [ctypes.c_void_p, ctypes.c_int32]),
    "swk_yuv_deinterlace": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Yuv), ctypes.POINTER(Deinterlace)] + [ctypes.c_int32] * 5 +
                            [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]),
    "swk_bgr_to_yuv420": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Input), ctypes.POINTER(Yuv420Dst)]),
    "swk_render_review": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Input), ctypes.POINTER(Review), ctypes.POINTER(Yuv420Dst)]),
    "swk_render_review_labels": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Input), ctypes.POINTER(Review), ctypes.c_void_p, ctypes.c_int32,
                                                  ctypes.POINTER(Yuv420Dst)]),
    "swk_review_font": (None, [ctypes.c_void_p]),
    "swk_render_review_panels": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(Input), ctypes.POINTER(Review), ctypes.c_void_p, ctypes.c_int32,
                                                  ctypes.POINTER(ReviewPanel), ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Yuv420Dst)]),
    "swk_review_label_palette": (None, [ctypes.c_void_p]),
    "swk_bgr2gray": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_ialm": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_rpca_epilogue": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "swk_bilateral_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p]),
    "swk_thresh_tozero_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]),
    "swk_grey_open3x3_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_grey_open_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 5 + [ctypes.c_void_p]),
    "swk_resize_linear_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 6 + [ctypes.c_void_p]),
    "swk_ccl_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_regionprops_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_segment_shapes_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_int64] * 2 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_stabilize_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_int64] * 2 + [ctypes.c_int32] * 5 +
                         [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int32]),
    "swk_stabilize_subpel_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_int64] * 2 + [ctypes.c_int32] * 5 +
                                [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int32]),
    "swk_classifier_input": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "swk_set_sparse_speculation": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_double]),
    "swk_set_integer_start": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
    "swk_last_integer_start_windows": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]),
    "swk_debug_ialm_start": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double] + [ctypes.c_void_p] * 7),
    "swk_debug_ialm_first_step": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double] + [ctypes.c_void_p] * 7),
    "swk_last_host_stage": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "swk_debug_resize_table": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_debug_filter_fused": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_int64, ctypes.POINTER(Params)] + [ctypes.c_void_p] * 4),
    "swk_debug_force_ccl_multi_kernel": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
    "swk_debug_max_windows": (ctypes.c_int32, [ctypes.c_void_p]),
    "swk_debug_ccl_frame_props": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 6 + [ctypes.c_void_p] * 3),
    "swk_last_eig_sweeps": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]),
    "swk_set_norm_speculation": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_double]),
    "swk_set_norm_guard": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_double]),
    "swk_prof_guard_windows": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]),
    "swk_last_stopping_norms": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "swk_set_start_refine": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_double]),
    "swk_prof_refined_windows": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_prof_pass_bytes_per_element": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]),
    "swk_prof_redo_batches": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]),
    "swk_prof_redo_windows": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]),
    "swk_nhwc_bias_relu_place": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 8 + [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 6),
    "swk_set_cnn_tuning": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]),
    "swk_nhwc_conv7x7s2_bias_relu": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "swk_nhwc_conv1x1_bias_relu_place": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 8 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p] + [ctypes.c_int32] * 6),
    "swk_nhwc_conv3x3_bias_relu_place": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p] + [ctypes.c_int32] * 6),
    "swk_nhwc_conv3x3_winograd_bias_relu_place": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p] + [ctypes.c_int32] * 6),
    "swk_winograd_f2x2_3x3_weights": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p] + [ctypes.c_int32] * 6),
    "swk_winograd_f2x2_3x3_weights_bf16s": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_nhwc_maxpool3s2_conv1x1_bias_relu_place": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p] + [ctypes.c_int32] * 5 + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "swk_nhwc_maxpool3s2": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_nhwc_head2_relu_mean": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]),
    "swk_nhwc_head2_dropout_relu_mean": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                          ctypes.c_int32, ctypes.c_void_p]),
    "swk_segment_inputs": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_segment_inputs_last": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_device_alloc": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    "swk_device_free": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]),
    "swk_device_read": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "swk_classifier_input_window": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "swk_track_costs": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_lsap": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_tracker_create": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    "swk_tracker_destroy": (None, [ctypes.c_void_p]),
    "swk_track_window": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "swk_tracker_export": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64] + [ctypes.c_void_p] * 6),
    "swk_tracker_import": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 4),
    "swk_debug_tracker_force_assignment": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]),
    "swk_median_blur_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_otsu_threshold_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_canny_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_dilate_up_u8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "swk_roi_mask": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "swk_pinned_alloc": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    "swk_pinned_free": (ctypes.c_int32, [ctypes.c_void_p]),
    "swk_cut_boxes": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "swk_stage_frames": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32]),
    "swk_prof_enable": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
    "swk_prof_reset": (ctypes.c_int32, [ctypes.c_void_p]),
    "swk_prof_get": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "swk_prof_window_iters": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    "swk_set_ialm_variant": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
    "swk_set_pass_tuning": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
    "swk_set_eig_method": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
}
EXPORTS = sorted(_SIGS)


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7, like /opt/rocm's).  If libswk.so
    is loaded first it pulls in the system runtime, torch then loads its bundled copy as a SECOND HIP runtime in the
    process and sees no device (measured: torch.cuda.is_available() turns False).  Loading torch's copy first makes it
    the process's one runtime: libswk's request for libamdhip64.so.7 binds to it by SONAME and a later `import torch`
    finds its own file already mapped -- which is also what happens when torch is imported before this module.
    torch itself is NOT imported here."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """dlopen libswk.so and type its entry points.  Raises SwkError when the library has not
    been built (python swiftwatcher_amd/csrc/build.py) -- never falls back to anything."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise SwkError("libswk.so not built: run `python swiftwatcher_amd/csrc/build.py` "
                               "(there is no CPU fallback)")
            _preload_torch_hip_runtime()
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(lib, name)          # AttributeError = ABI mismatch, let it surface
                fn.restype = res
                fn.argtypes = args
            if lib.swk_abi_version() != ABI_VERSION:
                raise SwkError("libswk.so ABI version mismatch")
            _lib = lib
    return _lib


def default_params(**overrides):
    p = Params()
    load().swk_params_default(ctypes.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError("unknown swk parameter %r" % k)
        setattr(p, k, v)
    return p


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class _SerialisedLib:
    """The library's entry points with a lock held for the duration of every call.  A swk_ctx is not thread-safe
    (include/swk.h), ctypes drops the GIL while a call runs, and the counting loop's producer thread (pipeline.py,
    windows_per_call > 1) segments the next windows while the consumer thread cuts classifier inputs on the same
    context: every call on one Context is therefore serialised here."""

    def __init__(self, lib, lock):
        self._lib, self._lock = lib, lock

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        lock = self._lock

        def call(*args):
            with lock:
                return fn(*args)
        call.__name__ = name
        setattr(self, name, call)
        return call


class Context:
    """One per process per GPU (swk_ctx).  The C object is not thread-safe; this wrapper serialises calls on it."""

    def __init__(self, device=0, max_windows=0, max_n=0, max_Hc=0, max_Wc=0):
        self._lock = threading.RLock()
        self._lib = _SerialisedLib(load(), self._lock)
        self._h = ctypes.c_void_p()
        rc = self._lib.swk_ctx_create(device, max_windows, max_n, max_Hc, max_Wc, ctypes.byref(self._h))
        if rc != 0:
            msg = self._lib.swk_last_error(None)
            self._h = None
            raise SwkError("swk_ctx_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.device = device
        self.generation = 0          # batches run on this context: what a batch left on the device is gone once it moves on
        self._plane_pool = {}        # size -> free device buffers of that size (stage images kept on the GPU, see DevicePlanes)

    def close(self):
        if getattr(self, "_h", None):
            for ptrs in self._plane_pool.values():
                for p in ptrs:
                    self._lib.swk_device_free(self._h, ctypes.c_void_p(p))
            self._plane_pool = {}
            self._lib.swk_ctx_destroy(self._h)
            self._h = None

    # ---- device memory the caller keeps (stage images that are only copied to the host when somebody reads them) ----
    def device_alloc(self, nbytes):
        ptr = ctypes.c_void_p()
        self._check(self._lib.swk_device_alloc(self._h, int(nbytes), ctypes.byref(ptr)))
        return ptr.value

    def device_free(self, ptr):
        if getattr(self, "_h", None) and ptr:
            self._check(self._lib.swk_device_free(self._h, ctypes.c_void_p(ptr)))

    def device_read(self, ptr, shape, dtype=np.uint8):
        out = np.empty(shape, dtype)
        self._check(self._lib.swk_device_read(self._h, ctypes.c_void_p(ptr), _ptr(out), out.nbytes))
        return out

    def staging(self, shape):
        """A page-locked uint8 staging array of this shape, kept for the calling thread's next call with the same shape (calls on a
        context are synchronous: the upload out of it has finished when batch_run returns; a thread that segments ahead and the
        loop's own thread never share one)."""
        key = (threading.get_ident(), tuple(shape))
        with self._lock:
            cache = self.__dict__.setdefault("_staging", {})
            arr = cache.get(key)
            if arr is None:
                if len(cache) >= 3:
                    cache.pop(next(iter(cache)))          # (an evicted array lives on while its user holds it)
                arr = cache[key] = pinned_empty(shape, np.uint8, device=self.device)
        return arr

    def take_planes(self, nbytes):
        """A device buffer of nbytes from the context's free list (or a new one): see DevicePlanes."""
        with self._lock:
            free = self._plane_pool.get(nbytes)
            if free:
                return free.pop()
        return self.device_alloc(nbytes)

    def give_planes(self, ptr, nbytes, keep=4):
        if not getattr(self, "_h", None):
            return
        with self._lock:
            free = self._plane_pool.setdefault(nbytes, [])
            if len(free) < keep:
                free.append(ptr)
                return
        self.device_free(ptr)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.swk_last_error(self._h)
            raise SwkError("libswk error %d: %s" % (rc, msg.decode() if msg else "?"))

    @property
    def device_bytes(self):
        return int(self._lib.swk_ctx_device_bytes(self._h))

    # ---- profiling hooks ----
    def prof_enable(self, on=True):
        self._check(self._lib.swk_prof_enable(self._h, int(bool(on))))

    def prof_reset(self):
        self._check(self._lib.swk_prof_reset(self._h))

    def prof(self):
        out = {}
        for i, name in enumerate(KERNEL_FAMILIES):
            ms, n = ctypes.c_double(), ctypes.c_int64()
            self._check(self._lib.swk_prof_get(self._h, i, ctypes.byref(ms), ctypes.byref(n)))
            out[name] = (ms.value, n.value)
        wi = ctypes.c_int64()
        self._check(self._lib.swk_prof_window_iters(self._h, ctypes.byref(wi)))
        out["window_iters"] = wi.value
        return out

    def set_ialm_variant(self, variant):
        self._check(self._lib.swk_set_ialm_variant(self._h, int(variant)))

    def set_pass_tuning(self, flags):
        self._check(self._lib.swk_set_pass_tuning(self._h, int(flags)))

    def set_sparse_speculation(self, factor):
        self._check(self._lib.swk_set_sparse_speculation(self._h, float(factor)))

    def set_integer_start(self, on):
        self._check(self._lib.swk_set_integer_start(self._h, int(bool(on))))

    def set_norm_guard(self, rel):
        self._check(self._lib.swk_set_norm_guard(self._h, float(rel)))

    @property
    def guard_windows(self):
        v = ctypes.c_int64(0)
        self._check(self._lib.swk_prof_guard_windows(self._h, ctypes.byref(v)))
        return v.value

    def set_start_refine(self, tau):
        """Estimated first-iteration error above which a window gets the accurate start (csrc/ialm_refine.hip); <= 0: never."""
        self._check(self._lib.swk_set_start_refine(self._h, float(tau)))

    @property
    def refined_windows(self):
        """(windows whose first iteration was refined, windows that wanted it and did not get it) since the context was made."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.swk_prof_refined_windows(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def last_stopping_norms(self, cap=4096):
        """(ratio ||Z||_F / ||X||_F of the last stopping test, bound on its relative error) per window of the last batch."""
        r, e = np.zeros(cap), np.zeros(cap)
        n = self._lib.swk_last_stopping_norms(self._h, _ptr(r), _ptr(e), cap)
        if n < 0:
            self._check(n)
        return r[:min(n, cap)], e[:min(n, cap)]

    def set_norm_speculation(self, factor):
        self._check(self._lib.swk_set_norm_speculation(self._h, float(factor)))

    @property
    def pass_bytes_per_element(self):
        v = ctypes.c_double(0)
        self._check(self._lib.swk_prof_pass_bytes_per_element(self._h, ctypes.byref(v)))
        return v.value

    @property
    def last_eig_sweeps(self):
        v = ctypes.c_int32(0)
        self._check(self._lib.swk_last_eig_sweeps(self._h, ctypes.byref(v)))
        return v.value

    @property
    def last_integer_start_windows(self):
        v = ctypes.c_int32(0)
        self._check(self._lib.swk_last_integer_start_windows(self._h, ctypes.byref(v)))
        return v.value

    def debug_ialm_start(self, windows, lmbda=0.01):
        """The start of the IALM alone on uint8 windows [nwin][n][P] (swk_debug_ialm_start), with the context's current pass
        variant and integer-start switch: dict of G [nwin][n][n] (the first Gram matrix as the small-matrix step reads it,
        unscaled), sumsq, maxv, int_gram, dual_norm, mu_0, thr_0, dnorm per window, nblk and gram8_ran of the batch."""
        x = np.ascontiguousarray(windows, np.uint8)
        nwin, n, P = x.shape
        G = np.zeros((nwin, n, n), np.float64)
        sumsq, maxv = np.zeros(nwin, np.uint64), np.zeros(nwin, np.uint32)
        int_gram, scal = np.zeros(nwin, np.int32), np.zeros((nwin, 4), np.float64)
        nblk, ran = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._check(self._lib.swk_debug_ialm_start(self._h, _ptr(x), nwin, n, P, float(lmbda), _ptr(G), _ptr(sumsq), _ptr(maxv),
                                                   _ptr(int_gram), _ptr(scal), _ptr(nblk), _ptr(ran)))
        return dict(G=G, sumsq=sumsq, maxv=maxv, int_gram=int_gram, dual_norm=scal[:, 0], mu_0=scal[:, 1], thr_0=scal[:, 2],
                    dnorm=scal[:, 3], nblk=int(nblk[0]), gram8_ran=int(ran[0]))

    def debug_ialm_first_step(self, windows, lmbda=0.01):
        """The start and the first step of the IALM alone on uint8 windows [nwin][n][P] (swk_debug_ialm_first_step), with the
        context's current pass variant, integer-start switch, solver and refinement threshold: dict of B_fin, B_std [nwin][n][n]
        (B_1 as iteration 1's pass would read it -- A_1 = M_1 B_1, M_1 pixels x frames -- and as the small-matrix step left it),
        refine, cond_sum, sweeps, int_gram, dual_norm, mu_0, thr_0, dnorm per window."""
        x = np.ascontiguousarray(windows, np.uint8)
        nwin, n, P = x.shape
        B_fin, B_std = np.zeros((nwin, n, n), np.float64), np.zeros((nwin, n, n), np.float64)
        refine, sweeps, int_gram = np.zeros(nwin, np.int32), np.zeros(nwin, np.int32), np.zeros(nwin, np.int32)
        cond_sum, scal = np.zeros(nwin, np.float64), np.zeros((nwin, 4), np.float64)
        self._check(self._lib.swk_debug_ialm_first_step(self._h, _ptr(x), nwin, n, P, float(lmbda), _ptr(B_fin), _ptr(B_std),
                                                        _ptr(refine), _ptr(cond_sum), _ptr(sweeps), _ptr(int_gram), _ptr(scal)))
        return dict(B_fin=B_fin, B_std=B_std, refine=refine, cond_sum=cond_sum, sweeps=sweeps, int_gram=int_gram,
                    dual_norm=scal[:, 0], mu_0=scal[:, 1], thr_0=scal[:, 2], dnorm=scal[:, 3])

    def last_host_stage(self, cap=256):
        """How each group of the last batch call reached the device (swk_last_host_stage): a list of STAGE_DENSE / STAGE_WHOLE /
        STAGE_ROWS / STAGE_2D, STAGE_DEVICE for a group read in place."""
        kinds = np.zeros(cap, np.int32)
        n = self._lib.swk_last_host_stage(self._h, _ptr(kinds), cap)
        if n < 0:
            self._check(n)
        return [int(k) for k in kinds[:min(n, cap)]]

    @property
    def redo_batches(self):
        v = ctypes.c_int64(0)
        self._check(self._lib.swk_prof_redo_batches(self._h, ctypes.byref(v)))
        return v.value

    @property
    def redo_windows(self):
        v = ctypes.c_int64(0)
        self._check(self._lib.swk_prof_redo_windows(self._h, ctypes.byref(v)))
        return v.value

    def set_eig_method(self, method):
        self._check(self._lib.swk_set_eig_method(self._h, int(method)))

    # ---- hot path ----
    def batch_run_raw(self, inp, params, out):
        """swk_batch_run.  Returns the batch's generation: the value Context.generation has while what this batch left on the device
        is still there (another thread's batch may already have moved it on by the time the caller looks at the attribute)."""
        with self._lock:
            self.generation += 1
            generation = self.generation
            self._check(self._lib.swk_batch_run(self._h, ctypes.byref(inp), ctypes.byref(params), ctypes.byref(out)))
        return generation

    def _group_io(self, frames, nwin, n, crop, reverse_frames, seg_cap, stages, want_A, want_E, device_stages=False):
        """One group's (Input, Output, result dict): frames checked, result arrays allocated and wired into the Output.
        frames: u8 (nwin*n, H, W[, 3]), contiguous along columns / channels; a numpy array, or a torch tensor on this context's
        GPU (read in place, SWK_MEM_DEVICE)."""
        F = nwin * n
        on_device = hasattr(frames, "data_ptr") and getattr(frames, "is_cuda", False)
        shape = tuple(frames.shape)
        if str(frames.dtype) != ("torch.uint8" if on_device else "uint8") or shape[0] != F or len(shape) not in (3, 4):
            raise ValueError("frames must be uint8 (nwin*n, H, W[, 3])")
        if on_device:
            strides, base = tuple(int(x) for x in frames.stride()), frames.data_ptr()          # (elements = bytes for uint8)
        else:
            strides, base = frames.strides, frames.ctypes.data
        ch = 1 if len(shape) == 3 else shape[3]
        if (len(shape) == 4 and (strides[3] != 1 or strides[2] != ch)) or (len(shape) == 3 and strides[2] != 1):
            raise ValueError("frames must be contiguous along columns/channels")
        H, W = shape[1], shape[2]
        x0, y0, Wc, Hc = crop if crop is not None else (0, 0, W, H)
        if x0 < 0 or y0 < 0 or x0 + Wc > W or y0 + Hc > H:
            raise ValueError("crop rectangle outside the frame")
        inp = Input(frames=base + ((F - 1) * strides[0] if reverse_frames else 0), mem=MEM_DEVICE if on_device else MEM_HOST,
                    channels=ch, nwin=nwin, n=n, Hc=Hc, Wc=Wc, x0=x0, y0=y0,
                    frame_stride=-strides[0] if reverse_frames else strides[0], row_stride=strides[1])
        res = {}
        out = Output(mem=MEM_HOST, seg_cap=seg_cap)
        if device_stages and stages:
            planes = res["planes"] = DevicePlanes(self, tuple(stages), F, Hc, Wc)
            out.planes_on_device = 1
            for name in stages:
                setattr(out, name, planes.pointer(name))
        else:
            for name in stages:
                res[name] = np.empty((F, Hc, Wc), np.uint8)
                setattr(out, name, res[name].ctypes.data)
        P = Hc * Wc
        if want_A:
            res["A"] = np.empty((nwin, P, n), np.float64)
            out.A = res["A"].ctypes.data
        if want_E:
            res["E"] = np.empty((nwin, P, n), np.float64)
            out.E = res["E"].ctypes.data
        res["iters"] = np.zeros(nwin, np.int32)
        res["nseg"] = np.zeros(F, np.int32)
        res["segs"] = np.zeros((F, seg_cap), SEGMENT_DTYPE)
        out.iters = res["iters"].ctypes.data
        out.nseg = res["nseg"].ctypes.data
        out.segs = res["segs"].ctypes.data
        return inp, out, res

    def batch_run(self, frames, nwin, n, crop=None, params=None, stages=STAGES, want_A=False, want_E=False, seg_cap=255,
                  device_stages=False, reverse_frames=False):
        """Host-buffer convenience wrapper.

        frames: u8 array (nwin*n, H, W, 3) or (nwin*n, H, W), C-contiguous in the last two/three axes
        crop:   (x0, y0, Wc, Hc) inside each frame, or None for the whole frame
        Returns dict with the requested stage stacks (nwin*n, Hc, Wc) u8, 'iters' (nwin,),
        'nseg' (nwin*n,), 'segs' structured array (nwin*n, seg_cap), 'generation' (see batch_run_raw), optionally 'A'/'E' (nwin, P, n).
        device_stages=True: the stage stacks stay on the GPU -- res['planes'] is a DevicePlanes whose read(stage, frame)
        copies one image to the host when somebody asks for it (swk_output.planes_on_device).
        reverse_frames=True: frame j of the batch is frames[F - 1 - j] (negative frame stride): a window that lies in memory in
        the order it was read becomes a queue (position 0 = newest) without being reversed.
        """
        inp, out, res = self._group_io(frames, nwin, n, crop, reverse_frames, seg_cap, stages, want_A, want_E, device_stages)
        res["generation"] = self.batch_run_raw(inp, params or default_params(), out)          # for swk_segment_inputs_last
        return res

    def batch_run_groups(self, groups, params=None, stages=STAGES, want_A=False, want_E=False, seg_cap=255, device_stages=False):
        """swk_batch_run_groups: several groups of windows (one video's windows each, each with its own geometry) in ONE call.
        groups: dicts with batch_run's per-batch arguments -- frames, nwin, n, and optionally crop, reverse_frames, seg_cap.
        frames may also be a device tensor (torch, on this context's GPU, C-contiguous along rows / columns / channels): it is
        read in place (SWK_MEM_DEVICE).  Returns one dict per group, in the shape batch_run returns; every dict carries the
        call's 'generation' (swk_segment_inputs_last then serves all groups' segments, group order, then frame order).
        device_stages=True: every group's stage stacks stay on the GPU (res['planes'], as batch_run's)."""
        params = params or default_params()
        G = len(groups)
        if G < 1:
            raise ValueError("no groups")
        ins = (Input * G)()
        outs = (Output * G)()
        results = []
        for g, grp in enumerate(groups):
            ins[g], outs[g], res = self._group_io(grp["frames"], int(grp["nwin"]), int(grp["n"]), grp.get("crop"),
                                                  bool(grp.get("reverse_frames", False)), int(grp.get("seg_cap", seg_cap)), stages,
                                                  want_A, want_E, device_stages)
            results.append(res)
        with self._lock:
            self.generation += 1
            generation = self.generation
            self._check(self._lib.swk_batch_run_groups(self._h, ins, G, ctypes.byref(params), outs))
        for res in results:
            res["generation"] = generation
        return results

    # ---- decoder hand-over ----
    def yuv420_to_bgr(self, y, u, v=None, rect=None, device_out=False):
        """swk_yuv420_to_bgr: 8-bit 4:2:0 frames -> BGR (cv2.cvtColor COLOR_YUV2BGR_I420 / _NV12 of OpenCV 4.1.0 restated, include/swk.h).
        y: uint8 (count, H, W) or (H, W).  I420: u, v uint8 (count, ceil(H/2), ceil(W/2)).  NV12: v=None and u the interleaved plane,
        (count, ceil(H/2), ceil(W/2), 2) or (count, ceil(H/2), 2 ceil(W/2)).  All numpy arrays, or all torch tensors on this
        context's GPU (read in place); contiguous along a row, any row pitch and frame stride (views are fine).
        rect: (x0, y0, Wr, Hr) inside the frame, None = the whole frame.  Returns BGR (count, Hr, Wr, 3) (no count axis for a 2-D y):
        a numpy array, or with device_out=True a torch uint8 tensor on the GPU -- what batch_run / batch_run_groups take as frames."""
        on_device = hasattr(y, "data_ptr") and getattr(y, "is_cuda", False)
        planes = [y, u] + ([v] if v is not None else [])
        want = "torch.uint8" if on_device else "uint8"
        if not on_device:
            planes = [p if isinstance(p, np.ndarray) and p.dtype == np.uint8 and p.ndim and p.strides[-1] == 1 else np.ascontiguousarray(p, np.uint8)
                      for p in planes]
        if any((hasattr(p, "data_ptr") and getattr(p, "is_cuda", False)) != on_device or str(p.dtype) != want for p in planes):
            raise ValueError("the planes must be uint8, all numpy arrays or all tensors on the context's GPU")
        single = len(planes[0].shape) == 2
        if single:
            planes = [p[None] for p in planes]

        def geometry(p):
            if on_device:
                return tuple(p.shape), tuple(int(x) for x in p.stride()), p.data_ptr()
            return p.shape, p.strides, p.ctypes.data
        (yshape, ystr, yptr), (cshape, cstr, uptr) = geometry(planes[0]), geometry(planes[1])
        if len(yshape) != 3 or ystr[2] != 1:
            raise ValueError("y must be (count, H, W), contiguous along a row")
        count, H, W = yshape
        ch, cw = (H + 1) // 2, (W + 1) // 2
        if v is not None:
            vshape, vstr, vptr = geometry(planes[2])
            if tuple(cshape) != (count, ch, cw) or tuple(vshape) != (count, ch, cw) or cstr[2] != 1 or tuple(vstr) != tuple(cstr):
                raise ValueError("u and v must be (count, ceil(H/2), ceil(W/2)) with equal strides, contiguous along a row")
            layout = YUV_I420
        else:
            vptr = None
            ok = (len(cshape) == 4 and tuple(cshape) == (count, ch, cw, 2) and cstr[3] == 1 and cstr[2] == 2) or \
                 (len(cshape) == 3 and tuple(cshape) == (count, ch, 2 * cw) and cstr[2] == 1)
            if not ok:
                raise ValueError("the NV12 chroma plane must be (count, ceil(H/2), ceil(W/2), 2) or (count, ceil(H/2), 2 ceil(W/2))")
            layout = YUV_NV12
        x0, y0, Wr, Hr = rect if rect is not None else (0, 0, W, H)
        src = Yuv420(y=yptr, u=uptr, v=vptr, mem=MEM_DEVICE if on_device else MEM_HOST, layout=layout, H=H, W=W,
                     y_row_stride=ystr[1], y_frame_stride=ystr[0], c_row_stride=cstr[1], c_frame_stride=cstr[0])
        shape = (count, int(Hr), int(Wr), 3) if Hr > 0 and Wr > 0 and count > 0 else (1, 1, 1, 3)          # (the library refuses those)
        if device_out:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % self.device)
            optr, omem = ctypes.c_void_p(out.data_ptr()), MEM_DEVICE
        else:
            out = np.empty(shape, np.uint8)
            optr, omem = _ptr(out), MEM_HOST
        self._check(self._lib.swk_yuv420_to_bgr(self._h, ctypes.byref(src), count, int(x0), int(y0), int(Hr), int(Wr), optr, omem))
        return out[0] if single else out

    def _yuv_source(self, y, u, v, subsampling, bits, msb_aligned, full_range):
        """(Yuv struct, count, H, W, single, the arrays the struct points into) of yuv_to_bgr's plane arguments"""
        bits, (sx, sy) = int(bits), (int(subsampling[0]), int(subsampling[1]))
        B = 2 if bits > 8 else 1
        np_dtype = np.uint16 if B == 2 else np.uint8
        on_device = hasattr(y, "data_ptr") and getattr(y, "is_cuda", False)
        if u is None and v is not None:
            raise ValueError("v without u")
        planes = [y] + ([u] if u is not None else []) + ([v] if v is not None else [])
        want = ("torch.uint16" if B == 2 else "torch.uint8") if on_device else np.dtype(np_dtype).name
        if not on_device:
            planes = [p if isinstance(p, np.ndarray) and p.dtype == np_dtype and p.ndim and p.strides[-1] == B else np.ascontiguousarray(p, np_dtype)
                      for p in planes]
        if any((hasattr(p, "data_ptr") and getattr(p, "is_cuda", False)) != on_device or str(p.dtype) != want for p in planes):
            raise ValueError("the planes must be %s, all numpy arrays or all tensors on the context's GPU" % np.dtype(np_dtype).name)
        single = len(planes[0].shape) == 2
        if single:
            planes = [p[None] for p in planes]

        def geometry(p):          # shape, strides in BYTES, address
            if on_device:
                return tuple(p.shape), tuple(int(x) * B for x in p.stride()), p.data_ptr()
            return tuple(p.shape), tuple(p.strides), p.ctypes.data
        yshape, ystr, yptr = geometry(planes[0])
        if len(yshape) != 3 or ystr[2] != B:
            raise ValueError("y must be (count, H, W), contiguous along a row")
        count, H, W = yshape
        uptr = vptr = None
        cstr = (0, 0)
        if u is None:
            layout = YUV_MONO
        else:
            if not (0 <= sx <= 2 and 0 <= sy <= 1):
                ch = cw = -1                                         # (the library refuses the shifts; no shape can be checked)
            else:
                ch, cw = ((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1
            cshape, cstr, uptr = geometry(planes[1])
            if v is not None:
                vshape, vstr, vptr = geometry(planes[2])
                if ch >= 0 and (cshape != (count, ch, cw) or vshape != cshape or cstr[2] != B or vstr != cstr):
                    raise ValueError("u and v must be (count, %d, %d) with equal strides, contiguous along a row" % (ch, cw))
                layout = YUV_PLANAR
            else:
                ok = (len(cshape) == 4 and cshape == (count, ch, cw, 2) and cstr[3] == B and cstr[2] == 2 * B) or \
                     (len(cshape) == 3 and cshape == (count, ch, 2 * cw) and cstr[2] == B)
                if ch >= 0 and not ok:
                    raise ValueError("the interleaved chroma plane must be (count, %d, %d, 2) or (count, %d, %d)" % (ch, cw, ch, 2 * cw))
                layout = YUV_SEMIPLANAR
        src = Yuv(y=yptr, u=uptr, v=vptr, mem=MEM_DEVICE if on_device else MEM_HOST, layout=layout, H=H, W=W,
                  y_row_stride=ystr[1], y_frame_stride=ystr[0], c_row_stride=cstr[1], c_frame_stride=cstr[0],
                  sx=sx, sy=sy, bits=bits, msb_aligned=int(bool(msb_aligned)), full_range=int(bool(full_range)))
        return src, count, H, W, single, planes

    def yuv_to_bgr(self, y, u=None, v=None, *, subsampling=(1, 1), bits=8, msb_aligned=False, full_range=False, rect=None, device_out=False):
        """swk_yuv_to_bgr: planar, semiplanar or mono YUV frames of 8..16 bits, limited or full range -> BGR (the definition in
        include/swk.h).  y: (count, H, W) or (H, W), uint8 at bits = 8 and uint16 above.  subsampling = (sx, sy), the chroma shifts:
        (0, 0) 4:4:4, (1, 0) 4:2:2, (1, 1) 4:2:0, (2, 0) 4:1:1; a chroma plane is (count, ceil(H / 2^sy), ceil(W / 2^sx)).  Planar: u
        and v.  Semiplanar (NV12, NV16, NV24, P010, P016, P210): v=None and u the interleaved plane, (count, ch, cw, 2) or
        (count, ch, 2 cw).  Mono: u=None.  msb_aligned: 16-bit words that hold the sample in their upper bits (P010).  All numpy
        arrays, or all torch tensors on this context's GPU (read in place); contiguous along a row, any row pitch and frame stride.
        rect: (x0, y0, Wr, Hr) inside the frame, None = the whole frame.  Returns BGR (count, Hr, Wr, 3) (no count axis for a 2-D y):
        a numpy array, or with device_out=True a torch uint8 tensor on the GPU -- what batch_run / batch_run_groups take as frames."""
        src, count, H, W, single, _keep = self._yuv_source(y, u, v, subsampling, bits, msb_aligned, full_range)
        x0, y0, Wr, Hr = rect if rect is not None else (0, 0, W, H)
        shape = (count, int(Hr), int(Wr), 3) if Hr > 0 and Wr > 0 and count > 0 else (1, 1, 1, 3)          # (the library refuses those)
        if device_out:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % self.device)
            optr, omem = ctypes.c_void_p(out.data_ptr()), MEM_DEVICE
        else:
            out = np.empty(shape, np.uint8)
            optr, omem = _ptr(out), MEM_HOST
        self._check(self._lib.swk_yuv_to_bgr(self._h, ctypes.byref(src), count, int(x0), int(y0), int(Hr), int(Wr), optr, omem))
        return out[0] if single else out

    def yuv_deinterlace(self, frames_or_planes, rect, tff, rate=2, temporal=True, has_prev=False, has_next=False, parity0=(0, 0),
                        want_planes=False, *, subsampling=(1, 1), bits=8, msb_aligned=False, full_range=False, device_out=False,
                        want_bgr=True):
        """swk_yuv_deinterlace: the fields of interlaced frames as whole pictures (the definition in include/swk.h).
        frames_or_planes: the planes (y, u, v), (y, uv) or (y,) as yuv_to_bgr takes them, with its format keywords -- or a list of
        io_y4m frames of one format (Yuv420Frame, YuvFrame, or the frames of a pipe's reader that hold one rectangle), of which the
        rectangle grown by the definition's footprint is gathered; the format and parity0 then come from the frames.
        rect: (x0, y0, Wr, Hr) in the picture, None = the whole picture.  tff: the top field is the earlier one.  rate: 2 = both
        fields of every frame, 1 = the first one.  has_prev / has_next: the first / last frame is context only.
        Returns BGR (nout, Hr, Wr, 3), nout = rate * (count - has_prev - has_next): a numpy array, or with device_out=True a torch
        tensor on the GPU.  want_planes: (BGR, (Y, U, V)) with the deinterlaced samples (U = V = None for mono); want_bgr=False: BGR
        is None."""
        if not isinstance(frames_or_planes, tuple) and hasattr(frames_or_planes[0], "y"):
            planes, fmt, rect, parity0 = _gather_fields(frames_or_planes, rect)
            subsampling, bits, full_range, msb_aligned = fmt[0], fmt[1], fmt[2], False
        else:
            planes = tuple(frames_or_planes)
        y, u, v = (tuple(planes) + (None, None))[:3]
        src, count, H, W, _single, _keep = self._yuv_source(y, u, v, subsampling, bits, msb_aligned, full_range)
        if _single:
            raise ValueError("deinterlacing takes frame stacks (count, H, W)")
        x0, y0, Wr, Hr = (int(c) for c in (rect if rect is not None else (0, 0, W, H)))
        d = Deinterlace(tff=int(bool(tff)), rate=int(rate), temporal=int(bool(temporal)), has_prev=int(bool(has_prev)),
                        has_next=int(bool(has_next)), y_parity0=int(parity0[0]), c_parity0=int(parity0[1]))
        nout = int(rate) * (count - d.has_prev - d.has_next)
        ok = Hr > 0 and Wr > 0 and nout > 0 and x0 >= 0 and y0 >= 0 and 0 <= src.sx <= 2 and 0 <= src.sy <= 1          # (else the library refuses)
        sx, sy = (0, 0) if u is None else (src.sx, src.sy)
        ch, cw = (((y0 + Hr - 1) >> sy) - (y0 >> sy) + 1, ((x0 + Wr - 1) >> sx) - (x0 >> sx) + 1) if ok else (1, 1)
        luma, chroma = (nout * Hr * Wr, 0 if u is None else nout * ch * cw) if ok else (1, 0)
        dt = np.uint16 if src.bits > 8 else np.uint8
        bgr = pl = None
        bptr = pptr = None
        mem = MEM_DEVICE if device_out else MEM_HOST
        if device_out:
            import torch
            if want_bgr:
                bgr = torch.empty((nout, Hr, Wr, 3) if ok else (1, 1, 1, 3), dtype=torch.uint8, device="cuda:%d" % self.device)
                bptr = ctypes.c_void_p(bgr.data_ptr())
            if want_planes:
                pl = torch.empty(luma + 2 * chroma, dtype=torch.uint16 if src.bits > 8 else torch.uint8, device="cuda:%d" % self.device)
                pptr = ctypes.c_void_p(pl.data_ptr())
        else:
            if want_bgr:
                bgr = np.empty((nout, Hr, Wr, 3) if ok else (1, 1, 1, 3), np.uint8)
                bptr = _ptr(bgr)
            if want_planes:
                pl = np.empty(luma + 2 * chroma, dt)
                pptr = _ptr(pl)
        self._check(self._lib.swk_yuv_deinterlace(self._h, ctypes.byref(src), ctypes.byref(d), count, x0, y0, Hr, Wr, bptr, mem, pptr, mem))
        if not want_planes:
            return bgr
        Y = pl[:luma].reshape(nout, Hr, Wr)
        if u is None:
            return bgr, (Y, None, None)
        return bgr, (Y, pl[luma:luma + chroma].reshape(nout, ch, cw), pl[luma + chroma:].reshape(nout, ch, cw))

    # ---- review video ----
    def _review_io(self, frames, rect, layout, device_out, dst, out_hw=None):
        """(Input, Yuv420Dst, result planes) of bgr_to_yuv420 / render_review.  frames: uint8 (F, H, W, 3) BGR or (F, H, W) gray, a
        numpy array or a torch tensor on this context's GPU (read in place), contiguous along columns / channels, any row pitch and
        frame stride.  dst: a ready Yuv420Dst (the planes are then the caller's business) or None.  out_hw: Input -> the size of the
        result's frames where it is not the rectangle's (a mosaic)."""
        on_device = hasattr(frames, "data_ptr") and getattr(frames, "is_cuda", False)
        shape = tuple(frames.shape)
        if str(frames.dtype) != ("torch.uint8" if on_device else "uint8") or len(shape) not in (3, 4):
            raise ValueError("frames must be uint8 (F, H, W[, C])")
        if on_device:
            strides, base = tuple(int(x) for x in frames.stride()), frames.data_ptr()
        else:
            strides, base = frames.strides, frames.ctypes.data
        ch = 1 if len(shape) == 3 else shape[3]
        if (len(shape) == 4 and (strides[3] != 1 or strides[2] != ch)) or (len(shape) == 3 and strides[2] != 1):
            raise ValueError("frames must be contiguous along columns/channels")
        F, H, W = shape[:3]
        x0, y0, Wc, Hc = rect if rect is not None else (0, 0, W, H)
        if x0 < 0 or y0 < 0 or x0 + Wc > W or y0 + Hc > H:
            raise ValueError("rectangle outside the frame")
        inp = Input(frames=base, mem=MEM_DEVICE if on_device else MEM_HOST, channels=ch, nwin=1, n=F, Hc=Hc, Wc=Wc, x0=x0, y0=y0,
                    frame_stride=strides[0], row_stride=strides[1])
        if dst is not None:
            return inp, dst, None
        if layout not in ("i420", "nv12"):
            raise ValueError('layout is "i420" or "nv12"')
        Fa, Ha, Wa = max(F, 1), max(Hc, 1), max(Wc, 1)               # (the library refuses empty ones)
        if out_hw is not None:
            Ha, Wa = out_hw(inp)
        hc, wc = (Ha + 1) // 2, (Wa + 1) // 2
        cshape = (Fa, hc, wc) if layout == "i420" else (Fa, hc, wc, 2)
        nplanes = 3 if layout == "i420" else 2
        if device_out:
            import torch
            planes = [torch.empty(sh, dtype=torch.uint8, device="cuda:%d" % self.device) for sh in [(Fa, Ha, Wa)] + [cshape] * (nplanes - 1)]
            ptrs = [p.data_ptr() for p in planes]
        else:
            planes = [np.empty(sh, np.uint8) for sh in [(Fa, Ha, Wa)] + [cshape] * (nplanes - 1)]
            ptrs = [p.ctypes.data for p in planes]
        crow = wc * (1 if layout == "i420" else 2)
        dst = Yuv420Dst(y=ptrs[0], u=ptrs[1], v=ptrs[2] if nplanes == 3 else None, mem=MEM_DEVICE if device_out else MEM_HOST,
                        layout=YUV_I420 if layout == "i420" else YUV_NV12, y_row_stride=Wa, y_frame_stride=Ha * Wa,
                        c_row_stride=crow, c_frame_stride=hc * crow)
        return inp, dst, tuple(planes)

    def bgr_to_yuv420(self, frames, rect=None, layout="i420", device_out=False, dst=None):
        """swk_bgr_to_yuv420: BGR (F, H, W, 3) or gray (F, H, W) uint8 frames -> 8-bit 4:2:0 (cv2.cvtColor COLOR_BGR2YUV_I420 of OpenCV
        4.1.0 restated, include/swk.h; chroma from each cell's top-left pixel).  frames: a numpy array or a torch tensor on this
        context's GPU.  rect: (x0, y0, Wr, Hr) inside the frame, None = the whole frame.  Returns (y, u, v) for layout "i420" --
        y (F, Hr, Wr), u and v (F, ceil(Hr / 2), ceil(Wr / 2)) -- or (y, uv) for "nv12", uv (F, ceil(Hr / 2), ceil(Wr / 2), 2): numpy
        arrays, or with device_out=True torch uint8 tensors on the GPU.  dst: a Yuv420Dst of the caller's (any strides, host or
        device); nothing is returned then."""
        inp, dst, planes = self._review_io(frames, rect, layout, device_out, dst)
        self._check(self._lib.swk_bgr_to_yuv420(self._h, ctypes.byref(inp), ctypes.byref(dst)))
        return planes

    def render_review(self, frames, boxes=None, marks=None, frame_style=None, mask=None, styles=None, mask_style=0, mark_arm=0, border=0,
                      rect=None, layout="i420", device_out=False, dst=None, labels=None, _panels=None):
        """swk_render_review: bgr_to_yuv420 of the frames composed with an overlay (include/swk.h): boxes -- REVIEW_BOX_DTYPE records
        or rows (frame, r0, c0, r1, c1, style), ascending frame --, marks -- REVIEW_MARK_DTYPE records or rows (frame, r, c, style),
        ascending frame --, frame_style (F,) int32 border style per frame, mask (Hr, Wr) uint8 tinted in mask_style where != 0, styles
        -- REVIEW_STYLE_DTYPE records or rows (b, g, r, fill_alpha, line_alpha); style k is styles[k - 1], 0 draws nothing.
        labels (None: swk_render_review is called; else swk_render_review_labels, the fifth layer) -- REVIEW_LABEL_DTYPE records or
        tuples (frame, r, c, style, plate, scale, text), ascending frame, text a str or bytes of the font's character set."""
        def records(a, dtype, cols):
            if a is None:
                return np.zeros(0, dtype)
            if isinstance(a, np.ndarray) and a.dtype == dtype:
                return np.ascontiguousarray(a)
            rows = np.asarray(a, dtype=np.int64).reshape(-1, len(cols))
            out = np.zeros(len(rows), dtype)
            for k, name in enumerate(cols):
                out[name] = rows[:, k]
            return out
        boxes = records(boxes, REVIEW_BOX_DTYPE, ("frame", "r0", "c0", "r1", "c1", "style"))
        marks = records(marks, REVIEW_MARK_DTYPE, ("frame", "r", "c", "style"))
        if isinstance(styles, np.ndarray) and styles.dtype == REVIEW_STYLE_DTYPE:
            styles = np.ascontiguousarray(styles)
        else:
            rows = np.asarray(styles if styles is not None else [], dtype=np.int64).reshape(-1, 5)
            if rows.size and (rows[:, :3].min() < 0 or rows[:, :3].max() > 255):
                raise ValueError("a style's colour is three bytes (b, g, r)")
            styles = np.zeros(len(rows), REVIEW_STYLE_DTYPE)
            for k, name in enumerate(("b", "g", "r", "fill_alpha", "line_alpha")):
                styles[name] = rows[:, k]
        out_hw = None
        if _panels is not None:
            specs, cols = _panels
            out_hw = lambda inp: panel_layout(max(inp.Hc, 1), max(inp.Wc, 1), 1 + len(specs), max(cols, 1))[:2]          # noqa: E731
        inp, dst, planes = self._review_io(frames, rect, layout, device_out, dst, out_hw)
        if frame_style is not None:
            frame_style = np.ascontiguousarray(frame_style, np.int32)
            if frame_style.shape != (inp.n,):
                raise ValueError("frame_style holds one style per frame")
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (inp.Hc, inp.Wc):
                raise ValueError("mask must be (Hr, Wr)")
        rv = Review(mask=mask.ctypes.data if mask is not None else None, mask_style=int(mask_style),
                    boxes=boxes.ctypes.data if len(boxes) else None, nboxes=len(boxes),
                    marks=marks.ctypes.data if len(marks) else None, nmarks=len(marks), mark_arm=int(mark_arm),
                    frame_style=frame_style.ctypes.data if frame_style is not None else None, border=int(border),
                    styles=styles.ctypes.data if len(styles) else None, nstyles=len(styles))
        if labels is None and _panels is None:
            self._check(self._lib.swk_render_review(self._h, ctypes.byref(inp), ctypes.byref(rv), ctypes.byref(dst)))
            return planes
        labels = label_records(labels if labels is not None else ())
        if _panels is not None:
            structs, keep = self._panel_structs(specs, inp)
            self._check(self._lib.swk_render_review_panels(self._h, ctypes.byref(inp), ctypes.byref(rv), labels.ctypes.data if len(labels) else None,
                                                           len(labels), structs, len(specs), int(cols), ctypes.byref(dst)))
            del keep
            return planes
        self._check(self._lib.swk_render_review_labels(self._h, ctypes.byref(inp), ctypes.byref(rv), labels.ctypes.data if len(labels) else None,
                                                       len(labels), ctypes.byref(dst)))
        return planes

    def _panel_structs(self, specs, inp):
        """(ReviewPanel array or None, the arrays it points into) of render_review_panels' panel dicts."""
        if not specs:
            return None, ()
        F = inp.nwin * inp.n
        structs, keep = (ReviewPanel * len(specs))(), []
        for k, spec in enumerate(specs):
            spec = dict(spec)
            plane, kind = spec.pop("plane"), spec.pop("kind", "gray")
            if kind not in ("gray", "labels", PANEL_GRAY, PANEL_LABELS):
                raise ValueError('a panel\'s kind is "gray" or "labels"')
            p = structs[k]
            p.kind = PANEL_LABELS if kind in ("labels", PANEL_LABELS) else PANEL_GRAY
            p.gain, p.layers = int(spec.pop("gain", 1)), int(spec.pop("layers", 0))
            if isinstance(plane, dict):                               # a raw plane: ptr, frame_stride, row_stride, mem
                p.plane, p.mem = plane["ptr"], plane.get("mem", MEM_DEVICE)
                p.frame_stride, p.row_stride = plane["frame_stride"], plane["row_stride"]
            else:
                on_device = hasattr(plane, "data_ptr") and getattr(plane, "is_cuda", False)
                shape = tuple(plane.shape)
                if str(plane.dtype) != ("torch.uint8" if on_device else "uint8") or shape != (F, inp.Hc, inp.Wc):
                    raise ValueError("a panel's plane is uint8 (F, Hr, Wr)")
                strides = tuple(int(x) for x in plane.stride()) if on_device else plane.strides
                if strides[2] != 1:
                    raise ValueError("a panel's plane must be contiguous along columns")
                p.plane, p.mem = (plane.data_ptr() if on_device else plane.ctypes.data), (MEM_DEVICE if on_device else MEM_HOST)
                p.frame_stride, p.row_stride = strides[0], strides[1]
                keep.append(plane)
            caption = spec.pop("caption", None)
            if spec:
                raise ValueError("unknown panel entries: %s" % ", ".join(sorted(spec)))
            rec = label_records([(0,) + tuple(caption) if caption is not None else (0, 0, 0, 0, 0, 1, b"")])          # (none: len 0 at a valid scale)
            ctypes.memmove(ctypes.addressof(p.caption), rec.ctypes.data, 64)
        return structs, keep

    def render_review_panels(self, frames, panels=(), cols=1, **kw):
        """swk_render_review_panels: render_review's frames (its remaining arguments; labels=None: none) as cell 0 of a mosaic whose
        further cells are stage images of the same frames (include/swk.h; panel_layout gives the geometry).  panels: dicts with
        plane -- uint8 (F, Hr, Wr), a numpy array (any frame and row strides) or a torch tensor on this context's GPU, or a dict
        (ptr, frame_stride, row_stride[, mem]) naming device memory --, kind "gray" (default) or "labels", gain (gray, 1..255,
        default 1), layers (bits 0..3: mask, boxes, marks, border drawn on the panel; default 0) and caption -- None or
        (r, c, style, plate, scale, text).  cols: cells per mosaic row.  Returns render_review's planes at the mosaic's size."""
        return self.render_review(frames, _panels=(list(panels), int(cols)), **kw)

    # ---- stage-level entry points ----
    def bgr2gray(self, bgr, gray_mode=GRAY_Q14):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        single = bgr.ndim == 3
        b4 = bgr[None] if single else bgr
        cnt, H, W, _ = b4.shape
        out = np.empty((cnt, H, W), np.uint8)
        self._check(self._lib.swk_bgr2gray(self._h, _ptr(b4), cnt, H, W, gray_mode, _ptr(out)))
        return out[0] if single else out

    def ialm(self, planes, lmbda=0.01, tol=0.001, maxiter=100, want_E=True):
        """planes: u8 (n, P).  Returns A (P, n), E (P, n) or None, iterations."""
        planes = np.ascontiguousarray(planes, np.uint8)
        n, P = planes.shape
        A = np.empty((P, n), np.float64)
        E = np.empty((P, n), np.float64) if want_E else None
        it = np.zeros(1, np.int32)
        self._check(self._lib.swk_ialm(self._h, _ptr(planes), n, P, lmbda, tol, maxiter, _ptr(A), _ptr(E), _ptr(it)))
        return A, E, int(it[0])

    def rpca_epilogue(self, E):
        E = np.ascontiguousarray(E, np.float64)
        out = np.empty(E.shape, np.uint8)
        self._check(self._lib.swk_rpca_epilogue(self._h, _ptr(E), E.size, _ptr(out)))
        return out

    def _planes(self, a):
        a = np.ascontiguousarray(a, np.uint8)
        return (a[None], True) if a.ndim == 2 else (a, False)

    def bilateral_u8(self, src, d=7, sigma_color=15.0, sigma_space=1.0, use_fma=False):
        s, single = self._planes(src)
        out = np.empty_like(s)
        self._check(self._lib.swk_bilateral_u8(self._h, _ptr(s), s.shape[0], s.shape[1], s.shape[2], d,
                                               sigma_color, sigma_space, int(bool(use_fma)), _ptr(out)))
        return out[0] if single else out

    def thresh_tozero_u8(self, src, thresh=15):
        s = np.ascontiguousarray(src, np.uint8)
        out = np.empty_like(s)
        self._check(self._lib.swk_thresh_tozero_u8(self._h, _ptr(s), s.size, thresh, _ptr(out)))
        return out

    def grey_open3x3_u8(self, src):
        s, single = self._planes(src)
        out = np.empty_like(s)
        self._check(self._lib.swk_grey_open3x3_u8(self._h, _ptr(s), s.shape[0], s.shape[1], s.shape[2], _ptr(out)))
        return out[0] if single else out

    def grey_open_u8(self, src, size):
        """scipy.ndimage.grey_opening(size=(kh, kw)) on u8 images, any window."""
        s, single = self._planes(src)
        out = np.empty_like(s)
        self._check(self._lib.swk_grey_open_u8(self._h, _ptr(s), s.shape[0], s.shape[1], s.shape[2], int(size[0]), int(size[1]), _ptr(out)))
        return out[0] if single else out

    def resize_linear_u8(self, frame, dsize):
        """cv2.resize(frame, dsize=(width, height)) (INTER_LINEAR) for one (H, W[, C]) u8 frame."""
        f = np.ascontiguousarray(frame, np.uint8)
        H, W = f.shape[:2]
        ch = 1 if f.ndim == 2 else f.shape[2]
        dW, dH = int(dsize[0]), int(dsize[1])
        out = np.empty((dH, dW) + ((ch,) if f.ndim == 3 else ()), np.uint8)
        self._check(self._lib.swk_resize_linear_u8(self._h, _ptr(f), 1, H, W, ch, dH, dW, _ptr(out)))
        return out

    def ccl_u8(self, src, connectivity=8, label_order=ORDER_BLOCK2X2):
        s, single = self._planes(src)
        lab = np.empty(s.shape, np.int32)
        nc = np.zeros(s.shape[0], np.int32)
        self._check(self._lib.swk_ccl_u8(self._h, _ptr(s), s.shape[0], s.shape[1], s.shape[2], connectivity,
                                         label_order, _ptr(lab), _ptr(nc)))
        return (int(nc[0]), lab[0]) if single else (nc, lab)

    def classifier_input(self, crops, mean, std, want_patches=False, net_ptr=None, pad=100, channels_last=False):
        """swk_classifier_input_window for a list of HxWx3 uint8 crops.  Returns (patches or None, net or None):
        net is a float32 host array (n, 3, S, S), S = 24 + 2 pad, unless net_ptr (a device pointer with room for
        it) is given.  pad = 100 is the reference's full 224x224 input.  channels_last: the network input is written
        [S][S][3] per segment (a torch.channels_last tensor) instead of planes."""
        n = len(crops)
        flat = [np.ascontiguousarray(c, np.uint8).reshape(-1) for c in crops]
        sizes = np.array([f.size for f in flat], np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        packed = np.concatenate(flat) if n else np.zeros(0, np.uint8)
        hw = np.array([[c.shape[0], c.shape[1]] for c in crops], np.int32)
        m = np.asarray(mean, np.float32)
        s = np.asarray(std, np.float32)
        patches = np.empty((n, 24, 24, 3), np.uint8) if want_patches else None
        net = None
        if net_ptr is None:
            net = np.empty((n, 3, 24 + 2 * pad, 24 + 2 * pad), np.float32)
            nptr, nmem = _ptr(net), MEM_HOST
        else:
            nptr, nmem = ctypes.c_void_p(net_ptr), MEM_DEVICE
        self._check(self._lib.swk_classifier_input_window(self._h, _ptr(packed), packed.size, _ptr(offsets), _ptr(hw), n,
                                                          _ptr(m), _ptr(s), int(pad), 1 if channels_last else 0, _ptr(patches), nptr,
                                                          nmem))
        return patches, net

    def segment_inputs(self, inp, frame_hw, segs_ptr, nseg_ptr, seg_cap, mean, std, net_ptr, net_cap, first=0, pad=8,
                       min_seg_size=(24, 24), seg_frame_ptr=None, channels_last=False):
        """swk_segment_inputs: classifier inputs cut on the device from the frames (inp, device-resident BGR) and the
        region records of a batch_run with device outputs.  Returns (total segments in the batch, skipped boxes)."""
        m = np.asarray(mean, np.float32)
        s = np.asarray(std, np.float32)
        total = ctypes.c_int32(0)
        skipped = ctypes.c_int32(0)
        self._check(self._lib.swk_segment_inputs(self._h, ctypes.byref(inp), int(frame_hw[0]), int(frame_hw[1]),
                                                 ctypes.c_void_p(segs_ptr), ctypes.c_void_p(nseg_ptr), int(seg_cap),
                                                 int(min_seg_size[0]), int(min_seg_size[1]), _ptr(m), _ptr(s), int(pad),
                                                 1 if channels_last else 0, int(first), int(net_cap), ctypes.c_void_p(net_ptr),
                                                 ctypes.c_void_p(seg_frame_ptr) if seg_frame_ptr else None,
                                                 ctypes.byref(total), ctypes.byref(skipped)))
        return total.value, skipped.value

    def segment_inputs_last(self, generation, mean, std, net_ptr, net_cap, first=0, pad=8, min_seg_size=(24, 24),
                            seg_frame_ptr=None, channels_last=False, known_total=-1):
        """swk_segment_inputs_last: the same for the batch this context ran LAST (its own device copy of the frames, its own
        region records).  generation = Context.generation right after that batch_run: raises StaleBatch when the context
        has run another batch since (the buffers hold something else now).  Returns (total, skipped)."""
        m = np.asarray(mean, np.float32)
        s = np.asarray(std, np.float32)
        total = ctypes.c_int32(int(known_total))
        skipped = ctypes.c_int32(0)
        with self._lock:                 # nothing may slip in between the generation test and the call
            if generation != self.generation:
                raise StaleBatch("the context has run another batch since")
            rc = self._lib.swk_segment_inputs_last(self._h, int(min_seg_size[0]), int(min_seg_size[1]), _ptr(m), _ptr(s), int(pad),
                                                   1 if channels_last else 0, int(first), int(net_cap), ctypes.c_void_p(net_ptr),
                                                   ctypes.c_void_p(seg_frame_ptr) if seg_frame_ptr else None,
                                                   ctypes.byref(total), ctypes.byref(skipped))
            if rc == ERR_STALE:
                raise StaleBatch("the context no longer holds that batch")
            self._check(rc)
        return total.value, skipped.value

    def debug_resize_table(self, first, count, route=1):
        """swk_debug_resize_table: (bounds (count, 24, 2), coeffs (count, 24, 343)) int32, the device's Pillow resize tables of the
        input sizes first .. first + count - 1 (route 1: the large-crop kernel's, sizes up to 4096; route 0: the <= 512 kernels')."""
        bounds = np.empty((count, 24, 2), np.int32)
        coeffs = np.empty((count, 24, 343), np.int32)
        self._check(self._lib.swk_debug_resize_table(self._h, int(first), int(count), int(route), _ptr(bounds), _ptr(coeffs)))
        return bounds, coeffs

    def debug_filter_fused(self, src, params=None, geom=None, bilateral=True, thresh=True):
        """swk_debug_filter_fused: the batch calls' fused filter kernel alone, on planes of the caller's choosing.  src: (count, H, W)
        u8 planes (the uniform launcher), or with geom = [(H, W, byte offset), ...] a flat u8 buffer that holds the planes (the
        per-frame-geometry launcher).  bilateral / thresh = False hand the launcher a null pointer for that stage.  Returns a dict
        of the stages asked for and "opened", shaped like src, and "guard": (3, DEBUG_GUARD_BYTES) u8, the bytes behind the device's
        opened, bilateral and thresholded outputs (DEBUG_FILL where untouched)."""
        s = np.ascontiguousarray(src, np.uint8)
        p = params if params is not None else default_params()
        if geom is None:
            if s.ndim != 3:
                raise ValueError("planes must be (count, H, W)")
            count, H, W, tab, total = s.shape[0], s.shape[1], s.shape[2], None, s.size
        else:
            if s.ndim != 1:
                raise ValueError("with geom the planes lie in a flat buffer")
            tab = np.array([tuple(int(v) for v in g) for g in geom], DEBUG_PLANE_DTYPE)
            count, H, W, total = len(tab), 0, 0, s.size
        out = {k: np.empty_like(s) for k, on in (("bilateral", bilateral), ("thresh", thresh), ("opened", True)) if on}
        guard = np.zeros((3, DEBUG_GUARD_BYTES), np.uint8)
        self._check(self._lib.swk_debug_filter_fused(self._h, _ptr(s), count, H, W, _ptr(tab), total, ctypes.byref(p),
                                                     _ptr(out.get("bilateral")), _ptr(out.get("thresh")), _ptr(out["opened"]), _ptr(guard)))
        out["guard"] = guard
        return out

    def debug_ccl_frame_props(self, opened, connectivity=8, label_order=ORDER_BLOCK2X2, seg_cap=255):
        """swk_debug_ccl_frame_props: the batch calls' one-workgroup labeller with region records alone, on (count, H, W) u8 planes of
        the caller's choosing.  Returns (labels (count, H, W) u8, segs (count, seg_cap), nseg (count,))."""
        s = np.ascontiguousarray(opened, np.uint8)
        if s.ndim != 3:
            raise ValueError("planes must be (count, H, W)")
        lab = np.empty_like(s)
        segs = np.zeros((s.shape[0], seg_cap), SEGMENT_DTYPE)
        nseg = np.zeros(s.shape[0], np.int32)
        self._check(self._lib.swk_debug_ccl_frame_props(self._h, _ptr(s), s.shape[0], s.shape[1], s.shape[2], int(connectivity),
                                                        int(label_order), int(seg_cap), _ptr(lab), _ptr(segs), _ptr(nseg)))
        return lab, segs, nseg

    def force_ccl_multi_kernel(self, on=True):
        """swk_debug_force_ccl_multi_kernel: ccl_u8 and the batch calls label every frame size by the multi-kernel path (results never
        depend on it)."""
        self._check(self._lib.swk_debug_force_ccl_multi_kernel(self._h, int(bool(on))))

    def max_windows(self):
        """swk_debug_max_windows: the largest window count of one IALM (sub-)batch the device takes (its grid y extent)."""
        v = int(self._lib.swk_debug_max_windows(self._h))
        if v < 0:
            self._check(v)
        return v

    def regionprops_u8(self, labels, seg_cap=255):
        s, single = self._planes(labels)
        segs = np.zeros((s.shape[0], seg_cap), SEGMENT_DTYPE)
        nseg = np.zeros(s.shape[0], np.int32)
        self._check(self._lib.swk_regionprops_u8(self._h, _ptr(s), s.shape[0], s.shape[1], s.shape[2], seg_cap,
                                                 _ptr(segs), _ptr(nseg)))
        return (segs[0, :nseg[0]], int(nseg[0])) if single else (segs, nseg)

    def segment_shapes_raw(self, ptr, mem, count, H, W, frame_stride, row_stride, seg_cap, shapes, nseg):
        """swk_segment_shapes_u8 on a raw plane pointer; shapes / nseg: the arrays it fills (or None, to probe its refusals)."""
        self._check(self._lib.swk_segment_shapes_u8(self._h, ptr, int(mem), int(count), int(H), int(W), int(frame_stride), int(row_stride),
                                                    int(seg_cap), _ptr(shapes), _ptr(nseg)))

    def segment_shapes_u8(self, labels, seg_cap=255):
        """swk_segment_shapes_u8: the shape sums (SHAPE_DTYPE records, ascending label: record k of frame f is the region of
        regionprops_u8's segs[f][k]) of u8 label planes.  labels: a host array (F, H, W) or (H, W) of any frame and row strides
        (copied up), or planes that are on the GPU and are read where they lie -- a DevicePlanes with a "labels" stage, a torch
        uint8 tensor (F, H, W) on this context's GPU, or a dict (ptr, shape=(F, H, W)[, frame_stride, row_stride]) naming device
        memory.  Returns (records (F, seg_cap), nseg (F,)); for one (H, W) plane (records[:nseg], nseg)."""
        single = False
        keep = labels
        if isinstance(labels, DevicePlanes):
            F, H, W = labels.F, labels.Hc, labels.Wc
            ptr, mem, fs, rs = labels.pointer("labels"), MEM_DEVICE, H * W, W
        elif isinstance(labels, dict):
            F, H, W = (int(x) for x in labels["shape"])
            ptr, mem = labels["ptr"], labels.get("mem", MEM_DEVICE)
            rs = int(labels.get("row_stride", W))
            fs = int(labels.get("frame_stride", H * rs))
        elif hasattr(labels, "data_ptr") and getattr(labels, "is_cuda", False):
            if str(labels.dtype) != "torch.uint8" or labels.dim() != 3 or labels.stride(2) != 1:
                raise ValueError("device label planes are uint8 (F, H, W), contiguous along columns")
            F, H, W = (int(x) for x in labels.shape)
            ptr, mem, fs, rs = labels.data_ptr(), MEM_DEVICE, int(labels.stride(0)), int(labels.stride(1))
        else:
            s = np.asarray(labels)
            if s.dtype != np.uint8 or s.ndim not in (2, 3):
                raise ValueError("label planes are uint8 (F, H, W) or (H, W)")
            single = s.ndim == 2
            if single:
                s = s[None]
            if s.strides[2] != 1 or s.strides[1] < s.shape[2]:
                s = np.ascontiguousarray(s)
            keep = s
            F, H, W = s.shape
            ptr, mem, fs, rs = s.ctypes.data, MEM_HOST, s.strides[0], s.strides[1]
        shapes = np.zeros((F, seg_cap), SHAPE_DTYPE)
        nseg = np.zeros(F, np.int32)
        self.segment_shapes_raw(ptr, mem, F, H, W, fs, rs, seg_cap, shapes, nseg)
        del keep
        return (shapes[0, :nseg[0]], int(nseg[0])) if single else (shapes, nseg)

    def stabilize_raw(self, ptr, mem, count, Hs, Ws, frame_stride, row_stride, y0, x0, Ho, Wo, search, anchor_ptr, anchor_mem, anchor_bytes,
                      gray_mode, shifts, table, out_ptr, out_mem):
        """swk_stabilize_u8 on raw pointers; shifts / table: the host arrays it fills (table may be None)."""
        self._check(self._lib.swk_stabilize_u8(self._h, ptr, int(mem), int(count), int(Hs), int(Ws), int(frame_stride), int(row_stride),
                                               int(y0), int(x0), int(Ho), int(Wo), int(search), anchor_ptr, int(anchor_mem),
                                               int(anchor_bytes), int(gray_mode), _ptr(shifts), _ptr(table), out_ptr, int(out_mem)))

    def stabilize(self, frames, rect, search, anchor, gray_mode=GRAY_Q14, device_out=False, table=False):
        """swk_stabilize_u8: for every BGR frame the integer shift (|dy|, |dx| <= search, rectangles that leave the frame excluded) at
        which the grey of its rectangle differs least, in summed absolute difference, from the anchor, and the frame's pixels there.
        frames: uint8 (count, Hs, Ws, 3) -- a numpy array of any frame and row strides (copied up), or a torch tensor on this
        context's GPU (read in place) --, contiguous along a pixel row.  rect = (y0, x0, Ho, Wo): the nominal rectangle.  anchor:
        uint8 (Ho, Wo), numpy or a tensor on the GPU.  Returns (shifts: SHIFT_DTYPE records (count,), the table (count, 2 search + 1,
        2 search + 1) uint64 indexed [f, dy + search, dx + search] with UINT64_MAX at excluded candidates, or None without
        table=True, pixels (count, Ho, Wo, 3): a numpy array, or with device_out=True a torch uint8 tensor on the GPU)."""
        a = self._stabilize_args(frames, rect, search, anchor, device_out)
        shifts = np.zeros(max(a["count"], 1), SHIFT_DTYPE)
        tab = np.zeros((max(a["count"], 1), a["side"], a["side"]), np.uint64) if table else None
        self.stabilize_raw(*a["source"], *a["rect"], a["search"], *a["anchor"], gray_mode, shifts, tab, *a["out_ptr"])
        return shifts, tab, a["out"]

    def stabilize_subpel_raw(self, ptr, mem, count, Hs, Ws, frame_stride, row_stride, y0, x0, Ho, Wo, search, anchor_ptr, anchor_mem,
                             anchor_bytes, gray_mode, shifts, table, sub_table, out_ptr, out_mem):
        """swk_stabilize_subpel_u8 on raw pointers; shifts (SUBSHIFT_DTYPE) / table / sub_table: the host arrays it fills (the tables
        may be None)."""
        self._check(self._lib.swk_stabilize_subpel_u8(self._h, ptr, int(mem), int(count), int(Hs), int(Ws), int(frame_stride),
                                                      int(row_stride), int(y0), int(x0), int(Ho), int(Wo), int(search), anchor_ptr,
                                                      int(anchor_mem), int(anchor_bytes), int(gray_mode), _ptr(shifts), _ptr(table),
                                                      _ptr(sub_table), out_ptr, int(out_mem)))

    def stabilize_subpel(self, frames, rect, search, anchor, gray_mode=GRAY_Q14, device_out=False, table=False):
        """swk_stabilize_subpel_u8: stabilize()'s integer search, then the 25 quarter-pixel shifts around its winner, each scored on
        the grey resampled with the 4-tap Catmull-Rom filter (include/swk.h), and the frame's B, G and R resampled at the chosen one.
        Arguments as stabilize().  Returns (shifts: SUBSHIFT_DTYPE records (count,) -- dy, dx of the integer stage, qy_total and
        qx_total in quarter pixels --, None or with table=True the pair (stage 1's table as stabilize()'s, the quarter-pixel table
        (count, 5, 5) uint64 indexed [f, qy + 2, qx + 2], UINT64_MAX at excluded candidates), pixels as stabilize()'s)."""
        a = self._stabilize_args(frames, rect, search, anchor, device_out)
        shifts = np.zeros(max(a["count"], 1), SUBSHIFT_DTYPE)
        tab = np.zeros((max(a["count"], 1), a["side"], a["side"]), np.uint64) if table else None
        sub = np.zeros((max(a["count"], 1), 5, 5), np.uint64) if table else None
        self.stabilize_subpel_raw(*a["source"], *a["rect"], a["search"], *a["anchor"], gray_mode, shifts, tab, sub, *a["out_ptr"])
        return shifts, ((tab, sub) if table else None), a["out"]

    def _stabilize_args(self, frames, rect, search, anchor, device_out):
        """What stabilize and stabilize_subpel pass on: source = (ptr, mem, count, Hs, Ws, frame stride, row stride), rect, search,
        anchor = (ptr, mem, bytes), out and out_ptr = (ptr, mem), side of the integer table; keep: what must outlive the call."""
        def on_gpu(a):
            return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)
        keep = [frames, anchor]
        if on_gpu(frames):
            if str(frames.dtype) != "torch.uint8" or frames.dim() != 4 or frames.shape[3] != 3 or frames.stride(3) != 1 or frames.stride(2) != 3:
                raise ValueError("device frames are uint8 (count, Hs, Ws, 3), contiguous along a row")
            count, Hs, Ws = (int(x) for x in frames.shape[:3])
            fptr, fmem, fs, rs = frames.data_ptr(), MEM_DEVICE, int(frames.stride(0)), int(frames.stride(1))
        else:
            a = np.asarray(frames)
            if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
                raise ValueError("frames are uint8 (count, Hs, Ws, 3)")
            if a.strides[3] != 1 or a.strides[2] != 3 or a.strides[1] < 3 * a.shape[2]:
                a = np.ascontiguousarray(a)
            keep.append(a)
            count, Hs, Ws = a.shape[:3]
            fptr, fmem, fs, rs = a.ctypes.data, MEM_HOST, a.strides[0], a.strides[1]
        if on_gpu(anchor):
            if str(anchor.dtype) != "torch.uint8" or not anchor.is_contiguous():
                raise ValueError("a device anchor is a contiguous uint8 tensor")
            aptr, amem, abytes = anchor.data_ptr(), MEM_DEVICE, int(anchor.numel())
        else:
            an = np.ascontiguousarray(anchor, np.uint8)
            keep.append(an)
            aptr, amem, abytes = an.ctypes.data, MEM_HOST, an.size
        y0, x0, Ho, Wo = (int(v) for v in rect)
        search = int(search)
        shape = (count, Ho, Wo, 3) if Ho > 0 and Wo > 0 and count > 0 else (1, 1, 1, 3)          # (the library refuses those)
        if device_out:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % self.device)
            optr, omem = out.data_ptr(), MEM_DEVICE
        else:
            out = np.empty(shape, np.uint8)
            optr, omem = out.ctypes.data, MEM_HOST
        return dict(source=(fptr, fmem, count, Hs, Ws, fs, rs), rect=(y0, x0, Ho, Wo), search=search, anchor=(aptr, amem, abytes),
                    out=out, out_ptr=(optr, omem), count=count, side=2 * search + 1 if 0 <= search <= 16 else 1, keep=keep)


def _gather_fields(frames, rect):
    """((Y, U, V) stacks, ((sx, sy), bits, full_range), the rectangle inside them, parity0) for Context.yuv_deinterlace over io_y4m
    frames of one format.  The stacks hold the chroma cells of the rectangle grown by one chroma row and three chroma columns on every
    side, clipped to the picture, and those cells' luma samples: every row and column of the definition's footprint that the picture
    has, so the stacks' borders act as borders only where they are the picture's."""
    first = frames[0]
    H, W = first.shape[:2]
    sx, sy = getattr(first, "sx", 1), getattr(first, "sy", 1)
    bits, full = getattr(first, "bits", 8), getattr(first, "full_range", False)
    mono = first.u is None
    oy, ox = getattr(first, "origin", (0, 0))
    fmt = lambda f: (f.shape, getattr(f, "sx", 1), getattr(f, "sy", 1), getattr(f, "bits", 8), getattr(f, "full_range", False),          # noqa: E731
                     f.u is None, getattr(f, "origin", (0, 0)), f.y.shape)
    if any(fmt(f) != fmt(first) for f in frames):
        raise ValueError("the frames of one deinterlacing call have one format and hold one rectangle")
    x0, y0, Wr, Hr = (int(c) for c in (rect if rect is not None else (0, 0, W, H)))
    if x0 < 0 or y0 < 0 or Wr < 1 or Hr < 1 or x0 + Wr > W or y0 + Hr > H:
        raise ValueError("rectangle outside the frame")
    CH, CW = ((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1
    ca, cb = max((y0 >> sy) - 1, 0), min(((y0 + Hr - 1) >> sy) + 2, CH)
    cl, cr = max((x0 >> sx) - 3, 0), min(((x0 + Wr - 1) >> sx) + 4, CW)
    la, lb, ll, lr = ca << sy, min(cb << sy, H), cl << sx, min(cr << sx, W)
    hh, hw = first.y.shape
    if la < oy or ll < ox or lb > oy + hh or lr > ox + hw:
        raise ValueError("the frames do not hold the rectangle plus the deinterlacer's footprint (one row, three columns)")
    Y = np.stack([f.y[la - oy:lb - oy, ll - ox:lr - ox] for f in frames])
    U = V = None
    if not mono:
        coy, cox = oy >> sy, ox >> sx
        U = np.stack([f.u[ca - coy:cb - coy, cl - cox:cr - cox] for f in frames])
        V = np.stack([f.v[ca - coy:cb - coy, cl - cox:cr - cox] for f in frames])
    return (Y, U, V), ((sx, sy), bits, full), (x0 - ll, y0 - la, Wr, Hr), (la & 1, ca & 1)


def stage_frames(frames, y0, y1, x0, x1, dst, threads=4):
    """dst[i] = frames[i][y0:y1, x0:x1] for a list of equally shaped uint8 frames (H, W[, C]) whose rows are contiguous, by
    swk_stage_frames (threads of the library, GIL released); frames that do not qualify are copied by numpy."""
    f0 = frames[0]
    px = f0.strides[1] if f0.ndim >= 2 else 1
    ok = all(f.dtype == np.uint8 and f.shape == f0.shape and f.strides == f0.strides for f in frames) and \
        f0.ndim in (2, 3) and (f0.ndim == 2 or (f0.strides[2] == 1 and f0.strides[1] == f0.shape[2])) and \
        (f0.ndim == 3 or f0.strides[1] == 1) and f0.strides[0] >= f0.shape[1] * px and dst.flags.c_contiguous
    if not ok:
        for i, f in enumerate(frames):
            dst[i] = f[y0:y1, x0:x1]
        return
    ptrs = (ctypes.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    rc = load().swk_stage_frames(ptrs, len(frames), f0.strides[0], y0, y1 - y0, x0 * px, (x1 - x0) * px, dst.ctypes.data, threads)
    if rc:
        raise SwkError("swk_stage_frames failed (%d)" % rc)


def cut_boxes(arrays, frame_of, boxes):
    """swk_cut_boxes: boxes (count, 4) int32 rows [r0, r1) x columns [c0, c1) of arrays[frame_of[i]] (equally shaped, row-contiguous
    uint8 arrays), copied densely into ONE new buffer.  Returns (buffer, offsets int64 (count,))."""
    a0 = arrays[0]
    px = a0.strides[1]
    h = np.maximum(boxes[:, 1] - boxes[:, 0], 0).astype(np.int64)
    w = np.maximum(boxes[:, 3] - boxes[:, 2], 0).astype(np.int64)
    sizes = h * w * px
    offsets = np.zeros(len(boxes), np.int64)
    if len(boxes) > 1:
        np.cumsum(sizes[:-1], out=offsets[1:])
    out = np.empty(int(sizes.sum()) if len(boxes) else 0, np.uint8)
    if len(boxes):
        ptrs = (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        fo = np.ascontiguousarray(frame_of, np.int32)
        bx = np.ascontiguousarray(boxes, np.int32)
        rc = load().swk_cut_boxes(ptrs, len(arrays), a0.strides[0], px, len(boxes), fo.ctypes.data, bx.ctypes.data, offsets.ctypes.data,
                                  out.ctypes.data)
        if rc:
            raise SwkError("swk_cut_boxes failed (%d)" % rc)
    return out, offsets


class DevicePlanes:
    """The u8 stage images of one batch_run kept on the GPU: one device buffer [stage][frame][Hc][Wc] taken from the
    context's free list and handed back when the last reader is gone.  read(stage, frame) copies ONE image to the
    host (swk_device_read).  The reference stores six images per frame (data_structures.py:183-208) and its counting
    loop reads none of them."""

    def __init__(self, ctx, stages, F, Hc, Wc):
        self.ctx, self.stages, self.F, self.Hc, self.Wc = ctx, stages, F, Hc, Wc
        self.plane = F * Hc * Wc
        self.nbytes = (self.plane + 3) // 4 * 4 * len(stages)          # every stack starts on a dword
        self.ptr = ctx.take_planes(self.nbytes)

    def pointer(self, stage):
        return self.ptr + self.stages.index(stage) * ((self.plane + 3) // 4 * 4)

    def read(self, stage, frame):
        return self.ctx.device_read(self.pointer(stage) + frame * self.Hc * self.Wc, (self.Hc, self.Wc))

    def read_stack(self, stage):
        return self.ctx.device_read(self.pointer(stage), (self.F, self.Hc, self.Wc))

    def __del__(self):
        try:
            if self.ptr:
                self.ctx.give_planes(self.ptr, self.nbytes)
                self.ptr = 0
        except Exception:
            pass


def track_costs(prev_c, prev_hist0, prev_has_hist, curr_c):
    """swk_track_costs: (n_prev + n_curr)^2 float64 cost matrix (host-side, no GPU needed)."""
    n_prev, n_curr = len(prev_c), len(curr_c)
    pc = np.ascontiguousarray(prev_c, np.float64).reshape(n_prev, 2)
    ph = np.ascontiguousarray(prev_hist0, np.float64).reshape(n_prev, 2)
    hh = np.ascontiguousarray(prev_has_hist, np.uint8).reshape(n_prev)
    cc = np.ascontiguousarray(curr_c, np.float64).reshape(n_curr, 2)
    packed = np.concatenate([pc.ravel(), ph.ravel(), cc.ravel()])
    return track_costs_packed(packed, hh.tobytes(), n_prev, n_curr)


def track_costs_packed(packed, has_hist, n_prev, n_curr):
    """The same from ONE float64 array [prev centroids (n_prev, 2) | first-of-history centroids (n_prev, 2) | current centroids
    (n_curr, 2)] and a bytes object of n_prev flags: the per-frame call of the tracker (two array objects per call instead of
    nine -- at a few dozen segments the marshalling, not the arithmetic, is the cost)."""
    n = n_prev + n_curr
    cost = np.empty((n, n), np.float64)
    base = packed.ctypes.data
    rc = _track_costs_fn()(base, base + 16 * n_prev, has_hist, base + 32 * n_prev, n_prev, n_curr, cost.ctypes.data)
    if rc:
        raise SwkError("swk_track_costs failed (%d)" % rc)
    return cost


_fast = {}


def _track_costs_fn():
    fn = _fast.get("costs")
    if fn is None:
        fn = _fast["costs"] = load().swk_track_costs
    return fn


def lsap(cost):
    """swk_lsap: column assigned to every row (same result as scipy.optimize.linear_sum_assignment)."""
    if cost.dtype != np.float64 or not cost.flags.c_contiguous:
        cost = np.ascontiguousarray(cost, np.float64)
    nr, nc = cost.shape
    out = np.empty(nr, np.int32)
    fn = _fast.get("lsap")
    if fn is None:
        fn = _fast["lsap"] = load().swk_lsap
    rc = fn(cost.ctypes.data, nr, nc, out.ctypes.data)
    if rc:
        raise SwkError("swk_lsap failed (%d)" % rc)
    return out


ERR_CAPACITY, ERR_TRACK_STATUS = -4, -7


class Tracker:
    """A swk_tracker handle (include/swk.h): SegmentTracker's state between frames, stepped a whole window per call.  Host code, no GPU,
    no Context.  Not thread-safe, like the handle."""

    def __init__(self, roi_mask, event_capacity=32, ordinal_capacity=1024):
        mask = np.asarray(roi_mask)
        if mask.ndim != 2:
            raise ValueError("the ROI mask is a 2-D array")
        mask = np.ascontiguousarray(np.where(mask == 255, 255, 0), np.uint8)          # all the tracker asks of it is `== 255`
        self._lib = load()
        handle = ctypes.c_void_p()
        rc = self._lib.swk_tracker_create(mask.ctypes.data, mask.shape[0], mask.shape[1], ctypes.byref(handle))
        if rc:
            raise SwkError("swk_tracker_create failed (%d)" % rc)
        self._handle = handle
        self._fn = self._lib.swk_track_window
        self.event_capacity, self.ordinal_capacity = int(event_capacity), int(ordinal_capacity)
        self._offsets = self._ordinals = None
        self._out32 = np.zeros(2, np.int32)           # n_events, frames_done
        self._out64 = np.zeros(3, np.int64)           # n_ordinals, first_ordinal, min_live

    def __del__(self):
        try:
            if self._handle:
                self._lib.swk_tracker_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    def track_window(self, nseg, centroids):
        """swk_track_window.  nseg: segments per frame; centroids: their (row, col) pairs, flat or (total, 2).  Returns (status_error,
        frames_done, first_ordinal, min_live, event offsets, event ordinals), the last two as lists (CSR).  status_error: frame
        `frames_done` holds a segment without a status (SWK_ERR_TRACK_STATUS); the frames before it are applied.  Event buffers that
        turn out too small are enlarged and the call is made again: the refused call changed nothing."""
        counts = np.ascontiguousarray(nseg, np.int32).reshape(-1)
        cents = np.ascontiguousarray(centroids, np.float64).reshape(-1)
        if counts.size and int(counts.min()) < 0:
            raise ValueError("a negative segment count")
        if cents.size != 2 * int(counts.sum()):
            raise ValueError("%d centroid values for %d segments" % (cents.size, int(counts.sum())))
        o32, o64 = self._out32, self._out64
        p32, p64 = o32.ctypes.data, o64.ctypes.data
        while True:
            if self._offsets is None or len(self._offsets) != self.event_capacity + 1:
                self._offsets = np.empty(self.event_capacity + 1, np.int64)
            if self._ordinals is None or len(self._ordinals) != max(self.ordinal_capacity, 1):
                self._ordinals = np.empty(max(self.ordinal_capacity, 1), np.int64)
            rc = self._fn(self._handle, counts.size, counts.ctypes.data, cents.ctypes.data, self.event_capacity, self.ordinal_capacity,
                          self._offsets.ctypes.data, self._ordinals.ctypes.data, p32, p64, p32 + 4, p64 + 8, p64 + 16)
            if rc != ERR_CAPACITY:
                break
            self.event_capacity = max(self.event_capacity, 2 * int(o32[0]))
            self.ordinal_capacity = max(self.ordinal_capacity, 2 * int(o64[0]))
        if rc not in (0, ERR_TRACK_STATUS):
            raise SwkError("swk_track_window failed (%d)" % rc)
        n_events, done = o32.tolist()
        n_ordinals, first, min_live = o64.tolist()
        return (rc == ERR_TRACK_STATUS, done, first, min_live, self._offsets[:n_events + 1].tolist(), self._ordinals[:n_ordinals].tolist())

    def export_state(self):
        """swk_tracker_export: (centroids (n, 2), ordinals (n,), chain offsets (n + 1,), chain ordinals) of the live segments."""
        n32, n64 = ctypes.c_int32(0), ctypes.c_int64(0)
        seg_cap, ord_cap = 0, 0
        while True:
            cents, ords = np.empty((seg_cap, 2), np.float64), np.empty(seg_cap, np.int64)
            offs, chain = np.zeros(seg_cap + 1, np.int64), np.empty(max(ord_cap, 1), np.int64)
            rc = self._lib.swk_tracker_export(self._handle, seg_cap, ord_cap, cents.ctypes.data, ords.ctypes.data, offs.ctypes.data,
                                              chain.ctypes.data, ctypes.byref(n32), ctypes.byref(n64))
            if rc != ERR_CAPACITY:
                break
            seg_cap, ord_cap = n32.value, n64.value
        if rc:
            raise SwkError("swk_tracker_export failed (%d)" % rc)
        return cents[:n32.value], ords[:n32.value], offs[:n32.value + 1], chain[:n64.value]

    def import_state(self, centroids, chain_lengths, chain_first):
        """swk_tracker_import: the live segments' centroids (n, 2), the lengths of their chains and the centroids of the chains' first
        members (n, 2; ignored where a chain is empty).  Returns the first ordinal of the numbering the header describes."""
        lens = np.ascontiguousarray(chain_lengths, np.int64).reshape(-1)
        cents = np.ascontiguousarray(centroids, np.float64).reshape(-1)
        first = np.ascontiguousarray(chain_first, np.float64).reshape(-1)
        if cents.size != 2 * lens.size or first.size != 2 * lens.size:
            raise ValueError("one centroid pair and one first-of-chain pair per segment")
        out = ctypes.c_int64(0)
        rc = self._lib.swk_tracker_import(self._handle, lens.size, cents.ctypes.data, lens.ctypes.data, first.ctypes.data, ctypes.byref(out))
        if rc:
            raise SwkError("swk_tracker_import failed (%d)" % rc)
        return out.value

    def force_assignment(self, col4row, skip_frames=0):
        """swk_debug_tracker_force_assignment (include/swk_debug.h): the tests' white-box hook."""
        a = np.ascontiguousarray(col4row, np.int32).reshape(-1)
        rc = self._lib.swk_debug_tracker_force_assignment(self._handle, int(skip_frames), a.ctypes.data, a.size)
        if rc:
            raise SwkError("swk_debug_tracker_force_assignment failed (%d)" % rc)


def pinned_empty(shape, dtype=np.uint8, device=0):
    """numpy array in page-locked host memory (swk_pinned_alloc on `device`): staging buffer for host -> device input,
    freed when the array (and every view of it) is gone.  Falls back to ordinary memory when pinning fails: pinning is
    an optimisation, never a requirement."""
    import weakref
    count = int(np.prod(shape))
    nbytes = max(count * np.dtype(dtype).itemsize, 1)
    lib = load()
    ptr = ctypes.c_void_p()
    if lib.swk_pinned_alloc(int(device), nbytes, ctypes.byref(ptr)) != 0 or not ptr.value:
        return np.empty(shape, dtype)
    buf = (ctypes.c_uint8 * nbytes).from_address(ptr.value)      # numpy keeps this object alive as .base
    weakref.finalize(buf, lib.swk_pinned_free, ctypes.c_void_p(ptr.value))
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


# ---- ROI mask of a video (host side, no GPU): image_filtering.py:99-180 ----
def _host_call(name, *args):
    rc = getattr(load(), name)(*args)
    if rc:
        raise SwkError("%s failed (%d)" % (name, rc))


def median_blur_u8(image, ksize):
    a = np.ascontiguousarray(image, np.uint8)
    ch = 1 if a.ndim == 2 else a.shape[2]
    out = np.empty_like(a)
    _host_call("swk_median_blur_u8", _ptr(a), a.shape[0], a.shape[1], ch, int(ksize), _ptr(out))
    return out


def otsu_threshold_u8(image):
    """(threshold, binary image): cv2.threshold(image, 0, 255, THRESH_BINARY + THRESH_OTSU)."""
    a = np.ascontiguousarray(image, np.uint8)
    out = np.empty_like(a)
    t = ctypes.c_int32(0)
    _host_call("swk_otsu_threshold_u8", _ptr(a), a.size, _ptr(out), ctypes.byref(t))
    return t.value, out


def canny_u8(image, low, high):
    a = np.ascontiguousarray(image, np.uint8)
    out = np.empty_like(a)
    _host_call("swk_canny_u8", _ptr(a), a.shape[0], a.shape[1], int(low), int(high), _ptr(out))
    return out


def dilate_up_u8(image, N):
    a = np.ascontiguousarray(image, np.uint8)
    out = np.empty_like(a)
    _host_call("swk_dilate_up_u8", _ptr(a), a.shape[0], a.shape[1], int(N), _ptr(out))
    return out


def roi_mask(frame, corners):
    """swk_roi_mask: (crop_region [(x0, y0), (x1, y1)], mask uint8 (Hc, Wc)) from the first BGR frame and the two
    chimney corners ((x1, y1), (x2, y2))."""
    if hasattr(frame, "as_full_frame"):          # a ROI-stream frame (io_roi_stream.RoiFrame): the stored rectangle pasted into a blank frame
        frame = frame.as_full_frame()
    if not isinstance(frame, np.ndarray):        # a frame that converts itself (io_y4m.Yuv420Frame): the BGR frame it stands for
        frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.strides[2] != 1 or frame.strides[1] != 3:
        frame = np.ascontiguousarray(frame, np.uint8)
    c = np.array([corners[0][0], corners[0][1], corners[1][0], corners[1][1]], np.int32)
    crop = np.zeros(4, np.int32)
    left, right = min(c[0], c[2]), max(c[0], c[2])
    width = int(right - left)
    hc, wc = int(0.5 * width) + int(0.125 * width), width + 2 * int(0.125 * width)
    mask = np.empty((max(hc, 1), max(wc, 1)), np.uint8)
    _host_call("swk_roi_mask", _ptr(frame), frame.shape[0], frame.shape[1], frame.strides[0], _ptr(c), _ptr(crop), _ptr(mask), mask.size)
    return [(int(crop[0]), int(crop[1])), (int(crop[2]), int(crop[3]))], mask


_default_ctx = {}
_ctx_lock = threading.Lock()


def default_context(device=0):
    """Process-wide context used by the image_filtering.* drop-in functions."""
    with _ctx_lock:
        ctx = _default_ctx.get(device)
        if ctx is None:
            ctx = _default_ctx[device] = Context(device)
    return ctx
