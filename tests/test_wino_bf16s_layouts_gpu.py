"""The shared-filter layouts of the split-bf16 Winograd expands against the present layout on the GPU: the same inputs, the same split
weights, a sentinel-filled destination -- the whole destination equal bit for bit (swk_set_cnn_tuning knob 2: 1 = present, 2 = shared)."""
import ctypes

import pytest
import torch

# n, cin, cout, t, dH, off, dC, c_off
CASES = [
    (1, 48, 192, 3, 1, 0, 192, 0),             # a single tile: one valid lane in one tile group
    (33, 48, 192, 4, 2, 0, 192, 0),            # 33 tiles: the second tile group's waves hold one valid tile
    (1, 32, 128, 5, 3, 0, 128, 0),             # 3 x 3 outputs: clipped 2 x 2 tiles
    (2, 48, 192, 14, 12, 0, 192, 0),           # 72 tiles: a partial last task
    (70, 64, 256, 7, 5, 0, 256, 0),            # 630 tiles end in a partial task
    (130, 32, 128, 5, 3, 0, 128, 0),           # 520 tiles = 4 tasks of 128 + 8 tiles
    (3, 32, 128, 16, 14, 0, 128, 0),           # 147 tiles: a partial 128-tile task
    (3, 32, 128, 16, 17, 1, 256, 128),         # off-centre placement in a 2 cout destination (tests/test_wino_bf16s.py)
    (2, 48, 192, 14, 15, 2, 384, 192),
    (2, 64, 256, 18, 19, 2, 512, 256),
    # more tasks than resident workgroups: the task loop, the re-setup at position 15, the filter-phase wrap
    (350, 48, 192, 16, 14, 0, 192, 0),         # 17,150 tiles
    (700, 32, 128, 16, 14, 0, 128, 0),         # 34,300 tiles
    (300, 64, 256, 18, 16, 0, 256, 0),         # 19,200 tiles
]

_weights = {}


def _operands(lib, dev, cin, cout):
    if (cin, cout) not in _weights:
        g = torch.Generator(device="cpu").manual_seed(cin + cout)
        w = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).contiguous()
        ws = torch.empty(3 * 16 * cin * cout, dtype=torch.int16)
        assert lib.swk_winograd_f2x2_3x3_weights_bf16s(w.data_ptr(), cout, cin, ws.data_ptr()) == 0
        _weights[(cin, cout)] = (ws.to(dev), (torch.randn((cout,), generator=g) * 0.3).to(dev))
    return _weights[(cin, cout)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout,t,dH,off,dC,c_off", CASES)
def test_shared_filter_layout_equals_the_present_one_bit_for_bit(n, cin, cout, t, dH, off, dC, c_off):
    from swiftwatcher_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws, bias = _operands(lib, dev, cin, cout)
    g = torch.Generator(device=dev).manual_seed(1000 * n + t)
    x = torch.randn((n, t, t, cin), generator=g, device=dev)          # channels-last, as the kernel reads it
    out = []
    try:
        for layout in (1, 2):
            assert lib.swk_set_cnn_tuning(2, layout) == 0
            d = torch.full((n, dH, dH, dC), -7.0, device=dev)
            assert lib.swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place(stream, x.data_ptr(), n, t, cin, ws.data_ptr(), bias.data_ptr(), cout,
                                                                       d.data_ptr(), dH, dH, dC, off, off, c_off) == 0
            torch.cuda.synchronize()
            out.append(d)
    finally:
        assert lib.swk_set_cnn_tuning(2, 0) == 0
    o = t - 2
    placed = out[0][:, off:off + o, off:off + o, c_off:c_off + cout]
    assert bool((placed >= 0).all()) and bool((placed > 0).any())          # ReLU outputs replaced the sentinel in the placed block ...
    assert int((out[0] == -7.0).sum()) == out[0].numel() - placed.numel()  # ... and nothing else
    assert torch.equal(out[0], out[1])
