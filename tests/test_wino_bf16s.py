"""The split-bf16 Winograd F(2x2, 3x3) expands (csrc/cnn_wino3x3_bf16s.hip): the host filter transform's split layout, the kernel's code
generation (no GPU needed), its float32-grade accuracy against float64 on the GPU, and the operand caches of a two-chain forward."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (cin, cout) -> k-steps per filter phase of the dispatched configuration; waves per workgroup = cout / 32
SHAPES = {(16, 64): 1, (32, 128): 2, (48, 192): 3, (64, 256): 2}


def _spp(cin, cout):
    return SHAPES.get((cin, cout), cin // 16)


def _lib():
    from swiftwatcher_amd import _lib
    return _lib.load()


def _split_weights(lib, w, cout, cin):
    ncol = 32 * (-(-cout // 32))
    out = np.full(3 * 16 * cin * ncol, 0xFFFF, np.uint16)
    rc = lib.swk_winograd_f2x2_3x3_weights_bf16s(w.ctypes.data_as(ctypes.c_void_p), cout, cin, out.ctypes.data_as(ctypes.c_void_p))
    return rc, out


def _f32_weights(lib, w, cout, cin):
    """U of swk_winograd_f2x2_3x3_weights as [xi][nu][ci][co] (its layout as tests/test_classifier.py reads it)."""
    CG = -(-cout // 32)
    out = np.full(16 * cin * 32 * CG, np.nan, np.float32)
    assert lib.swk_winograd_f2x2_3x3_weights(w.ctypes.data_as(ctypes.c_void_p), cout, cin, out.ctypes.data_as(ctypes.c_void_p)) == 0
    if (cin, cout) != (64, 256):
        out = out.reshape(16, 1, cin // 16, 2, 2, CG, 32, 4)
        return out.transpose(0, 2, 3, 4, 7, 5, 1, 6).reshape(4, 4, cin, 32 * CG)
    out = out.reshape(16, cin // 16, CG, 2, 2, 32, 4)
    return out.transpose(0, 1, 3, 4, 6, 2, 5).reshape(4, 4, cin, 32 * CG)


@pytest.mark.parametrize("cin,cout", [(16, 64), (32, 128), (48, 192), (64, 256), (32, 40), (16, 8)])
def test_split_filter_transform_is_exact_and_laid_out_as_a_operands(cin, cout):
    """u1 + u2 + u3 (three bf16 parts, reassembled in float64) equals the float32 U of swk_winograd_f2x2_3x3_weights bit for bit; the
    layout is [p][phase][column block][k-step of the phase][part][lane][8] with lane = 32 (k half) + output channel % 32; the parts are
    round-to-nearest-even, so each is at most half an ulp of the remainder before it; padding channels are zero."""
    lib = _lib()
    rng = np.random.default_rng(cin * 1000 + cout)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.exp(rng.uniform(-6, 6, (cout, cin, 1, 1)))).astype(np.float32)
    rc, out = _split_weights(lib, w, cout, cin)
    assert rc == 0
    CG, S, spp = -(-cout // 32), cin // 16, _spp(cin, cout)
    parts = out.reshape(16, S // spp, CG, spp, 3, 2, 32, 8)               # p, phase, cb, sub, part, k half, r, j
    parts = parts.transpose(4, 0, 1, 3, 5, 7, 2, 6).reshape(3, 4, 4, cin, 32 * CG)          # part, xi, nu, ci, co
    f = (parts.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    U = _f32_weights(lib, w, cout, cin)
    total = f[0] + f[1] + f[2]
    assert np.array_equal(total[..., :cout], U[..., :cout].astype(np.float64))
    assert not f[..., cout:].any()
    # round to nearest: |remainder after part k| <= half an ulp of part k in bf16 (8 significant bits)
    r1 = U[..., :cout].astype(np.float64) - f[0][..., :cout]
    assert np.all(np.abs(r1) <= np.abs(f[0][..., :cout]) * 2.0 ** -8 + 1e-300)


def test_split_filter_transform_refuses_bad_shapes():
    lib = _lib()
    w = np.ones((8, 24, 3, 3), np.float32)
    out = np.zeros(16, np.uint16)
    for cout, cin in ((8, 24), (8, 8), (0, 16), (8, 0)):
        assert lib.swk_winograd_f2x2_3x3_weights_bf16s(w.ctypes.data_as(ctypes.c_void_p), cout, cin, out.ctypes.data_as(ctypes.c_void_p)) != 0
    assert lib.swk_winograd_f2x2_3x3_weights_bf16s(None, 8, 16, out.ctypes.data_as(ctypes.c_void_p)) != 0


@pytest.fixture(scope="module")
def wino_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    from swiftwatcher_amd.csrc import build
    out = tmp_path_factory.mktemp("asm") / "cnn_wino3x3_bf16s.s"
    src = os.path.join(ROOT, "swiftwatcher_amd", "csrc", "cnn_wino3x3_bf16s.hip")
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]
    subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", str(out)])
    return open(out).read().splitlines()


@pytest.mark.parametrize("cin,cout", sorted(SHAPES))
def test_split_winograd_codegen(wino_asm, cin, cout):
    """Every instantiation the dispatcher uses: no scratch, two waves per SIMD (256 registers), bf16 MFMAs and no f32 ones, the filter
    stream by LDS-DMA."""
    nblk, spp = cout // 32, SHAPES[(cin, cout)]
    sym = "_ZN3swk26k_wino3x3_bf16s_relu_placeILi%dELi%dEEEv" % (nblk, spp)
    start = next(i for i, l in enumerate(wino_asm) if l.startswith(sym) and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(wino_asm)) if wino_asm[i].startswith(".Lfunc_end"))
    body, meta = wino_asm[start:end], "\n".join(wino_asm[end:end + 120])
    count = lambda pat: sum(1 for l in body if re.search(pat, l))
    assert count(r"scratch_") == 0
    assert int(re.search(r"ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"NumVgprs: (\d+)", meta).group(1)) + int(re.search(r"NumAgprs: (\d+)", meta).group(1)) <= 256
    assert int(re.search(r"Occupancy: (\d+)", meta).group(1)) >= 2
    assert count(r"v_mfma_f32_32x32x16_bf16") >= 6 * 2 * spp
    assert count(r"v_mfma_f32_32x32x2_?f32") == 0
    assert count(r"global_load_lds_dwordx4") >= 3 * spp


CASES = [  # n, cin, cout, t, dH, off, dC, c_off (those of test_winograd_conv3x3_kernel_against_torch)
    (3, 32, 128, 16, 17, 1, 256, 128), (9, 32, 128, 12, 10, 0, 256, 128), (2, 48, 192, 14, 12, 0, 384, 192),
    (3, 48, 192, 16, 14, 0, 384, 192), (2, 64, 256, 18, 19, 2, 512, 256), (5, 64, 256, 13, 11, 0, 512, 256),
    (1, 64, 256, 3, 1, 0, 256, 0), (1, 32, 128, 5, 3, 0, 128, 0), (70, 64, 256, 7, 5, 0, 256, 0), (33, 48, 192, 4, 2, 0, 192, 0),
    (7, 16, 64, 12, 10, 0, 128, 64), (5, 16, 64, 14, 12, 0, 128, 64), (130, 16, 64, 5, 3, 0, 64, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("spread", [False, True])
def test_split_winograd_kernel_is_float32_accurate(spread):
    """swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place against a float64 convolution: its error is at most 1.5 x the float32 Winograd
    kernel's on the same data, or 4e-7 of the output scale; activations spread over 1e4 in the second run.  The sentinel outside the
    placed block is untouched, and a segment's outputs do not depend on the batch it is in.  (The bound here is the float32 kernel's own
    error; both kernels against float64 and a CPU float32 F(2x2, 3x3), and bit-exact on integer inputs: tests/test_cnn_accuracy.py.)"""
    lib = _lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(17 + spread)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for n, cin, cout, t, dH, off, dC, c_off in CASES:
        x = torch.randn((n, cin, t, t), generator=g)
        if spread:
            x = x * torch.pow(10.0, torch.rand((n, cin, t, t), generator=g) * 4.0 - 2.0)
        wcpu = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).contiguous()
        bcpu = torch.randn((cout,), generator=g) * 0.3 * (10.0 if spread else 1.0)
        ref = torch.relu(torch.nn.functional.conv2d(x.double(), wcpu.double(), bcpu.double()))
        xd = x.to(dev).contiguous(memory_format=torch.channels_last)
        bias = bcpu.to(dev)
        ww = torch.empty(16 * cin * cout, dtype=torch.float32)
        assert lib.swk_winograd_f2x2_3x3_weights(wcpu.data_ptr(), cout, cin, ww.data_ptr()) == 0
        ws = torch.empty(3 * 16 * cin * cout, dtype=torch.int16)
        assert lib.swk_winograd_f2x2_3x3_weights_bf16s(wcpu.data_ptr(), cout, cin, ws.data_ptr()) == 0
        ww, ws = ww.to(dev), ws.to(dev)
        sentinel = torch.full((n, dC, dH, dH), -7.0, device=dev).contiguous(memory_format=torch.channels_last)
        d32, dsp = sentinel.clone(), sentinel.clone()
        torch.cuda.synchronize()
        args = (n, t, cin)
        tail = (bias.data_ptr(), cout)
        assert lib.swk_nhwc_conv3x3_winograd_bias_relu_place(stream, xd.data_ptr(), *args, ww.data_ptr(), *tail, d32.data_ptr(), dH, dH, dC,
                                                             off, off, c_off) == 0
        rc = lib.swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place(stream, xd.data_ptr(), *args, ws.data_ptr(), *tail, dsp.data_ptr(), dH, dH,
                                                                 dC, off, off, c_off)
        assert rc == 0, (rc, n, cin, cout, t)
        # one segment alone, placed in a one-segment destination
        k = n // 2
        one = sentinel[k:k + 1].clone()
        xk = xd[k:k + 1].contiguous(memory_format=torch.channels_last)
        assert lib.swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place(stream, xk.data_ptr(), 1, t, cin, ws.data_ptr(), *tail, one.data_ptr(),
                                                                   dH, dH, dC, off, off, c_off) == 0
        torch.cuda.synchronize()
        o = t - 2
        scale = max(float(ref.abs().max()), 1.0)
        blk = (slice(None), slice(c_off, c_off + cout), slice(off, off + o), slice(off, off + o))
        e32 = float((d32[blk].cpu().double() - ref).abs().max())
        esp = float((dsp[blk].cpu().double() - ref).abs().max())
        assert esp <= max(1.5 * e32, 4e-7 * scale), (esp, e32, scale, n, cin, cout, t)
        mask = torch.ones_like(dsp, dtype=torch.bool)
        mask[blk] = False
        assert bool((dsp[mask] == -7.0).all())
        assert torch.equal(one, dsp[k:k + 1])
    # shapes outside the Fire ratio are refused
    assert lib.swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place(stream, xd.data_ptr(), 1, 4, 16, ws.data_ptr(), bias.data_ptr(), 32,
                                                               dsp.data_ptr(), 2, 2, 32, 0, 0, 0) != 0


@pytest.mark.gpu
def test_first_two_chain_forward_behind_a_busy_stream_equals_one_chain():
    """A fresh classifier's first forward of 1,024 rows or more runs as two chains, the upper half on a side stream.  Its operand
    tensors (conv1's, the 3x3 expands' in both Winograd layouts, the head's) are made on the current stream before the chains fork,
    so with that stream held up by a long-running kernel the lower half still finds them complete: the scores equal a one-chain
    forward's bit for bit."""
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    from oracle import classifier_ref as ref
    g = torch.Generator(device="cpu").manual_seed(21)
    for split in (True, False):
        clf = SegmentClassifier.from_state_dict(ref.random_state_dict(15), batch_size=2048)
        clf.cropped.wino_split_bf16 = split
        assert clf._split_rows == 1024
        x = torch.randn((2048, 3, 40, 40), generator=g).to(clf.device).contiguous(memory_format=torch.channels_last)
        torch.cuda.synchronize()
        torch.cuda._sleep(200_000_000)                 # ~0.1 s of spinning on the current stream, ahead of everything below
        two = clf._forward(x).clone()
        torch.cuda.synchronize()
        assert clf._side_stream is not None
        clf._split_rows = 0
        one = clf._forward(x).clone()
        assert torch.equal(two, one), split
