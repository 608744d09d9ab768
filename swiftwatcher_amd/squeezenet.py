"""The classifier's network: SqueezeNet 1.0 in plain torch (SqueezeNet10, Fire) and its receptive-field cropped evaluation
(CroppedSqueezeNet10), whose convolutions run on the library's own HIP kernels (csrc/cnn_*.hip; MIOpen only with
SWK_OWN_CNN_KERNELS=0, the tests' cross-check).  segment_classification.py builds the reference's SegmentClassifier on top."""
import ctypes
import os
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # segment_classification.py:23
IMAGENET_STD = (0.229, 0.224, 0.225)
RESIZE = 24                                  # :20
PAD = (224 - 24) // 2                        # :21


class Fire(nn.Module):
    """torchvision.models.squeezenet.Fire: 1x1 squeeze, then 1x1 and 3x3 expands concatenated."""

    def __init__(self, inplanes, squeeze_planes, expand1x1_planes, expand3x3_planes):
        super().__init__()
        self.squeeze = nn.Conv2d(inplanes, squeeze_planes, kernel_size=1)
        self.squeeze_activation = nn.ReLU(inplace=True)
        self.expand1x1 = nn.Conv2d(squeeze_planes, expand1x1_planes, kernel_size=1)
        self.expand1x1_activation = nn.ReLU(inplace=True)
        self.expand3x3 = nn.Conv2d(squeeze_planes, expand3x3_planes, kernel_size=3, padding=1)
        self.expand3x3_activation = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.squeeze_activation(self.squeeze(x))
        return torch.cat([self.expand1x1_activation(self.expand1x1(x)),
                          self.expand3x3_activation(self.expand3x3(x))], 1)


class SqueezeNet10(nn.Module):
    """SqueezeNet 1.0 with the module names of torchvision's, so model.pt's state_dict
    (features.{0,3,4,5,7,8,9,10,12}.*, classifier.1.*) loads with strict=True."""

    def __init__(self, num_classes=2):
        super().__init__()
        self.num_classes = num_classes
        self.features = nn.Sequential(
            nn.Conv2d(3, 96, kernel_size=7, stride=2), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True),
            Fire(96, 16, 64, 64), Fire(128, 16, 64, 64), Fire(128, 32, 128, 128),
            nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True),
            Fire(256, 32, 128, 128), Fire(256, 48, 192, 192), Fire(384, 48, 192, 192), Fire(384, 64, 256, 256),
            nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True),
            Fire(512, 64, 256, 256))
        self.classifier = nn.Sequential(nn.Dropout(p=0.5), nn.Conv2d(512, num_classes, kernel_size=1),
                                        nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d((1, 1)))

    def forward(self, x):
        return torch.flatten(self.classifier(self.features(x)), 1)


def _nhwc(t):
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


class Launcher:
    """The library's swk_nhwc_* entry points for ONE forward: bound to PyTorch's current stream on `device` and to the forward's row
    count k.  Every method takes tensors (channels-last, float32) and reads shapes and pointers from them; a refusal of the library
    raises, naming the entry point.  The library is looked up when the launcher is made, through _lib.load(), never kept across
    forwards: tools/bench_convs.py substitutes _lib.load with a proxy that times these calls."""

    W3 = {"direct": "swk_nhwc_conv3x3_bias_relu_place", "f32": "swk_nhwc_conv3x3_winograd_bias_relu_place",
          "bf16s": "swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place"}

    def __init__(self, device, k):
        self.lib = _lib.load()
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        self.k = k

    def _call(self, name, *args):
        rc = getattr(self.lib, name)(self.stream, *args)
        if rc:
            raise RuntimeError("%s failed (%d)" % (name, rc))

    def conv1(self, x, first, count, w, bias, dest):
        """7x7 stride-2 convolution + bias + ReLU of the square tiles x: output rows/cols [first, first + count) -> dest."""
        self._call("swk_nhwc_conv7x7s2_bias_relu", x.data_ptr(), self.k, x.shape[2], first, count, w.data_ptr(), bias.data_ptr(),
                   w.shape[0], dest.data_ptr())

    def conv1x1(self, src, crop, size, w, bias, dest, off, c_off):
        """1x1 convolution + bias + ReLU of the size x size square of src at (crop, crop) -> dest at (off, off), channel c_off on.
        w: the convolution's (cout, cin, 1, 1) weight -- a 1 x 1 kernel is the same memory in both layouts."""
        self._call("swk_nhwc_conv1x1_bias_relu_place", src.data_ptr(), self.k, src.shape[2], src.shape[3], src.shape[1], crop, crop,
                   size, size, w.data_ptr(), bias.data_ptr(), w.shape[0], dest.data_ptr(), dest.shape[2], dest.shape[3], dest.shape[1],
                   off, off, c_off)

    def conv3x3(self, src, kind, w, bias, dest, off, c_off):
        """Valid 3x3 convolution + bias + ReLU of the square tiles src on the kernel `kind` (CroppedSqueezeNet10._w3_kind), w in that
        kernel's layout -> dest at (off, off), channel c_off on."""
        assert src.shape[2] == src.shape[3]
        self._call(self.W3[kind], src.data_ptr(), self.k, src.shape[2], src.shape[1], w.data_ptr(), bias.data_ptr(), bias.shape[0],
                   dest.data_ptr(), dest.shape[2], dest.shape[3], dest.shape[1], off, off, c_off)

    def maxpool(self, src, dst):
        self._call("swk_nhwc_maxpool3s2", src.data_ptr(), self.k, src.shape[2], src.shape[3], src.shape[1], dst.data_ptr())

    def pool_squeeze(self, src, w, bias, dest, off, ring=None, live_off=0, live_n=0):
        """Max-pool of src + the 1x1 squeeze behind it -> dest at (off, off).  ring: the tile whose ring every tile of src shares
        (written once, CroppedSqueezeNet10._buffers): only the live square (live_off, live_n) is then read per segment."""
        self._call("swk_nhwc_maxpool3s2_conv1x1_bias_relu_place", src.data_ptr(), self.k, src.shape[2], src.shape[1], w.data_ptr(),
                   bias.data_ptr(), w.shape[0], dest.data_ptr(), dest.shape[2], dest.shape[3], dest.shape[1], off, off,
                   None if ring is None else ring.data_ptr(), live_off, live_n)

    def bias_relu_place(self, e, crop, size, bias, dest, off, c_off):
        """Bias + ReLU of the size x size square of the convolution output e at (crop, crop) -> dest at (off, off), channel c_off on."""
        e = _nhwc(e)
        self._call("swk_nhwc_bias_relu_place", e.data_ptr(), self.k, e.shape[2], e.shape[3], e.shape[1], crop, crop, size, size,
                   bias.data_ptr(), dest.data_ptr(), dest.shape[2], dest.shape[3], dest.shape[1], off, off, c_off)

    def head(self, x, hw, hb, ring, n_pos):
        """The two-class head (1x1 convolution + ReLU + mean over n_pos positions, ring = the summed positions outside x) as one kernel
        with a fixed summation order (csrc/cnn_aux.hip): scores that do not depend on the batch's row count.  -> (k, 2)."""
        out = torch.empty((self.k, 2), dtype=torch.float32, device=x.device)
        self._call("swk_nhwc_head2_relu_mean", x.data_ptr(), self.k, x.shape[2] * x.shape[3], x.shape[1], hw.data_ptr(), hb.data_ptr(),
                   ring.data_ptr(), n_pos, out.data_ptr())
        return out

    def dropout_head(self, x, pos, bg, n_pos, hw, hb, keys, seed, samples):
        """swk_nhwc_head2_dropout_relu_mean: x (k, c, h, w) channels-last, the live positions `pos` of the last Fire's output; bg
        (n_pos, c) or None (every position live); keys (k,) int64 tensor holding the uint64 keys.  -> (k, samples, 2)."""
        if not (x.is_contiguous(memory_format=torch.channels_last) and hw.shape[0] == 2 and keys.shape[0] == self.k and keys.is_contiguous()):
            raise RuntimeError("the dropout head needs a channels-last tensor, a two-class head and one key per segment")
        out = torch.empty((self.k, samples, 2), dtype=torch.float32, device=x.device)
        self._call("swk_nhwc_head2_dropout_relu_mean", x.data_ptr(), self.k, x.shape[2] * x.shape[3], x.shape[1], pos.data_ptr(),
                   None if bg is None else bg.data_ptr(), n_pos, hw.data_ptr(), hb.data_ptr(), keys.data_ptr(),
                   ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), samples, out.data_ptr())
        return out


def _affected(lo, hi, k, st, pad, out_size):
    """Outputs of a (k, stride, pad) window layer that see any input index in [lo, hi]."""
    a = -((-(lo + pad - k + 1)) // st)          # ceil
    b = (hi + pad) // st
    return max(a, 0), min(b, out_size - 1)


class PlanEntry(NamedTuple):
    """One layer of features[3:] in CroppedSqueezeNet10.plan."""
    kind: str                                # "fire" or "pool"
    layer: nn.Module                         # the Fire / MaxPool2d of model.features
    tile: torch.Tensor                       # (1, c, t, t): the layer's input for the blank image around the live square, halo included
    off: int                                 # row and column of the live square in the tile
    n: int                                   # side of the live square (the layer's input values that depend on the segment)
    pad: Optional[Tuple[int, int]]           # fire: zero rows/cols (before, after) the tile lacks where it reaches the map's edge
    crop: Optional[Tuple[int, int]]          # fire: (first row/col in the tile, side) of the output square the next layer reads


class CroppedSqueezeNet10:
    """Receptive-field cropped evaluation of SqueezeNet10 for this classifier's inputs.

    Every input is a 24x24 patch in the middle of a 224x224 image whose other 89 % is ONE constant (Pad(100) then
    Normalize, segment_classification.py:21-23).  Outside the patch's receptive field every activation is therefore
    the same for every segment: it is computed once, from a blank image, when the model is loaded.  Per batch only
    the affected square of each feature map is evaluated -- on a tile cut from that background map (which supplies
    the halo a 3x3 window needs) with the live values pasted in its middle and the layer run without padding:

        input 40x40 (rows 92..131) -> conv1 17x17 (46..62 of 109) -> pool 8x8 (23..30 of 54)
        -> fire2..4: 10, 12, 14 -> pool 8x8 (9..16 of 27) -> fire5..8: 10, 12, 14, 16 -> pool 9x9 (2..10 of 13)
        -> fire9 11x11 -> 1x1 head + ReLU on 11x11, plus the head's constant ring, / 169.

    Same arithmetic per output as the full network (0.128 instead of 0.733 GMAC per segment); results differ from
    it only by float32 summation order inside the convolution kernels and in the final average.

    Three routes, one function each, chosen per call (the tests flip the switches on a live object): _forward_own, the library's own
    kernels (the default, and all the benchmark runs); _forward_miopen, MIOpen's convolutions (own_kernels = False, the tests'
    cross-check); _forward_torch, plain torch on the CPU."""

    IN_LO, IN_HI = 92, 131            # rows/cols of the 224-pixel input the tile covers (patch at 100..123)

    def __init__(self, model, border):
        """model: SqueezeNet10 in eval mode on its device; border: (3,) tensor, the normalised pad value."""
        self.model = model
        dev = next(model.parameters()).device
        feats = list(model.features)
        with torch.no_grad():
            x = border.to(dev, torch.float32).view(1, 3, 1, 1).expand(1, 3, 224, 224).contiguous()
            maps = []                  # maps[i] = input of features[i] for the blank image
            for layer in feats:
                maps.append(x)
                x = layer(x)
            head = torch.relu(model.classifier[1](x))                 # (1, 2, 13, 13)
        lo, hi = PAD, PAD + RESIZE - 1
        size = 224
        self.plan = []                 # one PlanEntry per features[i] from the first Fire on
        # conv1 + ReLU + pool are run on the input tile directly
        assert isinstance(feats[0], nn.Conv2d) and feats[0].padding == (0, 0)
        out_size = maps[1].shape[-1]
        lo, hi = _affected(lo, hi, 7, 2, 0, out_size)
        need = (2 * lo, 2 * hi + 6)
        assert need[0] >= self.IN_LO and need[1] <= self.IN_HI
        assert (2 * lo - self.IN_LO) % 2 == 0
        self.conv_skip = (2 * lo - self.IN_LO) // 2          # conv outputs the tile yields before the first affected one
        conv_lo = lo - self.conv_skip
        conv_hi = conv_lo + (self.IN_HI - self.IN_LO + 1 - 7) // 2
        size = out_size
        # the first pool works on conv rows [conv_lo, conv_hi] (all computed from the tile, background included)
        out_size = maps[3].shape[-1]
        plo, phi = _affected(lo, hi, 3, 2, 0, out_size)
        assert 2 * plo >= conv_lo and 2 * phi + 2 <= conv_hi
        self.pool1_slice = (2 * plo - conv_lo, 2 * phi + 2 - conv_lo + 1)
        lo, hi, size = plo, phi, out_size
        for i in range(3, len(feats)):
            layer = feats[i]
            in_map = maps[i]
            if isinstance(layer, Fire):
                a, b = max(lo - 1, 0), min(hi + 1, size - 1)
                n0, n1 = a - 1, b + 1                       # inputs the 3x3 expand needs; may leave the map by one
                c0, c1 = max(n0, 0), min(n1, size - 1)
                tile = in_map[:, :, c0:c1 + 1, c0:c1 + 1].contiguous()
                self.plan.append(PlanEntry("fire", layer, tile, lo - c0, hi - lo + 1, (c0 - n0, n1 - c1), (a - c0, b - a + 1)))
                lo, hi = a, b
            else:                                            # MaxPool2d(3, 2, ceil_mode=True)
                out_size = maps[i + 1].shape[-1] if i + 1 < len(feats) else x.shape[-1]
                a, b = _affected(lo, hi, 3, 2, 0, out_size)
                n0, n1 = 2 * a, 2 * b + 2
                assert n0 >= 0 and n1 <= size - 1            # no clipped window among the affected ones
                tile = in_map[:, :, n0:n1 + 1, n0:n1 + 1].contiguous()
                self.plan.append(PlanEntry("pool", layer, tile, lo - n0, hi - lo + 1, None, None))
                lo, hi, size = a, b, out_size
        self.final = (lo, hi, size)
        self.final_bg = x[:, :, lo:hi + 1, lo:hi + 1].contiguous()          # the last Fire's output for the blank image, live square
        ring = head.clone()
        ring[:, :, lo:hi + 1, lo:hi + 1] = 0
        self.ring_sum = ring.sum(dim=(2, 3))                 # (1, 2): the head's input-independent positions
        self.n_pos = float(size * size)
        # what the dropout head reads (swk_nhwc_head2_dropout_relu_mean): the last Fire's output for the blank image at every position,
        # channels-last (its ring is dropped per segment and sample like the live square, so ring_sum cannot stand in for it), and the
        # position of each live pixel in the full map, raster order
        self.head_bg = x.permute(0, 2, 3, 1).reshape(size * size, x.shape[1]).contiguous()
        self.head_pos = torch.tensor([r * size + c for r in range(lo, hi + 1) for c in range(lo, hi + 1)], dtype=torch.int32, device=dev)
        # input-independent squeeze output of every Fire tile (with the map's own zero padding where a tile reaches
        # the edge): the ring of the persistent squeeze buffers
        self.sq_bg = []
        with torch.no_grad():
            for p in self.plan:
                if p.kind != "fire":
                    self.sq_bg.append(None)
                    continue
                sq = p.layer.squeeze_activation(p.layer.squeeze(p.tile))
                if p.pad[0] or p.pad[1]:
                    sq = F.pad(sq, (p.pad[0], p.pad[1], p.pad[0], p.pad[1]))
                self.sq_bg.append(sq.contiguous())
        # what the own kernels (_forward_own) are written for (csrc/cnn_conv1.hip, csrc/cnn_aux.hip): constants of SqueezeNet10(2),
        # checked here once instead of on every forward
        conv1, head = feats[0], model.classifier[1]
        side = self.IN_HI - self.IN_LO + 1
        if conv1.out_channels != 96 or side % 2 or 2 * (self.pool1_slice[1] - 1) + 8 > side:
            raise ValueError("the own-kernel route of the cropped forward needs a 96-channel conv1 and an even input tile that holds the first pool's rows")
        if head.out_channels != 2 or head.in_channels not in (256, 512, 768, 1024):
            raise ValueError("the own-kernel route of the cropped forward needs a two-class head with 256, 512, 768 or 1024 input channels")
        # the persistent per-layer buffers (_buffers): _buf = (bufs, live), _aux = the own routes' conv1 / pool outputs; `version` counts
        # their reallocations (new addresses: captured graphs of the old ones are void)
        self._cap = 0
        self._buf = self._aux = None
        self.version = 0
        # channels-last on the GPU: what the library's convolution kernels read and write
        self.memory_format = torch.channels_last if dev.type == "cuda" else torch.contiguous_format
        if self.memory_format == torch.channels_last:
            model.to(memory_format=torch.channels_last)
        # a Fire tile that reaches the map's edge needs zero padding the kernels do not do: such a plan runs on _forward_torch
        self._interior = all(p.kind != "fire" or not (p.pad[0] or p.pad[1]) for p in self.plan)
        # The two cross-checks the tests keep: own_kernels = False routes every convolution through MIOpen (+ the placement kernel),
        # winograd = False runs the 3x3 expands on the direct kernel (csrc/cnn_conv3x3.hip) instead of F(2x2, 3x3).
        self.own_kernels = os.environ.get("SWK_OWN_CNN_KERNELS", "1") == "1"
        self.winograd = True
        # the Winograd expands with float32 products as six bf16 matrix-core products of split operands (csrc/cnn_wino3x3_bf16s.hip);
        # False (or SWK_WINO_SPLIT_BF16=0) keeps them on the f32 matrix cores (csrc/cnn_wino3x3.hip)
        self.wino_split_bf16 = os.environ.get("SWK_WINO_SPLIT_BF16", "1") == "1"
        # max-pool + the squeeze behind it as one kernel (csrc/cnn_poolsq.hip): the pooled tensor never goes to memory
        self.fuse_pool = os.environ.get("SWK_FUSE_POOL", "1") == "1"
        # the operand tensors the own kernels read, made once: "conv1", "head", and (j, kind) for the 3x3 expand of plan entry j
        self._operands = {}

    def macs_per_segment(self):
        """Multiply-accumulates of one forward per segment: (executed, useful).  "useful" prices every convolution output the next
        layer reads as a direct convolution (the figure to compare networks and hardware with); "executed" is what the kernels
        really multiply: the Winograd F(2x2, 3x3) kernel does 16 instead of 36 per 2 x 2 outputs (tiles padded to even sizes), the
        MIOpen path (fused kernels off) runs the 1x1 expands over the whole squeeze tile.  The full 224 x 224 network does 0.7326 G."""
        m = self.model
        c1 = m.features[0]
        side = (self.IN_HI - self.IN_LO + 1 - 7) // 2 + 1
        executed = useful = side * side * c1.out_channels * c1.in_channels * 49
        last_n = None
        on_gpu = self.ring_sum.is_cuda and self.memory_format == torch.channels_last and self.own_kernels
        for p in self.plan:
            if p.kind != "fire":
                continue
            t = p.tile.shape[2] + p.pad[0] + p.pad[1]
            sq, e1, e3 = p.layer.squeeze, p.layer.expand1x1, p.layer.expand3x3
            executed += p.n * p.n * sq.out_channels * sq.in_channels
            e1_side = p.n if on_gpu else t      # the fused kernel only computes the outputs that depend on the segment
            executed += e1_side * e1_side * e1.out_channels * e1.in_channels
            if on_gpu and self._w3_kind(e3, 1, t) != "direct":
                tiles = ((t - 2 + 1) // 2) ** 2
                executed += tiles * 16 * e3.out_channels * e3.in_channels
            else:
                executed += (t - 2) ** 2 * e3.out_channels * e3.in_channels * 9
            useful += p.n * p.n * sq.out_channels * sq.in_channels
            useful += p.crop[1] ** 2 * (e1.out_channels * e1.in_channels + e3.out_channels * e3.in_channels * 9)
            last_n = p.crop[1]
        head = m.classifier[1]
        executed += last_n * last_n * head.out_channels * head.in_channels
        useful += last_n * last_n * head.out_channels * head.in_channels
        return int(executed), int(useful)

    def _buffers(self, batch):
        """Persistent per-layer tiles for up to `batch` segments: self._buf = (bufs, live), whose rings hold the background values and
        are written once (a forward pass only overwrites the live centres), and self._aux (channels-last, so GPU only): the conv1
        and pool outputs of the two GPU routes, plain scratch."""
        if batch <= self._cap:
            return
        dev = self.ring_sum.device

        def filled(bg):
            return bg.expand(batch, -1, -1, -1).contiguous(memory_format=self.memory_format)

        def scratch(c, h):
            return torch.empty((batch, c, h, h), dtype=torch.float32, device=dev).contiguous(memory_format=torch.channels_last)

        bufs = [filled(sq if p.kind == "fire" else p.tile) for p, sq in zip(self.plan, self.sq_bg)]
        # live (ring-free) inputs of the Fires that follow a Fire, and of the head
        live = []
        for j, p in enumerate(self.plan):
            nxt = self.plan[j + 1] if j + 1 < len(self.plan) else None
            if p.kind == "fire" and (nxt is None or nxt.kind == "fire"):
                # initialised with the blank image's values: the expand1x1 outputs on the ring of the square (squeeze values that do
                # not depend on the segment) are never recomputed, a forward writes the expand1x1 centre and all of expand3x3
                bg = self.final_bg if nxt is None else nxt.tile[:, :, nxt.off:nxt.off + nxt.n, nxt.off:nxt.off + nxt.n]
                assert bg.shape[2] == p.crop[1] and bg.shape[1] == p.layer.expand1x1.out_channels + p.layer.expand3x3.out_channels
                live.append(filled(bg))
            else:
                live.append(None)
        aux = None
        if self.memory_format == torch.channels_last:
            a, b = self.pool1_slice
            conv1_c = self.model.features[0].out_channels
            aux = {"conv1": scratch(conv1_c, b - a), "pool_in": scratch(conv1_c, (b - a - 3) // 2 + 1),
                   "pool_out": [scratch(p.tile.shape[1], (p.tile.shape[2] - 3) // 2 + 1) for p in self.plan if p.kind == "pool"]}
        self._buf, self._aux, self._cap = (bufs, live), aux, batch
        self.version += 1

    def _fire_dest(self, j, bufs, live, rows):
        """Where the outputs of the Fire at plan entry j go: (tensor, row and column of the output square in it) -- live[j] at 0, or,
        in front of a pool, straight into the centre of the pool's tile."""
        if live[j] is not None:
            return live[j][rows], 0
        assert self.plan[j + 1].n == self.plan[j].crop[1]
        return bufs[j + 1][rows], self.plan[j + 1].off

    def _gpu_path(self, tiles):
        return tiles.is_cuda and self.memory_format == torch.channels_last and self._interior

    def reserve(self, batch):
        """Persistent tiles for `batch` segments and every per-layer operand tensor, made now (on the current stream)."""
        self._buffers(batch)
        self._prepare_operands()

    def _prepare_operands(self):
        """The operand tensors the own kernels read (conv1's weights, the 3x3 expands' in the layout of the kernel each one runs on, the
        head's), made on the current stream.  Made lazily by the first forward that needs one, they would be enqueued on whichever stream
        that forward runs on: in a two-chain forward (SegmentClassifier._forward_two_streams) the side stream, whose copy the other chain
        then may read before it has landed -- so reserve() makes them all before the chains fork."""
        if not (self.own_kernels and self.ring_sum.is_cuda and self.memory_format == torch.channels_last):
            return
        self._conv1_operand()
        for j, p in enumerate(self.plan):
            if p.kind == "fire":
                # (a forward of so many rows that the capacity rule of _w3_kind sends it to the direct kernel makes that operand itself)
                self._w3_operand(j, p.layer.expand3x3, self._w3_kind(p.layer.expand3x3, 1, self.sq_bg[j].shape[2]))
        self._head_operand()

    def _conv1_operand(self):
        if "conv1" not in self._operands:
            self._operands["conv1"] = self.model.features[0].weight.detach().contiguous(memory_format=torch.contiguous_format).clone()
        return self._operands["conv1"]

    def _head_operand(self):
        if "head" not in self._operands:
            head = self.model.classifier[1]
            self._operands["head"] = (head.weight.detach().reshape(head.out_channels, -1).contiguous(), head.bias.detach().contiguous(),
                                      self.ring_sum.reshape(-1).contiguous())
        return self._operands["head"]

    def _w3_kind(self, conv, k, side):
        """The kernel a 3x3 expand of k tiles of side x side runs on: "bf16s" / "f32" (Winograd F(2x2, 3x3), split-bf16 or f32
        products) or "direct".  The Winograd kernels index their source with 32 bits: one of 2^32 bytes or more runs on the direct one."""
        cin, cout = conv.in_channels, conv.out_channels
        if self.winograd and cout == 4 * cin and cin in (16, 32, 48, 64) and k * side * side * cin * 4 < (1 << 32):
            # (16 -> 64 measured slower on the split kernel, 77 / 101 against 73 / 93 us per 4,096 rows: it stays on the f32 one)
            return "bf16s" if self.wino_split_bf16 and cin != 16 else "f32"
        return "direct"

    def _w3_operand(self, j, conv, kind):
        """The weights of the 3x3 expand of plan entry j in the layout of the kernel `kind` runs on, made once per layer and kind."""
        w = self._operands.get((j, kind))
        if w is not None:
            return w
        cin, cout = conv.in_channels, conv.out_channels
        if kind == "direct":          # [co][ci][3][3] -> [tap][ci][co]
            w = conv.weight.detach().permute(2, 3, 1, 0).contiguous(memory_format=torch.contiguous_format)
        else:                         # G g G^T in the kernel's operand layout (host code of the library)
            wc = conv.weight.detach().to("cpu", torch.float32).contiguous()
            ncol = 32 * (-(-cout // 32))
            if kind == "bf16s":
                fn, out = "swk_winograd_f2x2_3x3_weights_bf16s", torch.empty(3 * 16 * cin * ncol, dtype=torch.int16)          # bf16 bit patterns
            else:
                fn, out = "swk_winograd_f2x2_3x3_weights", torch.empty(16 * cin * ncol, dtype=torch.float32)
            if getattr(_lib.load(), fn)(wc.data_ptr(), cout, cin, out.data_ptr()):
                raise RuntimeError("%s failed" % fn)
            w = out.to(conv.weight.device)
        self._operands[(j, kind)] = w
        return w

    @torch.no_grad()
    def __call__(self, tiles, row0=0, dropout=None):
        """tiles: (B, 3, 40, 40) float32 = rows/cols 92..131 of the normalised 224x224 input.  row0: first row of the persistent
        per-layer tiles this forward works in (two forwards on disjoint row ranges may run side by side on two streams).
        dropout = (keys, seed, samples): instead of the eval-mode scores, (B, samples, 2) scores under the reference's live Dropout(0.5)
        (keys: (B,) int64 device tensor of the segments' uint64 keys); the library's HIP kernel only."""
        if not self._gpu_path(tiles):
            return self._forward_torch(tiles, row0, dropout)
        with torch.cuda.device(tiles.device):            # the kernels go to this device's current stream
            if self.own_kernels:
                return self._forward_own(tiles, row0, dropout)
            return self._forward_miopen(tiles, row0, dropout)

    def _forward_torch(self, tiles, row0, dropout):
        """Plain torch, layer by layer: the CPU, or a plan with edge padding."""
        if dropout is not None:
            raise RuntimeError("dropout sampling runs on the library's HIP head kernel: it needs the GPU path")
        if row0:
            raise ValueError("row0 is a feature of the GPU path")
        m = self.model
        k = tiles.shape[0]
        self._buffers(k)
        bufs, live = self._buf
        rows = slice(0, k)
        x = torch.relu(m.features[0](tiles.contiguous(memory_format=self.memory_format)))
        a, b = self.pool1_slice
        x = m.features[2](x[:, :, a:b, a:b])
        for j, p in enumerate(self.plan):
            if p.kind == "pool":
                x = p.layer(bufs[j][rows])                   # centre written by the Fire before it
                continue
            fire, sq = p.layer, bufs[j][rows]
            o = p.off + p.pad[0]
            torch.clamp_min(fire.squeeze(x), 0, out=sq[:, :, o:o + p.n, o:o + p.n])
            e3 = F.conv2d(sq, fire.expand3x3.weight, fire.expand3x3.bias)            # valid: the halo is in the tile
            e1 = F.conv2d(sq, fire.expand1x1.weight, fire.expand1x1.bias)
            c, cn = p.crop
            c1 = fire.expand1x1.out_channels
            dest, doff = self._fire_dest(j, bufs, live, rows)
            dest = dest[:, :, doff:doff + cn, doff:doff + cn]
            cp = c + p.pad[0]
            torch.clamp_min(e1[:, :, cp:cp + cn, cp:cp + cn], 0, out=dest[:, :c1])
            torch.clamp_min(e3, 0, out=dest[:, c1:])
            x = dest
        s = torch.relu(m.classifier[1](x)).sum(dim=(2, 3))
        return (s + self.ring_sum) / self.n_pos

    def _forward_own(self, tiles, row0, dropout):
        """The library's own kernels on PyTorch's current stream, every one convolution + bias + ReLU + placement into the next
        layer's tile: conv1 (csrc/cnn_conv1.hip), the 1x1 squeezes and expands on the f32 matrix cores (csrc/cnn_conv1x1.hip), the 3x3
        expands on the kernel _w3_kind names, the max-pools inside the squeezes behind them (fuse_pool) or on their own, the head."""
        k = tiles.shape[0]
        self._buffers(row0 + k)
        (bufs, live), aux = self._buf, self._aux
        rows = slice(row0, row0 + k)
        run = Launcher(tiles.device, k)
        a, b = self.pool1_slice
        c1buf = aux["conv1"][rows]
        # conv1 on the rows the first pool reads
        run.conv1(_nhwc(tiles), a, b - a, self._conv1_operand(), self.model.features[0].bias, c1buf)
        x = aux["pool_in"][rows]
        # to_pool: (a tensor whose max-pool the next squeeze reads, fused into it; the tile whose ring it shares; its live square)
        to_pool = (c1buf, None, 0, 0) if self.fuse_pool else None          # conv1's output has no ring; the pool tiles behind fire4 and fire8 do
        if to_pool is None:
            run.maxpool(c1buf, x)
        pool_out = iter(aux["pool_out"])
        for j, p in enumerate(self.plan):
            if p.kind == "pool":
                x = next(pool_out)[rows]
                if self.fuse_pool:
                    to_pool = (bufs[j][rows], bufs[j][0:1], p.off, p.n)
                else:
                    run.maxpool(bufs[j][rows], x)
                continue
            fire, sq = p.layer, bufs[j][rows]
            dest, doff = self._fire_dest(j, bufs, live, rows)
            if to_pool is not None:
                assert (to_pool[0].shape[2] - 3) // 2 + 1 == p.n
                run.pool_squeeze(to_pool[0], fire.squeeze.weight, fire.squeeze.bias, sq, p.off, *to_pool[1:])
                to_pool = None
            else:
                run.conv1x1(x, 0, p.n, fire.squeeze.weight, fire.squeeze.bias, sq, p.off, 0)
            # expand1x1 only where the squeeze output depends on the segment (n x n inside the crop[1] x crop[1] square: the ring keeps
            # the blank image's values the buffers were created with)
            run.conv1x1(sq, p.off, p.n, fire.expand1x1.weight, fire.expand1x1.bias, dest, doff + p.off - p.crop[0], 0)
            # the 3x3 expand: a valid convolution over the squeeze tile
            e3 = fire.expand3x3
            kind = self._w3_kind(e3, k, sq.shape[2])
            run.conv3x3(sq, kind, self._w3_operand(j, e3, kind), e3.bias, dest, doff, fire.expand1x1.out_channels)
            x = dest
        hw, hb, ring = self._head_operand()
        if dropout is not None:
            keys, seed, samples = dropout
            return run.dropout_head(x, self.head_pos, self.head_bg, int(self.n_pos), hw, hb, keys, seed, samples)
        return run.head(x, hw, hb, ring, self.n_pos)

    def _forward_miopen(self, tiles, row0, dropout):
        """The same forward with the convolutions alone left to MIOpen: bias + ReLU + placement into the next tile is one HIP kernel per
        convolution output (swk_nhwc_bias_relu_place), max-pooling another (swk_nhwc_maxpool3s2), both on PyTorch's current stream.
        Same float32 operations per element as _forward_torch."""
        if dropout is not None:
            raise RuntimeError("dropout sampling runs on the library's HIP head kernel (own kernels, a two-class head)")
        k = tiles.shape[0]
        self._buffers(row0 + k)
        (bufs, live), aux = self._buf, self._aux
        rows = slice(row0, row0 + k)
        run = Launcher(tiles.device, k)
        conv1, head = self.model.features[0], self.model.classifier[1]
        a, b = self.pool1_slice
        c1buf = aux["conv1"][rows]
        run.bias_relu_place(F.conv2d(_nhwc(tiles), conv1.weight, None, stride=conv1.stride), a, b - a, conv1.bias, c1buf, 0, 0)
        x = aux["pool_in"][rows]
        run.maxpool(c1buf, x)
        pool_out = iter(aux["pool_out"])
        for j, p in enumerate(self.plan):
            if p.kind == "pool":
                x = next(pool_out)[rows]
                run.maxpool(bufs[j][rows], x)
                continue
            fire, sq = p.layer, bufs[j][rows]
            c, cn = p.crop
            dest, doff = self._fire_dest(j, bufs, live, rows)
            run.bias_relu_place(F.conv2d(x, fire.squeeze.weight, None), 0, p.n, fire.squeeze.bias, sq, p.off, 0)
            run.bias_relu_place(F.conv2d(sq, fire.expand1x1.weight, None), c, cn, fire.expand1x1.bias, dest, doff, 0)
            run.bias_relu_place(F.conv2d(sq, fire.expand3x3.weight, None), 0, cn, fire.expand3x3.bias, dest, doff, fire.expand1x1.out_channels)
            x = dest
        # the 512 -> 2 head (1 x 1 convolution + ReLU + spatial sum) as a plain matrix product over the channels-last pixels: no
        # convolution library on this path, hence no kernel search per batch shape
        px = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])                       # (B * live positions, 512): a view of the NHWC memory
        s = torch.relu(F.linear(px, head.weight.view(head.out_channels, -1), head.bias))
        s = s.view(k, -1, head.out_channels).sum(dim=1)
        return (s + self.ring_sum) / self.n_pos
