"""Drop-in for the reference's swiftwatcher/segment_classification.py (SegmentClassifier :14-44,
setup_model :47-67): same constructor and call signature, same preprocessing chain, same
keep-if-argmax==1 rule and 1..k relabelling -- with the SqueezeNet-1.0 forward batched over all
segments of the call; PyTorch-ROCm holds the tensors and streams, and the convolutions run on the library's own
HIP kernels (csrc/cnn_*.hip; MIOpen only with SWK_OWN_CNN_KERNELS=0, the tests' cross-check).

Differences from the reference, all deliberate:
  * the network is built in plain torch (torchvision is not needed) and is NOT fetched from the
    internet: setup_model's `pretrained=True` download is overwritten by model.pt anyway (:17, :51);
  * the model runs in eval() mode under no_grad: the reference never leaves train mode, so its
    Dropout(0.5) is live and its decisions are random; eval mode is the deterministic definition;
  * segments are classified in one batch instead of one 602 KB H2D copy + sync per segment;
  * by default only the part of each feature map the 24x24 patch can influence is evaluated
    (CroppedSqueezeNet10, 5.7x fewer MACs: 0.128 instead of 0.733 G per segment, same arithmetic per output); cropped=False runs the full network.

The reference's own behaviour -- Dropout(0.5) live in front of the head, every decision one draw -- can be SAMPLED: dropout_scores /
keep_probability score a segment under many dropout masks in one launch (swk_nhwc_head2_dropout_relu_mean), and
SegmentClassifier(dropout_seed=...) decides by one such realisation.  The mask is the library's own counter-based one (include/swk.h),
not torch's generator stream: the distribution of the reference's decision is reproduced, not a single run of it.
"""
import os
import threading

import numpy as np
import torch

# the network and its cropped evaluation live in squeezenet.py; their names stay importable from here
from .squeezenet import IMAGENET_MEAN, IMAGENET_STD, PAD, RESIZE, CroppedSqueezeNet10, Fire, Launcher, SqueezeNet10, _affected  # noqa: F401


def setup_model(num_classes):
    """segment_classification.py:47-67 minus the ImageNet download: the 2-class head replaces
    classifier[1] there, and every weight is then overwritten by model.pt."""
    model = SqueezeNet10(num_classes)
    for p in model.parameters():
        p.requires_grad = False
    return model


def resize_segment(segment_image):
    """ToPILImage -> Resize((24, 24)) of the reference's transform list (:19-20): PIL's bilinear
    resampling with its support scaling, on the uint8 HxWx3 crop taken as RGB (:30-32 feed BGR crops
    as they are).  A 24x24 crop passes through unchanged, like PIL."""
    if segment_image.shape[0] == RESIZE and segment_image.shape[1] == RESIZE:
        return np.ascontiguousarray(segment_image)
    from PIL import Image
    bil = getattr(Image, "Resampling", Image).BILINEAR
    return np.asarray(Image.fromarray(np.ascontiguousarray(segment_image)).resize((RESIZE, RESIZE), bil))


class SegmentClassifier:
    """segment_classification.py:14-44."""

    @classmethod
    def from_state_dict(cls, state, **kw):
        """Same as the constructor, from an in-memory state_dict (synthetic-weight benchmarks, tests)."""
        import io
        buf = io.BytesIO()
        torch.save(state, buf)
        buf.seek(0)
        return cls(buf, **kw)

    def __init__(self, model_path, device=None, batch_size=1024, cropped=True, dropout_seed=None):
        """dropout_seed: None = the eval-mode classifier (the parity definition).  An int: __call__, classify_frames and the device
        hand-over (predict_last_batch) decide by sample 0 of dropout_scores under that seed -- ONE realisation of a reference run, whose
        Dropout(0.5) is live; every segment's draw is fixed by its key (data_structures.segment_keys)."""
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("SegmentClassifier runs on the MI355X (PyTorch-ROCm); pass device='cpu' "
                                   "explicitly to run the torch CPU kernels instead")
            device = "cuda:0"
        self.device = torch.device(device)
        # MIOpen's exhaustive find instead of its immediate-mode heuristic for the convolutions left to it (the head; everything with
        # the fused kernels off): scoped to this classifier's forwards (torch.backends.cudnn.flags in _run), not set process-wide
        self._cudnn_benchmark = self.device.type == "cuda" and os.environ.get("SWK_CUDNN_BENCHMARK", "1") == "1"
        self.batch_size = batch_size
        self.model = setup_model(2)
        state = torch.load(model_path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(state, strict=True)
        self.model = self.model.to(self.device).eval()
        mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        self._mean, self._std = mean, std
        # Pad(100) puts zeros around the 24x24 patch BEFORE ToTensor/Normalize: the border is (0-mean)/std
        self._border = ((0.0 - mean) / std).expand(1, 3, 224, 224).contiguous()
        self.cropped = CroppedSqueezeNet10(self.model, ((0.0 - mean) / std).view(3)) if cropped else None
        # measurement hook (bench.py): with timing on, every network forward is bracketed by events on torch's
        # current stream; net_time() sums them
        self.timing = False
        self._events = []
        # device-side input buffers of scores_from_device / predict_last_batch: two slots, each with the event of the last forward
        # that read it (a slot is handed to the library's stream again only after that event)
        self._slots = None
        self._lock = threading.RLock()          # one scoring at a time (see _scores_device)
        # forwards of this many rows or more run as two chains on two streams (_forward_two_streams); 0 = never
        self._split_rows = int(os.environ.get("SWK_CNN_SPLIT_ROWS", "1024")) if self.device.type == "cuda" else 0
        self._side_stream = None
        self._graphs = {}
        self._use_graphs = self.device.type == "cuda" and os.environ.get("SWK_HIP_GRAPHS", "1") == "1"
        self._graph_error = None
        self.dropout_seed = None if dropout_seed is None else int(dropout_seed)
        self._full_head = None

    def preprocess(self, segment_images, window=False):
        """(:18-24, :31-33) for a list of HxWx3 uint8 crops -> float32 (B, 3, 224, 224) on the device, or with
        window=True only rows/cols 92..131 of it, (B, 3, 40, 40), which is all the cropped network reads.
        On the GPU the whole chain (Pillow-exact resize, pad, /255, normalise) is one HIP kernel that writes the
        network's input tensor in place (swk_classifier_input_window); crops larger than 512 px or a CPU device
        use the torch / Pillow statements below."""
        lo, hi = (CroppedSqueezeNet10.IN_LO, CroppedSqueezeNet10.IN_HI + 1) if window else (0, 224)
        if self.device.type == "cuda" and all(max(im.shape[0], im.shape[1]) <= 512 for im in segment_images):
            from . import _lib
            x = torch.empty((len(segment_images), 3, hi - lo, hi - lo), dtype=torch.float32, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()     # the library fills x on its own stream
            _lib.default_context(self.device.index or 0).classifier_input(segment_images, IMAGENET_MEAN, IMAGENET_STD,
                                                                          net_ptr=x.data_ptr(), pad=PAD - lo)
            # (x is a fresh allocation: the caching allocator may hand out a block whose last reader is still queued on
            # torch's stream -- hence the synchronize above, before the library's stream writes it)
            return x
        patches = np.stack([resize_segment(im) for im in segment_images])              # (B, 24, 24, 3) u8
        t = torch.from_numpy(patches).to(self.device).permute(0, 3, 1, 2).to(torch.float32).div_(255.0)   # ToTensor
        t = (t - self._mean) / self._std                                               # Normalize
        x = self._border[:, :, lo:hi, lo:hi].repeat(t.shape[0], 1, 1, 1)
        x[:, :, PAD - lo:PAD - lo + RESIZE, PAD - lo:PAD - lo + RESIZE] = t
        return x

    @torch.no_grad()
    def _bucket(self, k):
        """Batch size the network is run at for k inputs: a counting loop hands over a different number of segments every call, and
        a few fixed shapes keep the per-shape state small (persistent tiles are sized by the largest; with the fused kernels off
        MIOpen searches once per shape) -- so on the GPU the batch is padded to a multiple of 64 up to 512 rows, beyond that to a
        multiple of 512 up to batch_size.  The padding rows are scored and thrown away."""
        if self.device.type != "cuda":
            return k
        if k >= self.batch_size:
            return max(self.batch_size, k)
        if k <= 512:                         # a FrameQueue window's worth of segments: 64-row steps
            return min(self.batch_size, -(-k // 64) * 64)
        return min(self.batch_size, -(-k // 512) * 512)

    def _forward(self, x):
        net = self.cropped
        if net is not None and net.own_kernels:
            if self._split_rows and x.shape[0] >= self._split_rows and net._gpu_path(x):
                return self._forward_two_streams(x)
            return net(x)
        # (nothing of the default GPU path is a MIOpen convolution: the setting only matters for the full network and the cross-check)
        forward = self.model if net is None else net
        if not self._cudnn_benchmark:
            return forward(x)
        with torch.backends.cudnn.flags(enabled=True, benchmark=True):
            return forward(x)

    def _full_head_operand(self, n_pos):
        """What the dropout head reads on the full network: the head's weights and bias, and every position as a live one."""
        if self._full_head is None or self._full_head[2].shape[0] != n_pos:
            head = self.model.classifier[1]
            self._full_head = (head.weight.detach().reshape(head.out_channels, -1).contiguous(), head.bias.detach().contiguous(),
                               torch.arange(n_pos, dtype=torch.int32, device=self.device))
        return self._full_head

    @torch.no_grad()
    def _forward_dropout(self, x, keys, samples, seed):
        """(k, samples, 2) scores of the network inputs x under the reference's live Dropout(0.5): everything up to the last Fire's
        output is the eval forward's (SqueezeNet has no batch norm: train mode differs from eval mode in the head alone), then the
        dropout head.  One chain on the current stream, never captured; every operand it reads was made on this stream before
        (CroppedSqueezeNet10.__init__ and reserve)."""
        if self.device.type != "cuda":
            raise RuntimeError("dropout sampling runs on the library's HIP head kernel: it needs the GPU")
        samples = int(samples)
        if not 1 <= samples <= 256:
            raise ValueError("samples must be 1..256")
        if self.cropped is not None:
            if not (self.cropped.own_kernels and self.cropped._gpu_path(x)):
                raise RuntimeError("dropout sampling runs on the library's own kernels (SWK_OWN_CNN_KERNELS=1, channels-last)")
            self.cropped.reserve(x.shape[0])
            return self.cropped(x, dropout=(keys, int(seed), samples))
        with torch.cuda.device(self.device):
            with torch.backends.cudnn.flags(enabled=True, benchmark=self._cudnn_benchmark):
                f = self.model.features(x)
            f = f.contiguous(memory_format=torch.channels_last)
            n_pos = f.shape[2] * f.shape[3]
            hw, hb, pos = self._full_head_operand(n_pos)
            return Launcher(self.device, f.shape[0]).dropout_head(f, pos, None, n_pos, hw, hb, keys, int(seed), samples)

    def _keys_tensor(self, keys, k):
        if not (isinstance(keys, np.ndarray) and keys.dtype in (np.uint64, np.int64)):
            # anything else goes through Python ints, two's complement in 64 bits (numpy would round a list that mixes a negative key
            # with one of 2**63 or more through float64)
            keys = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(keys, dtype=object).reshape(-1)], dtype=np.uint64)
        keys = np.ascontiguousarray(keys.reshape(-1)).view(np.int64)
        if keys.shape[0] != k:
            raise ValueError("%d keys for %d segments" % (keys.shape[0], k))
        return torch.from_numpy(keys.copy()).to(self.device)

    def dropout_scores(self, segment_images, keys, samples=32, seed=0):
        """Scores of every segment under `samples` realisations of the reference's live Dropout(0.5): float32 (k, samples, 2) on the
        device.  keys: one uint64 per segment (data_structures.segment_keys: (parent frame number << 8) | label); the mask of sample s
        is a function of (seed, key, s, position, channel) alone (include/swk.h), so a segment's scores do not depend on the batch it is
        scored in.  Cropped and full network alike; the mask is the library's own, not torch's generator stream."""
        with self._lock:
            kt = self._keys_tensor(keys, len(segment_images))
            out = []
            for i in range(0, len(segment_images), self.batch_size):
                chunk = segment_images[i:i + self.batch_size]
                x = self.preprocess(chunk, window=self.cropped is not None)
                out.append(self._forward_dropout(x, kt[i:i + len(chunk)], samples, seed))
            return torch.cat(out) if out else torch.zeros((0, int(samples), 2), device=self.device)

    def keep_probability(self, segments, samples=32, seed=0):
        """Per segment (Segment objects), the share of `samples` dropout realisations that keep it: score[1] > score[0] (a tie drops
        the segment, as torch.max picks index 0).  float64 numpy array (k,)."""
        from .data_structures import segment_keys
        if not segments:
            return np.zeros(0, np.float64)
        keys = segment_keys([s.parent_frame_number for s in segments], [s.label for s in segments])
        sc = self.dropout_scores([s.segment_image for s in segments], keys, samples, seed)
        return (sc[:, :, 1] > sc[:, :, 0]).sum(dim=1).cpu().numpy().astype(np.float64) / float(int(samples))

    def _predict_images(self, segments):
        """Predicted class of each segment from its image: eval mode, or sample 0 under dropout_seed."""
        images = [s.segment_image for s in segments]
        if self.dropout_seed is None:
            return torch.max(self.scores(images), 1)[1].cpu().numpy()
        from .data_structures import segment_keys
        keys = segment_keys([s.parent_frame_number for s in segments], [s.label for s in segments])
        return torch.max(self.dropout_scores(images, keys, 1, self.dropout_seed)[:, 0], 1)[1].cpu().numpy()

    def _forward_two_streams(self, x):
        """A large forward as two forwards on disjoint rows of the persistent tiles, the second on a side stream.  The kernels of a
        forward alternate between the matrix pipe (3 x 3 expands, 70 % busy at 1 TB/s) and memory (squeezes, expand1x1: half the HBM
        rate), and every one of its 34 launches ends with a tail of part-filled CUs; two chains fill each other's gaps: 13.86 against
        14.66 ms per 8,192 rows (tools/r4/two_stream_forward.py; three chains 13.97, four 14.48; tools/r4/chunked_forward.py: 2,048 rows
        as 2 x 1,024 take 9 % less than as one chain, 1,024 as 2 x 512 8 % less; window-sized forwards gain nothing, see _forward_graphed).  Same kernels on the same rows, the
        head included (swk_nhwc_head2_relu_mean sums in an order fixed by the shapes): the scores are the single chain's bit for bit."""
        k = x.shape[0]
        half = -(-k // 2 // 512) * 512
        cur = torch.cuda.current_stream(self.device)
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self.device)
        side = self._side_stream
        self.cropped.reserve(k)                     # the tiles grow on THIS stream, before either half looks them up
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            hi = self.cropped(x[half:], row0=half)
        lo = self.cropped(x[:half])
        cur.wait_stream(side)
        hi.record_stream(cur)
        return torch.cat([lo, hi])

    def _forward_graphed(self, x):
        """A window's worth of segments (<= 512 rows) is some thirty kernels of a few microseconds each: launched one by one from
        Python they cost more host time than GPU time.  The forward on a persistent input slot is captured once per (slot, rows) as a
        HIP graph and replayed with one launch.  Anything that goes wrong while capturing switches this off for the classifier."""
        key = (x.data_ptr(), int(x.shape[0]), self.cropped.version)
        entry = self._graphs.get(key)
        if entry is None:
            try:
                self._forward(x)                                            # kernel attributes, persistent tiles, library handles
                torch.cuda.current_stream(self.device).synchronize()
                graph = torch.cuda.CUDAGraph()
                # thread-local capture mode: another thread may be inside the library meanwhile (a reader that segments ahead:
                # stream synchronisations, allocations) -- under the default, global mode those calls fail while this one captures
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    # (two halves on two streams inside the graph -- forwards on disjoint rows of the persistent tiles, row0 --
                    # were measured: 3.11 against 3.17 ms per window of the counting loop, no gain; one chain it is)
                    out = self._forward(x)
                if len(self._graphs) >= 24:
                    self._graphs.clear()
                entry = self._graphs[key] = (graph, out)
            except Exception as exc:                                        # noqa: BLE001
                self._use_graphs = False
                self._graph_error = repr(exc)
                torch.cuda.synchronize(self.device)
                return self._forward(x)
        entry[0].replay()
        return entry[1]

    def _run(self, x, k, persistent=False):
        """Scores of the first k rows of x (x has _bucket(k) rows).  persistent: x is one of the classifier's own input slots."""
        if persistent and self._use_graphs and x.shape[0] <= 512 and self.cropped is not None and not self.timing:
            return self._forward_graphed(x)[:k]
        if self.timing and self.device.type == "cuda":
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = self._forward(x)[:k]
            b.record()
            self._events.append((a, b, int(x.shape[0])))
            return out
        return self._forward(x)[:k]

    def net_time(self, reset=True):
        """(milliseconds, rows pushed through the network, forwards) of the timed forwards since the last reset."""
        if self._events:
            torch.cuda.synchronize(self.device)
        ms = sum(a.elapsed_time(b) for a, b, _ in self._events)
        rows, calls = sum(r for _, _, r in self._events), len(self._events)
        if reset:
            self._events = []
        return ms, rows, calls

    def _scores_unlocked(self, segment_images):
        out = []
        for i in range(0, len(segment_images), self.batch_size):
            chunk = segment_images[i:i + self.batch_size]
            k, b = len(chunk), self._bucket(len(chunk))
            x = self.preprocess(chunk, window=self.cropped is not None)
            if b != k:
                x = torch.cat([x, x[:1].expand(b - k, -1, -1, -1)])
            out.append(self._run(x, k))
        return torch.cat(out) if out else torch.zeros((0, 2), device=self.device)

    def _device_slots(self, side, nhwc):
        key = (side, nhwc, self.batch_size)
        if self._slots is None or self._slots[0] != key:
            fmt = torch.channels_last if nhwc else torch.contiguous_format
            xb = [torch.empty((self.batch_size, 3, side, side), dtype=torch.float32, device=self.device, memory_format=fmt) for _ in range(2)]
            fb = [torch.empty((self.batch_size,), dtype=torch.int32, device=self.device) for _ in range(2)]
            torch.cuda.current_stream(self.device).synchronize()          # fresh blocks: nothing queued on torch's stream may still read them
            self._slots = (key, xb, fb, [None, None])
        return self._slots[1:]

    def scores(self, segment_images):
        with self._lock:
            return self._scores_unlocked(segment_images)

    def _scores_device(self, cut, keys=None):
        """_scores_device_unlocked under the classifier's lock: the input slots, their events, the captured graphs and the forward's
        buffers belong to the classifier, and two threads score through one classifier when a reader segments (and scores) ahead
        beside the counting loop (io_frames.PresegmentingReader, pipeline.py windows_per_call): one scoring at a time."""
        with self._lock:
            return self._scores_device_unlocked(cut, keys)

    @torch.no_grad()
    def _scores_device_unlocked(self, cut, keys=None):
        """Scores of a device-resident batch.  cut(net_ptr, frame_ptr, net_cap, first, pad, channels_last) -> (total, skipped) writes
        the network inputs of segments [first, first + net_cap) (a library call: its own stream, synchronous).  Two input slots: the
        library cuts and resamples chunk i + 1 while PyTorch's stream runs the network on chunk i; a slot is written again only after
        the forward that read it has finished (its event) -- also across calls, the slots and events belong to the classifier.
        keys (one uint64 per segment of the batch, with dropout_seed set): the scores are sample 0 of the dropout head instead."""
        if self.device.type != "cuda":
            raise RuntimeError("device-resident scoring needs the GPU")
        pad = PAD - CroppedSqueezeNet10.IN_LO if self.cropped is not None else PAD
        side = RESIZE + 2 * pad
        bs = self.batch_size
        # the cropped network's convolution kernels read channels-last: the input is written that way (a copy per forward less)
        nhwc = self.cropped is not None and self.cropped.memory_format == torch.channels_last
        xb, fb, done = self._device_slots(side, nhwc)

        def produce(slot, first):
            if done[slot] is not None:
                done[slot].synchronize()
            total, skipped = cut(xb[slot].data_ptr(), fb[slot].data_ptr(), bs, first, pad, nhwc)
            if skipped:
                raise RuntimeError("%d segment boxes were empty or had a side above 4096 pixels" % skipped)
            return total

        scores, frames_of = [], []
        total = produce(0, 0)
        kt = self._keys_tensor(keys, total) if keys is not None else None
        first, i = 0, 0
        while first < total:
            slot = i & 1
            k = min(bs, total - first)
            if kt is not None:
                scores.append(self._forward_dropout(xb[slot][:k], kt[first:first + k], 1, self.dropout_seed)[:, 0])
            else:
                scores.append(self._run(xb[slot][:self._bucket(k)], k, persistent=True).clone())     # rows past k hold an earlier chunk: scored, dropped
            frames_of.append(fb[slot][:k].clone())
            done[slot] = torch.cuda.Event()
            done[slot].record(torch.cuda.current_stream(self.device))
            first += k
            i += 1
            if first < total:
                produce(i & 1, first)
        if not scores:
            return torch.zeros((0, 2), device=self.device), torch.zeros((0,), dtype=torch.int32, device=self.device)
        return torch.cat(scores), torch.cat(frames_of)

    def scores_from_device(self, ctx, inp, frame_hw, segs, nseg, seg_cap, min_seg_size=(24, 24)):
        """The classifier on a whole batch_run without leaving the GPU: inp is the swk_input of that call (device
        frames), segs / nseg its device region records (torch tensors).  The crops of extract_segment_images
        (image_filtering.py:338-369) are cut, resized and normalised by swk_segment_inputs into the network's input
        tensor, batch_size segments at a time.  Returns (scores (T, 2), frame index (T,) int32), both on the device,
        segments in frame order then ascending label -- the order FrameQueue hands them to __call__."""
        def cut(net_ptr, frame_ptr, cap, first, pad, nhwc):
            return ctx.segment_inputs(inp, frame_hw, segs.data_ptr(), nseg.data_ptr(), seg_cap, IMAGENET_MEAN, IMAGENET_STD, net_ptr, cap,
                                      first=first, pad=pad, min_seg_size=min_seg_size, seg_frame_ptr=frame_ptr, channels_last=nhwc)
        return self._scores_device(cut)

    def predict_last_batch(self, ctx, generation, total, min_seg_size=(24, 24), keys=None):
        """Predicted class of every segment of the batch `ctx` ran last (FrameQueue.segment_queue's window), in batch order: an int64
        device tensor (total,), not waited for.  The inputs are cut from what that batch left on the device (swk_segment_inputs_last);
        raises _lib.StaleBatch when the context has moved on.  keys: the segments' dropout keys in batch order, needed (and only
        read) when the classifier has a dropout_seed."""
        if self.dropout_seed is not None and keys is None:
            raise ValueError("a classifier with a dropout_seed needs the segments' keys")
        if self.dropout_seed is None:
            keys = None
        def cut(net_ptr, frame_ptr, cap, first, pad, nhwc):
            return ctx.segment_inputs_last(generation, IMAGENET_MEAN, IMAGENET_STD, net_ptr, cap, first=first, pad=pad,
                                           min_seg_size=min_seg_size, seg_frame_ptr=frame_ptr, channels_last=nhwc, known_total=total)
        scores, _ = self._scores_device(cut) if keys is None else self._scores_device(cut, keys)
        if scores.shape[0] != total:
            raise RuntimeError("the device holds %d segments, the window has %d" % (scores.shape[0], total))
        return torch.max(scores, 1)[1]                                   # :36-39

    def classify_frames(self, frames):
        """__call__ for many frames with ONE scoring batch: every frame's segments replaced by the kept ones,
        relabelled 1..k per frame (:41-42)."""
        if any(fr.segments for fr in frames):
            for fr, kept in zip(frames, self._keep_and_relabel([fr.segments for fr in frames])):
                fr.segments = kept

    def _window_predictions(self, segments):
        """Segments that FrameQueue.segment_queue made carry their window (data_structures.WindowBatch) and their index in it:
        the first call of a window scores ALL its segments in one device-resident batch, the others look their rows up.  None
        when the segments are not such a group or the window's device state is gone (the caller then scores their images)."""
        if self.device.type != "cuda":
            return None
        batch = getattr(segments[0], "_batch", None)
        if batch is None or any(getattr(s, "_batch", None) is not batch for s in segments):
            return None
        if (self.device.index or 0) != batch.ctx.device:
            return None
        table = batch.predictions(self)
        if table is None:
            return None
        return [table[s._index] for s in segments]

    def __call__(self, segments):
        """:26-44: keep segments whose argmax is class 1 (ties / all-zero scores give 0 and are
        dropped, as torch.max does), relabel the kept ones 1..k."""
        return self._keep_and_relabel([segments])[0] if segments else []

    def _keep_and_relabel(self, groups):
        """The segments of every group (a frame's) that the classifier keeps, relabelled 1..k per group; all groups are scored as ONE
        batch."""
        segs = [s for g in groups for s in g]
        pred = self._window_predictions(segs)                 # segments of one segment_windows / segment_queue call: device-resident
        if pred is None:
            pred = self._predict_images(segs)
        out, i = [], 0
        for g in groups:
            kept = [s for s, y in zip(g, pred[i:i + len(g)]) if y == 1]
            i += len(g)
            for j, s in enumerate(kept):
                s.label = j + 1
            out.append(kept)
        return out
