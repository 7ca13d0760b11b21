"""The uint8 input side (reference datasets.build_dataloader: timm's fast_collate + PrefetchLoader).

The reference's loaders hand over uint8 NCHW batches and normalise them on the GPU with mean * 255 / std * 255.  The two classes
here are that contract on the HIP path: the bytes cross the bus (4x fewer than fp32) and one `vr_normalize_u8` pass -- or, in
training, the `vr_token_mix_u8` pass of `SwitchTokenMix(input_norm=...)` -- makes the fp32 batch the model reads.

  DevicePrefetchLoader   timm's PrefetchLoader: host batches, copied one batch ahead on a side stream.
  ResidentU8Batches      a hold-out set kept on the device as uint8 (a quarter of its fp32 size), re-iterable: what
                         evo_eval.score_candidate / score_population and engine.evaluate take as `batches`.
  pad_collate_u8         a collate function for decoded images of different sizes: one zero-padded uint8 canvas per batch.
  DeviceCropLoader       canvases in, cropped / resized / mirrored uint8 [B,3,S,S] device batches out (vr_resample_u8 with the boxes
                         of a vitres.resized_crop transform): what the two classes above, SwitchTokenMix(input_norm=) and
                         Mixup(input_norm=) take.  augment=RandAugment(...) (vitres.rand_augment) runs the recipes' --aa stage on
                         the cropped batch as well (vr_rand_augment_u8), so the default recipe's whole pixel chain is on the device.

  jpeg_collate           a collate function for ENCODED files: baseline JPEG streams are Huffman-decoded on the host
                         (libvitres_jpeg.so, vitres.jpeg) into one coefficient blob per batch; anything else is decoded by PIL.
  DeviceJpegLoader       those blobs in, the canvases pad_collate_u8 would have made out -- on the device (vr_jpeg_reconstruct_u8:
                         dequantise, inverse DCT, chroma upsampling, colour conversion, placement): what DeviceCropLoader takes.

  ragged_collate_u8      pad_collate_u8's ragged sibling: every image in planes of its OWN size in one flat buffer (no canvas of the
                         batch maxima), with the plane table vr_resample_ragged_u8 reads.  DeviceCropLoader takes its batches too.
  RaggedCanvas           what DeviceJpegLoader(ragged=True) yields in the canvas's place: the flat device buffer and its plane table
                         (vr_jpeg_reconstruct_ragged_u8).  Memory, traffic and the resample's cost then follow the batch's pixels,
                         not B times its largest image, and no image is too large for the crop (sides up to 8192).

What is not here: the entropy decoding of JPEG stays on host cores (in the loader's workers); progressive, arithmetic-coded and
non-JPEG files are decoded there entirely, by PIL.  ColorJitter is not implemented: timm skips it
whenever auto_augment is set, so no shipped recipe runs it.  Random
erasing, which timm applies to the normalised image, cannot happen there any more: `erase=` (a vitres.random_erasing.RandomErasing)
folds it into the normalising pass -- here with normalize=True, in the mix (`SwitchTokenMix(..., erase=)`, `Mixup(..., erase=)`) in training.
"""
import io

import numpy as np
import torch

from . import jpeg as J
from . import kernels as K


class _Upload:
    """The copies of one batch: every tensor a loader sends to the device goes through here, so what has to be kept alive across
    the two streams is known here and nowhere else.  With a side stream the copies are non-blocking and issued on it (pinned host
    batches make them asynchronous), int tables are staged in pinned memory, and hand_over() makes the current stream wait for them
    and own the tensors.  side=None (not a GPU): plain copies, nothing to overlap or to wait for."""

    def __init__(self, device, side):
        self.device, self.side, self.moved, self.copied = device, side, [], None

    def __call__(self, t):
        if t.is_cuda:                             # (a RaggedCanvas's buffer, made on the consumer's stream: nothing to copy or to keep)
            return t
        if self.side is None:
            return t.to(self.device)
        with torch.cuda.stream(self.side):
            t = t.to(self.device, non_blocking=True)
        self.moved.append(t)
        return t

    def table(self, array):
        """A host int array as an int32 device tensor."""
        host = torch.empty(array.shape, dtype=torch.int32, pin_memory=self.side is not None)
        host.numpy()[...] = array
        return self(host)

    def issued(self):
        self.copied = None if self.side is None else self.side.record_event()

    def hand_over(self):
        if self.copied is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self.copied)
            for t in self.moved:                  # (allocated on the side stream, used on this one)
                t.record_stream(cur)


class _LookAheadLoader:
    """timm's PrefetchLoader pattern, once: while a batch is consumed the next one is fetched from the wrapped loader, staged and
    copied to `device` on a side stream; every batch is handed over on the current stream.  A subclass says what a batch needs:
      _stage(up, *batch)   at upload time, in the loader's order: the host checks, the random draws, and up(tensor) / up.table(array)
                           for whatever goes to the device; returns the arguments of _launch
      _launch(*staged)     at hand-over, on the current stream, after the copies: the kernels; returns what is yielded
    __len__, .sampler and .dataset are the wrapped loader's."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)

    def __len__(self):
        return len(self.loader)

    @property
    def sampler(self):
        return self.loader.sampler

    @property
    def dataset(self):
        return self.loader.dataset

    def _upload(self, side, batch):
        up = _Upload(self.device, side)
        staged = self._stage(up, *batch)
        up.issued()
        return up, staged

    def _hand_over(self, up, staged):
        up.hand_over()
        return self._launch(*staged)

    def __iter__(self):
        side = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        ahead = None
        for batch in self.loader:
            nxt = self._upload(side, batch)
            if ahead is not None:
                yield self._hand_over(*ahead)
            ahead = nxt
        if ahead is not None:
            yield self._hand_over(*ahead)


class DevicePrefetchLoader(_LookAheadLoader):
    """Counterpart of timm's PrefetchLoader over a loader of (uint8 NCHW CPU batch, target) pairs: the next batch is copied to
    `device` on a side stream while the current one is consumed, and every batch is yielded as (normalize_u8(batch), target) on the
    current stream.  normalize=False yields the uint8 device batch itself -- the training loop's form, where
    SwitchTokenMix(input_norm=(mean, std)) normalises inside the mix.  mean / std: per-channel, 0..1 units.  Pinned host batches
    (pin_memory=True) make the copies asynchronous.  erase=RandomErasing(...): every batch is yielded erased as well
    (vr_normalize_u8_erase, the same pass); with normalize=False the mix owns the erase and erase= here raises.  __len__, .sampler
    and .dataset are the wrapped loader's."""

    def __init__(self, loader, device, mean=K.IMAGENET_DEFAULT_MEAN, std=K.IMAGENET_DEFAULT_STD, normalize=True, erase=None):
        if erase is not None and not normalize:
            raise ValueError("DevicePrefetchLoader(normalize=False, erase=...): random erasing works on normalised pixels, so it "
                             "belongs to whoever normalises -- pass erase= to SwitchTokenMix / Mixup(input_norm=...) instead")
        super().__init__(loader, device)
        self.normalize, self.erase = normalize, erase
        self.norm = K.norm_constants(mean, std)

    def _stage(self, up, batch, target):
        if batch.dtype != torch.uint8:
            raise TypeError("DevicePrefetchLoader takes uint8 NCHW batches (timm's fast_collate), got %s" % batch.dtype)
        return up(batch), up(target)

    def _launch(self, u8, target):
        if self.erase is not None:
            B, _, H, W = u8.shape
            return K.normalize_u8_erase(u8, *self.norm, self.erase.next_args(B, H, W, u8.device if u8.is_cuda else None)), target
        return (K.normalize_u8(u8, *self.norm) if self.normalize else u8), target


class ResidentU8Batches:
    """A re-iterable over a uint8 image set [N,C,H,W] and its targets [N] that live on the device: yields (fp32 batch, targets)
    with the batch normalised by vr_normalize_u8 into one of TWO alternating output buffers -- nothing is allocated per batch, the
    last batch is short when batch_size does not divide N.  A yielded batch is valid until the batch after next is requested (of
    this or a later iteration): consumers that only launch work on the current stream, as the evaluation loops do, need nothing
    more.  mean / std: per-channel, 0..1 units."""

    def __init__(self, images_u8, targets, batch_size, mean=K.IMAGENET_DEFAULT_MEAN, std=K.IMAGENET_DEFAULT_STD):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
            raise TypeError("ResidentU8Batches takes a uint8 [N,C,H,W] tensor, got %s %s" % (images_u8.dtype, tuple(images_u8.shape)))
        if targets.shape[0] != images_u8.shape[0] or batch_size <= 0:
            raise ValueError("ResidentU8Batches: one target per image and a positive batch size expected")
        self.images, self.targets, self.batch_size = images_u8.contiguous(), targets, int(batch_size)
        self.norm = K.norm_constants(mean, std)
        n = min(self.batch_size, self.images.shape[0])
        self._bufs = [torch.empty((n,) + tuple(self.images.shape[1:]), dtype=torch.float32, device=self.images.device)
                      for _ in range(2)]
        self._turn = 0

    def __len__(self):
        return (self.images.shape[0] + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for lo in range(0, self.images.shape[0], self.batch_size):
            u8 = self.images[lo:lo + self.batch_size]
            out = self._bufs[self._turn][:u8.shape[0]]
            self._turn ^= 1
            yield K.normalize_u8(u8, *self.norm, out=out), self.targets[lo:lo + self.batch_size]


def _sample_labels(samples, what):
    """The labels of a non-empty list of (image, label) samples as an int64 tensor."""
    if not samples:
        raise ValueError("%s: an empty batch" % what)
    return torch.as_tensor(np.asarray([int(label) for _, label in samples], dtype=np.int64))


def _decoded_samples(samples, what):
    """(images, sizes int32 [B,2] of (h, w), labels int64 [B]) of a list of (HWC uint8 array, label): non-empty arrays of one channel
    count, or TypeError."""
    labels = _sample_labels(samples, what)
    images = [np.asarray(img) for img, _ in samples]
    for img in images:
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != images[0].shape[2] or 0 in img.shape:
            raise TypeError("%s takes non-empty HWC uint8 arrays of one channel count, got %s %s" % (what, img.dtype, img.shape))
    return images, np.array([img.shape[:2] for img in images], dtype=np.int32), labels


def pad_collate_u8(samples):
    """Collate a list of (HWC uint8 array, label) -- decoded images of any sizes, one channel count -- into
    (canvas uint8 [B,C,Hs,Ws], sizes int32 [B,2] of (h, w), labels int64 [B]): every image sits in the top-left corner of its
    canvas plane, the rest is zero; Hs and Ws are the batch maxima rounded up to a multiple of 4 (vr_resample_u8 reads rows as
    dwords).  What a DataLoader(collate_fn=pad_collate_u8) hands to DeviceCropLoader."""
    images, sizes, labels = _decoded_samples(samples, "pad_collate_u8")
    Hs, Ws = ((int(v) + 3) // 4 * 4 for v in sizes.max(axis=0))
    canvas = np.zeros((len(images), images[0].shape[2], Hs, Ws), dtype=np.uint8)
    for b, img in enumerate(images):
        canvas[b, :, :img.shape[0], :img.shape[1]] = img.transpose(2, 0, 1)
    return torch.from_numpy(canvas), torch.from_numpy(sizes), labels


def ragged_collate_u8(samples):
    """pad_collate_u8 without the canvas: a list of (HWC uint8 array, label) -- decoded images of any sizes, one channel count --
    into (flat uint8 [n], planes int32 [B,8], sizes int32 [B,2] of (h, w), labels int64 [B]), plain tensors so that pin_memory=True
    works.  Every image lies in C planes of its own size (kernels.ragged_layout: pitch = its width rounded up to 4, rows = its
    height, channel c at off + c * rows * pitch, every sample on a multiple of 16 bytes); pad columns and the bytes between
    samples are zero.  The first reserved word of every record notes the channel count (the device ignores it).  What a DataLoader(collate_fn=ragged_collate_u8) hands to DeviceCropLoader."""
    images, sizes, labels = _decoded_samples(samples, "ragged_collate_u8")
    C = images[0].shape[2]
    planes, nbytes = K.ragged_layout(sizes, C)
    planes["reserved"][:, 0] = C              # (for DeviceCropLoader: the device ignores the reserved words)
    flat = np.zeros(nbytes, dtype=np.uint8)
    for img, p in zip(images, planes):
        h, w = img.shape[:2]
        off, pitch = int(p["off"]), int(p["pitch"])
        flat[off:off + C * h * pitch].reshape(C, h, pitch)[:, :, :w] = img.transpose(2, 0, 1)
    return (torch.from_numpy(flat), torch.from_numpy(planes.view(np.int32).reshape(len(images), K.RAGGED_PLANE_INTS)),
            torch.from_numpy(sizes), labels)


class RaggedCanvas:
    """A batch of images in ragged planes on the device: .flat (uint8 [n]), .planes (the device table, int32 [B,8]), .host_planes
    (its host copy, a kernels.ragged_planes array) and .channels.  What DeviceJpegLoader(ragged=True) yields where the padded form
    yields a canvas; DeviceCropLoader takes either."""

    def __init__(self, flat, planes, host_planes, channels=3):
        self.flat, self.planes, self.host_planes, self.channels = flat, planes, host_planes, int(channels)

    def plane(self, b, size=None):
        """Sample b's planes as a [C, rows, pitch] view of .flat ([C, h, w] with size=(h, w))."""
        p = self.host_planes[b]
        off, rows, pitch = int(p["off"]), int(p["rows"]), int(p["pitch"])
        view = self.flat[off:off + self.channels * rows * pitch].view(self.channels, rows, pitch)
        return view if size is None else view[:, :int(size[0]), :int(size[1])]


class DeviceCropLoader(_LookAheadLoader):
    """Over a loader of (canvas uint8 [B,C,Hs,Ws], sizes [B,2], labels) host batches (pad_collate_u8): yields
    (uint8 [B,C,S,S] on `device`, labels on `device`), the canvas cropped, resized and mirrored by vr_resample_u8 with the boxes
    `transform.draw(sizes)` makes (a vitres.resized_crop.RandomResizedCrop or ResizeCenterCrop: .draw, .size, .filter).  The canvas,
    the box table and the labels are copied one batch ahead on a side stream (the DevicePrefetchLoader pattern; pinned host batches
    make the copies asynchronous); the boxes are drawn, and checked against the canvas, in the loader's order when a batch is
    uploaded.  The output is what DevicePrefetchLoader, SwitchTokenMix(input_norm=), Mixup(input_norm=) and ResidentU8Batches take;
    nothing is normalised here.  augment=RandAugment(...) (vitres.rand_augment: .draw(B), .fill, .size): the batch's op table is drawn
    after its boxes, copied with them, and vr_rand_augment_u8 runs on the cropped batch (3 channels); augment=None adds nothing.
    A loader of ragged batches -- (flat, planes, sizes, labels) of ragged_collate_u8, or (RaggedCanvas, sizes, labels) of
    DeviceJpegLoader(ragged=True) -- is taken as well: the same draws, checked against every sample's own plane, through
    vr_resample_ragged_u8, whose workspace is kept and grown as batches need.  The yielded batches are the same bytes wherever the
    padded route works; the ragged one has no image too large for it.
    __len__, .sampler and .dataset are the wrapped loader's."""

    def __init__(self, loader, transform, device, augment=None):
        super().__init__(loader, device)
        self.transform, self.augment = transform, augment
        self._rws = None                      # the ragged resample's workspace
        if augment is not None:
            size = (transform.size, transform.size) if isinstance(transform.size, int) else tuple(transform.size)
            if tuple(augment.size) != size:
                raise ValueError("DeviceCropLoader: the augmentation draws for %s images, the transform makes %s" % (augment.size, size))

    def _stage(self, up, *batch):
        if len(batch) == 4 or isinstance(batch[0], RaggedCanvas):
            return self._stage_ragged(up, *batch)
        canvas, sizes, labels = batch
        if canvas.dtype != torch.uint8 or canvas.dim() != 4:
            raise TypeError("DeviceCropLoader takes uint8 [B,C,Hs,Ws] canvases (pad_collate_u8), got %s %s" % (canvas.dtype,
                                                                                                              tuple(canvas.shape)))
        B, _, Hs, Ws = canvas.shape
        sizes = np.asarray(sizes, dtype=np.int64)
        if sizes.shape != (B, 2) or (sizes[:, 0] > Hs).any() or (sizes[:, 1] > Ws).any():
            raise ValueError("DeviceCropLoader: sizes must hold one (h, w) inside the %d x %d canvas per sample" % (Hs, Ws))
        _, table, ops = self._draw(up, sizes, lambda boxes: K.check_resample_boxes(boxes, B, Hs, Ws, self.transform.size))
        canvas = up(canvas)
        return (lambda: K.resample_u8(canvas, table, self.transform.size, self.transform.filter)), ops, up(labels)

    def _stage_ragged(self, up, flat, planes, sizes, labels=None):
        if isinstance(flat, RaggedCanvas):    # (already on the device: DeviceJpegLoader(ragged=True) yields (canvas, sizes, labels))
            flat, planes, sizes, labels, C = flat.flat, flat.host_planes.copy(), planes, sizes, flat.channels
        else:
            if flat.dtype != torch.uint8 or flat.dim() != 1 or planes.dtype != torch.int32 or planes.dim() != 2:
                raise TypeError("DeviceCropLoader takes ragged batches as (flat uint8 [n], planes int32 [B,8], sizes, labels) "
                                "(ragged_collate_u8)")
            planes = np.ascontiguousarray(planes.numpy()).view(K.RAGGED_PLANE_DTYPE).reshape(-1).copy()
            C = int(planes["reserved"][0, 0]) or 3   # (ragged_collate_u8's note of the channel count: a flat buffer does not say)
        sizes = np.asarray(sizes, dtype=np.int64)
        K.check_ragged_planes(planes, C, int(flat.numel()), sizes, "DeviceCropLoader")
        size = self.transform.size
        boxes, table, ops = self._draw(up, sizes, lambda boxes: K.check_ragged_boxes(boxes, planes, size))
        need = K.ragged_ws_offsets(planes, C, K._out_size(size)[1], boxes[:, 3])     # (fills the planes' ws_off: before they are staged)
        bounds = K.ragged_bounds(planes)
        flat, planes = up(flat), up.table(planes.view(np.int32).reshape(-1, K.RAGGED_PLANE_INTS))

        def resample():
            if self._rws is None or self._rws.numel() < need:
                self._rws = torch.empty(need, dtype=torch.uint8, device=self.device)
            return K.resample_ragged_u8(flat, planes, table, C, size, self.transform.filter, workspace=self._rws, bounds=bounds)
        return resample, ops, up(labels)

    def _draw(self, up, sizes, check):
        """A batch's random draws, in their order -- the boxes, then the RandAugment table -- each checked on the host and staged:
        (the checked host box table, the device one, the device op table or None)."""
        boxes = check(self.transform.draw(sizes))
        table = up.table(boxes)
        ops = None if self.augment is None else up.table(K.check_ra_table(self.augment.draw(len(sizes)), len(sizes)))
        return boxes, table, ops

    def _launch(self, resample, ops, labels):
        crop = resample()
        return (crop if ops is None else K.rand_augment_u8(crop, ops, self.augment.fill)), labels


def _pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def jpeg_collate(samples):
    """Collate a list of (encoded file bytes, label) into
    (blob uint8 [n], descs int32 [B,16], qtabs int16 [B,3,64] (uint16 bits), sizes int32 [B,2] of (h, w), labels int64 [B]) --
    plain tensors, so pin_memory=True works -- for DeviceJpegLoader / kernels.jpeg_reconstruct_u8.  A stream vitres.jpeg.probe calls
    supported is Huffman-decoded straight into the blob (record kind 0: quantised coefficients, per component, 128 bytes a block).
    Every other file, and every stream whose entropy decode fails, is decoded by PIL's Image.open(...).convert('RGB') and stored as
    planar pixels (kind 1): the fallback is PIL's result by construction, PIL's exception for a file it cannot read included.  Every
    image starts on a multiple of 128 bytes, every component on a multiple of its block size (128 bytes, 64 for pixels)."""
    labels = _sample_labels(samples, "jpeg_collate")
    B = len(samples)
    files = [data if isinstance(data, (bytes, np.ndarray)) else bytes(data) for data, _ in samples]
    infos, raws, slots, total = [], [], [], 0
    for data in files:
        info = J.probe(data)
        raw = None if info["supported"] else _pil_rgb(data)
        H, W = (info["height"], info["width"]) if raw is None else raw.shape[:2]
        size = 3 * 64 * (-(-H // 8)) * (-(-W // 8))                        # as raw pixels (what a failed entropy decode falls back to)
        if raw is None:
            size = max(size, 128 * sum(info["blocks"]))
        size = -(-size // 128) * 128
        infos.append(info)
        raws.append(raw)
        slots.append((total, size))
        total += size
    blob = np.zeros(total, dtype=np.uint8)
    descs = K.jpeg_descs(B)
    qtabs = np.zeros((B, 3, 64), dtype=np.uint16)
    sizes = np.zeros((B, 2), dtype=np.int32)
    for b, (data, info, raw, (lo, size)) in enumerate(zip(files, infos, raws, slots)):
        d = descs[b]
        if raw is None:
            try:
                J.entropy_decode(data, coef=blob[lo:lo + size].view(np.int16), qtab=qtabs[b])
            except J.JpegError:
                blob[lo:lo + size] = 0
                qtabs[b] = 0
                raw = _pil_rgb(data)
        if raw is None:
            d["kind"], d["width"], d["height"], d["ncomp"] = K._lib.VR_JPEG_COEF, info["width"], info["height"], info["ncomp"]
            d["hs"], d["vs"] = info["hs"], info["vs"]
            off = lo
            for c in range(info["ncomp"]):
                d["off"][c], d["bw"][c], d["bh"][c] = off // K.JPEG_OFF_UNIT, info["bw"][c], info["bh"][c]
                off += 128 * info["blocks"][c]
        else:
            H, W = raw.shape[:2]
            bh, bw = -(-H // 8), -(-W // 8)
            d["kind"], d["width"], d["height"], d["ncomp"], d["hs"], d["vs"] = K._lib.VR_JPEG_RAW, W, H, 3, 1, 1
            planes = blob[lo:lo + 3 * 64 * bh * bw].reshape(3, bh * 8, bw * 8)
            planes[:, :H, :W] = raw.transpose(2, 0, 1)
            for c in range(3):
                d["off"][c], d["bw"][c], d["bh"][c] = (lo + c * 64 * bh * bw) // K.JPEG_OFF_UNIT, bw, bh
        sizes[b] = d["height"], d["width"]
    return (torch.from_numpy(blob), torch.from_numpy(descs.view(np.int32).reshape(B, K.JPEG_DESC_INTS)),
            torch.from_numpy(qtabs.view(np.int16)), torch.from_numpy(sizes), labels)


class DeviceJpegLoader(_LookAheadLoader):
    """Over a loader of jpeg_collate batches (DataLoader(..., collate_fn=jpeg_collate, pin_memory=True)): yields
    (canvas uint8 [B,3,Hs,Ws] on `device`, sizes [B,2] on the host, labels), the triple DeviceCropLoader takes from a pad_collate_u8
    loader -- the same bytes, made on the device by vr_jpeg_reconstruct_u8 from the coefficients the workers decoded.  Hs, Ws are the
    batch maxima rounded up to multiples of 4.  The blob, the record table and the quantisation tables are copied one batch ahead on
    a side stream (the DevicePrefetchLoader pattern); the records are checked against the blob and the canvas on the host copy when
    a batch is uploaded.  The canvases alternate between TWO buffers and the launches share one workspace, all kept and grown as
    batches need: a yielded canvas is valid until the batch after next is requested, which is what a consumer that launches on the
    current stream -- DeviceCropLoader -- needs.  ragged=True: a RaggedCanvas in the canvas's place (vr_jpeg_reconstruct_ragged_u8:
    every image in planes of its own size, kernels.ragged_layout of the batch's sizes) -- the same pixels in memory that follows
    the batch's pixels instead of B times its largest image; the two flat buffers alternate and grow in the same way.
    __len__, .sampler and .dataset are the wrapped loader's."""

    def __init__(self, loader, device, ragged=False):
        super().__init__(loader, device)
        self.ragged = bool(ragged)
        self._canvas, self._ws, self._turn = [None, None], None, 0

    def _stage(self, up, blob, descs, qtabs, sizes, labels):
        if blob.dtype != torch.uint8 or blob.dim() != 1 or descs.dtype != torch.int32 or descs.dim() != 2:
            raise TypeError("DeviceJpegLoader takes jpeg_collate batches (blob uint8 [n], descs int32 [B,16], ...)")
        Hs, Ws = ((int(v) + 3) // 4 * 4 for v in np.asarray(sizes).max(axis=0))
        K.check_jpeg_table(descs.numpy(), int(blob.numel()), Hs, Ws)
        planes = None
        if self.ragged:
            layout, nbytes = K.ragged_layout(np.asarray(sizes), 3)
            planes = (layout, nbytes, up.table(K.check_ragged_planes(layout, 3, nbytes, np.asarray(sizes), "DeviceJpegLoader")))
        return up(blob), up(descs), up(qtabs), sizes, labels, Hs, Ws, planes

    def _buffer(self, held, nbytes):
        if held is None or held.numel() < nbytes:
            held = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return held

    def _launch(self, blob, descs, qtabs, sizes, labels, Hs, Ws, planes):
        B = int(descs.shape[0])
        turn, self._turn = self._turn, self._turn ^ 1
        nbytes = B * 3 * Hs * Ws if planes is None else planes[1]
        self._canvas[turn] = self._buffer(self._canvas[turn], nbytes)
        self._ws = self._buffer(self._ws, K.jpeg_ws_bytes(blob.numel()))
        flat = self._canvas[turn][:nbytes]
        if planes is None:
            return K.jpeg_reconstruct_u8(blob, descs, qtabs, Hs, Ws, out=flat.view(B, 3, Hs, Ws), workspace=self._ws), sizes, labels
        layout, _, table = planes
        K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, table, dst=flat, workspace=self._ws, bounds=K.ragged_bounds(layout))
        return RaggedCanvas(flat, table, layout, 3), sizes, labels
