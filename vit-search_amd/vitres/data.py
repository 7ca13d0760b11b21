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

What is not here: decoding stays with the loader that produces the uint8 canvases.  ColorJitter is not implemented: timm skips it
whenever auto_augment is set, so no shipped recipe runs it.  Random
erasing, which timm applies to the normalised image, cannot happen there any more: `erase=` (a vitres.random_erasing.RandomErasing)
folds it into the normalising pass -- here with normalize=True, in the mix (`SwitchTokenMix(..., erase=)`, `Mixup(..., erase=)`) in training.
"""
import numpy as np
import torch

from . import kernels as K


class DevicePrefetchLoader:
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
        self.loader, self.device, self.normalize, self.erase = loader, torch.device(device), normalize, erase
        self.norm = K.norm_constants(mean, std)

    def __len__(self):
        return len(self.loader)

    @property
    def sampler(self):
        return self.loader.sampler

    @property
    def dataset(self):
        return self.loader.dataset

    def _upload(self, side, batch, target):
        if batch.dtype != torch.uint8:
            raise TypeError("DevicePrefetchLoader takes uint8 NCHW batches (timm's fast_collate), got %s" % batch.dtype)
        if side is None:                      # (not a GPU: nothing to overlap; the normaliser itself has no CPU form)
            return batch.to(self.device), target.to(self.device), None
        with torch.cuda.stream(side):
            return batch.to(self.device, non_blocking=True), target.to(self.device, non_blocking=True), side.record_event()

    def __iter__(self):
        side = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        ahead = None
        for batch, target in self.loader:
            nxt = self._upload(side, batch, target)
            if ahead is not None:
                yield self._hand_over(*ahead)
            ahead = nxt
        if ahead is not None:
            yield self._hand_over(*ahead)

    def _hand_over(self, u8, target, copied):
        if copied is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(copied)
            u8.record_stream(cur)             # (allocated on the side stream, used on this one)
            target.record_stream(cur)
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


def pad_collate_u8(samples):
    """Collate a list of (HWC uint8 array, label) -- decoded images of any sizes, one channel count -- into
    (canvas uint8 [B,C,Hs,Ws], sizes int32 [B,2] of (h, w), labels int64 [B]): every image sits in the top-left corner of its
    canvas plane, the rest is zero; Hs and Ws are the batch maxima rounded up to a multiple of 4 (vr_resample_u8 reads rows as
    dwords).  What a DataLoader(collate_fn=pad_collate_u8) hands to DeviceCropLoader."""
    if not samples:
        raise ValueError("pad_collate_u8: an empty batch")
    images = [np.asarray(img) for img, _ in samples]
    for img in images:
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != images[0].shape[2] or 0 in img.shape:
            raise TypeError("pad_collate_u8 takes non-empty HWC uint8 arrays of one channel count, got %s %s" % (img.dtype, img.shape))
    sizes = np.array([img.shape[:2] for img in images], dtype=np.int32)
    Hs, Ws = ((int(v) + 3) // 4 * 4 for v in sizes.max(axis=0))
    canvas = np.zeros((len(images), images[0].shape[2], Hs, Ws), dtype=np.uint8)
    for b, img in enumerate(images):
        canvas[b, :, :img.shape[0], :img.shape[1]] = img.transpose(2, 0, 1)
    labels = torch.as_tensor(np.asarray([int(label) for _, label in samples], dtype=np.int64))
    return torch.from_numpy(canvas), torch.from_numpy(sizes), labels


class DeviceCropLoader:
    """Over a loader of (canvas uint8 [B,C,Hs,Ws], sizes [B,2], labels) host batches (pad_collate_u8): yields
    (uint8 [B,C,S,S] on `device`, labels on `device`), the canvas cropped, resized and mirrored by vr_resample_u8 with the boxes
    `transform.draw(sizes)` makes (a vitres.resized_crop.RandomResizedCrop or ResizeCenterCrop: .draw, .size, .filter).  The canvas,
    the box table and the labels are copied one batch ahead on a side stream (the DevicePrefetchLoader pattern; pinned host batches
    make the copies asynchronous); the boxes are drawn, and checked against the canvas, in the loader's order when a batch is
    uploaded.  The output is what DevicePrefetchLoader, SwitchTokenMix(input_norm=), Mixup(input_norm=) and ResidentU8Batches take;
    nothing is normalised here.  augment=RandAugment(...) (vitres.rand_augment: .draw(B), .fill, .size): the batch's op table is drawn
    after its boxes, copied with them, and vr_rand_augment_u8 runs on the cropped batch (3 channels); augment=None adds nothing.
    __len__, .sampler and .dataset are the wrapped loader's."""

    def __init__(self, loader, transform, device, augment=None):
        self.loader, self.transform, self.device, self.augment = loader, transform, torch.device(device), augment
        if augment is not None:
            size = (transform.size, transform.size) if isinstance(transform.size, int) else tuple(transform.size)
            if tuple(augment.size) != size:
                raise ValueError("DeviceCropLoader: the augmentation draws for %s images, the transform makes %s" % (augment.size, size))

    def __len__(self):
        return len(self.loader)

    @property
    def sampler(self):
        return self.loader.sampler

    @property
    def dataset(self):
        return self.loader.dataset

    def _upload(self, side, canvas, sizes, labels):
        if canvas.dtype != torch.uint8 or canvas.dim() != 4:
            raise TypeError("DeviceCropLoader takes uint8 [B,C,Hs,Ws] canvases (pad_collate_u8), got %s %s" % (canvas.dtype,
                                                                                                              tuple(canvas.shape)))
        B, _, Hs, Ws = canvas.shape
        sizes = np.asarray(sizes, dtype=np.int64)
        if sizes.shape != (B, 2) or (sizes[:, 0] > Hs).any() or (sizes[:, 1] > Ws).any():
            raise ValueError("DeviceCropLoader: sizes must hold one (h, w) inside the %d x %d canvas per sample" % (Hs, Ws))
        table = K.check_resample_boxes(self.transform.draw(sizes), B, Hs, Ws, self.transform.size)
        host = torch.empty(table.shape, dtype=torch.int32, pin_memory=side is not None)
        host.numpy()[...] = table
        ops = None
        if self.augment is not None:
            ra = K.check_ra_table(self.augment.draw(B), B)
            ops = torch.empty(ra.shape, dtype=torch.int32, pin_memory=side is not None)
            ops.numpy()[...] = ra
        if side is None:                      # (not a GPU: nothing to overlap; the kernel itself has no CPU form)
            return (canvas.to(self.device), host.to(self.device), labels.to(self.device), None,
                    None if ops is None else ops.to(self.device))
        with torch.cuda.stream(side):
            canvas, host, labels = (t.to(self.device, non_blocking=True) for t in (canvas, host, labels))
            ops = None if ops is None else ops.to(self.device, non_blocking=True)
            return canvas, host, labels, side.record_event(), ops

    def __iter__(self):
        side = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        ahead = None
        for canvas, sizes, labels in self.loader:
            nxt = self._upload(side, canvas, sizes, labels)
            if ahead is not None:
                yield self._hand_over(*ahead)
            ahead = nxt
        if ahead is not None:
            yield self._hand_over(*ahead)

    def _hand_over(self, canvas, table, labels, copied, ops=None):
        if copied is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(copied)
            for t in (canvas, table, labels) + (() if ops is None else (ops,)):  # (allocated on the side stream, used on this one)
                t.record_stream(cur)
        crop = K.resample_u8(canvas, table, self.transform.size, self.transform.filter)
        if ops is None:
            return crop, labels
        return K.rand_augment_u8(crop, ops, self.augment.fill), labels
