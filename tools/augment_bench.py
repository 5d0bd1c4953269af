"""Training augmentation at the flagship batch (8 x 3 x 512 x 512 fp32 images, int64 masks), one process, one GPU:

  RandomFlipRotate (images + masks, one launch) us | torch.clone of the same two tensors (the bandwidth yardstick) us |
  the added cost of ImagePreprocessor.preprocess with augmentation over preprocess without it, per 1080p image at 512^2.

Times are HIP events.  The batch call includes its host work (draws, coefficient table, its host-to-device copy); `kernel_us` times
the kernel alone by replaying one launch through the C ABI.  Prints one JSON line per measurement.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/augment_bench.py` for the per-kernel times (profiles/augment_kernel_stats.csv)."""
import ctypes as C

from benchkit import emit, timed  # first: benchkit sets the import path
import numpy as np
import torch

import mgunet
from mgunet import _lib
from mgunet.gat import _context

WARMUP = 5

def main():
    dev = torch.device("cuda:0")
    B, Cc, H, W = 8, 3, 512, 512
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, Cc, H, W), generator=g).to(dev)
    y = torch.randint(0, 2, (B, H, W), generator=g).to(dev)
    mbytes = (x.numel() * 4 + y.numel() * 8) * 2 / 1e6
    aug = mgunet.RandomFlipRotate(mask_fill=-100)
    call = timed(lambda: aug(x, y, generator=g), 50, WARMUP, park=False)
    # the kernel alone: one fixed table, launched through the ABI with preallocated outputs
    params = aug.draw(B, W, H, g).to(dev)
    ox, oy = torch.empty_like(x), torch.empty_like(y)
    si, so = (C.c_int64 * 4)(*x.stride()), (C.c_int64 * 4)(*ox.stride())
    fill = (C.c_float * Cc)(*aug.fill)
    ctx = _context(dev)
    L, stream = _lib.lib(), _lib.current_stream_ptr(dev)

    def launch():
        _lib.check(L.mgu_augment_flip_rotate(ctx.handle, x.data_ptr(), ox.data_ptr(), B, Cc, H, W, si, so, fill, y.data_ptr(), oy.data_ptr(),
                                             -100, params.data_ptr(), stream), ctx.handle)

    kern = timed(launch, 200, WARMUP)
    clone = timed(lambda: (x.clone(), y.clone()), 200, WARMUP)
    emit(what="augment_batch", shape=[B, Cc, H, W], masks="int64", call_us=round(call * 1e3, 2), kernel_us=round(kern * 1e3, 2),
         clone_us=round(clone * 1e3, 2), kernel_over_clone=round(kern / clone, 3), moved_MB=round(mbytes, 1),
         kernel_TBps=round(mbytes / 1e6 / (kern * 1e-3), 2), clone_TBps=round(mbytes / 1e6 / (clone * 1e-3), 2))
    # preprocess of one 1080p BGR image at 512^2, with and without the fused augmentation (same launches)
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev)
    plain = mgunet.ImagePreprocessor(resize_dim=(H, W))
    augp = mgunet.ImagePreprocessor(resize_dim=(H, W), apply_augmentation=True)
    out = torch.empty((3, H, W), device=dev)
    t0 = timed(lambda: plain.preprocess(img, out=out), 50, WARMUP, park=False)
    t1 = timed(lambda: augp.preprocess(img, out=out), 50, WARMUP, park=False)
    emit(what="preprocess_1080p_to_512", plain_us=round(t0 * 1e3, 2), augmented_us=round(t1 * 1e3, 2), added_us=round((t1 - t0) * 1e3, 2))


if __name__ == "__main__":
    main()
