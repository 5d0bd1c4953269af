"""Writes tests/golden/augment.npz: PIL's own output for the training augmentation of ImagePreprocessor(apply_augmentation=True)
(preprocessing/image_preprocessing/image_preprocess.py:44-51: Resize -> RandomHorizontalFlip -> RandomRotation, NEAREST, fill 0), on
the cases tests/test_augment_host.py and tests/test_gpu_augment.py pin the HIP path to.

    python tools/make_augment_golden.py

Dev-box tool (needs numpy and PIL, not the reference); nothing on the GPU side runs it.  Case k holds:
  k_src  (Hs, Ws, 3) uint8 RGB source          k_dst   (H, W) resize target        k_flip, k_angle  the draw
  k_img  (H, W, 3) uint8: PIL resize((W, H), BILINEAR) -> transpose(FLIP_LEFT_RIGHT) if flip -> rotate(angle, NEAREST, fillcolor=(0,0,0))
  k_msrc (Hs, Ws) uint8 label map              k_mask  (H, W) uint8: L-mode rotation (fill 0) of the flipped, nearest-resized k_msrc
  k_inb  (H, W) uint8: the same rotation of an all-255 image -- 255 where a pixel comes from inside the image
The nearest resize is cv2.resize(INTER_NEAREST) as preprocess_mask uses it: source index min(floor(dst * (1 / (dst / src))), src - 1)."""
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "augment.npz")

#        source      target     flip  angle
CASES = [((37, 53), (32, 48), 0, 0.0),
         ((37, 53), (32, 48), 1, 0.0),            # flip alone
         ((70, 93), (64, 64), 0, 15.0),
         ((70, 93), (64, 64), 1, -15.0),
         ((64, 64), (64, 64), 1, 15.0),           # no resize
         ((33, 100), (45, 31), 0, -7.5),          # odd, H != W
         ((50, 40), (17, 23), 1, 11.25),
         ((72, 54), (54, 72), 0, -3.14159),
         ((41, 41), (40, 40), 1, 1e-9),
         ((90, 60), (60, 90), 0, -14.999)]


def nearest(m, H, W):
    Hs, Ws = m.shape
    ify, ifx = 1.0 / (H / Hs), 1.0 / (W / Ws)
    sy = np.minimum(np.floor(np.arange(H) * ify).astype(np.int64), Hs - 1)
    sx = np.minimum(np.floor(np.arange(W) * ifx).astype(np.int64), Ws - 1)
    return np.ascontiguousarray(m[sy][:, sx])


def augment(pil, flip, angle, fill):
    if flip:
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(pil.rotate(angle, Image.NEAREST, expand=False, center=None, fillcolor=fill))


def main():
    rng = np.random.default_rng(31)
    rng_angles = [float(a) for a in rng.uniform(-15, 15, 4)]
    cases = CASES + [((60, 80), (48, 64), i & 1, a) for i, a in enumerate(rng_angles)]
    out = {"ncases": np.int64(len(cases))}
    for k, (src, dst, flip, angle) in enumerate(cases):
        H, W = dst
        img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
        msrc = rng.integers(0, 6, src, dtype=np.uint8)
        resized = Image.fromarray(img).resize((W, H), Image.BILINEAR)
        out[f"{k}_src"], out[f"{k}_dst"] = img, np.array(dst, np.int64)
        out[f"{k}_flip"], out[f"{k}_angle"] = np.int64(flip), np.float64(angle)
        out[f"{k}_img"] = augment(resized, flip, angle, (0, 0, 0))
        out[f"{k}_msrc"] = msrc
        out[f"{k}_mask"] = augment(Image.fromarray(nearest(msrc, H, W), "L"), flip, angle, 0)
        out[f"{k}_inb"] = augment(Image.new("L", (W, H), 255), flip, angle, 0)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(cases), "cases")


if __name__ == "__main__":
    main()
