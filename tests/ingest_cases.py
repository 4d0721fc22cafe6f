"""The image lists the ingest tests share (tests/test_ingest_cpu.py, tests/test_gpu_ingest.py): raw uint8 images as PIL, and a float32
restatement of the kernel's step sequence (texocr_amd/csrc/ingest.h).  Holds no tests."""
import numpy as np

# (height, width): 1x1; a whole patch; one short of it in height; past it in both; row bytes that are no multiple of 4; two blocks of rows
MIXED_SIZES = [(1, 1), (16, 16), (15, 16), (17, 33), (32, 100), (48, 160)]
MODES = ["L", "RGB", "RGBA"]


def mixed_list(seed=3):
    """one list that mixes L, RGB and RGBA over MIXED_SIZES (every size in every mode), random pixels"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for k, (h, w) in enumerate(MIXED_SIZES * 3):
        mode = MODES[(k + k // len(MIXED_SIZES)) % 3]
        ch = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
        a = rng.randint(0, 256, (h, w, ch)).astype(np.uint8)
        out.append(Image.fromarray(a[..., 0] if ch == 1 else a))
    return out


def sweep_list():
    """three 256x256 RGB images whose pixels are (row, col, (7 row + 13 col) mod 256), the channels rotated between images: every value
    of every channel meets every value of another"""
    from PIL import Image
    r, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    base = np.stack([r, c, (7 * r + 13 * c) % 256], axis=-1).astype(np.uint8)
    return [Image.fromarray(np.ascontiguousarray(np.roll(base, k, axis=-1))) for k in range(3)]


def flat_list():
    """an all-0 and an all-255 image in every mode, sizes that need a pad"""
    from PIL import Image
    out = []
    for v in (0, 255):
        out.append(Image.fromarray(np.full((20, 37), v, np.uint8)))
        out.append(Image.fromarray(np.full((5, 50, 3), v, np.uint8)))
        out.append(Image.fromarray(np.full((33, 18, 4), v, np.uint8)))
    return out


def kernel_steps(a: np.ndarray) -> np.ndarray:
    """(H, W) or (H, W, ch) uint8 -> (H, W) float32 by the kernel's own sequence, every step a separately rounded float32 operation:
    a_c = float(c) / 255.0f;  s = (0.2989f a_r + 0.587f a_g) + 0.114f a_b;  out = 1.0f - s;  ch == 1: r = g = b; alpha is not read"""
    f = np.float32
    if a.ndim == 2:
        a = a[..., None]
    unit = (np.arange(256, dtype=np.float32) / f(255.0)).astype(np.float32)
    ar = unit[a[..., 0]]
    ag = ar if a.shape[2] == 1 else unit[a[..., 1]]
    ab = ar if a.shape[2] == 1 else unit[a[..., 2]]
    pr = (f(0.2989) * ar).astype(np.float32)
    pg = (f(0.587) * ag).astype(np.float32)
    pb = (f(0.114) * ab).astype(np.float32)
    s = ((pr + pg).astype(np.float32) + pb).astype(np.float32)
    return (f(1.0) - s).astype(np.float32)
