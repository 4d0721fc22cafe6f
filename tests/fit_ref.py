"""The reference of the fit-to-canvas ingest (texocr.h: txo_ingest_u8_fit; texocr_amd/csrc/ingest_fit.h): PIL's 8-bit BILINEAR resample
restated with Python integers and Python floats (IEEE doubles, one rounding per operation) only, plus the fit rule.  tests/golden/fit_cases.npz
pins it to PIL without PIL; the GPU tests compare the engine against it.  Holds no tests."""
import numpy as np

BITS = 22                # PIL's PRECISION_BITS for 8-bit channels
MAX_SCALE = 32           # in / out per axis the engine accepts
TAPS = 2 * MAX_SCALE + 1


def fit_size(h, w, Fh, Fw):
    """(h, w) -> the fitted (h', w') under the target (Fh, Fw): unchanged if it fits, else the binding side becomes the target's"""
    if h <= Fh and w <= Fw:
        return h, w
    if w * Fh <= h * Fw:
        return Fh, max(1, (w * Fh) // h)
    return max(1, (h * Fw) // w), Fw


def axis_coeffs(n_in, n_out):
    """one axis -> [(xmin, n, [K_0 .. K_{n-1}])] per output pixel"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        k = []
        for x in range(n):
            t = (x + xmin - center + 0.5) * ss
            t = -t if t < 0.0 else t
            k.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in k:
            ww = ww + v
        if ww != 0.0:
            k = [v / ww for v in k]
        out.append((xmin, n, [int(0.5 + v * 4194304.0) for v in k]))
    return out


def resample_axis(a, n_out, axis):
    """uint8 array -> uint8 array with `axis` resampled to n_out pixels: clamp((2^21 + sum K src) >> 22, 0, 255) in integers"""
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx, (xmin, n, K) in enumerate(axis_coeffs(src.shape[0], n_out)):
        acc = (1 << (BITS - 1)) + np.tensordot(np.asarray(K, np.int64), src[xmin:xmin + n], axes=(0, 0))
        assert int(acc.max()) < 2 ** 31                                  # the engine's accumulator is an int32
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(a, h2, w2):
    """(H, W) or (H, W, 3) uint8 -> (h2, w2[, 3]): horizontal pass first, then vertical; a pass whose axis keeps its size is skipped"""
    if w2 != a.shape[1]:
        a = resample_axis(a, w2, 1)
    if h2 != a.shape[0]:
        a = resample_axis(a, h2, 0)
    return np.ascontiguousarray(a)


def fit(a, Fh, Fw):
    """the channels the ingest reads ((H, W), (H, W, 3), or (H, W, 4) with the alpha dropped) fitted to (Fh, Fw); an image that fits is
    returned as it is, alpha and all"""
    h, w = a.shape[:2]
    fh, fw = fit_size(h, w, Fh, Fw)
    if (fh, fw) == (h, w):
        return a
    return resize(a[..., :3] if a.ndim == 3 else a, fh, fw)
