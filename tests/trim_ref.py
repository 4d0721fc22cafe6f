"""The trim rule of texocr.h "Trim-to-ink ingest", restated by brute force for the tests (tests/test_trim_cpu.py,
tests/test_gpu_ingest_trim.py): per-pixel Python loops over plain integers, no numpy reductions, nothing shared with ops.trim_view or
the kernel.  Holds no tests."""


def view(a, level=127, margin=2):
    """a: uint8 array (H, W) or (H, W, ch), ch in {1, 3, 4} -> (y0, x0, h', w').  A pixel is ink iff min(read channels) <= level (L as it is;
    R, G, B of RGB / RGBA; the alpha is never read).  The ink box grows by `margin` on every side and is clamped to the image; an image
    without ink keeps (0, 0, H, W)."""
    assert 0 <= level <= 254 and margin >= 0
    rows = a.tolist()
    h, w = len(rows), len(rows[0])
    ymin = xmin = ymax = xmax = None
    for y in range(h):
        for x in range(w):
            px = rows[y][x]
            read = [px] if isinstance(px, int) else px[:3]
            if min(read) <= level:
                ymin = y if ymin is None else min(ymin, y)
                ymax = y if ymax is None else max(ymax, y)
                xmin = x if xmin is None else min(xmin, x)
                xmax = x if xmax is None else max(xmax, x)
    if ymin is None:
        return 0, 0, h, w
    y0, y1 = max(0, ymin - margin), min(h, ymax + 1 + margin)
    x0, x1 = max(0, xmin - margin), min(w, xmax + 1 + margin)
    return y0, x0, y1 - y0, x1 - x0


def crop(a, v):
    """the contiguous copy a[y0:y0 + h, x0:x0 + w] of the view v"""
    import numpy as np
    y0, x0, h, w = v
    return np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
