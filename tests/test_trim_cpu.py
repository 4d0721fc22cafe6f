"""No-GPU checks of the trim-to-ink and region ingest (txo_ingest_trim_views / txo_ingest_u8_view, ops.trim_view, ops.pack_u8(trim= /
regions=), TeXOCRWrapper trim='ink'): the rule in numpy against the brute-force restatement tests/trim_ref.py; the wrapper's host path
against the wrapper on the cropped image; the refusals of the two entry points, none of which needs a device; the host plan that stages a
repeated object once; the fake operators and the defaults.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import trim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS, MARGINS = (0, 1, 127, 254), (0, 1, 2, 50)


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _i32(rows):
    flat = [int(v) for r in rows for v in r]
    return (C.c_int32 * max(len(flat), 1))(*flat)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def _random_images():
    """small images of every channel count: sparse ink on white, values that straddle every level of LEVELS"""
    rng = np.random.RandomState(5)
    out = []
    for k in range(36):
        h, w, ch = int(rng.randint(1, 24)), int(rng.randint(1, 40)), (1, 3, 4)[k % 3]
        a = np.full((h, w, ch), 255, np.uint8)
        n = int(rng.randint(0, 6))
        a[rng.randint(0, h, n), rng.randint(0, w, n), rng.randint(0, ch, n)] = rng.choice([0, 1, 2, 127, 128, 254, 255], n)
        if k % 4 == 0:
            a = rng.randint(0, 256, (h, w, ch)).astype(np.uint8)
        out.append(a[..., 0] if ch == 1 and k % 2 else a)
    return out


def test_trim_view_equals_the_brute_force_rule_on_random_images():
    from texocr_amd import ops
    imgs = _random_images()
    assert {a.shape[2] if a.ndim == 3 else 1 for a in imgs} == {1, 3, 4}
    partial = 0
    for a in imgs:
        for level in LEVELS:
            for margin in MARGINS:
                want = trim_ref.view(a, level, margin)
                got = ops.trim_view(a, level, margin)
                assert got == want and all(isinstance(v, int) for v in got), (a.shape, level, margin, got, want)
                partial += want != (0, 0) + a.shape[:2]
    assert partial > 100                                          # the list really trims
    assert ops.trim_view(imgs[1]) == trim_ref.view(imgs[1], 127, 2)   # the defaults: level 127, margin 2


def test_trim_view_edge_cases():
    from texocr_amd import ops
    white = np.full((9, 11), 255, np.uint8)
    for level in LEVELS[:3]:
        a = white.copy()
        a[3, 4], a[6, 8] = level, level + 1                       # a byte equal to the level is ink, one above it is not
        assert ops.trim_view(a, level, 0) == trim_ref.view(a, level, 0) == (3, 4, 1, 1)
    a = white.copy()
    a[3, 4], a[6, 8] = 254, 255
    assert ops.trim_view(a, 254, 0) == trim_ref.view(a, 254, 0) == (3, 4, 1, 1)
    # ink in one channel only, each channel in turn: min over the read channels
    for c in range(3):
        a = np.full((8, 8, 3), 255, np.uint8)
        a[5, 2, c] = 100
        assert ops.trim_view(a, 127, 1) == trim_ref.view(a, 127, 1) == (4, 1, 3, 3)
    # RGBA: white RGB under alpha 0 is not ink; the alpha of a neighbour plays no part in a black pixel's being ink
    a = np.full((6, 7, 4), 255, np.uint8)
    a[..., 3] = 0
    assert ops.trim_view(a, 127, 2) == trim_ref.view(a, 127, 2) == (0, 0, 6, 7)
    a[2, 3, :3] = 0
    a[2, 4, 3] = 0                                                # (already 0: the neighbour's alpha alone)
    assert ops.trim_view(a, 127, 0) == trim_ref.view(a, 127, 0) == (2, 3, 1, 1)
    a[..., 3] = 255
    assert ops.trim_view(a, 127, 0) == (2, 3, 1, 1)
    # blank, all ink, 1x1
    assert ops.trim_view(white, 127, 2) == trim_ref.view(white, 127, 2) == (0, 0, 9, 11)
    black = np.zeros((9, 11, 3), np.uint8)
    for margin in MARGINS:
        assert ops.trim_view(black, 0, margin) == trim_ref.view(black, 0, margin) == (0, 0, 9, 11)
    for v, ch in ((0, 1), (255, 1), (127, 3), (128, 4)):
        one = np.full((1, 1, ch), v, np.uint8)
        assert ops.trim_view(one, 127, 50) == trim_ref.view(one, 127, 50) == (0, 0, 1, 1)
    # the margin clamps on every side on its own
    a = white.copy()
    a[1, 1] = a[7, 9] = 0
    assert ops.trim_view(a, 127, 2) == trim_ref.view(a, 127, 2) == (0, 0, 9, 11)
    assert ops.trim_view(a, 127, 1) == (0, 0, 9, 11) and ops.trim_view(a, 127, 0) == (1, 1, 7, 9)
    for bad in (dict(level=255), dict(level=-1), dict(margin=-1)):
        with pytest.raises(ValueError, match="ingest: the trim (level|margin) is"):
            ops.trim_view(a, **bad)


# ---- the wrapper's host path -----------------------------------------------------------------------------------------------------------------
def _stub_wrapper(monkeypatch, canvas=(32, 96)):
    """a TeXOCRWrapper with no engine behind it: only what _images reads (the canvas), and .cuda() is the identity"""
    from texocr_amd.config import Dims
    from texocr_amd.wrapper import TeXOCRWrapper
    w = TeXOCRWrapper.__new__(TeXOCRWrapper)
    w.dims = Dims(canvas=canvas[0], canvas_w=canvas[1], in_channels=1)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    return w


def _framed(h, w, box, mode, seed):
    """a PIL image (h, w) of white with random dark pixels inside box = (y0, x0, y1, x1), a light-grey rim around them"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    y0, x0, y1, x1 = box
    ch = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
    a = np.full((h, w, ch), 255, np.uint8)
    a[max(0, y0 - 1):y1 + 1, max(0, x0 - 1):x1 + 1, :3] = 200                  # lighter than the level: kept by the margin only
    a[y0:y1, x0:x1, :3] = rng.randint(0, 256, (y1 - y0, x1 - x0, min(ch, 3)))
    a[y0, x0, :3] = a[y1 - 1, x1 - 1, :3] = 0                                  # the ink box is exactly `box`
    return Image.fromarray(a[..., 0] if ch == 1 else a)


def test_host_path_trim_equals_the_wrapper_on_the_cropped_image(monkeypatch):
    from texocr_amd import ops
    from texocr_amd.wrapper import TeXOCRWrapper
    w = _stub_wrapper(monkeypatch)
    imgs = [_framed(40, 120, (10, 30, 25, 90), "RGB", 0), _framed(30, 50, (0, 0, 30, 50), "L", 1), _framed(200, 400, (80, 100, 106, 186), "RGBA", 2),
            _framed(90, 300, (5, 10, 80, 290), "RGB", 3), _framed(20, 20, (7, 7, 8, 8), "L", 4).convert("P")]
    for level, margin in ((127, 2), (127, 0), (10, 5)):
        rule = TeXOCRWrapper._trim_rule("ink", level, margin)
        views = [trim_ref.view(np.asarray(im if im.mode != "P" else im.convert("RGB")), level, margin) for im in imgs]
        assert views[0] == (10 - margin, 30 - margin, 15 + 2 * margin, 60 + 2 * margin) or level != 127
        crops = [im.crop((x0, y0, x0 + vw, y0 + vh)) for im, (y0, x0, vh, vw) in zip(imgs, views)]
        for fit in ("none", "canvas"):
            got = w._images(imgs, "host", fit, rule)
            want = w._images(crops, "host", fit)
            assert len(got) == len(want) == len(imgs)
            for g, r in zip(got, want):
                assert g.shape == r.shape and torch.equal(g, r)
        # image 2 (200 x 400) is beyond the 32 x 96 canvas; its ink is 26 x 86, and with the default margin the view fits: no fit is needed
        vh, vw = views[2][2:]
        assert (vh, vw) == (30, 90) or (level, margin) != (127, 2)
        assert tuple(w._images(imgs[2:3], "host", "none", rule)[0].shape) == (1, (vh + 15) // 16 * 16, (vw + 15) // 16 * 16)
    # an image whose view is the whole of it is handed on as the very object it was; trim='none' is today's path
    assert TeXOCRWrapper._trimmed(imgs[1], (127, 2)) is imgs[1]
    assert TeXOCRWrapper._trim_rule("none", 127, 2) is None
    assert tuple(w._images(imgs[:1], "host")[0].shape) == (1, 48, 128)
    with pytest.raises(ValueError, match="trim must be 'none' or 'ink'"):
        TeXOCRWrapper._trim_rule("tight", 127, 2)
    with pytest.raises(ValueError, match=r"ingest: the trim level is 255; it must lie in \[0, 254\]"):
        TeXOCRWrapper._trim_rule("ink", 255, 2)
    with pytest.raises(ValueError, match="ingest: the trim margin is -3; it must be >= 0"):
        TeXOCRWrapper._trim_rule("ink", 127, -3)
    assert ops.TRIM_LEVEL == 127 and ops.TRIM_MARGIN == 2


# ---- the refusals, none of which needs a device ----------------------------------------------------------------------------------------------
def test_trim_views_refusals_without_a_device(lib):
    from texocr_amd import _lib
    off = (C.c_int64 * 2)(0, 4096)
    out = (C.c_int32 * 8)()
    ok = _i32([(16, 16, 3), (47, 301, 1)])

    def call(shapes=ok, B=2, level=127, margin=2, offsets=off, views=out):
        rc = lib.txo_ingest_trim_views(None, None, offsets, shapes, B, level, margin, views, None)
        return rc, lib.txo_last_error().decode()
    for kw, frag in [
        (dict(level=255), "the trim level is 255; it must lie in [0, 254]"),
        (dict(level=-1), "the trim level is -1"),
        (dict(margin=-1), "the trim margin is -1; it must be >= 0"),
        (dict(shapes=_i32([(16, 16, 2), (47, 301, 1)])), "image 0 has ch = 2"),
        (dict(shapes=_i32([(16, 16, 3), (47, 0, 1)])), "image 1 is 47x0"),
        (dict(B=0), "no images"),
        (dict(shapes=None), "null shapes"),
        (dict(offsets=None), "null offsets"),
        (dict(offsets=(C.c_int64 * 2)(0, -1)), "image 1 has a negative byte offset"),
        (dict(), "null argument"),                                # a good call: only now does the missing engine matter
        (dict(level=0, margin=0), "null argument"),
        (dict(level=254, margin=2 ** 31 - 1), "null argument"),
    ]:
        rc, msg = call(**kw)
        assert rc == _lib.TXO_E_INVALID and frag in msg, (kw, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert list(out) == [0] * 8                                   # nothing is written on a refusal


def test_view_refusals_without_a_device(lib):
    """a view that is empty or reaches outside its image, then every refusal of txo_ingest_u8 / txo_ingest_u8_fit judged on the VIEW's size:
    TXO_E_INVALID with a message naming the image, before the engine or the device is looked at"""
    from texocr_amd import _lib
    off = (C.c_int64 * 2)(0, 4096)
    sizes = (C.c_int32 * 4)()
    shapes = _i32([(40, 60, 3), (100, 400, 1)])
    good = [(4, 5, 30, 50), (10, 20, 47, 301)]

    def call(views=good, shapes=shapes, B=2, C_=1, Fh=0, Fw=0, Hc=48, Wc=304, offsets=off, scratch=C.c_void_p(64), nbytes=1 << 20):
        v = None if views is None else _i32(views)
        rc = lib.txo_ingest_u8_view(None, None, offsets, shapes, v, B, C_, Fh, Fw, Hc, Wc, None, sizes, scratch, nbytes, None)
        return rc, lib.txo_last_error().decode()
    for kw, frag in [
        (dict(views=[(4, 5, 0, 50), good[1]]), "image 0 has the view 0x50 at (4, 5); both sides must be >= 1"),
        (dict(views=[good[0], (10, 20, 47, -1)]), "image 1 has the view 47x-1 at (10, 20); both sides must be >= 1"),
        (dict(views=[(-1, 5, 30, 50), good[1]]), "image 0 has the view 30x50 at (-1, 5), which reaches outside the image's 40x60"),
        (dict(views=[(4, 11, 30, 50), good[1]]), "image 0 has the view 30x50 at (4, 11), which reaches outside the image's 40x60"),
        (dict(views=[good[0], (54, 20, 47, 301)]), "image 1 has the view 47x301 at (54, 20), which reaches outside the image's 100x400"),
        (dict(views=[good[0], (0, -3, 47, 301)]), "reaches outside the image's 100x400"),
        (dict(views=None), "null views"),
        (dict(shapes=_i32([(40, 60, 2), (100, 400, 1)])), "image 0 has ch = 2"),
        (dict(shapes=_i32([(40, 60, 3), (0, 400, 1)])), "image 1 is 0x400"),
        (dict(B=0), "no images"),
        (dict(shapes=None), "null shapes"),
        (dict(offsets=None), "null offsets"),
        (dict(offsets=(C.c_int64 * 2)(0, -1)), "image 1 has a negative byte offset"),
        # txo_ingest_u8's, on the view: 47x301 rounds up to 48x304
        (dict(Wc=300), "image 1 is 47x301, 48x304 rounded up to multiples of 16: it does not fit the container's 48x300"),
        (dict(Hc=32), "image 1 is 47x301, 48x304 rounded up"),
        (dict(Wc=306), "multiple of 4"),
        (dict(C_=0), "channel count"),
        # txo_ingest_u8_fit's, on the view: 47x301 -> 14x96 under 32x96, 47 rows x 96 bytes of scratch
        (dict(Fh=32, Fw=100, Hc=32, Wc=96), "the fit target is 32x100; both sides must be positive multiples of 16"),
        (dict(Fh=32, Fw=0, Hc=32, Wc=96), "the fit target is 32x0"),
        (dict(Fh=32, Fw=96, Hc=32, Wc=80), "image 1 is 14x96, 16x96 rounded up to multiples of 16: it does not fit the container's 32x80"),
        (dict(Fh=32, Fw=96, Hc=32, Wc=96, nbytes=4511), "the fit scratch is 4511 bytes; the horizontal passes of this list need 4512 bytes"),
        (dict(Fh=32, Fw=96, Hc=32, Wc=96, scratch=None), "the fit scratch is null"),
        (dict(Fh=16, Fw=16, Hc=16, Wc=16, shapes=_i32([(40, 60, 3), (3, 4000, 1)]), views=[good[0], (0, 0, 3, 4000)]),
         "image 1 is 3x4000, 1x16 fitted to 16x16: an axis shrinks by more than 32 times"),
        (dict(), "null argument"),                                # good lists: only now does the missing engine matter
        (dict(Fh=32, Fw=96, Hc=32, Wc=96), "null argument"),
        (dict(views=[(0, 0, 40, 60), (0, 0, 100, 400)], Hc=112, Wc=400), "null argument"),
    ]:
        rc, msg = call(**kw)
        assert rc == _lib.TXO_E_INVALID and frag in msg, (kw, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert list(sizes) == [0, 0, 0, 0]                            # nothing is written on a refusal
    # the view's size is what counts: the full images (40x60, 100x400) would not fit this container, the views do
    rc, msg = call(views=[(0, 0, 16, 16), (50, 200, 16, 16)], Hc=16, Wc=16)
    assert rc == _lib.TXO_E_INVALID and "null argument" in msg


def test_symbols_header_and_readme(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name, nargs in (("txo_ingest_trim_views", 9), ("txo_ingest_u8_view", 16)):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and (name + "(") in hdr
        decl = hdr[hdr.index("int " + name + "("):]
        assert len(decl[:decl.index(");")].split(",")) == len(_lib.SYMBOLS[name][1]) == nargs
    assert "SYNCHRONOUS" in hdr[hdr.index("txo_ingest_trim_views  "):hdr.index("txo_ingest_u8_view  ")]
    assert f"({len(_lib.SYMBOLS)} entry points)" in open(os.path.join(ROOT, "README.md")).read()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------
def test_plan_stages_a_repeated_object_once():
    from PIL import Image
    from texocr_amd import ops
    rng = np.random.RandomState(0)
    page = rng.randint(0, 256, (50, 70, 3)).astype(np.uint8)
    other = rng.randint(0, 256, (9, 5)).astype(np.uint8)
    pil = Image.fromarray(page)
    for obj in (page, pil, torch.from_numpy(page)):
        staged, dev, src, shapes = ops.plan_u8([obj, other, obj, obj])
        assert dev == [] and staged.numel() == (page.size + 15) // 16 * 16 + (other.size + 15) // 16 * 16
        assert src.tolist() == [[0, 0], [0, (page.size + 15) // 16 * 16], [0, 0], [0, 0]]
        assert shapes.tolist() == [[50, 70, 3], [9, 5, 1], [50, 70, 3], [50, 70, 3]]
        assert np.array_equal(staged[:page.size].numpy(), page.reshape(-1))
    # equal pixels in two objects are two images: only an object that IS the same is shared
    staged, _, src, _ = ops.plan_u8([page, page.copy()])
    assert src.tolist() == [[0, 0], [0, (page.size + 15) // 16 * 16]] and staged.numel() == 2 * ((page.size + 15) // 16 * 16)
    # a list without repeats is planned as ever
    staged, _, src, _ = ops.plan_u8([other, page])
    assert src.tolist() == [[0, 0], [0, 48]] and staged.numel() == 48 + (page.size + 15) // 16 * 16


def test_pack_u8_refuses_trim_with_regions():
    from texocr_amd import ops
    with pytest.raises(ValueError, match="trim and regions"):
        ops.pack_u8([np.zeros((4, 4), np.uint8)], 1, "cpu", engine=0, trim=(127, 2), regions=[[0, 0, 2, 2]])


def test_fake_implementations_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    from texocr_amd.config import Dims

    class Stub:
        dims = Dims(canvas=64, in_channels=3)
    i = ops.register_engine(Stub())
    try:
        with FakeTensorMode():
            buf, src, shapes = torch.empty((100,), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int32)
            views = torch.ops.texocr.ingest_trim_views([buf], src, shapes, i, 127, 2)
            box, sizes = torch.ops.texocr.ingest_u8_view([buf], src, shapes, torch.zeros((2, 4), dtype=torch.int32), i, 3, 0, 0, 32, 48)
        assert tuple(views.shape) == (2, 4) and views.dtype == torch.int32 and views.device.type == "cpu"
        assert tuple(box.shape) == (2, 3, 32, 48) and box.dtype == torch.float32
        assert tuple(sizes.shape) == (2, 2) and sizes.dtype == torch.int32 and sizes.device.type == "cpu"
    finally:
        ops.unregister_engine(i)


def test_every_default_keeps_todays_behaviour():
    import inspect
    from texocr_amd import ops
    from texocr_amd.model import HipEngine, OCRModel
    from texocr_amd.wrapper import TeXOCRWrapper
    for fn in (TeXOCRWrapper.batch, TeXOCRWrapper.__call__):
        p = inspect.signature(fn).parameters
        assert (p["trim"].default, p["trim_level"].default, p["trim_margin"].default) == ("none", 127, 2)
    for fn in (OCRModel.ingest, HipEngine.ingest):
        p = inspect.signature(fn).parameters
        assert p["trim"].default is False and p["regions"].default is None
    p = inspect.signature(ops.pack_u8).parameters
    assert p["trim"].default is None and p["regions"].default is None
    assert inspect.signature(ops.trim_view).parameters["level"].default == 127 and inspect.signature(ops.trim_view).parameters["margin"].default == 2
    pk = ops.PackedImages(torch.zeros((1, 1, 16, 16)), torch.tensor([[16, 16]], dtype=torch.int32))       # existing constructions keep working
    assert pk.views is None and len(pk) == 1
