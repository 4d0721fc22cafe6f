"""No-GPU checks of the fit-to-canvas ingest (txo_ingest_u8_fit / texocr::ingest_u8_fit / ops.pack_u8(fit=) / TeXOCRWrapper fit='canvas'):
the reference tests/fit_ref.py against PIL's recorded bytes (tests/golden/fit_cases.npz) and against PIL itself where it imports; the fit
rule and the coefficient table of the library -- the very function the kernels run -- against fit_ref; the refusals that need no device;
the fake operator; and the wrapper's host path, which calls PIL for oversized images only."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import fit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def fixture_cases():
    z = np.load(os.path.join(GOLDEN, "fit_cases.npz"))
    return z, json.load(open(os.path.join(GOLDEN, "fit_cases.json")))["cases"]


def _i32(rows):
    flat = [int(v) for r in rows for v in r]
    return (C.c_int32 * max(len(flat), 1))(*flat)


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def test_fit_ref_reproduces_every_fixture_case(fixture_cases):
    z, cases = fixture_cases
    assert len(cases) >= 16 and {c["mode"] for c in cases} == {"L", "RGB", "RGBA"}
    oversized = 0
    for c in cases:
        a = z["src_" + c["name"]]
        assert a.dtype == np.uint8 and a.shape[:2] == (c["h"], c["w"])
        assert fit_ref.fit_size(c["h"], c["w"], c["Fh"], c["Fw"]) == (c["fh"], c["fw"]), c["name"]
        got = fit_ref.fit(a, c["Fh"], c["Fw"])
        if (c["fh"], c["fw"]) == (c["h"], c["w"]):
            assert got is a and "out_" + c["name"] not in z.files, c["name"]          # an image that fits is not touched
            continue
        oversized += 1
        ref = z["out_" + c["name"]]
        assert got.dtype == np.uint8 and got.shape == ref.shape and got.shape[:2] == (c["fh"], c["fw"]), c["name"]
        assert np.array_equal(got, ref), (c["name"], int((got != ref).sum()))
    assert oversized >= 12
    for name in ("white_64x512", "white_rgb_40x130"):                                  # the clamp: all-255 stays exactly 255
        assert int(z["out_" + name].min()) == 255 and int(fit_ref.fit(z["src_" + name], 16, 16).min()) == 255


def test_fit_ref_equals_pil_on_random_shapes():
    """about 100 seeded shapes in L, RGB and RGBA-as-RGB under small targets; the only test here that needs PIL (the fixture duplicates it)"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    n = 0
    while n < 100:
        Fh, Fw = [(32, 96), (16, 16), (48, 32)][n % 3]
        h, w = int(rng.integers(1, 8 * Fh)), int(rng.integers(1, 8 * Fw))
        fh, fw = fit_ref.fit_size(h, w, Fh, Fw)
        if (fh, fw) == (h, w) or h > 32 * fh or w > 32 * fw:
            continue
        ch = (1, 3, 4)[n % 3]
        a = rng.integers(0, 256, (h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
        if n % 4 == 0:
            a = (rng.integers(0, 2, a.shape) * 255).astype(np.uint8)
        img = Image.fromarray(a)
        ref = np.asarray((img if ch == 1 else img.convert("RGB")).resize((fw, fh), Image.BILINEAR))
        assert np.array_equal(fit_ref.fit(a, Fh, Fw), ref), (h, w, ch, Fh, Fw)
        n += 1


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
RULE_CASES = [  # (h, w, Fh, Fw): fits; exact ties w * Fh == h * Fw; one pixel over on either side; the clamps to 1; a 64-bit product
    (1, 1, 32, 96), (32, 96, 32, 96), (20, 50, 32, 96), (64, 192, 32, 96), (320, 960, 32, 96), (33, 99, 32, 96),
    (33, 96, 32, 96), (32, 97, 32, 96), (33, 97, 32, 96), (31, 97, 32, 96), (33, 95, 32, 96),
    (300, 1, 32, 96), (1, 400, 32, 96), (2, 3000, 32, 96), (1000, 3, 32, 96), (160, 1009, 160, 1008), (161, 1008, 160, 1008),
    (5120, 32256, 160, 1008), (100000, 70000, 160, 1008), (2000000000, 2000000000, 672, 672),
]


def test_fit_size_equals_txo_ingest_fit(lib):
    from texocr_amd import ops
    for h, w, Fh, Fw in RULE_CASES:
        want = fit_ref.fit_size(h, w, Fh, Fw)
        assert ops.fit_size(h, w, Fh, Fw) == want, (h, w)
        assert want[0] <= Fh and want[1] <= Fw and min(want) >= 1
        out = (C.c_int32 * 2)()
        rc = lib.txo_ingest_fit(_i32([(h, w, 1)]), 1, Fh, Fw, out)
        if h > 32 * want[0] or w > 32 * want[1]:
            assert rc == -1 and "image 0 is %dx%d" % (h, w) in lib.txo_last_error().decode() and list(out) == [0, 0]
        else:
            assert rc == 0 and tuple(out) == want, (h, w, tuple(out), want)
    assert ops.fit_size(33, 99, 32, 96) == (32, 96) and ops.fit_size(300, 1, 32, 96) == (32, 1) and ops.fit_size(2, 3000, 32, 96) == (1, 96)
    # a whole list in one call; an image that fits is unchanged
    shapes = [(20, 50, 3), (47, 301, 3), (70, 500, 4), (1024, 3072, 1)]
    out = (C.c_int32 * 8)()
    assert lib.txo_ingest_fit(_i32(shapes), 4, 32, 96, out) == 0
    assert list(out) == [20, 50, 14, 96, 13, 96, 32, 96]
    assert tuple(ops.fit_shapes(torch.tensor(shapes, dtype=torch.int32), 32, 96).reshape(-1).tolist()) == (20, 50, 3, 14, 96, 3, 13, 96, 4, 32, 96, 1)


# ---- the coefficient table: the function the kernels run, on the host ----------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [
    (192, 96), (96, 32), (3072, 96), (1024, 32),             # integer scales 2, 3, 32
    (97, 96), (1009, 1008), (33, 32), (301, 96), (500, 96),   # just above 1; odd ratios
    (2, 1), (7, 1), (32, 1), (1, 1),                          # out = 1
    (32256, 1008), (5120, 160),                               # the largest legal in for the default canvas
    (96, 96), (5, 9),                                         # scale 1 and an upscale: the filter is not widened
])
def test_fit_coeffs_equal_fit_ref(lib, n_in, n_out):
    from texocr_amd import _lib
    T = _lib.TXO_FIT_TAPS
    xmin, n, K = (C.c_int32 * n_out)(), (C.c_int32 * n_out)(), (C.c_int32 * (n_out * T))()
    assert lib.txo_ingest_fit_coeffs(n_in, n_out, xmin, n, K) == 0, lib.txo_last_error().decode()
    ref = fit_ref.axis_coeffs(n_in, n_out)
    K = np.frombuffer(K, dtype=np.int32).reshape(n_out, T)
    assert T == fit_ref.TAPS == 65 and max(r[1] for r in ref) <= T
    for xx, (rx, rn, rk) in enumerate(ref):
        assert (xmin[xx], n[xx]) == (rx, rn) and rx >= 0 and rx + rn <= n_in, xx       # the window lies inside the source
        assert K[xx, :rn].tolist() == rk and not K[xx, rn:].any(), xx
        assert abs(int(K[xx].sum()) - (1 << 22)) <= rn and min(rk) >= 0, xx


def test_fit_coeffs_refusals(lib):
    a = (C.c_int32 * 65)()
    for n_in, n_out, frag in [(33, 1, "33 -> 1: the axis shrinks by more than 32 times"), (32257, 1008, "32257 -> 1008"), (0, 4, "in >= 1"), (4, 0, "out >= 1")]:
        assert lib.txo_ingest_fit_coeffs(n_in, n_out, a, a, a) == -1 and frag in lib.txo_last_error().decode()
    assert lib.txo_ingest_fit_coeffs(4, 1, None, a, a) == -1 and "null argument" in lib.txo_last_error().decode()


# ---- the refusals, none of which needs a device ----------------------------------------------------------------------------------------------
def test_scratch_bytes(lib):
    need = C.c_int64(-1)
    assert lib.txo_ingest_fit_scratch(_i32([(1, 1, 1), (32, 96, 3), (20, 50, 4)]), 3, 32, 96, C.byref(need)) == 0 and need.value == 0
    # 47x301 RGB -> 47 rows of 96 fitted columns of 3 bytes; 70x500 RGBA keeps 3 channels; 300x1 keeps its width: no intermediate
    shapes = [(47, 301, 3), (70, 500, 4), (300, 1, 3), (1, 400, 1)]
    want = sum((h * fw * c + 15) // 16 * 16 for h, fw, c in [(47, 96, 3), (70, 96, 3), (1, 96, 1)])
    assert lib.txo_ingest_fit_scratch(_i32(shapes), 4, 32, 96, C.byref(need)) == 0 and need.value == want
    # one pixel too high: the width follows (32x93), so there is an intermediate of 33 rows
    assert lib.txo_ingest_fit_scratch(_i32([(33, 96, 1)]), 1, 32, 96, C.byref(need)) == 0 and need.value == (33 * 93 + 15) // 16 * 16
    assert lib.txo_ingest_fit_scratch(_i32([(33, 96, 1)]), 1, 32, 96, None) == -1


def test_fit_refusals_without_a_device(lib):
    """as with txo_ingest_u8: everything about the list, the target, the container and the scratch is refused with TXO_E_INVALID and a
    message naming the image before the engine or the device is looked at"""
    from texocr_amd import _lib
    off = (C.c_int64 * 2)(0, 4096)
    sizes = (C.c_int32 * 4)()
    ok = _i32([(16, 16, 3), (47, 301, 3)])                         # the second one is oversized: 14x96 fitted, 13536 bytes of scratch

    def call(shapes=ok, B=2, C_=1, Fh=32, Fw=96, Hc=32, Wc=96, offsets=off, scratch=C.c_void_p(64), nbytes=1 << 20):
        rc = lib.txo_ingest_u8_fit(None, None, offsets, shapes, B, C_, Fh, Fw, Hc, Wc, None, sizes, scratch, nbytes, None)
        return rc, lib.txo_last_error().decode()
    for kw, frag in [
        (dict(shapes=_i32([(16, 16, 3), (3, 100000, 1)])), "image 1 is 3x100000, 1x96 fitted to 32x96: an axis shrinks by more than 32 times"),
        (dict(shapes=_i32([(1025, 3072, 1), (16, 16, 1)])), "image 0 is 1025x3072, 32x95 fitted to 32x96: an axis shrinks by more than 32 times"),
        (dict(Fh=0), "the fit target is 0x96; both sides must be positive multiples of 16"),
        (dict(Fh=-16), "the fit target is -16x96"),
        (dict(Fw=100), "the fit target is 32x100; both sides must be positive multiples of 16"),
        (dict(Fh=24), "the fit target is 24x96"),
        (dict(nbytes=13535), "the fit scratch is 13535 bytes; the horizontal passes of this list need 13536 bytes"),
        (dict(scratch=None), "the fit scratch is null; the horizontal passes of this list need 13536 bytes"),
        (dict(shapes=_i32([(16, 16, 2), (47, 301, 3)])), "image 0 has ch = 2"),
        (dict(shapes=_i32([(16, 16, 3), (0, 301, 3)])), "image 1 is 0x301"),
        (dict(B=0), "no images"),
        (dict(shapes=None), "null shapes"),
        (dict(offsets=None), "null offsets"),
        (dict(offsets=(C.c_int64 * 2)(0, -1)), "image 1 has a negative byte offset"),
        (dict(Hc=16, Wc=96, shapes=_i32([(17, 16, 3), (47, 301, 3)])), "image 0 is 17x16, 32x16 rounded up"),
        (dict(Wc=80), "image 1 is 14x96, 16x96 rounded up to multiples of 16: it does not fit the container's 32x80"),   # (the FITTED size)
        (dict(Wc=98), "multiple of 4"),
        (dict(C_=0), "channel count"),
        (dict(), "null argument"),                                # a good list: only now does the missing engine matter
    ]:
        rc, msg = call(**kw)
        assert rc == _lib.TXO_E_INVALID and frag in msg, (kw, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    # with nothing oversized no scratch is asked for: the call gets as far as the missing engine
    rc, msg = call(shapes=_i32([(16, 16, 3), (32, 96, 1)]), scratch=None, nbytes=0)
    assert rc == _lib.TXO_E_INVALID and "null argument" in msg
    assert list(sizes) == [0, 0, 0, 0]                            # nothing is written on a refusal


def test_symbols_header_and_readme(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name in ("txo_ingest_fit", "txo_ingest_fit_scratch", "txo_ingest_fit_coeffs", "txo_ingest_u8_fit"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and (name + "(") in hdr
    assert "#define TXO_FIT_TAPS %d" % _lib.TXO_FIT_TAPS in hdr
    assert f"({len(_lib.SYMBOLS)} entry points)" in open(os.path.join(ROOT, "README.md")).read()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------
def test_fake_implementation_gives_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    from texocr_amd.config import Dims

    class Stub:
        dims = Dims(canvas=64, in_channels=3)
    stub = Stub()
    i = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            box, sizes = torch.ops.texocr.ingest_u8_fit([torch.empty((100,), dtype=torch.uint8)], torch.zeros((2, 2), dtype=torch.int64),
                                                        torch.zeros((2, 3), dtype=torch.int32), i, 3, 32, 96, 32, 48)
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
        assert inspect.signature(fn).parameters["fit"].default == "none"
    for fn in (OCRModel.ingest, HipEngine.ingest):
        assert inspect.signature(fn).parameters["fit"].default is False
    assert inspect.signature(ops.pack_u8).parameters["fit"].default is None


def _stub_wrapper(monkeypatch, canvas=(32, 96)):
    """a TeXOCRWrapper with no engine behind it: only what _images / _fitted read (the canvas), and .cuda() is the identity"""
    from texocr_amd.config import Dims
    from texocr_amd.wrapper import TeXOCRWrapper
    w = TeXOCRWrapper.__new__(TeXOCRWrapper)
    w.dims = Dims(canvas=canvas[0], canvas_w=canvas[1], in_channels=1)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    return w


def test_host_path_fit_calls_pil_only_for_oversized_images(monkeypatch, fixture_cases):
    from PIL import Image                                          # (the wrapper's host path IS a call into PIL: no skip)
    from texocr_amd.wrapper import preprocess_image
    z, cases = fixture_cases
    w = _stub_wrapper(monkeypatch)
    calls = []
    real = Image.Image.resize

    def spy(self, size, resample=None, *a, **k):
        calls.append((self.size, self.mode, size, resample))
        return real(self, size, resample, *a, **k)
    monkeypatch.setattr(Image.Image, "resize", spy)
    batch = [c for c in cases if (c["Fh"], c["Fw"]) == (32, 96) and c["name"] != "over_1024x3072"]
    imgs = [Image.fromarray(z["src_" + c["name"]]) for c in batch]
    out = w._images(imgs, "host", "canvas")
    over = [c for c in batch if (c["fh"], c["fw"]) != (c["h"], c["w"])]
    assert len(calls) == len(over) == 8 and len(batch) - len(over) == 4
    for (size, mode, target, resample), c in zip(calls, over):
        assert size == (c["w"], c["h"]) and target == (c["fw"], c["fh"]) and resample == Image.BILINEAR
        assert mode == ("L" if c["mode"] == "L" else "RGB"), c["name"]                 # RGBA went through convert('RGB') first
    for x, c, im in zip(out, batch, imgs):
        fitted = fit_ref.fit(z["src_" + c["name"]], 32, 96)
        assert tuple(x.shape) == (1, (c["fh"] + 15) // 16 * 16, (c["fw"] + 15) // 16 * 16), c["name"]
        assert torch.equal(x, preprocess_image(Image.fromarray(fitted))), c["name"]
    # an image that fits is handed on as the very object it was
    assert w._fitted(imgs[0]) is imgs[0] and w._fitted(imgs[3]) is imgs[3]
    # fit='none' is today's path: PIL's resize is not called, the sizes stay
    calls.clear()
    assert [tuple(x.shape) for x in w._images(imgs[3:6], "host")] == [(1, 32, 64), (1, 48, 96), (1, 32, 112)] and calls == []
    with pytest.raises(ValueError, match="fit must be 'none' or 'canvas'"):
        w._images(imgs[:1], "host", "stretch")
    # the scale-32 refusal names the image in the engine's words (test_fit_refusals_without_a_device has the same text from the library)
    with pytest.raises(ValueError, match="ingest: image 1 is 3x100000, 1x96 fitted to 32x96: an axis shrinks by more than 32 times"):
        w._images([imgs[0], Image.fromarray(np.zeros((3, 100000), np.uint8))], "host", "canvas")
