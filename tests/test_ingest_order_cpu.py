"""No-GPU check of the ORDER in which the ingest entry points refuse (txo_ingest_u8, txo_ingest_u8_fit, txo_ingest_u8_view,
txo_ingest_trim_views): every call below carries two faults and passes a null engine, so every check that needs neither an engine nor a
device is reachable; the fault that is checked first must be the one reported.  Each case also makes the call with the second fault alone
(where that needs no engine), so that the first one is seen to win and not merely to be the only fault present."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _i32(rows):
    if rows is None:
        return None
    flat = [int(v) for r in rows for v in r]
    return (C.c_int32 * max(len(flat), 1))(*flat)


def _i64(vals):
    return None if vals is None else (C.c_int64 * len(vals))(*vals)


SIZES = (C.c_int32 * 8)()
ALIGNED, MISALIGNED = C.c_void_p(4096), C.c_void_p(4104)     # never dereferenced: every call below is refused before the device is looked at


def _u8(lib, shapes=((16, 16, 3), (17, 33, 1)), B=2, C_=1, Hc=32, Wc=48, offsets=(0, 1024), box=None, pix=None):
    return lib.txo_ingest_u8(None, pix, _i64(offsets), _i32(shapes), B, C_, Hc, Wc, box, SIZES, None)


# (47, 301, 3) is 14x96 under the target 32x96 and needs 47 x 96 x 3 bytes of scratch, rounded up to 16
def _fit(lib, shapes=((16, 16, 3), (47, 301, 3)), B=2, C_=1, Fh=32, Fw=96, Hc=32, Wc=96, offsets=(0, 1024), nbytes=1 << 20):
    return lib.txo_ingest_u8_fit(None, None, _i64(offsets), _i32(shapes), B, C_, Fh, Fw, Hc, Wc, None, SIZES, C.c_void_p(64), nbytes, None)


GOOD_VIEWS = ((4, 5, 30, 50), (10, 20, 47, 301))


def _view(lib, views=GOOD_VIEWS, shapes=((40, 60, 3), (100, 400, 1)), B=2, C_=1, Fh=0, Fw=0, Hc=48, Wc=304, offsets=(0, 8192)):
    return lib.txo_ingest_u8_view(None, None, _i64(offsets), _i32(shapes), _i32(views), B, C_, Fh, Fw, Hc, Wc, None, SIZES, C.c_void_p(64),
                                  1 << 20, None)


def _trim(lib, shapes=((16, 16, 3), (47, 301, 1)), B=2, level=127, margin=2, offsets=(0, 4096)):
    return lib.txo_ingest_trim_views(None, None, _i64(offsets), _i32(shapes), B, level, margin, SIZES, None)


NULL_ARG, NEG_OFF = "ingest: null argument", "has a negative byte offset"
NO_FIT = "it does not fit the container's"

# (entry, the call with both faults, the message that wins, the call with the second fault alone, its message -- None: it needs an engine)
CASES = [
    # txo_ingest_u8: the list, the container, the null arguments, the alignment
    (_u8, dict(B=0, shapes=None), "no images", dict(shapes=None), "null shapes"),
    (_u8, dict(shapes=((0, 16, 3), (17, 33, 2))), "image 0 is 0x16", dict(shapes=((16, 16, 3), (17, 33, 2))), "image 1 has ch = 2"),
    (_u8, dict(shapes=((0, 16, 2), (17, 33, 1))), "image 0 has ch = 2", dict(shapes=((0, 16, 3), (17, 33, 1))), "image 0 is 0x16"),
    (_u8, dict(shapes=((16, 16, 3), (17, 0, 1)), offsets=None), "image 1 is 17x0", dict(offsets=None), "null offsets"),
    (_u8, dict(offsets=None, C_=0), "null offsets", dict(C_=0), "channel count must be >= 1"),
    (_u8, dict(Wc=46), "multiple of 4", dict(Wc=32), "image 1 is 17x33, 32x48 rounded up to multiples of 16: " + NO_FIT + " 32x32"),
    (_u8, dict(shapes=((17, 16, 3), (16, 16, 1)), Hc=16, offsets=(0, -1)), "image 0 is 17x16, 32x16 rounded up",
     dict(offsets=(0, -1)), "image 1 " + NEG_OFF),
    (_u8, dict(Hc=16), "image 1 is 17x33, 32x48 rounded up", dict(), NULL_ARG),
    (_u8, dict(box=MISALIGNED, pix=ALIGNED), NULL_ARG, None, None),
    # txo_ingest_u8_fit: the list, the target, the scale limit, the container on the FITTED sizes, the scratch, the null arguments
    (_fit, dict(shapes=((16, 16, 3), (47, 301, 5)), Fw=100), "image 1 has ch = 5", dict(Fw=100), "the fit target is 32x100"),
    (_fit, dict(shapes=((16, 16, 3), (3, 100000, 1)), Fh=20), "the fit target is 20x96",
     dict(shapes=((16, 16, 3), (3, 100000, 1))), "image 1 is 3x100000, 1x96 fitted to 32x96: an axis shrinks by more than 32 times"),
    (_fit, dict(shapes=((16, 16, 3), (3, 100000, 1)), offsets=None), "an axis shrinks by more than 32 times", dict(offsets=None), "null offsets"),
    (_fit, dict(Wc=80, nbytes=16), "image 1 is 14x96, 16x96 rounded up to multiples of 16: " + NO_FIT + " 32x80",
     dict(nbytes=16), "the fit scratch is 16 bytes; the horizontal passes of this list need 13536 bytes"),
    (_fit, dict(nbytes=13535), "the fit scratch is 13535 bytes", dict(), NULL_ARG),
    # txo_ingest_u8_view: the list, the two arrays, every view in turn, then txo_ingest_u8's / txo_ingest_u8_fit's checks on the views
    (_view, dict(shapes=((40, 60, 3), (100, 0, 1)), offsets=None), "image 1 is 100x0", dict(offsets=None), "null offsets"),
    (_view, dict(offsets=None, views=None), "null offsets", dict(views=None), "null views"),
    (_view, dict(offsets=(-1, 8192), views=((4, 5, 0, 50), GOOD_VIEWS[1])), "image 0 " + NEG_OFF,
     dict(views=((4, 5, 0, 50), GOOD_VIEWS[1])), "image 0 has the view 0x50 at (4, 5); both sides must be >= 1"),
    (_view, dict(offsets=(0, -1), views=((4, 11, 30, 50), GOOD_VIEWS[1])), "image 0 has the view 30x50 at (4, 11), which reaches outside",
     dict(offsets=(0, -1)), "image 1 " + NEG_OFF),
    (_view, dict(views=(GOOD_VIEWS[0], (54, 20, 47, 301)), Fh=20, Fw=96), "image 1 has the view 47x301 at (54, 20), which reaches outside",
     dict(Fh=20, Fw=96), "the fit target is 20x96"),
    # txo_ingest_trim_views: the list, the offsets, the level, the margin, the null arguments
    (_trim, dict(shapes=((16, 16, 3), (47, 301, 2)), level=255), "image 1 has ch = 2", dict(level=255), "the trim level is 255"),
    (_trim, dict(offsets=(0, -1), level=255), "image 1 " + NEG_OFF, dict(level=255), "the trim level is 255"),
    (_trim, dict(level=-1, margin=-1), "the trim level is -1", dict(margin=-1), "the trim margin is -1"),
    (_trim, dict(margin=-1), "the trim margin is -1", dict(), NULL_ARG),
]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_the_first_of_two_faults_is_the_one_reported(lib, k):
    from texocr_amd import _lib
    entry, both, first, second_alone, second = CASES[k]
    for kw, frag in [(both, first)] + ([(second_alone, second)] if second_alone is not None else []):
        rc = entry(lib, **kw)
        msg = lib.txo_last_error().decode()
        assert rc == _lib.TXO_E_INVALID and frag in msg, (entry.__name__, kw, msg)
    assert list(SIZES) == [0] * 8                                  # nothing is written on a refusal


def test_a_view_is_judged_on_its_own_size(lib):
    """a view that fits the container although its image does not is accepted as far as the missing engine"""
    from texocr_amd import _lib
    assert _view(lib, Hc=48, Wc=304) == _lib.TXO_E_INVALID and lib.txo_last_error().decode() == NULL_ARG   # the images: 48x64 and 112x400
    assert _view(lib, Fh=32, Fw=96, Hc=32, Wc=96) == _lib.TXO_E_INVALID and lib.txo_last_error().decode() == NULL_ARG
