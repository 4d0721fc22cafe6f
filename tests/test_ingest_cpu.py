"""No-GPU checks of the device-side image ingest (txo_ingest_u8 / texocr::ingest_u8 / ops.pack_u8): the host packing up to, but not into,
the operator; the new symbols and their refusals at the C ABI; and the kernel's step sequence, restated in float32 numpy, against
wrapper.preprocess_image on the lists the GPU tests run."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ingest_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the specification ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_list", "sweep_list", "flat_list"])
def test_kernel_steps_equal_preprocess_image(name):
    """the separately rounded float32 steps the kernel takes are preprocess_image's numpy expressions, bit for bit; its pad is 0.0"""
    from texocr_amd.wrapper import preprocess_image
    for k, im in enumerate(getattr(cases, name)()):
        a = np.asarray(im)
        h, w = a.shape[:2]
        ref = preprocess_image(im)[0].numpy()
        assert ref.shape == ((h + 15) // 16 * 16, (w + 15) // 16 * 16)
        assert np.array_equal(ref[:h, :w], cases.kernel_steps(a)), (name, k)
        assert not ref[h:].any() and not ref[:, w:].any(), (name, k)


def test_white_is_not_the_pad_value():
    """the luma weights sum to 0.9999: white maps to 9.9957e-05, so a pad of exactly 0.0 can be told from white pixels"""
    white = cases.kernel_steps(np.full((1, 1, 3), 255, np.uint8))[0, 0]
    assert abs(float(white) - 9.9957e-05) < 1e-9 and white != 0
    assert cases.kernel_steps(np.zeros((1, 1), np.uint8))[0, 0] == np.float32(1.0)


# ---- the host packing of pack_u8 -------------------------------------------------------------------------------------------------------
def test_plan_offsets_alignment_and_shapes():
    from texocr_amd import ops
    imgs = cases.mixed_list()
    staged, dev, src, shapes = ops.plan_u8(imgs)
    assert dev == [] and staged.dtype == torch.uint8 and staged.ndim == 1 and not staged.is_cuda
    assert src.dtype == torch.int64 and tuple(src.shape) == (len(imgs), 2) and shapes.dtype == torch.int32 and tuple(shapes.shape) == (len(imgs), 3)
    end = 0
    for b, im in enumerate(imgs):
        a = np.asarray(im)
        k, off = src[b].tolist()
        h, w, ch = shapes[b].tolist()
        assert (h, w) == a.shape[:2] and ch == {"L": 1, "RGB": 3, "RGBA": 4}[im.mode]
        assert k == 0 and off % ops.U8_ALIGN == 0 and off >= end                     # aligned, in list order, no overlap
        assert np.array_equal(staged[off:off + a.size].numpy(), a.reshape(-1))        # interleaved channels, rows tightly packed
        end = off + a.size
    assert staged.numel() >= end and staged.numel() - end < ops.U8_ALIGN
    assert ops.box_u8(shapes) == (48, 160)
    assert ops.box_u8(torch.tensor([[1, 1, 1], [17, 33, 3]], dtype=torch.int32)) == (32, 48)


def test_plan_takes_pil_numpy_and_tensors_alike():
    from PIL import Image
    from texocr_amd import ops
    rng = np.random.RandomState(0)
    a3 = rng.randint(0, 256, (9, 21, 3)).astype(np.uint8)
    a1 = rng.randint(0, 256, (7, 5)).astype(np.uint8)
    ref = ops.plan_u8([Image.fromarray(a3), Image.fromarray(a1)])
    for lst in ([a3, a1], [torch.from_numpy(a3), torch.from_numpy(a1)], [np.asfortranarray(a3), torch.from_numpy(a1.T.copy()).T]):
        got = ops.plan_u8(lst)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    # a channel count the kernel does not take is the ENGINE's to refuse: the plan records it
    assert ops.plan_u8([np.zeros((4, 4, 2), np.uint8)])[3].tolist() == [[4, 4, 2]]
    assert ops.plan_u8([])[3].shape == (0, 3) and ops.plan_u8([])[0].numel() == 0


def test_plan_mode_conversion():
    """modes other than L / RGB / RGBA go through convert('RGB'), as preprocess_image does with every mode"""
    from PIL import Image
    from texocr_amd import ops
    rng = np.random.RandomState(1)
    rgb = Image.fromarray(rng.randint(0, 256, (6, 10, 3)).astype(np.uint8))
    for mode in ("P", "1", "LA", "CMYK", "I;16", "F"):
        im = rgb.convert("L").convert(mode) if mode in ("I;16", "F", "1", "LA") else rgb.convert(mode)
        staged, _, _, shapes = ops.plan_u8([im])
        assert shapes.tolist() == [[6, 10, 3]], mode
        assert np.array_equal(staged[:180].numpy(), np.asarray(im.convert("RGB")).reshape(-1)), mode


@pytest.mark.parametrize("bad,frag", [
    (np.zeros((4, 4, 3), np.float32), "uint8"), (torch.zeros((4, 4), dtype=torch.int16), "uint8"),
    (np.zeros((4,), np.uint8), r"\(H, W\)"), (np.zeros((1, 4, 4, 3), np.uint8), r"\(H, W\)"), ("image.png", "PIL image"),
])
def test_plan_refuses_what_is_not_an_image_of_bytes(bad, frag):
    from texocr_amd import ops
    with pytest.raises(ValueError, match="image 1 must be .*" + frag):
        ops.plan_u8([np.zeros((4, 4), np.uint8), bad])


def test_packed_images_pass_through_pack_ragged():
    from texocr_amd import ops
    box, sizes = torch.zeros((2, 1, 32, 48)), torch.tensor([[16, 48], [32, 16]], dtype=torch.int32)
    p = ops.PackedImages(box, sizes)
    out = ops.pack_ragged(p)
    assert out[0] is box and out[1] is sizes                                          # untouched: no copy, no check of its own
    assert len(p) == 2 and p.device == box.device and p.grids(16) == [(1, 3), (2, 1)]
    # pack_ragged keeps its behaviour for lists
    b2, s2 = ops.pack_ragged([torch.ones((1, 16, 48)), torch.ones((1, 32, 16))])
    assert torch.equal(s2, sizes) and b2.shape == box.shape and float(b2.sum()) == 16 * 48 + 32 * 16


def test_fake_implementation_gives_the_shapes():
    """texocr::ingest_u8 traces without a GPU (FakeTensorMode), like every other operator"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    from texocr_amd.config import Dims

    class Stub:
        dims = Dims(canvas=64, in_channels=3)
    stub = Stub()
    i = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            box, sizes = torch.ops.texocr.ingest_u8([torch.empty((100,), dtype=torch.uint8)], torch.zeros((2, 2), dtype=torch.int64),
                                                    torch.zeros((2, 3), dtype=torch.int32), i, 3, 32, 48)
        assert tuple(box.shape) == (2, 3, 32, 48) and box.dtype == torch.float32
        assert tuple(sizes.shape) == (2, 2) and sizes.dtype == torch.int32 and sizes.device.type == "cpu"
    finally:
        ops.unregister_engine(i)


def test_wrapper_and_model_expose_the_switch():
    import inspect
    from texocr_amd.model import HipEngine, OCRModel
    from texocr_amd.wrapper import TeXOCRWrapper
    for fn in (TeXOCRWrapper.batch, TeXOCRWrapper.__call__):
        assert inspect.signature(fn).parameters["ingest"].default == "host"
    assert callable(OCRModel.ingest) and callable(HipEngine.ingest)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def _i32(rows):
    flat = [int(v) for r in rows for v in r]
    return (C.c_int32 * max(len(flat), 1))(*flat)


def test_symbols_exported(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name in ("txo_ingest_u8", "txo_ingest_box"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and (name + "(") in hdr


def test_ingest_box(lib):
    from texocr_amd import _lib
    hc, wc = C.c_int32(0), C.c_int32(0)
    assert lib.txo_ingest_box(_i32([(1, 1, 1), (17, 33, 3), (48, 20, 4)]), 3, C.byref(hc), C.byref(wc)) == 0
    assert (hc.value, wc.value) == (48, 48)
    for shapes, n, frag in [([(1, 1, 2)], 1, "image 0 has ch = 2"), ([(4, 4, 3), (0, 4, 3)], 2, "image 1 is 0x4"), ([(4, -1, 1)], 1, "image 0 is 4x-1"),
                            ([(4, 4, 3)], 0, "no images")]:
        assert lib.txo_ingest_box(_i32(shapes), n, C.byref(hc), C.byref(wc)) == _lib.TXO_E_INVALID
        assert frag in lib.txo_last_error().decode(), lib.txo_last_error().decode()
    assert lib.txo_ingest_box(None, 1, C.byref(hc), C.byref(wc)) == _lib.TXO_E_INVALID
    assert lib.txo_ingest_box(_i32([(4, 4, 3)]), 1, None, None) == _lib.TXO_E_INVALID


def test_ingest_refusals_without_a_device(lib):
    """the list and the container are checked before the engine or the device is looked at: every refusal below answers TXO_E_INVALID with
    a message naming the image, on a machine without a GPU and with no engine"""
    from texocr_amd import _lib
    off = (C.c_int64 * 2)(0, 64)
    sizes = (C.c_int32 * 4)()
    ok = _i32([(16, 16, 3), (17, 33, 1)])

    def call(shapes, B=2, C_=1, Hc=32, Wc=48, offsets=off, sizes_out=sizes):
        rc = lib.txo_ingest_u8(None, None, offsets, shapes, B, C_, Hc, Wc, None, sizes_out, None)
        return rc, lib.txo_last_error().decode()
    for kw, frag in [
        (dict(shapes=_i32([(16, 16, 3), (17, 33, 2)])), "image 1 has ch = 2"),
        (dict(shapes=_i32([(16, 16, 5), (17, 33, 1)])), "image 0 has ch = 5"),
        (dict(shapes=_i32([(16, 0, 3), (17, 33, 1)])), "image 0 is 16x0"),
        (dict(shapes=ok, B=0), "no images"),
        (dict(shapes=ok, B=-3), "no images"),
        (dict(shapes=None), "null shapes"),
        (dict(shapes=ok, offsets=None), "null offsets"),
        (dict(shapes=ok, offsets=(C.c_int64 * 2)(0, -1)), "image 1 has a negative byte offset"),
        (dict(shapes=ok, Hc=16), "image 1 is 17x33, 32x48 rounded up"),
        (dict(shapes=ok, Wc=32), "image 1 is 17x33, 32x48 rounded up"),
        (dict(shapes=ok, Wc=50), "multiple of 4"),
        (dict(shapes=ok, C_=0), "channel count"),
        (dict(shapes=ok), "null argument"),                       # a good list: only now does the missing engine matter
    ]:
        rc, msg = call(**kw)
        assert rc == _lib.TXO_E_INVALID and frag in msg, (kw, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert list(sizes) == [0, 0, 0, 0]                            # nothing is written on a refusal


def test_a_c_program_links_against_the_new_symbols(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "ingest_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "texocr.h"
int main(void) {
    const int32_t shapes[2][3] = {{17, 33, 3}, {40, 20, 1}};
    const int64_t offsets[2] = {0, 1696};
    int32_t hc = 0, wc = 0, sizes[2][2];
    int rc = txo_ingest_box(&shapes[0][0], 2, &hc, &wc);
    printf("box %d -> %d x %d\n", rc, hc, wc);
    rc = txo_ingest_u8(NULL, NULL, offsets, &shapes[0][0], 2, 1, hc, wc, NULL, &sizes[0][0], NULL);
    printf("no engine -> %d (%s)\n", rc, txo_last_error());
    const int32_t bad[1][3] = {{4, 4, 2}};
    rc = txo_ingest_box(&bad[0][0], 1, &hc, &wc);
    printf("ch 2 -> %d (%s)\n", rc, txo_last_error());
    return 0;
}
''')
    exe = str(tmp_path / "ingest_abi")
    libdir = os.path.join(ROOT, "texocr_amd")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-ltexocr_hip",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "box 0 -> 48 x 48" in out and "no engine -> -1 (ingest: null argument)" in out and "ch 2 -> -1 (ingest: image 0 has ch = 2" in out
