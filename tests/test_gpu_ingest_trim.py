"""Trim-to-ink and region ingest on the GPU (txo_ingest_trim_views / txo_ingest_u8_view, texocr_amd/csrc/ingest_trim.h and the pitched
forms of the ingest kernels): the views the device finds equal the brute-force rule tests/trim_ref.py element for element, the container of
the views equals the existing pack_u8 of contiguous host copies bit for bit (with and without the fit), and everything downstream is
identical by either ingest and to the wrapper on host-cropped images.  Every comparison is exact; outputs start as NaN (TXO_DEBUG_POISON)."""
import json
import os

import numpy as np
import pytest
import torch

import ingest_cases
import trim_ref
from gpu_harness import knobs
from texocr_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda", 0)


def _wrapper(tmp, img_size, dtype="fp32", max_batch=3):
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(GOLDEN, "tokenizer_vocab_1k.json")))
    path = str(tmp / "vocab.txt")
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(path)
    cfg = default_config(img_size=list(img_size), max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = path
    w = TeXOCRWrapper(cfg, dtype=dtype, max_batch=max_batch)
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 5))
    return w


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """the tiny model on a 32 x 96 canvas; max_batch holds the longest list of this file (the ingest needs no more of the engine)"""
    return _wrapper(tmp_path_factory.mktemp("trim"), (32, 96), max_batch=96)


def _white(h, w, ch):
    return np.full((h, w) if ch == 1 else (h, w, ch), 255, np.uint8)


def _sparse(h, w, ch, seed):
    """white with a few pixels of a few values around the levels the tests use, in any channel (the alpha included)"""
    rng = np.random.RandomState(seed)
    a = np.full((h, w, ch), 255, np.uint8)
    n = 1 + seed % 4
    a[rng.randint(0, h, n), rng.randint(0, w, n), rng.randint(0, ch, n)] = rng.choice([0, 1, 2, 127, 128, 254], n)
    return a[..., 0] if ch == 1 else a


def _framed(h, w, box, ch, seed):
    """white (h, w, ch) with noise inside box = (y0, x0, y1, x1) whose corners are black, so the ink box at level 127 is exactly `box`"""
    rng = np.random.RandomState(seed)
    y0, x0, y1, x1 = box
    a = np.full((h, w, ch), 255, np.uint8)
    a[y0:y1, x0:x1, :3] = rng.randint(0, 256, (y1 - y0, x1 - x0, min(ch, 3)))
    a[y0, x0, :3] = a[y1 - 1, x1 - 1, :3] = 0
    return a[..., 0] if ch == 1 else a


def _on_device_at_odd_offset(a, off):
    """a (numpy uint8) -> a contiguous device tensor of its shape whose first byte lies at an odd address"""
    buf = torch.zeros((a.size + 16,), dtype=torch.uint8, device=DEV)
    buf[off:off + a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
    t = buf[off:off + a.size].view(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 2 == 1
    return t


def _rule_list():
    """-> (what goes to pack_u8 / plan_u8, the same images as numpy arrays), L / RGB / RGBA mixed"""
    arrs = [np.asarray(im) for im in ingest_cases.mixed_list()]                      # MIXED_SIZES in every mode, random pixels: ink everywhere
    arrs += [_sparse(h, w, (1, 3, 4)[k % 3], k) for k, (h, w) in enumerate(ingest_cases.MIXED_SIZES * 2)]   # ... and sparse ink on white
    strip, column = _white(1, 5000, 1), _white(3000, 1, 1)                        # one image over many blocks: the atomics decide
    strip[0, [1234, 4321]] = 0
    column[[17, 2900], 0] = 100
    arrs += [strip, column]
    for w in (17, 33):                                                            # rows start at every byte phase of a 16-byte load
        a = _white(19, w, 3)
        a[3, 1, 2] = a[15, w - 2, 0] = 127
        arrs.append(a)
    for y, x in ((0, 0), (0, 36), (19, 0), (19, 36), (0, 18), (19, 18), (10, 0), (10, 36)):   # one ink pixel in each corner, on each edge
        a = _white(20, 37, (3, 4, 1)[(y + x) % 3])
        a[y, x] = 0
        arrs.append(a)
    for a in (_framed(60, 90, (1, 1, 59, 89), 3, 0), _framed(60, 90, (2, 2, 58, 88), 4, 1), _framed(7, 9, (3, 4, 4, 5), 1, 2)):
        arrs.append(a)                                                            # margins that clamp on every side (and one that does not)
    items = list(arrs)
    # a blank image packed between two all-black neighbours, no byte between them, the blank one at an odd address
    n0, n1, n2 = 7 * 9, 5 * 11 * 3, 3 * 5
    buf = torch.zeros((n0 + n1 + n2,), dtype=torch.uint8, device=DEV)
    buf[n0:n0 + n1] = 255
    trio = [buf[:n0].view(7, 9), buf[n0:n0 + n1].view(5, 11, 3), buf[n0 + n1:].view(3, 5)]
    assert trio[1].data_ptr() % 2 == 1 and trio[1].data_ptr() + n1 == trio[2].data_ptr()
    items += trio
    arrs += [t.cpu().numpy() for t in trio]
    # device-resident tensors at odd byte offsets
    for k, a in enumerate((_sparse(33, 47, 3, 40), _framed(25, 70, (5, 9, 20, 61), 4, 41), _sparse(40, 13, 1, 42))):
        items.append(_on_device_at_odd_offset(a, 1 + 2 * k))
        arrs.append(a)
    return items, arrs


@pytest.fixture(scope="module")
def rule_list():
    return _rule_list()


def _views(w, items, level, margin):
    from texocr_amd import ops
    staged, dev, src, shapes = ops.plan_u8(items)
    return torch.ops.texocr.ingest_trim_views([staged.to(DEV)] + dev, src, shapes, w.model._engine.id, level, margin)


# ---- 1. the views against the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,margin", [(127, 2), (0, 0), (254, 50), (1, 1)])
def test_views_equal_the_rule(small, rule_list, level, margin):
    items, arrs = rule_list
    assert len(items) == len(arrs) <= small.model._engine.max_batch and {a.shape[2] if a.ndim == 3 else 1 for a in arrs} == {1, 3, 4}
    want = [trim_ref.view(a, level, margin) for a in arrs]
    got = _views(small, items, level, margin)
    assert got.dtype == torch.int32 and not got.is_cuda and tuple(got.shape) == (len(arrs), 4)
    bad = [(b, arrs[b].shape, tuple(got[b].tolist()), want[b]) for b in range(len(arrs)) if tuple(got[b].tolist()) != want[b]]
    assert not bad, bad
    if (level, margin) == (127, 2):
        trio = len(arrs) - 6                                      # the blank image between the black ones comes back whole, they do too
        assert want[trio:trio + 3] == [(0, 0, 7, 9), (0, 0, 5, 11), (0, 0, 3, 5)]
        strip = [a.shape for a in arrs].index((1, 5000))
        assert arrs[strip + 1].shape == (3000, 1) and want[strip] == (0, 1232, 1, 3092) and want[strip + 1] == (15, 0, 2888, 1)
        assert sum(v != (0, 0) + a.shape[:2] for v, a in zip(want, arrs)) >= 15      # the list really trims


# ---- 2. the container ------------------------------------------------------------------------------------------------------------------------
def _pack(w, items, channels, **kw):
    from texocr_amd import ops
    with knobs(TXO_DEBUG_POISON=1):                                # the output starts as NaN: an element left unwritten fails torch.equal
        got = ops.pack_u8(items, channels, DEV, engine=w.model._engine.id, **kw)
    box = got.box.cpu()
    assert not torch.isnan(box).any(), "an element of the container was left unwritten"
    return box, got.sizes, got.views


def _fit_list():
    """views under the target 32 x 96 that need a horizontal pass only, a vertical pass only, both, and neither (checked by the test)"""
    strip, column = _white(1, 130, 1), _white(60, 1, 4)
    strip[0, 10:110:3] = 0
    strip[0, 109] = 0
    column[10:50:2, 0, :3] = 30
    column[49, 0, 1] = 0
    return [_framed(40, 120, (12, 30, 27, 90), 3, 0),              # 19 x 64: fits
            _framed(100, 300, (20, 25, 80, 275), 1, 1),           # 64 x 254: both passes
            strip,                                                # 1 x 104: the width shrinks, the height cannot
            column,                                               # 44 x 1: the height shrinks, the width cannot
            _framed(200, 400, (80, 100, 106, 186), 4, 2),         # 30 x 90 out of an image far beyond the target: fits
            _white(20, 30, 3),                                    # blank: whole
            _framed(70, 500, (10, 8, 60, 488), 3, 3),             # 54 x 484: both
            _framed(48, 80, (0, 0, 48, 80), 4, 4)]                # ink to every border: the whole image, tightly packed rows; both


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("fit", [None, (32, 96)])
def test_container_equals_pack_u8_of_host_crops(small, rule_list, channels, fit):
    from texocr_amd import ops
    items = arrs = _fit_list()
    trim = (127, 2)
    want_views = [trim_ref.view(a, *trim) for a in arrs]
    assert want_views[:5] == [(10, 28, 19, 64), (18, 23, 64, 254), (0, 8, 1, 104), (8, 0, 44, 1), (78, 98, 30, 90)] and want_views[5] == (0, 0, 20, 30)
    if fit is not None:                                           # the property the list was chosen for, on the CPU
        kinds = set()
        for (_, _, vh, vw) in want_views:
            fh, fw = ops.fit_size(vh, vw, *fit)
            kinds.add((fw != vw, fh != vh))
        assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    crops = [trim_ref.crop(a, v) for a, v in zip(arrs, want_views)]
    ref_box, ref_sizes, ref_views = _pack(small, crops, channels, fit=fit)
    assert ref_views is None
    box, sizes, views = _pack(small, items, channels, fit=fit, trim=trim)
    assert views.tolist() == [list(v) for v in want_views] and views.dtype == torch.int32 and not views.is_cuda
    assert torch.equal(sizes, ref_sizes) and tuple(box.shape) == tuple(ref_box.shape)
    bad = [(b, int((box[b] != ref_box[b]).sum())) for b in range(len(arrs)) if not torch.equal(box[b], ref_box[b])]
    assert not bad, bad
    if fit is None and channels == 1:
        # ... and on the long mixed list of test 1, host and device images alike; model.ingest is the same call
        items, arrs = rule_list
        want_views = [trim_ref.view(a, *trim) for a in arrs]
        ref_box, ref_sizes, _ = _pack(small, [trim_ref.crop(a, v) for a, v in zip(arrs, want_views)], 1)
        box, sizes, views = _pack(small, items, 1, trim=trim)
        assert views.tolist() == [list(v) for v in want_views] and torch.equal(sizes, ref_sizes) and torch.equal(box, ref_box)
        got = small.model.ingest(items, trim=True)
        assert torch.equal(got.views, views) and torch.equal(got.sizes, sizes) and torch.equal(got.box.cpu(), box)


# ---- 3. regions --------------------------------------------------------------------------------------------------------------------------------
REGIONS = [(0, 0, 120, 200), (10, 20, 30, 100), (15, 60, 30, 100), (0, 0, 1, 1), (119, 199, 1, 1), (40, 0, 17, 200), (0, 77, 120, 33), (50, 90, 47, 101)]


@pytest.mark.parametrize("fit", [None, (32, 96)])
def test_regions_of_one_page(small, fit):
    from texocr_amd import ops
    rng = np.random.RandomState(9)
    page = rng.randint(0, 256, (120, 200, 3)).astype(np.uint8)
    slices = [np.ascontiguousarray(page[y0:y0 + h, x0:x0 + w]) for y0, x0, h, w in REGIONS]
    ref_box, ref_sizes, _ = _pack(small, slices, 1, fit=fit)
    dev_page = _on_device_at_odd_offset(page, 3)
    for obj in (dev_page, page):
        staged, dev, src, shapes = ops.plan_u8([obj] * len(REGIONS))
        if obj is dev_page:                                       # the page's bytes are used where they lie, once
            assert staged.numel() == 0 and len(dev) == 1 and dev[0].data_ptr() == dev_page.data_ptr() and src.tolist() == [[1, 0]] * 8
        else:                                                     # ... or staged once
            assert staged.numel() == page.size and dev == [] and src.tolist() == [[0, 0]] * 8
        box, sizes, views = _pack(small, [obj] * len(REGIONS), 1, fit=fit, regions=REGIONS)
        assert views.tolist() == [list(r) for r in REGIONS]
        assert torch.equal(sizes, ref_sizes) and tuple(box.shape) == tuple(ref_box.shape)
        bad = [(b, int((box[b] != ref_box[b]).sum())) for b in range(len(REGIONS)) if not torch.equal(box[b], ref_box[b])]
        assert not bad, bad
    got = small.model.ingest([dev_page] * 8, fit=fit is not None, regions=torch.tensor(REGIONS))
    assert torch.equal(got.sizes, ref_sizes) and torch.equal(got.box.cpu(), ref_box)


# ---- 4. - 5. end to end ------------------------------------------------------------------------------------------------------------------------
def _pil_list():
    """five images for the 64 x 256 canvas with white around the ink: two of them beyond the canvas whose ink fits it, one blank"""
    from PIL import Image
    out = []
    for k, (h, w, box, ch) in enumerate([(60, 240, (20, 50, 45, 200), 3), (300, 700, (100, 300, 140, 500), 3), (50, 90, (0, 0, 50, 90), 1),
                                         (150, 200, (60, 10, 110, 190), 4), (30, 30, None, 1)]):
        a = _white(h, w, ch) if box is None else _framed(h, w, box, ch, 10 + k)
        if box is not None and ch != 1:
            a[max(0, box[0] - 1), box[1]:box[3], :3] = 180       # an anti-aliased rim lighter than the level: inside the margin
        out.append(Image.fromarray(a))
    return out


def _host_crops(pil, level=127, margin=2):
    out = []
    for im in pil:
        y0, x0, h, w = trim_ref.view(np.asarray(im), level, margin)
        out.append(im.crop((x0, y0, x0 + w, y0 + h)))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v, (u, v)


def test_oversized_image_whose_ink_fits_is_accepted(tmp_path):
    from PIL import Image
    w = _wrapper(tmp_path, (64, 256), max_batch=3)
    pil = _pil_list()
    big = pil[1]                                                  # 300 x 700; its ink and the margin are 44 x 204
    crop = _host_crops([big])[0]
    assert crop.size == (204, 44)
    want = w.batch([crop], max_len=12, decode="greedy")
    for ingest in ("host", "device"):
        _same(w.batch([big], max_len=12, decode="greedy", ingest=ingest, trim="ink", fit="none"), want)
        _same([w(big, max_len=12, decode="greedy", ingest=ingest, trim="ink")], [w(crop, max_len=12, decode="greedy")])
        # the same calls without trim still raise today's messages
        with pytest.raises(ValueError, match="ragged batches: image 0 is larger than the position-embedding canvas"):
            w.batch([big], max_len=12, decode="greedy", ingest=ingest)
        with pytest.raises(ValueError, match="image size 304x704 exceeds the 64x256 canvas"):
            w(big, max_len=12, decode="greedy", ingest=ingest)
        # ink that does not fit: today's refusal, with the trimmed size
        wide = Image.fromarray(_framed(300, 700, (100, 100, 140, 500), 3, 3))
        with pytest.raises(ValueError, match="ragged batches: image 0 is larger than the position-embedding canvas"):
            w.batch([wide], max_len=12, decode="greedy", ingest=ingest, trim="ink")
        with pytest.raises(ValueError, match="image size 48x416 exceeds the 64x256 canvas"):
            w(wide, max_len=12, decode="greedy", ingest=ingest, trim="ink")
    # the views come back in source pixels
    assert w.model.ingest([big], trim=(127, 2)).views.tolist() == [[98, 298, 44, 204]]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_batch_and_call_agree_by_either_ingest_and_with_host_crops(tmp_path, dtype):
    """trim='ink': tokens, LaTeX, log-probabilities and maps are identical by either ingest and to the wrapper on host-cropped PIL images --
    greedy, seeded sampling, beam, align -- over a list longer than max_batch"""
    w = _wrapper(tmp_path, (64, 256), dtype=dtype, max_batch=3)
    pil = _pil_list()
    crops = _host_crops(pil)
    assert [c.size for c in crops] == [(154, 29), (204, 44), (90, 50), (184, 54), (30, 30)]
    for kw in (dict(decode="greedy", return_logp=True), dict(decode="sample", seed=11, return_logp=True), dict(decode="beam", beams=3, return_logp=True),
               dict(decode="greedy", return_align=True)):
        want = w.batch(crops, max_len=12, **kw)
        host = w.batch(pil, max_len=12, ingest="host", trim="ink", **kw)
        dev = w.batch(pil, max_len=12, ingest="device", trim="ink", **kw)
        assert len(want) == len(pil) > w.model._engine.max_batch
        _same(host, want)
        _same(dev, want)
        if kw.get("return_align"):
            for (toks, _, maps), c in zip(dev, crops):
                assert tuple(maps.shape) == (len(toks), (c.size[1] + 15) // 16, (c.size[0] + 15) // 16)
    for im, c in zip(pil[:2], crops[:2]):
        want = [w(c, max_len=12, decode="greedy", return_logp=True, return_align=True)]
        _same([w(im, max_len=12, decode="greedy", return_logp=True, return_align=True, trim="ink")], want)
        _same([w(im, max_len=12, decode="greedy", return_logp=True, return_align=True, trim="ink", ingest="device")], want)
    # another level and margin; trim in front of the fit (150 x 200 at margin 40 is 130 x 200: beyond the canvas again)
    crops = [_host_crops([im], 10, 40)[0] for im in pil]
    assert crops[3].size == (200, 130)
    want = w.batch(crops, max_len=12, decode="greedy", fit="canvas")
    for ingest in ("host", "device"):
        _same(w.batch(pil, max_len=12, decode="greedy", ingest=ingest, fit="canvas", trim="ink", trim_level=10, trim_margin=40), want)
    # trim='none' is every default
    _same(w.batch(pil[::2], max_len=12, decode="greedy", trim="none", ingest="device"), w.batch(pil[::2], max_len=12, decode="greedy"))
    with pytest.raises(ValueError, match="trim must be 'none' or 'ink'"):
        w.batch(pil, trim="tight", ingest="device")


# ---- 6. refusals reach Python --------------------------------------------------------------------------------------------------------------
def test_refusals_reach_python(small):
    from texocr_amd import ops
    eng = small.model._engine
    good = _framed(20, 40, (5, 5, 15, 30), 3, 0)
    staged, dev, src, shapes = ops.plan_u8([good, _white(17, 33, 1)])
    bufs = [staged.to(DEV)]
    with pytest.raises(ValueError, match=r"ingest: the trim level is 255; it must lie in \[0, 254\]"):
        torch.ops.texocr.ingest_trim_views(bufs, src, shapes, eng.id, 255, 2)
    with pytest.raises(ValueError, match="ingest: the trim margin is -1; it must be >= 0"):
        torch.ops.texocr.ingest_trim_views(bufs, src, shapes, eng.id, 127, -1)
    with pytest.raises(ValueError, match=r"ingest: the trim level is -2"):
        small.model.ingest([good], trim=(-2, 2))
    with pytest.raises(ValueError, match="trim and regions"):
        small.model.ingest([good], trim=(127, 2), regions=[[0, 0, 4, 4]])
    with pytest.raises(ValueError, match=r"ingest: image 1 has the view 17x34 at \(0, 0\), which reaches outside the image's 17x33"):
        small.model.ingest([good, _white(17, 33, 1)], regions=[[0, 0, 20, 40], [0, 0, 17, 34]])
    with pytest.raises(ValueError, match=r"ingest: image 0 has the view 0x4 at \(3, 3\); both sides must be >= 1"):
        small.model.ingest([good], regions=[[3, 3, 0, 4]])
    with pytest.raises(ValueError, match=r"ingest: image 0 has the view -5x-5 at \(3, 3\); both sides must be >= 1"):
        small.model.ingest([good], fit=True, regions=[[3, 3, -5, -5]])
    with pytest.raises(ValueError, match="regions needs one"):
        small.model.ingest([good], regions=[[0, 0, 4, 4], [0, 0, 4, 4]])
    views = torch.tensor([[5, 5, 10, 25], [0, 0, 17, 33]], dtype=torch.int32)
    with pytest.raises(ValueError, match=r"image 1 is 17x33, 32x48 rounded up to multiples of 16: it does not fit the container's 32x32"):
        torch.ops.texocr.ingest_u8_view(bufs, src, shapes, views, eng.id, 1, 0, 0, 32, 32)
    with pytest.raises(ValueError, match="the fit target is 32x100; both sides must be positive multiples of 16"):
        torch.ops.texocr.ingest_u8_view(bufs, src, shapes, views, eng.id, 1, 32, 100, 32, 48)
    with pytest.raises(ValueError, match=r"image 1: 17x34x1 bytes from offset \d+ reach beyond bufs\[0\]"):      # the bound check stays on the full image
        torch.ops.texocr.ingest_u8_view(bufs, src, torch.tensor([[20, 40, 3], [17, 34, 1]], dtype=torch.int32), views, eng.id, 1, 0, 0, 32, 48)
    # ... and the engine is as it was
    got = torch.ops.texocr.ingest_trim_views(bufs, src, shapes, eng.id, 127, 2)
    assert got.tolist() == [[3, 3, 14, 29], [0, 0, 17, 33]]
    box, sizes = torch.ops.texocr.ingest_u8_view(bufs, src, shapes, got, eng.id, 1, 0, 0, 32, 48)
    assert sizes.tolist() == [[16, 32], [32, 48]] and float(box[0, 0, 2, 2]) == 1.0


# ---- 7. the torch-free route -----------------------------------------------------------------------------------------------------------------
def test_torch_free_c_program_matches_the_python_path(tmp_path):
    """examples/ingest_trim_tiny.c: plain C + the HIP runtime API: txo_ingest_trim_views + txo_ingest_box + txo_ingest_u8_view +
    txo_generate_ragged, then regions of one page; it checks itself against the host, and what it fed and got equals pack_u8(trim=)"""
    import subprocess
    import sys
    from texocr_amd import build as b, ops
    from texocr_amd.config import Dims
    from texocr_amd.model import model_from_dims
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = b.build_example(verbose=False, name="ingest_trim_tiny")
    blob, dump = str(tmp_path / "tiny.bin"), str(tmp_path / "dump.bin")
    subprocess.run([sys.executable, os.path.join(root, "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob, dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for frag in ("equal the rule on the host", "equals the host crop and preprocessing bit for bit", "equal the host container's",
                 "equals the host crops bit for bit", "level 255 -> -1 (ingest: the trim level is 255", "a view beyond its image -> -1 (ingest: image 1 has the view"):
        assert frag in r.stdout, (frag, r.stdout)
    raw = open(dump, "rb").read()
    B, C_, Hc, Wc = np.frombuffer(raw, np.int32, 4, 0).tolist()
    at = 16
    shapes = np.frombuffer(raw, np.int32, 3 * B, at).reshape(B, 3); at += 12 * B
    views = np.frombuffer(raw, np.int32, 4 * B, at).reshape(B, 4); at += 16 * B
    sizes = np.frombuffer(raw, np.int32, 2 * B, at).reshape(B, 2); at += 8 * B
    offsets = np.frombuffer(raw, np.int64, B, at); at += 8 * B
    total = int(np.frombuffer(raw, np.int64, 1, at)[0]); at += 8
    pix = np.frombuffer(raw, np.uint8, total, at); at += total
    box = np.frombuffer(raw, np.float32, B * C_ * Hc * Wc, at).reshape(B, C_, Hc, Wc)
    assert at + box.nbytes == len(raw) and B == 3
    arrs = [pix[o:o + h * w * ch].reshape((h, w) if ch == 1 else (h, w, ch)) for o, (h, w, ch) in zip(offsets.tolist(), shapes.tolist())]
    assert any(h > 64 or w > 64 for h, w, _ in shapes.tolist()) and int(sizes.max()) <= 64       # beyond the tiny canvas; its ink is not
    meta = json.load(open(os.path.join(GOLDEN, "tiny.json")))
    model = model_from_dims(Dims(**meta["dims"]), dtype="fp32", max_batch=3)
    with knobs(TXO_DEBUG_POISON=1):
        got = ops.pack_u8(arrs, C_, DEV, engine=model._engine.id, trim=(127, 2))
    assert got.views.tolist() == views.tolist() == [list(trim_ref.view(a, 127, 2)) for a in arrs]
    assert got.sizes.tolist() == sizes.tolist() and tuple(got.box.shape) == box.shape
    assert torch.equal(got.box.cpu(), torch.from_numpy(box.copy()))
