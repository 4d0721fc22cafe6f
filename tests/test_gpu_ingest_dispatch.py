"""What one ingest call puts on the stream, pinned with profiling on: every dispatch of an ingest kernel carries one pair of events
(txo_profile_read kind 4), so the count after a call is the number of kernels it launched -- the descriptor fill of the ink search and
the copies are not counted.  The container tests say WHAT is written; this one says in how many launches."""
import pytest
import torch

from test_gpu_ingest import _wrapper

# the fit target of every case, and what ops.fit_size makes of the three shapes under it
FIT = (32, 32)
FITTED = {(16, 16): (16, 16), (16, 64): (8, 32), (40, 1): (32, 1)}


def test_fitted_sizes_of_the_cases():
    """no GPU: 16x16 is not oversized, 16x64 shrinks along both axes, 40x1 keeps its width (no horizontal pass)"""
    from texocr_amd import ops
    for (h, w), want in FITTED.items():
        assert ops.fit_size(h, w, *FIT) == want


@pytest.mark.gpu
def test_dispatches_per_call(tmp_path):
    from texocr_amd import ops
    eng = _wrapper(tmp_path).model._engine
    g = torch.Generator().manual_seed(3)

    def img(h, w):
        return torch.randint(0, 256, (h, w), dtype=torch.uint8, generator=g).numpy()

    def pack(images, **kw):
        return lambda: ops.pack_u8(images, 1, "cuda", engine=eng.id, **kw)

    def trim_views():
        staged, dev, src, shapes = ops.plan_u8([img(16, 16), img(20, 36)])
        return torch.ops.texocr.ingest_trim_views([staged.cuda()] + dev, src, shapes, eng.id, 127, 2)

    try:
        for what, call, want in [
            ("plain", pack([img(16, 16), img(20, 36)]), 1),
            ("fit, nothing oversized: plain ingest's launch", pack([img(16, 16)], fit=FIT), 1),
            ("fit to 8x32: a horizontal pass and the fused vertical pass", pack([img(16, 64)], fit=FIT), 2),
            ("fit to 32x1: the width is kept, no horizontal pass", pack([img(40, 1)], fit=FIT), 1),
            ("ink search", trim_views, 1),
            ("a region narrower than its image: the pitched kernel", pack([img(24, 40)], regions=[(2, 3, 20, 30)]), 1),
        ]:
            eng.profile(1)                                         # (also forgets the events of the call before)
            call()
            torch.cuda.synchronize()
            assert eng.profile_read(4)[1] == want, what
    finally:
        eng.profile(0)
