"""What the generate family refuses, and in which order (include/texocr.h: the nine txo_generate* entries and the three beam searches).

Every entry is called through the C ABI on a tiny engine -- width 64, one layer, max_batch 4, max_len 8, images of 16 x 32 and 32 x 48 -- with
one thing wrong, then with two things wrong that are adjacent in the entry's order of checks: the return code and the whole message are
asserted, and the order with them (of two refusals that apply, the earlier one answers).  The three families check in different orders:

  from BOS (txo_generate, _logp, _from_enc, _from_enc_logp):  null argument -> max_len -> window -> batch
  ragged   (txo_generate_ragged, _logp):                      null argument -> ragged refusals -> max_len -> ragged forward -> window -> batch
  prompted (txo_generate_prefix, _from_enc, _ragged):         null argument -> [ragged refusals] -> max_len -> B -> P -> prefix_len[b] -> table
                                                              -> workspace -> batch
  beam     (txo_generate_beam, txo_beam_search, _ragged):     null argument -> beams -> max_len -> rows -> [out -> length_alpha] -> batch

The expected texts are written out here, as the engine's source has them.  Behind a refused call TXO_Q_LAST_COMPACTIONS and TXO_Q_LAST_RAGGED
are read: the entries from BOS, the prompted ones and txo_beam_search reset both also when they refuse; txo_generate_ragged / _logp set them
only once the batch is accepted, and txo_generate_beam never touches them.  Almost every case returns before any launch.

The last test pins what the nine entries share: on one input their tokens (and log-probabilities) are bit for bit the same wherever two of them
mean the same decode."""
import ctypes as C

import pytest
import torch

from gpu_harness import build, rgb_images
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_RAGGED, TXO_E_INVALID, TXO_E_STATE, TxoBeamOut
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

TINY = Dims(canvas=32, canvas_w=48, in_channels=3, embed_dim=64, enc_heads=1, enc_layers=1, dec_heads=1, dec_layers=1, enc_exp=1, dec_exp=1,
            vocab=16, max_len=8, bos=14, eos=13, pad=15)

# ---- the texts ---------------------------------------------------------------------------------------------------------------------
NOT_READY = "weights not finalized"
NULL = "null argument"
NULL_PREFIX = "prefix decode: null argument"
MAX_LEN = "max_len must be >= 1"
WINDOW = ("max_len exceeds the decoder's max_length and the sliding window's multi-position forward needs a vocabulary "
          "size that is a multiple of 8 and max_length <= max_batch * max_tokens (use decoder.generate's stepwise loop)")
CHANNELS = "image channel count does not match in_channels"
SIZE = "image height/width must be positive multiples of 16"
BATCH = "batch exceeds engine max_batch"
TOKENS = "token count exceeds engine max_tokens"
RAG_LATENT = "ragged batches: the latent cross-attention form (TXO_LATENT=1) is not supported; a ragged decode runs in the K/V form"
RAG_FORWARD = "ragged batches: max_len exceeds the decoder's max_length (the sliding window of a ragged batch needs txo_set_ragged_forward(e, 1))"
RAG_WINDOW = ("ragged batches: max_len exceeds the decoder's max_length and the sliding window's multi-position forward needs a "
              "vocabulary size that is a multiple of 8 and max_length <= max_batch * max_tokens")
RAG_BATCH = "ragged batches: batch exceeds engine max_batch"
RAG_IMAGE = "ragged batches: image 1 height/width must be positive multiples of 16"
P_MAX_LEN = "prefix decode: max_len must be >= 1"
P_BATCH = "prefix decode: batch exceeds engine max_batch"
P_COLUMNS = "prefix decode: the prefix needs at least one column"
P_LEN1 = "prefix decode: prefix_len[1] must be in [1, P]"
P_LEN0 = "prefix decode: prefix_len[0] must be in [1, P]"
P_TABLE = "prefix decode: the longest prefix - 1 + max_len exceeds the decoder's max_length (a prompted decode does not slide the window)"
P_WORKSPACE = "prefix decode: the shortest prefix does not fit the multi-position pass's workspace (max_batch * max_tokens rows)"
BEAMS = "beams must be in [1, 8]"
BEAM_MAX_LEN = "max_len exceeds the decoder's max_length (a KV cache cannot slide the window)"
BEAM_ROWS = "images * beams exceeds engine max_batch"
BEAM_OUT = "beam search: null out / out->tokens"
BEAM_ALPHA = "beam search: length_alpha must be finite and >= 0"

FROM_BOS = ("txo_generate", "txo_generate_logp", "txo_generate_from_enc", "txo_generate_from_enc_logp")
RAGGED = ("txo_generate_ragged", "txo_generate_ragged_logp")
PROMPTED = ("txo_generate_prefix", "txo_generate_prefix_from_enc", "txo_generate_prefix_ragged")
BEAM = ("txo_generate_beam", "txo_beam_search", "txo_beam_search_ragged")


# ---- engines: built once for the module, only ever asked to refuse (and for two small decodes) ----------------------------------------
class Rig:
    """one engine and device buffers large enough for every call made on it; B images of H x W (ragged: that container, `sizes` inside it)"""

    def __init__(self, max_batch=4, max_tokens=0, sizes=((16, 32), (32, 48)), weights=True, **kw):
        self.d, _, self.m = build(TINY, seed=3, max_batch=max_batch, max_tokens=max_tokens, **kw)
        self.eng = self.m._engine
        if weights:
            self.eng._ensure()                                                    # (the module uploads its weights before the first call otherwise)
        self.B = len(sizes)
        self.H, self.W = max(h for h, _ in sizes), max(w for _, w in sizes)
        self.N = 1 + (self.H // 16) * (self.W // 16)
        self.sizes = sizes
        self.img = rgb_images(8, self.H, self.W, seed=5).cuda()                 # (8 slots: the cases with too many images point at real memory)
        self.enc = torch.zeros((8, 8, TINY.embed_dim), device="cuda")
        self.toks = torch.zeros((64, 16), dtype=torch.int64, device="cuda")
        self.f32 = [torch.zeros((64, 16 * TINY.vocab), device="cuda") for _ in range(3)]
        self.prefix = torch.full((8, 8), TINY.bos, dtype=torch.int64, device="cuda")

    def query(self, what):
        return self.eng.query(what)

    def call(self, name, null=(), **o):
        """entry `name` with valid arguments except for what `o` overrides and the pointers `null` names -> (return code, message)"""
        p = dict(B=self.B, C=3, H=self.H, W=self.W, N=self.N, max_len=4, eos=-1, P=2, lens=None, beams=2, alpha=0.0, sizes=self.sizes, out=True)
        p.update(o)
        ptr = lambda key, t: None if key in null else t.data_ptr()
        sizes = None if "sizes" in null else (C.c_int32 * (2 * len(p["sizes"])))(*[v for hw in p["sizes"] for v in hw])
        lens = None if p["lens"] is None else (C.c_int32 * len(p["lens"]))(*p["lens"])
        n = C.c_int32(0)
        img = (ptr("img", self.img), p["B"], p["C"], p["H"], p["W"])
        src = (ptr("enc", self.enc), p["B"], p["N"]) if "from_enc" in name else img + (sizes,) if "ragged" in name else img
        toks, logits, logp, plogp = ptr("tokens", self.toks), ptr("logits", self.f32[0]), ptr("logp", self.f32[1]), ptr("prefix_logp", self.f32[2])
        if name in PROMPTED:
            args = src + (ptr("prefix", self.prefix), p["P"], lens, p["max_len"], p["eos"], toks, C.byref(n), logp, plogp)
        elif name in RAGGED:
            args = src + (p["max_len"], p["eos"], toks, C.byref(n)) + ((logp,) if name.endswith("_logp") else ())
        elif name in FROM_BOS:
            args = src + (p["max_len"], p["eos"], toks, C.byref(n), logits) + ((logp,) if name.endswith("_logp") else ())
        elif name == "txo_generate_beam":
            args = src + (p["beams"], p["max_len"], p["eos"], toks, logits, None, C.byref(n))
        else:
            out = TxoBeamOut(ptr("out_tokens", self.toks), logits, None, None, p["alpha"])
            args = src + (p["beams"], p["max_len"], p["eos"], C.byref(out) if p["out"] else None, C.byref(n))
        rc = getattr(self.eng.lib, name)(None if "engine" in null else self.eng.handle, *args, None)
        torch.cuda.synchronize()
        return rc, self.eng.lib.txo_last_error().decode()

    def refuses(self, name, text, code=TXO_E_INVALID, **kw):
        assert self.call(name, **kw) == (code, text), (name, kw)


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.fixture(scope="module")
def small():
    """max_batch * max_tokens = 3 < max_len = 8: the window's second precondition fails, and a prefix of five columns does not fit the workspace"""
    return Rig(max_batch=1, max_tokens=3, sizes=((16, 32),))


@pytest.fixture(scope="module")
def latent():
    """TXO_LATENT=1: what every ragged entry refuses first"""
    return Rig(latent=1)


@pytest.fixture(scope="module")
def unloaded():
    """an engine without weights: the first thing the ragged refusals and the batch checks look at"""
    return Rig(weights=False)


def _img(name):
    return "from_enc" not in name


# ---- null arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FROM_BOS + RAGGED + PROMPTED + BEAM)
def test_null_arguments(rig, name):
    text = NULL_PREFIX if name in PROMPTED else NULL
    required = ["engine", "img" if _img(name) else "enc"]
    if name not in ("txo_beam_search", "txo_beam_search_ragged"):
        required.append("tokens")
    if "ragged" in name:
        required.append("sizes")
    if name in PROMPTED:
        required.append("prefix")
    elif name.endswith("_logp"):
        required.append("logp")
    for what in required:
        rig.refuses(name, text, null=(what,))
    rig.refuses(name, text, null=(required[1],), max_len=0)                      # ... and it answers before anything else is looked at
    rig.refuses(name, text, null=(required[1],), beams=0, P=0)


# ---- from BOS: max_len -> window -> batch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FROM_BOS)
def test_from_bos(rig, small, unloaded, name):
    unloaded.refuses(name, NOT_READY, code=TXO_E_STATE)
    unloaded.refuses(name, MAX_LEN, max_len=0)                                    # max_len before batch (whose first look is at the weights)
    batch = dict(C=1) if _img(name) else dict(B=5)
    batch_text = CHANNELS if _img(name) else BATCH
    rig.refuses(name, MAX_LEN, max_len=0)
    small.refuses(name, WINDOW, max_len=9)
    rig.refuses(name, batch_text, **batch)
    if _img(name):
        rig.refuses(name, SIZE, H=24)
        rig.refuses(name, BATCH, B=5)
        small.refuses(name, TOKENS, W=48)
    else:
        rig.refuses(name, TOKENS, N=8)
    rig.refuses(name, MAX_LEN, max_len=0, **batch)                                # max_len before batch (max_len and window exclude each other)
    small.refuses(name, WINDOW, max_len=9, **(dict(C=1) if _img(name) else dict(B=5)))   # window before batch
    assert rig.call(name, max_len=9)[0] == 0                                      # (this engine slides the window: 9 > max_len = 8 is accepted)


# ---- ragged: ragged refusals -> max_len -> ragged forward -> window -> batch ------------------------------------------------------------
@pytest.mark.parametrize("name", RAGGED)
def test_ragged(rig, small, latent, unloaded, name):
    unloaded.refuses(name, NOT_READY, code=TXO_E_STATE, max_len=0)                # ragged refusals (the weights first) before max_len
    latent.refuses(name, RAG_LATENT)
    rig.refuses(name, MAX_LEN, max_len=0)
    rig.refuses(name, RAG_FORWARD, max_len=9)
    rig.refuses(name, CHANNELS, C=1)
    rig.refuses(name, RAG_BATCH, B=5, sizes=((16, 16),) * 5)
    rig.refuses(name, RAG_IMAGE, sizes=((16, 32), (24, 48)))
    latent.refuses(name, RAG_LATENT, max_len=0)                                   # ragged refusals before max_len
    rig.refuses(name, MAX_LEN, max_len=0, C=1)                                    # max_len before batch
    rig.refuses(name, RAG_FORWARD, max_len=9, C=1)                                # ragged forward before batch
    small.refuses(name, RAG_FORWARD, max_len=9)                                   # ... and before window
    assert small.eng.lib.txo_set_ragged_forward(small.eng.handle, 1) == 0
    try:
        small.refuses(name, RAG_WINDOW, max_len=9)
        small.refuses(name, RAG_WINDOW, max_len=9, C=1)                           # window before batch
    finally:
        assert small.eng.lib.txo_set_ragged_forward(small.eng.handle, 0) == 0


# ---- prompted: [ragged refusals] -> max_len -> B -> P -> prefix_len[b] -> table -> workspace -> batch -----------------------------------
@pytest.mark.parametrize("name", PROMPTED)
def test_prompted(rig, small, latent, unloaded, name):
    unloaded.refuses(name, NOT_READY, code=TXO_E_STATE)
    unloaded.refuses(name, NOT_READY if name.endswith("_ragged") else P_MAX_LEN, code=TXO_E_STATE if name.endswith("_ragged") else TXO_E_INVALID,
                     max_len=0)
    batch = dict(C=1) if _img(name) else dict(N=8)
    batch_text = CHANNELS if _img(name) else TOKENS
    five = dict(B=5, sizes=((16, 16),) * 5)
    rig.refuses(name, P_MAX_LEN, max_len=0)
    rig.refuses(name, P_BATCH, **five)
    rig.refuses(name, P_BATCH, B=0, sizes=())
    rig.refuses(name, P_COLUMNS, P=0)
    rig.refuses(name, P_LEN1, lens=(1, 0))
    rig.refuses(name, P_LEN1, lens=(2, 3))
    rig.refuses(name, P_TABLE, P=4, max_len=6)
    rig.refuses(name, P_TABLE, P=4, lens=(1, 4), max_len=6)                       # (the LONGEST prefix counts)
    small.refuses(name, P_WORKSPACE, P=5, max_len=4)
    small.refuses(name, P_WORKSPACE, P=6, lens=(5,), max_len=3)
    rig.refuses(name, batch_text, **batch)
    if name.endswith("_ragged"):
        latent.refuses(name, RAG_LATENT)
        latent.refuses(name, RAG_LATENT, max_len=0)                               # ragged refusals before max_len
        rig.refuses(name, RAG_IMAGE, sizes=((16, 32), (24, 48)))
    else:
        latent.refuses(name, P_MAX_LEN, max_len=0)                                # (nothing ragged about it)
    rig.refuses(name, P_MAX_LEN, max_len=0, **five)                               # max_len before B
    rig.refuses(name, P_BATCH, P=0, **five)                                       # B before P
    rig.refuses(name, P_COLUMNS, P=0, lens=(0, 0))                                # P before prefix_len
    rig.refuses(name, P_LEN0, P=4, lens=(0, 4), max_len=6)                        # prefix_len before table
    small.refuses(name, P_TABLE, P=5, max_len=5)                                  # table before workspace
    small.refuses(name, P_WORKSPACE, P=5, max_len=4, **batch)                     # workspace before batch


# ---- beam: beams -> max_len -> rows -> [out -> length_alpha] -> batch -------------------------------------------------------------------
@pytest.mark.parametrize("name", BEAM)
def test_beam(rig, latent, name):
    for beams in (0, 9):
        rig.refuses(name, BEAMS, beams=beams)
    for max_len in (0, 9):
        rig.refuses(name, BEAM_MAX_LEN, max_len=max_len)
    rig.refuses(name, BEAM_ROWS, beams=3)
    rig.refuses(name, BEAM_ROWS, B=0, sizes=())
    rig.refuses(name, CHANNELS, C=1)
    rig.refuses(name, BEAMS, beams=0, max_len=0)                                  # beams before max_len
    rig.refuses(name, BEAM_MAX_LEN, max_len=9, beams=3)                           # max_len before rows
    if name == "txo_generate_beam":
        rig.refuses(name, BEAM_ROWS, beams=3, C=1)                                # rows before batch
        return
    rig.refuses(name, BEAM_OUT, out=False)
    rig.refuses(name, BEAM_OUT, null=("out_tokens",))
    for alpha in (-0.5, float("nan"), float("inf")):
        rig.refuses(name, BEAM_ALPHA, alpha=alpha)
    rig.refuses(name, BEAM_ROWS, beams=3, out=False)                              # rows before out
    rig.refuses(name, BEAM_OUT, out=False, alpha=-1.0)                            # (out before length_alpha: there is no alpha without it)
    rig.refuses(name, BEAM_ALPHA, alpha=-1.0, C=1)                                # length_alpha before batch
    if name.endswith("_ragged"):
        latent.refuses(name, RAG_LATENT)
        latent.refuses(name, BEAM_ALPHA, alpha=-1.0)                              # ... which is where the ragged refusals stand
        rig.refuses(name, RAG_IMAGE, sizes=((16, 32), (24, 48)))


# ---- what a query sees behind a refused call --------------------------------------------------------------------------------------------
def test_queries_behind_a_refusal(rig):
    def ragged_decode():
        assert rig.call("txo_generate_ragged")[0] == 0
        assert (rig.query(Q_LAST_RAGGED), rig.query(Q_LAST_COMPACTIONS)) == (1, 0)

    # reset, also by the refusal: the entries from BOS, the prompted ones, txo_beam_search / _ragged
    for name in FROM_BOS + PROMPTED:
        ragged_decode()
        rig.refuses(name, P_MAX_LEN if name in PROMPTED else MAX_LEN, max_len=0)
        assert (rig.query(Q_LAST_RAGGED), rig.query(Q_LAST_COMPACTIONS)) == (0, 0), name
    for name in ("txo_beam_search", "txo_beam_search_ragged"):
        ragged_decode()
        rig.refuses(name, BEAMS, beams=0)
        assert rig.query(Q_LAST_RAGGED) == 0, name
    # left as they were: txo_generate_beam always (refused or not), txo_generate_ragged / _logp when they refuse; a null argument anywhere
    ragged_decode()
    rig.refuses("txo_generate_beam", BEAMS, beams=0)
    assert rig.query(Q_LAST_RAGGED) == 1
    assert rig.call("txo_generate_beam")[0] == 0
    assert rig.query(Q_LAST_RAGGED) == 1
    for name in RAGGED:
        rig.refuses(name, MAX_LEN, max_len=0)
        rig.refuses(name, CHANNELS, C=1)
        assert rig.query(Q_LAST_RAGGED) == 1, name
    rig.refuses("txo_generate", NULL, null=("tokens",))
    assert rig.query(Q_LAST_RAGGED) == 1
    assert rig.call("txo_generate")[0] == 0
    assert rig.query(Q_LAST_RAGGED) == 0
    for name in RAGGED:                                                           # ... so behind a fixed batch they still say "not ragged"
        rig.refuses(name, MAX_LEN, max_len=0)
        assert rig.query(Q_LAST_RAGGED) == 0, name


# ---- the nine entries agree ---------------------------------------------------------------------------------------------------------------
def test_the_nine_entries_agree():
    """fp32, two images of 32 x 48, eight positions without an eos test: images vs. their encoder rows, with and without logp, a ragged batch
    of equal sizes vs. the fixed batch, a prefix of the BOS column vs. none -- the same tokens bit for bit, and the same logp wherever asked"""
    r = Rig(sizes=((32, 48), (32, 48)))
    enc = r.m.encoder(r.img[:2])
    assert tuple(enc.shape) == (2, r.N, TINY.embed_dim)
    r.enc[:2, :r.N] = enc
    r.enc = r.enc[:, :r.N].contiguous()
    got = {}
    for name in FROM_BOS + RAGGED + PROMPTED:
        r.toks.fill_(-7)
        r.f32[1].fill_(float("nan"))
        assert r.call(name, max_len=8, P=1)[0] == 0, name
        got[name] = (r.toks.view(-1)[:16].view(2, 8).clone(), r.f32[1].view(-1)[:16].view(2, 8).clone())   # (rows are max_len apart)
    toks, logp = got["txo_generate_logp"]
    assert int(toks.min()) >= 0 and int(toks.max()) < TINY.vocab and bool(torch.isfinite(logp).all())
    for name, (t, lp) in got.items():
        assert torch.equal(t, toks), name
        if name.endswith("_logp") or name in PROMPTED:
            assert torch.equal(lp, logp), name
