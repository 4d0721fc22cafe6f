"""GPU tests of the decode session's transitions (texocr_amd/csrc/session.h: Session, ImageBatch): what one call leaves behind must
not reach the next.  A sequence of calls on ONE engine gives, call by call, bit-identical results -- tokens, logits, scores and the
TXO_Q_LAST_* answers -- to the same call made on a freshly built engine with the same weights (fp32; torch.equal, no tolerance: both
sides run the same kernels on the same operands).  Captured step graphs are compared with eager launches the same way."""
import pytest
import torch

from gpu_harness import SHAPE_CASES, STOP_DIMS, STOP_ENV, build, knobs, on_path, rgb_images, stop_case
from texocr_amd import _lib, ops, synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_LATENT, Q_LAST_PERSISTENT, Q_LAST_RAGGED, Q_LAST_ROW_RANGES

pytestmark = pytest.mark.gpu

QUERIES = (Q_LAST_PERSISTENT, Q_LAST_RAGGED, Q_LAST_LATENT, Q_LAST_ROW_RANGES)
SESSION_QUERIES = (2,)             # of QUERIES: answered from the open session; the others are results of the last generate


def _sized_images(sizes, seed):
    return [torch.from_numpy(synth.synth_images(1, 3, h, w, seed=seed + i))[0].cuda() for i, (h, w) in enumerate(sizes)]


def _answer(m, call):
    """(the call's tensors, the engine's TXO_Q_LAST_* answers behind it)"""
    out = call(m)
    torch.cuda.synchronize()
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [o.clone() for o in out], [m._engine.query(q) for q in QUERIES]


def _assert_sequence_equals_fresh_engines(d, sd, calls, max_batch, env=None, no_generate=()):
    """every call of `calls` [(name, fn(m))] on ONE engine, in order, against the same call on an engine built for it alone.
    `no_generate`: names of calls that decode no batch of their own -- behind them the results of the last generate still stand."""
    _, _, one = build(d, sd=sd, max_batch=max_batch, env=env)
    for name, call in calls:
        before_q = [one._engine.query(q) for q in QUERIES]
        got, got_q = _answer(one, call)
        _, _, fresh = build(d, sd=sd, max_batch=max_batch, env=env)
        want, want_q = _answer(fresh, call)
        assert len(got) == len(want), name
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(g, w), f"{name}: output {i} differs from a fresh engine's"
        if name in no_generate:
            want_q = [w if i in SESSION_QUERIES else b for i, (w, b) in enumerate(zip(want_q, before_q))]
        assert got_q == want_q, f"{name}: TXO_Q_LAST_* {got_q} on the used engine, expected {want_q}"
    return one


def _score_c_abi(m, img, trg, mask8):
    eng = m._engine
    eng._ensure()
    B, Cc, H, W = img.shape
    L = trg.shape[1]
    logp = torch.full((B, L - 1), float("nan"), device="cuda")
    top1 = torch.full((B, L - 1), -7, device="cuda", dtype=torch.int64)
    top1_logp = torch.full((B, L - 1), float("nan"), device="cuda")
    with torch.cuda.device(eng.device):
        _lib.check(eng.lib.txo_score(eng.handle, img.data_ptr(), B, Cc, H, W, trg.data_ptr(), mask8.data_ptr(), L, logp.data_ptr(),
                                     top1.data_ptr(), top1_logp.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return logp, top1, top1_logp


def test_call_sequence_equals_fresh_engines_width_256():
    """(a) width 256 / 8 heads (the persistent launch exists): persistent generate, beam search, ragged generate, txo_score with a mask,
    decode_begin + two steps, generate with launches, generate with logits, the first generate again"""
    d = SHAPE_CASES["calib256"][0]
    sd = synth.synth_state_dict(d, 3)
    x = rgb_images(3, 48, 80, seed=9).cuda()
    ragged = _sized_images([(32, 32), (48, 96), (16, 64)], 40)
    gen = torch.Generator().manual_seed(5)
    trg = torch.randint(0, d.vocab - 3, (3, 7), generator=gen).cuda()
    trg[:, 0] = d.bos
    mask8 = torch.ones((3, 7), dtype=torch.uint8)
    mask8[0, 5:] = 0
    mask8[2, 3:] = 0
    mask8 = mask8.cuda()

    def steps(m):
        eng = m._engine
        eng.decode_begin(m.encoder(x))
        lg0, t0 = eng.decode_step(0, torch.full((3,), d.bos, dtype=torch.int64, device="cuda"))
        lg1, t1 = eng.decode_step(1, t0)
        return lg0, t0, lg1, t1

    first = ("generate, persistent launch", lambda m: on_path(m, True, lambda: m.generate(x, 12)))
    calls = [first,
             ("generate_beam, 2 beams", lambda m: m.generate(x, 12, beam=2, return_beams=True)),
             ("generate_ragged", lambda m: m.generate_ragged(ragged, 12)),
             ("txo_score with a mask", lambda m: _score_c_abi(m, x, trg, mask8)),
             ("decode_begin + two decode_steps", steps),
             ("generate, launches", lambda m: on_path(m, False, lambda: m.generate(x, 12))),
             ("generate with logits", lambda m: m.generate(x, 12, return_logits=True)),
             ("the first generate again", first[1])]
    _assert_sequence_equals_fresh_engines(d, sd, calls, max_batch=8, no_generate=("txo_score with a mask", "decode_begin + two decode_steps"))


def test_call_sequence_behind_a_compacted_row_stop_generate():
    """(b) a stop='row' generate that compacts its rows, then a plain and a ragged generate on the same engine; the ragged generate
    closes its session, so a txo_decode_step behind it is refused (TXO_E_STATE) until a new txo_decode_begin"""
    d, sd, img = stop_case(rows=40)
    assert d is STOP_DIMS
    x = img.cuda()
    ragged = _sized_images([(32, 48), (16, 64), (64, 32), (48, 48)], 70)

    def row_stop(m):
        t = m.generate(x, d.max_len, stop="row")
        assert m._engine.query(Q_LAST_COMPACTIONS) > 0          # (else the case is vacuous)
        return t

    calls = [("generate, stop='row'", row_stop),
             ("generate", lambda m: m.generate(x, d.max_len)),
             ("generate_ragged", lambda m: m.generate_ragged(ragged, d.max_len))]
    one = _assert_sequence_equals_fresh_engines(d, sd, calls, max_batch=40, env=STOP_ENV)
    eng = one._engine
    nxt = torch.empty((4,), dtype=torch.int64, device="cuda")
    with torch.cuda.device(eng.device):
        rc = eng.lib.txo_decode_step(eng.handle, None, 0, None, nxt.data_ptr(), None)
    assert rc == _lib.TXO_E_STATE and eng.lib.txo_last_error().decode() == "txo_decode_begin has not been called"


def test_replayed_graphs_fixed_ragged_fixed_equal_eager():
    """(c) TXO_GRAPH=1 at 2 images: fixed, ragged, fixed on one engine equal the eager launches.  The ragged batch has the fixed one's
    rows and slot stride (16 keys), so its captured step differs from the fixed-shape one in the ragged form alone."""
    d = SHAPE_CASES["w128"][0]
    sd = synth.synth_state_dict(d, 3)
    x = rgb_images(2, 48, 80, seed=9).cuda()
    ragged = _sized_images([(48, 80), (16, 32)], 40)
    assert int(ops.ragged_tokens(ops.pack_ragged(ragged)[1]).max()) == 1 + 3 * 5
    _, _, eager = build(d, sd=sd, max_batch=2)
    with knobs(TXO_GRAPH=0):
        want_fixed, want_ragged = eager.generate(x, 12), eager.generate_ragged(ragged, 12)
    _, _, m = build(d, sd=sd, max_batch=2)
    with knobs(TXO_GRAPH=1):
        got = [m.generate(x, 12), m.generate_ragged(ragged, 12), m.generate(x, 12)]
        assert m._engine.query(Q_LAST_PERSISTENT) == 0
    for name, g, w in zip(("fixed", "ragged", "fixed again"), got, (want_fixed, want_ragged, want_fixed)):
        assert torch.equal(g, w), f"replayed step graph, {name}: differs from eager launches"


# ---- the binding's record of the session (texocr_amd/ops.py: Session) against the engine's --------------------------------------------
def _tiny_model():
    d = STOP_DIMS
    _, _, m = build(d, sd=synth.synth_state_dict(d, 7), max_batch=8)
    return d, m, m._engine


def test_beam_search_leaves_the_bindings_row_count_equal_to_the_engines():
    """decode_begin on 2 images, a beam search on 3: the engine is left with an open session of one row per image (engine.hip, struct
    Rows in generate_beam), so a decode_step behind it writes 3 rows of logits and tokens -- the binding must size them for 3, not 2"""
    d, m, eng = _tiny_model()
    x2, x3 = rgb_images(2, 32, 48, seed=9).cuda(), rgb_images(3, 32, 48, seed=10).cuda()
    eng.decode_begin(m.encoder(x2))
    m.generate(x3, 8, beam=2)
    bos = torch.full((3,), d.bos, dtype=torch.int64, device="cuda")
    logits, tok = eng.decode_step(0, bos)
    torch.cuda.synchronize()
    assert logits.shape == (3, d.vocab) and tok.shape == (3,)
    assert int(tok.min()) >= 0 and int(tok.max()) < d.vocab
    with pytest.raises(ValueError, match="batch does not match"):
        torch.ops.texocr.decode_step(bos[:2].contiguous(), eng.id, 0, 2, True)


def test_ragged_generate_closes_the_bindings_session_too():
    """behind generate_ragged the engine has no session; the binding knows, and refuses the session's operators itself"""
    d, m, eng = _tiny_model()
    m.generate_ragged(_sized_images([(32, 48), (16, 64)], 70), 8)
    nxt = torch.empty((2,), dtype=torch.int64, device="cuda")
    with torch.cuda.device(eng.device):                                    # the engine's own word on it, and a known last error
        assert eng.lib.txo_decode_step(eng.handle, None, 0, None, nxt.data_ptr(), None) == _lib.TXO_E_STATE
    said = eng.lib.txo_last_error()
    assert said == b"txo_decode_begin has not been called"
    bos = torch.full((2,), d.bos, dtype=torch.int64, device="cuda")
    mask = torch.ones((2, 4), dtype=torch.bool, device="cuda")
    mask[0, 3] = False
    for call in (lambda: eng.decode_step(0, bos), lambda: eng.decode_prefill(bos[:, None].contiguous()), lambda: eng.set_key_mask(mask)):
        with pytest.raises(RuntimeError, match="needs a session started by"):
            call()
    assert eng.lib.txo_last_error() == said                                # none of the three reached the engine
    eng.decode_begin(m.encoder(rgb_images(2, 32, 48, seed=9).cuda()))
    logits, tok = eng.decode_step(0, bos)
    assert logits.shape == (2, d.vocab) and bool(torch.isfinite(logits).all()) and tok.shape == (2,)
