"""GPU tests of beam search (BASELINE config 5 asks for it; the reference has none, SURVEY D3: a build extension).

Convention: parity is anchored at beams=1 == greedy and at the oracle's independent CPU restatement of the same definition (tokens
exact, scores within 2e-3 in fp32); one row range against two bit for bit.  Beyond the 24 positions over which float64 and fp32 still
decide every candidate alike, every step is pinned on its own: tests/beam_ref.py replays it in float64 from the engine's state before
it (the test_beam_replay_* tests: the whole positional table, every beam count, both selection paths, every attention form)."""
import dataclasses

import numpy as np
import pytest
import torch

import beam_ref as br
import ref64
from gpu_harness import BF16_BOUND, SHAPE_CASES, build, knobs, oracle, rgb_images, teacher_forced_stepwise
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_LATENT, Q_LAST_LATENT_SELF, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("latent", [None, 1], ids=["kv_form", "latent_form"])
@pytest.mark.parametrize("vocab", [1000, 1100], ids=["rows_in_registers", "general_path"])
def test_beam_search_extension(vocab, latent):
    """BASELINE config 5 asks for beam search; the reference has none, so parity is anchored at
    beams=1 == greedy, plus agreement with the oracle's independent CPU restatement of the same definition.
    Both forms of beam_select_kernel (csrc/step.h): an image's k rows in registers up to 1024 entries, the general path beyond."""
    cpu_ref = oracle()
    d = Dims(canvas=224, vocab=vocab)
    # latent_form: the cross attention against the raw encoder rows, an image's k beams as ONE row of k * heads heads (16 per tile)
    d, sd, m = build(d, seed=0, max_batch=12, latent=latent)
    img = torch.from_numpy(synth.synth_images(3, 3, 64, 96, seed=41))
    m.eos_token = None
    greedy = m.generate(img.cuda(), 24)
    assert torch.equal(m.generate(img.cuda(), 24, beam=1), greedy)
    assert m._engine.query(Q_LAST_LATENT) == (1 if latent else 0)
    sdt = cpu_ref.to_torch_sd(sd)
    enc = cpu_ref.encode(sdt, img)
    for k, eos in ((4, None), (3, int(greedy[0, 5]))):
        m.eos_token = eos
        toks, scores = m.generate(img.cuda(), 24, beam=k, return_beams=True)
        ref_t, ref_s = cpu_ref.beam_search_cached(sdt, enc, d.bos, eos, 24, k)
        assert toks.shape[:2] == (3, k) and toks.shape[2] == ref_t.shape[2]
        np.testing.assert_allclose(scores.cpu().numpy(), ref_s.numpy(), atol=2e-3)
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())                  # best first
        assert torch.equal(toks.cpu(), ref_t), (k, eos)
        best = m.generate(img.cuda(), 24, beam=k)
        assert torch.equal(best, toks[:, 0])
        assert torch.equal(m.generate(img.cuda(), 24, beam=k), best)          # deterministic
        # two row ranges on two streams (the default from 256 beam rows on): ranges are whole images, slots range-local -> the same bits
        with knobs(TXO_LANES=2):
            toks2, scores2 = m.generate(img.cuda(), 24, beam=k, return_beams=True)
            assert m._engine.query(Q_LAST_ROW_RANGES) == 2
        assert torch.equal(toks2, toks) and torch.equal(scores2, scores)
    with pytest.raises(ValueError):
        m.generate(img.cuda(), 24, beam=9)
    with pytest.raises(ValueError):
        m.generate(torch.rand(5, 3, 64, 96, device="cuda"), 24, beam=3)       # 15 rows > max_batch 12


def test_beam_search_two_row_ranges_at_300_rows_bit_identical_to_one():
    """From 256 beam rows on, beam search decodes two row ranges (whole images each) on two streams, in bf16 with the latent cross
    attention whose tiles take up to 16 heads = two beams of an image: same tokens and scores as ONE range."""
    d = Dims(canvas=224, max_len=16)
    _, _, m = build(d, seed=9, dtype="bf16", max_batch=300)
    img = torch.from_numpy(synth.synth_images(60, 3, 32, 64, seed=17)).cuda()
    m.eos_token = None
    t2, s2 = m.generate(img, 12, beam=5, return_beams=True)
    assert m._engine.query(Q_LAST_ROW_RANGES) == 2 and m._engine.query(Q_LAST_LATENT) == 1
    with knobs(TXO_LANES=1):
        t1, s1 = m.generate(img, 12, beam=5, return_beams=True)
        assert m._engine.query(Q_LAST_ROW_RANGES) == 1
    assert torch.equal(t1, t2) and torch.equal(s1, s2)
    # with an eos (the most frequent token of the best beams): finished beams repeat eos at no cost, the loop stops only when EVERY
    # range's beams are finished -- same length, same beams, same scores on one range and on two
    vals, counts = np.unique(t2[:, 0].cpu().numpy(), return_counts=True)
    m.eos_token = int(vals[counts.argmax()])
    e2 = m.generate(img, 12, beam=5, return_beams=True)
    with knobs(TXO_LANES=1):
        e1 = m.generate(img, 12, beam=5, return_beams=True)
    assert e1[0].shape == e2[0].shape and torch.equal(e1[0], e2[0]) and torch.equal(e1[1], e2[1])
    assert not torch.equal(e2[0], t2[:, :, :e2[0].shape[2]]) or e2[0].shape[2] < 12      # the eos changed something


# ---- every step replayed in float64 (tests/beam_ref.py) -------------------------------------------------------------------------------
# The pairs (n, n + 1): the first positions, the latent tile (16 keys), its wave count x 16 (64, 128), the 256-key pass of dec_attn and
# the last slot of the bf16 width-256 slot table, the end of a 300-position decode.
CHECKPOINTS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 299)

# bf16: eps = 2 x BEAM_LONG_BF16_BOUND (once for the logit, once for the log-sum-exp, as tests/test_gpu_score.py).  BF16_BOUND["logits"]
# was calibrated over 24 positions; at the lengths decoded here the engine's already pinned non-beam route (teacher_forced_stepwise,
# TXO_NET_STEPWISE=1) is measured on the beams' own prefixes, printed and asserted against the same bound, and where that route itself
# exceeds it the bound is 1.5 x its measured maximum.  Never calibrated on the beam route.
# Measured on MI355X: NOT YET -- no GPU run of these tests has been made; the constant stands at the 24-position bound (0.0557), and the
# plain route's assertion in _plain_route_error says at once whether 300 positions need the 1.5 x rule.  Put both figures here then.
BEAM_LONG_BF16_BOUND = BF16_BOUND["logits"]


def _long_dims(case="calib256", max_len=320, vocab=1000):
    return dataclasses.replace(SHAPE_CASES[case][0], max_len=max_len, vocab=vocab, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


class _Ref:
    """The float64 side of one set of weights: encoder rows of the images, and the log-probabilities after a prefix, kept per (image,
    prefix) -- forms that decode the same beams share them."""

    def __init__(self, d, sd, img):
        self.d, self.sd, self.img = d, sd, img
        self.s64 = ref64.sd64(sd)
        self.enc64 = ref64.encode(self.s64, img)
        self.kept = {}

    def logp(self, tokens):
        tokens = np.asarray(tokens, np.int64)
        B, k, n = tokens.shape
        want = [(b, tokens[b, j].tobytes()) for b in range(B) for j in range(k)]
        miss = sorted({w for w in want if w not in self.kept})
        if miss:
            rows = np.stack([np.frombuffer(p, np.int64) for _, p in miss]).reshape(len(miss), 1, n)
            enc = self.enc64[[b for b, _ in miss]]
            for key, lp in zip(miss, br.prefix_logp64(self.s64, enc, self.d.bos, rows)[:, 0]):
                self.kept[key] = lp
        return np.stack([self.kept[w] for w in want]).reshape(B, k, -1)


_REFS = {}


def _ref(d, images=4, bias_eos=0.0, dup_first=False):
    """one float64 reference per set of weights for the whole module"""
    key = (d, images, bias_eos, dup_first)
    if key not in _REFS:
        sd = synth.synth_state_dict(d, 3)
        img = rgb_images(images, 64, 64, 7)
        if bias_eos:
            b = sd["decoder.net.to_logits.bias"].copy()
            b[d.eos] += bias_eos
            sd["decoder.net.to_logits.bias"] = b
        if dup_first:
            # the greedy first token a of image 0 once more as a' = a + 1: the same logits row, bias and embedding -> a and a' are
            # equal candidates wherever one of them is one, and so are the beams that differ only in them
            s64 = ref64.sd64(sd)
            a = int(ref64.generate(s64, ref64.encode(s64, img[:1]), d.bos, None, 1)[0][0, 0])
            assert a + 1 < d.eos
            for name in ("decoder.net.to_logits.weight", "decoder.net.to_logits.bias", "decoder.net.token_embedding.weight"):
                w = sd[name].copy()
                w[a + 1] = w[a]
                sd[name] = w
        _REFS[key] = _Ref(d, sd, img)
        _REFS[key].first = a if dup_first else None
    return _REFS[key]


def _states(m, img, k, lengths):
    """{n: (tokens (B, k, n), scores (B, k))} of one decode per length"""
    out = {}
    for n in sorted(set(lengths)):
        t, s = m.generate(img, n, beam=k, return_beams=True)
        assert t.shape == (img.shape[0], k, n) and s.dtype == torch.float32
        out[n] = (t.cpu().numpy(), s.cpu().numpy())
    return out


def _eps_fp32(a, b):
    return br.eps_fp32(a[1], b[1])


def _eps_bf16(a, b):
    return 2 * BEAM_LONG_BF16_BOUND


def _replay(tag, ref, m, images, k, pairs, dtype="fp32", eos=None, check_form=None):
    """decodes at every length the pairs need and replays every pair; prints the maxima; returns (states, report)"""
    img = ref.img[:images].cuda()
    m.eos_token = eos
    pairs = list(pairs)
    states = _states(m, img, k, [n + d for n in pairs for d in (0, 1) if n + d > 0])
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    if check_form:
        check_form()
    enc = ref.enc64[:images]
    rep = br.replay_pairs(ref.s64, enc, ref.d.bos, eos, states, pairs, _eps_bf16 if dtype == "bf16" else _eps_fp32, logp_of=ref.logp)
    last = states[max(states)][1]
    eps = _eps_bf16(None, None) if dtype == "bf16" else br.eps_fp32(last)
    print(f"\nbeam replay {tag}: {rep.steps} steps up to position {max(states)}, k = {k}, {images} images, scores down to "
          f"{float(last[np.isfinite(last)].min()):.1f}: "
          f"max |score increment - float64 log-prob| {rep.inc_err:.3e} (eps <= {eps:.3e}), smallest selection slack {rep.slack:.3e} "
          f"(float64's own smallest margin {rep.gap:.1e}), bit-equal score pairs {rep.ties}")
    assert rep.steps == len(pairs)
    return states, rep


def _plain_route_error(tag, ref, m, images, k, state):
    """The engine's non-beam decode route on the beams' own prefixes (one row per beam), against float64: max |dlogit| over every
    position, and max |dlogp| at the beams' tokens.  What the bf16 bound is calibrated on."""
    toks = state[0].reshape(images * k, -1)
    img = ref.img[:images].repeat_interleave(k, 0)
    lg, _ = teacher_forced_stepwise(m, ref.d, img.cuda(), toks)
    prefix = torch.cat([torch.full((toks.shape[0], 1), ref.d.bos, dtype=torch.long), torch.from_numpy(toks[:, :-1])], 1)
    lg64 = ref64.decoder_net(ref.s64, prefix, ref.enc64[:images].repeat_interleave(k, 0))
    err = float((lg.double() - lg64).abs().max())
    ids = torch.from_numpy(toks)[..., None]
    dlp = float((torch.log_softmax(lg.double(), -1).gather(2, ids) - torch.log_softmax(lg64, -1).gather(2, ids)).abs().max())
    print(f"plain route {tag} (teacher forced stepwise, {toks.shape[0]} rows x {toks.shape[1]} positions): max |dlogit| {err:.4f}, "
          f"max |dlogp at the beams' tokens| {dlp:.4f}; bf16 bound {BEAM_LONG_BF16_BOUND:.4f}")
    assert err < BEAM_LONG_BF16_BOUND, (err, "the plain route exceeds the bound at this length: recalibrate BEAM_LONG_BF16_BOUND on it")
    return err


def _form(m, latent, lat_self=0, ranges=1):
    def check():
        q = m._engine.query
        assert (q(Q_LAST_LATENT), q(Q_LAST_LATENT_SELF), q(Q_LAST_ROW_RANGES)) == (latent, lat_self, ranges)
    return check


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_beam_replay_whole_length_kv_form(dtype):
    """(a) 300 positions in the K/V form, k = 5: the BEAM instantiation of dec_attn_tile reads the self-attention history through
    pth[] in passes of 256 keys -- the checkpoints sit on both sides of the second pass -- and the back-pointer chain is 300 long."""
    ref = _ref(_long_dims())
    _, _, m = build(ref.d, sd=ref.sd, dtype=dtype, max_batch=10, latent=0)
    states, _ = _replay(f"K/V form {dtype}", ref, m, 2, 5, CHECKPOINTS, dtype, check_form=_form(m, 0))
    if dtype == "bf16":
        _plain_route_error("K/V form", ref, m, 2, 5, states[300])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_beam_replay_whole_length_latent_cross_attention(dtype):
    """(b) the same with the cross attention in latent form (an image's 5 beams are ONE row of 40 heads, 16 to a tile)."""
    ref = _ref(_long_dims())
    _, _, m = build(ref.d, sd=ref.sd, dtype=dtype, max_batch=10, latent=1)
    states, _ = _replay(f"latent cross attention {dtype}", ref, m, 2, 5, CHECKPOINTS, dtype, check_form=_form(m, 1))
    if dtype == "bf16":
        _plain_route_error("latent form", ref, m, 2, 5, states[300])


def test_beam_replay_bf16_latent_beams_across_tiles():
    """(b) bf16 w768_h20 at k = 3: 60 heads of an image span several latent tiles per row."""
    ref = _ref(_long_dims("w768_h20", max_len=80), images=2)
    _, _, m = build(ref.d, sd=ref.sd, dtype="bf16", max_batch=6, latent=1)
    states, _ = _replay("w768_h20 bf16 latent", ref, m, 2, 3, [n for n in CHECKPOINTS if n <= 65], "bf16", check_form=_form(m, 1))
    _plain_route_error("w768_h20 latent", ref, m, 2, 3, states[66])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_beam_replay_latent_self_history(dtype):
    """(c) TXO_LATENT_SELF=1: the self attention reads the z history through the latent core's slot tables (lat_attn.h: LA_PATH_TILES
    tiles x 16 keys x the wave count).  fp32: 8 waves, 512 positions, decoded to 258.  bf16 at width 256: 4 waves, exactly 256
    positions -- the positional table ends on the last slot the table covers, and the decode runs to it."""
    max_len = 320 if dtype == "fp32" else 256
    ref = _ref(_long_dims(max_len=max_len))
    _, _, m = build(ref.d, sd=ref.sd, dtype=dtype, max_batch=10, latent=1, env={"TXO_LATENT_SELF": "1"})
    pairs = [n for n in CHECKPOINTS if n <= 257] if dtype == "fp32" else [n for n in CHECKPOINTS if n <= 129] + [254, 255]
    states, _ = _replay(f"latent self history {dtype}", ref, m, 2, 5, pairs, dtype, check_form=_form(m, 1, lat_self=1))
    if dtype == "bf16":
        _plain_route_error("latent self history", ref, m, 2, 5, states[256])


@pytest.mark.parametrize("k,vocab", [(k, 1000) for k in range(1, 9)] + [(k, v) for v in (1024, 1025, 1100) for k in (2, 8)])
def test_beam_replay_every_beam_count_and_both_select_paths(k, vocab):
    """(d) k = 1 ... 8 on the register path of beam_select_kernel (V = 1000), and k = 2, 8 at its last size (1024) and on the general
    path (1025, 1100).  k = 8 at V = 1000 also replays every step up to 24 and must select, before its last round, a candidate of beam 7
    with a token >= 768: that is bit 31 of the register path's `taken` mask.  k = 1 is greedy, token for token."""
    ref = _ref(_long_dims(max_len=80, vocab=vocab), images=2)
    _, _, m = build(ref.d, sd=ref.sd, max_batch=16, latent=0)
    pairs = [n for n in CHECKPOINTS if n <= 65]
    if (k, vocab) == (8, 1000):
        pairs = sorted(set(pairs) | set(range(24)))
    states, rep = _replay(f"k = {k}, V = {vocab}", ref, m, 2, k, pairs, check_form=_form(m, 0))
    if k == 1:
        assert np.array_equal(m.generate(ref.img.cuda(), 66).cpu().numpy(), states[66][0][:, 0])
    if (k, vocab) == (8, 1000):
        hits = sum(int(((rep.parents[n][:, :-1] == 7) & (states[n + 1][0][:, :-1, n] >= 768)).sum()) for n in pairs)
        print(f"selections that set bit 31 of `taken` before the last round: {hits}")
        assert hits >= 1


def test_beam_replay_eos_exact_against_float64():
    """(e) eos favoured by + 2.0 on its logit, 6 images, k = 5: the float64 oracle finishes every beam within 30 positions and never
    decides by less than 1e-3 (asserted first), so the engine has to give its tokens, its step count and its scores within 2e-3; and
    every step is replayed: finished beams frozen at their score, the loop stopping when the last one finishes."""
    d = _long_dims()
    ref = _ref(d, images=6, bias_eos=2.0)
    want_t, want_s = ref64.beam_search(ref.s64, ref.enc64, d.bos, d.eos, 64, 5)
    steps = want_t.shape[2]
    oracle_states = br.search64(ref.logp, 6, 5, d.eos, 64)                    # the oracle's search with every state kept
    assert max(oracle_states) == steps and np.array_equal(oracle_states[steps][0], want_t.numpy())
    np.testing.assert_allclose(oracle_states[steps][1], want_s.numpy(), rtol=0, atol=1e-9)
    own = br.replay_pairs(ref.s64, ref.enc64, d.bos, d.eos, oracle_states, range(steps), lambda a, b: 1e-9, logp_of=ref.logp)
    print(f"\nfloat64 beam search with eos: {steps} steps, smallest margin {own.gap:.2e}")
    assert steps <= 30 and own.gap > 1e-3 and bool((want_t[:, :, -1] == d.eos).all())
    _, _, m = build(d, sd=ref.sd, max_batch=30, latent=0)
    m.eos_token = d.eos
    t, s = m.generate(ref.img.cuda(), 64, beam=5, return_beams=True)
    assert t.shape[2] == steps and torch.equal(t.cpu(), want_t)
    np.testing.assert_allclose(s.cpu().numpy(), want_s.numpy(), atol=2e-3)
    _replay("eos, every step", ref, m, 6, 5, range(steps), eos=d.eos, check_form=_form(m, 0))


def test_beam_replay_two_row_ranges():
    """(f) case (a) in fp32 on two row ranges (TXO_LANES=2, 4 images): each range has its own slot tables, range-local."""
    ref = _ref(_long_dims())
    _, _, m = build(ref.d, sd=ref.sd, max_batch=20, latent=0)
    with knobs(TXO_LANES=2):
        _replay("two row ranges fp32", ref, m, 4, 5, (64, 65, 256, 257), check_form=_form(m, 0, ranges=2))


@pytest.mark.parametrize("vocab", [1000, 1100], ids=["rows_in_registers", "general_path"])
def test_beam_replay_tie_rule(vocab):
    """(g) equal candidates are ranked by the lower flat index parent * V + token on both selection paths.  Token a' = a + 1 is a copy
    of image 0's first greedy token a: after one position a and a' head the beams with bit-equal scores, a first; after two, the
    beams continuing [a] and [a'] come in equal pairs.  The replay checks the flat-index order of every bit-equal pair."""
    ref = _ref(_long_dims(max_len=80, vocab=vocab), images=2, dup_first=True)
    _, _, m = build(ref.d, sd=ref.sd, max_batch=8, latent=0)
    states, rep = _replay(f"tie rule, V = {vocab}", ref, m, 2, 4, (0, 1, 2), check_form=_form(m, 0))
    a = ref.first
    for n in (1, 2):
        s0 = states[n][1][0]
        assert int((s0[:-1] == s0[1:]).sum()) >= 1, (n, s0)
    assert states[1][0][0, :2, 0].tolist() == [a, a + 1]
    assert rep.ties >= 2
