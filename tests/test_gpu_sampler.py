"""decode='sample', every draw against the host restatement of the sampler (tests/sampler_ref.py).

Sampling is deterministic: Philox4x32-10 keyed by (seed; row of the batch, position) gives u, the kept set is the k largest logits
(ties lowest index first), and the token is where u * total falls in the kept entries' CDF (include/texocr.h: txo_set_sampling).  Each
case decodes with return_logits=True (the exact fp32 values the sampler read) or recomputes the logits of the decoded sequence, and
predicts every token on the host.  Where u * total lies more than BAND of the kept mass away from a CDF boundary the token must be the
host's; inside the band (fp32 sums in another order) it must be one of the two kept tokens around that boundary.  The fraction of
draws inside the band is printed per case.  Feedback: the logits the engine returned are those of its own sampled sequence, teacher
forced through the float64 oracle (tests/ref64.py), so every drawn token is the token the next position was fed.

Reached, and asserted where txo_engine_query can tell: the register sampler with 16-byte row loads (V 1000, 1020, 1024) and one-logit
loads (999, 950, 16, 10: the last two keep k = 1), the LDS sampler (1025, 1100, 8192, the largest vocabulary the device's LDS takes),
the persistent decode kernel and the launch path, one and two row ranges, stop='row' with compactions, generate_window beyond the
positional table, and decoder.generate's stepwise loop (start prefix, padding mask, sliding window)."""
import dataclasses

import numpy as np
import pytest
import torch

import ref64
import sampler_ref as sr
from gpu_harness import BF16_BOUND, SHAPE_CASES, STOP_ENV, both_paths, build, first_eos, knobs, rgb_images, stop_case
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES, Q_SAMPLE_VOCAB_MAX
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

BAND = 2e-5                    # of the kept mass: float32 sums of up to a few thousand terms stay well inside it
STEPS = 24
ROWS = 21
SEEDS = (0, 7, 2 ** 32 + 5, 2 ** 64 - 1)
TEMPS = (0.3, 1.0, 5.0)


def _dims(vocab, base="calib256"):
    """config.yml decoder widths (the persistent launch exists for them), 1 encoder / 2 decoder layers, 128x128 canvas"""
    return dataclasses.replace(SHAPE_CASES[base][0], vocab=vocab, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


def _tiny(vocab, max_len):
    return Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=2, vocab=vocab,
                max_len=max_len, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


def _form(V):
    """the sampler body a vocabulary reaches (step.h: sample_in_regs; sample_row_regs loads 16 bytes when V and a lane's chunk are
    multiples of 4)"""
    if V > 64 * 16:
        return "lds"
    per = (V + 63) // 64
    return "regs16" if V % 4 == 0 and per % 4 == 0 else "regs1"


def _check(name, tok, lg, temp, seeds, rows, ts):
    """tok (n,) drawn from lg (n, V) under keys (seeds, rows, ts) (broadcast); returns the host draws"""
    tok = np.asarray(tok).reshape(-1)
    V = lg.shape[-1]
    d = sr.draw(np.asarray(lg, dtype=np.float32).reshape(-1, V), temp, seeds, rows, ts)
    outside = d.dist > BAND
    bad = np.nonzero(outside & (tok != d.token))[0]
    assert bad.size == 0, (f"{name}: {bad.size} of {tok.size} draws differ from the host rule away from any boundary; first at {bad[:4]}: "
                           f"engine {tok[bad[:4]]}, host {d.token[bad[:4]]}")
    near = ~outside
    assert bool(((tok == d.pair[:, 0]) | (tok == d.pair[:, 1]))[near].all()), f"{name}: a draw near a boundary is not next to it"
    frac = float(near.mean())
    print(f"\n[sampler] {name}: {tok.size} draws checked, {frac:.4%} inside the band")
    # 2 * BAND * (kept entries) is the expected in-band fraction (0.4 % at k = 99): a case must not decide its draws in the band
    assert frac < max(0.02, 8 * sr.topk_of(V) * BAND), (name, frac)
    return d


def _check_engine(name, tok, lg, temp, seed):
    """generate() from BOS: token i of batch row b is keyed by (seed; b, i) (sampler_ref.keys_for('engine', ...))"""
    tok, lg = tok.cpu().numpy(), lg.cpu().numpy()
    B, n = tok.shape
    return _check(name, tok, lg, temp, seed, np.repeat(np.arange(B), n), np.tile(np.arange(n), B))


def _context_logits(net, start, tok, L):
    """(B, n, V) logits of every output token i from its own context -- output[:, :T0 + i], its last L tokens once it is longer than
    the positional table (decoder.py:99-100) -- through net(tokens (B, t)) -> (B, t, V)"""
    full = torch.cat([start, tok], 1)
    T0, n = start.shape[1], tok.shape[1]
    inside = min(n, L - T0 + 1)                       # tokens whose context fits the table
    out = [net(full[:, :T0 - 1 + inside])[:, T0 - 1:T0 - 1 + inside]] if inside > 0 else []
    out += [net(full[:, T0 + i - L:T0 + i])[:, -1:] for i in range(max(inside, 0), n)]
    return torch.cat([o.double().cpu() for o in out], 1)


def _feedback(sd, img, start, tok, lg, L, bound, rows=None):
    """max |engine logits - float64 logits of the engine's own sequence|"""
    s64 = ref64.sd64(sd)
    start, tok, lg = start.cpu(), tok.cpu(), lg.cpu()
    if rows is not None:
        img, start, tok, lg = img[rows], start[rows], tok[rows], lg[rows]
    enc64 = ref64.encode(s64, img)
    tf = _context_logits(lambda x: ref64.decoder_net(s64, x, enc64), start, tok, L)
    err = float((lg.double() - tf).abs().max())
    assert err < bound, err
    return err


def _bos(d, B):
    return torch.full((B, 1), d.bos, dtype=torch.long)


# vocabulary: (sampler body, temperature, seed)
VOCABS = {1000: ("regs16", 0.3, 7), 1020: ("regs16", 1.0, 2 ** 32 + 5), 1024: ("regs16", 5.0, 2 ** 64 - 1), 999: ("regs1", 0.3, 0),
          950: ("regs1", 1.0, 7), 16: ("regs1", 1.0, 2 ** 32 + 5), 10: ("regs1", 1.0, 7), 1025: ("lds", 1.0, 2 ** 32 + 5),
          1100: ("lds", 0.3, 7), 8192: ("lds", 1.0, 2 ** 64 - 1)}


@pytest.mark.parametrize("vocab", list(VOCABS))
def test_every_draw_on_each_sampler_form(vocab):
    """fp32, 21 rows x 24 positions.  Up to 1024 entries the persistent launch and the launch path are EACH checked against the host
    (V = 10 takes launches only); beyond, the LDS sampler on the launch path.  The logits are fed back through float64 within 1e-4."""
    form, temp, seed = VOCABS[vocab]
    assert _form(vocab) == form
    d = _dims(vocab)
    sd = synth.synth_state_dict(d, 3)
    _, _, m = build(d, sd=sd, max_batch=ROWS)
    m.eos_token = None
    img = rgb_images(ROWS, 64, 64, 21)
    x = img.cuda()
    kw = dict(temp=temp, decode="sample", seed=seed, return_logits=True)
    if vocab <= 1024 and vocab != 10:
        (tp, lp), (tl, ll) = both_paths(m, x, STEPS, **kw)
        runs = {"persistent": (tp, lp), "launches": (tl, ll)}
    else:
        with knobs(TXO_PERSIST=0):
            tl, ll = m.generate(x, STEPS, **kw)
        assert m._engine.query(Q_LAST_PERSISTENT) == 0
        runs = {"launches": (tl, ll)}
    for path, (t, lg) in runs.items():
        assert t.shape == (ROWS, STEPS) and lg.shape == (ROWS, STEPS, vocab)
        _check_engine(f"V={vocab} ({form}) {path}, temp {temp}, seed {seed}", t, lg, temp, seed)
    err = _feedback(sd, img, _bos(d, ROWS), tl, ll, d.max_len, 1e-4)
    print(f"[sampler] V={vocab}: fed back through float64, max |dlogit| {err:.2e}")


@pytest.mark.parametrize("vocab", [1000, 1100])
def test_every_temperature_and_seed(vocab):
    """temperatures 0.3 / 1.0 / 5.0 x seeds 0, 7, 2^32 + 5, 2^64 - 1 (the last two: a nonzero high key half) on the default path: the
    persistent launch at 1000 entries, the LDS sampler on launches at 1100"""
    d = _dims(vocab)
    _, _, m = build(d, seed=5, max_batch=ROWS)
    m.eos_token = None
    x = rgb_images(ROWS, 64, 64, 22).cuda()
    for temp in TEMPS:
        for seed in SEEDS:
            t, lg = m.generate(x, STEPS, temp=temp, decode="sample", seed=seed, return_logits=True)
            assert m._engine.query(Q_LAST_PERSISTENT) == int(vocab <= 1024)
            _check_engine(f"V={vocab} temp {temp} seed {seed}", t, lg, temp, seed)


def test_bf16_both_paths():
    """bf16 at config widths: persistent launch and launches each against the host; the logits fed back through float64 within the
    bf16 bound test_gpu_shapes.py asserts for these widths"""
    d = _dims(1000)
    sd = synth.synth_state_dict(d, 3)
    _, _, m = build(d, sd=sd, dtype="bf16", max_batch=ROWS)
    m.eos_token = None
    img = rgb_images(ROWS, 64, 64, 23)
    (tp, lp), (tl, ll) = both_paths(m, img.cuda(), STEPS, temp=0.3, decode="sample", seed=2 ** 32 + 5, return_logits=True)
    _check_engine("bf16 persistent", tp, lp, 0.3, 2 ** 32 + 5)
    _check_engine("bf16 launches", tl, ll, 0.3, 2 ** 32 + 5)
    err = _feedback(sd, img, _bos(d, ROWS), tp, lp, d.max_len, BF16_BOUND["logits"])
    print(f"[sampler] bf16: fed back through float64, max |dlogit| {err:.4f}")


def test_the_benchmarks_own_configuration():
    """bench.py's sampled decode: bf16, 64 images of 224x672, temperature 0.3, 256 positions (the persistent launch).  Two rows are
    fed back through float64 and compared over the oracle's top 5 of every position, the bound test_gpu_parity.py asserts at this
    shape (test_bf16_benchmark_shape_vs_reference_every_position)."""
    d = Dims(canvas=672)
    sd = synth.synth_state_dict(d, 0)
    _, _, m = build(d, sd=sd, dtype="bf16", max_batch=64, max_tokens=589)
    m.eos_token = None
    img = torch.from_numpy(synth.synth_images(64, 3, 224, 672, seed=4321))
    t, lg = m.generate(img.cuda(), 256, temp=0.3, decode="sample", seed=1, return_logits=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 1
    assert t.shape == (64, 256)
    _check_engine("bench configuration (bf16, 64 x 256, temp 0.3)", t, lg, 0.3, 1)
    rows = [6, 41]
    s64 = ref64.sd64(sd)
    enc64 = ref64.encode(s64, img[rows])
    tok = t.cpu()[rows]
    tf = ref64.decoder_net(s64, torch.cat([_bos(d, 2), tok[:, :-1]], 1), enc64)
    top5 = tf.topk(5, dim=-1).indices
    err = float((torch.gather(lg.cpu()[rows].double(), 2, top5) - torch.gather(tf, 2, top5)).abs().max())
    print(f"[sampler] bench configuration: rows {rows} fed back through float64, max |dlogit| over the top 5 {err:.4f}")
    assert err < 0.038, err


def test_two_row_ranges_key_by_the_batch_row():
    """256 bf16 rows on two row ranges (TXO_LANES=2): the second range starts at row 128, its draws are keyed by the batch row"""
    d = _dims(1000)
    _, _, m = build(d, seed=3, dtype="bf16", max_batch=256)
    m.eos_token = None
    x = rgb_images(256, 16, 16, 24).cuda()
    with knobs(TXO_LANES=2):
        t, lg = m.generate(x, STEPS, temp=1.0, decode="sample", seed=7, return_logits=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and m._engine.query(Q_LAST_ROW_RANGES) == 2
    _check_engine("bf16 256 rows, two row ranges", t, lg, 1.0, 7)


def test_row_stop_compactions_key_by_the_batch_row():
    """stop='row' with a compaction every other position: a row that moves to another slot keeps its key.  The compacting decode
    returns no logits (a finished row's would be missing), so its tokens are predicted from the logits of the same decode with the
    global stop, up to each row's first eos."""
    d, sd, img = stop_case()
    _, _, m = build(d, sd=sd, max_batch=40, env=STOP_ENV)
    x = img.cuda()
    seed, temp = 2 ** 32 + 5, 0.5
    with knobs(TXO_LANES=2):
        glob, lg = m.generate(x, d.max_len, temp=temp, decode="sample", seed=seed, return_logits=True)
        row = m.generate(x, d.max_len, temp=temp, decode="sample", seed=seed, stop="row")
        assert m._engine.query(Q_LAST_ROW_RANGES) == 2 and m._engine.query(Q_LAST_COMPACTIONS) >= 2
    host = _check_engine("global stop, two ranges", glob, lg, temp, seed)
    g = glob.cpu().numpy()
    want = np.where(host.dist > BAND, host.token, g.reshape(-1)).reshape(g.shape)
    r = row.cpu().numpy()
    first = first_eos(r, d.eos)
    assert len(set(first)) >= 4, first
    n = min(r.shape[1], g.shape[1])
    for b, f in enumerate(first):
        upto = n if f < 0 else f + 1
        assert np.array_equal(r[b, :upto], want[b, :upto]), (b, upto)


def test_positions_beyond_256():
    """a positional table of 300 (test_multipass_attention_panels): keys past position 256"""
    d = _tiny(96, 300)
    sd = synth.synth_state_dict(d, 11)
    _, _, m = build(d, sd=sd, max_batch=2)
    m.eos_token = None
    img = rgb_images(2, 64, 64, 51)
    t, lg = m.generate(img.cuda(), 290, temp=1.0, decode="sample", seed=2 ** 64 - 1, return_logits=True)
    assert t.shape == (2, 290)
    _check_engine("290 positions", t, lg, 1.0, 2 ** 64 - 1)
    _feedback(sd, img, _bos(d, 2), t, lg, d.max_len, 1e-4)


def test_generate_window_beyond_the_table():
    """max_len beyond an 8-entry table with V % 8 == 0: the engine slides the window itself (generate_window), token i keyed by
    (seed; row, i); the fed-back logits are those of each token's own window"""
    d = _tiny(96, 8)
    sd = synth.synth_state_dict(d, 12)
    _, _, m = build(d, sd=sd, max_batch=4)
    m.eos_token = None
    img = rgb_images(4, 64, 64, 52)
    t, lg = m.generate(img.cuda(), 20, temp=1.0, decode="sample", seed=2 ** 32 + 5, return_logits=True)
    assert t.shape == (4, 20)
    for i in (0, 7, 8, 19):
        assert sr.keys_for("engine", 1, d.max_len, i, 2 ** 32 + 5) == (2 ** 32 + 5, i)
    _check_engine("generate_window", t, lg, 1.0, 2 ** 32 + 5)
    err = _feedback(sd, img, _bos(d, 4), t, lg, d.max_len, 1e-4)
    print(f"[sampler] generate_window: fed back through float64, max |dlogit| {err:.2e}")


def test_stepwise_loop_keys():
    """decoder.generate's general loop (V % 8 != 0, so no one-pass prefill): a BOS start and a 3-token start prefix, both sliding past
    the 8-entry table, and a padded start inside it.  Keys: sampler_ref.keys_for('stepwise', ...); logits: the engine's own decoder.net
    on each token's context (single-position steps, the loop's kernels), and float64 for the unmasked runs."""
    d = _tiny(90, 8)
    sd = synth.synth_state_dict(d, 13)
    _, _, m = build(d, sd=sd, max_batch=4)
    img = rgb_images(4, 64, 64, 53)
    enc = m.encoder(img.cuda())
    seed, temp, L = 2 ** 32 + 5, 1.0, d.max_len
    rng = np.random.default_rng(0)
    prefix = torch.from_numpy(rng.integers(0, d.vocab - 3, (4, 3))).long()

    def keys(T0, n):
        k = [sr.keys_for("stepwise", T0, L, i, seed) for i in range(n)]
        s = np.tile(np.array([q[0] for q in k], dtype=np.uint64), 4)
        p = np.tile(np.array([q[1] for q in k]), 4)
        return s, np.repeat(np.arange(4), n), p

    for name, start, n in (("BOS start", _bos(d, 4), 14), ("3-token start", prefix, 10)):
        t = m.decoder.generate(start.cuda(), None, n, temp=temp, decode="sample", seed=seed, enc=enc)
        assert t.shape == (4, n)
        lg = _context_logits(lambda x: m.decoder.net(x.cuda(), enc=enc), start, t.cpu(), L)
        _check(f"stepwise, {name}", t.cpu().numpy(), lg.float().numpy(), temp, *keys(start.shape[1], n))
        _feedback(sd, img, start, t, lg, L, 1e-4)
    mask = torch.tensor([[0, 1, 1], [1, 1, 1], [0, 0, 1], [1, 0, 1]], dtype=torch.bool)
    n = 5
    t = m.decoder.generate(prefix.cuda(), None, n, temp=temp, decode="sample", seed=seed, enc=enc, mask=mask.cuda())
    full = torch.cat([prefix, t.cpu()], 1)
    mfull = torch.cat([mask, torch.ones((4, n), dtype=torch.bool)], 1)
    lg = m.decoder.net(full[:, :2 + n].cuda(), mask=mfull[:, :2 + n].cuda(), enc=enc)[:, 2:].cpu()
    _check("stepwise, padded start", t.cpu().numpy(), lg.numpy(), temp, *keys(3, n))


@pytest.mark.parametrize("vocab", [1000, 1100])
def test_the_index_order_tie_rule(vocab):
    """Seven of every eight to_logits rows zero with one shared bias: those logits are EXACTLY equal, and with the bias at the median
    of the other logits the k-th value falls inside that tie group at most positions.  The engine keeps the lowest-index ties
    (include/texocr.h; the reference's torch.topk leaves the order unspecified): register sampler (1000, both decode paths) and LDS
    sampler (1100)."""
    d = _dims(vocab)
    sd = synth.synth_state_dict(d, 3)
    free = np.arange(vocab) % 8 == 3
    w = sd["decoder.net.to_logits.weight"].copy()
    b = sd["decoder.net.to_logits.bias"].copy()
    w[~free] = 0
    b[~free] = 0
    sd["decoder.net.to_logits.weight"] = w
    x = rgb_images(ROWS, 64, 64, 25).cuda()
    _, _, m0 = build(d, sd=dict(sd, **{"decoder.net.to_logits.bias": b}), max_batch=ROWS)
    m0.eos_token = None
    _, lg0 = m0.generate(x, STEPS, return_logits=True)
    level = np.float32(np.median(lg0.cpu().numpy()[..., free]))
    del m0
    b[~free] = level
    sd["decoder.net.to_logits.bias"] = b
    _, _, m = build(d, sd=sd, max_batch=ROWS)
    m.eos_token = None
    kw = dict(temp=1.0, decode="sample", seed=7, return_logits=True)
    if vocab <= 1024:
        (tp, lp), (tl, ll) = both_paths(m, x, STEPS, **kw)
        runs = {"persistent": (tp, lp), "launches": (tl, ll)}
    else:
        tl, ll = m.generate(x, STEPS, **kw)
        assert m._engine.query(Q_LAST_PERSISTENT) == 0
        runs = {"launches": (tl, ll)}
    k = sr.topk_of(vocab)
    for path, (t, lg) in runs.items():
        l = lg.cpu().numpy()
        assert bool((l[..., ~free] == level).all())                       # the precondition: one exact tie group
        above = (l[..., free] > level).sum(-1)
        straddle = (above < k) & (above + int((~free).sum()) > k)
        assert straddle.mean() >= 0.5, straddle.mean()
        _check_engine(f"ties V={vocab} {path} (k-th value inside the tie group at {straddle.mean():.0%} of the positions)", t, lg, 1.0, 7)
        on_tie = ~free[t.cpu().numpy().reshape(-1)]
        assert on_tie.mean() > 0.05, on_tie.mean()                        # the rule decides real draws


def test_sampling_refuses_a_vocabulary_beyond_the_lds_and_takes_the_largest_that_fits():
    """Beyond 1024 entries the sampler stages a row in LDS (V * 4 bytes per workgroup): set_sampling refuses a vocabulary the device's
    limit (txo_engine_query TXO_Q_SAMPLE_VOCAB_MAX) cannot take -- before anything is launched -- and the largest one that fits draws
    like every other"""
    _, _, m = build(_tiny(64, 8), seed=1, max_batch=2)
    vmax = m._engine.query(Q_SAMPLE_VOCAB_MAX)
    assert vmax >= 65536 // 4, vmax
    del m
    x = rgb_images(2, 64, 64, 54).cuda()
    _, _, m = build(_tiny(vmax + 1, 8), seed=1, max_batch=2)
    with pytest.raises(ValueError, match="LDS"):
        m._engine.set_sampling(True)
    with pytest.raises(ValueError, match="LDS"):
        m.generate(x, 4, decode="sample", seed=1)
    m.eos_token = None
    assert m.generate(x, 4).shape == (2, 4)                               # greedy decoding is unaffected
    del m
    _, _, m = build(_tiny(vmax, 8), seed=1, max_batch=2)
    m.eos_token = None
    t, lg = m.generate(x, 6, temp=1.0, decode="sample", seed=7, return_logits=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and lg.shape == (2, 6, vmax)
    _check_engine(f"largest vocabulary the LDS takes ({vmax})", t, lg, 1.0, 7)
