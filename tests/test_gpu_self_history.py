"""The single-position decode where the SELF-attention history ends its slots and passes (tests/history_cases.py;
tests/test_history_cases_cpu.py proves that the checkpoints reach every seam of every form and that the oracle's margins and the
probe's float64 floor hold), against a float64 run of the oracle (tests/ref64.py; tests/attn_ref.py under a key mask) over a positional
table of 520: one, two and three passes of 256 keys, the statistics slot reused by the third.

A. the launch forms -- plain, fused (TXO_SELF_FUSED=1) and key-masked -- through decoder.net under TXO_NET_STEPWISE=1: 520 steps;
B. the persistent launch (calib256 dims), 5 rows in both types, 72 and 128 bf16 rows, 136 fp32 rows: generate(520), equal to the launches bit for bit;
C. the latent self attention (TXO_LATENT_SELF=1) outside beam search, table 300;
D. one multi-position pass over 520 positions, and a step behind a prefill of 256 / 257 / 512 / 513 tokens;
E. stop='row' compacting rows whose history is longer than one pass.
A batch is two DISTINCT images over five slots; float64 runs once per distinct image.  Per case:
- the form that ran, through Q_LAST_PERSISTENT / Q_LAST_LATENT_SELF / Q_LAST_ROW_RANGES;
- every copy of an image gives bit-identical logits (and tokens);
- logits against float64: the maximum over the table and at every checkpoint, printed; fp32 within 1e-4 and the oracle's tokens up to
  its first margin below 2e-5, bf16 within BF16_LONG_BOUND;
- A, one decoder layer: the one-key probe.  Replacing the token at history position p changes NO bit before p and the logits of EVERY
  position from p on (float64 moves by >= 1e-3 there); in fp32 the change agrees with float64's within 2e-4.  Under a key mask that
  covers p the replacement changes no bit at any position that is not masked itself.

Measured on MI355X: see DESIGN.md section 4, "Self-attention history"."""
import numpy as np
import pytest
import torch

import history_cases as hc
from gpu_harness import BF16_BOUND, STOP_ENV, assert_tokens_exact_up_to_margin, both_paths, build, knobs
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_LATENT, Q_LAST_LATENT_SELF, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES

pytestmark = pytest.mark.gpu

FP32_BOUND = 1e-4
PROBE_FP32 = 2e-4                                 # |engine's change - float64's change| of the one-key probe
# the step behind a prefill against the multi-position pass at the same position: tests/test_gpu_ragged_forward.py (STEP_VS_PREFILL, fp32)
# and tests/test_gpu_parity.py::test_prefill_equals_cached_steps_and_continues (bf16)
STEP_VS_PREFILL = {"fp32": 2e-5, "bf16": 0.08}
# bf16 against float64 at histories of up to 520 keys, the PLAIN stepwise route alone (group A, form "plain"; max over both widths),
# measured on MI355X (2026-10-21): 0.0274 at width 256, 0.0285 at width 64, per checkpoint 0.012 - 0.024 with no growth along the history.
# None: not above gpu_harness.BF16_BOUND["logits"] (0.0557), which then stays the bound of every form
BF16_PLAIN_LONG = None
BF16_LONG_BOUND = BF16_BOUND["logits"] if BF16_PLAIN_LONG is None else max(BF16_BOUND["logits"], 1.5 * BF16_PLAIN_LONG)


def _engine(name, dtype, rows, latent=None, env=None):
    d, sd, _ = hc.weights(name)
    m = build(d, sd=sd, dtype=dtype, max_batch=rows, latent=latent, env=env)[2]
    m.eos_token = None
    return d, m


def _forms(m):
    q = m._engine.query
    return q(Q_LAST_PERSISTENT), q(Q_LAST_LATENT_SELF), q(Q_LAST_ROW_RANGES)


def _first_slots(slots):
    first = {}
    for b, s in enumerate(slots):
        first.setdefault(s, b)
    return [first[s] for s in sorted(first)]


def _assert_copies_identical(name, slots, *tensors):
    first = _first_slots(slots)
    for b, s in enumerate(slots):
        for x in tensors:
            if not torch.equal(x[b], x[first[s]]):
                pos = (x[b] != x[first[s]]).reshape(x.shape[1], -1).any(-1).nonzero().flatten().tolist()
                raise AssertionError(f"{name}: slot {b} differs from slot {first[s]} of the same image at positions {pos[:12]} ..")
    return first


def _assert_against_float64(name, dtype, lg, ref_lg, skip=()):
    """lg (2, n, V): one row per distinct image; ref_lg the float64 logits.  Prints the maximum over the table and per checkpoint"""
    bound = FP32_BOUND if dtype == "fp32" else BF16_LONG_BOUND
    err = (lg.cpu().double() - ref_lg).abs().amax(-1).amax(0)                   # per position
    for p in skip:
        err[p] = 0.0
    n = err.shape[0]
    at = ", ".join(f"{t}: {float(err[t]):.2e}" for t in hc.CHECKPOINTS if t < n and t not in skip)
    print(f"\n{name}: logits max |d| against float64 over {n} positions {float(err.max()):.3e} at {int(err.argmax())} (bound {bound:.1e}); {at}")
    assert float(err.max()) < bound, (name, float(err.max()), int(err.argmax()), bound)
    return float(err.max())


def _stepwise(m, prefix, enc, mask=None):
    with knobs(TXO_NET_STEPWISE=1):
        return m.decoder.net(prefix, mask=mask, enc=enc)


LAUNCH_FORMS = ("plain", "fused", "masked")
_GRID = [pytest.param(w, t, id=f"{w}-{t}") for w in hc.WIDTHS for t in ("fp32", "bf16")]


def _launch_engine(name, dtype, form):
    d, m = _engine(name, dtype, len(hc.FIVE), latent=0, env={"TXO_SELF_FUSED": "1"} if form == "fused" else None)
    ref = hc.reference(name)
    slots = torch.tensor(hc.FIVE)
    return d, m, ref, m.encoder(ref.img[slots].cuda()), ref.prefix[slots].cuda()


def _only(*masked):
    m = torch.ones((len(hc.FIVE), hc.T_HIST), dtype=torch.bool)
    m[:, list(masked)] = False
    return m.cuda()


# ---- A. the launch forms, 520 single-position steps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["", "_own"], ids=["synth", "own_key"])
@pytest.mark.parametrize("form", LAUNCH_FORMS)
@pytest.mark.parametrize("width,dtype", _GRID)
def test_launch_forms_over_three_passes(width, dtype, form, model):
    """model "_own": every self attention's k projection is its q projection, so key t carries at least a tenth of the softmax at
    position t.  On the plain and masked forms key t is the ONE key of the last pass at t = 256 / 512 and its token is also the step's
    input, so the probe cannot isolate it; here float64 moves by > 2 x the bf16 bound when it is dropped (test_history_cases_cpu.py)"""
    name = f"A-{form}-{width}{model}-{dtype}"
    width += model
    d, m, ref, enc, prefix = _launch_engine(width, dtype, form)
    # (the masked form against the UNMASKED reference: the mask covers the last position alone, which no other position attends)
    lg = _stepwise(m, prefix, enc, mask=_only(hc.T_HIST - 1) if form == "masked" else None)
    assert _forms(m) == (0, 0, 1) and m._engine.query(Q_LAST_LATENT) == 0
    assert lg.shape == (len(hc.FIVE), hc.T_HIST, d.vocab)
    keep = hc.T_HIST - 1 if form == "masked" else hc.T_HIST
    first = _assert_copies_identical(name, hc.FIVE, lg[:, :keep])
    _assert_against_float64(name, dtype, lg[first, :keep], ref.logits[:, :keep])
    if dtype == "fp32":
        assert_tokens_exact_up_to_margin(lg[first, :keep].argmax(-1).cpu().numpy(), ref.toks[:, :keep].numpy(), ref.logits[:, :keep])
    if form == "fused":
        # no query reports the knob: the fused launch projects k / v in another kernel and scores key t apart, so it rounds differently
        # (measured: all 520 positions differ in some bit, in both types and widths); the plain form's bits here would mean TXO_SELF_FUSED was not read
        plain = _stepwise(_launch_engine(width, dtype, "plain")[1], prefix, enc)
        differ = int((plain != lg).any(-1).any(0).sum())
        print(f"    fused against plain: {differ} of {hc.T_HIST} positions differ in some bit, max |d| {float((plain - lg).abs().max()):.3e}")
        assert differ > hc.T_HIST // 2, f"{name}: the fused engine gives the plain form's bits at {hc.T_HIST - differ} positions"


@pytest.mark.parametrize("which", ["holes", "left_pad"])
@pytest.mark.parametrize("width,dtype", _GRID)
def test_key_masked_form_against_the_masked_reference(width, dtype, which):
    """masks over 0 / 255 / 256 / 511 and over a left-padded block of 40, two decoder layers: the logits of every position that is not
    masked itself against attn_ref's float64 under the same mask; replacing the tokens AT the masked positions changes no bit of them"""
    name = f"A-masked-{which}-{width}-{dtype}"
    d, m, ref, enc, prefix = _launch_engine(width, dtype, "masked")
    valid = hc.key_masks()[which]
    mask = valid[None].expand(len(hc.FIVE), -1).contiguous().cuda()
    lg = _stepwise(m, prefix, enc, mask=mask)
    assert _forms(m) == (0, 0, 1) and m._engine.query(Q_LAST_LATENT) == 0
    first = _assert_copies_identical(name, hc.FIVE, lg[:, valid.cuda()])
    _assert_against_float64(name, dtype, lg[first], hc.masked_reference(width, which), skip=(~valid).nonzero().flatten().tolist())
    other = prefix.clone()
    other[:, ~valid.cuda()] = (prefix[:, ~valid.cuda()] + 1) % (d.vocab - 3)
    lg2 = _stepwise(m, other, enc, mask=mask)
    diff = (lg2 != lg).any(-1)[:, valid.cuda()]
    assert not bool(diff.any()), f"{name}: a masked key is read: {int(diff.sum())} (row, position) pairs changed with the masked tokens"


@pytest.mark.parametrize("form", LAUNCH_FORMS)
@pytest.mark.parametrize("width,dtype", _GRID)
def test_one_key_probe(width, dtype, form):
    """one decoder layer: the token at p reaches the logits of t >= p through key / value p of that layer alone"""
    name1 = width + "_1l"
    name = f"A-probe-{form}-{width}-{dtype}"
    d, m, ref, enc, prefix = _launch_engine(name1, dtype, form)
    base64, moved64 = hc.probe(name1)
    slots = torch.tensor(hc.FIVE)
    # (masked form: the mask covers the last position alone; its own logits are unspecified, every other position sees every key)
    mask = _only(hc.T_HIST - 1) if form == "masked" else None
    keep = hc.T_HIST - 1 if form == "masked" else hc.T_HIST
    base = _stepwise(m, prefix, enc, mask=mask)[:, :keep]
    assert _forms(m) == (0, 0, 1)
    _assert_against_float64(name, dtype, base[_first_slots(hc.FIVE)], base64[:, :keep])
    worst = 0.0
    for p in hc.PROBE_P:
        x64, lg64 = moved64[p]
        moved = _stepwise(m, x64[slots].cuda(), enc, mask=mask)[:, :keep]
        assert torch.equal(moved[:, :p], base[:, :p]), f"{name}: the token at {p} changes logits BEFORE {p}: a read behind the causal limit"
        same = ~(moved[:, p:] != base[:, p:]).any(-1)
        assert not bool(same.any()), (f"{name}: key {p} is not read at (row, position) "
                                      f"{[(int(b), p + int(t)) for b, t in same.nonzero()[:8]]} .. ({int(same.sum())} in all)")
        if dtype == "fp32":
            got = (moved[:, p:] - base[:, p:]).cpu().double()
            err = float((got - (lg64 - base64)[slots][:, p:keep]).abs().max())
            worst = max(worst, err)
            assert err < PROBE_FP32, (name, p, err)
    if dtype == "fp32":
        print(f"\n{name}: the probe's change against float64's, max |d| {worst:.3e} (bound {PROBE_FP32:.0e})")


@pytest.mark.parametrize("width,dtype", _GRID)
def test_key_masked_probe_converse_one_layer(width, dtype):
    """the converse on the probe's own model: with position p masked, replacing its token changes no bit at any other position"""
    name1 = width + "_1l"
    d, m, ref, enc, prefix = _launch_engine(name1, dtype, "masked")
    _, moved64 = hc.probe(name1)
    slots = torch.tensor(hc.FIVE)
    for p in hc.MASKED_P:                                                        # (every masked p is a probed p)
        mask = _only(p)
        base = _stepwise(m, prefix, enc, mask=mask)
        moved = _stepwise(m, moved64[p][0][slots].cuda(), enc, mask=mask)
        others = [t for t in range(hc.T_HIST) if t != p]
        assert torch.equal(base[:, others], moved[:, others]), (width, dtype, p)
    assert _forms(m) == (0, 0, 1) and m._engine.query(Q_LAST_LATENT) == 0


# ---- B. the persistent launch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,dtype,slots", [
    pytest.param("calib256", "fp32", hc.FIVE, id="fp32-B5"), pytest.param("calib256", "bf16", hc.FIVE, id="bf16-B5"),
    pytest.param("calib256", "bf16", hc.ROWS72, id="bf16-B72"), pytest.param("calib256", "bf16", hc.ROWS128, id="bf16-B128"),
    pytest.param("calib256", "fp32", hc.ROWS136, id="fp32-B136"),
    pytest.param("calib256_own", "fp32", hc.FIVE, id="own_key-fp32-B5"), pytest.param("calib256_own", "bf16", hc.FIVE, id="own_key-bf16-B5")])
def test_persistent_launch_over_three_passes(model, dtype, slots):
    """5 rows: idle groups through all three passes; 128 rows: two full attention rounds per group; 72 rows: idle groups in the second
    round; 136 fp32 rows: two 16-row tiles per team (history_cases.persist_attn_rounds).  The own-key model: key t, spliced in by selects, is the one key of the last pass at
    t = 256 / 512 -- dropping it moves float64 by more than twice the bound, on the engine's own sequence too (asserted below)"""
    name = f"B-{model}-B{len(slots)}-{dtype}"
    d, m = _engine(model, dtype, len(slots))
    ref = hc.reference(model)
    x = ref.img[torch.tensor(slots)].cuda()
    (tok, lg), (tok_l, lg_l) = both_paths(m, x, hc.T_HIST, return_logits=True)           # (asserts Q_LAST_PERSISTENT per path)
    assert m._engine.query(Q_LAST_ROW_RANGES) == 1 and m._engine.query(Q_LAST_LATENT_SELF) == 0
    assert tok.shape == (len(slots), hc.T_HIST) and lg.shape == (len(slots), hc.T_HIST, d.vocab)
    # same passes -> same bits: the early history request and the splice of key t change no bit on any pass
    if not (torch.equal(tok, tok_l) and torch.equal(lg, lg_l)):
        pos = (lg != lg_l).any(-1).any(0).nonzero().flatten().tolist()
        raise AssertionError(f"{name}: the persistent launch differs from the launches at positions {pos[:12]} .. ({len(pos)} in all), "
                             f"max |d| {float((lg - lg_l).abs().max()):.3e}")
    first = _assert_copies_identical(name, slots, tok, lg)
    own = tok[first].cpu()
    _assert_against_float64(name, dtype, lg[first], hc.feedback(model, own))
    if dtype == "fp32":
        assert_tokens_exact_up_to_margin(own.numpy(), ref.toks.numpy(), ref.logits)
    if model.endswith("_own"):
        effect = hc.own_key_effect(model, own)                                  # (float64 alone, on the sequence the engine decoded)
        print(f"    float64 max_v |dlogit| of dropping key t at t, on the engine's sequence: {effect}")
        assert min(effect.values()) >= hc.OWN_FLOOR, (name, effect)


# ---- C. the latent self attention outside beam search -----------------------------------------------------------------------------------
@pytest.mark.parametrize("width,dtype", _GRID)
def test_latent_self_history(width, dtype):
    name = f"C-{width}-{dtype}"
    name3 = width + "_t300"
    d, m = _engine(name3, dtype, len(hc.FIVE), latent=1, env={"TXO_LATENT_SELF": "1"})
    ref = hc.reference(name3)
    tok, lg = m.generate(ref.img[torch.tensor(hc.FIVE)].cuda(), hc.T_LAT, return_logits=True)
    # bf16 at width 256 runs the tile on four waves: its slot tables end at 256 positions and the engine declines the form (K/V history)
    want = int(hc.lat_self_ok(d, dtype, hc.T_LAT))
    assert _forms(m) == (0, want, 1) and m._engine.query(Q_LAST_LATENT) == 1, (name, _forms(m), want)
    assert want == (0 if (width, dtype) == ("calib256", "bf16") else 1)
    assert tok.shape == (len(hc.FIVE), hc.T_LAT)
    first = _assert_copies_identical(name, hc.FIVE, tok, lg)
    own = tok[first].cpu()
    _assert_against_float64(name, dtype, lg[first], hc.feedback(name3, own))
    if dtype == "fp32":
        assert_tokens_exact_up_to_margin(own.numpy(), ref.toks.numpy(), ref.logits)


# ---- D. one multi-position pass, and the step behind it ------------------------------------------------------------------------------
STEP_BEHIND = (256, 257, 512, 513)


@pytest.mark.parametrize("width,dtype", _GRID)
def test_multi_position_pass_and_the_step_behind_it(width, dtype):
    name = f"D-{width}-{dtype}"
    d, sd, _ = hc.weights(width)
    rows = -(-hc.T_HIST // d.n_pos)                                           # the pass's workspace: max_batch * max_tokens rows >= 520
    m = build(d, sd=sd, dtype=dtype, max_batch=max(rows, len(hc.FIVE)), latent=0)[2]
    ref = hc.reference(width)
    slots = torch.tensor(hc.FIVE)
    enc, prefix = m.encoder(ref.img[slots].cuda()), ref.prefix[slots].cuda()
    one = m.decoder.net(prefix, enc=enc)
    first = _assert_copies_identical(name, hc.FIVE, one)
    _assert_against_float64(name + " one pass", dtype, one[first], ref.logits)
    if dtype == "fp32":
        assert_tokens_exact_up_to_margin(one[first].argmax(-1).cpu().numpy(), ref.toks.numpy(), ref.logits)
    eng, xt = m._engine, prefix.t().contiguous()
    for t in STEP_BEHIND:
        eng.decode_begin(enc)
        eng.decode_prefill(prefix[:, :t].contiguous(), want_logits=False)
        step = eng.decode_step(t, xt[t])[0]
        _assert_copies_identical(f"{name} step {t}", hc.FIVE, step[:, None])
        d_one = float((step - one[:, t]).abs().max())
        d_64 = float((step[first].cpu().double() - ref.logits[:, t]).abs().max())
        print(f"    step {t} behind a prefill of {t}: max |d| against the pass {d_one:.3e} (bound {STEP_VS_PREFILL[dtype]:.0e}), against float64 {d_64:.3e}")
        assert d_one < STEP_VS_PREFILL[dtype], (name, t, d_one)
        assert d_64 < (FP32_BOUND if dtype == "fp32" else BF16_LONG_BOUND), (name, t, d_64)
    assert _forms(m) == (0, 0, 1) and m._engine.query(Q_LAST_LATENT) == 0        # (a session's steps are launches, on calib256 too)


# ---- E. a compaction of two-pass histories ---------------------------------------------------------------------------------------------
def test_row_stop_compacts_two_pass_histories():
    d, sd, img, want, _, first = hc.stop_case()
    _, _, m = build(d, sd=sd, max_batch=hc.STOP_ROWS, env=dict(STOP_ENV, TXO_STOP_GRAPH="0"))
    tok = m.generate(img.cuda(), d.max_len, stop="row")
    assert _forms(m) == (0, 0, 1)
    plan = hc.compactions(first, d.max_len)
    got = m._engine.query(Q_LAST_COMPACTIONS)
    print(f"\nE: {got} compactions; restated (positions decoded, rows before, after, live rows moved): {plan}")
    assert got > 0 and got == len(plan)
    # (the engine reports the count, not the positions: with the count equal to the restatement's, its last compactions are the restated ones)
    assert any(t1 >= 257 and moved > 0 for t1, _, _, moved in plan)
    bad = [b for b in range(hc.STOP_ROWS) if not np.array_equal(tok[b].cpu().numpy(), want[b].numpy())]
    assert not bad, f"rows {bad} differ from the oracle (first eos {[first[b] for b in bad]})"
