"""The single-position decode where its passes, tiles and forms switch (tests/decode_cases.py; tests/test_decode_cases_cpu.py proves that
each case reaches the branch it is listed for and that the oracle decides every fp32 token by >= 2e-5), against a float64 run of the oracle
(tests/ref64.py), eight greedy positions per case: every position reads the whole cross panel.

A. K/V form (csrc/dec_attn.h), launches: 159 / 160 / 161 / 320 / 321 keys in fp32 and 319 / 320 / 321 / 640 / 641 in bf16 -- one, two and three
   register passes, the last pass one key, exactly full and one short -- at 2 and 3 decoder heads;
B. ragged (dec_attn_ragged_kernel): 20 slots of images with 2 / 160 / 161 / 321 keys (bf16: 2 / 320 / 321 / 641), so that the rows of one
   16-row tile take different pass counts;
C. latent form (csrc/lat_attn.h): 16 * NW keys, one more, and the later round boundaries of the 8-wave and the 4-wave tile, at widths 64,
   256 (8 heads) and 768 (12 heads, bf16);
D. generate() with default knobs at the row counts where the persistent launch, the latent form, the second row range and the wide
   projection blocks begin (calib256 / calib768 dims, 65 keys).
A batch is three DISTINCT images placed at several slots; the float64 decode is computed once per distinct image.  Per case:
- the path that ran (Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES, Q_LAST_LATENT) is the restated expectation;
- every copy of an image gives bit-identical tokens and logits (D: copies on both sides of the range boundary; B: every ragged row is, in
  fp32, bit-identical to the same engine's run of that image alone);
- logits against float64 per distinct image: fp32 within 1e-4 and the oracle's tokens at every position; bf16 within
  decode_cases.bf16_bound (gpu_harness.BF16_BOUND["logits"]) over the positions computed from the oracle's own prefix;
- last-key sensitivity, no tolerance: with the pixels of every image's last patch replaced, and with only the last encoder row of every
  image replaced (the decode from encoder rows: nothing but key N - 1 differs), the step-0 logits of every row change.  A key dropped
  from 641 moves a logit by less than the bf16 bound; the patch form alone passes a kernel that never reads key N - 1 (the encoder layer
  spreads the patch over every row), the row form does not;
- B: NaN in the container's rows behind an image's n_b changes no bit of its logits.

Measured on MI355X, worst max |dlogit| against float64 per group (fp32 bound 1e-4, bf16 bound 0.0557; every case prints its own):
  A  fp32 1.6e-6 (w64_h2, 320 keys)     bf16 0.0351 (w64_h3, 321 keys; the other 9 cases 0.0209 - 0.0256)
  B  fp32 1.5e-6                        bf16 0.0216; every ragged row equals the image's run alone bit for bit, in bf16 too
  C  fp32 2.2e-6 (w256_h8, 256 keys)    bf16 0.0246 (w64_h2, 127 keys; width 256: 0.0225, width 768: 0.0237)
  D  fp32 2.0e-6                        bf16 0.0230 (calib256 at 128 rows, the persistent launch; launches 0.0206; calib768 0.0209)
No bf16 case came near its bound at 640 / 641 keys (0.0209 - 0.0256), so decode_cases.BF16_REBOUND is empty."""
import pytest
import torch

import decode_cases as dc
from gpu_harness import BF16_BOUND, assert_tokens_exact_up_to_margin, build, knobs, rgb_images
from texocr_amd._lib import Q_LAST_LATENT, Q_LAST_PERSISTENT, Q_LAST_RAGGED, Q_LAST_ROW_RANGES, Q_PERSIST_FALLBACKS

pytestmark = pytest.mark.gpu

PATH_Q = (Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES, Q_LAST_LATENT)


def _engine(case):
    d, sd, _ = dc.weights(case.dims)
    m = build(d, sd=sd, dtype=case.dtype, max_batch=case.rows, max_tokens=case.n, latent=case.latent)[2]
    m.eos_token = None
    return m


def _generate(case, m, n_pos, img=None, enc=None):
    """generate() with logits under the case's knobs; asserts the path that ran"""
    d = dc.DIMS[case.dims]
    env = {} if case.persist is None else {"TXO_PERSIST": case.persist}
    with knobs(**env):
        tok, lg = m.generate(img, n_pos, return_logits=True) if enc is None else m._engine.generate(None, n_pos, None, enc=enc, return_logits=True)
    got = tuple(m._engine.query(q) for q in PATH_Q)
    want = dc.expected_path(d, case.dtype, case.rows, case.persist, case.latent)[0]
    assert got == want, f"{case.id}: (persistent, ranges, latent) = {got}, expected {want}"
    assert m._engine.query(Q_PERSIST_FALLBACKS) == 0
    assert tok.shape == (case.rows, n_pos) and lg.shape == (case.rows, n_pos, d.vocab)
    return tok, lg


def _first_slots(slots):
    first = {}
    for b, s in enumerate(slots):
        first.setdefault(s, b)
    return first


def _assert_copies_identical(name, slots, tok, lg):
    first = _first_slots(slots)
    for b, s in enumerate(slots):
        a = first[s]
        if a != b and not (torch.equal(tok[b], tok[a]) and torch.equal(lg[b], lg[a])):
            pos = (lg[b] != lg[a]).any(-1).nonzero().flatten().tolist()
            raise AssertionError(f"{name}: slot {b} differs from slot {a} of the same image: tokens {tok[b].tolist()} / {tok[a].tolist()}, "
                                 f"logits at positions {pos}, max |d| {float((lg[b] - lg[a]).abs().max()):.3e}")
    return first


def _agreeing(tok, ref_tok):
    """the positions whose logits were computed from the oracle's own prefix (up to and including the first differing token)"""
    neq = tok != ref_tok
    return int(neq.argmax()) + 1 if neq.any() else len(tok)


def _assert_against_float64(name, dtype, n, first, tok, lg, ref_toks, ref_lg):
    """ref_toks / ref_lg: per distinct image.  Prints the maximum; fp32 1e-4 and exact tokens, bf16 the calibrated bound"""
    bound = 1e-4 if dtype == "fp32" else dc.bf16_bound(n, BF16_BOUND["logits"])
    worst, lines = 0.0, []
    for s, b in first.items():
        t, rt = tok[b].cpu().numpy(), ref_toks[s].numpy()
        if dtype == "fp32":
            assert_tokens_exact_up_to_margin(t[None], rt[None], ref_lg[s][None])
        upto = _agreeing(t, rt)
        err = float((lg[b, :upto].cpu().double() - ref_lg[s][:upto]).abs().max())
        lines.append(f"image {s} (slot {b}): {err:.3e} over {upto} positions")
        worst = max(worst, err)
    print(f"\n{name}: logits max |d| against float64 {worst:.3e} (bound {bound:.1e}); " + "; ".join(lines))
    assert worst < bound, (name, worst, bound)
    if dtype == "fp32":                           # (the oracle's margins are >= 2e-5 at every position: test_decode_cases_cpu.py)
        assert all(_agreeing(tok[b].cpu().numpy(), ref_toks[s].numpy()) == len(ref_toks[s]) for s, b in first.items())


def _other_patch(seed):
    return rgb_images(1, 16, 16, seed)[0]


def _replace_last_row(enc, last):
    """enc (B, Ns, D) with row last[b] of image b replaced by other, larger values"""
    out = enc.clone()
    for b, k in enumerate(last):
        out[b, k] = 1.0 - 3.0 * enc[b, k]
    return out


def _assert_every_row_changed(name, what, before, after):
    same = [b for b in range(before.shape[0]) if torch.equal(before[b], after[b])]
    assert not same, f"{name}: the step-0 logits of {len(same)} rows do not depend on {what}: rows {same[:16]}"


def _check_fixed(case):
    m = _engine(case)
    ref = dc.case_reference(case)
    x = ref.img[torch.tensor(case.slots)].cuda()
    tok, lg = _generate(case, m, dc.STEPS, img=x)
    first = _assert_copies_identical(case.id, case.slots, tok, lg)
    _assert_against_float64(case.id, case.dtype, case.n, first, tok, lg, ref.toks, ref.logits)
    # ---- last-key sensitivity: the last patch's pixels ...
    x2 = x.clone()
    x2[..., case.h - 16:, case.w - 16:] = _other_patch(77).cuda()
    _assert_every_row_changed(case.id, "the last patch's pixels", lg[:, 0], _generate(case, m, 1, img=x2)[1][:, 0])
    # ... and the last encoder row alone
    enc = m.encoder(x)
    assert enc.shape[1] == case.n
    base = _generate(case, m, 1, enc=enc)[1][:, 0]
    moved = _generate(case, m, 1, enc=_replace_last_row(enc, [case.n - 1] * case.rows))[1][:, 0]
    _assert_every_row_changed(case.id, "key N - 1", base, moved)


def _params(cases):
    return [pytest.param(c, id=c.id) for c in cases]


@pytest.mark.parametrize("case", _params(dc.A_CASES))
def test_kv_form_at_the_pass_boundaries(case):
    _check_fixed(case)


@pytest.mark.parametrize("case", _params(dc.C_CASES))
def test_latent_form_at_the_tile_rounds(case):
    _check_fixed(case)


@pytest.mark.parametrize("case", _params(dc.D_CASES))
def test_generate_at_the_row_seams(case):
    _check_fixed(case)


def _ragged_logits(eng, enc, ntok, prefix):
    """teacher-forced single-position steps of a ragged session: (B, positions, V)"""
    eng.decode_begin_ragged(enc, ntok)
    return torch.stack([eng.decode_step(t, prefix[t])[0] for t in range(prefix.shape[0])], 1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ragged_rows_of_different_pass_counts(dtype):
    ns, slots = dc.B_NS[dtype], dc.B_SLOTS
    name = f"B-{dc.B_DIMS}-N{'/'.join(map(str, ns))}-B{len(slots)}-{dtype}"
    d, sd, _ = dc.weights(dc.B_DIMS)
    refs = dc.ragged_reference(dtype)
    m = build(d, sd=sd, dtype=dtype, max_batch=len(slots), max_tokens=max(ns))[2]
    m.eos_token = None
    eng = m._engine
    dev = [refs[s].img[0].cuda() for s in slots]
    lens = [ns[s] for s in slots]
    ref_toks, ref_lg = [r.toks[0] for r in refs], [r.logits[0] for r in refs]
    # ---- generate_ragged: tokens
    tok = m.generate_ragged(dev, dc.STEPS)
    got = tuple(eng.query(q) for q in PATH_Q) + (eng.query(Q_LAST_RAGGED),)
    assert got == (0, 1, 0, 1), f"{name}: (persistent, ranges, latent, ragged) = {got}"
    assert tok.shape == (len(slots), dc.STEPS)
    # ---- teacher-forced steps of a ragged session (the oracle's greedy tokens are its own teacher-forced prefix): logits
    enc, ntok = m.encoder.forward_ragged(dev)
    assert ntok.tolist() == lens and enc.shape == (len(slots), max(ns), d.embed_dim)
    prefix = torch.stack([torch.cat([torch.tensor([d.bos]), ref_toks[s][:-1]]) for s in slots]).t().contiguous().cuda()
    lg = _ragged_logits(eng, enc, ntok, prefix)
    first = _assert_copies_identical(name, slots, tok, lg)
    full = [ref_toks[s] for s in slots]
    _assert_against_float64(name, dtype, max(ns), first, torch.stack(full), lg, ref_toks, ref_lg)      # (teacher forced: every position)
    if dtype == "fp32":
        assert_tokens_exact_up_to_margin(tok.cpu().numpy(), torch.stack(full).numpy(), torch.stack([ref_lg[s] for s in slots]))
    # ---- NaN behind every image's n_b: no bit of any logit changes
    spoiled = enc.clone()
    for b, nb in enumerate(lens):
        spoiled[b, nb:] = float("nan")
    assert bool(torch.isfinite(lg).all())
    assert torch.equal(_ragged_logits(eng, spoiled, ntok, prefix), lg), f"{name}: rows behind an image's n_b are read"
    # ---- last-key sensitivity: the last encoder row of every image alone, then the last patch's pixels
    bos = prefix[:1]
    moved = _ragged_logits(eng, _replace_last_row(enc, [nb - 1 for nb in lens]), ntok, bos)
    _assert_every_row_changed(name, "key n_b - 1", lg[:, 0], moved[:, 0])
    dev2 = [im.clone() for im in dev]
    for im in dev2:
        im[:, -16:, -16:] = _other_patch(77).cuda()
    enc2, _ = m.encoder.forward_ragged(dev2)
    _assert_every_row_changed(name, "the last patch's pixels", lg[:, 0], _ragged_logits(eng, enc2, ntok, bos)[:, 0])
    # ---- the same engine on every image alone: generate() and a fixed-shape session
    worst = 0.0
    for s, b in first.items():
        solo_tok = m.generate(dev[b][None], dc.STEPS)
        assert eng.query(Q_LAST_RAGGED) == 0
        eng.decode_begin(m.encoder(dev[b][None]))
        solo_lg = torch.stack([eng.decode_step(t, prefix[t, b:b + 1].contiguous())[0] for t in range(dc.STEPS)], 1)[0]
        diff = float((solo_lg - lg[b]).abs().max())
        worst = max(worst, diff)
        print(f"    image {s} ({ns[s]} keys) alone: tokens identical {torch.equal(solo_tok[0], tok[b])}, step logits max |d| {diff:.3e}")
        if dtype == "fp32":
            assert torch.equal(solo_tok[0], tok[b]), (name, s, solo_tok[0].tolist(), tok[b].tolist())
            assert torch.equal(solo_lg, lg[b]), (name, s, diff)
