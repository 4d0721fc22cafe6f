"""Token selection and scoring on scripted logits rows (tests/logit_scripts.py; tests/test_logit_scripts_cpu.py proves where every script puts
its maximum).  The logits head's weight is zero and its bias is the script, so every row at every position IS the script -- asserted bit for
bit first, in every case -- and the kernels that walk a row in pieces have to find a maximum that sits in the last float4, the first float4
of the second sweep, lane 63's last slot, behind V - 1 of an odd vocabulary, the tail tile of the score walk or thread 255's fourth register,
and have to give the lower index of two equal entries across lanes, sweeps, waves, threads and lane groups.

Expectation (float64, logit_scripts.expect): the arg-max, lowest index among equals; logp = v[pick] - logsumexp(v).  Bounds, none new:
test_gpu_logp.SAME_LOGITS (1e-5: logp against the log-softmax of the same call's logits) for every generate(), test_gpu_score.FP32_LOGP (2e-4)
for score() in fp32 and bf16 alike (with a zero head weight nothing is rounded to bf16), beam_ref.eps_fp32 for the beam replay, and
test_gpu_sampler._check for every draw.

Measured on MI355X, worst |dlogp| against float64 per group (every case prints its own; fp32 and bf16 equal to the digit):
  greedy / prompted 4.8e-7 (V = 1028; the +-80 row 1.5e-7 at most)      rules / guard / closing 6.5e-7 (V = 1025)
  beam score increments 7.9e-7 (general path), 4.8e-7 (registers)        score 8.2e-7 (V = 1027)
The (-0.0, +0.0) script: 0 of 504 returned rows keep the -0.0 ("Scripted logits", with the mutation table)."""
import numpy as np
import pytest
import torch

import beam_ref as br
import logit_scripts as ls
import sampler_ref as sr
from gpu_harness import both_paths, build, knobs, on_path, rgb_images
from test_gpu_logp import SAME_LOGITS
from test_gpu_sampler import _check_engine, _dims
from test_gpu_score import FP32_LOGP
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES

pytestmark = pytest.mark.gpu

ROWS, STEPS = 5, 6
WIDE_ROWS = 130                       # bf16: two row ranges (TXO_LANES=2)


class _Engine:
    """one model per (V, dtype) with a zero logits head; load(row) puts a script into the head's bias (a reload replaces the engine's
    weights: model.py: HipEngine.load_state_dict)"""

    def __init__(self, V, dtype="fp32", rows=ROWS):
        self.d = _dims(V)
        self.sd = synth.synth_state_dict(self.d, 3)
        self.sd["decoder.net.to_logits.weight"] = np.zeros_like(self.sd["decoder.net.to_logits.weight"])
        self.m = build(self.d, sd=self.sd, dtype=dtype, max_batch=rows)[2]
        self.m.eos_token = None
        self.img = rgb_images(rows, 32, 32, 5).cuda()
        self.V, self.dtype = V, dtype

    def load(self, row):
        self.row = np.ascontiguousarray(row, np.float32)
        self.m.load_state_dict(dict(self.sd, **{"decoder.net.to_logits.bias": self.row.copy()}))
        return self.m

    def assert_logits_are_the_script(self, name, lg, signed_zeros=True):
        got = lg.detach().cpu().numpy().reshape(-1, self.V)
        if signed_zeros:
            same = got.view(np.uint32) == self.row.view(np.uint32)[None]
        else:
            same = got == self.row[None]
        assert bool(same.all()), (f"{name}: the returned logits are not the script at {int((~same).sum())} of {same.size} entries; first at "
                                  f"{np.argwhere(~same)[:3].tolist()}")


def _assert_picks(name, tok, want):
    tok = tok.cpu().numpy()
    want = np.broadcast_to(np.asarray(want, np.int64), tok.shape)
    bad = np.argwhere(tok != want)
    assert bad.size == 0, f"{name}: {len(bad)} of {tok.size} tokens differ; first (row, position) {bad[0].tolist()}: {int(tok[tuple(bad[0])])}, expected {int(want[tuple(bad[0])])}"


def _logp_error(name, logp, want, worst):
    e = float(np.abs(logp.cpu().numpy().astype(np.float64) - np.broadcast_to(want, tuple(logp.shape))).max())
    worst[0] = max(worst[0], e)
    assert e < SAME_LOGITS, f"{name}: max |logp - float64| {e:.3e} (bound {SAME_LOGITS:.0e})"
    return e


# ---- greedy and prompted -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", list(ls.VOCABS))
def test_greedy_and_prompted_pick_the_scripted_maximum(V, dtype):
    """Per script: the persistent launch and the launch path (return_logits: the premise), captured steps, stop='row', bf16 also 130 rows
    on two row ranges; then a prompted decode that forces the arg-max for up to three positions and picks three more -- its prefix_logp
    and logp are the unprompted logp's bits (step.h's promise above argmax_step_kernel)."""
    eng = _Engine(V, dtype, WIDE_ROWS if dtype == "bf16" else ROWS)
    x = eng.img[:ROWS]
    worst, worst_wide = [0.0], [0.0]
    for s in ls.greedy_scripts(V):
        m = eng.load(s.row)
        e = ls.expect(s.row)
        want_lp = e.logp[e.pick]
        acc = worst_wide if s.kind == "wide" else worst
        runs = both_paths(m, x, STEPS, return_logits=True, return_logp=True)
        for path, (tok, lg, lp) in zip(("persistent", "launches"), runs):
            name = f"{s.id} {dtype} {path}"
            assert tok.shape == (ROWS, STEPS) and lg.shape == (ROWS, STEPS, V)
            eng.assert_logits_are_the_script(name, lg)
            _assert_picks(name, tok, e.pick)
            err = _logp_error(name, lp, want_lp, acc)
            if s.kind == "wide":
                print(f"\n{name}: values over {float(s.row.min()):.0f} .. {float(s.row.max()):.0f}, logp {want_lp:.6f}: |dlogp| {err:.3e} (bound {SAME_LOGITS:.0e})")
        lp0 = runs[1][2]
        assert torch.equal(runs[0][2], lp0), f"{s.id}: the persistent launch's logp differs from the launch path's"
        with knobs(TXO_GRAPH=1, TXO_PERSIST=0):
            tg, lpg = m.generate(x, STEPS, return_logp=True)
        _assert_picks(f"{s.id} captured steps", tg, e.pick)
        assert torch.equal(lpg, lp0)
        m.eos_token = next(v for v in range(V - 3, -1, -1) if v not in s.top)       # (an eos no script picks: stop='row' only changes the loop)
        tr, lpr = on_path(m, False, lambda: m.generate(x, STEPS, stop="row", return_logp=True))
        m.eos_token = None
        _assert_picks(f"{s.id} stop='row'", tr, e.pick)
        assert torch.equal(lpr, lp0)
        if dtype == "bf16":
            with knobs(TXO_LANES=2):
                tw, lgw, lpw = m.generate(eng.img, STEPS, return_logits=True, return_logp=True)
            assert (m._engine.query(Q_LAST_PERSISTENT), m._engine.query(Q_LAST_ROW_RANGES)) == (0, 2)
            eng.assert_logits_are_the_script(f"{s.id} two row ranges", lgw)
            _assert_picks(f"{s.id} two row ranges", tw, e.pick)
            _logp_error(f"{s.id} two row ranges", lpw, want_lp, acc)
        # prompted: rows forced for 0, 1, 2, 3, 3 positions (the forced token is the arg-max), three picks behind
        prefix = torch.full((ROWS, 4), e.pick, dtype=torch.int64)
        prefix[:, 0] = eng.d.bos
        plen = [1, 2, 3, 4, 4]
        tp, lpp, plp = m.generate(x, 3, prefix=prefix.cuda(), prefix_len=plen, return_logp=True)
        assert m._engine.query(Q_LAST_PERSISTENT) == 0
        _assert_picks(f"{s.id} prompted", tp, e.pick)
        assert torch.equal(lpp, lp0[:, :3]), f"{s.id}: a prompted decode's logp differs from the unprompted bits"
        for b, n in enumerate(plen):
            assert torch.equal(plp[b, 1:n], lp0[b, 1:n]), f"{s.id}: prefix_logp of row {b} differs from the unprompted logp's bits"
            assert not bool(plp[b, n:].any()) and float(plp[b, 0]) == 0.0
    print(f"\nV={V} {dtype}: {len(ls.greedy_scripts(V))} scripts, worst |dlogp| {worst[0]:.3e}, wide row {worst_wide[0]:.3e} (bound {SAME_LOGITS:.0e})")


# ---- rules and guard ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", list(ls.VOCABS))
def test_rules_and_guard_pick_the_runner_up_then_the_third(V):
    """A two-state ban table that forbids the script's maximum in state 1 (every token leads there), the (1, 1) guard that bans the previous
    pick, and both: the picks are logit_scripts.replay's (maximum, runner-up, third, runner-up, ...), logp is the raw row's.  On 1028 and
    1027 also the closing decode: the budget binds at the last pick, which has to be eos."""
    eng = _Engine(V)
    x = eng.img
    worst = [0.0]
    for s in [t for t in ls.greedy_scripts(V) if t.kind != "wide"]:
        m = eng.load(s.row)
        e = ls.expect(s.row)
        rules = ls.ban_table(V, [s.top[0]])
        for tag, kw in (("rules", dict(rules=rules)), ("guard", dict(repeat_guard=ls.GUARD)), ("rules+guard", dict(rules=rules, repeat_guard=ls.GUARD))):
            want = ls.replay(s.row, STEPS, rules=kw.get("rules"), guard=kw.get("repeat_guard"))[0]
            assert tag != "rules+guard" or want[:3].tolist() == list(s.top)          # (rules: the runner-up stays; guard: it alternates)
            out = m.generate(x, STEPS, return_logits=True, return_logp=True, **kw)
            tok, lg, lp = out[:3]
            name = f"{s.id} {tag}"
            assert m._engine.query(Q_LAST_PERSISTENT) == 0
            eng.assert_logits_are_the_script(name, lg)
            _assert_picks(name, tok, want[None, :])
            _logp_error(name, lp, e.logp[want][None, :], worst)
            if "rules" in kw:
                assert out[-1].cpu().tolist() == [[1, 0]] * ROWS
    if V in ls.CLOSE_VOCABS:
        s = ls.single(V, 1023)
        m = eng.load(s.row)
        eos = eng.d.eos
        rules = ls.ban_table(V, [s.top[0]], eos=eos)
        want = ls.replay(s.row, STEPS, rules=rules, eos=eos, close=True)[0]
        assert want.tolist() == [s.top[0]] + [s.top[1]] * (STEPS - 2) + [eos]
        m.eos_token = eos
        tok, lg, lp, _ = m.generate(x, STEPS, return_logits=True, return_logp=True, rules=rules, close=True)
        m.eos_token = None
        eng.assert_logits_are_the_script(f"{s.id} closing", lg)
        _assert_picks(f"{s.id} closing", tok, want[None, :])
        _logp_error(f"{s.id} closing", lp, ls.expect(s.row).logp[want][None, :], worst)
    print(f"\nV={V} rules / guard: worst |dlogp| {worst[0]:.3e} (bound {SAME_LOGITS:.0e})")


# ---- sampler -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", ls.SAMPLER_VOCABS)
def test_sampler_with_the_kth_place_a_scripted_pair(V):
    """21 rows x 24 positions, temperatures 0.3 and 1.0; the k-th largest entry (k = the reference's top-k of V) is a pair of equal bits
    on both sides of lane 1's first slot (1025: also 1023 | 1024): the lower index is kept, the other never drawn.  The last script's pair
    is (-0.0, +0.0): the head computes 0 + bias, so a -0.0 in the bias may come back as +0.0 -- the logits are compared by value there, the
    count of surviving -0.0 is printed, and every draw follows the host rule ON THE RETURNED LOGITS (order of the bits: sampler_ref)."""
    eng = _Engine(V, rows=21)
    form = ls.sampler_form(V)
    for s in ls.sampler_scripts(V):
        m = eng.load(s.row)
        for temp, seed in ((0.3, 7), (1.0, 2 ** 32 + 5)):
            kw = dict(temp=temp, decode="sample", seed=seed, return_logits=True)
            if V <= 1024:
                runs = dict(zip(("persistent", "launches"), both_paths(m, eng.img, 24, **kw)))
            else:
                runs = {"launches": on_path(m, False, lambda: m.generate(eng.img, 24, **kw))}
            for path, (tok, lg) in runs.items():
                name = f"{s.id} ({form}) {path} temp {temp}"
                eng.assert_logits_are_the_script(name, lg, signed_zeros=not s.zeros)
                got = lg.cpu().numpy()
                if s.zeros:
                    print(f"\n{name}: {int(np.signbit(got[..., s.pair[0]]).sum())} of {got.shape[0] * got.shape[1]} returned rows keep the -0.0")
                d = _check_engine(name, tok, lg, temp, seed)
                t = tok.cpu().numpy().reshape(-1)
                kept = sr.kept_mask(got.reshape(-1, V), sr.topk_of(V))
                assert bool(kept[np.arange(t.size), t].all()), f"{name}: a token outside the kept set was drawn"
                if not s.zeros:
                    a, b = s.pair
                    assert int((t == a).sum()) >= 1 and not (t == b).any(), f"{name}: the pair at the k-th place: {int((t == a).sum())} draws of {a}, {int((t == b).sum())} of {b}"
                assert np.array_equal(t[d.dist > 2e-5], d.token[d.dist > 2e-5])


# ---- beam search ---------------------------------------------------------------------------------------------------------------------------
def _beam_states(search, n_max):
    out = {}
    for n in range(1, n_max + 1):
        t, sc = search(n)
        out[n] = (t.cpu().numpy(), sc.cpu().numpy())
    return out


@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("V", ls.BEAM_VOCABS)
def test_beam_selection_on_scripted_rows(V, k):
    """Registers (1024) and the general path (1025), four steps, every step replayed (beam_ref.replay_pairs: ancestry, increments, order,
    the flat-index rule on bit-equal scores, selection) against the closed form -- every beam sees the same row.  Step 1 is exact: the k
    largest entries in order, ties to the lower index.  Then the ruled and the guarded kernels under the same ban table / the (1, 1) guard."""
    eng = _Engine(V, rows=2 * k)
    eng.m.rules_beam = True
    eng.m.guard_beam = True
    x = eng.img[:2]
    eps = lambda a, b: br.eps_fp32(a[1], b[1])
    inc, ties = 0.0, 0
    for s in ls.beam_scripts(V):
        m = eng.load(s.row)
        order = np.argsort(-s.row.astype(np.float64), kind="stable")[:k]
        rules = ls.ban_table(V, [s.top[0]])
        for tag, kw in (("plain", {}), ("rules", dict(rules=rules)), ("guard", dict(repeat_guard=ls.GUARD)), ("rules+guard", dict(rules=rules, repeat_guard=ls.GUARD))):
            name = f"{s.id} k={k} {tag}"
            if tag == "plain":
                states = _beam_states(lambda n: m.generate(x, n, beam=k, return_beams=True), 4)
            else:
                states = _beam_states(lambda n: (lambda r: (r.tokens, r.scores))(m.beam_search(x, k, n, **kw)), 4)
            assert states[1][0][:, :, 0].tolist() == [order.tolist()] * 2, f"{name}: step 1 is not the row's k largest in order"
            np.testing.assert_allclose(states[1][1], np.broadcast_to(ls.expect(s.row).logp[order], (2, k)), rtol=0, atol=br.eps_fp32(states[1][1]))
            rep = br.replay_pairs(None, None, eng.d.bos, None, states, range(4), eps,
                                  logp_of=ls.beam_logp_of(s.row, kw.get("rules"), kw.get("repeat_guard")))
            inc, ties = max(inc, rep.inc_err), ties + rep.ties
            assert rep.steps == 4 and (s.kind != "tie" or rep.ties >= 2), name
    print(f"\nbeam V={V} k={k}: max |score increment - float64| {inc:.3e}, {ties} bit-equal score pairs checked against the flat-index rule")


# ---- scoring ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", ls.SCORE_VOCABS)
def test_score_on_scripted_rows(V, dtype):
    """score_rows_kernel at M = 5, 15 and 85 rows (1, 3, 17 images x 5 positions): top1 exact with the lower index of equals (the merge
    of the four lane groups), logp and top1_logp within test_gpu_score.FP32_LOGP of float64 -- in bf16 too."""
    eng = _Engine(V, dtype, rows=17)
    L = 6
    worst = 0.0
    for s in ls.score_scripts(V):
        m = eng.load(s.row)
        e = ls.expect(s.row)
        cycle = [t for t in (0, 63, 64, V - 1) + tuple(s.top[:2]) if 0 <= t < V]
        for rows in (1, 3, 17):
            trg = torch.tensor([[eng.d.bos] + [cycle[(b * (L - 1) + p) % len(cycle)] for p in range(L - 1)] for b in range(rows)], dtype=torch.int64)
            m._engine.decode_begin(m.encoder(eng.img[:rows]))
            logp, top1, top1_logp = m._engine.decode_score(trg.cuda())
            name = f"{s.id} {dtype} M={rows * (L - 1)}"
            assert logp.shape == (rows, L - 1)
            _assert_picks(name, top1, e.pick)
            e1 = float(np.abs(logp.cpu().numpy().astype(np.float64) - e.logp[trg[:, 1:].numpy()]).max())
            e2 = float(np.abs(top1_logp.cpu().numpy().astype(np.float64) - e.logp[e.pick]).max())
            worst = max(worst, e1, e2)
            assert e1 < FP32_LOGP and e2 < FP32_LOGP, (name, e1, e2)
    print(f"\nscore V={V} {dtype}: worst |dlogp| {worst:.3e} (bound {FP32_LOGP:.0e})")
