"""The pick kernels of the repeat guard (csrc/step_guard.h) at long periods, long runs and long histories, on scripted decoders.

tests/test_gpu_guard.py decodes random weights, which loop with period 1 or 2: its longest scan with a consequence has 14 comparisons, the
kernels admit 255.  Here the logits follow a script (tests/guard_zoo.py; tests/test_guard_zoo_cpu.py pins on the CPU oracle that the
script's ranks lie >= 100 x the bf16 logit error apart), so a pick is known on the host: the first token of the position's ranking that
tests/guard_ref.py (brute force, on the row's full history) does not ban.  Where logits come back every pick is also test_gpu_guard's
host replay on the engine's own rows; sampled draws go through test_gpu_sampler._check on the masked rows.  Everything runs on the launch
path and asserts Q_LAST_GUARDED == 1."""
import numpy as np
import pytest
import torch

import guard_ref
import ref64
import guard_zoo as gz
from gpu_harness import STOP_ENV, build, knobs, rgb_images
from test_gpu_guard import replay_greedy
from test_gpu_sampler import _check as check_draws
from test_gpu_sampler import _form
from texocr_amd import guard
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_GUARDED, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES

pytestmark = pytest.mark.gpu


def _model(d, script, dtype="fp32", max_batch=8, env=None, eos=None):
    sd = gz.scripted_sd(d, script)
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=max_batch, env=env)
    m.eos_token = eos
    return m


def _prefix(d, hists):
    """histories -> (prefix (B, 1 + longest) int64 on the GPU: bos, the history, pad; lengths)"""
    pre = torch.full((len(hists), 1 + max(len(h) for h in hists)), d.pad, dtype=torch.int64)
    for r, h in enumerate(hists):
        pre[r, 0] = d.bos
        pre[r, 1:1 + len(h)] = torch.tensor(list(h), dtype=torch.int64)
    return pre.cuda(), [1 + len(h) for h in hists]


def _expect(script, history, n, P, R, eos=None, banned=guard_ref.banned):
    """the n picks behind `history` on the host: at each, the first token of the position's ranking that the guard does not ban (the eos is
    never banned and ends the row).  P = 0: no guard"""
    h, out = list(history), []
    for _ in range(n):
        ban = banned(h, P, R, eos) if P else set()
        pick = next(x for x in script[min(len(h), len(script) - 1)] if x not in ban)
        out.append(pick)
        h.append(pick)
        if eos is not None and pick == eos:
            break
    return out


def _in_force(history, token, P, R):
    """the periods by which `token` is banned behind `history`"""
    return {p for p in range(1, P + 1) if guard_ref.ends_in_copies(list(history) + [int(token)], p, R + 1)}


def _guarded(m):
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and m._engine.query(Q_LAST_GUARDED) == 1


# ---- 1. the boundary table, through prefix= ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("R", gz.REPEATS)
def test_boundary_table(R, dtype):
    """guard (p, R) for p in 1, 2, 3, 5, 8, 15, 16 behind guard_zoo.boundary's prefixes: m_p = R * p - 2 (not banned), R * p - 1 (banned), a
    mismatch at the last compared pair (not banned) and one pair further back (banned).  No combination is dropped: the positional table
    has 320 entries and the longest case, (16, 16), needs 273 prefix columns and 17 picks; its binding scan has 255 comparisons.  ((1, 1)
    has no mismatch row: it compares nothing.)  Each group runs without and with a BOS-only row: without, the multi-position pass consumes
    the shortest prefix and the longer ones are committed in the loop; with, every forced token is committed in the loop.
    Asserted: the first pick and the p picks behind it are the host's; the forced tokens' log-probabilities are the unguarded call's bits;
    fp32: every row equals the same call on that row alone, bit for bit (the prompted entries return no logits), and the sampled call at
    temperature 0.3 draws every token from the guard-masked rows of decoder.net on the row's own tokens (test_gpu_sampler._check)."""
    d = gz.dims(gz.BOUNDARY_V, gz.TABLE)
    script = gz.const_script(gz.BOUNDARY_RANKING, gz.TABLE)
    m = _model(d, script, dtype, max_batch=32)                   # (32 x 17 workspace rows: the multi-position pass takes a shortest prefix of 254)
    a = gz.BOUNDARY_RANKING[0]
    img = rgb_images(5, 32, 48, 95).cuda()
    enc = m.encoder(img)
    rows = gz.boundary_rows(R)
    longest, seed = 0, 11
    for p in gz.PERIODS:
        group = [(kind, h) for q, kind, h in rows if q == p]
        n = p + 1
        for bos_row in (False, True):
            hists = [h for _, h in group] + ([()] if bos_row else [])
            kinds = [k for k, _ in group] + (["bos"] if bos_row else [])
            B = len(hists)
            pre, lens = _prefix(d, hists)
            toks, logp, plogp = m.generate(img[:B], n, prefix=pre, prefix_len=lens, return_logp=True, repeat_guard=(p, R))
            _guarded(m)
            _, _, plogp0 = m.generate(img[:B], n, prefix=pre, prefix_len=lens, return_logp=True)
            assert torch.equal(plogp, plogp0), (p, R)                 # a forced token is never masked, and is scored as ever
            got = toks.cpu().tolist()
            for r, (kind, h) in enumerate(zip(kinds, hists)):
                assert got[r] == _expect(script, h, n, p, R), (p, R, kind, got[r])
                if kind in ("under", "broken", "bos"):
                    assert got[r][0] == a, (p, R, kind)
                else:
                    assert got[r][0] != a and a in guard_ref.banned(h, p, R), (p, R, kind)
                    longest = max(longest, R * p - 1)
                if dtype == "fp32":
                    t1 = m.generate(img[r:r + 1], n, prefix=pre[r:r + 1, :lens[r]], repeat_guard=(p, R))
                    assert torch.equal(t1[0], toks[r]), (p, R, kind)
            if dtype == "fp32" and bos_row:
                ts = m.generate(img[:B], n, prefix=pre, prefix_len=lens, decode="sample", temp=0.3, seed=seed, repeat_guard=(p, R))
                _guarded(m)
                tk, masked, rr, tt = ts.cpu().numpy(), [], [], []
                for r, h in enumerate(hists):
                    seq = [d.bos] + list(h) + tk[r, :-1].tolist()
                    lg = m.decoder.net(torch.tensor([seq], dtype=torch.int64).cuda(), enc=enc[r:r + 1])[0, len(h):].float().cpu().numpy()
                    for j in range(n):
                        masked.append(guard_ref.mask(lg[j], seq[1:1 + len(h) + j], p, R)[0])
                        rr.append(r)
                        tt.append(len(h) + j)
                    assert [i for i in guard_ref.violations(list(h) + tk[r].tolist(), p, R) if i >= len(h)] == [], (p, R, r)
                check_draws(f"guard zoo boundary ({p}, {R})", tk.reshape(-1), np.stack(masked), 0.3, seed, np.asarray(rr), np.asarray(tt))
    print(f"\n[guard] boundary table R={R} {dtype}: periods {list(gz.PERIODS)}, longest binding scan {longest} comparisons")
    assert longest == R * 16 - 1 and (R < 16 or longest >= 200)


# ---- 2. several periods at once --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gz.RULERS, ids=lambda c: f"V{c.vocab}")
def test_ruler_bans_four_tokens_by_four_periods(case):
    """behind a b a c a b a d a b a c a b a the guards (8, 1) and (16, 1) ban {a, b, c, d} (periods 1, 2, 4, 8: four lanes, one map; where
    the ids fall is tests/test_guard_zoo_cpu.py's test_ban_placement); the script ranks a > b > c > d > x, so the pick is x, and the
    picks behind it are the host's.  V = 64 / 67: the 16-byte and the scalar stream; 1000 / 1030: the register and the LDS sampler, where
    every draw of the sampled call at temperature 0.3 is sampler_ref's on the guard-masked row (test_gpu_sampler._check; a prompted decode
    returns no logits, so the rows are the float64 oracle's for the engine's own tokens, rounded to float32: at this temperature a CDF
    boundary moves by less than 1e-9 of the mass per 1e-4 of logit error, far inside _check's band)"""
    d = gz.dims(case.vocab, 32, case.low_specials)
    script = gz.const_script(case.letters + (case.x,), 32)
    h = gz.ruler(*case.letters)
    n = 12
    s64 = ref64.sd64(gz.scripted_sd(d, script))
    enc64 = ref64.encode(s64, rgb_images(3, 32, 48, 96))
    for dtype in ("fp32", "bf16"):
        m = _model(d, script, dtype)
        img = rgb_images(3, 32, 48, 96).cuda()
        pre, lens = _prefix(d, [h, (), h[:7]])
        for P in (8, 16):
            toks = m.generate(img, n, prefix=pre, prefix_len=lens, repeat_guard=(P, 1))
            _guarded(m)
            got = toks.cpu().tolist()
            assert got[0][0] == case.x and guard_ref.banned(h, P, 1) == set(case.letters)
            for r, hh in enumerate([h, (), h[:7]]):
                assert got[r] == _expect(script, hh, n, P, 1), (P, r, got[r])
            if dtype == "fp32":
                free = m.generate(img, n, prefix=pre, prefix_len=lens)
                assert free.cpu().tolist()[0] == [case.letters[0]] * n                      # vacuity: unguarded, the first rank at every pick
                ts = m.generate(img, n, prefix=pre, prefix_len=lens, decode="sample", temp=0.3, seed=5, repeat_guard=(P, 1))
                _guarded(m)
                tk, masked, rr, tt = ts.cpu().numpy(), [], [], []
                for r, hh in enumerate([h, (), h[:7]]):
                    seq = [d.bos] + list(hh) + tk[r, :-1].tolist()
                    lg = ref64.decoder_net(s64, torch.tensor([seq], dtype=torch.int64), enc64[r:r + 1])[0, len(hh):].float().numpy()
                    for j in range(n):
                        masked.append(guard_ref.mask(lg[j], seq[1:1 + len(hh) + j], P, 1)[0])
                        rr.append(r)
                        tt.append(len(hh) + j)
                assert tk[0, 0] == case.x                                                    # four bans in the map, and the sampler read them
                check_draws(f"guard zoo ruler V={case.vocab} ({P}, 1) {_form(case.vocab)}", tk.reshape(-1), np.stack(masked), 0.3, 5,
                            np.asarray(rr), np.asarray(tt))
    print(f"\n[guard] ruler V={case.vocab} ({case.stream}): ban set {sorted(case.letters)} by periods [1, 2, 4, 8], pick {case.x}")


# ---- 3. long free-running decodes, every pick replayed -------------------------------------------------------------------------------------
def _replayed(m, img, n, g, script, tag):
    toks, logits = m.generate(img, n, return_logits=True, repeat_guard=g)
    _guarded(m)
    assert toks.shape == (img.shape[0], n)
    want, bound, yields, _ = replay_greedy(*g, logits, toks)
    tk = toks.cpu().numpy()
    assert np.array_equal(tk, want) and yields == 0, tag
    assert bool(bound.any()), f"{tag}: the raw arg-max was never banned"
    raw = logits.float().cpu().numpy().argmax(-1)
    periods = set()
    for b, t in zip(*np.nonzero(bound)):
        periods |= _in_force(tk[b, :t], raw[b, t], *g)
    assert guard.violations(tk, *g) == [[]] * tk.shape[0], tag
    return tk, bound, periods


@pytest.mark.parametrize("g", gz.LOOP_GUARDS, ids=str)
@pytest.mark.parametrize("period", sorted(gz.LOOPS))
def test_long_decode_every_pick_is_the_replay(period, g):
    """scripts of period 5, 8, 16 decoded for 300 positions under (16, 3), (8, 16), (16, 16): every pick is test_gpu_guard.replay_greedy's
    on the engine's own logits, none skipped, and, in fp32, the host's from the script.  The script's own period is among the periods in
    force wherever the guard admits it ((8, 16) admits no period 16: nothing binds, and the decode is the script); under (16, 16) the
    period-16 script binds for the first time at position 271, behind 255 comparisons"""
    L = gz.LOOPS[period]
    d = gz.dims(L.vocab, gz.TABLE)
    script = gz.loop_script(L.block, L.escapes, gz.TABLE)
    img = rgb_images(2, 32, 48, 13).cuda()
    n = 300
    for dtype in ("fp32", "bf16") if g == (16, 3) or (g, period) == ((16, 16), 16) else ("fp32",):
        m = _model(d, script, dtype)
        if period > g[0]:
            toks, logits = m.generate(img, n, return_logits=True, repeat_guard=g)
            _guarded(m)
            want, bound, _, _ = replay_greedy(*g, logits, toks)
            assert np.array_equal(toks.cpu().numpy(), want) and not bound.any() and toks.cpu().tolist()[0] == gz.first_choices(script, n)
            continue
        tk, bound, periods = _replayed(m, img, n, g, script, (period, g, dtype))
        assert period in periods, (period, g, periods)
        first = int(np.nonzero(bound.any(0))[0][0])
        assert first == (g[1] + 1) * period - 1, first              # behind R * p - 1 matches and the p tokens they are counted against
        scan = max(g[1] * p - 1 for p in periods)
        if dtype == "fp32":
            assert tk.tolist() == [_expect(script, (), n, *g, banned=guard.banned)] * 2
            free = m.generate(img, n)
            assert all(guard.violations(free.cpu().numpy(), *g)), "the free decode does not loop: the case is vacuous"
        print(f"\n[guard] loop {period} {g} {dtype}: periods in force {sorted(periods)}, first ban at position {first}, longest binding scan "
              f"{scan} comparisons, the guard decided {int(bound.sum())} of {bound.size} picks")
        if g == (16, 16) and period == 16:
            assert scan == 255 and first == 271


def test_long_decode_in_the_sliding_window():
    """a positional table of 64 entries, V = 64 (a multiple of 8), 300 positions under (16, 3): 236 picks lie in the sliding window, where
    every pick reads the last slot's ranking and the guard alone makes the sequence (c^3 e c^3 e c^3 then both are banned, ...); the history
    is the whole output, not the window.  Every pick is the replay, each row equals its image alone, and the script's period 5 is in force
    inside the table"""
    L, g, n = gz.LOOPS[5], (16, 3), 300
    d = gz.dims(64, 64)
    script = gz.loop_script(L.block, L.escapes, 64)
    m = _model(d, script)
    img = rgb_images(2, 32, 48, 13).cuda()
    tk, bound, periods = _replayed(m, img, n, g, script, "window")
    assert {1, 5} <= periods and bool(bound[:, 64:].any()), periods
    assert tk.tolist() == [_expect(script, (), n, *g, banned=guard.banned)] * 2
    for r in range(2):
        assert torch.equal(m.generate(img[r:r + 1], n, repeat_guard=g)[0].cpu(), torch.from_numpy(tk[r])), r
    print(f"\n[guard] sliding window (16, 3): periods in force {sorted(periods)}, {int(bound[:, 64:].sum())} binding picks beyond the table")


@pytest.mark.parametrize("vocab", [67, 1000, 1030])
def test_long_decode_sampled(vocab):
    """one sampled decode per sampler form (one-logit loads, 16-byte loads, LDS), period 8 under (8, 3), 120 positions at temperature 0.5:
    every draw is sampler_ref's on the guard-masked row of the engine's own logits"""
    L = gz.loop(8, vocab)
    d = gz.dims(vocab, gz.TABLE)
    script = gz.loop_script(L.block, L.escapes, gz.TABLE)
    m = _model(d, script)
    B, n, g, seed = 2, 120, (8, 3), 2 ** 32 + 5
    img = rgb_images(B, 32, 48, 13).cuda()
    toks, logits = m.generate(img, n, temp=0.5, decode="sample", seed=seed, return_logits=True, repeat_guard=g)
    _guarded(m)
    tk, lg = toks.cpu().numpy(), logits.float().cpu().numpy()
    masked, n_ban, periods = np.empty_like(lg), 0, set()
    for b in range(B):
        for t in range(n):
            masked[b, t], ban, y = guard_ref.mask(lg[b, t], tk[b, :t], *g)
            assert not y
            if int(lg[b, t].argmax()) in ban:
                n_ban += 1
                periods |= _in_force(tk[b, :t], lg[b, t].argmax(), *g)
    assert n_ban >= B and 8 in periods, (n_ban, periods)
    check_draws(f"guard zoo loop V={vocab}", tk, masked.reshape(-1, vocab), 0.5, seed, np.repeat(np.arange(B), n), np.tile(np.arange(n), B))
    assert guard.violations(tk, *g) == [[]] * B
    print(f"\n[guard] sampled loop V={vocab} ({_form(vocab)}): {n_ban} picks whose arg-max was banned, periods in force {sorted(periods)}")


# ---- 4. plumbing at long reach ---------------------------------------------------------------------------------------------------------
PLUMB_G = (8, 3)                                                   # reach 31 tokens: more than one compaction interval of 16
PLUMB_TABLE = gz.PLUMB_TABLE


def _check_rows(got, script, hists, n, eos, pad, guarded=True):
    viol = 0
    for r, h in enumerate(hists):
        want = _expect(script, h, n, *(PLUMB_G if guarded else (0, 0)), eos=eos, banned=guard.banned)
        row = got[r]
        if guarded:
            assert row[:len(want)] == want and all(x == pad for x in row[len(want):]), (r, row, want)
        kept = list(h) + (row[:row.index(eos) + 1] if eos is not None and eos in row else row)
        viol += len([i for i in guard.violations(kept, *PLUMB_G, eos)[0] if i >= len(h)])
        if guarded and r % 5 == 0:
            assert [i for i in guard_ref.violations(kept, *PLUMB_G, eos) if i >= len(h)] == [], r
    return viol


def test_row_stop_with_compactions_at_long_reach():
    """stop='row' with a compaction every other position, 40 rows that end between position 33 and 135: a row's history behind a compaction
    is read by its row of the BATCH, 31 tokens back.  Every row is the host's and equals its own solo call bit for bit; unguarded, the
    same call violates"""
    B, n = 40, 100
    d = gz.dims(64, PLUMB_TABLE)
    script, hists = gz.staggered(gz.LOOPS[8], B, eos=d.eos)
    m = _model(d, script, max_batch=B, env=STOP_ENV, eos=d.eos)
    img = rgb_images(B, 32, 48, 81).cuda()
    pre, lens = _prefix(d, hists)
    toks = m.generate(img, n, prefix=pre, prefix_len=lens, stop="row", repeat_guard=PLUMB_G)
    _guarded(m)
    assert m._engine.query(Q_LAST_COMPACTIONS) >= 1
    got = toks.cpu().tolist()
    assert _check_rows(got, script, hists, n, d.eos, d.pad) == 0
    ends = {len(h) + row.index(d.eos) for h, row in zip(hists, got)}
    assert len(ends) >= 10 and max(ends) - min(ends) >= 64, ends  # rows end at different positions: rows move while others still scan
    for r in range(B):
        t1 = m.generate(img[r:r + 1], n, prefix=pre[r:r + 1, :lens[r]], stop="row", repeat_guard=PLUMB_G)
        k = min(toks.shape[1], t1.shape[1])
        assert torch.equal(toks[r, :k], t1[0, :k]) and bool((toks[r, k:] == d.pad).all()), r
    m.eos_token = None                                            # vacuity: without eos and guard the rows loop on
    free = m.generate(img, n, prefix=pre, prefix_len=lens).cpu().tolist()
    assert _check_rows(free, script, hists, n, None, d.pad, guarded=False) > 0


def test_row_ranges_captured_steps_and_ragged_at_long_reach():
    """TXO_LANES=2 (40 rows), TXO_GRAPH=1 against 0, generate_ragged on three sizes: under a period-8 script and guard (8, 3), behind
    prefixes that differ per row.  Each result is the host's, equals every row decoded alone bit for bit, and the unguarded call violates"""
    B, n = 40, 80
    d = gz.dims(64, PLUMB_TABLE)
    script, hists = gz.staggered(gz.LOOPS[8], B)
    m = _model(d, script, max_batch=B)
    img = rgb_images(B, 32, 48, 81).cuda()
    pre, lens = _prefix(d, hists)
    with knobs(TXO_LANES=2):
        toks, logp, _ = m.generate(img, n, prefix=pre, prefix_len=lens, return_logp=True, repeat_guard=PLUMB_G)
        assert m._engine.query(Q_LAST_ROW_RANGES) == 2
    _guarded(m)
    assert _check_rows(toks.cpu().tolist(), script, hists, n, None, d.pad) == 0
    for r in range(B):
        t1 = m.generate(img[r:r + 1], n, prefix=pre[r:r + 1, :lens[r]], repeat_guard=PLUMB_G)
        assert torch.equal(toks[r], t1[0]), r                     # (tokens: alone, the multi-position pass takes the row's whole prefix)
    free = m.generate(img, n, prefix=pre, prefix_len=lens).cpu().tolist()
    assert _check_rows(free, script, hists, n, None, d.pad, guarded=False) > 0
    # captured steps
    with knobs(TXO_GRAPH=1):
        tg, lg, _ = m.generate(img, n, prefix=pre, prefix_len=lens, return_logp=True, repeat_guard=PLUMB_G)
    with knobs(TXO_GRAPH=0):
        te, le, _ = m.generate(img, n, prefix=pre, prefix_len=lens, return_logp=True, repeat_guard=PLUMB_G)
    assert torch.equal(tg, te) and torch.equal(lg, le) and torch.equal(te, toks)
    # a ragged batch of three sizes behind three different prefixes: each row is the host's and its own solo call
    imgs = [rgb_images(1, h, w, 91 + i)[0].cuda() for i, (h, w) in enumerate([(32, 64), (48, 48), (16, 32)])]
    pick = [5, 17, 30]
    rpre, rlens = _prefix(d, [hists[r] for r in pick])
    tr = m.generate_ragged(imgs, n, prefix=rpre, prefix_len=rlens, repeat_guard=PLUMB_G)
    _guarded(m)
    assert _check_rows(tr.cpu().tolist(), script, [hists[r] for r in pick], n, None, d.pad) == 0
    for i, im in enumerate(imgs):
        t1 = m.generate(im[None], n, prefix=rpre[i:i + 1, :rlens[i]], repeat_guard=PLUMB_G)
        assert torch.equal(tr[i], t1[0]), i
    assert _check_rows(m.generate_ragged(imgs, n, prefix=rpre, prefix_len=rlens).cpu().tolist(), script, [hists[r] for r in pick], n, None, d.pad,
                       guarded=False) > 0
