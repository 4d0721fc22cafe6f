"""tests/guard_zoo.py pinned on the host: the scripted decoders on oracle/cpu_ref.py (the free greedy decode is the script's first choices,
consecutive ranks lie >= 100 x the bf16 logit error apart), every generated history's ban set on tests/guard_ref.py (brute force) and
texocr_amd.guard.banned on it, the window csrc/beam_guard.h stages, and where the cases' bans fall in the kernels' bit map."""
import numpy as np
import pytest
import torch

import guard_ref
import guard_zoo as gz
from oracle import cpu_ref
from texocr_amd import guard, synth

MIN_GAP = 100 * gz.BF16_LOGIT_ERROR


def _scripts():
    """(name, dims, script, positions decoded) of every script the GPU tests build"""
    out = [("boundary", gz.dims(gz.BOUNDARY_V, gz.TABLE), gz.const_script(gz.BOUNDARY_RANKING, gz.TABLE), gz.TABLE)]
    for r in gz.RULERS:
        out.append((f"ruler V={r.vocab}", gz.dims(r.vocab, 32, r.low_specials), gz.const_script(r.letters + (r.x,), 32), 32))
    for p, L in gz.LOOPS.items():
        out.append((f"loop {p}", gz.dims(L.vocab, gz.TABLE), gz.loop_script(L.block, L.escapes, gz.TABLE), 300))
    out.append(("loop 5, table 64", gz.dims(64, 64), gz.loop_script(gz.LOOPS[5].block, gz.LOOPS[5].escapes, 64), 64))
    for eos in (None, 61):
        out.append((f"staggered eos={eos}", gz.dims(64, gz.PLUMB_TABLE), gz.staggered(gz.LOOPS[8], 2, eos)[0], gz.PLUMB_TABLE))
    for p, V in ((8, 64), (16, 67), (5, 1100), (8, 1100), (16, 64), (5, 67)):       # the beam tests: a table of 64 entries
        L = gz.loop(p, V)
        out.append((f"beam loop {p} V={V}", gz.dims(V, 64), gz.loop_script(L.block, L.escapes, 64), 64))
    L = gz.LOOPS[8]
    out.append(("beam loop 8, eos second at 0", gz.dims(64, 64), gz.loop_script(L.block, L.escapes, 64, at={0: [L.block[0], 61] + list(L.escapes[:2])}), 64))
    for V in (67, 1000, 1030):
        L = gz.loop(8, V)
        out.append((f"loop 8 V={V}", gz.dims(V, gz.TABLE), gz.loop_script(L.block, L.escapes, gz.TABLE), 300))
    return out


@pytest.mark.parametrize("case", _scripts(), ids=lambda c: c[0])
def test_the_oracle_decodes_the_script_with_a_wide_margin(case):
    name, d, script, n = case
    sd = cpu_ref.to_torch_sd(gz.scripted_sd(d, script))
    img = torch.from_numpy(synth.synth_images(2, 3, 32, 48, seed=13))
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, None, n, collect_logits=True)
    assert np.array_equal(toks.numpy(), np.asarray([gz.first_choices(script, n)] * 2)), name
    lg = logits.numpy()
    gap = np.inf
    for t in range(n):
        r = list(script[t])
        ranked = lg[:, t, r]
        others = np.delete(lg[:, t], r, axis=1).max(1)
        steps = np.concatenate([ranked[:, :-1] - ranked[:, 1:], (ranked[:, -1] - others)[:, None]], 1)
        gap = min(gap, float(steps.min()))
    print(f"\n[guard zoo] {name}: smallest gap between consecutive ranks {gap:.3f} (required {MIN_GAP})")
    assert gap >= MIN_GAP, (name, gap)


def _both(h, P, R, eos=None):
    ban = guard_ref.banned(h, P, R, eos)
    assert guard.banned(h, P, R, eos) == ban, (h, P, R)
    return ban


def test_boundary_histories():
    """(i) and (iii) do not ban the block's first token, (ii) and the twin do; their m_p are R * p - 2 and >= R * p - 1; the block's
    tokens are distinct, so only period p can ban its first token (a shorter period bans a filler at most)"""
    longest = 0
    for R in gz.REPEATS:
        for p, kind, h in gz.boundary_rows(R):
            a = gz.boundary_block(p)[0]
            ban = _both(h, p, R)
            m = gz.trailing_matches(h, p)
            if kind in ("under", "broken"):
                assert (m == R * p - 2 or (len(h) == 0 and R * p == 1)) and a not in ban, (p, R, kind)   # ((1, 1): the empty history)
            else:
                assert m == R * p - 1 and a in ban, (p, R, kind)
                longest = max(longest, R * p - 1)
            if kind == "broken":
                n = len(h)
                assert h[n - R * p + 1] != h[n - R * p + 1 - p] and n - R * p + 1 - p == 0       # the last compared pair
            if kind == "twin":
                n = len(h)
                assert h[n - R * p] != h[n - R * p - p] and n - R * p - p == 0                   # one pair further back: never compared
        assert len(gz.boundary_rows(R)) <= 64 - 1
    assert longest == 255
    assert max(len(h) for R in gz.REPEATS for _, _, h in gz.boundary_rows(R)) + 1 + 16 <= gz.TABLE   # bos + the longest prefix + p picks fit the table
    assert [k for p, k, _ in gz.boundary_rows(1) if p == 1] == ["under", "at", "twin"]               # (1, 1) compares nothing: no (iii)


def test_ruler():
    for r in gz.RULERS:
        h = gz.ruler(*r.letters)
        for P in (8, 16):
            assert _both(h, P, 1) == set(r.letters)
        assert [p for p in range(1, 17) if guard_ref.ends_in_copies(list(h) + [h[len(h) - p]], p, 2)] == [1, 2, 4, 8]
        assert _both(h, 7, 1) == set(r.letters[:3]) and _both(h, 8, 2) == set()
        assert r.x not in h and not ({r.x, *r.letters} & gz.specials(gz.dims(r.vocab, 32, r.low_specials)))


def _histories(P, R, rng):
    W = gz.window(P, R)
    out = [gz.periodic(tuple(range(P)), W), gz.periodic(tuple(range(P)), W + 7), gz.ruler(0, 1, 2, 3) * 3]
    for Rr in gz.REPEATS:
        out += [h for _, _, h in gz.boundary_rows(Rr)]
    for _ in range(6):
        out.append(tuple(rng.integers(0, 3, int(rng.integers(1, 2 * W + 4))).tolist()))
    for _ in range(6):                                            # noisy periodic ones: long runs that break somewhere
        q = int(rng.integers(1, P + 1))
        h = np.asarray(gz.periodic(tuple(rng.integers(0, 3, q).tolist()), int(rng.integers(W, 2 * W + 4))))
        h[rng.integers(0, len(h), 1 + len(h) // 64)] = 2
        out.append(tuple(h.tolist()))
    return out


@pytest.mark.parametrize("P", [1, 2, 3, 5, 8, 15, 16])
def test_the_beam_window_is_as_far_as_any_scan_looks(P):
    """banned(h) == banned(h[-W:]) with W = (R + 1) * P - 1, and one history per (P, R) for which W - 1 tokens are not enough"""
    rng = np.random.default_rng(100 + P)
    for R in (1, 2, 3, 5, 8, 15, 16):
        W = gz.window(P, R)
        for h in _histories(P, R, rng):
            assert guard.banned(h, P, R) == guard.banned(h[-W:], P, R), (P, R, h)
        for h in _histories(P, R, rng)[:12]:
            assert guard_ref.banned(h, P, R) == guard_ref.banned(h[-W:], P, R) == guard.banned(h, P, R), (P, R, h)
        h = gz.periodic(tuple(range(P)), W)
        assert 0 in guard_ref.banned(h, P, R) and 0 not in guard_ref.banned(h[-(W - 1):] if W > 1 else (), P, R), (P, R)   # (R = 1: period 1 bans the last token as well)


def test_ban_placement():
    """where the cases' bans fall in the V-bit map of guard_stage: a case list that loses one of these fails here"""
    bans = {r.vocab: set(r.letters) for r in gz.RULERS}
    last = {r.vocab: max(set(range(r.vocab)) - gz.specials(gz.dims(r.vocab, 32, r.low_specials))) for r in gz.RULERS}
    assert any(0 in b for b in bans.values())
    assert all(last[V] in b for V, b in bans.items())                                      # the last ordinary id, at every vocabulary
    assert last[67] == 66 and gz.in_partial_word(bans[67], 67) and gz.in_partial_word(bans[1030], 1030)
    assert sum(v >= 64 for v in bans[67]) == 2 and sum(v >= 1024 for v in bans[1030]) == 2  # two lanes, one partial word
    assert all(gz.share_word(b) for b in bans.values())
    assert all(gz.share_request(b) for V, b in bans.items() if V % 4 == 0) and {64, 1000} <= {V for V in bans if V % 4 == 0}
    assert all(len(b) == 4 for b in bans.values())                                         # ban sets of more than two tokens
    # the boundary table bans id 0; its ranking holds 0 and 1 (one request) and the last ordinary id
    a, b, c = gz.BOUNDARY_RANKING[:3]
    assert a == 0 and (a >> 2) == (b >> 2) and c == gz.BOUNDARY_V - 4 and not set(gz.BOUNDARY_RANKING) & (set(gz.FILLERS) | {gz.ODD})
    # the loops: a block's tokens share words and requests; the first escape is the last ordinary id
    for L in list(gz.LOOPS.values()) + [gz.loop(8, 1000), gz.loop(8, 1030)]:
        assert gz.share_word(set(L.block)) and 0 in L.block and L.escapes[0] == L.vocab - 4
        assert not set(L.block) & set(L.escapes) and not (set(L.block) | set(L.escapes)) & gz.specials(gz.dims(L.vocab, 64))
