"""tests/logit_scripts.py proven from its own restatement: every script puts its maximum -- or each member of its tie -- in the sweep, lane,
slot, tile or thread it is listed for; the restated constants are the headers' own; every script that is not a tie is decided by >= 1e-3 in
float64; the host rule alone keeps the sampler scripts under the in-band cap tests/test_gpu_sampler.py applies."""
import os
import re

import numpy as np
import pytest

import logit_scripts as ls
import sampler_ref as sr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "texocr_amd", "csrc")
BAND, ROWS, STEPS = 2e-5, 21, 24                      # tests/test_gpu_sampler.py


def _text(header):
    return open(os.path.join(CSRC, header)).read()


def test_restated_constants_are_the_headers():
    step = _text("step.h")
    assert ls.SR_PER == int(re.search(r"constexpr int SR_PER = (\d+);", step).group(1)) == 16
    assert ls.VPT == int(re.search(r"constexpr int VPT = (\d+);", step).group(1)) == 4
    assert ls.SC_VT == int(re.search(r"constexpr int SC_VT = (\d+);", _text("score.h")).group(1)) == 4
    assert "for (int v0 = 0; v0 < V; v0 += 16 * SC_VT)" in _text("score.h") and "const int v = v0 + j * 16 + lg * 4 + r;" in _text("score.h")
    assert "return V <= 64 * SR_PER && !TXO_SAMPLER_LDS;" in step and "if (V <= 256 * VPT) {" in step
    assert "if ((V & 3) == 0 && (per & 3) == 0) {" in step and "const int per = (V + 63) / 64, j0 = lane * per;" in step
    # the greedy stream and its copies: 256 float4 per sweep, four unroll slots of 64 lanes -- step.h, step_prefix.h, twice step_rules.h,
    # step_guard.h, and the pick stage of persist.h
    copies = {"step.h": 1, "step_prefix.h": 1, "step_rules.h": 2, "step_guard.h": 1, "persist.h": 1}
    for header, n in copies.items():
        text = _text(header)
        assert len(re.findall(r"for \(int base = 0; base < n4; base \+= (\d+)\)", text)) == n, header
        assert {int(x) for x in re.findall(r"base < n4; base \+= (\d+)\)", text)} == {ls.SWEEP4}, header
        assert text.count("const int j4 = base + u * 64 + lane;") >= n, header
    assert ls.SWEEP4 == ls.UNROLL * ls.LANES


def test_the_walks_restated():
    g = ls.greedy_place
    # the float4 stream: (f4, sweep, unroll slot, lane, component)
    assert g(1024, 0) == (True, 0, 0, 0, 0) and g(1024, 3) == (True, 0, 0, 0, 3) and g(1024, 4) == (True, 0, 0, 1, 0)
    assert g(1024, 252) == (True, 0, 0, 63, 0) and g(1024, 255) == (True, 0, 0, 63, 3) and g(1024, 256) == (True, 0, 1, 0, 0)
    assert g(1024, 1020) == (True, 0, 3, 63, 0) and g(1024, 1023) == (True, 0, 3, 63, 3)                 # lane 63's last slot
    assert g(1028, 1024) == (True, 1, 0, 0, 0) and g(1028, 1027) == (True, 1, 0, 0, 3)                   # the second sweep: ONE float4, lane 0
    assert g(2048, 2047) == (True, 1, 3, 63, 3) and g(2052, 2048) == (True, 2, 0, 0, 0) and g(2052, 2051) == (True, 2, 0, 0, 3)
    assert [ls.greedy_sweeps(V) for V in (64, 960, 1024, 1028, 2048, 2052)] == [1, 1, 1, 2, 2, 3]
    # the scalar loop: (f4, iteration, 0, lane, 0)
    assert g(63, 62) == (False, 0, 0, 62, 0) and g(65, 64) == (False, 1, 0, 0, 0) and g(1025, 1024) == (False, 16, 0, 0, 0)
    assert g(1027, 1023) == (False, 15, 0, 63, 0) and g(1027, 1026) == (False, 16, 0, 2, 0)
    assert [ls.greedy_place(V, 0).f4 for V in ls.VOCABS] == [V % 4 == 0 for V in ls.VOCABS]
    # the sampler: form, chunk, real slots of a lane
    forms = {63: "regs1", 64: "regs1", 65: "regs1", 128: "regs1", 129: "regs1", 960: "regs1", 1024: "regs16", 1025: "lds", 1027: "lds",
             1028: "lds", 2048: "lds", 2052: "lds"}
    assert {V: ls.sampler_form(V) for V in ls.VOCABS} == forms
    assert [ls.sampler_per(V) for V in (63, 64, 65, 960, 1024, 1025)] == [1, 1, 2, 15, 16, 17]
    assert [ls.sampler_nin(65, l) for l in (0, 31, 32, 33, 63)] == [2, 2, 1, 0, 0]                        # lanes 33 - 63 empty
    assert ls.sampler_nin(63, 62) == 1 and ls.sampler_nin(63, 63) == 0 and ls.sampler_nin(960, 63) == 15 and ls.sampler_nin(1025, 60) == 5
    assert ls.sampler_place(1024, 15) == (0, 15) and ls.sampler_place(1024, 16) == (1, 0) and ls.sampler_place(1025, 1024) == (60, 4)
    # the beam selection: (registers, thread, register, wave)
    b = ls.beam_place
    assert b(1024, 255) == (True, 255, 0, 3) and b(1024, 256) == (True, 0, 1, 0) and b(1024, 767) == (True, 255, 2, 3)
    assert b(1024, 768) == (True, 0, 3, 0) and b(1024, 1023) == (True, 255, 3, 3)                        # thread 255's fourth register
    assert b(1025, 1024) == (False, 0, 4, 0) and b(1025, 1023, parent=1) == (False, 0, 8, 0) and b(1025, 255) == (False, 255, 0, 3)
    # the score walk: (tile, j, lane group, r)
    s = ls.score_place
    assert s(129, 0) == (0, 0, 0, 0) and s(129, 4) == (0, 0, 1, 0) and s(129, 8) == (0, 0, 2, 0) and s(129, 12) == (0, 0, 3, 0)
    assert s(129, 16) == (0, 1, 0, 0) and s(129, 63) == (0, 3, 3, 3) and s(129, 64) == (1, 0, 0, 0) and s(129, 128) == (2, 0, 0, 0)
    assert {V: (ls.score_tiles(V), ls.score_clamped_rows(V)) for V in ls.SCORE_VOCABS} == {
        63: (1, 1), 64: (1, 0), 65: (2, 63), 128: (2, 0), 129: (3, 63), 1027: (17, 61)}


def _by_name(scripts):
    return {s.name: s for s in scripts}


def test_every_gap_the_suite_had_has_its_script():
    """the placements the random-weight rows never controlled, each named with the script that holds its maximum there"""
    g = {V: _by_name(ls.greedy_scripts(V)) for V in ls.VOCABS}
    for V in (64, 128, 960, 1024, 1028, 2048, 2052):                       # the last float4 of a row
        p = ls.greedy_place(V, g[V][f"max{V - 1}"].top[0])
        assert p.f4 and (p.sweep * ls.SWEEP4 + p.slot * ls.LANES + p.lane, p.comp) == (ls.n4(V) - 1, 3)
    for V in (1028, 2048, 2052):                                           # the first float4 of the second sweep
        assert ls.greedy_place(V, g[V]["max1024"].top[0])[:4] == (True, 1, 0, 0)
    for V in (1024, 1028, 2048):                                           # lane 63's last slot
        assert ls.greedy_place(V, g[V]["max1023"].top[0]) == (True, 0, 3, 63, 3)
    for V in (63, 65, 129, 1025, 1027):                                    # behind V - 1 of a vocabulary that is no multiple of 4
        s = g[V][f"max{V - 1}"]
        assert not ls.greedy_place(V, s.top[0]).f4 and s.top[0] == V - 1
    assert ls.greedy_place(1025, 1024).sweep == 16 and ls.greedy_place(1027, 1026).sweep == 16      # scalar branch beyond one sweep of 1024
    sc = {V: _by_name(ls.score_scripts(V)) for V in ls.SCORE_VOCABS}
    for V in (65, 129, 1027):                                              # the tail tile of the score walk
        assert ls.score_place(V, sc[V][f"max{V - 1}"].top[0]).tile == ls.score_tiles(V) - 1 and ls.score_clamped_rows(V) > 0
    assert ls.score_place(63, sc[63]["max62"].top[0]) == (0, 3, 3, 2) and ls.score_clamped_rows(63) == 1
    bm = _by_name(ls.beam_scripts(1024))                                   # thread 255's fourth register
    assert ls.beam_place(1024, bm["max1023"].top[0]) == (True, 255, 3, 3) and ls.beam_place(1024, bm["max768"].top[0]) == (True, 0, 3, 0)
    # ties across lanes, unroll slots, sweeps, waves of the beam block, threads, lane groups and tiles
    a, b = g[1028]["tie1023_1024"].top[:2]
    assert ls.greedy_place(1028, a).sweep == 0 and ls.greedy_place(1028, b).sweep == 1
    a, b = g[1024]["tie255_256"].top[:2]
    assert (ls.greedy_place(1024, a).lane, ls.greedy_place(1024, a).slot) == (63, 0) and (ls.greedy_place(1024, b).lane, ls.greedy_place(1024, b).slot) == (0, 1)
    assert (ls.beam_place(1024, 255).wave, ls.beam_place(1024, 256).wave) == (3, 0)
    assert (ls.beam_place(1024, 767).thread, ls.beam_place(1024, 1023).thread) == (255, 255)             # one thread, two registers
    for V in ls.SCORE_VOCABS:
        pairs = {(ls.score_place(V, a).lg, ls.score_place(V, b).lg) for a, b in ls.score_pairs(V) if ls.score_place(V, a).tile == ls.score_place(V, b).tile and b < 17}
        assert {(0, 1), (0, 2), (1, 2), (3, 0)} <= pairs, (V, pairs)                                       # xor16, xor32, both, and the higher group first
    assert ls.score_place(129, 63).tile == 0 and ls.score_place(129, 64).tile == 1 and (63, 64) in ls.score_pairs(129)
    for V in (64, 128, 960, 1024):                                         # the sampler's last two chunks: lanes 62 | 63
        per = ls.sampler_per(V)
        assert (63 * per - 1, 63 * per) in ls.tie_pairs(V)
        assert ls.sampler_place(V, 63 * per - 1) == (62, per - 1) and ls.sampler_place(V, 63 * per) == (63, 0)


@pytest.mark.parametrize("V", list(ls.VOCABS))
def test_every_script_is_what_it_says(V):
    scripts = ls.greedy_scripts(V) + (ls.score_scripts(V) if V in ls.SCORE_VOCABS else []) + (ls.beam_scripts(V) if V in ls.BEAM_VOCABS else [])
    assert len({s.name for s in ls.greedy_scripts(V)}) == len(ls.greedy_scripts(V))
    names = {s.name for s in ls.greedy_scripts(V)}
    assert {f"max{i}" for i in (0, 3, 4, V - 4, V - 2, V - 1)} <= names and "equal" in names and {f"tie0_{V - 1}", f"tie{V - 2}_{V - 1}"} <= names
    assert all(f"max{i}" in names for i in ls.SINGLES if i < V) and (("tie255_256" in names) == (V > 256)) and (("tie1023_1024" in names) == (V > 1024))
    assert any(s.kind == "wide" for s in ls.greedy_scripts(V)) == (V > 1024)
    for s in scripts:
        row = s.row
        assert row.dtype == np.float32 and row.shape == (V,) and bool(np.isfinite(row).all()) and float(np.abs(row).max()) <= 1e4
        e = ls.expect(row)
        assert e.pick == s.top[0], s.id
        order = np.argsort(-row.astype(np.float64), kind="stable")[:3]
        assert tuple(order.tolist()) == tuple(s.top), (s.id, order, s.top)                  # first, runner-up, third -- ties lowest index first
        if s.kind == "tie":
            a, b = s.top[:2]
            assert row[a].tobytes() == row[b].tobytes() and a < b and e.margin == 0.0, s.id
            assert row[s.top[1]] - row[s.top[2]] >= 1e-3
        elif s.kind == "equal":
            assert len({x.tobytes() for x in row}) == 1
        else:
            assert e.margin >= 1e-3, (s.id, e.margin)
            assert row[s.top[1]] - row[s.top[2]] >= 1e-3 and row[s.top[2]] - np.sort(row)[-4] >= 1e-3
            if s.kind == "single":                                                         # the runner-up sits across a seam: another lane or sweep
                p, q = ls.greedy_place(V, s.top[0]), ls.greedy_place(V, s.top[1])
                assert (p.sweep, p.slot, p.lane) != (q.sweep, q.slot, q.lane), s.id
        if s.kind == "wide":
            # (the maximum beyond the 1024 entries of the first sweep, the runner-up inside them; scalar rows: a later iteration of its lane)
            assert s.top[0] >= 4 * ls.SWEEP4 > s.top[1] and float(row.max() - row.min()) > 150
            assert ls.greedy_place(V, s.top[0]).sweep > ls.greedy_place(V, s.top[1]).sweep >= 0
        elif s.kind != "equal":
            assert float(np.abs(row).max()) < 16                                           # the premise of test_gpu_logp.SAME_LOGITS
        # the masked replays the GPU test asserts: second, then third
        rules = ls.ban_table(V, [s.top[0]])
        assert ls.replay(row, 4, rules=rules)[0].tolist() == [s.top[0], s.top[1], s.top[1], s.top[1]]
        assert ls.replay(row, 4, guard=ls.GUARD)[0].tolist() == [s.top[0], s.top[1], s.top[0], s.top[1]]
        assert ls.replay(row, 4, rules=rules, guard=ls.GUARD)[0].tolist() == [s.top[0], s.top[1], s.top[2], s.top[1]]
    if V in ls.CLOSE_VOCABS:
        s = ls.single(V, 1023)
        eos = V - 3
        toks = ls.replay(s.row, 4, rules=ls.ban_table(V, [s.top[0]], eos=eos), eos=eos, close=True)[0].tolist()
        assert toks == [s.top[0], s.top[1], s.top[1], eos]                                 # the budget binds at the last pick only
    assert (ls.greedy_place(1028, 0).f4, ls.greedy_place(1027, 0).f4) == (True, False)


@pytest.mark.parametrize("V", ls.SAMPLER_VOCABS)
def test_sampler_scripts_under_the_host_rule(V):
    k = sr.topk_of(V)
    per = ls.sampler_per(V)
    scripts = ls.sampler_scripts(V)
    assert scripts[0].pair == (per - 1, per) and ls.sampler_place(V, per - 1)[0] == 0 and ls.sampler_place(V, per) == (1, 0)     # j0 of lane 1
    assert (V != 1025) or scripts[1].pair == (1023, 1024)
    for s in scripts:
        a, b = s.pair
        kept = sr.kept_mask(s.row[None], k)[0]
        assert int(kept.sum()) == k and int((s.row > s.row[b]).sum()) == k - 1
        if s.zeros:                                        # equal as floats, ordered by their bits: +0.0 is the k-th largest, -0.0 is out
            assert s.row[a] == s.row[b] and np.signbit(s.row[a]) and not np.signbit(s.row[b]) and s.kept == b
            assert sr.order_keys(s.row[a:a + 1])[0] < sr.order_keys(s.row[b:b + 1])[0]
        else:
            assert s.row[a].tobytes() == s.row[b].tobytes() and s.kept == a
        assert kept[s.kept] and not kept[a + b - s.kept], s.id
        for temp, seed in ((0.3, 7), (1.0, 2 ** 32 + 5)):
            d = sr.draw(np.broadcast_to(s.row, (ROWS * STEPS, V)), temp, seed, np.repeat(np.arange(ROWS), STEPS), np.tile(np.arange(STEPS), ROWS))
            frac = float((d.dist <= BAND).mean())
            hits = int((d.token == s.kept).sum())
            print(f"{s.id} temp {temp}: {frac:.4%} of the host draws inside the band, {hits} draws on the kept member of the pair")
            assert frac < max(0.02, 8 * k * BAND), (s.id, frac)
            assert hits >= 1 and not (d.token == a + b - s.kept).any(), s.id              # the pair decides real draws
