"""The checkpoints of tests/history_cases.py reach every seam they are listed for, proven from the restated arithmetic of the
self-attention history, per storage type and form; the restated constants are read back from the headers.  On the float64 oracle alone:
the greedy decodes the GPU tests compare with and their margins, the floor of the one-key probe, and the schedule of the compaction
case."""
import os
import re

import pytest
import torch

import decode_cases as dc
import history_cases as hc
import ref64

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "texocr_amd", "csrc")
TYPES = ("fp32", "bf16")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_restated_constants_are_the_headers():
    eng, da, ps = _src("engine.hip"), _src("dec_attn.h"), _src("persist.h")
    assert "constexpr int NLS = sizeof(T) == 2 ? 8 : 16;" in eng and (hc.NLS["bf16"], hc.NLS["fp32"]) == (8, 16)
    assert "PS_ATTN(ATT_SELF, APRO_NONE, (sizeof(T) == 2 ? 8 : 16), s, t + 1);" in ps
    assert "constexpr int KPB = KPI * 4;" in da and "constexpr int KPI = 64 / LPR;" in da and "constexpr int LPR = DH / PER16;" in da
    assert "const int nslot = V_EARLY ? (L - base + KPB - 1) / KPB : NL;" in da
    assert "for (int base = NL * KPB, slot = 1; base < L; base += NL * KPB, slot ^= 1)" in da
    assert "int L = MODE == ATT_CROSS ? a.len : (FUSED ? t : t + 1);" in da
    assert "constexpr bool HIST_EARLY = COH && MODE == ATT_SELF && !FUSED && !BEAM;" in da
    assert "clamp_row = valid ? max(t - 1, 0) : 0;" in da and "min(key, a.lmax - 1)" in da
    assert "float m_run = (MODE == ATT_SELF && FUSED) ? s_new : -3.0e38f" in da
    assert "for (int base = KEYS_PER_PASS; base < L; base += KEYS_PER_PASS) __syncthreads();" in da
    assert {t: hc.kpb(t) for t in TYPES} == {"fp32": 16, "bf16": 32} and {t: hc.keys_per_pass(t) for t in TYPES} == {"fp32": 256, "bf16": 256}
    assert hc.LA_PATH_TILES == int(re.search(r"constexpr int LA_PATH_TILES = (\d+);", _src("lat_attn.h")).group(1))
    assert "Tmax <= 16 * waves * LA_PATH_TILES" in eng
    assert hc.POLL_AHEAD == int(re.search(r"CHUNK = \d+, AHEAD = (\d+);", _src("lanes.h")).group(1))
    from gpu_harness import STOP_ENV
    assert (int(STOP_ENV["TXO_STOP_EVERY"]), int(STOP_ENV["TXO_STOP_GAIN"])) == (hc.STOP_EVERY, hc.STOP_GAIN)


def test_the_table_and_the_checkpoints():
    assert hc.T_HIST == 520 and hc.CHECKPOINTS == (0, 1, 15, 16, 17, 31, 32, 33, 254, 255, 256, 257, 258, 511, 512, 513, 519)
    assert hc.PROBE_P == (0, 15, 16, 31, 32, 255, 256, 257, 511, 512, 518) and max(hc.CHECKPOINTS) == hc.T_HIST - 1
    for name in hc.WIDTHS:
        d, d1, d3 = hc.DIMS[name], hc.DIMS[name + "_1l"], hc.DIMS[name + "_t300"]
        assert (d.max_len, d1.max_len, d3.max_len) == (hc.T_HIST, hc.T_HIST, hc.T_LAT) and (d.dec_layers, d1.dec_layers, d3.dec_layers) == (2, 1, 2)
        assert d.canvas_hw == hc.IMG and d.vocab % 8 == 0                      # (the multi-position pass takes the vocabulary)
    c256, w64 = hc.DIMS["calib256"], hc.DIMS["w64_h2"]
    assert (c256.embed_dim, c256.dec_heads, w64.embed_dim, w64.dec_heads) == (256, 8, 64, 2)
    # the persistent launch is calib256's default at 5 rows in both types and at 128 bf16 rows; the 64-wide model has none
    assert all(dc.persist_usable(c256, t, r) for t, r in (("fp32", 5), ("bf16", 5), ("bf16", 128))) and not dc.persist_usable(w64, "fp32", 5, persist=1)
    assert set(hc.FIVE) == set(hc.ROWS128) == {0, 1} and len(hc.ROWS128) == 128 and all(hc.FIVE.count(s) >= 2 for s in (0, 1))
    assert dc.persist_usable(c256, "bf16", 72) and set(hc.ROWS72) == {0, 1} and len(hc.ROWS72) == 72


def test_persistent_attention_rounds():
    """what the three row counts of group B reach in PS_ATTN, restated from persist.h's team arithmetic (the constants and the lines are
    read back).  5 rows: one row per team, 8 pairs on 64 groups -- 8 idle groups count the tile's barriers through all three passes.
    128 rows: 16 rows per team (ONE 16-row tile), 128 pairs -- two full rounds per group (the barrier between two tiles of a group),
    no idle group.  72 rows: 9 rows per team, the second round has 8 pairs beside 8 idle groups"""
    ps = _src("persist.h")
    assert "constexpr int PS_TEAMS = 8, PS_TEAM_BLOCKS = 32," in ps and (hc.PS_TEAMS, hc.PS_TEAM_BLOCKS) == (8, 32)
    for line in ("const int rpt = (a.B + PS_TEAMS - 1) / PS_TEAMS;", "const int sa = grp * PS_TEAM_BLOCKS + rank;", "constexpr int NSB = PS_TEAM_BLOCKS * 2;",
                 "const int np_ = nr * HEADS;", "if (base_ + rank < np_) {", "if (p_ >= np_) dec_attn_idle<T, MODE, APRO, NLV>((LK), ts);",
                 "const int nrt = (nr + DG_BM - 1) / DG_BM;"):
        assert line in ps, line
    heads = hc.DIMS["calib256"].dec_heads
    assert hc.persist_attn_rounds(5, heads) == [(1, 1, [(8, 8)])] * 5
    assert hc.persist_attn_rounds(128, heads) == [(16, 1, [(64, 0), (64, 0)])] * 8
    assert hc.persist_attn_rounds(72, heads) == [(9, 1, [(64, 0), (8, 8)])] * 8
    # two 16-row tiles per team need more than 128 rows, which only the fp32 engine decodes on the persistent launch
    assert hc.persist_attn_rounds(136, heads) == [(17, 2, [(64, 0), (64, 0), (8, 8)])] * 8 and len(hc.ROWS136) == 136
    c256 = hc.DIMS["calib256"]
    assert dc.persist_usable(c256, "fp32", 136) and not dc.persist_usable(c256, "bf16", 136)
    assert all(tiles == 1 for rows in range(1, 129) for _, tiles, _ in hc.persist_attn_rounds(rows, heads))


@pytest.mark.parametrize("form", hc.KV_FORMS)
@pytest.mark.parametrize("dtype", TYPES)
def test_checkpoints_reach_every_seam_of_the_kv_forms(dtype, form):
    at = {t: hc.passes(dtype, form, t) for t in hc.CHECKPOINTS}
    count = {t: len(p) for t, p in at.items()}
    kpp, k = hc.keys_per_pass(dtype), hc.kpb(dtype)
    # the last position of one pass, the first of two, the first of three
    last1 = [t for t in hc.CHECKPOINTS if hc.hist_len(form, t) == kpp]
    first2 = [t for t in hc.CHECKPOINTS if hc.hist_len(form, t) == kpp + 1]
    first3 = [t for t in hc.CHECKPOINTS if hc.hist_len(form, t) == 2 * kpp + 1]
    assert len(last1) == len(first2) == len(first3) == 1
    assert (count[last1[0]], count[first2[0]], count[first3[0]]) == (1, 2, 3)
    assert at[last1[0]][-1] == hc.Pass(0, 0, hc.NLS[dtype], k)                  # every slot, the last one full
    assert at[first2[0]][-1] == hc.Pass(kpp, 1, 1, 1) and at[first3[0]][-1] == hc.Pass(2 * kpp, 0, 1, 1)
    assert [p.slot for p in at[first3[0]]] == [0, 1, 0]                          # the first reuse of statistics slot 0
    assert max(count.values()) == 3 and count[hc.T_HIST - 1] == 3
    # a full and a one-key last slot at the first slot boundary of this type's KPB
    fills = {(len(p), p[-1].nslot, p[-1].last_fill) for p in at.values()}
    assert {(1, 1, k), (1, 2, 1)} <= fills, (dtype, form, sorted(fills))
    # ... and the other type's boundary lies inside a slot here or on it: both KPB sizes are checkpoints in both types
    for other in (16, 32):
        assert {other, other + 1} <= {hc.hist_len(form, t) for t in hc.CHECKPOINTS}
    # the new key: spliced from t = 1 on (persistent), scored apart (fused: no cached key at t = 0), else read from the cache
    assert hc.new_key(form, 1) == {"plain": "cache", "fused": "apart", "masked": "cache", "persistent": "spliced"}[form]
    assert (hc.hist_len(form, 0) == 0) == (form == "fused") and at[0][0].nslot == (0 if form == "fused" else 1)
    # a group without a tile counts the tile's barriers at every checkpoint (dec_attn_idle)
    if form == "persistent":
        assert all(a == b for a, b in (hc.idle_barriers(dtype, form, t) for t in range(hc.T_HIST)))
    # the probe replaces keys on both sides of every seam: the last of a slot and the first of the next, of a pass and of the next
    assert {k - 1, k, kpp - 1, kpp, kpp + 1, 2 * kpp - 1, 2 * kpp} <= set(hc.PROBE_P)


@pytest.mark.parametrize("width,dtype", [(w, t) for w in hc.WIDTHS for t in TYPES])
def test_checkpoints_of_the_latent_self_form(width, dtype):
    d = hc.DIMS[width + "_t300"]
    ok = hc.lat_self_ok(d, dtype, hc.T_LAT)
    assert ok == ((width, dtype) != ("calib256", "bf16"))                        # four waves: the slot tables end at 256 positions
    assert hc.lat_self_ok(d, dtype, 256) and not hc.lat_self_ok(d, dtype, 513)
    if not ok:
        return
    shapes = {t: hc.lat_self_shape(t, d.embed_dim, dtype) for t in hc.CHECKPOINTS if t < hc.T_LAT}
    assert all(s.nw == 8 for s in shapes.values())
    assert {s.nt_w for s in shapes.values()} == {1, 2, 3}                        # rounds of 128 keys
    assert shapes[255].last_tile_keys == 16 and shapes[255].idle == 0 and shapes[256].last_tile_keys == 1 and shapes[256].idle == 7
    assert shapes[15].last_tile_keys == 16 and shapes[16].last_tile_keys == 1 and shapes[16].ntiles == 2
    assert hc.lat_self_shape(hc.T_LAT - 1, d.embed_dim, dtype).nt_w == 3


ORACLES = [n for w in hc.WIDTHS for n in (w, w + "_1l", w + "_t300", w + "_own")]


@pytest.mark.parametrize("name", ORACLES)
def test_oracle_margins(name):
    """the float64 greedy decode of the two images over the whole table.  The GPU tests compare fp32 tokens up to the first margin below
    2e-5 (assert_tokens_exact_up_to_margin); here: where that is, and that the two images are distinct sequences"""
    ref = hc.reference(name)
    d = hc.DIMS[name]
    assert ref.toks.shape == (2, d.max_len) and ref.logits.shape == (2, d.max_len, d.vocab)
    m = ref64.margins(ref.logits)
    small = [(int(b), int(t)) for b, t in (m < 2e-5).nonzero()]
    print(f"\n{name}: smallest top-1 / top-2 margin {ref.margin:.3e}; margins below 2e-5 at {small}")
    assert not small, (name, small)              # every fp32 token of the table is decided
    assert not torch.equal(ref.toks[0], ref.toks[1]) and bool((ref.prefix[:, 0] == d.bos).all())
    assert torch.equal(ref.prefix[:, 1:], ref.toks[:, :-1])


@pytest.mark.parametrize("name", [w + "_1l" for w in hc.WIDTHS])
def test_probe_floor(name):
    """float64 moves by >= 1e-3 at EVERY position from p on, for every probed p and both images: 'the logits differ' never rests on
    rounding; and nothing before p moves at all (the oracle is causal)"""
    base, moved = hc.probe(name)
    ref = hc.reference(name)
    assert float((base - ref.logits).abs().max()) < 1e-12                       # (the multi-position oracle is the cached one)
    worst = {}
    for p in hc.PROBE_P:
        x, lg = moved[p]
        assert int((x != ref.prefix).sum()) == 2 and bool((x[:, p] != ref.prefix[:, p]).all())
        assert torch.equal(lg[:, :p], base[:, :p])
        worst[p] = float((lg - base).abs().amax(-1)[:, p:].min())
    print(f"\n{name}: smallest max_v |dlogit| over (image, t >= p) per p: " + ", ".join(f"{p}: {v:.2e}" for p, v in worst.items()))
    assert min(worst.values()) >= hc.PROBE_FLOOR, worst


@pytest.mark.parametrize("width", hc.WIDTHS)
def test_own_key_model(width):
    """plain, masked and persistent forms: the last pass holds ONE key at t = 256 and t = 512, and that key is key t itself, whose token
    is also the step's input -- the probe cannot isolate it.  On the own-key model (k projection := q projection) float64 moves by more
    than twice the bf16 bound when that key is dropped, so the float64 bound alone tells, in both types"""
    name = width + "_own"
    for dtype in TYPES:
        for form in ("plain", "masked", "persistent"):
            for t in hc.OWN_T:
                assert hc.passes(dtype, form, t)[-1].nslot == 1 and hc.passes(dtype, form, t)[-1].last_fill == 1
                assert hc.passes(dtype, form, t)[-1].base == t
    _, sd, s64 = hc.weights(name)
    _, sd0, _ = hc.weights(width)
    changed = sorted(k for k in sd if not (sd[k] == sd0[k]).all())
    assert changed == [f"{hc.SELF_PREFIX}{s}.1.k.weight" for s in (0, 3)]
    ref = hc.reference(name)
    assert float((hc.without_own_key(s64, ref.prefix, ref.enc, ()) - ref.logits).abs().max()) < 1e-12
    effect = hc.own_key_effect(name, ref.toks)
    print(f"\n{name}: float64 max_v |dlogit| of dropping key t at t: {effect}")
    from gpu_harness import BF16_BOUND
    assert min(effect.values()) >= hc.OWN_FLOOR > 2 * BF16_BOUND["logits"]


def test_key_masks():
    masks = hc.key_masks()
    assert (~masks["holes"]).nonzero().flatten().tolist() == list(hc.MASKED_P) == [0, 255, 256, 511]
    assert (~masks["left_pad"]).nonzero().flatten().tolist() == list(range(40))
    assert set(hc.MASKED_P) <= set(hc.PROBE_P)
    # under the mask the reference moves where it is not masked itself (the mask is not a no-op), and is finite there
    for which, valid in masks.items():
        lg = hc.masked_reference("w64_h2", which)
        ref = hc.reference("w64_h2")
        after = [t for t in range(hc.T_HIST) if valid[t] and t > int((~valid).nonzero()[0])]
        assert bool(torch.isfinite(lg[:, valid]).all()) and float((lg - ref.logits)[:, after].abs().amax(-1).min()) > 1e-6


def test_compaction_schedule():
    d, _, _, want, lg, first = hc.stop_case()
    assert d.max_len == hc.T_LAT and want.shape == (hc.STOP_ROWS, hc.T_LAT)
    assert sum(0 <= f < 200 for f in first) >= 8, sorted(first)
    assert sum(f < 0 or f > 260 for f in first) >= 8, sorted(first)
    m = ref64.margins(lg)
    small = min(float(m[b, :(f + 1 if f >= 0 else hc.T_LAT)].min()) for b, f in enumerate(first))
    print(f"\nE: first eos {sorted(first)}; smallest margin up to each row's eos {small:.3e}")
    assert small >= 2e-5
    plan = hc.compactions(first, d.max_len)
    print(f"E: compactions (positions decoded, rows before, after, live rows moved): {plan}")
    late = [c for c in plan if c[0] >= 257]
    assert late and all(moved > 0 for _, _, _, moved in late)
    # the rows such a compaction moves are decoded on behind it: a history moved wrongly shows in their later tokens
    t1 = late[-1][0]
    assert sum(f < 0 or f > t1 + 8 for f in first) >= late[-1][3] >= 8
    # restatement against a schedule worked out by hand: no row finishes -> no compaction; one row at position 2 of 4 rows -> the request
    # behind position 1 (read behind 5) does not see it yet, the next one behind position 5 is read behind position 9
    assert hc.compactions([-1] * 4, 40, rows=4) == []
    assert hc.compactions([-1, 2, -1, -1], 40, rows=4) == [(10, 4, 3, 2)]
