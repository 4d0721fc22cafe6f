"""Every case of tests/decode_cases.py reaches the branch it is listed for, proven from the restated dispatch arithmetic: an edit of a
table cannot quietly stop a case testing what it claims.  The restated constants are read back from the headers.  On the float64 oracle
alone: every distinct image's greedy decode over the positions the GPU tests compare, and its smallest top-1 / top-2 margin -- the fp32
cases decide every token by at least 2e-5, so the fp32 engine has to give the oracle's tokens at every position."""
import os
import re

import pytest

import decode_cases as dc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "texocr_amd", "csrc")

COUNT = {"one": 1, "two": 2, "three": 3, "four": 4, "five": 5}


def _lat(c):
    return dc.lat_shape(c.n, dc.DIMS[c.dims].embed_dim, c.dtype)


def _passes(k):
    return lambda c: dc.passes(c.n, c.dtype)[0] == k


def _rounds(k):
    return lambda c: _lat(c).nt_w == k and _lat(c).ntiles > (k - 1) * _lat(c).nw


# what each listed reason means, as a predicate of the case
CLAIMS = {
    "one pass": _passes(1), "two passes": _passes(2), "three passes": _passes(3),
    "last pass one key": lambda c: dc.passes(c.n, c.dtype)[1] == 1 and dc.passes(c.n, c.dtype)[0] > 1,
    "last pass full": lambda c: dc.passes(c.n, c.dtype)[1] == dc.keys_per_pass(c.dtype),
    "last pass one short": lambda c: dc.passes(c.n, c.dtype)[1] == dc.keys_per_pass(c.dtype) - 1,
    "one round": _rounds(1), "two rounds": _rounds(2), "three rounds": _rounds(3), "four rounds": _rounds(4), "five rounds": _rounds(5),
    "idle waves": lambda c: _lat(c).idle == _lat(c).nw - 1,          # ONE wave starts the round
    "no idle wave": lambda c: _lat(c).idle == 0,
    "last tile one key": lambda c: _lat(c).last_tile_keys == 1,
    "last tile full": lambda c: _lat(c).last_tile_keys == 16,
    "last tile one short": lambda c: _lat(c).last_tile_keys == 15,
    "row seam": lambda c: dc.expected_path(dc.DIMS[c.dims], c.dtype, c.rows) == (c.expect[0], list(c.expect[1])),
}


@pytest.mark.parametrize("case", dc.ALL_CASES, ids=lambda c: c.id)
def test_case_reaches_every_branch_it_is_listed_for(case):
    d = dc.DIMS[case.dims]
    assert case.why, "a case has to say what it is for"
    for why in case.why:
        assert CLAIMS[why](case), (case.id, why)
    d.check_image(3, case.h, case.w)
    assert d.n_tokens(case.h, case.w) == case.n and d.enc_layers == 1 and d.dec_layers == 2
    assert set(case.slots) == set(range(case.distinct)) and 3 <= case.distinct <= 4
    assert all(case.slots.count(s) >= 2 for s in range(case.distinct))          # every image at several slots
    # the path the GPU test asserts through Q_LAST_PERSISTENT / Q_LAST_ROW_RANGES / Q_LAST_LATENT
    path, sizes = dc.expected_path(d, case.dtype, case.rows, case.persist, case.latent)
    if case.group == "A":
        assert d.canvas_hw == dc.CANVAS and (case.latent, case.persist) == (0, 0) and path == (0, 1, 0)
    elif case.group == "C":
        assert d.canvas_hw == dc.CANVAS and case.latent == 1 and path == (0, 1, 1) and dc.latent_ok(d.embed_dim, case.dtype)
    else:
        assert (case.latent, case.persist) == (None, None) and (path, tuple(sizes)) == case.expect and case.n == 65


def test_the_tables_hold_the_cases_the_suite_lacked():
    assert {n: dc.n_tokens(*hw) for n, hw in dc.SIZE_OF.items()} == {n: n for n in dc.SIZE_OF}
    assert all(h <= dc.CANVAS[0] and w <= dc.CANVAS[1] and h % 16 == 0 and w % 16 == 0 for h, w in dc.SIZE_OF.values())
    assert (dc.keys_per_pass("fp32"), dc.keys_per_pass("bf16")) == (160, 320)
    # A: the pass boundary from both sides and on it, one, two and three passes, at 2 and 3 decoder heads
    for dn, heads in (("w64_h2", 2), ("w64_h3", 3)):
        assert dc.DIMS[dn].dec_heads == heads and dc.DIMS[dn].embed_dim == 64
        for t, ns in (("fp32", [159, 160, 161, 320, 321]), ("bf16", [319, 320, 321, 640, 641])):
            mine = [c for c in dc.A_CASES if c.dims == dn and c.dtype == t]
            assert sorted(c.n for c in mine) == ns
            assert [dc.passes(n, t) for n in ns] == [(1, dc.keys_per_pass(t) - 1), (1, dc.keys_per_pass(t)), (2, 1), (2, dc.keys_per_pass(t)), (3, 1)]
    # B: at least 17 slots; the rows of the first 16-row tile take 1, 1, 2 and 3 passes, the smallest image is two keys
    assert len(dc.B_SLOTS) >= 17 and set(dc.B_SLOTS[:16]) == set(dc.B_SLOTS[16:]) == {0, 1, 2, 3}
    for t, ns in dc.B_NS.items():
        assert [dc.passes(n, t)[0] for n in ns] == [1, 1, 2, 3] and ns[0] == 2
        lens = [ns[s] for s in dc.B_SLOTS]
        assert [dc.ragged_len(lens, r, max(ns)) for r in range(len(lens))] == lens
        assert dc.passes(ns[1], t)[1] == dc.keys_per_pass(t) and dc.passes(ns[2], t)[1] == 1 and dc.passes(ns[3], t)[1] == 1
    # C: 16 * NW keys, one more, and the later round boundaries, on the 8-wave and on the 4-wave tile, for all three request depths
    assert [dc.lat_waves(w, t) for w, t in ((64, "fp32"), (64, "bf16"), (256, "fp32"), (256, "bf16"), (768, "bf16"))] == [8, 8, 8, 4, 4]
    seen = {}
    for c in dc.C_CASES:
        s = dc.lat_shape(c.n, dc.DIMS[c.dims].embed_dim, c.dtype)
        seen.setdefault((c.dims, c.dtype), set()).add((s.nt_w, s.idle > 0))
        assert c.n in (16 * s.nw * s.nt_w - 1, 16 * s.nw * s.nt_w, 16 * s.nw * (s.nt_w - 1) + 1), c.id
    for key, got in seen.items():
        assert {(1, False), (2, True)} <= got and any(r >= 3 and idle for r, idle in got), (key, got)
    assert {(dn, t): dc.lat_shape(128, dc.DIMS[dn].embed_dim, t).nf for dn, t in seen} == {
        ("w64_h2", "fp32"): 2, ("w64_h2", "bf16"): 2, ("w256_h8", "fp32"): 0, ("w256_h8", "bf16"): 2, ("w768_h12", "bf16"): 1}
    assert not dc.latent_ok(768, "fp32") and not dc.latent_ok(128, "bf16")
    # D: both sides of every seam
    rows = lambda dn, t: sorted(c.rows for c in dc.D_CASES if (c.dims, c.dtype) == (dn, t))
    assert rows("calib256", "bf16") == [128, 129, 223, 224, 225] and rows("calib256", "fp32") == [256, 257]
    assert rows("calib768", "bf16") == [127, 128, 255, 256]
    assert len({c.id for c in dc.ALL_CASES}) == len(dc.ALL_CASES)


def test_row_seams_restated():
    c256, c768 = dc.DIMS["calib256"], dc.DIMS["calib768"]
    assert (c256.embed_dim, c256.dec_heads, c256.dec_exp, c768.embed_dim, c768.dec_heads, c768.dec_exp) == (256, 8, 4, 768, 12, 4)
    assert dc.split(224, 2) == [(0, 112), (112, 112)] and dc.split(225, 2) == [(0, 128), (128, 97)] and dc.split(20, 2) == [(0, 16), (16, 4)]
    assert dc.split(257, 1) == [(0, 257)] and dc.split(8, 2) == [(0, 8)]
    # the persistent launch: bf16 up to 128 rows, fp32 up to 256; the 768-wide one is opt-in; TXO_LATENT=1 takes it away
    assert [dc.persist_usable(c256, "bf16", r) for r in (128, 129)] == [True, False]
    assert [dc.persist_usable(c256, "fp32", r) for r in (256, 257)] == [True, False]
    assert not dc.persist_usable(c768, "bf16", 64) and dc.persist_usable(c768, "bf16", 64, persist=1)
    assert not dc.persist_usable(c256, "bf16", 64, latent=1) and not dc.persist_usable(dc.DIMS["w64_h2"], "fp32", 9, persist=1)
    # every image of a D case has copies in every range: the bit-identity of an image's copies crosses the range boundary
    for c in dc.D_CASES:
        first = 0
        for nb in c.expect[1]:
            assert set(c.slots[first:first + nb]) == set(range(c.distinct)), c.id
            first += nb
        assert first == c.rows
    # the folded latent out-projection takes 32 x 16 blocks from 129 rows of ONE range on; the wide decoder 64-row blocks from 128 rows
    blocks = lambda dn, t, rows: [dc.out_proj_block(dc.DIMS[dn], t, nb, bool(dc.expected_path(dc.DIMS[dn], t, rows)[0][2]))
                                  for nb in dc.expected_path(dc.DIMS[dn], t, rows)[1]]
    assert [blocks("calib256", "bf16", r) for r in (129, 223, 224, 225)] == [[(32, 16)], [(32, 16)], [(16, 32)] * 2, [(16, 32)] * 2]
    assert [blocks("calib768", "bf16", r) for r in (127, 128, 255, 256)] == [[(16, 32)], [(64, 32)], [(64, 32)], [(64, 32)] * 2]
    assert blocks("calib256", "fp32", 257) == [(16, 32)]


def _const(header, pattern):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(pattern, text)
    assert m, (header, pattern)
    return int(m.group(1))


def test_restated_constants_are_the_headers():
    assert dc.DA_NL_CROSS == _const("dec_attn.h", r"#define TXO_NL_CROSS (\d+)")
    assert dc.DH == _const("common.h", r"constexpr int DH = (\d+)")
    assert dc.PERSIST_MAX_BF16_GREEDY == _const("engine.hip", r"PERSIST_MAX_BF16_GREEDY = (\d+)")
    assert dc.WIDE_MID_ROWS == _const("engine.hip", r"wide_mid_rows = (\d+)")
    assert _const("engine.hip", r"wide_min_rows = (\d+)") > 65535
    assert dc.PS_MAXLD == _const("persist.h", r"PS_MAXLD = (\d+)") and dc.DG_BM == _const("dec_gemm.h", r"DG_BM = (\d+)")
    text = open(os.path.join(CSRC, "common.h")).read()
    assert [int(x) for x in re.findall(r"PER16 = (\d+)", text)] == [dc.PER16["fp32"], dc.PER16["bf16"]]
    assert [int(x) for x in re.findall(r"KCHUNK = (\d+)", text)] == [dc.KCHUNK["fp32"], dc.KCHUNK["bf16"]]
    lat = open(os.path.join(CSRC, "lat_attn.h")).read()
    assert "return D_ <= 256 ? 8 : 4;" in lat and "nt_w = (ntiles + NW - 1) / NW" in lat and "KC <= 8 ? 2 : (NW == 4 ? 1 : 0)" in lat
    assert "static constexpr bool lat_nw4 = sizeof(T) == 2;" in open(os.path.join(CSRC, "engine.hip")).read()


def _distinct_references():
    keys = {(c.dims, c.h, c.w, c.distinct, c.dtype) for c in dc.ALL_CASES}
    keys |= {(dc.B_DIMS, *dc.SIZE_OF[n], 1, t) for t, ns in dc.B_NS.items() for n in ns}
    merged = {}
    for dn, h, w, k, t in keys:
        merged.setdefault((dn, h, w, k), set()).add(t)
    return sorted((k, tuple(sorted(v))) for k, v in merged.items())


@pytest.mark.parametrize("key,dtypes", _distinct_references(), ids=lambda v: "-".join(map(str, v)) if isinstance(v[0], str) else None)
def test_oracle_margins(key, dtypes):
    """the float64 greedy decode of every distinct image over the positions compared; fp32 cases: every token decided by >= 2e-5"""
    ref = dc.reference(*key)
    assert ref.toks.shape == (key[3], dc.STEPS) and ref.logits.shape[:2] == (key[3], dc.STEPS)
    print(f"\n{key}: smallest top-1 / top-2 margin {ref.margin:.3e} ({', '.join(dtypes)})")
    if "fp32" in dtypes:
        assert ref.margin >= 2e-5, (key, ref.margin)
