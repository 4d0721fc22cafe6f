"""Every case of tests/encoder_cases.py reaches the branch it is listed for, proven from the restated dispatch arithmetic (CU count 256):
an edit of a table cannot quietly stop a case testing what it claims.  The restated constants are read back from the headers."""
import os
import re

import pytest

import encoder_cases as ec

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "texocr_amd", "csrc")


def _ffn_in_walk(c, sb_mb=ec.PP_SB_MB):
    N, K = ec.row_gemms(ec.dims(c.dims))["ffn_in"]
    return ec.pp_walk(c.rows, N, K, sb_mb=sb_mb)


def _layer_pp(c, rows=None):
    """the encoder-layer GEMMs (the cross K/V projection apart) on the LDS-DMA kernel at the case's rows"""
    return [g for g in ec.pp_gemms(ec.dims(c.dims), c.rows if rows is None else rows) if g != "cross_kv"]


def _nbh(c):
    return len(c.slots) * ec.dims(c.dims).enc_heads


# what each listed reason means, as a predicate of the case
CLAIMS = {
    "exact key stage": lambda c: ec.attn_shape(c.n)[2] == 0 and ec.last_stage_key_tiles(c.n) == 4,
    "one past a key stage": lambda c: ec.attn_shape(c.n)[2] == ec.EA_KSTAGE - 1 and ec.attn_shape(c.n)[1] >= 2 and ec.last_stage_key_tiles(c.n) == 1,
    "one short of a query block": lambda c: c.n % ec.EA_QBLK == ec.EA_QBLK - 1 and ec.attn_shape(c.n)[2] == 1 and ec.idle_query_waves(c.n) == 0,
    "exact query block": lambda c: c.n % ec.EA_QBLK == 0 and ec.idle_query_waves(c.n) == 0,
    "one past a query block": lambda c: c.n % ec.EA_QBLK == 1 and ec.attn_shape(c.n)[0] >= 2,
    "idle query waves": lambda c: ec.idle_query_waves(c.n) == 3,
    "two query blocks": lambda c: ec.attn_shape(c.n)[0] == 2,
    "retired slots": lambda c: _nbh(c) % 8 != 0 and ec.attn_shape(c.n)[0] > 1 and ec.retired_blocks(ec.attn_shape(c.n)[0], _nbh(c)) > 0,
    "mostly gemm_big": lambda c: c.rows >= ec.PP_BM and len(_layer_pp(c)) == 1,
    "pp every gemm": lambda c: c.rows >= ec.PP_BM and len(ec.pp_gemms(ec.dims(c.dims), c.rows)) == 5,
    "one row in the last panel": lambda c: c.rows % ec.PP_BM == 1 and c.rows % ec.GB_BM == 1 and c.rows > ec.PP_BM,
    "short last panel": lambda c: c.rows % ec.PP_BM != 0,
    # B: the seam exists at this width (some GEMM takes the LDS-DMA kernel from 256 rows on, another never does)
    "below pp": lambda c: c.rows < ec.PP_BM and not ec.pp_gemms(ec.dims(c.dims), c.rows) and 0 < len(ec.pp_gemms(ec.dims(c.dims), ec.PP_BM)) < 5,
    "one short of pp": lambda c: c.rows in (ec.PP_BM - 2, ec.PP_BM - 1),
    "pp split": lambda c: c.rows >= ec.PP_BM and 0 < len(ec.pp_gemms(ec.dims(c.dims), c.rows)) < 5,
    "exact row panel": lambda c: c.rows % ec.PP_BM == 0,
    "two rows in the last panel": lambda c: c.rows % ec.PP_BM == 2 and c.rows > ec.PP_BM,
    "two tiles per workgroup": lambda c: ec.CUS < _ffn_in_walk(c).n_tiles <= 2 * ec.CUS and _ffn_in_walk(c).grid == ec.CUS,
    "narrower last band": lambda c: _ffn_in_walk(c).ct < _ffn_in_walk(c).tiles_n and _ffn_in_walk(c).tiles_n % _ffn_in_walk(c).ct != 0,
    "bands 6 6 4": lambda c: (_ffn_in_walk(c).tiles_m, _ffn_in_walk(c).tiles_n, _ffn_in_walk(c).n_tiles, _ffn_in_walk(c).bands) == (18, 16, 288, [6, 6, 4]),
    "one super-block": lambda c: not c.env and _ffn_in_walk(c).super_blocks == [18],
    "super-blocks 16 2": lambda c: _ffn_in_walk(c, int(dict(c.env)["TXO_PP_SB_MB"])).super_blocks == [16, 2],
}


@pytest.mark.parametrize("case", ec.ALL_CASES, ids=lambda c: c.id + ("-sb" if c.env else ""))
def test_case_reaches_every_branch_it_is_listed_for(case):
    d = ec.dims(case.dims)
    assert case.why, "a case has to say what it is for"
    for why in case.why:
        assert CLAIMS[why](case), (case.id, why)
    d.check_image(3, case.h, case.w)                               # fits the 256 x 2032 canvas
    assert d.n_tokens(case.h, case.w) == case.n <= ec.MAX_TOKENS
    assert d.enc_layers == 1 and d.canvas_hw == ec.CANVAS
    assert set(case.slots) == set(range(case.distinct))


def test_the_tables_hold_the_cases_the_suite_lacked():
    assert {n: ec.n_tokens(h, w) for n, (h, w, _) in ec.TOKEN_COUNTS.items()} == {n: n for n in (64, 65, 127, 128, 129, 193, 256, 257)}
    for dn in ec.A_DIMS:
        mine = [c for c in ec.A_CASES if c.dims == dn]
        assert sorted(c.n for c in mine if c.slots == ec.FIVE) == sorted(ec.TOKEN_COUNTS)
        assert [c.rows for c in mine if len(c.slots) == 1] == [257]
        # both copies of each image: at least two slots, at different offsets inside a 256-row panel and a 128-query block
        for c in mine:
            if len(c.slots) > 1 and c.n % ec.EA_QBLK:
                starts = [b * c.n for b, s in enumerate(c.slots) if s == 0]
                assert len({s % ec.PP_BM for s in starts}) == len(starts) == 3
    assert ec.dims("w192_h3").enc_heads == 3 and ec.dims("w256_h3").enc_heads == 5 and ec.dims("w512").embed_dim == 512
    for dn in ec.B_DIMS:
        assert sorted(c.rows for c in ec.B_CASES if c.dims == dn) == [128, 130, 254, 255, 256, 258]
        assert all(c.distinct == 4 for c in ec.B_CASES)
    # bf16 crosses M >= 256 from both sides at every B width
    for dn in ec.B_DIMS:
        assert not ec.pp_gemms(ec.dims(dn), 255) and ec.pp_gemms(ec.dims(dn), 256)
    assert ec.pp_gemms(ec.dims("w384_h6"), 256) == ["attn_out", "cross_kv", "ffn_in"]      # 2 * D = 768 fits; D = 384 and 3 * inner = 1152 do not
    assert ec.C_CASE.rows == ec.C_CASE_SB.rows == 4369 and ec.dims("w512").enc_exp == 4
    assert len({(c.id, c.env) for c in ec.ALL_CASES}) == len(ec.ALL_CASES)


def test_gemm_pp_fits_restated():
    assert ec.gemm_pp_fits(256, 256, 128)
    assert not ec.gemm_pp_fits(255, 256, 128) and not ec.gemm_pp_fits(256, 384, 128) and not ec.gemm_pp_fits(256, 256, 64)
    assert not ec.gemm_pp_fits(256, 256, 160) and not ec.gemm_pp_fits(2 ** 22, 256, 512) and ec.gemm_pp_fits(2 ** 22 - 1, 256, 512)


@pytest.mark.parametrize("sb_mb", [ec.PP_SB_MB, 4, 0])
@pytest.mark.parametrize("rev", [0, 1])
def test_restated_walk_visits_every_tile_once(sb_mb, rev):
    """the walk of case C (and of shapes the suite already pins) is a permutation of the output tiles: the restatement is a usable
    model of gemm_pp.h's tile_origin"""
    for M, N, K in [(4369, 4096, 512), (4369, 1536, 512), (257, 4096, 512), (8 * 589, 6144, 768), (4096, 2048, 256)]:
        wk = ec.pp_walk(M, N, K, sb_mb=sb_mb)
        tiles = ec.walk_tiles(wk, rev)
        assert sorted(tiles) == [(r, c) for r in range(wk.tiles_m) for c in range(wk.tiles_n)], (M, N, K)


def test_attention_grid_covers_every_block_once():
    for n in ec.TOKEN_COUNTS:
        nq = ec.attn_shape(n)[0]
        for nbh in (3, 5, 15, 25, 40):
            for rev in (0, 1):
                got = [b for b in (ec.ea_block(i, nq, nbh, rev) for i in range(ec.ea_grid(nq, nbh))) if b is not None]
                assert sorted(got) == [(bh, q) for bh in range(nbh) for q in range(nq)]
    assert [ec.attn_shape(n) for n in (64, 65, 127, 128, 129, 193, 256, 257)] == [
        (1, 1, 0), (1, 2, 63), (1, 2, 1), (1, 2, 0), (2, 3, 63), (2, 4, 63), (2, 4, 0), (3, 5, 63)]
    rows = ec.edge_rows(257)
    assert (list(rows["last row"]), rows["last query block"], rows["last key stage"], rows["interior"]) == (
        [256], range(256, 257), range(256, 257), range(0, 256))
    assert ec.edge_rows(193)["last query block"] == range(128, 193) and ec.edge_rows(193)["interior"] == range(0, 128)


def _const(header, name):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", text)
    assert m, (header, name)
    return int(m.group(1))


def test_restated_constants_are_the_headers():
    assert (ec.EA_QBLK, ec.EA_KSTAGE) == (_const("enc_attn.h", "EA_QBLK"), _const("enc_attn.h", "EA_KSTAGE"))
    assert (ec.PP_BM, ec.PP_BN, ec.PP_BK, ec.PP_SB_MB) == tuple(_const("gemm_pp.h", n) for n in ("PP_BM", "PP_BN", "PP_BK", "PP_SB_MB"))
    assert ec.GB_BM == _const("gemm_big.h", "GB_BM")
