"""Alternatives per token without a GPU: the reference rule on ties, the scripted rows' own expectations, the wrapper's pairing of ids to
pieces, and the header / binding lists (tests/test_abi_cpu.py's own checks see the new entries; they pass unchanged)."""
import os
import re

import numpy as np
import pytest

import alts_ref
from texocr_amd import _lib, ops
from texocr_amd.tokenizer import RegExTokenizer
from texocr_amd.wrapper import pair_alts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_equal_entries_come_in_ascending_index():
    x = np.array([1.0, 3.0, 3.0, -2.0, 3.0, 0.5], np.float32)
    ids, logp = alts_ref.alts(x, 5)
    assert ids.tolist() == [1, 2, 4, 0, 5]
    assert logp[0] == logp[1] == logp[2] and np.all(np.diff(logp) <= 0)
    assert abs(np.exp(alts_ref.alts(x, 6)[1]).sum() - 1.0) < 1e-12
    ids, logp = alts_ref.alts(np.full((2, 9), 1.25, np.float32), 8)
    assert ids.tolist() == [list(range(8))] * 2 and np.allclose(logp, -np.log(9.0))


def test_first_alternative_is_argmax():
    x = np.random.default_rng(0).standard_normal((7, 65)).astype(np.float32)
    x[3, 10] = x[3, 50] = x[3].max() + 1
    assert alts_ref.alts(x, 1)[0][:, 0].tolist() == np.argmax(x, axis=-1).tolist()


@pytest.mark.parametrize("V", [63, 65, 1024, 1028, 2052, 64, 129, 1027])
def test_scripts_expect_their_raised_entries_first(V):
    """every script's expected order is unambiguous: the raised entries in the stated order lead the stable sort, and each lane layout
    is what the script says (one lane / eight lanes)"""
    names = set()
    for name, row, idx in alts_ref.scripts(V):
        names.add(name)
        assert row.dtype == np.float32 and row.shape == (V,)
        ids, _ = alts_ref.alts(row, min(8, V))
        n = min(len(idx), 8)
        assert ids[:n].tolist() == idx[:n], (V, name)
    assert {"one_lane", "eight_lanes", "three_equal", "equal", f"seam{V - 1}"} <= names
    lanes = [{lane for lane in range(64) if i in alts_ref.lane_entries(V, lane)} for i in range(V)]
    assert all(len(s) == 1 for s in lanes)                                       # every entry is streamed by exactly one lane
    one = dict((n, i) for n, _, i in alts_ref.scripts(V))
    assert len({next(iter(lanes[i])) for i in one["one_lane"]}) == 1
    assert [next(iter(lanes[i])) for i in one["eight_lanes"]] == [ln for ln in range(63, 55, -1) if alts_ref.lane_entries(V, ln)]   # (V = 63: lane 63 is empty)
    a, b, c = one["three_equal"][:3]
    assert len({next(iter(lanes[i])) for i in (a, b, c)}) == (2 if V != 63 else 3)       # two of the three in one lane (V = 63: a lane holds one entry)


def test_wrapper_pairs_ids_with_pieces():
    tok = RegExTokenizer.from_tables(260, {"<PAD>": 256, "<BOS>": 257, "<EOS>": 258}, [(92, 97, 259)])
    ids = [[259, 97, 258], [98, 256, 257], [99, 99, 99]]
    logp = [[-0.1, -2.5, -3.0], [-0.5, -1.0, -4.0], [0.0, 0.0, 0.0]]
    got = pair_alts(tok, ids, logp, 2)                                           # cut where the tokens are cut
    assert got == [[("\\a", -0.1), ("a", -2.5), ("<EOS>", -3.0)], [("b", -0.5), ("<PAD>", -1.0), ("<BOS>", -4.0)]]


def test_header_binding_and_query_code():
    header = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name in ("txo_set_alternatives", "txo_last_alternatives", "txo_decode_score_alts", "txo_score_alts"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in _lib.SYMBOLS
    assert int(re.search(r"#define\s+TXO_Q_LAST_ALTS\s+(\d+)", header).group(1)) == _lib.Q_LAST_ALTS == 10
    assert ops.ALTS_MAX == 8


@pytest.mark.parametrize("k", [0, 9, -1, True, 2.0])
def test_check_alts_refuses(k):
    with pytest.raises(ValueError, match="alternatives"):
        ops.check_alts(k, 100)


def test_check_alts_names_the_vocabulary():
    with pytest.raises(ValueError, match="alternatives.*vocabulary"):
        ops.check_alts(8, 5)
    assert ops.check_alts(8, 8) == 8


def test_score_case_leaves_out_at_most_one_percent_on_the_oracle():
    """tests/test_gpu_alts.py::test_score_random_weights compares ranks only where the float64 gap to both neighbours exceeds the margin: on
    the oracle's own logits of that case the places left out stay inside its 1 % cap"""
    import dataclasses
    import torch
    from oracle import cpu_ref
    from texocr_amd import synth
    from gpu_harness import SHAPE_CASES
    c = alts_ref.SCORE_CASE
    V = c["vocab"]
    d = dataclasses.replace(SHAPE_CASES["calib256"][0], vocab=V, bos=V - 2, eos=V - 3, pad=V - 1)     # test_gpu_sampler._dims
    sd = cpu_ref.to_torch_sd(synth.synth_state_dict(d, c["weight_seed"]))
    img = torch.from_numpy(synth.synth_images(c["rows"], 3, *c["image_hw"], seed=c["image_seed"]))
    trg = alts_ref.score_targets(d.bos, V)
    lg = cpu_ref.teacher_forced_logits_cached(sd, cpu_ref.encode(sd, img), trg[:, :-1]).double().numpy()
    assert lg.shape == (c["rows"], c["L"] - 1, V)
    _, keep = alts_ref.ranked_places(lg, 8)
    left = int((~keep).sum())
    print(f"\noracle: {left} of {keep.size} (row, rank) places inside the {alts_ref.MARGIN:.0e} margin")
    assert left <= 0.01 * keep.size
