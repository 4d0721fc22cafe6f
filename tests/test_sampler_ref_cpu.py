"""The host sampler reference (tests/sampler_ref.py) on its own, no GPU: Philox4x32-10 known-answer vectors, the float32 u, the kept
set's tie rule and k, and agreement with the oracle's statement of the reference sampler (oracle/cpu_ref.py: sample_probs)."""
import numpy as np
import pytest
import torch

import sampler_ref as sr
from oracle import cpu_ref


# Random123's known-answer vectors for philox4x32_10: (counter; key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(v) for v in sr.philox4x32_10(ctr, key)) == out


def test_philox_vectorised_equals_one_by_one():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, (37, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, (37, 2), dtype=np.uint64).astype(np.uint32)
    many = sr.philox4x32_10(ctr, key)
    for i in range(37):
        assert np.array_equal(many[i], sr.philox4x32_10(ctr[i], key[i]))


def test_u_is_the_float32_expression():
    # (c0 >> 8) + 0.5f: exact below 2^23, round-to-nearest-even above
    c0 = np.array([0, 0xFF, 0x100, (2 ** 23 - 1) << 8, (2 ** 23) << 8, (2 ** 23 + 1) << 8, (2 ** 24 - 2) << 8, 0xFFFFFFFF], np.uint64)
    u = sr.u_from_c0(c0.astype(np.uint32))
    assert u.dtype == np.float32
    want = np.array([0.5, 0.5, 1.5, 2 ** 23 - 0.5, 2 ** 23, 2 ** 23 + 2, 2 ** 24 - 2, 2 ** 24]) / 2 ** 24
    assert np.array_equal(u.astype(np.float64), want)
    assert float(u[0]) > 0 and float(u[-1]) == 1.0                 # u lies in (0, 1]


def test_uniform_keys():
    # key = (seed lo, seed hi), counter = (row, t, 0, 0)
    seed = 2 ** 32 + 5
    c0 = sr.philox4x32_10((3, 11, 0, 0), (5, 1))[0]
    assert sr.uniform(seed, 3, 11) == sr.u_from_c0(c0)
    assert sr.uniform(seed, 3, 11) != sr.uniform(5, 3, 11)             # the high key half counts
    assert sr.uniform(7, 3, 11) != sr.uniform(7, 11, 3)                # row and position are not interchangeable
    top = sr.philox4x32_10((1, 2, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert sr.uniform(2 ** 64 - 1, 1, 2) == sr.u_from_c0(top)
    grid = sr.uniform(9, np.arange(4)[:, None], np.arange(6)[None, :])
    assert grid.shape == (4, 6) and grid[2, 5] == sr.uniform(9, 2, 5)


def test_k_matches_the_model_and_the_oracle():
    assert sr.topk_of(1000) == 99 and sr.topk_of(1100) == 109 and sr.topk_of(16) == 1 and sr.topk_of(10) == 1
    for V in (12, 100, 999, 1000, 1024, 8192):
        assert sr.topk_of(V) == int((1 - 0.9) * V)


@pytest.mark.parametrize("V,temp", [(1000, 0.3), (1000, 1.0), (1100, 5.0), (999, 0.7)])
def test_kept_probabilities_equal_the_oracle_sample_probs(V, temp):
    rng = np.random.default_rng(V)
    lg = (rng.standard_normal((16, V)) * 2).astype(np.float32)
    assert all(len(np.unique(r)) == V for r in lg)                                    # no ties
    mine = sr.kept_probs(lg, temp, sr.topk_of(V))
    ref = cpu_ref.sample_probs(torch.from_numpy(lg).double(), temp).numpy()
    assert np.abs(mine - ref).max() < 1e-12
    # and the draw follows that distribution's inverse CDF
    d = sr.draw(lg, temp, 3, np.arange(16), 4)
    assert bool(mine[np.arange(16), d.token].min() > 0)


def test_ties_straddling_the_kth_value_keep_the_lowest_indices():
    # k = int(0.1 * 30) = 2 at V = 30 (float rounding: 20 gives 1); one value above, four tied at the k-th value (indices 3, 7, 11, 15)
    V = 30
    x = np.full((1, V), -5.0, np.float32)
    x[0, 9] = 2.0
    x[0, [3, 7, 11, 15]] = 1.0
    assert sr.topk_of(V) == 2
    kept = sr.kept_mask(x, 2)[0]
    assert set(np.nonzero(kept)[0]) == {3, 9}
    # k = 4: three of the four ties
    assert set(np.nonzero(sr.kept_mask(x, 4)[0])[0]) == {3, 7, 9, 11}
    # draws only ever return kept entries, and the tie kept is the lowest index
    p = sr.kept_probs(x, 1.0, 2)[0]
    assert p[3] > 0 and p[7] == 0 and abs(p[3] - 1 / (1 + np.e)) < 1e-15
    toks = {int(sr.draw_u(x, 1.0, u, 2).token[0]) for u in np.linspace(0.01, 1.0, 50)}
    assert toks == {3, 9}


def test_ties_use_the_kernels_key_order():
    # +0.0 and -0.0 compare equal as floats, but the kernel's order-preserving key puts -0.0 below +0.0
    x = np.array([[-0.0, 0.0, -1.0, -2.0]], np.float32)
    assert set(np.nonzero(sr.kept_mask(x, 1)[0])[0]) == {1}


@pytest.mark.parametrize("V", [10, 16])
def test_k_clamps_to_one_and_the_draw_is_the_arg_max(V):
    rng = np.random.default_rng(V)
    lg = rng.standard_normal((64, V)).astype(np.float32)
    d = sr.draw(lg, 1.0, 7, np.arange(64), 0)
    assert np.array_equal(d.token, lg.argmax(1)) and bool(np.isinf(d.dist).all())


def test_tiny_temperature_gives_the_arg_max():
    rng = np.random.default_rng(1)
    lg = rng.standard_normal((200, 1000)).astype(np.float32)
    d = sr.draw(lg, 1e-4, 11, np.arange(200), 3)
    assert np.array_equal(d.token, lg.argmax(1))


def test_u_at_its_extremes():
    rng = np.random.default_rng(2)
    lg = rng.standard_normal((8, 1000)).astype(np.float32)
    kept = sr.kept_mask(lg, 99)
    first = np.argmax(kept, 1)
    last = 999 - np.argmax(kept[:, ::-1], 1)
    lo = sr.draw_u(lg, 1.0, sr.u_from_c0(np.zeros(8, np.uint32)))
    hi = sr.draw_u(lg, 1.0, sr.u_from_c0(np.full(8, 0xFFFFFFFF, np.uint32)))
    assert np.array_equal(lo.token, first) and np.array_equal(hi.token, last)
    # u = 1 puts u * total at the end of the CDF: the nearest boundary is the one in front of the last kept entry
    assert bool((hi.dist > 0).all()) and np.array_equal(hi.pair[:, 1], last)


def test_boundary_distance_and_pair():
    x = np.log(np.array([[1.0, 1.0, 2.0]], np.float32))            # masses 1, 1, 2 of 4 at temp 1, k = 3
    for u, tok, dist, pair in [(0.2, 0, 0.05, (0, 1)),(0.3, 1, 0.05, (0, 1)), (0.45, 1, 0.05, (1, 2)), (0.9, 2, 0.4, (1, 2))]:
        d = sr.draw_u(x, 1.0, np.float32(u), 3)
        assert int(d.token[0]) == tok and abs(float(d.dist[0]) - dist) < 1e-6 and tuple(d.pair[0]) == pair, (u, d)


def test_keys_for_each_decode_path():
    assert sr.keys_for("engine", 1, 8, 0, 5) == (5, 0)
    assert sr.keys_for("engine", 1, 8, 20, 5) == (5, 20)            # generate_window beyond the table: the token index
    assert sr.keys_for("stepwise", 3, 8, 0, 5) == (5, 2)            # the last start token's position
    assert sr.keys_for("stepwise", 3, 8, 5, 5) == (5, 7)            # the output fills the table
    assert sr.keys_for("stepwise", 3, 8, 6, 5) == (11, 7)           # the window slides: seed + i at the last position
    assert sr.keys_for("stepwise", 1, 8, 9, 2 ** 64 - 3) == (6, 7)  # modulo 2^64
    with pytest.raises(ValueError):
        sr.keys_for("beam", 1, 8, 0, 0)
