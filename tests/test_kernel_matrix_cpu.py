"""CPU checks of tests/kernel_matrix.py: the tuning table covers every tuning key, the generated codes have exactly
the requested degrees, and the oracle treats empty columns and single-edge rows as the reference's kernels do."""
import os
import re

import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import capi, channel
import kernel_matrix as km

HERE = os.path.dirname(os.path.abspath(__file__))


def _test_functions(module):
    with open(os.path.join(HERE, module + ".py")) as f:
        return set(re.findall(r"^def (test_\w+)\(", f.read(), re.M))


def test_every_tuning_key_has_a_case():
    keys = km.all_tune_keys()
    assert set(km.TUNE_CASES) == keys, sorted(keys ^ set(km.TUNE_CASES))
    for key, case in km.TUNE_CASES.items():
        module, name = case["test"].split("::")
        assert name in _test_functions(module), (key, case["test"])
        if case["tune"] is None:
            # covered by an existing test of another module: it must name the key in its tuning
            assert module != "test_gpu_kernel_matrix", key
            with open(os.path.join(HERE, module + ".py")) as f:
                assert '"%s"' % key in f.read(), (key, module)
            continue
        assert key in case["tune"], key
        cfg = capi.DecoderConfig()
        capi.apply_tune(cfg, case["tune"])          # a valid tuning dict
    # the streaming plans set the keys their table entries promise
    plan_keys = set().union(*(set(t) for t in km.FLOOD_PLANS.values()))
    for key in ("merge", "check_wide", "rows_per_wave", "cols_per_wave", "q_order", "syn_xcd", "tiles_first"):
        assert key in plan_keys, key


def _assert_code(rows, cols, M, N, row_degs, col_degs):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    key = rows * N + cols
    assert np.all(np.diff(key) > 0)                  # strictly ascending row-major: no duplicate edge
    assert rows.min() >= 0 and rows.max() < M and cols.min() >= 0 and cols.max() < N
    rd, cd = km.degree_maps(rows, cols, M, N)
    assert rd == {d: n for d, n in row_degs.items() if n}
    assert cd == {d: n for d, n in col_degs.items() if n}
    g = L.Graph(rows, cols, M, N)
    info = g.info()
    assert (info["M"], info["N"], info["E"]) == (M, N, rows.size)
    assert info["max_row_deg"] == max(row_degs) and info["max_col_deg"] == max(col_degs)
    g.close()


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_irregular_code_has_the_requested_degrees(seed):
    # the degree mix of the issue's prototype: M = 136, N = 408, E = 1485
    row_degs = {0: 4, 1: 8, 2: 12, 3: 16, 8: 16, 9: 16, 16: 16, 17: 16, 24: 10, 25: 8, 32: 6, 33: 4, 40: 4}
    E = sum(d * n for d, n in row_degs.items())
    col_degs = {0: 8, 1: 20, 2: 60, 4: 40, 5: 30, 8: 20, 9: 20, 16: 10, 17: 4, 20: 4}
    col_degs[3] = (E - sum(d * n for d, n in col_degs.items())) // 3
    col_degs[1] += E - sum(d * n for d, n in col_degs.items())
    rows, cols, M, N = km.irregular_code(row_degs, col_degs, seed)
    assert (M, N) == (sum(row_degs.values()), sum(col_degs.values()))
    _assert_code(rows, cols, M, N, row_degs, col_degs)
    again = km.irregular_code(row_degs, col_degs, seed)             # seeded: the same graph
    assert np.array_equal(again[0], rows) and np.array_equal(again[1], cols)
    with pytest.raises(ValueError):
        km.irregular_code({2: 1}, {1: 3}, seed)                     # edge sums differ
    with pytest.raises(ValueError):
        km.irregular_code({3: 2}, {2: 1, 4: 1}, seed)               # a degree-4 column in two rows


def test_matrix_and_ira_codes():
    rows, cols, M, N = km.matrix_code()
    rd, cd = km.degree_maps(rows, cols, M, N)
    assert rd == km.MATRIX_ROW_DEGS
    assert all(cd[d] >= n for d, n in km.MATRIX_COL_FIXED.items())
    assert set(cd) == set(km.MATRIX_COL_FIXED) | {3}
    _assert_code(rows, cols, M, N, rd, cd)
    # no row shares a degree-2 column with the next row of its class: nothing for column-local fusion
    assert not any(km.linkable_rows(rows, cols, M, N).values())
    for d in (3, 9, 16):
        rows, cols, M, N, K = km.ira_code(d, 40, {5: 3, 20: 2}, seed=d)
        rd = np.bincount(rows, minlength=M)
        assert (rd[:40] == d).all() and sorted(rd[40:]) == [5, 5, 5, 20, 20]
        cd = np.bincount(cols, minlength=N)
        assert (cd[K:-1] == 2).all() and cd[-1] == 1 and (cd[:K] >= 3).all()
        assert km.linkable_rows(rows, cols, M, N)[d] == 39            # the whole staircase
        _assert_code(rows, cols, M, N, *km.degree_maps(rows, cols, M, N))


def test_oracle_on_empty_columns_and_single_edge_rows():
    """A degree-1 row sends +1000 to its only edge (min-sum: the minimum over no other edge keeps its start value);
    a degree-0 column's hard bit comes from its channel value alone: 0 if y > 0, else 1."""
    row_degs = {0: 2, 1: 3, 3: 6, 4: 4}
    col_degs = {0: 3, 1: 5, 2: 10, 3: 4}
    rows, cols, M, N = km.irregular_code(row_degs, col_degs, 3)
    og = oracle.Graph(rows, cols, M, N, 8)
    rd = np.bincount(rows, minlength=M)
    cd = np.bincount(cols, minlength=N)
    one = np.nonzero(rd[rows] == 1)[0]                # edges of the degree-1 rows
    empty = np.nonzero(cd == 0)[0]
    assert one.size == 3 and empty.size == 3
    y = channel.awgn_frames(N, 0, 6, 0.9, seed=11)
    y[:, empty] = np.array([[0.5, -0.5, 0.0], [-2.0, 3.0, -0.0], [1e-30, -1e-30, 7.0],
                            [0.0, 0.0, 0.0], [-1.0, -1.0, 1.0], [2.0, 2.0, -2.0]], np.float32)
    y[:3, cols[one]] *= -1.0                          # single-edge rows on negative values too
    o = oracle.decode(og, y, "ms", max_iter=5, tap_iter=1)
    assert (o["taps"]["r"][:, one] == 1000.0).all()
    assert np.array_equal(o["hard"][:, empty], np.where(y[:, empty] > 0, 0, 1).astype(np.uint8))
    assert np.array_equal(o["taps"]["post"][:, empty], y[:, empty])
