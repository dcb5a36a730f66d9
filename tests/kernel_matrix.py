"""Codes and tuning cases for tests/test_gpu_kernel_matrix.py (helpers, not a test module).

The wimax, DVB-S2-profile and BG1-profile codes of the other tests have few degree mixes.  The codes made here
put rows and columns of every degree class the streaming flooding kernels distinguish on one graph, so that every
unrolled body, bucket launch and generic kernel runs against the oracle.

Who runs the matrix code: sp, ms and ms16 in tests/test_gpu_kernel_matrix.py, bp and bp16 in tests/test_gpu_bp.py
(bp_cases.matrix()); the corrected and one-byte arithmetics -- msc, msc16, ms8, msc8, msi4/5/6/8, msci4/5/6/8 -- in
tests/test_gpu_flood_matrix.py (flood_matrix_cases.py), which also holds the matrix code without its rows above degree 32,
the one on which round 1 reads the channel array."""
import numpy as np

from myldpccppapi_amd import capi, channel, codes


def irregular_code(row_degs, col_degs, seed):
    """A simple bipartite graph with exactly the given degree multisets ({degree: count} maps, equal edge sums).

    Seeded Gale-Ryser greedy: rows in descending degree each take the columns with the most sockets left, ties
    broken at random.  Rows and columns get their degrees in a seeded random order, so that the classes
    interleave.  Returns (rows, cols, M, N): the edges in strictly ascending row-major order."""
    rng = np.random.default_rng(seed)
    rdeg = np.repeat(np.array(sorted(row_degs), np.int64), [row_degs[d] for d in sorted(row_degs)])
    cdeg = np.repeat(np.array(sorted(col_degs), np.int64), [col_degs[d] for d in sorted(col_degs)])
    if rdeg.sum() != cdeg.sum():
        raise ValueError("row and column degree sums differ: %d != %d" % (rdeg.sum(), cdeg.sum()))
    rdeg, cdeg = rng.permutation(rdeg), rng.permutation(cdeg)
    M, N = rdeg.size, cdeg.size
    left = cdeg.copy()
    rows, cols = [], []
    for m in sorted(range(M), key=lambda m: (-rdeg[m], m)):
        d = int(rdeg[m])
        if d == 0:
            continue
        order = np.lexsort((rng.random(N), -left))        # most sockets left first, random among equals
        pick = order[:d]
        if d > N or left[pick].min() <= 0:
            raise ValueError("degree sequences are not bigraphic")
        left[pick] -= 1
        rows.append(np.full(d, m, np.int64))
        cols.append(pick)
    assert not left.any()
    r, c = codes.row_major(np.concatenate(rows), np.concatenate(cols))
    return r, c, M, N


def degree_maps(rows, cols, M, N):
    """({row degree: count}, {column degree: count}) of an edge list."""
    rd = np.bincount(rows, minlength=M)
    cd = np.bincount(cols, minlength=N)
    return ({int(d): int(n) for d, n in zip(*np.unique(rd, return_counts=True))},
            {int(d): int(n) for d, n in zip(*np.unique(cd, return_counts=True))})


def linkable_rows(rows, cols, M, N):
    """Per row degree: how many rows share a degree-2 column with the next row of the same degree, the
    column's first edge in the first row (what build_classes in engine_flood.hip may fuse into the check kernel)."""
    rows, cols = np.asarray(rows), np.asarray(cols)
    rd = np.bincount(rows, minlength=M)
    cd = np.bincount(cols, minlength=N)
    by_row = [set() for _ in range(M)]
    for r, c in zip(rows, cols):
        if cd[c] == 2:
            by_row[r].add(int(c))
    out = {}
    for d in range(2, int(rd.max()) + 1):
        ids = np.nonzero(rd == d)[0]
        out[d] = sum(1 for a, b in zip(ids[:-1], ids[1:]) if by_row[a] & by_row[b])
    return out


# Row degrees of the matrix code: every degree of the unrolled check bodies (1 ... 32), the generic kernels above
# them (33, 40) and empty rows; 3 to 5 rows each, so that rows_per_wave 2, 3 and 5 leave remainders.
MATRIX_ROW_DEGS = {**{d: 3 + d % 3 for d in range(0, 34)}, 40: 3}
# Column degrees: empty columns, every unrolled variable-node body (1 ... 16) and the generic kernel (17, 20).
MATRIX_COL_FIXED = {**{d: 6 for d in range(0, 17) if d != 3}, 17: 3, 20: 3}


def matrix_code(seed=20261016):
    """The irregular code of the streaming tests: MATRIX_ROW_DEGS, MATRIX_COL_FIXED and degree-3 columns for
    the rest of the edges (a degree-2 or degree-4 column absorbs a remainder of 1 or 2 if need be)."""
    E = sum(d * n for d, n in MATRIX_ROW_DEGS.items())
    col = dict(MATRIX_COL_FIXED)
    rest = E - sum(d * n for d, n in col.items())
    col[3], r = divmod(rest, 3)
    if r == 1:
        col[4] += 1
        col[3] -= 1
    elif r == 2:
        col[2] += 1
    return irregular_code(MATRIX_ROW_DEGS, col, seed)


def ira_code(d, n_link, extra, info_col_deg=3, seed=1):
    """IRA (staircase) code for the column-fused check kernel: n_link rows of degree d, each with the staircase
    parity columns p_{i-1}, p_i (degree 2, p_last of degree 1) and information edges, followed by `extra` rows
    ({degree: count}, degrees != d) on information columns only.  Information columns have degree
    info_col_deg (a few one higher to absorb the remainder).  Returns (rows, cols, M, N, K)."""
    assert d not in extra and d >= 3
    rng = np.random.default_rng(seed)
    n_extra = sum(extra.values())
    M = n_link + n_extra
    info_rdeg = np.array([d - 1] + [d - 2] * (n_link - 1) +
                         [k for k in sorted(extra) for _ in range(extra[k])], np.int64)
    E_info = int(info_rdeg.sum())
    K = E_info // info_col_deg
    cdeg = np.full(K, info_col_deg, np.int64)
    cdeg[:E_info - K * info_col_deg] += 1
    rows, cols = [], []
    left = cdeg.copy()
    for m in sorted(range(M), key=lambda m: (-info_rdeg[m], m)):
        k = int(info_rdeg[m])
        pick = np.lexsort((rng.random(K), -left))[:k]
        if left[pick].min() <= 0:
            raise ValueError("information degrees are not bigraphic")
        left[pick] -= 1
        rows.append(np.full(k, m, np.int64))
        cols.append(pick)
    # staircase: p_i in rows i and i + 1 (i < n_link - 1), p_last in row n_link - 1 only
    p = np.arange(n_link, dtype=np.int64)
    rows += [p, p[:-1] + 1]
    cols += [K + p, K + p[:-1]]
    r, c = codes.row_major(np.concatenate(rows), np.concatenate(cols))
    return r, c, M, K + n_link, K


# One entry per tuning key of capi.TUNE_FIELDS / capi.TUNE_INTS: the tuning dict of a case the kernel-matrix
# module runs, and the test that runs it.  Keys that other modules already cover name that test instead
# ("tune": None).  The forms of the column-fused check kernel (link_*) run in fp32 and sum-product there; with fp16
# messages, plain and corrected, tests/test_gpu_fp16.py::test_fp16_column_fused_forms runs them all again.  The launch
# plans of the streaming kernels (FLOOD_PLANS below: merge, check_wide, rows_per_wave, cols_per_wave, q_order, syn_xcd,
# tiles_first) run in fp32 here; the corrected and one-byte arithmetics (msc, msc16, ms8, msc8, msi*, msci*) get their degree
# matrix, under the same plans, in tests/test_gpu_flood_matrix.py::test_every_degree_class.
_KM = "test_gpu_kernel_matrix"
TUNE_CASES = {
    "fused": dict(tune={"fused": True, "ldsp": False}, test=_KM + "::test_one_launch_kernels_on_qc_shapes"),
    "ldsp": dict(tune={"fused": True, "ldsp": True}, test=_KM + "::test_one_launch_kernels_on_qc_shapes"),
    "ldsp_ext": dict(tune={"fused": True, "ldsp": True, "ldsp_ext": False}, test=_KM + "::test_one_launch_kernels_on_qc_shapes"),
    "ldsp_pack": dict(tune={"fused": True, "ldsp": True, "ldsp_pack": False}, test=_KM + "::test_one_launch_kernels_on_qc_shapes"),
    "link_narrow": dict(tune={"link_narrow": False}, test=_KM + "::test_column_fused_forms"),
    "check_wide": dict(tune={"check_wide": True}, test=_KM + "::test_streaming_flooding_every_degree_class"),
    "syn_xcd": dict(tune={"syn_xcd": False}, test=_KM + "::test_streaming_flooding_every_degree_class"),
    "fused_pack": dict(tune={"fused": True, "ldsp": False, "fused_pack": False}, test=_KM + "::test_one_launch_kernels_on_qc_shapes"),
    "fused_loop": dict(tune={"fused": True, "ldsp": False, "fused_loop": True}, test=_KM + "::test_one_launch_kernels_on_qc_shapes"),
    "device_tail": dict(tune=None, test="test_gpu_parity::test_device_side_tail_for_asynchronous_callers"),
    "merge": dict(tune={"merge": False}, test=_KM + "::test_streaming_flooding_every_degree_class"),
    "link_deep": dict(tune={"link_deep": True}, test=_KM + "::test_column_fused_forms"),
    "link_half": dict(tune={"link_half": True}, test=_KM + "::test_column_fused_forms"),
    "link_guided": dict(tune=None, test="test_gpu_parity::test_column_local_fusion_on_staircase_code"),
    "tiles_first": dict(tune={"tiles_first": True}, test=_KM + "::test_streaming_flooding_every_degree_class"),
    "rows_per_wave": dict(tune={"rows_per_wave": 3}, test=_KM + "::test_streaming_flooding_every_degree_class"),
    "cols_per_wave": dict(tune={"cols_per_wave": 3}, test=_KM + "::test_streaming_flooding_every_degree_class"),
    "link_rows": dict(tune={"link_rows": 5}, test=_KM + "::test_column_fused_forms"),
    "compact": dict(tune=None, test="test_gpu_parity::test_tail_compaction_of_running_frames"),
    "ldsp_grid": dict(tune=None, test="test_gpu_parity::test_layered_streaming_and_fused_paths_agree"),
    "ldsp_per_cu": dict(tune={"fused": True, "ldsp": True, "ldsp_per_cu": 1}, test=_KM + "::test_record_kernel_grid_and_waves"),
    "ldsp_waves": dict(tune={"fused": True, "ldsp": True, "ldsp_waves": 12}, test=_KM + "::test_record_kernel_grid_and_waves"),
    "place": dict(tune=None, test="test_gpu_fullsize::test_placement_search_keeps_results_and_reports_what_it_saw"),
    "q_order": dict(tune={"q_order": -1}, test=_KM + "::test_streaming_flooding_every_degree_class"),
}

# launch plans of the streaming flooding test (the irregular matrix code)
FLOOD_PLANS = {
    "default": {},
    "merge_off": {"merge": False},
    "check_wide": {"check_wide": True},
    "per_wave_1": {"rows_per_wave": 1, "cols_per_wave": 1},
    "per_wave_3": {"rows_per_wave": 3, "cols_per_wave": 3},
    "per_wave_5": {"rows_per_wave": 5, "cols_per_wave": 5},
    "q_order_edge": {"q_order": -1},
    "syn_xcd_off": {"syn_xcd": False},
    "tiles_first": {"tiles_first": True},
}


def all_tune_keys():
    return set(capi.TUNE_FIELDS) | set(capi.TUNE_INTS)


# ---- shared by test_gpu_kernel_matrix.py and test_gpu_ms_correction.py

def channel_frames(N, frames, lo, hi, seed):
    """All-zero codeword over AWGN, the noise level of each frame drawn from [lo, hi] (frames stop at every
    iteration from 1 to max_iter)."""
    y = channel.awgn_frames(N, 0, frames, 1.0, seed=seed)
    sd = np.random.default_rng(seed).uniform(lo, hi, frames).astype(np.float32)[:, None]
    return (np.float32(1) + (y - np.float32(1)) * sd).astype(np.float32)


def qc_base(z, mb, info_w, nb_info, seed, empty_col=None):
    """mb layers: layer l has info_w[l] information block columns and parity block column nb_info + l (a diagonal:
    the last entry of each layer, met by that layer only).  Every information block column is used at least once
    (except `empty_col`, used by none)."""
    rng = np.random.default_rng(seed)
    nb = nb_info + mb
    base = -np.ones((mb, nb), np.int64)
    cand = [j for j in range(nb_info) if j != empty_col]
    for l in range(mb):
        base[l, rng.choice(cand, info_w[l], replace=False)] = rng.integers(0, z, info_w[l])
        base[l, nb_info + l] = rng.integers(0, z)
    for j in cand:
        if (base[:nb_info, j] < 0).all():
            l = int(np.argmin((base >= 0).sum(axis=1)))
            base[l, j] = rng.integers(0, z)
    return base


# name: (z, base, expected one-launch eligibility: fused (LDS-resident), fused sum-product, record kernel)
QC_SHAPES = {
    "z24": (24, qc_base(24, 4, [5, 6, 7, 4], 10, seed=1), dict(fused=True, sp=True, ldsp=True)),
    "z200_4waves": (200, qc_base(200, 4, [3, 4, 3, 2], 5, seed=2), dict(fused=True, sp=True, ldsp=True)),
    "z600_maxw16": (600, qc_base(600, 3, [3, 2, 3], 5, seed=3), dict(fused=False, sp=False, ldsp=True)),
    "row28": (16, qc_base(16, 3, [27, 5, 9], 27, seed=4), dict(fused=True, sp=False, ldsp=False)),
    "empty_block_col": (32, qc_base(32, 4, [4, 5, 4, 5], 9, seed=5, empty_col=4), None),
}


def ldsp_shape(name):
    """flood_ldsp_kernel[G x B, F] -> (G, B, F)"""
    inner = name[name.index("[") + 1:name.index("]")]
    gb, f = inner.split(",")
    g, b = gb.split("x")
    return int(g), int(b), int(f)
