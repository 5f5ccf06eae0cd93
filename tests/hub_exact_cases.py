"""Shared by tests/test_hub_exact.py (host) and tests/test_hub_exact_gpu.py (device): the two hybrid patterns of the exact hub rows
(dasp_plan_set_hub_exact), with the cancellation values and the model of tests/tp_exact_cases.py.

Both patterns have n = 140000 columns = 5 column blocks of 32768 (the last one 8928 wide), and with two_phase = 1 their rows of >= 128 x 5 nonzeros become
hub rows (column-blocked), every other row stays in the two-phase streams:
  "hub"    exact_cases.pattern("hub"): 5106 rows, hub rows of 40000, 33000 and 9000.
  "hubs2"  about 3000 rows of 7; six rows of 40000 -- about 48000 hub elements per column block against units of 32768, so the plan has more units than
           column blocks and most blocks' pieces are spread over two workgroups; one row of 9000 whose columns all lie in 40000 .. 60000, inside column
           block 1, so four of its five (row, block) pieces are empty and are never written; rows of 0, 1 and 2.

What makes a test on these mean something is asserted here, on the CPU, for every case handed out: on EVERY hub row an f32 sum and an f64 sum of the
products in storage order both miss the model in the f16 bits of the result -- hub kernels that still add in floating point cannot pass."""
import numpy as np

import exact_cases as X
import tp_exact_cases as T

N = X.HUB_N
COL_BLOCK = 32768
N_CB = (N + COL_BLOCK - 1) // COL_BLOCK
HUB_MIN = 128 * N_CB                   # the hybrid's rule: a hub row holds at least one whole step of the hub kernel per column block
HUBS2_SEED = 31

assert N_CB == 5


def hub_rows(rp):
    """the rows a forced two-phase plan of these patterns hands to the hub kernels"""
    return np.flatnonzero(np.diff(np.asarray(rp, np.int64)) >= HUB_MIN)


def hubs2_pattern():
    import util
    lens = [7] * 1500 + [40000] * 3 + [0, 1, 2] + [7] * 1500 + [40000] * 3 + [9000, 2, 0, 1]
    rp, ci, _ = util.csr_from_lengths(lens, N, HUBS2_SEED)
    r = lens.index(9000)
    ci = np.array(ci)
    ci[rp[r]:rp[r + 1]] = np.random.default_rng(HUBS2_SEED + 1).integers(40000, 60001, 9000)
    assert ci[rp[r]:rp[r + 1]].min() // COL_BLOCK == 1 and ci[rp[r]:rp[r + 1]].max() // COL_BLOCK == 1
    return rp, ci, N


def in_order(rp, p, dtype):
    """the hub rows' sums accumulated in `dtype` in storage order, rounded to f16 like a result: {row: f16}"""
    rp = np.asarray(rp, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        return {int(r): np.cumsum(p[rp[r]:rp[r + 1]].astype(dtype), dtype=dtype)[-1].astype(np.float32).astype(np.float16) for r in hub_rows(rp)}


_patterns = {}
_cache = {}


def pattern(name):
    if name not in _patterns:
        _patterns[name] = X.pattern("hub") if name == "hub" else X._freeze(*hubs2_pattern())
    return _patterns[name]


def case(name, seed):
    """(rp, ci, n, a, x, want) of "hub" or "hubs2": cancellation values, the model's y in natural row order; computed once, shared, read-only"""
    key = (name, seed)
    if key not in _cache:
        if name == "hub":
            rp, ci, n, a, x, want = T.case("hub", seed)
        else:
            rp, ci, n = pattern(name)
            a, x = T.cancellation_values(rp, ci, n, seed)
            want = T.model_spmv(rp, ci, a, x)
            for arr in (a, x, want):
                arr.setflags(write=False)
        hubs = hub_rows(rp)
        assert hubs.size == (3 if name == "hub" else 7) and n == N
        p = T._products(a, np.asarray(x)[np.asarray(ci, np.int64)])
        for dtype in (np.float32, np.float64):
            got = in_order(rp, p, dtype)
            for r in hubs:
                assert not T.same_bits(got[int(r)], want[r]), (name, seed, int(r), dtype.__name__, float(got[int(r)]), float(want[r]))
        _cache[key] = (rp, ci, n, a, x, want)
    return _cache[key]
