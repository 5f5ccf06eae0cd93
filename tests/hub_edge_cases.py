"""Shared by tests/test_hub_edges.py (host) and tests/test_hub_edges_gpu.py (device): two patterns that put the hub-row kernels (Plan::lcb, longcb.cpp; the five
kernel pairs that walk lcb.unit / lcb.ptr and the partial buffer [column block][hub row]) at the edges of their unit tables, the three plan forms they are built
in, and the value families of the other *_cases.py on them.  A hub row here is a row of >= 64 nonzeros: every form is built with long_cb = 1, block_longest = 64.

"crowd"       n = 70 000 = 3 f16 column blocks of 32768 (the last one 4464 wide) / 5 f64 blocks of 16384; 500 stream rows of 0..39 columns around 1302 hub rows.
              Hub index (the position among the hub rows, which is the row's index in every lcb table):
                1300 crowd rows of 64, 128, 129, 200, 65, 127 columns (cycling) inside [0, 16384): one-step pieces without a pad (128) and with 127 pads (129);
                5, 700, 1029, 1290 hold 3 more columns inside [32768, 49152); 1100 holds 130 more inside [65536, 70000);
                1050 holds 40 000: 17000 in [0, 32768), 20000 in [32768, 65536) -- 157 steps of f16 block 1 --, 3000 in [65536, 70000);
                1200 holds every column of [32768, 65536): one piece of 256 steps.
              f16 block 1 then has a unit of exactly 1024 pieces (0 .. 1023: two of them hold a step each, 1022 are empty pieces INSIDE a unit), a unit of
              1 + 157 + 256 = 414 steps (1024 .. 1200: a second pass of the step loop that ends inside a group of 16) and a last one; f16 block 2 (f64 block 4) has
              1024 empty pieces that belong to NO unit in front of its only unit; block 0's units are cut by their elements and hold about 190 one- and two-step pieces.
"manyblocks"  n = 300 x 32768 - 1000: 300 f16 column blocks / 600 f64 ones, the last one partial; about 290 stream rows around hub rows of 3000, 9000, 700, 64 and
              2000 random columns and one of 500 columns that all lie in f16 blocks 257 and 258: a reduce kernel that strides the column blocks by 64 or 256 reaches
              that row's pieces only in a later trip of its loop.

That these edges are really in the built plans, and that the value families still tell a wrong kernel from a right one on these shapes, is asserted on the CPU in
tests/test_hub_edges.py.  Everything handed out is computed once, shared and read-only."""
import numpy as np

import exact_cases as X
import semiring_cases as S
import tp_exact_cases as T
import wide_cases as W

PATTERNS = ("crowd", "manyblocks")
HUB_MIN = 64
FORMS = {
    "hybrid": dict(precision=16, two_phase=1, long_cb=1, block_longest=HUB_MIN),
    "panels64": dict(precision=64, two_phase=-1, col_panels=2, long_cb=1, block_longest=HUB_MIN),
    "panels16": dict(precision=16, two_phase=-1, col_panels=2, long_cb=1, block_longest=HUB_MIN),
}
F16_CB, F64_CB = 32768, 16384

CROWD_N = 70000
CROWD_LENS = (64, 128, 129, 200, 65, 127)
CROWD_HUBS = 1302
CROWD_THREE, CROWD_TAIL, CROWD_WIDE, CROWD_FULL = (5, 700, 1029, 1290), 1100, 1050, 1200          # hub indices
MANY_N = 300 * F16_CB - 1000
MANY_LENS = (3000, 9000, 700, 64, 2000)
MANY_LATE = 500                                                                                    # the row inside f16 blocks 257 and 258
MANY_LATE_BLOCKS = (257, 259)
HUB_ROWS = {"crowd": CROWD_HUBS, "manyblocks": len(MANY_LENS) + 1}

_patterns = {}
_cache = {}


def _csr(rows, n):
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([c.size for c in rows])
    return X._freeze(rp, np.concatenate(rows), n)


def _stream_rows(rng, k, n):
    """k rows of 0..39 random columns, every 25th one empty"""
    return [np.sort(rng.choice(n, 0 if i % 25 == 0 else int(rng.integers(0, 40)), replace=False)) for i in range(k)]


def _crowd(hubs=CROWD_HUBS):
    rng = np.random.default_rng(41)
    rows = _stream_rows(rng, 250, CROWD_N)
    k = 0
    for i in range(hubs):
        if i == CROWD_WIDE:
            c = np.concatenate([rng.choice(F16_CB, 17000, replace=False), F16_CB + rng.choice(F16_CB, 20000, replace=False),
                                2 * F16_CB + rng.choice(CROWD_N - 2 * F16_CB, 3000, replace=False)])
        elif i == CROWD_FULL:
            c = F16_CB + np.arange(F16_CB)
        else:
            c = rng.choice(F64_CB, CROWD_LENS[k % len(CROWD_LENS)], replace=False)
            k += 1
            if i in CROWD_THREE:
                c = np.concatenate([c, F16_CB + rng.choice(F64_CB, 3, replace=False)])
            if i == CROWD_TAIL:
                c = np.concatenate([c, 2 * F16_CB + rng.choice(CROWD_N - 2 * F16_CB, 130, replace=False)])
        rows.append(np.sort(c))
    rows += _stream_rows(rng, 250, CROWD_N)
    return _csr(rows, CROWD_N)


def _manyblocks():
    rng = np.random.default_rng(43)
    rows = _stream_rows(rng, 150, MANY_N)
    for L in MANY_LENS[:3]:
        rows.append(np.sort(rng.choice(MANY_N, L, replace=False)))
    rows += _stream_rows(rng, 20, MANY_N)
    for L in MANY_LENS[3:]:
        rows.append(np.sort(rng.choice(MANY_N, L, replace=False)))
    b0, b1 = MANY_LATE_BLOCKS
    rows.append(np.sort(b0 * F16_CB + rng.choice((b1 - b0) * F16_CB, MANY_LATE, replace=False)))
    rows += _stream_rows(rng, 120, MANY_N)
    return _csr(rows, MANY_N)


def pattern(name):
    """name -> (rp, ci, n), read-only int32 arrays"""
    if name not in _patterns:
        _patterns[name] = _crowd() if name == "crowd" else _manyblocks()
    return _patterns[name]


def hub_rows(rp):
    """the rows that every form hands to the hub kernels, in hub index order"""
    return np.flatnonzero(np.diff(np.asarray(rp, np.int64)) >= HUB_MIN)


def late_row(rp):
    """"manyblocks": the hub index of the row whose columns all lie in f16 blocks 257 and 258 (the last hub row)"""
    return int(hub_rows(rp).size - 1)


def _shared(key, make):
    if key not in _cache:
        out = make()
        for arr in out:
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def exact_case(name, seed):
    """(rp, ci, n, a, x, y) of exact_cases.exact_values: float64, all exact in f16, y in natural row order"""
    rp, ci, n = pattern(name)
    return (rp, ci, n) + _shared(("exact", name, seed), lambda: X.exact_values(rp, ci, n, seed))


def cancel_case(name, seed):
    """(rp, ci, n, a, x, want): tp_exact_cases.cancellation_values (float16) and the exact model's y (float16, natural row order)"""
    rp, ci, n = pattern(name)

    def make():
        a, x = T.cancellation_values(rp, ci, n, seed)
        return a, x, T.model_spmv(rp, ci, a, x)
    return (rp, ci, n) + _shared(("cancel", name, seed), make)


def wide_case(name, e, seed=W.SEED):
    """(rp, ci, n, a, x, k, want): wide_cases.values at scale 2^e and float32(exact row sum), natural row order"""
    rp, ci, n = pattern(name)

    def make():
        a, x, k = W.values(rp, ci, n, seed, e)
        return a, x, k, W.to_f32(W.row_sums(rp, ci, a, k), e)
    return (rp, ci, n) + _shared(("wide", name, e, seed), make)


def semiring_case(name, seed=S.SEED):
    """(rp, ci, n, a, x, {semiring: want}): semiring_cases.values and its model, natural row order"""
    rp, ci, n = pattern(name)

    def make():
        a, x = S.values(rp, ci, n, seed)
        return (a, x) + tuple(S.model(s, rp, ci, a, x) for s in S.SEMIRINGS)
    a, x, *want = _shared(("semiring", name, seed), make)
    return rp, ci, n, a, x, dict(zip(S.SEMIRINGS, want))


def in_order_f16(rp, p, rows, dtype):
    """the sums of `rows` accumulated in `dtype` in storage order from the exact products p (float64), rounded to f32 and f16 like a result"""
    rp = np.asarray(rp, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([np.cumsum(p[rp[r]:rp[r + 1]].astype(dtype), dtype=dtype)[-1] for r in rows], np.float64).astype(np.float32).astype(np.float16)
