"""CPU tests of the device Hungarian solver's written rule (`assigner.lsap_wave_rule_host`: the parallel column selection of
csrc/lsap_device.hip in numpy) against scipy's INDICES, its status codes, and the gate `ops.lsap_device_ok` at its edges.
`problem_set()` is also what tests/test_assign_device_gpu.py hands to the kernel."""
import functools

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import cgg_amd  # noqa: F401
from cgg_amd import assigner, ops


@functools.lru_cache(maxsize=None)
def problem_set():
    """-> tuple of (f32 matrix, scipy rows, scipy cols): random rectangular both ways, integer costs (ties everywhere), binary
    costs, constant / single-row / single-column / tall matrices, squares past one lane stride, +inf entries with a feasible
    column. Computed once; nobody writes to the arrays."""
    rng = np.random.RandomState(0)
    mats = []
    for _ in range(60):
        nr, nc = rng.randint(1, 40), rng.randint(1, 40)
        mats.append(rng.randn(nr, nc).astype(np.float32))
    for _ in range(60):
        nr, nc = rng.randint(1, 25), rng.randint(1, 25)
        mats.append(rng.randint(0, 3, (nr, nc)).astype(np.float32))
    for _ in range(30):
        nr, nc = rng.randint(1, 25), rng.randint(1, 25)
        mats.append(rng.randint(0, 2, (nr, nc)).astype(np.float32))
    mats += [np.zeros((5, 9), np.float32), np.ones((9, 5), np.float32), np.zeros((1, 7), np.float32),
             np.zeros((7, 1), np.float32), rng.rand(100, 13).astype(np.float32), rng.rand(100, 1).astype(np.float32),
             np.zeros((70, 70), np.float32), np.zeros((65, 130), np.float32)]
    m = rng.rand(6, 8).astype(np.float32)
    m[m < 0.3] = np.inf                                   # forbidden pairs, still feasible
    m[:, 0] = 0.5
    mats.append(m)
    out = []
    for x in mats:
        x.setflags(write=False)
        r, c = linear_sum_assignment(x)
        out.append((x, r.astype(np.int64), c.astype(np.int64)))
    return tuple(out)


def test_wave_rule_returns_scipys_indices():
    assert len(problem_set()) == 159
    for x, wr, wc in problem_set():
        r, c, status = assigner.lsap_wave_rule_host(x)
        assert status == 0, x.shape
        assert r.dtype == np.int64 and c.dtype == np.int64
        assert r.tolist() == wr.tolist() and c.tolist() == wc.tolist(), x.shape


def test_wave_rule_status_codes():
    good = np.array([[3.0, 1.0, 2.0], [1.0, 5.0, 4.0]], np.float32)
    for bad, code in ((np.nan, ops.LSAP_INVALID), (-np.inf, ops.LSAP_INVALID)):
        x = good.copy()
        x[1, 2] = bad
        r, c, status = assigner.lsap_wave_rule_host(x)
        assert status == code == 1 and r.tolist() == [0, 1] and c.tolist() == [0, 1]      # identity pairing k -> (k, k)
    r, c, status = assigner.lsap_wave_rule_host(np.full((2, 2), np.inf, np.float32))
    assert status == ops.LSAP_INFEASIBLE == 2 and r.tolist() == [0, 1] and c.tolist() == [0, 1]
    r, c, status = assigner.lsap_wave_rule_host(np.full((5, 3), np.inf, np.float32))
    assert status == 2 and r.tolist() == [0, 1, 2] and c.tolist() == [0, 1, 2]
    assert assigner.lsap_wave_rule_host(good)[2] == ops.LSAP_OK == 0


def test_status_check_names_the_problem_with_the_host_solvers_messages():
    ops.lsap_status_check((0, 0))
    with pytest.raises(ops.CggError, match=r'problem 6: .*invalid numeric entries'):
        ops.lsap_status_check((1, 7))
    with pytest.raises(ops.CggError, match=r'problem 0: .*infeasible'):
        ops.lsap_status_check((2, 1))


def test_device_gate_at_its_edges():
    """The gate is host arithmetic on the library's own LDS formula and the limit it reports (gfx950's where there is no device)."""
    limit = int(ops._lib_().cgg_dynamic_lds_limit())
    assert 64 * 1024 <= limit <= 160 * 1024
    for nr, nc in ((0, 5), (5, 0), (0, 0), (-1, 3), (1025, 1), (1, 1025), (1025, 1025)):
        assert not ops.lsap_device_ok(nr, nc), (nr, nc)
    for nr, nc in ((1, 1), (1024, 1), (1, 1024), (100, 20), (200, 60), (100, 100)):
        assert ops.lsap_device_ok(nr, nc), (nr, nc)
    # staged f32 cost + state (u f64 | v, dist f64 | path, row4col, remaining i32 | col4row i32 | SR, SC bytes), 16-byte rounded
    need = lambda n: (4 * n * n + 42 * n + 15) // 16 * 16         # noqa: E731
    fits = max(n for n in range(1, 1025) if need(n) <= limit)
    assert fits < 1024
    assert ops.lsap_device_lds_bytes(fits, fits) == need(fits) and ops.lsap_device_lds_bytes(fits + 1, fits + 1) == need(fits + 1)
    assert ops.lsap_device_ok(fits, fits) and not ops.lsap_device_ok(fits + 1, fits + 1)
    # the transpose is what is staged: the gate is symmetric, and a long thin problem fits where its square would not
    assert ops.lsap_device_lds_bytes(100, 13) == ops.lsap_device_lds_bytes(13, 100) == (4 * 1300 + 13 * 13 + 29 * 100 + 15) // 16 * 16
    assert ops.lsap_device_ok(1024, 8) and not ops.lsap_device_ok(1024, 1024)
