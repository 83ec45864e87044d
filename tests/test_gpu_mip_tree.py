"""Resident branch and bound: a small MIP's whole tree -- node
LPs, node stack, incumbent -- inside launches of k_resident_tree.  The rules
are the oracle's (orc_solve_mip) and the node LPs are bit-identical, so every
comparison is exact: status, objective, x, node and LP-iteration counts against
oracle.solve_mip, and trace and statistics against the per-node host loop
(ELP_RESIDENT_TREE=0) on the same library."""
import functools
import math
import time

import numpy as np
import pytest

from conftest import load_known_answers, load_mip_known_answers

pytestmark = pytest.mark.gpu

MIP = {r["name"]: r for r in load_mip_known_answers()}
LPS = {r["name"]: r for r in load_known_answers()}
TRACE = 4096
# the fields that may differ between the tree and the per-node path
NOT_COMPARED = ("host_polls", "resident_launches", "resident_ticks")


def gen(seed, m, n, ub):
    rng = np.random.default_rng(seed)
    A = rng.integers(1, 40, (m, n)).astype(float)
    b = np.floor(A.sum(axis=1) * 0.37 * ub / 3) + 0.5
    c = rng.integers(1, 60, n).astype(float)
    return A, np.ones(m, np.int32), b, c, np.zeros(n), np.full(n, float(ub)), True


def gen_mixed(seed, m, n):
    """Minimise; >= rows and one == row through an integer point; lower bounds
    -4, 0 and (last column) -infinity, upper 5.5; every other column integer.
    Every third seed lets the free column fall for ever: an unbounded relaxation."""
    rng = np.random.default_rng(1000 + seed)
    A = rng.integers(-9, 30, (m, n)).astype(float)
    x0 = rng.integers(0, 4, n).astype(float)
    dirs = np.full(m, 2, np.int32)
    dirs[m // 2] = 3
    if seed % 3 == 2:
        A[:, n - 1] = -np.abs(A[:, n - 1])
        A[m // 2, n - 1] = 0.0
    b = A @ x0
    b[dirs == 2] -= rng.integers(0, 6, m)[dirs == 2] + 0.5
    c = rng.integers(1, 50, n).astype(float)
    lo = np.where(np.arange(n) % 3 == 0, -4.0, 0.0)
    lo[n - 1] = -np.inf
    up = np.full(n, 5.5)
    is_int = (np.arange(n) % 2 == 0).astype(np.int32)
    return (A, dirs, b, c, lo, up, False), is_int


# (m, n, ub, seed) and the oracle's (nodes, LP iterations) under Devex
GENERATED = {(1, 5, 3, 0): (29, 29), (2, 3, 7, 0): (23, 28), (5, 10, 3, 0): (153, 339), (10, 20, 1, 0): (203, 619),
             (64, 40, 1, 2): (2179, 20733), (6, 70, 1, 0): (4287, 15479)}
MIXED = [(m, n, seed) for (m, n) in ((4, 7), (8, 12), (12, 20)) for seed in range(6)]


@functools.lru_cache(maxsize=None)
def _model(key):
    """(args, is_int) of a named reference MIP, ("gen", m, n, ub, seed) or ("mixed", m, n, seed)"""
    if isinstance(key, str):
        r = MIP[key]
        return (r["A"], r["dir"], r["rhs"], r["obj"], r["lo"], r["up"], r["maximize"]), r["is_int"]
    if key[0] == "gen":
        _, m, n, ub, seed = key
        return gen(seed, m, n, ub), np.ones(n, np.int32)
    _, m, n, seed = key
    return gen_mixed(seed, m, n)


@functools.lru_cache(maxsize=None)
def _oracle(key, pricing=1, csc=False, max_nodes=0, max_iter=0, simplex=0):
    from oracle import solve_mip
    args, is_int = _model(key)
    ctl = {"price_rule": pricing}
    if csc:
        ctl["price_mode"] = 1
    if max_iter:
        ctl["max_iter"] = max_iter
    if simplex:
        ctl["simplex"] = simplex
    return solve_mip(*args, is_int, max_nodes=max_nodes, **ctl)


def _gpu(gpu, key, pricing=1, csc=False, model=None, **ctl):
    args, is_int = model if model is not None else _model(key)
    solve = gpu.solve_sparse if csc else gpu.solve_dense
    if csc:
        ctl.setdefault("basis", 1)
    return solve(*args, is_int=is_int, trace=TRACE, pricing=pricing, **ctl)


def _same(g, o):
    """(the oracle reports objective and x of an incumbent only: status 0, or 1 with one found)"""
    assert g.status == o.status, (g.status, o.status)
    if o.status == 0 or (o.status == 1 and o.objval != 0.0):
        assert g.objval == o.objval, (g.objval, o.objval)
        np.testing.assert_array_equal(g.x, o.x)
    assert g.stats["mip_nodes"] == o.stats["nodes"]
    assert g.stats["mip_lp_iterations"] == o.stats["lp_iterations"]
    assert g.mip["nodes"] == o.stats["nodes"] and g.mip["lp_iterations"] == o.stats["lp_iterations"]


def _in_tree(g):
    """the whole search ran inside the tree kernel"""
    assert g.mip["tree_launches"] >= 1, g.mip
    assert g.mip["tree_nodes"] == g.mip["nodes"], g.mip
    assert g.mip["handbacks"] == 0, g.mip
    assert g.stats["resident"] == 1 and g.stats["resident_launches"] == g.mip["tree_launches"]


def _parity_cases():
    out = []
    for name in ("investments", "cyingair"):
        for csc in (False, True):
            for pricing in (0, 1):
                out.append(pytest.param(name, pricing, csc, id=f"{name}-{'csc' if csc else 'dense'}-p{pricing}"))
    for (m, n, ub, seed) in GENERATED:
        for pricing in (0, 1):
            out.append(pytest.param(("gen", m, n, ub, seed), pricing, False, id=f"gen{m}x{n}u{ub}s{seed}-p{pricing}"))
    return out


@pytest.mark.parametrize("key,pricing,csc", _parity_cases())
def test_parity_with_the_oracle(gpu, key, pricing, csc):
    g = _gpu(gpu, key, pricing, csc)
    _in_tree(g)
    o = _oracle(key, pricing, csc)
    _same(g, o)
    if isinstance(key, str):
        assert g.mip["tree_launches"] == 1  # (the default slice: 20 ms)
    elif pricing == 1:
        assert o.status == 0 and (o.stats["nodes"], o.stats["lp_iterations"]) == GENERATED[key[1:]]


@pytest.mark.parametrize("key,pricing,csc", _parity_cases())
def test_same_as_the_per_node_path(gpu, monkeypatch, key, pricing, csc):
    g = _gpu(gpu, key, pricing, csc)
    monkeypatch.setenv("ELP_RESIDENT_TREE", "0")
    h = _gpu(gpu, key, pricing, csc)
    assert h.mip["tree_launches"] == 0 and h.mip["tree_nodes"] == 0 and h.mip["handbacks"] == 0
    assert g.status == h.status
    assert g.objval == h.objval
    np.testing.assert_array_equal(g.x, h.x)
    np.testing.assert_array_equal(g.trace, h.trace)
    for k in g.stats:
        if k.startswith("seconds_") or k in NOT_COMPARED:
            continue
        assert g.stats[k] == h.stats[k], (k, g.stats[k], h.stats[k])
    assert g.mip["max_open"] == h.mip["max_open"]


def test_mixed_generator_covers_both_kinds():
    """what the mixed set is for: long trees and the unbounded exit (the oracle alone)"""
    res = [_oracle(("mixed", m, n, s)) for (m, n, s) in MIXED]
    assert sum(o.status == 0 and o.stats["nodes"] > 50 for o in res) >= 3
    assert sum(o.status == 3 and o.stats["nodes"] == 1 for o in res) >= 3


@pytest.mark.parametrize("pricing", [0, 1])
@pytest.mark.parametrize("m,n,seed", MIXED)
def test_mixed_senses_and_bounds(gpu, m, n, seed, pricing):
    key = ("mixed", m, n, seed)
    g = _gpu(gpu, key, pricing)
    _in_tree(g)
    _same(g, _oracle(key, pricing))


@pytest.mark.parametrize("k", [1, 7])
def test_pause_and_resume(gpu, monkeypatch, k):
    monkeypatch.setenv("ELP_TREE_SLICE_NODES", str(k))
    g = _gpu(gpu, "cyingair")
    o = _oracle("cyingair")
    assert g.mip["tree_launches"] == math.ceil(o.stats["nodes"] / k) == {1: 241, 7: 35}[k]
    _in_tree(g)
    _same(g, o)
    monkeypatch.delenv("ELP_TREE_SLICE_NODES")
    np.testing.assert_array_equal(g.trace, _gpu(gpu, "cyingair").trace)


@pytest.mark.parametrize("key", [("gen", 5, 10, 3, 0), "cyingair"], ids=["gen5x10", "cyingair"])
def test_hand_back_on_a_full_stack(gpu, monkeypatch, key):
    monkeypatch.setenv("ELP_TREE_STACK", "2")
    g = _gpu(gpu, key)
    assert g.mip["tree_launches"] >= 1
    assert g.mip["handbacks"] == 1, g.mip
    assert 0 < g.mip["tree_nodes"] < g.mip["nodes"], g.mip
    _same(g, _oracle(key))
    monkeypatch.delenv("ELP_TREE_STACK")
    full = _gpu(gpu, key)
    np.testing.assert_array_equal(g.trace, full.trace)
    assert g.mip["max_open"] == full.mip["max_open"] > 2


def test_node_limit(gpu):
    want = {1: (1, 1, 9), 2: (1, 2, 12), 5: (1, 5, 19), 60: (1, 60, 86), 240: (1, 240, 375), 241: (0, 241, 375)}
    for cap, exp in want.items():
        o = _oracle("cyingair", max_nodes=cap)
        assert (o.status, o.stats["nodes"], o.stats["lp_iterations"]) == exp, cap
        g = _gpu(gpu, "cyingair", max_nodes=cap)
        _in_tree(g)
        _same(g, o)
        if cap == 60:
            assert g.objval == 124.6


def test_iteration_budget(gpu):
    want = {1: (1, 1, 1), 3: (1, 1, 3), 100: (1, 70, 100), 374: (1, 239, 374), 375: (1, 239, 375), 380: (0, 241, 375)}
    for cap, exp in want.items():
        o = _oracle("cyingair", max_iter=cap)
        assert (o.status, o.stats["nodes"], o.stats["lp_iterations"]) == exp, cap
        g = _gpu(gpu, "cyingair", max_iter=cap)
        _in_tree(g)
        _same(g, o)


def test_time_limit(gpu):
    model = (gen(0, 30, 60, 3), np.ones(60, np.int32))
    t0 = time.time()
    g = _gpu(gpu, None, model=model, time_limit=0.05)
    el = time.time() - t0
    assert g.status in (1, 7)
    assert el < 5.0
    assert g.mip["tree_launches"] >= 1


def test_root_cases(gpu):
    """integer bounds rounded at the root (a cold load before the tree), and a
    root the rounding makes infeasible (decided at the load, no launch)"""
    from oracle import solve_mip
    A, d, b, c, lo, up, mx = gen(0, 5, 10, 3)
    lo, up = lo.copy(), up.copy()
    lo[0], up[1], lo[2], up[2] = 0.5, 2.5, 0.2, 1.8
    ii = np.ones(10, np.int32)
    o = solve_mip(A, d, b, c, lo, up, mx, ii)
    assert (o.status, o.stats["nodes"], o.stats["lp_iterations"], o.objval) == (0, 19, 20, 74.0)
    g = _gpu(gpu, None, model=((A, d, b, c, lo, up, mx), ii))
    _in_tree(g)
    _same(g, o)
    lo[3], up[3] = 0.2, 0.8
    o = solve_mip(A, d, b, c, lo, up, mx, ii)
    assert (o.status, o.stats["nodes"], o.stats["lp_iterations"]) == (2, 1, 0)
    g = _gpu(gpu, None, model=((A, d, b, c, lo, up, mx), ii))
    assert g.status == 2 and g.stats["mip_nodes"] == 1 and g.stats["mip_lp_iterations"] == 0
    assert g.mip["tree_launches"] == 0


@pytest.mark.parametrize("key,ctl", [("students", {}), ("investments", {"simplex": 5}), ("investments", {"resident": 2})],
                         ids=["m275", "primal_primal", "resident_off"])
def test_not_eligible(gpu, key, ctl):
    g = _gpu(gpu, key, **ctl)
    assert g.mip["tree_launches"] == 0 and g.mip["tree_nodes"] == 0 and g.mip["handbacks"] == 0
    _same(g, _oracle(key, simplex=ctl.get("simplex", 0)))


def _load(gpu, key, p=None):
    args, is_int = _model(key)
    if p is None:
        p = gpu.Problem(*args[0].shape)
        p.set_trace(TRACE)
    p.load_dense(*args)
    p.set_int(is_int)
    return p


def _identical(a, b):
    assert a.status == b.status and a.objval == b.objval
    np.testing.assert_array_equal(a.x, b.x)
    np.testing.assert_array_equal(a.trace, b.trace)
    for k in a.stats:
        if not k.startswith("seconds_") and k not in NOT_COMPARED:
            assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])
    assert a.mip == b.mip


def test_reuse(gpu):
    """A handle's shape is fixed at elp_create, so a handle is loaded again with
    its own model; the other model takes the destroyed handle's resources -- the
    tree record among them, grown for the larger n -- through the next create."""
    fresh = {k: _gpu(gpu, k) for k in ("investments", "cyingair")}
    p = _load(gpu, "investments")
    try:
        first = p.solution(p.solve())
        _in_tree(first)
        _identical(first, fresh["investments"])
        _load(gpu, "investments", p)
        again = p.solution(p.solve())
        _in_tree(again)
        _identical(again, fresh["investments"])
    finally:
        p.close()
    p = _load(gpu, "cyingair")
    try:
        g = p.solution(p.solve())
        _in_tree(g)
        _identical(g, fresh["cyingair"])
    finally:
        p.close()


def test_batch(gpu):
    def lp(name):
        r = LPS[name]
        p = gpu.Problem(*r["A"].shape)
        p.set_trace(TRACE)
        p.load_dense(r["A"], r["dir"], r["rhs"], r["obj"], r["lo"], r["up"], r["maximize"])
        return p

    make = [lambda: lp("readme"), lambda: _load(gpu, "investments"), lambda: lp("dop"), lambda: _load(gpu, "cyingair")]
    alone = []
    for mk in make:
        p = mk()
        try:
            alone.append(p.solution(p.solve()))
        finally:
            p.close()
    ps = [mk() for mk in make]
    try:
        sts, nb = gpu.solve_batch(ps)
        sols = [p.solution(st) for p, st in zip(ps, sts)]
    finally:
        for p in ps:
            p.close()
    assert sols[1].mip["tree_launches"] >= 1 and sols[3].mip["tree_launches"] >= 1
    assert nb == 2
    for g, a in zip(sols, alone):
        _identical(g, a)
        np.testing.assert_array_equal(g.basis, a.basis)
    assert sols[0].mip is None and sols[2].mip is None
    _same(sols[1], _oracle("investments"))
    _same(sols[3], _oracle("cyingair"))
