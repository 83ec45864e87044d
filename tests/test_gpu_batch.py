"""elp_solve_batch: the members the resident solver takes run
as one launch of k_resident_batch, one workgroup per LP; every other member is
solved by elp_solve inside the call.  The contract is `for i: elp_solve(hs[i])`
handle for handle and bit for bit, so every oracle comparison is
test_gpu_resident._same (status and trace equal, basis equal, objective and x
to 1e-12), and every comparison with a handle solved alone is exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import load_known_answers, load_mip_known_answers, load_sparse_lps
from fuzz_lps import fuzz_set

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOWN = load_known_answers()
BY_NAME = {r["name"]: r for r in KNOWN}
RULES = [(1, 6), (0, 6), (1, 5), (0, 5)]  # (pricing, simplex), alternating per handle
TRACE = 200000
# every elp_stats field that is not a timing (resident_ticks counts device clock ticks)
STAT_KEYS = ("iterations", "phase1_iterations", "bound_flips", "degenerate", "refactors", "bump_dim", "y_rows",
             "host_polls", "gj_refactors", "mip_nodes", "mip_lp_iterations", "max_inv_resid", "resident",
             "resident_launches", "dual_iterations", "simplex", "basis", "price_bytes", "iter_bytes")


def _same(g, o):
    """test_gpu_resident._same"""
    assert g.status == o.status, (g.status, o.status)
    np.testing.assert_array_equal(g.trace, o.trace)
    if g.status in (0, 1):
        np.testing.assert_array_equal(g.basis, o.basis)
        assert abs(g.objval - o.objval) <= 1e-12 * max(1.0, abs(o.objval))
        if len(o.x):
            np.testing.assert_allclose(g.x, o.x, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(o.x).max()))
    if g.status == 3:
        assert g.objval == o.objval
        np.testing.assert_array_equal(g.x, o.x)


def _identical(a, b, solved=True):
    """two GPU solutions, bit for bit (a batched member against the handle solved
    alone).  solved=False: the load decided the LP (lower > upper) and no solve
    ever wrote x, y or the basis -- elp_get_solution then reports whatever the
    handle's device buffers hold, and a handle created after another was
    destroyed recycles that one's buffers (measured: -0.0 in the batch, a
    leftover -26.33 in the lone handle created after the MIP's); status, trace
    and stats are what is defined."""
    assert a.status == b.status, (a.status, b.status)
    np.testing.assert_array_equal(a.trace, b.trace)
    if solved:
        np.testing.assert_array_equal(a.basis, b.basis, err_msg="basis")
        np.testing.assert_array_equal(a.x, b.x, err_msg="x")
        np.testing.assert_array_equal(a.y, b.y, err_msg="y")
        assert a.objval == b.objval or (np.isnan(a.objval) and np.isnan(b.objval))
    for k in STAT_KEYS:
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


def _args(rec):
    return (rec["A"], rec["dir"], rec["rhs"], rec["obj"], rec["lo"], rec["up"], rec["maximize"])


def _decided_at_load(rec):
    return rec["A"].shape[0] < 1 or bool(np.any(np.asarray(rec["lo"]) > np.asarray(rec["up"])))


def _load(gpu, rec, csc=False, is_int=None, **ctl):
    """a loaded Problem (the caller closes it)"""
    m, n = rec["A"].shape
    if csc:
        ctl.setdefault("basis", 1)
    p = gpu.Problem(m, n, **ctl)
    p.set_trace(TRACE)
    if csc:
        colptr, rowind, val, _ = gpu.csc_arrays(rec["A"])
        p.load_csc(colptr, rowind, val, *_args(rec)[1:])
    else:
        p.load_dense(*_args(rec))
    if is_int is not None:
        p.set_int(is_int)
    return p


def _oracle(rec, csc=False, **octl):
    from oracle import solve_dense as orc
    if csc:
        octl["price_mode"] = 1
    return orc(*_args(rec), trace_cap=TRACE, **octl)


def _close(ps):
    for p in ps:
        p.close()


def _known_batch(gpu, with_csc):
    ps, want, eligible = [], [], 0
    try:
        for csc in ((False, True) if with_csc else (False,)):
            for i, rec in enumerate(KNOWN):
                rule, simplex = RULES[i % 4]
                ps.append(_load(gpu, rec, csc=csc, pricing=rule, simplex=simplex))
                want.append(_oracle(rec, csc=csc, price_rule=rule, simplex=simplex))
                eligible += not _decided_at_load(rec)
        sts, nb = gpu.solve_batch(ps)
        assert nb == eligible
        k = 0
        for csc in ((False, True) if with_csc else (False,)):
            for rec in KNOWN:
                g = ps[k].solution(sts[k])
                try:
                    _same(g, want[k])
                    assert g.status == rec["expected"]["status"]
                    if not _decided_at_load(rec):
                        assert g.stats["resident"] == 1 and g.stats["resident_launches"] == 1
                        assert g.stats["host_polls"] == 1
                    else:
                        assert g.stats["resident"] == 0 and g.stats["resident_launches"] == 0
                except AssertionError as e:  # name the LP
                    raise AssertionError(f"{rec['name']} csc={csc}: {e}") from None
                k += 1
    finally:
        _close(ps)


def test_known_answers_one_batch(gpu):
    """Every known answer in one launch, pricing and simplex type alternating
    per handle: each against the oracle under the same controls."""
    _known_batch(gpu, with_csc=False)


def test_dense_and_csc_members_together(gpu):
    """The same records through elp_load_dense and elp_load_csc in one grid:
    neighbouring workgroups take the kernel's two load paths."""
    _known_batch(gpu, with_csc=True)


def _mixed_specs():
    big = next(r for r in load_sparse_lps() if r["m"] > 64)
    mip = next(r for r in load_mip_known_answers() if r["name"] == "investments")
    # (record, how it is loaded, batched?)
    return [
        (BY_NAME["readme"], {}, True),
        (big, {"csc": True}, False),                     # m > 64: the pipeline
        (mip, {"is_int": mip["is_int"]}, False),         # branch and bound
        (BY_NAME["lower_gt_upper"], {}, False),          # decided at the load
        (BY_NAME["dop"], {}, True),
        (BY_NAME["infeasible"], {}, True),               # (m = 2: the launch finds it infeasible)
        (BY_NAME["unbounded"], {}, False),               # m = 0
        (BY_NAME["brass"], {"resident": 2}, False),      # resident solver off
    ]


def test_mixed_eligibility(gpu):
    """Eligible and ineligible members interleaved: every member as a fresh
    handle solved alone by elp_solve gives it, in either order of the batch."""
    specs = _mixed_specs()
    alone = []
    for rec, kw, _ in specs:
        p = _load(gpu, rec, **kw)
        try:
            alone.append(p.solution(p.solve()))
        finally:
            p.close()
    for order in (list(range(len(specs))), list(reversed(range(len(specs))))):
        ps = [_load(gpu, specs[i][0], **specs[i][1]) for i in order]
        try:
            sts, nb = gpu.solve_batch(ps)
            assert nb == sum(1 for _, _, b in specs if b)
            for p, st, i in zip(ps, sts, order):
                rec, kw, batched = specs[i]
                g = p.solution(st)
                try:
                    _identical(g, alone[i], solved=not np.any(rec["lo"] > rec["up"]))
                    if batched:
                        assert g.stats["resident"] == 1 and g.stats["resident_launches"] == 1
                    elif "is_int" not in kw:
                        assert g.stats["resident"] == 0
                    # (the MIP: elp_solve's branch and bound sends its node LPs to the
                    #  single-LP resident launch, in the batch as alone -- _identical
                    #  holds its resident / resident_launches to the lone handle's)
                except AssertionError as e:
                    raise AssertionError(f"{rec['name']}: {e}") from None
        finally:
            _close(ps)
    assert alone[2].status == specs[2][0]["expected"]["status"]
    assert alone[1].stats["resident"] == 0


def test_fuzz_batches(gpu):
    """fuzz_set(120), dense and CSC, in grids of at most 64 handles: sizes, LDS
    carve-outs, pricing rules and refactor periods differ between neighbouring
    workgroups.  Every trace is the oracle's."""
    fuzz = fuzz_set(120)
    seen, ran = set(), 0
    for b0 in range(0, len(fuzz), 32):
        chunk = fuzz[b0:b0 + 32]
        ps, want = [], []
        try:
            for rec in chunk:
                ctl = {"pricing": rec["seed"] % 2, "refactor_period": 5 + rec["seed"] % 40}
                octl = {"price_rule": rec["seed"] % 2, "refactor_period": 5 + rec["seed"] % 40}
                for csc in (False, True):
                    ps.append(_load(gpu, rec, csc=csc, **ctl))
                    want.append(_oracle(rec, csc=csc, **octl))
            assert len(ps) <= 64
            sts, nb = gpu.solve_batch(ps)
            for k, (p, st) in enumerate(zip(ps, sts)):
                rec = chunk[k // 2]
                g = p.solution(st)
                try:
                    _same(g, want[k])
                except AssertionError as e:
                    raise AssertionError(f"f{rec['seed']}_{rec['m']}x{rec['n']} csc={k % 2}: {e}") from None
                seen.add(g.status)
                ran += g.stats["resident"]
            assert nb == sum(p.stats()["resident"] for p in ps)
        finally:
            _close(ps)
    assert {0, 2, 3} <= seen
    assert ran >= len(fuzz)  # (most fit; m > 64 takes the pipeline)


def _klee_minty(n):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_sparse import klee_minty
    A, dirs, rhs, obj, lo, up, mx = klee_minty(n)
    return {"name": f"klee_minty_{n}", "A": A.toarray(), "dir": dirs, "rhs": rhs, "obj": obj, "lo": lo, "up": up,
            "maximize": mx}


def test_isolation_from_a_timed_out_neighbour(gpu):
    """A Klee-Minty cube of 2^18 - 1 Dantzig pivots stops on its 5 ms time
    limit; its neighbours in the same launch reach their oracle answers."""
    km18, km6, dop = _klee_minty(18), _klee_minty(6), BY_NAME["dop"]
    ps = [_load(gpu, km6, pricing=0, scaling=0),
          _load(gpu, km18, pricing=0, scaling=0, resident=1, time_limit=0.005),
          _load(gpu, dop)]
    try:
        sts, nb = gpu.solve_batch(ps)
        assert nb == 3
        assert sts[1] == 7
        assert 0 < ps[1].stats()["iterations"] < 2 ** 18 - 1
        _same(ps[0].solution(sts[0]), _oracle(km6, price_rule=0, scaling=0))
        _same(ps[2].solution(sts[2]), _oracle(dop))
        assert sts[0] == 0 and sts[2] == 0
        assert ps[0].stats()["iterations"] == 2 ** 6 - 1
    finally:
        _close(ps)


def test_after_the_batch(gpu):
    """What later calls read is the single launch's: the sensitivity report is
    bit-equal to the report after elp_solve, and elp_solve on a batch-solved
    handle returns the final status without a launch."""
    recs = [BY_NAME[k] for k in ("dop", "transport", "modified_simple", "brass")]
    ps = [_load(gpu, r) for r in recs]
    try:
        sts, nb = gpu.solve_batch(ps)
        assert nb == len(recs) and sts == [0] * len(recs)
        for p, rec in zip(ps, recs):
            q = _load(gpu, rec)
            try:
                assert q.solve() == 0
                a, b = p.sensitivity(), q.sensitivity()
                for key in ("objfrom", "objtill", "duals", "dualsfrom", "dualstill"):
                    np.testing.assert_array_equal(a[key], b[key], err_msg=f"{rec['name']} {key}")
                _identical(p.solution(0), q.solution(0))
            finally:
                q.close()
            before = p.stats()
            assert p.solve() == 0
            after = p.stats()
            assert after["resident_launches"] == before["resident_launches"] == 1
            assert after["host_polls"] == before["host_polls"]
    finally:
        _close(ps)


def test_batch_of_one(gpu):
    rec = BY_NAME["dop"]
    p = _load(gpu, rec)
    try:
        sts, nb = gpu.solve_batch([p])
        assert nb == 1
        _same(p.solution(sts[0]), _oracle(rec))
    finally:
        p.close()


def test_nothing_eligible(gpu):
    recs = [BY_NAME[k] for k in ("dop", "brass", "unbounded", "lower_gt_upper")]
    ps = [_load(gpu, r, resident=2) for r in recs]
    qs = [_load(gpu, r, resident=2) for r in recs]
    try:
        sts, nb = gpu.solve_batch(ps)
        assert nb == 0
        for p, q, st, rec in zip(ps, qs, sts, recs):
            _identical(p.solution(st), q.solution(q.solve()), solved=not np.any(rec["lo"] > rec["up"]))
            assert p.stats()["resident"] == 0
    finally:
        _close(ps + qs)


def test_duplicate_handle_is_refused(gpu):
    """ELP_E_ARG before anything runs: both handles solve correctly afterwards."""
    from easylp_amd._lib import load
    lib = load()
    ra, rb = BY_NAME["dop"], BY_NAME["transport"]
    a, b = _load(gpu, ra), _load(gpu, rb)
    try:
        hs = (ctypes.c_void_p * 3)(a._h, b._h, a._h)
        st = (ctypes.c_int32 * 3)(-9, -9, -9)
        nb = ctypes.c_int64(-1)
        assert lib.elp_solve_batch(hs, 3, st, ctypes.byref(nb)) == -1
        assert b"twice" in lib.elp_last_error()
        assert list(st) == [-9, -9, -9] and nb.value == 0
        assert a.stats()["resident_launches"] == 0 and a.stats()["iterations"] == 0
        assert b.stats()["resident_launches"] == 0 and b.stats()["iterations"] == 0
        with pytest.raises(gpu.solver._lib.ElpError):
            gpu.solve_batch([a, a])
        sts, nbv = gpu.solve_batch([a, b])
        assert nbv == 2
        _same(a.solution(sts[0]), _oracle(ra))
        _same(b.solution(sts[1]), _oracle(rb))
    finally:
        _close([a, b])


def test_solve_dense_batch(gpu):
    """The one-shot wrapper: tuples and dicts, per-LP overrides."""
    dop, brass = BY_NAME["dop"], BY_NAME["brass"]
    lps = [_args(dop),
           {"A": brass["A"], "dirs": brass["dir"], "rhs": brass["rhs"], "obj": brass["obj"], "lo": brass["lo"],
            "up": brass["up"], "maximize": brass["maximize"], "trace": TRACE, "pricing": 0, "sensitivity": True},
           _args(dop) + (TRACE,)]
    sols = gpu.solve_dense_batch(lps, simplex=5)
    assert [s.stats["batched"] for s in sols] == [1, 1, 1]
    assert sols[0].trace is None and sols[1].sens is not None
    _same(sols[1], _oracle(brass, price_rule=0, simplex=5))
    _same(sols[2], _oracle(dop, simplex=5))
    assert sols[0].objval == sols[2].objval
