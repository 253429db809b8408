"""The host form of the bounded L-BFGS (csrc/lbfgs_host.h, exported as lc_batched_lbfgs) against its restatement in
tests/_lbfgs.py, on analytic objectives: no GPU, but the built liblcmi.so, which these tests call through ctypes (without it
_lib.lib() raises, as for the suite's other ABI tests).  Library and restatement call the same Python objective, in double, with
their sums in the same (sequential) order, so x, the final loss and the number of evaluations are compared on raw bits.
Should a build contract the host arithmetic into fused multiply-adds the test says so and bounds the difference by 4 x the
restatement's own difference between its two summation orders instead.

tests/host/lbfgs_main.cpp runs the wrap, rejected-pair, line-search-failure and lock-step cases over the unmodified header
under the host compiler's address and undefined-behaviour sanitizers, as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _lbfgs as L
from tests.test_device_call_cpu import HOST, ROOT, _compiler


def host_lbfgs(evalfn, x0, lo, hi, maxiter, code=None):
    """lc_batched_lbfgs through ctypes.  Returns (rc, x, f_final, evaluations, calls)."""
    from lightcurver_amd import _lib
    lib = _lib.lib()
    x = np.array(x0, dtype=np.float64)
    nb, D = x.shape
    lo = np.ascontiguousarray(np.broadcast_to(lo, x.shape), dtype=np.float64)
    hi = np.ascontiguousarray(np.broadcast_to(hi, x.shape), dtype=np.float64)
    calls = [0]

    def cb(user, X, F, G):
        calls[0] += 1
        if code is not None and calls[0] == code[0]:
            return code[1]
        Xa = np.ctypeslib.as_array(X, (nb, D))
        f, g = evalfn(Xa.copy())
        np.ctypeslib.as_array(F, (nb,))[:] = f
        np.ctypeslib.as_array(G, (nb, D))[:] = g
        return 0
    fn = _lib.LBFGS_EVAL(cb)
    f = np.full(nb, -7.0)
    ne = C.c_int(-1)
    dp = _lib.dp
    rc = lib.lc_batched_lbfgs(nb, D, x.ctypes.data_as(dp), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), int(maxiter), fn,
                              None, f.ctypes.data_as(dp), C.byref(ne))
    return rc, x, f, ne.value, calls[0]


def compare(evalfn, x0, lo, hi, maxiter):
    """The library against the restatement on one problem set; returns the restatement's result."""
    rc, x, f, ne, calls = host_lbfgs(evalfn, x0, lo, hi, maxiter)
    ref = L.restate(evalfn, x0, lo, hi, maxiter, order='sequential')
    assert rc == 0 and ne == calls
    assert ne == ref['evaluations'], (ne, ref['evaluations'])
    if np.array_equal(L.bits(x), L.bits(ref['x'])) and np.array_equal(L.bits(f), L.bits(ref['f'])):
        return ref
    # only a build that fuses the host's multiply-adds may come here
    _, _, dx, df = L.order_difference(evalfn, x0, lo, hi, maxiter)
    print('lc_batched_lbfgs is not bit-equal to its restatement: this build contracts the host arithmetic; worst |dx|',
          np.abs(x - ref['x']).max(), 'against the restatement\'s own order difference', dx.max())
    assert np.all(np.abs(x - ref['x']) <= L.REASSOCIATION_MARGIN * dx)            # per variable
    assert np.all(np.abs(f - ref['f']) <= L.REASSOCIATION_MARGIN * df)
    return ref


@pytest.fixture(scope='module')
def rosen():
    """The restatement at maxiter 300 of every Rosenbrock size, computed once."""
    out = {}
    for D in L.ROSEN_DIMS:
        x0, lo, hi = L.rosenbrock_problems(D)
        out[D] = (x0, lo, hi, L.restate(L.batch_eval(L.rosenbrock), x0, lo, hi, 300))
    return out


@pytest.mark.parametrize('maxiter', L.ROSEN_MAXITER)
@pytest.mark.parametrize('D', L.ROSEN_DIMS)
def test_rosenbrock_bits(D, maxiter, rosen):
    x0, lo, hi, full = rosen[D]
    ref = compare(L.batch_eval(L.rosenbrock), x0, lo, hi, maxiter)
    assert np.all(ref['iters'] <= maxiter)
    assert np.all(ref['x'] >= lo) and np.all(ref['x'] <= hi)
    # the iterates of a shorter run are the first iterates of the long one
    for b in range(4):
        for k, it in enumerate(ref['iterates'][b]):
            assert np.array_equal(L.bits(it), L.bits(full['iterates'][b][k]))
    if maxiter == 0:
        assert ref['evaluations'] == 1 and np.array_equal(ref['x'], np.clip(x0, lo, hi))
    if maxiter == 13 and D > 2:
        assert max(ref['dropped']) > 0, 'no problem stored more than 10 pairs: the wrap of the memory was not reached'
    if maxiter == 300:
        assert all(s in ('ftol', 'gtol') for s in ref['stop']), ref['stop']
        assert ref['x'][0, 0] == 0.5 and ref['x'][1, D - 1] == 1.5          # the bounds that end active
        assert np.all(np.abs(ref['x'][2] - 1.0) < 1e-4)                      # the free problem is at the optimum
        assert np.array_equal(ref['iterates'][3][0], np.clip(x0[3], -2.0, 2.0)) and not np.array_equal(x0[3], ref['iterates'][3][0])


def test_pair_that_fails_the_curvature_guard():
    x0, lo, hi = L.double_well_problem()
    ref = compare(L.batch_eval(L.double_well), x0, lo, hi, 60)
    assert ref['rejected'][0] > 0, 'the trajectory stored no pair with s . y <= 0'
    assert ref['stop'][0] in ('ftol', 'gtol')


def test_failed_line_search_keeps_the_last_accepted_point():
    x0, lo, hi = L.lying_problem()
    ev = L.batch_eval(L.lying_bowl)
    ref = compare(ev, x0, lo, hi, 60)
    assert ref['ls_failed'][0] and ref['iters'][0] >= 1
    assert np.array_equal(ref['x'][0], ref['iterates'][0][-1])
    # (the library's x was compared with ref['x'] on raw bits; its loss is that of the point it kept)
    rc, x, f, ne, _ = host_lbfgs(ev, x0, lo, hi, 60)
    assert f[0] == L.lying_bowl(x[0])[0] and f[0] <= 1.0


def test_infinite_start_beside_healthy_problems():
    D = 7
    x0, lo, hi = L.rosenbrock_problems(D)
    lo[3], hi[3] = -np.inf, np.inf                       # unbounded, so that "untouched" means the caller's own bits
    x0[3, 0] = 11.0
    fns = [L.rosenbrock] * 3 + [L.walled(L.rosenbrock)]
    ref = compare(L.batch_eval(fns), x0, lo, hi, 300)
    rc, x, f, ne, _ = host_lbfgs(L.batch_eval(fns), x0, lo, hi, 300)
    assert np.array_equal(L.bits(x[3]), L.bits(x0[3])) and np.isinf(f[3]) and ref['iters'][3] == 0
    # the other three are what they are without the sick one
    alone = L.restate(L.batch_eval(L.rosenbrock), x0[:3], lo[:3], hi[:3], 300)
    assert np.array_equal(L.bits(x[:3]), L.bits(alone['x'])) and np.array_equal(L.bits(f[:3]), L.bits(alone['f']))


@pytest.mark.parametrize('maxiter', (13, 300))
def test_bits_do_not_depend_on_the_company(maxiter):
    D = 7
    x0, lo, hi = L.rosenbrock_problems(D)
    ev = L.batch_eval(L.rosenbrock)
    rc, x4, f4, ne4, _ = host_lbfgs(ev, x0, lo, hi, maxiter)
    assert rc == 0
    worst = 0
    for b in range(4):
        rc, x1, f1, ne1, _ = host_lbfgs(ev, x0[b:b + 1], lo[b:b + 1], hi[b:b + 1], maxiter)
        assert rc == 0
        assert np.array_equal(L.bits(x1[0]), L.bits(x4[b])) and np.array_equal(L.bits(f1), L.bits(f4[b:b + 1]))
        worst = max(worst, ne1)
    assert ne4 == worst                                  # lock step: the batch costs what its slowest problem costs


def test_callback_code_and_refused_arguments():
    from lightcurver_amd import _lib
    lib = _lib.lib()
    x0, lo, hi = L.rosenbrock_problems(7)
    x0 = np.clip(x0, lo, hi)
    ev = L.batch_eval(L.rosenbrock)
    for at in (1, 2, 5):                                 # at the start, at the first trial, in the middle
        rc, x, f, ne, calls = host_lbfgs(ev, x0, lo, hi, 300, code=(at, 37 + at))
        assert rc == 37 + at and calls == at
        assert np.array_equal(L.bits(x), L.bits(x0)) and np.all(f == -7.0) and ne == -1
    dp = _lib.dp
    x = np.ascontiguousarray(x0)
    cb = _lib.LBFGS_EVAL(lambda *a: 0)
    px, pl, ph = x.ctypes.data_as(dp), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp)
    null, nocb = C.cast(None, dp), C.cast(None, _lib.LBFGS_EVAL)
    for args in ((0, 7, px, pl, ph, 5, cb), (4, 0, px, pl, ph, 5, cb), (-1, 7, px, pl, ph, 5, cb), (4, 7, null, pl, ph, 5, cb),
                 (4, 7, px, null, ph, 5, cb), (4, 7, px, pl, null, 5, cb), (4, 7, px, pl, ph, -1, cb),
                 (4, 7, px, pl, ph, 5, nocb)):
        assert lib.lc_batched_lbfgs(*args, None, None, None) == -1, args[:2] + args[5:6]
    assert np.array_equal(x, x0)
    # the outputs are optional
    assert lib.lc_batched_lbfgs(4, 7, px, pl, ph, 0, _lib.LBFGS_EVAL(lambda u, X, F, G: 0), None, None, None) == 0


def test_restatement_reaches_the_scipy_optimum():
    """Independence: the restatement shares no code with scipy's L-BFGS-B, and on bounded problems both end at one optimum."""
    from scipy.optimize import minimize
    x0, lo, hi = L.rosenbrock_problems(7)
    ref = L.restate(L.batch_eval(L.rosenbrock), x0, lo, hi, 300)
    for b in (0, 1):
        res = minimize(L.rosenbrock, np.clip(x0[b], lo[b], hi[b]), jac=True, method='L-BFGS-B', bounds=list(zip(lo[b], hi[b])),
                       options=dict(maxiter=1000, ftol=1e-15, gtol=1e-10))
        print('problem', b, 'restatement', ref['f'][b], 'scipy', res.fun, 'difference', ref['f'][b] - res.fun)
        assert abs(ref['f'][b] - res.fun) <= L.SCIPY_F_TOL
        assert ref['f'][b] > 0.01                        # a bound is active: the optimum is not the free one


def test_the_two_orders_and_types_of_the_restatement():
    """The switches change what they say and nothing else: the butterfly is a sum (equal to the sequential one where every
    partial sum is exact), and a float32 run follows the float64 one to float32 accuracy over its first steps."""
    v = np.arange(1.0, 53.0)
    assert L.sum_butterfly(v) == L.sum_sequential(v) == 52 * 53 / 2
    w = np.arange(1.0, 1050.0, dtype=np.float32)
    assert L.sum_butterfly(w) == L.sum_sequential(w) == 1049 * 1050 / 2
    rng = np.random.default_rng(5)
    r = rng.standard_normal(52)
    assert abs(L.sum_butterfly(r) - L.sum_sequential(r)) <= 52 * 2.0 ** -53 * np.abs(r).sum()
    x0, lo, hi = L.rosenbrock_problems(7)
    ev = L.batch_eval(L.rosenbrock)
    a, b, dx, df = L.order_difference(ev, x0, lo, hi, 5)
    assert np.array_equal(a['iters'], b['iters']) and dx.max() < 1e-12
    c = L.restate(ev, x0, lo, hi, 3, dtype=np.float32)
    d = L.restate(ev, x0, lo, hi, 3)
    assert c['x'].dtype == np.float32 and np.array_equal(c['iters'], d['iters'])
    assert np.abs(c['x'] - d['x']).max() < 1e-3


@pytest.mark.parametrize('config', ('bounded', 'full', 'spare'))
def test_joint_problems_and_step_checker_on_the_oracle(config):
    """The problems of the joint form's GPU test, on the oracle's float64 loss: the float32 restatement with the joint
    driver's stops runs the full ladder, fills its memory, meets its bounds, and takes no Armijo decision as close to the
    threshold as the GPU test leaves out.  The one-step-ahead checker of the GPU test passes on the trace of that run."""
    su = L.joint_setup(config)
    assert len(su['x0']) == (1049 if config == 'full' else 20)
    K = L.JOINT_K[config]
    t, r = L.trace_of_restatement(L.joint_oracle_eval(su), su['x0'], su['lo'], su['hi'], K, su['blocks'])
    out = L.check_steps(t)
    print(config, out, 'trials', r['trials'][0])
    assert out['steps'] == K and out['steps'] > L.MEM and r['dropped'][0] > 0
    assert out['left_out'] == 0 and out['decisions'] >= K
    assert out['left_out'] <= L.ARMIJO_LEFT_OUT_MAX * out['decisions']
    if config == 'spare':      # the case the ring's spare slot is for
        assert r['rejected_full'][0] >= 1 and out['lost_pairs'] == r['rejected_full'][0] and out['power'] > 100
    assert out['worst'] <= 1.0
    if config == 'bounded':
        assert out['held'] > 0
        sl = su['blocks']['a']
        assert (t.x[K][sl] == su['hi'][sl]).sum() >= 8                                   # the cap on the fluxes ends active


def test_joint_problem_that_ends_on_ftol_on_the_oracle():
    """The configuration whose stops the GPU test checks: on the oracle's loss the float32 restatement ends on ftol before
    maxiter, and the stop checker passes on its trace and names that reason."""
    su = L.joint_setup('stops')
    K = L.JOINT_K['stops']
    t, r = L.trace_of_restatement(L.joint_oracle_eval(su), su['x0'], su['lo'], su['hi'], K, su['blocks'])
    assert r['stop'][0] == 'ftol' and L.MEM - 2 <= t.last < K
    assert L.check_stops(t) == 'ftol'
    # the checker sees a fit that runs on past its ftol stop: the same trace, said to have been left at an earlier maxiter
    longer, _ = L.trace_of_restatement(L.joint_oracle_eval(su), su['x0'], su['lo'], su['hi'], K, su['blocks'])
    longer.f = list(longer.f)
    longer.f[t.last - 2] = longer.f[t.last - 3]
    with pytest.raises(AssertionError):
        L.check_stops(longer)


def test_host_program_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found (CXX, c++, g++, clang++): the host program cannot be built')
    exe = str(tmp_path / 'lbfgs_main')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'lightcurver_amd', 'csrc'),
                            os.path.join(HOST, 'lbfgs_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'all checks passed' in run.stdout
