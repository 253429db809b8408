"""The float64 restatement of the field-distortion kernels (tests/_distortion.py) pinned against oracle/model.py and torch
autograd on the matrix set the device is tried at (tests/test_distortion_limits_gpu.py), and the host chain rule
``quadratic_forms`` against autograd of ``moffat_distorted`` for all 13 parameters (until now reached only through a 2e-4
finite-difference check on the device).  Everything here is float64 against float64: 1e-12 relative."""
import numpy as np
import pytest
import torch

from oracle import model as om
from tests import _distortion as D

N_GRID = (16, 33, 48)
TOL = 1e-12


def _A(a00, a01, a11):
    return om.T([[a00, a01], [a01, a11]])


def _star_matrices():
    """(case name, star, a00, a01, a11) of every star of every case."""
    out = []
    for name, coef, xy in D.CASES:
        a00, a01, a11, det = D.matrices(coef[None], xy[None])
        out += [(name, s, a00[0, s], a01[0, s], a11[0, s]) for s in range(D.STARS)]
    return out


def test_matrix_set_is_inside_the_supported_range():
    names = [c[0] for c in D.CASES]
    assert len(set(names)) == len(names) == 1 + 6 + 2 + 1 + 2 + 12 + 1
    assert sorted(n for n in names if n.startswith('corner')) == sorted(
        ['corner0.5,1.5,-0.5', 'corner0.5,1.5,+0.5', 'corner1.5,0.5,-0.5', 'corner1.5,0.5,+0.5', 'corner1.5,1.5,-0.5',
         'corner1.5,1.5,+0.5'])
    for name, coef, xy in D.CASES:
        assert np.abs(coef).max() <= 0.25 and np.abs(xy).max() <= 0.5, name
        assert np.array_equal(coef, np.float32(coef)) and np.array_equal(xy, np.float32(xy)), name
        for dtype in (np.float64, np.float32):
            a00, a01, a11, det = D.matrices(dtype(coef[None]), dtype(xy[None]), dtype)
            assert max(np.abs(a00 - 1).max(), np.abs(a11 - 1).max(), np.abs(a01).max()) <= 0.5, name
            assert det.min() > D.DET_MIN, name
        assert len({(a, b, c) for a, b, c in zip(a00[0], a01[0], a11[0])}) == (1 if name == 'identity' else D.STARS), name
    first = {name: tuple(float(v[0, 0]) for v in D.matrices(coef[None], xy[None])[:3]) for name, coef, xy in D.CASES}
    assert first['corner1.5,0.5,-0.5'] == (1.5, -0.5, 0.5) and first['shear+0.5'] == (1.0, 0.5, 1.0)
    assert first['hv2hu1'] == (1.5, 0.25, 0.75) and first['hv1hu2'] == (0.75, 0.25, 1.5)
    assert np.allclose(first['near-singular'], (0.55, 0.5, 0.55), atol=1e-7)
    # the window of the adjoint kernel, as it computes it: the two cases that tell hv from hu
    hw = lambda a, b: min(int(np.floor(np.float32(abs(a)) + np.float32(abs(b)) + np.float32(0.501))), 2)
    assert (hw(1.5, 0.25), hw(0.25, 0.75)) == (2, 1)


@pytest.mark.parametrize('N', N_GRID)
def test_warp_and_adjoint_equal_oracle_and_autograd(N):
    rng = np.random.default_rng(N)
    B = D.noise_grid(rng, N).astype(np.float64)
    g = rng.standard_normal((N, N))
    worst = 0.0
    for name, s, a00, a01, a11 in _star_matrices():
        if s >= 3 and N != 16:          # every star at the smallest grid, the first three of every case at the others
            continue
        op = D.warp_operator(N, a00, a01, a11)
        Bt = om.T(B).requires_grad_(True)
        ref = om.warp_grid(Bt, _A(a00, a01, a11))
        (gref,) = torch.autograd.grad((ref * om.T(g)).sum(), Bt)
        w, a = op.warp(B), op.adjoint(g)
        assert np.abs(w - ref.detach().numpy()).max() <= TOL * np.abs(ref.detach().numpy()).max(), (name, s)
        assert np.abs(a - gref.numpy()).max() <= TOL * np.abs(gref.numpy()).max(), (name, s)
        # <W b, g> = <b, W^T g>
        lhs, rhs = (w * g).sum(), (B * a).sum()
        worst = max(worst, abs(lhs - rhs) / np.abs(w * g).sum())
    assert worst < 1e-13


def test_dense_operator_and_frame_adjoint():
    N = 12
    rng = np.random.default_rng(5)
    name, coef, xy = D.CASES[-1]
    a00, a01, a11, _ = D.matrices(coef[None], xy[None])
    ops = [D.warp_operator(N, a00[0, s], a01[0, s], a11[0, s]) for s in range(4)]
    B, g = rng.standard_normal((N, N)), rng.standard_normal((4, N, N))
    M = [op.dense() for op in ops]
    assert np.abs(M[0] @ B.ravel() - ops[0].warp(B).ravel()).max() < 1e-13
    total = sum(m.T @ gs.ravel() for m, gs in zip(M, g))
    assert np.abs(total - D.adjoint(ops, g).ravel()).max() < 1e-13
    assert np.abs(ops[0].warp_abs(B).ravel() - np.abs(M[0]) @ np.abs(B.ravel())).max() < 1e-13
    assert np.abs(ops[0].adjoint_abs(g[0]).ravel() - np.abs(M[0]).T @ np.abs(g[0].ravel())).max() < 1e-13


def test_position_rounding_is_the_same_operator_up_to_float32_positions():
    """Exactly the float64 operator where the float32 positions are exact (the corners: A^-1 has entries 0.5, 1, 3), a
    float32-sized perturbation of it elsewhere."""
    N = 33
    rng = np.random.default_rng(6)
    B = D.noise_grid(rng, N).astype(np.float64)
    for name, coef, xy in D.CASES:
        a = D.matrices(coef[None], xy[None])
        a32 = D.matrices(np.float32(coef[None]), np.float32(xy[None]), np.float32)
        for flux in (True, False):
            ref = D.warp_operator(N, a[0][0, 0], a[1][0, 0], a[2][0, 0], flux=flux).warp(B)
            for divide in (False, True):
                got = D.position_rounding(N, a32[0][0, 0], a32[1][0, 0], a32[2][0, 0], flux=flux, divide=divide).warp(B)
                if name == 'identity' or name.startswith('corner'):
                    assert np.array_equal(got, ref), name
                else:
                    assert 0 < np.abs(got - ref).max() < 1e-3 * np.abs(ref).max(), name


def test_apply_distortion_restated():
    N = 31
    rng = np.random.default_rng(7)
    psf = np.abs(D.noise_grid(rng, N)).astype(np.float64)
    for name, coef, xy in D.CASES:
        a00, a01, a11, _ = D.matrices(coef[None], xy[None])
        for s in (0, 5):
            w = D.warp_operator(N, a00[0, s], a01[0, s], a11[0, s], flux=False).warp(psf)
            ref = om.apply_distortion(psf, coef, xy[s, 0], xy[s, 1]).numpy()
            assert np.abs(w / w.sum() - ref).max() <= TOL * ref.max(), (name, s)


# ---- Moffat by its quadratic form and the chain rule of the facade --------------------------------------------------------------
def _thetas(n, ss):
    """Nearly round (fwhm_x = fwhm_y) and strongly elongated Moffats, the FWHM at the facade's bounds included."""
    lo, hi = 0.5 / ss, n / 2.0
    out = []
    for fx, fy in ((3.0, 3.0), (lo, lo), (hi, hi), (3.0, 3.0 * (1 + 1e-9)), (lo, 4 * lo), (hi, hi / 4), (1.5, 6.0)):
        for phi in (0.5, -0.5):
            for beta in (1.1, 2.5, 50.0):
                out.append((fx, fy, phi, beta))
    return out


def _complex_step_jacobian(theta, xy, ss):
    """d q / d theta [13][4] of quadratic_forms, exact to rounding (the function is analytic in every parameter)."""
    from lightcurver_amd.starred.procedures.psf_routines import quadratic_forms
    J = np.zeros((13, 4))
    for k in range(13):
        t = theta.astype(np.complex128).reshape(1, 13)
        t[0, k] += 1e-30j
        J[k] = quadratic_forms(t, xy.reshape(1, 1, 2).astype(np.complex128), ss)[0, 0].imag / 1e-30
    return J


@pytest.mark.parametrize('n,ss', [(16, 1), (16, 2)])
def test_quadratic_forms_raster_and_chain_rule_equal_autograd(n, ss):
    from lightcurver_amd.starred.procedures.psf_routines import quadratic_forms
    N = n * ss
    rng = np.random.default_rng(n + ss)
    gT = rng.standard_normal((N, N))
    picks = [D.CASES[i] for i in (0, 1, 6, 9, 13, len(D.CASES) - 1)]
    for i, (fx, fy, phi, beta) in enumerate(_thetas(n, ss)):
        name, coef, xy = picks[i % len(picks)]
        s = i % D.STARS
        theta = np.concatenate([[fx, fy, phi, beta], coef])
        q = quadratic_forms(theta[None], xy[None, s:s + 1], ss)[0, 0]
        p = {k: om.T(v).requires_grad_(True) for k, v in zip(('fwhm_x', 'fwhm_y', 'phi', 'beta'), (fx, fy, phi, beta))}
        dist = om.T(coef).requires_grad_(True)
        A = om.distortion_matrix(dist, om.T(xy[s, 0]), om.T(xy[s, 1]))
        ref = om.moffat_distorted(N, ss, p['fwhm_x'], p['fwhm_y'], p['phi'], p['beta'], A)
        M = D.moffat_q(N, q)
        assert np.abs(M - ref.detach().numpy()).max() <= TOL * ref.detach().numpy().max(), (name, fx, fy, phi, beta)
        grads = torch.autograd.grad((ref * om.T(gT)).sum(), [p['fwhm_x'], p['fwhm_y'], p['phi'], p['beta'], dist])
        gref = np.concatenate([np.atleast_1d(g.numpy()) for g in grads])
        # d / dq against autograd through q alone ...
        gq, scale = D.moffat_q_grad(N, q, gT, scale=True)
        Jq = _complex_step_jacobian(theta, xy[s], ss)
        got = Jq @ gq
        # ... and the 13 parameters through the chain rule.  A component is a sum over q that cancels (d / d phi of a round
        # Moffat is zero, and autograd returns its own rounding of the other gradients there): the error is relative to the
        # terms of that sum
        size = np.abs(Jq) @ scale
        assert np.all(np.abs(got - gref) <= 1e-10 * size + TOL * np.abs(gref) + 1e-14 * np.abs(gref).max()), \
            (name, fx, fy, phi, beta, got, gref)
        assert np.abs(gref).max() > 0


def test_moffat_q_grad_equals_autograd():
    N = 33
    rng = np.random.default_rng(9)
    gT = rng.standard_normal((N, N))
    idx = torch.arange(N, dtype=om.DT) - (N - 1) // 2
    x, y = idx[None, :], idx[:, None]
    for q in ([0.1, 0.0, 0.1, 2.5], [0.4, 0.15, 0.1, 1.1], [0.02, -0.03, 0.3, 50.0], [16.0, 0.0, 16.0, 50.0],
              [1e-3, 2e-4, 4e-3, 1.1]):
        qt = om.T(q).requires_grad_(True)
        m = (1.0 + qt[0] * x * x + 2.0 * qt[1] * x * y + qt[2] * y * y) ** (-qt[3])
        m = m / m.sum()
        (gref,) = torch.autograd.grad((m * om.T(gT)).sum(), qt)
        assert np.abs(D.moffat_q(N, q) - m.detach().numpy()).max() <= TOL * float(m.detach().max())
        got, scale = D.moffat_q_grad(N, q, gT, scale=True)
        assert np.all(np.abs(got - gref.numpy()) <= TOL * scale), q
