"""``FisherCovariance`` for the use the reference makes of it - the 1-sigma of the fluxes with everything else fixed
(lightcurver/utilities/starred_utilities.py:36-38, ``diagonal_only=True``) - and its full form with only the fluxes free
(``diagonal_only=False``): the Fisher information of the fluxes is block diagonal over the epochs, each block M x M, and
the marginal 1-sigma comes from its inverse.

With the source positions (and optionally the epochs' means) free as well the information is an arrowhead - per-epoch local
blocks (a_e, mean_e), one shared block (c_x, c_y) and the couplings - whose inverse comes from the Schur complement of the
shared block: ``arrowhead_covariance`` is the float64 restatement of what the device computes
(``JointFit.fisher_positions``), ``dense_from_arrowhead`` assembles dense matrices from the blocks.  Everything else (dx,
dy, alpha, h) stays fixed: the result is conditional on the registration and the background.

With the epochs' translations free too (``JointFit.fisher_shifts``) the local block grows by dx_e, dy_e - a_e, mean_e, dx_e,
dy_e - and the same two functions take it with ``shifts=True``; the positions are then free only under a prior (a common
translation of the sources is a gauge of the shifts)."""
import numpy as np

from ..deconvolution.deconvolution import nest_kwargs

PIVOT = 1e-6          # a Cholesky pivot not above PIVOT times its diagonal entry: the block is numerically singular
DENSE_LIMIT = 4096    # parameters beyond which dense_from_arrowhead refuses

FREE_SETS = (['a'], ['a', 'mean'], ['a', 'c_x', 'c_y'], ['a', 'c_x', 'c_y', 'mean'])
# ... and with the translations of the epochs free (both), in the order of the parameter class
SHIFT_SETS = (['a', 'dx', 'dy'], ['a', 'dx', 'dy', 'mean'], ['a', 'c_x', 'c_y', 'dx', 'dy'],
              ['a', 'c_x', 'c_y', 'dx', 'dy', 'mean'])


def block_diagonal(blocks):
    """Dense (E * M, E * M) array with the (E, M, M) ``blocks`` on its diagonal, in the epoch-major order of ``a``."""
    blocks = np.asarray(blocks)
    E, M, _ = blocks.shape
    out = np.zeros((E * M, E * M), blocks.dtype)
    for e in range(E):
        out[e * M:(e + 1) * M, e * M:(e + 1) * M] = blocks[e]
    return out


def _cholesky_inverse(S):
    """Inverse of the symmetric S by its Cholesky factor, or None when a pivot is not above PIVOT times its diagonal entry."""
    m = S.shape[0]
    L = np.zeros((m, m))
    for r in range(m):
        for c in range(r + 1):
            s = S[r, c] - L[r, :c] @ L[c, :c]
            if r == c:
                if not s > PIVOT * S[r, r]:
                    return None
                L[r, r] = np.sqrt(s)
            else:
                L[r, c] = s / L[c, c]
    Li = np.linalg.solve(L, np.eye(m)) if m else L
    return Li.T @ Li


def arrowhead_covariance(F_local, F_cross, F_shared, shifts=False):
    """Inverse of the arrowhead information in float64: ``F_local`` (E, Lp, Lp), ``F_cross`` (E, Lp, S), ``F_shared`` (S, S)
    (S may be 0) -> dict C_local, C_cross, C_shared of the same shapes, sigma_local (E, Lp), sigma_shared (S,), B (E, Lp, S).
      B_e = F_loc,e^-1 F_x,e;  S = F_cc - sum_e F_x,e^T B_e (epoch order);  C_cc = S^-1;  C_x,e = -B_e C_cc;
      C_loc,e = F_loc,e^-1 + B_e C_cc B_e^T;  cov(loc_e, loc_f) = B_e C_cc B_f^T for e != f (dense_from_arrowhead).
    A parameter whose diagonal entry is zero is left out (sigma = +inf, zero rows and columns of C); a Cholesky pivot of a
    local block or of S that is not above 1e-6 times its diagonal entry makes every C and sigma NaN.  ``shifts``: the local
    block ends with dx_e, dy_e (the solve is the same; Lp must then be at least 2)."""
    if shifts and np.shape(F_local)[1] < 2:
        raise ValueError('local blocks with the shifts hold dx_e, dy_e at least')
    Fl = np.asarray(F_local, np.float64)
    E, Lp, _ = Fl.shape
    Fs = np.zeros((0, 0)) if F_shared is None else np.asarray(F_shared, np.float64)
    S = Fs.shape[0]
    Fx = np.zeros((E, Lp, S)) if F_cross is None or S == 0 else np.asarray(F_cross, np.float64).reshape(E, Lp, S)
    Inv, B = np.zeros((E, Lp, Lp)), np.zeros((E, Lp, S))
    out_local = np.zeros((E, Lp), bool)
    ok = True
    G = np.zeros((S, S))
    for e in range(E):
        keep = np.flatnonzero(np.diag(Fl[e]) > 0)
        out_local[e] = ~np.isin(np.arange(Lp), keep)
        inv = _cholesky_inverse(Fl[e][np.ix_(keep, keep)])
        if inv is None:
            ok = False
            continue
        Inv[e][np.ix_(keep, keep)] = inv
        B[e][keep] = inv @ Fx[e][keep]
        G += Fx[e][keep].T @ B[e][keep]
    keep_s = np.flatnonzero(np.diag(Fs) > 0)
    Ccc = np.zeros((S, S))
    if ok:
        inv = _cholesky_inverse((Fs - G)[np.ix_(keep_s, keep_s)])
        if inv is None:
            ok = False
        else:
            Ccc[np.ix_(keep_s, keep_s)] = inv
    res = {'B': B}
    if not ok:
        res.update(C_local=np.full((E, Lp, Lp), np.nan), C_cross=np.full((E, Lp, S), np.nan),
                   C_shared=np.full((S, S), np.nan), sigma_local=np.full((E, Lp), np.nan), sigma_shared=np.full(S, np.nan))
        return res
    Cx = -B @ Ccc
    Cl = Inv - Cx @ np.swapaxes(B, 1, 2)
    sl = np.sqrt(np.maximum(np.einsum('eii->ei', Cl), 0.0))
    sl[out_local] = np.inf
    ss = np.sqrt(np.maximum(np.diag(Ccc), 0.0))
    ss[~np.isin(np.arange(S), keep_s)] = np.inf
    res.update(C_local=Cl, C_cross=Cx, C_shared=Ccc, sigma_local=sl, sigma_shared=ss)
    return res


def dense_from_arrowhead(local, cross, shared, M, covariance=False, shifts=False):
    """Dense matrix of the arrowhead blocks in the order a (E * M, epoch-major), c_x, c_y, mean (E) - the order of
    ``set_free`` - then, with ``shifts`` (local blocks a_e, mean_e, dx_e, dy_e), dx (E), dy (E).
    ``covariance=False``: the blocks are those of the information (different epochs do not couple);
    ``covariance=True``: those of its inverse, and the local parameters of two epochs e != f get
    C_x,e C_cc^-1 C_x,f^T (= B_e C_cc B_f^T).  ValueError above 4096 parameters."""
    local = np.asarray(local, np.float64)
    E, Lp, _ = local.shape
    shared = np.zeros((0, 0)) if shared is None else np.asarray(shared, np.float64)
    S = shared.shape[0]
    cross = np.zeros((E, Lp, S)) if cross is None or S == 0 else np.asarray(cross, np.float64).reshape(E, Lp, S)
    nsh = 2 if shifts else 0
    if Lp - nsh not in (M, M + 1):
        raise ValueError(f'local blocks of {Lp} parameters for {M} sources')
    P = E * Lp + S
    if P > DENSE_LIMIT:
        raise ValueError(f'{P} parameters: a dense matrix is built up to {DENSE_LIMIT}')
    # position of local parameter (e, k) and of the shared ones in the dense order
    pos = np.empty((E, Lp), int)
    pos[:, :M] = np.arange(E * M).reshape(E, M)
    has_mean = Lp - nsh > M
    if has_mean:
        pos[:, M] = E * M + S + np.arange(E)
    if shifts:
        first = E * M + S + (E if has_mean else 0)
        pos[:, Lp - 2] = first + np.arange(E)
        pos[:, Lp - 1] = first + E + np.arange(E)
    sh = E * M + np.arange(S)
    D = np.zeros((P, P))
    D[np.ix_(sh, sh)] = shared
    for e in range(E):
        D[np.ix_(pos[e], pos[e])] = local[e]
        D[np.ix_(pos[e], sh)] = cross[e]
        D[np.ix_(sh, pos[e])] = cross[e].T
    if covariance and np.isnan(shared).any():
        D[:] = np.nan
    elif covariance and S and E > 1:
        keep = np.flatnonzero(np.diag(shared) > 0)
        Si = np.zeros((S, S))
        if keep.size:
            Si[np.ix_(keep, keep)] = np.linalg.inv(shared[np.ix_(keep, keep)])
        for e in range(E):
            left = cross[e] @ Si
            for f in range(E):
                if f != e:
                    D[np.ix_(pos[e], pos[f])] = left @ cross[f].T
    return D


class FisherCovariance:
    """``free`` of the parameter class: ['a'] (the reference's use), ['a', 'mean'], ['a', 'c_x', 'c_y'] or
    ['a', 'c_x', 'c_y', 'mean'].  Beyond ['a'] the information comes from ``JointFit.fisher_positions`` (with the Gaussian
    prior on c_x, c_y of the loss, if it has one), conditional on dx, dy, alpha and h.  Each of the four also with 'dx',
    'dy' (both): ``JointFit.fisher_shifts``, conditional on alpha and h only; 'c_x', 'c_y' beside the shifts need the
    prior (the library refuses them without)."""

    def __init__(self, param_class, optimizer_class, diagonal_only=True):
        free = list(param_class.free)
        if free not in [list(f) for f in FREE_SETS + SHIFT_SETS]:
            raise NotImplementedError("Fisher information is built for the fluxes 'a', optionally with the positions "
                                      "'c_x', 'c_y' (both), 'mean' and / or the shifts 'dx', 'dy' (both) free")
        self._free = free
        self._shifts = 'dx' in free
        self._positions = 'c_x' in free
        self._mean = 'mean' in free
        self._param = param_class
        self._optim = optimizer_class
        self.diagonal_only = bool(diagonal_only)
        self._sigma = None
        self._F = self._C = None
        self._arrow = None

    @property
    def _flux_only(self):
        return self._free == ['a']

    def compute_fisher_information(self):
        fit = self._optim._loss.configure()
        fit.set_params(**self._param._current)
        if self._flux_only:
            if self.diagonal_only:
                self._sigma = fit.fisher_flux_sigma()
            else:
                self._F, self._C, self._sigma = fit.fisher_flux_covariance()
            return
        call = fit.fisher_shifts if self._shifts else fit.fisher_positions
        self._arrow = call(positions=self._positions, mean=self._mean)
        self._M = self._arrow['F_local'].shape[1] - (1 if self._mean else 0) - (2 if self._shifts else 0)

    def _sigmas(self):
        """name -> 1-sigma of the free blocks beyond ['a']."""
        A, M = self._arrow, self._M
        if self.diagonal_only:
            with np.errstate(divide='ignore'):
                loc = 1.0 / np.sqrt(np.einsum('eii->ei', A['F_local'].astype(np.float64)))
                sh = 1.0 / np.sqrt(np.diag(A['F_shared'].astype(np.float64)))
            out = {'a': loc[:, :M].reshape(-1)}
            if self._mean:
                out['mean'] = loc[:, M]
            if self._shifts:
                out['dx'], out['dy'] = loc[:, -2], loc[:, -1]
        else:
            out = {'a': A['sigma_a'], 'mean': A['sigma_mean']}
            if self._shifts:
                out['dx'], out['dy'] = A['sigma_dx'], A['sigma_dy']
            sh = A['sigma_c']
        if self._positions:
            out['c_x'], out['c_y'] = sh[:M], sh[M:]
        return out

    def get_kwargs_sigma(self):
        """1-sigma of every free parameter in the nested kwargs shape: with ``diagonal_only=False`` the marginal errors
        sqrt(diag C), with ``diagonal_only=True`` 1 / sqrt(diag F)."""
        flat = {k: np.zeros_like(v) for k, v in self._param._current.items()}
        if self._flux_only:
            if self._sigma is None:
                self.compute_fisher_information()
            flat['a'] = self._sigma
            return nest_kwargs(flat)
        if self._arrow is None:
            self.compute_fisher_information()
        sig = self._sigmas()
        for k in self._free:
            flat[k] = np.asarray(sig[k], dtype=flat[k].dtype).reshape(flat[k].shape)
        return nest_kwargs(flat)

    def _blocks(self):
        if self.diagonal_only:
            raise NotImplementedError('the full Fisher matrix needs diagonal_only=False')
        if self._flux_only:
            if self._F is None:
                self.compute_fisher_information()
            return self._F, self._C
        if self._arrow is None:
            self.compute_fisher_information()
        return self._arrow['F_local'], self._arrow['C_local']

    @property
    def flux_covariance_blocks(self):
        """(E, M, M): the covariance of the fluxes of every epoch, marginal over whatever else is free (with the positions
        free the fluxes of different epochs are correlated as well: ``covariance_matrix``)."""
        C = self._blocks()[1]
        return C if self._flux_only else np.ascontiguousarray(C[:, :self._M, :self._M])

    @property
    def position_covariance(self):
        """(2M, 2M): the marginal covariance of (c_x, c_y)."""
        if not self._positions:
            raise NotImplementedError("the positions are not free")
        self._blocks()
        return self._arrow['C_shared']

    def _dense(self, covariance):
        A = self._arrow
        k = 'C' if covariance else 'F'
        return dense_from_arrowhead(A[k + '_local'], A[k + '_cross'] if self._positions else None,
                                    A[k + '_shared'] if self._positions else None, self._M, covariance=covariance,
                                    shifts=self._shifts)

    @property
    def fisher_matrix(self):
        """Dense Fisher information in the order a, c_x, c_y, mean, dx, dy of the free blocks ((E * M, E * M), block diagonal over the
        epochs, with only the fluxes free)."""
        F = self._blocks()[0]
        return block_diagonal(F) if self._flux_only else self._dense(False)

    @property
    def covariance_matrix(self):
        """Dense covariance, the inverse of ``fisher_matrix``, in the same order."""
        C = self._blocks()[1]
        return block_diagonal(C) if self._flux_only else self._dense(True)
