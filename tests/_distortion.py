"""Checker for the field-distortion kernels (csrc/psf_distort.h, csrc/distort.hip): a float64 NumPy restatement of the
resampling of DESIGN.md §3 as an explicit sparse operator, of the Moffat given by its quadratic form and its gradient, and
the set of matrices the device is tried at.

Not part of the product path.  ``tests/test_distortion_cpu.py`` pins every function here against ``oracle/model.py`` and
torch autograd; ``tests/test_distortion_limits_gpu.py`` compares the device with them."""
import numpy as np

EPS32 = 2.0 ** -24          # half an ulp of float32: the relative error of one rounding


def matrices(coef, xy, dtype=np.float64):
    """coef [F][9] (dilation_x, dilation_y, shear; c0, c1, c2 each), xy [F][S][2] -> a00, a01, a11, det, each [F][S].
    Every operation is one rounding of ``dtype``, in the order the device evaluates ``1 + c0 + c1 x + c2 y``."""
    c = np.asarray(coef, dtype).reshape(-1, 9)[:, None, :]
    p = np.asarray(xy, dtype).reshape(c.shape[0], -1, 2)
    x, y = p[..., 0], p[..., 1]
    one = dtype(1.0)
    a00 = one + c[..., 0] + c[..., 1] * x + c[..., 2] * y
    a11 = one + c[..., 3] + c[..., 4] * x + c[..., 5] * y
    a01 = c[..., 6] + c[..., 7] * x + c[..., 8] * y
    return a00, a01, a11, a00 * a11 - a01 * a01


class Operator:
    """out[row] = sum vals * in[col] on flattened N x N grids, as a COO triple (taps outside the grid are left out)."""

    def __init__(self, N, rows, cols, vals):
        self.N, self.rows, self.cols, self.vals = N, rows, cols, vals

    def warp(self, B):
        b = np.asarray(B, np.float64).reshape(-1)
        return np.bincount(self.rows, self.vals * b[self.cols], minlength=self.N * self.N).reshape(self.N, self.N)

    def adjoint(self, g):
        v = np.asarray(g, np.float64).reshape(-1)
        return np.bincount(self.cols, self.vals * v[self.rows], minlength=self.N * self.N).reshape(self.N, self.N)

    def warp_abs(self, B):
        """sum |w * value| per destination pixel: the scale of the float32 products and sums of the forward kernel."""
        b = np.abs(np.asarray(B, np.float64).reshape(-1))
        return np.bincount(self.rows, np.abs(self.vals) * b[self.cols], minlength=self.N * self.N).reshape(self.N, self.N)

    def adjoint_abs(self, g):
        v = np.abs(np.asarray(g, np.float64).reshape(-1))
        return np.bincount(self.cols, np.abs(self.vals) * v[self.rows], minlength=self.N * self.N).reshape(self.N, self.N)

    def dense(self):
        M = np.zeros((self.N * self.N, self.N * self.N))
        np.add.at(M, (self.rows, self.cols), self.vals)
        return M


def _operator(N, X, Y, scale):
    """Bilinear taps at the sample positions X, Y [N][N] (float64 arithmetic from here on), zeros outside, times scale."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    x0, y0 = np.floor(X), np.floor(Y)
    fx, fy = X - x0, Y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    dest = np.arange(N * N).reshape(N, N)
    rows, cols, vals = [], [], []
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < N) & (xx >= 0) & (xx < N)
            rows.append(dest[ok])
            cols.append((yy * N + xx)[ok])
            vals.append((wy * wx * scale)[ok])
    return Operator(N, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def warp_operator(N, a00, a01, a11, flux=True):
    """warp_grid of DESIGN.md §3 for one matrix: out(u) = bilinear_0(B, c + A^-1 (u - c)) / det A, c = (N - 1) // 2.
    flux=False leaves the division by det A out (apply_distortion renormalises to unit sum instead)."""
    a00, a01, a11 = float(a00), float(a01), float(a11)
    det = a00 * a11 - a01 * a01
    i00, i01, i11 = a11 / det, -a01 / det, a00 / det
    c = float((N - 1) // 2)
    q = np.arange(N, dtype=np.float64) - c
    qx, qy = q[None, :], q[:, None]
    return _operator(N, c + i00 * qx + i01 * qy, c + i01 * qx + i11 * qy, 1.0 / det if flux else 1.0)


def position_rounding(N, a00, a01, a11, flux=True, divide=False):
    """The same operator with the sample positions in np.float32: det, A^-1 (through the reciprocal of det as
    psf_warp_kernel forms it, or by division as distort_psf_kernel does) and X, Y, one float32 rounding per operation.
    The entries are taken as float32 (``matrices(..., dtype=np.float32)``).  Only to measure what float32 positions cost."""
    f = np.float32
    a00, a01, a11 = f(a00), f(a01), f(a11)
    det = a00 * a11 - a01 * a01
    idet = f(1.0) / det
    if divide:
        i00, i01, i11 = a11 / det, -a01 / det, a00 / det
    else:
        i00, i01, i11 = a11 * idet, -a01 * idet, a00 * idet
    c = f((N - 1) // 2)
    q = np.arange(N, dtype=f) - c
    qx, qy = q[None, :], q[:, None]
    X = c + i00 * qx + i01 * qy
    Y = c + i01 * qx + i11 * qy
    assert X.dtype == f and Y.dtype == f
    return _operator(N, X, Y, float(idet) if flux else 1.0)


def adjoint(ops, g):
    """Transpose of the resampling of one frame: ops[s] and g[s] of its stars, summed."""
    return sum(op.adjoint(gs) for op, gs in zip(ops, g))


# ---- Moffat from its quadratic form q = (q11, q12, q22, beta): (1 + q11 x^2 + 2 q12 x y + q22 y^2)^-beta, unit sum ------------
def _moffat_terms(N, q):
    q11, q12, q22, beta = (float(v) for v in q)
    c = (N - 1) // 2
    idx = np.arange(N, dtype=np.float64) - c
    x, y = idx[None, :], idx[:, None]
    base = 1.0 + q11 * x * x + 2.0 * q12 * x * y + q22 * y * y
    return x, y, base, beta


def moffat_q(N, q):
    x, y, base, beta = _moffat_terms(N, q)
    M = base ** (-beta)
    return M / M.sum()


def moffat_q_grad(N, q, gT, scale=False):
    """d (sum gT * moffat_q) / d (q11, q12, q22, beta).  scale=True also returns, per component, the size of the terms that
    cancel in it (what an error of the sums is relative to)."""
    x, y, base, beta = _moffat_terms(N, q)
    g = np.asarray(gT, np.float64).reshape(N, N)
    M = base ** (-beta)
    Mb1 = -beta * M / base
    d = [Mb1 * x * x, Mb1 * 2.0 * x * y, Mb1 * y * y, -np.log(base) * M]
    S, G = M.sum(), (g * M).sum()
    out = np.array([((g * dk).sum() - G * dk.sum() / S) / S for dk in d])
    if not scale:
        return out
    return out, np.array([(np.abs(g * dk).sum() + abs(G) * np.abs(dk).sum() / S) / S for dk in d])


# ---- the matrix set ------------------------------------------------------------------------------------------------------------
DET_MIN = 1e-3            # the limit of lc_apply_distortion and lc_psf_batch_set_distortion
STARS = 16


def _case_at(name, d00, d11, d01, sx, sy, rng):
    """Coefficients that give the matrix identity + (d00, d11, d01) at the position (sx / 2, sy / 2): every d split as
    d / 2 + (sx d / 2) x + (sy d / 2) y, so |coefficient| <= 0.25 for |d| <= 0.5 and the signs of x and y matter.  The
    other 15 positions of the frame are random: their matrices lie between the identity and this one."""
    coef = np.array([[d / 2, sx * d / 2, sy * d / 2] for d in (d00, d11, d01)]).reshape(9)
    xy = rng.uniform(-0.5, 0.5, (STARS, 2))
    xy[0] = (0.5 * sx, 0.5 * sy)
    xy[1] = (-0.5 * sx, -0.5 * sy)          # the identity, in the same frame
    return name, coef, xy


def make_cases():
    """[(name, coef[9], xy[16][2])]: the first position of every case carries the matrix the name speaks of.  All in
    float32-representable float64, |coefficient| <= 0.25, |x|, |y| <= 0.5, every det > DET_MIN (test_distortion_cpu.py)."""
    rng = np.random.default_rng(20240611)
    signs = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
    cases = [_case_at('identity', 0.0, 0.0, 0.0, 1, 1, rng)]
    k = 0
    # the corners a00, a11 in {0.5, 1.5} x a01 in {-0.5, +0.5}: a00 = a11 = 0.5 is singular for both signs of a01 (det = 0);
    # the six others have det = 0.5 (a00 != a11) or 2 (a00 = a11 = 1.5)
    for d00 in (-0.5, 0.5):
        for d11 in (-0.5, 0.5):
            for d01 in (-0.5, 0.5):
                if (1 + d00) * (1 + d11) - d01 * d01 > DET_MIN:
                    cases.append(_case_at(f'corner{1 + d00:g},{1 + d11:g},{d01:+g}', d00, d11, d01, *signs[k % 4], rng))
                    k += 1
    cases.append(_case_at('shear+0.5', 0.0, 0.0, 0.5, -1, 1, rng))
    cases.append(_case_at('shear-0.5', 0.0, 0.0, -0.5, 1, -1, rng))
    cases.append(_case_at('near-singular', -0.45, -0.45, 0.5, 1, 1, rng))         # det = 0.0525
    cases.append(_case_at('hv2hu1', 0.5, -0.25, 0.25, -1, -1, rng))               # |a00| + |a01| = 1.75, |a01| + |a11| = 1
    cases.append(_case_at('hv1hu2', -0.25, 0.5, 0.25, 1, -1, rng))
    n = 0
    while n < 12:           # seeded random: nine free coefficients, the first star in a corner of the field
        coef = rng.uniform(-0.25, 0.25, 9)
        xy = rng.uniform(-0.5, 0.5, (STARS, 2))
        xy[0] = 0.5 * np.array(signs[n % 4])
        if matrices(np.float32(coef), np.float32(xy))[3].min() > 0.05:
            cases.append((f'random{n}', coef, xy))
            n += 1
    # one frame whose 16 stars all have different matrices: every coefficient of x and y at the bound
    coef = 0.25 * np.array([0.3, 1, -1, -0.2, -1, 1, 0.1, 1, 1])
    cases.append(('sixteen', coef, rng.uniform(-0.5, 0.5, (STARS, 2))))
    return [(name, np.float32(c).astype(np.float64), np.float32(p).astype(np.float64)) for name, c, p in cases]


CASES = make_cases()
CORNERS = [c for c in CASES if c[0].startswith('corner')]


def noise_grid(rng, N):
    """float32 noise of unit scale over the whole grid, its largest values on the outermost two rows and columns."""
    B = np.clip(rng.standard_normal((N, N)), -3.5, 3.5)
    ring = np.ones((N, N), bool)
    ring[2:N - 2, 2:N - 2] = False
    B[ring] = (np.sign(B[ring]) + (B[ring] == 0)) * (4.0 + np.abs(B[ring]))
    return B.astype(np.float32)
