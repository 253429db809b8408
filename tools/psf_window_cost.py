"""What windowing a PSF stamp wider than the joint fit's grid costs, on the float64 oracle alone: for
stamps of side P > N = ss n, the oracle's model with the stamps themselves (conv_same takes any kernel size) against its
model with the N x N window joint.place_psf keeps - the largest difference over the model's peak - and the largest
fraction of a stamp's flux outside the window.  No device is used.

    python tools/psf_window_cost.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightcurver_amd.joint import place_psf, psf_flux_outside  # noqa: E402
from lightcurver_amd.synthetic import make_narrow_psf, make_roi_dataset  # noqa: E402
from oracle import model as om  # noqa: E402


def cost(n, P, ss=2, E=4, M=2, seed=0):
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=seed)
    rng = np.random.default_rng(seed + 1)
    stamps = np.stack([make_narrow_psf(rng, P, ss)[0] for _ in range(E)])
    p = {k: om.T(np.array(v, dtype=np.float64)) for k, v in ds['truth'].items()}
    full = om.deconv_model(p, om.T(stamps), ss, n).numpy()
    window = om.deconv_model(p, om.T(place_psf(stamps, n * ss)), ss, n).numpy()
    return np.abs(full - window).max() / np.abs(full).max(), psf_flux_outside(stamps, n * ss)


if __name__ == '__main__':
    print('(n, P, ss)      model difference / peak    flux outside the window')
    for n, P in ((24, 64), (32, 64), (16, 48)):
        worst = [cost(n, P, seed=s) for s in range(5)]
        d, f = max(w[0] for w in worst), max(w[1] for w in worst)
        print(f'({n}, {P}, 2)   {d:.1e}                    {f:.1e}')
