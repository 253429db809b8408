"""Golden values for ``estimate_seeing``, captured from the REFERENCE's own function:
    python tests/golden/make_seeing_golden.py <path of the reference checkout>
The reference module (lightcurver/processes/frame_characterization.py) does not import without ephem and astropy, but
the function needs only NumPy and a mapping with 'FWHM': its definition alone is compiled out of the module's source.
Only inputs and outputs are stored (seeing_golden.npz); the reference source never travels."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_estimate_seeing(root):
    path = os.path.join(root, 'lightcurver', 'processes', 'frame_characterization.py')
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'estimate_seeing']
    scope = {'np': np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, 'exec'), scope)
    return scope['estimate_seeing']


def cases():
    rng = np.random.default_rng(2010)
    stars = rng.normal(4.2, 0.25, 60)
    out = {
        # more than 10 with a clear peak inside the range, some galaxies and cosmics around it
        'clear_peak': np.concatenate([stars, rng.uniform(6.0, 14.0, 12), rng.uniform(1.0, 2.0, 5)]),
        # the peak in the first bin of the first histogram
        'peak_first_bin': np.concatenate([rng.uniform(1.5, 1.9, 30), rng.uniform(2.5, 6.0, 8)]),
        # the peak in the last bin: the range ends at 3 x the median
        'peak_last_bin': np.concatenate([rng.uniform(0.5, 1.4, 9), np.full(3, 2.0), rng.uniform(5.6, 5.99, 8)]),
        # The branch for an empty window of +-1 around the refined peak cannot be reached with finite values: the fullest
        # bin of the second histogram is 0.4 wide and not empty, and its values lie within 0.2 of its centre.  The nearest
        # input: the values of the second histogram sit on its two outer edges, the last one closed.
        'narrow_window_edges': np.concatenate([np.full(6, 4.85), np.full(6, 8.85), np.full(3, 6.0), np.full(2, 12.0)]),
        'few': rng.normal(3.5, 0.3, 7),
        'one': np.array([2.75]),
        'ten': rng.normal(5.0, 0.5, 10),
        'none': np.zeros(0),
        'all_below_range': rng.uniform(0.5, 1.2, 20),
    }
    return out


def main():
    fn = load_estimate_seeing(sys.argv[1])
    store = {}
    for name, fwhm in cases().items():
        store[f'{name}__fwhm'] = np.asarray(fwhm, np.float64)
        store[f'{name}__seeing'] = np.float64(fn({'FWHM': np.asarray(fwhm, np.float64)}))
        print(name, len(fwhm), store[f'{name}__seeing'])
    np.savez(os.path.join(HERE, 'seeing_golden.npz'), **store)


if __name__ == '__main__':
    main()
