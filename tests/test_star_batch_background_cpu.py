"""The scope of the batched star photometry with a background per star is decided by the library (no device needed to ask):
exactly the stamp sizes whose joint fit has a single-workgroup update, and the Python side asks the library rather than
keeping a list of its own."""


def test_background_batch_scope_is_the_single_workgroup_sizes():
    from lightcurver_amd import _lib
    from lightcurver_amd.joint import background_batch_supported
    lib = _lib.lib()
    got = {(n, ss) for ss in (1, 2) for n in range(2, 130, 2) if lib.lc_joint_groups_background_supported(n, ss)}
    assert got == {(16, 2), (24, 2), (32, 2), (16, 1)}
    assert all(lib.lc_joint_supported(n, ss) for n, ss in got)
    assert not lib.lc_joint_groups_background_supported(64, 2) and lib.lc_joint_supported(64, 2)
    assert all(background_batch_supported(n, ss) == ((n, ss) in got) for ss in (1, 2) for n in range(2, 130, 2))


def test_ring_at_median_variance_is_what_the_embedded_fit_uses():
    import numpy as np
    from lightcurver_amd.joint import ring_at_median_variance
    rng = np.random.default_rng(0)
    E, n, pad = 3, 6, 2
    sigma2 = rng.uniform(0.5, 2.0, (E, n, n)).astype(np.float32)
    var = np.full((E, n + 2 * pad, n + 2 * pad), 1e20, np.float32)
    var[:, pad:pad + n, pad:pad + n] = sigma2
    out = ring_at_median_variance(var, sigma2, pad)
    assert out.dtype == np.float32 and out is not var and np.all(var[:, 0, 0] == 1e20)
    assert np.array_equal(out[:, pad:pad + n, pad:pad + n], sigma2)
    for e in range(E):
        ring = out[e].copy()
        ring[pad:pad + n, pad:pad + n] = np.nan
        assert np.all(ring[~np.isnan(ring)] == np.float32(np.median(sigma2[e])))
