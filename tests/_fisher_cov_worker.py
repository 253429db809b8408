"""One rank of the two-process flux-covariance test (tests/test_fisher_covariance_gpu.py): the sharded two-stage ROI fit
(processes/roi_modelling.model_roi_cutouts_sharded) with return_flux_covariance=True, each rank its contiguous half of the
epochs on GPU 0, the shared block summed by a gloo all-reduce.  Rank 0 then builds one object over all epochs at the
gathered parameters and saves its covariance and diagonal 1-sigma beside the gathered ones.
usage: RANK=r WORLD_SIZE=w MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/_fisher_cov_worker.py out.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from lightcurver_amd import _lib
    from lightcurver_amd.distributed import shard_epochs
    from lightcurver_amd.joint import JointFit
    from lightcurver_amd.processes.roi_modelling import global_scale, initial_point_source_fluxes, model_roi_cutouts_sharded
    from lightcurver_amd.synthetic import make_roi_dataset
    E, M, n, ss = 10, 2, 32, 2
    ds = make_roi_dataset(E=E, M=M, n=n, ss=ss, seed=4343)
    lo, hi = shard_epochs(E, world, rank)
    ctx = _lib.Context(0)
    off = (n - 1) / 2.0
    xs, ys = np.asarray(ds['truth']['c_x']) + off, np.asarray(ds['truth']['c_y']) + off
    scale = global_scale(ds['data'][lo:hi])
    a0 = initial_point_source_fluxes(ds['data'] / scale, xs, ys, 3.0)
    res = model_roi_cutouts_sharded(ds['data'][lo:hi], ds['noisemap'][lo:hi], ds['psf'][lo:hi], ss, xs, ys,
                                    np.asarray(a0) * scale, scale, roi_deconv_translations_iters=20, roi_deconv_all_iters=40,
                                    ctx=ctx, return_flux_covariance=True)
    if rank == 0:
        data = np.array(ds['data'], dtype=np.float64) / scale
        noisemap = np.array(ds['noisemap'], dtype=np.float64) / scale
        j = JointFit(data, noisemap ** 2, ds['psf'], ss, M, ctx)
        try:
            j.set_params(**res['flat_final'])
            j.set_free(['a'])
            _, cov_one, _ = j.fisher_flux_covariance()
            sigma_one = j.fisher_flux_sigma()
        finally:
            j.close()
        np.savez(out, cov=res['fluxes_covariance'], sigma=res['fluxes_sigma'], cov_one=cov_one, sigma_one=sigma_one)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
