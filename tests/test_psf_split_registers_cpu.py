"""Register budget of the two-workgroup PSF-fit kernels (csrc/psf_kernels.h, psf_fit_kernel<C, true>).

The C2 instantiation (PsfCfg<64,2,8,8,true,8>) runs at the 256-register limit of two waves per SIMD, the C3 one
(PsfCfg<128,2,16,1,false,8>) at the 128 registers a 1024-thread workgroup may have; what does not fit goes to scratch
memory inside the iteration loop.  Work on the hand-off between the two workgroups must not add to that: no more spilled
vector registers than the build of commit 0662cf3 ("Detect cosmic rays in star and ROI stamps on the device"), read from
that commit with the flags of csrc/Makefile: 5 at N = 64, 36 at N = 128.

hipcc cross-compiles without a GPU; the figures come from -Rpass-analysis=kernel-resource-usage of csrc/psf_batch.hip."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'lightcurver_amd', 'csrc')

# mangled template arguments of the two instantiations, two-workgroup form (the trailing Lb1E), and the spilled VGPRs of
# commit 0662cf3
PARENT_SPILLS = {
    'PsfCfgILi64ELi2ELi8ELi8ELb1ELi8EEELb1EE': 5,
    'PsfCfgILi128ELi2ELi16ELi1ELb0ELi8EEELb1EE': 36,
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'), reason='no hipcc')
def test_two_workgroup_kernels_spill_no_more_than_before(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    out = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-Rpass-analysis=kernel-resource-usage',
                          '-c', 'psf_batch.hip', '-o', str(tmp_path / 'pb.o')], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r'remark:\s+(VGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]): (\d+)', line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    for key, parent in PARENT_SPILLS.items():
        hit = [(k, v) for k, v in usage.items() if 'psf_fit_kernel' in k and key in k]
        assert len(hit) == 1, (key, sorted(usage))
        k, v = hit[0]
        print(k, v)
        assert v['VGPRs Spill'] <= parent, (k, v, parent)
