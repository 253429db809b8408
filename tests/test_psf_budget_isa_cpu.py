"""Instruction and register budget of the C2 two-workgroup PSF kernel (PsfCfg<64,2,8,8,true,8>, SPLIT) against the build of
the commit before the change that keeps the starlet's transpose addresses live and requests the operands of the transposed
row pass a star ahead (csrc/starlet_device.h: LIVE_ADDR, csrc/psf_kernels.h: P5), read from the assembly hipcc makes of
csrc/psf_batch.hip with the flags of csrc/Makefile.

That build held, in this kernel, 56 v_mul_lo_u32 (48 of them in the starlet: two per transpose), 30 v_med3_i32, 209 vector
registers and no scratch.  tests/golden/psf_budget_parent_resources.json holds what -Rpass-analysis=kernel-resource-usage
reported for every kernel of psf_batch.hip and joint_fit.hip in that build, as [VGPRs, spilled VGPRs, scratch bytes per lane,
waves per SIMD]: the live addresses must not leak into the joint fit's starlet, the one-workgroup form or the N = 128 kernel."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'lightcurver_amd', 'csrc')
C2_SPLIT = 'PsfCfgILi64ELi2ELi8ELi8ELb1ELi8EEELb1EE'
# the two-workgroup kernels whose starlet takes the live addresses: C2 and n = 16 at ss = 2 (n = 24, twelve lanes per line, runs
# the LDS form of the starlet, which has no such flag)
MAY_CHANGE = (C2_SPLIT, 'PsfCfgILi32ELi2ELi4ELi8ELb1ELi8EEELb1EE')
PARENT = {'v_mul_lo_u32': 56, 'v_med3_i32': 30, 'NumVgprs': 209, 'ScratchSize': 0}
STARLET_BARRIERS = 24   # 6 scales x (forward, adjoint) x (to columns, to rows)

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'), reason='no hipcc')


def compile_report(tmp, source):
    """(assembly text, {kernel: [VGPRs, spilled VGPRs, scratch bytes per lane, waves per SIMD]}) of one source file."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    asm = tmp / (source + '.s')
    out = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '--cuda-device-only', '-S',
                          '-Rpass-analysis=kernel-resource-usage', source, '-o', str(asm)],
                         cwd=CSRC, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    found, name = {}, None
    for line in out.stderr.split('\n'):
        m = re.search(r'remark: +(.*?)(?: \[-Rpass|$)', line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith('Function Name:'):
            name = text.split(':', 1)[1].strip()
            found[name] = {}
        elif name and ':' in text:
            k, v = text.rsplit(':', 1)
            found[name][k.strip()] = v.strip()
    res = {k: [int(v['VGPRs']), int(v['VGPRs Spill']), int(v['ScratchSize [bytes/lane]']), int(v['Occupancy [waves/SIMD]'])]
           for k, v in found.items()}
    return asm.read_text(), res


@pytest.fixture(scope='module')
def psf_batch(tmp_path_factory):
    return compile_report(tmp_path_factory.mktemp('budget'), 'psf_batch.hip')


@pytest.fixture(scope='module')
def parent_resources():
    with open(os.path.join(HERE, 'golden', 'psf_budget_parent_resources.json')) as fh:
        return json.load(fh)


def c2_kernel(asm):
    """Instruction lines of the C2 two-workgroup kernel and its .amdhsa / comment metadata."""
    names = set(re.findall(r'^(_Z\w*psf_fit_kernel\w*):', asm, re.M))
    hit = [k for k in names if C2_SPLIT in k]
    assert len(hit) == 1, sorted(names)
    body = re.split(r'^' + hit[0] + r':.*$', asm, maxsplit=1, flags=re.M)[1]
    code, rest = body.split('s_endpgm', 1)
    lines = [l.split(';')[0].strip() for l in code.split('\n')]
    lines = [l for l in lines if l and not l.startswith('.') and not l.endswith(':')]
    meta = rest.split('.end_amdhsa_kernel', 1)[0] + rest.split('.end_amdhsa_kernel', 1)[1][:4000]
    return lines, meta


def count(lines, op):
    return sum(1 for l in lines if l.split()[0] == op)


def starlet_region(lines):
    """Indices (first, last) of the first and the last barrier of the starlet: its passes are the only code that multiplies
    through DPP (v_fmac_f32_dpp, v_mul_f32_dpp); a barrier follows the first pass and the last one."""
    ops = [l.split()[0] for l in lines]
    marks = [i for i, op in enumerate(ops) if op in ('v_fmac_f32_dpp', 'v_mul_f32_dpp')]
    barriers = [i for i, op in enumerate(ops) if op == 's_barrier']
    first = min(b for b in barriers if b > marks[0])
    last = min(b for b in barriers if b > marks[-1])
    return first, last, sum(1 for b in barriers if first <= b <= last)


def test_c2_kernel_budget(psf_batch):
    lines, meta = c2_kernel(psf_batch[0])
    counts = {op: count(lines, op) for op in ('v_mul_lo_u32', 'v_med3_i32')}
    first, last, nbar = starlet_region(lines)
    inside = [l for l in lines[first:last + 1] if l.split()[0] == 'v_mul_lo_u32']
    vgprs = int(re.search(r'; NumVgprs: (\d+)', meta).group(1))
    scratch = int(re.search(r'; ScratchSize: (\d+)', meta).group(1))
    print(counts, 'starlet barriers', nbar, 'v_mul_lo_u32 between them', len(inside), 'NumVgprs', vgprs, 'ScratchSize', scratch)
    assert nbar == STARLET_BARRIERS, nbar
    assert counts['v_mul_lo_u32'] < PARENT['v_mul_lo_u32'], counts
    assert not inside, inside
    assert scratch == 0
    assert vgprs <= 256
    assert counts['v_med3_i32'] <= PARENT['v_med3_i32'], counts


def test_scan_finds_the_parents_multiplies():
    """The region scan itself, on a made-up kernel: a multiply between the starlet's barriers is seen, one outside is not."""
    k = ['v_mul_lo_u32 v1, v2, s3', 'v_mul_f32_dpp v4, v1, v5 row_shr:1', 's_barrier', 'v_mul_lo_u32 v1, v2, s3',
         'v_fmac_f32_dpp v4, v1, v5 row_shr:1', 's_barrier', 'v_mul_lo_u32 v1, v2, s3', 's_barrier']
    first, last, nbar = starlet_region(k)
    assert (first, last, nbar) == (2, 5, 2)
    assert sum(1 for l in k[first:last + 1] if l.split()[0] == 'v_mul_lo_u32') == 1


@pytest.mark.parametrize('source', ['psf_batch.hip', 'joint_fit.hip'])
def test_other_kernels_keep_their_registers(source, psf_batch, parent_resources, tmp_path):
    res = psf_batch[1] if source == 'psf_batch.hip' else compile_report(tmp_path, source)[1]
    want = parent_resources[source]
    assert set(res) == set(want), sorted(set(res) ^ set(want))
    moved = {k: (want[k], res[k]) for k in want if res[k] != want[k] and not any(m in k for m in MAY_CHANGE)}
    print(source, len(res), 'kernels;', {k: (want[k], res[k]) for k in want if res[k] != want[k]})
    assert not moved, moved
    for k in res:   # and those that may change neither spill nor lose a wave
        if any(m in k for m in MAY_CHANGE):
            assert res[k][1] <= want[k][1] and res[k][2] <= want[k][2] and res[k][3] >= want[k][3], (k, want[k], res[k])
