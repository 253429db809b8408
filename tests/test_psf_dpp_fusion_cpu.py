"""Lane exchanges of the PSF-fit kernels ride on the arithmetic that uses them (csrc/starlet_device.h: dpp_taps, dpp_gated,
line_sum, wave_sum4), read from the assembly hipcc makes of csrc/psf_batch.hip with the flags of csrc/Makefile.

The compiler folds a DPP lane move into a following add or product, not into a fused multiply-add, so the starlet's taps are
written in assembly - where the compiler's hazard recogniser does not look.  A DPP read needs two wait states after a VALU
write of the register it reads; a stale read gives wrong numbers silently.  So beside the counts a linear scan checks every
DPP instruction of every psf_fit_kernel instantiation against the vector writes in front of it.

The build of the parent commit held 471 v_mov_b32_dpp and no v_fmac_f32_dpp in the C2 kernel (PsfCfg<64,2,8,8,true,8>, two
workgroups per frame); every one of those moves fed a multiply-add, a product or an add."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'lightcurver_amd', 'csrc')
C2_SPLIT = 'PsfCfgILi64ELi2ELi8ELi8ELb1ELi8EEELb1EE'

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'), reason='no hipcc')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    """{mangled name: [instruction or label lines]} of every psf_fit_kernel instantiation."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    asm = tmp_path_factory.mktemp('dpp') / 'psf_batch.s'
    out = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '--cuda-device-only', '-S',
                          'psf_batch.hip', '-o', str(asm)], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found, name = {}, None
    for line in asm.read_text().split('\n'):
        m = re.match(r'^(_Z\w*psf_fit_kernel\w*):', line)
        if m:
            name = m.group(1)
            found[name] = []
            continue
        text = line.split(';')[0].strip()
        if name is None or not text or text.startswith('.') and not text.endswith(':'):
            continue
        found[name].append(text)
        if text == 's_endpgm':
            name = None
    assert found
    return found


def count(lines, op):
    return sum(1 for l in lines if l.split()[0] == op)


def vgprs(operand):
    """Vector registers an operand names: v7 -> {7}, v[4:5] -> {4, 5}, anything else -> {}."""
    m = re.fullmatch(r'v(\d+)', operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r'v\[(\d+):(\d+)\]', operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def stale_dpp_reads(lines):
    """DPP instructions whose DPP source (src0) was written by a v_* instruction fewer than two wait states earlier.
    s_nop N counts N + 1 wait states, any other instruction 1; the scan restarts at labels."""
    bad, age = [], {}   # age[r]: wait states that have passed since a v_* instruction wrote v<r>
    for i, text in enumerate(lines):
        if text.endswith(':'):
            age = {}
            continue
        op, _, rest = text.partition(' ')
        ops = [o.strip() for o in rest.split(',')]
        if op.endswith('_dpp'):
            src0 = ops[1].split()[0].strip('-|')
            for r in vgprs(src0):
                if age.get(r, 99) < 2:
                    bad.append((i, text, age[r]))
        m = re.fullmatch(r's_nop (\d+)', text)
        step = int(m.group(1)) + 1 if m else 1
        for r in age:
            age[r] += step
        if op.startswith('v_'):
            for r in vgprs(ops[0].split()[0]):
                age[r] = 0
    return bad


def test_scan_sees_a_stale_read():
    """The scan itself: one and two wait states between a write and the DPP read of the same register."""
    base = ['v_add_f32_e32 v1, v2, v3', 'v_fmac_f32_dpp v4, v1, v5 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1']
    assert stale_dpp_reads(base)
    assert stale_dpp_reads([base[0], 's_nop 0', base[1]])
    assert not stale_dpp_reads([base[0], 's_nop 1', base[1]])
    assert not stale_dpp_reads([base[0], 'v_mov_b32_e32 v9, v2', 's_nop 0', base[1]])
    assert stale_dpp_reads(['v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7]', 's_nop 0', 'v_mov_b32_dpp v8, v1 quad_perm:[1,0,3,2]'])
    assert not stale_dpp_reads([base[0], '.LBB0_1:', base[1]])


def test_c2_kernel_fuses_its_lane_moves(kernels):
    hit = [k for k in kernels if C2_SPLIT in k]
    assert len(hit) == 1, sorted(kernels)
    lines = kernels[hit[0]]
    counts = {op: count(lines, op) for op in ('v_mov_b32_dpp', 'v_fmac_f32_dpp', 'v_mul_f32_dpp', 'v_add_f32_dpp')}
    print(hit[0], counts)
    assert counts['v_mov_b32_dpp'] <= 48, counts
    assert counts['v_fmac_f32_dpp'] >= 320, counts


def test_no_dpp_read_within_two_wait_states_of_a_vector_write(kernels):
    assert any(C2_SPLIT in k for k in kernels)
    for name, lines in sorted(kernels.items()):
        bad = stale_dpp_reads(lines)
        print(name, len(lines), 'lines,', sum(1 for l in lines if l.split()[0].endswith('_dpp')), 'DPP instructions,', len(bad), 'stale')
        assert not bad, (name, bad[:5])
