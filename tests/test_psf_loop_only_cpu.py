"""The C2 two-workgroup PSF kernel (PsfCfg<64,2,8,8,true,8>, SPLIT) compiled for the launch it gets (csrc/psf_kernels.h,
LOOP_ONLY and TOP_LIVE; DESIGN.md, "PSF fit: the two-workgroup loop without its launch constants"), read from the assembly hipcc
makes of csrc/psf_batch.hip with the flags of csrc/Makefile, beside the same source with both switches off
(-DLC_LOOP_ONLY=0 -DLC_LOOP_TOP_LIVE=0), which is the kernel before the change.

Stores to global memory.  With the switches off the kernel holds 37 global_store_* instructions (19 dword, 18 dwordx4): those
below and the stores of the eval outputs, out_model in the column pass of both task loops, out_gT, out_ggrid, out_gstars,
out_loss and out_chi2.  Compiled for the loop, 26 are left, and each is accounted for:
  dwordx4, 14: the hand-off stores of either role in their two flavours (2 quads x 2 flavours x 2 roles = 8), the final state
               B, mB, sB (2 quads x 3 = 6)
  dword,   12: role 1's l1 value in its two flavours (2), the XCD word of either role (2), the flag in its two flavours (2), the
               abort word from the test hook and from the polling lane (2), the loss history (1), the final stars and their two
               moments (3)
The bound is that number: a store to an eval output cannot come back without passing it.

The loop top.  Instructions from the header of the iteration loop to the first s_barrier behind it in the text are counted in
both builds: 140 before, 72 with both switches.  This is a count in text order, not along the path of a wave of role 0: it
includes the block of the schedule entry, which three lanes run, and depends on how the compiler lays the blocks out (role 0's
come first: the thread's addresses, the zeroed accumulators, down to the barrier that opens the second group of stars).  The
test asserts the drop, not the figures."""
import os
import re
import shutil
import subprocess
from collections import Counter

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'lightcurver_amd', 'csrc')
C2_SPLIT = 'PsfCfgILi64ELi2ELi8ELi8ELb1ELi8EEELb1EE'
N32_SPLIT = 'PsfCfgILi32ELi2ELi4ELi8ELb1ELi8EEELb1EE'
STORES_FOR_THE_LOOP = 26      # 14 dwordx4 + 12 dword, listed above
EVAL_OUTPUT_STORES = 11       # what the switched-off build holds beyond them

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'), reason='no hipcc')


def compile_kernels(tmp, tag, *flags):
    """{kernel: (instruction lines, raw lines, [VGPRs, scratch bytes per lane, waves per SIMD])} of psf_batch.hip's PSF kernels."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    asm = tmp / (tag + '.s')
    out = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '--cuda-device-only', '-S',
                          '-Rpass-analysis=kernel-resource-usage', *flags, 'psf_batch.hip', '-o', str(asm)],
                         cwd=CSRC, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.split('\n'):
        m = re.search(r'remark: +(.*?)(?: \[-Rpass|$)', line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith('Function Name:'):
            name = text.split(':', 1)[1].strip()
            res[name] = {}
        elif name and ':' in text:
            k, v = text.rsplit(':', 1)
            res[name][k.strip()] = v.strip()
    text = asm.read_text()
    found = {}
    for k in set(re.findall(r'^(_Z\w*psf_fit_kernel\w*):', text, re.M)):
        raw = re.split(r'^' + k + r':.*$', text, maxsplit=1, flags=re.M)[1].split('s_endpgm', 1)[0].split('\n')
        r = res[k]
        found[k] = (instructions(raw), raw,
                    [int(r['VGPRs']), int(r['ScratchSize [bytes/lane]']), int(r['Occupancy [waves/SIMD]'])])
    return found


def instructions(raw):
    lines = [l.split(';')[0].strip() for l in raw]
    return [l for l in lines if l and not l.startswith('.') and not l.endswith(':')]


def pick(kernels, tag):
    hit = [k for k in kernels if tag in k]
    assert len(hit) == 1, sorted(kernels)
    return kernels[hit[0]]


def stores(lines):
    return Counter(l.split()[0] for l in lines if l.startswith('global_store_'))


def loop_top(raw):
    """Instructions between the header of the iteration loop - the outermost loop with the most loops inside - and the first
    s_barrier that follows it in the text."""
    def children(i):   # the header's own comment lines, which follow it at once
        k = i + 1
        while k < len(raw) and 'Child Loop' in raw[k]:
            k += 1
        return k - i - 1
    heads = [i for i, l in enumerate(raw) if 'This Loop Header: Depth=1' in l]
    assert heads
    head = max(heads, key=children)
    assert children(head) >= 4, raw[head:head + 16]
    n = 0
    for l in instructions(raw[head + 1:]):
        if l.split()[0] == 's_barrier':
            return n
        n += 1
    raise AssertionError('no barrier behind the loop header')


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('loop_only')
    return compile_kernels(tmp, 'new'), compile_kernels(tmp, 'parent', '-DLC_LOOP_ONLY=0', '-DLC_LOOP_TOP_LIVE=0')


def test_c2_kernel_stores_only_what_the_loop_stores(builds):
    new, parent = (stores(pick(b, C2_SPLIT)[0]) for b in builds)
    print('global stores, switches off:', dict(parent), sum(parent.values()), ' compiled for the loop:', dict(new), sum(new.values()))
    assert sum(parent.values()) >= STORES_FOR_THE_LOOP + EVAL_OUTPUT_STORES, parent   # the scan sees the eval outputs' stores
    assert sum(new.values()) <= STORES_FOR_THE_LOOP, new
    assert set(new) <= {'global_store_dword', 'global_store_dwordx4'}, new


def test_c2_kernel_resources(builds):
    vgprs, scratch, waves = pick(builds[0], C2_SPLIT)[2]
    print('C2 two-workgroup kernel: VGPRs', vgprs, 'scratch', scratch, 'waves per SIMD', waves, '; switches off:', pick(builds[1], C2_SPLIT)[2])
    assert vgprs <= 256 and scratch == 0 and waves == 2


def test_c2_loop_top_is_shorter(builds):
    new, parent = (loop_top(pick(b, C2_SPLIT)[1]) for b in builds)
    print('loop header to first s_barrier: switches off', parent, ', with them', new)
    assert new < parent


def test_n32_kernel_takes_the_launch_facts_too(builds):
    """N = 32 (n = 16): fewer stores, and neither more registers nor scratch nor fewer waves than with the switch off."""
    new, parent = (pick(b, N32_SPLIT) for b in builds)
    print('N = 32 two-workgroup kernel:', parent[2], '->', new[2], 'stores', sum(stores(parent[0]).values()), '->', sum(stores(new[0]).values()))
    assert sum(stores(new[0]).values()) < sum(stores(parent[0]).values())
    assert new[2][0] <= parent[2][0] and new[2][1] <= parent[2][1] and new[2][2] >= parent[2][2]


def test_the_other_kernels_are_the_same_code(builds):
    """Every kernel but those two - the one-workgroup forms, N = 48 and N = 128 in two workgroups - is instruction for instruction
    what it is with the switches off."""
    new, parent = builds
    assert set(new) == set(parent)
    for k in new:
        if C2_SPLIT in k or N32_SPLIT in k:
            continue
        assert new[k][0] == parent[k][0], k


def test_loop_top_scan_on_a_made_up_kernel():
    raw = ['.LBB0_1: ; =>This Loop Header: Depth=1', ' s_nop 0', ' s_barrier',
           '.LBB0_2: ; =>This Loop Header: Depth=1', '; Child Loop BB0_3 Depth 2', '; Child Loop BB0_4 Depth 2',
           '; Child Loop BB0_5 Depth 2', '; Child Loop BB0_6 Depth 2', ' s_cmp_lg_u32 s0, s1', ' v_mov_b32_e32 v1, v0 ; copy',
           '.LBB0_3:', ' ds_write_b32 v1, v2', ' s_barrier', ' s_nop 0']
    assert loop_top(raw) == 3
