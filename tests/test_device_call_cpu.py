"""Error paths of the device-buffer ownership header (csrc/device_call.h), which cannot and must not be provoked on a
GPU: tests/host/device_call_main.cpp includes the real header over a stand-in HIP runtime (tests/host/hip/hip_runtime.h)
that fails the k-th runtime call, and checks for every k that the call reports LC_ERR_DEVICE with a message and leaves
no allocation behind, and that grow_history leaves the old buffer in place.  The program is built with the host
compiler's address and undefined-behaviour sanitizers and run on its own; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, 'tests', 'host')


def _compiler():
    for cxx in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(cxx) if cxx else None
        if path:
            return path
    return None


def test_device_call_error_paths(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found (CXX, c++, g++, clang++): the host program cannot be built')
    exe = str(tmp_path / 'device_call_main')
    # the stand-in hip/hip_runtime.h comes first on the include path; device_call.h is the library's own, unmodified
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', '-I', HOST,
                            '-I', os.path.join(ROOT, 'lightcurver_amd', 'csrc'),
                            os.path.join(HOST, 'device_call_main.cpp'), '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'all checks passed' in run.stdout
