"""The launchers' shared host logic (poisson_cnn_amd/csrc/pcnn_host.h: pcnn_reserve / pcnn_drop for the handle-owned buffers, the convolution descriptor
check) as a stand-alone g++ program with the HIP runtime calls stubbed over malloc (tests/host/test_pcnn_host.cpp): no GPU, no HIP library, no Python
extension.  Built plain and under AddressSanitizer + UndefinedBehaviorSanitizer, whose leak and double-free checks stand behind "every block is freed
exactly once"."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'test_pcnn_host.cpp')
ROCM_INCLUDE = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'include')
FLAGS = ['g++', '-std=c++17', '-Wall', '-D__HIP_PLATFORM_AMD__', '-I' + ROCM_INCLUDE]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None or not os.path.exists(os.path.join(ROCM_INCLUDE, 'hip', 'hip_runtime_api.h')),
                                reason='needs g++ and the HIP API header')


def test_pcnn_host_logic(tmp_path):
    exe = tmp_path / 'test_pcnn_host'
    subprocess.run(FLAGS + ['-O2', '-o', str(exe), SRC], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, r.stdout + r.stderr


def test_pcnn_host_logic_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = tmp_path / 'test_pcnn_host_san'
    r = subprocess.run(FLAGS + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', str(exe), SRC],
                       capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0 and ('asan' in r.stderr.lower() or 'ubsan' in r.stderr.lower() or 'sanitize' in r.stderr.lower()):
        pytest.skip('this toolchain has no sanitizer runtime: ' + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, (r.stdout + r.stderr)[-3000:]
