"""Every header of em_pose_amd/csrc compiles on its own (CPU: hipcc cross-compiles): an interface or helper header
includes what its own declarations need and leans on nothing its includer happened to include first."""
import glob
import os
import shutil
import subprocess

import pytest

from em_pose_amd import build as B

HEADERS = sorted(os.path.basename(h) for h in glob.glob(os.path.join(B.CSRC, '*.h')))


def _hipcc():
    cand = B._hipcc()
    return cand if os.path.isabs(cand) else shutil.which(cand)


def test_there_are_headers_to_check():
    assert 'options.h' in HEADERS and 'launch.h' in HEADERS and 'api_internal.h' in HEADERS

@pytest.mark.skipif(_hipcc() is None, reason='hipcc not found')
@pytest.mark.parametrize('header', HEADERS)
def test_header_compiles_on_its_own(header):
    p = subprocess.run([_hipcc(), '--offload-arch=' + B.ARCH, '-std=c++17', '--cuda-device-only', '-fsyntax-only',
                        '-x', 'hip', header], cwd=B.CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
