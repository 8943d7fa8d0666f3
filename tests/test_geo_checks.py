"""Host walks of the kernel geometry headers (no GPU).

Each tests/<name>_geo_check.cpp is compiled against ops/csrc/<name>_geo.h —
the header the kernel itself calls for its LDS offsets, staging lane maps,
source maps, fragment-read addresses and wait counts — and run: it visits
every lane of every staging piece and fragment read for the GPU test shapes
and lists what it checks in its header comment. tests/geo_check.h holds what
the four programs share.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'real_time_helmet_detection_amd',
                    'ops', 'csrc')


def _host_compiler():
    for cc in (os.environ.get('CXX'), 'g++', 'c++', 'clang++'):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    return None


@pytest.mark.parametrize('name', ['conv_halo', 'conv_halo_fp8', 'wgrad_tr',
                                  'wgrad_row'])
def test_geometry(name, tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found')
    exe = str(tmp_path / (name + '_geo_check'))
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-I', CSRC, '-I', HERE,
                    os.path.join(HERE, name + '_geo_check.cpp'), '-o', exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'all geometry checks passed' in r.stdout
