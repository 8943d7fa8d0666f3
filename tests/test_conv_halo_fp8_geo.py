"""Host walk of the halo-tile fp8 conv geometry (no GPU).

Compiles tests/conv_halo_fp8_geo_check.cpp against
ops/csrc/conv_halo_fp8_geo.h — the header the kernel itself calls for its
LDS offsets, piece -> source map, fragment offsets and wait counts — and
runs it: every lane of every patch piece, weight piece and fragment read for
the GPU test shapes.
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


def test_conv_halo_fp8_geometry(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found')
    exe = str(tmp_path / 'conv_halo_fp8_geo_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                    os.path.join(HERE, 'conv_halo_fp8_geo_check.cpp'),
                    '-o', exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'all geometry checks passed' in r.stdout
