"""Host walk of the tap-row wgrad geometry (no GPU).

Compiles tests/wgrad_row_geo_check.cpp against ops/csrc/wgrad_row_geo.h — the
header wgrad_row.hip itself calls for its apron image, shifted fragment
reads, source map, edge masks and chunk rule — and runs it: fill image
against read map, 1-way banking for the three shifts, sources inside the
image, masks on exactly the image-row edge pixels, chunk lengths multiples
of 128.
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


def test_wgrad_row_geometry(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found')
    exe = str(tmp_path / 'wgrad_row_geo_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                    os.path.join(HERE, 'wgrad_row_geo_check.cpp'), '-o', exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'all geometry checks passed' in r.stdout
