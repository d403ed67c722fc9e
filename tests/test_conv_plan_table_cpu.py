"""The convolution planner (csrc/conv_plan.h behind pasta_conv2d_plan, pasta_conv2d_workspace, pasta_conv2d_wgrad_plan and the two weight-gradient
workspace queries) held to a recorded table, its lattice builders and workspace layout held to their definitions by a stand-alone host
program, and the kernel names of the header held to their Python mirror.  Host arithmetic only; no device.

tests/golden/conv_plan_table.npz was recorded by tools/conv_plan_table.py.  A change that moves a plan on purpose records it again and says so;
a refactor must not move one entry."""

import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from torch_utils import custom_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pasta-gan_amd', 'csrc')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import conv_plan_table as table  # noqa: E402


def _header_enum(prefix):
    """{name without prefix: value} of the enumerators ``prefix*`` of include/pasta_hip.h."""
    with open(os.path.join(ROOT, 'include', 'pasta_hip.h')) as f:
        text = f.read()
    return {name: int(value) for name, value in re.findall(r'^\s*%s(\w+)\s*=\s*(\d+)\s*,?\s*/\*' % prefix, text, re.M)}


@pytest.fixture(scope='module')
def recorded():
    return table.load()


def test_planners_answer_the_recorded_table(recorded):
    descs, wscale, fwd0, ws0 = recorded
    fwd, ws = table.answers(custom_ops.get_plugin(), descs, wscale)
    bad = np.flatnonzero((fwd != fwd0).any(axis=(1, 2)) | (ws != ws0).any(axis=1))
    assert len(bad) == 0, [(dict(zip(table.INT_FIELDS, descs[i].tolist())), fwd[i].tolist(), fwd0[i].tolist(), ws[i].tolist(), ws0[i].tolist()) for i in bad[:3]]


def test_table_reaches_every_kernel(recorded):
    _, _, fwd, ws = recorded
    fwd_names, wgrad_names = _header_enum('PASTA_FWD_'), _header_enum('PASTA_WGRAD_')
    assert sorted(fwd_names.values()) == list(range(14)) and sorted(wgrad_names.values()) == list(range(7))
    assert set(fwd[:, :, 5][fwd[:, :, 0] == 1].tolist()) == set(fwd_names.values())
    assert set(ws[:, 2][ws[:, 1] == 1].tolist()) == set(wgrad_names.values())


def test_python_kernel_names_equal_the_header():
    for prefix, names in (('FWD_', _header_enum('PASTA_FWD_')), ('WGRAD_', _header_enum('PASTA_WGRAD_'))):
        mirror = {n[len(prefix):]: getattr(custom_ops, n) for n in dir(custom_ops) if n.startswith(prefix)}
        assert mirror == names and names


def _host_compiler():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    return cxx


def test_planner_header_is_plain_cxx():
    """conv_plan.h compiles with the host compiler alone, no HIP include path, without a warning; and conv_igemm.hip includes no kernel header."""
    res = subprocess.run([_host_compiler(), '-std=c++17', '-Wall', '-Wextra', '-fsyntax-only', '-x', 'c++', os.path.join(CSRC, 'conv_plan.h')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and not res.stdout.strip(), res.stdout
    for name, banned in (('conv_plan.h', r'#include\s*[<"]hip|__device__|\bdim3\b|hipStream_t'), ('host_common.h', r'#include\s*[<"]hip')):
        with open(os.path.join(CSRC, name)) as f:
            assert not re.search(banned, f.read()), name
    with open(os.path.join(CSRC, 'conv_igemm.hip')) as f:
        assert not re.findall(r'#include\s*"conv_(?:fwd|wgrad)_\w*\.h"', f.read())


def test_lattices_and_workspace_against_their_definitions(recorded, tmp_path):
    """tests/host/conv_plan_check.cpp under the address and undefined-behaviour sanitizers (the host program alone; the sanitizer runtimes are
    linked statically, so that the program runs whatever else the process environment loads)."""
    descs, _, _, ws = recorded
    listing = tmp_path / 'descriptors.txt'
    np.savetxt(listing, np.concatenate([descs.astype(np.int64), ws[:, :1]], axis=1), fmt='%d')
    cxx = _host_compiler()
    gnu = 'clang' not in subprocess.run([cxx, '--version'], stdout=subprocess.PIPE, text=True).stdout
    exe = tmp_path / 'conv_plan_check'
    cmd = [cxx, '-std=c++17', '-O2', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    cmd += ['-static-libasan', '-static-libubsan'] if gnu else ['-static-libsan']
    res = subprocess.run(cmd + [os.path.join(ROOT, 'tests', 'host', 'conv_plan_check.cpp'), '-o', str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    res = subprocess.run([str(exe), str(listing)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    m = re.search(r'(\d+) lattice configurations, (\d+) workspaces', res.stdout)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) == int((ws[:, 0] >= 0).sum()), res.stdout
