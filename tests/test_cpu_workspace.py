"""The workspace carver (csrc/gd3d_workspace.h) and the two header-only carves built on it (csrc/simota_common.h,
csrc/rpn_proposal_common.h) without a GPU: a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carves_stay_inside_their_own_size_under_the_sanitizers(tmp_path):
    """tests/hostmath/workspace_carve.cpp (its own main) compiled with -fsanitize=address,undefined and run as a program on the CPU:
    every carve sized at address 0, a heap block of exactly that size carved at every base misalignment 0..255 (self-aligning
    contract) or at an aligned base (caller-aligned contract), every buffer written in full: 256-byte aligned, inside the block, no
    byte shared.  A sanitizer build belongs on a CPU-only machine: with a GPU present the test skips before it compiles anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    from mmdet3d_gaussian_amd import _lib
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'workspace_carve')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           os.path.join(ROOT, 'tests', 'hostmath', 'workspace_carve.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
