"""The `_cpu` twins of the voxel query ops (csrc/voxel_query_cpu.cpp) against the numpy restatement of tests/voxel_query_ref.py: the
cases of tests/voxel_query_cases.py, every comparison an exact equality.  No GPU needed; tests/test_gpu_voxel_query.py runs the same
cases on the kernels."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd

import voxel_query_cases as cases

CPU = torch.device('cpu')
CHANNELS = [(c, u) for c in (0, 1, 3, 16, 17, 64, 67) for u in (True, False) if c > 0 or u]


def test_surface():
    for name in ('voxel_query_index', 'voxel_point_indices', 'voxel_query_coords', 'voxel_query', 'VoxelQueryIndex', 'VoxelQueryAndGroup'):
        assert name in amd.__all__ and hasattr(amd, name)
    assert amd.load_library().gd3d_vsa_voxel_index_workspace_bytes(1000) % 256 == 0


@pytest.mark.parametrize('coors_dtype', [torch.int32, torch.int64], ids=['i32', 'i64'])
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_query_matches_the_restatement(name, coors_dtype):
    cases.check_query_case(amd, name, CPU, coors_dtype)


@pytest.mark.parametrize('C,use_xyz', CHANNELS)
def test_grouped_block_matches_the_restatement(C, use_xyz):
    cases.check_group_case(amd, 'w63', CPU, C, use_xyz)


def test_grouped_block_at_nsample_1024():
    cases.check_group_case(amd, 'ns1024', CPU, 3, True)


def test_query_coords():
    cases.check_coords(amd, CPU)


def test_a_callers_table_with_garbage():
    cases.check_garbage_table(amd, CPU)


def test_member_sets_equal_ball_querys():
    cases.check_against_ball_query(amd, CPU)


def test_inclusive_where_ball_query_is_strict():
    cases.check_inclusive_vs_ball_query(amd, CPU)


def test_entries_write_every_element_and_nothing_else():
    cases.check_entries_write_everything_and_nothing_else(amd, CPU)


def test_backward():
    cases.check_backward(amd, CPU)


def test_other_float_dtypes_are_evaluated_in_fp32():
    scene, calls, results = cases.case('w27')
    rng_, radius, nsample = calls[0]
    t = cases.t
    index = amd.voxel_query_index(t(scene.coors, CPU, torch.int32), scene.shape, scene.B)
    feats = torch.randn(len(scene.xyz), 5, dtype=torch.float64)
    mod = amd.VoxelQueryAndGroup(rng_, radius, nsample)
    out, idx = mod(t(scene.xyz, CPU).double(), t(scene.new_xyz, CPU).double(), t(scene.new_coords, CPU).long(), index, feats)
    want, _ = mod(t(scene.xyz, CPU), t(scene.new_xyz, CPU), t(scene.new_coords, CPU), index, feats.float())
    assert out.dtype == torch.float64 and torch.equal(out, want.double())
    cases.same(idx, results[0]['idx'], 'idx')


def test_empty_sizes():
    cases.check_empty_sizes(amd, CPU)


def test_argument_errors():
    cases.check_argument_errors(amd, CPU)


def test_host_twins_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/voxel_query_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/voxel_query_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap buffers, `coors` and query cells at the ends of
    their types, a table of garbage, NaN, +-inf and 1e30 points.  The device kernels share that window, key and cell code.  A sanitizer
    build belongs on a CPU-only machine: with a GPU present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    import os
    import subprocess
    from mmdet3d_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'voxel_query_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all', '-ffp-contract=off',
           '-pthread', os.path.join(root, 'tests', 'hostmath', 'voxel_query_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'voxel_query_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
