"""CPU side of tests/test_gpu_ref_kernels.py: the recipe that compiles the reference's device kernels (oracle/Makefile targets
`ref_vsa`, `ref_vox`) builds from nothing, exports what the driver (oracle/ref_kernels.py) calls and leaves nothing else behind; the
cases hold what they name (asserted when tests/ref_kernel_cases.py is imported); the product's `_cpu` twins agree with the
restatement on them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle
from oracle import ref_kernels as rk

REF = '/root/reference'


@pytest.mark.skipif(not os.path.isdir(REF), reason='the reference tree is absent: nothing to compile the reference kernels from')
def test_recipe_builds_both_libraries_from_a_clean_directory(tmp_path):
    out = tmp_path / '_ref'
    run = subprocess.run(['make', '-C', oracle.HERE, 'ref_vsa', 'ref_vox', f'OUT={out}'], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert sorted(os.listdir(out)) == ['ref_vox.so', 'ref_vsa.so']                      # the shared objects and nothing else
    lib = ctypes.CDLL(str(out / 'ref_vsa.so'))
    for name in rk.VSA_ENTRIES:
        assert getattr(lib, name) is not None                                          # every extern "C" entry resolves
    exported = subprocess.run(['nm', '-D', '--defined-only', str(out / 'ref_vox.so')], capture_output=True, text=True).stdout
    assert 'PyInit_ref_vox' in exported
    # what build() left in the tree: shared objects only, no copy of the reference's text, translated or not
    shipped = os.path.join(oracle.HERE, '_ref')
    if os.path.isdir(shipped):
        assert all(f.endswith('.so') for f in os.listdir(shipped)), os.listdir(shipped)


@pytest.mark.skipif(not os.path.isdir(REF), reason='the reference tree is absent: nothing to compile the reference kernels from')
def test_built_tree_loads_both_libraries():
    oracle.build()
    assert oracle.ref_vsa_path() and oracle.ref_vox_path()
    assert rk.load_vsa() is not None
    mod = rk.load_vox()
    assert mod is not None and all(hasattr(mod, name) for name in rk.VOX_ENTRIES)
    assert [rk.fps_block(n) for n in (1, 2, 3, 63, 64, 65, 1000, 1023, 1024, 1025, 5000, 16385)] == \
        [1, 2, 2, 32, 64, 64, 512, 512, 1024, 1024, 1024, 1024]


def test_driver_refuses_what_the_kernels_would_not_survive():
    """the host-side checks are the only bounds the reference kernels have"""
    ok = np.array([[0, 1], [2, 0], [0, 0]])
    rk._idx_in_samples(ok, np.array([2, 0, 1]), np.array([3, 0, 1]), 'idx')
    for bad, icnt, fcnt in ((np.array([[0, 3]]), [1], [3]), (np.array([[-1, 0]]), [1], [3]), (np.array([[0, 0]]), [0, 1], [5, 0])):
        with pytest.raises(AssertionError):
            rk._idx_in_samples(bad, np.array(icnt), np.array(fcnt), 'idx')
    with pytest.raises(AssertionError):
        rk._dev(torch.zeros(3, 3), torch.float32, (3, 3), 'a CPU tensor')


def test_twins_agree_with_the_restatement_on_the_cases():
    """the cases assert themselves at import; here the `_cpu` twins meet the restatement on them, so that a GPU failure in
    tests/test_gpu_ref_kernels.py is a statement about the reference kernel or the device, not about the case"""
    import mmdet3d_gaussian_amd as amd
    import ref_kernel_cases as cases
    t = torch.from_numpy
    xyz, new_xyz = (t(np.array(a)) for a in cases.bq_cloud())
    pc, qc = t(cases.BQ_POINTS.copy()), t(cases.BQ_QUERIES.copy())
    for ns in cases.BQ_NSAMPLE:
        idx, mask = amd.ball_query(cases.bq_radius(ns), ns, xyz, pc, new_xyz, qc)
        want = cases.bq_reference(ns)
        assert np.array_equal(idx.numpy(), want[0]) and np.array_equal(mask.numpy(), want[2])
    for n in cases.FPS_SMALL + cases.FPS_LARGE:
        m = max(cases.fps_npoints(n))
        assert np.array_equal(amd.furthest_point_sample(t(np.array(cases.fps_cloud(n))), m).numpy(), cases.fps_reference(n)[0])
    assert np.array_equal(amd.furthest_point_sample(t(np.array(cases.fps_tied())), cases.FPS_TIED_NPOINT).numpy()[0],
                          cases.fps_tied_reference()[0])
    s = cases.vq_scene()
    index = amd.voxel_query_index(t(s['coors']), cases.VQ_SHAPE, cases.VQ_B)
    for r in cases.VQ_RANGES:
        for ns in cases.VQ_NSAMPLE:
            idx, mask = amd.voxel_query(r, cases.vq_radius(r, ns), ns, t(s['xyz']), t(s['new_xyz']), t(s['new_coords']), index)
            want = cases.vq_reference(r, ns)
            assert np.array_equal(idx.numpy(), want['idx']) and np.array_equal(mask.numpy(), want['mask'])
