"""Hard voxelization, dynamic voxelization and the mean voxel encoder on the CPU (csrc/hard_voxel_cpu.cpp, the `_cpu` twins): every
named case of tests/hard_voxel_ref.py against the numpy fp32 restatement of the sequential walk, EXACTLY — every output is an
integer, a copy, or the fixed-order mean, so there is no tolerance anywhere; the wrappers' list and stacked forms; `pvrcnn_voxelize`
against the reference's `voxelize` loop written out with the restated op; the `Voxelization` mode switch; the argument checks; and the
twins under sanitizers as a stand-alone program.  tests/test_gpu_hard_voxel.py runs the same helpers on the device."""
import os
import subprocess

import numpy as np
import pytest
import torch

import hard_voxel_ref as ref
import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd import _lib, voxelize

OUTPUTS = ('voxels', 'mean', 'coors', 'num_points', 'voxel_batch_cnt', 'num')


def case_of(name):
    return ref.sweep_case() if name == 'sweep' else ref.CASES[name]


def stacked(case, dev):
    """the case's samples as the op takes them in stacked form: rows (N, C) — a `[:, :C]` view of a wider tensor when the case pads —
    and the counts"""
    rows = np.concatenate(case['samples'], 0)
    t = torch.from_numpy(rows).to(dev)
    cnt = torch.tensor([len(s) for s in case['samples']], dtype=torch.int32, device=dev)
    return (t[:, :case['C']] if case['pad'] else t), cnt


def run_static(case, dev, with_voxels=True):
    """the one call, upper-bound outputs and `num` included -> dict of numpy arrays"""
    pts, cnt = stacked(case, dev)
    assert pts.stride(0) == case['C'] + case['pad'] or pts.size(0) == 0
    pts, cnt = voxelize._stacked(pts, cnt, 'test')
    assert pts.stride(0) == case['C'] + case['pad'] or pts.size(0) == 0, 'a row-strided view is read where it lies'
    out = voxelize._launch(pts, cnt, case['voxel_size'], case['point_cloud_range'], case['P'], case['MV'], case['F'], with_voxels, True)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def check_case(name, dev):
    """every output of the static call equals the restatement bit for bit, tail rows included; returns the outputs"""
    got, want = run_static(case_of(name), dev), ref.expected(name)
    for k in OUTPUTS:
        assert ref.same_bits(got[k], want[k]), f'{name}: {k} differs from the restatement on {dev}'
    V = int(want['num'][0])
    assert (got['coors'][V:] == -1).all() and (got['num_points'][V:] == 0).all() and not got['voxels'][V:].any() and not got['mean'][V:].any()
    return got


def check_dynamic(name, dev):
    case = case_of(name)
    pts, cnt = stacked(case, dev)
    got = amd.dynamic_voxelize(pts, case['voxel_size'], case['point_cloud_range'], cnt)
    assert got.dtype == torch.int32 and ref.same_bits(got.cpu().numpy(), ref.expected(name)['dynamic']), name
    return got


def check_mean_without_voxels(name, dev):
    case = case_of(name)
    lean, full = run_static(case, dev, with_voxels=False), ref.expected(name)
    assert lean['voxels'] is None
    for k in OUTPUTS[1:]:
        assert ref.same_bits(lean[k], full[k]), f'{name}: {k} without voxels'


def check_voxel_mean(name, dev):
    """the encoder alone on the restatement's voxels gives the restatement's mean bits"""
    case, want = case_of(name), ref.expected(name)
    got = amd.HardSimpleVFE(case['F'])(torch.from_numpy(want['voxels'].copy()).to(dev), torch.from_numpy(want['num_points'].copy()).to(dev), None)
    assert ref.same_bits(got.cpu().numpy(), want['mean']), name


def check_public_forms(name, dev):
    """hard_voxelize's list form, stacked form and static form agree, sliced to V"""
    case, want = case_of(name), ref.expected(name)
    V = int(want['num'][0])
    pts, cnt = stacked(case, dev)
    args = (case['voxel_size'], case['point_cloud_range'], case['P'], case['MV'])
    a = amd.hard_voxelize(pts, *args, points_batch_cnt=cnt, num_features=case['F'], with_mean=True)
    split = list(torch.split(pts, [len(s) for s in case['samples']]))
    b = amd.hard_voxelize(split, *args, num_features=case['F'], with_mean=True)
    s = amd.hard_voxelize(split, *args, num_features=case['F'], with_mean=True, static=True)
    for x, y, z, k in zip(a, b, s, ('voxels', 'coors', 'num_points', 'voxel_batch_cnt', 'mean')):
        full = want[k] if k == 'voxel_batch_cnt' else want[k][:V]
        assert ref.same_bits(x.cpu().numpy(), full) and ref.same_bits(y.cpu().numpy(), full) and ref.same_bits(z.cpu().numpy(), want[k]), (name, k)
    assert a[1].dtype == torch.int32 and a[2].dtype == torch.int32 and a[3].dtype == torch.int32 and a[0].shape[1:] == (case['P'], case['C'])


def reference_voxelize_loop(points, layer):
    """PVRCNN.voxelize (pv_rcnn.py:66-86) written out: the voxel layer per sample, cat, one F.pad per sample"""
    voxels, coors, num_points = [], [], []
    for res in points:
        v, c, n = layer(res)
        voxels.append(v); coors.append(c); num_points.append(n)
    coors_batch = [torch.nn.functional.pad(c, (1, 0), mode='constant', value=i) for i, c in enumerate(coors)]
    return dict(voxels=torch.cat(voxels, 0), num_points=torch.cat(num_points, 0), coors=torch.cat(coors_batch, 0))


class RestatedLayer:
    """mmdet3d's Voxelization of one sample, through the numpy restatement"""

    def __init__(self, cfg, training):
        self.cfg, self.mv = cfg, cfg['max_voxels'][0 if training else 1]

    def __call__(self, pts):
        o = ref.hard_voxelize_ref([pts.cpu().numpy()], self.cfg['voxel_size'], self.cfg['point_cloud_range'], self.cfg['max_num_points'],
                                  self.mv, pts.size(1), pts.size(1))
        V = int(o['num'][0])
        return torch.from_numpy(o['voxels'][:V]), torch.from_numpy(o['coors'][:V, 1:]), torch.from_numpy(o['num_points'][:V])


def check_pvrcnn_voxelize(dev):
    cfg = dict(max_num_points=5, point_cloud_range=list(ref.KITTI['point_cloud_range']), voxel_size=list(ref.KITTI['voxel_size']),
               max_voxels=(60, 90))
    rng = np.random.default_rng(3)
    points = [torch.from_numpy(ref._inside(rng, n, ref.KITTI, margin=0.02) * np.array([0.05, 0.05, 1, 1], np.float32)) for n in (300, 0, 150)]
    for training in (True, False):
        want = reference_voxelize_loop(points, RestatedLayer(cfg, training))
        got = amd.pvrcnn_voxelize([p.to(dev) for p in points], cfg, training)
        assert got['batch_size'] == 3 and set(got) == {'voxels', 'num_points', 'coors', 'voxel_features', 'batch_size'}
        for k in ('voxels', 'num_points', 'coors'):
            assert ref.same_bits(got[k].cpu().numpy(), want[k].numpy()), (k, training)
        vfe = want['voxels'].numpy()
        acc = np.zeros((len(vfe), 4), np.float32)
        for k in range(5):
            acc = acc + vfe[:, k]                    # zero padding adds nothing: the sequential sum of the filled slots
        assert ref.same_bits(got['voxel_features'].cpu().numpy(), acc / want['num_points'].numpy()[:, None].astype(np.float32)), training
    assert int(got['coors'][:, 0].max()) == 2 and got['voxels'].size(0) == 90 + 0 + 90     # both samples hit the test limit


def check_voxelization_module(dev):
    """mmdet3d's surface: one sample in, (voxels, coors (V, 3) zyx, num_points) out; the (train, test) pair follows .train() / .eval();
    -1 routes to the dynamic coors"""
    case, want = ref.CASES['voxel_cut_mv16'], ref.expected('voxel_cut_mv16')
    pts = torch.from_numpy(case['samples'][0]).to(dev)
    layer = amd.Voxelization(case['voxel_size'], case['point_cloud_range'], case['P'], max_voxels=(16, 1000), deterministic=False)
    assert layer.grid_size.tolist() == [16, 16, 4] and layer.pcd_shape == [16, 16, 1]
    layer.train()
    v, c, n = layer(pts)
    assert v.shape == (16, 3, 4) and ref.same_bits(c.cpu().numpy(), want['coors'][:16, 1:]) and ref.same_bits(v.cpu().numpy(), want['voxels'][:16])
    assert ref.same_bits(n.cpu().numpy(), want['num_points'][:16])
    layer.eval()
    v, c, n = layer(pts)
    assert v.shape == (40, 3, 4) and c.shape == (40, 3)
    one = ref.hard_voxelize_ref(case['samples'][:1], case['voxel_size'], case['point_cloud_range'], 3, 1000, 4, 4)
    assert ref.same_bits(v.cpu().numpy(), one['voxels'][:40]) and ref.same_bits(c.cpu().numpy(), one['coors'][:40, 1:])
    dyn = ref.dynamic_voxelize_ref(case['samples'][:1], case['voxel_size'], case['point_cloud_range'])[:, 1:]
    for kwargs in (dict(max_num_points=-1, max_voxels=(-1, -1)), dict(max_num_points=-1, max_voxels=20000), dict(max_num_points=3, max_voxels=-1)):
        got = amd.Voxelization(case['voxel_size'], case['point_cloud_range'], **kwargs)(pts)
        assert isinstance(got, torch.Tensor) and ref.same_bits(got.cpu().numpy(), dyn)
    faces = torch.from_numpy(ref.CASES['faces_and_non_finite']['samples'][0]).to(dev)
    got = amd.Voxelization(case['voxel_size'], case['point_cloud_range'], -1, -1)(faces)
    assert ref.same_bits(got.cpu().numpy(), ref.expected('faces_and_non_finite')['dynamic'][:len(faces), 1:])


def check_irregular_counts(dev):
    """counts that overrun the stack, and a negative count with rows left over: a negative count owns nothing, a sample owns no row
    past the stack, and rows of no sample are dropped (counted in num[1], -1 in the dynamic coors)"""
    case = ref.CASES['voxel_cut_mv16']
    rows = np.concatenate(case['samples'], 0)                              # 150 rows
    pts = torch.from_numpy(rows).to(dev)
    n = len(rows)
    for counts, owned in (([60, 60, 60], [(0, 60), (60, 120), (120, n)]), ([50, -3, 40], [(0, 50), (50, 50), (50, 90)])):
        samples = [rows[a:b] for a, b in owned]
        want = ref.hard_voxelize_ref(samples, case['voxel_size'], case['point_cloud_range'], 3, 12, 4, 4)     # 3 x 12 rows < the points owned
        left = n - owned[-1][1]
        cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
        out = voxelize._launch(pts, cnt, case['voxel_size'], case['point_cloud_range'], 3, 12, 4, True, True)
        for k in OUTPUTS[:-1]:
            assert ref.same_bits(out[k].cpu().numpy(), want[k]), (counts, k)
        assert out['num'].tolist() == [int(want['num'][0]), int(want['num'][1]) + left], counts
        dyn = amd.dynamic_voxelize(pts, case['voxel_size'], case['point_cloud_range'], cnt).cpu().numpy()
        want_dyn = ref.dynamic_voxelize_ref(samples, case['voxel_size'], case['point_cloud_range'])
        assert ref.same_bits(dyn[:n - left], want_dyn) and (dyn[n - left:] == -1).all(), counts


# ---- the tests ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_hard_voxelize_twin_equals_the_restatement(name):
    check_case(name, 'cpu')
    check_mean_without_voxels(name, 'cpu')


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_dynamic_voxelize_and_the_encoder_alone_equal_the_restatement(name):
    check_dynamic(name, 'cpu')
    check_voxel_mean(name, 'cpu')


def test_sweep_case_equals_the_restatement():
    check_case('sweep', 'cpu')


def test_the_cases_hold_what_they_claim():
    """the generators' own conditions: the cuts cut, the faces fall where the issue says, the keys pass 32 bits"""
    e = ref.expected
    for P in (1, 5, 32):
        n = e(f'slot_cut_p{P}')['num_points']
        assert sorted(n[n > 0].tolist()) == sorted(([P - 1] if P > 1 else []) + [P, P, P, P])                 # P-1, P, P+1 -> P, 3P -> P, 2P+1 -> P
    cut = e('voxel_cut_mv16')
    assert cut['voxel_batch_cnt'].tolist() == [16, 10] and cut['num'].tolist() == [26, 0]
    assert int(cut['num_points'][:16].sum()) > 16, 'later points joined kept voxels after the limit was reached'
    assert int(cut['num_points'][:16].sum()) < len(ref.CASES['voxel_cut_mv16']['samples'][0]), 'points of cut cells were skipped'
    assert e('voxel_cut_mv1')['voxel_batch_cnt'].tolist() == [1, 1]
    faces = e('faces_and_non_finite')['dynamic'][:27]
    kept = (faces[:, 0] >= 0).reshape(3, 9)
    # lo, hi, one ulp below hi, one ulp below lo, nan, +-inf, +-1e30.  On x (lo = 0) the subtraction is exact and the point one ulp below hi
    # lies in the last cell; on y (lo = -4) and z (lo = -2) the fp32 subtraction p - lo rounds that point up to the full span (a tie, to
    # even), the quotient is the grid size, and the point is dropped: the stated operation order decides, here as in mmdet3d
    assert kept.tolist() == [[True, False, True] + [False] * 6] + [[True] + [False] * 8] * 2
    assert faces[0, 3] == 0 and faces[2, 3] == 15 and faces[9, 2] == 0 and faces[18, 1] == 0                    # cell 0 at lo, the last cell below hi
    assert ref.grid_of(**ref.KITTI) == (1408, 1600, 40) and amd.voxelize.grid_size(**ref.KITTI) == (1408, 1600, 40)
    assert e('kitti_rounded_grid')['num'][1] >= 3
    assert 50 * 1408 * 1600 * 40 > 2 ** 32 and e('keys_past_32_bits')['voxel_batch_cnt'].tolist() == [8] * 50
    assert e('every_point_dropped')['num'].tolist() == [0, 42] and e('n0')['num'].tolist() == [0, 0]
    assert e('three_samples_middle_empty')['voxel_batch_cnt'][1] == 0
    d = e('duplicates')
    assert d['num_points'][0] == 5 and ref.same_bits(d['voxels'][0, 0], d['voxels'][0, 4])


@pytest.mark.parametrize('name', ['three_samples_middle_empty', 'voxel_cut_mv16', 'trailing_columns_c4', 'num_features_3_of_4', 'n0', 'every_point_dropped'])
def test_list_stacked_and_static_forms_agree(name):
    check_public_forms(name, 'cpu')


def test_pvrcnn_voxelize_equals_the_reference_loop():
    check_pvrcnn_voxelize('cpu')


def test_voxelization_module_mode_switch_and_dynamic_route():
    check_voxelization_module('cpu')


def test_counts_that_overrun_the_stack_and_negative_counts():
    check_irregular_counts('cpu')


def test_other_dtypes_and_strides():
    case, want = ref.CASES['n65'], ref.expected('n65')
    pts = torch.from_numpy(case['samples'][0])
    args = (case['voxel_size'], case['point_cloud_range'], case['P'], case['MV'])
    got = amd.hard_voxelize(pts.double(), *args)                           # evaluated in fp32
    assert got[0].dtype == torch.float32 and ref.same_bits(got[0].numpy(), want['voxels'][:int(want['num'][0])])
    got = amd.hard_voxelize(pts.t().contiguous().t(), *args)               # a column-major view takes one copy
    assert ref.same_bits(got[1].numpy(), want['coors'][:int(want['num'][0])])
    p = pts.clone().requires_grad_(True)
    assert not amd.hard_voxelize(p, *args)[0].requires_grad                # no gradient


def test_argument_errors_raise():
    pts = torch.from_numpy(ref.CASES['n65']['samples'][0])
    vs, rng = ref.SMALL['voxel_size'], ref.SMALL['point_cloud_range']
    bad = [lambda: amd.hard_voxelize(pts, vs, rng, 0, 10), lambda: amd.hard_voxelize(pts, vs, rng, 5, 0),
           lambda: amd.hard_voxelize(pts, vs[:2], rng, 5, 10), lambda: amd.hard_voxelize(pts, vs, rng[:5], 5, 10),
           lambda: amd.hard_voxelize(pts, (0.5, 0.0, 1.0), rng, 5, 10), lambda: amd.hard_voxelize(pts, vs, (0, 0, 0, 8, -1, 4), 5, 10),
           lambda: amd.hard_voxelize(pts[:, :2], vs, rng, 5, 10), lambda: amd.hard_voxelize(pts.long(), vs, rng, 5, 10),
           lambda: amd.hard_voxelize(pts[0], vs, rng, 5, 10), lambda: amd.hard_voxelize([], vs, rng, 5, 10),
           lambda: amd.hard_voxelize([pts, pts[:, :3]], vs, rng, 5, 10), lambda: amd.hard_voxelize([pts], vs, rng, 5, 10, points_batch_cnt=torch.tensor([65])),
           lambda: amd.hard_voxelize(pts, vs, rng, 5, 10, points_batch_cnt=torch.tensor([65.0])),
           lambda: amd.hard_voxelize(pts, vs, rng, 5, 10, with_mean=True, num_features=5), lambda: amd.hard_voxelize(pts, vs, rng, 5, 10, with_voxels=False),
           lambda: amd.hard_voxelize(pts, (1e-7, 0.5, 1.0), rng, 5, 10), lambda: amd.dynamic_voxelize(pts[:, :2], vs, rng),
           lambda: amd.voxel_mean(torch.zeros(3, 5, 4), torch.zeros(2, dtype=torch.int32)), lambda: amd.voxel_mean(torch.zeros(3, 5, 4), torch.zeros(3)),
           lambda: amd.HardSimpleVFE(5)(torch.zeros(3, 5, 4), torch.zeros(3, dtype=torch.int32), None),
           lambda: amd.Voxelization(vs, rng, 5, (1, 2, 3)), lambda: amd.pvrcnn_voxelize(pts, dict(), True)]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f'call {i} did not raise')
    lib = _lib.load()                                                      # the C entry points' own codes: nothing is touched
    size, low, i3 = np.array(vs, np.float32), np.array(rng[:3], np.float32), np.array([16, 16, 4], np.int32)
    common = lambda n, b, g: (None, n, 4, 4, None, b, size.ctypes.data, low.ctypes.data, g.ctypes.data)
    tail = (None,) * 7
    assert lib.gd3d_hard_voxelize_cpu(*common(1 << 31, 1, i3), 5, 10, 4, *tail) == 10002                          # N > 2^31 - 1
    assert lib.gd3d_hard_voxelize_cpu(*common(8, 1024, np.array([1 << 24] * 3, np.int32)), 5, 10, 4, *tail) == 10002    # B * G >= 2^62
    assert lib.gd3d_hard_voxelize_cpu(*common(8, 1, np.array([(1 << 24) + 1, 4, 4], np.int32)), 5, 10, 4, *tail) == 10002
    num = np.zeros(2, np.int64)
    assert lib.gd3d_hard_voxelize_cpu(*common(8, 1, i3), 0, 10, 4, *tail[:6], num.ctypes.data) == 10001          # max_num_points < 1
    assert lib.gd3d_hard_voxelize_cpu(*common(8, 1, i3), 5, 0, 4, *tail[:6], num.ctypes.data) == 10001           # max_voxels < 1
    assert lib.gd3d_hard_voxelize_workspace_bytes(0, 1, 10) == 256 and lib.gd3d_hard_voxelize_workspace_bytes(80000, 4, 16000) % 256 == 0
    for name in ('hard_voxelize', 'dynamic_voxelize', 'Voxelization', 'HardSimpleVFE', 'voxel_mean', 'pvrcnn_voxelize'):
        assert name in amd.__all__


def test_host_twins_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/hard_voxel_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/hard_voxel_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap buffers over the face and the cut cases.  The device
    kernels share the cell code.  A sanitizer build belongs on a CPU-only machine: with a GPU present the test skips before it compiles
    or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'hard_voxel_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all', '-ffp-contract=off',
           os.path.join(root, 'tests', 'hostmath', 'hard_voxel_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'hard_voxel_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
