"""The pillar encoders' point decoration on the CPU (csrc/pillar_feat_cpu.cpp, the `_cpu` twins of `point_voxel_stats` and
`pillar_decorate`): against the RECORDED results of the reference's own modules (tests/golden/pillar_feat.npz), against the numpy
restatement of the fixed sequence (tests/pillar_feat_ref.py) on the named cases of tests/pillar_feat_cases.py, the input forms (views,
int64 rows, appended columns, `out=`), the modules, the argument checks, and the twins under sanitizers as a stand-alone program.
Exact equality everywhere except where the reference itself leaves the order of a sum open (`f_cluster`, against the float64
recording with a worst-case rounding bound) and for the distance (3 ulp).  tests/test_gpu_pillar_feat.py runs the same helpers on the
device."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import pillar_feat_cases as cases
import pillar_feat_ref as ref
import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd import _lib, pillar_feat

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pillar_feat.npz'))
FLAG_SETS = [dict(zip(ref.FLAG_NAMES, bits)) for bits in itertools.product((False, True), repeat=6)]
DECO_FLAGS = list(itertools.product((False, True), repeat=3))


def index_of(coors, dev):
    """what point_voxel_stats takes as its second argument on `dev`: a Scatter on the GPU, the rows on the CPU"""
    t = coors if isinstance(coors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(coors))
    t = t.to(dev)
    return amd.Scatter(t) if t.is_cuda else t


def run_stats(case, dev, cols=3, append=False, coors_dtype=None, **flags):
    pts = torch.from_numpy(case['points']).to(dev)[:, :cols]
    coors = torch.from_numpy(case['coors'])
    if coors_dtype is not None:
        coors = coors.to(coors_dtype)
    return amd.point_voxel_stats(pts, index_of(coors, dev), case['voxel_size'], case['point_cloud_range'], append_features=append, **flags)


def check_stats(name, dev, cols=3, append=False, coors_dtype=None, **flags):
    """the op on `dev` equals the numpy restatement bit for bit; returns the result"""
    case = cases.STATS[name]
    got = run_stats(case, dev, cols, append, coors_dtype, **flags)
    want = ref.stats_ref(case['points'][:, :cols], case['coors'], case['voxel_size'], case['point_cloud_range'], append_features=append, **flags)
    assert got.dtype == torch.float32 and got.device.type == torch.device(dev).type
    assert ref.same_bits(got.cpu().numpy(), want), f'{name}: differs from the restatement on {dev} ({flags}, cols={cols}, append={append})'
    return got


def run_deco(case, dev, flags=(True, True, False)):
    return amd.pillar_decorate(torch.from_numpy(case['features']).to(dev), torch.from_numpy(case['num_points']).to(dev),
                               torch.from_numpy(case['coors']).to(dev), case['voxel_size'], case['point_cloud_range'], *flags)


def check_deco(shape, dev, garbage=None):
    """all eight flag sets of one shape equal the restatement bit for bit; returns the last result"""
    case = cases.make_deco(*shape, garbage=garbage)
    for flags in DECO_FLAGS:
        got = run_deco(case, dev, flags)
        want = ref.decorate_ref(case['features'], case['num_points'], case['coors'], case['voxel_size'], case['point_cloud_range'], *flags)
        assert got.shape == want.shape and ref.same_bits(got.cpu().numpy(), want), f'{shape} {flags} garbage={garbage} on {dev}'
    return got


def check_views_and_forms(dev):
    """xyz as a strided view of (N, 4) and of (N, 5), 0 / 1 / 2 appended columns, int64 rows, `out=` at a column offset"""
    case = cases.STATS['three_samples_dropped']
    base = check_stats('three_samples_dropped', dev)
    p5 = torch.from_numpy(case['points']).to(dev)
    p4 = p5[:, :4].contiguous()
    idx = index_of(case['coors'], dev)
    geom = (case['voxel_size'], case['point_cloud_range'])
    for view in (p4[:, :3], p5[:, :3]):
        assert view.stride(0) in (4, 5) and not view.is_contiguous()
        assert torch.equal(amd.point_voxel_stats(view, idx, *geom), base)
    for cols in (3, 4, 5):
        got = check_stats('three_samples_dropped', dev, cols=cols, append=True)
        assert got.size(1) == 25 + cols - 3 and torch.equal(got[:, :25], base) and torch.equal(got[:, 25:], p5[:, 3:cols])
    check_stats('three_samples_dropped', dev, coors_dtype=torch.int64)
    check_stats('v75_unbatched', dev, coors_dtype=torch.int64, cols=4, append=True)
    # the KITTI dynamic config's 10 channels and a second "view" side by side in one preallocated tensor, no cat
    flags = dict(with_cluster_center=False, with_covariance=False, with_voxel_center=False, with_voxel_point_count=False)
    N = p5.size(0)
    wide = torch.full((N, 3 + 10 + 25 + 2), -77.0, device=dev)
    a = amd.point_voxel_stats(p4, idx, *geom, append_features=True, out=(wide, 3), **flags)
    b = amd.point_voxel_stats(p5[:, :3], idx, *geom, out=(wide, 13))
    assert a.data_ptr() == wide[:, 3:].data_ptr() and a.shape == (N, 10) and b.shape == (N, 25)
    assert torch.equal(wide[:, 13:38], base) and torch.equal(wide[:, 3:13], run_stats(case, dev, 4, True, **flags))
    assert (wide[:, :3] == -77.0).all() and (wide[:, 38:] == -77.0).all(), 'columns outside the op\'s were written'


def check_modules(dev):
    case = cases.STATS['sizes_1_to_9']
    xyz, idx = torch.from_numpy(case['points']).to(dev)[:, :3], index_of(case['coors'], dev)
    calc = amd.PointVoxelStatsCalculator(case['voxel_size'], case['point_cloud_range'], with_covariance=False, with_voxel_center=False)
    assert calc.out_channels == 13 and amd.PointVoxelStatsCalculator(case['voxel_size'], case['point_cloud_range']).out_channels == 25
    got = calc(xyz, idx)
    assert got.shape == (len(xyz), 13) and torch.equal(got, run_stats(case, dev, with_covariance=False, with_voxel_center=False))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        calc(torch.from_numpy(case['points']).to(dev)[:, :4], idx)
    deco = cases.make_deco(37, 33, 5)
    mod = amd.PillarFeatureDecorator(with_distance=True, voxel_size=deco['voxel_size'], point_cloud_range=deco['point_cloud_range'])
    assert mod.out_channels(5) == 12
    assert torch.equal(mod(*(torch.from_numpy(deco[k]).to(dev) for k in ('features', 'num_points', 'coors'))), run_deco(deco, dev, (True, True, True)))
    with pytest.raises(RuntimeError, match='legacy'):
        amd.PillarFeatureDecorator(legacy=True)


def f_cluster_bound(features, num_points):
    """(P + 2) * 2^-24 * max|x| over the voxel's filled slots, per voxel and channel: an n-term fp32 mean in any order plus one
    subtraction"""
    V, P, _ = features.shape
    valid = np.arange(P)[None, :] < np.minimum(num_points, P)[:, None]
    peak = np.where(valid[:, :, None], np.abs(features[:, :, :3].astype(np.float64)), 0.0).max(1)      # (V, 3)
    return (P + 2) * 2.0 ** -24 * peak


def check_decoration_against_statements(got, statements32, statements64, features, num_points, C):
    """`got` (cluster, centre, distance all on) against the torch statements evaluated in fp32 and in float64 on the same input: every
    channel but f_cluster bit for bit on filled slots and value-equal on padded ones; f_cluster within the rounding bound of the
    float64 result; the distance within 3 ulp"""
    V, P, _ = features.shape
    valid = np.arange(P)[None, :] < np.minimum(num_points, P)[:, None]
    exact = list(range(C)) + list(range(C + 3, C + 6))
    for ch in exact:
        assert ref.same_bits(got[..., ch][valid], statements32[..., ch][valid]), f'channel {ch} on filled slots'
    assert (got[~valid] == 0).all() and (statements32[~valid] == 0).all(), 'padded slots'
    assert not np.signbit(got[~valid]).any(), 'padded slots are +0'
    err = np.abs(got[..., C:C + 3].astype(np.float64) - statements64[..., C:C + 3])
    bound = f_cluster_bound(features, num_points)[:, None, :]
    print('f_cluster: largest error / bound =', float((err / np.maximum(bound, 1e-300))[valid].max()) if valid.any() else 0.0)
    assert (err <= bound)[valid].all(), 'f_cluster beyond (P + 2) * 2^-24 * max|x|'
    dist, dist64 = got[..., C + 6][valid], statements64[..., C + 6][valid]
    ulp = np.spacing(np.abs(dist64).astype(np.float32)).astype(np.float64)
    print('distance: largest error in ulp =', float((np.abs(dist - dist64) / ulp).max()) if valid.any() else 0.0)
    assert (np.abs(dist.astype(np.float64) - dist64) <= 3 * ulp).all(), 'distance beyond 3 ulp'


# ---- the tests ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['stats_a', 'stats_b'])
def test_stats_twin_equals_the_recorded_reference_bit_for_bit(name):
    """all 25 channels of the reference's own PointVoxelStatsCalculator.forward, run in fp32 over a sequential stand-in Scatter"""
    g = lambda k: GOLDEN[f'{name}.{k}']
    want = g('out32')
    assert want.dtype == np.float32 and want.shape[1] == 25
    got = amd.point_voxel_stats(torch.from_numpy(g('xyz')), torch.from_numpy(g('coors')), g('voxel_size').tolist(), g('point_cloud_range').tolist())
    assert ref.same_bits(got.numpy(), want)
    assert ref.same_bits(ref.stats_ref(g('xyz'), g('coors'), g('voxel_size').tolist(), g('point_cloud_range').tolist()), want), 'the restatement itself'
    assert np.abs(got.numpy().astype(np.float64) - g('out64')).max() < 1e-3           # the float64 run of the same statements is nearby
    got32 = amd.point_voxel_stats(torch.from_numpy(g('xyz')), torch.from_numpy(g('coors')).int(), g('voxel_size').tolist(), g('point_cloud_range').tolist())
    assert torch.equal(got32, got)


def test_stats_twin_equals_the_restatement_on_all_64_flag_sets():
    widths = set()
    for flags in FLAG_SETS:
        widths.add(check_stats('sizes_1_to_9', 'cpu', **flags).size(1))
    assert min(widths) == 3 and max(widths) == 25
    check_stats('three_samples_dropped', 'cpu', cols=5, append=True, **FLAG_SETS[0])      # no flag at all: a copy, one launch


@pytest.mark.parametrize('name', sorted(cases.STATS))
def test_stats_cases_equal_the_restatement(name):
    check_stats(name, 'cpu')
    check_stats(name, 'cpu', cols=5, append=True, with_cluster_center=False, with_covariance=False, with_voxel_center=False,
                with_voxel_point_count=False)


def test_the_cases_hold_what_they_claim():
    S = cases.STATS
    assert len(S['n0']['points']) == 0 and len(S['n1']['points']) == 1
    assert (S['every_point_dropped']['coors'] < 0).any(1).all() and [0, 5, -1, 2] in S['every_point_dropped']['coors'].tolist()
    _, counts, _ = ref.group(S['one_voxel_300']['coors'])
    assert counts.tolist() == [300]
    assert sorted(set(ref.group(S['sizes_1_to_9']['coors'])[1].tolist())) == [1, 2, 3, 4, 5, 7, 8, 9]
    pmap, counts, _ = ref.group(S['v75_unbatched']['coors'])
    N = len(pmap)
    assert len(counts) == 75 and 75 % 16 and 75 % 4 and (pmap < 0).sum() == 10 and N > 64 and (N * 25) % 256 and (N * 10) % 256
    c = S['three_samples_dropped']['coors']
    assert sorted(set(c[(c >= 0).all(1)][:, 0].tolist())) == [0, 1, 2] and [0, 5, -1, 2] in c.tolist() and [-1, -1, -1, -1] in c.tolist()
    out = ref.stats_ref(S['nonfinite']['points'], S['nonfinite']['coors'], S['nonfinite']['voxel_size'], S['nonfinite']['point_cloud_range'])
    pm = ref.group(S['nonfinite']['coors'])[0]
    poisoned = np.unique(pm[~np.isfinite(S['nonfinite']['points']).all(1) & (pm >= 0)])
    assert len(poisoned) == 4 and len(np.unique(pm[np.isnan(out[:, 3:6]).any(1) & (pm >= 0)])) == 2, 'a NaN point, and +inf with -inf'
    assert np.isfinite(out[~np.isin(pm, poisoned) & (pm >= 0)]).all(), 'a non-finite point reaches its own voxel only'
    assert not np.isfinite(out[np.isin(pm, poisoned)][:, 3:6]).all(1).any()
    far = S['near_1e4']['points'][:, :3]
    assert far.min() > 9999.9 and far.max() < 10000.1 and np.ptp(far, 0).max() < 0.06
    for shape in cases.DECO_SHAPES:
        n = cases.make_deco(*shape)['num_points']
        assert shape[0] < 3 or {0, shape[1], shape[1] + 2} <= set(n.tolist())


def test_views_appended_columns_int64_rows_and_out():
    check_views_and_forms('cpu')


def test_decoration_twin_against_the_recorded_reference():
    """PillarFeatureNet.forward's decoration as the reference computed it (PFN layers stubbed to identity), in fp32 and in float64"""
    g = lambda k: GOLDEN[f'deco_a.{k}']
    feats, num, coors = g('features'), g('num_points'), g('coors')
    got = amd.pillar_decorate(torch.from_numpy(feats), torch.from_numpy(num), torch.from_numpy(coors), g('voxel_size').tolist(),
                              g('point_cloud_range').tolist(), True, True, True).numpy()
    assert got.shape == g('out32').shape == (50, 9, 12)
    check_decoration_against_statements(got, g('out32'), g('out64'), feats, num, feats.shape[2])
    valid = np.arange(9)[None, :] < num[:, None]
    assert np.signbit(g('out32')[~valid]).any(), 'the reference\'s x * 0 mask leaves -0 in padded slots; the op writes +0'


@pytest.mark.parametrize('shape', cases.DECO_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_decoration_cases_equal_the_restatement(shape):
    check_deco(shape, 'cpu')


def test_decoration_ignores_what_lies_in_padded_slots():
    """finite garbage: zeros in the padded slots, as the reference's mask gives, and the filled slots as if the padding were zero
    (the reference's own sum would add the garbage into the mean: the op's contract is that padded input is not read); NaN garbage:
    zeros, where the reference's NaN * 0 gives NaN"""
    for shape in ((300, 5, 4), (37, 33, 5)):
        clean = check_deco(shape, 'cpu')
        for garbage in ('finite', 'nan'):
            got = check_deco(shape, 'cpu', garbage=garbage)
            assert torch.equal(got, clean) and not torch.isnan(got).any()
    case = cases.make_deco(300, 5, 4, garbage='finite')
    t = {k: torch.from_numpy(case[k]) for k in ('features', 'num_points', 'coors')}
    n = t['num_points'].clamp(max=5)
    want = ref.decorate_statements(t['features'], n, t['coors'], case['voxel_size'], case['point_cloud_range'], False, True, True)
    got = run_deco(case, 'cpu', (False, True, True))
    valid = (torch.arange(5)[None, :] < n[:, None])
    assert torch.equal(got[~valid], want[~valid] + 0.0) and (got[~valid] == 0).all()
    assert ref.same_bits(got[..., :7][valid].numpy(), want[..., :7][valid].numpy())


def test_modules():
    check_modules('cpu')


def test_other_dtypes_and_no_gradient():
    case = cases.STATS['sizes_1_to_9']
    base = run_stats(case, 'cpu')
    pts = torch.from_numpy(case['points'])[:, :3]
    coors = torch.from_numpy(case['coors'])
    geom = (case['voxel_size'], case['point_cloud_range'])
    assert torch.equal(amd.point_voxel_stats(pts.double(), coors, *geom), base)                     # evaluated in fp32
    assert torch.equal(amd.point_voxel_stats(pts.t().contiguous().t(), coors, *geom), base)         # a column-major view takes one copy
    assert torch.equal(amd.point_voxel_stats(pts, coors.to(torch.int16), *geom), base)
    assert not amd.point_voxel_stats(pts.clone().requires_grad_(True), coors, *geom).requires_grad
    deco = cases.make_deco(37, 33, 5)
    t = [torch.from_numpy(deco[k]) for k in ('features', 'num_points', 'coors')]
    want = run_deco(deco, 'cpu')
    assert torch.equal(amd.pillar_decorate(t[0].double(), t[1].long(), t[2].long(), deco['voxel_size'], deco['point_cloud_range']), want)
    assert not amd.pillar_decorate(t[0].clone().requires_grad_(True), t[1], t[2], deco['voxel_size'], deco['point_cloud_range']).requires_grad


def test_argument_errors_raise():
    case = cases.STATS['sizes_1_to_9']
    pts, coors = torch.from_numpy(case['points']), torch.from_numpy(case['coors'])
    vs, rng = case['voxel_size'], case['point_cloud_range']
    N = len(pts)
    f, n, c = (torch.from_numpy(v) for v in (lambda d: (d['features'], d['num_points'], d['coors']))(cases.make_deco(20, 64, 3)))
    bad = [lambda: amd.point_voxel_stats(pts[:, :2], coors, vs, rng), lambda: amd.point_voxel_stats(pts.long(), coors, vs, rng),
           lambda: amd.point_voxel_stats(pts, coors[:-1], vs, rng), lambda: amd.point_voxel_stats(pts, coors[:, :2], vs, rng),
           lambda: amd.point_voxel_stats(pts, coors.float(), vs, rng), lambda: amd.point_voxel_stats(pts, None, vs, rng),
           lambda: amd.point_voxel_stats(pts, coors, vs[:2], rng), lambda: amd.point_voxel_stats(pts, coors, vs, rng[:2]),
           lambda: amd.point_voxel_stats(pts, coors, vs, rng, out=(torch.zeros(N, 24), 0)),
           lambda: amd.point_voxel_stats(pts, coors, vs, rng, out=(torch.zeros(N, 30), 6)),
           lambda: amd.point_voxel_stats(pts, coors, vs, rng, out=(torch.zeros(N + 1, 30), 0)),
           lambda: amd.point_voxel_stats(pts, coors, vs, rng, out=(torch.zeros(N, 30, dtype=torch.float64), 0)),
           lambda: amd.point_voxel_stats(pts, coors, vs, rng, out=(torch.zeros(30, N).t(), 0)),
           lambda: amd.pillar_decorate(f[:, :, :2], n, c, vs, rng), lambda: amd.pillar_decorate(f[0], n, c, vs, rng),
           lambda: amd.pillar_decorate(f, n[:-1], c, vs, rng), lambda: amd.pillar_decorate(f, n.float(), c, vs, rng),
           lambda: amd.pillar_decorate(f, n, c[:, 1:], vs, rng), lambda: amd.pillar_decorate(f, n, c, vs[:1], rng),
           lambda: amd.pillar_decorate(f[:, :0], n, c, vs, rng)]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f'call {i} did not raise')
    lib = _lib.load()                                                      # the C entry points' own codes: nothing is touched
    g3 = np.ones(3, np.float32)
    stats = lambda n, stride, C, ndim, V, flags, ostride: lib.gd3d_point_voxel_stats_cpu(None, n, stride, C, None, 0, ndim, None, None, None, None, V,
                                                                                       g3.ctypes.data, g3.ctypes.data, flags, None, None, ostride)
    assert stats(8, 3, 3, 4, 2, 127, 25) == 10001                          # null operands with N > 0
    assert stats(8, 2, 3, 4, 2, 0, 3) == 10001 and stats(8, 3, 3, 2, 2, 0, 3) == 10001 and stats(8, 3, 3, 4, 9, 0, 3) == 10001
    assert stats(8, 3, 3, 4, 2, 128, 3) == 10001 and stats(8, 3, 3, 4, 2, 127, 24) == 10001
    assert stats(1 << 31, 3, 3, 4, 2, 0, 3) == 10002 and stats(8, 300, 300, 4, 2, 0, 3) == 10002 and stats(8, 3, 3, 9, 2, 0, 3) == 10002
    assert stats(0, 3, 3, 4, 0, 127, 25) == 0
    deco = lambda V, P, C, flags: lib.gd3d_pillar_decorate_cpu(None, None, None, V, P, C, g3.ctypes.data, g3.ctypes.data, flags, None)
    assert deco(4, 5, 4, 7) == 10001 and deco(4, 0, 4, 0) == 10001 and deco(4, 5, 2, 0) == 10001 and deco(4, 5, 4, 8) == 10001
    assert deco(1 << 31, 5, 4, 0) == 10002 and deco(4, 5, 300, 0) == 10002 and deco(4, 1 << 28, 4, 0) == 10002 and deco(0, 5, 4, 7) == 0
    for name in ('point_voxel_stats', 'PointVoxelStatsCalculator', 'pillar_decorate', 'PillarFeatureDecorator'):
        assert name in amd.__all__
    assert pillar_feat.stats_width(pillar_feat.stats_flags(append_features=True), 5) == 27


def test_host_twins_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/pillar_feat_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/pillar_feat_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap buffers over every flag set.  The device kernels
    share the per-element code.  A sanitizer build belongs on a CPU-only machine: with a GPU present the test skips before it compiles
    or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'pillar_feat_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all', '-ffp-contract=off',
           os.path.join(root, 'tests', 'hostmath', 'pillar_feat_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'pillar_feat_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
