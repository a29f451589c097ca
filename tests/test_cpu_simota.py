"""The SimOTA BEV assigner without a GPU: the `_cpu` twin (csrc/simota_cpu.cpp) against the numpy restatement of include/gd3d.h
(tests/simota_ref.py) — EXACT on every named case in the list, stacked and shared-prior forms — and against the outputs the
reference's own sim_ota_3d_assigner.py recorded (tests/golden/simota.npz); the error of the fixed-sequence logarithm; argument
errors and exported names; the prior generator against the reference's statements; the twin under the address and undefined-
behaviour sanitizers as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import simota_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('gt_inds', 'labels', 'max_overlaps', 'pos_cnt', 'pos_inds', 'pos_gt_inds')


def t(a, dev='cpu'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def call_forms(name, dev='cpu'):
    """-> [(form, result dict of numpy arrays, g_cap)] of a case through `simota_assign`'s forms"""
    case = ref.CASES[name]
    p = dict(case['params'])
    kw = dict(candidate_topk=p['topk'], center_radius=p.get('radius', 0.5), match_init=p.get('match_init', 2.0))
    s = case['samples']
    sc, bx, pr, gt, lb, pcnt, gcnt = ref.stacked(case)
    out = []
    lists = [[t(x[k], dev) for x in s] for k in ('scores', 'boxes')]
    priors = t(pr, dev) if case['shared'] else [t(x['priors'], dev) for x in s]
    r = amd.simota_assign(lists[0], lists[1], priors, [t(x['gts'], dev) for x in s], [t(x['labels'], dev) for x in s],
                          shared_priors=case['shared'], **kw)
    out.append(('list', {k: v.cpu().numpy() for k, v in r.items()}, int(gcnt.max())))
    r = amd.simota_assign(t(sc, dev), t(bx, dev), t(pr, dev), t(gt, dev), t(lb, dev), prior_batch_cnt=t(pcnt, dev), gt_batch_cnt=t(gcnt, dev),
                          shared_priors=case['shared'], **kw)
    out.append(('stacked', {k: v.cpu().numpy() for k, v in r.items()}, min(len(gt), 1024, 16384 // p['topk'])))
    return out


def same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        a, b = (got[k].view(np.uint32), want[k].view(np.uint32)) if k == 'max_overlaps' else (got[k], want[k])
        bad = np.nonzero((a != b).reshape(-1))[0]
        assert bad.size == 0, (what, k, bad[:8], got[k].reshape(-1)[bad[:8]], want[k].reshape(-1)[bad[:8]])


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_twin_equals_the_restatement_in_every_form(name):
    for form, got, g_cap in call_forms(name):
        same(got, ref.expected(name, g_cap), (name, form))


def test_cases_reach_what_they_are_named_for():
    """the oracle's own bookkeeping: conflicts whose row minimum is a third gt, costs tied at a k boundary, dynamic-k sums at an
    integer and a hair below it, V below K, empty samples, positives in every sized sample"""
    st = {}
    ref.expected('crowd', stats=st)
    assert st['conflicts'] >= 5 and st['third'] >= 1, st
    st = {}
    ref.expected('identical_gts', stats=st)
    e = ref.expected('identical_gts')
    assert st['conflicts'] == e['pos_cnt'][0] > 0 and set(e['gt_inds']) == {0, 1}, st
    st = {}
    e = ref.expected('all_clamped', stats=st)
    assert st['tie_at_k'] == 2 and e['pos_cnt'][0] > 0, st
    st = {}
    ref.expected('dynamic_k_edge', stats=st)
    assert st['sums'] == [2.0, float(np.nextafter(np.float32(2), np.float32(0))), float(np.nextafter(np.float32(2), np.float32(4)))], st['sums']
    assert list(ref.expected('dynamic_k_edge')['pos_cnt']) == [2 + 1 + 2]
    st = {}
    ref.expected('dense_queue', stats=st)
    assert len(st['cand'][0]) > 2 * 1024 + 256, len(st['cand'][0])
    e = ref.expected('few_candidates')
    assert 0 < e['pos_cnt'][0] <= 3
    e = ref.expected('empties')
    assert e['pos_cnt'][1] == e['pos_cnt'][2] == e['pos_cnt'][3] == 0 and e['pos_cnt'][0] > 0 and e['pos_cnt'][4] > 0
    st = {}
    ref.expected('faces', stats=st)       # on a face and exactly center_radius away: outside; the floats next inside: candidates
    assert list(st['cand'][0]) == [1, 4, 5, 7, 8], st['cand']
    for name in ('sizes_topk1', 'sizes_topk10', 'sizes_topk32', 'hostile', 'shared_grid'):
        e = ref.expected(name)
        assert (e['pos_cnt'] > 0).sum() >= 2, (name, e['pos_cnt'])


def test_device_counts_past_the_rows_are_clamped():
    """counts larger than the rows left, negative counts and rows past the counts' sum: what the clamped segments say"""
    case = ref.CASES['empties']
    sc, bx, pr, gt, lb, pcnt, gcnt = ref.stacked(case)
    for pc, gc in (([100, 50, 10 ** 6, 5], [3, -2, 10 ** 6, 1]), ([40, 40], [2, 2]), ([10 ** 9], [10 ** 9])):
        pc, gc = np.array(pc, np.int32), np.array(gc, np.int32)
        got = amd.simota_assign(t(sc), t(bx), t(pr), t(gt), t(lb), prior_batch_cnt=t(pc), gt_batch_cnt=t(gc))
        g_cap = min(len(gt), 1024)
        want = ref.assign_batch(sc, bx, pr, gt, lb, pc, gc, g_cap)
        same({k: v.numpy() for k, v in got.items()}, want, list(pc))


def _host_driver(tmp_path, sanitize):
    from mmdet3d_gaussian_amd import _lib
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'simota_sanitize')
    flags = ['-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all'] if sanitize else []
    cmd = [cxx, '-std=c++17', '-O1', '-g', *flags, '-ffp-contract=off', os.path.join(ROOT, 'tests', 'hostmath', 'simota_sanitize.cpp'),
           os.path.join(ROOT, 'mmdet3d-gaussian_amd', 'csrc', 'simota_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


FX_LOGF_WORST_ULP = 0.80     # the figure include/gd3d.h, csrc/fx_log.h and DESIGN.md §3.17 document


def test_fx_logf_error_against_fp64_and_the_host_libm(tmp_path):
    """2^20 log-uniform fp32 values of [1e-8, 2], every binade edge (the power of two, its two neighbours) and the 4096 values next
    below 1: fx_logf's worst error against fp64 log, in ulps of the correctly rounded result, is at most the host libm's logf's
    worst plus one ulp (a contraction-free polynomial loses about one rounding) and at most the documented figure.  The numpy
    restatement of tests/simota_ref.py gives the compiled sequence's bits."""
    rng = np.random.default_rng(0)
    x = np.exp(rng.uniform(np.log(1e-8), np.log(2.0), 1 << 20)).astype(np.float32)
    edges = np.float32(2.0) ** np.arange(-27, 2, dtype=np.float32)
    below = np.float32(1.0).view(np.uint32) - np.arange(1, 4097, dtype=np.uint32)
    x = np.concatenate([x, edges, np.nextafter(edges, np.float32(0)), np.nextafter(edges, np.float32(4)), below.view(np.float32)])
    x = x[(x >= np.float32(1e-8)) & (x <= np.float32(2.0))]
    exe = _host_driver(tmp_path, sanitize=False)
    x.tofile(str(tmp_path / 'x.bin'))
    subprocess.run([exe, 'logf', str(tmp_path / 'x.bin'), str(tmp_path / 'y.bin')], check=True, timeout=120)
    y = np.fromfile(str(tmp_path / 'y.bin'), np.float32)
    fx, libm = y[:len(x)], y[len(x):]
    want = np.log(x.astype(np.float64))
    ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
    ulp = np.where(want == 0, np.float64(np.spacing(np.float32(0))), ulp)
    e_fx, e_libm = np.abs(fx - want) / ulp, np.abs(libm - want) / ulp
    print(f'fx_logf worst {e_fx.max():.4f} ulp at {x[e_fx.argmax()]!r}; libm logf worst {e_libm.max():.4f} ulp; {len(x)} values')
    assert e_fx.max() <= e_libm.max() + 1.0
    assert e_fx.max() <= FX_LOGF_WORST_ULP
    assert np.array_equal(ref.fx_logf(x).view(np.uint32), fx.view(np.uint32))
    special = np.array([0.0, -0.0, np.inf, 1e-45, 1e-39, 1.0], np.float32)
    got = ref.fx_logf(special)
    assert got[0] == -np.inf and got[1] == -np.inf and got[2] == np.inf and got[5] == 0.0
    assert abs(got[3] - np.log(np.float64(special[3]))) < 1e-4 and abs(got[4] - np.log(np.float64(special[4]))) < 1e-4
    assert np.isnan(ref.fx_logf(np.array([-1.0, np.nan], np.float32))).all()


def test_argument_errors_and_exports():
    for n in ('simota_assign', 'SimOTABEVAssigner', 'Point3DRangeGenerator'):
        assert n in amd.__all__ and hasattr(amd, n)
    s = ref.CASES['few_candidates']['samples'][0]
    a = [t(s[k]) for k in ('scores', 'boxes', 'priors', 'gts', 'labels')]
    ok = amd.simota_assign([a[0]], [a[1]], [a[2]], [a[3]], [a[4]])
    assert ok['pos_inds'].shape == (1, 10) and ok['gt_inds'].dtype == torch.int64 and ok['pos_cnt'].dtype == torch.int32
    for bad in (dict(candidate_topk=0), dict(candidate_topk=33), dict(center_radius=float('nan'))):
        with pytest.raises(RuntimeError):
            amd.simota_assign([a[0]], [a[1]], [a[2]], [a[3]], [a[4]], **bad)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.simota_assign([a[0]], [a[1][:, :6]], [a[2]], [a[3]], [a[4]])
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.simota_assign([a[0]], [a[1]], [a[2][:-1]], [a[3]], [a[4]])
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.simota_assign([a[0]], [a[1]], [a[2]], [a[3]], [a[4].float()])
    with pytest.raises(RuntimeError, match='stacked tensors need'):
        amd.simota_assign(*a)
    with pytest.raises(RuntimeError, match='carry their own counts'):
        amd.simota_assign([a[0]], [a[1]], [a[2]], [a[3]], [a[4]], prior_batch_cnt=torch.tensor([40]))
    with pytest.raises(RuntimeError, match='gts'):
        amd.simota_assign([a[0]], [a[1]], [a[2]], [torch.zeros(1025, 7)], [torch.zeros(1025, dtype=torch.long)])
    with pytest.raises(RuntimeError, match='classes'):
        amd.simota_assign([torch.zeros(40, 33)], [a[1]], [a[2]], [a[3]], [a[4]])
    with pytest.raises(RuntimeError, match='debug'):
        amd.SimOTABEVAssigner(debug=True)
    # the C entry's own checks
    lib = amd.load_library()
    assert lib.gd3d_simota_workspace_bytes(1000, 4, 64, 10) >= 1000 * 4 + 3 * 4 * 64 * 10 * 4
    args = lambda **o: [None, None, None, o.get('rows', 0), o.get('stride', 2), 0, 256, 0, None, None, 256, 0, o.get('B', 1), o.get('C', 3),  # noqa: E731
                        o.get('G_cap', 0), 0.5, o.get('K', 10), 3.0, 1.0, 2.0, None, None, None, 256, None, None, None, 0]
    assert lib.gd3d_simota_assign_cpu(*args(B=0)) == 10001
    assert lib.gd3d_simota_assign_cpu(*args(stride=1)) == 10001
    assert lib.gd3d_simota_assign_cpu(*args(rows=5)) == 10001
    assert lib.gd3d_simota_assign_cpu(*args(K=33)) == 10002
    assert lib.gd3d_simota_assign_cpu(*args(C=33)) == 10002
    assert lib.gd3d_simota_assign_cpu(*args(G_cap=1025)) == 10002
    assert lib.gd3d_simota_assign_cpu(*args(G_cap=600, K=32)) == 10002
    assert lib.gd3d_simota_assign_cpu(*args(B=1025)) == 10002


def test_non_fp32_inputs_and_strided_priors():
    """fp64 / fp16 inputs are evaluated in fp32; priors are read through their strides (a (P, 4) tensor's first two columns)"""
    s = ref.CASES['few_candidates']['samples'][0]
    want = amd.simota_assign([t(s['scores'])], [t(s['boxes'])], [t(s['priors'])], [t(s['gts'])], [t(s['labels'])])
    wide = torch.cat([t(s['priors']), torch.full((len(s['priors']), 5), 9.0)], 1)[:, :4]
    got = amd.simota_assign([t(s['scores']).double()], [t(s['boxes']).double()], [wide], [t(s['gts']).double()], [t(s['labels']).int()])
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k


def test_assigner_class_follows_the_reference_surface():
    s = ref.CASES['identical_gts']['samples'][0]
    a = amd.SimOTABEVAssigner(center_radius=0.5, candidate_topk=10, iou_weight=3.0, dir_weight=0.0, cls_weight=1.0, match_init=2.0)
    r = a.assign(t(s['scores']), t(s['boxes']), t(s['priors']), t(s['gts']), gt_labels=t(s['labels']))
    e = ref.expected('identical_gts')
    assert r.num_gts == 2 and np.array_equal(r.gt_inds.numpy(), e['gt_inds']) and np.array_equal(r.labels.numpy(), e['labels'])
    assert np.array_equal(r.max_overlaps.numpy().view(np.uint32), e['max_overlaps'].view(np.uint32))
    assert a.assign(t(s['scores']), t(s['boxes']), t(s['priors']), t(s['gts'])).labels is None
    r = a.assign(t(s['scores']), t(s['boxes']), t(s['priors']), torch.zeros(0, 7), gt_labels=torch.zeros(0, dtype=torch.long))
    assert r.num_gts == 0 and not r.gt_inds.any() and not r.max_overlaps.any() and (r.labels == -1).all()


def test_point_3d_range_generator_equals_the_reference_statements():
    """core/anchor/point_3d_generator.py:28-47 evaluated with CPU torch"""
    ranges = [[0.0, -39.68, -3.0, 69.12, 39.68, 1.0], [-5.5, 1.25, 0.0, 7.75, 9.0, 0.0]]
    gen = amd.Point3DRangeGenerator(ranges, base=2)
    assert gen.num_levels == 2
    sizes = [(1, 31, 27), (5, 4)]
    got = gen.grid_priors(sizes, device='cpu')
    assert all(torch.equal(x, y) for x, y in zip(got, gen.grid_anchors(sizes, device='cpu')))
    for i, fs in enumerate(sizes):
        fs = [1, fs[0], fs[1]] if len(fs) == 2 else list(fs)
        r = torch.tensor(ranges[i])
        yc = torch.linspace(r[1], r[3], fs[1])
        xc = torch.linspace(r[0], r[2], fs[2])
        gx, gy = torch.meshgrid(xc, yc, indexing='ij')
        stride = torch.full_like(gx, (2 * (r[2] - r[0]) / (fs[2] - 1)).item())
        want = torch.stack((gx, gy, stride), dim=-1).permute((1, 0, 2)).contiguous()
        assert got[i].dtype == torch.float32 and got[i].shape == (fs[1], fs[2], 3) and torch.equal(got[i], want)
    with pytest.raises(AssertionError):
        gen.grid_priors([(4, 4)], device='cpu')


def test_golden_outputs_of_the_reference_assigner():
    """tests/golden/simota.npz: what the reference's own sim_ota_3d_assigner.py returned on the CPU (tests/golden/make_golden_simota.py:
    every recorded case keeps a margin at each k boundary, dynamic-k sum and conflict).  gt_inds and labels EXACTLY, max_overlaps to
    the bit, on every recorded case."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'simota.npz'))
    n = int(z['num_cases'])
    assert n >= 6
    for i in range(n):
        g = lambda k: z[f'c{i}_{k}']   # noqa: E731
        a = amd.SimOTABEVAssigner(center_radius=float(g('center_radius')), candidate_topk=int(g('candidate_topk')), iou_weight=float(g('iou_weight')),
                                  cls_weight=float(g('cls_weight')), match_init=float(g('match_init')))
        r = a.assign(t(g('pred_scores')), t(g('decoded_bboxes')), t(g('priors')), t(g('gt_bboxes')), gt_labels=t(g('gt_labels')))
        assert np.array_equal(r.gt_inds.numpy(), g('gt_inds')), i
        assert np.array_equal(r.labels.numpy(), g('labels')), i
        assert np.array_equal(r.max_overlaps.numpy().view(np.uint32), g('max_overlaps').astype(np.float32).view(np.uint32)), i
    assert int(z['cases_with_conflicts']) >= 1 and int(z['cases_with_clamped_costs']) >= 1


def test_host_twin_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/simota_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/simota_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap blocks, empty samples, counts past the rows, a
    short shared grid, NaN, +-inf and +-1e30 values, labels outside [0, C).  The device kernels share that decision code.  A sanitizer
    build belongs on a CPU-only machine: with a GPU present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    exe = _host_driver(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
