"""The evaluation matcher (csrc/eval_match.hip) on the device, on every kernel path `eval_match_coco` dispatches to and at the sizes
where a path changes (tests/match_cases.py), against the CPU oracle: integer-exact.  The oracle itself is pinned on the same cases
against the reference's compiled matcher (tests/test_oracle_rbox.py); what the cases exercise is asserted in tests/test_cpu_rbox.py."""
import numpy as np
import pytest
import torch

import match_cases
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    import mmdet3d_gaussian_amd as m
    assert torch.cuda.is_available()
    m.load_library()
    return m


def _dev(x):
    return torch.tensor(x).cuda()       # copies: the table's arrays are read-only


def _case(G, D):
    return next(c for c in match_cases.CASES if (c.G, c.D) == (G, D))


def _check(amd, case, args, want):
    got = amd.match_coco(*[_dev(x) for x in args])
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (case.T, case.D)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f'{int((got != want).sum())} of {want.size} differ, first at (t, d) = {np.argwhere(got != want)[0]}'
    twin = amd.match_coco(*[torch.tensor(x) for x in args])        # CPU tensors: eval_match_coco_cpu
    assert twin.device.type == 'cpu' and np.array_equal(twin.numpy(), want)


@pytest.mark.parametrize('case', match_cases.CASES, ids=lambda c: c.id)
def test_match_coco_case_table_vs_oracle(amd, case):
    _check(amd, case, match_cases.inputs(case), match_cases.expected(case))


@pytest.mark.parametrize('case', match_cases.LARGE_CASES, ids=lambda c: c.id)
def test_match_coco_lds_bitmask_up_to_the_maximum_vs_oracle(amd, case):
    """G = 393184 | 393185: the taken bitmask reaches and passes 48 KiB of LDS (the kernel opts in to more); G = 2^20: the documented
    maximum, 128 KiB.  An error of the opt-in call comes back as the entry's return code and fails the test with that code."""
    free, _ = torch.cuda.mem_get_info()
    if free < (2 << 30):
        pytest.skip('needs 2 GB of free HBM')
    args = match_cases.build(case)
    want = oracle.match_coco(*args)
    try:
        _check(amd, case, args, want)
    finally:
        del args
        torch.cuda.empty_cache()


def test_match_coco_device_entry_argument_rules(amd):
    G = match_cases.G_MAX + 1
    flags = torch.zeros(G, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='10002'):                  # GD3D_E_TOOLARGE
        amd.match_coco(torch.zeros((1, G), device='cuda'), [0.5], flags, flags)
    del flags
    none = torch.zeros(0, dtype=torch.bool, device='cuda')
    # no ground truth: every detection unmatched; T x D words through the vector body and the tail of fill_words_kernel
    for T, D in ((1, 1), (1, 3), (2, 2), (1, 5), (5, 205)):
        got = amd.match_coco(torch.zeros((D, 0), device='cuda'), torch.linspace(0, 1, T), none, none)
        assert got.dtype == torch.int32 and got.shape == (T, D) and bool((got == -1).all()), (T, D)
    some = torch.zeros(5, dtype=torch.bool, device='cuda')
    got = amd.match_coco(torch.zeros((0, 5), device='cuda'), [0.1, 0.2], some, some)
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (2, 0)
    got = amd.match_coco(torch.zeros((7, 5), device='cuda'), torch.zeros(0), some, some)
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (0, 7)
    with pytest.raises(RuntimeError, match='5 gts but 4 ignore'):
        amd.match_coco(torch.zeros((7, 5), device='cuda'), [0.1], some[:4], some)
    with pytest.raises(RuntimeError, match='5 gts but 5 ignore / 6 crowd'):
        amd.match_coco(torch.zeros((7, 5), device='cuda'), [0.1], some, torch.zeros(6, dtype=torch.bool, device='cuda'))
    with pytest.raises(RuntimeError, match='must be 2-D'):
        amd.match_coco(torch.zeros(5, device='cuda'), [0.1], some, some)


@pytest.mark.parametrize('G,D', [(129, 33), (513, 63)])
def test_match_coco_wrapper_input_forms_equal_the_plain_call(amd, G, D):
    case = _case(G, D)
    cost, thrs, ign, crowd = match_cases.inputs(case)
    want = match_cases.expected(case)
    plain = amd.match_coco(_dev(cost), _dev(thrs), _dev(ign), _dev(crowd))
    assert np.array_equal(plain.cpu().numpy(), want)
    view = _dev(np.ascontiguousarray(cost.T)).t()                    # (D, G) view of a (G, D) buffer
    assert view.shape == (D, G) and not view.is_contiguous()
    forms = {
        'transposed view': (view, _dev(thrs), _dev(ign), _dev(crowd)),
        'float64 numpy costs': (cost.astype(np.float64), _dev(thrs), _dev(ign), _dev(crowd)),
        'uint8 flags': (_dev(cost), _dev(thrs), _dev(ign.astype(np.uint8)), _dev(crowd.astype(np.uint8))),
        'bool and uint8 flags': (_dev(cost), _dev(thrs), _dev(ign), _dev(crowd.astype(np.uint8))),
        'thresholds as a list': (_dev(cost), [float(t) for t in thrs], _dev(ign), _dev(crowd)),
        'all numpy': (np.array(cost), np.array(thrs), np.array(ign), np.array(crowd)),
    }
    for name, args in forms.items():
        got = amd.match_coco(*args)
        assert got.is_cuda and got.dtype == torch.int32 and torch.equal(got, plain), name


@pytest.mark.parametrize('D,G', [(1, 1), (255, 1), (257, 3), (3, 257)])
@pytest.mark.parametrize('dcols,gcols', [(2, 7), (7, 9), (9, 2)])
def test_trans_bev_bit_equal_to_the_oracle(amd, D, G, dcols, gcols):
    """One thread per (det, gt) in blocks of 256: one block, one short of two, and past a block from either side; every column count
    on either side.  Coordinates at 1e18 stay finite (squares of 1e36), at 1e20 their squares overflow to inf; one row is NaN."""
    rng = np.random.default_rng(D * 1000 + G + dcols)
    det = rng.uniform(-80, 80, (D, dcols)).astype(np.float32)
    gt = rng.uniform(-80, 80, (G, gcols)).astype(np.float32)
    big, small = (det, gt) if D >= G else (gt, det)
    big[0, :2] = 1e18
    big[-1, :2] = (1e20, -1e20)
    if len(big) > 2:
        big[1, :2] = (np.nan, 0.0)
    if len(small) > 1:
        small[-1, :2] = np.nan
    want = oracle.eval_trans_bev(det, gt)
    assert np.isposinf(want).any() and (np.isnan(want).any() or D * G == 1) and (np.isfinite(want).any() or D * G == 1)
    got = amd.trans_bev(_dev(det), _dev(gt))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (D, G)
    got = got.cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
