"""The flexible mAP on CPU tensors (the `_cpu` twins of csrc/eval_ap.hip and the evaluator of eval_map.py above them) against the three
restatements of tests/eval_ap_ref.py, and those against each other.  No GPU needed.

Bounds (derived, not measured; u = 2^-53):
  * num_det exact; recall bit-equal to c_D / den;
  * ap against the exact value on Fractions: the header sums the envelope exactly and rounds twice (the sum, the division), so
    |ap - exact| <= (2u + u^2) * exact — tighter than the (n_tp + 2) * 2u an ordered fp64 sum would need;
  * ap against the vectorised form, which rounds the same exact sum (math.fsum) once and divides: bit-equal;
  * ap against the literal fp64 area: n_tp * 2^-51 * max(1, recall) — the literal form subtracts neighbouring recalls, each of
    which carries u * recall;
  * the evaluator's fp32 mAP within one fp32 spacing of the literal's.
"""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import eval_ap_ref as ref
import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd import _lib, evaluation

R, CHUNK = evaluation.ap_tile_rows(), evaluation.ap_scan_chunk_tiles()
CASES = ref.build_cases(R, CHUNK, big=False)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_map.npz')
AFFINITY_TYPES = {'iou3d': 'LidarIOU3D', 'ioubev': 'LidarIOUBEV', 'trans': 'LidarCenterTransBEV'}


def run(case, device='cpu'):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(device)  # noqa: E731
    nd, rc, ap = amd.ap_accumulate(t(case['group'], None), t(case['score'], None), t(case['tp'], np.int32), t(case['msk'], np.int32),
                                   t(case['num_gt'], None), case['T'])
    assert nd.dtype == torch.int64 and rc.dtype == torch.float64 and ap.dtype == torch.float64
    assert nd.shape == rc.shape == ap.shape == (case['K'], case['T']) and nd.device.type == device
    return nd.cpu().numpy(), rc.cpu().numpy(), ap.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


_VECTOR = {}


def vector(case):
    """the vectorised form of a case, computed once and shared (read-only)"""
    if case['name'] not in _VECTOR:
        _VECTOR[case['name']] = ref.vector_accumulate(case)
    return _VECTOR[case['name']]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_twin_equals_the_vectorised_definition(case):
    nd, rc, ap = run(case)
    want_nd, want_rc, want_ap, _ = vector(case)
    assert np.array_equal(nd, want_nd)
    assert np.array_equal(bits(rc), bits(want_rc)), np.abs(rc - want_rc).max()
    assert np.array_equal(bits(ap), bits(want_ap)), np.abs(ap - want_ap).max()


def case_named(name, cases=CASES):
    return next(c for c in cases if c['name'].startswith(name))


def test_all_true_positives_and_one_true_positive_analytically():
    """Whole tiles of e = 1: ap = recall = 1 and num_det = n to the bit; with num_gt = 0 the sum n_1 is divided by 1e-7.  One true
    positive at the last of n ranks: the envelope is the fp64 quotient 1 / n at that row alone."""
    case = case_named('all_true_positives')
    n0, n1 = (int(s) for s in case['sizes'])
    assert case['num_gt'].tolist() == [n0, 0] and n0 > 3 * R
    nd, rc, ap = run(case)
    assert (nd[0] == n0).all() and (rc[0] == 1.0).all() and (ap[0] == 1.0).all()
    assert (nd[1] == n1).all() and (rc[1] == float(n1) / 1e-7).all() and (ap[1] == float(n1) / 1e-7).all()
    case = case_named('one_true_positive_at_the_last_rank')
    n, den = int(case['sizes'][0]), float(case['num_gt'][0])
    assert n == 2 * R + 3 and den > 0
    nd, rc, ap = run(case)
    assert (nd[0] == n).all() and (rc[0] == 1.0 / den).all() and (ap[0] == (1.0 / n) / den).all()


def _small_cases():
    rng = np.random.default_rng(77)
    out = [ref._random_case(f'small_{n}', rng, n, 3, 3, round_to=1) for n in (0, 1, 2, 50, 300)]
    c = ref._random_case('small_special', rng, 200, 2, 2)
    c['score'] = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -1.0, 1e-40], np.float32)[rng.integers(0, 7, 200)]
    c['num_gt'][1] = 0
    return out + [c]


@pytest.mark.parametrize('case', _small_cases(), ids=lambda c: c['name'])
def test_twin_and_vector_form_against_exact_fractions(case):
    exact = ref.exact_accumulate(case)
    u = Fraction(1, 2 ** 53)
    for got in (run(case)[2], ref.vector_accumulate(case)[2]):
        for k in range(case['K']):
            for t in range(case['T']):
                err = abs(Fraction(float(got[k, t])) - exact[k][t])
                print(case['name'], k, t, float(err), float(exact[k][t]))
                assert err <= (2 * u + u * u) * exact[k][t]


def _distinct_cases():
    rng = np.random.default_rng(5)
    out = []
    for n, K, T in ((0, 1, 1), (1, 1, 2), (R + 3, 2, 2), (3 * R + 17, 3, 3), (20000, 2, 2)):
        c = ref._random_case(f'distinct_{n}', rng, n, K, T, stray=False)
        c['score'] = ref.distinct_scores(rng, n)
        out.append(c)
    return out


@pytest.mark.parametrize('case', _distinct_cases(), ids=lambda c: c['name'])
def test_literal_form_against_the_definition_and_the_twin(case):
    """The reference's lines with mmdet's looped envelope, per group, against the vectorised definition and the twin."""
    T = case['T']
    v_nd, v_rc, v_ap, n_tp = ref.vector_accumulate(case)
    nd, rc, ap = run(case)
    tp, msk = ref.unpack(case['tp'] & case['msk'], T), ref.unpack(case['msk'], T)
    for k in range(case['K']):
        rows = case['group'] == k
        num_gt = int(case['num_gt'][k])
        lit64 = ref.literal_accumulate(num_gt, case['score'][rows], tp[:, rows], msk[:, rows], T, fp64_ap=True)
        lit32 = ref.literal_accumulate(num_gt, case['score'][rows], tp[:, rows], msk[:, rows], T)
        for t in range(T):
            assert lit64[t][0] == v_nd[k, t] == nd[k, t]
            assert float(lit64[t][1]) == v_rc[k, t] == rc[k, t]
            bound = n_tp[k, t] * 2.0 ** -51 * max(1.0, v_rc[k, t])
            print(case['name'], k, t, abs(lit64[t][2] - v_ap[k, t]), bound)
            assert abs(lit64[t][2] - v_ap[k, t]) <= bound and abs(lit64[t][2] - ap[k, t]) <= bound
            assert abs(float(lit32[t][2]) - float(np.float32(ap[k, t]))) <= np.spacing(np.float32(lit32[t][2]))


# ---- tp_records ------------------------------------------------------------------------------------------------------------------------

def _literal_records(matched, det_flag, gt_flag, T):
    """mean_ap_flexible.py:115-123 (matched None: :98-104), with matches outside [-1, G) counted as -1"""
    D = len(det_flag)
    if matched is None:
        return np.zeros((T, D), bool), np.repeat(det_flag[None, :], T, axis=0)
    m = np.where((matched >= 0) & (matched < len(gt_flag)), matched, -1)
    tp = m > -1
    msk_fp = det_flag[None, :] & (m == -1)
    msk_tp = (gt_flag[m] if len(gt_flag) else np.zeros_like(tp)) & (m > -1)
    return tp, msk_fp | msk_tp


@pytest.mark.parametrize('D,G,T,how', [(0, 5, 2, 'match'), (1, 1, 1, 'match'), (300, 40, 2, 'match'), (257, 9, 32, 'match'),
                                       (64, 7, 3, 'empty'), (33, 0, 2, 'no_gt'), (100, 6, 4, 'out_of_range')])
def test_tp_records_against_the_literal_lines(D, G, T, how):
    rng = np.random.default_rng(D + G + T)
    det_flag, gt_flag = rng.uniform(0, 1, D) < 0.7, rng.uniform(0, 1, G) < 0.6
    score = rng.uniform(0, 1, D).astype(np.float32)
    matched = None if how == 'empty' else rng.integers(-1, max(G, 1), (T, D)).astype(np.int32)
    if how == 'no_gt':
        matched[:] = -1
    if how == 'out_of_range':
        matched[rng.uniform(0, 1, (T, D)) < 0.3] = rng.choice([-7, G, G + 5, 2 ** 31 - 1, -2 ** 31])
    tp, msk = _literal_records(matched, det_flag, gt_flag, T)
    g, s, tpb, mskb = amd.tp_records(None if matched is None else torch.from_numpy(matched), torch.from_numpy(det_flag), torch.from_numpy(gt_flag),
                                     torch.from_numpy(score), 11, num_thrs=T)
    assert g.device.type == 'cpu' and np.array_equal(g.numpy(), np.full(D, 11, np.int32)) and np.array_equal(s.numpy(), score)
    assert np.array_equal(tpb.numpy().view(np.uint32), ref.pack(tp)) and np.array_equal(mskb.numpy().view(np.uint32), ref.pack(msk))
    # into rows of a record buffer: the rows around the block are left alone
    out = tuple(torch.full((D + 9,), -1, dtype=dt) for dt in (torch.int32, torch.float32, torch.int32, torch.int32))
    amd.tp_records(None if matched is None else torch.from_numpy(matched), torch.from_numpy(det_flag), torch.from_numpy(gt_flag),
                   torch.from_numpy(score), 3, num_thrs=T, out=out, row=4)
    assert np.array_equal(out[2][4:4 + D].numpy().view(np.uint32), ref.pack(tp)) and np.array_equal(out[0][4:4 + D].numpy(), np.full(D, 3))
    assert all((c[:4] == -1).all() and (c[4 + D:] == -1).all() for c in out)


def test_argument_errors():
    lib = _lib.load()
    z = np.zeros(8, np.int64)
    p = z.ctypes.data
    for T, K, want in ((0, 1, 10001), (33, 1, 10001), (2, 0, 10001), (2, (1 << 20) + 1, 10002)):
        assert lib.eval_ap_accumulate_cpu(p, p, p, p, p, 2, K, T, p, p, p, 1) == want
        assert lib.eval_ap_workspace_bytes(2, K, T) == 0
    assert lib.eval_ap_accumulate_cpu(p, p, p, p, p, -1, 1, 1, p, p, p, 1) == 10001
    assert lib.eval_ap_accumulate_cpu(None, p, p, p, p, 2, 1, 1, p, p, p, 1) == 10001
    assert lib.eval_ap_accumulate_cpu(p, p, p, p, p, 1 << 31, 1, 1, p, p, p, 1) == 10002
    assert lib.eval_tp_records_cpu(None, p, p, p, 0, 2, 2, 0, p, p, p, p) == 10001
    assert lib.eval_tp_records_cpu(None, p, p, p, 0, 2, 2, 33, p, p, p, p) == 10001
    assert lib.eval_tp_records_cpu(None, p, None, p, 0, 2, 2, 1, p, p, p, p) == 10001
    # (the size of a legal workspace needs the sort's scratch, which the runtime only tells with a device: tests/test_gpu_eval_ap.py)
    assert ctypes.c_int32(lib.eval_ap_tile_rows()).value == R and R % 256 == 0 and CHUNK >= 1
    i32, f32 = (lambda n: torch.zeros(n, dtype=torch.int32)), (lambda n: torch.zeros(n))
    with pytest.raises(RuntimeError, match='thresholds'):
        amd.ap_accumulate(i32(4), f32(4), i32(4), i32(4), torch.ones(1, dtype=torch.int64), 0)
    with pytest.raises(RuntimeError, match='thresholds'):
        amd.ap_accumulate(i32(4), f32(4), i32(4), i32(4), torch.ones(1, dtype=torch.int64), 33)
    with pytest.raises(RuntimeError, match='groups'):
        amd.ap_accumulate(i32(4), f32(4), i32(4), i32(4), torch.ones(0, dtype=torch.int64), 2)
    with pytest.raises(RuntimeError, match='rows'):
        amd.ap_accumulate(i32(4), f32(5), i32(4), i32(4), torch.ones(1, dtype=torch.int64), 2)
    with pytest.raises(RuntimeError, match='matched must be'):
        amd.tp_records(torch.zeros((2, 5), dtype=torch.int32), torch.zeros(4, dtype=torch.bool), torch.zeros(3, dtype=torch.bool), f32(4), 0)
    with pytest.raises(RuntimeError, match='detection flags'):
        amd.tp_records(None, torch.zeros(3, dtype=torch.bool), torch.zeros(3, dtype=torch.bool), f32(4), 0, num_thrs=2)


# ---- the shared arithmetic against Python's integers -----------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def apmath(tmp_path_factory):
    """tests/hostmath/eval_ap_math.cpp: csrc/eval_ap_common.h compiled for the host with -ffp-contract=off, as both product units are"""
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    so = str(tmp_path_factory.mktemp('eval_ap_math') / 'libevalapmath.so')
    cmd = [cxx, '-O1', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', os.path.join(ROOT, 'tests', 'hostmath', 'eval_ap_math.cpp'), '-o', so]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = ctypes.CDLL(so)
    for f in ('hostmath_limbs_of', 'hostmath_limbs_to_double', 'hostmath_score_key', 'hostmath_record_key'):
        getattr(lib, f).restype = None
    return lib


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _limbs_to_double(lib, limbs):
    limbs = np.ascontiguousarray(limbs, np.uint64).reshape(-1, 4)
    out = np.empty(len(limbs), np.float64)
    lib.hostmath_limbs_to_double(_vp(limbs), ctypes.c_long(len(limbs)), _vp(out))
    return out


def _total(l):
    return int(l[0]) + (int(l[1]) << 21) + (int(l[2]) << 42) + (int(l[3]) << 63)


def _unnormalised(rng, total):
    """four limb sums below 2^53, not normalised, whose weighted sum is `total` (< 2^116): the normal form, then units moved down"""
    l = [total & 0x1fffff, (total >> 21) & 0x1fffff, (total >> 42) & 0x1fffff, total >> 63]
    assert l[3] < 1 << 53
    for k in (3, 2, 1):
        a = min(l[k], ((1 << 53) - 1 - l[k - 1]) >> 21, int(rng.integers(0, 1 << 32)))
        if rng.uniform() < 0.8:
            l[k] -= a
            l[k - 1] += a << 21
    assert all(0 <= x < 1 << 53 for x in l) and _total(l) == total
    return l


def test_limbs_to_double_on_unnormalised_limb_sums_against_python_integers(apmath):
    """What only the device's finish kernel asks of limbs_to_double: limb sums of up to 53 bits each, whose carries `l1 >> 43`,
    `l2 >> 22`, `l3 >> 1` count.  The result must be the total of 2^-84 units rounded once, to nearest even: float(Fraction)."""
    rng = np.random.default_rng(84)
    rows = []
    for _ in range(20000):                               # random limbs of random lengths
        rows.append([int(rng.integers(0, 1 << 53)) >> int(rng.integers(0, 54)) for _ in range(4)])
    top = (1 << 53) - 1
    rows += [[top] * 4, [top, 0, 0, 0], [0, top, 0, 0], [0, 0, top, 0], [0, 0, 0, top], [0, top, top, 0], [top, top, 0, 1], [0, 0, 0, 0],
             [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1 << 31], [0, 1 << 52, 1 << 52, 1 << 52]]
    halfway = 0
    for bits_ in range(54, 116):                         # totals of every length with the cut exactly halfway, one below and one above
        for _ in range(40):
            m = (1 << 52) | int(rng.integers(0, 1 << 52))          # the 53 kept bits: odd and even last bits
            for delta in (-1, 0, 1):
                total = (m << (bits_ - 53)) + (1 << (bits_ - 54)) + delta
                assert total.bit_length() == bits_
                rows.append(_unnormalised(rng, total))
                halfway += 1
    assert halfway >= 62 * 3 * 40 and any(r[1] >> 43 for r in rows) and any(r[2] >> 22 for r in rows)
    got = _limbs_to_double(apmath, np.array(rows, np.uint64))
    want = np.array([float(Fraction(_total(r), 1 << 84)) for r in rows])
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, (rows[bad[0]], got[bad[0]], want[bad[0]])


def test_limbs_of_represents_the_fp64_quotient_exactly(apmath):
    rng = np.random.default_rng(85)
    j = rng.integers(1, 1 << 31, 200000)
    c = np.minimum(j, rng.integers(1, 1 << 31, 200000) >> rng.integers(0, 31, 200000)).clip(1)
    e = np.concatenate([c / j, [1.0, 2.0 ** -31, 1.0 / (2 ** 31 - 1), 0.0, 1.0 / 3.0, (2.0 ** 31 - 2) / (2.0 ** 31 - 1)]])
    assert (c >= 1).all() and (c <= j).all() and (e[:len(c)] == c.astype(np.float64) / j.astype(np.float64)).all()
    limbs = np.empty((len(e), 4), np.uint32)
    apmath.hostmath_limbs_of(_vp(e), ctypes.c_long(len(e)), _vp(limbs))
    assert (limbs[:, :3] < 1 << 21).all() and (limbs[:, 3] <= 1 << 21).all()
    assert limbs[len(c)].tolist() == [0, 0, 0, 1 << 21] and limbs[len(c) + 3].tolist() == [0, 0, 0, 0]
    for q, l in zip(e.tolist(), limbs.tolist()):
        num, den = q.as_integer_ratio()                  # den: a power of two, at most 2^84 for these quotients
        assert (1 << 84) % den == 0 and _total(l) == num * ((1 << 84) // den), (q, l)
    # and back: a single e survives the round trip
    assert np.array_equal(bits(_limbs_to_double(apmath, limbs.astype(np.uint64))), bits(e))


def test_record_key_order_is_the_rank_order_on_special_scores(apmath):
    """Ascending record_key (stable) = group, then `rank_order`: NaN of either sign and any payload first, -0 == +0, denormals,
    +-inf; groups outside [0, K) — the ends of int32 among them — sort last, as group K."""
    rng = np.random.default_rng(86)
    K = 5
    special = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                        0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x3f800000, 0xbf800000,
                        0x3f000000, 0x3f000001], np.uint32).view(np.float32)
    n = 4000
    score = special[rng.integers(0, len(special), n)]
    score[::7] = rng.uniform(-2, 2, len(score[::7])).astype(np.float32)
    group = rng.choice(np.array([0, 1, 2, 3, 4, -1, K, K + 1, 2 ** 31 - 1, -2 ** 31, -7], np.int64), n).astype(np.int32)
    key = np.empty(n, np.uint64)
    apmath.hostmath_record_key(_vp(group), _vp(score), ctypes.c_long(n), ctypes.c_int32(K), _vp(key))
    word = np.empty(n, np.uint32)
    apmath.hostmath_score_key(_vp(score), ctypes.c_long(n), _vp(word))
    g = np.where((group >= 0) & (group < K), group, K).astype(np.int64)
    assert np.array_equal(key >> np.uint64(32), g.astype(np.uint64)) and np.array_equal((key & np.uint64(0xffffffff)).astype(np.uint32), word)
    with np.errstate(invalid='ignore'):                  # the signalling NaNs, widened
        order = ref.rank_order(score)
    want = order[np.argsort(g[order], kind='stable')]
    assert np.array_equal(np.argsort(key, kind='stable'), want)
    assert np.array_equal(np.argsort(word, kind='stable'), order)
    assert (word[np.isnan(score)] == 0).all() and (word[~np.isnan(score)] > 0).all()


def test_host_twin_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/eval_ap_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/eval_ap_sanitize.cpp, its own main) under
    -fsanitize=address,undefined,float-cast-overflow and run as a program on the CPU: exactly sized heap blocks, n = 0, a NULL
    `matched`, G = 0, matches and groups outside their ranges, NaN and infinite scores, T = 32, K = 1 and a few thousand, 1, 3 and
    all threads.  The device kernels share the key, limb and finish code.  A sanitizer build belongs on a CPU-only machine: with a GPU
    present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'eval_ap_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all', '-ffp-contract=off',
           '-pthread', os.path.join(ROOT, 'tests', 'hostmath', 'eval_ap_sanitize.cpp'),
           os.path.join(ROOT, 'mmdet3d-gaussian_amd', 'csrc', 'eval_ap_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the surface -------------------------------------------------------------------------------------------------------------------------

def test_registries_build_the_reference_config_dicts():
    classes = ['Car', 'Pedestrian', 'Cyclist']
    b = amd.build_eval_breakdown(dict(type='RangeBreakdown', ranges={'0-30': (0, 30), '30+': (30, 1e9)}, apply_to=['Car']), classes=classes)
    assert isinstance(b, amd.RangeBreakdown) and b.names == ['0-30', '30+'] and b.breakdown_names(0) == ['0-30', '30+'] and b.breakdown_names(1) == []
    boxes = np.array([[3, 4, 0, 1, 2, 3, 0], [30, 40, 0, 1, 1, 1, 0]], np.float32)
    assert b.breakdown(boxes, 0).tolist() == [[True, False], [False, True]] and b.breakdown(boxes, 1).shape == (0, 2)
    assert b.breakdown(boxes, 0, dict(ignore=np.array([True, False]))).tolist() == [[False, False], [False, True]]
    assert b.breakdown(boxes, 0, dict(distance=np.array([100.0, 1.0]))).tolist() == [[False, True], [True, False]]
    assert b.breakdown(torch.from_numpy(boxes), 0).tolist() == [[True, False], [False, True]]
    v = amd.build_eval_breakdown(dict(type='VolumeBreakdown', ranges={'small': (0, 3), 'big': (3, 100)}), classes=classes)
    assert v.breakdown(boxes, 2).tolist() == [[False, True], [True, False]]
    assert v.breakdown(boxes, 2, dict(volumn=np.array([1.0, 50.0]))).tolist() == [[True, False], [False, True]]
    assert amd.build_eval_breakdown(dict(type='NoBreakdown'), classes=classes).breakdown(boxes, 1).tolist() == [[True, True]]
    a = amd.build_eval_affinity_calculator(dict(type='LidarIOU3D'))
    assert isinstance(a, amd.LidarIOU3D) and a.z_offset == 0.5 and a.LARGER_CLOSER
    assert amd.build_eval_affinity_calculator(dict(type='LidarIOUBEV')).LARGER_CLOSER
    assert not amd.build_eval_affinity_calculator(dict(type='LidarCenterTransBEV')).LARGER_CLOSER
    m = amd.build_eval_matcher(dict(type='MatcherCoCo'), match_thrs=[0.5, 0.7], affinity_cost_negate=True)
    assert isinstance(m, amd.MatcherCoCo) and m.match_thrs == [0.5, 0.7] and m.negate
    with pytest.raises(KeyError):
        amd.build_eval_tp_metric(dict(type='Anything'))
    with pytest.raises(AssertionError, match='crowd'):
        a(torch.zeros(1, 7), torch.zeros(1, 7), np.zeros(1, bool))
    for name in ('EVAL_MATCHERS', 'EVAL_AFFINITYCALS', 'EVAL_BREAKDOWNS', 'EVAL_TPMETRIC'):
        assert isinstance(getattr(amd, name), amd.Registry)


def test_exports():
    names = ['tp_records', 'ap_accumulate', 'FlexibleStatisticsEval', 'eval_map_flexible', 'NoBreakdown', 'RangeBreakdown', 'VolumeBreakdown',
             'LidarIOU3D', 'LidarIOUBEV', 'LidarCenterTransBEV', 'MatcherCoCo', 'EVAL_MATCHERS', 'EVAL_AFFINITYCALS', 'EVAL_BREAKDOWNS',
             'EVAL_TPMETRIC', 'build_eval_matcher', 'build_eval_affinity_calculator', 'build_eval_breakdown', 'build_eval_tp_metric']
    for n in names:
        assert n in amd.__all__ and hasattr(amd, n), n
    assert 'out of this build' not in evaluation.__doc__


# ---- the evaluator end to end on CPU tensors -----------------------------------------------------------------------------------------------

def as_tensors(det_results, device):
    return [[torch.from_numpy(d).to(device) for d in frame] for frame in det_results]


def check_against_literal(got, want):
    """integers exact, recall bit-equal, the fp32 mAP within one fp32 spacing of the literal's"""
    assert len(got) == len(want)
    for (gk, gv), (wk, wv) in zip(got, want):
        assert gk == wk
        assert gv['num_det'] == wv['num_det'] and gv['num_gt'] == wv['num_gt'], (gk, gv, wv)
        assert float(gv['recall']) == float(wv['recall']), (gk, gv, wv)
        assert isinstance(gv['mAP'], np.float32)
        assert abs(float(gv['mAP']) - float(wv['mAP'])) <= np.spacing(np.float32(wv['mAP'])), (gk, gv, wv)


RANGES = {'0-30m': (0, 30), '30-50m': (30, 50), '50m+': (50, 1e9)}
CLASSES = ['Car', 'Pedestrian', 'Cyclist']


def safe_dataset(affinity, thrs, frames=60):
    """a random dataset none of whose (oracle) affinities lies within 1e-5 of a threshold: the seed is redrawn until all of it does"""
    for seed in range(100, 140):
        det, anno = ref.random_dataset(seed, frames, 3, 24, 8)
        margin = min(ref.affinity_margin(ref.literal_single(d, a, CLASSES, [RANGES], affinity, thrs)[1], thrs) for d, a in zip(det, anno))
        if margin > 1e-5:
            return det, anno
    raise AssertionError('no seed gives a dataset clear of the thresholds')


@pytest.mark.parametrize('affinity,thrs', [('iou3d', [0.5, 0.7]), ('ioubev', [0.3, 0.5, 0.7]), ('trans', [0.5, 2.0])])
def test_evaluator_on_cpu_tensors_against_the_literal_reference_lines(affinity, thrs):
    det, anno = safe_dataset(affinity, thrs)
    want = ref.literal_eval(det, anno, CLASSES, [RANGES], affinity, thrs)
    fse = amd.FlexibleStatisticsEval(CLASSES, thrs, [dict(type='RangeBreakdown', ranges=RANGES)], dict(type=AFFINITY_TYPES[affinity]),
                                     dict(type='MatcherCoCo'), [], 0)
    got = fse.statistics_eval(as_tensors(det, 'cpu'), anno)
    assert sum(v['num_det'] for _, v in got) > 1000 and any(v['mAP'] > 0.1 for _, v in got)
    check_against_literal(got, want)
    # per frame: the reference's tuples
    for f in (0, 5, 7):
        mine = fse.statistics_single((as_tensors(det, 'cpu')[f], anno[f]))
        theirs = ref.literal_single(det[f], anno[f], CLASSES, [RANGES], affinity, thrs)[0]
        assert len(mine) == len(theirs)
        for a, b in zip(mine, theirs):
            assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[5], b[5])
            assert np.array_equal(a[4] & a[5], b[4] & b[5])       # what of tp counts: the bits under the mask
    # one group through the reference's own accumulate signature
    info = ref.literal_single(det[0], anno[0], CLASSES, [RANGES], affinity, thrs)[0][0]
    one = fse.statistics_accumulate(info)
    lit = ref.literal_accumulate(info[2], info[3], info[4], info[5], len(thrs))
    assert [v['num_det'] for _, v in one] == [x[0] for x in lit]


def test_eval_map_flexible_reports_and_prints_a_plain_table(capsys):
    det, anno = ref.random_dataset(3, 12, 3, 20, 6)
    report = amd.eval_map_flexible(as_tensors(det, 'cpu'), anno, match_thrs=[0.5], classes=CLASSES, nproc=8,
                                   breakdowns=[dict(type='RangeBreakdown', ranges=RANGES, apply_to=['Car'])],
                                   report_config=[('map', lambda x: x['breakdown'] == 'All'), ('car_near', lambda x: x['breakdown'] == '0-30m')])
    text = capsys.readouterr().out
    assert list(report) == ['map', 'car_near'] and 0 <= report['map'] <= 1
    rows = [line for line in text.splitlines() if line.startswith('|')]
    assert len(rows) == 1 + 4 + 1 + 1 and 'Class' in rows[0] and 'Recall' in rows[0]       # Car: All + 3 ranges; the others: All
    k = next(i for i in range(len(anno)) if len(anno[i]['gt_labels']) and all(len(d) for d in det[i]))
    bad = dict(anno[k], gt_attrs=dict(anno[k]['gt_attrs'], iscrowd=np.zeros(len(anno[k]['gt_labels']), bool)))
    with pytest.raises(AssertionError, match='crowd'):      # the reference's assertion (affinity.py:10)
        amd.eval_map_flexible(as_tensors(det, 'cpu')[k:k + 1], [bad], classes=CLASSES, logger='silent')


# ---- the golden fixture recorded from the reference -------------------------------------------------------------------------------------------

def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    frames, num_cls = int(z['frames']), len(z['classes'])
    det = [[z[f'det.{f}.{c}'] for c in range(num_cls)] for f in range(frames)]
    anno = [dict(gt_bboxes=z[f'gt_bboxes.{f}'], gt_labels=z[f'gt_labels.{f}'], gt_attrs=dict(ignore=z[f'gt_ignore.{f}'])) for f in range(frames)]
    ranges = {str(n): (float(lo), float(hi)) for n, (lo, hi) in zip(z['range_names'], z['range_bounds'])}
    return z, det, anno, [str(c) for c in z['classes']], ranges, [float(t) for t in z['match_thrs']]


def golden_results(z, cfg):
    return [(dict(class_name=str(c), breakdown=str(b), match_threshold=float(t)), dict(num_det=int(nd), num_gt=int(ng), recall=float(r), mAP=m))
            for c, b, t, nd, ng, r, m in zip(z[f'{cfg}.cls'], z[f'{cfg}.bkd'], z[f'{cfg}.thr'], z[f'{cfg}.num_det'], z[f'{cfg}.num_gt'],
                                             z[f'{cfg}.recall'], z[f'{cfg}.mAP'])]


def check_golden(device):
    z, det, anno, classes, ranges, thrs = load_golden()
    for cfg in ('iou3d', 'ioubev', 'trans'):
        fse = amd.FlexibleStatisticsEval(classes, thrs, [dict(type='RangeBreakdown', ranges=ranges)], dict(type=AFFINITY_TYPES[cfg]),
                                         dict(type='MatcherCoCo'), [], 0)
        got = fse.statistics_eval(as_tensors(det, device), anno)
        check_against_literal(got, golden_results(z, cfg))
        # the per-frame tuples the reference produced
        for f in range(len(det)):
            mine = fse.statistics_single((as_tensors(det, device)[f], anno[f]))
            p = f'{cfg}.info.{f}'                      # the frame's tuples side by side
            assert [a[2] for a in mine] == z[p + '.gt_count'].tolist() and [len(a[3]) for a in mine] == z[p + '.rows'].tolist()
            assert np.array_equal(np.concatenate([a[3] for a in mine]), z[p + '.score'])
            tp, msk = np.concatenate([a[4] for a in mine], axis=1), np.concatenate([a[5] for a in mine], axis=1)
            assert np.array_equal(msk, z[p + '.msk']) and np.array_equal(tp & msk, z[p + '.tp'] & z[p + '.msk'])


def test_golden_fixture_meets_its_conditions():
    """All scores of a class distinct over the dataset; no (oracle) affinity within 1e-5 of a threshold."""
    z, det, anno, classes, ranges, thrs = load_golden()
    assert len(det) >= 25 and len(classes) == 3 and thrs == [0.5, 0.7] and any(a['gt_attrs']['ignore'].any() for a in anno)
    for c in range(len(classes)):
        s = np.concatenate([frame[c][:, -1] for frame in det])
        assert s.dtype == np.float32 and len(np.unique(s)) == len(s)
    for cfg in ('iou3d', 'ioubev', 'trans'):
        margin = min(ref.affinity_margin(ref.literal_single(d, a, classes, [ranges], cfg, thrs)[1], thrs) for d, a in zip(det, anno))
        assert margin > 1e-5, (cfg, margin)


def test_evaluator_on_cpu_tensors_against_the_golden_fixture():
    check_golden('cpu')
