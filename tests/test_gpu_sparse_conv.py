"""Sparse 3D convolution on the MI355X (csrc/sparse_conv.hip): the cases of tests/sparse_conv_ref.py on cuda:0, through the helpers of
tests/test_cpu_sparse_conv.py.  The integer outputs exactly equal the numpy restatement and the `_cpu` twin; the values lie within the
derived bound (L + 2) 2^-24 A of the fp64 dense-conv3d oracle and are bit-identical from run to run; bands around every output and
around both workspaces stay untouched; the 20 000-row sweeps; the modules, the shared index, dense(), the encoder; the static form
recorded and replayed in one graph on fresh inputs; the device guard; the index build over 300 samples, at max_out 0 and 1 and at batch
size 0; non-finite inputs; `out` and `gx` 4 bytes past an aligned address."""
import ctypes

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_ref as ref
from mmdet3d_gaussian_amd import _lib
from test_cpu_sparse_conv import (ENC_SHAPES, INT_OUTPUTS, SWEEPS, VALUE_CASES, check_bad_arguments, check_batch_zero, check_dense, check_encoder,
                                  check_index, check_many_samples, check_max_out_0_and_1, check_modules_equal_functional,
                                  check_nonfinite_containment, check_shared_indice_key, check_values, run_index, run_values)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = -77.0           # the sentinel of the guard test


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_index_on_the_device(name):
    got = check_index(name, DEV)                                  # the restatement's integers, tail rows included
    twin, again = run_index(ref.case_of(name), 'cpu'), run_index(ref.case_of(name), DEV)
    for k in INT_OUTPUTS:
        if getattr(got, k) is not None:
            assert torch.equal(getattr(got, k).cpu(), getattr(twin, k)), f'{name}: {k} differs from the twin'
            assert torch.equal(getattr(got, k), getattr(again, k)), f'{name}: {k} differs from run to run'


@pytest.mark.parametrize('name', VALUE_CASES)
def test_values_within_the_derived_bound_and_the_same_bits_from_run_to_run(name):
    got = run_values(name, DEV)
    check_values(name, DEV, got)
    again = run_values(name, DEV)
    for k in ('out', 'gx', 'gw', 'gb'):
        if got[k] is not None:
            assert got[k].tobytes() == again[k].tobytes(), f'{name}: {k} differs from run to run'


@pytest.mark.parametrize('name', SWEEPS)
def test_sweep_of_20000_rows(name):
    """about 20 000 rows over 3 samples at 16 -> 32: 313 workgroups of the forward kernel, 64 partial sums per offset in the weight gradient"""
    index = check_index(name, DEV)
    got = run_values(name, DEV, index)
    check_values(name, DEV, got)
    again = run_values(name, DEV, index)
    for k in ('out', 'gx', 'gw', 'gb'):
        assert got[k].tobytes() == again[k].tobytes(), f'{name}: {k} differs from run to run'


def test_dynamic_form_returns_exact_size_views():
    case, want = ref.CASES['s2p1_max_out_at'], ref.expected_index('s2p1_max_out_at')
    got = run_index(case, DEV, max_out=None)
    for k in INT_OUTPUTS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k


GUARD_CASES = ['subm_inactive_rows_scattered_and_tail', 's2p1_max_out_below', 's2p1_max_out_above', 'down_7x11x13_c16_32', 's2p011_7x11x13_c3_7',
               'subm_rows_1', 's2p1_rows_tile_plus_1',
               # whole 64-row tiles inactive or past num[0]; 64 -> 64 with one offset a row
               'subm_inactive_block', 's2p1_inactive_block', 's2p1_max_out_far_above', 'subm_isolated_c64_64', 's2p1_isolated_c64_64']


def run_c_entries_between_bands(name, shift):
    """the C entry points on sentinel-filled buffers with a guard band either side of every output and of both workspaces: every row of
    every output is written, the bands stay untouched.  `out` and `gx` start `shift` floats past a 16-byte aligned address."""
    case, want = ref.case_of(name), ref.expected_index(name)
    X, W, bias, gY = (None if a is None else torch.from_numpy(a).to(DEV) for a in ref.operands(name))
    coors = torch.from_numpy(case['coors']).to(DEV)
    N, B, (K, Cin, Cout), R = len(coors), case['B'], W.shape, len(want['nbr'])
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    G, band = 64, 4096
    ints = dict(out_coors=R * 4, nbr=R * K, nbr_t=N * K, out_batch_cnt=B)
    bufs = {k: torch.full((n + 2 * G,), 77, dtype=torch.int32, device=DEV) for k, n in ints.items()}
    bufs['num'] = torch.full((2 + 2 * G,), 77, dtype=torch.int64, device=DEV)
    floats = dict(out=R * Cout, gx=N * Cin, gw=K * Cin * Cout, gb=Cout)
    bufs.update({k: torch.full((n + 2 * G,), S, device=DEV) for k, n in floats.items()})
    off = {k: G + (shift if k in ('out', 'gx') else 0) for k in bufs}
    at = lambda k: bufs[k][off[k]:].data_ptr()
    assert all(at(k) % 16 == (4 * shift if k in ('out', 'gx') else 0) for k in floats)

    def banded(nbytes):
        assert nbytes % 256 == 0
        w = torch.full((nbytes + 2 * band,), 0x5a, dtype=torch.uint8, device=DEV)
        assert (w.data_ptr() + band) % 256 == 0
        return w
    work_i = banded(lib.gd3d_sparse_conv_index_workspace_bytes(N, K, int(case['subm'])))
    work_w = banded(lib.gd3d_sparse_conv_backward_weight_workspace_bytes(R, K, Cin, Cout))
    i3 = lambda v: (ctypes.c_int32 * 3)(*v)
    _lib.check(lib.gd3d_sparse_conv_index(coors.data_ptr(), N, B, i3(case['shape']), i3(case['kernel']), i3(case['stride']), i3(case['padding']),
                                          int(case['subm']), R, work_i.data_ptr() + band, at('out_coors'), at('nbr'), None if case['subm'] else at('nbr_t'),
                                          at('num'), at('out_batch_cnt'), stream), 'gd3d_sparse_conv_index')
    _lib.check(lib.gd3d_sparse_conv_forward(X.data_ptr(), W.data_ptr(), None if bias is None else bias.data_ptr(), at('nbr'), at('num'), N, R, K, Cin, Cout,
                                            at('out'), stream), 'gd3d_sparse_conv_forward')
    _lib.check(lib.gd3d_sparse_conv_backward_input(gY.data_ptr(), W.data_ptr(), at('nbr') if case['subm'] else at('nbr_t'), int(case['subm']), N, R, K, Cin,
                                                   Cout, at('gx'), stream), 'gd3d_sparse_conv_backward_input')
    _lib.check(lib.gd3d_sparse_conv_backward_weight(X.data_ptr(), gY.data_ptr(), at('nbr'), at('num'), N, R, K, Cin, Cout, work_w.data_ptr() + band, at('gw'),
                                                    None if bias is None else at('gb'), stream), 'gd3d_sparse_conv_backward_weight')
    torch.cuda.synchronize()
    sizes = dict(ints, num=2, **floats)
    for k, t in bufs.items():
        guard = S if t.dtype == torch.float32 else 77
        assert (t[:off[k]] == guard).all() and (t[off[k] + sizes[k]:] == guard).all(), f'{k}: a guard band was written'
    for k in INT_OUTPUTS:
        if want[k] is None:
            assert (bufs[k] == 77).all(), 'nbr_t of a submanifold index is not written'
        else:
            assert np.array_equal(bufs[k][G:-G].cpu().numpy().reshape(want[k].shape), want[k]), k
    for w in (work_i, work_w):
        assert (w[:band] == 0x5a).all() and (w[-band:] == 0x5a).all(), 'a workspace band was written'
    o64 = ref.expected_values(name)[0]
    got = {k: (None if o64[k] is None else bufs[k][off[k]:off[k] + floats[k]].cpu().numpy().reshape(o64[k].shape)) for k in floats}
    check_values(name, DEV, got)                                  # every element written: no sentinel survives the bound
    return got


@pytest.mark.parametrize('name', GUARD_CASES)
def test_nothing_is_written_beyond_the_outputs_and_the_workspaces(name):
    run_c_entries_between_bands(name, 0)


@pytest.mark.parametrize('name', [n for n in GUARD_CASES if ref.CASES[n]['cout'] % 4 == 0])
def test_out_and_gx_4_bytes_past_an_aligned_address_take_the_element_wise_stores(name):
    """Co % 4 == 0 with a misaligned base: the scalar stores of the same arithmetic, the same bits, nothing outside the outputs"""
    assert ref.CASES[name]['cin'] % 4 == 0
    got, aligned = run_c_entries_between_bands(name, 1), run_c_entries_between_bands(name, 0)
    for k in ('out', 'gx'):
        assert got[k].tobytes() == aligned[k].tobytes(), f'{name}: {k} differs between the 16-byte and the element-wise stores'


@pytest.mark.parametrize('geom', ['subm', 's2p1'])
def test_index_over_300_samples(geom):
    check_many_samples(geom, DEV)
    twin, got = run_index(ref.many_samples_case(geom), 'cpu'), run_index(ref.many_samples_case(geom), DEV)
    for k in INT_OUTPUTS:
        if getattr(got, k) is not None:
            assert torch.equal(getattr(got, k).cpu(), getattr(twin, k)), f'{geom}: {k} differs from the twin'


def test_static_form_at_max_out_0_and_1():
    check_max_out_0_and_1(DEV)


def test_batch_size_zero_leaves_every_row_inactive():
    check_batch_zero(DEV)


@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p1_9x12x10_c5_16'])
def test_a_non_finite_value_reaches_only_what_reads_it(name):
    check_nonfinite_containment(name, DEV)


def test_modules_equal_the_functional_form():
    check_modules_equal_functional(DEV)


def test_layers_sharing_an_indice_key_build_one_index(monkeypatch):
    check_shared_indice_key(DEV, monkeypatch)


def test_dense_and_its_gradient_equal_index_put_and_gather():
    check_dense(DEV)


@pytest.mark.parametrize('grid', ENC_SHAPES)
def test_mlvl_sparse_encoder_follows_the_per_layer_fp64_oracle(grid):
    check_encoder(DEV, grid)


def test_bad_arguments_raise():
    check_bad_arguments(DEV)
    with pytest.raises(RuntimeError, match='is on'):
        case = ref.CASES['subm_rows_tile']
        amd.sparse_conv(torch.zeros(64, 4), torch.zeros(27, 4, 8), None, run_index(case, DEV))


def test_static_form_under_graph_capture():
    """sparse_conv_index(max_out=...) -> sparse_conv -> a second sparse_conv on the same index -> a strided layer -> sparse_to_dense, on the
    static rows of a voxelization (tail rows -1): recorded on a single stream in ONE graph, replayed on fresh coordinates and features in
    the static buffers, and compared with the eager run bit for bit"""
    shape, B, N, MO = (9, 12, 10), 2, 200, 160
    rng = np.random.default_rng(12)

    def rows(n_active):
        c = np.full((N, 4), -1, np.int32)
        c[:n_active] = ref.random_coors(rng, n_active, shape, B)
        return torch.from_numpy(c)
    coors, feats = rows(180).to(DEV), torch.randn(N, 16, device=DEV)
    torch.manual_seed(13)
    w1, w2, w3, b1 = torch.randn(27, 16, 16, device=DEV) / 20, torch.randn(27, 16, 16, device=DEV) / 20, torch.randn(27, 16, 32, device=DEV) / 20, torch.randn(16, device=DEV)

    def step():
        sub = amd.sparse_conv_index(coors, shape, B, 3, 1, 1, True)
        y = amd.sparse_conv(amd.sparse_conv(feats, w1, b1, sub), w2, None, sub)
        down = amd.sparse_conv_index(coors, shape, B, 3, 2, 1, False, max_out=MO)
        z = amd.sparse_conv(y, w3, None, down)
        return [sub.nbr, y, down.out_coors, down.nbr, down.nbr_t, down.num, down.out_batch_cnt, z, amd.sparse_to_dense(z, down.out_coors, down.out_shape, B)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = [t.clone() for t in step()]                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, warm):
        assert torch.equal(got, want)
    coors.copy_(rows(120))
    feats.copy_(torch.randn(N, 16, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[2], warm[2]) and 0 < int(eager[5][0]) <= MO
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
    want = ref.index_ref(coors.cpu().numpy(), shape, B, *ref.GEOMS['s2p1'], max_out=MO)
    assert np.array_equal(captured[2].cpu().numpy(), want['out_coors']) and np.array_equal(captured[4].cpu().numpy(), want['nbr_t'])
    assert not captured[1][120:].any() and not captured[7][int(want['num'][0]):].any(), 'tail rows are zero, bias or not'


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible devices')
def test_a_call_on_another_devices_tensors_leaves_the_callers_device_current():
    torch.cuda.set_device(0)
    name = 's2p1_9x12x10_c5_16'
    want = ref.expected_index(name)
    got = run_index(ref.CASES[name], 'cuda:1')
    assert torch.cuda.current_device() == 0
    for k in INT_OUTPUTS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k
    check_values(name, 'cuda:1')
    assert torch.cuda.current_device() == 0
