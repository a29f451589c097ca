"""The sparse decoder on the MI355X: the checks of tests/test_cpu_sparse_inverse.py and tests/test_cpu_sparse_pool.py on
cuda:0, through their helpers — the inverse convolution on every geometry, channel pair and dead layout within `sparse_conv`'s bounds, the
pooling kernels on every channel path, row count and value case bit-equal to the oracle — and what only the device can show: the same
bits from run to run, the device against the twin, and a static conv -> pool -> inverse conv stack in one graph."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_ref as ref
import sparse_decoder_ref as dref
import test_cpu_sparse_inverse as inv
import test_cpu_sparse_pool as pool
from sparse_twins import refuse_twins

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---- the inverse convolution -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('geom', sorted(inv.GEOMS))
def test_inverse_every_geometry(geom):
    inv.check_inverse(DEV, 'fp32', geom, 16, 32)


@pytest.mark.parametrize('pair,kind', inv.PAIR_CASES, ids=lambda v: v if isinstance(v, str) else f'{v[0]}_{v[1]}')
def test_inverse_channel_pairs_in_every_type(pair, kind):
    inv.check_inverse(DEV, kind, 'k3s2p1_remainder', *pair)


@pytest.mark.parametrize('kind', inv.KINDS)
def test_inverse_without_bias_and_rows_without_a_neighbour_under_a_bias(kind):
    inv.check_inverse(DEV, kind, 'k2s2p0_remainder', 16, 32, bias=False)
    got, lone = inv.check_inverse(DEV, kind, 'k2s2p0_remainder', 5, 4, bias=True)
    assert lone.sum() > 20


@pytest.mark.parametrize('max_out', ['above', 'below'])
@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
def test_inverse_static_forward_index(kind, max_out):
    inv.check_inverse(DEV, kind, 'k3s2p1_remainder', 16, 32, max_out=max_out)


def test_inverse_static_form_carries_the_exact_forms_bits():
    inv.check_static_against_exact(DEV)


@pytest.mark.parametrize('kind', ['fp32', 'fp16'])
def test_inverse_inactive_input_rows(kind):
    inv.check_inverse(DEV, kind, 'k3s2p1_divides', 16, 32, inactive=True)


def test_inverse_modules_and_bad_arguments():
    inv.check_modules(DEV)


@pytest.mark.parametrize('kind', inv.KINDS)
def test_fused_inverse_module_within_the_fused_bound(kind):
    inv.check_fused_module(DEV, kind)


@pytest.mark.parametrize('kind', inv.KINDS)
def test_inverse_same_bits_from_run_to_run(kind):
    (X, W, b, gY), _, _, _ = inv.expected('k3s2p1_remainder', 16, 32, True, kind)
    index = inv.run_index('k3s2p1_remainder', DEV)
    first, second = inv.run_inverse(DEV, kind, index, X, W, b, gY), inv.run_inverse(DEV, kind, index, X, W, b, gY)
    assert all(np.array_equal(first[k], second[k]) for k in first)


# ---- the max pooling -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', pool.KINDS)
@pytest.mark.parametrize('geom', sorted(pool.GEOMS))
def test_pool_every_window_size(geom, kind):
    pool.check_geometry(DEV, kind, geom, 16)


@pytest.mark.parametrize('kind,C', [(k, c) for k in pool.KINDS for c in pool.CHANNELS[k]])
def test_pool_every_channel_path(kind, C):
    pool.check_geometry(DEV, kind, 'k2s2', C)


@pytest.mark.parametrize('kind,name,R,C', pool.ROW_CASES, ids=lambda v: str(v))
def test_pool_row_counts_around_a_workgroup_and_past_the_grid(kind, name, R, C):
    pool.check_tables(DEV, kind, R, R + 3, 2, C, 400 + R % 89)


@pytest.mark.parametrize('kind', pool.KINDS)
@pytest.mark.parametrize('form', ['above', 'below', 'inactive'])
def test_pool_dead_rows(form, kind):
    if form == 'inactive':
        pool.check_geometry(DEV, kind, 'k3s2p1', 16, inactive=True)
    else:
        pool.check_geometry(DEV, kind, 'k3s2p1', 16, max_out=form)


@pytest.mark.parametrize('kind', pool.KINDS)
def test_pool_negative_inputs_an_inf_window_and_one_nan(kind):
    pool.check_values(DEV, kind)


@pytest.mark.parametrize('kind', pool.KINDS)
def test_pool_every_tied_input_receives_the_gradient(kind):
    pool.check_ties(DEV, kind)


@pytest.mark.parametrize('kind', pool.KINDS)
@pytest.mark.parametrize('C', [16, 20])
def test_pool_c_entries_between_guard_bands_aligned_and_one_element_off(C, kind):
    pool.check_guards_and_alignment(DEV, kind, C)


def test_pool_module_static_form_and_bad_arguments():
    pool.check_module(DEV)


@pytest.mark.parametrize('kind', pool.KINDS)
@pytest.mark.parametrize('C', [5, 64])
def test_pool_device_equals_the_twin_and_itself_bit_for_bit(C, kind):
    coors, idx, _ = pool.case_of('k3s2p1', 'below')
    X, gY = pool.draws((len(coors), C), kind, 90 + C), pool.draws((len(idx['nbr']), C), kind, 91 + C)
    first = pool.run_pool(DEV, kind, pool.run_index('k3s2p1', DEV, 'below'), X, gY)
    second = pool.run_pool(DEV, kind, pool.run_index('k3s2p1', DEV, 'below'), X, gY)
    twin = pool.run_pool('cpu', kind, pool.run_index('k3s2p1', 'cpu', 'below'), X, gY)
    for a, b, c in zip(first, second, twin):
        assert pool.same_bits(a, b) and pool.same_bits(a, c)


def test_device_tensors_never_reach_a_twin(monkeypatch):
    """a `_cpu` twin called with the address of device memory would fault the process: the twins are replaced by functions that raise"""
    refuse_twins(monkeypatch, lambda name: 'sparse_max_pool' in name and name.endswith('_cpu'))
    coors, idx, _ = pool.case_of('k2s2')
    X, gY = pool.draws((len(coors), 8), 'fp32', 1), pool.draws((len(idx['nbr']), 8), 'fp32', 2)
    with pytest.raises(AssertionError, match='_cpu was called'):
        pool.run_pool('cpu', 'fp32', pool.run_index('k2s2', 'cpu'), X, gY)
    out, gx = pool.run_pool(DEV, 'fp32', pool.run_index('k2s2', DEV), X, gY)
    assert out.any() and gx.any()


# ---- SparseUNet and the static stack ---------------------------------------------------------------------------------------------------

def test_unet_shapes_row_order_and_index_builds(monkeypatch):
    inv.check_unet_shapes_and_index_calls(DEV, monkeypatch)


def test_unet_every_parameter_gets_a_gradient():
    inv.check_unet_gradients(DEV, inv.UNET_SHAPE, skip=('conv_out',))
    inv.check_unet_gradients(DEV, inv.UNET_TALL)


@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
def test_unet_fused_follows_the_unfused_model_layer_by_layer(kind):
    inv.check_unet_fused(DEV, kind)


def test_unet_bf16_trains_and_converts():
    inv.check_unet_bf16_and_converted(DEV)


def test_static_conv_pool_inverse_stack_under_graph_capture():
    """SparseConv3d(k3 s2 p1, max_out) -> SparseMaxPool3d(k2 s2, max_out) -> SparseInverseConv3d over the conv's index, forward and backward on
    the static rows of a voxelization (tail rows -1): recorded on one stream in ONE graph, replayed on fresh coordinates, features and
    upstream gradients, and compared with the eager run on the same inputs bit for bit."""
    shape, B, N, MO, MP = (9, 12, 10), 2, 200, 230, 90
    rng = np.random.default_rng(27)

    def rows(n_active):
        c = np.full((N, 4), -1, np.int32)
        c[:n_active] = ref.random_coors(rng, n_active, shape, B)
        return torch.from_numpy(c)
    torch.manual_seed(28)
    conv = amd.SparseConv3d(8, 16, 3, 2, 1, bias=False, indice_key='down', max_out=MO).to(DEV)
    pooling = amd.SparseMaxPool3d(2, 2, 0, max_out=MP)
    up = amd.SparseInverseConv3d(16, 8, 3, 'down', bias=False).to(DEV)
    params = list(conv.parameters()) + list(up.parameters())
    coors, feats = rows(180).to(DEV), torch.randn(N, 8, device=DEV).requires_grad_(True)
    g_pool, g_up = torch.randn(MP, 16, device=DEV), torch.randn(N, 8, device=DEV)

    def step():
        mid = conv(amd.SparseConvTensor(feats, coors, shape, B))
        pooled, back = pooling(mid), up(mid)
        assert back.indices.data_ptr() == coors.data_ptr() and list(mid.indice_dict) == ['down']      # no read: the step is captured
        return [pooled.indices, pooled.features, back.features] + list(torch.autograd.grad([pooled.features, back.features], [feats] + params, [g_pool, g_up]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        coors.copy_(rows(120))
        feats.copy_(torch.randn(N, 8, device=DEV))
        g_pool.copy_(torch.randn(MP, 16, device=DEV))
        g_up.copy_(torch.randn(N, 8, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    eager = step()
    assert len(replayed) == len(eager) == 3 + 1 + len(params)
    for got, want in zip(replayed, eager):
        assert torch.equal(got, want)
    first = ref.index_ref(coors.cpu().numpy(), shape, B, *ref.GEOMS['s2p1'], max_out=MO)
    kept = int(ref.index_ref(first['out_coors'], first['out_shape'], B, (2, 2, 2), (2, 2, 2), (0, 0, 0), False, max_out=MP)['num'][0])
    pooled, back, gfeat = replayed[1], replayed[2], replayed[3]
    assert 0 < kept < MP and pooled[:kept].any() and not pooled[kept:].any(), 'the pooled tail rows are zero'
    assert back[:120].any() and not back[120:].any() and not gfeat[120:].any(), 'inactive input rows are zero, forward and backward'
    assert all(torch.isfinite(t).all() for t in replayed[1:])
