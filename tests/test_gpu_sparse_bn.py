"""Live-row batch normalisation on the MI355X (gd3d_sparse_bn_*; csrc/sparse_bn.hip): the checks of
tests/test_cpu_sparse_bn.py on cuda:0, through its helpers — every channel path, row counts around the tile and past the partial cap,
every dead layout with NaN in the dead rows, every mode, in fp32, fp16 and bf16, within the derived bound and bit-identical from run to
run; the static against the exact form; the ill-conditioned variance; the C entries between guard bands; non-finite values; the
converted encoders — and a static conv -> norm -> conv -> norm + residual stack, forward and backward in training mode, in one graph."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_bn_ref as bref
import sparse_conv_ref as ref
from sparse_bn_ref import KINDS
from sparse_twins import refuse_twins
from test_cpu_sparse_bn import (CHANNELS, LAYOUTS, MODES, ROW_CASES, check_case, check_converted_encoder, check_guards, check_ill_conditioned, check_nonfinite,
                                check_static_against_exact, layout, operands, rows_layout, run_ours)
from test_cpu_sparse_conv_fused import randomise_batchnorms

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C', CHANNELS)
def test_every_channel_path_within_the_bound_and_the_same_bits_from_run_to_run(C, kind):
    check_case(DEV, kind, *layout('subm_inactive_rows_scattered_and_tail'), C, 100 + C, f'channels C={C}')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ROW_CASES)
def test_row_counts_around_the_tile_and_past_the_cap(name, kind):
    check_case(DEV, kind, *rows_layout(*ROW_CASES[name]), 16, 200 + ROW_CASES[name][0] % 97, name)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', LAYOUTS)
def test_dead_layouts_nan_in_dead_rows(name, kind):
    check_case(DEV, kind, *layout(name), 16, 300, name)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('mode', MODES, ids=lambda m: ''.join(k[:2] + str(int(v)) for k, v in m.items()))
def test_all_modes(mode, kind):
    check_case(DEV, kind, *layout('subm_inactive_block'), 32, 400, 'modes ' + ' '.join(k for k, v in mode.items() if v), **mode)


def test_static_form_agrees_with_the_exact_form_and_batchnorm1d_does_not():
    check_static_against_exact(DEV)


@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
def test_ill_conditioned_variance(kind):
    check_ill_conditioned(DEV, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C', [16, 20, 7])
def test_c_entries_between_guard_bands_aligned_and_shifted(C, kind):
    check_guards(DEV, kind, C)


@pytest.mark.parametrize('kind', KINDS)
def test_a_non_finite_element_stays_in_its_channel(kind):
    check_nonfinite(DEV, kind)


@pytest.mark.parametrize('block_type', ['conv_module', 'basicblock'])
def test_converted_encoder_trains_next_to_the_unconverted_one(block_type, monkeypatch):
    check_converted_encoder(DEV, block_type, monkeypatch)


def test_device_tensors_never_reach_a_twin(monkeypatch):
    """a `_cpu` twin called with the address of device memory would fault the process: the twins are replaced by functions that raise"""
    refuse_twins(monkeypatch, lambda name: 'sparse_bn' in name and name.endswith('_cpu'))
    coors, shape, B = layout('subm_inactive_block')
    live = bref.live_rows(coors, shape, B)
    with pytest.raises(AssertionError, match='_cpu was called'):          # the replacement is in place: CPU tensors do reach it
        run_ours('cpu', 'bf16', coors, shape, B, operands(len(coors), 16, 1, 'bf16'), live, 0.0)
    for kind in KINDS:
        assert run_ours(DEV, kind, coors, shape, B, operands(len(coors), 16, 1, kind), live, 0.0)['out'].any()


def test_static_stack_trains_under_graph_capture():
    """SparseConv3d(k3 s2 p1, max_out) -> SparseBatchNorm1d('relu') -> SubMConv3d -> SparseBatchNorm1d with a residual, forward and backward
    in TRAINING mode on the static rows of a voxelization (tail rows -1): recorded on one stream in ONE graph, replayed on fresh
    coordinates, features and upstream gradient, and compared with the eager run on the same inputs bit for bit — outputs, gradients, running
    buffers and batch counters.  The rows past the count stay zero through both norms."""
    shape, B, N, MO = (9, 12, 10), 2, 200, 230
    rng = np.random.default_rng(17)

    def rows(n_active):
        c = np.full((N, 4), -1, np.int32)
        c[:n_active] = ref.random_coors(rng, n_active, shape, B)
        return torch.from_numpy(c)
    torch.manual_seed(18)
    conv1, bn1 = amd.SparseConv3d(16, 32, 3, 2, 1, bias=False, max_out=MO), amd.SparseBatchNorm1d(32, activation='relu')
    conv2, bn2 = amd.SubMConv3d(32, 32, 3, bias=False), amd.SparseBatchNorm1d(32)
    net = randomise_batchnorms(torch.nn.ModuleList([conv1, bn1, conv2, bn2]), 19).to(DEV).train()
    params = list(net.parameters())
    buffers = [b for m in (bn1, bn2) for b in (m.running_mean, m.running_var, m.num_batches_tracked)]
    start = [b.clone() for b in buffers]
    coors, feats, gy = rows(180).to(DEV), torch.randn(N, 16, device=DEV).requires_grad_(True), torch.randn(MO, 32, device=DEV)

    def step():
        h = bn1(conv1(amd.SparseConvTensor(feats, coors, shape, B)))
        y = bn2(conv2(h), residual=h.features)
        return [y.indices, y.features] + list(torch.autograd.grad(y.features, [feats] + params, gy))

    def reset():
        with torch.no_grad():
            for b, s in zip(buffers, start):
                b.copy_(s)

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
        feats.copy_(torch.randn(N, 16, device=DEV))
        gy.copy_(torch.randn(MO, 32, device=DEV))
    reset()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured] + [b.clone() for b in buffers]
    reset()
    eager = step() + buffers
    assert len(replayed) == len(eager) == 2 + 1 + len(params) + 6
    for got, want in zip(replayed, eager):
        assert torch.equal(got, want)
    kept = int(ref.index_ref(coors.cpu().numpy(), shape, B, *ref.GEOMS['s2p1'], max_out=MO)['num'][0])
    out = replayed[1]
    assert 0 < kept < MO and out[:kept].any() and not out[kept:].any(), 'tail rows are zero through both norms'
    assert all(torch.isfinite(t).all() for t in replayed[1:]) and int(bn1.num_batches_tracked) == int(start[2]) + 1
    assert not torch.equal(bn1.running_mean, start[0]) and not torch.equal(bn2.running_var, start[4])
