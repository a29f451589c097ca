"""The fused sparse convolution layer on the MI355X (gd3d_sparse_conv_forward_fused[_16]; csrc/sparse_conv.hip, csrc/sparse_conv_16.hip;
DESIGN.md §3.20): the checks of tests/test_cpu_sparse_conv_fused.py on cuda:0, through its helpers — every combination of scale,
residual and ReLU in fp32, fp16 and bf16 within the derived bound and bit-identical from run to run; bit identity with the plain
entry; dead rows; the C entries between guard bands with the residual aligned and shifted; non-finite values; the gradients; the fused
encoders layer by layer — and the static form of a fused strided + fused submanifold stack recorded and replayed in one graph."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_ref as ref
from sparse_twins import refuse_twins
from test_cpu_sparse_conv_fused import (DEAD_CASES, FUSED_CASES, KINDS, check_bit_identity, check_dead_rows, check_fused_encoder, check_fused_values,
                                        check_gradients, check_guards, check_nonfinite, randomise_batchnorms, run_fused)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', FUSED_CASES)
def test_fused_within_the_derived_bound_in_every_combination_and_the_same_bits_from_run_to_run(name, kind):
    check_fused_values(name, DEV, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p011_7x11x13_c3_7', 's2p1_channel_tiles_c24_40', 'subm_7x11x13_c64_64'])
def test_shift_alone_and_a_scale_of_ones_give_the_plain_entrys_bits(name, kind):
    check_bit_identity(name, DEV, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', DEAD_CASES)
def test_dead_rows_are_exactly_zero_under_a_shift_and_a_nan_residual(name, kind):
    check_dead_rows(name, DEV, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_channel_tiles_c32_32', 's2p011_7x11x13_c3_7', 's2p1_max_out_above', 'subm_7x11x13_c64_64', 's2p1_max_out_far_above'])
def test_c_entries_between_bands_with_the_residual_aligned_and_shifted(name, kind):
    """the 16-byte residual loads fall back to element-wise loads on their own, whichever way the output is stored: the same bits"""
    check_guards(name, DEV, kind)


@pytest.mark.parametrize('kind', KINDS)
def test_non_finite_values_pass_and_stay_where_they_are(kind):
    check_nonfinite(DEV, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p1_9x12x10_c5_16'])
def test_gradients_follow_the_fp64_chain(name, kind):
    check_gradients(name, DEV, kind)


@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
@pytest.mark.parametrize('block_type', ['conv_module', 'basicblock'])
def test_fused_encoder_follows_the_unfused_modules_layer_by_layer(block_type, kind, monkeypatch):
    check_fused_encoder(DEV, block_type, kind, monkeypatch)


def test_device_tensors_never_reach_a_twin(monkeypatch):
    """a `_cpu` twin called with the address of device memory would fault the process: the fused twins are replaced by functions that raise"""
    refuse_twins(monkeypatch, lambda name: 'forward_fused' in name and name.endswith('_cpu'))
    with pytest.raises(AssertionError, match='_cpu was called'):          # the replacement is in place: CPU tensors do reach it
        run_fused('subm_9x12x10_c4_16', 'cpu', 'bf16', True, True, 'relu')
    for kind in KINDS:
        assert run_fused('subm_9x12x10_c4_16', DEV, kind, True, True, 'relu').any()


def test_static_form_of_a_fused_two_layer_stack_under_graph_capture():
    """fused SparseConv3d(k3 s2 p1, max_out) + BatchNorm + ReLU -> fused SubMConv3d + BatchNorm + ReLU in bf16, forward and backward, on the
    static rows of a voxelization (tail rows -1): recorded on a single stream in ONE graph, replayed on fresh coordinates, features and
    upstream gradient in the static buffers, and compared with the eager run of the same inputs bit for bit.  The rows past the count
    are zero through both layers: the contract of `sparse_conv` survives the module."""
    shape, B, N, MO = (9, 12, 10), 2, 200, 230        # 248 outputs of the first 180 rows (capped), 216 of the fresh 120 (a tail)
    rng = np.random.default_rng(17)

    def rows(n_active):
        c = np.full((N, 4), -1, np.int32)
        c[:n_active] = ref.random_coors(rng, n_active, shape, B)
        return torch.from_numpy(c)
    torch.manual_seed(18)
    net = amd.SparseSequential(amd.SparseConv3d(16, 32, 3, 2, 1, bias=True, max_out=MO, compute_dtype=torch.bfloat16), torch.nn.BatchNorm1d(32), torch.nn.ReLU(),
                               amd.SubMConv3d(32, 32, 3, bias=False, compute_dtype=torch.bfloat16), torch.nn.BatchNorm1d(32), torch.nn.ReLU())
    net = amd.fuse_sparse_conv_bn(randomise_batchnorms(net, 19).to(DEV).eval())
    assert [type(m) for m in net] == [amd.FusedSparseConv] * 2 and net[0].max_out == MO
    params = list(net.parameters())
    assert len(params) == 3
    coors, feats, gy = rows(180).to(DEV), torch.randn(N, 16, device=DEV).requires_grad_(True), torch.randn(MO, 32, device=DEV).bfloat16()

    def step():
        y = net(amd.SparseConvTensor(feats, coors, shape, B))
        return [y.indices, y.features] + list(torch.autograd.grad(y.features, [feats] + params, gy))

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
    with torch.no_grad():
        coors.copy_(rows(120))
        feats.copy_(torch.randn(N, 16, device=DEV))
        gy.copy_(torch.randn(MO, 32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert captured[1].dtype == torch.bfloat16 and captured[2].dtype == torch.float32 and captured[3].dtype == torch.float32
    assert not torch.equal(eager[0], warm[0]) and not torch.equal(eager[1], warm[1])
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
    kept = int(ref.index_ref(coors.cpu().numpy(), shape, B, *ref.GEOMS['s2p1'], max_out=MO)['num'][0])
    assert 0 < kept < MO and captured[1][:kept].any() and not captured[1][kept:].any(), 'tail rows are zero, shift or not'
    assert not captured[2][120:].any() and all(torch.isfinite(t).all() for t in captured[1:])
