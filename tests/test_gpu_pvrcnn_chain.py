"""PV-RCNN's op hand-offs end to end on the MI355X: the checks of tests/test_cpu_pvrcnn_chain.py on cuda:0 — every stage boundary of
the kernels' chain EQUAL to the chained oracle of tests/pvrcnn_chain_ref.py (`bev_interpolate` within its own suite's bound), sample
isolation, the stride-mismatch control, the empty middle sample — and what only the device has: the device chain EQUAL to the `_cpu`
twins' chain on every tensor (the interpolated features too, as tests/test_gpu_vsa_bev.py compares that op's forward with its twin),
two eager runs with equal bits, and stages A-E recorded on one stream in ONE graph, replayed on fresh points with other per-sample
counts and an empty sample, against the eager run and against the oracle on those inputs."""
import pytest
import torch

import pvrcnn_chain_ref as ref
from test_cpu_pvrcnn_chain import (Chain, check_chain, check_empty_sample, check_mid_chain_truncation, check_sample_isolation,
                                   check_stride_mismatch_is_visible, differing_keys, points_side, run_chain)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.contiguous().numpy().tobytes() == b.contiguous().numpy().tobytes()


@pytest.mark.parametrize('variant', ref.VARIANTS)
def test_every_stage_boundary_equals_the_chained_oracle(variant):
    check_chain(DEV, variant)


@pytest.mark.parametrize('variant', ref.VARIANTS)
def test_the_device_chain_equals_the_twin_chain(variant):
    inp = ref.case(variant)[0]
    got, _ = run_chain(DEV, inp)
    twin, _ = run_chain('cpu', inp)
    assert set(got) == set(twin)
    for k in got:
        assert got[k].dtype == twin[k].dtype and torch.equal(got[k], twin[k]), f'{k}: the device chain is the twin chain'


def test_samples_do_not_leak_into_each_other():
    check_sample_isolation(DEV)


def test_a_stride_mismatch_is_visible():
    check_stride_mismatch_is_visible(DEV)


def test_an_empty_sample_finds_empty_balls():
    check_empty_sample(DEV)


def test_a_level_truncated_mid_chain_is_seen_downstream():
    check_mid_chain_truncation(DEV)


def test_two_eager_runs_give_equal_bits():
    inp = ref.case('truncated')[0]
    chain = Chain(inp, DEV)
    a = {k: v.cpu() for k, v in chain.run().items()}
    b = {k: v.cpu() for k, v in chain.run().items()}
    for k in a:
        assert same_bits(a[k], b[k]), k


def test_stages_a_to_e_in_one_graph():
    """hard_voxelize -> the four layers -> both keypoint sources -> both queries at three levels and both alignments -> dense() ->
    bev_interpolate, recorded on a single stream in ONE graph after a warm-up on a side stream; replayed on the recorded inputs, then
    on fresh points with other per-sample counts — sample 1 has none — in the static buffers: equal to the eager run on the same
    buffers, and to the chained oracle on those inputs"""
    variant = 'truncated'
    inp, want, _ = ref.case(variant)
    chain = Chain(inp, DEV, with_roi=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = {k: v.clone() for k, v in chain.run().items()}         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = chain.run()
    graph.replay()
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(captured[k], first[k]), k
    assert not differing_keys({k: v.cpu() for k, v in captured.items()}, points_side(want), 'graph, recorded inputs')
    chain.load(ref.replay_inputs(variant))
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.cpu() for k, v in captured.items()}
    eager = chain.run()
    assert replayed['A.voxel_batch_cnt'][1] == 0 and not torch.equal(replayed['C.raw.kp'], first['C.raw.kp'].cpu())
    for k in replayed:
        assert same_bits(replayed[k], eager[k].cpu()), k
    check_empty_sample(DEV, variant, got=replayed)
