#!/usr/bin/env python3
"""Live-row batch normalisation on the GPU (gd3d_sparse_bn_*), us per call, against what the unconverted modules run —
`nn.BatchNorm1d.train()` -> `nn.ReLU` (plus the identity add of a block tail) — on the same tensors in the same process, at the row
counts and widths of PV-RCNN's levels: 64 000 x 16, 36 217 x 32 and 9 292 x 64, in fp32 and in bf16, every row live (the torch chain has
no notion of a dead row: with dead rows it computes something else).
Per shape and type, in training mode with the ReLU:
  forward            : ours = sparse_batch_norm(..., activation='relu')               chain = relu(bn(x))
  forward + backward : the same followed by autograd.grad w.r.t. features, weight and bias
  block tail         : with the residual                                               chain = relu(bn(x) + identity)
with the kernel launches of both sides, the bytes each of our launches has to move (from the shapes) beside an in-process copy of the
same size, and a converted against an unconverted `MlvlSparseEncoder.train()` step, forward + backward, on `pvrcnn_voxelize`'s voxels.
Per side: device events around back-to-back calls, the median of 5 batches after a warm-up; launches and the kernels' device time from
torch.profiler; forward + backward also as a captured graph, replayed (eager calls of this size are bound by the host on both sides)."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
from sparse_conv_time import B, SHAPE, VOXEL_LAYER, launches, synthetic_points, timed  # noqa: E402

dev = torch.device('cuda:0')
LEVELS = ((64000, 16, SHAPE), (36217, 32, (21, 800, 704)), (9292, 64, (11, 400, 352)))


def copy_us(nbytes):
    """an in-process device copy that moves `nbytes` in all (half read, half written), us"""
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), 50)[0]


def replayed(fn):
    """fn captured into one graph on a side stream -> the median us of a replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return timed(graph.replay, 50)[0]


def main():
    rng = np.random.default_rng(11)
    relu = torch.nn.ReLU()
    for rows, C, shape in LEVELS:
        cells = rng.choice(B * shape[0] * shape[1] * shape[2], size=rows, replace=False)
        plane = shape[1] * shape[2]
        c = np.stack([cells // (shape[0] * plane), cells // plane % shape[0], cells // shape[2] % shape[1], cells % shape[2]], 1).astype(np.int32)
        coors = torch.from_numpy(c).to(dev)
        for kind, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
            torch.manual_seed(0)
            x = (torch.randn(rows, C, device=dev) * 1.5 + 0.3).to(dtype).requires_grad_(True)
            identity, gy = torch.randn(rows, C, device=dev).to(dtype), torch.randn(rows, C, device=dev).to(dtype)
            bn = torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).to(dev).train()
            ours = amd.SparseBatchNorm1d.from_batchnorm(copy.deepcopy(bn), 'relu')
            wrt = lambda m: [x, m.weight, m.bias]
            f_ours = lambda res=None: amd.sparse_batch_norm(x, coors, shape, B, ours.weight, ours.bias, ours.running_mean, ours.running_var, ours.num_batches_tracked,
                                                            training=True, momentum=0.01, eps=1e-3, residual=res, activation='relu')
            sides = {
                'forward': dict(ours=lambda: f_ours(), chain=lambda: relu(bn(x))),
                'forward + backward': dict(ours=lambda: torch.autograd.grad(f_ours(), wrt(ours), gy), chain=lambda: torch.autograd.grad(relu(bn(x)), wrt(bn), gy)),
                'block tail forward': dict(ours=lambda: f_ours(identity), chain=lambda: relu(bn(x) + identity)),
                'block tail forward + backward': dict(ours=lambda: torch.autograd.grad(f_ours(identity), wrt(ours), gy),
                                                      chain=lambda: torch.autograd.grad(relu(bn(x) + identity), wrt(bn), gy)),
            }
            es, array = x.element_size(), rows * C * x.element_size()
            # what our launches have to move: the statistics sweep reads the rows twice (the second time out of the cache) and the coordinates,
            # the normalising sweep reads the rows (+ the residual) and the coordinates and writes the output
            moved = {'forward': dict(stats=2 * array + 32 * rows, norm=2 * array + 16 * rows),
                     'block tail forward': dict(stats=2 * array + 32 * rows, norm=3 * array + 16 * rows)}
            for tag, pair in sides.items():
                rec = dict(what=f'{rows} x {C}, {kind}, {tag}', element_bytes=es)
                with torch.no_grad():
                    a, b = f_ours(identity if 'tail' in tag else None), relu(bn(x) + identity) if 'tail' in tag else relu(bn(x))
                rec['max_abs_diff_ours_vs_chain'] = float((a.float() - b.float()).abs().max())
                for side in ('ours', 'chain'):
                    med, low = timed(pair[side], 50)
                    n, dur = launches(pair[side])
                    rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
                    rec[f'{side}_kernels_device_us_sum'] = round(sum(dur.values()), 1)
                    if side == 'ours':
                        rec['ours_kernels_device_us'] = dur
                    if 'backward' in tag:                                # the step as a captured graph: what is left when the host is out of the way
                        rec[f'{side}_graph_replay_us_median'] = replayed(pair[side])
                rec['chain_over_ours'] = round(rec['chain_us_median'] / rec['ours_us_median'], 2)
                rec['ours_not_slower_than_chain'] = bool(rec['ours_us_median'] <= rec['chain_us_median'])
                if tag in moved:
                    rec['bytes_moved_by_launch'] = moved[tag]
                    rec['copy_of_the_same_bytes_us'] = {k: copy_us(v) for k, v in moved[tag].items()}
                print(json.dumps(rec), flush=True)

    vox = amd.pvrcnn_voxelize([synthetic_points(np.random.default_rng(7)).to(dev) for _ in range(B)], VOXEL_LAYER, True)
    coors, feats = vox['coors'], vox['voxel_features'].float().contiguous()
    for kind, dtype in (('fp32', None), ('bf16', torch.bfloat16)):
        torch.manual_seed(1)
        enc = amd.MlvlSparseEncoder(in_channels=feats.size(1), sparse_shape=list(SHAPE), compute_dtype=dtype).to(dev).train()
        conv = copy.deepcopy(enc).convert_norm()
        rec = dict(what=f'MlvlSparseEncoder.train() forward + backward, {kind}', voxels=coors.size(0))
        for side, net in (('converted', conv), ('unconverted', enc)):
            params = [p for p in net.parameters()]

            def step(net=net, params=params):
                out = net(feats, coors, B)['spatial_features']
                return torch.autograd.grad(out.float().sum(), params)
            med, low = timed(step, 5)
            n, _ = launches(step)
            rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
        rec['unconverted_over_converted'] = round(rec['unconverted_us_median'] / rec['converted_us_median'], 2)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
