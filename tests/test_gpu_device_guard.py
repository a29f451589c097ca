"""The wrappers launch on the device of their TENSORS, whichever device is current, and leave the caller's device current
(_host.on_device under _host.call_extras).  Needs two visible devices."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd

pytestmark = pytest.mark.gpu


def _targets(dev):
    boxes = torch.tensor([[-1.3, 0.7, -0.5, 1.6, 3.9, 1.5, 0.3], [2.1, -2.2, -0.4, 0.6, 0.8, 1.7, -1.1]], device=dev)
    labels = torch.tensor([0, 1], device=dev)
    cfg = dict(grid_size=[32, 32, 1], point_cloud_range=[-3.2, -3.2, -3.0, 3.2, 3.2, 1.0], voxel_size=[0.2, 0.2, 4.0],
               out_size_factor=4, gaussian_overlap=0.1, min_radius=2)
    heat, anno, pos, start = amd.extras.center_head_get_targets([boxes], [labels], [['car'], ['pedestrian']], cfg, padded=True)
    return [h.cpu() for h in heat] + [anno.cpu(), pos.cpu(), start.cpu()]


def _cls_dir(dev):
    g = torch.Generator().manual_seed(7)
    cls = torch.randn((1, 2, 4, 4), generator=g).to(dev).requires_grad_(True)
    dirs = torch.randn((1, 4, 4, 4), generator=g).to(dev).requires_grad_(True)
    labels = torch.randint(0, 2, (1, 32), generator=g).to(dev)          # 1 = num_classes = background
    dir_targets = torch.randint(0, 2, (1, 32), generator=g).to(dev)
    weights = torch.ones((1, 32), device=dev)
    l_cls, l_dir = amd.extras.anchor_head_cls_dir_loss(dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0),
                                                       dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.2), cls, dirs,
                                                       labels, weights, dir_targets, (labels == 0).float(), 1, num_total_samples=3.0)
    (l_cls + l_dir).backward()
    return [l_cls.detach().cpu(), l_dir.detach().cpu(), cls.grad.cpu(), dirs.grad.cpu()]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible devices')
@pytest.mark.parametrize('call', [_targets, _cls_dir])
def test_a_call_on_another_devices_tensors_leaves_the_callers_device_current(call):
    """1 sample, 2 boxes, an 8 x 8 map / (1, 2 * 1, 4, 4) class maps on cuda:1 while cuda:0 is current: the results equal those
    of the same call on cuda:0 tensors bit for bit, and cuda:0 is still current afterwards."""
    torch.cuda.set_device(0)
    want = call(torch.device('cuda:0'))
    got = call(torch.device('cuda:1'))
    assert torch.cuda.current_device() == 0
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(x, y)
