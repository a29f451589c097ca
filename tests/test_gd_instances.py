"""tests/gd_instances.py lists every compiled (loss type, fun, flag) instance of the GD-loss kernels.  Here the same set is
derived from the product itself: its loss types and funs (gd_loss.LOSS_TYPES / FUNS), the fun domain that GDLoss.__init__
asserts and the `_cpu` twin's launcher enforces (check_instance() of csrc/gd3d_instances.h, which the HIP launchers call
too), and the flags.  A loss type or fun the
product gains fails here until the list covers it.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

import gd_instances


def _domain(lt, fun):
    """the fun domain per loss type (gaussian_distance_loss.py:267-270; check_instance in csrc/gd3d_instances.h)"""
    return fun in (('nlog', 'expm1', 'none') if lt == 'kfiou3d' else ('log1p', 'none'))


def test_instance_list_is_every_instance_the_product_accepts():
    from mmdet3d_gaussian_amd import gd_loss
    derived = set()
    for lt in gd_loss.LOSS_TYPES:
        for fun in gd_loss.FUNS:
            if _domain(lt, fun):
                # kfiou3d accepts `sqrt` and ignores it: one instance per fun, flag off
                for flag in ((False,) if lt == 'kfiou3d' else (True, False)):
                    derived.add((lt, fun, flag))
    assert len(gd_instances.INSTANCES) == len(set(gd_instances.INSTANCES))
    assert set(gd_instances.INSTANCES) == derived
    assert len(derived) == 27
    assert tuple(gd_loss.LOSS_TYPES) == gd_instances.LOSS_TYPES


@pytest.mark.parametrize('lt', gd_instances.LOSS_TYPES)
def test_fun_domain_is_the_one_the_product_enforces(lt):
    """GDLoss's constructor and the `_cpu` twin's launcher accept exactly the funs of the domain rule above."""
    import mmdet3d_gaussian_amd as amd
    from mmdet3d_gaussian_amd import _lib, gd_loss
    lib = amd.load_library()
    p = torch.rand(3, 7) + 0.5
    t = torch.rand(3, 7) + 0.5
    loss = torch.empty(3)
    for fun in gd_loss.FUNS:
        if _domain(lt, fun):
            amd.GDLoss(lt, fun=fun)
        else:
            with pytest.raises(AssertionError):
                amd.GDLoss(lt, fun=fun)
        for flag in (True, False):
            prm = gd_loss.make_params(lt, fun, 1.0, 1.0, (0, 0, 0.5), {gd_instances.flag_name(lt): flag})
            rc = lib.gd3d_loss_fused_cpu(ctypes.byref(prm), p.data_ptr(), t.data_ptr(), None, None, 3, 1.0, loss.data_ptr(),
                                         None, None, None, None, 1)
            assert (rc == 0) == _domain(lt, fun), (lt, fun, flag, rc)


def test_kfiou3d_flag_is_accepted_and_ignored():
    """why kfiou3d has one instance per fun: `sqrt` changes nothing in the product (nor in the fp64 oracle)"""
    import oracle
    import mmdet3d_gaussian_amd as amd
    g = torch.Generator().manual_seed(0)
    t = torch.rand(64, 7, generator=g) * 4 + 0.5
    p = t + torch.randn(64, 7, generator=g) * 0.1
    for fun in ('nlog', 'expm1', 'none'):
        a = amd.GDLoss('kfiou3d', fun=fun, reduction='none', sqrt=True)(p, t)
        b = amd.GDLoss('kfiou3d', fun=fun, reduction='none', sqrt=False)(p, t)
        assert torch.equal(a, b)
        r = [oracle.gd_loss(p.numpy(), t.numpy(), oracle.make_params('kfiou3d', fun=fun, sqrt=s))['loss'] for s in (True, False)]
        assert np.array_equal(r[0], r[1])


def test_hyper_parameter_draws():
    for i, (lt, fun, flag) in enumerate(gd_instances.INSTANCES):
        d = gd_instances.hyper(i, 'default')
        assert d['alpha'] == 1.0 and d['center_offset'] == (0.0, 0.0, 0.5) and d[gd_instances.flag_name(lt)] == flag
        h = gd_instances.hyper(i, 'drawn')
        assert h == gd_instances.hyper(i, 'drawn')                      # seeded
        assert h['tau'] in (0.0, 0.5, 1.0, 1.75, 3.0) and 0.3 <= h['alpha'] <= 3.0 and np.float32(h['alpha']) == h['alpha']
        assert all(-0.5 <= c <= 0.5 and np.float32(c) == c for c in h['center_offset'])
        assert h[gd_instances.flag_name(lt)] == (True if lt == 'kfiou3d' else flag)
    assert sorted({gd_instances.count(i) for i in range(len(gd_instances.INSTANCES))}) == sorted(gd_instances.COUNTS)
