"""Every (loss type, fun, flag) instance of the GD-loss kernels, written out once for the suites that sweep them.

The GD-loss kernels are templates: `fused_kernel` (csrc/gd3d_loss.hip), `head_anchor_kernel` (csrc/gd3d_anchor_head.hip)
and `head_center_kernel` (csrc/gd3d_center_head.hip) are compiled once per (loss type, fun, flag), where flag is `normalize`
for gwd3d and `sqrt` for the others; csrc/gd3d_instances.h is the one table every launcher takes its instance from.  The fun
domain is the one its check_instance() enforces (GDLoss.__init__ asserts the same, gaussian_distance_loss.py:267-270): kfiou3d takes
{none, expm1, nlog}, every other loss {none, log1p}.  kfiou3d accepts `sqrt` and ignores it (ref :228): it has one
instance per fun, compiled with the flag off.  tests/test_gd_instances.py derives this set from the product and asserts it
equals INSTANCES, so a new loss type or fun fails there until it is listed here.

`hyper(i, kind)` gives instance i its hyper-parameters: the reference defaults (`kind='default'`) or a seeded non-default
draw (`kind='drawn'`) from the distributions tests/test_param_sweep.py's `_case` uses."""
import numpy as np

LOSS_TYPES = ('gwd3d', 'kld3d', 'bd3d', 'jd3d', 'kld3d_symmax', 'kld3d_symmin', 'kfiou3d')

INSTANCES = tuple(
    [(lt, fun, flag) for lt in LOSS_TYPES[:6] for fun in ('log1p', 'none') for flag in (True, False)] +
    [('kfiou3d', fun, False) for fun in ('nlog', 'expm1', 'none')])

# positive counts spread deterministically over the instances (tile edges of the 256-thread head kernels, and a large one)
COUNTS = (1, 255, 256, 257, 5000)


def flag_name(lt):
    return 'normalize' if lt == 'gwd3d' else 'sqrt'


def ident(inst):
    lt, fun, flag = inst
    return f'{lt}.{fun}.{flag_name(lt)}={int(flag)}'


def count(i):
    return COUNTS[i % len(COUNTS)]


def hyper(i, kind):
    """GDLoss keyword arguments of instance i (fun, tau, alpha, center_offset and its flag).

    'default': alpha 1, center_offset (0, 0, 0.5) and tau 1, as the shipped configs set it (kfiou3d: tau 0, which it ignores).
    'drawn'  : tau in {0, 0.5, 1, 1.75, 3}, alpha and center_offset fp32 in [0.3, 3] and
               [-0.5, 0.5]^3 (gd3d_params carries floats), seeded by i; kfiou3d
               is given sqrt=True, which must change nothing."""
    lt, fun, flag = INSTANCES[i]
    kw = dict(fun=fun)
    if kind == 'default':
        kw.update(tau=0.0 if lt == 'kfiou3d' else 1.0, alpha=1.0, center_offset=(0.0, 0.0, 0.5))
    elif kind == 'drawn':
        rng = np.random.default_rng(1000 + i)
        kw.update(tau=float(rng.choice([0.0, 0.5, 1.0, 1.75, 3.0])), alpha=float(np.float32(rng.uniform(0.3, 3.0))),
                  center_offset=tuple(float(np.float32(x)) for x in rng.uniform(-0.5, 0.5, 3)))
    else:
        raise ValueError(kind)
    kw[flag_name(lt)] = True if (lt == 'kfiou3d' and kind == 'drawn') else flag
    return kw
