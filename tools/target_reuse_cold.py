"""Run from the repository root.  Per-dispatch time of the fused kld3d launch at 10 M pairs, two patterns, in one process of the library GD3D_LIB selects:
   repeat: every launch on the same target (what the benchmark step does);
   rotate: three targets in turn, so that every launch reads a target nobody read just before."""
import json, statistics, sys, torch
sys.path.insert(0, '.')
import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd import gd_loss as gdl
amd.load_library()
n = 10_000_000
dev = torch.device('cuda:0')
g = torch.Generator(device=dev).manual_seed(0)
arena = torch.rand(6 * n, 7, device=dev, generator=g) + 0.5
tg = [arena[k * n:(k + 1) * n] for k in range(3)]
pr = [arena[(3 + k) * n:(4 + k) * n].detach().requires_grad_(True) for k in range(3)]
mod = amd.build_loss(dict(type='GDLoss', loss_type='kld3d', fun='log1p', tau=1.0, loss_weight=5.0))
out = {}
for pattern in ('repeat', 'rotate', 'repeat', 'rotate'):
    ev = []
    for i in range(60):
        k = i % 3
        t = tg[0] if pattern == 'repeat' else tg[k]
        gdl.PROFILE_EVENTS = ev if i >= 12 else None
        pr[k].grad = None
        mod(pr[k], t).backward()
    gdl.PROFILE_EVENTS = None
    torch.cuda.synchronize()
    out.setdefault(pattern, []).extend(tm.elapsed_ms() * 1e3 for tm in ev)
print(json.dumps({p: round(statistics.median(v), 1) for p, v in out.items()}))
