"""Heat-map classification loss of the CenterPoint heads for all tasks in one pass (csrc/heat_focal.hip).

What `CenterGDHead.loss` does per task at /root/reference/mmdet3d_gaussian/models/dense_heads/gd_centerpoint_head.py:403-411
— mmdet3d's `clip_sigmoid` on the head's heat-map logits, `num_pos = target.eq(1).sum().item()` (a host sync per task) and
mmdet's `GaussianFocalLoss(..., avg_factor=max(num_pos, 1))` (both third party, absent here: restated from the published
text) — as two launches forward for every task together, one launch backward and no host sync.  GPU tensors only.
"""
import torch

from . import _host, _lib
from ._host import cfg_get, f32c

CLIP_EPS = 1e-4      # mmdet3d clip_sigmoid(x, eps=1e-4)
LOG_EPS = 1e-12      # mmdet gaussian_focal_loss: eps = 1e-12


def _cfg(loss_cls):
    kind = cfg_get(loss_cls, 'type', type(loss_cls).__name__)
    if kind != 'GaussianFocalLoss':
        raise RuntimeError(f'center_head_heatmap_loss: loss_cls is {kind!r}; the reference heads configure GaussianFocalLoss')
    if cfg_get(loss_cls, 'reduction', 'mean') != 'mean':
        raise RuntimeError("center_head_heatmap_loss: reduction must be 'mean' (sum / avg_factor), as the reference configures it")
    return float(cfg_get(loss_cls, 'alpha', 2.0)), float(cfg_get(loss_cls, 'gamma', 4.0)), float(cfg_get(loss_cls, 'loss_weight', 1.0))


def _tasks(logits, targets, grads):
    arr = (_lib.HeatFocalTask * len(logits))()
    for t, (x, y) in enumerate(zip(logits, targets)):
        arr[t].logits, arr[t].target, arr[t].n = x.data_ptr(), y.data_ptr(), x.numel()
        arr[t].grad = grads[t].data_ptr() if grads[t] is not None else None
    return arr


class _HeatFocal(torch.autograd.Function):
    @staticmethod
    def _launch(cfg, xs, targets, need):
        """One gd3d_heat_focal_loss launch set -> (per-task gradient maps | None, out (3, T): losses, factors, num_pos)."""
        alpha, gamma, weight = cfg
        T = len(xs)
        dev = xs[0].device
        grads = [torch.empty_like(x) if nd else None for x, nd in zip(xs, need)]
        arr = _tasks(xs, targets, grads)
        out = torch.empty((3, T), dtype=torch.float32, device=dev)        # losses, factors, num_pos
        ws = torch.empty(_lib.load_extras().gd3d_heat_focal_workspace_bytes(arr, T), dtype=torch.uint8, device=dev)
        _host.call_extras('gd3d_heat_focal_loss', dev, (arr, T, alpha, gamma, CLIP_EPS, LOG_EPS, weight, out[0].data_ptr(), out[1].data_ptr(),
                                                        out[2].data_ptr(), ws.data_ptr()))
        return grads, out

    @staticmethod
    def forward(ctx, cfg, targets, *logits):
        need = [bool(ctx.needs_input_grad[2 + t]) for t in range(len(logits))]
        xs = [f32c(x) for x in logits]
        grads, out = _HeatFocal._launch(cfg, xs, targets, need)
        # the fp32 logits and targets a retain_graph replay re-launches from go through save_for_backward: version-checked (an
        # in-place edit between forward and that backward raises instead of returning another input's gradients) and released
        # with the graph; ctx.state holds no input tensor
        ctx.save_for_backward(*xs, *targets)
        ctx.state = (cfg, grads, out, need, [x.dtype for x in logits], [x.shape for x in logits])
        ctx.used = False
        losses, num_pos = out[0], out[2]
        ctx.mark_non_differentiable(num_pos)
        return losses, num_pos

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_losses, _grad_num_pos):
        cfg, grads, out, need, dtypes, shapes = ctx.state
        saved = ctx.saved_tensors
        T = len(saved) // 2
        xs, targets = list(saved[:T]), list(saved[T:])
        if ctx.used:   # retain_graph replay: the maps of the first backward were scaled in place and handed over: launch again,
            grads, out = _HeatFocal._launch(cfg, xs, targets, need)   # as the loss / anchor-head / centre-head nodes do
        else:
            ctx.state = (cfg, None, None, need, dtypes, shapes)
        ctx.used = True
        up = grad_losses.to(torch.float32).contiguous()
        _host.call_extras('gd3d_heat_focal_scale', xs[0].device, (_tasks(xs, targets, grads), T, out[1].data_ptr(), up.data_ptr()))
        res = [None if g is None else (g.view(shp) if dt == torch.float32 else g.view(shp).to(dt)) for g, dt, shp in zip(grads, dtypes, shapes)]
        return (None, None) + tuple(res)


def center_head_heatmap_loss(loss_cls, heatmap_logits, heatmap_targets):
    """loss_cls        : the head's `loss_cls` (an mmdet GaussianFocalLoss module, or its config dict: alpha, gamma, loss_weight,
                      reduction='mean');
    heatmap_logits  : per task the head's RAW heat-map output (B, C_t, H, W) — before any sigmoid (the reference replaces
                      preds_dict['heatmap'] by its clipped sigmoid in place at :405; this function leaves it alone);
    heatmap_targets : per task the Gaussian target maps of `get_targets` (same shapes).
    Returns (losses (T,), num_pos (T,)) on the device: losses[t] = `task{t}.loss_heatmap`, differentiable wrt the logits;
    num_pos[t] = number of target cells equal to 1 (what the reference passes on as avg_factor of the regression losses)."""
    if len(heatmap_logits) != len(heatmap_targets) or not heatmap_logits:
        raise RuntimeError(f'center_head_heatmap_loss: {len(heatmap_logits)} logit maps and {len(heatmap_targets)} target maps')
    if len(heatmap_logits) > 16:
        raise RuntimeError('center_head_heatmap_loss: at most 16 tasks per call')
    _host.gpu_only(heatmap_logits[0], 'center_head_heatmap_loss')
    targets = []
    for t, (x, y) in enumerate(zip(heatmap_logits, heatmap_targets)):
        if x.shape != y.shape or x.device != y.device:
            raise RuntimeError(f'task {t}: logits {tuple(x.shape)} on {x.device} vs targets {tuple(y.shape)} on {y.device}')
        targets.append(f32c(y.detach()))
    return _HeatFocal.apply(_cfg(loss_cls), targets, *heatmap_logits)
