#!/usr/bin/env python3
"""Times the voxel-set-abstraction ops (mmdet3d_gaussian_amd.vsa, csrc/vsa.hip) at the shapes of the reference's PV-RCNN KITTI
config (configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py:75-91,147-154): B = 4, 2048 keypoints per sample, 16384 raw points
per sample, the (radius, nsample) pairs of the raw-point level and the four voxel levels with their channel counts, and the RoI-grid
shape B x 128 x 216 queries over the keypoints.  One process, device events around `reps` back-to-back calls after a warm-up.

Each op is compared with
  (a) a plain-torch formulation of the same op on the same GPU — what a user has without these kernels: per sample a distance
      matrix, a mask and a cumulative count for the ball query; index_select (+ its autograd) for grouping; the per-sample, per-pick
      Python loop for FPS;
  (b) for the grouping forward and backward, the bytes the op must move over the copy rate measured in this process.
    python tools/vsa_time.py [--out FILE] [--reps 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet3d_gaussian_amd as amd  # noqa: E402

B, KEYPOINTS = 4, 2048
# name, points per sample, C, ((radius, nsample), ...): rawpoint_sa_config and voxel_sa_configs (x1, x2, x4, x8 strides)
LEVELS = (('raw', 16384, 1, ((0.4, 16), (0.8, 16))),
          ('x1', 16384, 16, ((0.4, 16), (0.8, 16))),
          ('x2', 8192, 32, ((0.8, 16), (1.2, 32))),
          ('x4', 4096, 64, ((1.2, 16), (2.4, 32))),
          ('x8', 2048, 64, ((2.4, 16), (4.8, 32))))
ROI = ('roi_grid', KEYPOINTS, 128, ((0.8, 16), (1.6, 16)), 128 * 216)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps       # us per call


def cloud(n_per, gen):
    """points as a KITTI sweep lies: x 0..70.4, y -40..40, z -3..1, denser near the sensor"""
    r = torch.rand(B * n_per, generator=gen, device='cuda') ** 1.5 * 70.4
    y = (torch.rand(B * n_per, generator=gen, device='cuda') * 2 - 1) * torch.clamp(r * 0.8, max=40.0)
    z = torch.rand(B * n_per, generator=gen, device='cuda') * 4 - 3
    return torch.stack((r, y, z), 1).contiguous()


def torch_ball_query(radius, nsample, xyz, n_per, new_xyz, m_per):
    r2 = radius * radius
    out, empty, ar = [], [], torch.arange(n_per, device=xyz.device)
    for b in range(B):
        p, q = xyz[b * n_per:(b + 1) * n_per], new_xyz[b * m_per:(b + 1) * m_per]
        d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        mask = d2 < r2
        rank = mask.cumsum(1)
        pos = torch.where(mask & (rank <= nsample), rank - 1, nsample)
        buf = torch.zeros((m_per, nsample + 1), dtype=torch.int64, device=xyz.device)
        buf.scatter_(1, pos, ar.expand(m_per, n_per))
        cnt = rank[:, -1].clamp(max=nsample)
        idx = torch.where(torch.arange(nsample, device=xyz.device)[None] < cnt[:, None], buf[:, :nsample], buf[:, :1])
        out.append(idx * (cnt > 0)[:, None])
        empty.append(cnt == 0)
    return torch.cat(out).to(torch.int32), torch.cat(empty)


def torch_grouping(feats, n_per, idx, m_per):
    start = torch.arange(B, device=feats.device).repeat_interleave(m_per) * n_per
    rows = (start[:, None] + idx.long()).reshape(-1)
    return feats.index_select(0, rows).reshape(idx.shape[0], idx.shape[1], -1).permute(0, 2, 1).contiguous()


def torch_fps(xyz, n_per, npoint):
    out = []
    for b in range(B):
        p = xyz[b * n_per:(b + 1) * n_per]
        t = torch.full((n_per,), 1e10, device=xyz.device)
        old = torch.zeros((), dtype=torch.int64, device=xyz.device)
        picks = [old]
        for _ in range(1, npoint):
            t = torch.minimum(t, ((p - p[old]) ** 2).sum(-1))
            old = t.argmax()
            picks.append(old)
        out.append(torch.stack(picks))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vsa_time.py measures on the GPU: no device found')
    gen = torch.Generator(device='cuda').manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; B = {B}; us per call, mean of {args.reps} back-to-back calls')
    big = torch.empty(512 << 20, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(big)
    copy_us = timed(lambda: dst.copy_(big), 10)
    rate = 2 * big.numel() / (copy_us * 1e-6)
    say(f'# copy rate (512 MiB read + 512 MiB written): {rate / 1e12:.2f} TB/s')
    del big, dst
    raw = cloud(16384, gen)
    cnt_raw = torch.full((B,), 16384, dtype=torch.int32, device='cuda')
    say('\n## furthest point sampling: 16384 points per sample -> 2048 keypoints')
    fps_us = timed(lambda: amd.furthest_point_sample_stacked(raw, cnt_raw, KEYPOINTS), max(2, args.reps // 4), warmup=1)
    torch_us = timed(lambda: torch_fps(raw, 16384, KEYPOINTS), 1, warmup=1)
    say(f'fps_stacked            {fps_us:10.1f} us   plain torch (per-sample loop) {torch_us:12.1f} us   x{torch_us / fps_us:.1f}')
    picks = amd.furthest_point_sample_stacked(raw, cnt_raw, KEYPOINTS)
    keypoints = torch.cat([raw[b * 16384:(b + 1) * 16384][picks[b]] for b in range(B)]).contiguous()

    say('\n## ball query / QueryAndGroup / backward;  floor = bytes moved (idx + gathered rows read + block written) at the copy rate')
    say(f'{"level":9}{"N/sample":>9}{"M/sample":>9}{"C":>4}{"radius":>7}{"ns":>4} | {"query":>8}{"torch":>10} | {"fused fwd":>10}{"torch":>10}{"floor":>8} | '
        f'{"fused bwd":>10}{"torch":>10}{"floor":>8}   (us)')
    for name, n_per, c, pairs, *rest in LEVELS + (ROI,):
        m_per = rest[0] if rest else KEYPOINTS
        pts = keypoints if name == 'roi_grid' else (raw if n_per == 16384 else cloud(n_per, gen))
        if name == 'roi_grid':   # grid points around the keypoints
            sel = torch.randint(0, KEYPOINTS, (B, m_per), generator=gen, device='cuda') + torch.arange(B, device='cuda')[:, None] * KEYPOINTS
            qry = (keypoints[sel.reshape(-1)] + torch.randn(B * m_per, 3, generator=gen, device='cuda') * 0.5).contiguous()
        else:
            qry = keypoints
        pc = torch.full((B,), n_per, dtype=torch.int32, device='cuda')
        qc = torch.full((B,), m_per, dtype=torch.int32, device='cuda')
        feats = torch.randn(B * n_per, c, generator=gen, device='cuda').requires_grad_()
        for radius, ns in pairs:
            mod = amd.QueryAndGroup(radius, ns)
            q_us = timed(lambda: amd.ball_query(radius, ns, pts, pc, qry, qc), args.reps)
            tq_us = timed(lambda: torch_ball_query(radius, ns, pts, n_per, qry, m_per), 2, warmup=1)
            idx, mask = amd.ball_query(radius, ns, pts, pc, qry, qc)
            differ = int((idx != torch_ball_query(radius, ns, pts, n_per, qry, m_per)[0]).any(1).sum())
            if differ:   # torch's reduction order is its own: a point within an ulp of the radius may fall on the other side
                say(f'# {name} r={radius}: {differ} of {idx.shape[0]} idx rows differ from the plain-torch formulation')
            with torch.no_grad():
                f_us = timed(lambda: mod(pts, pc, qry, qc, feats), args.reps)

                def torch_fwd():
                    i, empty = torch_ball_query(radius, ns, pts, n_per, qry, m_per)
                    g = torch.cat([torch_grouping(pts, n_per, i, m_per) - qry[:, :, None], torch_grouping(feats, n_per, i, m_per)], 1)
                    return g * (~empty)[:, None, None]
                tf_us = timed(torch_fwd, 2, warmup=1)
            out, _ = mod(pts, pc, qry, qc, feats)
            gout = torch.randn_like(out)
            b_us = timed(lambda: torch.autograd.grad(out, feats, gout, retain_graph=True), args.reps)
            tout = torch_grouping(feats, n_per, idx, m_per)
            tg = gout[:, 3:].contiguous()
            tb_us = timed(lambda: torch.autograd.grad(tout, feats, tg, retain_graph=True), max(2, args.reps // 4))
            m = B * m_per
            fwd_bytes = m * ns * 4 + m * ns * (c + 3) * 4 + m * (c + 3) * ns * 4
            bwd_bytes = m * ns * 4 + m * c * ns * 4 + m * ns * c * 4 + B * n_per * c * 4
            say(f'{name:9}{n_per:9d}{m_per:9d}{c:4d}{radius:7.1f}{ns:4d} | {q_us:8.1f}{tq_us:10.1f} | {f_us:10.1f}{tf_us:10.1f}{fwd_bytes / rate * 1e6:8.1f} | '
                f'{b_us:10.1f}{tb_us:10.1f}{bwd_bytes / rate * 1e6:8.1f}')
            del out, tout, gout, tg
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
