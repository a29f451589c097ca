#!/usr/bin/env python3
"""Record the flexible mAP fixture FROM THE REAL REFERENCE evaluator (build machine only: needs /root/reference).

    make -C oracle ref_eval && python3 -B tests/golden/make_golden_eval_map.py

The reference's five evaluation files (core/evaluation/{builder,affinity,matcher,breakdown,mean_ap_flexible}.py) are loaded by path,
from where they lie, under a synthetic package; its compiled helpers are oracle/_ref/ref_eval*.so = ops/eval/{affinity,matcher}.cpp.
Three third-party packages are absent from this image and stubbed below: mmcv (Registry / build_from_cfg / the progress bars /
print_log), terminaltables (AsciiTable) and mmdet — whose `average_precision(mode='area')` is restated here and is THE ONLY RESTATED
ARITHMETIC in the fixture (plus `np.bool`, which the numpy of this image no longer has).

FlexibleStatisticsEval.statistics_eval runs with nproc = 0 on about 30 frames, 3 classes, ignore labels, thresholds [0.5, 0.7] and
one RangeBreakdown, once per affinity: LidarIOU3D, LidarIOUBEV, LidarCenterTransBEV (not negated).  The seed is redrawn until the
WHOLE fixture is clear of ties: all scores of a class distinct over the dataset (the reference leaves ties to quicksort) and no
affinity within 1e-5 of a threshold (so that another implementation's last bits cannot move a match).  No case is dropped.
tests/golden/eval_map.npz receives the inputs, the per-frame tp_score_info and the final results: data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import eval_ap_ref as ref  # noqa: E402
import oracle  # noqa: E402

REF_EVAL = os.path.join(os.environ.get('GD3D_REFERENCE_ROOT', '/root/reference'), 'mmdet3d_gaussian', 'core', 'evaluation')
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
RANGES = {'0-30m': (0, 30), '30-50m': (30, 50), '50m+': (50, 1e9)}
THRS = [0.5, 0.7]
CONFIGS = {'iou3d': 'LidarIOU3D', 'ioubev': 'LidarIOUBEV', 'trans': 'LidarCenterTransBEV'}
FRAMES = 30


class _Registry:
    def __init__(self, name):
        self.name, self.modules = name, {}

    def register_module(self, *a, **k):
        def deco(cls):
            self.modules[cls.__name__] = cls
            return cls
        return deco


def _build_from_cfg(cfg, registry, default_args=None):
    args = dict(cfg)
    for k, v in (default_args or {}).items():
        args.setdefault(k, v)
    return registry.modules[args.pop('type')](**args)


def _average_precision(recalls, precisions, mode='area'):
    """mmdet.core.evaluation.mean_ap.average_precision for 1-D input, mode='area'"""
    assert mode == 'area' and recalls.ndim == 1
    return ref.average_precision_area(recalls, precisions)


class _AsciiTable:
    def __init__(self, data):
        self.table = '\n'.join(' | '.join(str(c) for c in row) for row in data)


def load_reference_evaluator():
    sys.dont_write_bytecode = True
    if not hasattr(np, 'bool'):
        np.bool = bool
    ev = oracle.load_ref_eval()
    assert ev is not None, 'build oracle/_ref first (make -C oracle ref_eval)'

    def module(name, **attrs):
        m = sys.modules[name] = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    module('mmcv')
    module('mmcv.utils', Registry=_Registry, build_from_cfg=_build_from_cfg, print_log=lambda msg, logger=None: None)
    module('mmcv.utils.progressbar', track_iter_progress=lambda x: x, track_parallel_progress=None)
    for name in ('mmdet', 'mmdet.core', 'mmdet.core.evaluation'):
        module(name)
    module('mmdet.core.evaluation.mean_ap', average_precision=_average_precision)
    module('terminaltables', AsciiTable=_AsciiTable)
    for name in ('_refpkg', '_refpkg.core', '_refpkg.core.evaluation', '_refpkg.ops', '_refpkg.ops.eval'):
        module(name)
    module('_refpkg.ops.eval.eval_utils', trans_bev=ev.trans_bev, iou_3d=ev.iou_3d, iou_bev=ev.iou_bev, match_coco=ev.match_coco)
    mods = {}
    for f in ('builder', 'affinity', 'matcher', 'breakdown', 'mean_ap_flexible'):
        name = '_refpkg.core.evaluation.' + f
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF_EVAL, f + '.py'))
        mods[f] = sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[f])
    return mods['mean_ap_flexible']


def clear_of_ties(det, anno):
    for c in range(len(CLASSES)):
        s = np.concatenate([frame[c][:, -1] for frame in det])
        if len(np.unique(s)) != len(s):
            return False
    for cfg in CONFIGS:
        for d, a in zip(det, anno):
            if ref.affinity_margin(ref.literal_single(d, a, CLASSES, [RANGES], cfg, THRS)[1], THRS) <= 1e-5:
                return False
    return True


def main():
    maf = load_reference_evaluator()
    seed = 2026
    while True:
        det, anno = ref.random_dataset(seed, FRAMES, len(CLASSES), 24, 8)
        if clear_of_ties(det, anno):
            break
        seed += 1
    out = dict(frames=np.int64(FRAMES), seed=np.int64(seed), classes=np.array(CLASSES), match_thrs=np.array(THRS, np.float64),
               range_names=np.array(list(RANGES)), range_bounds=np.array(list(RANGES.values()), np.float64))
    for f in range(FRAMES):
        for c in range(len(CLASSES)):
            out[f'det.{f}.{c}'] = det[f][c]
        out[f'gt_bboxes.{f}'], out[f'gt_labels.{f}'] = anno[f]['gt_bboxes'], anno[f]['gt_labels']
        out[f'gt_ignore.{f}'] = anno[f]['gt_attrs']['ignore']
    for cfg, calc in CONFIGS.items():
        fse = maf.FlexibleStatisticsEval(CLASSES, THRS, [dict(type='RangeBreakdown', ranges=RANGES)], dict(type=calc), dict(type='MatcherCoCo'),
                                         [], 0)
        for f in range(FRAMES):
            info = fse.statistics_single((det[f], anno[f]))
            # the frame's tuples side by side (one entry per tuple would cost the archive more in names than in data)
            p = f'{cfg}.info.{f}'
            out[p + '.gt_count'] = np.array([t[2] for t in info], np.int64)
            out[p + '.rows'] = np.array([len(t[3]) for t in info], np.int64)
            out[p + '.score'] = np.concatenate([t[3] for t in info])
            out[p + '.tp'] = np.concatenate([t[4] for t in info], axis=1)
            out[p + '.msk'] = np.concatenate([t[5] for t in info], axis=1)
        res = fse.statistics_eval(det, anno)
        out[f'{cfg}.cls'] = np.array([k['class_name'] for k, _ in res])
        out[f'{cfg}.bkd'] = np.array([k['breakdown'] for k, _ in res])
        out[f'{cfg}.thr'] = np.array([k['match_threshold'] for k, _ in res], np.float64)
        out[f'{cfg}.num_det'] = np.array([v['num_det'] for _, v in res], np.int64)
        out[f'{cfg}.num_gt'] = np.array([v['num_gt'] for _, v in res], np.int64)
        out[f'{cfg}.recall'] = np.array([v['recall'] for _, v in res], np.float64)
        out[f'{cfg}.mAP'] = np.array([v['mAP'] for _, v in res], np.float32)
        print(cfg, 'mAP', np.round(out[f'{cfg}.mAP'], 3).tolist())
    path = os.path.join(HERE, 'eval_map.npz')
    np.savez_compressed(path, **out)
    print('eval_map.npz', os.path.getsize(path), 'bytes; seed', seed)


if __name__ == '__main__':
    main()
