#!/bin/bash
# Run ON THE GPU BOX: per-kernel times of the configs[4] NMS stand-in, single class vs the batched call (tools/nms_batched_one.py)
# usage: FORMS="single batched batched_c multi" tools/nms_batched_kernels.sh      (default forms: single batched batched_c)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export TMPDIR=/tmp
for form in ${FORMS:-single batched batched_c}; do
  rm -rf /tmp/kt_nb
  echo "== $form"
  GD3D_HOST=python python3 $ROOT/tools/nms_batched_one.py $form 2>&1 | grep "us per call"
  (cd /tmp && GD3D_HOST=python rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kt_nb -- python3 $ROOT/tools/nms_batched_one.py $form > /dev/null 2>&1)
  python3 $ROOT/tools/nms_kstats.py /tmp/kt_nb
done
