"""build_ref_vox.py — TEST INFRASTRUCTURE.  Recipe for oracle/_ref/ref_vox.so: the REFERENCE's own dynamic scatter
(ops/voxel/src/scatter_points_cuda.cu, voxelization.cpp, voxelization.h) as a torch extension for gfx950.

Its host code is real ATen (`at::unique_dim`, `AT_DISPATCH_FLOATING_TYPES`), so unlike the VSA kernels (ref_vsa_bind.hip) it cannot be
compiled against stub headers.  torch's extension builder translates the sources and writes the result beside them, and the reference
tree is read-only, so the build runs on a COPY in a temporary directory outside the repository; only the shared object comes back.
No text of the reference, translated or not, stays in the tree.

usage: build_ref_vox.py <reference root> <output directory>
"""
import os
import shutil
import sys
import tempfile


def main(ref_root, out_dir):
    src = os.path.join(ref_root, 'mmdet3d_gaussian', 'ops', 'voxel', 'src')
    names = ('scatter_points_cuda.cu', 'voxelization.cpp', 'voxelization.h')
    if not all(os.path.isfile(os.path.join(src, n)) for n in names):
        print(f'reference tree absent ({src}): keeping prebuilt ref_vox (if any)')
        return 0
    os.environ['PYTORCH_ROCM_ARCH'] = 'gfx950'
    os.environ['MAX_JOBS'] = str(min(int(os.environ.get('MAX_JOBS', '16')), 16))
    from torch.utils import cpp_extension
    with tempfile.TemporaryDirectory(prefix='ref_vox_') as tmp:
        work, shim, bld = (os.path.join(tmp, d) for d in ('src', 'shim', 'build'))
        os.makedirs(work)
        os.makedirs(os.path.join(shim, 'THC'))
        os.makedirs(bld)
        for n in names:
            shutil.copy(os.path.join(src, n), os.path.join(work, n))
        open(os.path.join(shim, 'THC', 'THC.h'), 'w').close()      # current torch ships no THC
        # the reference defines reduceAdd under `#ifdef __CUDA_ARCH__` only, which a HIP device pass does not define
        cpp_extension.load(name='ref_vox', sources=[os.path.join(work, 'voxelization.cpp'), os.path.join(work, 'scatter_points_cuda.cu')],
                           extra_include_paths=[shim], extra_cflags=['-DWITH_CUDA', '-O2'],
                           extra_cuda_cflags=['-DWITH_CUDA', '-D__CUDA_ARCH__=600', '-O2'], with_cuda=True, build_directory=bld,
                           is_python_module=False, verbose=False)
        os.makedirs(out_dir, exist_ok=True)
        shutil.copy(os.path.join(bld, 'ref_vox.so'), os.path.join(out_dir, 'ref_vox.so'))
    print(f'built {os.path.join(out_dir, "ref_vox.so")}')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
