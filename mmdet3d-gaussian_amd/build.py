"""Build recipe of libgd3d.so (hand-written HIP for gfx950 behind the C ABI of include/gd3d.h) and of _gd3d_node.so
(the C++ autograd node GDLoss calls it through).

libgd3d.so: plain ``hipcc --offload-arch=gfx950``: no torch headers, no hipify, no cmake.  _gd3d_node.so: one host
translation unit (csrc/torch_node.cpp) against the torch headers of the running interpreter, no kernel in it.  Both are
built IN-TREE (mmdet3d-gaussian_amd/) so that they travel to the GPU box with the snapshot.
"""
import concurrent.futures
import hashlib
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, 'csrc')
LIB_PATH = os.path.join(PKG_DIR, 'libgd3d.so')
ARCH = 'gfx950'

# per-translation-unit flags:
#  * gd3d_loss.hip, gd3d_anchor_head.hip, gd3d_center_head.hip (the GD-loss kernels, one unit per kernel family, compiled
#    in parallel): 1-ulp v_rcp/v_sqrt instead of the ~10-instruction correctly-rounded sequences
#    (the losses are graded at 1e-5; the kernel must stay HBM-bound, not VALU-bound);
#  * rbox.hip: correctly-rounded IEEE division/sqrt and NO fma contraction, because the NMS keep
#    indices must be bit-identical to a CPU evaluation of the same fp32 operation sequence.
SOURCES = {   # the SURVEY.md §8 surface: libgd3d.so (include/gd3d.h)
    'gd3d_loss.hip': ['-fno-hip-fp32-correctly-rounded-divide-sqrt', '-ffp-contract=fast'],
    'gd3d_anchor_head.hip': ['-fno-hip-fp32-correctly-rounded-divide-sqrt', '-ffp-contract=fast'],
    'gd3d_center_head.hip': ['-fno-hip-fp32-correctly-rounded-divide-sqrt', '-ffp-contract=fast'],
    'rbox.hip': ['-ffp-contract=off'],
    'voxel_scatter.hip': [],
    'device_sort.hip': [],                     # the one unit that includes rocPRIM: the radix sorts and scans of the three units below (integer code)
    'voxel_index.hip': [],                     # device_sort.h's radix sort + scan between hand-written kernels
    'eval_match.hip': ['-ffp-contract=off'],
    'coders.hip': ['-ffp-contract=off'],      # same rounding sequence as the torch elementwise ops it replaces
    'vsa.hip': ['-ffp-contract=off'],         # ball-query membership and FPS arg-max decisions replay bit for bit in vsa_cpu.cpp
    'pib.hip': ['-ffp-contract=off'],         # point-in-box decisions and RoI grid points replay bit for bit in pib_cpu.cpp
    'roi_head.hip': ['-ffp-contract=off'],    # label / mask decisions and the target yaw's folds replay bit for bit in roi_head_cpu.cpp
    'roi_sample.hip': ['-ffp-contract=off'],  # the 3D IoU, hence every assignment and draw, replays bit for bit in roi_sample_cpu.cpp
    'seg_head.hip': ['-ffp-contract=off'],    # n_pos, the winner columns and the backward's row sums replay bit for bit in seg_head_cpu.cpp
    'vsa_bev.hip': ['-ffp-contract=off'],     # pixel coordinates, weights, interpolated values and voxel centres replay bit for bit in vsa_bev_cpu.cpp
    'hard_voxel.hip': ['-ffp-contract=off'],  # a point's cell and the voxel mean replay bit for bit in hard_voxel_cpu.cpp; sort + scans from device_sort.h
    'pillar_feat.hip': ['-ffp-contract=off'],  # the voxel table, the centres, the offsets and the distance replay bit for bit in pillar_feat_cpu.cpp
    'view_net.hip': ['-ffp-contract=off'],     # the view transforms, the cells, the canvas and the sampled features replay bit for bit in view_net_cpu.cpp
    'simota.hip': ['-ffp-contract=off'],       # memberships, the IoU, the costs on fx_logf, both selections and every match replay bit for bit in simota_cpu.cpp
    'sparse_conv.hip': ['-ffp-contract=off'],  # every table of the index build replays bit for bit in sparse_conv_cpu.cpp; explicit fmaf for the values; sorts + scan from device_sort.h
    'sparse_conv_16.hip': ['-ffp-contract=off'],  # the fp16 / bf16 forms on v_mfma_f32_16x16x32: the epilogues' fp32 sequences stay as written
    'sparse_conv_wgrad.hip': ['-ffp-contract=off'],  # the weight and bias gradient, one source for fp32 / fp16 / bf16: explicit fmaf in a fixed order
    'sparse_conv_wgrad_16.hip': ['-ffp-contract=off'],  # stage one of the 16-bit weight gradient on v_mfma_f32_16x16x32; the wave sums in a fixed order, the rest is sparse_conv_wgrad.hip's
    'sparse_dense.hip': ['-ffp-contract=off'],     # dense() and its backward for 4- and 2-byte elements: copies only, flagged as the rest of the sparse conv
    'sparse_bn.hip': ['-ffp-contract=off'],    # live-row BatchNorm: every multiply-add is an explicit fmaf, the order of every sum is fixed
    'sparse_pool.hip': ['-ffp-contract=off'],  # sparse max pooling: copies and plain fp32 adds in a fixed order replay bit for bit in sparse_pool_cpu.cpp
    'voxel_query.hip': ['-ffp-contract=off'],   # memberships, slots, keys and query cells replay bit for bit in voxel_query_cpu.cpp; sort from device_sort.h, gather from vsa_gather.h
    'eval_ap.hip': ['-ffp-contract=off'],       # keys, counts, the fp64 precisions and the exact envelope sum replay bit for bit in eval_ap_cpu.cpp; sort from device_sort.h
    'eval_frames.hip': ['-ffp-contract=off'],    # the affinities are rbox.hip's, the matcher eval_match.hip's, the records eval_ap.hip's: same bits, and in eval_frames_cpu.cpp
    'rpn_proposal.hip': ['-ffp-contract=off'],  # the order keys, the sigmoid and the decode on fx_expf, the threshold and the direction fix replay bit for bit in rpn_proposal_cpu.cpp
}
# The frozen round-3 extras OUTSIDE §8 (DESIGN_EXTRAS.md; include/gd3d_extras.h): a library of their own since round 6,
# libgd3d_extras.so, linked against libgd3d.so (the inference slices call its rnms_* entry points) and loaded only by
# mmdet3d_gaussian_amd.extras' modules (_lib.load_extras()).  What ships as libgd3d.so is the §8 translation units only.
EXTRA_SOURCES = {
    'center_infer.hip': ['-ffp-contract=off'],    # decode as coders.hip; the NMS boxes feed bit-exact keep decisions
    'anchor_targets.hip': ['-ffp-contract=off'],   # IoU and thresholds decide as the torch elementwise ops do
    'anchor_cls.hip': [],                       # elementwise focal + direction loss with gradient, graded at 1e-5
    'heat_focal.hip': ['-fno-hip-fp32-correctly-rounded-divide-sqrt', '-ffp-contract=fast'],   # elementwise loss + gradient, graded at 1e-5
    'anchor_infer.hip': ['-ffp-contract=off'],    # delta decode in the reference's operation order; boxes feed the NMS
    'center_targets.hip': ['-ffp-contract=off'],  # gaussian_radius in the reference's fp32 operation order
}
EXTRAS_PATH = os.path.join(PKG_DIR, 'libgd3d_extras.so')
# libgd3d.so exports what include/gd3d.h declares and nothing else (a file of csrc/: part of source_hash())
VERSION_SCRIPT = os.path.join(CSRC, 'gd3d.map')
COMMON = ['--offload-arch=' + ARCH, '-O3', '-fPIC', '-std=c++17', '-Wall', '-Wno-unused-function']

# host translation units (the `_cpu` twins of include/gd3d.h): compiled by the ROCm toolchain's own clang++ as plain C++
# (csrc/gd3d_device.h uses clang vector extensions), for the x86-64-v3 level (AVX2 + FMA: the per-pair math is written in
# explicit fmaf(), which must be an instruction, not a libm call), same contraction mode as the device build of the loss
HOST_SOURCES = {
    'gd3d_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=fast', '-pthread'],
    'rbox_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],   # same single-operation sequence as rbox.hip: bit-identical decisions
    'vsa_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],    # same for vsa.hip: idx, cnt, mask and FPS picks bit-identical
    'pib_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],    # same for pib.hip: box_idx, flags, targets and grid points bit-identical
    'roi_head_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],   # same for roi_head.hip: label, reg_mask and the weights bit-identical
    'roi_sample_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],   # same for roi_sample.hip: every output bit-identical
    'seg_head_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],     # same for seg_head.hip: n_pos and the winner columns bit-identical
    'vsa_bev_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],      # same for vsa_bev.hip: the forward, the centres and the counts bit-identical
    'hard_voxel_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],   # same for hard_voxel.hip: every output bit-identical
    'pillar_feat_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],  # same for pillar_feat.hip: every output bit-identical
    'view_net_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],     # same for view_net.hip: every forward output bit-identical
    'simota_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],       # same for simota.hip: every output bit-identical
    'sparse_conv_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],  # same for sparse_conv.hip: every integer output bit-identical
    'sparse_conv_16_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],  # widen, sparse_conv_cpu.cpp's loops, one rounding; _Float16 through F16C
    'sparse_bn_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],      # sparse_bn.hip's element sequences, the sums in fp64 per tile
    'sparse_pool_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],    # same for sparse_pool.hip: every output bit-identical
    'voxel_query_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],    # same for voxel_query.hip: every output bit-identical
    'rpn_proposal_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],   # same for rpn_proposal.hip: every output bit-identical
    'eval_ap_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],        # same for eval_ap.hip: every output bit-identical
    'eval_frames_cpu.cpp': ['-march=x86-64-v3', '-ffp-contract=off', '-pthread'],    # same for eval_frames.hip: the existing twins per problem
}
HOST_COMMON = ['-O3', '-fPIC', '-std=c++17', '-Wall', '-Wno-unused-function']


def hipcc_path():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def host_cxx_path():
    """The ROCm toolchain's own clang++ (host compiler of the `_cpu` twins and of the optional C++ node), or None."""
    for c in ('/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++', shutil.which('amdclang++') or ''):
        if c and os.path.exists(c):
            return c
    return None


NODE_SOURCE = 'torch_node.cpp'
NODE_PATH = os.path.join(PKG_DIR, '_gd3d_node.so')
NODE_HASH_PATH = NODE_PATH + '.srchash'


def _deps():
    out = []
    for root, _, files in os.walk(CSRC):
        out += [os.path.join(root, f) for f in files if f != NODE_SOURCE]
    out.append(os.path.join(PKG_DIR, '..', 'include', 'gd3d.h'))
    out.append(os.path.join(PKG_DIR, '..', 'include', 'gd3d_extras.h'))
    out.append(os.path.abspath(__file__))
    return out


HASH_PATH = LIB_PATH + '.srchash'


def source_hash():
    """Content hash of everything the library is built from (mtimes do not survive a snapshot to another box)."""
    h = hashlib.sha256()
    for d in sorted(os.path.normpath(x) for x in _deps()):
        if os.path.exists(d):
            h.update(os.path.basename(d).encode())
            with open(d, 'rb') as f:
                h.update(f.read())
    return h.hexdigest()


def is_stale():
    if not os.path.isfile(LIB_PATH) or not os.path.isfile(EXTRAS_PATH) or not os.path.isfile(HASH_PATH):
        return True
    with open(HASH_PATH) as f:
        return f.read().strip() != source_hash()


def build(force=False, verbose=False):
    """Compile every HIP translation unit for gfx950 and link libgd3d.so (the §8 surface) and libgd3d_extras.so (the frozen
    extras, linked against it).  Returns libgd3d.so's path."""
    if not force and not is_stale():
        return LIB_PATH
    hipcc = hipcc_path()
    if not os.path.exists(hipcc):
        raise RuntimeError('hipcc not found: cannot build libgd3d.so')
    objdir = os.path.join(PKG_DIR, 'build', str(os.getpid()))  # per process: ranks may build concurrently
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for src, flags in list(SOURCES.items()) + list(EXTRA_SOURCES.items()):
        path = os.path.join(CSRC, src)
        if not os.path.isfile(path):
            continue
        obj = os.path.join(objdir, src.replace('.hip', '.o'))
        jobs.append((src, obj, [hipcc] + COMMON + flags + ['-c', path, '-o', obj]))
    cxx = host_cxx_path()
    if cxx is None:
        raise RuntimeError('the ROCm clang++ (host compiler of the _cpu twins) was not found next to hipcc: cannot build libgd3d.so')
    for src, flags in HOST_SOURCES.items():
        path = os.path.join(CSRC, src)
        obj = os.path.join(objdir, src.replace('.cpp', '.o'))
        jobs.append((src, obj, [cxx] + HOST_COMMON + flags + ['-c', path, '-o', obj]))

    def compile_one(job):
        src, obj, cmd = job
        if verbose:
            print(' '.join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'compiling {src} failed:\n{r.stderr[-4000:]}')
        return obj
    # the translation units are independent: one hipcc per core, at most 8 (each takes 5-25 s and ~1 GB)
    workers = max(1, min(8, os.cpu_count() or 1, len(jobs)))
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        objs = dict(zip((j[0] for j in jobs), pool.map(compile_one, jobs)))
    main_objs = [objs[s_] for s_ in list(SOURCES) + list(HOST_SOURCES) if s_ in objs]
    extra_objs = [objs[s_] for s_ in EXTRA_SOURCES if s_ in objs]
    tmp = f'{LIB_PATH}.{os.getpid()}.tmp'
    cmd = [hipcc, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-pthread', '-Wl,--version-script=' + VERSION_SCRIPT, '-o', tmp] + \
          main_objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'link failed:\n{r.stderr[-4000:]}')
    os.replace(tmp, LIB_PATH)  # atomic
    # the extras: their own image, resolving rnms_* from libgd3d.so next to it ($ORIGIN: the pair travels together)
    tmp = f'{EXTRAS_PATH}.{os.getpid()}.tmp'
    cmd = [hipcc, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-pthread', '-o', tmp] + extra_objs + \
          ['-L' + PKG_DIR, '-l:libgd3d.so', '-Wl,-rpath,$ORIGIN']
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'link of libgd3d_extras.so failed:\n{r.stderr[-4000:]}')
    os.replace(tmp, EXTRAS_PATH)
    with open(HASH_PATH + f'.{os.getpid()}', 'w') as f:
        f.write(source_hash())
    os.replace(HASH_PATH + f'.{os.getpid()}', HASH_PATH)
    shutil.rmtree(objdir, ignore_errors=True)
    return LIB_PATH


def node_source_hash():
    """The node is rebuilt when its source, the C header, the flags or the torch it was compiled against change.  The
    compiler's PATH is not part of it: a box without the compiler can still verify (and load) a matching prebuilt binary."""
    import torch
    h = hashlib.sha256()
    h.update(torch.__version__.encode())
    for d in (os.path.join(CSRC, NODE_SOURCE), os.path.join(PKG_DIR, '..', 'include', 'gd3d.h')):
        with open(d, 'rb') as f:
            h.update(f.read())
    h.update(repr(node_command('OUT', cxx='CXX')).encode())
    return h.hexdigest()


def node_command(out, cxx=None):
    import sysconfig
    import torch
    tdir = os.path.dirname(os.path.abspath(torch.__file__))
    tlib = os.path.join(tdir, 'lib')
    return [cxx or host_cxx_path(), '-std=c++17', '-O2', '-fPIC', '-shared', '-Wall', '-Wno-unused-function',
            '-D__HIP_PLATFORM_AMD__=1', '-DUSE_ROCM=1', '-DTORCH_EXTENSION_NAME=_gd3d_node',
            f'-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}',
            '-isystem', os.path.join(tdir, 'include'), '-isystem', os.path.join(tdir, 'include', 'torch', 'csrc', 'api', 'include'),
            '-isystem', '/opt/rocm/include', '-isystem', sysconfig.get_paths()['include'],
            os.path.join(CSRC, NODE_SOURCE), '-o', out,
            '-L' + tlib, '-ltorch', '-ltorch_cpu', '-lc10', '-lc10_hip', '-ltorch_hip', '-ltorch_python', '-ldl',
            '-Wl,-rpath,' + tlib]


def node_is_stale():
    if not os.path.isfile(NODE_PATH) or not os.path.isfile(NODE_HASH_PATH):
        return True
    with open(NODE_HASH_PATH) as f:
        return f.read().strip() != node_source_hash()


def build_node(force=False, verbose=False):
    """Compile csrc/torch_node.cpp (host C++, ~25 s) into _gd3d_node.so.  It resolves the C ABI from libgd3d.so at run
    time (`bind`), so the two are built independently."""
    if not force and not node_is_stale():
        return NODE_PATH
    if host_cxx_path() is None:
        raise RuntimeError('the ROCm clang++ was not found: cannot build the optional C++ node (_gd3d_node.so)')
    tmp = f'{NODE_PATH}.{os.getpid()}.tmp'
    cmd = node_command(tmp)
    if verbose:
        print(' '.join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'compiling {NODE_SOURCE} failed:\n{r.stderr[-4000:]}')
    os.replace(tmp, NODE_PATH)
    with open(NODE_HASH_PATH + f'.{os.getpid()}', 'w') as f:
        f.write(node_source_hash())
    os.replace(NODE_HASH_PATH + f'.{os.getpid()}', NODE_HASH_PATH)
    return NODE_PATH


if __name__ == '__main__':
    print(build(force=True, verbose=True))
    print(build_node(force=True, verbose=True))
