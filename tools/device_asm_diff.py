#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 kernels?   No GPU needed.

    python tools/device_asm_diff.py OLD_TREE NEW_TREE [--units gd3d_] [--jobs 8] [--keep DIR] [--rename REGEX=REPL ...]

Compiles every HIP translation unit that each tree's mmdet3d-gaussian_amd/build.py lists (its SOURCES and EXTRA_SOURCES,
with that tree's own flags; --units keeps the file names that start with the prefix) to device-only assembly and compares
the trees kernel by kernel, whichever translation unit a kernel is in: the function body with its kernel descriptor
(.amdhsa_* lines) and the resource figures printed behind it (registers, LDS, scratch, occupancy).  The only
normalisation is the function's index inside local labels (.LBB<i>_<k>, .Lfunc_end<i>, .LJTI<i>_<k>), which depends on the
function's position in its file (and with its digits, the padding in front of a comment).
Prints the kernels that are only in one tree, the ones that differ (with a unified diff), and exits 1 if any body or
resource figure differs; kernels present on one side only are listed and do not fail the run.  A kernel that several units of one
tree define (a library template instantiated in each) counts once when its copies are the same; one whose copies differ is listed
with its units under a heading of its own, and its first copy is the one compared.
--rename REGEX=REPL (repeatable) is re.sub(REGEX, REPL) over OLD's assembly text before anything is read from it, for a kernel whose
mangled name changed because a template argument moved to another namespace: the renamed kernels then pair up and are compared as
the others are.  A substitution and nothing more.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import runpy
import subprocess
import sys
import tempfile

LOCAL = re.compile(r'(\.L(?:BB|func_end|func_begin|JTI|tmp)|\bBB)\d+')   # BB<i>_<k>: the same labels named in comments
PAD = re.compile(r'[ \t]+;')   # the comment column behind a label moves with the number of digits of <i>


def compile_tree(tree, out, prefix, jobs):
    b = runpy.run_path(os.path.join(tree, 'mmdet3d-gaussian_amd', 'build.py'), run_name='build_recipe')
    units = {**b['SOURCES'], **b['EXTRA_SOURCES']}
    cmds = []
    for src, flags in units.items():
        path = os.path.join(b['CSRC'], src)
        if src.startswith(prefix) and os.path.isfile(path):
            s_path = os.path.join(out, src + '.s')
            cmds.append((s_path, [b['hipcc_path']()] + b['COMMON'] + flags + ['--cuda-device-only', '-S', path, '-o', s_path]))

    def one(c):
        r = subprocess.run(c[1], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(' '.join(c[1]) + '\n' + r.stderr[-4000:])
        return c[0]
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        return list(pool.map(one, cmds))


def kernels(paths, renames=()):
    """kernel name -> (normalised body lines, descriptor lines), and name -> [units] for every name that is defined more than
    once: with the same body and figures in every copy it counts once; with copies that differ, the first one read is compared"""
    out, units, differ = {}, {}, set()
    for p in paths:
        text = open(p).read()
        for pattern, repl in renames:
            text = re.sub(pattern, repl, text)
        lines = text.split('\n')
        names = [ln.split()[1] for ln in lines if ln.strip().startswith('.amdhsa_kernel ')]
        for name in names:
            start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ':'))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
            # the resource figures the compiler prints behind the function: .set <name>.num_vgpr ..., "; Kernel info:"
            d1 = end + 1
            while lines[d1].lstrip().startswith(('.size', '.set', ';', '.section\t.AMDGPU.csdata')):
                d1 += 1
            norm = [PAD.sub(' ;', LOCAL.sub(lambda m: m.group(1), ln)) for ln in lines[start:d1]]
            copy = (norm[:end - start], norm[end - start:])
            units.setdefault(name, []).append(os.path.basename(p)[:-2])
            if out.setdefault(name, copy) != copy:
                differ.add(name)
    return out, {n: (u, n in differ) for n, u in units.items() if len(u) > 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--units', default='', help='only translation units whose file name starts with this')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--keep', help='write the assembly to DIR/old and DIR/new instead of a temporary directory')
    ap.add_argument('--rename', action='append', default=[], metavar='REGEX=REPL', help="re.sub over OLD's assembly before it is read")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        root = a.keep or tmp
        sides = []
        for tag, tree in (('old', a.old), ('new', a.new)):
            d = os.path.join(root, tag)
            os.makedirs(d, exist_ok=True)
            renames = [r.split('=', 1) for r in a.rename] if tag == 'old' else ()
            sides.append(kernels(compile_tree(os.path.abspath(tree), d, a.units, a.jobs), renames))
    (old, old_dup), (new, new_dup) = sides
    for tag, dup in (('OLD', old_dup), ('NEW', new_dup)):
        bad_dup = sorted(n for n, (_, d) in dup.items() if d)
        print(f'defined in more than one unit in {tag}: {len(dup) - len(bad_dup)} with identical copies, {len(bad_dup)} with DIFFERING COPIES')
        for n in bad_dup:
            print('   ', n, 'in', ', '.join(dup[n][0]))
    for tag, names in (('only in OLD', sorted(set(old) - set(new))), ('only in NEW', sorted(set(new) - set(old)))):
        print(f'{tag}: {len(names)}')
        for n in names:
            print('   ', n)
    bad = 0
    for n in sorted(set(old) & set(new)):
        for what, o, w in (('body', old[n][0], new[n][0]), ('resources', old[n][1], new[n][1])):
            if o != w:
                bad += 1
                print(f'DIFFERS ({what}): {n}')
                print('\n'.join(list(difflib.unified_diff(o, w, 'old', 'new', lineterm='', n=2))[:200]))
    print(f'kernels: old {len(old)}, new {len(new)}, common {len(set(old) & set(new))}, differing {bad}')
    print('VERDICT:', 'device code of the common kernels is identical' if bad == 0 else 'device code differs')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
