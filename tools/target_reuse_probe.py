"""Driver of tools/target_reuse_probe.hip: builds it (hipcc --offload-arch=gfx950, into tools/build/, untracked) and runs it
in several processes, because buffer placement moves a streaming pass by up to 5 % per process.

    python tools/target_reuse_probe.py --procs 5 --reps 9 --out DIR     # build if needed, run, condense
    python tools/target_reuse_probe.py --build-only

Writes DIR/probe_raw_<flush>.jsonl (one line per process, size, variant and order) and prints the condensed table: per variant
and order the median over processes of each pass's median time, and of pass 1's time over passes 2 and 3.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'target_reuse_probe.hip')
BIN = os.path.join(HERE, 'build', 'target_reuse_probe')


def build(force=False):
    if not force and os.path.isfile(BIN) and os.path.getmtime(BIN) >= os.path.getmtime(SRC):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', SRC, '-o', BIN]
    subprocess.run(cmd, check=True)
    return BIN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--procs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--sizes', default='150,280,400', help='sizes of the shared buffer in MB')
    ap.add_argument('--flush', choices=('dirty', 'clean'), default='dirty',
                    help='what the cache-evicting pass in front of each triple leaves behind: dirty lines (it writes) or clean ones')
    ap.add_argument('--out', default=None)
    ap.add_argument('--timeout', type=float, default=120.0, help='seconds per process')
    ap.add_argument('--build-only', action='store_true')
    args = ap.parse_args()
    exe = build()
    if args.build_only:
        print(exe)
        return 0
    rows = []
    for proc in range(args.procs):
        r = subprocess.run([exe, str(args.reps), args.sizes, args.flush], capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:   # a failed process ends the run: nothing more is started on the device
            sys.stderr.write(r.stderr)
            print(f'process {proc} exited with {r.returncode}', file=sys.stderr)
            return 1
        for line in r.stdout.splitlines():
            if line.startswith('{'):
                d = json.loads(line)
                d['proc'] = proc
                rows.append(d)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f'probe_raw_{args.flush}.jsonl'), 'w') as f:
            for d in rows:
                f.write(json.dumps(d) + '\n')
    groups = {}
    for d in rows:
        groups.setdefault((d['B_MB'], d['variant'], d['order']), []).append(d)
    print(f'flush: {args.flush}; {args.procs} processes x {args.reps} repetitions; per pass: median over processes of the per-process median, us')
    print(f'{"B MB":>6}  {"variant":<24} {"order":<12} {"pass 1":>7} {"pass 2":>7} {"pass 3":>7}  {"p1/p2":>6} {"p1/p3":>6}'
          f'  {"p1/p2 range":>13}')
    for (mb, var, order), ds in groups.items():
        p = [statistics.median(d['pass_us'][k] for d in ds) for k in range(3)]
        r2 = [d['speedup_2'] for d in ds]
        print(f'{mb:6.0f}  {var:<24} {order:<12} {p[0]:7.1f} {p[1]:7.1f} {p[2]:7.1f}  '
              f'{statistics.median(r2):6.3f} {statistics.median(d["speedup_3"] for d in ds):6.3f}  '
              f'{min(r2):6.3f}-{max(r2):.3f}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
