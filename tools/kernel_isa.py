"""Compare the device assembly of two builds of csrc/*.hip, kernel by kernel, in both flavors (no GPU needed).

    python tools/kernel_isa.py <tree or .s dir> <tree or .s dir> [--asm DIR]

A tree (a checkout, or any directory above a csrc/ with .hip files) is compiled with build.py's flags plus
--cuda-device-only -S into DIR/a or DIR/b (default: a temporary directory) as <file>.<flavor>.s; a directory that
already holds such .s files is used as it is.  Prints `<file> <flavor>: N kernels, N identical`, every kernel that
differs, and exits non-zero on any difference.  Local labels carry the ordinal of their function in the file (.LBB<f>_<n>,
.Lfunc_end<f>); the ordinal is dropped, so moving a kernel inside its file is no difference.
"""
import argparse, glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from prcv2025reid_amd.build import FLAGS, FLAVORS, HIPCC

META = ('.vgpr_count', '.sgpr_count', '.vgpr_spill_count', '.private_segment_fixed_size')


def asm_dir(path, out):
    """Directory of <file>.<flavor>.s for `path`: itself if it holds .s files, else compiled from its csrc/*.hip."""
    if glob.glob(os.path.join(path, '*.s')):
        return path
    srcs = sorted(glob.glob(os.path.join(path, '**', 'csrc', '*.hip'), recursive=True))
    if not srcs:
        sys.exit(f'{path}: neither .s files nor csrc/*.hip')
    os.makedirs(out, exist_ok=True)
    jobs = [(src, [HIPCC] + FLAGS + defs + ['--cuda-device-only', '-S', src, '-o',
                   os.path.join(out, f'{os.path.basename(src)[:-4]}.{flavor}.s')]) for flavor, _, defs in FLAVORS for src in srcs]
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        for (src, cmd), r in zip(jobs, pool.map(lambda j: subprocess.run(j[1], capture_output=True, text=True), jobs)):
            if r.returncode != 0:
                sys.exit(f'hipcc failed on {src}:\n{r.stdout}{r.stderr}')
    return out


def kernels(path):
    """{kernel symbol: (instruction-stream lines, metadata tuple)} of one .s file."""
    text = open(path).read()
    out = {}
    for entry in re.split(r'^  - ', text.split('.amdgpu_metadata')[1], flags=re.M)[1:]:
        keys = dict(re.findall(r'^(?:    )?(\.\w+): +(\S+)$', entry, re.M))    # kernel-level keys (arguments sit deeper)
        if '.name' not in keys:                                                 # (an amdhsa.printf entry)
            continue
        body = re.search(rf'^{re.escape(keys[".name"])}:.*?^\.Lfunc_end\d+:', text, re.M | re.S).group(0)
        lines = [re.sub(r'\.L(BB|func_end)\d+', r'.L\1', l) for l in (re.sub(r'\s*;.*', '', l).strip() for l in body.split('\n'))
                 if l and '__hip_cuid_' not in l]
        out[keys['.name']] = (lines, tuple(keys.get(k) for k in META))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a'); ap.add_argument('b'); ap.add_argument('--asm', default=None, help='where compiled .s files go')
    args = ap.parse_args()
    root = args.asm or tempfile.mkdtemp(prefix='kernel_isa_')
    da = asm_dir(args.a, os.path.join(root, 'a'))   # one tree after the other: at most 16 compiles at a time
    db = asm_dir(args.b, os.path.join(root, 'b'))
    names = sorted({os.path.basename(p) for d in (da, db) for p in glob.glob(os.path.join(d, '*.s'))})
    bad = 0
    for n in names:
        pa, pb = os.path.join(da, n), os.path.join(db, n)
        label = ' '.join(n[:-2].rsplit('.', 1))
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f'{label}: only in {da if os.path.exists(pa) else db}'); bad += 1
            continue
        ka, kb = kernels(pa), kernels(pb)
        diff = [k for k in sorted(set(ka) | set(kb)) if ka.get(k) != kb.get(k)]
        print(f'{label}: {len(set(ka) | set(kb))} kernels, {len(set(ka) | set(kb)) - len(diff)} identical')
        for k in diff:
            a, b = ka.get(k), kb.get(k)
            print(f'  DIFFERS {k}: ' + ('only in one build' if not (a and b) else
                  f'{len(a[0])} vs {len(b[0])} lines, ' + ', '.join(f'{m[1:]} {x} vs {y}' for m, x, y in zip(META, a[1], b[1]))))
        bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
