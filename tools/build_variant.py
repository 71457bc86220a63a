#!/usr/bin/env python3
"""A/B variant of the library, or of tools/pc_probe.hip, built by the product's recipe
(pyratslam_amd/_build.py: its per-source flags, every object of its SOURCES).

usage: tools/build_variant.py NAME --source posecell.hip [--out abtmp/NAME.so] [--file OTHER.hip]
                              [--edit 'old=>new' ...] [--probe] [-- extra hipcc flags ...]

One source is compiled again, the other objects are the product build's.  --file: another
file in its place; --edit: literal substitutions applied to a copy of the whole csrc/
directory in abtmp/NAME/ (each must match in exactly one file, so an edit reaches the
headers too; the product sources stay untouched), compiled with the copy ahead of csrc/ on
the include path.  --probe: abtmp/NAME_probe, tools/pc_probe.hip against that copy.
"""
import argparse
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyratslam_amd import _build  # noqa: E402


def edited_copy(name, edits):
    copy = os.path.join(ROOT, 'abtmp', name)
    shutil.copytree(_build.CSRC, copy, dirs_exist_ok=True)
    files = sorted(os.listdir(copy))
    for e in edits:
        old, new = e.split('=>', 1)
        hits = [f for f in files if old in open(os.path.join(copy, f)).read()]
        if len(hits) != 1:
            raise SystemExit('edit must match in exactly one file of csrc/, matches %s: %s' % (hits, old))
        p = os.path.join(copy, hits[0])
        s = open(p).read()
        open(p, 'w').write(s.replace(old, new))
    return copy


def run(cmd):
    print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('name')
    ap.add_argument('--source', required=True, choices=_build.SOURCES)
    ap.add_argument('--out')
    ap.add_argument('--file')
    ap.add_argument('--edit', action='append', default=[])
    ap.add_argument('--probe', action='store_true')
    argv = sys.argv[1:]
    cut = argv.index('--') if '--' in argv else len(argv)
    a, flags = ap.parse_args(argv[:cut]), argv[cut + 1:]
    os.chdir(ROOT)   # (relative --file / --out paths: from the repository root)
    os.makedirs(os.path.join(ROOT, 'abtmp'), exist_ok=True)
    os.makedirs(os.path.join(ROOT, 'tools', 'ab'), exist_ok=True)
    include, path = [], a.file
    if a.edit or a.probe:
        copy = edited_copy(a.name, a.edit)
        include, path = [copy], os.path.join(copy, a.source)
    if a.probe:   # one command, compile and link: the object's command without -c, plus rs_common.cpp
        out = a.out or os.path.join(ROOT, 'abtmp', a.name + '_probe')
        cmd = _build.compile_cmd(a.source, out, path=os.path.join(ROOT, 'tools', 'pc_probe.hip'),
                                 include=include, flags=flags)
        cmd.remove('-c')
        cmd.insert(cmd.index('-o'), os.path.join(_build.CSRC, 'rs_common.cpp'))
        run(cmd)
    else:
        out = a.out or os.path.join(ROOT, 'abtmp', a.name + '.so')
        _build.build()   # the other sources' objects
        obj = os.path.join(ROOT, 'tools', 'ab', '%s.%s.o' % (a.name, a.source.rsplit('.', 1)[0]))
        run(_build.compile_cmd(a.source, obj, path=path, include=include, flags=flags))
        run(_build.link_cmd([obj if s == a.source else _build.obj_path(s) for s in _build.SOURCES], out))
    print(os.path.relpath(out, ROOT))


if __name__ == '__main__':
    main()
