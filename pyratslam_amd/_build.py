"""Build libratslam_hip.so in-tree with hipcc for gfx950 (no JIT cache, no pip).

``python -m pyratslam_amd._build`` or ``__graft_entry__.build()``.  compile_cmd() and
link_cmd() are the one recipe: the tests and tools that compile a source (the assembly
guard, tools/kernel_resources.py, tools/build_variant.py) take their commands from here.
"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, 'csrc')
INCLUDE = os.path.join(ROOT, 'include')
LIB = os.path.join(HERE, 'libratslam_hip.so')
OBJDIR = os.path.join(HERE, 'build')
# the translation units (posecell.hip includes its pc_*.h parts, view_templates.hip its
# vt_*.h parts: one object each, so the file-wide flags below reach every kernel of either)
SOURCES = ['rs_common.cpp', 'posecell.hip', 'view_templates.hip', 'view_templates_float.hip',
           'visual_odometer.hip', 'experience_map.hip', 'pose_ensemble.hip']
# per-source flags: the plane scan's batch takes are single-lane atomics; the
# wave-aggregating atomic optimizer only adds a readfirstlane round trip to them.
# The pose-cell stencils keep scalar FMAs: SLP packing into v_pk_fma_f32 pairs the
# filter taps into register pairs and doubles the VGPRs of the conv_xy passes
# (pc_fused_rows 90 -> 220, pc_path_rows<128> 85 -> 146), halving occupancy.
# The plane scan is scheduled for ILP: its query-plane reads, issued a row ahead, then
# land a few planes into the row before instead of next to their use.
EXTRA = {'view_templates.hip': ['-mllvm', '-amdgpu-atomic-optimizer-strategy=None',
                                '-mllvm', '-amdgpu-sched-strategy=max-ilp'],
         # pc_step_halo's first 9 arguments (the union image's addresses, the partial sums) preloaded
         # into scalar registers (pc_halo.h, before pc_step_halo)
         'posecell.hip': ['-fno-slp-vectorize', '-mllvm', '-amdgpu-kernarg-preload-count=9'],
         # the ensemble's stencils keep scalar FMAs for the same reason (pce_run_kernel 86 -> 66 VGPRs)
         'pose_ensemble.hip': ['-fno-slp-vectorize'],
         # the linked map's float64 rule is defined operation by operation (em_rule.h): a
         # fused multiply-add would round x + w * sx once where NumPy rounds twice
         'experience_map.hip': ['-ffp-contract=off']}
ARCH = os.environ.get('PYRATSLAM_ARCH', 'gfx950')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def headers():
    """Every header an object may depend on: csrc/*.h and the ABI."""
    return sorted(glob.glob(os.path.join(CSRC, '*.h'))) + [os.path.join(INCLUDE, 'ratslam_abi.h')]


def obj_path(src):
    return os.path.join(OBJDIR, src.rsplit('.', 1)[0] + '.o')


def compile_cmd(src, out, kind='obj', path=None, include=(), flags=()):
    """The hipcc command that compiles source ``src`` of SOURCES, with its EXTRA flags, into ``out``.

    kind: 'obj' (the product object), 'asm' (the device-only assembly listing) or 'remarks'
    (device-only, with the kernel-resource-usage remarks on stderr).  path: another file
    compiled under ``src``'s flags (an edited copy); include: directories searched ahead
    of csrc/ (a copy's headers); flags: further flags of a variant."""
    lang = ['-x', 'hip'] if src.endswith('.hip') else []
    mode = {'obj': ['-c'], 'asm': ['-S', '--cuda-device-only'],
            'remarks': ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c']}[kind]
    return [HIPCC, f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function',
            *(f'-I{d}' for d in include), f'-I{INCLUDE}', f'-I{CSRC}', *lang, *EXTRA.get(src, []), *flags,
            *mode, path or os.path.join(CSRC, src), '-o', out]


def link_cmd(objs, lib):
    """The command that links the library from one object per source of SOURCES."""
    return [HIPCC, f'--offload-arch={ARCH}', '-shared', '-fPIC', '-o', lib, *objs,
            '-L/opt/rocm/lib', '-lrccl', '-Wl,-rpath,/opt/rocm/lib']


def _newer(src, dst):
    return not os.path.exists(dst) or os.path.getmtime(src) > os.path.getmtime(dst)


def _run(cmd, verbose):
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)


def build(verbose=False, force=False):
    """Compile every HIP/C++ source of the library and link it; returns the .so path."""
    os.makedirs(OBJDIR, exist_ok=True)
    hdr_mtime = max(os.path.getmtime(h) for h in headers() + [os.path.abspath(__file__)])
    objs = []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        obj = obj_path(src)
        objs.append(obj)
        stale = force or _newer(path, obj) or (os.path.exists(obj) and os.path.getmtime(obj) < hdr_mtime)
        if stale:
            _run(compile_cmd(src, obj), verbose)
    if force or any(_newer(o, LIB) for o in objs):
        _run(link_cmd(objs, LIB), verbose)
    return LIB


if __name__ == '__main__':
    print(build(verbose=True, force='--force' in sys.argv))
