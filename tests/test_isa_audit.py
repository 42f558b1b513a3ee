"""Emitted-code audit of the LDS-DMA ring kernels (no GPU needed: hipcc cross-compiles to gfx950 assembly).

Every ring kernel hands a stage from its loading side to its reading side with `s_waitcnt vmcnt(N)` + `s_barrier`.
hipcc 7.2 does not treat that pair as a fence for LDS reads: in `conv_patch3x3_kernel<64>` it had hoisted the first
weight-fragment reads of stage t above the wait and the barrier (found in round 3 as a one-in-2400 irreproducible launch
when forwards overlapped on several HIP streams - csrc/dir_common.h `ring_barrier`).  The fix is a barrier bracketed by
`__builtin_amdgcn_sched_barrier(0)`; these tests keep a raw `s_barrier` from coming back: no kernel source calls the
builtin directly, and in the assembly of every ring kernel at least one barrier sits between two
`; sched_barrier mask(0x00000000)` markers while no barrier that follows a hand-written `s_waitcnt` (an inline-asm
block) is left without them.

A second audit covers the other half of a hand-off, over every kernel of every source: a wave's own LDS writes must have
completed (`s_waitcnt lgkmcnt(0)`) before the barrier that publishes them."""
import glob
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'deep-image-retrieval_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
RING_SOURCES = ['conv_igemm', 'conv_pair', 'conv_patch', 'conv_patchlc', 'conv_patchw', 'conv_patchs2', 'conv_persist', 'conv_persistlc', 'conv_ring', 'conv_seam3', 'conv_wreg', 'conv_wregd', 'conv_c3c1lc',
                'sim_split', 'index_i8', 'ivf', 'stem_pool', 'stem_u8']
RING_KERNELS = re.compile(r'conv_igemm_kernel|conv_patch3x3\w*_kernel|conv_patch64_lc_kernel|conv1x1_persist_kernel|conv1x1_ring_kernel|'
                          r'conv1x1_wreg_kernel|conv1x1_lc_kernel|conv1x1_wregd_kernel|conv_c3c1ds_lc_kernel|sim_split\w*_kernel|whiten_split_kernel|sim_i8_kernel|ivf_scan_i8_kernel|stem_pool_persist_kernel|conv_pair_kernel|conv_pair_patch64_kernel|conv_seam3_kernel|stem_pool_pair_persist_kernel|stem_pool_u8_kernel')


ALL_SOURCES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(CSRC, '*.hip')))
needs_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason='hipcc not available')


def _asm(name, out_dir):
    out = os.path.join(out_dir, name + '.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only',
                    os.path.join(CSRC, name + '.hip'), '-o', out], check=True, capture_output=True)
    return open(out).read()


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    """gfx950 assembly of every csrc/*.hip, compiled once for the module: {source name: text}."""
    out_dir = str(tmp_path_factory.mktemp('asm'))
    with ThreadPoolExecutor(max_workers=16) as ex:
        return dict(zip(ALL_SOURCES, ex.map(lambda n: _asm(n, out_dir), ALL_SOURCES)))


def _functions(text, prefix=r'_ZN3dir'):
    """[(mangled name, [stripped body lines])] of the functions of one assembly file, in order."""
    func, funcs = None, []
    for line in text.split('\n'):
        m = re.match(r'^(%s\w+):' % prefix, line)
        if m:
            func = (m.group(1), [])
            funcs.append(func)
        elif func is not None:
            func[1].append(line.strip())
    return funcs


@needs_hipcc
def test_ring_kernels_fence_their_hand_off_barriers(asm):
    checked, kernels = 0, 0
    for name in RING_SOURCES:
        for func, body in _functions(asm[name]):
            if not RING_KERNELS.search(func):
                continue
            kernels += 1
            lines = [l for l in body if l and not l.startswith('.')]
            fenced_here = 0
            for i, l in enumerate(lines):
                if not l.startswith('s_barrier'):
                    continue
                prev = lines[i - 1] if i else ''
                nxt = lines[i + 1] if i + 1 < len(lines) else ''
                fenced = prev.startswith('; sched_barrier mask(0x00000000)') and nxt.startswith('; sched_barrier mask(0x00000000)')
                after_asm_wait = any(t.startswith(';;#ASMEND') for t in lines[max(0, i - 3):i])
                assert fenced or not after_asm_wait, '%s (%s.hip): raw s_barrier behind a hand-written wait' % (func, name)
                fenced_here += int(fenced)
            assert fenced_here >= 1, '%s (%s.hip): no fenced hand-off barrier' % (func, name)
            checked += fenced_here
    assert kernels >= 42 and checked >= 64, (kernels, checked)


# LDS writes and atomics: they count on lgkmcnt, and s_barrier waits for no counter.  (Reads, ds_permute / ds_bpermute and
# ds_swizzle write no LDS; LDS-DMA loads count on vmcnt, which the hand-off barriers above are audited for.)
DS_WRITE = re.compile(r'^ds_(write|store|add|sub|rsub|inc|dec|min|max|and|or|xor|mskor|wrxchg|cmpst|cmpswap|cond_xchg|pk_add|'
                      r'append|consume)\w*$')
# {(source name, kernel name regex): reason} - LDS writes a barrier may publish without lgkmcnt(0).  There are none.
LDS_PUBLISH_EXCEPTIONS = {}


@needs_hipcc
def test_lds_writes_complete_before_the_barrier_that_publishes_them(asm):
    """On gfx950 a wave's ds_write is in flight until its lgkmcnt drops, and the compiler puts no wait in front of a bare
    s_barrier: a write the barrier is meant to publish can still be pending when another wave reads that LDS after it.  Every
    LDS write or atomic must therefore reach an `s_waitcnt ... lgkmcnt(0)` before the next s_barrier, in the linear order of
    each function's assembly (as conv_c3c1lc.hip's hand-off does)."""
    bad, writes, barriers, funcs = {}, 0, 0, 0
    for name, text in asm.items():
        for func, body in _functions(text, prefix=r'_Z'):
            funcs += 1
            pending = None
            for l in body:
                if not l or l.startswith(('.', ';')):
                    continue
                op = l.split()[0]
                if DS_WRITE.match(op):
                    pending = l
                    writes += 1
                elif op == 's_waitcnt' and 'lgkmcnt(0)' in l:
                    pending = None
                elif op == 's_barrier':
                    barriers += 1
                    if pending is not None:
                        if not any(src == name and re.search(k, func) for src, k in LDS_PUBLISH_EXCEPTIONS):
                            bad.setdefault((name, func), []).append(pending)
                        pending = None
    assert funcs >= 150 and writes >= 2000 and barriers >= 400, (funcs, writes, barriers)
    if bad:
        import subprocess as sp
        demangle = lambda f: sp.run(['c++filt', f], capture_output=True, text=True).stdout.strip() or f
        pytest.fail('LDS writes reach an s_barrier with no s_waitcnt lgkmcnt(0) in between (add one before ring_barrier()):\n' +
                    '\n'.join('  %s.hip: %s - %d barrier(s), last write before one: %s' % (src, demangle(f), len(w), w[-1])
                               for (src, f), w in sorted(bad.items())))


def test_no_kernel_calls_the_raw_barrier_builtin():
    """No source and no header calls the raw builtin, except the one call that IS ring_barrier() (dir_common.h): a raw barrier
    cannot come back through a shared header (conv_device.h) either."""
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert len(files) >= 30 and os.path.join(CSRC, 'conv_device.h') in files
    for f in files:
        src = open(f).read()
        if os.path.basename(f) == 'dir_common.h':
            body = re.search(r'__device__ __forceinline__ void ring_barrier\(\) \{\n(.*?)\n\}\n', src, re.S)
            assert body and body.group(1).count('__builtin_amdgcn_s_barrier') == 1
            src = src.replace(body.group(0), '')
        assert '__builtin_amdgcn_s_barrier' not in src, '%s: use ring_barrier() (dir_common.h)' % os.path.basename(f)
