"""Launch extents, the checks that need no GPU: the inventory (tests/launch_limits.py) against the launch sites of the
sources, its formulas at the edge, every refusal through the C ABI and the host query.

The refusals launch nothing because the guard under test returns first: every pointer is a 16-byte aligned HOST address.
Without a GPU a missing guard shows as a HIP error and a failed assertion here."""
import ctypes
import os
import re

import pytest

from launch_limits import FILES, ROWS, Y_LIMIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'deep-image-retrieval_amd', 'csrc')
DIR_ERR_INVALID = -1


@pytest.fixture(scope='module')
def lib():
    from dirtorch_amd import _lib
    return _lib.load()


def _limit(lib, row):
    return lib.dir_launch_max_threads() if row.axis == 'x' else Y_LIMIT


def _id(row):
    return '%s-%s-%s' % (row.file, row.kernel, row.axis)


def _launch_sites(name):
    """[(kernel name)] of every hipLaunchKernelGGL in csrc/<name>.hip, comments dropped; a launch through a function pointer
    (`auto kern = cond ? a_kernel<..> : ..`) counts under the kernel the pointer is chosen from."""
    src = open(os.path.join(CSRC, name + '.hip')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    out = []
    for m in re.finditer(r'hipLaunchKernelGGL\(\s*\(?\s*(\w+)', src):
        kernel = m.group(1)
        if not kernel.endswith('_kernel'):
            chosen = re.search(r'\bauto\s+%s\s*=[^;]*?(\w+_kernel)\b' % kernel, src)
            assert chosen, '%s.hip launches %s, which is neither a kernel nor a pointer chosen among kernels' % (name, kernel)
            kernel = chosen.group(1)
        assert re.search(r'__global__[^;{]*\b%s\(' % kernel, src), '%s.hip: no __global__ %s' % (name, kernel)
        out.append(kernel)
    return out


def test_host_query(lib):
    L = lib.dir_launch_max_threads()
    assert 0 < L < 1 << 32 and L % 256 == 0
    assert L + 256 >= 1 << 32, 'the largest multiple of 256 below 2^32'
    header = open(os.path.join(ROOT, 'include', 'dir_engine.h')).read()
    assert 'int64_t dir_launch_max_threads(void);' in header
    from dirtorch_amd import _lib
    assert _lib.SIGNATURES['dir_launch_max_threads'] == (ctypes.c_int64, [])
    common = open(os.path.join(CSRC, 'dir_common.h')).read()
    assert re.search(r'kMaxLaunchThreads = 0x%xu;' % L, common)
    # one rule in one place: no source of the inventory keeps a limit of its own
    for name in FILES:
        src = open(os.path.join(CSRC, name + '.hip')).read()
        assert '0x7fffffffL' not in src and '0xffffff00' not in src and '(unsigned)ceil_div(N, 4)' not in src, name


def test_inventory_lists_every_launch_site():
    assert len(set(FILES)) == len(FILES) == 16
    found = {}
    for name in FILES:
        for kernel in _launch_sites(name):
            found[(name, kernel)] = found.get((name, kernel), 0) + 1
    listed = {}
    for row in ROWS:
        assert listed.setdefault((row.file, row.kernel), row.sites) == row.sites, 'rows of %s disagree on the sites' % row.kernel
    assert set(listed) == set(found), 'launches without a row: %s; rows without a launch: %s' % (
        sorted(set(found) - set(listed)), sorted(set(listed) - set(found)))
    assert listed == found
    for row in ROWS:
        assert row.kind in ('split', 'refuse', 'bounded') and row.entry.startswith('dir_')
        if row.kind == 'bounded':
            assert isinstance(row.why, str) and len(row.why) > 20
        else:
            assert row.axis in ('x', 'y') and callable(row.extent) and callable(row.first)
    assert [r.kernel for r in ROWS if r.kind == 'split'] == ['gather_scores_kernel']
    # an axis is decided once per pair
    keys = [(r.file, r.kernel, r.axis, r.kind, r.vary) for r in ROWS]
    assert len(set(keys)) == len(keys)


def test_a_deleted_row_fails_the_completeness_check():
    """The check above is the one that notices a launch without a row: without gather_scores' row the sets differ."""
    listed = {(r.file, r.kernel) for r in ROWS if r.kernel != 'gather_scores_kernel'}
    found = {('index_i8', k) for k in _launch_sites('index_i8')}
    assert found - listed == {('index_i8', 'gather_scores_kernel')}


@pytest.mark.parametrize('row', [r for r in ROWS if r.kind != 'bounded'], ids=_id)
def test_formula_at_the_edge(lib, row):
    limit = _limit(lib, row)
    sizes = row.first(limit)
    assert row.extent(**sizes) > limit
    below = dict(sizes)
    below[row.vary] -= row.step
    assert below[row.vary] > 0 and 0 < row.extent(**below) <= limit
    assert all(0 < v < 1 << 31 or (v == 0 and k in ('items', 'iters')) for k, v in sizes.items()), 'sizes are ints of the C ABI'


# ---- the refusals ------------------------------------------------------------------------------------------------------
def _calls(lib, p):
    """entry -> a call with every argument valid (host pointer p, null stream) for the sizes of a row's first(L)."""
    big = 1 << 62
    assert lib.dir_topk_max_k() == 2048      # the k of the knn_graph row
    return {
        'dir_quantize_rows_i8': lambda N: lib.dir_quantize_rows_i8(p, 4, N, 4, p, 64, p, None),
        'dir_similarity_i8': lambda N, Q: lib.dir_similarity_i8(p, 64, p, Q, p, 64, p, N, 64, p, N, None),
        'dir_quantize_rows_fp4': lambda N: lib.dir_quantize_rows_fp4(p, 4, N, 4, p, 32, p, 8, p, None),
        'dir_similarity_fp4': lambda N, Q: lib.dir_similarity_fp4(p, 32, p, 8, p, Q, p, 32, p, 8, p, N, 64, p, N, None),
        'dir_quantize_rows_bin': lambda N: lib.dir_quantize_rows_bin(p, 4, N, 4, p, 16, p, None),
        'dir_code_sums': lambda Q: lib.dir_code_sums(p, 4, Q, 4, p, None),
        'dir_similarity_bin': lambda N, Q: lib.dir_similarity_bin(p, 64, p, Q, p, 16, p, N, 64, p, N, None),
        'dir_segment_sums': lambda S: lib.dir_segment_sums(p, 1, 1, 1, p, p, S, p, 1, None),
        'dir_ivf_scan_i8': lambda Q, width, items: lib.dir_ivf_scan_i8(p, 64, p, Q, p, 64, p, p, 1, 64, p, 1, p, p, p, p, items, p, p,
                                                                       width, width, None),
        'dir_ivfpq_base': lambda Q, nprobe: lib.dir_ivfpq_base(p, 4, Q, p, 4, 1, 4, 1, p, nprobe, p, None),
        'dir_ivfpq_scan': lambda Q, width: lib.dir_ivfpq_scan(p, p, Q, 4, p, 4, p, 1, p, 1, p, p, 1, p, p, width, width, None),
        'dir_pq_encode': lambda N, M: lib.dir_pq_encode(p, M, N, M, M, p, p, M, None),
        'dir_pq_lut': lambda Q, M: lib.dir_pq_lut(p, M, Q, M, M, p, p, None),
        'dir_rank_counts': lambda Q: lib.dir_rank_counts(p, 1, Q, 1, p, 1, p, p, None),
        'dir_expand_descriptors': lambda n: lib.dir_expand_descriptors(p, n, p, 1, 1, 0, 1.0, 0, p, p, 4 * n, None),
        'dir_revisitop_ap': lambda Q, modes: lib.dir_revisitop_ap(p, Q, 1, p, p, p, p, p, p, modes, p, p, None),
        'dir_label_rank': lambda Q: lib.dir_label_rank(p, 1, Q, 1, p, p, p, 1, p, p, p, p, None),
        'dir_expand_lists': lambda n: lib.dir_expand_lists(p, 1, n, p, 1, 1, 1, p, p, 1, 1, 1.0, p, 1, None),
        'dir_knn_graph': lambda N, k: lib.dir_knn_graph(p, p, k, N, k, 3.0, p, k, None),
        'dir_diffusion_seed': lambda N, Q: lib.dir_diffusion_seed(p, p, 1, Q, 1, N, 3.0, p, Q, None),
        'dir_diffusion_solve': lambda N, Q, iters: lib.dir_diffusion_solve(p, 1, p, 1, N, 1, p, Q, Q, 0.5, iters, p, Q, p, big, None),
        'dir_prep_input': lambda B, H, W: lib.dir_prep_input(p, 1, (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(1, 1, 1), p,
                                                             B, H, W, 0, None),
        'dir_maxpool_3x3s2': lambda B, H, W, C: lib.dir_maxpool_3x3s2(p, p, B, H, W, C, 0, None),
        'dir_global_pool': lambda B, C: lib.dir_global_pool(p, p, B, 1, 1, C, 0, 3.0, 1e-6, 0.0, 0, None),
        'dir_upsample_add': lambda B, H, W, C: lib.dir_upsample_add(p, p, p, B, H, W, H // 2, W // 2, C, 0, None),
        'dir_l2norm_rows': lambda rows: lib.dir_l2norm_rows(p, rows, 1, 1e-12, None),
        'dir_multiscale_pool': lambda N, D: lib.dir_multiscale_pool(p, p, 1, N, D, 0, 3.0, None),
        'dir_resize_bilinear_u8': lambda B, H, W, OH, OW: lib.dir_resize_bilinear_u8(p, p, B, H, W, OH, OW, p, big, None),
        'dir_gemm_nt_f32': lambda NP, NQ: lib.dir_gemm_nt_f32(p, 4, p, 4, p, NP, NP, NQ, 4, None, None, None, None),
    }


@pytest.mark.parametrize('row', [r for r in ROWS if r.kind == 'refuse'], ids=_id)
def test_refusal_needs_no_gpu(lib, row):
    """The first inadmissible size of the row, everything else valid: DIR_ERR_INVALID, and the message names the entry and
    the extent.  (One step lower is admissible and WOULD launch: that side is the formula test's, in Python alone.)"""
    raw = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) // 16 * 16)
    sizes = row.first(_limit(lib, row))
    rc = _calls(lib, p)[row.entry](**sizes)
    msg = lib.dir_last_error()
    assert rc == DIR_ERR_INVALID, (rc, msg)
    assert msg.startswith(row.entry[4:].replace('resize_bilinear_u8', 'resize').replace('maxpool_3x3s2', 'maxpool').encode() + b':'), msg
    assert row.keyword in msg, msg
    assert (b'2^32' in msg) == (row.axis == 'x') and (b'65535' in msg) == (row.axis == 'y'), msg


def test_every_refused_entry_has_a_call(lib):
    calls = _calls(lib, ctypes.c_void_p(16))
    assert {r.entry for r in ROWS if r.kind == 'refuse'} == set(calls)


def test_gather_scores_states_no_pair_limit(lib):
    """The split entry refuses no Q * R: with R = 0 columns of candidates the largest int Q is DIR_OK and launches nothing,
    and the message of the retired 2^33 guard is gone from the source."""
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) // 16 * 16)
    assert lib.dir_gather_scores(p, 1, (1 << 31) - 1, p, 1, 1, 1, p, 0, 0, p, 0, None) == 0
    assert '2^33' not in open(os.path.join(CSRC, 'index_i8.hip')).read()
