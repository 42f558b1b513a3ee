"""The inverted file over sign-bit rows, host side (no GPU): the numpy restatement (tests/ivfbin_ref.py) is the composition
it claims to be and the fixture of tests/test_ivfbin_gpu.py has the properties those tests rely on; the library exports
dir_code_sums and dir_ivf_scan_bin, header and ctypes signatures agree, and the entries check their arguments and their
launch extents before anything is launched; the scan kernel compiles for gfx950 within its budget."""
import ctypes
import os
import re

import numpy as np
import pytest

import bin_ref
import index_ref
import ivf_ref
import ivfbin_ref
from topk_ref import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 16


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained():
    q, b = bin_ref.rerank_sets()
    return q, b, ivf_ref.train(b, NL, iters=10, seed=0)


def test_every_list_probed_is_the_flat_binary_search(trained):
    """nprobe = nlist masks nothing: the composition equals bin_ref.search, ids and value bits."""
    q, b, centroids = trained
    for k in (10, 100):
        got, want = ivfbin_ref.search(q, b, centroids, k, NL), bin_ref.search(q, b, k)
        assert (got[0] == want[0]).all() and (bits(got[1]) == bits(want[1])).all()
    own = np.arange(33, dtype=np.int32) * 5
    got, want = ivfbin_ref.search(q, b, centroids, 10, NL, exclude=own), bin_ref.search(q, b, 10, exclude=own)
    assert (got[0] == want[0]).all() and (bits(got[1]) == bits(want[1])).all()


def test_fixture_lists_are_uneven_and_some_query_runs_short(trained):
    """16 lists over the 3000 rows: one longer than a tile of the scan (256 rows) and one shorter than 64; at nprobe = 1,
    k = 100 some query has fewer than 100 candidates and ends in (-1, NaN), and no query is empty."""
    q, b, centroids = trained
    store = ivfbin_ref.build(b, centroids)
    lens = np.diff(store['list_off'])
    print('list sizes %d .. %d' % (lens.min(), lens.max()))
    assert lens.sum() == 3000 and lens.max() > 256 and lens.min() < 64
    cand = lens[ivf_ref.probe(*index_ref.quantize(q), centroids, 1)[:, 0]]
    idx, vals = ivfbin_ref.search(q, b, centroids, 100, 1)
    short = cand < 100
    print('%d queries run short at nprobe = 1, k = 100' % short.sum())
    assert short.any() and (idx[short, -1] == -1).all() and np.isnan(vals[short, -1]).all()
    assert (idx[~short] >= 0).all() and (idx[:, 0] >= 0).all()
    assert ((idx >= 0).sum(axis=1) == np.minimum(cand, 100)).all()


def test_store_is_a_stable_sort_of_the_bit_rows_by_the_int8_lists(trained):
    q, b, centroids = trained
    store, i8 = ivfbin_ref.build(b, centroids), ivf_ref.build(b, centroids)
    assert (store['ids'] == i8['ids']).all() and (store['list_off'] == i8['list_off']).all()      # the same lists
    codes, scales = bin_ref.quantize(b)
    assert (store['codes'] == codes[store['ids']]).all() and (bits(store['scales']) == bits(scales[store['ids']])).all()
    for l in range(NL):
        assert (np.diff(store['ids'][store['list_off'][l]:store['list_off'][l + 1]]) > 0).all()


def test_probed_search_is_a_plain_loop_over_the_probed_lists(trained):
    """One query at a time: the rows of its probed lists, scored by bin_ref.score, ranked by topk_ref."""
    from topk_ref import topk_ref_rows
    q, b, centroids = trained
    store = ivfbin_ref.build(b, centroids)
    (qc, qs), (bb, bs) = index_ref.quantize(q), bin_ref.quantize(b)
    for nprobe in (1, 3):
        probed = ivf_ref.probe(qc, qs, centroids, nprobe)
        got = ivfbin_ref.search(q, b, centroids, 20, nprobe)
        for i in range(0, 33, 4):
            cand = np.concatenate([store['ids'][store['list_off'][l]:store['list_off'][l + 1]] for l in probed[i]])
            s = bin_ref.score(qc[i:i + 1], qs[i:i + 1], bb[cand], bs[cand], 200)
            if len(cand) < 20:
                s = np.concatenate([s, np.zeros((1, 20 - len(cand)), np.float32)], axis=1)
                cand = np.concatenate([cand, np.full(20 - len(cand), -1, np.int32)])
            want = topk_ref_rows(s, 20, ids=cand[None].astype(np.int32))
            assert (got[0][i] == want[0][0]).all() and (bits(got[1][i]) == bits(want[1][0])).all(), (nprobe, i)


# ---- the library's host-side checks ------------------------------------------------------------------------------------
SCAN_ARGS = ['qcodes', 'ldq', 'qscales', 'qsums', 'Q', 'bits', 'ldb', 'bscales', 'ids', 'N', 'D', 'list_off', 'nlist', 'pair_off',
             'pair_q', 'pair_col', 'item_off', 'items', 'scores', 'out_ids', 'lds', 'width', 'stream']
SUMS_ARGS = ['qcodes', 'ldq', 'Q', 'D', 'qsums', 'stream']


def test_library_header_and_signatures_carry_the_entries():
    from dirtorch_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dir_engine.h')).read()
    for name, args in (('dir_ivf_scan_bin', SCAN_ARGS), ('dir_code_sums', SUMS_ARGS)):
        assert hasattr(lib, name), 'missing export ' + name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args)
        m = re.search(r'\nint %s\((.*?)\);' % name, header, re.S)
        assert m and len(m.group(1).split(',')) == len(args)
        assert [a.split()[-1].lstrip('*') for a in m.group(1).split(',')] == args
    assert 'dir_ivf_scan_bin         Q * width <= L, items * 768 <= L' in header           # the launch-limit table
    assert 'dir_code_sums            Q * 64 <= L' in header
    from dirtorch_amd import retrieve
    assert retrieve.INDEX_KINDS['ivfbin'] == ('IVFBinaryIndex', ('nlist',), True)


def _scan(lib, p):
    def scan(qc=p, ldq=256, qs=p, qsums=p, Q=3, bits=p, ldb=32, bs=p, ids=p, N=40, D=200, list_off=p, nlist=4, pair_off=p, pair_q=p,
             pair_col=p, item_off=p, items=2, scores=p, out_ids=p, lds=64, width=50):
        return lib.dir_ivf_scan_bin(qc, ldq, qs, qsums, Q, bits, ldb, bs, ids, N, D, list_off, nlist, pair_off, pair_q, pair_col,
                                    item_off, items, scores, out_ids, lds, width, None)
    return scan


def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    raw = ctypes.create_string_buffer(256 + 16)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) // 16 * 16)
    err = lib.dir_last_error
    scan = _scan(lib, p)
    assert scan(D=0) == -1 and b'D < 1' in err()
    assert scan(D=131073, ldq=131136, ldb=16400) == -1 and b'exceeds' in err()
    assert scan(ldq=192) == -1 and b'ldq' in err()                                   # below pad64(200) = 256
    assert scan(ldb=16) == -1 and b'ldb' in err()                                    # below bin_width(200) = 32
    assert scan(lds=49) == -1 and b'lds' in err()
    for name in ('Q', 'N', 'nlist', 'items', 'width'):
        assert scan(**{name: -1}) == -1 and b'negative' in err(), name
    for name in ('qc', 'qs', 'qsums', 'bits', 'bs', 'ids', 'list_off', 'pair_off', 'pair_q', 'pair_col', 'item_off', 'scores',
                 'out_ids'):
        assert scan(**{name: None}) == -1 and b'null' in err(), name
    assert scan(ldb=40) == -1 and scan(ldq=264) == -1 and b'16' in err()            # the scan moves 16-byte pieces
    off = ctypes.c_void_p(p.value + 8)
    assert scan(bits=off) == -1 and b'16-byte' in err() and scan(qc=off) == -1 and b'16-byte' in err()
    assert scan(ldb=1 << 23) == -1 and b'2^23' in err()                              # ldb * 256 rows within one descriptor
    assert scan(Q=1 << 23, lds=1, width=1) == -1 and b'2^31' in err()                # Q * ldq within one descriptor
    assert scan(nlist=0) == -1
    assert scan(Q=0) == 0 and scan(width=0, lds=0) == 0                              # nothing to do: DIR_OK, nothing launched
    assert scan(Q=0, qc=None, scores=None) == 0

    def sums(qc=p, ldq=200, Q=3, D=200, out=p):
        return lib.dir_code_sums(qc, ldq, Q, D, out, None)
    assert sums(D=0) == -1 and b'D < 1' in err()
    assert sums(D=131073, ldq=131073) == -1 and b'exceeds' in err()
    assert sums(ldq=199) == -1 and b'ldq' in err()
    assert sums(Q=-1) == -1 and b'negative' in err()
    assert sums(qc=None) == -1 and b'null' in err() and sums(out=None) == -1 and b'null' in err()
    assert sums(Q=0) == 0 and sums(Q=0, qc=None, out=None) == 0


def test_launch_extents_are_refused_without_a_gpu():
    """tests/test_launch_limits_cpu.py's manner for the launches of the two entries: the first inadmissible size, everything
    else valid, is DIR_ERR_INVALID with a message that names the entry and the product."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    raw = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) // 16 * 16)
    L = lib.dir_launch_max_threads()
    assert L == 2 ** 32 - 256

    def call(Q, width, items):
        return lib.dir_ivf_scan_bin(p, 64, p, p, Q, p, 16, p, p, 1, 64, p, 1, p, p, p, p, items, p, p, width, width, None)

    # one thread per id slot, 256 a workgroup
    Q, width = 65536, L // 65536 + 1
    assert -(-Q * width // 256) * 256 > L >= -(-Q * (width - 1) // 256) * 256 and width < 1 << 31
    assert call(Q, width, 0) == -1
    msg = lib.dir_last_error()
    assert msg.startswith(b'ivf_scan_bin:') and b'Q * width' in msg and b'2^32' in msg and b'cut the queries' in msg, msg
    # 768 threads per work item
    items = L // 768 + 1
    assert items * 768 > L >= (items - 1) * 768 and items < 1 << 31
    assert call(1, 1, items) == -1
    msg = lib.dir_last_error()
    assert msg.startswith(b'ivf_scan_bin:') and b'items * 768' in msg and b'2^32' in msg and b'cut the queries' in msg, msg
    # one wave per row of code_sums, four rows a workgroup
    Q = L // 64 + 1
    assert -(-Q // 4) * 256 > L >= -(-(Q - 1) // 4) * 256 and Q < 1 << 31
    assert lib.dir_code_sums(p, 1, Q, 1, p, None) == -1
    msg = lib.dir_last_error()
    assert msg.startswith(b'code_sums:') and b'Q * 64' in msg and b'2^32' in msg and b'cut the rows' in msg, msg


def test_scan_kernel_runs_on_the_int8_matrix_cores_without_scratch(tmp_path):
    """gfx950 assembly of csrc/ivf_bin.hip: every matrix instruction of the scan kernel is v_mfma_i32_32x32x32_i8, no
    scratch, no spills, within the registers of three waves per SIMD (768 threads), and every hand-off barrier between the
    two scheduler fences of ring_barrier()."""
    import shutil
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path / 'ivf_bin.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only',
                    os.path.join(ROOT, 'deep-image-retrieval_amd', 'csrc', 'ivf_bin.hip'), '-o', out], check=True,
                   capture_output=True)
    text = open(out).read()
    body = text[text.index('_ZN3dir19ivf_scan_bin_kernel'):]
    body = body[:body.index('.end_amdhsa_kernel')]
    lines = [l.strip() for l in body.split('\n') if l.strip() and not l.strip().startswith('.')]
    mfma = [l for l in lines if l.startswith('v_mfma')]
    assert len(mfma) >= 4 and all(l.startswith('v_mfma_i32_32x32x32_i8') for l in mfma)
    barriers = [i for i, l in enumerate(lines) if l.startswith('s_barrier')]
    assert len(barriers) >= 2
    for i in barriers:
        assert lines[i - 1].startswith('; sched_barrier mask(0x00000000)') and lines[i + 1].startswith('; sched_barrier mask(0x00000000)')
    meta = text[text.index('amdhsa.kernels'):]
    meta = meta[meta.index('_ZN3dir19ivf_scan_bin_kernel'):]
    assert int(re.search(r'\.private_segment_fixed_size:\s*(\d+)', meta).group(1)) == 0
    assert int(re.search(r'\.vgpr_spill_count:\s*(\d+)', meta).group(1)) == 0
    assert int(re.search(r'\.vgpr_count:\s*(\d+)', meta).group(1)) <= 168
