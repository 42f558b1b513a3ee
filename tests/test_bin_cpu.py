"""The binary descriptor index, host side (no GPU): the properties of the format the GPU tests compare against bit for bit
(tests/bin_ref.py) - the bit order, the scale's summation order, the degenerate rows, the integer bound that fixes the
widest row - the library's argument checks through the C ABI, the condition the GPU re-rank test rests on, and the
emitted code of the scan."""
import ctypes

import numpy as np

import bin_ref
import index_ref
from topk_ref import topk_ref_rows


def test_bits_are_numpys_little_packbits_of_the_clear_sign_bits():
    for D in (1, 7, 8, 9, 127, 128, 129, 200, 1000, 2048, 2049):
        r = np.random.RandomState(D)
        x = (r.standard_normal((6, D)) * np.exp(r.uniform(-20, 20, (6, 1)))).astype(np.float32)
        if D > 1:                                                   # (a row of zeros only has no bits: test_degenerate_rows)
            x[1, ::3] = -0.0                                        # -0.0 codes as 0,
            x[2, ::3] = 0.0                                         # +0.0 as 1
        bits, scales = bin_ref.quantize(x)
        ldb = bin_ref.width(D)
        assert bits.shape == (6, ldb) and bits.dtype == np.uint8 and ldb % 16 == 0 and 8 * ldb >= D > 8 * ldb - 128
        assert scales.shape == (6,) and scales.dtype == np.float32
        nb = (D + 7) // 8
        want = np.packbits(~np.signbit(x), axis=1, bitorder='little')
        assert (bits[:, :nb] == want).all() and not bits[:, nb:].any()
        if D % 8:
            assert not (bits[:, nb - 1] >> (D % 8)).any()           # the bits past D of the last byte
        for k in (0, D // 2, D - 1):
            assert (((bits[:, k >> 3] >> (k & 7)) & 1) == ~np.signbit(x[:, k])).all()
        s = bin_ref.signs(bits, D)
        assert (s == np.where(np.signbit(x), -1, 1)).all()


def test_scale_is_sumsq_over_sumabs_in_the_stated_order():
    """Against fp64: each sum is D / 64 + 5 additions deep per chain (and one rounding per square), the division one more
    rounding.  The order is pinned on values where it shows: the chain of lane 0 reaches 2^24 and swallows the ones that
    follow it, a sum in ascending k or a pairwise one does not."""
    r = np.random.RandomState(11)
    for D in (1, 5, 64, 255, 256, 257, 2048, 4100):
        x = (r.standard_normal((9, D)) * np.exp(r.uniform(-10, 10, (9, 1)))).astype(np.float32)
        _, scales = bin_ref.quantize(x)
        x64 = x.astype(np.float64)
        want = (x64 * x64).sum(axis=1) / np.abs(x64).sum(axis=1)
        depth = (D + 255) // 256 * 4 + 6
        assert (np.abs(scales - want) <= (2 * depth + 3) * 2.0 ** -24 * want).all(), D
    x = np.zeros((1, 1024), np.float32)
    x[0, 0] = 2.0 ** 24                                             # chain 0: 2^24, then k = 1, 2, 3, 256 .. 259, ...: + 1 each, lost
    x[0, 1:4] = x[0, 256:260] = x[0, 512:516] = 1
    x[0, 4:8] = 1                                                   # chain 1: 4, kept by the butterfly (2^24 + 4 is a float)
    _, scales = bin_ref.quantize(x)
    sumabs = np.float32(2.0 ** 24 + 4)
    sumsq = np.float32(2.0 ** 48)                                   # the squares of the ones vanish beside 2^48 either way
    assert scales[0] == sumsq / sumabs
    assert np.float32(np.float64(2.0 ** 48) / (2.0 ** 24 + 15)) != scales[0]        # what a sum that keeps every one gives


def test_degenerate_rows():
    x = np.ones((9, 70), np.float32)
    x[0] = 0
    x[1] = -0.0
    x[2, 5] = np.nan
    x[3, 69] = np.inf
    x[4, 0] = -np.inf
    x[5] = np.float32(3e38)                                         # sumabs overflows
    x[6] = np.float32(1e20)                                         # sumsq overflows, sumabs does not
    x[7] = -1
    bits, scales = bin_ref.quantize(x)
    assert not bits[:8].any()                                       # (row 7: every sign bit set)
    assert (scales[[0, 1, 5, 6]].view(np.uint32) == 0).all() and np.isnan(scales[2:5]).all()
    assert scales[7] == 1 and scales[8] == 1
    assert (bits[8, :8] == 0xff).all() and bits[8, 8] == 0x3f and not bits[8, 9:].any()
    q = np.ones((2, 70), np.int8)
    s = bin_ref.score(q, np.ones(2, np.float32), bits, scales, 70)
    assert np.isnan(s[:, 2:5]).all() and (s[:, [0, 1, 5, 6]] == 0).all() and (s[:, 7] == -70).all() and (s[:, 8] == 70).all()


def test_the_integer_bound_fixes_the_widest_row():
    """127 * D < 2^24 holds at D = 131072, the int8 index's widest row, so (float)t is exact; t of the worst pair - every
    query code 127 against all ones - is that bound and needs all 24 bits."""
    assert 127 * bin_ref.MAX_DIM < 2 ** 24 and 127 * bin_ref.MAX_DIM > 2 ** 23
    q = np.full((2, bin_ref.MAX_DIM), 127, np.int8)
    q[1] = -127
    bits = np.zeros((3, bin_ref.width(bin_ref.MAX_DIM)), np.uint8)
    bits[0] = 0xff
    bits[2] = 0x55
    t = bin_ref.dot(q, bits, bin_ref.MAX_DIM)
    assert t.tolist() == [[16646144, -16646144, 0], [-16646144, 16646144, 0]]
    assert (np.float32(t).astype(np.int64) == t).all()
    try:
        from dirtorch_amd import _lib
        lib = _lib.load()
    except (OSError, ImportError):
        lib = None
    if lib is not None:
        assert lib.dir_index_bin_max_dim() == bin_ref.MAX_DIM == lib.dir_index_i8_max_dim()


def test_score_is_the_inner_product_of_the_query_codes_and_the_signs():
    r = np.random.RandomState(76)
    for D in (1, 33, 200, 2048):
        q = (r.standard_normal((9, D)) * np.exp(r.uniform(-3, 3, (9, 1)))).astype(np.float32)
        b = (r.standard_normal((50, D)) * np.exp(r.uniform(-3, 3, (50, 1)))).astype(np.float32)
        qc, qs = index_ref.quantize(q)
        bits, bs = bin_ref.quantize(b)
        got = bin_ref.score(qc, qs, bits, bs, D)
        t = qc[:, :D].astype(np.int64) @ np.where(np.signbit(b), -1, 1).astype(np.int64).T
        assert (bin_ref.dot(qc, bits, D) == t).all()
        want = (t.astype(np.float64) * qs.astype(np.float64)[:, None]) * bs.astype(np.float64)[None, :]
        assert got.dtype == np.float32 and (np.abs(got - want) <= 2.0 ** -23 * np.abs(want)).all()    # two roundings
        # the kernel's form: 2 * sum qc_k b_k - sum qc_k
        on = np.unpackbits(bits, axis=1, bitorder='little')[:, :D].astype(np.int64)
        assert (2 * (qc[:, :D].astype(np.int64) @ on.T) - qc[:, :D].astype(np.int64).sum(axis=1)[:, None] == t).all()


def test_rerank_recovers_the_exact_lists():
    """What tests/test_bin_gpu.py's re-rank case rests on: with a shortlist of R = 1280 (k = 10) or 2048 (k = 100) from the
    binary scan, the k best of the shortlist by exact score ARE the k best of the database, for all 33 queries; at
    R = k they are not.  The smallest R that holds is printed: 1108 and 1978 when this was written."""
    q, b = bin_ref.rerank_sets()
    quant = bin_ref.score(*index_ref.quantize(q), *bin_ref.quantize(b), 200)
    exact = (q.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
    order = topk_ref_rows(quant, 3000)[0]
    place = np.empty_like(order)
    place[np.arange(33)[:, None], order] = np.arange(3000)[None, :]              # the rank of every row in the binary lists
    for k, R in ((10, 1280), (100, 2048)):
        want = topk_ref_rows(exact, k)[0]
        print('k = %d: the smallest shortlist that holds every exact list is %d' % (
            k, 1 + int(place[np.arange(33)[:, None], want].max())))
        same = {}
        for r in (k, R):
            cand = topk_ref_rows(quant, r)[0]
            got = topk_ref_rows(np.take_along_axis(exact, cand.astype(np.int64), axis=1), k, ids=cand)[0]
            same[r] = int((got == want).all(axis=1).sum())
        print('k = %d: %d of 33 lists exact at R = k, %d at R = %d' % (k, same[k], same[R], R))
        assert same[R] == 33
        assert same[k] < 33                      # the shortlist is doing work


def test_retrieve_knows_the_kind():
    from dirtorch_amd import retrieve
    assert retrieve.INDEX_KINDS['bin'] == ('BinaryIndex', (), False)
    from dirtorch_amd import index
    assert issubclass(index.BinaryIndex, index._CodedIndex)


# ---- the library's host-side checks ------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    assert lib.dir_index_bin_max_dim() == 131072
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dir_last_error

    def quant(X=p, ldx=200, N=5, D=200, bits=p, ldb=32, scales=p):
        return lib.dir_quantize_rows_bin(X, ldx, N, D, bits, ldb, scales, None)

    assert quant(D=0) == -1 and b'D < 1' in err()
    assert quant(D=131073, ldx=131073, ldb=16400) == -1 and b'exceeds' in err()
    assert quant(ldb=28) == -1 and b'ldb' in err()                # ceil(D / 8) = 25, but below D rounded up to 128, over 8
    assert quant(ldx=199) == -1 and b'ldx' in err()
    assert quant(N=-1) == -1 and b'negative' in err()
    for name in ('X', 'bits', 'scales'):
        assert quant(**{name: None}) == -1 and b'null' in err(), name
    assert quant(ldb=34) == -1 and b'ldb % 4' in err()
    assert quant(N=0, X=None, bits=None, scales=None) == 0

    def sim(qc=p, ldq=256, qs=p, Q=3, bits=p, ldb=32, bs=p, N=40, D=200, scores=p, lds=40):
        return lib.dir_similarity_bin(qc, ldq, qs, Q, bits, ldb, bs, N, D, scores, lds, None)

    assert sim(D=0) == -1 and b'D < 1' in err()
    assert sim(D=131073, ldq=131136, ldb=16400) == -1 and b'exceeds' in err()
    assert sim(ldq=199) == -1 and b'ldq' in err()
    assert sim(ldb=16) == -1 and b'ldb' in err()
    assert sim(lds=39) == -1 and b'lds' in err()
    assert sim(Q=-1) == -1 and sim(N=-1) == -1 and b'negative' in err()
    for name in ('qc', 'qs', 'bits', 'bs', 'scores'):
        assert sim(**{name: None}) == -1 and b'null' in err(), name
    assert sim(ldb=40) == -1 and b'16' in err()                   # the scan moves 16-byte pieces
    assert sim(Q=0) == 0 and sim(N=0, lds=0) == 0                 # nothing to do: DIR_OK, nothing launched
    # launch limits (include/dir_engine.h): refused by name before anything is launched
    L = lib.dir_launch_max_threads()
    N = (L // 64 // 4 + 1) * 4                                    # one wave per row, four rows per workgroup
    assert quant(N=N) == -1 and b'quantize_rows_bin: N * 64' in err()
    N = (L // 768 + 1) * 256                                      # 768 threads per 256 rows
    assert N < 1 << 31 and sim(N=N, lds=N) == -1 and b'similarity_bin: N * 3' in err()
    assert sim(Q=65535 * 96 + 1) == -1 and b'65535 * 96' in err()


# ---- the emitted code of the scan --------------------------------------------------------------------------------------
def test_scan_kernel_runs_on_the_int8_matrix_cores_without_scratch(tmp_path):
    """gfx950 assembly of csrc/index_bin.hip: the scan's matrix instructions are v_mfma_i32_32x32x32_i8 and nothing else
    (twelve per sub-slab of 128 k: four steps of 32 k x three query row blocks), it spills nothing, and each hand-off
    barrier sits between the two scheduler fences of ring_barrier().  The register budget: 768 threads and 144 KB of LDS
    make one workgroup per CU, three waves per SIMD, which leaves a wave 512 / 3 = 170 registers, 168 in whole granules
    of 8 - the budget of the int8 and fp4 scans."""
    import os
    import re
    import shutil
    import subprocess
    import pytest
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'index_bin.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only',
                    os.path.join(root, 'deep-image-retrieval_amd', 'csrc', 'index_bin.hip'), '-o', out], check=True,
                   capture_output=True)
    text = open(out).read()
    body = text[text.index('_ZN3dir14sim_bin_kernel'):]
    body = body[:body.index('s_endpgm')]
    lines = [l.strip() for l in body.split('\n') if l.strip() and not l.strip().startswith('.')]
    mfma = [l for l in lines if l.startswith('v_mfma') or l.startswith('v_smfma') or l.startswith('v_dot')]
    assert len(mfma) == 12 and all(l.startswith('v_mfma_i32_32x32x32_i8') for l in mfma)
    barriers = [i for i, l in enumerate(lines) if l.startswith('s_barrier')]
    assert len(barriers) >= 2
    for i in barriers:
        assert lines[i - 1].startswith('; sched_barrier mask(0x00000000)') and lines[i + 1].startswith('; sched_barrier mask(0x00000000)')
    assert not any(l.startswith('scratch_') for l in lines)
    meta = text[text.index('amdhsa.kernels'):]
    meta = meta[meta.index('_ZN3dir14sim_bin_kernel'):]
    assert int(re.search(r'\.private_segment_fixed_size:\s*(\d+)', meta).group(1)) == 0
    assert int(re.search(r'\.vgpr_count:\s*(\d+)', meta).group(1)) <= 168
