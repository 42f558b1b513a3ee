"""The int8 descriptor index, host side (no GPU): the properties of the quantisation the GPU tests compare against bit for bit
(tests/index_ref.py), the library's argument checks through the C ABI - they run before anything is launched - and the
condition the GPU re-rank test rests on, held here by the restatement alone."""
import ctypes

import numpy as np

import index_ref
from synth import synth_descriptors
from topk_ref import topk_ref_rows


def _rows():
    r = np.random.RandomState(71)
    for D in (1, 63, 64, 65, 200, 2048):
        x = (r.standard_normal((37, D)) * np.exp(r.uniform(-20, 20, (37, 1)))).astype(np.float32)
        yield D, x
    yield 200, synth_descriptors(6, 300, 200)


def test_quantisation_properties():
    for D, x in _rows():
        codes, scales = index_ref.quantize(x)
        assert codes.dtype == np.int8 and scales.dtype == np.float32
        assert codes.shape == (len(x), index_ref.pad64(D)) and not codes[:, D:].any()
        assert codes.min() >= -127 and codes.max() <= 127
        top = np.abs(x).argmax(axis=1)
        assert (np.abs(codes[np.arange(len(x)), top].astype(int)) == 127).all()       # the largest entry maps to +-127
        assert (scales == np.abs(x).max(axis=1) / np.float32(127)).all()
        # reconstruction in fp64: half a step, plus 127 * 2^-23 of a step each for the roundings of inv and the multiply
        # and for those of scale and the reconstruction
        err = np.abs(x.astype(np.float64) - codes[:, :D].astype(np.float64) * scales.astype(np.float64)[:, None])
        assert (err <= (0.5 + 2.0 ** -15) * scales.astype(np.float64)[:, None]).all(), D


def test_degenerate_rows():
    x = np.ones((6, 70), np.float32)
    x[0] = 0
    x[1] = np.float32(1e-40)                    # subnormal: 127 / amax overflows
    x[2, 5] = np.nan
    x[3, 69] = np.inf
    x[4, 0] = -np.inf
    codes, scales = index_ref.quantize(x)
    assert not codes[:5].any()
    assert scales[0] == 0 and scales[1] == 0 and np.isnan(scales[2:5]).all()
    assert (codes[5, :70] == 127).all() and scales[5] == np.float32(1) / np.float32(127)
    # entries at exactly half a step round to even: amax = 127 makes inv exactly 1
    h = np.array([[127, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 125.5, 126.5, -126.5]], np.float32)
    codes, scales = index_ref.quantize(h)
    assert codes[0, :10].tolist() == [127, 0, 2, 2, 0, -2, -2, 126, 126, -126] and scales[0] == 1


def test_score_is_the_int32_form():
    r = np.random.RandomState(72)
    cq = r.randint(-127, 128, (9, 192)).astype(np.int8)
    cb = r.randint(-127, 128, (50, 192)).astype(np.int8)
    sq, sb = r.rand(9).astype(np.float32), r.rand(50).astype(np.float32)
    want = ((cq.astype(np.int32) @ cb.astype(np.int32).T).astype(np.float32) * sq[:, None]) * sb[None, :]
    got = index_ref.score(cq, sq, cb, sb)
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()
    big = np.full((1, 131072), 127, np.int8)
    assert index_ref.dots(big, big)[0, 0] == 2114060288


def test_rerank_recovers_the_exact_lists():
    """What tests/test_index_gpu.py's re-rank case rests on: with a shortlist of R = 4k from the quantised scan, the k best
    of the shortlist by exact score ARE the k best of the database, for all 33 queries; at R = k they are not."""
    q, b = synth_descriptors(5, 33, 200), synth_descriptors(6, 3000, 200)
    quant = index_ref.score(*index_ref.quantize(q), *index_ref.quantize(b))
    exact = (q.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
    for k, R in ((10, 40), (100, 400)):
        want = topk_ref_rows(exact, k)[0]
        same = {}
        for r in (k, R):
            cand = topk_ref_rows(quant, r)[0]
            got = topk_ref_rows(np.take_along_axis(exact, cand.astype(np.int64), axis=1), k, ids=cand)[0]
            same[r] = int((got == want).all(axis=1).sum())
        print('k = %d: %d of 33 lists exact at R = k, %d at R = %d' % (k, same[k], same[R], R))
        assert same[R] == 33
        assert same[k] < 33                      # the shortlist is doing work


# ---- the library's host-side checks ------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    assert lib.dir_index_i8_max_dim() == 131072
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dir_last_error

    def quant(X=p, ldx=200, N=5, D=200, codes=p, ldc=256, scales=p):
        return lib.dir_quantize_rows_i8(X, ldx, N, D, codes, ldc, scales, None)

    assert quant(D=0) == -1 and b'D < 1' in err()
    assert quant(D=131073, ldx=131073, ldc=131136) == -1 and b'exceeds' in err()
    assert quant(ldc=199) == -1 and b'ldc' in err()
    assert quant(ldc=200) == -1 and b'ldc' in err()              # below D rounded up to 64
    assert quant(ldx=199) == -1 and b'ldx' in err()
    assert quant(N=-1) == -1 and b'negative' in err()
    assert quant(X=None) == -1 and b'null' in err()
    assert quant(codes=None) == -1 and quant(scales=None) == -1
    assert quant(N=0, X=None, codes=None, scales=None) == 0

    def sim(qc=p, ldq=256, qs=p, Q=3, bc=p, ldb=256, bs=p, N=40, D=200, scores=p, lds=40):
        return lib.dir_similarity_i8(qc, ldq, qs, Q, bc, ldb, bs, N, D, scores, lds, None)

    assert sim(D=0) == -1 and b'D < 1' in err()
    assert sim(D=131073, ldq=131136, ldb=131136) == -1 and b'exceeds' in err()
    assert sim(ldq=199) == -1 and b'ldq' in err()
    assert sim(ldb=199) == -1 and b'ldb' in err()
    assert sim(lds=39) == -1 and b'lds' in err()
    assert sim(Q=-1) == -1 and sim(N=-1) == -1 and b'negative' in err()
    for name in ('qc', 'qs', 'bc', 'bs', 'scores'):
        assert sim(**{name: None}) == -1 and b'null' in err(), name
    assert sim(ldb=264) == -1 and b'16' in err()                 # the scan moves 16-byte pieces
    assert sim(Q=0) == 0 and sim(N=0, lds=0) == 0                # nothing to do: DIR_OK, nothing launched

    def gather(qm=p, ldq=200, Q=3, db=p, ldb=200, N=40, D=200, cand=p, ldcand=8, R=8, scores=p, ldsc=8):
        return lib.dir_gather_scores(qm, ldq, Q, db, ldb, N, D, cand, ldcand, R, scores, ldsc, None)

    assert gather(D=0) == -1 and b'D < 1' in err()
    assert gather(ldq=199) == -1 and gather(ldb=199) == -1 and b'ld' in err()
    assert gather(ldcand=7) == -1 and gather(ldsc=7) == -1 and b'R' in err()
    assert gather(Q=-1) == -1 and gather(N=-1) == -1 and gather(R=-1, ldcand=0, ldsc=0) == -1 and b'negative' in err()
    for name in ('qm', 'db', 'cand', 'scores'):
        assert gather(**{name: None}) == -1 and b'null' in err(), name
    assert gather(Q=0) == 0 and gather(N=0) == 0


# ---- the emitted code of the scan --------------------------------------------------------------------------------------
def test_scan_kernel_runs_on_the_int8_matrix_cores_behind_fenced_barriers(tmp_path):
    """gfx950 assembly of csrc/index_i8.hip: the scan multiplies on v_mfma_i32_32x32x32_i8 (twelve per K slab: four steps
    of 32 k x three query row blocks), spills nothing, and each of its hand-off barriers - the loaders' and the
    consumers' - sits between the two scheduler fences of ring_barrier() (tests/test_isa_audit.py holds the other ring
    kernels to the same rule)."""
    import os
    import re
    import shutil
    import subprocess
    import pytest
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'index_i8.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only',
                    os.path.join(root, 'deep-image-retrieval_amd', 'csrc', 'index_i8.hip'), '-o', out], check=True,
                   capture_output=True)
    text = open(out).read()
    body = text[text.index('_ZN3dir13sim_i8_kernel'):]
    body = body[:body.index('s_endpgm')]
    lines = [l.strip() for l in body.split('\n') if l.strip() and not l.strip().startswith('.')]
    assert sum(l.startswith('v_mfma_i32_32x32x32_i8') for l in lines) == 12
    assert not any(l.startswith('v_mfma_f32') for l in lines)
    barriers = [i for i, l in enumerate(lines) if l.startswith('s_barrier')]
    assert len(barriers) >= 2
    for i in barriers:
        assert lines[i - 1].startswith('; sched_barrier mask(0x00000000)') and lines[i + 1].startswith('; sched_barrier mask(0x00000000)')
    meta = text[text.index('amdhsa.kernels'):]
    meta = meta[meta.index('_ZN3dir13sim_i8_kernel'):]
    assert int(re.search(r'\.private_segment_fixed_size:\s*(\d+)', meta).group(1)) == 0
