"""The fp4 descriptor index, host side (no GPU): the properties of the format the GPU tests compare against bit for bit
(tests/fp4_ref.py) - the tie table, the three-binade clamp, the degenerate rows, the integer bound that fixes the widest
row - the library's argument checks through the C ABI, and the condition the GPU re-rank test rests on."""
import ctypes

import numpy as np

import fp4_ref
from topk_ref import topk_ref_rows

MID = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5], np.float32)          # the midpoints of the grid
MID_TO = np.array([0, 1, 1, 2, 2, 4, 4], np.float32)                       # ... go to the even code
SAT = np.array([5.0000005, 6, 6.5, 7, 7.9999995], np.float32)              # (5, 8) -> 6


def _values(codes, exps, D):
    """the stored values in units of the row scale"""
    return fp4_ref.integers(codes, exps, D).astype(np.float64) / 8


def test_ties_go_to_the_even_code_in_every_binade_of_the_clamp():
    """Three blocks at the levels E, E - 1, E - 2, each holding every midpoint of the grid, the values just beside them,
    the saturating range and both signs, for rows from the smallest to the largest scale."""
    for E in (-62, -31, -1, 0, 17, 125):
        row = np.zeros(96, np.float32)
        want = np.zeros(96)
        for blk, level in enumerate((E, E - 1, E - 2)):
            step = np.float32(2.0) ** np.float32(level)
            up, down = np.nextafter(MID, np.float32(8)), np.nextafter(MID, np.float32(0))
            y = np.concatenate([MID, -MID, up, down, [6, 7.9999995, -7, 4]]).astype(np.float32)
            w = np.concatenate([MID_TO, -MID_TO, fp4_ref.GRID[1:8], fp4_ref.GRID[0:7], [6, 6, -6, 4]])
            assert len(y) == len(w) == 32 and np.abs(y).max() >= 4   # the block's level: amax in [4, 8) steps
            row[32 * blk:32 * blk + 32] = y * step
            want[32 * blk:32 * blk + 32] = w * 2.0 ** (level - E)
        codes, exps, scales = fp4_ref.quantize(row[None])
        assert exps[0, :3].tolist() == [127, 126, 125] and scales[0] == np.float32(2.0) ** np.float32(E), E
        got = _values(codes, exps, 96)[0]
        assert (got == want).all(), (E, np.flatnonzero(got != want)[:5])
    # the table of the definition, as codes
    assert fp4_ref.round_codes(MID).tolist() == [0, 2, 2, 4, 4, 6, 6]
    assert fp4_ref.round_codes(SAT).tolist() == [7] * 5


def test_blocks_below_the_third_binade_are_clamped():
    """A row whose blocks span eight binades: the block bytes are 127, 126, 125, 125, ..., a clamped block is coded on
    the grid of E - 2 (values below a quarter of its step vanish), and no block's error exceeds the top block's bound."""
    D = 256
    x = np.zeros((1, D), np.float32)
    r = np.random.RandomState(3)
    for b in range(8):
        x[0, 32 * b:32 * b + 32] = r.uniform(-1, 1, 32) * 2.0 ** -b
        x[0, 32 * b] = 1.5 * 2.0 ** -b                             # amax_b in [2^-b, 2^(1-b))
    codes, exps, scales = fp4_ref.quantize(x)
    assert exps[0].tolist() == [127, 126] + [125] * 6 and scales[0] == 2.0 ** -2       # E = floor(log2 1.5) - 2
    v = fp4_ref.dequantize(codes, exps, scales, D)[0]
    step = 2.0 ** (-2 - 2)                                          # the clamped blocks' unit, 2^(E - 2)
    tail = x[0, 64:].astype(np.float64)
    assert (v[64:] == np.sign(tail) * fp4_ref.GRID[fp4_ref.round_codes(np.abs(tail / step).astype(np.float32))] * step).all()
    assert (v[np.abs(x[0]) <= 0.25 * step] == 0).all() and (np.abs(x[0]) <= 0.25 * step).sum() > 8
    assert (np.abs(v - x[0]) <= 2.0 ** -2).all()                    # half of the widest gap (4 .. 6) at the top level
    assert not ((codes[0] & 0x0f) == 8).any() and not ((codes[0] >> 4) == 8).any()          # a value that rounds to zero is +0


def test_layout_and_padding():
    for D in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2048, 2500):
        r = np.random.RandomState(D)
        x = (r.standard_normal((5, D)) * np.exp(r.uniform(-20, 20, (5, 1)))).astype(np.float32)
        codes, exps, scales = fp4_ref.quantize(x)
        ldc, lde = fp4_ref.widths(D)
        assert codes.shape == (5, ldc) and exps.shape == (5, lde) and ldc % 16 == 0 and 2 * ldc >= D and lde % 8 == 0
        assert codes.dtype == np.uint8 and exps.dtype == np.uint8 and scales.dtype == np.float32
        nb = (D + 31) // 32
        assert (exps[:, nb:] == 127).all() and (exps[:, :nb] >= 125).all() and (exps[:, :nb] <= 127).all()
        assert (exps[:, :nb] == 127).any(axis=1).all()              # a top block in every row
        assert not codes[:, (D + 1) // 2:].any() and (D % 2 == 0 or not (codes[:, D // 2] >> 4).any())
        # even k in the low nibble: the largest entry of a row is coded 4 or 6 at its place
        top = np.abs(x).argmax(axis=1)
        nib = (codes[np.arange(5), top // 2] >> (4 * (top % 2))) & 7
        assert np.isin(nib, (6, 7)).all()
        err = np.abs(fp4_ref.dequantize(codes, exps, scales, D) - x)
        assert (err <= 2 * scales.astype(np.float64)[:, None]).all()      # saturation: [6, 8) steps of the top level -> 6


def test_degenerate_rows():
    x = np.ones((8, 70), np.float32)
    x[0] = 0
    x[1] = np.float32(1e-40)                                        # subnormal
    x[2] = np.float32(2.0 ** -61)                                   # normal, below 2^-60
    x[3, 5] = np.nan
    x[4, 69] = np.inf
    x[5, 0] = -np.inf
    x[6] = 0
    x[6, 40] = -np.float32(2.0 ** -60)                              # the smallest row that is kept; a single non-zero
    codes, exps, scales = fp4_ref.quantize(x)
    assert not codes[:6].any() and (exps[:6] == 127).all()
    assert (scales[:3].view(np.uint32) == 0).all() and np.isnan(scales[3:6]).all()
    assert scales[6] == np.float32(2.0 ** -62) and exps[6].tolist() == [125, 127, 125, 127, 127, 127, 127, 127]
    assert codes[6, 20] == 0x0e and not np.delete(codes[6], 20).any()                 # -4 * 2^-62: sign, code 6, low nibble
    assert (codes[7, :35] == 0x66).all() and scales[7] == 0.25                         # 1 = 4 * 2^-2


def test_the_integer_bound_fixes_the_widest_row():
    """36 * 64 * D < 2^24 holds at D = 7281 and breaks at 7282; the worst row - every code +-6 at the top level - scores
    exactly that against itself."""
    assert 36 * 64 * fp4_ref.MAX_DIM < 2 ** 24 <= 36 * 64 * (fp4_ref.MAX_DIM + 1)
    x = np.full((1, fp4_ref.MAX_DIM), 6, np.float32)
    c, e, s = fp4_ref.quantize(x)
    assert s[0] == 1 and (e[0, :228] == 127).all()
    ints = fp4_ref.integers(c, e, fp4_ref.MAX_DIM)
    assert (ints == 48).all() and int((ints * ints).sum()) == 36 * 64 * fp4_ref.MAX_DIM == 16775424
    assert fp4_ref.acc(c, e, c, e, fp4_ref.MAX_DIM)[0, 0] == 36 * fp4_ref.MAX_DIM
    try:
        from dirtorch_amd import _lib
        lib = _lib.load()
    except (OSError, ImportError):
        lib = None
    if lib is not None:
        assert lib.dir_index_fp4_max_dim() == fp4_ref.MAX_DIM


def test_score_is_the_inner_product_of_the_dequantised_rows():
    r = np.random.RandomState(75)
    for D in (1, 33, 200, 2048):
        q = (r.standard_normal((9, D)) * np.exp(r.uniform(-3, 3, (9, 1)))).astype(np.float32)
        b = (r.standard_normal((50, D)) * np.exp(r.uniform(-3, 3, (50, 1)))).astype(np.float32)
        b[:, 32:64] *= np.float32(0.01)                             # a block that reaches the clamp
        pq, pb = fp4_ref.quantize(q), fp4_ref.quantize(b)
        got = fp4_ref.score(*pq, *pb, D)
        want = fp4_ref.dequantize(*pq, D) @ fp4_ref.dequantize(*pb, D).T
        assert got.dtype == np.float32 and (got.astype(np.float64) == want).all()


def test_rerank_recovers_the_exact_lists():
    """What tests/test_fp4_gpu.py's re-rank case rests on: with a shortlist of R = 4k from the fp4 scan, the k best of the
    shortlist by exact score ARE the k best of the database, for all 33 queries; at R = k they are not."""
    q, b = fp4_ref.rerank_sets()
    quant = fp4_ref.score(*fp4_ref.quantize(q), *fp4_ref.quantize(b), 200)
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
    assert lib.dir_index_fp4_max_dim() == 7281
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dir_last_error

    def quant(X=p, ldx=200, N=5, D=200, codes=p, ldc=128, exps=p, lde=8, scales=p):
        return lib.dir_quantize_rows_fp4(X, ldx, N, D, codes, ldc, exps, lde, scales, None)

    assert quant(D=0) == -1 and b'D < 1' in err()
    assert quant(D=7282, ldx=7282, ldc=3648, lde=232) == -1 and b'exceeds' in err()
    assert quant(ldc=100) == -1 and b'ldc' in err()               # D / 2, but below D rounded up to 64, halved
    assert quant(lde=7) == -1 and b'lde' in err()
    assert quant(ldx=199) == -1 and b'ldx' in err()
    assert quant(N=-1) == -1 and b'negative' in err()
    for name in ('X', 'codes', 'exps', 'scales'):
        assert quant(**{name: None}) == -1 and b'null' in err(), name
    assert quant(ldc=129) == -1 and b'ldc % 2' in err()
    assert quant(N=0, X=None, codes=None, exps=None, scales=None) == 0

    def sim(qc=p, ldq=128, qe=p, ldqe=8, qs=p, Q=3, bc=p, ldb=128, be=p, ldbe=8, bs=p, N=40, D=200, scores=p, lds=40):
        return lib.dir_similarity_fp4(qc, ldq, qe, ldqe, qs, Q, bc, ldb, be, ldbe, bs, N, D, scores, lds, None)

    assert sim(D=0) == -1 and b'D < 1' in err()
    assert sim(D=7282, ldq=3648, ldb=3648, ldqe=232, ldbe=232) == -1 and b'exceeds' in err()
    assert sim(ldq=99) == -1 and b'ldq' in err()
    assert sim(ldqe=6) == -1 and b'ldqe' in err()
    assert sim(ldb=112) == -1 and b'ldb' in err()
    assert sim(ldbe=7) == -1 and b'ldbe' in err()
    assert sim(lds=39) == -1 and b'lds' in err()
    assert sim(Q=-1) == -1 and sim(N=-1) == -1 and b'negative' in err()
    for name in ('qc', 'qe', 'qs', 'bc', 'be', 'bs', 'scores'):
        assert sim(**{name: None}) == -1 and b'null' in err(), name
    assert sim(ldb=136) == -1 and b'16' in err()                  # the scan moves 16-byte pieces
    assert sim(ldbe=12) == -1 and b'8' in err()                   # ... and reads the block bytes of a slab in one load
    assert sim(Q=0) == 0 and sim(N=0, lds=0) == 0                 # nothing to do: DIR_OK, nothing launched
    # launch limits (include/dir_engine.h): refused by name before anything is launched
    L = lib.dir_launch_max_threads()
    N = (L // 64 // 4 + 1) * 4                                    # one wave per row, four rows per workgroup
    assert quant(N=N) == -1 and b'quantize_rows_fp4: N * 64' in err()
    N = (L // 768 + 1) * 256                                      # 768 threads per 256 rows
    assert N < 1 << 31 and sim(N=N, lds=N) == -1 and b'similarity_fp4: N * 3' in err()
    assert sim(Q=65535 * 96 + 1) == -1 and b'65535 * 96' in err()


# ---- the emitted code of the scan --------------------------------------------------------------------------------------
def test_scan_kernel_runs_on_the_scaled_matrix_cores_without_scratch(tmp_path):
    """gfx950 assembly of csrc/index_fp4.hip: the scan multiplies on v_mfma_scale_f32_32x32x64_f8f6f4 with fp4 operands on
    both sides (twelve per K slab: four steps of 64 k x three query row blocks, op_sel walking the four scale bytes),
    spills nothing, stays within the registers of three waves per SIMD, and each hand-off barrier sits between the two
    scheduler fences of ring_barrier()."""
    import os
    import re
    import shutil
    import subprocess
    import pytest
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'index_fp4.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only',
                    os.path.join(root, 'deep-image-retrieval_amd', 'csrc', 'index_fp4.hip'), '-o', out], check=True,
                   capture_output=True)
    text = open(out).read()
    body = text[text.index('_ZN3dir14sim_fp4_kernel'):]
    body = body[:body.index('s_endpgm')]
    lines = [l.strip() for l in body.split('\n') if l.strip() and not l.strip().startswith('.')]
    mfma = [l for l in lines if l.startswith('v_mfma')]
    assert len(mfma) == 12 and all(l.startswith('v_mfma_scale_f32_32x32x64_f8f6f4') and 'cbsz:4 blgp:4' in l for l in mfma)
    barriers = [i for i, l in enumerate(lines) if l.startswith('s_barrier')]
    assert len(barriers) >= 2
    for i in barriers:
        assert lines[i - 1].startswith('; sched_barrier mask(0x00000000)') and lines[i + 1].startswith('; sched_barrier mask(0x00000000)')
    meta = text[text.index('amdhsa.kernels'):]
    meta = meta[meta.index('_ZN3dir14sim_fp4_kernel'):]
    assert int(re.search(r'\.private_segment_fixed_size:\s*(\d+)', meta).group(1)) == 0
    assert int(re.search(r'\.vgpr_count:\s*(\d+)', meta).group(1)) <= 168
