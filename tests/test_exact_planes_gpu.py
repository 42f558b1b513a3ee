"""The fp32 GEMM, similarity and whitening kernels (csrc/gemm_f32.hip, csrc/sim_split.hip) bit for bit, every element, on the
operands of tests/exact_planes.py: lattices on which the plane split is exact, the plane products the kernels drop are zero and
every partial sum fits 22 bits, so that the expected score is ONE fp32 number whatever the order, the K rotation, the accumulator
split, the split-K slicing or the sharding (tests/test_exact_planes_cpu.py holds the conditions on the inputs).  Every comparison
is torch.equal over all elements (+0 == -0); a failure reports the first differing (query row, database row) with its tile, strip
and blocks and the difference in units of the leg's resolution.

What is launched: ops.similarity (six-product default, the one-role kernel behind DIRTORCH_AMD_SIM_V1, the fp16 pair form, the
exact chain behind DIRTORCH_AMD_SIM_EXACT - all four against the same reference and each other), distributed.score_gathered /
merge_score_blocks against the un-sharded call, ops.gemm_nt on every shape of test_gemm_nt_f32 with and without qsub / alpha /
bias and through the C ABI on padded pitches, ops.pca_whiten with both roles sparse, with and without mean and alpha, and the
10^6-distractor size with every one of its 7 x 10^7 scores.

That the tests bite - arithmetic-only mutants of the kernels, built into a second library, against these tests and against the
tolerance tests that were there before (test_split_similarity_vs_fp64, test_pair_similarity_vs_fp64,
test_split_whitening_vs_fp64, test_gemm_nt_f32) - is recorded in the table at the end of this docstring.

Measured on the MI355X (share = differing elements of a failing case; "old" = the four tolerance tests named above):
  mutant                                                       old tests                         this file
  sim_split_lc_kernel<false> without l*h'                      split_similarity 3 of 4 shapes    six-1 all shapes, sharded, 10^6: 79-85 %
  ... without m*m'                                             split_similarity 4 of 4           six-4 all shapes, sharded: 87-91 %
  ... without l*h' in accumulator block j == 2 only            split_similarity 2 of 4           six-1, every shape with > 64 queries, 10^6: 7-28 %
  sim_split_lc_kernel<true> without l*h' in half-slab s == 1   pair_similarity 4 of 4            pair-1 all shapes, sharded, 10^6: 93-100 %
  whiten_split_kernel scalar store scaled by alpha[q]          all pass                          pca_whiten 33536x256x97, both roles: 74 %
  sim_split_kernel (DIRTORCH_AMD_SIM_V1) without h*l'          all pass (never launched)         six-2 all shapes: 79-85 %
  gemm_splitk_finalize_kernel starting at slice 1              gemm_nt_f32 7 of 7 split shapes   gemm_nt 7 of 7, large qsub, 2 pitch cases: 99.9 %
  gemm_nt_f32_kernel without "keep the K tail zero"            all pass                          all pass - the block is dead code: the
      gather zero-fills the K tail of P and of qsub as well, so 0 - qsub is 0 and multiplies a 0; no input can tell the two apart
(the old tests catch a product lost everywhere through "no worse than the exact chain + 1e-7" and the two planted scores of +-1;
they lose sight of it when it is lost in one block or in a kernel they do not launch).
"""
import pytest
import torch

import exact_planes as E

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _id(shape):
    return 'x'.join(str(v) for v in shape)


def _seed(*shape):
    return sum(v * (i + 3) for i, v in enumerate(shape)) % 100003


def _check(got, want, what, leg):
    E.report_mismatch(got, want, what, E.leg_resolution(leg))


def _similarity_paths(ops, monkeypatch, q, d, unit_range):
    """{path: scores} of every device path ops.similarity can take on these operands."""
    out = {'pair' if unit_range else 'six': ops.similarity(q, d, unit_range=unit_range)}
    if unit_range:
        out['six'] = ops.similarity(q, d)               # (a pair lattice has two bf16 planes per operand: exact there as well)
    monkeypatch.setenv('DIRTORCH_AMD_SIM_V1', '1')
    out['v1'] = ops.similarity(q, d, unit_range=unit_range)
    monkeypatch.delenv('DIRTORCH_AMD_SIM_V1')
    monkeypatch.setenv('DIRTORCH_AMD_SIM_EXACT', '1')
    out['exact'] = ops.similarity(q, d, unit_range=unit_range)
    monkeypatch.delenv('DIRTORCH_AMD_SIM_EXACT')
    return out


def _run_similarity(leg, shape, monkeypatch, unit_range):
    from dirtorch_amd import ops
    Q, N, D = shape
    assert N >= 32768 and D % 32 == 0                    # the split kernels' side of the dispatch
    seed = _seed(*shape)
    q, d = E.operands(leg, Q, N, D, DEV, seed)
    for shift in E.query_shifts(leg, Q, D):
        if shift:
            q = E.queries(leg, Q, D, DEV, seed, shift)
        want = E.reference(q, d)
        got = _similarity_paths(ops, monkeypatch, q, d, unit_range)
        for path, s in got.items():
            assert s.shape == (Q, N)
            _check(s, want, '%s %s shift %d, %s path vs fp64' % (leg, _id(shape), shift, path), leg)
        _check(got['v1'], got['six'], '%s %s: one-role kernel vs default' % (leg, _id(shape)), leg)


@pytest.mark.parametrize('shape', E.SIM_SHAPES, ids=_id)
@pytest.mark.parametrize('leg', E.SIX_LEGS)
def test_six_product_similarity(leg, shape, monkeypatch):
    """sim_split_lc_kernel<false>, sim_split_kernel (DIRTORCH_AMD_SIM_V1) and the exact chain: one number per score."""
    _run_similarity(leg, shape, monkeypatch, False)


@pytest.mark.parametrize('shape', E.SIM_SHAPES, ids=_id)
@pytest.mark.parametrize('leg', E.PAIR_LEGS)
def test_pair_similarity(leg, shape, monkeypatch):
    """sim_split_lc_kernel<true> (unit_range) next to the six-product kernels and the exact chain on the same operands."""
    _run_similarity(leg, shape, monkeypatch, True)


@pytest.mark.parametrize('leg', E.SHARD_LEGS)
@pytest.mark.parametrize('W', [2, 8])
def test_sharded_scoring_is_the_unsharded_call(W, leg):
    """The padded-block layout of test_sharded_scoring_with_unequal_shards: there the K walk of a row depends on where its tile
    sits and the scores agree to 5e-7; here every association gives the same number, so sharded == un-sharded == fp64."""
    from dirtorch_amd import distributed as dd
    from dirtorch_amd import ops
    Q, N, D = E.SHARD_SHAPE
    unit = E.LEGS[leg][0] == 'fp16'
    sim = (lambda a, b: ops.similarity(a, b, unit_range=True)) if unit else ops.similarity
    q, d = E.operands(leg, Q, N, D, DEV, _seed(Q, N, D, W))
    sizes, rows = dd.shard_sizes(N, W), dd.padded_rows(N, W)
    assert rows * W != N and min(h - l for l, h in sizes) >= 32768
    gathered = torch.zeros(W * rows, D, device=DEV)
    for r, (l, h) in enumerate(sizes):
        gathered[r * rows:r * rows + (h - l)] = d[l:h]
    s_desc = dd.score_gathered(q, gathered, N, W, sim)
    blocks = torch.stack([sim(q, gathered[r * rows:(r + 1) * rows]) for r in range(W)])
    s_score = dd.merge_score_blocks(blocks, N, W)
    del gathered, blocks
    s_one = sim(q, d)
    want = E.reference(q, d)
    _check(s_one, want, '%s un-sharded vs fp64' % leg, leg)
    _check(s_desc, s_one, '%s W = %d: score_gathered vs un-sharded' % (leg, W), leg)
    _check(s_score, s_one, '%s W = %d: merge_score_blocks vs un-sharded' % (leg, W), leg)


# ---- ops.gemm_nt -------------------------------------------------------------------------------------------------------------------
def _gemm_want(lat, P, alpha, bias):
    want = E.reference(lat, P).double()
    if alpha is not None:
        want = want * alpha.double()
    if bias is not None:
        want = want + bias.double()
    w32 = want.float()
    assert torch.equal(w32.double(), want)
    return w32


@pytest.mark.parametrize('shape', E.GEMM_SHAPES, ids=_id)
def test_gemm_nt(shape):
    """gemm_nt_f32_kernel<1..4>, its split-K form + finalize, the gather path (K = 1031) and gemm_nt_small_kernel<4> / <8>, with
    qsub / alpha / bias on the lattice in every combination the callers use, and without."""
    from dirtorch_amd import _lib, ops
    NP, NQ, K = shape
    slices = _lib.load().dir_gemm_splitk_factor(NP, NQ, K)
    assert (slices > 1) == (shape in E.GEMM_SPLIT), (shape, slices)
    seed = _seed(*shape)
    P, lat, _, _, _ = E.gemm_operands(NP, NQ, K, DEV, seed, False)
    got = ops.gemm_nt(P, lat)
    assert got.shape == (NQ, NP)
    _check(got, _gemm_want(lat, P, None, None), 'gemm %s plain' % _id(shape), 'gemm')
    P, lat, qsub, bias, alpha = E.gemm_operands(NP, NQ, K, DEV, seed, True)
    Q = lat + qsub
    for what, s, b, a in (('qsub + bias + alpha', qsub, bias, alpha), ('qsub', qsub, None, None), ('bias', None, bias, None),
                          ('qsub + alpha', qsub, None, alpha)):
        got = ops.gemm_nt(P, Q if s is not None else lat, s, b, a)
        _check(got, _gemm_want(lat, P, a, b), 'gemm %s %s' % (_id(shape), what), 'gemm-epi')


@pytest.mark.parametrize('shape', E.GEMM_BIG_QSUB, ids=_id)
def test_gemm_nt_k_tail_with_a_large_qsub(shape):
    """K % 4 != 0 with |qsub| a thousand times the lattice values: a zero-filled K tail that let `0 - qsub` through, on either
    operand, would be off by thousands of units."""
    from dirtorch_amd import ops
    NP, NQ, K = shape
    assert K % 4 != 0
    P, lat, qsub, bias, alpha = E.gemm_operands(NP, NQ, K, DEV, _seed(*shape), True, big_qsub=True)
    Q = lat + qsub
    assert torch.equal(Q - qsub, lat)
    _check(ops.gemm_nt(P, Q, qsub, bias, alpha), _gemm_want(lat, P, alpha, bias), 'gemm %s large qsub' % _id(shape), 'gemm-epi')
    _check(ops.gemm_nt(P, Q, qsub), _gemm_want(lat, P, None, None), 'gemm %s large qsub alone' % _id(shape), 'gemm-epi')


@pytest.mark.parametrize('shape,path', [((96, 40, 96), 'vector'), ((2048, 64, 2048), 'vector'), ((33, 7, 96), 'vector'),
                                        ((130, 70, 64), 'gather'), ((300, 70, 1031), 'gather')],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else v)
def test_gemm_nt_row_pitches(shape, path):
    """dir_gemm_nt_f32 takes ldp, ldq, ldo through the C ABI and ops.gemm_nt always passes K / NP: here P, Q and out are views of
    wider buffers (ldp = K + 4, ldq = K + 8, ldo = NP + 4: 16-byte loads and stores stay legal; ldp = K + 1, ldo = NP + 1: the
    element-wise gather and scalar stores), the padding filled with NaN: a read outside the logical rows poisons a score, a write
    outside them clears a NaN."""
    from dirtorch_amd._lib import call, ptr, stream_ptr
    NP, NQ, K = shape
    ldp, ldq, ldo = (K + 4, K + 8, NP + 4) if path == 'vector' else (K + 1, K + 8, NP + 1)
    P, lat, qsub, bias, alpha = E.gemm_operands(NP, NQ, K, DEV, _seed(*shape), True)
    nan = float('nan')
    Pb, Qb, out = (torch.full((NP, ldp), nan, device=DEV), torch.full((NQ, ldq), nan, device=DEV),
                   torch.full((NQ, ldo), nan, device=DEV))
    Pb[:, :K] = P
    Qb[:, :K] = lat + qsub
    call('dir_gemm_nt_f32', ptr(Pb), ldp, ptr(Qb), ldq, ptr(out), ldo, NP, NQ, K, ptr(qsub), ptr(bias), ptr(alpha), stream_ptr())
    _check(out[:, :NP].contiguous(), _gemm_want(lat, P, alpha, bias), 'gemm %s %s pitches' % (_id(shape), path), 'gemm-epi')
    assert bool(torch.isnan(out[:, NP:]).all()), 'a store landed in the padding of the output rows'
    assert bool(torch.isnan(Pb[:, K:]).all()) and bool(torch.isnan(Qb[:, K:]).all())


# ---- ops.pca_whiten ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', E.WHITEN_SHAPES, ids=_id)
@pytest.mark.parametrize('leg', E.WHITEN_LEGS)
def test_pca_whiten(leg, shape):
    """whiten_split_kernel<true / false> (vector and scalar stores, tile counts that are not a multiple of 8 with several component
    blocks) and the exact chain on the same data: X = lattice + a strong common mean, components in the queries' place; pair-2 =
    sparse components against dense X - mean, pair-1 = the transposed roles."""
    from dirtorch_amd import ops
    N, D, v = shape
    assert N >= 32768 and D % 32 == 0
    seed = _seed(*shape)
    comps, lat = E.operands(leg, v, N, D, DEV, seed, alphas=E.WHITEN_ALPHAS)
    prod = E.reference(lat, comps)                                        # [N, v]
    mean = E.lattice_mean(D, DEV, seed)
    X = lat + mean
    assert torch.equal(X - mean, lat)
    alpha = torch.tensor(E.WHITEN_ALPHAS, device=DEV)[torch.arange(v, device=DEV) % len(E.WHITEN_ALPHAS)].contiguous()
    scaled = prod * alpha
    assert torch.equal(scaled.double(), prod.double() * alpha.double())
    for use_mean in (True, False):
        for use_alpha in (True, False):
            want = scaled if use_alpha else prod
            for unit in (True, False):
                got = ops.pca_whiten(X if use_mean else lat, comps, mean if use_mean else None, alpha if use_alpha else None,
                                     unit_range=unit)
                assert got.shape == (N, v)
                _check(got.t(), want.t(), 'whiten %s %s mean %d alpha %d %s' % (leg, _id(shape), use_mean, use_alpha,
                                                                                  'two-plane' if unit else 'exact chain'), leg)


# ---- the 10^6-distractor size, every score --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('leg', E.BIG_LEGS)
def test_million_distractors_every_score(leg):
    """BASELINE config D's real dimensions (70 x 1 006 322 x 2048: rows beyond the 4 GB a buffer descriptor spans, 3 931 tiles),
    all 7 x 10^7 scores against the chunked device-fp64 reference.  (Lattice scores tie by the thousand, so nothing about AP is
    asserted here; test_million_distractors_ranking keeps its AP check on real-valued descriptors.)"""
    from dirtorch_amd import ops
    Q, N, D = E.BIG_SHAPE
    q, d = E.operands(leg, Q, N, D, DEV, _seed(Q, N, D))
    try:
        got = ops.similarity(q, d, unit_range=E.LEGS[leg][0] == 'fp16')
        want = E.reference(q, d)
        _check(got, want, '%s %s' % (leg, _id(E.BIG_SHAPE)), leg)
    finally:
        del d
        torch.cuda.empty_cache()
