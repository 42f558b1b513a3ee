"""The launch-extent inventory: one row per (file, kernel) that a hipLaunchKernelGGL of the retrieval and pointwise sources
launches, with what keeps its grid expressible.

The rule (csrc/dir_common.h): a dispatch holds gridDim.x * blockDim.x as a 32-bit count of threads, so a launch stays within
dir_launch_max_threads() = 2^32 - 256 threads on x and within 65535 workgroups on y.  A row says how its launch obeys it:

  split    the launcher cuts the work into several launches (gather_scores only: its pairs are independent);
  refuse   the entry returns DIR_ERR_INVALID before anything is launched; `first(L)` gives the sizes of the first inadmissible
           call for a limit L (L = dir_launch_max_threads() for axis 'x', 65535 for axis 'y'), `vary` the size that one `step`
           lower is admissible again, `keyword` what the message must contain;
  bounded  another rule of the same entry already holds the extent below the limit: `why` is the one-line derivation.

`extent(**sizes)` is the launch's thread count on x (axis 'x') or its workgroup count on y (axis 'y') as the launcher
computes it.  A pair may have two rows, one per axis.  `sites` is the number of hipLaunchKernelGGL calls of the pair in the file.

tests/test_launch_limits_cpu.py requires this table to equal the launch sites it parses out of FILES, checks the formulas
at the edge and makes every refusal through the C ABI without a GPU.

Out of scope: the conv kernels (conv_*.hip, stem_*.hip) and engine.hip.  Their launches go through conv_launch under the
rule that an activation tensor of one engine call stays below 2^31 bytes, which tests/test_model_gpu.py tests."""
from collections import namedtuple

FILES = ('index_i8', 'index_fp4', 'index_bin', 'ivf', 'ivfpq', 'pq', 'topk', 'ranking', 'label_rank', 'expand_lists',
         'diffusion', 'pointwise', 'resize', 'gemm_f32', 'cov_f32', 'sim_split')

Y_LIMIT = 65535

Row = namedtuple('Row', 'file kernel sites entry kind axis extent first vary step keyword why')


def _up(n, m):
    return -(-n // m)


def split(file, kernel, sites, entry, extent, first, vary):
    return Row(file, kernel, sites, entry, 'split', 'x', extent, first, vary, 1, None, None)


def refuse(file, kernel, sites, entry, extent, first, vary, keyword, axis='x', step=1):
    return Row(file, kernel, sites, entry, 'refuse', axis, extent, first, vary, step, keyword, None)


def bounded(file, kernel, sites, entry, why):
    return Row(file, kernel, sites, entry, 'bounded', None, None, None, None, None, None, why)


ROWS = [
    # ---- index_i8.hip ---------------------------------------------------------------------------------------------------
    refuse('index_i8', 'quantize_rows_i8_kernel', 1, 'dir_quantize_rows_i8',
           lambda N, **_: _up(N, 4) * 256, lambda L: dict(N=4 * (L // 256) + 1), 'N', b'N * 64'),
    bounded('index_i8', 'code_image_kernel', 1, 'dir_similarity_i8',
            'x = ceil(pad64(D) / 128) * 256 <= 2^18 by D <= dir_index_i8_max_dim() = 131072; y = ceil(Q / 96), which the '
            'entry holds to 65535 before this launch (the sim_i8_kernel row)'),
    refuse('index_i8', 'sim_i8_kernel', 1, 'dir_similarity_i8',
           lambda N, **_: _up(N, 256) * 768, lambda L: dict(N=256 * (L // 768) + 1, Q=1), 'N', b'N * 3'),
    refuse('index_i8', 'sim_i8_kernel', 1, 'dir_similarity_i8',
           lambda Q, **_: _up(Q, 96), lambda L: dict(N=1, Q=96 * L + 1), 'Q', b'65535', axis='y'),
    split('index_i8', 'gather_scores_kernel', 1, 'dir_gather_scores',
          lambda Q, R, **_: _up(Q * R, 4) * 256, lambda L: dict(Q=4 * (L // 256) // 64 + 1, R=64), 'Q'),
    # ---- index_fp4.hip, index_bin.hip (their refusals are index_i8.hip's rows_launch and flat_scan_launch) --------------------
    refuse('index_fp4', 'quantize_rows_fp4_kernel', 1, 'dir_quantize_rows_fp4',
           lambda N, **_: _up(N, 4) * 256, lambda L: dict(N=4 * (L // 256) + 1), 'N', b'N * 64'),
    bounded('index_fp4', 'fp4_image_kernel', 1, 'dir_similarity_fp4',
            'x = ceil(pad64(D) / 256) * 256 <= 2^13 by D <= dir_index_fp4_max_dim() = 7281; y = ceil(Q / 96), which the '
            'entry holds to 65535 before this launch (the sim_fp4_kernel row)'),
    refuse('index_fp4', 'sim_fp4_kernel', 1, 'dir_similarity_fp4',
           lambda N, **_: _up(N, 256) * 768, lambda L: dict(N=256 * (L // 768) + 1, Q=1), 'N', b'N * 3'),
    refuse('index_fp4', 'sim_fp4_kernel', 1, 'dir_similarity_fp4',
           lambda Q, **_: _up(Q, 96), lambda L: dict(N=1, Q=96 * L + 1), 'Q', b'65535', axis='y'),
    refuse('index_bin', 'quantize_rows_bin_kernel', 1, 'dir_quantize_rows_bin',
           lambda N, **_: _up(N, 4) * 256, lambda L: dict(N=4 * (L // 256) + 1), 'N', b'N * 64'),
    refuse('index_bin', 'code_sums_kernel', 2, 'dir_code_sums',
           lambda Q, **_: _up(Q, 4) * 256, lambda L: dict(Q=4 * (L // 256) + 1), 'Q', b'Q * 64'),
    bounded('index_bin', 'code_sums_kernel', 2, 'dir_similarity_bin',
            'the scan-side site: x = ceil(Q / 96) * 24 * 256 <= 65535 * 6144 < 2^29, ceil(Q / 96) held to 65535 by the entry '
            'before this launch (the sim_bin_kernel row)'),
    refuse('index_bin', 'sim_bin_kernel', 1, 'dir_similarity_bin',
           lambda N, **_: _up(N, 256) * 768, lambda L: dict(N=256 * (L // 768) + 1, Q=1), 'N', b'N * 3'),
    refuse('index_bin', 'sim_bin_kernel', 1, 'dir_similarity_bin',
           lambda Q, **_: _up(Q, 96), lambda L: dict(N=1, Q=96 * L + 1), 'Q', b'65535', axis='y'),
    # ---- ivf.hip --------------------------------------------------------------------------------------------------------
    bounded('ivf', 'segment_sums_kernel', 1, 'dir_segment_sums', 'x = ceil(D / 256) * 256 <= 2^31 + 255 for an int D'),
    refuse('ivf', 'segment_sums_kernel', 1, 'dir_segment_sums',
           lambda S, **_: S, lambda L: dict(S=L + 1), 'S', b'65535', axis='y'),
    refuse('ivf', 'fill_ids_kernel', 1, 'dir_ivf_scan_i8',
           lambda Q, width, **_: _up(Q * width, 256) * 256, lambda L: dict(Q=65536, width=L // 65536 + 1, items=0), 'width',
           b'Q * width'),
    refuse('ivf', 'ivf_scan_i8_kernel', 1, 'dir_ivf_scan_i8',
           lambda items, **_: items * 768, lambda L: dict(Q=1, width=1, items=L // 768 + 1), 'items', b'items * 768'),
    # ---- ivfpq.hip (no id fill of its own: the scan writes the -1 of every empty column) -----------------------------------
    refuse('ivfpq', 'ivfpq_base_kernel', 1, 'dir_ivfpq_base',
           lambda Q, nprobe, **_: Q * nprobe * 128, lambda L: dict(Q=L // 128 + 1, nprobe=1), 'Q', b'Q * nprobe'),
    refuse('ivfpq', 'ivfpq_scan_kernel', 1, 'dir_ivfpq_scan',
           lambda Q, width, **_: Q * _up(width, 1024) * 1024, lambda L: dict(Q=L // 1024 + 1, width=1), 'Q', b'Q * width'),
    # ---- pq.hip ---------------------------------------------------------------------------------------------------------
    refuse('pq', 'pq_encode_kernel', 1, 'dir_pq_encode',
           lambda N, M, **_: _up(N, 256) * M * 256, lambda L: dict(N=256 * (L // 256 // 64) + 1, M=64), 'N', b'N * M'),
    refuse('pq', 'pq_lut_kernel', 1, 'dir_pq_lut',
           lambda Q, M, **_: _up(Q, 32) * M * 256, lambda L: dict(Q=32 * (L // 256 // 64) + 1, M=64), 'Q', b'Q * M'),
    bounded('pq', 'pq_scan_kernel', 1, 'dir_pq_scan',
            'x = ceil(N / (1024 * rows)) * 1024 <= N + 1023 < 2^31 + 2^10 for an int N; y = ceil(Q / qper) with qper >= '
            'ceil(Q / 65535) chosen by the launcher'),
    # ---- topk.hip -------------------------------------------------------------------------------------------------------
    bounded('topk', 'topk_select_kernel', 2, 'dir_topk',
            'x = ceil(N / 16384) * 512 <= 2^26 for an int N; y = the queries of a pass, cut to 65535 by the launcher\'s loop'),
    # ---- ranking.hip ----------------------------------------------------------------------------------------------------
    bounded('ranking', 'rank_sort_kernel', 1, 'dir_rank_counts',
            'x = Q * 256 < 2^24: the entry refuses Q > 65535 (the rank_hist_kernel row) before any launch'),
    refuse('ranking', 'rank_hist_kernel', 1, 'dir_rank_counts',
           lambda Q, **_: Q, lambda L: dict(Q=L + 1), 'Q', b'65535', axis='y'),
    bounded('ranking', 'rank_finalize_kernel', 1, 'dir_rank_counts', 'x = Q * 256 < 2^24, as rank_sort_kernel'),
    refuse('ranking', 'expand_rows_kernel', 1, 'dir_expand_descriptors',
           lambda n, **_: n * 256, lambda L: dict(n=L // 256 + 1), 'n', b'rows of a pass'),
    refuse('ranking', 'revisitop_ap_kernel', 1, 'dir_revisitop_ap',
           lambda Q, **_: Q * 256, lambda L: dict(Q=L // 256 + 1, modes=1), 'Q', b'Q * 256'),
    refuse('ranking', 'revisitop_ap_kernel', 1, 'dir_revisitop_ap',
           lambda modes, **_: modes, lambda L: dict(Q=1, modes=L + 1), 'modes', b'65535', axis='y'),
    # ---- label_rank.hip -------------------------------------------------------------------------------------------------
    bounded('label_rank', 'label_check_kernel', 1, 'dir_label_rank',
            'x = ceil(max(N, C, Q) / 256) * 256 <= 2^31 + 255 for int sizes'),
    refuse('label_rank', 'label_rank_kernel', 1, 'dir_label_rank',
           lambda Q, **_: Q * 512, lambda L: dict(Q=L // 512 + 1), 'Q', b'Q * 512'),
    # ---- expand_lists.hip -----------------------------------------------------------------------------------------------
    refuse('expand_lists', 'expand_lists_kernel', 1, 'dir_expand_lists',
           lambda n, **_: n * 256, lambda L: dict(n=L // 256 + 1), 'n', b'n * 256'),
    # ---- diffusion.hip --------------------------------------------------------------------------------------------------
    refuse('diffusion', 'knn_affinity_kernel', 1, 'dir_knn_graph',
           lambda N, k, **_: _up(N * k, 256) * 256, lambda L: dict(N=L // 2048 + 1, k=2048), 'N', b'N * k'),
    bounded('diffusion', 'knn_degree_kernel', 1, 'dir_knn_graph', 'x = ceil(N / 256) * 256 <= 2^31 + 255 for an int N'),
    bounded('diffusion', 'knn_normalise_kernel', 1, 'dir_knn_graph', 'the grid of knn_affinity_kernel, refused by the same check'),
    refuse('diffusion', 'diffusion_zero_kernel', 1, 'dir_diffusion_seed',
           lambda N, Q, **_: _up(N * Q, 256) * 256, lambda L: dict(N=L // 65536 + 1, Q=65536), 'N', b'N * Q'),
    bounded('diffusion', 'diffusion_seed_kernel', 1, 'dir_diffusion_seed', 'x = ceil(Q / 64) * 64 <= 2^31 + 63 for an int Q'),
    refuse('diffusion', 'diffusion_result_kernel', 2, 'dir_diffusion_solve',
           lambda N, Q, **_: _up(N * Q, 256) * 256, lambda L: dict(N=L // 65536 + 1, Q=65536, iters=0), 'N', b'N * Q'),
    bounded('diffusion', 'diffusion_init_kernel', 1, 'dir_diffusion_solve',
            'x = ceil(slabs / spb) * threads with threads <= 64 * cg * spb + 63 and cg <= ceil(Q / 4): at most N * Q / 4 + 2^10 '
            'under the N * Q check of the entry'),
    refuse('diffusion', 'diffusion_init_kernel', 1, 'dir_diffusion_solve',
           lambda Q, **_: _up(_up(Q, 4), 16), lambda L: dict(N=1, Q=64 * L + 1, iters=1), 'Q', b'65535', axis='y'),
    bounded('diffusion', 'diffusion_apply_kernel', 1, 'dir_diffusion_solve', 'the grid of diffusion_init_kernel'),
    bounded('diffusion', 'diffusion_update_kernel', 1, 'dir_diffusion_solve', 'the grid of diffusion_init_kernel'),
    bounded('diffusion', 'diffusion_finish_kernel', 3, 'dir_diffusion_solve',
            'x = ceil(Qp / 64) * 64 with Qp = Q rounded up to 4: <= 2^31 + 63 for an int Q'),
    bounded('diffusion', 'diffusion_direction_kernel', 1, 'dir_diffusion_solve',
            'x = N * Qp / 4 rounded up to 256: below N * Q + 256 under the N * Q check of the entry (Qp <= Q + 3 <= 4 Q)'),
    # ---- pointwise.hip --------------------------------------------------------------------------------------------------
    refuse('pointwise', 'prep_input_kernel', 1, 'dir_prep_input',
           lambda B, H, W, **_: _up(B * _up(H, 2) * _up(W, 2), 256) * 256, lambda L: dict(B=L // 4096 + 1, H=128, W=128), 'B',
           b'must stay below 2^32'),
    refuse('pointwise', 'maxpool_kernel', 2, 'dir_maxpool_3x3s2',
           lambda B, H, W, C, **_: _up(B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * (C // 8), 256) * 256,
           lambda L: dict(B=L // 4096 + 1, H=127, W=127, C=8), 'B', b'must stay below 2^32'),
    refuse('pointwise', 'global_pool_kernel', 1, 'dir_global_pool',
           lambda C, **_: C // 64 * 256, lambda L: dict(B=1, C=64 * (L // 256 + 1)), 'C', b'C * 4', step=64),
    refuse('pointwise', 'global_pool_kernel', 1, 'dir_global_pool',
           lambda B, **_: B, lambda L: dict(B=L + 1, C=64), 'B', b'65535', axis='y'),
    refuse('pointwise', 'upsample_add_kernel', 2, 'dir_upsample_add',
           lambda B, H, W, C, **_: _up(B * H * W * (C // 8), 256) * 256, lambda L: dict(B=L // 4096 + 1, H=64, W=64, C=8), 'B',
           b'must stay below 2^32'),
    refuse('pointwise', 'l2norm_rows_kernel', 1, 'dir_l2norm_rows',
           lambda rows, **_: rows * 256, lambda L: dict(rows=L // 256 + 1), 'rows', b'rows * 256'),
    refuse('pointwise', 'multiscale_pool_kernel', 1, 'dir_multiscale_pool',
           lambda N, D, **_: _up(N * D, 256) * 256, lambda L: dict(N=L // 65536 + 1, D=65536), 'N', b'N * D'),
    # ---- resize.hip -----------------------------------------------------------------------------------------------------
    bounded('resize', 'resample_coeffs_kernel', 2, 'dir_resize_bilinear_u8',
            'x = OW or OH rounded up to 256, launched only with the pass of that axis, whose B * H * OW * 3 or B * OH * OW * 3 '
            'the entry holds below the limit first'),
    refuse('resize', 'resample_pass_kernel', 2, 'dir_resize_bilinear_u8',
           lambda B, H, OW, **_: _up(B * H * OW * 3, 256) * 256, lambda L: dict(B=1, H=1, W=1, OH=1, OW=L // 3 + 1), 'OW',
           b'B * H * OW * 3'),
    refuse('resize', 'resample_pass_kernel', 2, 'dir_resize_bilinear_u8',
           lambda B, OH, OW, **_: _up(B * OH * OW * 3, 256) * 256, lambda L: dict(B=1, H=1, W=1, OH=L // 3 + 1, OW=1), 'OH',
           b'B * OH * OW * 3'),
    # ---- gemm_f32.hip ---------------------------------------------------------------------------------------------------
    refuse('gemm_f32', 'gemm_nt_small_kernel', 2, 'dir_gemm_nt_f32',
           lambda NP, **_: _up(NP, 8) * 256, lambda L: dict(NP=8 * (L // 256) + 1, NQ=1), 'NP', b'NP * 32'),
    refuse('gemm_f32', 'gemm_nt_f32_kernel', 1, 'dir_gemm_nt_f32',
           lambda NP, NQ, **_: _up(NP, 128) * _up(NQ, 32 * (4 if NQ >= 97 else 3 if NQ >= 65 else 2 if NQ >= 33 else 1)) * 256,
           lambda L: dict(NP=128 * (L // 256) + 1, NQ=33), 'NP', b'tiles * 256'),
    bounded('gemm_f32', 'gemm_splitk_finalize_kernel', 1, 'dir_gemm_nt_f32',
            'launched only with split-K, which gemm_splitk_factor grants below 128 output tiles of at most 128 x 128: '
            'x = NP * NQ rounded up to 256 <= 2^21'),
    # ---- cov_f32.hip ----------------------------------------------------------------------------------------------------
    bounded('cov_f32', 'cov_gram_kernel', 2, 'dir_cov_accumulate',
            'x = tiles * 256 with tiles <= 65535 ("D too large" otherwise); y = the row slices, capped by the launcher'),
    bounded('cov_f32', 'cov_reduce_kernel', 1, 'dir_cov_accumulate',
            'x = tiles * tile^2 + D rounded up to 256 with tiles <= 65535 tiles of 128 x 128: below 2^30 + 2^31'),
    # ---- sim_split.hip (internal: reached from dir_similarity* and dir_pca_whiten_l2_unit only where *_admissible says so;
    # a shape it turns away runs on gemm_nt_f32, whose own rows are above) -------------------------------------------------
    bounded('sim_split', 'split_queries_kernel', 3, 'dir_similarity',
            'x = K / 32 * 256 with K * 4 bytes of a row below 2^23; y = the query blocks, which similarity_split_admissible and '
            'whiten_split_admissible hold to 65535'),
    bounded('sim_split', 'whiten_split_kernel', 2, 'dir_pca_whiten_l2_unit',
            'whiten_split_admissible holds 8 * ceil(tiles / 8) * qblocks * 768 within the limit'),
    bounded('sim_split', 'sim_split_lc_kernel', 2, 'dir_similarity',
            'similarity_split_admissible holds ceil(NP / 256) * 768 within the limit and the query blocks on y to 65535'),
    bounded('sim_split', 'sim_split_kernel', 1, 'dir_similarity',
            '512 threads on the grid of sim_split_lc_kernel: below its extent'),
]
