// pointwise.h — launchers of the HBM-bound kernels (pointwise.hip) and the fp32 NT GEMM (gemm_f32.hip).
#pragma once
#include <vector>

#include "dir_common.h"

namespace dir {

int prep_input(const void* img, int fmt, const float* mean3, const float* std3, void* out, int B,
               int H, int W, int dtype, hipStream_t stream);
int maxpool_3x3s2(const void* x, void* y, int B, int H, int W, int C, int dtype, hipStream_t stream);
// out row b starts at out + b * ldo (the FPN heads pool two maps into one concatenated row)
int global_pool(const void* x, float* out, int ldo, int B, int H, int W, int C, int pooling, float p,
                float eps, float center_bias, int dtype, hipStream_t stream);
int upsample_add(const void* x, const void* low, void* y, int B, int H, int W, int h, int w, int C,
                 int dtype, hipStream_t stream, int* ovf = nullptr);
int l2norm_rows(float* x, int rows, int cols, float eps, hipStream_t stream);
size_t resize_workspace_bytes(int B, int H, int W, int OH, int OW);
int resize_bilinear_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int OH, int OW, void* ws,
                       size_t ws_bytes, hipStream_t stream);
int multiscale_pool(const float* x, float* out, int S, int N, int D, int mode, float gemp,
                    hipStream_t stream);
int stem_pool_launch(const void* s2d, const void* w, const float* bias, void* y, int B, int H2, int W2,
                     int OH, int OW, int dtype, hipStream_t stream, int* ovf = nullptr);
// the paired-fp16 forms of prep_input and of the stem (conv_pair.hip, DIR_FP16P): every tensor is two fp16 planes
int prep_input_pair(const void* img, int fmt, const float* mean3, const float* std3, void* out_hi, void* out_lo, int B,
                    int H, int W, hipStream_t stream);
int stem_pool_pair_launch(const void* s2d_hi, const void* s2d_lo, const void* w_hi, const void* w_lo, const float* bias,
                          void* y_hi, void* y_lo, int B, int H2, int W2, int OH, int OW, hipStream_t stream,
                          int* ovf = nullptr);
// DIR_FP16P on the raw uint8 feed (stem_u8.hip): one exact plane of u / 256, Normalize folded into the filter pair / bias / border table
int fold_stem_u8(const float* w, const float* scale, const float* bias, const float* mean3, const float* std3,
                 std::vector<uint16_t>& hi, std::vector<uint16_t>& lo, std::vector<float>& b2, std::vector<float>& corr);
int prep_input_u8(const void* img, void* out, int B, int H, int W, hipStream_t stream);
// img: the uint8 NHWC image (RAW form when stem_pool_u8_raw_ok: no prep launch, s2d may be null) or null (s2d = prep_input_u8's plane)
bool stem_pool_u8_raw_ok(const void* img, int B, int H, int W);
int stem_pool_u8_launch(const void* img, const void* s2d, const void* w_hi, const void* w_lo, const float* bias, const float* corr,
                        void* y_hi, void* y_lo, int B, int H, int W, hipStream_t stream, int* ovf = nullptr, int seg_tiles = 0);
// ... and the generic paired stem on the same kernel structure (stem_u8.hip XPAIR): what stem_pool_pair_launch runs by default
bool stem_pool_pair_raw_ok(const void* img_f32, int B, int H, int W);
int stem_pool_pair_walk_launch(const void* s2d_hi, const void* s2d_lo, const void* w_hi, const void* w_lo, const float* bias,
                               void* y_hi, void* y_lo, int B, int H2, int W2, int OH, int OW, hipStream_t stream, int* ovf = nullptr,
                               const void* img_f32 = nullptr, int H = 0, int W = 0);
int rank_counts(const float* scores, int lds, int Q, int N, const int* probe_idx, int P, int* counts,
                float* probe_scores, hipStream_t stream);
int revisitop_ap(const int* probe_idx, int Q, int P, const int* counts, const float* pscores, const int* pos_off,
                 const int* pos_list, const int* junk_off, const int* junk_list, int modes, double* terms,
                 double* ap_out, hipStream_t stream);
// class-labelled datasets (label_rank.hip): sklearn AP and the best rank of a same-class image, per query
int label_rank(const float* scores, int lds, int Q, int N, const int* labels, const int* class_off,
               const int* class_members, int C, const int* qclass, const int* qself, double* ap, int* best_rank,
               hipStream_t stream);
// ranked neighbour lists (topk.hip): the k best items of every row under the order rank_counts counts in
int topk_max_k();
size_t topk_workspace_bytes(int Q, int N, int k);
int topk(const float* scores, int lds, int Q, int N, int k, const int* ids, const int* exclude, int* out_idx,
         float* out_score, void* workspace, size_t workspace_bytes, hipStream_t stream);
// the int8 descriptor index (index_i8.hip): per-row codes + scales, the scan on the int8 matrix cores, the shortlist re-score
int index_i8_max_dim();
int quantize_rows_i8(const float* X, int ldx, int N, int D, int8_t* codes, int ldc, float* scales, hipStream_t stream);
bool similarity_i8_admissible(const int8_t* bcodes, int ldb, int D);
int similarity_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                  const float* bscales, int N, int D, float* scores, int lds, hipStream_t stream);
int gather_scores(const float* queries, int ldq, int Q, const float* database, int ldb, int D, const int* cand, int ldcand,
                  int R, float* scores, int ldsc, hipStream_t stream);
// the fp4 descriptor index (index_fp4.hip): e2m1 codes + e8m0 block bytes + row scales, the scan on the scaled matrix cores
int index_fp4_max_dim();
int quantize_rows_fp4(const float* X, int ldx, int N, int D, uint8_t* codes, int ldc, uint8_t* exps, int lde, float* scales,
                      hipStream_t stream);
bool similarity_fp4_admissible(const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, int D);
int similarity_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                   const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, int N, int D,
                   float* scores, int lds, hipStream_t stream);
// the binary descriptor index (index_bin.hip): sign bits + row scales, the scan on the int8 matrix cores against int8 queries
// (code_image: index_i8.hip's query image [qblocks][T][96][128], the launch of its code_image_kernel)
hipError_t code_image(const int8_t* qcodes, int ldq, int Q, int D, int8_t* img, int T, int qblocks, hipStream_t stream);
// ... and the admission rule of the database operand of the three flat scans (index_i8.hip): 16-byte pieces, one 2 GB
// descriptor per tile - the one condition of the binary index (their launchers are templates: flat_scan.h)
bool flat_scan_admissible(const void* rows, int ldb);
int index_bin_max_dim();
int quantize_rows_bin(const float* X, int ldx, int N, int D, uint8_t* bits, int ldb, float* scales, hipStream_t stream);
int similarity_bin(const int8_t* qcodes, int ldq, const float* qscales, int Q, const uint8_t* bits, int ldb,
                   const float* bscales, int N, int D, float* scores, int lds, hipStream_t stream);
// the inverted-file int8 index (ivf.hip): the sums of a k-means step, the scan of the probed lists
int segment_sums(const float* X, int ldx, int N, int D, const int* order, const int* seg_off, int S, float* sums, int lds,
                 hipStream_t stream);
// ... and what the three list-major scans share on the host: the admission rule of their code operands (16-byte pieces,
// one 2 GB descriptor each) and the step before their kernel (the two launch-extent refusals under the entry's name `who`,
// then id -1 in every slot)
bool ivf_scan_admissible(const void* qcodes, int ldq, int Q, const void* bcodes, int ldb);
int ivf_scan_begin(const char* who, long Q, int width, int items, int* out_ids, int lds, hipStream_t stream);
int ivf_scan_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                int lds, int width, hipStream_t stream);
// the inverted file over fp4 codes (ivf_fp4.hip): the list-major scan of the probed lists on the scaled matrix cores
bool ivf_scan_fp4_admissible(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, int Q, const uint8_t* bcodes,
                             int ldb, const uint8_t* bexps, int ldbe, int D);
int ivf_scan_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                 const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, const int* ids, int N,
                 int D, const int* list_off, int nlist, const int* pair_off, const int* pair_q, const int* pair_col,
                 const int* item_off, int items, float* scores, int* out_ids, int lds, int width, hipStream_t stream);
// the probe tables of both scans by list, made on the device in one launch (ivf_plan.hip)
int ivf_plan_max_pairs();
int ivf_plan(const int* probe, int Q, int nprobe, const int* list_off, int nlist, int* col_off, int* pair_off, int* pair_q,
             int* pair_col, int* item_off, int* counts, hipStream_t stream);
// the inverted file over sign-bit rows (ivf_bin.hip): the list-major scan of the probed lists on the int8 matrix cores;
// code_sums (index_bin.hip): the query sums it takes, the launch of code_sums_kernel
int code_sums(const int8_t* qcodes, int ldq, int Q, int D, int* qsums, hipStream_t stream);
int ivf_scan_bin(const int8_t* qcodes, int ldq, const float* qscales, const int* qsums, int Q, const uint8_t* bits, int ldb,
                 const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                 const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                 int lds, int width, hipStream_t stream);
// the product-quantised index (pq.hip): 8-bit codes per sub-space, the tables of a query, the scan that adds their entries
int pq_max_m();
int pq_encode(const float* X, int ldx, int N, int D, int M, const float* codebooks, uint8_t* codes, int ldc, hipStream_t stream);
int pq_lut(const float* queries, int ldq, int Q, int D, int M, const float* codebooks, float* lut, hipStream_t stream);
int pq_scan(const float* lut, int Q, int M, const uint8_t* codes, int ldc, int N, float* scores, int lds, hipStream_t stream);
// the IVF-PQ index (ivfpq.hip): the coarse terms of the probed lists, the query-major scan of their residual codes
int ivfpq_scan_cols();
int ivfpq_base(const float* queries, int ldq, int Q, const float* centroids, int ldc, int nlist, int D, int M, const int* probe,
               int nprobe, float* base, hipStream_t stream);
int ivfpq_scan(const float* lut, const float* base, int Q, int M, const uint8_t* codes, int ldc, const int* ids, int N,
               const int* list_off, int nlist, const int* probe, const int* col_off, int nprobe, float* scores, int* out_ids,
               int lds, int width, hipStream_t stream);
int expand_descriptors(const float* descs, int n, const float* db, int m, int D, int k, float alpha,
                       int self_set, float* out, float* sim, size_t sim_bytes, hipStream_t stream);
// the same expansion from neighbour lists (expand_lists.hip): a gather of k + 1 rows per output row, no score matrix
int expand_lists(const float* descs, int ldd, int n, const float* db, int ldb, int D, const int* idx, const float* vals,
                 int ldl, int k, float alpha, float* out, int ldo, hipStream_t stream);
// diffusion on the kNN graph of the database (diffusion.hip): the mutual, normalised graph in the list layout, the seed
// columns of a query set, conjugate gradients on (I - alpha S) F = Y for all columns at once
int knn_graph(const int* idx, const float* vals, int ldl, int N, int k, float gamma, float* S, int lds, hipStream_t stream);
int diffusion_seed(const int* qidx, const float* qvals, int ldq, int Q, int kq, int N, float gamma, float* Y, int ldy,
                   hipStream_t stream);
int diffusion_slab_rows();
size_t diffusion_workspace_bytes(int N, int Q);
int diffusion_solve(const int* idx, int ldl, const float* S, int lds, int N, int k, const float* Y, int ldy, int Q, float alpha,
                    int iters, float* F, int ldf, void* workspace, hipStream_t stream);
// truncated diffusion (diffusion_local.hip): the subgraph of every query's T best rows, its solve in one workgroup, and
// the spread of the list scores over a [Q][N] score row
int diffusion_subgraph(const int* idx, int ldl, const float* S, int lds, int N, int k, const int* cidx, const float* cvals, int ldc,
                       int Q, int T, int kq, float gamma, int one_hot, int* cid, int* lidx, float* lw, float* y, int ldt,
                       hipStream_t stream);
int diffusion_solve_local(const int* lidx, const float* lw, int k, const float* y, const int* cid, int ldt, int Q, int T, float alpha,
                          int iters, float* f, int ldf, hipStream_t stream);
int diffusion_spread(float* scores, int lds, int Q, int N, const int* cid, const float* f, int ldt, int T, hipStream_t stream);
// scratch (optional): fp32 workspace for the split-K partial sums of shapes with few output tiles; without one
// the partials live in stream-ordered memory (hipMallocAsync)
constexpr size_t kGemmSplitKMaxBytes = 64u << 20;
int gemm_splitk_factor(int NP, int NQ, int K);
int gemm_nt_f32(const float* P, int ldp, const float* Q, int ldq, float* out, int ldo, int NP,
                int NQ, int K, const float* qsub, const float* bias, const float* alpha,
                hipStream_t stream, float* scratch = nullptr, size_t scratch_bytes = 0);
// the N-dependent half of a PCA fit (cov_f32.hip): gram += (X - shift)^T (X - shift), sums += column sums, both fp64
int cov_chain_rows();
int cov_accumulate(const float* X, int ldx, int N, int D, const float* shift, double* gram, double* sums,
                   hipStream_t stream);
// large-database similarity on the bf16 matrix cores at fp32 accuracy (sim_split.hip)
size_t similarity_split_workspace_bytes(int NQ, int K);
bool similarity_split_admissible(const float* P, int ldp, const float* Q, int ldq, int NP, int NQ, int K);
// unit_range: operands known to lie in (-64, 64) (L2-normalised descriptors): two fp16 planes instead of three bf16 ones
int similarity_split(const float* P, int ldp, const float* Q, int ldq, float* out, int ldo, int NP, int NQ, int K,
                     void* workspace, size_t workspace_bytes, hipStream_t stream, bool unit_range = false);

// PCA whitening of a large descriptor set on two fp16 planes per operand (sim_split.hip): out[n][j] = alpha[j] <X[n] - mean, C[j]>
size_t whiten_split_workspace_bytes(int v, int K);
bool whiten_split_admissible(const float* X, int ldx, int N, int K, int v);
int whiten_split(const float* X, int ldx, int N, const float* comps, int ldc, int v, int K, const float* mean, const float* alpha,
                 float* out, int ldo, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace dir
