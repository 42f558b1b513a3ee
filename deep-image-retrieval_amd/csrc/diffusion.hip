// diffusion.hip — diffusion re-ranking on the database's kNN graph (dir_knn_graph, dir_diffusion_seed, dir_diffusion_solve).
//
// The graph stays in the [N][k] layout of the neighbour lists it is made from: S[i][t] is the normalised mutual affinity of
// row i and row idx[i][t], +0 for a dead slot.  The solve is conjugate gradients on (I - alpha S) f = y for Q columns at
// once, a fixed number of iterations, everything enqueued on the caller's stream.  include/dir_engine.h states every
// number as a chain of single fp32 operations; the numpy restatement is tests/diffusion_ref.py.
//
// The vectors of the solve are row-major [N][Qp], Qp = Q rounded up to 4, the padding columns zero.  The hot kernel is
// the apply step: row i of S p needs rows idx[i][0 .. k) of p, a gather of k rows of 4 Qp bytes.  A lane owns four
// consecutive columns (one 16-byte load per gathered row) of the rows i = slab * 256 + chain + 64 m of one of the 64
// chains of a slab of 256 rows, so a wave carries several rows at once; a lane takes two of its rows at a time, the rows of
// four slots of each are requested before the first is added (eight gathers in flight), the ids and weights of the next
// four slots are requested before those adds, and the adds stay in slot order.  A dead slot reads the lane's own row of p (an address that is always
// valid) and its add is dropped by a select.  The kernel is latency- and request-bound, not bandwidth-bound.
//
// dot(u, v) of a column never depends on the launch: a slab is kDiffSlab = 256 consecutive rows, row r of it belongs to
// chain r mod 64, a chain adds its (up to four) products in ascending row order from +0, the 64 chains are added as a
// tree (s = 32, 16, 8, 4, 2, 1: chain[c] += chain[c + s]), and one thread per column adds the slab partials in ascending slab
// order from +0.  (A slab of 256 rows keeps that last, serial pass short at 10^6 rows: 3931 partials a column.)
#include "dir_common.h"
#include "diffusion_device.h"
#include "pointwise.h"

// products THEN sums, never a fused multiply-add (see expand_lists.hip)
#pragma clang fp contract(off)

namespace dir {

// (kDiffSlab = 256 rows per slab, kDiffChains = 64 chains, kDiffPer rows of a chain: diffusion_device.h)
static_assert(kDiffPer % 2 == 0, "a lane takes the rows of its chain two at a time");
constexpr int kDiffMaxCg = 16;     // column groups (of 4 columns) a workgroup covers: 64 columns
constexpr int kDiffUnroll = 4;     // gathered rows requested ahead of the adds, per row
constexpr int kDiffAhead = 64;     // slab partials the finishing thread of a column requests at a time
constexpr int kDiffPair = 2;       // rows of a chain a lane works on at a time
constexpr int kDiffThreads = 1024;  // the largest workgroup: 64 chains x 16 column groups
constexpr int kDiffFew = 256;       // threads of a workgroup that takes several slabs of a narrow solve

// (diff_weight, the power rule, and diff_igamma: diffusion_device.h)

// ---- the graph -------------------------------------------------------------------------------------------------------
// one thread per slot (i, t): its liveness, its weight, the first slot of row j that holds i, the minimum of the two weights
__global__ void __launch_bounds__(256) knn_affinity_kernel(const int* __restrict__ idx, const float* __restrict__ vals, int ldl,
                                                           int N, int k, float gamma, int igamma, float* __restrict__ S,
                                                           int lds) {
    const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (size_t)N * k) return;
    const int i = (int)(slot / k), t = (int)(slot % k);
    const int* irow = idx + (size_t)i * ldl;
    const int j = irow[t];
    const float v = vals[(size_t)i * ldl + t];
    bool live = j >= 0 && j < N && j != i && v > 0.f;
    for (int e = 0; live && e < t; ++e) live = irow[e] != j;
    float a = 0.f;
    if (live) {
        const int* jrow = idx + (size_t)j * ldl;
        int back = -1;
        for (int e = 0; e < k && back < 0; ++e)
            if (jrow[e] == i) back = e;            // the first slot that holds i: the only one that can be live
        if (back >= 0) {
            const float vb = vals[(size_t)j * ldl + back];
            if (vb > 0.f) {
                const float w = diff_weight(v, gamma, igamma), wb = diff_weight(vb, gamma, igamma);
                a = wb < w ? wb : w;
            }
        }
    }
    S[(size_t)i * lds + t] = a;
}

// one thread per row: deg = the chain over its slots, dinv = 1 / sqrtf(deg) (two correctly rounded operations)
__global__ void __launch_bounds__(256) knn_degree_kernel(const float* __restrict__ S, int lds, int N, int k,
                                                         float* __restrict__ dinv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float deg = 0.f;
    for (int t = 0; t < k; ++t) deg = deg + S[(size_t)i * lds + t];
    dinv[i] = deg > 0.f ? 1.f / sqrtf(deg) : 0.f;
}

// one thread per slot: S = a * (dinv[i] * dinv[j]); a slot of affinity 0 stays +0 and its id is not dereferenced
__global__ void __launch_bounds__(256) knn_normalise_kernel(const int* __restrict__ idx, int ldl, int N, int k,
                                                            const float* __restrict__ dinv, float* __restrict__ S, int lds) {
    const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (size_t)N * k) return;
    const int i = (int)(slot / k), t = (int)(slot % k);
    const float a = S[(size_t)i * lds + t];
    if (!(a != 0.f)) return;                       // (a NaN cannot occur: a is a minimum of powers of positive numbers)
    const int j = idx[(size_t)i * ldl + t];        // live, so 0 <= j < N
    const float d = dinv[i] * dinv[j];
    S[(size_t)i * lds + t] = a * d;
}

int knn_graph(const int* idx, const float* vals, int ldl, int N, int k, float gamma, float* S, int lds, hipStream_t stream) {
    if (N <= 0 || k <= 0) return DIR_OK;
    if (!launch_fits(((long)N * k + 255) / 256, 256)) return fail(DIR_ERR_INVALID, "knn_graph: N * k must stay below 2^32 (one thread per slot)");
    float* dinv = nullptr;
    DIR_HIP_CHECK(hipMallocAsync((void**)&dinv, (size_t)N * sizeof(float), stream));   // stream-ordered: freed after the kernels
    const size_t slots = (size_t)N * k;
    const unsigned gs = (unsigned)((slots + 255) / 256), gr = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(knn_affinity_kernel, dim3(gs), dim3(256), 0, stream, idx, vals, ldl, N, k, gamma, diff_igamma(gamma), S, lds);
    hipLaunchKernelGGL(knn_degree_kernel, dim3(gr), dim3(256), 0, stream, (const float*)S, lds, N, k, dinv);
    hipLaunchKernelGGL(knn_normalise_kernel, dim3(gs), dim3(256), 0, stream, idx, ldl, N, k, (const float*)dinv, S, lds);
    const hipError_t le = hipGetLastError();
    const hipError_t fe = hipFreeAsync(dinv, stream);
    DIR_HIP_CHECK(le);
    DIR_HIP_CHECK(fe);
    return DIR_OK;
}

// ---- the seeds -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) diffusion_zero_kernel(float* __restrict__ Y, int ldy, int N, int Q) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * Q) return;
    Y[(e / Q) * ldy + e % Q] = 0.f;
}

// one thread per query walks its list in slot order, so a later slot that names the same row overwrites an earlier one
__global__ void __launch_bounds__(64) diffusion_seed_kernel(const int* __restrict__ qidx, const float* __restrict__ qvals,
                                                            int ldq, int Q, int kq, int N, float gamma, int igamma,
                                                            float* __restrict__ Y, int ldy) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= Q) return;
    for (int t = 0; t < kq; ++t) {
        const int j = qidx[(size_t)q * ldq + t];
        const float v = qvals[(size_t)q * ldq + t];
        if (j >= 0 && j < N && v > 0.f) Y[(size_t)j * ldy + q] = diff_weight(v, gamma, igamma);
    }
}

int diffusion_seed(const int* qidx, const float* qvals, int ldq, int Q, int kq, int N, float gamma, float* Y, int ldy,
                   hipStream_t stream) {
    if (N <= 0 || Q <= 0) return DIR_OK;
    if (!launch_fits(((long)N * Q + 255) / 256, 256)) return fail(DIR_ERR_INVALID, "diffusion_seed: N * Q must stay below 2^32");
    const size_t elems = (size_t)N * Q;
    hipLaunchKernelGGL(diffusion_zero_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, stream, Y, ldy, N, Q);
    if (kq > 0)
        hipLaunchKernelGGL(diffusion_seed_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, stream, qidx, qvals, ldq, Q, kq, N,
                           gamma, diff_igamma(gamma), Y, ldy);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- the solve -------------------------------------------------------------------------------------------------------
int diffusion_slab_rows() { return kDiffSlab; }

static inline int diff_qp(int Q) { return (Q + 3) / 4 * 4; }
static inline size_t diff_slabs(int N) { return ((size_t)N + kDiffSlab - 1) / kDiffSlab; }

// x, r, p, ap [N][Qp]; the slab partials [slabs][Qp]; rr, a, b [Qp] - every region a multiple of 16 bytes
size_t diffusion_workspace_bytes(int N, int Q) {
    if (N <= 0 || Q <= 0) return 0;
    const size_t qp = (size_t)diff_qp(Q);
    return (4 * (size_t)N * qp + diff_slabs(N) * qp + 3 * qp) * sizeof(float);
}

// How a workgroup is cut: cg column groups x 64 chains x spb slabs (spb > 1 only while that stays within 256 threads; the
// column groups spread evenly over the fewest workgroups of at most 16).  Nothing here enters a result: a thread owns whole
// chains of whole slabs and the tree joins the chains of one slab.
struct DiffCut {
    int cg;        // column groups of this launch's workgroups (<= 16)
    int spb;       // slabs per workgroup
    int threads;   // active threads rounded up to whole waves
    dim3 grid;
};

static DiffCut diff_cut(int N, int Qp) {
    DiffCut c;
    const int ncg = Qp / 4;
    const int across = (ncg + kDiffMaxCg - 1) / kDiffMaxCg;
    c.cg = (ncg + across - 1) / across;
    c.spb = kDiffFew / (kDiffChains * c.cg) > 1 ? kDiffFew / (kDiffChains * c.cg) : 1;
    c.threads = (c.spb * kDiffChains * c.cg + 63) / 64 * 64;
    c.grid = dim3((unsigned)((diff_slabs(N) + c.spb - 1) / c.spb), (unsigned)((ncg + c.cg - 1) / c.cg));
    return c;
}

// the place of a thread in the cut; `on` is false for a thread without columns or slab
struct DiffPlace {
    bool on;
    int col;         // the first of the thread's four columns
    int chain;
    size_t row0;     // first row of the thread's slab
    size_t slab;
};

__device__ __forceinline__ DiffPlace diff_place(int cg, int spb, int N, int Qp) {
    const int tid = threadIdx.x;
    DiffPlace p;
    const int sl = tid / (kDiffChains * cg);
    p.chain = (tid / cg) % kDiffChains;
    p.col = (blockIdx.y * cg + tid % cg) * 4;
    p.slab = (size_t)blockIdx.x * spb + sl;
    p.row0 = p.slab * kDiffSlab;
    p.on = sl < spb && p.col < Qp && p.row0 < (size_t)N;
    return p;
}

// the tree over the 64 chains of a slab and the store of its partial; every thread of the workgroup calls it
__device__ __forceinline__ void diff_slab_partial(f32x4_t sum, const DiffPlace& pl, int cg, float* __restrict__ part, int Qp,
                                                  f32x4_t* s_red) {
    const int tid = threadIdx.x;
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    s_red[tid] = pl.on ? sum : zero;
    __syncthreads();
    for (int s = kDiffChains / 2; s > 0; s >>= 1) {
        if (pl.on && pl.chain < s) {
            const f32x4_t o = s_red[tid + s * cg];
            f32x4_t m = s_red[tid];
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = m[e] + o[e];
            s_red[tid] = m;
        }
        __syncthreads();
    }
    if (pl.on && pl.chain == 0) *(f32x4_t*)(part + pl.slab * Qp + pl.col) = s_red[tid];
}

// x = 0, r = p = y (padding columns zero), the slab partials of dot(r, r)
__global__ void __launch_bounds__(kDiffThreads) diffusion_init_kernel(const float* __restrict__ Y, int ldy, int N, int Q, int Qp,
                                                                      int cg, int spb, float* __restrict__ x,
                                                                      float* __restrict__ r, float* __restrict__ p,
                                                                      float* __restrict__ part) {
    __shared__ f32x4_t s_red[kDiffThreads];
    const DiffPlace pl = diff_place(cg, spb, N, Qp);
    f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
    if (pl.on) {
        for (int m = 0; m < kDiffPer; ++m) {
            const size_t i = pl.row0 + pl.chain + (size_t)m * kDiffChains;
            if (i >= (size_t)N) break;
            f32x4_t y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (pl.col + e < Q) y[e] = Y[i * ldy + pl.col + e];
            const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
            *(f32x4_t*)(x + i * Qp + pl.col) = zero;
            *(f32x4_t*)(r + i * Qp + pl.col) = y;
            *(f32x4_t*)(p + i * Qp + pl.col) = y;
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] = sum[e] + y[e] * y[e];
        }
    }
    diff_slab_partial(sum, pl, cg, part, Qp, s_red);
}

// ap = p - alpha * (S p), the slab partials of dot(p, ap)
__global__ void __launch_bounds__(kDiffThreads) diffusion_apply_kernel(const int* __restrict__ idx, int ldl,
                                                                       const float* __restrict__ S, int lds, int N, int k,
                                                                       int Qp, int cg, int spb, float alpha,
                                                                       const float* __restrict__ p, float* __restrict__ ap,
                                                                       float* __restrict__ part) {
    __shared__ f32x4_t s_red[kDiffThreads];
    const DiffPlace pl = diff_place(cg, spb, N, Qp);
    f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
    if (pl.on) {
        // the rows of a chain go two at a time: 2 x 4 gathered rows in flight, the ids and weights of the next four slots
        // requested before the adds of these; the chain still adds row by row
        for (int m = 0; m < kDiffPer; m += kDiffPair) {
            const size_t i0 = pl.row0 + pl.chain + (size_t)m * kDiffChains;
            if (i0 >= (size_t)N) break;
            bool there[kDiffPair];
            const int* irow[kDiffPair];
            const float* srow[kDiffPair];
            const float* own[kDiffPair];
            f32x4_t g[kDiffPair];
            int jn[kDiffPair][kDiffUnroll];
            float wn[kDiffPair][kDiffUnroll];
#pragma unroll
            for (int h = 0; h < kDiffPair; ++h) {
                const size_t i = i0 + (size_t)h * kDiffChains;
                there[h] = m + h < kDiffPer && i < (size_t)N;
                const size_t at = there[h] ? i : i0;                 // an absent row reads row i0's tables and adds nothing
                irow[h] = idx + at * ldl;
                srow[h] = S + at * lds;
                own[h] = p + at * Qp + pl.col;
                g[h] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < kDiffUnroll; ++u) {
                    jn[h][u] = u < k ? irow[h][u] : -1;
                    wn[h][u] = u < k ? srow[h][u] : 0.f;
                }
            }
            for (int t = 0; t < k; t += kDiffUnroll) {
                f32x4_t row[kDiffPair][kDiffUnroll];
                float w[kDiffPair][kDiffUnroll];
                bool on[kDiffPair][kDiffUnroll];
#pragma unroll
                for (int h = 0; h < kDiffPair; ++h) {
#pragma unroll
                    for (int u = 0; u < kDiffUnroll; ++u) {
                        const int j = jn[h][u];
                        w[h][u] = wn[h][u];
                        on[h][u] = there[h] && j >= 0 && j < N && w[h][u] != 0.f;
                        row[h][u] = *(const f32x4_t*)(on[h][u] ? p + (size_t)j * Qp + pl.col : own[h]);
                    }
                }
#pragma unroll
                for (int h = 0; h < kDiffPair; ++h) {
#pragma unroll
                    for (int u = 0; u < kDiffUnroll; ++u) {
                        const int tn = t + kDiffUnroll + u;
                        jn[h][u] = tn < k ? irow[h][tn] : -1;
                        wn[h][u] = tn < k ? srow[h][tn] : 0.f;
                    }
                }
#pragma unroll
                for (int h = 0; h < kDiffPair; ++h) {
#pragma unroll
                    for (int u = 0; u < kDiffUnroll; ++u) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float s = g[h][e] + w[h][u] * row[h][u][e];
                            g[h][e] = on[h][u] ? s : g[h][e];
                        }
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < kDiffPair; ++h) {
                if (there[h]) {
                    const f32x4_t pi = *(const f32x4_t*)own[h];
                    f32x4_t a;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[e] = pi[e] - alpha * g[h][e];
                        sum[e] = sum[e] + pi[e] * a[e];
                    }
                    *(f32x4_t*)(ap + (i0 + (size_t)h * kDiffChains) * Qp + pl.col) = a;
                }
            }
        }
    }
    diff_slab_partial(sum, pl, cg, part, Qp, s_red);
}

// x = x + a p, r = r - a ap, the slab partials of dot(r, r)
__global__ void __launch_bounds__(kDiffThreads) diffusion_update_kernel(int N, int Qp, int cg, int spb,
                                                                        const float* __restrict__ a, const float* __restrict__ p,
                                                                        const float* __restrict__ ap, float* __restrict__ x,
                                                                        float* __restrict__ r, float* __restrict__ part) {
    __shared__ f32x4_t s_red[kDiffThreads];
    const DiffPlace pl = diff_place(cg, spb, N, Qp);
    f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
    if (pl.on) {
        const f32x4_t av = *(const f32x4_t*)(a + pl.col);
        const size_t first = (pl.row0 + pl.chain) * Qp + pl.col, step = (size_t)kDiffChains * Qp;
        f32x4_t pv[kDiffPer], apv[kDiffPer], xv[kDiffPer], rv[kDiffPer];
#pragma unroll
        for (int m = 0; m < kDiffPer; ++m) {      // the loads of the chain's rows first, then its sum row by row
            const bool in = pl.row0 + pl.chain + (size_t)m * kDiffChains < (size_t)N;
            const size_t at = in ? first + m * step : pl.row0 * Qp + pl.col;      // (an absent row re-reads the slab's first row, which exists, and stores nothing)
            pv[m] = *(const f32x4_t*)(p + at);
            apv[m] = *(const f32x4_t*)(ap + at);
            xv[m] = *(const f32x4_t*)(x + at);
            rv[m] = *(const f32x4_t*)(r + at);
        }
#pragma unroll
        for (int m = 0; m < kDiffPer; ++m) {
            if (pl.row0 + pl.chain + (size_t)m * kDiffChains < (size_t)N) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xv[m][e] = xv[m][e] + av[e] * pv[m][e];
                    rv[m][e] = rv[m][e] - av[e] * apv[m][e];
                    sum[e] = sum[e] + rv[m][e] * rv[m][e];
                }
                *(f32x4_t*)(x + first + m * step) = xv[m];
                *(f32x4_t*)(r + first + m * step) = rv[m];
            }
        }
    }
    diff_slab_partial(sum, pl, cg, part, Qp, s_red);
}

// p = r + b p
__global__ void __launch_bounds__(256) diffusion_direction_kernel(size_t quads, int Qp, const float* __restrict__ b,
                                                                  const float* __restrict__ r, float* __restrict__ p) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= quads) return;
    const f32x4_t bv = *(const f32x4_t*)(b + (e * 4) % Qp);
    const f32x4_t rv = *(const f32x4_t*)(r + e * 4);
    f32x4_t pv = *(const f32x4_t*)(p + e * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) pv[c] = rv[c] + bv[c] * pv[c];
    *(f32x4_t*)(p + e * 4) = pv;
}

// One thread per column finishes a dot product: the slab partials in ascending slab order from +0.
// MODE 0: rr = dot.   MODE 1: a = dot > 0 ? rr / dot : 0.   MODE 2: b = rr > 0 ? dot / rr : 0, then rr = dot.
template <int MODE>
__global__ void __launch_bounds__(64) diffusion_finish_kernel(const float* __restrict__ part, size_t slabs, int Qp,
                                                              float* __restrict__ rr, float* __restrict__ out) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= Qp) return;
    float d = 0.f;
    for (size_t s0 = 0; s0 < slabs; s0 += kDiffAhead) {      // a batch of partials requested, then added in order
        float v[kDiffAhead];
#pragma unroll
        for (int u = 0; u < kDiffAhead; ++u) v[u] = s0 + u < slabs ? part[(s0 + u) * Qp + c] : 0.f;
#pragma unroll
        for (int u = 0; u < kDiffAhead; ++u)
            if (s0 + u < slabs) d = d + v[u];
    }
    if constexpr (MODE == 0) {
        rr[c] = d;
    } else if constexpr (MODE == 1) {
        out[c] = d > 0.f ? rr[c] / d : 0.f;
    } else {
        const float old = rr[c];
        out[c] = old > 0.f ? d / old : 0.f;
        rr[c] = d;
    }
}

// F[i][0 .. Q) = x[i][0 .. Q), or zeros without x
__global__ void __launch_bounds__(256) diffusion_result_kernel(const float* __restrict__ x, int Qp, int N, int Q,
                                                               float* __restrict__ F, int ldf) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * Q) return;
    const size_t i = e / Q, c = e % Q;
    F[i * ldf + c] = x ? x[i * Qp + c] : 0.f;
}

int diffusion_solve(const int* idx, int ldl, const float* S, int lds, int N, int k, const float* Y, int ldy, int Q, float alpha,
                    int iters, float* F, int ldf, void* workspace, hipStream_t stream) {
    if (N <= 0 || Q <= 0) return DIR_OK;
    if (!launch_fits(((long)N * Q + 255) / 256, 256)) return fail(DIR_ERR_INVALID, "diffusion_solve: N * Q must stay below 2^32");
    if (iters > 0 && Q > kMaxGridYZ * 4 * kDiffMaxCg)   // (diff_cut's grid.y: workgroups of 64 columns)
        return fail(DIR_ERR_INVALID, "diffusion_solve: more than 65535 * 64 columns in one call");
    const unsigned gres = (unsigned)(((size_t)N * Q + 255) / 256);
    if (iters <= 0) {
        hipLaunchKernelGGL(diffusion_result_kernel, dim3(gres), dim3(256), 0, stream, (const float*)nullptr, 0, N, Q, F, ldf);
        DIR_HIP_CHECK(hipGetLastError());
        return DIR_OK;
    }
    const int Qp = diff_qp(Q);
    const size_t slabs = diff_slabs(N), vec = (size_t)N * Qp;
    float* x = (float*)workspace;
    float* r = x + vec;
    float* p = r + vec;
    float* ap = p + vec;
    float* part = ap + vec;
    float* rr = part + slabs * Qp;
    float* a = rr + Qp;
    float* b = a + Qp;
    const DiffCut c = diff_cut(N, Qp);
    const dim3 gfin((unsigned)((Qp + 63) / 64));
    const size_t quads = vec / 4;
    hipLaunchKernelGGL(diffusion_init_kernel, c.grid, dim3(c.threads), 0, stream, Y, ldy, N, Q, Qp, c.cg, c.spb, x, r, p, part);
    hipLaunchKernelGGL(diffusion_finish_kernel<0>, gfin, dim3(64), 0, stream, (const float*)part, slabs, Qp, rr, (float*)nullptr);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(diffusion_apply_kernel, c.grid, dim3(c.threads), 0, stream, idx, ldl, S, lds, N, k, Qp, c.cg, c.spb, alpha,
                           (const float*)p, ap, part);
        hipLaunchKernelGGL(diffusion_finish_kernel<1>, gfin, dim3(64), 0, stream, (const float*)part, slabs, Qp, rr, a);
        hipLaunchKernelGGL(diffusion_update_kernel, c.grid, dim3(c.threads), 0, stream, N, Qp, c.cg, c.spb, (const float*)a,
                           (const float*)p, (const float*)ap, x, r, part);
        hipLaunchKernelGGL(diffusion_finish_kernel<2>, gfin, dim3(64), 0, stream, (const float*)part, slabs, Qp, rr, b);
        if (it + 1 < iters)      // (the direction after the last step is not used)
            hipLaunchKernelGGL(diffusion_direction_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, quads, Qp,
                               (const float*)b, (const float*)r, p);
    }
    hipLaunchKernelGGL(diffusion_result_kernel, dim3(gres), dim3(256), 0, stream, (const float*)x, Qp, N, Q, F, ldf);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir
