// diffusion_local.hip — truncated diffusion: every query solved on the subgraph of its T best database rows
// (dir_diffusion_subgraph, dir_diffusion_solve_local, dir_diffusion_spread).
//
// diffusion.hip runs conjugate gradients over all N rows for every query batch.  Iscen et al. restrict the system of a query
// to its T best rows; at T <= 2048 the vectors of one query fit a workgroup, so the whole solve is ONE launch: a workgroup
// per query, all iterations inside it, no global synchronisation and no workspace.  include/dir_engine.h states every number
// (the recurrence and the dot product are dir_diffusion_solve's with N := T); the numpy restatement is
// tests/diffusion_trunc_ref.py on top of tests/diffusion_ref.py.
//
// The local graph is slot-major, lidx / lw [Q][k][ldt]: lane a of a wave reads slot t of local row a, consecutive addresses
// across the lanes, and those reads do not depend on p, so the ids and weights of the next four slots are requested before
// the adds of the current four.  p is gathered from LDS; x, r and ap belong to the lane that owns the row and stay in its
// registers (two rows a lane at T > 512, one below), so LDS holds p and the products of a dot: 16 KiB.
#include "dir_common.h"
#include "diffusion_device.h"
#include "pointwise.h"

// products THEN sums, never a fused multiply-add (see expand_lists.hip)
#pragma clang fp contract(off)

namespace dir {

constexpr int kLocalMaxRows = 2048;    // T <= this: dir_topk_max_k(), checked in c_api.hip
constexpr int kLocalThreads = 1024;    // the largest workgroup of the three kernels
constexpr int kLocalHash = 4096;       // slots of the id table: twice the rows, so a probe always meets an empty slot
constexpr int kLocalUnroll = 4;        // slots requested ahead of the adds, per row
constexpr int kLocalTwoRows = 512;     // above this T a lane of the solve owns two rows
static_assert(kLocalHash >= 2 * kLocalMaxRows && (kLocalHash & (kLocalHash - 1)) == 0, "an open-addressed table, half empty");
static_assert(kLocalMaxRows <= 2 * kLocalThreads, "a lane owns at most two rows");
static_assert(kLocalMaxRows / kDiffSlab * kDiffChains <= kLocalThreads, "one lane per chain of every slab");

// ---- the subgraph ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned local_hash(int id) { return ((unsigned)id * 2654435761u) >> 20; }   // 12 bits

// the first slot of the list that holds `id`, -1 when none does
__device__ __forceinline__ int local_find(const int* keys, const int* first, int id) {
    unsigned h = local_hash(id);
    for (;;) {
        const int key = keys[h];
        if (key == id) return first[h];
        if (key == -1) return -1;
        h = (h + 1) & (kLocalHash - 1);
    }
}

// One workgroup per query.  The ids in [0, N) of the list go into an LDS table (linear probing; the place of a key depends
// on the order of the insertions, what is found under it does not: the minimum of the slots that hold it).  A slot is live
// when the table answers its own number.  Then T x k look-ups, lane = local row, so the stores are coalesced.
__global__ void __launch_bounds__(kLocalThreads) diffusion_subgraph_kernel(
        const int* __restrict__ idx, int ldl, const float* __restrict__ S, int lds, int N, int k, const int* __restrict__ cidx,
        const float* __restrict__ cvals, int ldc, int T, int kq, float gamma, int igamma, int one_hot, int* __restrict__ cid,
        int* __restrict__ lidx, float* __restrict__ lw, float* __restrict__ y, int ldt) {
    __shared__ int s_key[kLocalHash];
    __shared__ int s_first[kLocalHash];
    __shared__ int s_cid[kLocalMaxRows];
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t q = blockIdx.x;
    for (int h = tid; h < kLocalHash; h += nt) {
        s_key[h] = -1;
        s_first[h] = 0x7fffffff;
    }
    __syncthreads();
    for (int a = tid; a < T; a += nt) {
        const int id = cidx[q * ldc + a];
        if (id < 0 || id >= N) continue;
        unsigned h = local_hash(id);
        for (;;) {      // (at most T <= kLocalHash / 2 keys: an empty slot is always met)
            const int was = atomicCAS(&s_key[h], -1, id);
            if (was == -1 || was == id) break;
            h = (h + 1) & (kLocalHash - 1);
        }
        atomicMin(&s_first[h], a);
    }
    __syncthreads();
    for (int a = tid; a < T; a += nt) {
        const int id = cidx[q * ldc + a];
        const bool live = id >= 0 && id < N && local_find(s_key, s_first, id) == a;
        s_cid[a] = live ? id : -1;
        cid[q * ldt + a] = live ? id : -1;
        float seed = 0.f;
        if (one_hot) {
            seed = (a == 0 && live) ? 1.f : 0.f;
        } else if (a < kq && live) {
            const float v = cvals[q * ldc + a];
            if (v > 0.f) seed = diff_weight(v, gamma, igamma);
        }
        y[q * ldt + a] = seed;
    }
    __syncthreads();
    const int slots = T * k;      // <= 2048 * 2048
    for (int e = tid; e < slots; e += nt) {
        const int t = e / T, a = e - t * T;
        const int i = s_cid[a];
        int b = -1;
        float w = 0.f;
        if (i >= 0) {
            const float s = S[(size_t)i * lds + t];
            const int j = idx[(size_t)i * ldl + t];
            if (s != 0.f && j >= 0 && j < N) {
                b = local_find(s_key, s_first, j);      // a first slot is a live candidate
                w = b >= 0 ? s : 0.f;
            }
        }
        const size_t at = (q * k + t) * ldt + a;
        lidx[at] = b;
        lw[at] = w;
    }
}

int diffusion_subgraph(const int* idx, int ldl, const float* S, int lds, int N, int k, const int* cidx, const float* cvals, int ldc,
                       int Q, int T, int kq, float gamma, int one_hot, int* cid, int* lidx, float* lw, float* y, int ldt,
                       hipStream_t stream) {
    if (Q <= 0) return DIR_OK;
    if (!launch_fits(Q, kLocalThreads)) return fail(DIR_ERR_INVALID, "diffusion_subgraph: Q * 1024 must stay below 2^32 (a workgroup per query)");
    const int threads = T * (k > 0 ? k : 1) >= kLocalThreads ? kLocalThreads : 256;
    hipLaunchKernelGGL(diffusion_subgraph_kernel, dim3((unsigned)Q), dim3(threads), 0, stream, idx, ldl, S, lds, N, k, cidx, cvals, ldc,
                       T, kq, gamma, diff_igamma(gamma), one_hot, cid, lidx, lw, y, ldt);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- the solve -------------------------------------------------------------------------------------------------------
// dot of the products in s_prod[0 .. T), dir_diffusion_solve's order: lane c of wave s adds the rows of chain c of slab s,
// the 64 chains of a slab are one wave, so the tree is six shuffles (lane c takes chain[c] + chain[c + s]; the lanes
// at or past s carry values no lane below s reads afterwards); thread 0 then adds the slab partials in slab order and
// returns the dot - on thread 0 ONLY.  Every thread of the workgroup calls it.
__device__ __forceinline__ float local_dot(int T, const float* s_prod, float* s_part) {
    const int tid = threadIdx.x;
    const int slabs = (T + kDiffSlab - 1) / kDiffSlab;
    __syncthreads();                                     // the products are written
    if (tid < slabs * kDiffChains) {                     // whole waves: slabs * 64 <= blockDim.x
        const int base = (tid >> 6) * kDiffSlab + (tid & 63);
        float ch = 0.f;
#pragma unroll
        for (int m = 0; m < kDiffPer; ++m) {
            const int row = base + m * kDiffChains;
            if (row < T) ch = ch + s_prod[row];
        }
#pragma unroll
        for (int s = kDiffChains / 2; s > 0; s >>= 1) ch = ch + __shfl_down(ch, s, 64);
        if ((tid & 63) == 0) s_part[tid >> 6] = ch;
    }
    __syncthreads();
    float d = 0.f;
    if (tid == 0)
        for (int s = 0; s < slabs; ++s) d = d + s_part[s];
    return d;
}

// One workgroup per query, ROWS rows a lane (row = tid + h * blockDim.x), every iteration in this launch.
template <int ROWS>
__global__ void __launch_bounds__(kLocalThreads) diffusion_solve_local_kernel(
        const int* __restrict__ lidx, const float* __restrict__ lw, int k, const float* __restrict__ y, const int* __restrict__ cid,
        int ldt, int T, float alpha, int iters, float* __restrict__ f, int ldf) {
    __shared__ float s_p[kLocalMaxRows];
    __shared__ float s_prod[kLocalMaxRows];
    __shared__ float s_part[kLocalMaxRows / kDiffSlab];
    __shared__ float s_scal[2];
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t q = blockIdx.x;
    const int* li = lidx + q * k * ldt;
    const float* lv = lw + q * k * ldt;
    int row[ROWS], at[ROWS];
    bool there[ROWS];
    float x[ROWS], r[ROWS], p[ROWS], ap[ROWS];
#pragma unroll
    for (int h = 0; h < ROWS; ++h) {
        row[h] = tid + h * nt;
        there[h] = row[h] < T;
        at[h] = there[h] ? row[h] : 0;                   // an absent row reads row 0's tables (T >= 1) and adds nothing
        x[h] = 0.f;
        ap[h] = 0.f;
        r[h] = p[h] = there[h] ? y[q * ldt + row[h]] : 0.f;
        if (there[h]) {
            s_p[row[h]] = p[h];
            s_prod[row[h]] = r[h] * r[h];
        }
    }
    float rr = 0.f;
    if (iters > 0) {
        const float d = local_dot(T, s_prod, s_part);
        if (tid == 0) s_scal[1] = d;
        __syncthreads();
        rr = s_scal[1];
    }
    for (int it = 0; it < iters; ++it) {
        // g = the chain over the slots; the next four ids and weights are requested before these four adds
        float g[ROWS];
        int jn[ROWS][kLocalUnroll];
        float wn[ROWS][kLocalUnroll];
#pragma unroll
        for (int h = 0; h < ROWS; ++h) {
            g[h] = 0.f;
#pragma unroll
            for (int u = 0; u < kLocalUnroll; ++u) {
                jn[h][u] = u < k ? li[(size_t)u * ldt + at[h]] : -1;
                wn[h][u] = u < k ? lv[(size_t)u * ldt + at[h]] : 0.f;
            }
        }
        for (int t = 0; t < k; t += kLocalUnroll) {
            float w[ROWS][kLocalUnroll], v[ROWS][kLocalUnroll];
            bool on[ROWS][kLocalUnroll];
#pragma unroll
            for (int h = 0; h < ROWS; ++h) {
#pragma unroll
                for (int u = 0; u < kLocalUnroll; ++u) {
                    const int j = jn[h][u];
                    w[h][u] = wn[h][u];
                    on[h][u] = there[h] && j >= 0 && j < T && w[h][u] != 0.f;
                    v[h][u] = s_p[on[h][u] ? j : at[h]];      // a dead slot reads an address that is always valid
                }
            }
#pragma unroll
            for (int h = 0; h < ROWS; ++h) {
#pragma unroll
                for (int u = 0; u < kLocalUnroll; ++u) {
                    const int tn = t + kLocalUnroll + u;
                    jn[h][u] = tn < k ? li[(size_t)tn * ldt + at[h]] : -1;
                    wn[h][u] = tn < k ? lv[(size_t)tn * ldt + at[h]] : 0.f;
                }
            }
#pragma unroll
            for (int h = 0; h < ROWS; ++h) {
#pragma unroll
                for (int u = 0; u < kLocalUnroll; ++u) {
                    const float s = g[h] + w[h][u] * v[h][u];
                    g[h] = on[h][u] ? s : g[h];
                }
            }
        }
#pragma unroll
        for (int h = 0; h < ROWS; ++h) {
            if (there[h]) {
                ap[h] = p[h] - alpha * g[h];
                s_prod[row[h]] = p[h] * ap[h];
            }
        }
        const float pap = local_dot(T, s_prod, s_part);
        if (tid == 0) s_scal[0] = pap > 0.f ? rr / pap : 0.f;
        __syncthreads();
        const float a = s_scal[0];
#pragma unroll
        for (int h = 0; h < ROWS; ++h) {
            if (there[h]) {
                x[h] = x[h] + a * p[h];
                r[h] = r[h] - a * ap[h];
                s_prod[row[h]] = r[h] * r[h];
            }
        }
        const float rn = local_dot(T, s_prod, s_part);
        if (tid == 0) {
            s_scal[0] = rr > 0.f ? rn / rr : 0.f;
            s_scal[1] = rn;
        }
        __syncthreads();
        const float b = s_scal[0];
        rr = s_scal[1];
        if (it + 1 < iters) {      // (the direction after the last step is not used)
#pragma unroll
            for (int h = 0; h < ROWS; ++h) {
                if (there[h]) {
                    p[h] = r[h] + b * p[h];
                    s_p[row[h]] = p[h];
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int h = 0; h < ROWS; ++h) {
        if (there[h]) {
            // x first, then NaN over it for a dead candidate: two stores of one lane to one address, in program order.  (As one
            // select, hipcc 7 gave x and the NaN the same register in the two-row kernel and stored NaN for every row.)
            float* out = f + q * ldf + row[h];
            *out = x[h];
            if (cid && cid[q * ldt + row[h]] < 0) *out = __builtin_nanf("");
        }
    }
}

int diffusion_solve_local(const int* lidx, const float* lw, int k, const float* y, const int* cid, int ldt, int Q, int T, float alpha,
                          int iters, float* f, int ldf, hipStream_t stream) {
    if (Q <= 0) return DIR_OK;
    if (!launch_fits(Q, kLocalThreads)) return fail(DIR_ERR_INVALID, "diffusion_solve_local: Q * 1024 must stay below 2^32 (a workgroup per query)");
    const bool two = T > kLocalTwoRows;      // (two rows a lane: twice the loads in flight, half the waves at a barrier)
    const int threads = ((two ? (T + 1) / 2 : T) + 63) / 64 * 64;      // >= 64 * slabs either way: one lane per chain of a dot
    auto kern = two ? diffusion_solve_local_kernel<2> : diffusion_solve_local_kernel<1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)Q), dim3(threads), 0, stream, lidx, lw, k, y, cid, ldt, T, alpha, iters, f, ldf);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- the spread ------------------------------------------------------------------------------------------------------
// every score four lower: a cosine in [-1, 1] lands in [-5, -3], below every candidate's max(f, -2)
__global__ void __launch_bounds__(256) diffusion_shift_kernel(float* __restrict__ scores, int lds, int Q, int N) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)Q * N) return;
    float* s = scores + (e / N) * lds + e % N;
    *s = *s - 4.f;
}

// one thread per candidate: the live ones overwrite their column (the live ids of a query are distinct)
__global__ void __launch_bounds__(256) diffusion_place_kernel(float* __restrict__ scores, int lds, int Q, int N,
                                                              const int* __restrict__ cid, const float* __restrict__ f, int ldt, int T) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)Q * T) return;
    const size_t q = e / T, a = e % T;
    const int id = cid[q * ldt + a];
    if (id < 0 || id >= N) return;
    const float v = f[q * ldt + a];
    scores[q * lds + id] = v > -2.f ? v : -2.f;      // (a NaN fails the comparison: -2)
}

int diffusion_spread(float* scores, int lds, int Q, int N, const int* cid, const float* f, int ldt, int T, hipStream_t stream) {
    if (Q <= 0 || N <= 0) return DIR_OK;
    if (!launch_fits(((long)Q * N + 255) / 256, 256)) return fail(DIR_ERR_INVALID, "diffusion_spread: Q * N must stay below 2^32");
    if (!launch_fits(((long)Q * T + 255) / 256, 256)) return fail(DIR_ERR_INVALID, "diffusion_spread: Q * T must stay below 2^32");
    const size_t all = (size_t)Q * N, cand = (size_t)Q * T;
    hipLaunchKernelGGL(diffusion_shift_kernel, dim3((unsigned)((all + 255) / 256)), dim3(256), 0, stream, scores, lds, Q, N);
    if (T > 0)      // in stream order behind the shift, so the overwrite cannot race it
        hipLaunchKernelGGL(diffusion_place_kernel, dim3((unsigned)((cand + 255) / 256)), dim3(256), 0, stream, scores, lds, Q, N, cid, f,
                           ldt, T);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir
