// expand_lists.hip — alpha query expansion / database augmentation from neighbour LISTS (dir_expand_lists).
//
// ranking.hip's expand_rows_kernel finds the k neighbours of a row itself, in a full row of the n x m score matrix.  Here
// the neighbours arrive as lists - dir_topk's (idx, vals), exact or from any of the index classes - and what is left is a
// gather: out[i] = normalize((descs[i] + sum_t vals[i][t]^alpha * db[idx[i][t]]) / (k + 1)), k + 1 rows of 4 D bytes read
// per output row and one written.  include/dir_engine.h states every number as a chain of single fp32 operations; the
// numpy restatement is tests/expand_ref.py.
//
// One workgroup of 256 threads per output row.  Lane tau owns columns 4 tau .. 4 tau + 3 of every span of 1024 columns, so
// with 16-byte aligned rows and D % 4 == 0 (VEC) a row of a span is one global_load_dwordx4 per lane; any other D or
// pitch reads the same four columns as scalars.  The (id, weight) pairs of a row are staged 256 at a time in LDS and read
// back as wave-uniform values.  The kernel is latency-bound (a dependent id -> row gather, no reuse), so the rows of four
// picks are requested before the first of them is added; the adds run in list order regardless.  An empty slot (id -1)
// reads the lane's own descs columns instead (a cached address that is always valid) and its add is dropped by a select,
// so the loop has no branch between the loads.
#include "dir_common.h"
#include "pointwise.h"

// The definition is in products THEN sums, never a fused multiply-add, and hipcc contracts by default: every product and
// sum below is a plain operator under this pragma (the __fmul_rn / __fadd_rn of the HIP headers are plain operators
// written OUTSIDE it, which the backend may still fuse after inlining; its __fsqrt_rn is the approximate square root).
#pragma clang fp contract(off)

namespace dir {

constexpr int kExpSpan = 1024;    // columns per span: 256 lanes x 4
constexpr int kExpPicks = 256;    // (id, weight) pairs staged per pass
constexpr int kExpUnroll = 4;     // rows requested ahead of the adds
constexpr int kExpRegSpans = 2;   // spans whose sums stay in registers until the norm is known (D <= 2048)

// w = v^alpha: alpha multiplications from 1 for an integer alpha in 0..64, powf otherwise
__device__ __forceinline__ float expand_weight(float v, float alpha, int ialpha) {
    if (ialpha < 0) return powf(v, alpha);
    float w = 1.f;
    for (int e = 0; e < ialpha; ++e) w = w * v;
    return w;
}

// columns d0 .. d0 + 3 of a row, zeros at and past D
template <bool VEC>
__device__ __forceinline__ f32x4_t expand_load4(const float* __restrict__ row, int d0, int D) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (VEC) {
        if (d0 < D) v = *(const f32x4_t*)(row + d0);      // D % 4 == 0: the four columns are inside or outside together
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (d0 + e < D) v[e] = row[d0 + e];
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void expand_store4(float* __restrict__ row, int d0, int D, f32x4_t v) {
    if constexpr (VEC) {
        if (d0 < D) *(f32x4_t*)(row + d0) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (d0 + e < D) row[d0 + e] = v[e];
    }
}

// The mean of span `span` of output row i in this lane's four columns: descs, then the picks in list order, then * inv.
// Every thread of the workgroup calls it (it stages the list in LDS behind barriers).
template <bool VEC>
__device__ __forceinline__ f32x4_t expand_span(const float* __restrict__ drow, const float* __restrict__ db, int ldb, int D,
                                               const int* __restrict__ irow, const float* __restrict__ vrow, int k,
                                               float alpha, int ialpha, float inv, int span, int* s_j, float* s_w) {
    const int tid = threadIdx.x;
    const int d0 = span * kExpSpan + 4 * tid;
    f32x4_t acc = expand_load4<VEC>(drow, d0, D);
    for (int t0 = 0; t0 < k; t0 += kExpPicks) {
        const int cnt = k - t0 < kExpPicks ? k - t0 : kExpPicks;
        if (t0 > 0 || span > 0) __syncthreads();           // the previous pass has been read
        if (tid < cnt) {
            const int j = irow[t0 + tid];
            s_j[tid] = j;
            s_w[tid] = j >= 0 ? expand_weight(vrow[t0 + tid], alpha, ialpha) : 0.f;   // the vals of an empty slot are not read
        }
        __syncthreads();
        for (int t = 0; t < cnt; t += kExpUnroll) {
            f32x4_t r[kExpUnroll];
            float w[kExpUnroll];
            bool on[kExpUnroll];
#pragma unroll
            for (int u = 0; u < kExpUnroll; ++u) {
                const int j = t + u < cnt ? __builtin_amdgcn_readfirstlane(s_j[t + u]) : -1;
                on[u] = j >= 0;
                w[u] = on[u] ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, s_w[t + u]))) : 0.f;
                r[u] = expand_load4<VEC>(on[u] ? db + (size_t)j * ldb : drow, d0, D);
            }
#pragma unroll
            for (int u = 0; u < kExpUnroll; ++u) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sum = acc[e] + r[u][e] * w[u];
                    acc[e] = on[u] ? sum : acc[e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] * inv;
    return acc;
}

// REG: D <= kExpRegSpans * 1024 and the means wait in registers for the norm; otherwise they wait in the output row, which
// the lane that wrote them reads back.
template <bool VEC, bool REG>
__global__ void __launch_bounds__(256) expand_lists_kernel(const float* __restrict__ descs, int ldd,
                                                          const float* __restrict__ db, int ldb, int D,
                                                          const int* __restrict__ idx, const float* __restrict__ vals,
                                                          int ldl, int k, float alpha, int ialpha, float inv,
                                                          float* __restrict__ out, int ldo) {
    __shared__ int s_j[kExpPicks];
    __shared__ float s_w[kExpPicks];
    __shared__ float s_red[256];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    const float* drow = descs + i * ldd;
    const int* irow = idx + i * ldl;
    const float* vrow = vals + i * ldl;
    float* orow = out + i * ldo;
    const int spans = (D + kExpSpan - 1) / kExpSpan;
    float p = 0.f;                                          // this lane's sum of squares, its columns in ascending order
    f32x4_t keep[kExpRegSpans];
    if constexpr (REG) {
#pragma unroll
        for (int s = 0; s < kExpRegSpans; ++s) {
            if (s < spans) {
                keep[s] = expand_span<VEC>(drow, db, ldb, D, irow, vrow, k, alpha, ialpha, inv, s, s_j, s_w);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (s * kExpSpan + 4 * tid + e < D) p = p + keep[s][e] * keep[s][e];
            }
        }
    } else {
        for (int s = 0; s < spans; ++s) {
            const f32x4_t a = expand_span<VEC>(drow, db, ldb, D, irow, vrow, k, alpha, ialpha, inv, s, s_j, s_w);
            expand_store4<VEC>(orow, s * kExpSpan + 4 * tid, D, a);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (s * kExpSpan + 4 * tid + e < D) p = p + a[e] * a[e];
        }
    }
    s_red[tid] = p;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] = s_red[tid] + s_red[tid + s];
        __syncthreads();
    }
    const float nrm = sqrtf(s_red[0]);      // (correctly rounded, as is the division: hipcc's default for fp32)
    if constexpr (REG) {
#pragma unroll
        for (int s = 0; s < kExpRegSpans; ++s) {
            if (s < spans) {
                f32x4_t a = keep[s];
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = a[e] / nrm;
                expand_store4<VEC>(orow, s * kExpSpan + 4 * tid, D, a);
            }
        }
    } else {
        for (int s = 0; s < spans; ++s) {
            f32x4_t a = expand_load4<VEC>(orow, s * kExpSpan + 4 * tid, D);   // this lane's own stores
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = a[e] / nrm;
            expand_store4<VEC>(orow, s * kExpSpan + 4 * tid, D, a);
        }
    }
}

int expand_lists(const float* descs, int ldd, int n, const float* db, int ldb, int D, const int* idx, const float* vals,
                 int ldl, int k, float alpha, float* out, int ldo, hipStream_t stream) {
    if (n <= 0) return DIR_OK;
    if (!launch_fits(n, 256)) return fail(DIR_ERR_INVALID, "expand_lists: n * 256 must stay below 2^32 (one workgroup per row): cut the rows");
    const int ia = (int)alpha;
    const int ialpha = ((float)ia == alpha && ia >= 0 && ia <= 64) ? ia : -1;
    const float inv = 1.f / (float)(k + 1);
    const auto aligned = [](const void* p, int ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; };
    const bool vec = D % 4 == 0 && aligned(descs, ldd) && aligned(db, ldb) && aligned(out, ldo);
    const bool reg = D <= kExpRegSpans * kExpSpan;
    auto kern = vec ? (reg ? expand_lists_kernel<true, true> : expand_lists_kernel<true, false>)
                    : (reg ? expand_lists_kernel<false, true> : expand_lists_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(256), 0, stream, descs, ldd, db, ldb, D, idx, vals, ldl, k, alpha, ialpha,
                       inv, out, ldo);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir
