// label_rank.hip — device-side ranking of class-labelled datasets (ImageListLabels / ImageListLabelsQ): the sklearn AP
// and the best rank of a same-class image, per query, without downloading or sorting a score row.
//
// The reference builds an N-long ground truth per query (dirtorch/datasets/dataset.py:70-101), calls
// sklearn.metrics.average_precision_score on the row (dirtorch/utils/evaluation.py:41-43) and argsorts it again for the
// top-k hits (dirtorch/test_dir.py:153-178).  Both quantities have order-free forms:
//     AP        = (1/n_pos) * sum over positives p of pos_ge(s_p) / all_ge(s_p)
//                 all_ge(t) = #{kept j : s_j >= t},  pos_ge(t) = #{kept positive j : s_j >= t}
//                 (kept = every image but the query itself; tied scores share one threshold, -0 == +0)
//     best_rank = #{j : j places before the best-placed image of the class} under np.argsort(-scores, kind='stable'):
//                 score descending, index ascending on ties, NaN after every number; the query itself is NOT left out
// One workgroup per query.  The class members' scores are sorted in LDS, 4096 at a time; the row is then read once per
// slice (coalesced), every kept score binary-searched into the sorted thresholds and added to two LDS histograms (all
// items, positives); their suffix sums are all_ge / pos_ge of every threshold of the slice.  Both depend on the
// threshold and the row only, so slices need no merge.  The terms are summed in fp64 in a fixed order (no floating-point
// atomics): two runs give the same bits.
#include "dir_common.h"
#include "pointwise.h"

#include <algorithm>

namespace dir {

constexpr int kLabelThreads = 512;
constexpr int kLabelSlice = 4096;            // thresholds per pass (keys + two histograms: 48 KiB of LDS)
constexpr uint32_t kLabelPad = 0xffffffffu;  // sorts behind every number: unused slots, the query itself, NaN members

// ascending with the score for every non-NaN float, never 0 or kLabelPad for one; -0 and +0 share a key
__device__ __forceinline__ uint32_t label_score_key(float s) {
    if (s == 0.f) s = 0.f;
    const uint32_t b = __builtin_bit_cast(uint32_t, s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ bool label_non_finite(float s) {
    return (__builtin_bit_cast(uint32_t, s) & 0x7f800000u) == 0x7f800000u;
}

// position under np.argsort(-scores, kind='stable'): a smaller key places earlier
__device__ __forceinline__ uint64_t label_place_key(float s, long idx) {
    const uint32_t d = s == s ? ~label_score_key(s) : kLabelPad;
    return ((uint64_t)d << 32) | (uint32_t)idx;
}

// The tables come from the caller's device memory: everything label_rank_kernel indexes with is checked here first, and
// so is what its counts rely on - class_members lists every database image exactly once, under the class labels gives it.
// result[0] = error bits (0 = valid), result[1] = the largest class, result[2 + j] = times image j is listed (zeroed).
__global__ void __launch_bounds__(256) label_check_kernel(const int* __restrict__ labels, const int* __restrict__ class_off,
                                                         const int* __restrict__ members, int C, int N,
                                                         const int* __restrict__ qclass, const int* __restrict__ qself,
                                                         int Q, int* __restrict__ result) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    int err = 0;
    if (i < C) {
        const int a = class_off[i], b = class_off[i + 1];
        if (a < 0 || b < a || b > N || (i == 0 && a != 0) || (i == C - 1 && b != N))
            err |= 1;
        else
            atomicMax(&result[1], b - a);
    }
    if (C == 0 && N > 0 && i == 0) err |= 1;       // no class, but images
    if (i < N && i < class_off[C]) {             // entry i of class_members: a database index of the class that owns i
        const int m = members[i];
        if (m < 0 || m >= N) {
            err |= 2;
        } else {
            const int c = labels[m];
            if (c < 0 || c >= C || i < class_off[c] || i >= class_off[c + 1]) err |= 4;
            if (atomicAdd(&result[2 + m], 1) != 0) err |= 32;   // listed twice (so another image is not listed at all)
        }
    }
    if (i < Q) {
        if (qclass[i] < -1 || qclass[i] >= C) err |= 8;
        if (qself[i] < -1 || qself[i] >= N) err |= 16;
    }
    if (err) atomicOr(&result[0], err);
}

// cap: power of two >= min(largest class, kLabelSlice); dynamic LDS = 12 * cap bytes
__global__ void __launch_bounds__(kLabelThreads) label_rank_kernel(const float* __restrict__ scores, int lds, int N,
                                                                  const int* __restrict__ labels,
                                                                  const int* __restrict__ class_off,
                                                                  const int* __restrict__ members,
                                                                  const int* __restrict__ qclass,
                                                                  const int* __restrict__ qself, int cap,
                                                                  double* __restrict__ ap_out,
                                                                  int* __restrict__ rank_out) {
    constexpr int T = kLabelThreads;
    extern __shared__ __attribute__((aligned(16))) char lsm[];
    uint32_t* keys = (uint32_t*)lsm;   // [cap] sorted thresholds of the slice
    int* hall = (int*)(keys + cap);    // [cap] bin k at k - 1 (bin 0 = below every threshold, never needed); then all_ge
    int* hpos = hall + cap;            // [cap] the same over the positives; then pos_ge
    __shared__ uint64_t red_key[T];
    __shared__ double red_sum[T];
    __shared__ int part_a[T], part_p[T];
    __shared__ int s_flag, s_before;
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int c = qclass[q];
    const int a0 = c < 0 ? 0 : class_off[c];
    const int nc = c < 0 ? 0 : class_off[c + 1] - a0;
    if (nc == 0) {                     // no database image of the query's class
        if (tid == 0) {
            ap_out[q] = -1.0;
            rank_out[q] = N;
        }
        return;
    }
    const int self = qself[q];
    const float* row = scores + (size_t)q * lds;
    const int n_pos = nc - ((self >= 0 && labels[self] == c) ? 1 : 0);

    // the best-placed image of the class: smallest place key over ALL its members
    uint64_t best = ~0ull;
    for (int i = tid; i < nc; i += T) {
        const int idx = members[a0 + i];
        const uint64_t k = label_place_key(row[idx], idx);
        best = k < best ? k : best;
    }
    red_key[tid] = best;
    if (tid == 0) s_flag = 0, s_before = 0;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (tid < s && red_key[tid + s] < red_key[tid]) red_key[tid] = red_key[tid + s];
        __syncthreads();
    }
    best = red_key[0];

    double acc = 0.0;
    int before = 0, bad = 0;
    for (int s0 = 0; s0 < nc; s0 += kLabelSlice) {
        const int P = nc - s0 < kLabelSlice ? nc - s0 : kLabelSlice;
        int p2 = 2;
        while (p2 < P) p2 <<= 1;       // <= cap
        for (int i = tid; i < p2; i += T) {
            uint32_t k = kLabelPad;
            if (i < P) {
                const int idx = members[a0 + s0 + i];
                const float s = row[idx];
                if (idx != self && s == s) k = label_score_key(s);
            }
            keys[i] = k;
            hall[i] = 0;
            hpos[i] = 0;
        }
        __syncthreads();
        for (int len = 2; len <= p2; len <<= 1)
            for (int st = len >> 1; st > 0; st >>= 1) {
                for (int i = tid; i < p2 / 2; i += T) {
                    const int lo = ((i / st) * st * 2) + (i % st), hi = lo + st;
                    const bool up = ((lo & len) == 0);
                    const uint32_t x = keys[lo], y = keys[hi];
                    if ((x > y) == up) keys[lo] = y, keys[hi] = x;
                }
                __syncthreads();
            }
        const uint32_t kmin = keys[0];
        const bool first = s0 == 0;
        constexpr int U = 4;
        for (long base = 0; base < N; base += T * U) {
            float v[U];
            int lab[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long j = base + u * T + tid;
                v[u] = j < N ? row[j] : 0.f;
                lab[u] = j < N ? labels[j] : -1;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long j = base + u * T + tid;
                if (j >= N) continue;
                if (first) before += label_place_key(v[u], j) < best;
                if (j == self) continue;                     // the query itself is not a kept item of the AP
                if (label_non_finite(v[u])) {                // sklearn refuses the row
                    bad = 1;
                    continue;
                }
                const uint32_t kj = label_score_key(v[u]);
                if (kj < kmin) continue;                     // below every threshold: bin 0
                int pos = 0;                                 // #{i : keys[i] <= kj} in a power-of-two table
                for (int st = p2 >> 1; st > 0; st >>= 1)
                    if (keys[pos + st - 1] <= kj) pos += st;
                if (pos < p2 && keys[pos] <= kj) ++pos;      // pos >= 1 here
                atomicAdd(&hall[pos - 1], 1);
                if (lab[u] == c) atomicAdd(&hpos[pos - 1], 1);
            }
        }
        __syncthreads();
        // suffix sums of both histograms: every thread owns `per` consecutive bins
        const int per = p2 >= T ? p2 / T : 1;
        const int b0 = tid * per;
        int sa = 0, sp = 0;
        if (b0 < p2)
            for (int i = 0; i < per; ++i) sa += hall[b0 + i], sp += hpos[b0 + i];
        part_a[tid] = sa;
        part_p[tid] = sp;
        __syncthreads();
        for (int d = 1; d < T; d <<= 1) {                    // inclusive suffix scan (Hillis-Steele)
            const int ya = tid + d < T ? part_a[tid + d] : 0;
            const int yp = tid + d < T ? part_p[tid + d] : 0;
            __syncthreads();
            part_a[tid] += ya;
            part_p[tid] += yp;
            __syncthreads();
        }
        int ra = tid + 1 < T ? part_a[tid + 1] : 0;
        int rp = tid + 1 < T ? part_p[tid + 1] : 0;
        if (b0 < p2)
            for (int i = per - 1; i >= 0; --i) {
                ra += hall[b0 + i];
                rp += hpos[b0 + i];
                hall[b0 + i] = ra;
                hpos[b0 + i] = rp;
            }
        __syncthreads();
        for (int i = tid; i < P; i += T)                     // the pads sort last: they take no term
            if (keys[i] != kLabelPad && hall[i] > 0) acc += (double)hpos[i] / (double)hall[i];
        __syncthreads();                                     // the next slice reuses the tables
    }
    red_sum[tid] = acc;
    if (before) atomicAdd(&s_before, before);
    if (bad) atomicOr(&s_flag, 1);
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (tid < s) red_sum[tid] += red_sum[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        ap_out[q] = n_pos == 0 ? -1.0 : (s_flag ? (double)NAN : red_sum[0] / (double)n_pos);
        rank_out[q] = s_before;
    }
}

int label_rank(const float* scores, int lds, int Q, int N, const int* labels, const int* class_off,
               const int* class_members, int C, const int* qclass, const int* qself, double* ap, int* best_rank,
               hipStream_t stream) {
    if (Q <= 0) return DIR_OK;
    if (lds < N) return fail(DIR_ERR_INVALID, "label_rank: lds < N");
    if (!launch_fits(Q, kLabelThreads))
        return fail(DIR_ERR_INVALID, "label_rank: Q * 512 must stay below 2^32 (one workgroup per query): cut the queries");
    int* result = nullptr;
    const size_t result_bytes = ((size_t)N + 2) * sizeof(int);
    if (hipMallocAsync((void**)&result, result_bytes, stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DIR_ERR_NOMEM, "label_rank: no stream-ordered scratch for the table check");
    }
    int host[2] = {0, 0};
    hipError_t e = hipMemsetAsync(result, 0, result_bytes, stream);
    if (e == hipSuccess) {
        const long n = std::max<long>(std::max<long>(N, C), std::max<long>(Q, 1));
        hipLaunchKernelGGL(label_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, labels, class_off,
                           class_members, C, N, qclass, qself, Q, result);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host, result, 2 * sizeof(int), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // the verdict decides whether the ranking may be launched
    const hipError_t fe = hipFreeAsync(result, stream);
    if (e == hipSuccess) e = fe;
    DIR_HIP_CHECK(e);
    if (host[0] & 1) return fail(DIR_ERR_INVALID, "label_rank: class_off is not a CSR that ends at N");
    if (host[0] & 2) return fail(DIR_ERR_INVALID, "label_rank: class_members entry outside [0, N)");
    if (host[0] & 4) return fail(DIR_ERR_INVALID, "label_rank: class_members disagrees with labels");
    if (host[0] & 32) return fail(DIR_ERR_INVALID, "label_rank: class_members lists an image twice");
    if (host[0] & 8) return fail(DIR_ERR_INVALID, "label_rank: qclass outside [-1, C)");
    if (host[0] & 16) return fail(DIR_ERR_INVALID, "label_rank: qself outside [-1, N)");
    int cap = 2;
    while (cap < host[1] && cap < kLabelSlice) cap <<= 1;
    hipLaunchKernelGGL(label_rank_kernel, dim3(Q), dim3(kLabelThreads), (size_t)cap * 12, stream, scores, lds, N, labels,
                       class_off, class_members, qclass, qself, cap, ap, best_rank);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir
