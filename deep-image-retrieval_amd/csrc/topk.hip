// topk.hip — the k best database images of every query, ranked, without downloading or sorting a score row.
//
// The reference sorts every row of the Q x N score matrix on the host (np.argsort, dirtorch/datasets/generic.py:207-208)
// and picks neighbours with np.argpartition (dirtorch/test_dir.py:24-44).  Here a row is cut into slices of 16384 columns;
// one workgroup per (slice, query) reads its scores ONCE, keeps their order-preserving 32-bit keys (rank_key.h) in
// registers, 32 per thread, and radix-selects the slice's k best: three histogram passes over the key (11 + 11 + 10 bits)
// find the key of the k-th item, and, only when the cut falls inside a group of tied scores, three more over the ids of
// that group find the id of the k-th.  The survivors go to the workspace as (stored score bits, id) - a shorter row WITH
// an id table, i.e. the very input this kernel takes - so the same kernel reduces slices x k candidates again until one
// slice is left; that last launch sorts its k survivors in LDS (bitonic, 64-bit key = score key : id) and writes the lists.
//
// Order: item j ranks before item p when s_j > s_p, or s_j == s_p and id_j > id_p (the order dir_rank_counts counts
// in: np.argsort(row, kind='stable')[::-1]); -0 == +0; a NaN ranks after every number, -inf included, larger id first
// among NaNs.  In keys: a number has score_key_u32 >= 0x007fffff, a NaN gets 0x00200000, a column that takes no part
// (past N, id -1, the excluded id) gets 0 - it is never counted, so no selected digit prefix or threshold matches it.
// Ids are distinct within a row, so the 64-bit keys are, and "the k largest keys, in descending order" is ONE list: it
// does not depend on the slice size, the grid, the scheduling of workgroups or the order in which the LDS atomics below
// arrive - those only decide which histogram increment lands first and in which workspace slot a survivor waits, never
// which items survive or where they end up.
#include "dir_common.h"
#include "pointwise.h"
#include "rank_key.h"

#include <algorithm>

namespace dir {

constexpr int kTopkThreads = 512;
constexpr int kTopkSlice = 16384;        // columns per workgroup: 32 keys in the registers of every thread
constexpr int kTopkMaxK = 2048;          // the final sort's (key, column) table: 24 KiB
constexpr int kTopkBins = 2048;          // one histogram of 11-bit digits: 8 KiB
constexpr int kTopkMaxQ = 65535;         // queries per launch (gridDim.y)
constexpr uint32_t kKeyNaN = 1u << 21, kKeyOut = 0u;   // top digits 1 and 0; a number's top digit is >= 3

static_assert(kTopkMaxK <= kTopkSlice / 8, "every level must shrink its row");
static_assert(kTopkBins % kTopkThreads == 0, "every thread owns whole bins");
constexpr int kTopkItems = kTopkSlice / kTopkThreads;

__device__ __forceinline__ uint32_t topk_key(float s) { return s == s ? score_key_u32(s) : kKeyNaN; }

// The histogram of the top digit of every item that takes part.  Scores crowd into a few bins of that digit (one
// exponent), and 64 lanes adding to one LDS word are served one after the other: every wave takes the digits of the
// first two items of its first lane as leaders, a thread counts its items in the leaders' bins in registers and adds each
// count once; only the other items pay an atomic of their own.  Every lane calls it.
__device__ __forceinline__ void topk_count_top(int* hist, const uint32_t (&key)[kTopkItems]) {
    const uint32_t lead0 = __builtin_amdgcn_readfirstlane(key[0] >> 21), lead1 = __builtin_amdgcn_readfirstlane(key[1] >> 21);
    int cnt0 = 0, cnt1 = 0;
#pragma unroll
    for (int u = 0; u < kTopkItems; ++u) {
        const uint32_t b = key[u] >> 21;
        const bool on = key[u] != kKeyOut, is0 = b == lead0, is1 = b == lead1 && !is0;
        cnt0 += on && is0;
        cnt1 += on && is1;
        if (on && !is0 && !is1) atomicAdd(&hist[b], 1);
    }
    if (cnt0) atomicAdd(&hist[lead0], cnt0);
    if (cnt1) atomicAdd(&hist[lead1], cnt1);
}

// The bin that holds the want-th largest of the counted items, by suffix sums of hist (want is cut to their number):
// sel[0] = the bin, sel[1] = the item's position inside that bin (1-based, from the top), sel[2] = the bin's count;
// nothing is selected when nothing was counted.  Returns the number of counted items and leaves hist zeroed for the next
// pass.  Every thread calls it; wtot is [kTopkThreads / 64].
__device__ __forceinline__ int topk_pick_bin(int* hist, int want, int* wtot, int* sel) {
    constexpr int T = kTopkThreads, PER = kTopkBins / T, W = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c[PER], sum = 0;
#pragma unroll
    for (int b = 0; b < PER; ++b) c[b] = hist[tid * PER + b], sum += c[b];
    int incl = sum;                                        // inclusive suffix sum over the lanes of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_down(incl, d);
        if (lane + d < 64) incl += y;
    }
    if (lane == 0) wtot[wave] = incl;
    __syncthreads();
    int total = 0, above = incl - sum;                     // above = items in the bins of the threads after this one
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int t = wtot[w];
        total += t;
        if (w > wave) above += t;
    }
    want = want < total ? want : total;
#pragma unroll
    for (int b = PER - 1; b >= 0; --b) {
        if (above < want && above + c[b] >= want) {        // true for exactly one bin of the workgroup when want >= 1
            sel[0] = tid * PER + b;
            sel[1] = want - above;
            sel[2] = c[b];
        }
        above += c[b];
        hist[tid * PER + b] = 0;
    }
    __syncthreads();
    return total;
}

// One workgroup per (slice = blockIdx.x, query = blockIdx.y).  scores / ids: rows of pitch lds, N columns in use; ids
// NULL = the column is the id.  Not FINAL: the slice's best min(k, kept) items go to slots [slice * k, slice * k + k) of
// row q of cand_score / cand_id (pitch cand_ld), the rest of the k slots is (NaN, -1).  FINAL (one slice: N <= kTopkSlice):
// the row's list goes to out_idx / out_score [q][k], sorted, padded with (-1, NaN); p2 = power of two >= max(k, 2).
// Dynamic LDS: kTopkBins * 4 (+ p2 * 12 when FINAL) bytes.
template <bool FINAL>
__global__ void __launch_bounds__(kTopkThreads, 4) topk_select_kernel(const float* __restrict__ scores, int lds, int N, int k,
                                                                  const int* __restrict__ ids,
                                                                  const int* __restrict__ exclude,
                                                                  float* __restrict__ cand_score, int* __restrict__ cand_id,
                                                                  int cand_ld, int p2, int* __restrict__ out_idx,
                                                                  float* __restrict__ out_score) {
    constexpr int T = kTopkThreads, S = kTopkSlice, ITEMS = kTopkItems;
    extern __shared__ __attribute__((aligned(16))) char tsm[];
    int* hist = (int*)tsm;                                 // [kTopkBins]
    uint64_t* skey = (uint64_t*)(tsm + (size_t)kTopkBins * 4);   // FINAL: [p2] score key : id
    int* scol = (int*)(skey + (FINAL ? p2 : 0));           // FINAL: [p2] the survivor's column
    __shared__ int wtot[T / 64];
    __shared__ int sel[3];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int q = blockIdx.y;
    const int c0 = blockIdx.x * S;
    const int len = N - c0 < S ? N - c0 : S;               // >= 1: the grid has ceil(N / S) slices
    const float* row = scores + (size_t)q * lds + c0;
    const int* idrow = ids ? ids + (size_t)q * lds + c0 : nullptr;
    const int ex = exclude ? exclude[q] : -1;
    const auto id_of = [&](int i) { return idrow ? idrow[i] : c0 + i; };   // column u * T + tid of the slice is item u

    for (int i = tid; i < kTopkBins; i += T) hist[i] = 0;
    if (tid == 0) s_count = 0;
    // the one pass over HBM: the keys of the thread's columns, all loads in flight together
    uint32_t key[ITEMS];
#pragma unroll
    for (int h = 0; h < ITEMS; h += ITEMS / 2) {           // (two halves: 16 loads in flight per thread, 128 VGPRs in all)
        float v[ITEMS / 2];
        int id[ITEMS / 2];
#pragma unroll
        for (int u = 0; u < ITEMS / 2; ++u) {
            const int i = (h + u) * T + tid;
            v[u] = i < len ? row[i] : 0.f;
            id[u] = i < len ? id_of(i) : -1;
        }
#pragma unroll
        for (int u = 0; u < ITEMS / 2; ++u) key[h + u] = (id[u] >= 0 && id[u] != ex) ? topk_key(v[u]) : kKeyOut;
    }
    __syncthreads();
    topk_count_top(hist, key);
    __syncthreads();

    // kept = items that take part; kk = how many of them survive
    const int kept = topk_pick_bin(hist, k, wtot, sel);
    const int kk = kept < k ? kept : k;

    uint32_t tkey = 0xffffffffu;   // the survivors: key > tkey, or key == tkey and id >= tid_min
    int tid_min = 0;
    if (kk > 0) {                  // (uniform over the workgroup)
        const uint32_t d1 = (uint32_t)sel[0];
        int want = sel[1];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < ITEMS; ++u)                    // (d1 >= 1: a column that takes no part never matches)
            if ((key[u] >> 21) == d1) atomicAdd(&hist[(key[u] >> 10) & 0x7ffu], 1);
        __syncthreads();
        topk_pick_bin(hist, want, wtot, sel);
        const uint32_t d2 = (d1 << 11) | (uint32_t)sel[0];
        want = sel[1];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < ITEMS; ++u)
            if ((key[u] >> 10) == d2) atomicAdd(&hist[key[u] & 0x3ffu], 1);
        __syncthreads();
        topk_pick_bin(hist, want, wtot, sel);
        tkey = (d2 << 10) | (uint32_t)sel[0];
        want = sel[1];
        const int tied = sel[2];
        __syncthreads();
        if (want < tied) {         // the cut falls inside the group of items that share tkey: the `want` largest ids of it
#pragma unroll 1
            for (int u = 0; u < ITEMS; ++u)
                if (key[u] == tkey) atomicAdd(&hist[(uint32_t)id_of(u * T + tid) >> 20], 1);
            __syncthreads();
            topk_pick_bin(hist, want, wtot, sel);
            const uint32_t e1 = (uint32_t)sel[0];
            want = sel[1];
            __syncthreads();
#pragma unroll 1
            for (int u = 0; u < ITEMS; ++u)
                if (key[u] == tkey) {
                    const uint32_t id = (uint32_t)id_of(u * T + tid);
                    if ((id >> 20) == e1) atomicAdd(&hist[(id >> 10) & 0x3ffu], 1);
                }
            __syncthreads();
            topk_pick_bin(hist, want, wtot, sel);
            const uint32_t e2 = (e1 << 10) | (uint32_t)sel[0];
            want = sel[1];
            __syncthreads();
#pragma unroll 1
            for (int u = 0; u < ITEMS; ++u)
                if (key[u] == tkey) {
                    const uint32_t id = (uint32_t)id_of(u * T + tid);
                    if ((id >> 10) == e2) atomicAdd(&hist[id & 0x3ffu], 1);
                }
            __syncthreads();
            topk_pick_bin(hist, want, wtot, sel);
            tid_min = (int)((e2 << 10) | (uint32_t)sel[0]);
            __syncthreads();
        }
    }

    // the survivors take a slot each; which one depends on arrival, what happens to them afterwards does not.  A row
    // whose ids repeat (the caller's fault) can offer more than k: the slot check drops the excess instead of writing
    // past the table.
    float* cs = FINAL ? nullptr : cand_score + (size_t)q * cand_ld + (size_t)blockIdx.x * k;
    int* ci = FINAL ? nullptr : cand_id + (size_t)q * cand_ld + (size_t)blockIdx.x * k;
    if (kk > 0) {
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) {
            if (key[u] < tkey) continue;                   // (tkey >= kKeyNaN > kKeyOut)
            const int i = u * T + tid;
            const int id = id_of(i);
            if (key[u] == tkey && id < tid_min) continue;
            const int slot = atomicAdd(&s_count, 1);
            if (slot >= k) continue;
            if (FINAL) {
                skey[slot] = ((uint64_t)key[u] << 32) | (uint32_t)id;
                scol[slot] = i;
            } else {
                cs[slot] = row[i];
                ci[slot] = id;
            }
        }
    }
    __syncthreads();
    const int filled = s_count < k ? s_count : k;
    if (!FINAL) {
        for (int j = filled + tid; j < k; j += T) {
            cs[j] = NAN;
            ci[j] = -1;
        }
        return;
    }
    for (int j = filled + tid; j < p2; j += T) {
        skey[j] = 0;               // below every survivor's key (their score key is >= 1)
        scol[j] = 0;
    }
    __syncthreads();
    for (int n = 2; n <= p2; n <<= 1)      // bitonic sort, descending
        for (int st = n >> 1; st > 0; st >>= 1) {
            for (int i = tid; i < p2 / 2; i += T) {
                const int lo = ((i / st) * st * 2) + (i % st), hi = lo + st;
                const bool down = ((lo & n) == 0);
                const uint64_t a = skey[lo], b = skey[hi];
                if ((a < b) == down) {
                    const int ca = scol[lo], cb = scol[hi];
                    skey[lo] = b, skey[hi] = a;
                    scol[lo] = cb, scol[hi] = ca;
                }
            }
            __syncthreads();
        }
    for (int j = tid; j < k; j += T) {
        const bool real = j < filled;
        out_idx[(size_t)q * k + j] = real ? (int)(uint32_t)skey[j] : -1;
        out_score[(size_t)q * k + j] = real ? row[scol[j]] : NAN;   // the stored bits: -0, a NaN's payload
    }
}

// the rows of every level after the first: level[0] = slices(N) * k candidates, level[i + 1] = slices(level[i]) * k
static int topk_levels(int N, int k, long level[8]) {
    int n = 0;
    long cur = N;
    while (cur > kTopkSlice && n < 8) {
        cur = ((cur + kTopkSlice - 1) / kTopkSlice) * k;
        level[n++] = cur;
    }
    return n;
}

static size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

int topk_max_k() { return kTopkMaxK; }

// two ping-pong buffers of (score, id) planes: levels 0, 2, .. live in the first, levels 1, 3, .. in the second
size_t topk_workspace_bytes(int Q, int N, int k) {
    if (Q <= 0 || N <= 0 || k <= 0) return 0;
    long level[8];
    const int n = topk_levels(N, k, level);
    const size_t rows = (size_t)std::min(Q, kTopkMaxQ);
    size_t bytes = 0;
    if (n > 0) bytes += 2 * round256(rows * (size_t)level[0] * 4);
    if (n > 1) bytes += 2 * round256(rows * (size_t)level[1] * 4);
    return bytes;
}

int topk(const float* scores, int lds, int Q, int N, int k, const int* ids, const int* exclude, int* out_idx,
         float* out_score, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (Q <= 0) return DIR_OK;
    long level[8];
    const int nlev = topk_levels(N, k, level);
    if (nlev > 0 && level[nlev - 1] > kTopkSlice) return fail(DIR_ERR_INVALID, "topk: row too long");   // (N < 2^31: never)
    const size_t rows = (size_t)std::min(Q, kTopkMaxQ);
    char* buf[2] = {(char*)workspace, (char*)workspace + (nlev > 0 ? 2 * round256(rows * (size_t)level[0] * 4) : 0)};
    size_t plane[2] = {nlev > 0 ? round256(rows * (size_t)level[0] * 4) : 0, nlev > 1 ? round256(rows * (size_t)level[1] * 4) : 0};
    int p2 = 2;
    while (p2 < k) p2 <<= 1;
    const size_t lds_sel = (size_t)kTopkBins * 4, lds_fin = lds_sel + (size_t)p2 * 12;
    for (int q0 = 0; q0 < Q; q0 += kTopkMaxQ) {
        const int nq = Q - q0 < kTopkMaxQ ? Q - q0 : kTopkMaxQ;
        const float* cur_s = scores + (size_t)q0 * lds;
        const int* cur_id = ids ? ids + (size_t)q0 * lds : nullptr;
        const int* cur_ex = exclude ? exclude + q0 : nullptr;
        int cur_ld = lds, cur_n = N;
        for (int l = 0; l < nlev; ++l) {
            const int slices = (cur_n + kTopkSlice - 1) / kTopkSlice;
            float* os = (float*)buf[l & 1];
            int* oi = (int*)(buf[l & 1] + plane[l & 1]);
            hipLaunchKernelGGL(topk_select_kernel<false>, dim3(slices, nq), dim3(kTopkThreads), lds_sel, stream, cur_s, cur_ld,
                               cur_n, k, cur_id, cur_ex, os, oi, (int)level[l], 0, (int*)nullptr, (float*)nullptr);
            DIR_HIP_CHECK(hipGetLastError());
            cur_s = os, cur_id = oi, cur_ex = nullptr;
            cur_ld = cur_n = (int)level[l];
        }
        hipLaunchKernelGGL(topk_select_kernel<true>, dim3(1, nq), dim3(kTopkThreads), lds_fin, stream, cur_s, cur_ld, cur_n, k,
                           cur_id, cur_ex, (float*)nullptr, (int*)nullptr, 0, p2, out_idx + (size_t)q0 * k,
                           out_score + (size_t)q0 * k);
        DIR_HIP_CHECK(hipGetLastError());
    }
    return DIR_OK;
}

}  // namespace dir
