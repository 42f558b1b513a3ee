// ivf_plan.hip — the probe tables of a scan by list, made on the device in ONE launch.
//
// dir_ivf_scan_i8 / dir_ivf_scan_fp4 walk the probe table of a query chunk INVERTED: the (query, slot) pairs grouped by
// list, a CSR of the pairs and a CSR of the workgroups by list (include/dir_engine.h).  ops.ivf_probe_tables builds those
// with about thirty integer torch launches and reads two integers back; ivf_plan_kernel builds the same tables, bit for
// bit, from probe [Q][nprobe] and list_off [nlist + 1] in one workgroup of 1024 threads, and nothing comes back to the host.
//
// The ORDER of the pairs is part of the contract (by list; inside a list ascending in the flat index q * nprobe + p; empty
// slots last - the order of a stable sort of the lists), so nothing here depends on the arrival order of atomics:
//   1. key[f] = (list << 14) | f, an empty slot (a list outside [0, nlist)) keyed nlist; 30 bits, unique.  len[f] = the
//      length of the slot's list, 0 for an empty slot.
//   2. an exclusive scan of len over the flat index (uint32: wrap-around cancels in a difference) gives
//      col_off[f] = scan[f] - scan[first slot of f's query], and a workgroup max of col_off + len gives reach.
//   3. a bitonic sort of the keys in LDS (padded to a power of two with keys above every real one).
//   4. pair_q / pair_col of place i from the flat index in the low 14 bits of the sorted key i.
//   5. pair_off[l] = the lower bound of l << 14 in the sorted keys; a thread owns a run of consecutive lists, and a
//      workgroup exclusive scan of the runs' ceil(len / 256) * ceil(pairs / 32) gives item_off.
// LDS: 2 * 4 bytes per padded pair + 132: 128.1 KiB at the 16384 pairs the entry admits.
#include "dir_common.h"
#include "pointwise.h"

namespace dir {

static constexpr int kPlanThreads = 1024;
static constexpr int kPlanWaves = kPlanThreads / 64;
static constexpr int kPlanFlatBits = 14;
static constexpr int kPlanMaxPairs = 1 << kPlanFlatBits;        // the flat index takes the low 14 bits of a key
static constexpr int kPlanTileRows = 256, kPlanGroup = 32;      // the scans' cut: rows a tile, pairs a group
static constexpr uint32_t kPlanPadKey = 0x7fffffffu;

int ivf_plan_max_pairs() { return kPlanMaxPairs; }

// inclusive scan of one value per lane across the wave
__device__ __forceinline__ uint32_t plan_wave_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive scan of one value per thread across the workgroup -> (the sum of the threads before this one, the sum of all);
// part [kPlanWaves + 1] is LDS scratch, free again on return
__device__ __forceinline__ uint32_t plan_block_scan(uint32_t v, uint32_t* part, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = plan_wave_scan(v, lane);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const uint32_t w = lane < kPlanWaves ? part[lane] : 0u;
        const uint32_t ws = plan_wave_scan(w, lane);
        if (lane < kPlanWaves) part[lane] = ws - w;
        if (lane == kPlanWaves - 1) part[kPlanWaves] = ws;
    }
    __syncthreads();
    const uint32_t before = part[wave] + incl - v;
    total = part[kPlanWaves];
    __syncthreads();
    return before;
}

// the first place of keys[0 .. n) (ascending) that holds a key >= bound
__device__ __forceinline__ int plan_lower_bound(const uint32_t* keys, int n, uint32_t bound) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kPlanThreads) ivf_plan_kernel(const int* __restrict__ probe, int P, int nprobe, int Ppad,
                                                              const int* __restrict__ list_off, int nlist,
                                                              int* __restrict__ col_off, int* __restrict__ pair_off,
                                                              int* __restrict__ pair_q, int* __restrict__ pair_col,
                                                              int* __restrict__ item_off, int* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* keys = (uint32_t*)smem;                 // [Ppad]
    uint32_t* ex = keys + Ppad;                       // [Ppad + 1]: len, then its exclusive scan; ex[Ppad] = the sum
    uint32_t* part = ex + Ppad + 1;                   // [kPlanWaves + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 1. keys and lengths
    for (int f = tid; f < Ppad; f += kPlanThreads) {
        uint32_t key = kPlanPadKey, len = 0u;
        if (f < P) {
            const int l = probe[f];
            const bool real = (unsigned)l < (unsigned)nlist;
            if (real) len = (uint32_t)(list_off[l + 1] - list_off[l]);
            key = ((uint32_t)(real ? l : nlist) << kPlanFlatBits) | (uint32_t)f;
        }
        keys[f] = key;
        ex[f] = len;
    }
    __syncthreads();

    // 2. the exclusive scan of the lengths: thread t owns the E consecutive places from t * E
    {
        const int E = Ppad >= kPlanThreads ? Ppad / kPlanThreads : 1;
        const int f0 = tid * E;
        uint32_t sum = 0u;
        if (f0 < Ppad)
            for (int e = 0; e < E; ++e) sum += ex[f0 + e];
        uint32_t total;
        uint32_t run = plan_block_scan(sum, part, total);
        if (f0 < Ppad)
            for (int e = 0; e < E; ++e) {
                const uint32_t len = ex[f0 + e];
                ex[f0 + e] = run;
                run += len;
            }
        if (tid == 0) ex[Ppad] = total;
    }
    __syncthreads();
    int reach = 0;
    for (int f = tid; f < P; f += kPlanThreads) {
        const int q = f / nprobe;
        const int c = (int)(ex[f] - ex[q * nprobe]);
        col_off[f] = c;
        reach = max(reach, c + (int)(ex[f + 1] - ex[f]));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) reach = max(reach, __shfl_xor(reach, d, 64));
    if (lane == 0) part[wave] = (uint32_t)reach;
    __syncthreads();
    if (tid == 0) {
        int r = 0;
        for (int w = 0; w < kPlanWaves; ++w) r = max(r, (int)part[w]);
        counts[1] = r;
    }

    // 3. bitonic sort of the keys (part is read above and written again only after the barriers below)
    for (int k = 2; k <= Ppad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (Ppad >> 1); t += kPlanThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint32_t a = keys[i], b = keys[i | j];
                if ((a > b) == ((i & k) == 0)) {
                    keys[i] = b;
                    keys[i | j] = a;
                }
            }
            __syncthreads();
        }

    // 4. the pairs in their order
    for (int i = tid; i < P; i += kPlanThreads) {
        const int f = (int)(keys[i] & (uint32_t)(kPlanMaxPairs - 1));
        const int q = f / nprobe;
        pair_q[i] = q;
        pair_col[i] = (int)(ex[f] - ex[q * nprobe]);
    }

    // 5. the two CSRs by list: thread t owns the lists [l0, l1)
    const int run = (nlist + kPlanThreads - 1) / kPlanThreads;
    const int l0 = min(tid * run, nlist), l1 = min(l0 + run, nlist);
    uint32_t mine = 0u;
    if (l0 < l1) {
        int lb = plan_lower_bound(keys, P, (uint32_t)l0 << kPlanFlatBits);
        for (int l = l0; l < l1; ++l) {
            const int nb = plan_lower_bound(keys, P, (uint32_t)(l + 1) << kPlanFlatBits);
            const int len = list_off[l + 1] - list_off[l], pairs = nb - lb;
            pair_off[l] = lb;
            mine += (uint32_t)(((len + kPlanTileRows - 1) / kPlanTileRows) * ((pairs + kPlanGroup - 1) / kPlanGroup));
            lb = nb;
        }
        if (l1 == nlist) pair_off[nlist] = lb;
    }
    uint32_t items;
    uint32_t at = plan_block_scan(mine, part, items);
    for (int l = l0; l < l1; ++l) {
        const int len = list_off[l + 1] - list_off[l];
        const int pairs = (l + 1 < l1 || l1 == nlist ? pair_off[l + 1] : plan_lower_bound(keys, P, (uint32_t)(l + 1) << kPlanFlatBits)) -
                          pair_off[l];
        item_off[l] = (int)at;
        at += (uint32_t)(((len + kPlanTileRows - 1) / kPlanTileRows) * ((pairs + kPlanGroup - 1) / kPlanGroup));
    }
    if (tid == 0) {
        item_off[nlist] = (int)items;
        counts[0] = (int)items;
    }
}

int ivf_plan(const int* probe, int Q, int nprobe, const int* list_off, int nlist, int* col_off, int* pair_off, int* pair_q,
             int* pair_col, int* item_off, int* counts, hipStream_t stream) {
    if (Q <= 0) return DIR_OK;
    const int P = Q * nprobe;          // <= kPlanMaxPairs: the entry's check
    int Ppad = 2;
    while (Ppad < P) Ppad <<= 1;
    const int lds = (2 * Ppad + 1 + kPlanWaves + 1) * 4;
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)ivf_plan_kernel, (2 * kPlanMaxPairs + 1 + kPlanWaves + 1) * 4, attr_done));
    hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(kPlanThreads), lds, stream, probe, P, nprobe, Ppad, list_off, nlist,
                       col_off, pair_off, pair_q, pair_col, item_off, counts);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir
