// Segmentation metrics of the reference's evaluation step (src/utils/utils_eval.py: _test_step :18-194, _test_end :196-297),
// on the device. The reference runs them in sklearn / skimage / numpy on the CPU after copying the volume to the host:
//   reconstruction errors   l1_loss / mse_loss over all voxels, seg > 0 and seg == 0                   :36-41
//   AUROC / AUPRC           roc_curve + auc, average_precision_score over (residual, seg > 0)          :80-81, :549-558
//   find_best_val           the greedy 10-step threshold search (Zimmerer), dice at 20 probe points    :84-90, :504-546
//   component filter        label(connectivity = 3) + regionprops, components with filled_area <= 7   :98-99, :485-499
//   confusion counts        on the filtered mask (per row: on the unfiltered one)                      :102-139
//   anomaly scores          masked means of the residual per volume and per row                       :152-165
//   healthy thresholds      roc_curve against all-zero labels, first retained point with fpr > p       :277-286
// Volumes are flat [R][C] fp32 with R = rows (axis 0 of the reference's [H, W, D] volume, the axis its "per-slice" loop
// walks) and C = W * D voxels per row. Determinism: counts use integer atomics; every float sum is a per-block partial
// written to a slab and summed in a fixed order in float64; AUROC is exact (an integer sum of trapezoids over 2 P N).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cddpm.h"
#include "kernels.h"

namespace cddpm {

namespace {

constexpr int EB = 256;                   // threads per block of the wide kernels (4 waves)
constexpr int CURVE_BLOCKS = 256;         // fixed grid of the curve kernels: fixes the float64 summation order

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

// order-preserving map float -> uint32, with -0 folded onto +0 (they compare equal in numpy)
__device__ __forceinline__ uint32_t fkey(float v) {
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fval(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <typename T>
__device__ T block_sum(T v, T* sh) {          // fixed-order tree over the block (deterministic)
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = EB / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

// ---- pass 1: one block per row ---------------------------------------------------------------------------------------
// slab[r][0..6]: l1 all / lesion / healthy, l2 all / lesion / healthy, masked residual sum; rowi[r][0..2]: lesion, healthy
// (seg == 0) and mask counts. Also the sort input in memory order: keys = fkey(residual), labels = seg > 0.
__global__ __launch_bounds__(EB) void eval_rows_kernel(const float* __restrict__ recon, const float* __restrict__ orig,
                                                       const float* __restrict__ seg, const float* __restrict__ mask,
                                                       const float* __restrict__ diff, int C, double* __restrict__ slab,
                                                       int* __restrict__ rowi, uint32_t* __restrict__ keys,
                                                       int* __restrict__ labels) {
    __shared__ double shd[EB];
    __shared__ int shi[EB];
    const int r = blockIdx.x;
    const size_t base = (size_t)r * C;
    double a[7] = {0, 0, 0, 0, 0, 0, 0};
    int nles = 0, nhea = 0, nmask = 0;
    for (int c = threadIdx.x; c < C; c += EB) {
        const size_t i = base + c;
        const float e0 = recon[i] - orig[i];
        const float e1 = fabsf(e0), e2 = e0 * e0;           // the fp32 per-voxel terms torch averages
        const float sg = seg[i];
        a[0] += e1;
        a[3] += e2;
        if (sg > 0.f) { a[1] += e1; a[4] += e2; ++nles; }
        if (sg == 0.f) { a[2] += e1; a[5] += e2; ++nhea; }
        const float df = diff[i];
        if (mask[i] > 0.f) { a[6] += df; ++nmask; }
        keys[i] = fkey(df);
        labels[i] = sg > 0.f ? 1 : 0;
    }
    for (int k = 0; k < 7; ++k) {
        const double s = block_sum(a[k], shd);
        if (threadIdx.x == 0) slab[(size_t)r * 8 + k] = s;
    }
    const int sl = block_sum(nles, shi), sh = block_sum(nhea, shi), sm = block_sum(nmask, shi);
    if (threadIdx.x == 0) { rowi[r * 3 + 0] = sl; rowi[r * 3 + 1] = sh; rowi[r * 3 + 2] = sm; }
}

// ---- pass 2: one block sums the slab over rows in a fixed order ------------------------------------------------------
__global__ __launch_bounds__(EB) void eval_rows_reduce_kernel(const double* __restrict__ slab, const int* __restrict__ rowi,
                                                              int R, int C, double* __restrict__ rec,
                                                              float* __restrict__ row_score, int* __restrict__ row_label) {
    __shared__ double shd[EB];
    __shared__ long long shl[EB];
    double a[7] = {0, 0, 0, 0, 0, 0, 0};
    long long nles = 0, nhea = 0, nmask = 0;
    for (int r = threadIdx.x; r < R; r += EB) {
        for (int k = 0; k < 7; ++k) a[k] += slab[(size_t)r * 8 + k];
        nles += rowi[r * 3];
        nhea += rowi[r * 3 + 1];
        const int m = rowi[r * 3 + 2];
        nmask += m;
        // torch: the mean over an empty selection is NaN, which the reference maps to 0.0 (:157-160)
        row_score[r] = m ? (float)(slab[(size_t)r * 8 + 6] / (double)m) : 0.f;
        row_label[r] = rowi[r * 3] > 0 ? 1 : 0;
    }
    double s[7];
    for (int k = 0; k < 7; ++k) s[k] = block_sum(a[k], shd);
    const long long L = block_sum(nles, shl), Hh = block_sum(nhea, shl), M = block_sum(nmask, shl);
    if (threadIdx.x == 0) {
        const double n = (double)R * C;
        rec[CDDPM_EVAL_L1_ALL] = (float)(s[0] / n);
        rec[CDDPM_EVAL_L1_LESION] = L ? (double)(float)(s[1] / (double)L) : qnan();
        rec[CDDPM_EVAL_L1_HEALTHY] = Hh ? (double)(float)(s[2] / (double)Hh) : qnan();
        rec[CDDPM_EVAL_L2_ALL] = (float)(s[3] / n);
        rec[CDDPM_EVAL_L2_LESION] = L ? (double)(float)(s[4] / (double)L) : qnan();
        rec[CDDPM_EVAL_L2_HEALTHY] = Hh ? (double)(float)(s[5] / (double)Hh) : qnan();
        rec[CDDPM_EVAL_SCORE_VOL] = M ? (double)(float)(s[6] / (double)M) : qnan();
        rec[CDDPM_EVAL_LESION] = (double)L;
        rec[CDDPM_EVAL_VOXELS] = n;
    }
}

// ---- curve over (score, label) pairs sorted by descending score -----------------------------------------------------
// last[i] = 1 where a run of equal scores ends (sklearn's threshold_idxs)
__global__ __launch_bounds__(EB) void curve_bounds_kernel(const uint32_t* __restrict__ k, int n, int* __restrict__ last) {
    for (int i = blockIdx.x * EB + threadIdx.x; i < n; i += gridDim.x * EB) last[i] = (i == n - 1 || k[i] != k[i + 1]) ? 1 : 0;
}

// compact the distinct points: d = didx[i] - 1; fps = i + 1 - tps (sklearn's _binary_clf_curve)
__global__ __launch_bounds__(EB) void curve_compact_kernel(const uint32_t* __restrict__ k, const int* __restrict__ tps,
                                                           const int* __restrict__ last, const int* __restrict__ didx,
                                                           int n, uint32_t* __restrict__ ckey, int* __restrict__ cfps,
                                                           int* __restrict__ ctps) {
    for (int i = blockIdx.x * EB + threadIdx.x; i < n; i += gridDim.x * EB) {
        if (!last[i]) continue;
        const int d = didx[i] - 1;
        ckey[d] = k[i];
        ctps[d] = tps[i];
        cfps[d] = i + 1 - tps[i];
    }
}

// per distinct point d (M of them): twice the AUROC trapezoid times P N as an exact integer (integer atomics), the AUPRC
// term (R_d - R_{d-1}) P_d times P as a float64 block partial, and drop_intermediate's retained flag (roc_curve keeps a
// point where the second difference of fps or of tps is non-zero; the first and the last always stay)
__global__ __launch_bounds__(EB) void curve_points_kernel(const int* __restrict__ cfps, const int* __restrict__ ctps,
                                                          const int* __restrict__ mcount, unsigned long long* __restrict__ area2,
                                                          double* __restrict__ ap_slab, uint8_t* __restrict__ keep) {
    __shared__ double shd[EB];
    __shared__ unsigned long long shu[EB];
    const int M = *mcount;
    double ap = 0.0;
    unsigned long long ar = 0;
    for (int d = blockIdx.x * EB + threadIdx.x; d < M; d += CURVE_BLOCKS * EB) {
        const long long f = cfps[d], t = ctps[d];
        const long long f0 = d ? cfps[d - 1] : 0, t0 = d ? ctps[d - 1] : 0;
        ar += (unsigned long long)((f - f0) * (t + t0));
        if (t > t0) ap += (double)(t - t0) * ((double)t / (double)(t + f));
        bool k = (d == 0) || (d == M - 1);
        if (!k) {
            const long long f2 = cfps[d + 1], t2 = ctps[d + 1];
            k = (f2 - 2 * f + f0) != 0 || (t2 - 2 * t + t0) != 0;
        }
        keep[d] = k ? 1 : 0;
    }
    const double s = block_sum(ap, shd);
    const unsigned long long a = block_sum(ar, shu);
    if (threadIdx.x == 0) {
        ap_slab[blockIdx.x] = s;
        atomicAdd(area2, a);
    }
}

// one thread: AUROC / AUPRC from the totals, and per bound p the first distinct point with fpr > p (binary search; fpr is
// non-decreasing and fpr[M - 1] = 1, so the search always lands)
__global__ __launch_bounds__(64) void curve_finish_kernel(const int* __restrict__ cfps, const int* __restrict__ ctps,
                                                          const int* __restrict__ mcount,
                                                          const unsigned long long* __restrict__ area2,
                                                          const double* __restrict__ ap_slab, int* __restrict__ from,
                                                          double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const int M = *mcount;
    const long long P = ctps[M - 1], N = cfps[M - 1];
    double ap = 0.0;
    for (int b = 0; b < CURVE_BLOCKS; ++b) ap += ap_slab[b];
    out[0] = (P > 0 && N > 0) ? (double)*area2 / (2.0 * (double)P * (double)N) : qnan();   // auc(roc_curve(...))
    out[1] = P > 0 ? ap / (double)P : qnan();                                                 // average_precision_score
    const double bound[3] = {0.01, 0.05, 0.10};
    for (int j = 0; j < 3; ++j) {
        int lo = 0, hi = M - 1;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if ((double)cfps[mid] / (double)N > bound[j]) hi = mid; else lo = mid + 1;
        }
        from[j] = lo;
    }
}

// the first RETAINED point at or after from[j]: dropping intermediate points can move np.argmax(fpr > p)
__global__ __launch_bounds__(EB) void curve_first_keep_kernel(const uint8_t* __restrict__ keep, const int* __restrict__ mcount,
                                                              const int* __restrict__ from, int* __restrict__ first) {
    __shared__ int sh[EB];
    const int M = *mcount;
    int best[3] = {INT_MAX, INT_MAX, INT_MAX};
    for (int d = blockIdx.x * EB + threadIdx.x; d < M; d += CURVE_BLOCKS * EB) {
        if (!keep[d]) continue;
        for (int j = 0; j < 3; ++j)
            if (d >= from[j] && d < best[j]) best[j] = d;
    }
    for (int j = 0; j < 3; ++j) {               // block minimum first: one integer atomic per block and bound
        sh[threadIdx.x] = best[j];
        __syncthreads();
        for (int s = EB / 2; s > 0; s >>= 1) {
            if (threadIdx.x < s) sh[threadIdx.x] = min(sh[threadIdx.x], sh[threadIdx.x + s]);
            __syncthreads();
        }
        if (threadIdx.x == 0 && sh[0] != INT_MAX) atomicMin(&first[j], sh[0]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void curve_thresholds_kernel(const uint32_t* __restrict__ ckey, const int* __restrict__ mcount,
                                                              const int* __restrict__ first, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const int M = *mcount;
    for (int j = 0; j < 3; ++j) {
        const int d = first[j];
        out[2 + j] = (d >= 0 && d < M) ? (double)fval(ckey[d]) : qnan();
    }
}

// find_best_val (:504-546) on the sorted keys: #(x > q) is a binary search, the overlap the tps prefix at that index.
// Probe points in float64 (numpy 1.22: np.float32 - int between scalars promotes), compared in float32 (value-based
// casting rounds q for `x > q`). dice = 2 |P n G| / (|P| + |G|), NaN for 0 / 0; NaN comparisons as in numpy.
__device__ double dice_at(const uint32_t* k, const int* tps, int n, double q, long long G) {
    const uint32_t kq = fkey(__double2float_rn(q));
    int lo = 0, hi = n;                         // first index whose key is not above kq (keys descend)
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (k[mid] > kq) lo = mid + 1; else hi = mid;
    }
    const long long p = lo, pg = lo ? tps[lo - 1] : 0;
    const long long den = p + G;
    return den ? (double)(2 * pg) / (double)den : qnan();
}

// out: [0] best dice, [1] its threshold, [2] the threshold applied (the override in the test stage), [3] max(x)
__global__ __launch_bounds__(64) void best_val_kernel(const uint32_t* __restrict__ k, const int* __restrict__ tps, int n,
                                                      int use_override, double thr_override, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const long long G = tps[n - 1];
    double bottom = 0.0, top = (double)fval(k[0]);    // val_range = (0, max(x))
    double max_val = 0.0, max_point = 0.0;
    for (int step = 0; step < 10; ++step) {
        if (bottom == top) top = 1.0;
        const double w = top - bottom;
        const double center = bottom + w * 0.5, qb = bottom + w * 0.25, qt = bottom + w * 0.75;
        const double vb = dice_at(k, tps, n, qb, G), vt = dice_at(k, tps, n, qt, G);
        if (vb >= vt) {
            if (vb >= max_val) { max_val = vb; max_point = qb; }
            top = center;
        } else {
            if (vt >= max_val) { max_val = vt; max_point = qt; }
            bottom = center;
        }
    }
    out[0] = max_val;
    out[1] = max_point;
    out[2] = use_override ? thr_override : max_point;
    out[3] = (double)fval(k[0]);
}

// ---- threshold, per-row counts of the unfiltered mask, union-find initialisation: one block per row ------------------
__global__ __launch_bounds__(EB) void threshold_rows_kernel(const float* __restrict__ diff, const int* __restrict__ labels,
                                                            int C, const double* __restrict__ thr, uint8_t* __restrict__ pred,
                                                            int* __restrict__ lab, int* __restrict__ row_counts) {
    __shared__ int shi[EB];
    const float t = __double2float_rn(*thr);     // torch: tensor > python scalar compares in float32
    const int r = blockIdx.x;
    const size_t base = (size_t)r * C;
    int p = 0, pg = 0, g = 0;
    for (int c = threadIdx.x; c < C; c += EB) {
        const size_t i = base + c;
        const bool on = diff[i] > t;
        pred[i] = on ? 1 : 0;
        lab[i] = on ? (int)i : -1;
        p += on ? 1 : 0;
        pg += (on && labels[i]) ? 1 : 0;
        g += labels[i];
    }
    const int sp = block_sum(p, shi), spg = block_sum(pg, shi), sg = block_sum(g, shi);
    if (threadIdx.x == 0) { row_counts[r * 3] = sp; row_counts[r * 3 + 1] = spg; row_counts[r * 3 + 2] = sg; }
}

__device__ __forceinline__ int uf_find(int* lab, int x, int n) {
    for (int it = 0; it < n; ++it) {             // bounded: a parent chain is shorter than the volume
        const int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
    return x;
}

// 26-connectivity: each foreground voxel is linked with its foreground neighbours among the 13 that come earlier in
// memory order. The larger root is hooked under the smaller one by CAS, so a component's root is its smallest index.
__global__ __launch_bounds__(EB) void cc_union_kernel(const uint8_t* __restrict__ pred, int* __restrict__ lab, int D0, int D1,
                                                      int D2) {
    const int n = D0 * D1 * D2;
    for (int i = blockIdx.x * EB + threadIdx.x; i < n; i += gridDim.x * EB) {
        if (!pred[i]) continue;
        const int z = i % D2, y = (i / D2) % D1, x = i / (D1 * D2);
        for (int o = 0; o < 13; ++o) {
            // o < 9: (-1, dy, dz) for dy, dz in {-1, 0, 1}; o = 9..11: (0, -1, dz); o = 12: (0, 0, -1)
            const int dx = o < 9 ? -1 : 0;
            const int dy = o < 9 ? o / 3 - 1 : (o < 12 ? -1 : 0);
            const int dz = o < 9 ? o % 3 - 1 : (o < 12 ? o - 10 : -1);
            const int xx = x + dx, yy = y + dy, zz = z + dz;
            if (xx < 0 || yy < 0 || zz < 0 || yy >= D1 || zz >= D2) continue;
            const int j = (xx * D1 + yy) * D2 + zz;
            if (!pred[j]) continue;
            int a = uf_find(lab, i, n), b = uf_find(lab, j, n);
            for (int it = 0; it < n && a != b; ++it) {
                if (a < b) { const int t = a; a = b; b = t; }
                const int old = atomicCAS(&lab[a], a, b);
                if (old == a) break;
                a = uf_find(lab, old, n);
                b = uf_find(lab, b, n);
            }
        }
    }
}

// count the component sizes at their roots
__global__ __launch_bounds__(EB) void cc_size_kernel(int* __restrict__ lab, int* __restrict__ size, int n) {
    for (int i = blockIdx.x * EB + threadIdx.x; i < n; i += gridDim.x * EB) {
        if (lab[i] < 0) continue;
        atomicAdd(&size[uf_find(lab, i, n)], 1);
    }
}

// clear components of <= 7 voxels (filter != 0; skimage's filled_area equals the voxel count that small: a cavity needs a
// closed shell of 26 voxels), then the confusion counts of (pred, seg) on what is left
__global__ __launch_bounds__(EB) void cc_filter_kernel(uint8_t* __restrict__ pred, int* __restrict__ lab,
                                                       const int* __restrict__ size, const int* __restrict__ labels, int n,
                                                       int filter, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long shu[EB];
    unsigned long long c10 = 0, c11 = 0;
    for (int i = blockIdx.x * EB + threadIdx.x; i < n; i += gridDim.x * EB) {
        bool on = pred[i] != 0;
        if (on && filter && size[uf_find(lab, i, n)] <= 7) {
            on = false;
            pred[i] = 0;
        }
        if (on) { if (labels[i]) ++c11; else ++c10; }
    }
    const unsigned long long s10 = block_sum(c10, shu), s11 = block_sum(c11, shu);
    if (threadIdx.x == 0) {
        atomicAdd(&counts[0], s10);
        atomicAdd(&counts[1], s11);
    }
}

// the volume record's metric slots from the scratch results of the passes above
__global__ __launch_bounds__(64) void eval_finish_kernel(const double* __restrict__ sc, const unsigned long long* __restrict__ counts,
                                                         int voxel, int rows, double* __restrict__ rec) {
    if (threadIdx.x != 0) return;
    if (voxel) {
        rec[CDDPM_EVAL_AUROC] = sc[0];
        rec[CDDPM_EVAL_AUPRC] = sc[1];
        rec[CDDPM_EVAL_BEST_DICE] = sc[8];
        rec[CDDPM_EVAL_BEST_THRESHOLD] = sc[9];
        rec[CDDPM_EVAL_THRESHOLD] = sc[10];
        rec[CDDPM_EVAL_MAX] = sc[11];
        rec[CDDPM_EVAL_PRED1_SEG0] = (double)counts[0];
        rec[CDDPM_EVAL_PRED1_SEG1] = (double)counts[1];
    }
    if (rows) {
        rec[CDDPM_EVAL_ROW_AUROC] = sc[12];
        rec[CDDPM_EVAL_ROW_AUPRC] = sc[13];
    }
}

__global__ __launch_bounds__(64) void set_finish_kernel(const double* __restrict__ sc, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    out[CDDPM_EVAL_SET_AUROC] = sc[0];
    out[CDDPM_EVAL_SET_AUPRC] = sc[1];
    out[CDDPM_EVAL_SET_T1P] = sc[2];
    out[CDDPM_EVAL_SET_T5P] = sc[3];
    out[CDDPM_EVAL_SET_T10P] = sc[4];
    out[CDDPM_EVAL_SET_BEST_DICE] = sc[8];
    out[CDDPM_EVAL_SET_BEST_THRESHOLD] = sc[9];
    out[CDDPM_EVAL_SET_MAX] = sc[11];
}

template <typename L>
__global__ __launch_bounds__(EB) void pairs_kernel(const float* __restrict__ x, const L* __restrict__ y, int n, int zero_labels,
                                                   uint32_t* __restrict__ keys, int* __restrict__ labels) {
    for (int i = blockIdx.x * EB + threadIdx.x; i < n; i += gridDim.x * EB) {
        keys[i] = fkey(x[i]);
        labels[i] = (!zero_labels && y[i] != 0) ? 1 : 0;
    }
}

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

int grid_for(long long n) {
    const long long g = (n + EB - 1) / EB;
    return g < 1 ? 1 : (g > 4096 ? 4096 : (int)g);
}

// ---- workspace -------------------------------------------------------------------------------------------------------
struct EvalWs {
    uint32_t *keys, *keys_out, *ckey;
    int *labels, *lab_out, *tps, *didx, *last, *cfps, *ctps, *uf, *size;
    uint8_t *pred, *keep;
    double *slab, *ap_slab, *scratch;
    int *rowi, *mcount, *from, *first;
    unsigned long long *area2, *counts;
    void* cub;
    size_t cub_bytes;
};

size_t cub_bytes_for(int n) {
    size_t a = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                       (const int*)nullptr, (int*)nullptr, n);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (const int*)nullptr, (int*)nullptr, n);
    return a > b ? a : b;
}

// n items, R rows (0: a set search, no volume arrays). ckey reuses `keys` once the sort has read it.
size_t layout(int n, int R, char* base, EvalWs* w) {
    size_t cb = cub_bytes_for(n);
    if (R > 0) { const size_t cr = cub_bytes_for(R); cb = cb > cr ? cb : cr; }
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al(bytes ? bytes : 1); return p; };
    EvalWs t{};
    t.keys = (uint32_t*)take(4ull * n);
    t.keys_out = (uint32_t*)take(4ull * n);
    t.labels = (int*)take(4ull * n);
    t.lab_out = (int*)take(4ull * n);
    t.tps = (int*)take(4ull * n);
    t.didx = (int*)take(4ull * n);
    t.last = (int*)take(4ull * n);
    t.cfps = (int*)take(4ull * n);
    t.ctps = (int*)take(4ull * n);
    t.keep = (uint8_t*)take((size_t)n);
    if (R > 0) {
        t.uf = (int*)take(4ull * n);
        t.size = (int*)take(4ull * n);
        t.pred = (uint8_t*)take((size_t)n);
        t.slab = (double*)take(8ull * 8 * R);
        t.rowi = (int*)take(4ull * 3 * R);
    }
    t.ap_slab = (double*)take(8ull * CURVE_BLOCKS);
    t.scratch = (double*)take(8ull * 16);
    t.mcount = (int*)take(4);
    t.from = (int*)take(4 * 3);
    t.first = (int*)take(4 * 3);
    t.area2 = (unsigned long long*)take(8);
    t.counts = (unsigned long long*)take(8 * 2);
    t.cub = take(cb);
    t.cub_bytes = cb;
    t.ckey = t.keys;
    if (w) *w = t;
    return off;
}

#define EVCHECK(call)                                  \
    do {                                               \
        const hipError_t e_ = (call);                  \
        if (e_ != hipSuccess) return e_;               \
    } while (0)

// sort (keys, vals) descending, scan the labels, compact the distinct points; out[0..1] = AUROC / AUPRC, out[2..4] = the
// thresholds at the first retained point with fpr > 1 % / 5 % / 10 %. keys_out / tps stay valid for best_val_kernel.
hipError_t run_curve(EvalWs& w, const uint32_t* keys, const int* vals, int n, double* out, hipStream_t s) {
    size_t tb = w.cub_bytes;
    EVCHECK(hipcub::DeviceRadixSort::SortPairsDescending(w.cub, tb, keys, w.keys_out, vals, w.lab_out, n, 0, 32, s));
    tb = w.cub_bytes;
    EVCHECK(hipcub::DeviceScan::InclusiveSum(w.cub, tb, w.lab_out, w.tps, n, s));
    const int g = grid_for(n);
    hipLaunchKernelGGL(curve_bounds_kernel, dim3(g), dim3(EB), 0, s, w.keys_out, n, w.last);
    tb = w.cub_bytes;
    EVCHECK(hipcub::DeviceScan::InclusiveSum(w.cub, tb, w.last, w.didx, n, s));
    hipLaunchKernelGGL(curve_compact_kernel, dim3(g), dim3(EB), 0, s, w.keys_out, w.tps, w.last, w.didx, n, w.ckey, w.cfps,
                       w.ctps);
    EVCHECK(hipMemcpyAsync(w.mcount, w.didx + (n - 1), sizeof(int), hipMemcpyDeviceToDevice, s));
    EVCHECK(hipMemsetAsync(w.area2, 0, sizeof(unsigned long long), s));
    EVCHECK(hipMemsetAsync(w.first, 0x7f, 3 * sizeof(int), s));
    hipLaunchKernelGGL(curve_points_kernel, dim3(CURVE_BLOCKS), dim3(EB), 0, s, w.cfps, w.ctps, w.mcount, w.area2, w.ap_slab,
                       w.keep);
    hipLaunchKernelGGL(curve_finish_kernel, dim3(1), dim3(64), 0, s, w.cfps, w.ctps, w.mcount, w.area2, w.ap_slab, w.from, out);
    hipLaunchKernelGGL(curve_first_keep_kernel, dim3(CURVE_BLOCKS), dim3(EB), 0, s, w.keep, w.mcount, w.from, w.first);
    hipLaunchKernelGGL(curve_thresholds_kernel, dim3(1), dim3(64), 0, s, w.ckey, w.mcount, w.first, out);
    return hipGetLastError();
}

}  // namespace

size_t eval_workspace_bytes(int n, int rows) { return layout(n, rows, nullptr, nullptr); }

hipError_t launch_eval_volume(const float* recon, const float* orig, const float* seg, const float* mask, const float* diff,
                              int R, int D1, int D2, int flags, double thr_override, void* ws, size_t ws_bytes, double* rec,
                              float* row_score, int* row_label, int* row_counts, uint8_t* pred_out, hipStream_t s) {
    const int C = D1 * D2, n = R * C;
    EvalWs w;
    if (layout(n, R, (char*)ws, &w) > ws_bytes) return hipErrorInvalidValue;
    EVCHECK(hipMemsetAsync(rec, 0xff, CDDPM_EVAL_RECORD * sizeof(double), s));     // NaN where nothing is computed
    hipLaunchKernelGGL(eval_rows_kernel, dim3(R), dim3(EB), 0, s, recon, orig, seg, mask, diff, C, w.slab, w.rowi, w.keys,
                       w.labels);
    hipLaunchKernelGGL(eval_rows_reduce_kernel, dim3(1), dim3(EB), 0, s, w.slab, w.rowi, R, C, rec, row_score, row_label);
    const int voxel = (flags & CDDPM_EVAL_VOXEL_METRICS) ? 1 : 0, rows = (flags & CDDPM_EVAL_ROW_CURVE) ? 1 : 0;
    if (voxel) {
        EVCHECK(run_curve(w, w.keys, w.labels, n, w.scratch, s));
        hipLaunchKernelGGL(best_val_kernel, dim3(1), dim3(64), 0, s, w.keys_out, w.tps, n,
                           (flags & CDDPM_EVAL_THRESHOLD_OVERRIDE) ? 1 : 0, thr_override, w.scratch + 8);
        hipLaunchKernelGGL(threshold_rows_kernel, dim3(R), dim3(EB), 0, s, diff, w.labels, C, w.scratch + 10, w.pred, w.uf,
                           row_counts);
        const int filter = (flags & CDDPM_EVAL_COMPONENT_FILTER) ? 1 : 0;
        if (filter) {
            EVCHECK(hipMemsetAsync(w.size, 0, 4ull * n, s));
            hipLaunchKernelGGL(cc_union_kernel, dim3(grid_for(n)), dim3(EB), 0, s, w.pred, w.uf, R, D1, D2);
            hipLaunchKernelGGL(cc_size_kernel, dim3(grid_for(n)), dim3(EB), 0, s, w.uf, w.size, n);
        }
        EVCHECK(hipMemsetAsync(w.counts, 0, 2 * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(cc_filter_kernel, dim3(grid_for(n)), dim3(EB), 0, s, w.pred, w.uf, w.size, w.labels, n, filter,
                           w.counts);
        if (pred_out) EVCHECK(hipMemcpyAsync(pred_out, w.pred, (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    if (rows) {     // AUROC / AUPRC of the per-row scores against the per-row labels: the same curve code over R items
        hipLaunchKernelGGL(pairs_kernel<int>, dim3(grid_for(R)), dim3(EB), 0, s, row_score, row_label, R, 0, w.keys, w.labels);
        EVCHECK(run_curve(w, w.keys, w.labels, R, w.scratch + 12, s));
    }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(64), 0, s, w.scratch, w.counts, voxel, rows, rec);
    return hipGetLastError();
}

hipError_t launch_eval_set(const float* x, const int8_t* y, int n, int healthy, void* ws, size_t ws_bytes, double* out,
                           hipStream_t s) {
    EvalWs w;
    if (layout(n, 0, (char*)ws, &w) > ws_bytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pairs_kernel<int8_t>, dim3(grid_for(n)), dim3(EB), 0, s, x, y, n, healthy, w.keys, w.labels);
    EVCHECK(run_curve(w, w.keys, w.labels, n, w.scratch, s));
    hipLaunchKernelGGL(best_val_kernel, dim3(1), dim3(64), 0, s, w.keys_out, w.tps, n, 0, 0.0, w.scratch + 8);
    hipLaunchKernelGGL(set_finish_kernel, dim3(1), dim3(64), 0, s, w.scratch, out);
    return hipGetLastError();
}

}  // namespace cddpm
