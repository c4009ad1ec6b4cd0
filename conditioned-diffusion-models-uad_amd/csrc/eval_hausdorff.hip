// The Hausdorff distance of the reference's evaluation step (src/utils/utils_eval.py:131-135: HausPerVol, aggregated :240-241),
// on the device. The reference gets it from monai.metrics.compute_hausdorff_distance(diffs_thresholded, data_seg,
// include_background=False, distance_metric='euclidean', percentile=None, directed=False) on the CPU. Restated here (include/cddpm.h
// has the full rules; pinned to scipy bit for bit, unpinned to monai, which is not available to compare with):
//   masks       P = pred != 0, G = seg != 0; U = P | G
//   active axes with CDDPM_HAUSDORFF_SQUEEZE those along which U's bounding box is wider than one voxel, otherwise all three
//   edges       M & ~erode(M): a voxel of M is an edge unless both neighbours along every active axis are in M (outside the
//               volume counts as not in M); with no active axis (U is one voxel) the voxel is its own edge
//   distances   the exact squared Euclidean distance transform of both edge sets, separably: three line passes of
//               D[i] = min_j f[j] + (i - j)^2 in int32, f = 0 on an edge voxel and HD_FAR elsewhere
//   result      sqrt((double) max over edge(P) of d2(., edge(G)), and the reverse)
// Everything is integer arithmetic with integer atomics (min / max / add), so the result does not depend on the order of execution.
// Volumes are flat [R][D1][D2], D2 contiguous. Nothing allocates or synchronises; the bounding box never leaves the device.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cddpm.h"
#include "kernels.h"

namespace cddpm {

namespace {

constexpr int HB = 256;                   // threads per block (4 waves)
constexpr int HD_FAR = CDDPM_HAUSDORFF_FAR;   // "no edge voxel on this line yet": FAR + 3 * 1023^2 stays below 2^31
constexpr int TILE = 2048;                // int32 elements of one line tile in LDS (8 KB): K neighbouring lines of length L <= 1024
constexpr int PASS_BLOCKS = 128;          // grid of a line pass per field: with both fields one block per CU; tiles beyond it loop

// stats (int32): [0..2] bounding-box minimum per axis, [3..5] maximum (-1: U is empty), [6] #edge(P), [7] #edge(G),
// [8] max over edge(P) of d2 to edge(G), [9] the reverse
constexpr int ST_MIN = 0, ST_MAX = 3, ST_NEDGE = 6, ST_DIR = 8, ST_COUNT = 16;

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double pinf() { return __longlong_as_double(0x7ff0000000000000ll); }

__global__ __launch_bounds__(64) void hd_init_kernel(int* __restrict__ st) {
    const int t = threadIdx.x;
    if (t < ST_COUNT) st[t] = t < ST_MAX ? INT_MAX : (t < ST_NEDGE ? -1 : 0);
}

// block-wide reduction of v by OP over HB threads; the result is valid in thread 0
template <typename OP>
__device__ int block_reduce(int v, int* sh, OP op) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = HB / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = op(sh[t], sh[t + s]);
        __syncthreads();
    }
    const int r = sh[0];
    __syncthreads();
    return r;
}

// ---- pass 1: the bounding box of U = (pred != 0) | (seg != 0) -----------------------------------------------------------------
__global__ __launch_bounds__(HB) void hd_bbox_kernel(const uint8_t* __restrict__ pred, const float* __restrict__ seg, int D1, int D2,
                                                     int n, int* __restrict__ st) {
    __shared__ int sh[HB];
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
    for (int i = blockIdx.x * HB + threadIdx.x; i < n; i += gridDim.x * HB) {
        if (pred[i] == 0 && seg[i] == 0.f) continue;
        const int c[3] = {i / (D1 * D2), (i / D2) % D1, i % D2};
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], c[a]);
            hi[a] = max(hi[a], c[a]);
        }
    }
    for (int a = 0; a < 3; ++a) {
        const int l = block_reduce(lo[a], sh, [](int x, int y) { return min(x, y); });
        const int h = block_reduce(hi[a], sh, [](int x, int y) { return max(x, y); });
        if (threadIdx.x == 0 && h >= 0) {
            atomicMin(&st[ST_MIN + a], l);
            atomicMax(&st[ST_MAX + a], h);
        }
    }
}

// the active axes from the bounding box (every thread derives them itself: three loads of one cache line)
__device__ __forceinline__ void active_axes(const int* st, int squeeze, bool act[3]) {
    for (int a = 0; a < 3; ++a) act[a] = !squeeze || st[ST_MAX + a] > st[ST_MIN + a];
}

// ---- pass 2: the edge byte (bit 0: edge(P), bit 1: edge(G)), the edge counts and the start of both fields --------------------
__global__ __launch_bounds__(HB) void hd_edge_kernel(const uint8_t* __restrict__ pred, const float* __restrict__ seg, int R, int D1,
                                                     int D2, int n, int squeeze, uint8_t* __restrict__ edges,
                                                     int32_t* __restrict__ field, int* st) {
    __shared__ int sh[HB];
    bool act[3];
    active_axes(st, squeeze, act);                 // slots 0..5, complete since pass 1; this pass adds to slots 6 and 7 only
    const int dim[3] = {R, D1, D2}, stride[3] = {D1 * D2, D2, 1};
    int np = 0, ng = 0;
    for (int i = blockIdx.x * HB + threadIdx.x; i < n; i += gridDim.x * HB) {
        const bool p = pred[i] != 0, g = seg[i] != 0.f;
        bool ip = p, ig = g;                       // survives the erosion: both neighbours along every active axis are in the mask
        if (p || g) {
            const int c[3] = {i / (D1 * D2), (i / D2) % D1, i % D2};
            bool any = false;
            for (int a = 0; a < 3; ++a) {
                if (!act[a]) continue;
                any = true;
                const bool below = c[a] > 0, above = c[a] < dim[a] - 1;
                if (!below || !above) { ip = ig = false; continue; }
                const int j0 = i - stride[a], j1 = i + stride[a];
                ip = ip && pred[j0] != 0 && pred[j1] != 0;
                ig = ig && seg[j0] != 0.f && seg[j1] != 0.f;
            }
            if (!any) ip = ig = false;             // U is a single voxel: it is its own edge
        }
        const bool ep = p && !ip, eg = g && !ig;
        edges[i] = (uint8_t)((ep ? 1 : 0) | (eg ? 2 : 0));
        field[i] = ep ? 0 : HD_FAR;
        field[(size_t)n + i] = eg ? 0 : HD_FAR;
        np += ep ? 1 : 0;
        ng += eg ? 1 : 0;
    }
    const int sp = block_reduce(np, sh, [](int x, int y) { return x + y; });
    const int sg = block_reduce(ng, sh, [](int x, int y) { return x + y; });
    if (threadIdx.x == 0) {
        if (sp) atomicAdd(&st[ST_NEDGE], sp);
        if (sg) atomicAdd(&st[ST_NEDGE + 1], sg);
    }
}

// ---- pass 3 (once per axis): D[i] = min_j f[j] + (i - j)^2 along every line of one axis, in place, both fields (blockIdx.y) -----
// A line has L elements `ls` apart. Lines come in `outer` groups `os` apart of `inner` neighbouring lines `ks` apart; a tile is
// K <= inner neighbouring lines of one group, staged whole in LDS as tile[l * K + k], so a block owns every line it rewrites.
//   CONTIG = false (axes 0 and 1): ks = 1, the K lines are side by side in memory and a tile row of K elements is contiguous;
//   CONTIG = true (axis 2): ls = 1, ks = L, the K lines follow each other and the whole tile is one contiguous run of K * L.
// Threads walk the tile in memory order in both cases, so loads and stores are as contiguous as the layout allows.
template <bool CONTIG>
__global__ __launch_bounds__(HB) void hd_line_pass_kernel(int32_t* __restrict__ field, size_t n, int L, int ls, int outer, size_t os,
                                                          int inner, int ks, int K) {
    __shared__ int32_t tile[TILE];
    int32_t* __restrict__ f = field + (size_t)blockIdx.y * n;
    const int tiles_per_group = (inner + K - 1) / K;
    const long long tiles = (long long)outer * tiles_per_group;
    for (long long id = blockIdx.x; id < tiles; id += gridDim.x) {
        const int o = (int)(id / tiles_per_group), k0 = (int)(id % tiles_per_group) * K;
        const int kc = min(K, inner - k0);                      // lines of this tile
        int32_t* __restrict__ base = f + (size_t)o * os + (size_t)k0 * ks;
        const int cnt = kc * L;
        for (int e = threadIdx.x; e < cnt; e += HB) {
            const int l = CONTIG ? e % L : e / kc, k = CONTIG ? e / L : e % kc;
            tile[l * K + k] = base[(size_t)l * ls + (size_t)k * ks];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += HB) {
            const int i = CONTIG ? e % L : e / kc, k = CONTIG ? e / L : e % kc;
            int best = INT_MAX;
            for (int j = 0; j < L; ++j) {
                const int d = i - j;
                best = min(best, tile[j * K + k] + d * d);
            }
            base[(size_t)i * ls + (size_t)k * ks] = best;
        }
        __syncthreads();                                        // the next tile overwrites the LDS image
    }
}

// ---- pass 4: the two directed maxima -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void hd_max_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ field, int n,
                                                    int* __restrict__ st) {
    __shared__ int sh[HB];
    int pg = 0, gp = 0;
    for (int i = blockIdx.x * HB + threadIdx.x; i < n; i += gridDim.x * HB) {
        const uint8_t e = edges[i];
        if (e & 1) pg = max(pg, field[(size_t)n + i]);          // from edge(P) to the nearest voxel of edge(G)
        if (e & 2) gp = max(gp, field[i]);
    }
    const int mpg = block_reduce(pg, sh, [](int x, int y) { return max(x, y); });
    const int mgp = block_reduce(gp, sh, [](int x, int y) { return max(x, y); });
    if (threadIdx.x == 0) {
        if (mpg) atomicMax(&st[ST_DIR], mpg);
        if (mgp) atomicMax(&st[ST_DIR + 1], mgp);
    }
}

__global__ __launch_bounds__(64) void hd_finish_kernel(const int* __restrict__ st, int squeeze, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const int np = st[ST_NEDGE], ng = st[ST_NEDGE + 1];         // a non-empty mask always has an edge
    const bool both = np > 0 && ng > 0;
    const int m = max(st[ST_DIR], st[ST_DIR + 1]);
    out[CDDPM_HAUSDORFF_DISTANCE] = both ? sqrt((double)m) : ((np > 0 || ng > 0) ? pinf() : qnan());
    out[CDDPM_HAUSDORFF_D2_PRED_TO_SEG] = both ? (double)st[ST_DIR] : qnan();
    out[CDDPM_HAUSDORFF_D2_SEG_TO_PRED] = both ? (double)st[ST_DIR + 1] : qnan();
    out[CDDPM_HAUSDORFF_EDGES_PRED] = (double)np;
    out[CDDPM_HAUSDORFF_EDGES_SEG] = (double)ng;
    bool act[3];
    active_axes(st, squeeze, act);
    for (int a = 0; a < 3; ++a) out[CDDPM_HAUSDORFF_ACTIVE_AXIS0 + a] = act[a] ? 1.0 : 0.0;     // an empty U has min > max: none
}

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

int grid_for(long long n) {
    const long long g = (n + HB - 1) / HB;
    return g < 1 ? 1 : (g > 4096 ? 4096 : (int)g);
}

struct HdWs {
    int* stats;
    uint8_t* edges;
    int32_t* field;
};

size_t layout(size_t n, char* base, HdWs* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al(bytes); return p; };
    HdWs t{};
    t.stats = (int*)take(sizeof(int) * ST_COUNT);
    t.edges = (uint8_t*)take(n);
    t.field = (int32_t*)take(sizeof(int32_t) * 2 * n);
    if (w) *w = t;
    return off;
}

void line_pass(int32_t* field, size_t n, bool contig, int L, int ls, int outer, size_t os, int inner, int ks, hipStream_t s) {
    if (L == 1) return;                                         // D[0] = f[0]
    int K = TILE / L;                                           // L <= 1024: K >= 2
    if (K > inner) K = inner;
    const long long tiles = (long long)outer * ((inner + K - 1) / K);
    const dim3 grid((unsigned)(tiles < PASS_BLOCKS ? tiles : PASS_BLOCKS), 2);
    if (contig) hipLaunchKernelGGL(hd_line_pass_kernel<true>, grid, dim3(HB), 0, s, field, n, L, ls, outer, os, inner, ks, K);
    else hipLaunchKernelGGL(hd_line_pass_kernel<false>, grid, dim3(HB), 0, s, field, n, L, ls, outer, os, inner, ks, K);
}

}  // namespace

size_t hausdorff_workspace_bytes(int R, int D1, int D2) { return layout((size_t)R * D1 * D2, nullptr, nullptr); }

hipError_t launch_eval_hausdorff(const uint8_t* pred, const float* seg, int R, int D1, int D2, int squeeze, void* ws, size_t ws_bytes,
                                 double* out, uint8_t* edges_out, int32_t* dist2_out, hipStream_t s) {
    const size_t n = (size_t)R * D1 * D2;                       // <= 2^30: voxel indices fit an int
    HdWs w;
    if (layout(n, (char*)ws, &w) > ws_bytes) return hipErrorInvalidValue;
    const int g = grid_for((long long)n);
    hipLaunchKernelGGL(hd_init_kernel, dim3(1), dim3(64), 0, s, w.stats);
    hipLaunchKernelGGL(hd_bbox_kernel, dim3(g), dim3(HB), 0, s, pred, seg, D1, D2, (int)n, w.stats);
    hipLaunchKernelGGL(hd_edge_kernel, dim3(g), dim3(HB), 0, s, pred, seg, R, D1, D2, (int)n, squeeze, w.edges, w.field, w.stats);
    line_pass(w.field, n, true, D2, 1, 1, 0, R * D1, D2, s);                     // axis 2: R * D1 lines, one after the other
    line_pass(w.field, n, false, D1, D2, R, (size_t)D1 * D2, D2, 1, s);          // axis 1: per r, D2 lines side by side
    line_pass(w.field, n, false, R, D1 * D2, 1, 0, D1 * D2, 1, s);               // axis 0: D1 * D2 lines side by side
    hipLaunchKernelGGL(hd_max_kernel, dim3(g), dim3(HB), 0, s, w.edges, w.field, (int)n, w.stats);
    hipLaunchKernelGGL(hd_finish_kernel, dim3(1), dim3(64), 0, s, w.stats, squeeze, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (edges_out && (e = hipMemcpyAsync(edges_out, w.edges, n, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    if (dist2_out && (e = hipMemcpyAsync(dist2_out, w.field, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToDevice, s)) != hipSuccess)
        return e;
    return hipSuccess;
}

}  // namespace cddpm
