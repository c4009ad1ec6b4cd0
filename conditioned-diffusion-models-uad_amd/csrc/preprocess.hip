// Raw volumes preprocessed on the device: what the reference's datamodule does per volume on the CPU before a volume is cached (Train) or
// handed to test_step (Eval, which has no cache): sitk_reader's CurvatureFlow (src/datamodules/create_dataset.py:252-258) and
// get_transform's CropOrPad, RescaleIntensity and Resample (:196-218). include/cddpm.h ("Preprocessed volumes") has the full rules; pinned
// to numpy / scipy, unpinned to torchio and SimpleITK, which are not available to compare with. In the reference's order, each stage gated
// by a bit of `stages`:
//   smooth     v <- v + dt u, u the mean-curvature speed from clamped central differences, evaluated in double, stored as fp32 per iteration
//   crop / pad a per-axis index shift with zeros outside: never a pass of its own, every later pass reads through the view
//   rescale    cutoffs = percentiles of vol[mask > 0] (exact radix select over order-preserving keys), clip, map [min, max] to [0, 1]
//   resample   cubic B-spline with mirror boundaries at x = (i + 1/2) f - 1/2, coefficients and taps in double; labels take the nearest voxel
// The input is torchio's [H][W][D] (D contiguous); the output is the bank's slice-major [D'][H'][W'] (W contiguous). The one transposing
// pass goes through an LDS tile, and every pass after it walks [D][H][W] in memory order. The B-spline prefilter runs in place on a double
// volume: along H and D one thread owns a line and neighbouring threads neighbouring lines (side by side along W); along W, the contiguous
// axis, a block stages whole lines in LDS as the distance transform of eval_hausdorff.hip does, so a wave is never strided across lines.
// Everything that crosses workgroups is an integer atomic (counts, histogram bins, min / max of keys): bitwise reproducible. Nothing
// allocates or synchronises; the digit of every radix pass is chosen by a device pass and the host reads no value back.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cddpm.h"
#include "kernels.h"

namespace cddpm {

namespace {

constexpr int PB = 256;                           // threads per block (4 waves)
constexpr int MAXL = CDDPM_PREP_MAX_AXIS;         // 1024
constexpr int VOX_BLOCKS = 2048;                  // grid.x bound of a volume pass; voxels beyond it loop
constexpr int BINS = 256;                         // one radix digit: 8 bits, 4 passes over a 32-bit key
constexpr int TILE_D = 6144;                      // doubles of LDS (48 KiB) of the contiguous-axis line pass
constexpr int HORIZON = 40;                       // |z|^40 < 2e-23: beyond it the mirror initial sum is below double precision

// integer state of a call
enum { ST_STATUS = 0, ST_COUNT = 1, ST_MINKEY = 2, ST_MAXKEY = 3, ST_PREFIX = 4, ST_RANK = 8, ST_WORDS = 16 };
// double state: the rescale's parameters
enum { RP_LO = 0, RP_HI = 1, RP_MIN = 2, RP_MAX = 3, RP_APPLY = 4, RP_WORDS = 8 };

struct PrepGeom {
    int H, W, D;          // the input
    int h1, w1, d1;       // after crop / pad
    int oh, ow, od;       // source index = view index + offset (negative where the axis is padded in front)
    int h2, w2, d2;       // after resample
};

struct PrepWs {
    int32_t* st;          // [ST_WORDS]
    int32_t* hist;        // [4][BINS]
    double* rp;           // [RP_WORDS]
    double* wt;           // [3][MAXL][4]: the spline weights of every output index per axis (0 = H, 1 = W, 2 = D)
    int32_t* ix;          // [3][MAXL][4]: the mirrored input indices; [..][0] = -1: the sample point is outside the extent
    float* flow[2];       // [n0] each: the curvature flow's two work volumes
    double* coef;         // [n1] as [d1][h1][w1]: the B-spline coefficients
};

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

bool resamples(int stages, double f) { return (stages & CDDPM_PREP_RESAMPLE) && f != 1.0; }

size_t layout(size_t n0, size_t n1, int stages, double f, char* base, PrepWs* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al(bytes); return p; };
    PrepWs t{};
    t.st = (int32_t*)take(sizeof(int32_t) * ST_WORDS);
    t.hist = (int32_t*)take(sizeof(int32_t) * 4 * BINS);
    t.rp = (double*)take(sizeof(double) * RP_WORDS);
    t.wt = (double*)take(sizeof(double) * 3 * MAXL * 4);
    t.ix = (int32_t*)take(sizeof(int32_t) * 3 * MAXL * 4);
    if (stages & CDDPM_PREP_SMOOTH) {
        t.flow[0] = (float*)take(sizeof(float) * n0);
        t.flow[1] = (float*)take(sizeof(float) * n0);
    }
    if (resamples(stages, f)) t.coef = (double*)take(sizeof(double) * n1);
    if (w) *w = t;
    return off;
}

int out_len(int N, double f) { return (int)ceil((double)N / f); }

PrepGeom geometry(int H, int W, int D, int stages, int th, int tw, int td, double f) {
    PrepGeom g{};
    g.H = H; g.W = W; g.D = D;
    g.h1 = H; g.w1 = W; g.d1 = D;
    if (stages & CDDPM_PREP_CROPPAD) {
        // delta = target - size: ceil(|delta| / 2) voxels are added (delta > 0) or removed (delta < 0) in front
        auto front = [](int target, int size) { const int d = target - size; return d >= 0 ? -((d + 1) / 2) : (-d + 1) / 2; };
        g.h1 = th; g.w1 = tw; g.d1 = td;
        g.oh = front(th, H); g.ow = front(tw, W); g.od = front(td, D);
    }
    g.h2 = g.h1; g.w2 = g.w1; g.d2 = g.d1;
    if (resamples(stages, f)) { g.h2 = out_len(g.h1, f); g.w2 = out_len(g.w1, f); g.d2 = out_len(g.d1, f); }
    return g;
}

// the source index of view voxel (h, w, d), or -1 in the padding
__device__ __forceinline__ int view_index(const PrepGeom& g, int h, int w, int d) {
    const int sh = h + g.oh, sw = w + g.ow, sd = d + g.od;
    if ((unsigned)sh >= (unsigned)g.H || (unsigned)sw >= (unsigned)g.W || (unsigned)sd >= (unsigned)g.D) return -1;
    return (sh * g.W + sw) * g.D + sd;
}

// order-preserving key of an fp32 value; -0.0 takes the key of +0.0 (the two compare equal: a selection may return either)
__device__ __forceinline__ uint32_t key_of(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool bad(const int32_t* st) { return (st[ST_STATUS] & CDDPM_PREP_BAD_VALUE) != 0; }

// ---- pass 0: the call's state; a non-finite input value ----------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void prep_init_kernel(PrepWs w) {
    const int t = threadIdx.x;
    if (t < ST_WORDS) w.st[t] = t == ST_MINKEY ? -1 : 0;      // min over unsigned keys starts at 0xffffffff
    for (int i = t; i < 4 * BINS; i += PB) w.hist[i] = 0;
    if (t < RP_WORDS) w.rp[t] = 0.0;
}

__global__ __launch_bounds__(PB) void prep_check_kernel(const float* __restrict__ vol, int n, int32_t* __restrict__ st) {
    bool nonfinite = false;
    for (int i = blockIdx.x * PB + threadIdx.x; i < n; i += gridDim.x * PB) nonfinite = nonfinite || !isfinite(vol[i]);
    if (__syncthreads_or(nonfinite) && threadIdx.x == 0) atomicOr(&st[ST_STATUS], CDDPM_PREP_BAD_VALUE);
}

// ---- pass 1 (once per iteration): curvature flow, [H][W][D], neighbours clamped to the edge ------------------------------------------
__global__ __launch_bounds__(PB) void prep_flow_kernel(const float* __restrict__ src, float* __restrict__ dst, PrepGeom g, double dt, double s0,
                                                       double s1, double s2, const int32_t* __restrict__ st) {
    if (bad(st)) return;
    const int WD = g.W * g.D, n = g.H * WD;
    for (int i = blockIdx.x * PB + threadIdx.x; i < n; i += gridDim.x * PB) {
        const int h = i / WD, w = (i - h * WD) / g.D, d = i - h * WD - w * g.D;
        const int hm = (h > 0 ? h - 1 : h) * WD, hp = (h < g.H - 1 ? h + 1 : h) * WD, h0 = h * WD;
        const int wm = (w > 0 ? w - 1 : w) * g.D, wp = (w < g.W - 1 ? w + 1 : w) * g.D, w0 = w * g.D;
        const int dm = d > 0 ? d - 1 : d, dp = d < g.D - 1 ? d + 1 : d;
        auto at = [&](int a, int b, int c) { return (double)src[a + b + c]; };
        const double v = at(h0, w0, d);
        const double ap = at(hp, w0, d), am = at(hm, w0, d), bp = at(h0, wp, d), bm = at(h0, wm, d), cp = at(h0, w0, dp), cm = at(h0, w0, dm);
        const double dx0 = 0.5 * (ap - am) * s0, dx1 = 0.5 * (bp - bm) * s1, dx2 = 0.5 * (cp - cm) * s2;
        const double dxx0 = (ap - 2.0 * v + am) * s0 * s0, dxx1 = (bp - 2.0 * v + bm) * s1 * s1, dxx2 = (cp - 2.0 * v + cm) * s2 * s2;
        const double dxy01 = 0.25 * (at(hp, wp, d) - at(hp, wm, d) - at(hm, wp, d) + at(hm, wm, d)) * s0 * s1;
        const double dxy02 = 0.25 * (at(hp, w0, dp) - at(hp, w0, dm) - at(hm, w0, dp) + at(hm, w0, dm)) * s0 * s2;
        const double dxy12 = 0.25 * (at(h0, wp, dp) - at(h0, wp, dm) - at(h0, wm, dp) + at(h0, wm, dm)) * s1 * s2;
        const double q0 = dx0 * dx0, q1 = dx1 * dx1, q2 = dx2 * dx2, m = q0 + q1 + q2;
        double u = 0.0;
        if (!(m < 1e-9))
            u = (dxx0 * (q1 + q2) + dxx1 * (q0 + q2) + dxx2 * (q0 + q1) - 2.0 * (dx0 * dx1 * dxy01 + dx0 * dx2 * dxy02 + dx1 * dx2 * dxy12)) / m;
        dst[i] = (float)(v + dt * u);
    }
}

// the mask of view voxel with source index j: the caller's, or vol > 0
__device__ __forceinline__ bool masked(const uint8_t* __restrict__ mask, const float* __restrict__ src, int j) {
    return j >= 0 && (mask ? mask[j] != 0 : src[j] > 0.f);
}

// ---- pass 2: mask count, min and max of the whole view (padding included) -------------------------------------------------------------
__global__ __launch_bounds__(PB) void prep_stats_kernel(const float* __restrict__ src, const uint8_t* __restrict__ mask, PrepGeom g,
                                                        int32_t* __restrict__ st) {
    __shared__ uint32_t s_min, s_max;
    __shared__ int s_cnt;
    if (bad(st)) return;
    if (threadIdx.x == 0) { s_min = 0xffffffffu; s_max = 0u; s_cnt = 0; }
    __syncthreads();
    const int wd = g.w1 * g.d1, n = g.h1 * wd;
    uint32_t lo = 0xffffffffu, hi = 0u;
    int cnt = 0;
    for (int i = blockIdx.x * PB + threadIdx.x; i < n; i += gridDim.x * PB) {
        const int h = i / wd, w = (i - h * wd) / g.d1, d = i - h * wd - w * g.d1;
        const int j = view_index(g, h, w, d);
        const uint32_t k = key_of(j >= 0 ? src[j] : 0.f);
        lo = min(lo, k);
        hi = max(hi, k);
        cnt += masked(mask, src, j) ? 1 : 0;
    }
    atomicMin(&s_min, lo);
    atomicMax(&s_max, hi);
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin((uint32_t*)&st[ST_MINKEY], s_min);
        atomicMax((uint32_t*)&st[ST_MAXKEY], s_max);
        if (s_cnt) atomicAdd(&st[ST_COUNT], s_cnt);
    }
}

// ---- pass 3 (four times): the histogram of one digit of the masked keys, for the four ranks at once ---------------------------------
__global__ __launch_bounds__(PB) void prep_hist_kernel(const float* __restrict__ src, const uint8_t* __restrict__ mask, PrepGeom g, PrepWs ws,
                                                       int pass) {
    __shared__ int sh[4 * BINS];
    if (bad(ws.st) || ws.st[ST_COUNT] == 0) return;
    for (int i = threadIdx.x; i < 4 * BINS; i += PB) sh[i] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    uint32_t prefix[4];
    for (int r = 0; r < 4; ++r) prefix[r] = (uint32_t)ws.st[ST_PREFIX + r];
    const int wd = g.w1 * g.d1, n = g.h1 * wd;
    for (int i = blockIdx.x * PB + threadIdx.x; i < n; i += gridDim.x * PB) {
        const int h = i / wd, w = (i - h * wd) / g.d1, d = i - h * wd - w * g.d1;
        const int j = view_index(g, h, w, d);
        if (!masked(mask, src, j)) continue;
        const uint32_t k = key_of(src[j]);
        const uint32_t high = pass == 0 ? 0u : k >> (shift + 8), digit = (k >> shift) & 255u;
        for (int r = 0; r < 4; ++r)
            if (high == prefix[r]) atomicAdd(&sh[r * BINS + digit], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * BINS; i += PB)
        if (sh[i]) atomicAdd(&ws.hist[i], sh[i]);
}

// the rank of order statistic r (0, 1: around the low percentile; 2, 3: around the high one) among n values, and the fraction between
__device__ __forceinline__ int rank_of(int r, int n, double perc, double* frac) {
    const double v = perc * (double)(n - 1) / 100.0;
    int k = (int)floor(v);
    if (k > n - 1) k = n - 1;
    if (frac) *frac = v - (double)k;
    return (r & 1) ? min(k + 1, n - 1) : k;
}

// ---- pass 4 (after every histogram): choose the digit of each rank on the device -----------------------------------------------------
__global__ __launch_bounds__(PB) void prep_select_kernel(PrepWs ws, int pass, double perc_lo, double perc_hi) {
    int32_t* st = ws.st;
    const int n = st[ST_COUNT];
    if (bad(st) || n == 0) return;
    const int r = threadIdx.x;
    if (r < 4) {
        int rank = pass == 0 ? rank_of(r, n, r < 2 ? perc_lo : perc_hi, nullptr) : st[ST_RANK + r];
        int below = 0, digit = BINS - 1;
        for (int b = 0; b < BINS; ++b) {
            const int c = ws.hist[r * BINS + b];
            if (rank < below + c) { digit = b; break; }
            below += c;
        }
        st[ST_RANK + r] = rank - below;
        st[ST_PREFIX + r] = (int32_t)((pass == 0 ? 0u : ((uint32_t)st[ST_PREFIX + r] << 8)) | (uint32_t)digit);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * BINS; i += PB) ws.hist[i] = 0;
}

// ---- pass 5: cutoffs and the affine map, in double; the record ---------------------------------------------------------------------
__device__ __forceinline__ double lerp_np(double a, double b, double t) {      // numpy's _lerp
    return t >= 0.5 ? b - (b - a) * (1.0 - t) : a + (b - a) * t;
}

__global__ void prep_finalize_kernel(PrepWs ws, int rescale, double perc_lo, double perc_hi, double* __restrict__ record) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int32_t* st = ws.st;
    double rec[CDDPM_PREP_RECORD];
    for (int i = 0; i < CDDPM_PREP_RECORD; ++i) rec[i] = 0.0;
    int status = st[ST_STATUS];
    if (rescale && !(status & CDDPM_PREP_BAD_VALUE)) {
        const int n = st[ST_COUNT];
        rec[CDDPM_PREP_REC_COUNT] = (double)n;
        const double vmin = (double)value_of((uint32_t)st[ST_MINKEY]), vmax = (double)value_of((uint32_t)st[ST_MAXKEY]);
        if (n == 0) {
            status |= CDDPM_PREP_BAD_MASK | CDDPM_PREP_UNCHANGED;
            rec[CDDPM_PREP_REC_MIN] = vmin;
            rec[CDDPM_PREP_REC_MAX] = vmax;
        } else {
            double q[4], frac[2];
            for (int r = 0; r < 4; ++r) q[r] = (double)value_of((uint32_t)st[ST_PREFIX + r]);
            rank_of(0, n, perc_lo, &frac[0]);
            rank_of(2, n, perc_hi, &frac[1]);
            const double lo = lerp_np(q[0], q[1], frac[0]), hi = lerp_np(q[2], q[3], frac[1]);
            const double mn = fmin(fmax(vmin, lo), hi), mx = fmin(fmax(vmax, lo), hi);      // min and max of the clipped volume
            for (int r = 0; r < 4; ++r) rec[CDDPM_PREP_REC_STAT + r] = q[r];
            rec[CDDPM_PREP_REC_CUT_LO] = lo;
            rec[CDDPM_PREP_REC_CUT_HI] = hi;
            rec[CDDPM_PREP_REC_MIN] = mn;
            rec[CDDPM_PREP_REC_MAX] = mx;
            if (mx == mn) {
                status |= CDDPM_PREP_BAD_RANGE | CDDPM_PREP_UNCHANGED;
            } else {
                ws.rp[RP_LO] = lo; ws.rp[RP_HI] = hi; ws.rp[RP_MIN] = mn; ws.rp[RP_MAX] = mx; ws.rp[RP_APPLY] = 1.0;
            }
        }
        st[ST_STATUS] = status;
    }
    rec[CDDPM_PREP_REC_STATUS] = (double)status;
    for (int i = 0; i < CDDPM_PREP_RECORD; ++i) record[i] = rec[i];
}

// ---- pass 6: the view, rescaled, into [d1][h1][w1]: fp32 (the output) or double (the spline's samples). One h per blockIdx.z; a
// 32 x 32 tile of the (w, d) plane is read along d and written along w ----------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PB) void prep_materialize_kernel(const float* __restrict__ src, PrepGeom g, PrepWs ws, T* __restrict__ dst) {
    __shared__ double tile[32][33];
    if (bad(ws.st)) return;
    const bool apply = ws.rp[RP_APPLY] != 0.0;
    const double lo = ws.rp[RP_LO], hi = ws.rp[RP_HI], mn = ws.rp[RP_MIN], range = ws.rp[RP_MAX] - ws.rp[RP_MIN];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;        // 32 x 8
    const int h = blockIdx.z, w0 = blockIdx.y * 32, d0 = blockIdx.x * 32;
    for (int r = 0; r < 32; r += 8) {
        const int w = w0 + ty + r, d = d0 + tx;
        if (w < g.w1 && d < g.d1) {
            const int j = view_index(g, h, w, d);
            const float x = j >= 0 ? src[j] : 0.f;
            double v = (double)x;
            if (apply) v = (fmin(fmax(v, lo), hi) - mn) / range;
            tile[ty + r][tx] = v;
        }
    }
    __syncthreads();
    for (int r = 0; r < 32; r += 8) {
        const int d = d0 + ty + r, w = w0 + tx;
        if (w < g.w1 && d < g.d1) dst[((size_t)d * g.h1 + h) * g.w1 + w] = (T)tile[tx][ty + r];
    }
}

// ---- pass 7 (once per axis): the B-spline prefilter of one line, in place, scipy's spline_filter1d(order 3, mode 'mirror') -----------
// c: the line, `stride` apart; n >= 2. gain, the causal sum from the mirror initial value, the anticausal sum.
template <typename Index>
__device__ __forceinline__ void spline_line(double* __restrict__ c, Index stride, int n) {
    const double z = -0.26794919243112270647;                      // sqrt(3) - 2
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    if (n < 2) return;                                                // scipy leaves a line of one sample as it is
    double c0;
    if (n <= HORIZON) {                                               // the whole mirrored line, as scipy sums it
        double zn = 1.0;
        for (int i = 0; i < n - 1; ++i) zn *= z;                     // z^(n-1)
        double zi = z;
        c0 = gain * c[0] + zn * (gain * c[(Index)(n - 1) * stride]);
        for (int i = 1; i < n - 1; ++i) {
            c0 += zi * (gain * c[(Index)i * stride] + zn * (gain * c[(Index)(n - 1 - i) * stride]));
            zi *= z;
        }
        c0 /= 1.0 - zn * zn;
    } else {
        double zi = 1.0;
        c0 = 0.0;
        for (int i = 0; i < HORIZON; ++i) { c0 += zi * (gain * c[(Index)i * stride]); zi *= z; }
    }
    c[0] = c0;
    double prev = c0;
    for (int i = 1; i < n; ++i) {
        prev = gain * c[(Index)i * stride] + z * prev;
        c[(Index)i * stride] = prev;
    }
    double next = (z / (z * z - 1.0)) * (z * c[(Index)(n - 2) * stride] + prev);
    c[(Index)(n - 1) * stride] = next;
    for (int i = n - 2; i >= 0; --i) {
        next = z * (next - c[(Index)i * stride]);
        c[(Index)i * stride] = next;
    }
}

// lines along H (stride w1) or D (stride h1 w1): line l of group o starts at o * os + l; neighbouring threads hold neighbouring lines
__global__ __launch_bounds__(PB) void prep_spline_strided_kernel(double* __restrict__ coef, int n, size_t stride, int inner, int outer, size_t os,
                                                                 const int32_t* __restrict__ st) {
    if (bad(st)) return;
    const long long lines = (long long)inner * outer;
    for (long long l = (long long)blockIdx.x * PB + threadIdx.x; l < lines; l += (long long)gridDim.x * PB)
        spline_line<size_t>(coef + (size_t)(l / inner) * os + (size_t)(l % inner), stride, n);
}

// lines along W, the contiguous axis: K whole lines of n staged in LDS (row stride odd: the K threads of the recursion hit K banks),
// loaded and stored in memory order by the whole block
__global__ __launch_bounds__(PB) void prep_spline_contig_kernel(double* __restrict__ coef, int n, long long lines, int K,
                                                                const int32_t* __restrict__ st) {
    __shared__ double tile[TILE_D];
    if (bad(st)) return;
    const int ls = n | 1;
    const long long tiles = (lines + K - 1) / K;
    for (long long id = blockIdx.x; id < tiles; id += gridDim.x) {
        const long long l0 = id * K;
        const int kc = (int)min((long long)K, lines - l0), cnt = kc * n;
        double* __restrict__ base = coef + (size_t)l0 * n;
        for (int e = threadIdx.x; e < cnt; e += PB) tile[(e / n) * ls + e % n] = base[e];
        __syncthreads();
        if ((int)threadIdx.x < kc) spline_line<int>(tile + threadIdx.x * ls, 1, n);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += PB) base[e] = tile[(e / n) * ls + e % n];
        __syncthreads();                                             // the next tile overwrites the LDS image
    }
}

// ---- pass 8: the four taps of every output index, per axis ---------------------------------------------------------------------------
__device__ __forceinline__ int mirror(int i, int N) {               // whole-sample symmetric (d c b | a b c d | c b a), N >= 2
    const int P = 2 * (N - 1);
    int m = i % P;
    if (m < 0) m += P;
    return m < N ? m : P - m;
}

__global__ __launch_bounds__(PB) void prep_taps_kernel(PrepGeom g, PrepWs ws, double f) {
    const int a = blockIdx.x;
    if (bad(ws.st)) return;
    const int N = a == 0 ? g.h1 : (a == 1 ? g.w1 : g.d1), M = a == 0 ? g.h2 : (a == 1 ? g.w2 : g.d2);
    for (int i = threadIdx.x; i < M; i += PB) {
        double* wt = ws.wt + ((size_t)a * MAXL + i) * 4;
        int32_t* ix = ws.ix + ((size_t)a * MAXL + i) * 4;
        const double x = ((double)i + 0.5) * f - 0.5;
        if (x < -0.5 || !(x < (double)N - 0.5)) {                    // outside the extent: the default pixel, 0
            for (int k = 0; k < 4; ++k) { wt[k] = 0.0; ix[k] = -1; }
            continue;
        }
        const double fl = floor(x), y = x - fl, t = 1.0 - y;
        wt[0] = t * t * t / 6.0;
        wt[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
        wt[2] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
        wt[3] = 1.0 - wt[0] - wt[1] - wt[2];
        for (int k = 0; k < 4; ++k) ix[k] = mirror((int)fl - 1 + k, N);
    }
}

// ---- pass 9: 64 taps in double, rounded once, [d2][h2][w2] -----------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void prep_spline_eval_kernel(PrepGeom g, PrepWs ws, float* __restrict__ out) {
    if (bad(ws.st)) return;
    const int hw = g.h2 * g.w2, n = hw * g.d2;
    const double* __restrict__ c = ws.coef;
    for (int o = blockIdx.x * PB + threadIdx.x; o < n; o += gridDim.x * PB) {
        const int d = o / hw, h = (o - d * hw) / g.w2, w = o - d * hw - h * g.w2;
        const int32_t* ih = ws.ix + ((size_t)0 * MAXL + h) * 4;
        const int32_t* iw = ws.ix + ((size_t)1 * MAXL + w) * 4;
        const int32_t* id = ws.ix + ((size_t)2 * MAXL + d) * 4;
        if (ih[0] < 0 || iw[0] < 0 || id[0] < 0) { out[o] = 0.f; continue; }
        const double* wh = ws.wt + ((size_t)0 * MAXL + h) * 4;
        const double* ww = ws.wt + ((size_t)1 * MAXL + w) * 4;
        const double* wd = ws.wt + ((size_t)2 * MAXL + d) * 4;
        double acc = 0.0;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b)
                for (int k = 0; k < 4; ++k)
                    acc += c[((size_t)id[k] * g.h1 + ih[a]) * g.w1 + iw[b]] * (wh[a] * ww[b] * wd[k]);
        out[o] = (float)acc;
    }
}

// ---- labels: crop / pad and the nearest voxel, [H][W][D] -> [d2][h2][w2] uint8. lab == NULL: the label is vol > 0 -----------------------
__global__ __launch_bounds__(PB) void prep_labels_kernel(const uint8_t* __restrict__ lab, const float* __restrict__ vol, PrepGeom g, double f,
                                                         int resample, const int32_t* __restrict__ st, uint8_t* __restrict__ out) {
    if (st && bad(st)) return;
    const int hw = g.h2 * g.w2, n = hw * g.d2;
    for (int o = blockIdx.x * PB + threadIdx.x; o < n; o += gridDim.x * PB) {
        int d = o / hw, h = (o - d * hw) / g.w2, w = o - d * hw - h * g.w2;
        bool inside = true;
        if (resample) {
            const double xh = ((double)h + 0.5) * f - 0.5, xw = ((double)w + 0.5) * f - 0.5, xd = ((double)d + 0.5) * f - 0.5;
            inside = xh >= -0.5 && xh < (double)g.h1 - 0.5 && xw >= -0.5 && xw < (double)g.w1 - 0.5 && xd >= -0.5 && xd < (double)g.d1 - 0.5;
            h = (int)floor(xh + 0.5); w = (int)floor(xw + 0.5); d = (int)floor(xd + 0.5);
        }
        uint8_t v = 0;
        if (inside) {
            const int j = view_index(g, min(h, g.h1 - 1), min(w, g.w1 - 1), min(d, g.d1 - 1));
            if (j >= 0) v = lab ? lab[j] : (uint8_t)(vol[j] > 0.f ? 1 : 0);
        }
        out[o] = v;
    }
}

int blocks_for(long long n) {
    const long long g = (n + PB - 1) / PB;
    return g < 1 ? 1 : (g > VOX_BLOCKS ? VOX_BLOCKS : (int)g);
}

}  // namespace

size_t prep_workspace_bytes(int H, int W, int D, int stages, int th, int tw, int td, double f) {
    const PrepGeom g = geometry(H, W, D, stages, th, tw, td, f);
    return layout((size_t)H * W * D, (size_t)g.h1 * g.w1 * g.d1, stages, f, nullptr, nullptr);
}

hipError_t launch_prep_volume(const float* vol, const uint8_t* mask, int H, int W, int D, int stages, int iterations, int th, int tw, int td,
                              const double* par, void* ws, size_t ws_bytes, float* out, uint8_t* mask_out, double* record, hipStream_t s) {
    const double f = par[CDDPM_PREP_PAR_FACTOR], plo = par[CDDPM_PREP_PAR_PERC_LO], phi = par[CDDPM_PREP_PAR_PERC_HI];
    const PrepGeom g = geometry(H, W, D, stages, th, tw, td, f);
    const size_t n0 = (size_t)H * W * D, n1 = (size_t)g.h1 * g.w1 * g.d1, n2 = (size_t)g.h2 * g.w2 * g.d2;      // each <= 2^30
    PrepWs w;
    if (layout(n0, n1, stages, f, (char*)ws, &w) > ws_bytes) return hipErrorInvalidValue;
    const dim3 blk(PB);
    hipLaunchKernelGGL(prep_init_kernel, dim3(1), blk, 0, s, w);
    hipLaunchKernelGGL(prep_check_kernel, dim3((unsigned)blocks_for((long long)n0)), blk, 0, s, vol, (int)n0, w.st);
    const float* src = vol;
    if (stages & CDDPM_PREP_SMOOTH) {
        for (int it = 0; it < iterations; ++it) {
            float* dst = w.flow[it & 1];
            hipLaunchKernelGGL(prep_flow_kernel, dim3((unsigned)blocks_for((long long)n0)), blk, 0, s, src, dst, g, par[CDDPM_PREP_PAR_DT],
                               1.0 / par[CDDPM_PREP_PAR_SPACING], 1.0 / par[CDDPM_PREP_PAR_SPACING + 1], 1.0 / par[CDDPM_PREP_PAR_SPACING + 2],
                               w.st);
            src = dst;
        }
    }
    const dim3 vox((unsigned)blocks_for((long long)n1));
    const int rescale = (stages & CDDPM_PREP_RESCALE) ? 1 : 0;
    if (rescale) {
        hipLaunchKernelGGL(prep_stats_kernel, vox, blk, 0, s, src, mask, g, w.st);
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(prep_hist_kernel, vox, blk, 0, s, src, mask, g, w, pass);
            hipLaunchKernelGGL(prep_select_kernel, dim3(1), blk, 0, s, w, pass, plo, phi);
        }
    }
    hipLaunchKernelGGL(prep_finalize_kernel, dim3(1), dim3(64), 0, s, w, rescale, plo, phi, record);
    const dim3 tiles((unsigned)((g.d1 + 31) / 32), (unsigned)((g.w1 + 31) / 32), (unsigned)g.h1);
    const bool rs = resamples(stages, f);
    if (!rs) {
        hipLaunchKernelGGL(prep_materialize_kernel<float>, tiles, blk, 0, s, src, g, w, out);
    } else {
        hipLaunchKernelGGL(prep_materialize_kernel<double>, tiles, blk, 0, s, src, g, w, w.coef);
        const size_t hw = (size_t)g.h1 * g.w1;
        // scipy's order of axes: 0 (H), 1 (W), 2 (D)
        hipLaunchKernelGGL(prep_spline_strided_kernel, dim3((unsigned)blocks_for((long long)g.w1 * g.d1)), blk, 0, s, w.coef, g.h1, (size_t)g.w1,
                           g.w1, g.d1, hw, w.st);
        const int K = min(PB, TILE_D / (g.w1 | 1));                    // >= 5 whole lines at 1024
        const long long lines = (long long)g.h1 * g.d1;
        const long long wt = (lines + K - 1) / K;
        hipLaunchKernelGGL(prep_spline_contig_kernel, dim3((unsigned)(wt > 4 * VOX_BLOCKS ? 4 * VOX_BLOCKS : wt)), blk, 0, s, w.coef, g.w1, lines, K,
                           w.st);
        hipLaunchKernelGGL(prep_spline_strided_kernel, dim3((unsigned)blocks_for((long long)hw)), blk, 0, s, w.coef, g.d1, hw, (int)hw, 1,
                           (size_t)0, w.st);
        hipLaunchKernelGGL(prep_taps_kernel, dim3(3), blk, 0, s, g, w, f);
        hipLaunchKernelGGL(prep_spline_eval_kernel, dim3((unsigned)blocks_for((long long)n2)), blk, 0, s, g, w, out);
    }
    if (mask_out)
        hipLaunchKernelGGL(prep_labels_kernel, dim3((unsigned)blocks_for((long long)n2)), blk, 0, s, mask, src, g, f, rs ? 1 : 0, w.st, mask_out);
    return hipGetLastError();
}

hipError_t launch_prep_labels(const uint8_t* lab, int H, int W, int D, int stages, int th, int tw, int td, double f, uint8_t* out,
                              hipStream_t s) {
    const PrepGeom g = geometry(H, W, D, stages, th, tw, td, f);
    const size_t n2 = (size_t)g.h2 * g.w2 * g.d2;
    hipLaunchKernelGGL(prep_labels_kernel, dim3((unsigned)blocks_for((long long)n2)), dim3(PB), 0, s, lab, (const float*)nullptr, g, f,
                       resamples(stages, f) ? 1 : 0, (const int32_t*)nullptr, out);
    return hipGetLastError();
}

}  // namespace cddpm
