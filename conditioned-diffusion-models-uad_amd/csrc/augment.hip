// Augmented training slices drawn on the device from a bank of preprocessed volumes resident in HBM. Replaces, for the experiments'
// `aug_intensity: True`, what the reference's training datamodule does per item on the CPU (src/datamodules/create_dataset.py:220-250:
// get_augment -> torchio's RandomGamma, RandomBiasField, RandomBlur, RandomGhosting on the whole volume; :143-193: vol2slice keeps one
// slice). include/cddpm.h ("Augmented training slices") has the full rules; pinned to numpy / scipy, unpinned to torchio, which is not
// available to compare with. Per sample, in Compose's order, each stage gated by a bit of the sample's flags:
//   gamma      y = sign(x) |x|^gamma
//   bias       y = x exp(sum_i c_i X^a Y^b Z^c), coordinates u(i) = (2 i - L + 1) / (L - 1) per axis
//   blur       scipy.ndimage.gaussian_filter: separable, axis 0 (H), 1 (W), 2 (D), reflect boundary, double line sums, fp32 between passes
//   ghosting   y = x - I (c (*) x), a circular convolution along one axis with the comb kernel c; evaluated at the output slice only
// The bank is [N][D][H][W] fp32, so a slice is a contiguous [H][W] image and neighbouring lines along H and D sit side by side along W.
// Every pass gives one thread one output voxel and walks the volume in memory order: whatever the axis of the pass, the 2 r + 1 loads of
// a wave are 2 r + 1 runs along W, and the re-use between neighbouring outputs is the cache's (r <= 32, a line pass here needs no whole
// line in LDS as the distance transform of eval_hausdorff.hip does). gamma and bias are one pass in double, rounded once. A sample's
// arithmetic depends on its own table row only and runs in a fixed order: the result is bitwise independent of the batch around it.
// Nothing allocates or synchronises; a sample whose table row is out of range is flagged by the first kernel, which reads the two tables
// only, and no later kernel touches the bank, the workspace volumes or the output for it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cddpm.h"
#include "kernels.h"

namespace cddpm {

namespace {

constexpr int AB = 256;                           // threads per block (4 waves)
constexpr int MAXR = CDDPM_AUG_MAX_RADIUS;        // 32: sigma_voxel <= 8
constexpr int MAXL = CDDPM_AUG_MAX_AXIS;          // 1024
constexpr int NW = MAXR + 1;                      // one-sided weights w[0 .. r]
constexpr int VOX_BLOCKS = 2048;                  // grid.x bound of a volume pass; voxels beyond it loop

struct AugWs {
    int32_t* status;     // [B]: 0, or the CDDPM_AUG_BAD_* bits of the sample's table row
    int32_t* radius;     // [B][4]: blur radius per axis (-1: the pass is skipped), [3]: 1 when the ghosting stage runs
    double* weights;     // [B][3][NW]: normalised one-sided Gaussian weights
    double* comb;        // [B][MAXL]: the ghosting kernel c[0 .. L)
    float* vol;          // [B][2][n]: the two work volumes of a sample
};

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

size_t layout(size_t B, size_t n, char* base, AugWs* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al(bytes); return p; };
    AugWs t{};
    t.status = (int32_t*)take(sizeof(int32_t) * B);
    t.radius = (int32_t*)take(sizeof(int32_t) * 4 * B);
    t.weights = (double*)take(sizeof(double) * 3 * NW * B);
    t.comb = (double*)take(sizeof(double) * MAXL * B);
    t.vol = (float*)take(sizeof(float) * 2 * n * B);
    if (w) *w = t;
    return off;
}

struct AugGeom { int N, H, W, D; };

__device__ __forceinline__ int axis_len(const AugGeom& g, int ax) { return ax == 0 ? g.H : (ax == 1 ? g.W : g.D); }

// where a sample's volume is before blur pass `upto` (3: after the last): 0 = its bank volume, 1 / 2 = its work volumes.
// The pointwise pass writes volume 1; every blur pass that runs writes the volume it does not read.
__device__ __forceinline__ int volume_before(int flags, const int32_t* rad, int upto) {
    int cur = (flags & (CDDPM_AUG_GAMMA | CDDPM_AUG_BIAS)) ? 1 : 0;
    for (int ax = 0; ax < upto; ++ax)
        if (rad[ax] >= 0) cur = cur == 2 ? 1 : 2;
    return cur;
}

__device__ __forceinline__ const float* volume_ptr(int which, const float* bank, int volume, float* ws_vol, int b, size_t n) {
    return which == 0 ? bank + (size_t)volume * n : ws_vol + ((size_t)b * 2 + (which - 1)) * n;
}

// scipy's `reflect` (d c b a | a b c d | d c b a), as repeated reflection: valid for any distance from the line
__device__ __forceinline__ int reflect(int i, int L) {
    int m = i % (2 * L);
    if (m < 0) m += 2 * L;
    return m >= L ? 2 * L - 1 - m : m;
}

// ---- pass 0: check the sample's table row; the blur weights and the ghosting comb, in double ------------------------------------
__global__ __launch_bounds__(AB) void aug_prepare_kernel(const int32_t* __restrict__ meta, const float* __restrict__ par, AugGeom g,
                                                         AugWs w) {
    __shared__ int s_bad;
    const int b = blockIdx.x, t = threadIdx.x;
    const int32_t* m = meta + (size_t)b * CDDPM_AUG_META;
    const float* p = par + (size_t)b * CDDPM_AUG_PAR;
    const int volume = m[0], z = m[1], flags = m[2], gh = m[3] & 0xff, axis = m[3] >> 8;
    if (t == 0) {
        int bad = 0;
        if (volume < 0 || volume >= g.N) bad |= CDDPM_AUG_BAD_VOLUME;
        if (z < 0 || z >= g.D) bad |= CDDPM_AUG_BAD_Z;
        if (axis < 0 || axis > 2) bad |= CDDPM_AUG_BAD_AXIS;
        if (flags & ~CDDPM_AUG_ALL) bad |= CDDPM_AUG_BAD_FLAGS;
        for (int ax = 0; ax < 3; ++ax)
            if (!(p[CDDPM_AUG_PAR_SIGMA + ax] >= 0.f && p[CDDPM_AUG_PAR_SIGMA + ax] <= (float)CDDPM_AUG_MAX_SIGMA)) bad |= CDDPM_AUG_BAD_SIGMA;
        bool finite = isfinite(p[CDDPM_AUG_PAR_GAMMA]) && isfinite(p[CDDPM_AUG_PAR_INTENSITY]);
        for (int i = 0; i < CDDPM_AUG_BIAS_COEFS; ++i) finite = finite && isfinite(p[CDDPM_AUG_PAR_COEF + i]);
        if (!finite) bad |= CDDPM_AUG_BAD_VALUE;
        s_bad = bad;
        w.status[b] = bad;
    }
    __syncthreads();
    if (s_bad) return;
    if (t < 3) {                                              // one thread per axis: at most 33 weights
        const double sigma = (double)p[CDDPM_AUG_PAR_SIGMA + t];
        int r = -1;
        if ((flags & CDDPM_AUG_BLUR) && sigma > 1e-15) {
            r = (int)(4.0 * sigma + 0.5);                     // <= 32 for sigma <= 8
            double* wt = w.weights + ((size_t)b * 3 + t) * NW;
            double sum = 0.0;
            for (int k = -r; k <= r; ++k) sum += exp(-0.5 / (sigma * sigma) * (double)(k * k));
            for (int k = 0; k <= r; ++k) wt[k] = exp(-0.5 / (sigma * sigma) * (double)(k * k)) / sum;
        }
        w.radius[b * 4 + t] = r;
    }
    const bool ghost = (flags & CDDPM_AUG_GHOST) && gh > 0 && p[CDDPM_AUG_PAR_INTENSITY] != 0.f;
    if (t == 3) w.radius[b * 4 + 3] = ghost ? 1 : 0;
    if (!ghost) return;
    const int L = axis_len(g, axis), half = L / 2;
    double* c = w.comb + (size_t)b * MAXL;
    for (int d = t; d < L; d += AB) {
        double acc = 0.0;
        for (int s = 0; s < L; s += gh) {
            if (s == half) continue;                          // the DC plane is restored
            int a = ((s - half) * d) % L;                     // |(s - half) d| < 2^20: exact; the argument is reduced in integers
            if (a < 0) a += L;
            acc += cospi(2.0 * (double)a / (double)L);
        }
        c[d] = acc / (double)L;
    }
}

// ---- pass 1: gamma and bias field, one pointwise pass in double, rounded once -----------------------------------------------------
__device__ __forceinline__ double coord(int i, int L) { return L == 1 ? 0.0 : (double)(2 * i - L + 1) / (double)(L - 1); }

__global__ __launch_bounds__(AB) void aug_pointwise_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta,
                                                           const float* __restrict__ par, AugGeom g, AugWs w) {
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int32_t* m = meta + (size_t)b * CDDPM_AUG_META;
    const int flags = m[2];
    if (!(flags & (CDDPM_AUG_GAMMA | CDDPM_AUG_BIAS))) return;
    const float* p = par + (size_t)b * CDDPM_AUG_PAR;
    const int HW = g.H * g.W, n = HW * g.D;
    const float* __restrict__ src = bank + (size_t)m[0] * n;
    float* __restrict__ dst = w.vol + (size_t)b * 2 * n;
    const double gamma = (double)p[CDDPM_AUG_PAR_GAMMA];
    double coef[CDDPM_AUG_BIAS_COEFS];
    for (int i = 0; i < CDDPM_AUG_BIAS_COEFS; ++i) coef[i] = (double)p[CDDPM_AUG_PAR_COEF + i];
    for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
        double v = (double)src[i];
        if (flags & CDDPM_AUG_GAMMA) {
            const double a = pow(fabs(v), gamma);
            v = v > 0.0 ? a : (v < 0.0 ? -a : v);
        }
        if (flags & CDDPM_AUG_BIAS) {
            const int d = i / HW, h = (i - d * HW) / g.W, x = i - d * HW - h * g.W;
            double px[4], py[4], pz[4];                       // powers by repeated multiplication: 0^0 = 1
            px[0] = py[0] = pz[0] = 1.0;
            const double X = coord(h, g.H), Y = coord(x, g.W), Z = coord(d, g.D);
            for (int k = 1; k < 4; ++k) { px[k] = px[k - 1] * X; py[k] = py[k - 1] * Y; pz[k] = pz[k - 1] * Z; }
            double field = 0.0;
            int k = 0;
            for (int a = 0; a < 4; ++a)
                for (int bb = 0; bb < 4 - a; ++bb)
                    for (int c = 0; c < 4 - a - bb; ++c) field += coef[k++] * px[a] * py[bb] * pz[c];
            v *= exp(field);
        }
        dst[i] = (float)v;
    }
}

// ---- pass 2 (once per axis): one Gaussian line pass, in scipy's order of summation -------------------------------------------------
__global__ __launch_bounds__(AB) void aug_blur_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta, AugGeom g, AugWs w,
                                                      int ax) {
    __shared__ double sw[NW];
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int32_t* rad = w.radius + b * 4;
    const int r = rad[ax];
    if (r < 0) return;
    const int32_t* m = meta + (size_t)b * CDDPM_AUG_META;
    const int HW = g.H * g.W, n = HW * g.D;
    const int from = volume_before(m[2], rad, ax);
    const float* __restrict__ src = volume_ptr(from, bank, m[0], w.vol, b, (size_t)n);
    float* __restrict__ dst = w.vol + ((size_t)b * 2 + (from == 2 ? 0 : 1)) * n;
    if ((int)threadIdx.x <= r) sw[threadIdx.x] = w.weights[((size_t)b * 3 + ax) * NW + threadIdx.x];
    __syncthreads();
    const int L = axis_len(g, ax), stride = ax == 0 ? g.W : (ax == 1 ? 1 : HW);
    for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
        const int d = i / HW, h = (i - d * HW) / g.W, x = i - d * HW - h * g.W;
        const int c = ax == 0 ? h : (ax == 1 ? x : d);
        const float* __restrict__ line = src + (i - c * stride);
        double acc = (double)line[c * stride] * sw[0];
        for (int k = r; k >= 1; --k)                          // the outermost pair first, as scipy's symmetric correlate1d
            acc += ((double)line[reflect(c - k, L) * stride] + (double)line[reflect(c + k, L) * stride]) * sw[k];
        dst[i] = (float)acc;
    }
}

// ---- pass 3: ghosting at the output slice, and the slice itself -------------------------------------------------------------------
__global__ __launch_bounds__(AB) void aug_ghost_extract_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta,
                                                               const float* __restrict__ par, AugGeom g, AugWs w, float* __restrict__ out) {
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int32_t* rad = w.radius + b * 4;
    const int32_t* m = meta + (size_t)b * CDDPM_AUG_META;
    const int HW = g.H * g.W, z = m[1], axis = m[3] >> 8;
    const size_t n = (size_t)HW * g.D;
    const float* __restrict__ vol = volume_ptr(volume_before(m[2], rad, 3), bank, m[0], w.vol, b, n);
    const bool ghost = rad[3] != 0;
    const double I = (double)par[(size_t)b * CDDPM_AUG_PAR + CDDPM_AUG_PAR_INTENSITY];
    const double* __restrict__ c = w.comb + (size_t)b * MAXL;
    const int L = axis_len(g, axis), stride = axis == 0 ? g.W : (axis == 1 ? 1 : HW);
    float* __restrict__ o = out + (size_t)b * HW;
    for (int p = blockIdx.x * AB + threadIdx.x; p < HW; p += gridDim.x * AB) {
        const int i = z * HW + p;
        const float x = vol[i];
        if (!ghost) { o[p] = x; continue; }                   // flags without ghosting: the slice as the passes left it, bit for bit
        const int h = p / g.W, xw = p - h * g.W;
        const int pos = axis == 0 ? h : (axis == 1 ? xw : z);
        const float* __restrict__ line = vol + (i - pos * stride);
        double acc = 0.0;
        int k = pos;                                          // (pos - j) mod L, kept in [0, L)
        for (int j = 0; j < L; ++j) {
            acc += c[k] * (double)line[j * stride];
            k = k == 0 ? L - 1 : k - 1;
        }
        o[p] = (float)((double)x - I * acc);
    }
}

int blocks_for(long long n) {
    const long long g = (n + AB - 1) / AB;
    return g < 1 ? 1 : (g > VOX_BLOCKS ? VOX_BLOCKS : (int)g);
}

}  // namespace

size_t aug_workspace_bytes(int B, int H, int W, int D) { return layout((size_t)B, (size_t)H * W * D, nullptr, nullptr); }

hipError_t launch_aug_slices(const float* bank, int N, int H, int W, int D, const int32_t* meta, const float* par, int B, void* ws,
                             size_t ws_bytes, float* out, hipStream_t s) {
    const size_t n = (size_t)H * W * D;                       // <= 2^30: voxel indices of one volume fit an int
    AugWs w;
    if (layout((size_t)B, n, (char*)ws, &w) > ws_bytes) return hipErrorInvalidValue;
    const AugGeom g{N, H, W, D};
    const dim3 vox((unsigned)blocks_for((long long)n), (unsigned)B), pix((unsigned)blocks_for((long long)H * W), (unsigned)B);
    hipLaunchKernelGGL(aug_prepare_kernel, dim3((unsigned)B), dim3(AB), 0, s, meta, par, g, w);
    hipLaunchKernelGGL(aug_pointwise_kernel, vox, dim3(AB), 0, s, bank, meta, par, g, w);
    for (int ax = 0; ax < 3; ++ax) hipLaunchKernelGGL(aug_blur_kernel, vox, dim3(AB), 0, s, bank, meta, g, w, ax);
    hipLaunchKernelGGL(aug_ghost_extract_kernel, pix, dim3(AB), 0, s, bank, meta, par, g, w, out);
    return hipGetLastError();
}

}  // namespace cddpm
