// Augmented training slices drawn on the device from a bank of preprocessed volumes resident in HBM. Replaces what the reference's
// training datamodule does per item on the CPU (src/datamodules/create_dataset.py:220-250: get_augment -> torchio transforms on the
// whole volume; :143-193: vol2slice keeps one slice). Two entries share the kernels of this file:
//   cddpm_aug_slices     the policy group of `aug_intensity: True` (gamma, bias, blur, ghosting), one set of parameters per row
//   cddpm_aug_pipeline   get_augment's whole order as eleven gated slots: the individual bias, noise, ghosting, blur, gamma, the affine
//                        and the flip, then the policy group
// include/cddpm.h ("Augmented training slices", "The augmentation pipeline") has the full rules; pinned to numpy / scipy, unpinned to
// torchio, which is not available to compare with. The stages:
//   gamma      y = sign(x) |x|^gamma
//   bias       y = x exp(sum_i c_i X^a Y^b Z^c), coordinates u(i) = (2 i - L + 1) / (L - 1) per axis
//   blur       scipy.ndimage.gaussian_filter: separable, axis 0 (H), 1 (W), 2 (D), reflect boundary, double line sums, fp32 between passes
//   ghosting   y = x - I (c (*) x), a circular convolution along one axis with the comb kernel c; the policy slot, the last stage, is
//              evaluated at the output slice only, the individual slot at every voxel
//   noise      y = x + std n(v), n(v) the Box-Muller normal of voxel v's two Philox uniforms
//   affine     y(p) = trilinear(x, c + M (p - c)) inside the volume, min(x) outside; with the flip, at the mirrored p
// The bank is [N][D][H][W] fp32, so a slice is a contiguous [H][W] image and neighbouring lines along H and D sit side by side along W.
// Every pass gives one thread one output voxel and walks the volume in memory order: whatever the axis of the pass, the 2 r + 1 loads of
// a wave are 2 r + 1 runs along W, and the re-use between neighbouring outputs is the cache's (r <= 32, a line pass here needs no whole
// line in LDS as the distance transform of eval_hausdorff.hip does); the gather's eight loads per voxel are eight runs along W bent by
// at most 10 degrees. Every stage computes in double and rounds once. A pass that runs reads the volume the last one wrote (the bank
// where none ran) and writes the sample's other work volume: the first kernel lays that down per sample as a plan, one source per pass.
// A sample's arithmetic depends on its own table row only and runs in a fixed order: the result is bitwise independent of the batch
// around it. Nothing allocates or synchronises; a sample whose table row is out of range is flagged by the first kernel, which reads
// the two tables only, and no later kernel touches the bank, the workspace volumes or the output for it.
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
constexpr uint32_t NOISE_STREAM = 0x6002u;        // counter word 3 of the noise stage (augment.STREAM_AUG_NOISE)

// the passes of a sample, in order; plan[pass] is the volume the pass reads (0 = the bank volume, 1 / 2 = the work volumes), -1 when
// the pass does not run. cddpm_aug_slices uses the policy group's passes only.
enum { PL_BIAS, PL_NOISE, PL_GHOST, PL_BLUR, PL_GAMMA = PL_BLUR + 3, PL_GEOM, PL_POLICY, PL_POLICY_BLUR, PL_OUT = PL_POLICY_BLUR + 3, NPASS = 16 };

// one set of gamma / bias / blur / ghosting parameters of a table row: its flag bits, its first par column (the columns of a set
// follow CDDPM_AUG_PAR_*) and the meta column of its g | axis << 8
struct AugSet { int gamma, bias, blur, ghost, par0, ghost_col; };
// a table layout: row lengths, the known flag bits, and its sets -- the last one is the policy group; pipe: set[0] is the individual slots
struct AugTab { int meta_n, par_n, all, nsets, pipe; AugSet set[2]; };

constexpr AugTab SLICES_TAB = {CDDPM_AUG_META, CDDPM_AUG_PAR, CDDPM_AUG_ALL, 1, 0,
                               {{CDDPM_AUG_GAMMA, CDDPM_AUG_BIAS, CDDPM_AUG_BLUR, CDDPM_AUG_GHOST, 0, 3}, {0, 0, 0, 0, 0, 0}}};
constexpr AugTab PIPE_TAB = {CDDPM_PIPE_META, CDDPM_PIPE_PAR, CDDPM_PIPE_ALL, 2, 1,
                             {{CDDPM_PIPE_GAMMA, CDDPM_PIPE_BIAS, CDDPM_PIPE_BLUR, CDDPM_PIPE_GHOST, CDDPM_PIPE_PAR_SLOT, CDDPM_PIPE_META_GHOST},
                              {CDDPM_PIPE_POLICY_GAMMA, CDDPM_PIPE_POLICY_BIAS, CDDPM_PIPE_POLICY_BLUR, CDDPM_PIPE_POLICY_GHOST, CDDPM_PIPE_PAR_POLICY,
                               CDDPM_PIPE_META_POLICY_GHOST}}};

struct AugWs {
    int32_t* status;     // [B]: 0, or the CDDPM_AUG_BAD_* bits of the sample's table row
    int32_t* plan;       // [B][NPASS]: the source volume of every pass
    int32_t* radius;     // [B][nsets][4]: blur radius per axis (-1: the pass is skipped), [3]: 1 when the ghosting stage runs
    double* weights;     // [B][nsets][3][NW]: normalised one-sided Gaussian weights
    double* comb;        // [B][nsets][MAXL]: the ghosting kernel c[0 .. L)
    uint32_t* minkey;    // [B]: the minimum of the volume the affine reads, as an order-preserving key
    float* vol;          // [B][2][n]: the two work volumes of a sample
};

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

size_t layout(size_t B, size_t n, size_t nsets, char* base, AugWs* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al(bytes); return p; };
    AugWs t{};
    t.status = (int32_t*)take(sizeof(int32_t) * B);
    t.plan = (int32_t*)take(sizeof(int32_t) * NPASS * B);
    t.radius = (int32_t*)take(sizeof(int32_t) * 4 * nsets * B);
    t.weights = (double*)take(sizeof(double) * 3 * NW * nsets * B);
    t.comb = (double*)take(sizeof(double) * MAXL * nsets * B);
    t.minkey = (uint32_t*)take(sizeof(uint32_t) * B);
    t.vol = (float*)take(sizeof(float) * 2 * n * B);
    if (w) *w = t;
    return off;
}

struct AugGeom { int N, H, W, D; };

__device__ __forceinline__ int axis_len(const AugGeom& g, int ax) { return ax == 0 ? g.H : (ax == 1 ? g.W : g.D); }

__device__ __forceinline__ const float* volume_ptr(int which, const float* bank, int volume, float* ws_vol, int b, size_t n) {
    return which == 0 ? bank + (size_t)volume * n : ws_vol + ((size_t)b * 2 + (which - 1)) * n;
}

// the work volume a pass writes: the one it does not read
__device__ __forceinline__ float* other_ptr(int which, float* ws_vol, int b, size_t n) {
    return ws_vol + ((size_t)b * 2 + (which == 1 ? 1 : 0)) * n;
}

// scipy's `reflect` (d c b a | a b c d | d c b a), as repeated reflection: valid for any distance from the line
__device__ __forceinline__ int reflect(int i, int L) {
    int m = i % (2 * L);
    if (m < 0) m += 2 * L;
    return m >= L ? 2 * L - 1 - m : m;
}

// floats as unsigned keys of the same order, for an integer (exact, order-free) minimum
__device__ __forceinline__ uint32_t min_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool set_ghost_on(const AugSet& s, int flags, const int32_t* m, const float* p) {
    return (flags & s.ghost) && (m[s.ghost_col] & 0xff) > 0 && p[s.par0 + CDDPM_AUG_PAR_INTENSITY] != 0.f;
}
__device__ __forceinline__ bool set_blur_on(const AugSet& s, int flags, const float* p, int ax) {
    return (flags & s.blur) && (double)p[s.par0 + CDDPM_AUG_PAR_SIGMA + ax] > 1e-15;
}

// ---- pass 0: check the sample's table row; its plan; the blur weights and the ghosting combs, in double ---------------------------
__global__ __launch_bounds__(AB) void aug_prepare_kernel(const int32_t* __restrict__ meta, const float* __restrict__ par, AugGeom g,
                                                         AugWs w, AugTab tab) {
    __shared__ int s_bad;
    const int b = blockIdx.x, t = threadIdx.x;
    const int32_t* m = meta + (size_t)b * tab.meta_n;
    const float* p = par + (size_t)b * tab.par_n;
    const int volume = m[0], z = m[1], flags = m[2];
    if (t == 0) {
        int bad = 0;
        if (volume < 0 || volume >= g.N) bad |= CDDPM_AUG_BAD_VOLUME;
        if (z < 0 || z >= g.D) bad |= CDDPM_AUG_BAD_Z;
        if (flags & ~tab.all) bad |= CDDPM_AUG_BAD_FLAGS;
        bool finite = true;
        for (int si = 0; si < tab.nsets; ++si) {
            const AugSet& s = tab.set[si];
            const int axis = m[s.ghost_col] >> 8;
            if (axis < 0 || axis > 2) bad |= CDDPM_AUG_BAD_AXIS;
            for (int ax = 0; ax < 3; ++ax) {
                const float sg = p[s.par0 + CDDPM_AUG_PAR_SIGMA + ax];
                if (!(sg >= 0.f && sg <= (float)CDDPM_AUG_MAX_SIGMA)) bad |= CDDPM_AUG_BAD_SIGMA;
            }
            finite = finite && isfinite(p[s.par0 + CDDPM_AUG_PAR_GAMMA]) && isfinite(p[s.par0 + CDDPM_AUG_PAR_INTENSITY]);
            for (int i = 0; i < CDDPM_AUG_BIAS_COEFS; ++i) finite = finite && isfinite(p[s.par0 + CDDPM_AUG_PAR_COEF + i]);
        }
        if (tab.pipe)
            for (int i = CDDPM_PIPE_PAR_NOISE_STD; i < CDDPM_PIPE_PAR_MATRIX + 9; ++i) finite = finite && isfinite(p[i]);
        if (!finite) bad |= CDDPM_AUG_BAD_VALUE;
        s_bad = bad;
        w.status[b] = bad;
        if (!bad) {
            int32_t* plan = w.plan + (size_t)b * NPASS;
            int cur = 0;
            auto step = [&](int pass, bool on) {
                plan[pass] = on ? cur : -1;
                if (on) cur = cur == 1 ? 2 : 1;
            };
            if (tab.pipe) {
                const AugSet& s = tab.set[0];
                step(PL_BIAS, flags & s.bias);
                step(PL_NOISE, (flags & CDDPM_PIPE_NOISE) && p[CDDPM_PIPE_PAR_NOISE_STD] != 0.f);
                step(PL_GHOST, set_ghost_on(s, flags, m, p));
                for (int ax = 0; ax < 3; ++ax) step(PL_BLUR + ax, set_blur_on(s, flags, p, ax));
                step(PL_GAMMA, flags & s.gamma);
                step(PL_GEOM, flags & (CDDPM_PIPE_AFFINE | CDDPM_PIPE_FLIP));
                w.minkey[b] = 0xffffffffu;
            }
            const AugSet& s = tab.set[tab.nsets - 1];
            step(PL_POLICY, flags & (s.gamma | s.bias));
            for (int ax = 0; ax < 3; ++ax) step(PL_POLICY_BLUR + ax, set_blur_on(s, flags, p, ax));
            plan[PL_OUT] = cur;
        }
    }
    __syncthreads();
    if (s_bad) return;
    if (t < 3 * tab.nsets) {                                  // one thread per set and axis: at most 33 weights
        const int si = t / 3, ax = t - 3 * si;
        const AugSet& s = tab.set[si];
        const double sigma = (double)p[s.par0 + CDDPM_AUG_PAR_SIGMA + ax];
        int r = -1;
        if ((flags & s.blur) && sigma > 1e-15) {
            r = (int)(4.0 * sigma + 0.5);                     // <= 32 for sigma <= 8
            double* wt = w.weights + (((size_t)b * tab.nsets + si) * 3 + ax) * NW;
            double sum = 0.0;
            for (int k = -r; k <= r; ++k) sum += exp(-0.5 / (sigma * sigma) * (double)(k * k));
            for (int k = 0; k <= r; ++k) wt[k] = exp(-0.5 / (sigma * sigma) * (double)(k * k)) / sum;
        }
        w.radius[((size_t)b * tab.nsets + si) * 4 + ax] = r;
    }
    for (int si = 0; si < tab.nsets; ++si) {
        const AugSet& s = tab.set[si];
        const bool ghost = set_ghost_on(s, flags, m, p);
        if (t == 3) w.radius[((size_t)b * tab.nsets + si) * 4 + 3] = ghost ? 1 : 0;
        if (!ghost) continue;
        const int gh = m[s.ghost_col] & 0xff, axis = m[s.ghost_col] >> 8;
        const int L = axis_len(g, axis), half = L / 2;
        double* c = w.comb + ((size_t)b * tab.nsets + si) * MAXL;
        for (int d = t; d < L; d += AB) {
            double acc = 0.0;
            for (int sp = 0; sp < L; sp += gh) {
                if (sp == half) continue;                     // the DC plane is restored
                int a = ((sp - half) * d) % L;                // |(s - half) d| < 2^20: exact; the argument is reduced in integers
                if (a < 0) a += L;
                acc += cospi(2.0 * (double)a / (double)L);
            }
            c[d] = acc / (double)L;
        }
    }
}

// ---- gamma and bias field, one pointwise pass in double, rounded once: the stages whose bits are in gmask / bmask ------------------
__device__ __forceinline__ double coord(int i, int L) { return L == 1 ? 0.0 : (double)(2 * i - L + 1) / (double)(L - 1); }

__global__ __launch_bounds__(AB) void aug_pointwise_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta,
                                                           const float* __restrict__ par, AugGeom g, AugWs w, int meta_n, int par_n, int pass,
                                                           int gmask, int bmask, int par0) {
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int from = w.plan[(size_t)b * NPASS + pass];
    if (from < 0) return;
    const int32_t* m = meta + (size_t)b * meta_n;
    const int flags = m[2];
    const float* p = par + (size_t)b * par_n + par0;
    const int HW = g.H * g.W, n = HW * g.D;
    const float* __restrict__ src = volume_ptr(from, bank, m[0], w.vol, b, (size_t)n);
    float* __restrict__ dst = other_ptr(from, w.vol, b, (size_t)n);
    const double gamma = (double)p[CDDPM_AUG_PAR_GAMMA];
    double coef[CDDPM_AUG_BIAS_COEFS];
    for (int i = 0; i < CDDPM_AUG_BIAS_COEFS; ++i) coef[i] = (double)p[CDDPM_AUG_PAR_COEF + i];
    for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
        double v = (double)src[i];
        if (flags & gmask) {
            const double a = pow(fabs(v), gamma);
            v = v > 0.0 ? a : (v < 0.0 ? -a : v);
        }
        if (flags & bmask) {
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

// ---- (once per axis): one Gaussian line pass of set `si`, in scipy's order of summation --------------------------------------------
__global__ __launch_bounds__(AB) void aug_blur_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta, AugGeom g, AugWs w,
                                                      int meta_n, int nsets, int si, int ax, int pass) {
    __shared__ double sw[NW];
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int from = w.plan[(size_t)b * NPASS + pass];
    if (from < 0) return;
    const int r = w.radius[((size_t)b * nsets + si) * 4 + ax];
    const int32_t* m = meta + (size_t)b * meta_n;
    const int HW = g.H * g.W, n = HW * g.D;
    const float* __restrict__ src = volume_ptr(from, bank, m[0], w.vol, b, (size_t)n);
    float* __restrict__ dst = other_ptr(from, w.vol, b, (size_t)n);
    if ((int)threadIdx.x <= r) sw[threadIdx.x] = w.weights[(((size_t)b * nsets + si) * 3 + ax) * NW + threadIdx.x];
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

// y = x - I (c (*) x) at voxel i, position pos of its line of length L
__device__ __forceinline__ float ghost_at(const float* __restrict__ vol, int i, int pos, int L, int stride, const double* __restrict__ c,
                                          double I) {
    const float x = vol[i];
    const float* __restrict__ line = vol + (i - pos * stride);
    double acc = 0.0;
    int k = pos;                                              // (pos - j) mod L, kept in [0, L)
    for (int j = 0; j < L; ++j) {
        acc += c[k] * (double)line[j * stride];
        k = k == 0 ? L - 1 : k - 1;
    }
    return (float)((double)x - I * acc);
}

// ---- the policy group's ghosting at the output slice, and the slice itself ---------------------------------------------------------
__global__ __launch_bounds__(AB) void aug_ghost_extract_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta,
                                                               const float* __restrict__ par, AugGeom g, AugWs w, float* __restrict__ out,
                                                               int meta_n, int par_n, int nsets, int si, int par0, int ghost_col) {
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int32_t* m = meta + (size_t)b * meta_n;
    const int HW = g.H * g.W, z = m[1], axis = m[ghost_col] >> 8;
    const size_t n = (size_t)HW * g.D;
    const float* __restrict__ vol = volume_ptr(w.plan[(size_t)b * NPASS + PL_OUT], bank, m[0], w.vol, b, n);
    const bool ghost = w.radius[((size_t)b * nsets + si) * 4 + 3] != 0;
    const double I = (double)par[(size_t)b * par_n + par0 + CDDPM_AUG_PAR_INTENSITY];
    const double* __restrict__ c = w.comb + ((size_t)b * nsets + si) * MAXL;
    const int L = axis_len(g, axis), stride = axis == 0 ? g.W : (axis == 1 ? 1 : HW);
    float* __restrict__ o = out + (size_t)b * HW;
    for (int p = blockIdx.x * AB + threadIdx.x; p < HW; p += gridDim.x * AB) {
        const int i = z * HW + p;
        if (!ghost) { o[p] = vol[i]; continue; }              // flags without ghosting: the slice as the passes left it, bit for bit
        const int h = p / g.W, xw = p - h * g.W;
        o[p] = ghost_at(vol, i, axis == 0 ? h : (axis == 1 ? xw : z), L, stride, c, I);
    }
}

// ---- the individual ghosting slot: the same rule at every voxel, since later stages read them all -----------------------------------
__global__ __launch_bounds__(AB) void aug_ghost_volume_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta,
                                                              const float* __restrict__ par, AugGeom g, AugWs w) {
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int from = w.plan[(size_t)b * NPASS + PL_GHOST];
    if (from < 0) return;
    const int32_t* m = meta + (size_t)b * CDDPM_PIPE_META;
    const int HW = g.H * g.W, n = HW * g.D, axis = m[CDDPM_PIPE_META_GHOST] >> 8;
    const float* __restrict__ vol = volume_ptr(from, bank, m[0], w.vol, b, (size_t)n);
    float* __restrict__ dst = other_ptr(from, w.vol, b, (size_t)n);
    const double I = (double)par[(size_t)b * CDDPM_PIPE_PAR + CDDPM_PIPE_PAR_SLOT + CDDPM_AUG_PAR_INTENSITY];
    const double* __restrict__ c = w.comb + ((size_t)b * 2 + 0) * MAXL;
    const int L = axis_len(g, axis), stride = axis == 0 ? g.W : (axis == 1 ? 1 : HW);
    for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
        const int d = i / HW, h = (i - d * HW) / g.W, x = i - d * HW - h * g.W;
        dst[i] = ghost_at(vol, i, axis == 0 ? h : (axis == 1 ? x : d), L, stride, c, I);
    }
}

// ---- noise: y = x + std n(v), v the voxel's index in memory order ------------------------------------------------------------------
// Philox4x32-10 (the generator of small_kernels.hip and synth.py) keyed by the row's two key words at counter (v / 4, 0, 0, 0x6002);
// lane v % 4 of the quad takes cos / sin of the first pair or cos / sin of the second, as synth.normal_quads orders them. The normal
// is evaluated in double from the two fp32 uniforms.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ double u01d(uint32_t x) { return (double)(((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f)); }

__global__ __launch_bounds__(AB) void aug_noise_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta,
                                                       const float* __restrict__ par, AugGeom g, AugWs w) {
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int from = w.plan[(size_t)b * NPASS + PL_NOISE];
    if (from < 0) return;
    const int32_t* m = meta + (size_t)b * CDDPM_PIPE_META;
    const int n = g.H * g.W * g.D;
    const float* __restrict__ src = volume_ptr(from, bank, m[0], w.vol, b, (size_t)n);
    float* __restrict__ dst = other_ptr(from, w.vol, b, (size_t)n);
    const uint32_t k0 = (uint32_t)m[CDDPM_PIPE_META_KEY], k1 = (uint32_t)m[CDDPM_PIPE_META_KEY + 1];
    const double sd = (double)par[(size_t)b * CDDPM_PIPE_PAR + CDDPM_PIPE_PAR_NOISE_STD];
    for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
        uint32_t r[4];
        philox4x32_10((uint32_t)(i >> 2), 0u, 0u, NOISE_STREAM, k0, k1, r);
        const int lane = i & 3;
        const double ua = u01d(r[lane & 2]), ub = u01d(r[(lane & 2) + 1]);
        const double rad = sqrt(-2.0 * log(ua));
        const double nv = rad * ((lane & 1) ? sinpi(2.0 * ub) : cospi(2.0 * ub));
        dst[i] = (float)((double)src[i] + sd * nv);
    }
}

// ---- the minimum of the volume the affine reads: exact and order-free, an integer minimum over keys ---------------------------------
__global__ __launch_bounds__(AB) void aug_min_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta, AugGeom g, AugWs w) {
    __shared__ uint32_t s_key[AB / 64];
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int from = w.plan[(size_t)b * NPASS + PL_GEOM];
    const int32_t* m = meta + (size_t)b * CDDPM_PIPE_META;
    if (from < 0 || !(m[2] & CDDPM_PIPE_AFFINE)) return;
    const int n = g.H * g.W * g.D;
    const float* __restrict__ src = volume_ptr(from, bank, m[0], w.vol, b, (size_t)n);
    uint32_t key = 0xffffffffu;
    for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
        const uint32_t k = min_key(src[i]);
        key = k < key ? k : key;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)key, off, 64);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < AB / 64; ++k) key = s_key[k] < key ? s_key[k] : key;
        atomicMin(w.minkey + b, key);
    }
}

// ---- affine and flip, one gather: output voxel p takes the affine's sample at flip(p) ----------------------------------------------
__global__ __launch_bounds__(AB) void aug_geometry_kernel(const float* __restrict__ bank, const int32_t* __restrict__ meta,
                                                          const float* __restrict__ par, AugGeom g, AugWs w) {
    const int b = blockIdx.y;
    if (w.status[b]) return;
    const int from = w.plan[(size_t)b * NPASS + PL_GEOM];
    if (from < 0) return;
    const int32_t* m = meta + (size_t)b * CDDPM_PIPE_META;
    const int flags = m[2];
    const int HW = g.H * g.W, n = HW * g.D;
    const float* __restrict__ src = volume_ptr(from, bank, m[0], w.vol, b, (size_t)n);
    float* __restrict__ dst = other_ptr(from, w.vol, b, (size_t)n);
    const bool flip = flags & CDDPM_PIPE_FLIP, affine = flags & CDDPM_PIPE_AFFINE;
    double M[9];
    for (int k = 0; k < 9; ++k) M[k] = (double)par[(size_t)b * CDDPM_PIPE_PAR + CDDPM_PIPE_PAR_MATRIX + k];
    const float lowest = affine ? key_value(w.minkey[b]) : 0.f;
    const double c0 = 0.5 * (double)(g.H - 1), c1 = 0.5 * (double)(g.W - 1), c2 = 0.5 * (double)(g.D - 1);
    for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
        const int d = i / HW, hh = (i - d * HW) / g.W, x = i - d * HW - hh * g.W;
        const int h = flip ? g.H - 1 - hh : hh;
        if (!affine) { dst[i] = src[d * HW + h * g.W + x]; continue; }
        const double p0 = (double)h - c0, p1 = (double)x - c1, p2 = (double)d - c2;
        const double q0 = c0 + (M[0] * p0 + M[1] * p1 + M[2] * p2);
        const double q1 = c1 + (M[3] * p0 + M[4] * p1 + M[5] * p2);
        const double q2 = c2 + (M[6] * p0 + M[7] * p1 + M[8] * p2);
        if (!(q0 >= -0.5 && q0 <= (double)g.H - 0.5 && q1 >= -0.5 && q1 <= (double)g.W - 0.5 && q2 >= -0.5 && q2 <= (double)g.D - 0.5)) {
            dst[i] = lowest;
            continue;
        }
        const double f0 = floor(q0), f1 = floor(q1), f2 = floor(q2);
        const double t0 = q0 - f0, t1 = q1 - f1, t2 = q2 - f2;
        const int a0 = min(max((int)f0, 0), g.H - 1), b0 = min(max((int)f0 + 1, 0), g.H - 1);
        const int a1 = min(max((int)f1, 0), g.W - 1), b1 = min(max((int)f1 + 1, 0), g.W - 1);
        const int a2 = min(max((int)f2, 0), g.D - 1), b2 = min(max((int)f2 + 1, 0), g.D - 1);
        auto at = [&](int ih, int iw, int id) { return (double)src[id * HW + ih * g.W + iw]; };
        const double lo = (at(a0, a1, a2) * (1.0 - t1) + at(a0, b1, a2) * t1) * (1.0 - t0) + (at(b0, a1, a2) * (1.0 - t1) + at(b0, b1, a2) * t1) * t0;
        const double hi = (at(a0, a1, b2) * (1.0 - t1) + at(a0, b1, b2) * t1) * (1.0 - t0) + (at(b0, a1, b2) * (1.0 - t1) + at(b0, b1, b2) * t1) * t0;
        dst[i] = (float)(lo * (1.0 - t2) + hi * t2);
    }
}

int blocks_for(long long n) {
    const long long g = (n + AB - 1) / AB;
    return g < 1 ? 1 : (g > VOX_BLOCKS ? VOX_BLOCKS : (int)g);
}

// the policy group of table `t` (its last set): gamma and bias together, the blur, the ghosting at the slice
void launch_policy(const float* bank, const int32_t* meta, const float* par, int B, const AugGeom& g, const AugWs& w, const AugTab& t,
                   float* out, hipStream_t s) {
    const int si = t.nsets - 1;
    const AugSet& set = t.set[si];
    const dim3 vox((unsigned)blocks_for((long long)g.H * g.W * g.D), (unsigned)B), pix((unsigned)blocks_for((long long)g.H * g.W), (unsigned)B);
    hipLaunchKernelGGL(aug_pointwise_kernel, vox, dim3(AB), 0, s, bank, meta, par, g, w, t.meta_n, t.par_n, (int)PL_POLICY, set.gamma, set.bias,
                       set.par0);
    for (int ax = 0; ax < 3; ++ax)
        hipLaunchKernelGGL(aug_blur_kernel, vox, dim3(AB), 0, s, bank, meta, g, w, t.meta_n, t.nsets, si, ax, (int)PL_POLICY_BLUR + ax);
    hipLaunchKernelGGL(aug_ghost_extract_kernel, pix, dim3(AB), 0, s, bank, meta, par, g, w, out, t.meta_n, t.par_n, t.nsets, si, set.par0,
                       set.ghost_col);
}

}  // namespace

size_t aug_workspace_bytes(int B, int H, int W, int D) { return layout((size_t)B, (size_t)H * W * D, 1, nullptr, nullptr); }

size_t aug_pipeline_workspace_bytes(int B, int H, int W, int D) { return layout((size_t)B, (size_t)H * W * D, 2, nullptr, nullptr); }

hipError_t launch_aug_slices(const float* bank, int N, int H, int W, int D, const int32_t* meta, const float* par, int B, void* ws,
                             size_t ws_bytes, float* out, hipStream_t s) {
    const size_t n = (size_t)H * W * D;                       // <= 2^30: voxel indices of one volume fit an int
    AugWs w;
    if (layout((size_t)B, n, 1, (char*)ws, &w) > ws_bytes) return hipErrorInvalidValue;
    const AugGeom g{N, H, W, D};
    hipLaunchKernelGGL(aug_prepare_kernel, dim3((unsigned)B), dim3(AB), 0, s, meta, par, g, w, SLICES_TAB);
    launch_policy(bank, meta, par, B, g, w, SLICES_TAB, out, s);
    return hipGetLastError();
}

hipError_t launch_aug_pipeline(const float* bank, int N, int H, int W, int D, const int32_t* meta, const float* par, int B, void* ws,
                               size_t ws_bytes, float* out, hipStream_t s) {
    const size_t n = (size_t)H * W * D;
    AugWs w;
    if (layout((size_t)B, n, 2, (char*)ws, &w) > ws_bytes) return hipErrorInvalidValue;
    const AugGeom g{N, H, W, D};
    const AugTab& t = PIPE_TAB;
    const AugSet& slot = t.set[0];
    const dim3 vox((unsigned)blocks_for((long long)n), (unsigned)B), blk(AB);
    hipLaunchKernelGGL(aug_prepare_kernel, dim3((unsigned)B), blk, 0, s, meta, par, g, w, t);
    hipLaunchKernelGGL(aug_pointwise_kernel, vox, blk, 0, s, bank, meta, par, g, w, t.meta_n, t.par_n, (int)PL_BIAS, 0, slot.bias, slot.par0);
    hipLaunchKernelGGL(aug_noise_kernel, vox, blk, 0, s, bank, meta, par, g, w);
    hipLaunchKernelGGL(aug_ghost_volume_kernel, vox, blk, 0, s, bank, meta, par, g, w);
    for (int ax = 0; ax < 3; ++ax) hipLaunchKernelGGL(aug_blur_kernel, vox, blk, 0, s, bank, meta, g, w, t.meta_n, t.nsets, 0, ax, (int)PL_BLUR + ax);
    hipLaunchKernelGGL(aug_pointwise_kernel, vox, blk, 0, s, bank, meta, par, g, w, t.meta_n, t.par_n, (int)PL_GAMMA, slot.gamma, 0, slot.par0);
    hipLaunchKernelGGL(aug_min_kernel, vox, blk, 0, s, bank, meta, g, w);
    hipLaunchKernelGGL(aug_geometry_kernel, vox, blk, 0, s, bank, meta, par, g, w);
    launch_policy(bank, meta, par, B, g, w, t, out, s);
    return hipGetLastError();
}

}  // namespace cddpm
