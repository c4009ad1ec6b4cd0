// Training BatchNorm over NHWC fp32 tensors, forward and backward: the one implementation behind cddpm_op_enc_bn_* (the context encoder's
// ResNet-50, encoder_training.py) and cddpm_op_spark_bn_* (the sparse encoder, densify and decoder of SparK pre-training, spark_training.py).
//   y = act((active ? bn(z) : fill) s[b] + res), act = none | ReLU | ReLU6, s[b]: stochastic-depth scale of the residual branch per sample
// Options: a cell mask (active [B][f][f]: statistics over the ACTIVE pixels only, reference spark/encoder.py:25-35, n_act counted on the
// device), a fill value for the inactive pixels, evaluation mode (running statistics). Pieces:
//   bn_chan_partial / the two folds   per-channel sums of a pixel chunk in fp64, folded in the order of the chunks: batch statistics
//                          (+ running statistics as torch, momentum, unbiased variance) and the sums of the backward
//   bn_eval_stats          evaluation mode: the running statistics stand in for the batch's
//   bn_act / bn_bwd_apply  the two elementwise passes
// What differs between the two entry pairs is the caller's (cddpm_ops.hip): the number of pixel chunks (it fixes the order of the fp64
// sums and the grid), the planes per chunk of the backward's scratch (2 without a mask, 3 with the sum over inactive pixels for dfill),
// and whether fewer than two values per channel are reported (`status`) or folded. Nothing here uses float atomics.
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace cddpm {

// g *= the slope of ReLU (act 1) / ReLU6 (act 2) at the outputs y; act 0 is the caller's branch. ReLU is four selects, as in a
// ReLU-only kernel; ReLU6's cap is four more behind one uniform branch
__device__ __forceinline__ void bn_act_grad(float (&g)[4], const float (&y)[4], int act) {
    for (int i = 0; i < 4; ++i) g[i] = y[i] > 0.f ? g[i] : 0.f;
    if (act == 2)
        for (int i = 0; i < 4; ++i) g[i] = y[i] < 6.f ? g[i] : 0.f;
}
struct BnTrain {                      // what every call reads comes first, in one stretch of the argument block; the mask's fields last
    const float *z, *y, *dy, *mr, *sscale;
    double* part;                     // [nchunk][planes][C]
    long long N;
    int HW, C, act;
    int nchunk, planes;               // pixel chunks; backward: planes per chunk of `part` (2: no mask; 3: the last holds the sums over inactive pixels)
    int qpb, rows;                    // channel quads per workgroup; pixel lanes per workgroup (qpb rows <= 256)
    const unsigned char* active;      // [B][f][f] or nullptr (every pixel active)
    int f, ch, cw, W;                 // cells per side; pixels per cell: ch = H / f, cw = W / f; the row length
};
template <bool MASKED>
__device__ __forceinline__ bool bn_pixel_active(const BnTrain& a, long long p) {
    if (!MASKED) return true;
    const int b = (int)(p / a.HW), rem = (int)(p - (long long)b * a.HW);
    const int y = rem / a.W, x = rem - y * a.W;
    return a.active[((size_t)b * a.f + y / a.ch) * a.f + x / a.cw] != 0;
}
// per-channel sums over the pixels of one chunk, fp64: workgroup = (pixel chunk, qpb channel quads), thread = (channel quad, pixel lane).
// MODE 0: (sum z, sum z^2) over active pixels. MODE 1: g = dy act'(y) s[b]; (sum g, sum g zhat) over active pixels, zhat = (z - mean) rstd,
// and with a mask (sum g) over inactive ones. Q16 (C a multiple of 64): 16 quads x 16 lanes at compile time, the general plan's own split there
template <int MODE, bool MASKED, bool Q16>
__global__ __launch_bounds__(256) void bn_chan_partial_kernel(const BnTrain a) {
    constexpr int NS = (MODE == 1 && MASKED) ? 3 : 2;
    __shared__ double red[NS][16 * (64 + 1)];
    const int qpb = Q16 ? 16 : a.qpb, rows = Q16 ? 16 : a.rows, cw4 = qpb * 4, ld = Q16 ? 64 + 1 : cw4;
    const int planes = MODE == 0 ? 2 : a.planes;
    const int tid = threadIdx.x, q = tid % qpb, r = tid / qpb;
    const int c = (blockIdx.y * qpb + q) * 4;
    const bool valid = Q16 || (r < rows && c < a.C);
    const long long per = (a.N + a.nchunk - 1) / a.nchunk, p0 = per * blockIdx.x, p1 = p0 + per < a.N ? p0 + per : a.N;
    double s[NS][4];
    for (int j = 0; j < NS; ++j)
        for (int i = 0; i < 4; ++i) s[j][i] = 0.0;
    if (valid) {
        float mean[4] = {0, 0, 0, 0}, rstd[4] = {1, 1, 1, 1};
        if (MODE == 1)
            for (int i = 0; i < 4; ++i) { mean[i] = a.mr[c + i]; rstd[i] = a.mr[a.C + c + i]; }
        for (long long p = p0 + r; p < p1; p += rows) {
            const bool on = bn_pixel_active<MASKED>(a, p);
            if (MODE == 0) {
                if (!on) continue;
                const float4 zv = *reinterpret_cast<const float4*>(a.z + (size_t)p * a.C + c);
                const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
                for (int i = 0; i < 4; ++i) { s[0][i] += zz[i]; s[1][i] += (double)zz[i] * zz[i]; }
            } else {
                float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);          // z and dy are asked for together: one round trip, not two
                if (on) zv = *reinterpret_cast<const float4*>(a.z + (size_t)p * a.C + c);
                const float4 dv = *reinterpret_cast<const float4*>(a.dy + (size_t)p * a.C + c);
                float gg[4] = {dv.x, dv.y, dv.z, dv.w};
                if (a.act) {
                    const float4 yv = *reinterpret_cast<const float4*>(a.y + (size_t)p * a.C + c);
                    const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
                    bn_act_grad(gg, yy, a.act);
                }
                const float sc = a.sscale ? a.sscale[p / a.HW] : 1.f;
                if (on) {
                    const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
                    for (int i = 0; i < 4; ++i) {
                        const float g = gg[i] * sc;
                        s[0][i] += g;
                        s[1][i] += (double)g * ((zz[i] - mean[i]) * rstd[i]);
                    }
                } else {
                    for (int i = 0; i < 4; ++i) s[NS - 1][i] += gg[i] * sc;
                }
            }
        }
    }
    if (Q16 || r < rows)
        for (int j = 0; j < NS; ++j)
            for (int i = 0; i < 4; ++i) red[j][r * ld + 4 * q + i] = s[j][i];
    __syncthreads();
    if (tid < NS * cw4) {
        const int w = tid / cw4, cc = tid - w * cw4, ch = blockIdx.y * cw4 + cc;
        if (Q16 || ch < a.C) {
            double t = 0;
            for (int k = 0; k < rows; ++k) t += red[w][k * ld + cc];
            a.part[((size_t)blockIdx.x * planes + w) * a.C + ch] = t;
        }
    }
}
// batch statistics over the n active pixels (N without a mask): mr = (mean | rstd); running statistics as torch's BatchNorm in training
// mode (momentum, unbiased variance). n < 2: with `status` nothing is written but status = {1, n} (torch's BatchNorm1d raises there);
// without it, a single value per channel folds its biased variance
template <bool MASKED>
__global__ __launch_bounds__(256) void bn_stats_fold_kernel(const double* __restrict__ part, int nchunk, int C, long long N,
                                                            const unsigned char* __restrict__ active, int ncell, int cellpx, float eps, float momentum,
                                                            float* __restrict__ mr, float* __restrict__ run_mean, float* __restrict__ run_var,
                                                            int* __restrict__ status) {
    long long n = N;
    if (MASKED) {
        __shared__ int red[256];
        n = (long long)count_active_cells(active, ncell, red) * cellpx;
    }
    if (status) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { status[0] = n < 2; status[1] = (int)n; }
        if (n < 2) return;
    }
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0, s1 = 0;
    for (int k = 0; k < nchunk; ++k) { s0 += part[((size_t)k * 2) * C + c]; s1 += part[((size_t)k * 2 + 1) * C + c]; }
    const double mean = s0 / (double)n;
    double var = s1 / (double)n - mean * mean;
    if (var < 0) var = 0;
    mr[c] = (float)mean;
    mr[C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) {
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
        const double unb = n > 1 ? var * (double)n / (double)(n - 1) : var;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
    }
}
__global__ __launch_bounds__(256) void bn_eval_stats_kernel(const float* __restrict__ run_mean, const float* __restrict__ run_var, float eps, int C,
                                                            float* __restrict__ mr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    mr[c] = run_mean[c];
    mr[C + c] = (float)(1.0 / sqrt((double)run_var[c] + (double)eps));
}
template <bool MASKED>
__global__ __launch_bounds__(256) void bn_act_kernel(const BnTrain a, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     const float* __restrict__ fill, const float* __restrict__ res, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nq = a.C >> 2;
    if (e >= a.N * nq) return;
    const int c = 4 * (int)(e % nq);
    const long long p = e / nq;
    float4 o;
    if (bn_pixel_active<MASKED>(a, p)) {
        const float4 zv = *reinterpret_cast<const float4*>(a.z + (size_t)p * a.C + c);
        const float4 m = *reinterpret_cast<const float4*>(a.mr + c), rs = *reinterpret_cast<const float4*>(a.mr + a.C + c);
        const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
        o.x = (zv.x - m.x) * rs.x * g.x + b.x; o.y = (zv.y - m.y) * rs.y * g.y + b.y;
        o.z = (zv.z - m.z) * rs.z * g.z + b.z; o.w = (zv.w - m.w) * rs.w * g.w + b.w;
    } else {
        o = fill ? *reinterpret_cast<const float4*>(fill + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float sc = a.sscale ? a.sscale[p / a.HW] : 1.f;
    o.x *= sc; o.y *= sc; o.z *= sc; o.w *= sc;
    if (res) {
        const float4 rv = *reinterpret_cast<const float4*>(res + (size_t)p * a.C + c);
        o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w;
    }
    if (a.act) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    if (a.act == 2) { o.x = fminf(o.x, 6.f); o.y = fminf(o.y, 6.f); o.z = fminf(o.z, 6.f); o.w = fminf(o.w, 6.f); }
    *reinterpret_cast<float4*>(out + (size_t)p * a.C + c) = o;
}
// backward sums -> dgamma, dbeta, dfill and the two per-channel means of the elementwise pass (k = (sum g / n | sum g zhat / n) over the n
// active pixels; both 0 in evaluation mode, where the statistics do not depend on z)
template <bool MASKED>
__global__ __launch_bounds__(256) void bn_bwd_fold_kernel(const double* __restrict__ part, int nchunk, int planes, int C, long long N,
                                                          const unsigned char* __restrict__ active, int ncell, int cellpx, int training,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dfill,
                                                          float* __restrict__ k) {
    long long n = N;
    if (MASKED) {
        __shared__ int red[256];
        n = (long long)count_active_cells(active, ncell, red) * cellpx;
    }
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int j = 0; j < nchunk; ++j) {
        s0 += part[((size_t)j * planes) * C + c]; s1 += part[((size_t)j * planes + 1) * C + c];
        if (MASKED) s2 += part[((size_t)j * planes + 2) * C + c];
    }
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
    if (dfill) dfill[c] = (float)s2;
    const bool stats = training && n > 0;
    k[c] = stats ? (float)(s0 / (double)n) : 0.f;
    k[C + c] = stats ? (float)(s1 / (double)n) : 0.f;
}
// dz = active ? gamma rstd (g - k0 - zhat k1) : 0, g = dy act'(y) s[b]; dres (optional) = dy act'(y): the gradient of the shortcut operand
template <bool MASKED>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnTrain a, const float* __restrict__ gamma, const float* __restrict__ k,
                                                           float* __restrict__ dz, float* __restrict__ dres) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nq = a.C >> 2;
    if (e >= a.N * nq) return;
    const int c = 4 * (int)(e % nq);
    const long long p = e / nq;
    float4 dv = *reinterpret_cast<const float4*>(a.dy + (size_t)p * a.C + c);
    if (a.act) {
        const float4 yv = *reinterpret_cast<const float4*>(a.y + (size_t)p * a.C + c);
        const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
        float gg[4] = {dv.x, dv.y, dv.z, dv.w};
        bn_act_grad(gg, yy, a.act);
        dv = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bn_pixel_active<MASKED>(a, p)) {
        const float sc = a.sscale ? a.sscale[p / a.HW] : 1.f;
        const float4 zv = *reinterpret_cast<const float4*>(a.z + (size_t)p * a.C + c);
        const float4 m = *reinterpret_cast<const float4*>(a.mr + c), rs = *reinterpret_cast<const float4*>(a.mr + a.C + c);
        const float4 g = *reinterpret_cast<const float4*>(gamma + c);
        const float4 k0 = *reinterpret_cast<const float4*>(k + c), k1 = *reinterpret_cast<const float4*>(k + a.C + c);
        o.x = g.x * rs.x * (dv.x * sc - k0.x - (zv.x - m.x) * rs.x * k1.x);
        o.y = g.y * rs.y * (dv.y * sc - k0.y - (zv.y - m.y) * rs.y * k1.y);
        o.z = g.z * rs.z * (dv.z * sc - k0.z - (zv.z - m.z) * rs.z * k1.z);
        o.w = g.w * rs.w * (dv.w * sc - k0.w - (zv.w - m.w) * rs.w * k1.w);
    }
    if (dres) *reinterpret_cast<float4*>(dres + (size_t)p * a.C + c) = dv;      // both stores after every load: none of them waits for a store
    *reinterpret_cast<float4*>(dz + (size_t)p * a.C + c) = o;
}

static BnTrain bn_train_args(const BnShape& g, const float* z, const float* y, const float* dy, const float* mr, const float* sscale, int act,
                             int nchunk, int planes, double* part) {
    BnTrain a;
    a.z = z; a.y = y; a.dy = dy; a.mr = mr; a.sscale = sscale; a.active = g.active; a.f = g.f;
    a.ch = g.active ? g.H / g.f : 1; a.cw = g.active ? g.W / g.f : 1;
    a.W = g.W; a.HW = g.HW; a.C = g.C; a.act = act; a.N = g.N; a.nchunk = nchunk;
    a.qpb = g.C / 4 < 16 ? g.C / 4 : 16; a.rows = 256 / a.qpb; a.planes = planes; a.part = part;
    return a;
}
template <int MODE>
static void launch_bn_chan_partial(const BnTrain& a, hipStream_t s) {
    const dim3 grid(a.nchunk, (a.C / 4 + a.qpb - 1) / a.qpb);
    const bool q16 = a.C % 64 == 0;
    if (a.active) {
        if (q16) hipLaunchKernelGGL((bn_chan_partial_kernel<MODE, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((bn_chan_partial_kernel<MODE, true, false>), grid, dim3(256), 0, s, a);
    } else {
        if (q16) hipLaunchKernelGGL((bn_chan_partial_kernel<MODE, false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((bn_chan_partial_kernel<MODE, false, false>), grid, dim3(256), 0, s, a);
    }
}
static int bn_cells(const BnShape& g) { return g.active ? (int)(g.N / g.HW) * g.f * g.f : 0; }
static int bn_cell_pixels(const BnShape& g) { return g.active ? (g.H / g.f) * (g.W / g.f) : 1; }

void launch_bn_train_stats(const BnShape& g, const float* z, int nchunk, float eps, float momentum, float* run_mean, float* run_var, float* mr,
                           double* part, int* status, hipStream_t s) {
    const BnTrain a = bn_train_args(g, z, nullptr, nullptr, nullptr, nullptr, 0, nchunk, 2, part);
    launch_bn_chan_partial<0>(a, s);
    const auto fold = g.active ? bn_stats_fold_kernel<true> : bn_stats_fold_kernel<false>;
    hipLaunchKernelGGL(fold, dim3((g.C + 255) / 256), dim3(256), 0, s, part, nchunk, g.C, g.N, g.active, bn_cells(g), bn_cell_pixels(g), eps, momentum, mr,
                       run_mean, run_var, status);
}
void launch_bn_eval_stats(const float* run_mean, const float* run_var, float eps, int C, float* mr, hipStream_t s) {
    hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, s, run_mean, run_var, eps, C, mr);
}
void launch_bn_train_act(const BnShape& g, const float* z, const float* mr, const float* gamma, const float* beta, const float* sscale,
                         const float* res, const float* fill, int act, float* y, hipStream_t s) {
    const BnTrain a = bn_train_args(g, z, nullptr, nullptr, mr, sscale, act, 0, 0, nullptr);
    const dim3 grid((unsigned)((g.N * (g.C / 4) + 255) / 256));
    if (g.active) hipLaunchKernelGGL(bn_act_kernel<true>, grid, dim3(256), 0, s, a, gamma, beta, fill, res, y);
    else hipLaunchKernelGGL(bn_act_kernel<false>, grid, dim3(256), 0, s, a, gamma, beta, fill, res, y);
}
void launch_bn_train_backward(const BnShape& g, const float* z, const float* y, const float* dy, const float* mr, const float* gamma, const float* sscale,
                              int act, int training, int nchunk, int planes, float* dz, float* dres, float* dgamma, float* dbeta, float* dfill, float* k,
                              double* part, hipStream_t s) {
    const BnTrain a = bn_train_args(g, z, y, dy, mr, sscale, act, nchunk, planes, part);
    launch_bn_chan_partial<1>(a, s);
    const auto fold = g.active ? bn_bwd_fold_kernel<true> : bn_bwd_fold_kernel<false>;
    hipLaunchKernelGGL(fold, dim3((g.C + 255) / 256), dim3(256), 0, s, part, nchunk, planes, g.C, g.N, g.active, bn_cells(g), bn_cell_pixels(g), training,
                       dgamma, dbeta, dfill, k);
    const dim3 grid((unsigned)((g.N * (g.C / 4) + 255) / 256));
    if (g.active) hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, dim3(256), 0, s, a, gamma, k, dz, dres);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, dim3(256), 0, s, a, gamma, k, dz, dres);
}

}  // namespace cddpm
