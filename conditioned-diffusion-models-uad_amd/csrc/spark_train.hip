// Kernels of SparK masked pre-training (reference src/models/Spark_2D.py; src/models/modules/spark/{Spark_2D,encoder,decoder}.py): what
// the pre-training step needs beside the ResNet-50's training operators (encoder_train.hip). Everything NHWC fp32, memory- and
// launch-bound work: small channel counts (2048 -> 128 at f x f down to 4 -> 1 at the image's resolution), no matrix pipe. Pieces:
//   spark_chan_partial / folds   BatchNorm over the ACTIVE pixels only (encoder.py:25-35: BatchNorm1d over the gathered rows) or over
//                          all of them (active == nullptr: the decoder's BatchNorm2d, decoder.py:26-27), fp64 sums, n_act counted on
//                          the device from the cell mask; y = act((active ? bn(z) : fill) s[b] + res), act = none | ReLU | ReLU6
//   spark_mask_mul         y = x * active_ex (Spark_2D.py:150-151, encoder.py:19-22)
//   spark_conv_kernel      one 64 x 64-tile gather convolution in two index forms, any channel counts, weights read in place through
//                          strides: form 0 gathers ys = y stride + ky - pad (Conv2d forward, ConvTranspose2d input gradient), form 1
//                          gathers ys = (y + pad - ky) / stride where exact (Conv2d input gradient, ConvTranspose2d forward)
//   spark_wgrad_kernel     dW in the PyTorch layout over form 0, pixel ranges folded in a fixed order; spark_chan_sum: the bias gradient
//   spark_loss             spatial_loss with pix_norm 0 (Spark_2D.py:180-199) and the L1 mean, with the gradient of their weighted sum
// Nothing here uses float atomics: every reduction is a two-stage sum in a fixed order.
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace cddpm {

// number of set cells of active [ncell]; every thread of the 256-thread workgroup calls it and gets the count
__device__ __forceinline__ int spark_count_active(const unsigned char* __restrict__ active, int ncell, int* red) {
    int c = 0;
    for (int i = threadIdx.x; i < ncell; i += 256) c += active[i] != 0;
    red[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const int r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float spark_act_grad(float g, float y, int act) {
    if (act == 1) return y > 0.f ? g : 0.f;
    if (act == 2) return (y > 0.f && y < 6.f) ? g : 0.f;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm
struct SparkBn {
    const float *z, *y, *dy, *mr, *sscale;
    const unsigned char* active;      // [B][f][f] or nullptr (every pixel active)
    int f, ch, cw;                    // cells per side; pixels per cell: ch = H / f, cw = W / f
    int W, HW, C, act;
    long long N;
    int nchunk, qpb, rows;            // pixel chunks; channel quads per workgroup; pixel lanes per workgroup (qpb rows <= 256)
    double* part;                     // [nchunk][2 | 3][C]
};
__device__ __forceinline__ bool spark_pixel_active(const SparkBn& a, long long p) {
    if (!a.active) return true;
    const int b = (int)(p / a.HW), rem = (int)(p - (long long)b * a.HW);
    const int y = rem / a.W, x = rem - y * a.W;
    return a.active[((size_t)b * a.f + y / a.ch) * a.f + x / a.cw] != 0;
}
// per-channel sums over the pixels of one chunk, fp64. MODE 0: (sum z, sum z^2) over active pixels. MODE 1: g = dy act'(y) s[b];
// (sum g, sum g zhat) over active pixels, (sum g) over inactive ones
template <int MODE>
__global__ __launch_bounds__(256) void spark_chan_partial_kernel(const SparkBn a) {
    constexpr int NS = MODE == 0 ? 2 : 3;
    __shared__ double red[NS][1024];
    const int tid = threadIdx.x, q = tid % a.qpb, r = tid / a.qpb, cw4 = a.qpb * 4;
    const int c = (blockIdx.y * a.qpb + q) * 4;
    const bool valid = r < a.rows && c < a.C;
    const long long per = (a.N + a.nchunk - 1) / a.nchunk, p0 = per * blockIdx.x, p1 = p0 + per < a.N ? p0 + per : a.N;
    double s[NS][4];
    for (int j = 0; j < NS; ++j)
        for (int i = 0; i < 4; ++i) s[j][i] = 0.0;
    if (valid) {
        float mean[4] = {0, 0, 0, 0}, rstd[4] = {1, 1, 1, 1};
        if (MODE == 1)
            for (int i = 0; i < 4; ++i) { mean[i] = a.mr[c + i]; rstd[i] = a.mr[a.C + c + i]; }
        for (long long p = p0 + r; p < p1; p += a.rows) {
            const bool on = spark_pixel_active(a, p);
            if (MODE == 0) {
                if (!on) continue;
                const float4 zv = *reinterpret_cast<const float4*>(a.z + (size_t)p * a.C + c);
                const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
                for (int i = 0; i < 4; ++i) { s[0][i] += zz[i]; s[1][i] += (double)zz[i] * zz[i]; }
            } else {
                const float4 dv = *reinterpret_cast<const float4*>(a.dy + (size_t)p * a.C + c);
                float gg[4] = {dv.x, dv.y, dv.z, dv.w};
                if (a.act) {
                    const float4 yv = *reinterpret_cast<const float4*>(a.y + (size_t)p * a.C + c);
                    const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
                    for (int i = 0; i < 4; ++i) gg[i] = spark_act_grad(gg[i], yy[i], a.act);
                }
                const float sc = a.sscale ? a.sscale[p / a.HW] : 1.f;
                if (on) {
                    const float4 zv = *reinterpret_cast<const float4*>(a.z + (size_t)p * a.C + c);
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
    if (r < a.rows)
        for (int j = 0; j < NS; ++j)
            for (int i = 0; i < 4; ++i) red[j][r * cw4 + 4 * q + i] = s[j][i];
    __syncthreads();
    if (tid < NS * cw4) {
        const int w = tid / cw4, cc = tid - w * cw4, ch = blockIdx.y * cw4 + cc;
        if (ch < a.C) {
            double t = 0;
            for (int k = 0; k < a.rows; ++k) t += red[w][k * cw4 + cc];
            a.part[((size_t)blockIdx.x * NS + w) * a.C + ch] = t;
        }
    }
}
// batch statistics over the n_act active pixels: mr = (mean | rstd); running statistics as torch's BatchNorm in training mode (momentum,
// unbiased variance). n_act < 2: nothing is written but status = {1, n_act} (torch's BatchNorm1d raises there)
__global__ __launch_bounds__(256) void spark_bn_stats_fold_kernel(const double* __restrict__ part, int nchunk, int C, long long N,
                                                                  const unsigned char* __restrict__ active, int ncell, int cellpx, float eps,
                                                                  float momentum, float* __restrict__ mr, float* __restrict__ run_mean,
                                                                  float* __restrict__ run_var, int* __restrict__ status) {
    __shared__ int red[256];
    const long long n = active ? (long long)spark_count_active(active, ncell, red) * cellpx : N;
    if (blockIdx.x == 0 && threadIdx.x == 0 && status) { status[0] = n < 2; status[1] = (int)n; }
    if (n < 2) return;
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
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(var * (double)n / (double)(n - 1));
    }
}
// evaluation mode: the running statistics stand in for the batch's
__global__ __launch_bounds__(256) void spark_bn_eval_stats_kernel(const float* __restrict__ run_mean, const float* __restrict__ run_var, float eps, int C,
                                                                  float* __restrict__ mr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    mr[c] = run_mean[c];
    mr[C + c] = (float)(1.0 / sqrt((double)run_var[c] + (double)eps));
}
__global__ __launch_bounds__(256) void spark_bn_act_kernel(const SparkBn a, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ fill, const float* __restrict__ res, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nq = a.C >> 2;
    if (e >= a.N * nq) return;
    const int c = 4 * (int)(e % nq);
    const long long p = e / nq;
    float4 o;
    if (spark_pixel_active(a, p)) {
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
// backward sums -> dgamma, dbeta, dfill and the two per-channel means of the elementwise pass (k = (sum g / n_act | sum g zhat / n_act);
// both 0 in evaluation mode, where the statistics do not depend on z)
__global__ __launch_bounds__(256) void spark_bn_bwd_fold_kernel(const double* __restrict__ part, int nchunk, int C, long long N,
                                                                const unsigned char* __restrict__ active, int ncell, int cellpx, int training,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dfill,
                                                                float* __restrict__ k) {
    __shared__ int red[256];
    const long long n = active ? (long long)spark_count_active(active, ncell, red) * cellpx : N;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int j = 0; j < nchunk; ++j) {
        s0 += part[((size_t)j * 3) * C + c]; s1 += part[((size_t)j * 3 + 1) * C + c]; s2 += part[((size_t)j * 3 + 2) * C + c];
    }
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
    if (dfill) dfill[c] = (float)s2;
    const bool stats = training && n > 0;
    k[c] = stats ? (float)(s0 / (double)n) : 0.f;
    k[C + c] = stats ? (float)(s1 / (double)n) : 0.f;
}
// dz = active ? gamma rstd (g - k0 - zhat k1) : 0, g = dy act'(y) s[b]; dres (optional) = dy act'(y)
__global__ __launch_bounds__(256) void spark_bn_bwd_apply_kernel(const SparkBn a, const float* __restrict__ gamma, const float* __restrict__ k,
                                                                 float* __restrict__ dz, float* __restrict__ dres) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nq = a.C >> 2;
    if (e >= a.N * nq) return;
    const int c = 4 * (int)(e % nq);
    const long long p = e / nq;
    float4 dv = *reinterpret_cast<const float4*>(a.dy + (size_t)p * a.C + c);
    if (a.act) {
        const float4 yv = *reinterpret_cast<const float4*>(a.y + (size_t)p * a.C + c);
        dv.x = spark_act_grad(dv.x, yv.x, a.act); dv.y = spark_act_grad(dv.y, yv.y, a.act);
        dv.z = spark_act_grad(dv.z, yv.z, a.act); dv.w = spark_act_grad(dv.w, yv.w, a.act);
    }
    if (dres) *reinterpret_cast<float4*>(dres + (size_t)p * a.C + c) = dv;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (spark_pixel_active(a, p)) {
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
    *reinterpret_cast<float4*>(dz + (size_t)p * a.C + c) = o;
}
int spark_bn_chunks(long long N, int C) {
    long long n = N * C / 16384;            // >= 16 K elements per chunk; the folds read the chunks serially
    if (n > 128) n = 128;
    return n < 1 ? 1 : (int)n;
}
static SparkBn spark_bn_args(const float* z, const float* y, const float* dy, const float* mr, const float* sscale, const unsigned char* active,
                             int f, int H, int W, int C, int act, long long N, double* part) {
    SparkBn a;
    a.z = z; a.y = y; a.dy = dy; a.mr = mr; a.sscale = sscale; a.active = active; a.f = f; a.ch = H / f; a.cw = W / f;
    a.W = W; a.HW = H * W; a.C = C; a.act = act; a.N = N; a.nchunk = spark_bn_chunks(N, C);
    a.qpb = C / 4 < 16 ? C / 4 : 16; a.rows = 256 / a.qpb; a.part = part;
    return a;
}
static dim3 spark_bn_partial_grid(const SparkBn& a) { return dim3(a.nchunk, (a.C / 4 + a.qpb - 1) / a.qpb); }
void launch_spark_bn_stats(const float* z, const unsigned char* active, int f, int B, int H, int W, int C, float eps, float momentum, float* run_mean,
                           float* run_var, float* mr, double* part, int* status, hipStream_t s) {
    const long long N = (long long)B * H * W;
    const SparkBn a = spark_bn_args(z, nullptr, nullptr, nullptr, nullptr, active, f, H, W, C, 0, N, part);
    hipLaunchKernelGGL(spark_chan_partial_kernel<0>, spark_bn_partial_grid(a), dim3(256), 0, s, a);
    hipLaunchKernelGGL(spark_bn_stats_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, a.nchunk, C, N, active, B * f * f, a.ch * a.cw, eps,
                       momentum, mr, run_mean, run_var, status);
}
void launch_spark_bn_eval_stats(const float* run_mean, const float* run_var, float eps, int C, float* mr, hipStream_t s) {
    hipLaunchKernelGGL(spark_bn_eval_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, s, run_mean, run_var, eps, C, mr);
}
void launch_spark_bn_act(const float* z, const float* mr, const float* gamma, const float* beta, const float* sscale, const float* res,
                         const unsigned char* active, int f, const float* fill, int act, float* y, int B, int H, int W, int C, hipStream_t s) {
    const long long N = (long long)B * H * W, total = N * (C / 4);
    const SparkBn a = spark_bn_args(z, nullptr, nullptr, mr, sscale, active, f, H, W, C, act, N, nullptr);
    hipLaunchKernelGGL(spark_bn_act_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, gamma, beta, fill, res, y);
}
void launch_spark_bn_backward(const float* z, const float* y, const float* dy, const float* mr, const float* gamma, const float* sscale, int act,
                              const unsigned char* active, int f, int training, float* dz, float* dres, float* dgamma, float* dbeta, float* dfill,
                              float* k, double* part, int B, int H, int W, int C, hipStream_t s) {
    const long long N = (long long)B * H * W, total = N * (C / 4);
    const SparkBn a = spark_bn_args(z, y, dy, mr, sscale, active, f, H, W, C, act, N, part);
    hipLaunchKernelGGL(spark_chan_partial_kernel<1>, spark_bn_partial_grid(a), dim3(256), 0, s, a);
    hipLaunchKernelGGL(spark_bn_bwd_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, a.nchunk, C, N, active, B * f * f, a.ch * a.cw, training,
                       dgamma, dbeta, dfill, k);
    hipLaunchKernelGGL(spark_bn_bwd_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, gamma, k, dz, dres);
}

// ---------------------------------------------------------------------------------------------------------------- mask multiply
__global__ __launch_bounds__(256) void spark_mask_mul_kernel(const float* x /* may be y */, const unsigned char* __restrict__ active, float* y,
                                                             long long total, int H, int W, int C, int f, int ch, int cw) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    long long p = e / C;
    const int xx = (int)(p % W); p /= W;
    const int yy = (int)(p % H);
    const int b = (int)(p / H);
    y[e] = active[((size_t)b * f + yy / ch) * f + xx / cw] ? x[e] : 0.f;
}
void launch_spark_mask_mul(const float* x, const unsigned char* active, float* y, int B, int H, int W, int C, int f, hipStream_t s) {
    const long long total = (long long)B * H * W * C;
    hipLaunchKernelGGL(spark_mask_mul_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, active, y, total, H, W, C, f, H / f, W / f);
}

// ---------------------------------------------------------------------------------------------------------------- small-channel convolutions
// dst [B,Hd,Wd,Cd] = bias + sum over taps and source channels of src [B,Hs,Ws,Cs] (gathered) * w[cd wsd + cs wss + tap].
// Workgroup = 64 destination pixels x 64 destination channels, 16 source channels of one tap per step; channels beyond Cs / Cd are masked.
__global__ __launch_bounds__(256) void spark_conv_kernel(const SparkConv a) {
    __shared__ float As[16][64 + 4];
    __shared__ float Bs[16][64 + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long M = (long long)a.B * a.Hd * a.Wd;
    const long long p0 = (long long)blockIdx.x * 64;
    const int n0 = blockIdx.y * 64;
    const int lp = tid >> 2, lc4 = tid & 3;
    const long long pl = p0 + lp;
    int lb = 0, ly = 0, lx = 0;
    const bool lvalid = pl < M;
    if (lvalid) { long long t = pl; lx = (int)(t % a.Wd); t /= a.Wd; ly = (int)(t % a.Hd); lb = (int)(t / a.Hd); }
    const int bk = tid >> 4, bc4 = tid & 15;
    const bool vec = (a.Cs & 3) == 0;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    const int nck = (a.Cs + 15) / 16, nstep = a.K * a.K * nck;
    auto fetch = [&](int step, float (&av)[4], float (&bv)[4]) {
        const int t = step / nck, c0 = (step - t * nck) * 16;
        const int ky = t / a.K, kx = t - ky * a.K;
        int ys, xs;
        bool inb = lvalid;
        if (a.form == 0) { ys = ly * a.stride + ky - a.pad; xs = lx * a.stride + kx - a.pad; }
        else {
            const int ny = ly + a.pad - ky, nx = lx + a.pad - kx;
            inb = inb && ny >= 0 && nx >= 0 && (ny % a.stride) == 0 && (nx % a.stride) == 0;
            ys = ny / a.stride; xs = nx / a.stride;
        }
        inb = inb && ys >= 0 && ys < a.Hs && xs >= 0 && xs < a.Ws;
        const int c = c0 + 4 * lc4;
        av[0] = av[1] = av[2] = av[3] = 0.f;
        if (inb && c < a.Cs) {
            const float* sp = a.src + (((size_t)lb * a.Hs + ys) * a.Ws + xs) * a.Cs + c;
            if (vec) { const float4 v = *reinterpret_cast<const float4*>(sp); av[0] = v.x; av[1] = v.y; av[2] = v.z; av[3] = v.w; }
            else
                for (int i = 0; i < 4; ++i) if (c + i < a.Cs) av[i] = sp[i];
        }
        const int cs = c0 + bk;
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + 4 * bc4 + j;
            bv[j] = (cs < a.Cs && n < a.Cd) ? a.w[(size_t)n * a.wsd + (size_t)cs * a.wss + t] : 0.f;
        }
    };
    const int s0 = (int)((long long)nstep * blockIdx.z / a.Z), s1 = (int)((long long)nstep * (blockIdx.z + 1) / a.Z);
    float av[4], bv[4];
    if (s0 < s1) fetch(s0, av, bv);
    for (int step = s0; step < s1; ++step) {
        __syncthreads();
        As[4 * lc4 + 0][lp] = av[0]; As[4 * lc4 + 1][lp] = av[1]; As[4 * lc4 + 2][lp] = av[2]; As[4 * lc4 + 3][lp] = av[3];
        *reinterpret_cast<float4*>(&Bs[bk][4 * bc4]) = make_float4(bv[0], bv[1], bv[2], bv[3]);
        __syncthreads();
        if (step + 1 < s1) fetch(step + 1, av, bv);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4 a4 = *reinterpret_cast<const float4*>(&As[k][4 * ty]);
            const float4 b4 = *reinterpret_cast<const float4*>(&Bs[k][4 * tx]);
            const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(aa[i], bb[j], acc[i][j]);
        }
    }
    float* o = a.Z > 1 ? a.part + (size_t)blockIdx.z * M * a.Cd : a.dst;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long p = p0 + 4 * ty + i;
        if (p >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + 4 * tx + j;
            if (n < a.Cd) o[(size_t)p * a.Cd + n] = acc[i][j] + ((a.Z == 1 && a.bias) ? a.bias[n] : 0.f);
        }
    }
}
// dst[e] = ((plane 0 + plane 1) + ...) [+ bias[e % C]]: the fixed-order fold of contraction splits and of pixel ranges
__global__ __launch_bounds__(256) void spark_fold_planes_kernel(const float* __restrict__ part, int Z, long long n, const float* __restrict__ bias, int C,
                                                                float* __restrict__ dst) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s = part[e];
    for (int z = 1; z < Z; ++z) s += part[(size_t)z * n + e];
    if (bias) s += bias[e % C];
    dst[e] = s;
}
int spark_conv_split(long long M, int Cd, int Cs, int K) {
    const long long wgs = ((M + 63) / 64) * ((Cd + 63) / 64);
    const int nstep = K * K * ((Cs + 15) / 16);
    int Z = 1;
    while (Z < 32 && wgs * Z * 2 <= 512 && nstep / (Z * 2) >= 8) Z *= 2;
    return Z;
}
void launch_spark_conv(SparkConv a, hipStream_t s) {
    const long long M = (long long)a.B * a.Hd * a.Wd;
    a.Z = a.part ? spark_conv_split(M, a.Cd, a.Cs, a.K) : 1;
    hipLaunchKernelGGL(spark_conv_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)((a.Cd + 63) / 64), a.Z), dim3(256), 0, s, a);
    if (a.Z > 1) {
        const long long n = M * a.Cd;
        hipLaunchKernelGGL(spark_fold_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.part, a.Z, n, a.bias, a.Cd, a.dst);
    }
}

// dW[cd][cg][tap] = sum over the pixels q of d [B,Hq,Wq,Cd] of d[q][cd] * g[b, y stride + ky - pad, x stride + kx - pad][cg]  (g [B,Hg,Wg,Cg]):
// Conv2d: d = dy, g = x (dW [Cout][Cin][K][K]); ConvTranspose2d: d = x, g = dy (dW [Cin][Cout][K][K]).
// Workgroup = (64 cd, 64 cg, tap, pixel range); part [P][Cd Cg K K] in dW's own layout
__global__ __launch_bounds__(256) void spark_wgrad_kernel(const SparkWgrad a) {
    __shared__ float As[16][64 + 4];     // [pixel][cd]
    __shared__ float Bs[16][64 + 4];     // [pixel][cg]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int taps = a.K * a.K;
    const int cd0 = blockIdx.x * 64, cg0 = blockIdx.y * 64;
    const int t = blockIdx.z % taps, part = blockIdx.z / taps;
    const int ky = t / a.K, kx = t - ky * a.K;
    const long long M = (long long)a.B * a.Hq * a.Wq;
    const long long m0 = M * part / a.P, m1 = M * (part + 1) / a.P;
    const int lp = tid >> 4, lc4 = tid & 15;
    const bool vd = (a.Cd & 3) == 0, vg = (a.Cg & 3) == 0;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (long long q0 = m0; q0 < m1; q0 += 16) {
        const long long q = q0 + lp;
        float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (q < m1) {
            long long r = q;
            const int x = (int)(r % a.Wq); r /= a.Wq;
            const int y = (int)(r % a.Hq);
            const int b = (int)(r / a.Hq);
            const int cd = cd0 + 4 * lc4, cg = cg0 + 4 * lc4;
            if (cd < a.Cd) {
                const float* dp = a.d + (size_t)q * a.Cd + cd;
                if (vd) { const float4 v = *reinterpret_cast<const float4*>(dp); av[0] = v.x; av[1] = v.y; av[2] = v.z; av[3] = v.w; }
                else
                    for (int i = 0; i < 4; ++i) if (cd + i < a.Cd) av[i] = dp[i];
            }
            const int yg = y * a.stride + ky - a.pad, xg = x * a.stride + kx - a.pad;
            if (cg < a.Cg && yg >= 0 && yg < a.Hg && xg >= 0 && xg < a.Wg) {
                const float* gp = a.g + (((size_t)b * a.Hg + yg) * a.Wg + xg) * a.Cg + cg;
                if (vg) { const float4 v = *reinterpret_cast<const float4*>(gp); bv[0] = v.x; bv[1] = v.y; bv[2] = v.z; bv[3] = v.w; }
                else
                    for (int i = 0; i < 4; ++i) if (cg + i < a.Cg) bv[i] = gp[i];
            }
        }
        __syncthreads();
        *reinterpret_cast<float4*>(&As[lp][4 * lc4]) = make_float4(av[0], av[1], av[2], av[3]);
        *reinterpret_cast<float4*>(&Bs[lp][4 * lc4]) = make_float4(bv[0], bv[1], bv[2], bv[3]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4 a4 = *reinterpret_cast<const float4*>(&As[k][4 * ty]);
            const float4 b4 = *reinterpret_cast<const float4*>(&Bs[k][4 * tx]);
            const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(aa[i], bb[j], acc[i][j]);
        }
    }
    float* o = a.part + (size_t)part * a.Cd * a.Cg * taps;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cd = cd0 + 4 * ty + i;
        if (cd >= a.Cd) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cg = cg0 + 4 * tx + j;
            if (cg < a.Cg) o[((size_t)cd * a.Cg + cg) * taps + t] = acc[i][j];
        }
    }
}
int spark_wgrad_parts(long long M, int Cd, int Cg, int K) {
    const int per = ((Cd + 63) / 64) * ((Cg + 63) / 64) * K * K;
    long long P = (512 + per - 1) / per;
    if (P > M / 64) P = M / 64;
    if (P > 64) P = 64;
    return P < 1 ? 1 : (int)P;
}
void launch_spark_wgrad(SparkWgrad a, float* dw, hipStream_t s) {
    hipLaunchKernelGGL(spark_wgrad_kernel, dim3((a.Cd + 63) / 64, (a.Cg + 63) / 64, a.K * a.K * a.P), dim3(256), 0, s, a);
    const long long n = (long long)a.Cd * a.Cg * a.K * a.K;
    hipLaunchKernelGGL(spark_fold_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.part, a.P, n, nullptr, 1, dw);
}
// per-channel sum of x [M][C] (C <= 256): chunk partials in fp64, folded in the order of the chunks
__global__ __launch_bounds__(256) void spark_chan_sum_kernel(const float* __restrict__ x, long long M, int C, int nchunk, double* __restrict__ part) {
    __shared__ double red[256];
    const int rows = 256 / C, c = threadIdx.x % C, r = threadIdx.x / C;
    const long long per = (M + nchunk - 1) / nchunk, p0 = per * blockIdx.x, p1 = p0 + per < M ? p0 + per : M;
    double s = 0;
    if (r < rows)
        for (long long p = p0 + r; p < p1; p += rows) s += x[(size_t)p * C + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if ((int)threadIdx.x < C) {
        double t = 0;
        for (int k = 0; k < rows; ++k) t += red[k * C + threadIdx.x];
        part[(size_t)blockIdx.x * C + threadIdx.x] = t;
    }
}
__global__ __launch_bounds__(256) void spark_chan_sum_fold_kernel(const double* __restrict__ part, int nchunk, int C, float* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0;
    for (int k = 0; k < nchunk; ++k) s += part[(size_t)k * C + c];
    out[c] = (float)s;
}
int spark_chan_sum_chunks(long long M, int C) {
    long long n = M * C / 8192;
    if (n > 256) n = 256;
    return n < 1 ? 1 : (int)n;
}
void launch_spark_chan_sum(const float* x, long long M, int C, double* part, float* out, hipStream_t s) {
    const int nchunk = spark_chan_sum_chunks(M, C);
    hipLaunchKernelGGL(spark_chan_sum_kernel, dim3(nchunk), dim3(256), 0, s, x, M, C, nchunk, part);
    hipLaunchKernelGGL(spark_chan_sum_fold_kernel, dim3(1), dim3(256), 0, s, part, nchunk, C, out);
}

// ---------------------------------------------------------------------------------------------------------------- loss
// masked = sum over pixels of masked cells of (rec - inp)^2 / (p^2 (n_masked + 1e-8)), l1 = mean |rec - inp|;
// drec = w_mask d masked / d rec + w_l1 d l1 / d rec. One channel: rec, inp [B][H][W]; p^2 = (H / f)(W / f) pixels per cell.
// scaler given (the device block of the dynamic loss scaling, include/cddpm.h): both weights are multiplied by its scale first, a power of
// two, so drec carries the bits the plain call gives for weights S w_mask, S w_l1; the two loss terms are never scaled.
__global__ __launch_bounds__(256) void spark_loss_partial_kernel(const float* __restrict__ rec, const float* __restrict__ inp,
                                                                 const unsigned char* __restrict__ active, int f, int ncell, int H, int W, int ch, int cw,
                                                                 long long total, float w_mask, float w_l1, const int* __restrict__ scaler,
                                                                 float* __restrict__ drec, double* __restrict__ part) {
    __shared__ int cnt[256];
    __shared__ double red[2][256];
    const int n_masked = ncell - spark_count_active(active, ncell, cnt);
    if (scaler) {
        const float scale = reinterpret_cast<const float*>(scaler)[0];
        w_mask *= scale; w_l1 *= scale;
    }
    const float km = w_mask * 2.f / ((float)(ch * cw) * ((float)n_masked + 1e-8f)), kl = w_l1 / (float)total;
    const long long per = (total + gridDim.x - 1) / gridDim.x, e0 = per * blockIdx.x, e1 = e0 + per < total ? e0 + per : total;
    double sm = 0, sl = 0;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        long long p = e;
        const int x = (int)(p % W); p /= W;
        const int y = (int)(p % H);
        const int b = (int)(p / H);
        const bool masked = active[((size_t)b * f + y / ch) * f + x / cw] == 0;
        const float d = rec[e] - inp[e];
        sl += fabsf(d);
        if (masked) sm += (double)d * d;
        if (drec) drec[e] = (masked ? km * d : 0.f) + kl * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
    }
    red[0][threadIdx.x] = sm; red[1][threadIdx.x] = sl;
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0;
        for (int k = 0; k < 256; ++k) t += red[threadIdx.x][k];
        part[(size_t)blockIdx.x * 2 + threadIdx.x] = t;
    }
}
__global__ __launch_bounds__(256) void spark_loss_fold_kernel(const double* __restrict__ part, int nchunk, const unsigned char* __restrict__ active, int ncell,
                                                              int cellpx, long long total, float* __restrict__ loss) {
    __shared__ int cnt[256];
    const int n_masked = ncell - spark_count_active(active, ncell, cnt);
    if (threadIdx.x >= 2) return;
    double t = 0;
    for (int k = 0; k < nchunk; ++k) t += part[(size_t)k * 2 + threadIdx.x];
    loss[threadIdx.x] = threadIdx.x == 0 ? (float)(t / ((double)cellpx * ((double)n_masked + 1e-8))) : (float)(t / (double)total);
}
int spark_loss_chunks(long long total) {
    long long n = total / 4096;
    if (n > 256) n = 256;
    return n < 1 ? 1 : (int)n;
}
void launch_spark_loss(const float* rec, const float* inp, const unsigned char* active, int f, int B, int H, int W, float w_mask, float w_l1,
                       const int* scaler, float* loss, float* drec, double* part, hipStream_t s) {
    const long long total = (long long)B * H * W;
    const int nchunk = spark_loss_chunks(total);
    hipLaunchKernelGGL(spark_loss_partial_kernel, dim3(nchunk), dim3(256), 0, s, rec, inp, active, f, B * f * f, H, W, H / f, W / f, total, w_mask, w_l1,
                       scaler, drec, part);
    hipLaunchKernelGGL(spark_loss_fold_kernel, dim3(1), dim3(256), 0, s, part, nchunk, active, B * f * f, (H / f) * (W / f), total, loss);
}

}  // namespace cddpm
