// Kernels of SparK masked pre-training (reference src/models/Spark_2D.py; src/models/modules/spark/{Spark_2D,encoder,decoder}.py): what
// the pre-training step needs beside the ResNet-50's training operators (encoder_train.hip) and the sparse / dense BatchNorm behind
// cddpm_op_spark_bn_* (batchnorm_train.hip). Everything NHWC fp32, memory- and launch-bound work: small channel counts (2048 -> 128 at
// f x f down to 4 -> 1 at the image's resolution), no matrix pipe. Pieces:
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
    const int n_masked = ncell - count_active_cells(active, ncell, cnt);
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
    const int n_masked = ncell - count_active_cells(active, ncell, cnt);
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
