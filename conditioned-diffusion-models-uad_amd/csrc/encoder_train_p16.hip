// Precision-16 convolutions of the context encoder's training step: what the reference trainer's `precision: 16`
// (configs/trainer/default.yaml:7) computes for self.encoder under autocast (src/models/DDPM_2D.py:114-135: features = self(input) is inside the
// LightningModule's autocast region, and so is its backward). The arithmetic of include/cddpm.h ("Arithmetic of the training operators"): every
// operand element rounded to fp16 to nearest even with gradual underflow (as torch's .half(): |v| > 65504 -> inf), products accumulated in fp32
// on v_mfma_f32_16x16x32_f16, fp32 NHWC results, no pre-scales. Same three roles and the same shapes as encoder_train.hip's FMA tiles:
//   enc_conv_p16_kernel    forward (rows = output pixels) and input gradient (rows = INPUT pixels, gathered dz rows): a 64 x 64 tile per
//                          workgroup, 32 x 32 per wave. NHWC makes the A operand a contiguous 8-channel read per lane (two float4 + convert: lane
//                          l holds row l & 15, k = 8 (l >> 4) ... + 7); the fp16 weight image makes the B operand one 16-byte read per lane.
//                          No LDS: a wave's operands are whole cache lines and its neighbour's re-reads hit L1.
//   enc_wgrad_p16_kernel   dW: contraction over pixels, the strided axis of both operands, so x and dz go through LDS transposed ([channel][pixel]
//                          fp16 images, rounded on the way in), 64 ci x 64 co x one tap x one pixel range per workgroup, planes in dW's order
//   enc_pack_w_p16_kernel  the fp16 weight images, rounded once at packing
// Contraction splits go to planes that are folded in a fixed order (enc_fold_planes_kernel, enc_wgrad_p16_fold9_kernel): no float atomics, bit-identical runs.
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace cddpm {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// float -> fp16 conversions are plain casts: v_cvt_f16_f32 under the default round-to-nearest-even mode with fp16 denormals kept
static __device__ __forceinline__ h16x8 round8(const float4 a, const float4 b) {
    h16x8 r;
    r[0] = (_Float16)a.x; r[1] = (_Float16)a.y; r[2] = (_Float16)a.z; r[3] = (_Float16)a.w;
    r[4] = (_Float16)b.x; r[5] = (_Float16)b.y; r[6] = (_Float16)b.z; r[7] = (_Float16)b.w;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- weight images
// from the PyTorch tensor w [Cout][Cin][K][K]: wf [taps][Cin / 32][Cout][32] (forward: contraction over ci) and wd [taps][Cout / 32][Cin][32]
// (input gradient: contraction over co), i.e. [tap][k chunk][produced channel][k in chunk]: the 16 x 32 B fragment of one MFMA is 1 KiB in a row
__global__ __launch_bounds__(256) void enc_pack_w_p16_kernel(const float* __restrict__ w, int Cout, int Cin, int taps, _Float16* __restrict__ wf,
                                                             _Float16* __restrict__ wd) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)Cout * Cin * taps) return;
    const int t = (int)(e % taps), ci = (int)((e / taps) % Cin), co = (int)(e / ((long long)taps * Cin));
    const _Float16 v = (_Float16)w[e];
    if (wf) wf[(((size_t)t * (Cin / 32) + ci / 32) * Cout + co) * 32 + (ci & 31)] = v;
    if (wd) wd[(((size_t)t * (Cout / 32) + co / 32) * Cin + ci) * 32 + (co & 31)] = v;
}
void launch_enc_pack_w_p16(const float* w, int Cout, int Cin, int taps, void* wf, void* wd, hipStream_t s) {
    const long long n = (long long)Cout * Cin * taps;
    hipLaunchKernelGGL(enc_pack_w_p16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, Cout, Cin, taps, static_cast<_Float16*>(wf),
                       static_cast<_Float16*>(wd));
}

// ---------------------------------------------------------------------------------------------------------------- forward / input gradient
struct EncConvP16 {
    const float* src;      // forward: x [B,H,W,Kdim]; input gradient: dz [B,Ho,Wo,Kdim]
    const _Float16* w;     // [taps][Kdim / 32][Ndim][32]
    float* dst;            // forward: z [B,Ho,Wo,Ndim]; input gradient: dx [B,H,W,Ndim]
    int B, H, W, Ho, Wo;   // H, W: the convolution's input size; Ho, Wo: its output size
    int Kdim, Ndim, K, stride, transposed;
    int Z;                 // contraction split: blockIdx.z multiplies steps [nstep z / Z, nstep (z + 1) / Z) into plane z of `part`
    float* part;           // [Z][rows][Ndim] when Z > 1
};
__global__ __launch_bounds__(256) void enc_conv_p16_kernel(const EncConvP16 a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int Hr = a.transposed ? a.H : a.Ho, Wr = a.transposed ? a.W : a.Wo;       // geometry of the rows this launch produces
    const int Hs = a.transposed ? a.Ho : a.H, Ws = a.transposed ? a.Wo : a.W;       // ... and of the tensor it gathers from
    const long long M = (long long)a.B * Hr * Wr;
    const long long p0 = (long long)blockIdx.x * 64 + 32 * (wave >> 1);
    const int n0 = blockIdx.y * 64 + 32 * (wave & 1);
    int rb[2], ry[2], rx[2];
    bool rv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {                    // the two A fragments' rows of this lane
        long long t = p0 + 16 * i + fr;
        rv[i] = t < M;
        if (!rv[i]) t = 0;
        rx[i] = (int)(t % Wr); t /= Wr; ry[i] = (int)(t % Hr); rb[i] = (int)(t / Hr);
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int pad = a.K / 2, taps = a.K * a.K;
    const int nkc = a.Kdim / 64, nstep = taps * nkc;
    // one step = 64 contraction channels of one tap (two MFMA k-blocks); the next step's twelve 16-byte loads are in flight while this
    // step converts and multiplies
    auto fetch = [&](int step, float4 (&av)[2][2][2], h16x8 (&bv)[2][2]) {
        const int t = step / nkc, kc = step - t * nkc;
        const int ky = t / a.K, kx = t - ky * a.K;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int ys, xs;
            bool inb = rv[i];
            if (!a.transposed) { ys = ry[i] * a.stride + ky - pad; xs = rx[i] * a.stride + kx - pad; }
            else {
                const int ny = ry[i] + pad - ky, nx = rx[i] + pad - kx;
                inb = inb && ny >= 0 && nx >= 0 && (ny % a.stride) == 0 && (nx % a.stride) == 0;
                ys = ny / a.stride; xs = nx / a.stride;
            }
            inb = inb && ys >= 0 && ys < Hs && xs >= 0 && xs < Ws;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) av[i][ks][0] = av[i][ks][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (inb) {
                const float4* q = reinterpret_cast<const float4*>(a.src + (((size_t)rb[i] * Hs + ys) * Ws + xs) * a.Kdim + 64 * kc + 8 * fq);
                av[i][0][0] = q[0]; av[i][0][1] = q[1]; av[i][1][0] = q[8]; av[i][1][1] = q[9];
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bv[ks][j] = *reinterpret_cast<const h16x8*>(a.w + (((size_t)t * 2 * nkc + 2 * kc + ks) * a.Ndim + n0 + 16 * j + fr) * 32 + 8 * fq);
    };
    const int s0 = (int)((long long)nstep * blockIdx.z / a.Z), s1 = (int)((long long)nstep * (blockIdx.z + 1) / a.Z);
    float4 av[2][2][2];
    h16x8 bv[2][2];
    fetch(s0, av, bv);
    for (int step = s0; step < s1; ++step) {
        h16x8 fa[2][2], fb[2][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i) { fa[ks][i] = round8(av[i][ks][0], av[i][ks][1]); fb[ks][i] = bv[ks][i]; }
        if (step + 1 < s1) fetch(step + 1, av, bv);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[ks][i], fb[ks][j], acc[i][j], 0, 0, 0);
    }
    // C fragment: column = lane & 15, row = 4 (lane >> 4) + register
    float* o = a.Z > 1 ? a.part + (size_t)blockIdx.z * M * a.Ndim : a.dst;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = p0 + 16 * i + 4 * fq + r;
            if (p >= M) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) o[(size_t)p * a.Ndim + n0 + 16 * j + fr] = acc[i][j][r];
        }
}
// layers that give the chip fewer than 128 workgroups split their contraction, as enc_conv_split does for the FMA tiles (steps of 64 here: the same planes)
int enc_conv_p16_split(int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed) {
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const long long M = (long long)B * (transposed ? H * W : Ho * Wo);
    const long long wgs = ((M + 63) / 64) * ((transposed ? Cin : Cout) / 64);
    const int nstep = K * K * (transposed ? Cout : Cin) / 64;
    int Z = 1;
    while (Z < 8 && wgs * Z * 2 <= 256 && nstep / (Z * 2) >= 2) Z *= 2;
    return Z;
}
void launch_enc_conv_p16(const float* src, const void* w_img, float* dst, int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed,
                         float* part, hipStream_t s) {
    EncConvP16 a;
    a.Z = part ? enc_conv_p16_split(B, H, W, Cin, Cout, K, stride, transposed) : 1;
    a.part = part;
    a.src = src; a.w = static_cast<const _Float16*>(w_img); a.dst = dst; a.B = B; a.H = H; a.W = W;
    a.Ho = (H + stride - 1) / stride; a.Wo = (W + stride - 1) / stride;
    a.Kdim = transposed ? Cout : Cin; a.Ndim = transposed ? Cin : Cout; a.K = K; a.stride = stride; a.transposed = transposed;
    const long long M = (long long)B * (transposed ? H * W : a.Ho * a.Wo);
    hipLaunchKernelGGL(enc_conv_p16_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)(a.Ndim / 64), a.Z), dim3(256), 0, s, a);
    if (a.Z > 1) launch_enc_fold_planes(part, a.Z, M * a.Ndim / 4, dst, s);
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
// dW [Cout][Cin][K][K]: workgroup = (64 ci, 64 co, tap, pixel range), wave = 32 co x 32 ci (A = dz: rows co; B = x: columns ci, so a C row
// is 16 consecutive ci of one co, the PyTorch order); part [P][taps][Cout][Cin]. A step is 64 pixels: thread (c4, pair) rounds 4 channels of
// two neighbouring pixels of x (gathered at the tap) and of dz and writes them as fp16 pairs into the [channel][pixel] images, from which a
// lane's fragment (one channel, 8 consecutive pixels) is one 16-byte read. The next step's loads are in flight during the MFMAs.
// K = 1 with one pixel range writes dw itself; K = 1 otherwise folds the planes in order (enc_fold_planes_kernel); K = 3 folds and
// interleaves the taps (enc_wgrad_p16_fold9_kernel).
struct EncWgradP16 { const float* x; const float* dz; float* part; int B, H, W, Ho, Wo, Cin, Cout, K, stride, P; };
__global__ __launch_bounds__(256) void enc_wgrad_p16_kernel(const EncWgradP16 a) {
    __shared__ __attribute__((aligned(16))) _Float16 As[64][64 + 8];     // [co][pixel]
    __shared__ __attribute__((aligned(16))) _Float16 Bs[64][64 + 8];     // [ci][pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4, wr = wave >> 1, wc = wave & 1;
    const int taps = a.K * a.K, pad = a.K / 2;
    const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
    const int t = blockIdx.z % taps, part = blockIdx.z / taps;
    const int ky = t / a.K, kx = t - ky * a.K;
    const long long M = (long long)a.B * a.Ho * a.Wo;
    const long long m0 = M * part / a.P, m1 = M * (part + 1) / a.P;
    const int c4 = tid & 15, pp = tid >> 4;           // loader: channels 4 c4 ... + 3 of pixels 2 pp + 32 h, 2 pp + 32 h + 1 (h = 0, 1)
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 xv[2][2], dv[2][2];
    auto fetch = [&](long long q0) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const long long q = q0 + 32 * h + 2 * pp + e;
                xv[h][e] = dv[h][e] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q < m1) {
                    long long r = q;
                    const int xo = (int)(r % a.Wo); r /= a.Wo;
                    const int yo = (int)(r % a.Ho);
                    const int b = (int)(r / a.Ho);
                    const int yi = yo * a.stride + ky - pad, xi = xo * a.stride + kx - pad;
                    if (yi >= 0 && yi < a.H && xi >= 0 && xi < a.W)
                        xv[h][e] = *reinterpret_cast<const float4*>(a.x + (((size_t)b * a.H + yi) * a.W + xi) * a.Cin + ci0 + 4 * c4);
                    dv[h][e] = *reinterpret_cast<const float4*>(a.dz + (size_t)q * a.Cout + co0 + 4 * c4);
                }
            }
    };
    fetch(m0);
    for (long long q0 = m0; q0 < m1; q0 += 64) {
        __syncthreads();                              // the previous step's fragments have been read
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int px = 32 * h + 2 * pp;
            const float x0[4] = {xv[h][0].x, xv[h][0].y, xv[h][0].z, xv[h][0].w}, x1[4] = {xv[h][1].x, xv[h][1].y, xv[h][1].z, xv[h][1].w};
            const float d0[4] = {dv[h][0].x, dv[h][0].y, dv[h][0].z, dv[h][0].w}, d1[4] = {dv[h][1].x, dv[h][1].y, dv[h][1].z, dv[h][1].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                *reinterpret_cast<h16x2*>(&As[4 * c4 + c][px]) = h16x2{(_Float16)d0[c], (_Float16)d1[c]};
                *reinterpret_cast<h16x2*>(&Bs[4 * c4 + c][px]) = h16x2{(_Float16)x0[c], (_Float16)x1[c]};
            }
        }
        __syncthreads();
        if (q0 + 64 < m1) fetch(q0 + 64);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            h16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const h16x8*>(&As[32 * wr + 16 * i + fr][32 * ks + 8 * fq]);
                fb[i] = *reinterpret_cast<const h16x8*>(&Bs[32 * wc + 16 * i + fr][32 * ks + 8 * fq]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }
    float* o = a.part + (((size_t)part * taps + t) * a.Cout + co0 + 32 * wr) * a.Cin + ci0 + 32 * wc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) o[(size_t)(16 * i + 4 * fq + r) * a.Cin + 16 * j + fr] = acc[i][j][r];
}
// dw [Cout][Cin][9] = sum over the P planes, in order, of part [P][9][Cout Cin]
__global__ __launch_bounds__(256) void enc_wgrad_p16_fold9_kernel(const float* __restrict__ part, int P, long long n, float* __restrict__ dw) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * 9) return;
    const int t = (int)(e % 9);
    const long long oc = e / 9;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += part[((size_t)p * 9 + t) * n + oc];
    dw[e] = s;
}
// pixel ranges: enough workgroups for the chip (about 1024), at least two 64-pixel steps each, at most 64 planes
int enc_wgrad_p16_parts(int B, int Ho, int Wo, int Cin, int Cout, int K) {
    const long long M = (long long)B * Ho * Wo;
    const int per = (Cin / 64) * (Cout / 64) * K * K;
    long long P = (1024 + per - 1) / per;
    if (P > M / 128) P = M / 128;
    if (P > 64) P = 64;
    return P < 1 ? 1 : (int)P;
}
void launch_enc_wgrad_p16(const float* x, const float* dz, float* part, int P, float* dw, int B, int H, int W, int Cin, int Cout, int K, int stride,
                          hipStream_t s) {
    EncWgradP16 a;
    const bool direct = K == 1 && P == 1;
    a.x = x; a.dz = dz; a.part = direct ? dw : part; a.B = B; a.H = H; a.W = W; a.Ho = (H + stride - 1) / stride; a.Wo = (W + stride - 1) / stride;
    a.Cin = Cin; a.Cout = Cout; a.K = K; a.stride = stride; a.P = P;
    hipLaunchKernelGGL(enc_wgrad_p16_kernel, dim3(Cin / 64, Cout / 64, K * K * P), dim3(256), 0, s, a);
    const long long n = (long long)Cout * Cin;
    if (K == 3) hipLaunchKernelGGL(enc_wgrad_p16_fold9_kernel, dim3((unsigned)((n * 9 + 255) / 256)), dim3(256), 0, s, part, P, n, dw);
    else if (!direct) launch_enc_fold_planes(part, P, n / 4, dw, s);
}

}  // namespace cddpm
