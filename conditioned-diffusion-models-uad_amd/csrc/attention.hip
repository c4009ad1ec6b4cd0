// Mid-block self-attention core for gfx950: softmax(q k^T / sqrt(d)) v, d = 64, exact fp32 on
// v_mfma_f32_32x32x2_f32, flash-style (the N x N score matrix never leaves registers).
//
// Replaces QKVAttention.forward (src/models/modules/OpenAI_Unet.py:457-476): q,k,v = chunk(qkv, 3);
// heads are contiguous groups of 64 channels; w = softmax_fp32((q s)^T (k s)), s = 64^-1/4; a = w v^T.
// The two s factors are applied as one exact 2^-3 scale of q.
//
// Work split: workgroup = (sample, head, 128 queries); wave = 32 queries; key tiles of 64 through LDS.
//   S^T[key][query] = K . Q^T   : keys land in the 16 accumulator registers, the query on the lane, so the
//                                 softmax row reduction is 32 in-lane values + one exchange with lane^32.
//   O^T[c][query]  += V^T . P^T : the S^T accumulator IS the B operand (same lane = same query, register r of
//                                 lane-half h = key (r&3) + 8 (r>>2) + 4 h), no LDS round trip; the matching A
//                                 operand V[key(r,h)][c] is a conflict-free ds_read_b32 across 32 channels.
#include "kernels.h"
#include "conv_split.h"      // f32x16, f16x8, f16x4

namespace cddpm {

__global__ __launch_bounds__(256, 2) void attention_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                           int N, int C) {
    __shared__ float4 ldsK[64 * 16];   // [key][slot ^ (key & 15)]
    __shared__ float ldsV[64 * 64];    // [key][channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int heads = C >> 6;
    const int nqb = (N + 127) >> 7;
    int bid = blockIdx.x;
    const int qb = bid % nqb;
    bid /= nqb;
    const int hd = bid % heads;
    const int b = bid / heads;
    const int C3 = 3 * C;
    const float* base = qkv + (size_t)b * N * C3;

    // Q fragment of this lane's query: channels 8g + 4 lh + {0..3}, pre-scaled by 1/8
    const int query = qb * 128 + wave * 32 + li;
    const int qrow = min(query, N - 1);
    float4 qreg[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        float4 v = *reinterpret_cast<const float4*>(base + (size_t)qrow * C3 + hd * 64 + 8 * g + 4 * lh);
        v.x *= 0.125f; v.y *= 0.125f; v.z *= 0.125f; v.w *= 0.125f;
        qreg[g] = v;
    }

    f32x16 O[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[ct][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int k0 = 0; k0 < N; k0 += 64) {
        __syncthreads();   // previous tile fully consumed
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int key = e >> 4, slot = e & 15;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (k0 + key < N) {
                const float* rowp = base + (size_t)(k0 + key) * C3 + hd * 64 + 4 * slot;
                kv = *reinterpret_cast<const float4*>(rowp + C);
                vv = *reinterpret_cast<const float4*>(rowp + 2 * C);
            }
            ldsK[key * 16 + (slot ^ (key & 15))] = kv;
            *reinterpret_cast<float4*>(&ldsV[key * 64 + 4 * slot]) = vv;
        }
        __syncthreads();

        // ---- S^T = K . Q^T for 2 sub-tiles of 32 keys
        f32x16 S[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) S[kt][r] = 0.f;
            const int row = 32 * kt + li;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 kf = ldsK[row * 16 + ((2 * g + lh) ^ (row & 15))];
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qreg[g].x, S[kt], 0, 0, 0);
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qreg[g].y, S[kt], 0, 0, 0);
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qreg[g].z, S[kt], 0, 0, 0);
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qreg[g].w, S[kt], 0, 0, 0);
            }
        }

        // ---- online softmax over keys (registers + lane^32)
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (key >= N) S[kt][r] = -INFINITY;
                tmax = fmaxf(tmax, S[kt][r]);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __expf(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(S[kt][r] - m_new);
                S[kt][r] = p;
                psum += p;
            }
        psum += __shfl_xor(psum, 32, 64);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[ct][r] *= alpha;

        // ---- O^T += V^T . P^T
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float v0 = ldsV[key * 64 + li];
                const float v1 = ldsV[key * 64 + 32 + li];
                O[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, S[kt][r], O[0], 0, 0, 0);
                O[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, S[kt][r], O[1], 0, 0, 0);
            }
    }

    if (query < N) {
        const float inv = 1.0f / l_run;
        float* orow = out + ((size_t)b * N + query) * C + hd * 64;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float4 v;
                v.x = O[ct][4 * rq + 0] * inv;
                v.y = O[ct][4 * rq + 1] * inv;
                v.z = O[ct][4 * rq + 2] * inv;
                v.w = O[ct][4 * rq + 3] * inv;
                *reinterpret_cast<float4*>(orow + 32 * ct + 8 * rq + 4 * lh) = v;
            }
    }
}

void launch_attention(const float* qkv, float* out, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nqb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_kernel, dim3((unsigned)(B * heads * nqb)), dim3(256), 0, stream, qkv, out, N, C);
}

// ------------------------------------------------------------------------------------------------------------------
// The same forward with plain fp16 operands on v_mfma_f32_32x32x16_f16 (launch_attention_p16): the arithmetic of the reference's
// evaluation under `precision: 16` (fp16 autocast over QKVAttention.forward, OpenAI_Unet.py:457-476) with fp32 accumulators.
//   q (scaled by the exact 2^-3), k and v are rounded to fp16 (RNE) once, where they are staged; S and O accumulate in fp32; the
//   running max / sum softmax stays in fp32; P is rounded to fp16 only as the MFMA operand; the output is fp32.
// Work split and accumulator trick as above: workgroup = (sample, head, 128 queries), wave = 32 queries, key tiles of 64.
//   S^T[key][query] = K . Q^T   : 4 k-steps of 16 channels per 32-key sub-tile; A = a K row's 8 channels (ds_read_b128 of the
//                                 [key][channel] image, rows padded to 144 B: 16 consecutive rows cover the 16 four-bank groups),
//                                 B = the query's 8 channels, in registers for the whole kernel.
//   O^T[c][query]  += V^T . P^T : registers 8s .. 8s+7 of the S^T accumulator, rounded to fp16, ARE the B operand of k-step s:
//                                 element j of lane-half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3). The A operand is V^T[c][those
//                                 keys]: two 8-byte reads of the transposed [channel][key] image (rows padded to 136 B: 32
//                                 consecutive rows cover the 32 bank pairs), which the staging threads write as 4-key columns.
// One 64-key tile costs a wave 16 MFMAs of 32 cycles instead of 128 of 64.
__global__ __launch_bounds__(256, 2) void attention_p16_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                               int N, int C) {
    constexpr int KS = 72;   // fp16 elements of a K row (64 channels + 16 B)
    constexpr int VS = 68;   // fp16 elements of a V^T row (64 keys + 8 B)
    __shared__ __attribute__((aligned(16))) _Float16 ldsK[64 * KS];    // [key][channel]
    __shared__ __attribute__((aligned(16))) _Float16 ldsVt[64 * VS];   // [channel][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int heads = C >> 6;
    const int nqb = (N + 127) >> 7;
    int bid = blockIdx.x;
    const int qb = bid % nqb;
    bid /= nqb;
    const int hd = bid % heads;
    const int b = bid / heads;
    const int C3 = 3 * C;
    const float* base = qkv + (size_t)b * N * C3;

    // Q fragments of this lane's query: k-step s = channels 16 s + 8 lh + {0..7}, pre-scaled by 1/8, fp16
    const int query = qb * 128 + wave * 32 + li;
    const int qrow = min(query, N - 1);
    f16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float* qp = base + (size_t)qrow * C3 + hd * 64 + 16 * s + 8 * lh;
        const float4 a = *reinterpret_cast<const float4*>(qp);
        const float4 c = *reinterpret_cast<const float4*>(qp + 4);
        qf[s] = f16x8{(_Float16)(a.x * 0.125f), (_Float16)(a.y * 0.125f), (_Float16)(a.z * 0.125f), (_Float16)(a.w * 0.125f),
                      (_Float16)(c.x * 0.125f), (_Float16)(c.y * 0.125f), (_Float16)(c.z * 0.125f), (_Float16)(c.w * 0.125f)};
    }

    f32x16 O[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[ct][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int cq = tid & 15, kq = tid >> 4;     // staging: this thread's 4 channels x 4 keys of the tile
    for (int k0 = 0; k0 < N; k0 += 64) {
        float4 kv[4], vv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = k0 + 4 * kq + i;
            kv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            vv[i] = kv[i];
            if (key < N) {
                const float* rowp = base + (size_t)key * C3 + hd * 64 + 4 * cq;
                kv[i] = *reinterpret_cast<const float4*>(rowp + C);
                vv[i] = *reinterpret_cast<const float4*>(rowp + 2 * C);
            }
        }
        __syncthreads();   // previous tile fully consumed
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<f16x4*>(&ldsK[(4 * kq + i) * KS + 4 * cq]) =
                f16x4{(_Float16)kv[i].x, (_Float16)kv[i].y, (_Float16)kv[i].z, (_Float16)kv[i].w};
        *reinterpret_cast<f16x4*>(&ldsVt[(4 * cq + 0) * VS + 4 * kq]) = f16x4{(_Float16)vv[0].x, (_Float16)vv[1].x, (_Float16)vv[2].x, (_Float16)vv[3].x};
        *reinterpret_cast<f16x4*>(&ldsVt[(4 * cq + 1) * VS + 4 * kq]) = f16x4{(_Float16)vv[0].y, (_Float16)vv[1].y, (_Float16)vv[2].y, (_Float16)vv[3].y};
        *reinterpret_cast<f16x4*>(&ldsVt[(4 * cq + 2) * VS + 4 * kq]) = f16x4{(_Float16)vv[0].z, (_Float16)vv[1].z, (_Float16)vv[2].z, (_Float16)vv[3].z};
        *reinterpret_cast<f16x4*>(&ldsVt[(4 * cq + 3) * VS + 4 * kq]) = f16x4{(_Float16)vv[0].w, (_Float16)vv[1].w, (_Float16)vv[2].w, (_Float16)vv[3].w};
        __syncthreads();

        // ---- S^T = K . Q^T for 2 sub-tiles of 32 keys
        f32x16 S[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) S[kt][r] = 0.f;
            const _Float16* krow = &ldsK[(32 * kt + li) * KS + 8 * lh];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(krow + 16 * s), qf[s], S[kt], 0, 0, 0);
        }

        // ---- online softmax over keys (registers + lane^32), fp32
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (key >= N) S[kt][r] = -INFINITY;
                tmax = fmaxf(tmax, S[kt][r]);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __expf(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(S[kt][r] - m_new);
                S[kt][r] = p;
                psum += p;
            }
        psum += __shfl_xor(psum, 32, 64);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[ct][r] *= alpha;

        // ---- O^T += V^T . P^T
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (_Float16)S[kt][8 * s + j];
                const int key0 = 32 * kt + 16 * s + 4 * lh;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const _Float16* vp = &ldsVt[(32 * ct + li) * VS + key0];
                    const f16x4 lo = *reinterpret_cast<const f16x4*>(vp);
                    const f16x4 hi = *reinterpret_cast<const f16x4*>(vp + 8);
                    const f16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                    O[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, O[ct], 0, 0, 0);
                }
            }
    }

    if (query < N) {
        const float inv = 1.0f / l_run;
        float* orow = out + ((size_t)b * N + query) * C + hd * 64;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float4 v;
                v.x = O[ct][4 * rq + 0] * inv;
                v.y = O[ct][4 * rq + 1] * inv;
                v.z = O[ct][4 * rq + 2] * inv;
                v.w = O[ct][4 * rq + 3] * inv;
                *reinterpret_cast<float4*>(orow + 32 * ct + 8 * rq + 4 * lh) = v;
            }
    }
}

void launch_attention_p16(const float* qkv, float* out, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nqb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_p16_kernel, dim3((unsigned)(B * heads * nqb)), dim3(256), 0, stream, qkv, out, N, C);
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of the attention core, flash-style like the forward: the N x N matrices P and dS never leave registers.
// With S = (q / 8) . k, P = softmax_rows(S), a = P v and an upstream gradient dA:
//   D_i = sum_c dA_ic a_ic,   dP_ij = dA_i . v_j,   dS_ij = P_ij (dP_ij - D_i),
//   dq_i = (1/8) sum_j dS_ij k_j,   dk_j = sum_i dS_ij (q_i / 8),   dv_j = sum_i P_ij dA_i.
// Two kernels, both in the forward's layout trick (the accumulator of the first product IS the B operand of the second):
//   attention_bwd_q_kernel  : lane = query (as the forward). Sweep 1 over the key tiles is the forward itself (m_i, l_i, a_i -> D_i);
//                             sweep 2 forms S^T and dP^T = V . dA^T by MFMA, dS^T in registers, dQ^T += K^T . dS^T. Also writes
//                             (m_i + log l_i, D_i) per query for the second kernel.
//   attention_bwd_kv_kernel : lane = key. Per query tile: S = Q . K^T and dP = dA . V^T by MFMA (queries in the accumulator registers),
//                             P and dS in registers, dV^T += dA^T . P, dK^T += (Q/8)^T . dS.
// Exact fp32 products (v_mfma_f32_32x32x2_f32) as the forward. 7 N x N x 64 products + the forward's 2 instead of the 5 GEMM launches
// + 2 softmax passes over materialised [B heads][N][N] matrices of the first version (3.4 ms of a 16 x 128 x 128 training step).
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attention_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                 float* __restrict__ dqkv, float* __restrict__ stats /*[B][heads][N][2]*/,
                                                                 int N, int C) {
    __shared__ float4 ldsK[64 * 16];   // K tile, [key][slot ^ (key & 15)]
    __shared__ float4 ldsV4[64 * 16];  // V tile, same layout (A operand of dP^T = V . dA^T)
    __shared__ float ldsP[64 * 64];    // plain [key][channel]: V in sweep 1 (O^T += V^T P^T), K in sweep 2 (dQ^T += K^T dS^T)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int heads = C >> 6;
    const int nqb = (N + 127) >> 7;
    int bid = blockIdx.x;
    const int qb = bid % nqb;
    bid /= nqb;
    const int hd = bid % heads;
    const int b = bid / heads;
    const int C3 = 3 * C;
    const float* base = qkv + (size_t)b * N * C3;
    const int query = qb * 128 + wave * 32 + li;
    const int qrow = min(query, N - 1);
    float4 qreg[8], dareg[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        float4 v = *reinterpret_cast<const float4*>(base + (size_t)qrow * C3 + hd * 64 + 8 * g + 4 * lh);
        v.x *= 0.125f; v.y *= 0.125f; v.z *= 0.125f; v.w *= 0.125f;
        qreg[g] = v;
        dareg[g] = *reinterpret_cast<const float4*>(da + ((size_t)b * N + qrow) * C + hd * 64 + 8 * g + 4 * lh);
    }
    float m_run = -INFINITY, l_run = 0.f, Dq = 0.f;
    // ---------------- sweep 1: the forward (running max / sum, O^T) -> D
    {
        f32x16 O[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[ct][r] = 0.f;
        for (int k0 = 0; k0 < N; k0 += 64) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = tid + 256 * i;
                const int key = e >> 4, slot = e & 15;
                float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
                if (k0 + key < N) {
                    const float* rowp = base + (size_t)(k0 + key) * C3 + hd * 64 + 4 * slot;
                    kv = *reinterpret_cast<const float4*>(rowp + C);
                    vv = *reinterpret_cast<const float4*>(rowp + 2 * C);
                }
                ldsK[key * 16 + (slot ^ (key & 15))] = kv;
                *reinterpret_cast<float4*>(&ldsP[key * 64 + 4 * slot]) = vv;
            }
            __syncthreads();
            f32x16 S[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) S[kt][r] = 0.f;
                const int row = 32 * kt + li;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const float4 kf = ldsK[row * 16 + ((2 * g + lh) ^ (row & 15))];
                    S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qreg[g].x, S[kt], 0, 0, 0);
                    S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qreg[g].y, S[kt], 0, 0, 0);
                    S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qreg[g].z, S[kt], 0, 0, 0);
                    S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qreg[g].w, S[kt], 0, 0, 0);
                }
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= N) S[kt][r] = -INFINITY;
                    tmax = fmaxf(tmax, S[kt][r]);
                }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m_run, tmax);
            const float alpha = __expf(m_run - m_new);
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __expf(S[kt][r] - m_new);
                    S[kt][r] = pv;
                    psum += pv;
                }
            psum += __shfl_xor(psum, 32, 64);
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[ct][r] *= alpha;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const float v0 = ldsP[key * 64 + li];
                    const float v1 = ldsP[key * 64 + 32 + li];
                    O[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, S[kt][r], O[0], 0, 0, 0);
                    O[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, S[kt][r], O[1], 0, 0, 0);
                }
        }
        // D = sum_c dA_c a_c, a = O / l. O^T[c][query]: register 4 rq + x of tile ct = channel 32 ct + 8 rq + 4 lh + x, i.e. dareg[4 ct + rq]
        const float inv = 1.0f / l_run;
        float dsum = 0.f;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const float4 d4 = dareg[4 * ct + rq];
                dsum += d4.x * O[ct][4 * rq + 0] + d4.y * O[ct][4 * rq + 1] + d4.z * O[ct][4 * rq + 2] + d4.w * O[ct][4 * rq + 3];
            }
        dsum += __shfl_xor(dsum, 32, 64);
        Dq = dsum * inv;
    }
    const float lse = m_run + __logf(l_run);
    if (query < N && lh == 0) {
        float* st = stats + (((size_t)b * heads + hd) * N + query) * 2;
        st[0] = lse; st[1] = Dq;
    }
    // ---------------- sweep 2: dQ^T += K^T . dS^T
    f32x16 dQ[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[ct][r] = 0.f;
    for (int k0 = 0; k0 < N; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int key = e >> 4, slot = e & 15;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (k0 + key < N) {
                const float* rowp = base + (size_t)(k0 + key) * C3 + hd * 64 + 4 * slot;
                kv = *reinterpret_cast<const float4*>(rowp + C);
                vv = *reinterpret_cast<const float4*>(rowp + 2 * C);
            }
            ldsK[key * 16 + (slot ^ (key & 15))] = kv;
            ldsV4[key * 16 + (slot ^ (key & 15))] = vv;
            *reinterpret_cast<float4*>(&ldsP[key * 64 + 4 * slot]) = kv;
        }
        __syncthreads();
        f32x16 S[2], dP[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { S[kt][r] = 0.f; dP[kt][r] = 0.f; }
            const int row = 32 * kt + li;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 kf = ldsK[row * 16 + ((2 * g + lh) ^ (row & 15))];
                const float4 vf = ldsV4[row * 16 + ((2 * g + lh) ^ (row & 15))];
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qreg[g].x, S[kt], 0, 0, 0);
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qreg[g].y, S[kt], 0, 0, 0);
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qreg[g].z, S[kt], 0, 0, 0);
                S[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qreg[g].w, S[kt], 0, 0, 0);
                dP[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.x, dareg[g].x, dP[kt], 0, 0, 0);
                dP[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.y, dareg[g].y, dP[kt], 0, 0, 0);
                dP[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.z, dareg[g].z, dP[kt], 0, 0, 0);
                dP[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.w, dareg[g].w, dP[kt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float pv = (key < N) ? __expf(S[kt][r] - lse) : 0.f;
                S[kt][r] = pv * (dP[kt][r] - Dq);            // dS^T
            }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float k0v = ldsP[key * 64 + li];
                const float k1v = ldsP[key * 64 + 32 + li];
                dQ[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(k0v, S[kt][r], dQ[0], 0, 0, 0);
                dQ[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(k1v, S[kt][r], dQ[1], 0, 0, 0);
            }
    }
    if (query < N) {
        float* orow = dqkv + ((size_t)b * N + query) * C3 + hd * 64;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float4 v;
                v.x = dQ[ct][4 * rq + 0] * 0.125f; v.y = dQ[ct][4 * rq + 1] * 0.125f;
                v.z = dQ[ct][4 * rq + 2] * 0.125f; v.w = dQ[ct][4 * rq + 3] * 0.125f;
                *reinterpret_cast<float4*>(orow + 32 * ct + 8 * rq + 4 * lh) = v;
            }
    }
}

__global__ __launch_bounds__(256, 2) void attention_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                  float* __restrict__ dqkv, const float* __restrict__ stats, int N, int C) {
    __shared__ float4 ldsQ4[64 * 16];   // (Q / 8) tile, [query][slot ^ (query & 15)]: A operand of S = Q . K^T
    __shared__ float4 ldsA4[64 * 16];   // dA tile, same layout: A operand of dP = dA . V^T
    __shared__ float ldsQp[64 * 64];    // plain [query][channel] copies: A operands of dK^T += Q^T dS and dV^T += dA^T P
    __shared__ float ldsAp[64 * 64];
    __shared__ float ldsL[64], ldsD[64];   // per query: m + log l, D
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int heads = C >> 6;
    const int nkb = (N + 127) >> 7;
    int bid = blockIdx.x;
    const int kb = bid % nkb;
    bid /= nkb;
    const int hd = bid % heads;
    const int b = bid / heads;
    const int C3 = 3 * C;
    const float* base = qkv + (size_t)b * N * C3;
    const int keyi = kb * 128 + wave * 32 + li;
    const int krow = min(keyi, N - 1);
    float4 kreg[8], vreg[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        kreg[g] = *reinterpret_cast<const float4*>(base + (size_t)krow * C3 + C + hd * 64 + 8 * g + 4 * lh);
        vreg[g] = *reinterpret_cast<const float4*>(base + (size_t)krow * C3 + 2 * C + hd * 64 + 8 * g + 4 * lh);
    }
    f32x16 dK[2], dV[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dK[ct][r] = 0.f; dV[ct][r] = 0.f; }
    const float* st = stats + ((size_t)b * heads + hd) * N * 2;
    for (int q0 = 0; q0 < N; q0 += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int qq = e >> 4, slot = e & 15;
            float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), av = qv;
            if (q0 + qq < N) {
                qv = *reinterpret_cast<const float4*>(base + (size_t)(q0 + qq) * C3 + hd * 64 + 4 * slot);
                qv.x *= 0.125f; qv.y *= 0.125f; qv.z *= 0.125f; qv.w *= 0.125f;
                av = *reinterpret_cast<const float4*>(da + ((size_t)b * N + q0 + qq) * C + hd * 64 + 4 * slot);
            }
            ldsQ4[qq * 16 + (slot ^ (qq & 15))] = qv;
            ldsA4[qq * 16 + (slot ^ (qq & 15))] = av;
            *reinterpret_cast<float4*>(&ldsQp[qq * 64 + 4 * slot]) = qv;
            *reinterpret_cast<float4*>(&ldsAp[qq * 64 + 4 * slot]) = av;
        }
        if (tid < 64) {
            const bool ok = q0 + tid < N;
            ldsL[tid] = ok ? st[(size_t)(q0 + tid) * 2] : INFINITY;      // exp(S - inf) = 0: queries past the end contribute nothing
            ldsD[tid] = ok ? st[(size_t)(q0 + tid) * 2 + 1] : 0.f;
        }
        __syncthreads();
        // S[query][key] = (Q/8) . K^T and dP[query][key] = dA . V^T: queries in the accumulator registers, the key on the lane;
        // one 32-query sub-tile at a time (32 instead of 64 live accumulator registers for S and dP: no spills)
#pragma unroll 1
        for (int qt = 0; qt < 2; ++qt) {
            f32x16 S, dP;
#pragma unroll
            for (int r = 0; r < 16; ++r) { S[r] = 0.f; dP[r] = 0.f; }
            const int row = 32 * qt + li;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 qf = ldsQ4[row * 16 + ((2 * g + lh) ^ (row & 15))];
                const float4 af = ldsA4[row * 16 + ((2 * g + lh) ^ (row & 15))];
                S = __builtin_amdgcn_mfma_f32_32x32x2f32(qf.x, kreg[g].x, S, 0, 0, 0);
                S = __builtin_amdgcn_mfma_f32_32x32x2f32(qf.y, kreg[g].y, S, 0, 0, 0);
                S = __builtin_amdgcn_mfma_f32_32x32x2f32(qf.z, kreg[g].z, S, 0, 0, 0);
                S = __builtin_amdgcn_mfma_f32_32x32x2f32(qf.w, kreg[g].w, S, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, vreg[g].x, dP, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, vreg[g].y, dP, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, vreg[g].z, dP, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, vreg[g].w, dP, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = 32 * qt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float pv = __expf(S[r] - ldsL[qq]);
                const float ds = pv * (dP[r] - ldsD[qq]);
                const float a0 = ldsAp[qq * 64 + li], a1 = ldsAp[qq * 64 + 32 + li];
                const float x0 = ldsQp[qq * 64 + li], x1 = ldsQp[qq * 64 + 32 + li];
                dV[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, pv, dV[0], 0, 0, 0);
                dV[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, pv, dV[1], 0, 0, 0);
                dK[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, ds, dK[0], 0, 0, 0);
                dK[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, ds, dK[1], 0, 0, 0);
            }
        }
    }
    if (keyi < N) {
        float* krow_o = dqkv + ((size_t)b * N + keyi) * C3 + C + hd * 64;
        float* vrow_o = krow_o + C;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                *reinterpret_cast<float4*>(krow_o + 32 * ct + 8 * rq + 4 * lh) =
                    make_float4(dK[ct][4 * rq + 0], dK[ct][4 * rq + 1], dK[ct][4 * rq + 2], dK[ct][4 * rq + 3]);
                *reinterpret_cast<float4*>(vrow_o + 32 * ct + 8 * rq + 4 * lh) =
                    make_float4(dV[ct][4 * rq + 0], dV[ct][4 * rq + 1], dV[ct][4 * rq + 2], dV[ct][4 * rq + 3]);
            }
    }
}

// stats: [B][heads][N][2] floats of scratch
void launch_attention_backward_flash(const float* qkv, const float* da, float* dqkv, float* stats, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_bwd_q_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), 0, stream, qkv, da, dqkv, stats, N, C);
    hipLaunchKernelGGL(attention_bwd_kv_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), 0, stream, qkv, da, dqkv, stats, N, C);
}

// ------------------------------------------------------------------------------------------------------------------
// The same backward with plain fp16 operands on v_mfma_f32_32x32x16_f16 (launch_attention_backward_p16): the arithmetic of fp16
// autocast over QKVAttention.forward and its backward (the reference trains under `precision: 16`), with fp32 accumulators.
//   q . 2^-3, k, v and dA are rounded to fp16 (RNE, gradual underflow) once, where they are staged; S, dP, dQ, dK and dV accumulate in
//   fp32; the running max / sum, P = exp(S - lse), D_i = sum_c dA_ic a_ic (rounded dA, fp32 sweep-1 output) and dS = P (dP - D) are
//   fp32 VALU work; P and dS are rounded to fp16 only as MFMA operands; dqkv is fp32. |dA| >= 65504 rounds to +-inf as under autocast
//   and gives non-finite gradients of that sample (what the loss scale's device guard catches), never a finite wrong number.
// Two kernels, work split, masking and row statistics as the fp32 pair above; LDS images as attention_p16_kernel:
//   row images [row][channel], 144-B rows : A operands of the first products (ds_read_b128 of a row's 8 channels)
//   transposed images [channel][row], 136-B rows, written as 4-row columns : A operands of the second products (2 x ds_read_b64);
//   registers 8s .. 8s+7 of a first product's accumulator, rounded to fp16, are the B operand of k-step s of the second.
//   attention_bwd_q_p16_kernel  : sweep 1 = attention_p16_kernel (K rows, V^T); sweep 2: K rows, V rows, K^T (27 KB)
//   attention_bwd_kv_p16_kernel : k, v fragments in registers; per 64-query tile Q/8 and dA rows, (Q/8)^T and dA^T (35 KB)
// Per 64-row tile a wave issues 16 + 24 (q kernel, sweeps 1 + 2) and 32 (kv kernel) MFMAs of 32 cycles instead of 128 + 192 and 256 of 64.
// ------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int P16_RS = 72;   // fp16 elements of a row-image row (64 channels + 16 B)
constexpr int P16_TS = 68;   // fp16 elements of a transposed-image row (64 rows + 8 B)

__device__ __forceinline__ f16x4 p16_round4(float x, float y, float z, float w) {
    return f16x4{(_Float16)x, (_Float16)y, (_Float16)z, (_Float16)w};
}
// this staging thread's 4 rows x 4 channels (rows 4 kq + i, channels 4 cq + {0..3}) into a row image / a transposed image
__device__ __forceinline__ void p16_stage_rows(_Float16* img, int kq, int cq, const float4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<f16x4*>(&img[(4 * kq + i) * P16_RS + 4 * cq]) = p16_round4(v[i].x, v[i].y, v[i].z, v[i].w);
}
__device__ __forceinline__ void p16_stage_cols(_Float16* img, int kq, int cq, const float4 (&v)[4]) {
    *reinterpret_cast<f16x4*>(&img[(4 * cq + 0) * P16_TS + 4 * kq]) = p16_round4(v[0].x, v[1].x, v[2].x, v[3].x);
    *reinterpret_cast<f16x4*>(&img[(4 * cq + 1) * P16_TS + 4 * kq]) = p16_round4(v[0].y, v[1].y, v[2].y, v[3].y);
    *reinterpret_cast<f16x4*>(&img[(4 * cq + 2) * P16_TS + 4 * kq]) = p16_round4(v[0].z, v[1].z, v[2].z, v[3].z);
    *reinterpret_cast<f16x4*>(&img[(4 * cq + 3) * P16_TS + 4 * kq]) = p16_round4(v[0].w, v[1].w, v[2].w, v[3].w);
}
// 8 channels of a global row as one fp16 MFMA fragment, scaled by `scale` before rounding
__device__ __forceinline__ f16x8 p16_fragment(const float* p, float scale) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 c = *reinterpret_cast<const float4*>(p + 4);
    return f16x8{(_Float16)(a.x * scale), (_Float16)(a.y * scale), (_Float16)(a.z * scale), (_Float16)(a.w * scale),
                 (_Float16)(c.x * scale), (_Float16)(c.y * scale), (_Float16)(c.z * scale), (_Float16)(c.w * scale)};
}
// acc[ct] += T^T-image[channel 32 ct + li][rows row0 + {0..3}, row0 + 8 + {0..3}] . bf for both channel tiles
__device__ __forceinline__ void p16_second_product(f32x16 (&acc)[2], const _Float16* timg, int li, int row0, f16x8 bf) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const _Float16* tp = &timg[(32 * ct + li) * P16_TS + row0];
        const f16x4 lo = *reinterpret_cast<const f16x4*>(tp);
        const f16x4 hi = *reinterpret_cast<const f16x4*>(tp + 8);
        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7), bf, acc[ct], 0, 0, 0);
    }
}
}  // namespace

__global__ __launch_bounds__(256, 2) void attention_bwd_q_p16_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                     float* __restrict__ dqkv, float* __restrict__ stats /*[B][heads][N][2]*/,
                                                                     int N, int C) {
    __shared__ __attribute__((aligned(16))) _Float16 ldsK[64 * P16_RS];   // K rows [key][channel]
    __shared__ __attribute__((aligned(16))) _Float16 ldsV[64 * P16_RS];   // V rows [key][channel] (sweep 2: A operand of dP^T = V . dA^T)
    __shared__ __attribute__((aligned(16))) _Float16 ldsT[64 * P16_TS];   // [channel][key]: V^T in sweep 1, K^T in sweep 2
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int heads = C >> 6;
    const int nqb = (N + 127) >> 7;
    int bid = blockIdx.x;
    const int qb = bid % nqb;
    bid /= nqb;
    const int hd = bid % heads;
    const int b = bid / heads;
    const int C3 = 3 * C;
    const float* base = qkv + (size_t)b * N * C3;
    const int query = qb * 128 + wave * 32 + li;
    const int qrow = min(query, N - 1);
    const float* darow = da + ((size_t)b * N + qrow) * C + hd * 64;
    // fragments of this lane's query: k-step s = channels 16 s + 8 lh + {0..7}; q pre-scaled by 1/8
    f16x8 qf[4], daf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qf[s] = p16_fragment(base + (size_t)qrow * C3 + hd * 64 + 16 * s + 8 * lh, 0.125f);
        daf[s] = p16_fragment(darow + 16 * s + 8 * lh, 1.0f);
    }
    const int cq = tid & 15, kq = tid >> 4;     // staging: this thread's 4 channels x 4 keys of the tile
    float m_run = -INFINITY, l_run = 0.f, Dq = 0.f;
    // ---------------- sweep 1: the p16 forward (running max / sum, O^T) -> D
    {
        f32x16 O[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[ct][r] = 0.f;
        for (int k0 = 0; k0 < N; k0 += 64) {
            float4 kv[4], vv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + 4 * kq + i;
                kv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                vv[i] = kv[i];
                if (key < N) {
                    const float* rowp = base + (size_t)key * C3 + hd * 64 + 4 * cq;
                    kv[i] = *reinterpret_cast<const float4*>(rowp + C);
                    vv[i] = *reinterpret_cast<const float4*>(rowp + 2 * C);
                }
            }
            __syncthreads();   // previous tile fully consumed
            p16_stage_rows(ldsK, kq, cq, kv);
            p16_stage_cols(ldsT, kq, cq, vv);
            __syncthreads();
            f32x16 S[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) S[kt][r] = 0.f;
                const _Float16* krow = &ldsK[(32 * kt + li) * P16_RS + 8 * lh];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    S[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(krow + 16 * s), qf[s], S[kt], 0, 0, 0);
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= N) S[kt][r] = -INFINITY;
                    tmax = fmaxf(tmax, S[kt][r]);
                }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m_run, tmax);
            const float alpha = __expf(m_run - m_new);
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __expf(S[kt][r] - m_new);
                    S[kt][r] = pv;
                    psum += pv;
                }
            psum += __shfl_xor(psum, 32, 64);
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[ct][r] *= alpha;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    f16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (_Float16)S[kt][8 * s + j];
                    p16_second_product(O, ldsT, li, 32 * kt + 16 * s + 4 * lh, pf);
                }
        }
        // D = sum_c dA_c a_c, a = O / l, with the fp16-rounded dA. O^T[c][query]: register 4 rq + x of tile ct = channel
        // 32 ct + 8 rq + 4 lh + x -- not the channels of this lane's MFMA fragments, so those 32 values are read again
        const float inv = 1.0f / l_run;
        float dsum = 0.f;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const float4 d4 = *reinterpret_cast<const float4*>(darow + 32 * ct + 8 * rq + 4 * lh);
                dsum += (float)(_Float16)d4.x * O[ct][4 * rq + 0] + (float)(_Float16)d4.y * O[ct][4 * rq + 1] +
                        (float)(_Float16)d4.z * O[ct][4 * rq + 2] + (float)(_Float16)d4.w * O[ct][4 * rq + 3];
            }
        dsum += __shfl_xor(dsum, 32, 64);
        Dq = dsum * inv;
    }
    const float lse = m_run + __logf(l_run);
    if (query < N && lh == 0) {
        float* st = stats + (((size_t)b * heads + hd) * N + query) * 2;
        st[0] = lse; st[1] = Dq;
    }
    // ---------------- sweep 2: S^T = K . Q^T, dP^T = V . dA^T, dQ^T += K^T . dS^T
    f32x16 dQ[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[ct][r] = 0.f;
    for (int k0 = 0; k0 < N; k0 += 64) {
        float4 kv[4], vv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = k0 + 4 * kq + i;
            kv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            vv[i] = kv[i];
            if (key < N) {
                const float* rowp = base + (size_t)key * C3 + hd * 64 + 4 * cq;
                kv[i] = *reinterpret_cast<const float4*>(rowp + C);
                vv[i] = *reinterpret_cast<const float4*>(rowp + 2 * C);
            }
        }
        __syncthreads();   // previous tile (or sweep 1's last) fully consumed
        p16_stage_rows(ldsK, kq, cq, kv);
        p16_stage_rows(ldsV, kq, cq, vv);
        p16_stage_cols(ldsT, kq, cq, kv);
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16 S, dP;
#pragma unroll
            for (int r = 0; r < 16; ++r) { S[r] = 0.f; dP[r] = 0.f; }
            const _Float16* krow = &ldsK[(32 * kt + li) * P16_RS + 8 * lh];
            const _Float16* vrow = &ldsV[(32 * kt + li) * P16_RS + 8 * lh];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                S = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(krow + 16 * s), qf[s], S, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(vrow + 16 * s), daf[s], dP, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float pv = (key < N) ? __expf(S[r] - lse) : 0.f;
                S[r] = pv * (dP[r] - Dq);            // dS^T
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f16x8 dsf;
#pragma unroll
                for (int j = 0; j < 8; ++j) dsf[j] = (_Float16)S[8 * s + j];
                p16_second_product(dQ, ldsT, li, 32 * kt + 16 * s + 4 * lh, dsf);
            }
        }
    }
    if (query < N) {
        float* orow = dqkv + ((size_t)b * N + query) * C3 + hd * 64;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float4 v;
                v.x = dQ[ct][4 * rq + 0] * 0.125f; v.y = dQ[ct][4 * rq + 1] * 0.125f;
                v.z = dQ[ct][4 * rq + 2] * 0.125f; v.w = dQ[ct][4 * rq + 3] * 0.125f;
                *reinterpret_cast<float4*>(orow + 32 * ct + 8 * rq + 4 * lh) = v;
            }
    }
}

__global__ __launch_bounds__(256, 2) void attention_bwd_kv_p16_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                      float* __restrict__ dqkv, const float* __restrict__ stats, int N, int C) {
    __shared__ __attribute__((aligned(16))) _Float16 ldsQ[64 * P16_RS];    // (Q / 8) rows [query][channel]: A operand of S = Q . K^T
    __shared__ __attribute__((aligned(16))) _Float16 ldsA[64 * P16_RS];    // dA rows: A operand of dP = dA . V^T
    __shared__ __attribute__((aligned(16))) _Float16 ldsQt[64 * P16_TS];   // [channel][query] images: A operands of dK^T += (Q/8)^T dS
    __shared__ __attribute__((aligned(16))) _Float16 ldsAt[64 * P16_TS];   //                          and dV^T += dA^T P
    __shared__ float ldsL[64], ldsD[64];   // per query: m + log l, D
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int heads = C >> 6;
    const int nkb = (N + 127) >> 7;
    int bid = blockIdx.x;
    const int kb = bid % nkb;
    bid /= nkb;
    const int hd = bid % heads;
    const int b = bid / heads;
    const int C3 = 3 * C;
    const float* base = qkv + (size_t)b * N * C3;
    const int keyi = kb * 128 + wave * 32 + li;
    const int krow = min(keyi, N - 1);
    // fragments of this lane's key: k-step s = channels 16 s + 8 lh + {0..7}
    f16x8 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        kf[s] = p16_fragment(base + (size_t)krow * C3 + C + hd * 64 + 16 * s + 8 * lh, 1.0f);
        vf[s] = p16_fragment(base + (size_t)krow * C3 + 2 * C + hd * 64 + 16 * s + 8 * lh, 1.0f);
    }
    f32x16 dK[2], dV[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dK[ct][r] = 0.f; dV[ct][r] = 0.f; }
    const float* st = stats + ((size_t)b * heads + hd) * N * 2;
    const int cq = tid & 15, kq = tid >> 4;     // staging: this thread's 4 channels x 4 queries of the tile
    for (int q0 = 0; q0 < N; q0 += 64) {
        float4 qv[4], av[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int qq = q0 + 4 * kq + i;
            qv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            av[i] = qv[i];
            if (qq < N) {
                qv[i] = *reinterpret_cast<const float4*>(base + (size_t)qq * C3 + hd * 64 + 4 * cq);
                qv[i].x *= 0.125f; qv[i].y *= 0.125f; qv[i].z *= 0.125f; qv[i].w *= 0.125f;
                av[i] = *reinterpret_cast<const float4*>(da + ((size_t)b * N + qq) * C + hd * 64 + 4 * cq);
            }
        }
        float lq = INFINITY, dq_ = 0.f;      // exp(S - inf) = 0: queries past the end contribute nothing
        if (tid < 64 && q0 + tid < N) {
            lq = st[(size_t)(q0 + tid) * 2];
            dq_ = st[(size_t)(q0 + tid) * 2 + 1];
        }
        __syncthreads();   // previous tile fully consumed
        p16_stage_rows(ldsQ, kq, cq, qv);
        p16_stage_rows(ldsA, kq, cq, av);
        p16_stage_cols(ldsQt, kq, cq, qv);
        p16_stage_cols(ldsAt, kq, cq, av);
        if (tid < 64) { ldsL[tid] = lq; ldsD[tid] = dq_; }
        __syncthreads();
        // S[query][key] = (Q/8) . K^T and dP[query][key] = dA . V^T: queries in the accumulator registers, the key on the lane
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            f32x16 S, dP;
#pragma unroll
            for (int r = 0; r < 16; ++r) { S[r] = 0.f; dP[r] = 0.f; }
            const _Float16* qrow = &ldsQ[(32 * qt + li) * P16_RS + 8 * lh];
            const _Float16* arow = &ldsA[(32 * qt + li) * P16_RS + 8 * lh];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                S = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(qrow + 16 * s), kf[s], S, 0, 0, 0);
                dP = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(arow + 16 * s), vf[s], dP, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = 32 * qt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float pv = __expf(S[r] - ldsL[qq]);
                S[r] = pv;
                dP[r] = pv * (dP[r] - ldsD[qq]);     // dS
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f16x8 pf, dsf;
#pragma unroll
                for (int j = 0; j < 8; ++j) { pf[j] = (_Float16)S[8 * s + j]; dsf[j] = (_Float16)dP[8 * s + j]; }
                const int row0 = 32 * qt + 16 * s + 4 * lh;
                p16_second_product(dV, ldsAt, li, row0, pf);
                p16_second_product(dK, ldsQt, li, row0, dsf);
            }
        }
    }
    if (keyi < N) {
        float* krow_o = dqkv + ((size_t)b * N + keyi) * C3 + C + hd * 64;
        float* vrow_o = krow_o + C;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                *reinterpret_cast<float4*>(krow_o + 32 * ct + 8 * rq + 4 * lh) =
                    make_float4(dK[ct][4 * rq + 0], dK[ct][4 * rq + 1], dK[ct][4 * rq + 2], dK[ct][4 * rq + 3]);
                *reinterpret_cast<float4*>(vrow_o + 32 * ct + 8 * rq + 4 * lh) =
                    make_float4(dV[ct][4 * rq + 0], dV[ct][4 * rq + 1], dV[ct][4 * rq + 2], dV[ct][4 * rq + 3]);
            }
    }
}

// stats: [B][heads][N][2] floats of scratch, as launch_attention_backward_flash
void launch_attention_backward_p16(const float* qkv, const float* da, float* dqkv, float* stats, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_bwd_q_p16_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), 0, stream, qkv, da, dqkv, stats, N, C);
    hipLaunchKernelGGL(attention_bwd_kv_p16_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), 0, stream, qkv, da, dqkv, stats, N, C);
}

}  // namespace cddpm
