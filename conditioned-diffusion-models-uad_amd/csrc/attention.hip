// Self-attention core for gfx950: softmax(q k^T / sqrt(d)) v, d = 64, flash-style (the N x N score matrix never leaves registers),
// forward and backward, in three arithmetics: exact fp32 on v_mfma_f32_32x32x2_f32, plain fp16 operands on v_mfma_f32_32x32x16_f16, and
// h3 on the same 16-bit instruction: fp32-grade products from two-term fp16 splits (hi . hi + hi . lo + lo . hi), opt-in per handle / call.
//
// Replaces QKVAttention.forward (src/models/modules/OpenAI_Unet.py:457-476): q,k,v = chunk(qkv, 3);
// heads are contiguous groups of 64 channels; w = softmax_fp32((q s)^T (k s)), s = 64^-1/4; a = w v^T.
// The two s factors are applied as one exact 2^-3 scale of q.
//
// Ten kernels behind six launchers (per arithmetic a forward, a bwd_q and a bwd_kv kernel; h3 also the pass that takes each sample's
// largest |dA|); what they share exists once, as __device__ functions: the workgroup decode, the row store,
// the online-softmax tile step, per arithmetic the stage / first-product / second-product pieces, and per arithmetic the forward
// sweep over the key tiles, which is the forward kernel's body and sweep 1 of the bwd_q kernel. MFMA accumulators go through these
// helpers by value and come back in small structs, and the two sub-tiles of a tile are a two-element array walked by an unrolled
// loop: the same code with f32x16 (&)[2] parameters, or with the two sub-tiles spelled out as two calls, costs attention_kernel and
// attention_p16_kernel a wave per SIMD (161 -> 186 / 171 and 127 -> 140 VGPRs) at unchanged instruction counts.
#include "kernels.h"
#include "conv_split.h"      // f32x16, f16x8, f16x4

namespace cddpm {
namespace {

// Work split: workgroup = (sample, head, block of 128 rows); wave = 32 rows, one per lane li of lane-half lh; the other side of the
// N x N matrix comes in tiles of 64 rows through LDS. The rows are queries in the forward and the bwd_q kernels, keys in bwd_kv.
struct Wg {
    int tid, li, lh;
    int heads, hd, b, C3;
    int row;             // this lane's query / key; past the end in the last block's tail (loads clamp it, stores skip it)
    const float* base;   // qkv of sample b, [N][3C]
};
__device__ __forceinline__ Wg wg_decode(const float* qkv, int N, int C) {
    Wg w;
    w.tid = threadIdx.x;
    const int lane = w.tid & 63, wave = w.tid >> 6;
    w.li = lane & 31;
    w.lh = lane >> 5;
    w.heads = C >> 6;
    const int nblk = (N + 127) >> 7;
    int bid = blockIdx.x;
    const int blk = bid % nblk;
    bid /= nblk;
    w.hd = bid % w.heads;
    w.b = bid / w.heads;
    w.C3 = 3 * C;
    w.base = qkv + (size_t)w.b * N * w.C3;
    w.row = blk * 128 + wave * 32 + w.li;
    return w;
}

// A [64 channels][32 rows] fp32 accumulator (O^T, dQ^T, dK^T, dV^T): channel tiles 0 and 1, the row on the lane.
struct Acc2 { f32x16 t[2]; };

// An accumulator as 64 channels of its lane's global row: register 4 rq + x of tile ct = channel 32 ct + 8 rq + 4 lh + x.
__device__ __forceinline__ void store_row(float* row, Acc2 acc, int lh) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq)
            *reinterpret_cast<float4*>(row + 32 * ct + 8 * rq + 4 * lh) =
                make_float4(acc.t[ct][4 * rq + 0], acc.t[ct][4 * rq + 1], acc.t[ct][4 * rq + 2], acc.t[ct][4 * rq + 3]);
}
__device__ __forceinline__ void store_row(float* row, Acc2 acc, float scale, int lh) {
    acc.t[0] *= scale;
    acc.t[1] *= scale;
    store_row(row, acc, lh);
}

// Online softmax over one 64-key tile of S^T (keys k0 .. k0 + 63 in the registers of S0, S1; register r of lane-half h = key
// (r & 3) + 8 (r >> 2) + 4 h of its 32-key sub-tile), fp32 VALU in both arithmetics: keys past N are masked, the row reduction is
// 32 in-lane values + one exchange with lane^32. The caller folds alpha and psum into its running sum and rescales O by alpha.
struct SoftmaxTile { f32x16 P[2]; float m_new, alpha, psum; };
__device__ __forceinline__ SoftmaxTile softmax_tile(f32x16 S0, f32x16 S1, float m_run, int k0, int N, int lh) {
    f32x16 P[2] = {S0, S1};
    float psum = 0.f;
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (key >= N) P[kt][r] = -INFINITY;
            tmax = fmaxf(tmax, P[kt][r]);
        }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __expf(m_run - m_new);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __expf(P[kt][r] - m_new);
            P[kt][r] = p;
            psum += p;
        }
    psum += __shfl_xor(psum, 32, 64);
    return SoftmaxTile{{P[0], P[1]}, m_new, alpha, psum};
}

// What a forward sweep leaves per query: O^T (not yet divided by l), the running max and the running sum.
struct Sweep { Acc2 O; float m, l; };

// ------------------------------------------------------------------------------------------------------------------
// Exact fp32 on v_mfma_f32_32x32x2_f32.
//   first product  S^T[key][query] = K . Q^T   : keys land in the 16 accumulator registers, the query on the lane.
//   second product O^T[c][query]  += V^T . P^T : the S^T accumulator IS the B operand (same lane = same query, register r of
//                                 lane-half h = key (r&3) + 8 (r>>2) + 4 h), no LDS round trip; the matching A
//                                 operand V[key(r,h)][c] is a conflict-free ds_read_b32 across 32 channels.
// The backward's products have the same two shapes with other matrices in the roles of K, Q, V and P.
// ------------------------------------------------------------------------------------------------------------------

// This lane's B operand of a first product: channels 8 g + 4 lh + {0..3} of a global row, EIGHTH: scaled by the exact 2^-3.
template <bool EIGHTH>
__device__ __forceinline__ void f32_fragment(float4 (&f)[8], const float* row, int lh) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        float4 v = *reinterpret_cast<const float4*>(row + 8 * g + 4 * lh);
        if (EIGHTH) { v.x *= 0.125f; v.y *= 0.125f; v.z *= 0.125f; v.w *= 0.125f; }
        f[g] = v;
    }
}

// Stage rows r0 .. r0 + 63 (zero past N) of two matrices, 64 channels from pa / pb with row strides sa / sb, 256 threads x 4 float4
// each: into a swizzled image [row][slot ^ (row & 15)] (A operand of a first product) and / or a plain image [row][64] (A operand of
// a second product). A null image is skipped. EIGHTH_A: matrix a is scaled by the exact 2^-3.
template <bool EIGHTH_A>
__device__ __forceinline__ void f32_stage(int tid, int r0, int N, const float* pa, int sa, const float* pb, int sb,
                                          float4* swz_a, float* plain_a, float4* swz_b, float* plain_b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i;
        const int row = e >> 4, slot = e & 15;
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
        if (r0 + row < N) {
            av = *reinterpret_cast<const float4*>(pa + (size_t)(r0 + row) * sa + 4 * slot);
            if (EIGHTH_A) { av.x *= 0.125f; av.y *= 0.125f; av.z *= 0.125f; av.w *= 0.125f; }
            bv = *reinterpret_cast<const float4*>(pb + (size_t)(r0 + row) * sb + 4 * slot);
        }
        if (swz_a) swz_a[row * 16 + (slot ^ (row & 15))] = av;
        if (swz_b) swz_b[row * 16 + (slot ^ (row & 15))] = bv;
        if (plain_a) *reinterpret_cast<float4*>(&plain_a[row * 64 + 4 * slot]) = av;
        if (plain_b) *reinterpret_cast<float4*>(&plain_b[row * 64 + 4 * slot]) = bv;
    }
}

// swizzled image[row][64 channels] . frag: one 32 x 32 tile, image row `row` (32 sub + li) in this lane's A operand
__device__ __forceinline__ f32x16 f32_first_product(const float4* swz, int row, int lh, const float4 (&frag)[8]) {
    f32x16 acc = {};
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const float4 a = swz[row * 16 + ((2 * g + lh) ^ (row & 15))];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, frag[g].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, frag[g].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, frag[g].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, frag[g].w, acc, 0, 0, 0);
    }
    return acc;
}

// acc += plain image[row][channels 32 ct + li] x bv for both channel tiles: one register's step of a second product
__device__ __forceinline__ Acc2 f32_second_step(Acc2 acc, const float* plain, int row, int li, float bv) {
    const float a0 = plain[row * 64 + li];
    const float a1 = plain[row * 64 + 32 + li];
    acc.t[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc.t[0], 0, 0, 0);
    acc.t[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc.t[1], 0, 0, 0);
    return acc;
}
// acc += image^T . bf over the 32 rows of a sub-tile whose first-product accumulator is bf; row0 = 32 sub + 4 lh
__device__ __forceinline__ Acc2 f32_second_product(Acc2 acc, const float* plain, int li, int row0, f32x16 bf) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = f32_second_step(acc, plain, row0 + (r & 3) + 8 * (r >> 2), li, bf[r]);
    return acc;
}

// The forward over all key tiles for this lane's query (fragment qreg, pre-scaled by 1/8). ldsK: swizzled K tile, ldsV: plain V tile.
__device__ __forceinline__ Sweep f32_forward_sweep(const Wg& w, const float4 (&qreg)[8], float4* ldsK, float* ldsV, int N, int C) {
    const float* kp = w.base + C + w.hd * 64;
    Sweep f = {{}, -INFINITY, 0.f};
    for (int k0 = 0; k0 < N; k0 += 64) {
        __syncthreads();   // previous tile fully consumed
        f32_stage<false>(w.tid, k0, N, kp, w.C3, kp + C, w.C3, ldsK, nullptr, nullptr, ldsV);
        __syncthreads();
        f32x16 S[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) S[kt] = f32_first_product(ldsK, 32 * kt + w.li, w.lh, qreg);
        const SoftmaxTile t = softmax_tile(S[0], S[1], f.m, k0, N, w.lh);
        f.l = f.l * t.alpha + t.psum;
        f.m = t.m_new;
        f.O.t[0] *= t.alpha;
        f.O.t[1] *= t.alpha;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) f.O = f32_second_product(f.O, ldsV, w.li, 32 * kt + 4 * w.lh, t.P[kt]);
    }
    return f;
}

// ------------------------------------------------------------------------------------------------------------------
// Plain fp16 operands on v_mfma_f32_32x32x16_f16: the arithmetic of the reference under `precision: 16` (fp16 autocast over
// QKVAttention.forward, OpenAI_Unet.py:457-476, and its backward) with fp32 accumulators.
//   q (scaled by the exact 2^-3), k, v and dA are rounded to fp16 (RNE, gradual underflow) once, where they are staged; every product
//   accumulates in fp32; the softmax, D and dS stay fp32 VALU work; P and dS are rounded to fp16 only as MFMA operands; outputs are fp32.
//   first product  S^T[key][query] = K . Q^T   : 4 k-steps of 16 channels per 32-key sub-tile; A = a K row's 8 channels (ds_read_b128 of
//                                 the row image [key][channel], rows padded to 144 B: 16 consecutive rows cover the 16 four-bank
//                                 groups), B = the query's 8 channels, in registers for the whole kernel.
//   second product O^T[c][query]  += V^T . P^T : registers 8s .. 8s+7 of the S^T accumulator, rounded to fp16, ARE the B operand of
//                                 k-step s: element j of lane-half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3). The A operand is
//                                 V^T[c][those keys]: two 8-byte reads of the transposed image [channel][key] (rows padded to 136 B:
//                                 32 consecutive rows cover the 32 bank pairs), which the staging threads write as 4-key columns.
// One 64-key tile of the forward costs a wave 16 MFMAs of 32 cycles instead of 128 of 64.
// ------------------------------------------------------------------------------------------------------------------
constexpr int P16_RS = 72;   // fp16 elements of a row-image row (64 channels + 16 B)
constexpr int P16_TS = 68;   // fp16 elements of a transposed-image row (64 rows + 8 B)

__device__ __forceinline__ f16x4 p16_round4(float x, float y, float z, float w) {
    return f16x4{(_Float16)x, (_Float16)y, (_Float16)z, (_Float16)w};
}
// 8 channels of a global row as one fp16 MFMA fragment, scaled by `scale` before rounding
__device__ __forceinline__ f16x8 p16_fragment(const float* p, float scale) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 c = *reinterpret_cast<const float4*>(p + 4);
    return f16x8{(_Float16)(a.x * scale), (_Float16)(a.y * scale), (_Float16)(a.z * scale), (_Float16)(a.w * scale),
                 (_Float16)(c.x * scale), (_Float16)(c.y * scale), (_Float16)(c.z * scale), (_Float16)(c.w * scale)};
}
// this staging thread's 4 rows x 4 channels (rows r0 + 4 kq + i, zero past N; channels 4 cq + {0..3}) of two matrices, from pa / pb
// with row strides sa / sb. EIGHTH_A: matrix a is scaled by the exact 2^-3.
template <bool EIGHTH_A>
__device__ __forceinline__ void p16_gather(float4 (&av)[4], float4 (&bv)[4], const float* pa, int sa, const float* pb, int sb,
                                           int r0, int N, int kq, int cq) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = r0 + 4 * kq + i;
        av[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        bv[i] = av[i];
        if (row < N) {
            av[i] = *reinterpret_cast<const float4*>(pa + (size_t)row * sa + 4 * cq);
            if (EIGHTH_A) { av[i].x *= 0.125f; av[i].y *= 0.125f; av[i].z *= 0.125f; av[i].w *= 0.125f; }
            bv[i] = *reinterpret_cast<const float4*>(pb + (size_t)row * sb + 4 * cq);
        }
    }
}
// ... rounded into a row image / a transposed image
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
// row image[row][64 channels] . frag: one 32 x 32 tile, image row `row` (32 sub + li) in this lane's A operand
__device__ __forceinline__ f32x16 p16_first_product(const _Float16* rimg, int row, int lh, const f16x8 (&frag)[4]) {
    f32x16 acc = {};
    const _Float16* rp = &rimg[row * P16_RS + 8 * lh];
#pragma unroll
    for (int s = 0; s < 4; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(rp + 16 * s), frag[s], acc, 0, 0, 0);
    return acc;
}
// registers 8s .. 8s+7 of a first product's accumulator as the B operand of k-step s of the second
__device__ __forceinline__ f16x8 p16_operand(f32x16 acc, int s) {
    f16x8 bf;
#pragma unroll
    for (int j = 0; j < 8; ++j) bf[j] = (_Float16)acc[8 * s + j];
    return bf;
}
// acc[ct] += T^T-image[channel 32 ct + li][rows row0 + {0..3}, row0 + 8 + {0..3}] . bf for both channel tiles; row0 = 32 sub + 16 s + 4 lh
__device__ __forceinline__ Acc2 p16_second_product(Acc2 acc, const _Float16* timg, int li, int row0, f16x8 bf) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const _Float16* tp = &timg[(32 * ct + li) * P16_TS + row0];
        const f16x4 lo = *reinterpret_cast<const f16x4*>(tp);
        const f16x4 hi = *reinterpret_cast<const f16x4*>(tp + 8);
        acc.t[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7), bf, acc.t[ct], 0, 0, 0);
    }
    return acc;
}

// The forward over all key tiles for this lane's query (fragments qf, pre-scaled by 1/8). ldsK: K row image, ldsVt: V^T image.
__device__ __forceinline__ Sweep p16_forward_sweep(const Wg& w, const f16x8 (&qf)[4], _Float16* ldsK, _Float16* ldsVt, int N, int C) {
    const int cq = w.tid & 15, kq = w.tid >> 4;     // staging: this thread's 4 channels x 4 keys of the tile
    const float* kp = w.base + C + w.hd * 64;
    Sweep f = {{}, -INFINITY, 0.f};
    for (int k0 = 0; k0 < N; k0 += 64) {
        float4 kv[4], vv[4];
        p16_gather<false>(kv, vv, kp, w.C3, kp + C, w.C3, k0, N, kq, cq);
        __syncthreads();   // previous tile fully consumed
        p16_stage_rows(ldsK, kq, cq, kv);
        p16_stage_cols(ldsVt, kq, cq, vv);
        __syncthreads();
        f32x16 S[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) S[kt] = p16_first_product(ldsK, 32 * kt + w.li, w.lh, qf);
        const SoftmaxTile t = softmax_tile(S[0], S[1], f.m, k0, N, w.lh);
        f.l = f.l * t.alpha + t.psum;
        f.m = t.m_new;
        f.O.t[0] *= t.alpha;
        f.O.t[1] *= t.alpha;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s) f.O = p16_second_product(f.O, ldsVt, w.li, 32 * kt + 16 * s + 4 * w.lh, p16_operand(t.P[kt], s));
    }
    return f;
}

// ------------------------------------------------------------------------------------------------------------------
// h3: fp32-grade products from two-term fp16 splits on v_mfma_f32_32x32x16_f16, the attention member of the convolutions' h3 family.
//   An operand x of unknown scale (q / 8, k, v, and dA after its per-sample normalisation) is carried as hi = fp16(x) and
//   lo = fp16((x - hi) 2^11): the lift keeps lo out of fp16's subnormal range wherever hi is normal. Out of range (|x| >= 65520) hi is
//   +-inf and lo is -+inf or NaN: non-finite results, never a finite wrong number.
//   first product  (both operands of unknown scale; images and fragments as p16, once per term): the accumulator takes
//                  hi . lo + lo . hi first, is multiplied by 2^-11 (16 VALU multiplies), then takes hi . hi: 12 MFMAs per 32 x 32 tile,
//                  no second accumulator.
//   second product (the B operand y is P or dS, formed in registers at a known lift): three B operands fp16(y), fp16(y - fp16(y)) and
//                  fp16(y 2^-11) against the two images, acc += hi . fp16(y) + hi . (y - fp16(y)) + lo . fp16(y 2^-11): 3 MFMAs per
//                  k-step and channel tile, one accumulator. y's own lo is NOT lifted, so y must not be small: P is taken against the
//                  running maximum (forward) or normalised (backward) and lifted by 2^15 -- at N = 16384 a flat row's P 2^15 is 2, its lo
//                  has 13 bits -- and dS = P (dP - D) by 2^10 (dA normalised to [1, 2) per sample: a flat row at N = 16384 is near 2^-3 ...
//                  2^0, a two-key row near 2^10 ... 2^13). The lifts are exact powers of two and leave with the row store.
// One 64-key tile of the forward costs a wave 24 + 24 MFMAs of 32 cycles instead of 128 of 64.
// ------------------------------------------------------------------------------------------------------------------
constexpr float H3_LO = 2048.f, H3_LO_INV = 1.0f / 2048.f;
constexpr int H3_P_LIFT = 15, H3_DS_LIFT = 10;

struct H3x4 { f16x4 hi, lo; };
__device__ __forceinline__ H3x4 h3_split4(float x, float y, float z, float w) {
    H3x4 r;
    r.hi = p16_round4(x, y, z, w);
    r.lo = p16_round4((x - (float)r.hi[0]) * H3_LO, (y - (float)r.hi[1]) * H3_LO, (z - (float)r.hi[2]) * H3_LO, (w - (float)r.hi[3]) * H3_LO);
    return r;
}
// 8 channels of a global row, times the exact 2^e, as the hi and lo fragments of one k-step
__device__ __forceinline__ void h3_fragment(f16x8& hi, f16x8& lo, const float* p, int e) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 c = *reinterpret_cast<const float4*>(p + 4);
    const H3x4 s0 = h3_split4(ldexpf(a.x, e), ldexpf(a.y, e), ldexpf(a.z, e), ldexpf(a.w, e));
    const H3x4 s1 = h3_split4(ldexpf(c.x, e), ldexpf(c.y, e), ldexpf(c.z, e), ldexpf(c.w, e));
    hi = __builtin_shufflevector(s0.hi, s1.hi, 0, 1, 2, 3, 4, 5, 6, 7);
    lo = __builtin_shufflevector(s0.lo, s1.lo, 0, 1, 2, 3, 4, 5, 6, 7);
}
// what p16_gather read, split into a pair of row images / of transposed images
__device__ __forceinline__ void h3_stage_rows(_Float16* hi, _Float16* lo, int kq, int cq, const float4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const H3x4 s = h3_split4(v[i].x, v[i].y, v[i].z, v[i].w);
        *reinterpret_cast<f16x4*>(&hi[(4 * kq + i) * P16_RS + 4 * cq]) = s.hi;
        *reinterpret_cast<f16x4*>(&lo[(4 * kq + i) * P16_RS + 4 * cq]) = s.lo;
    }
}
__device__ __forceinline__ void h3_stage_cols(_Float16* hi, _Float16* lo, int kq, int cq, const float4 (&v)[4]) {
    const H3x4 s[4] = {h3_split4(v[0].x, v[1].x, v[2].x, v[3].x), h3_split4(v[0].y, v[1].y, v[2].y, v[3].y),
                       h3_split4(v[0].z, v[1].z, v[2].z, v[3].z), h3_split4(v[0].w, v[1].w, v[2].w, v[3].w)};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        *reinterpret_cast<f16x4*>(&hi[(4 * cq + c) * P16_TS + 4 * kq]) = s[c].hi;
        *reinterpret_cast<f16x4*>(&lo[(4 * cq + c) * P16_TS + 4 * kq]) = s[c].lo;
    }
}
// (row images)[row][64 channels] . (fragments): one 32 x 32 tile, image row `row` (32 sub + li) in this lane's A operand
__device__ __forceinline__ f32x16 h3_first_product(const _Float16* rhi, const _Float16* rlo, int row, int lh, const f16x8 (&fh)[4],
                                                   const f16x8 (&fl)[4]) {
    f32x16 acc = {};
    const int o = row * P16_RS + 8 * lh;
    f16x8 ah[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        ah[s] = *reinterpret_cast<const f16x8*>(rhi + o + 16 * s);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], fl[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(rlo + o + 16 * s), fh[s], acc, 0, 0, 0);
    }
    acc *= H3_LO_INV;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], fh[s], acc, 0, 0, 0);
    return acc;
}
// registers 8s .. 8s+7 of a first product's accumulator, times the exact 2^lift, as the three B operands of k-step s of the second
struct H3Operand { f16x8 hi, lo, sc; };
__device__ __forceinline__ H3Operand h3_operand(f32x16 acc, int s, int lift) {
    H3Operand b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float y = ldexpf(acc[8 * s + j], lift);
        b.hi[j] = (_Float16)y;
        b.lo[j] = (_Float16)(y - (float)b.hi[j]);
        b.sc[j] = (_Float16)(y * H3_LO_INV);
    }
    return b;
}
// acc[ct] += (T^T images)[channel 32 ct + li][rows row0 + {0..3}, row0 + 8 + {0..3}] . b for both channel tiles; row0 as p16_second_product
__device__ __forceinline__ Acc2 h3_second_product(Acc2 acc, const _Float16* thi, const _Float16* tlo, int li, int row0, const H3Operand& b) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int o = (32 * ct + li) * P16_TS + row0;
        const f16x8 ah = __builtin_shufflevector(*reinterpret_cast<const f16x4*>(thi + o), *reinterpret_cast<const f16x4*>(thi + o + 8),
                                                 0, 1, 2, 3, 4, 5, 6, 7);
        const f16x8 al = __builtin_shufflevector(*reinterpret_cast<const f16x4*>(tlo + o), *reinterpret_cast<const f16x4*>(tlo + o + 8),
                                                 0, 1, 2, 3, 4, 5, 6, 7);
        acc.t[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b.sc, acc.t[ct], 0, 0, 0);
        acc.t[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.lo, acc.t[ct], 0, 0, 0);
        acc.t[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.hi, acc.t[ct], 0, 0, 0);
    }
    return acc;
}

// The forward over all key tiles for this lane's query (fragments of q / 8). ldsK: K row images, ldsVt: V^T images, hi then lo.
// O comes back lifted by 2^H3_P_LIFT (P is taken against the running maximum, so the lift holds whatever N is); l is not lifted.
__device__ __forceinline__ Sweep h3_forward_sweep(const Wg& w, const f16x8 (&qh)[4], const f16x8 (&ql)[4], _Float16* ldsK, _Float16* ldsVt,
                                                  int N, int C) {
    const int cq = w.tid & 15, kq = w.tid >> 4;     // staging: this thread's 4 channels x 4 keys of the tile
    const float* kp = w.base + C + w.hd * 64;
    Sweep f = {{}, -INFINITY, 0.f};
    for (int k0 = 0; k0 < N; k0 += 64) {
        float4 kv[4], vv[4];
        p16_gather<false>(kv, vv, kp, w.C3, kp + C, w.C3, k0, N, kq, cq);
        __syncthreads();   // previous tile fully consumed
        h3_stage_rows(ldsK, ldsK + 64 * P16_RS, kq, cq, kv);
        h3_stage_cols(ldsVt, ldsVt + 64 * P16_TS, kq, cq, vv);
        __syncthreads();
        f32x16 S[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) S[kt] = h3_first_product(ldsK, ldsK + 64 * P16_RS, 32 * kt + w.li, w.lh, qh, ql);
        const SoftmaxTile t = softmax_tile(S[0], S[1], f.m, k0, N, w.lh);
        f.l = f.l * t.alpha + t.psum;
        f.m = t.m_new;
        f.O.t[0] *= t.alpha;
        f.O.t[1] *= t.alpha;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                f.O = h3_second_product(f.O, ldsVt, ldsVt + 64 * P16_TS, w.li, 32 * kt + 16 * s + 4 * w.lh, h3_operand(t.P[kt], s, H3_P_LIFT));
    }
    return f;
}

// acc 2^e, elementwise and exact (ldexp, so that no intermediate power of two has to be a float); poison: 1, or NaN
__device__ __forceinline__ Acc2 h3_unlift(Acc2 acc, int e, float poison) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.t[ct][r] = ldexpf(acc.t[ct][r] * poison, e);
    return acc;
}

// The backward's normalisation of dA, per sample: amax[b] holds the largest magnitude bits of sample b's dA (attention_h3_amax_kernel).
// dA 2^-e has its largest magnitude in [1, 2); a non-finite dA poisons its sample (and only it) with NaN; an all-zero dA keeps e = 0.
struct H3Norm { int e; float poison; };
__device__ __forceinline__ H3Norm h3_norm(const unsigned* amax, int b) {
    const unsigned m = amax[b];
    const int ex = (int)(m >> 23);
    return H3Norm{m == 0u ? 0 : max(ex, 1) - 127, ex == 255 ? NAN : 1.0f};
}
}  // namespace

__global__ __launch_bounds__(256, 2) void attention_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                           int N, int C) {
    __shared__ float4 ldsK[64 * 16];   // [key][slot ^ (key & 15)]
    __shared__ float ldsV[64 * 64];    // [key][channel]
    const Wg w = wg_decode(qkv, N, C);
    float4 qreg[8];
    f32_fragment<true>(qreg, w.base + (size_t)min(w.row, N - 1) * w.C3 + w.hd * 64, w.lh);
    const Sweep f = f32_forward_sweep(w, qreg, ldsK, ldsV, N, C);
    if (w.row < N) store_row(out + ((size_t)w.b * N + w.row) * C + w.hd * 64, f.O, 1.0f / f.l, w.lh);
}

void launch_attention(const float* qkv, float* out, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nqb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_kernel, dim3((unsigned)(B * heads * nqb)), dim3(256), 0, stream, qkv, out, N, C);
}

__global__ __launch_bounds__(256, 2) void attention_p16_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                               int N, int C) {
    __shared__ __attribute__((aligned(16))) _Float16 ldsK[64 * P16_RS];    // [key][channel]
    __shared__ __attribute__((aligned(16))) _Float16 ldsVt[64 * P16_TS];   // [channel][key]
    const Wg w = wg_decode(qkv, N, C);
    // Q fragments of this lane's query: k-step s = channels 16 s + 8 lh + {0..7}, pre-scaled by 1/8, fp16
    f16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = p16_fragment(w.base + (size_t)min(w.row, N - 1) * w.C3 + w.hd * 64 + 16 * s + 8 * w.lh, 0.125f);
    const Sweep f = p16_forward_sweep(w, qf, ldsK, ldsVt, N, C);
    if (w.row < N) store_row(out + ((size_t)w.b * N + w.row) * C + w.hd * 64, f.O, 1.0f / f.l, w.lh);
}

void launch_attention_p16(const float* qkv, float* out, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nqb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_p16_kernel, dim3((unsigned)(B * heads * nqb)), dim3(256), 0, stream, qkv, out, N, C);
}

__global__ __launch_bounds__(256, 2) void attention_h3_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                              int N, int C) {
    __shared__ __attribute__((aligned(16))) _Float16 ldsK[2 * 64 * P16_RS];    // hi, lo x [key][channel]
    __shared__ __attribute__((aligned(16))) _Float16 ldsVt[2 * 64 * P16_TS];   // hi, lo x [channel][key]
    const Wg w = wg_decode(qkv, N, C);
    // Q fragments of this lane's query: k-step s = channels 16 s + 8 lh + {0..7}, times 1/8, split
    f16x8 qh[4], ql[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) h3_fragment(qh[s], ql[s], w.base + (size_t)min(w.row, N - 1) * w.C3 + w.hd * 64 + 16 * s + 8 * w.lh, -3);
    const Sweep f = h3_forward_sweep(w, qh, ql, ldsK, ldsVt, N, C);
    if (w.row < N) store_row(out + ((size_t)w.b * N + w.row) * C + w.hd * 64, f.O, ldexpf(1.0f / f.l, -H3_P_LIFT), w.lh);
}

void launch_attention_h3(const float* qkv, float* out, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nqb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_h3_kernel, dim3((unsigned)(B * heads * nqb)), dim3(256), 0, stream, qkv, out, N, C);
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
    const Wg w = wg_decode(qkv, N, C);
    const int qrow = min(w.row, N - 1);
    float4 qreg[8], dareg[8];
    f32_fragment<true>(qreg, w.base + (size_t)qrow * w.C3 + w.hd * 64, w.lh);
    f32_fragment<false>(dareg, da + ((size_t)w.b * N + qrow) * C + w.hd * 64, w.lh);
    // ---------------- sweep 1: the forward (running max / sum, O^T) -> D
    const Sweep f = f32_forward_sweep(w, qreg, ldsK, ldsP, N, C);
    // D = sum_c dA_c a_c, a = O / l. O^T[c][query]: register 4 rq + x of tile ct = channel 32 ct + 8 rq + 4 lh + x, i.e. dareg[4 ct + rq]
    float dsum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const float4 d4 = dareg[4 * ct + rq];
            dsum += d4.x * f.O.t[ct][4 * rq + 0] + d4.y * f.O.t[ct][4 * rq + 1] + d4.z * f.O.t[ct][4 * rq + 2] + d4.w * f.O.t[ct][4 * rq + 3];
        }
    dsum += __shfl_xor(dsum, 32, 64);
    const float Dq = dsum * (1.0f / f.l);
    const float lse = f.m + __logf(f.l);
    if (w.row < N && w.lh == 0) {
        float* st = stats + (((size_t)w.b * w.heads + w.hd) * N + w.row) * 2;
        st[0] = lse; st[1] = Dq;
    }
    // ---------------- sweep 2: dQ^T += K^T . dS^T
    const float* kp = w.base + C + w.hd * 64;
    Acc2 dQ = {};
    for (int k0 = 0; k0 < N; k0 += 64) {
        __syncthreads();
        f32_stage<false>(w.tid, k0, N, kp, w.C3, kp + C, w.C3, ldsK, ldsP, ldsV4, nullptr);
        __syncthreads();
        f32x16 S[2], dP[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            S[kt] = f32_first_product(ldsK, 32 * kt + w.li, w.lh, qreg);
            dP[kt] = f32_first_product(ldsV4, 32 * kt + w.li, w.lh, dareg);
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * w.lh;
                const float pv = (key < N) ? __expf(S[kt][r] - lse) : 0.f;
                S[kt][r] = pv * (dP[kt][r] - Dq);            // dS^T
            }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) dQ = f32_second_product(dQ, ldsP, w.li, 32 * kt + 4 * w.lh, S[kt]);
    }
    if (w.row < N) store_row(dqkv + ((size_t)w.b * N + w.row) * w.C3 + w.hd * 64, dQ, 0.125f, w.lh);
}

__global__ __launch_bounds__(256, 2) void attention_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                  float* __restrict__ dqkv, const float* __restrict__ stats, int N, int C) {
    __shared__ float4 ldsQ4[64 * 16];   // (Q / 8) tile, [query][slot ^ (query & 15)]: A operand of S = Q . K^T
    __shared__ float4 ldsA4[64 * 16];   // dA tile, same layout: A operand of dP = dA . V^T
    __shared__ float ldsQp[64 * 64];    // plain [query][channel] copies: A operands of dK^T += Q^T dS and dV^T += dA^T P
    __shared__ float ldsAp[64 * 64];
    __shared__ float ldsL[64], ldsD[64];   // per query: m + log l, D
    const Wg w = wg_decode(qkv, N, C);
    const float* krowp = w.base + (size_t)min(w.row, N - 1) * w.C3 + C + w.hd * 64;
    float4 kreg[8], vreg[8];
    f32_fragment<false>(kreg, krowp, w.lh);
    f32_fragment<false>(vreg, krowp + C, w.lh);
    Acc2 dK = {}, dV = {};
    const float* st = stats + ((size_t)w.b * w.heads + w.hd) * N * 2;
    for (int q0 = 0; q0 < N; q0 += 64) {
        __syncthreads();
        f32_stage<true>(w.tid, q0, N, w.base + w.hd * 64, w.C3, da + (size_t)w.b * N * C + w.hd * 64, C, ldsQ4, ldsQp, ldsA4, ldsAp);
        if (w.tid < 64) {
            const bool ok = q0 + w.tid < N;
            ldsL[w.tid] = ok ? st[(size_t)(q0 + w.tid) * 2] : INFINITY;      // exp(S - inf) = 0: queries past the end contribute nothing
            ldsD[w.tid] = ok ? st[(size_t)(q0 + w.tid) * 2 + 1] : 0.f;
        }
        __syncthreads();
        // S[query][key] = (Q/8) . K^T and dP[query][key] = dA . V^T: queries in the accumulator registers, the key on the lane;
        // one 32-query sub-tile at a time (32 instead of 64 live accumulator registers for S and dP: no spills)
#pragma unroll 1
        for (int qt = 0; qt < 2; ++qt) {
            const f32x16 S = f32_first_product(ldsQ4, 32 * qt + w.li, w.lh, kreg);
            const f32x16 dP = f32_first_product(ldsA4, 32 * qt + w.li, w.lh, vreg);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = 32 * qt + (r & 3) + 8 * (r >> 2) + 4 * w.lh;
                const float pv = __expf(S[r] - ldsL[qq]);
                const float ds = pv * (dP[r] - ldsD[qq]);
                dV = f32_second_step(dV, ldsAp, qq, w.li, pv);
                dK = f32_second_step(dK, ldsQp, qq, w.li, ds);
            }
        }
    }
    if (w.row < N) {
        float* krow_o = dqkv + ((size_t)w.b * N + w.row) * w.C3 + C + w.hd * 64;
        store_row(krow_o, dK, w.lh);
        store_row(krow_o + C, dV, w.lh);
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
// The same backward in the fp16 arithmetic (launch_attention_backward_p16): two kernels, work split, masking and row statistics as
// the fp32 pair above. D_i = sum_c dA_ic a_ic takes the rounded dA and the fp32 sweep-1 output. |dA| >= 65504 rounds to +-inf as under
// autocast and gives non-finite gradients of that sample (what the loss scale's device guard catches), never a finite wrong number.
//   attention_bwd_q_p16_kernel  : sweep 1 = attention_p16_kernel (K rows, V^T); sweep 2: K rows, V rows, K^T (27 KB)
//   attention_bwd_kv_p16_kernel : k, v fragments in registers; per 64-query tile Q/8 and dA rows, (Q/8)^T and dA^T (35 KB)
// Per 64-row tile a wave issues 16 + 24 (q kernel, sweeps 1 + 2) and 32 (kv kernel) MFMAs of 32 cycles instead of 128 + 192 and 256 of 64.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attention_bwd_q_p16_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                     float* __restrict__ dqkv, float* __restrict__ stats /*[B][heads][N][2]*/,
                                                                     int N, int C) {
    __shared__ __attribute__((aligned(16))) _Float16 ldsK[64 * P16_RS];   // K rows [key][channel]
    __shared__ __attribute__((aligned(16))) _Float16 ldsV[64 * P16_RS];   // V rows [key][channel] (sweep 2: A operand of dP^T = V . dA^T)
    __shared__ __attribute__((aligned(16))) _Float16 ldsT[64 * P16_TS];   // [channel][key]: V^T in sweep 1, K^T in sweep 2
    const Wg w = wg_decode(qkv, N, C);
    const int qrow = min(w.row, N - 1);
    const float* darow = da + ((size_t)w.b * N + qrow) * C + w.hd * 64;
    // fragments of this lane's query: k-step s = channels 16 s + 8 lh + {0..7}; q pre-scaled by 1/8
    f16x8 qf[4], daf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qf[s] = p16_fragment(w.base + (size_t)qrow * w.C3 + w.hd * 64 + 16 * s + 8 * w.lh, 0.125f);
        daf[s] = p16_fragment(darow + 16 * s + 8 * w.lh, 1.0f);
    }
    // ---------------- sweep 1: the p16 forward (running max / sum, O^T) -> D
    const Sweep f = p16_forward_sweep(w, qf, ldsK, ldsT, N, C);
    // D = sum_c dA_c a_c, a = O / l, with the fp16-rounded dA. O^T[c][query]: register 4 rq + x of tile ct = channel
    // 32 ct + 8 rq + 4 lh + x -- not the channels of this lane's MFMA fragments, so those 32 values are read again
    float dsum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const float4 d4 = *reinterpret_cast<const float4*>(darow + 32 * ct + 8 * rq + 4 * w.lh);
            dsum += (float)(_Float16)d4.x * f.O.t[ct][4 * rq + 0] + (float)(_Float16)d4.y * f.O.t[ct][4 * rq + 1] +
                    (float)(_Float16)d4.z * f.O.t[ct][4 * rq + 2] + (float)(_Float16)d4.w * f.O.t[ct][4 * rq + 3];
        }
    dsum += __shfl_xor(dsum, 32, 64);
    const float Dq = dsum * (1.0f / f.l);
    const float lse = f.m + __logf(f.l);
    if (w.row < N && w.lh == 0) {
        float* st = stats + (((size_t)w.b * w.heads + w.hd) * N + w.row) * 2;
        st[0] = lse; st[1] = Dq;
    }
    // ---------------- sweep 2: S^T = K . Q^T, dP^T = V . dA^T, dQ^T += K^T . dS^T
    const int cq = w.tid & 15, kq = w.tid >> 4;     // staging: this thread's 4 channels x 4 keys of the tile
    const float* kp = w.base + C + w.hd * 64;
    Acc2 dQ = {};
    for (int k0 = 0; k0 < N; k0 += 64) {
        float4 kv[4], vv[4];
        p16_gather<false>(kv, vv, kp, w.C3, kp + C, w.C3, k0, N, kq, cq);
        __syncthreads();   // previous tile (or sweep 1's last) fully consumed
        p16_stage_rows(ldsK, kq, cq, kv);
        p16_stage_rows(ldsV, kq, cq, vv);
        p16_stage_cols(ldsT, kq, cq, kv);
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16 S = p16_first_product(ldsK, 32 * kt + w.li, w.lh, qf);
            const f32x16 dP = p16_first_product(ldsV, 32 * kt + w.li, w.lh, daf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * w.lh;
                const float pv = (key < N) ? __expf(S[r] - lse) : 0.f;
                S[r] = pv * (dP[r] - Dq);            // dS^T
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) dQ = p16_second_product(dQ, ldsT, w.li, 32 * kt + 16 * s + 4 * w.lh, p16_operand(S, s));
        }
    }
    if (w.row < N) store_row(dqkv + ((size_t)w.b * N + w.row) * w.C3 + w.hd * 64, dQ, 0.125f, w.lh);
}

__global__ __launch_bounds__(256, 2) void attention_bwd_kv_p16_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                      float* __restrict__ dqkv, const float* __restrict__ stats, int N, int C) {
    __shared__ __attribute__((aligned(16))) _Float16 ldsQ[64 * P16_RS];    // (Q / 8) rows [query][channel]: A operand of S = Q . K^T
    __shared__ __attribute__((aligned(16))) _Float16 ldsA[64 * P16_RS];    // dA rows: A operand of dP = dA . V^T
    __shared__ __attribute__((aligned(16))) _Float16 ldsQt[64 * P16_TS];   // [channel][query] images: A operands of dK^T += (Q/8)^T dS
    __shared__ __attribute__((aligned(16))) _Float16 ldsAt[64 * P16_TS];   //                          and dV^T += dA^T P
    __shared__ float ldsL[64], ldsD[64];   // per query: m + log l, D
    const Wg w = wg_decode(qkv, N, C);
    const float* krowp = w.base + (size_t)min(w.row, N - 1) * w.C3 + C + w.hd * 64;
    // fragments of this lane's key: k-step s = channels 16 s + 8 lh + {0..7}
    f16x8 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        kf[s] = p16_fragment(krowp + 16 * s + 8 * w.lh, 1.0f);
        vf[s] = p16_fragment(krowp + C + 16 * s + 8 * w.lh, 1.0f);
    }
    Acc2 dK = {}, dV = {};
    const float* st = stats + ((size_t)w.b * w.heads + w.hd) * N * 2;
    const int cq = w.tid & 15, kq = w.tid >> 4;     // staging: this thread's 4 channels x 4 queries of the tile
    for (int q0 = 0; q0 < N; q0 += 64) {
        float4 qv[4], av[4];
        p16_gather<true>(qv, av, w.base + w.hd * 64, w.C3, da + (size_t)w.b * N * C + w.hd * 64, C, q0, N, kq, cq);
        float lq = INFINITY, dq_ = 0.f;      // exp(S - inf) = 0: queries past the end contribute nothing
        if (w.tid < 64 && q0 + w.tid < N) {
            lq = st[(size_t)(q0 + w.tid) * 2];
            dq_ = st[(size_t)(q0 + w.tid) * 2 + 1];
        }
        __syncthreads();   // previous tile fully consumed
        p16_stage_rows(ldsQ, kq, cq, qv);
        p16_stage_rows(ldsA, kq, cq, av);
        p16_stage_cols(ldsQt, kq, cq, qv);
        p16_stage_cols(ldsAt, kq, cq, av);
        if (w.tid < 64) { ldsL[w.tid] = lq; ldsD[w.tid] = dq_; }
        __syncthreads();
        // S[query][key] = (Q/8) . K^T and dP[query][key] = dA . V^T: queries in the accumulator registers, the key on the lane
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            f32x16 S = p16_first_product(ldsQ, 32 * qt + w.li, w.lh, kf);
            f32x16 dP = p16_first_product(ldsA, 32 * qt + w.li, w.lh, vf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = 32 * qt + (r & 3) + 8 * (r >> 2) + 4 * w.lh;
                const float pv = __expf(S[r] - ldsL[qq]);
                S[r] = pv;
                dP[r] = pv * (dP[r] - ldsD[qq]);     // dS
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int row0 = 32 * qt + 16 * s + 4 * w.lh;
                dV = p16_second_product(dV, ldsAt, w.li, row0, p16_operand(S, s));
                dK = p16_second_product(dK, ldsQt, w.li, row0, p16_operand(dP, s));
            }
        }
    }
    if (w.row < N) {
        float* krow_o = dqkv + ((size_t)w.b * N + w.row) * w.C3 + C + w.hd * 64;
        store_row(krow_o, dK, w.lh);
        store_row(krow_o + C, dV, w.lh);
    }
}

// stats: [B][heads][N][2] floats of scratch, as launch_attention_backward_flash
void launch_attention_backward_p16(const float* qkv, const float* da, float* dqkv, float* stats, int B, int N, int C, hipStream_t stream) {
    const int heads = C / 64;
    const int nb = (N + 127) / 128;
    hipLaunchKernelGGL(attention_bwd_q_p16_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), 0, stream, qkv, da, dqkv, stats, N, C);
    hipLaunchKernelGGL(attention_bwd_kv_p16_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), 0, stream, qkv, da, dqkv, stats, N, C);
}

// ------------------------------------------------------------------------------------------------------------------
// The same backward in the h3 arithmetic (launch_attention_backward_h3): two kernels, work split, masking and row statistics as the
// pairs above, all seven N x N x 64 products and sweep 1's two as three-term split products. dA has no natural scale (a loss
// gradient, times a loss scale, over a batch mean), so a pass in front takes the largest magnitude of each SAMPLE's dA as an integer
// maximum of the magnitude bits (atomicMax on uint32: exact, order-free, two calls give the same bits) and both kernels work on
// dA 2^-e, e the exponent of that maximum: the statistics' D, dP and dS are those of the normalised gradient, and 2^e returns with the
// lifts in the row stores. D_i = sum_c dA_ic a_ic takes the normalised dA in fp32 and the fp32 sweep-1 output.
//   attention_bwd_q_h3_kernel  : sweep 1 = attention_h3_kernel (K rows, V^T); sweep 2: K rows, V rows, K^T, hi and lo each (53 KB)
//   attention_bwd_kv_h3_kernel : k, v fragments in registers; per 64-query tile Q/8 and dA rows, (Q/8)^T and dA^T, hi and lo each (70.5 KB)
// Per 64-row tile a wave issues 48 + 72 (q kernel, sweeps 1 + 2) and 96 (kv kernel) MFMAs of 32 cycles instead of 128 + 192 and 256 of 64.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_h3_amax_kernel(const float* __restrict__ da, unsigned* __restrict__ amax, long long per_sample) {
    const float4* p = reinterpret_cast<const float4*>(da + (size_t)blockIdx.y * per_sample);
    const long long n4 = per_sample >> 2;      // per_sample = N C, C a multiple of 64
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = p[i];
        m = max(max(m, __float_as_uint(v.x) & 0x7fffffffu), max(__float_as_uint(v.y) & 0x7fffffffu, __float_as_uint(v.z) & 0x7fffffffu));
        m = max(m, __float_as_uint(v.w) & 0x7fffffffu);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&amax[blockIdx.y], m);
}

__global__ __launch_bounds__(256, 2) void attention_bwd_q_h3_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                    float* __restrict__ dqkv, float* __restrict__ stats /*[B][heads][N][2]*/,
                                                                    const unsigned* __restrict__ amax /*[B]*/, int N, int C) {
    __shared__ __attribute__((aligned(16))) _Float16 ldsK[2 * 64 * P16_RS];   // K rows, hi and lo
    __shared__ __attribute__((aligned(16))) _Float16 ldsV[2 * 64 * P16_RS];   // V rows (sweep 2: A operand of dP^T = V . dA^T)
    __shared__ __attribute__((aligned(16))) _Float16 ldsT[2 * 64 * P16_TS];   // [channel][key]: V^T in sweep 1, K^T in sweep 2
    const Wg w = wg_decode(qkv, N, C);
    const H3Norm nm = h3_norm(amax, w.b);
    const int qrow = min(w.row, N - 1);
    const float* darow = da + ((size_t)w.b * N + qrow) * C + w.hd * 64;
    f16x8 qh[4], ql[4], dah[4], dal[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        h3_fragment(qh[s], ql[s], w.base + (size_t)qrow * w.C3 + w.hd * 64 + 16 * s + 8 * w.lh, -3);
        h3_fragment(dah[s], dal[s], darow + 16 * s + 8 * w.lh, -nm.e);
    }
    // ---------------- sweep 1: the h3 forward (running max / sum, O^T 2^15) -> D of the normalised dA
    const Sweep f = h3_forward_sweep(w, qh, ql, ldsK, ldsT, N, C);
    float dsum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const float4 d4 = *reinterpret_cast<const float4*>(darow + 32 * ct + 8 * rq + 4 * w.lh);
            dsum += ldexpf(d4.x, -nm.e) * f.O.t[ct][4 * rq + 0] + ldexpf(d4.y, -nm.e) * f.O.t[ct][4 * rq + 1] +
                    ldexpf(d4.z, -nm.e) * f.O.t[ct][4 * rq + 2] + ldexpf(d4.w, -nm.e) * f.O.t[ct][4 * rq + 3];
        }
    dsum += __shfl_xor(dsum, 32, 64);
    const float Dq = dsum * ldexpf(1.0f / f.l, -H3_P_LIFT);
    const float lse = f.m + __logf(f.l);
    if (w.row < N && w.lh == 0) {
        float* st = stats + (((size_t)w.b * w.heads + w.hd) * N + w.row) * 2;
        st[0] = lse; st[1] = Dq;
    }
    // ---------------- sweep 2: S^T = K . Q^T, dP^T = V . dA^T, dQ^T 2^10 += K^T . (dS^T 2^10)
    const int cq = w.tid & 15, kq = w.tid >> 4;     // staging: this thread's 4 channels x 4 keys of the tile
    const float* kp = w.base + C + w.hd * 64;
    Acc2 dQ = {};
    for (int k0 = 0; k0 < N; k0 += 64) {
        float4 kv[4], vv[4];
        p16_gather<false>(kv, vv, kp, w.C3, kp + C, w.C3, k0, N, kq, cq);
        __syncthreads();   // previous tile (or sweep 1's last) fully consumed
        h3_stage_rows(ldsK, ldsK + 64 * P16_RS, kq, cq, kv);
        h3_stage_rows(ldsV, ldsV + 64 * P16_RS, kq, cq, vv);
        h3_stage_cols(ldsT, ldsT + 64 * P16_TS, kq, cq, kv);
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16 S = h3_first_product(ldsK, ldsK + 64 * P16_RS, 32 * kt + w.li, w.lh, qh, ql);
            const f32x16 dP = h3_first_product(ldsV, ldsV + 64 * P16_RS, 32 * kt + w.li, w.lh, dah, dal);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * w.lh;
                const float pv = (key < N) ? __expf(S[r] - lse) : 0.f;
                S[r] = pv * (dP[r] - Dq);            // dS^T
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
                dQ = h3_second_product(dQ, ldsT, ldsT + 64 * P16_TS, w.li, 32 * kt + 16 * s + 4 * w.lh, h3_operand(S, s, H3_DS_LIFT));
        }
    }
    if (w.row < N) store_row(dqkv + ((size_t)w.b * N + w.row) * w.C3 + w.hd * 64, h3_unlift(dQ, nm.e - H3_DS_LIFT - 3, nm.poison), w.lh);
}

__global__ __launch_bounds__(256, 2) void attention_bwd_kv_h3_kernel(const float* __restrict__ qkv, const float* __restrict__ da,
                                                                     float* __restrict__ dqkv, const float* __restrict__ stats,
                                                                     const unsigned* __restrict__ amax /*[B]*/, int N, int C) {
    extern __shared__ __attribute__((aligned(16))) _Float16 h3_lds[];
    _Float16* ldsQ = h3_lds;                          // (Q / 8) rows [query][channel], hi and lo: A operand of S = Q . K^T
    _Float16* ldsA = ldsQ + 2 * 64 * P16_RS;          // dA rows: A operand of dP = dA . V^T
    _Float16* ldsQt = ldsA + 2 * 64 * P16_RS;         // [channel][query] images: A operands of dK^T += (Q/8)^T dS
    _Float16* ldsAt = ldsQt + 2 * 64 * P16_TS;        //                          and dV^T += dA^T P
    float* ldsL = reinterpret_cast<float*>(ldsAt + 2 * 64 * P16_TS);      // per query: m + log l, D
    float* ldsD = ldsL + 64;
    const Wg w = wg_decode(qkv, N, C);
    const H3Norm nm = h3_norm(amax, w.b);
    const float* krowp = w.base + (size_t)min(w.row, N - 1) * w.C3 + C + w.hd * 64;
    // fragments of this lane's key: k-step s = channels 16 s + 8 lh + {0..7}
    f16x8 kh[4], kl[4], vh[4], vl[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        h3_fragment(kh[s], kl[s], krowp + 16 * s + 8 * w.lh, 0);
        h3_fragment(vh[s], vl[s], krowp + C + 16 * s + 8 * w.lh, 0);
    }
    Acc2 dK = {}, dV = {};
    const float* st = stats + ((size_t)w.b * w.heads + w.hd) * N * 2;
    const int cq = w.tid & 15, kq = w.tid >> 4;     // staging: this thread's 4 channels x 4 queries of the tile
    for (int q0 = 0; q0 < N; q0 += 64) {
        float4 qv[4], av[4];
        p16_gather<true>(qv, av, w.base + w.hd * 64, w.C3, da + (size_t)w.b * N * C + w.hd * 64, C, q0, N, kq, cq);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            av[i] = make_float4(ldexpf(av[i].x, -nm.e), ldexpf(av[i].y, -nm.e), ldexpf(av[i].z, -nm.e), ldexpf(av[i].w, -nm.e));
        float lq = INFINITY, dq_ = 0.f;      // exp(S - inf) = 0: queries past the end contribute nothing
        if (w.tid < 64 && q0 + w.tid < N) {
            lq = st[(size_t)(q0 + w.tid) * 2];
            dq_ = st[(size_t)(q0 + w.tid) * 2 + 1];
        }
        __syncthreads();   // previous tile fully consumed
        h3_stage_rows(ldsQ, ldsQ + 64 * P16_RS, kq, cq, qv);
        h3_stage_rows(ldsA, ldsA + 64 * P16_RS, kq, cq, av);
        h3_stage_cols(ldsQt, ldsQt + 64 * P16_TS, kq, cq, qv);
        h3_stage_cols(ldsAt, ldsAt + 64 * P16_TS, kq, cq, av);
        if (w.tid < 64) { ldsL[w.tid] = lq; ldsD[w.tid] = dq_; }
        __syncthreads();
        // S[query][key] = (Q/8) . K^T and dP[query][key] = dA . V^T: queries in the accumulator registers, the key on the lane
#pragma unroll 1
        for (int qt = 0; qt < 2; ++qt) {
            f32x16 S = h3_first_product(ldsQ, ldsQ + 64 * P16_RS, 32 * qt + w.li, w.lh, kh, kl);
            f32x16 dP = h3_first_product(ldsA, ldsA + 64 * P16_RS, 32 * qt + w.li, w.lh, vh, vl);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = 32 * qt + (r & 3) + 8 * (r >> 2) + 4 * w.lh;
                const float pv = __expf(S[r] - ldsL[qq]);
                S[r] = pv;
                dP[r] = pv * (dP[r] - ldsD[qq]);     // dS
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int row0 = 32 * qt + 16 * s + 4 * w.lh;
                dV = h3_second_product(dV, ldsAt, ldsAt + 64 * P16_TS, w.li, row0, h3_operand(S, s, H3_P_LIFT));
                dK = h3_second_product(dK, ldsQt, ldsQt + 64 * P16_TS, w.li, row0, h3_operand(dP, s, H3_DS_LIFT));
            }
        }
    }
    if (w.row < N) {
        float* krow_o = dqkv + ((size_t)w.b * N + w.row) * w.C3 + C + w.hd * 64;
        store_row(krow_o, h3_unlift(dK, nm.e - H3_DS_LIFT, nm.poison), w.lh);
        store_row(krow_o + C, h3_unlift(dV, nm.e - H3_P_LIFT, nm.poison), w.lh);
    }
}
constexpr size_t H3_KV_LDS = (size_t)(4 * 64 * P16_RS + 4 * 64 * P16_TS) * sizeof(_Float16) + 128 * sizeof(float);

// stats: [B][heads][N][2] floats and amax: B uint32 of scratch
void launch_attention_backward_h3(const float* qkv, const float* da, float* dqkv, float* stats, unsigned* amax, int B, int N, int C,
                                  hipStream_t stream) {
    static bool attr = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_bwd_kv_h3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)H3_KV_LDS);
        return true;
    }();
    (void)attr;
    const int heads = C / 64;
    const int nb = (N + 127) / 128;
    const long long per_sample = (long long)N * C;
    const unsigned chunks = (unsigned)std::min<long long>(64, (per_sample / 4 + 255) / 256);
    (void)hipMemsetAsync(amax, 0, (size_t)B * sizeof(unsigned), stream);
    hipLaunchKernelGGL(attention_h3_amax_kernel, dim3(chunks, (unsigned)B), dim3(256), 0, stream, da, amax, per_sample);
    hipLaunchKernelGGL(attention_bwd_q_h3_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), 0, stream, qkv, da, dqkv, stats, amax, N, C);
    hipLaunchKernelGGL(attention_bwd_kv_h3_kernel, dim3((unsigned)(B * heads * nb)), dim3(256), H3_KV_LDS, stream, qkv, da, dqkv, stats, amax,
                       N, C);
}

}  // namespace cddpm
