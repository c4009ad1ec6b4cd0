// Shared pieces of the split-operand convolution kernel (conv_x6.hip; attention.hip takes the vector types): vector types, the MFMA
// wrappers per split family, the SiLU used while staging, the fp32 -> 16-bit-terms split, the LDS slot functions (swizzles) of the
// weight image and of the patch, and ConvTile, the one description of a workgroup's tile that kernel, packers and launcher share.
// See conv_x6.hip for the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

namespace cddpm {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

template <int NS> struct SplitT;
template <> struct SplitT<3> {
    typedef bf16x8 v8; typedef bf16x4 v4;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct SplitT<2> {
    typedef f16x8 v8; typedef f16x4 v4;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

__device__ __forceinline__ float silu_x6(float v) {
    // identical evaluation to conv_mfma.hip::silu_f (split-product exp2, ~1.5 ulp)
    const float t = fminf(-v * 1.44269502162933349609375f, 126.0f);
    float tl = __builtin_fmaf(-v, 1.44269502162933349609375f, -t);
    tl = __builtin_fmaf(-v, 1.925963033500011e-08f, tl);
    tl = (t < 126.0f) ? tl : 0.0f;
    float e = __builtin_amdgcn_exp2f(t);
    e = __builtin_fmaf(e, tl * 0.693147180559945f, e);
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}

// the same on four values, written on vectors so that the multiplies / fmas / adds issue as packed (v_pk_*_f32) instructions:
// 26 VALU instructions per quad instead of 46. Identical results for x > -87.3; below, where the exponent clamps, the
// correction term is left to run (it only pushes e further towards +inf and the result towards the limit 0).
__device__ __forceinline__ v4f silu_x6_v4(const v4f v) {
    const v4f nl2e = {-1.44269502162933349609375f, -1.44269502162933349609375f, -1.44269502162933349609375f, -1.44269502162933349609375f};
    const v4f nl2e_lo = {-1.925963033500011e-08f, -1.925963033500011e-08f, -1.925963033500011e-08f, -1.925963033500011e-08f};
    const v4f lim = {126.0f, 126.0f, 126.0f, 126.0f};
    const v4f ln2 = {0.693147180559945f, 0.693147180559945f, 0.693147180559945f, 0.693147180559945f};
    const v4f one = {1.0f, 1.0f, 1.0f, 1.0f};
    const v4f t = __builtin_elementwise_min(v * nl2e, lim);
    v4f tl = __builtin_elementwise_fma(v, nl2e, -t);
    tl = __builtin_elementwise_fma(v, nl2e_lo, tl);
    v4f e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y), __builtin_amdgcn_exp2f(t.z), __builtin_amdgcn_exp2f(t.w)};
    e = __builtin_elementwise_fma(e, tl * ln2, e);
    const v4f d = one + e;
    const v4f r = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z), __builtin_amdgcn_rcpf(d.w)};
    return v * r;
}

// split of four fp32 values into NS 16-bit quads (8 B each): t[0] = cvt(v), t[1] = cvt(v - t[0]), ...
template <int NS>
__device__ __forceinline__ void split_x4(const v4f v, typename SplitT<NS>::v4 (&t)[NS]) {
    typedef typename SplitT<NS>::v4 q4;
    v4f r = v;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        t[s] = __builtin_convertvector(r, q4);
        r = r - __builtin_convertvector(t[s], v4f);
    }
}

// ---- LDS slot functions. A pixel (patch) or cout row (weights) owns SP = 4 NS slots of 16 B; slot (split s, u = channel / 8).
// The weight image: NS = 3: row stride 12, slot 4 s + (u ^ ((row >> 2) & 3));  NS = 2: stride 8, (4 s + u) ^ ((row >> 1) & 7) -> 16
// consecutive rows x one slot cover all 16 four-bank groups: ds_read_b128 of a fragment is conflict free. The packed global image IS the
// LDS image, so the kernel's fragment reads, the host packer and the device packer all ask here.
constexpr __host__ __device__ int conv_wslot(int ns, int row, int s, int u) {
    return (ns == 3) ? (row * 12 + 4 * s + (u ^ ((row >> 2) & 3))) : (row * 8 + ((4 * s + u) ^ ((row >> 1) & 7)));
}
// (the 16 x 16 form keeps ONE base per operand and reaches the mid term 4 slots away under XOR)
static_assert(conv_wslot(2, 5, 1, 2) == (conv_wslot(2, 5, 0, 2) ^ 4) && conv_wslot(2, 126, 1, 3) == (conv_wslot(2, 126, 0, 3) ^ 4), "NS = 2: mid = hi ^ 4");
// The patch is written by the kernel, so its swizzle follows the reads: a ds_read_b128 is served in four groups of 16 lanes ({0-3,12-15,
// 20-27}, {4-11,16-19,28-31}, +32) over 64 banks of 4 B, a ds_write_b64 in 16 consecutive lanes over 32 banks (MI355X_MICROARCH.md, LDS).
//   32x32x16 (conv_slot_a; the bf16 form): a group reads 16 consecutive pixels at one u -> the weights' swizzle with the pixel as row;
//   16x16x32, row fragments (conv_swz16): a group reads 8 + 8 pixels at u and u ^ 1, from ANY start pixel (tap shifts) -> slot bit 0
//             must stay u's, so only bits 1, 2 are swizzled -- by the pixel's COLUMN in the patch (bits 1, 2 -> slot bit 1, 2; bit 0 ->
//             slot bit 2; the patch width is even, so column and pixel parity agree): a tap's row shift ky is then a plain address
//             offset and the fragment addresses are computed once per kernel, not once per tap. Pixel q, slot q * 8 + ((4 s + u) ^ swz16).
//   16x16x32, column fragments (conv_colfrag_pitch): no swizzle; patch row pitch PW * 8 + 2 slots (2 mod 16 times an odd number: the
//             8 rows of a column start in 8 different even slots), pixel (pr, pc) at pr * pitch + 8 pc, slot (4 s + u) ^ 4 (pc & 1).
// All are conflict-free for every tap; with the weights' swizzle the 16x16 reads took 7 LDS cycles instead of 4.
constexpr __host__ __device__ int conv_slot_a(int row, int s, int u) { return conv_wslot(3, row, s, u); }
constexpr __host__ __device__ int conv_swz16(int pc) { return (2 * ((pc >> 1) & 3)) ^ (4 * (pc & 1)); }
constexpr __host__ __device__ int conv_colfrag_pitch(int pw) { return pw * 8 + 2; }

// ---- The workgroup's tile, stated once: every constant of conv_split_kernel<TAPS, NS, HI1, NB> and its LDS layout. The kernel takes
// them from here and the launcher asks lds_bytes(); nothing is derived a second time.
//   TAPS 9: 3x3 | 1: 1x1 | 4: folded "nearest x2 upsample -> 3x3 conv", one parity class of the output per tile (see conv_mfma.hip)
//   NS   3: bf16 terms, 32x32x16 MFMA | 2: fp16 terms, 16x16x32 MFMA          HI1: hi x hi product only          NB: cout blocks per workgroup
template <int TAPS_, int NS_, bool HI1_ = false, int NB_ = 1>
struct ConvTile {
    static constexpr int TAPS = TAPS_, NS = NS_, NB = NB_;
    static constexpr bool HI1 = HI1_;
    static_assert(NB == 1 || (NB == 2 && NS == 2 && TAPS != 1), "two cout blocks per workgroup: 16 x 16 fp16 form, LDS-DMA loop (3x3 and folded 2x2) only");
    static constexpr int ROWS = 8;                          // image rows of a workgroup's pixel tile (x 32 columns), two per wave
    static constexpr int THREADS = 64 * ROWS;
    static constexpr int SP = 4 * NS;                       // 16-B slots per pixel / per cout row
    static constexpr bool M16 = (NS == 2);                  // the 16 x 16 form
    static constexpr bool UP2 = (TAPS == 4);
    static constexpr int PAD = (TAPS == 9) ? 1 : 0;
    static constexpr int PW = UP2 ? 33 : 32 + 2 * PAD;      // patch width  (pixels)
    static constexpr int PH = UP2 ? ROWS + 1 : ROWS + 2 * PAD;   // patch height (pixels)
    static constexpr int NPIX = PW * PH;                    // 340 | 256 | 297
    static constexpr int NK = (NPIX * 8 + THREADS - 1) / THREADS;   // 16-B (4-channel) patch entries per thread: 6 | 4 | 5
    static constexpr int FOLD = (TAPS == 9) ? 3 : (TAPS == 4 ? 2 : 1);   // taps per accumulation group: one row of taps
    static constexpr int WSLOTS = 128 * SP;                 // 16-B slots of a weight slab
    // taps per weight stage: the fp16 form stages a whole row of taps (3 of the 3x3, 2 of the folded 2x2) per workgroup
    // barrier -- one barrier (and one burst of fragment reads behind it) per 72 MFMAs of a wave instead of per 24, and the
    // stage is exactly one accumulation group (FOLD taps). The bf16 form's slabs are 1.5x larger: one tap per stage.
    static constexpr int TPS = (NS == 2) ? FOLD : 1;
    static constexpr int WSTAGE = TPS * WSLOTS;             // 16-B slots of one weight stage
    static constexpr int WK = WSLOTS / THREADS;             // 16-B pieces of ONE slab per thread: 3 | 2
    static_assert(WSLOTS % THREADS == 0, "weight slab must divide evenly");
    static_assert(TPS == 1 || (THREADS == 512 && WSLOTS == 1024), "LDS-DMA stage copy: one slab = 8 waves x 2 KB");
    static constexpr int NKX = (TAPS == 9) ? 3 : (UP2 ? 2 : 1);     // column shifts of a row of taps
    static_assert(!M16 || TPS == NKX, "16x16 form: a weight stage is one row of taps, so the column shift is the unrolled index");
    static constexpr int SKY = (TAPS == 1) ? 0 : 1, SKX = (TAPS == 9) ? 1 : 0;      // the 1x1 skip segment's (centre) tap
    // 16 x 16 form: which instantiations hold COLUMN fragments (conv_x6.hip, header). Results are identical either way; the 1x1 form has
    // one tap and nothing to reuse, and the 256-cout workgroups (NB = 2: 128 accumulator registers in one chain, 253 VGPRs as they are)
    // spill with the ring (3x3: 129 VGPRs, 176 B of scratch per lane), so they keep row fragments.
    static constexpr bool COLF = (NS == 2) && (TAPS != 1) && (NB == 1);
    static constexpr int CPITCH = conv_colfrag_pitch(PW);   // ... their patch row pitch in slots
    static constexpr int ASLOTS = COLF ? ((PH * CPITCH + 15) & ~15) : NPIX * SP;      // 16-B slots of the patch
    // epilogue transpose: one region of [64 pixels][32 couts] floats per wave, row stride TRS (36: conflict-free for the 16 x 16 C
    // layout); column fragments write into each other's regions, which sit 8 floats further apart so that the two row quads a store
    // instruction covers do not share banks
    static constexpr int TRS = M16 ? 36 : 32;
    static constexpr int TRW = 64 * TRS + (COLF ? 8 : 0);
    // LDS layout, in 16-B slots from the start of dynamic LDS: patch | two weight stages | GroupNorm/FiLM coefficients of the sample
    // (3 x Cin floats); the transpose regions (wave w at float w * TRW) alias all of it once the last stage is multiplied
    static constexpr int LDS_A = 0, LDS_W = ASLOTS, LDS_C = ASLOTS + 2 * WSTAGE;
    static constexpr size_t lds_bytes(size_t coef_floats) {
        const size_t main = (size_t)LDS_C * 16 + coef_floats * sizeof(float), tr = (size_t)ROWS * TRW * sizeof(float);
        return main > tr ? main : tr;
    }
};

}  // namespace cddpm
