// What the two host files of the C ABI share (cddpm_api.hip: handle, forward program, reverse loop; cddpm_ops.hip: the standalone
// operators): the handle itself, error reporting, per-launch profiling, operator temporaries, the one entry pattern of the operators
// and the two planning rules of a convolution launch. Nothing declared here is exported by libcddpm_hip.so.
#pragma once
#include "../../include/cddpm.h"
#include "kernels.h"

#include <cstring>
#include <map>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

namespace cddpm {

struct ConvW { float* wpk = nullptr; float* bias = nullptr; int wexp = 0; };   // wexp: fp16-split pre-scale exponent
struct NormW { float* gamma = nullptr; float* beta = nullptr; };

struct ResW {
    std::string prefix;
    int Cin = 0, Cout = 0;
    bool up = false, down = false, has_skip = false;
    NormW gn1, gn2;
    ConvW conv1, conv2, skip;
    float* conv1_up2 = nullptr;   // up blocks: conv1 folded with the nearest x2 upsample (4 parity classes x 2x2 taps)
    float* bias2 = nullptr;   // conv2 bias (+ skip_connection bias when has_skip)
    int eoff = 0;             // offset of this block's (scale | shift) slice in the sumE-wide tables
};
struct AttnW {
    std::string prefix;
    int C = 0;
    NormW norm;
    ConvW qkv, proj;
};

enum OpKind { OP_IN = 0, OP_RES = 1, OP_ATTN = 2, OP_HEAD = 3 };
struct Op {
    OpKind kind;
    int idx;          // index into res / attn
    bool concat;      // pop the skip stack and concatenate before this op (output path)
    bool push;        // push the result on the skip stack (input path)
    bool block_end;   // last op of a named block: tap point
    int block;        // block ordinal
};
struct BlockInfo { std::string name; int C; int ds; };

struct WeightSpec { std::string name; int64_t numel; };

// GroupNorm statistics records of one activation buffer (written by the producing conv's epilogue, or by the stand-alone sweep)
struct StatBuf {
    float* records;       // [B][records][C][2] fp32
    size_t capacity;      // of `records` in floats (checked before every producer launch)
    int valid_count;      // records valid in the current forward; STAT_NONE: the tensor has no statistics yet
};
constexpr int STAT_NONE = -1;

}  // namespace cddpm

struct cddpm_ctx {
    cddpm_unet_desc d;
    int device = 0;
    void* arena = nullptr;            // scratch of the standalone operators (cddpm_op_set_scratch); nullptr: hipMalloc per call
    size_t arena_bytes = 0;
    float* zero_bias = nullptr;       // 4096 zeros: the bias of an operator called without one
    std::string err;
    bool weights_loaded = false, schedule_set = false;
    int cond_B = -1;
    // convolution family of this handle (numbering of conv_mode(); cddpm_set_conv_family): what every launch and every packed
    // weight image of the handle uses. weights_dropped: a family change freed the images of the previous family.
    int family = cddpm::conv_mode();
    bool weights_dropped = false;
    // arithmetic of the handle's reconstruction path (cddpm_set_precision): 32 = fp32-grade products; 16 (h3 handles only) = plain
    // fp16 operands -- hi_only on every convolution conv_launch plans, the fp16-MFMA attention kernel, and the 256-cout workgroups
    // wherever the maximum geometry allows them. Not read by the cddpm_op_* operators.
    int precision = 32;
    // arithmetic of the attention blocks of a precision-32 reconstruction path (cddpm_set_attention_family; numbering of the
    // convolution families): 0 = exact fp32 MFMA, 2 = h3, fp32-grade three-term fp16 splits. A precision-16 handle runs the p16 kernel
    // whatever this says. Not read by the cddpm_op_* operators.
    int attn_family = 0;
    size_t weight_allocs_begin = 0;      // allocs[weight_allocs_begin ..) are what cddpm_load_weights uploaded

    std::vector<cddpm::ResW> res;
    std::vector<cddpm::AttnW> attn;
    std::vector<cddpm::Op> prog;
    std::vector<cddpm::BlockInfo> blocks;
    std::vector<float*> taps;
    std::vector<cddpm::WeightSpec> wspecs;
    std::vector<void*> allocs;

    // in / head convs, embedding MLPs
    float *in_w = nullptr, *in_b = nullptr;        // [C][9], [C]
    cddpm::NormW out_norm;
    float* head_w9 = nullptr;                      // [9][C]
    float head_bias = 0.f;
    float *te0_w = nullptr, *te0_b = nullptr, *te2_w = nullptr, *te2_b = nullptr;
    float *le0_w = nullptr, *le0_b = nullptr, *le2_w = nullptr, *le2_b = nullptr;
    float *emb_w = nullptr, *emb_b = nullptr;      // [sumE][E], [sumE]
    int sumE = 0, E = 0, half = 0;

    // tables
    float *tab = nullptr, *cpart = nullptr;        // [T][sumE], [Bmax][sumE]
    float *sched[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // coef1, coef2, logvar, sqrt_recip, sqrt_recipm1
    float *qs_sa = nullptr, *qs_s1 = nullptr;
    int objective = 0;
    int clip_denoised = 1;               // cddpm_set_clip_denoised
    // accumulation plan of the reverse loop (cddpm_set_accumulation_switch; OFF by default): steps t >= nb2_tmin run the Cout = 256
    // convolutions on 256-cout workgroups (two-level accumulation: faster, ~3x the rounding noise of a convolution), steps below it on
    // the three-level kernel. nb2_now: whether the forward in flight is such a step (single forwards outside the loop never are).
    int nb2_tmin = 1 << 30;
    int nb2_now = 0;
    int* d_t = nullptr;

    // workspace
    std::vector<float*> hs;                        // skip stack tensors (input path outputs)
    float *bufA = nullptr, *bufB = nullptr, *bufH = nullptr, *bufP0 = nullptr, *bufP1 = nullptr;
    float *qkvbuf = nullptr, *attbuf = nullptr, *headP = nullptr, *model_out = nullptr;
    float* coef = nullptr;
    float* kpart = nullptr;              // split-K planes of the small-batch plan (see plan_ksplit)
    int cur_H = 0, cur_W = 0;            // image size of the forward in flight (a layer's downsampling factor follows from it)
    std::map<const float*, cddpm::StatBuf> stat;      // statistics records of every activation buffer that can feed a GroupNorm
    float *scratch0 = nullptr, *scratch1 = nullptr;   // [max(T,Bmax)][half] for the embedding MLPs

    // optional per-kernel-class timing with HIP events on the launch stream (cddpm_set_profiling)
    struct ProfRec { hipEvent_t a, b; int cls; double flops; double bytes; };
    bool profiling = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    // consecutive launches on one stream share an event: the end of one is the begin of the next (half the event records
    // in the stream; a launch's time then includes the few-microsecond gap in front of it)
    hipEvent_t prof_last = nullptr;
    hipStream_t prof_last_stream = nullptr;

    // one reverse step (UNet forward + posterior step + t -= 1) captured as a HIP graph and replayed by cddpm_reverse;
    // everything that changes from step to step is read from device memory (d_t), so one graph serves every t
    struct StepGraph {
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        float* img = nullptr; const float* noise = nullptr; uint64_t seed = 0, slice0 = 0; int B = 0, H = 0, W = 0;
        uint64_t gen = 0;
        int nb2 = 0;                     // the accumulation plan the captured step was planned with
    } sg;
    uint64_t gen = 1;                    // bumped by whatever a captured graph would not see (weights, schedule, taps)
    hipStream_t gstream = nullptr;       // the legacy default stream cannot be captured: graphs run on a stream of the handle
    hipEvent_t gev_in = nullptr, gev_out = nullptr;
};

namespace cddpm {

// records the message on the handle (h == nullptr: as the calling thread's create error) and returns -1 (cddpm_api.hip)
int fail(cddpm_ctx* h, const char* fmt, ...);

#define HIPCHECK(h, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return fail(h, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// 0-4: the reconstruction path's classes; 5-8: the training operators (cddpm_op_*): weight-gradient GEMMs (+ their k-image passes),
// GroupNorm backward, everything of the context encoder, Adam + guard + weight re-packing. PC_NONE: an entry point without a record
enum ProfClass { PC_NONE = -1, PC_CONV3 = 0, PC_CONV1 = 1, PC_ATTN = 2, PC_GN = 3, PC_OTHER = 4, PC_WGRAD = 5, PC_GNBWD = 6, PC_ENC = 7, PC_OPT = 8, PC_COUNT = 9 };

struct Prof {
    cddpm_ctx* h; hipStream_t s; cddpm_ctx::ProfRec r; bool on;
    static hipEvent_t ev(cddpm_ctx* h) {
        if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    Prof(cddpm_ctx* h_, int cls, double flops, double bytes, hipStream_t s_) : h(h_), s(s_), on(h_->profiling && cls != PC_NONE) {
        if (!on) return;
        r.cls = cls; r.flops = flops; r.bytes = bytes; r.b = ev(h);
        if (h->prof_last && h->prof_last_stream == s) r.a = h->prof_last;
        else { r.a = ev(h); (void)hipEventRecord(r.a, s); }
    }
    ~Prof() {
        if (!on) return;
        (void)hipEventRecord(r.b, s);
        h->prof.push_back(r);
        h->prof_last = r.b;
        h->prof_last_stream = s;
    }
};

// ---- the one entry pattern of the standalone operators (cddpm_op_*; `h` and `stream` are the entry point's parameters) ----------
// OP_PROLOGUE: a NULL handle returns -1, a failed argument check its message; then the launch stream `s`, the handle's device and the
// profiling record of the call (PC_NONE: the entry point has none -- a record costs two event records on the stream when profiling
// is on, and cddpm_get_profile counts it as a launch). An operator with two messages puts an OP_CHECK with the first in front.
// OP_EPILOGUE: launch errors of the call.
#define OP_CHECK(cond, ...)                                       \
    if (!h) return -1;                                            \
    if (!(cond)) return fail(h, __VA_ARGS__);
#define OP_PROLOGUE(cls, flops, bytes, cond, ...)                 \
    OP_CHECK(cond, __VA_ARGS__)                                   \
    hipStream_t s = (hipStream_t)stream;                          \
    HIPCHECK(h, hipSetDevice(h->device));                         \
    Prof prof_(h, cls, flops, bytes, s);
#define OP_EPILOGUE()                                             \
    HIPCHECK(h, hipGetLastError());                               \
    return 0;

// ---- temporaries and parameters of the standalone operators ------------------------------------------------------------------
// Temporaries come from the handle's scratch arena when cddpm_op_set_scratch gave it one (re-used from its start by every call: calls
// on ONE stream are ordered, nothing synchronises -- what the training step runs on); without an arena, or for a `per_call` scratch
// (the kernel-test convolutions, which synchronise anyway and must not depend on how a trainer sized the arena), they are
// hipMalloc'ed for the call and freed after a stream synchronisation.
// A scratch without a handle only COUNTS: every request adds its rounded size to `off` and returns nullptr, nothing is allocated and
// nothing fails. An operator states its requests once, in a function of (OpScratch&, shape); run on a counting scratch that function
// is the operator's size query (cddpm_op_*_scratch), run on the real one it hands out the pointers.
struct OpScratch {
    cddpm_ctx* h;
    hipStream_t s;
    bool per_call;
    std::vector<void*> owned;
    size_t off = 0;
    bool failed = false;
    OpScratch() : h(nullptr), s(nullptr), per_call(false) {}
    OpScratch(cddpm_ctx* h_, hipStream_t s_, bool per_call_ = false) : h(h_), s(s_), per_call(per_call_) {}
    void* get(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (!h) { off += bytes; return nullptr; }
        if (h->arena && !per_call) {
            if (off + bytes > h->arena_bytes) { failed = true; off += bytes; return nullptr; }
            void* p = static_cast<char*>(h->arena) + off;
            off += bytes;
            return p;
        }
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); failed = true; return nullptr; }
        owned.push_back(p);
        return p;
    }
    template <class T> T* n(size_t count) { return static_cast<T*>(get(count * sizeof(T))); }
    // a parameter vector given in host OR device memory: device pointers are used where they lie, host ones are staged (the copy is
    // asynchronous: the host array must stay valid until the stream has run it). A counting scratch takes them to be on the device.
    const float* param(const float* p, size_t count) {
        if (!h) return p;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice) return p;
        (void)hipGetLastError();
        float* d = n<float>(count);
        if (d && hipMemcpyAsync(d, p, count * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) failed = true;
        return d;
    }
    ~OpScratch() {
        if (owned.empty()) return;
        (void)hipStreamSynchronize(s);
        for (void* p : owned) (void)hipFree(p);
    }
};
#define SCRATCH_CHECK(sc)                                                                                                   \
    if ((sc).failed) return fail(h, "operator scratch: %zu bytes needed, arena holds %zu (cddpm_op_set_scratch)", (sc).off, h->arena_bytes);

// ---- what a convolution launch is planned and accounted with -----------------------------------------------------------------
inline void zero_conv_args(ConvArgs& a, const cddpm_ctx* h) { memset(&a, 0, sizeof a); a.family = h->family; }

inline double conv_flops(const ConvArgs& a) {
    return 2.0 * a.B * a.H * a.W * a.Cout * ((double)(a.C0 + a.C1) * a.taps + a.S0 + a.S1);
}
// algorithmic bytes of one fused conv launch: every input read once, output written once, weights once
inline double conv_bytes(const ConvArgs& a) {
    const double px = (double)a.B * a.H * a.W, spx = (double)a.B * a.srcH * a.srcW;
    double b = spx * (a.C0 + a.C1) + px * (a.S0 + a.S1) + px * a.Cout;
    if (a.res) b += (a.res_up ? px / 4 : px) * a.Cout;
    b += (double)a.Cout * ((double)(a.C0 + a.C1) * a.taps + a.S0 + a.S1);
    return 4.0 * b;
}

// Workgroups of the 128-cout form of convolution `a` at geometry (B, H, W) -- the call's own, or the handle's maximum geometry
// scaled to the layer (cddpm_api.hip::conv_workgroups_at_max): tiles of 32 x 8 output pixels x 128 couts; the folded upsample runs its
// four parity classes on the half-resolution grid.
inline long long conv_workgroups(const ConvArgs& a, int B, int H, int W) {
    const bool up2 = (a.taps == 4);
    const int gh = up2 ? H / 2 : H, gw = up2 ? W / 2 : W;
    return (long long)B * (up2 ? 4 : 1) * ((gw + 31) / 32) * ((gh + 7) / 8) * (a.Cout / 128);
}

// When a launch takes the 256-cout workgroups (ConvArgs::nb2; two-level accumulation: faster, ~3x the rounding noise). conv_nb2_ok
// says whether the kernel can at `workgroups`, the 128-cout count at the geometry the policy plans for; the policy says who wants it:
enum Nb2Policy {
    // the reconstruction path (conv_launch): the steps the handle's accumulation switch names (nb2_now), and `workgroups` is taken at
    // the handle's MAXIMUM geometry -- a property of the handle like the split-K factor, never of the call, so that a slice's bits do
    // not depend on the batch it is computed in. The 1000-step chain feeds every rounding error back into itself. A precision-16
    // handle (operand rounding 2^-11: no 1e-4 chain to protect) wants the form on every step and in single forwards, at the same
    // maximum geometry: still a function of the handle alone.
    NB2_HANDLE_PLAN,
    // the training operators plan per call, and DO take the 256-cout workgroups wherever the call fills the chip with them: a gradient's
    // accuracy need (2e-5 of float64 autograd; SGD noise far above that) is not the 1000-step chain's, and the form is worth
    // +9...12 % per layer
    NB2_CALL_PLAN,
    // the kernel-test convolutions (weights from host memory) are compared with references at the three-level kernel's tolerance: only
    // when CDDPM_NB2=force asks for the 256-cout form everywhere (how the parity tests run their small shapes through it)
    NB2_FORCED_ONLY
};
inline void conv_set_nb2(ConvArgs& a, const cddpm_ctx* h, Nb2Policy policy, long long workgroups) {
    const int env = conv_nb2_env();
    const bool wanted = policy == NB2_HANDLE_PLAN ? (h->nb2_now || h->precision == 16 || env == 2) : policy == NB2_CALL_PLAN ? env >= 1 : env == 2;
    a.nb2 = (wanted && conv_nb2_ok(a.Cout, workgroups, 1, h->family)) ? 1 : 0;
}

// The small-batch split-K rule as plain arithmetic (cddpm_api.hip; exported as cddpm_conv_ksplit_plan): `workgroups_at_max` of the
// 128-cout form at the handle's maximum geometry, Cin main and Cskip skip-segment channels (multiples of 32), `taps` per main chunk.
// Returns S; S > 1 fills kbound[0 .. S].
int ksplit_rule(int family, long long workgroups_at_max, int Cin, int Cskip, int taps, short* kbound);
constexpr int KSPLIT_PLANE_FLOATS = 256 * 256 * 128;      // floats of cddpm_ctx::kpart: S * workgroups <= 256, a workgroup's tile <= 256 x 128 outputs

// One convolution of the reconstruction path as the handle plans it (cddpm_api.hip): statistics records when a.out has a StatBuf,
// hi_only by the handle's precision, then split-K + combine or one launch in the 128- / 256-cout form. `took`: the plan, for
// cddpm_op_conv_planned.
struct ConvPlanTaken { int S; short kbound[CDDPM_MAX_KSPLIT + 1]; int nb2; };
int conv_launch(cddpm_ctx* h, ConvArgs a, hipStream_t s, ConvPlanTaken* took = nullptr);

// widest concatenated GroupNorm / convolution input of the kernels (see check_program in cddpm_api.hip)
constexpr int MAX_CONCAT_CHANNELS = 1536;

}  // namespace cddpm

#pragma GCC visibility pop
