// C ABI of libcddpm_hip.so (declared in include/cddpm.h): handle, weight packing, embedding tables,
// the UNet forward program and the reverse-diffusion loop driver. Host code only; kernels live in
// conv_mfma.hip, norm_kernels.hip, small_kernels.hip and attention.hip.
//
// Data layout in HBM: every activation is NHWC fp32 ([B][H*W][C], 16-B aligned channel quads); the image
// itself has one channel, so the [B,1,H,W] boundary tensors need no conversion. Skip-stack tensors, three
// ping-pong activation buffers, the qkv/attention buffers, GroupNorm partials and coefficient planes, the
// packed weights and the [T][sumE] time-embedding table are allocated once in cddpm_create.
#include "../../include/cddpm.h"
#include "kernels.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace cddpm;

namespace {

struct ConvW { float* wpk = nullptr; float* bias = nullptr; int Cin = 0, Cout = 0, taps = 0; int wexp = 0; };   // wexp: fp16-split pre-scale exponent
struct NormW { float* gamma = nullptr; float* beta = nullptr; int C = 0; };

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

thread_local std::string g_create_error;

}  // namespace

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
    int family = conv_mode();
    bool weights_dropped = false;
    size_t weight_allocs_begin = 0;      // allocs[weight_allocs_begin ..) are what cddpm_load_weights uploaded

    std::vector<ResW> res;
    std::vector<AttnW> attn;
    std::vector<Op> prog;
    std::vector<BlockInfo> blocks;
    std::vector<float*> taps;
    std::vector<WeightSpec> wspecs;
    std::vector<void*> allocs;
    size_t alloc_bytes = 0;

    // in / head convs, embedding MLPs
    float *in_w = nullptr, *in_b = nullptr;        // [C][9], [C]
    NormW out_norm;
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
    std::vector<size_t> hs_elems;
    float *bufA = nullptr, *bufB = nullptr, *bufH = nullptr, *bufP0 = nullptr, *bufP1 = nullptr;
    float *qkvbuf = nullptr, *attbuf = nullptr, *headP = nullptr, *model_out = nullptr;
    float* coef = nullptr;
    float* kpart = nullptr;              // split-K planes of the small-batch plan (see plan_ksplit)
    int cur_H = 0, cur_W = 0;            // image size of the forward in flight (a layer's downsampling factor follows from it)
    // GroupNorm statistics records per activation buffer (written by the producing conv's epilogue, or by the
    // stand-alone sweep): buffer -> records storage, and how many records are valid in the current forward
    std::map<const float*, float*> stat_buf;
    std::map<const float*, int> stat_n;
    std::map<const float*, size_t> stat_cap;       // capacity of each records buffer in floats (checked before every producer launch)
    float *scratch0 = nullptr, *scratch1 = nullptr;   // [max(T,Bmax)][half] for the embedding MLPs
    int max_nsplit = 0;

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

namespace {

int fail(cddpm_ctx* h, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return -1;
}

// 0-4: the reconstruction path's classes; 5-8: the training operators (cddpm_op_*): weight-gradient GEMMs (+ their k-image passes),
// GroupNorm backward, everything of the context encoder, Adam + guard + weight re-packing
enum ProfClass { PC_CONV3 = 0, PC_CONV1 = 1, PC_ATTN = 2, PC_GN = 3, PC_OTHER = 4, PC_WGRAD = 5, PC_GNBWD = 6, PC_ENC = 7, PC_OPT = 8, PC_COUNT = 9 };

struct Prof {
    cddpm_ctx* h; hipStream_t s; cddpm_ctx::ProfRec r; bool on;
    static hipEvent_t ev(cddpm_ctx* h) {
        if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    Prof(cddpm_ctx* h_, int cls, double flops, double bytes, hipStream_t s_) : h(h_), s(s_), on(h_->profiling) {
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

double conv_flops(const ConvArgs& a) {
    return 2.0 * a.B * a.H * a.W * a.Cout * ((double)(a.C0 + a.C1) * a.taps + a.S0 + a.S1);
}
// algorithmic bytes of one fused conv launch: every input read once, output written once, weights once
double conv_bytes(const ConvArgs& a) {
    const double px = (double)a.B * a.H * a.W, spx = (double)a.B * a.srcH * a.srcW;
    double b = spx * (a.C0 + a.C1) + px * (a.S0 + a.S1) + px * a.Cout;
    if (a.res) b += (a.res_up ? px / 4 : px) * a.Cout;
    b += (double)a.Cout * ((double)(a.C0 + a.C1) * a.taps + a.S0 + a.S1);
    return 4.0 * b;
}
// Small-batch plan (fp16-split family). A layer launches B * tiles * (Cout / 128) workgroups of 256 pixels x 128 channels; when the
// HANDLE's largest geometry gives fewer than half the chip's 256 CUs a workgroup, the K loop of that layer is cut into S ranges run
// by S workgroups per tile (plane j of `kpart` each) and conv_reduce_kernel adds the planes in the order of j. S is a property of
// the handle (max_batch, max_h, max_w and the layer), never of the call: a slice's bits do not depend on the batch it is in, as long
// as it is computed on handles of the same maximum geometry (sharded runs: the same engine configuration on every rank).
constexpr int KSPLIT_PLANE_FLOATS = 256 * 256 * 128;      // S * workgroups <= 256, a workgroup's tile <= 256 x 128 outputs
int plan_ksplit(const cddpm_ctx* h, const ConvArgs& a, short* kbound) {
    if (h->family != 2 || h->cur_H <= 0) return 1;
    const bool up2 = (a.taps == 4);
    const int Hm = (int)((long long)a.H * h->d.max_h / h->cur_H), Wm = (int)((long long)a.W * h->d.max_w / h->cur_W);
    const int gh = up2 ? Hm / 2 : Hm, gw = up2 ? Wm / 2 : Wm;
    const long long nwg = (long long)h->d.max_batch * (up2 ? 4 : 1) * ((gw + 31) / 32) * ((gh + 7) / 8) * (a.Cout / 128);
    const int nch_main = (a.C0 + a.C1) / 32, nch_skip = (a.S0 + a.S1) / 32, nch = nch_main + nch_skip;
    const int units = nch_main * a.taps + nch_skip;           // taps to multiply per tile
    int S = 1;
    while (S < CDDPM_MAX_KSPLIT && nwg * (S * 2) <= 256 && units / (S * 2) >= 9 && S * 2 <= nch) S *= 2;
    if (S == 1) return 1;
    // consecutive chunk ranges of about units / S taps each, none empty
    int c = 0, acc = 0;
    kbound[0] = 0;
    for (int j = 1; j < S; ++j) {
        const int target = (int)((long long)units * j / S);
        while (c < nch - (S - j) && acc + (c < nch_main ? a.taps : 1) / 2 < target) { acc += (c < nch_main ? a.taps : 1); ++c; }
        if (c <= kbound[j - 1]) { acc += (c < nch_main ? a.taps : 1); ++c; }
        kbound[j] = (short)c;
    }
    kbound[S] = (short)nch;
    return S;
}

// workgroups of the 128-cout form at the HANDLE's maximum geometry (the quantity both plans are keyed on)
static long long conv_workgroups_at_max(const cddpm_ctx* h, const ConvArgs& a) {
    if (h->cur_H <= 0) return 0;
    const bool up2 = (a.taps == 4);
    const int Hm = (int)((long long)a.H * h->d.max_h / h->cur_H), Wm = (int)((long long)a.W * h->d.max_w / h->cur_W);
    const int gh = up2 ? Hm / 2 : Hm, gw = up2 ? Wm / 2 : Wm;
    return (long long)h->d.max_batch * (up2 ? 4 : 1) * ((gw + 31) / 32) * ((gh + 7) / 8) * (a.Cout / 128);
}
static long long conv_workgroups_of_call(const ConvArgs& a) {
    const bool up2 = (a.taps == 4);
    const int gh = up2 ? a.H / 2 : a.H, gw = up2 ? a.W / 2 : a.W;
    return (long long)a.B * (up2 ? 4 : 1) * ((gw + 31) / 32) * ((gh + 7) / 8) * (a.Cout / 128);
}

int conv_launch(cddpm_ctx* h, ConvArgs a, hipStream_t s) {
    auto it = h->stat_buf.find(a.out);       // outputs that can feed a GroupNorm get their statistics for free
    a.stats = (it != h->stat_buf.end()) ? it->second : nullptr;
    short kb[CDDPM_MAX_KSPLIT + 1] = {0};
    const int S = plan_ksplit(h, a, kb);
    if (S > 1) {
        if ((size_t)S * a.B * a.H * a.W * a.Cout > (size_t)KSPLIT_PLANE_FLOATS)
            return fail(h, "split-K planes of a %dx%dx%d conv output (B=%d, S=%d) exceed the workspace", a.H, a.W, a.Cout, a.B, S);
        const int nrec_r = conv_reduce_stat_records(a.H, a.W);
        if (a.stats && (size_t)a.B * nrec_r * a.Cout * 2 > h->stat_cap.at(a.out))
            return fail(h, "GroupNorm statistics records of a %dx%dx%d conv output do not fit their buffer", a.H, a.W, a.Cout);
        ConvArgs k = a;
        k.out = h->kpart; k.bias = nullptr; k.res = nullptr; k.stats = nullptr; k.ksplit = S;
        for (int j = 0; j <= S; ++j) k.kbound[j] = kb[j];
        {
            Prof p(h, a.taps == 1 ? PC_CONV1 : PC_CONV3, conv_flops(a), conv_bytes(a), s);
            launch_conv(k, s);
            launch_conv_reduce(h->kpart, S, a.bias, a.res, a.res_up, a.out, a.stats, a.B, a.H, a.W, a.Cout, s);
        }
        if (a.stats) h->stat_n[a.out] = nrec_r;
        return 0;
    }
    // large-batch plan: 256-cout workgroups where the handle's maximum geometry still fills the chip with them (a property of the
    // handle like S above, never of the call)
    a.nb2 = ((h->nb2_now || conv_nb2_env() == 2) && conv_nb2_ok(a.Cout, conv_workgroups_at_max(h, a), 1, h->family)) ? 1 : 0;
    const int nrec = (a.taps == 4) ? conv_stat_records_up2(a.H, a.W) : conv_stat_records(a.H, a.W);
    if (a.stats) {
        // a statically sized buffer against a shape-derived count: refuse to launch rather than write past the end
        const size_t need = (size_t)a.B * nrec * a.Cout * 2;
        if (need > h->stat_cap.at(a.out))
            return fail(h, "GroupNorm statistics records of a %dx%dx%d conv output (B=%d, %d records) need %zu floats, the buffer holds %zu",
                        a.H, a.W, a.Cout, a.B, nrec, need, h->stat_cap.at(a.out));
    }
    {
        Prof p(h, a.taps == 1 ? PC_CONV1 : PC_CONV3, conv_flops(a), conv_bytes(a), s);   // taps 4 = folded upsample + 3x3
        launch_conv(a, s);
    }
    if (a.stats) h->stat_n[a.out] = nrec;
    return 0;
}

#define HIPCHECK(h, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return fail(h, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

template <typename T>
int dev_alloc(cddpm_ctx* h, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(h, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    h->allocs.push_back(q);
    h->alloc_bytes += bytes;
    *p = reinterpret_cast<T*>(q);
    return 0;
}

bool in_list(const int* v, int n, int x) {
    for (int i = 0; i < n; ++i) if (v[i] == x) return true;
    return false;
}

int validate_desc(cddpm_ctx* h, const cddpm_unet_desc* d) {
    if (!d) return fail(h, "descriptor is NULL");
    if (d->in_channels != 1 || d->out_channels != 1)
        return fail(h, "in_channels/out_channels must be 1 (got %d/%d)", d->in_channels, d->out_channels);
    if (d->model_channels <= 0 || d->model_channels % 128 != 0 || d->model_channels > 512)
        return fail(h, "model_channels must be 128, 256, 384 or 512 (MFMA tile N = 128), got %d", d->model_channels);
    if (d->num_levels < 1 || d->num_levels > CDDPM_MAX_LEVELS) return fail(h, "num_levels out of range: %d", d->num_levels);
    for (int i = 0; i < d->num_levels; ++i)
        if (d->channel_mult[i] < 1 || d->channel_mult[i] * d->model_channels > 1024)
            return fail(h, "channel_mult[%d]=%d unsupported", i, d->channel_mult[i]);
    if (d->num_res_blocks < 1) return fail(h, "num_res_blocks must be >= 1");
    if (d->num_attention_resolutions < 0 || d->num_attention_resolutions > CDDPM_MAX_LEVELS)
        return fail(h, "num_attention_resolutions out of range");
    if (d->head_channels != 64) return fail(h, "head_channels must be 64, got %d", d->head_channels);
    if (d->cond_dim < 0 || d->cond_dim % 4 != 0) return fail(h, "cond_dim must be a non-negative multiple of 4");
    if (d->timesteps < 1) return fail(h, "timesteps must be >= 1");
    const int q = 1 << (d->num_levels - 1);
    if (d->max_batch < 1 || d->max_h < q || d->max_w < q || d->max_h % q || d->max_w % q || d->max_h % 4 || d->max_w % 4)
        return fail(h, "max_batch/max_h/max_w invalid (H, W must be multiples of %d and of 4)", q > 4 ? q : 4);
    // pixel indices are 32-bit in the small kernels and inside a sample in the convolutions
    if ((long long)d->max_batch * d->max_h * d->max_w >= (1ll << 30) || (long long)d->max_h * d->max_w >= (1ll << 24))
        return fail(h, "max_batch * max_h * max_w must stay below 2^30 pixels (and one slice below 2^24): split the batch");
    return 0;
}

// ---- program construction: mirrors UNetModel.__init__ (src/models/modules/OpenAI_Unet.py:604-797)
void add_norm_spec(cddpm_ctx* h, const std::string& p, int C) {
    h->wspecs.push_back({p + ".weight", C});
    h->wspecs.push_back({p + ".bias", C});
}
void add_conv_spec(cddpm_ctx* h, const std::string& p, int Cin, int Cout, int k) {
    h->wspecs.push_back({p + ".weight", (int64_t)Cout * Cin * k});
    h->wspecs.push_back({p + ".bias", Cout});
}

int make_res(cddpm_ctx* h, const std::string& prefix, int Cin, int Cout, bool up, bool down) {
    ResW r;
    r.prefix = prefix; r.Cin = Cin; r.Cout = Cout; r.up = up; r.down = down; r.has_skip = (Cin != Cout);
    r.eoff = h->sumE;
    h->sumE += 2 * Cout;
    add_norm_spec(h, prefix + ".in_layers.0", Cin);
    add_conv_spec(h, prefix + ".in_layers.2", Cin, Cout, 9);
    h->wspecs.push_back({prefix + ".emb_layers.1.weight", (int64_t)2 * Cout * h->E});
    h->wspecs.push_back({prefix + ".emb_layers.1.bias", 2 * Cout});
    add_norm_spec(h, prefix + ".out_layers.0", Cout);
    add_conv_spec(h, prefix + ".out_layers.3", Cout, Cout, 9);
    if (r.has_skip) add_conv_spec(h, prefix + ".skip_connection", Cin, Cout, 1);
    h->res.push_back(r);
    return (int)h->res.size() - 1;
}
int make_attn(cddpm_ctx* h, const std::string& prefix, int C) {
    AttnW a;
    a.prefix = prefix; a.C = C;
    add_norm_spec(h, prefix + ".norm", C);
    add_conv_spec(h, prefix + ".qkv", C, 3 * C, 1);
    add_conv_spec(h, prefix + ".proj_out", C, C, 1);
    h->attn.push_back(a);
    return (int)h->attn.size() - 1;
}

void build_program(cddpm_ctx* h) {
    const cddpm_unet_desc& d = h->d;
    const int C = d.model_channels;
    h->half = 4 * C;
    h->E = d.cond_dim > 0 ? 2 * h->half : h->half;
    if (d.cond_dim > 0) {
        h->wspecs.push_back({"label_emb.0.weight", (int64_t)h->half * d.cond_dim});
        h->wspecs.push_back({"label_emb.0.bias", h->half});
        h->wspecs.push_back({"label_emb.2.weight", (int64_t)h->half * h->half});
        h->wspecs.push_back({"label_emb.2.bias", h->half});
    }
    h->wspecs.push_back({"time_embed.0.weight", (int64_t)h->half * C});
    h->wspecs.push_back({"time_embed.0.bias", h->half});
    h->wspecs.push_back({"time_embed.2.weight", (int64_t)h->half * h->half});
    h->wspecs.push_back({"time_embed.2.bias", h->half});
    add_conv_spec(h, "input_blocks.0.0", 1, C, 9);

    auto new_block = [&](const std::string& name, int Cb, int ds) {
        h->blocks.push_back({name, Cb, ds});
        return (int)h->blocks.size() - 1;
    };
    std::vector<int> chans;
    int ch = C, ds = 1, idx = 1;
    int blk = new_block("input_blocks.0", C, 1);
    h->prog.push_back({OP_IN, 0, false, true, true, blk});
    chans.push_back(C);
    for (int level = 0; level < d.num_levels; ++level) {
        const int co = d.channel_mult[level] * C;
        for (int i = 0; i < d.num_res_blocks; ++i) {
            const std::string bn = "input_blocks." + std::to_string(idx);
            const bool at = in_list(d.attention_resolutions, d.num_attention_resolutions, ds);
            blk = new_block(bn, co, ds);
            h->prog.push_back({OP_RES, make_res(h, bn + ".0", ch, co, false, false), false, !at, !at, blk});
            ch = co;
            if (at) h->prog.push_back({OP_ATTN, make_attn(h, bn + ".1", ch), false, true, true, blk});
            chans.push_back(ch);
            ++idx;
        }
        if (level != d.num_levels - 1) {
            const std::string bn = "input_blocks." + std::to_string(idx);
            ds *= 2;
            blk = new_block(bn, ch, ds);
            h->prog.push_back({OP_RES, make_res(h, bn + ".0", ch, ch, false, true), false, true, true, blk});
            chans.push_back(ch);
            ++idx;
        }
    }
    blk = new_block("middle_block.0", ch, ds);
    h->prog.push_back({OP_RES, make_res(h, "middle_block.0", ch, ch, false, false), false, false, true, blk});
    blk = new_block("middle_block.1", ch, ds);
    h->prog.push_back({OP_ATTN, make_attn(h, "middle_block.1", ch), false, false, true, blk});
    blk = new_block("middle_block.2", ch, ds);
    h->prog.push_back({OP_RES, make_res(h, "middle_block.2", ch, ch, false, false), false, false, true, blk});
    idx = 0;
    for (int level = d.num_levels - 1; level >= 0; --level) {
        const int co = d.channel_mult[level] * C;
        for (int i = 0; i <= d.num_res_blocks; ++i) {
            const int ich = chans.back();
            chans.pop_back();
            const std::string bn = "output_blocks." + std::to_string(idx);
            const bool at = in_list(d.attention_resolutions, d.num_attention_resolutions, ds);
            const bool upb = (level > 0 && i == d.num_res_blocks);
            const int ds_out = upb ? ds / 2 : ds;
            blk = new_block(bn, co, ds_out);
            h->prog.push_back({OP_RES, make_res(h, bn + ".0", ch + ich, co, false, false), true, false, !at && !upb, blk});
            ch = co;
            int sub = 1;
            if (at) {
                h->prog.push_back({OP_ATTN, make_attn(h, bn + "." + std::to_string(sub), ch), false, false, !upb, blk});
                ++sub;
            }
            if (upb) {
                h->prog.push_back({OP_RES, make_res(h, bn + "." + std::to_string(sub), ch, ch, true, false), false, false, true, blk});
                ds /= 2;
            }
            ++idx;
        }
    }
    add_norm_spec(h, "out.0", ch);
    add_conv_spec(h, "out.2", ch, 1, 9);
    blk = new_block("out", 1, 1);
    h->prog.push_back({OP_HEAD, 0, false, false, true, blk});
    h->taps.assign(h->blocks.size(), nullptr);
}

// Shape limits of the kernels, checked on the built program (a descriptor can pass validate_desc and still concatenate
// more channels than a kernel's LDS arrays hold): a GroupNorm / convolution input of C0 + C1 channels needs
// 3 (C0 + C1) floats of coefficient cache beside the conv's patch and weight stages in 160 KB of LDS, and
// gn_finalize_kernel keeps one fp64 (sum, sum of squares) pair per concatenated channel in LDS.
constexpr int MAX_CONCAT_CHANNELS = 1536;
int check_program(cddpm_ctx* h, cddpm_ctx* err_to) {
    for (const ResW& r : h->res)
        if (r.Cin > MAX_CONCAT_CHANNELS)
            return fail(err_to, "ResBlock %s reads %d concatenated channels; this library supports at most %d "
                        "(model_channels x channel_mult too wide for the fused GroupNorm/convolution kernels)",
                        r.prefix.c_str(), r.Cin, MAX_CONCAT_CHANNELS);
    return 0;
}

size_t plan_workspace(cddpm_ctx* h, bool do_alloc, int* rc) {
    // returns the byte count; allocates when do_alloc
    const cddpm_unet_desc& d = h->d;
    const size_t B = d.max_batch, HW = (size_t)d.max_h * d.max_w;
    size_t total = 0;
    *rc = 0;
    auto want = [&](float** p, size_t elems) {
        total += elems * sizeof(float);
        if (do_alloc && *rc == 0) *rc = dev_alloc(h, p, elems);
    };
    // skip stack: one tensor per pushing op
    size_t maxact = 0, maxC = 0;
    h->hs.clear();
    h->hs_elems.clear();
    for (const Op& op : h->prog) {
        const BlockInfo& bi = h->blocks[op.block];
        const size_t elems = B * (HW / ((size_t)bi.ds * bi.ds)) * bi.C;
        if (op.kind != OP_HEAD) maxact = std::max(maxact, elems);
        if (op.push) {
            float* p = nullptr;
            want(&p, elems);
            h->hs.push_back(p);
            h->hs_elems.push_back(elems);
        }
    }
    for (const ResW& r : h->res) {
        maxC = std::max(maxC, (size_t)std::max(r.Cin, r.Cout));
        if (r.up) {   // conv1 output of an up block lives at the doubled resolution
            // covered by maxact through the block's own output size (same C, same resolution)
        }
    }
    for (const AttnW& a : h->attn) maxC = std::max(maxC, (size_t)a.C);
    want(&h->bufA, maxact);
    want(&h->bufB, maxact);
    want(&h->bufH, maxact);
    want(&h->bufP0, maxact / 4 + 16);
    want(&h->bufP1, maxact / 4 + 16);
    size_t maxqkv = 0, maxatt = 0;
    for (const Op& op : h->prog)
        if (op.kind == OP_ATTN) {
            const BlockInfo& bi = h->blocks[op.block];
            const AttnW& a = h->attn[op.idx];
            // an attention op inside an up block runs before the upsample: resolution of the block input
            int dsa = bi.ds;
            for (const Op& o2 : h->prog)
                if (o2.block == op.block && o2.kind == OP_RES && h->res[o2.idx].up) dsa = bi.ds * 2;
            const size_t n = HW / ((size_t)dsa * dsa);
            maxqkv = std::max(maxqkv, B * n * 3 * a.C);
            maxatt = std::max(maxatt, B * n * a.C);
        }
    want(&h->qkvbuf, maxqkv);
    want(&h->attbuf, maxatt);
    want(&h->headP, B * HW * 9);
    want(&h->model_out, B * HW);
    h->max_nsplit = gn_nsplit(1, (int)HW);
    {
        // statistics records: [B][records][C][2] fp32 per buffer that can feed a GroupNorm
        auto nrec_at = [&](int ds) {
            const int hh = d.max_h / ds, ww = d.max_w / ds;
            // a tensor may be produced by the plain conv, the folded-upsample conv (more, smaller tiles on small
            // images) or swept by gn_partial: size for the largest record count
            return std::max(std::max(conv_stat_records(hh, ww), conv_stat_records_up2(hh, ww)), gn_nsplit(1, hh * ww));
        };
        size_t pi = 0;
        for (const Op& op : h->prog)
            if (op.push) {
                const BlockInfo& bi = h->blocks[op.block];
                float* sp = nullptr;
                want(&sp, B * (size_t)nrec_at(bi.ds) * bi.C * 2);
                if (do_alloc) { h->stat_buf[h->hs[pi]] = sp; h->stat_cap[h->hs[pi]] = B * (size_t)nrec_at(bi.ds) * bi.C * 2; }
                ++pi;
            }
        size_t maxrc = 0;
        for (const BlockInfo& bi : h->blocks) maxrc = std::max(maxrc, (size_t)nrec_at(bi.ds) * bi.C);
        float* work[3] = {h->bufA, h->bufB, h->bufH};
        for (int i = 0; i < 3; ++i) {
            float* sp = nullptr;
            want(&sp, B * maxrc * 2);
            if (do_alloc) { h->stat_buf[work[i]] = sp; h->stat_cap[work[i]] = B * maxrc * 2; }
        }
    }
    want(&h->coef, 3 * B * maxC);
    want(&h->kpart, (size_t)KSPLIT_PLANE_FLOATS);
    // tables and embedding scratch
    const size_t rows = std::max<size_t>(d.timesteps, B);
    want(&h->tab, (size_t)d.timesteps * h->sumE);
    want(&h->cpart, B * (size_t)h->sumE);
    want(&h->scratch0, rows * std::max(h->half, d.model_channels));
    want(&h->scratch1, rows * h->half);
    for (int i = 0; i < 5; ++i) want(&h->sched[i], d.timesteps);
    want(&h->qs_sa, d.timesteps);
    want(&h->qs_s1, d.timesteps);
    total += B * sizeof(int);
    if (do_alloc && *rc == 0) *rc = dev_alloc(h, &h->d_t, B);
    // weights
    for (const WeightSpec& w : h->wspecs) total += (size_t)w.numel * sizeof(float);
    total += (size_t)h->sumE * sizeof(float);   // combined emb bias is part of wspecs already; slack
    return total;
}

struct HostWeights {
    std::map<std::string, std::pair<const float*, int64_t>> m;
    const float* get(const std::string& n) const { return m.at(n).first; }
};

int upload(cddpm_ctx* h, float** dst, const float* src, size_t n) {
    if (dev_alloc(h, dst, n)) return -1;
    HIPCHECK(h, hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int upload_norm(cddpm_ctx* h, const HostWeights& hw, const std::string& p, int C, NormW* n) {
    n->C = C;
    if (upload(h, &n->gamma, hw.get(p + ".weight"), C)) return -1;
    return upload(h, &n->beta, hw.get(p + ".bias"), C);
}

// wexp < 0: choose the pre-scale exponent from this tensor; >= 0: imposed (tensors accumulated into one output tile share it)
int upload_conv(cddpm_ctx* h, const HostWeights& hw, const std::string& p, int Cin, int Cout, int taps, ConvW* c,
                bool with_bias = true, int wexp = -1) {
    c->Cin = Cin; c->Cout = Cout; c->taps = taps;
    const float* w = hw.get(p + ".weight");
    c->wexp = wexp >= 0 ? wexp : conv_weight_exp(w, (size_t)Cout * Cin * taps, h->family);
    std::vector<float> pk(packed_conv_floats(Cout, Cin, taps, h->family));
    pack_conv_weights(w, Cout, Cin, taps, pk.data(), c->wexp, h->family);
    if (upload(h, &c->wpk, pk.data(), pk.size())) return -1;
    if (with_bias) return upload(h, &c->bias, hw.get(p + ".bias"), Cout);
    return 0;
}

// statistics records of a tensor for the current forward: fused by its producer, else swept here once
const float* stats_of(cddpm_ctx* h, const float* x, int C, int B, int HW, int* n, hipStream_t s) {
    auto it = h->stat_n.find(x);
    float* rec = h->stat_buf.at(x);
    if (it == h->stat_n.end()) {
        const int ns = gn_nsplit(B, HW);
        if ((size_t)B * ns * C * 2 > h->stat_cap.at(x)) {
            fail(h, "GroupNorm statistics sweep of a [%d,%d,%d] tensor needs %zu floats, the buffer holds %zu", B, HW, C,
                 (size_t)B * ns * C * 2, h->stat_cap.at(x));
            return nullptr;
        }
        Prof p(h, PC_GN, 0.0, 4.0 * B * (double)HW * C, s);
        launch_gn_partial(x, C, B, HW, ns, rec, s);
        h->stat_n[x] = ns;
        *n = ns;
    } else {
        *n = it->second;
    }
    return rec;
}

int gn_coef(cddpm_ctx* h, const float* x0, int C0, const float* x1, int C1, int B, int HW, const NormW& nw,
            bool film, int eoff, hipStream_t s) {
    int n0 = 0, n1 = 0;
    const float* r0 = stats_of(h, x0, C0, B, HW, &n0, s);
    const float* r1 = x1 ? stats_of(h, x1, C1, B, HW, &n1, s) : nullptr;
    if (!r0 || (x1 && !r1)) return -1;
    Prof p(h, PC_GN, 0.0, 8.0 * B * ((double)n0 * C0 + (double)n1 * C1), s);
    launch_gn_finalize(r0, C0, n0, r1, C1, n1, B, HW, nw.gamma, nw.beta, film ? h->tab : nullptr, h->cpart, h->sumE, eoff,
                       h->d_t, nullptr, h->coef, s);
    return 0;
}

void zero_conv_args(ConvArgs& a, const cddpm_ctx* h) { memset(&a, 0, sizeof a); a.family = h->family; }

// One ResBlock (src/models/modules/OpenAI_Unet.py:284-338): input x0 (+ x1 concatenated), output dst.
int run_res(cddpm_ctx* h, const ResW& r, const float* x0, int C0, const float* x1, int C1, float* dst, int B, int H,
            int W, hipStream_t s) {
    // H, W: resolution of the block INPUT
    if (gn_coef(h, x0, C0, x1, C1, B, H * W, r.gn1, false, 0, s)) return -1;
    ConvArgs a;
    zero_conv_args(a, h);
    a.B = B; a.Cout = r.Cout; a.taps = 9; a.wpk = r.conv1.wpk; a.bias = r.conv1.bias; a.out = h->bufH;
    a.wscale_inv = ldexpf(1.0f, -r.conv1.wexp);
    int Ho = H, Wo = W;
    const float* resid = x0;
    int res_up = 0;
    if (r.down) {
        Ho = H / 2; Wo = W / 2;
        {
            Prof pp(h, PC_OTHER, 0.0, 4.0 * B * (double)H * W * C0 * 1.5, s);
            launch_pool_act(x0, h->coef, h->bufP0, h->bufP1, B, H, W, C0, s);
        }
        a.src0 = h->bufP0; a.C0 = C0; a.srcH = Ho; a.srcW = Wo;
        resid = h->bufP1;
    } else if (r.up) {
        Ho = 2 * H; Wo = 2 * W;
        a.src0 = x0; a.C0 = C0; a.srcH = H; a.srcW = W; a.coef = h->coef; a.silu = 1;
        a.taps = 4; a.wpk = r.conv1_up2;      // folded upsample + conv
        res_up = 1;
    } else {
        a.src0 = x0; a.C0 = C0; a.src1 = x1; a.C1 = C1; a.srcH = H; a.srcW = W; a.coef = h->coef; a.silu = 1;
    }
    a.H = Ho; a.W = Wo;
    if (conv_launch(h, a, s)) return -1;
    // out_layers: GroupNorm * (1 + scale) + shift -> SiLU -> conv, + skip
    if (gn_coef(h, h->bufH, r.Cout, nullptr, 0, B, Ho * Wo, r.gn2, true, r.eoff, s)) return -1;
    ConvArgs c;
    zero_conv_args(c, h);
    c.B = B; c.H = Ho; c.W = Wo; c.Cout = r.Cout; c.taps = 9;
    c.src0 = h->bufH; c.C0 = r.Cout; c.srcH = Ho; c.srcW = Wo; c.coef = h->coef; c.silu = 1;
    c.wpk = r.conv2.wpk; c.bias = r.bias2; c.out = dst; c.wscale_inv = ldexpf(1.0f, -r.conv2.wexp);
    if (r.has_skip) {
        c.skip0 = x0; c.S0 = C0; c.skip1 = x1; c.S1 = C1; c.skip_wpk = r.skip.wpk;
    } else {
        c.res = resid; c.res_up = res_up;
    }
    return conv_launch(h, c, s);
}

// AttentionBlock (OpenAI_Unet.py:386-394)
int run_attn(cddpm_ctx* h, const AttnW& w, const float* x, float* dst, int B, int H, int W, hipStream_t s) {
    const int N = H * W;
    if (gn_coef(h, x, w.C, nullptr, 0, B, N, w.norm, false, 0, s)) return -1;
    ConvArgs a;
    zero_conv_args(a, h);
    a.B = B; a.H = H; a.W = W; a.Cout = 3 * w.C; a.taps = 1;
    a.src0 = x; a.C0 = w.C; a.srcH = H; a.srcW = W; a.coef = h->coef; a.silu = 0;
    a.wpk = w.qkv.wpk; a.bias = w.qkv.bias; a.out = h->qkvbuf; a.wscale_inv = ldexpf(1.0f, -w.qkv.wexp);
    if (conv_launch(h, a, s)) return -1;
    {
        Prof pa(h, PC_ATTN, 4.0 * B * (double)N * N * w.C, 4.0 * B * (double)N * 4 * w.C, s);
        launch_attention(h->qkvbuf, h->attbuf, B, N, w.C, s);
    }
    ConvArgs p;
    zero_conv_args(p, h);
    p.B = B; p.H = H; p.W = W; p.Cout = w.C; p.taps = 1;
    p.src0 = h->attbuf; p.C0 = w.C; p.srcH = H; p.srcW = W;
    p.wpk = w.proj.wpk; p.bias = w.proj.bias; p.res = x; p.out = dst; p.wscale_inv = ldexpf(1.0f, -w.proj.wexp);
    return conv_launch(h, p, s);
}

// a call that needs weights on a handle that has none: which of the two reasons
int weights_missing(cddpm_ctx* h) {
    if (h->weights_dropped)
        return fail(h, "the convolution family was changed after cddpm_load_weights: the packed weights of the previous family were "
                       "dropped, load the weights (and set the schedule) again");
    return fail(h, "weights not loaded (cddpm_load_weights)");
}

int check_call(cddpm_ctx* h, int B, int H, int W) {
    if (!h) return -1;
    if (!h->weights_loaded) return weights_missing(h);
    if (!h->schedule_set) return fail(h, "schedule not set (cddpm_set_schedule)");
    const int q = 1 << (h->d.num_levels - 1);
    if (B < 1 || B > h->d.max_batch) return fail(h, "B=%d outside [1, max_batch=%d]", B, h->d.max_batch);
    if (H < q || W < q || H % q || W % q || H % 4 || W % 4 || H > h->d.max_h || W > h->d.max_w ||
        (size_t)H * W > (size_t)h->d.max_h * h->d.max_w)
        return fail(h, "H=%d W=%d invalid for this handle (multiples of %d, max %dx%d)", H, W, q > 4 ? q : 4, h->d.max_h, h->d.max_w);
    if (h->cond_B != B) return fail(h, "cddpm_prepare_cond was last called for B=%d, this call has B=%d", h->cond_B, B);
    return 0;
}

// UNetModel.forward (OpenAI_Unet.py:823-1006); d_t must hold the per-sample timesteps.
int forward_impl(cddpm_ctx* h, const float* x, float* out, int B, int H, int W, hipStream_t s) {
    h->stat_n.clear();        // no tensor of this forward has statistics yet
    h->cur_H = H; h->cur_W = W;
    std::vector<int> stack;   // indices into h->hs
    int npush = 0;
    const float* cur = nullptr;
    int curC = 0, curds = 1;
    float* pp[2] = {h->bufA, h->bufB};
    int ppi = 0;
    for (size_t oi = 0; oi < h->prog.size(); ++oi) {
        const Op& op = h->prog[oi];
        const BlockInfo& bi = h->blocks[op.block];
        float* dst;
        if (op.push) dst = h->hs[npush];
        else { dst = pp[ppi]; ppi ^= 1; }
        const int Hc = H / curds, Wc = W / curds;
        switch (op.kind) {
            case OP_IN: {
                Prof pi(h, PC_OTHER, 18.0 * B * H * W * h->d.model_channels, 4.0 * B * (double)H * W * (h->d.model_channels + 1), s);
                launch_conv_in1(x, h->in_w, h->in_b, dst, B, H, W, h->d.model_channels, s);
            }
                curC = h->d.model_channels;
                break;
            case OP_RES: {
                const ResW& r = h->res[op.idx];
                const float* x1 = nullptr;
                int C1 = 0;
                if (op.concat) {
                    const int si = stack.back();
                    stack.pop_back();
                    x1 = h->hs[si];
                    C1 = r.Cin - curC;
                }
                if (dst == cur) { dst = pp[ppi]; ppi ^= 1; }
                if (run_res(h, r, cur, curC, x1, C1, dst, B, Hc, Wc, s)) return -1;
                curC = r.Cout;
                if (r.down) curds *= 2;
                if (r.up) curds /= 2;
                break;
            }
            case OP_ATTN:
                if (dst == cur) { dst = pp[ppi]; ppi ^= 1; }
                if (run_attn(h, h->attn[op.idx], cur, dst, B, Hc, Wc, s)) return -1;
                break;
            case OP_HEAD: {
                if (gn_coef(h, cur, curC, nullptr, 0, B, H * W, h->out_norm, false, 0, s)) return -1;
                Prof ph(h, PC_OTHER, 18.0 * B * H * W * curC, 4.0 * B * (double)H * W * (curC + 19), s);
                launch_head_dots(cur, h->coef, h->head_w9, h->headP, B, H * W, curC, s);
                launch_head_gather(h->headP, h->head_bias, nullptr, out, B, H, W, s);
                dst = nullptr;
                break;
            }
        }
        if (op.push) { stack.push_back(npush); ++npush; }
        if (dst) cur = dst;
        if (op.block_end && dst && h->taps[op.block]) {
            const size_t elems = (size_t)B * (H / bi.ds) * (W / bi.ds) * bi.C;
            HIPCHECK(h, hipMemcpyAsync(h->taps[op.block], dst, elems * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    HIPCHECK(h, hipGetLastError());
    return 0;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
// ---- temporaries and parameters of the standalone operators ------------------------------------------------------------------
// Temporaries come from the handle's scratch arena when cddpm_op_set_scratch gave it one (re-used from its start by every call: calls
// on ONE stream are ordered, nothing synchronises -- what the training step runs on); without an arena they are hipMalloc'ed for the
// call and freed after a stream synchronisation (the kernel tests).
struct OpScratch {
    cddpm_ctx* h;
    hipStream_t s;
    std::vector<void*> owned;
    size_t off = 0;
    bool failed = false;
    OpScratch(cddpm_ctx* h_, hipStream_t s_) : h(h_), s(s_) {}
    void* get(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (h->arena) {
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
    // a parameter vector given in host OR device memory: device pointers are used where they lie, host ones are staged
    const float* param(const float* p, size_t count) {
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

extern "C" {

const char* cddpm_last_error(cddpm_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

size_t cddpm_workspace_bytes(const cddpm_unet_desc* desc) {
    cddpm_ctx tmp;
    if (validate_desc(nullptr, desc)) return 0;
    tmp.d = *desc;
    build_program(&tmp);
    if (check_program(&tmp, nullptr)) return 0;
    int rc = 0;
    return plan_workspace(&tmp, false, &rc);
}

int cddpm_create(cddpm_handle* out, const cddpm_unet_desc* desc, int device) {
    if (!out) return fail(nullptr, "out is NULL");
    *out = nullptr;
    if (validate_desc(nullptr, desc)) return -1;
    {   // shape limits of the program, before any device is touched (testable without a GPU)
        cddpm_ctx tmp;
        tmp.d = *desc;
        build_program(&tmp);
        if (check_program(&tmp, nullptr)) return -1;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, "no HIP device available: %s", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, "device %d out of range (%d devices)", device, ndev);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(nullptr, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    cddpm_ctx* h = new cddpm_ctx();
    h->d = *desc;
    h->device = device;
    build_program(h);
    int rc = 0;
    plan_workspace(h, true, &rc);
    if (rc) {
        g_create_error = h->err;
        cddpm_destroy(h);
        return -1;
    }
    *out = h;
    return 0;
}

static void drop_step_graph(cddpm_ctx* h);
void cddpm_destroy(cddpm_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    drop_step_graph(h);
    if (h->gev_in) (void)hipEventDestroy(h->gev_in);
    if (h->gev_out) (void)hipEventDestroy(h->gev_out);
    if (h->gstream) (void)hipStreamDestroy(h->gstream);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->arena) (void)hipFree(h->arena);
    if (h->zero_bias) (void)hipFree(h->zero_bias);
    { hipEvent_t shared = nullptr;
      for (auto& r : h->prof) { if (r.a != shared) (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); shared = r.b; } }
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    delete h;
}

int cddpm_num_weights(cddpm_handle h) { return h ? (int)h->wspecs.size() : -1; }
const char* cddpm_weight_name(cddpm_handle h, int i) {
    return (h && i >= 0 && i < (int)h->wspecs.size()) ? h->wspecs[i].name.c_str() : nullptr;
}
int64_t cddpm_weight_numel(cddpm_handle h, int i) {
    return (h && i >= 0 && i < (int)h->wspecs.size()) ? h->wspecs[i].numel : -1;
}

int cddpm_num_blocks(cddpm_handle h) { return h ? (int)h->blocks.size() : -1; }
const char* cddpm_block_name(cddpm_handle h, int i) {
    return (h && i >= 0 && i < (int)h->blocks.size()) ? h->blocks[i].name.c_str() : nullptr;
}
int cddpm_set_tap(cddpm_handle h, int block, float* dst_dev) {
    if (!h) return -1;
    h->gen++;
    if (block < 0 || block >= (int)h->blocks.size()) return fail(h, "block %d out of range", block);
    h->taps[block] = dst_dev;
    return 0;
}
int cddpm_block_shape(cddpm_handle h, int block, int H, int W, int* C, int* h_out, int* w_out) {
    if (!h) return -1;
    if (block < 0 || block >= (int)h->blocks.size()) return fail(h, "block %d out of range", block);
    const BlockInfo& bi = h->blocks[block];
    if (C) *C = bi.C;
    if (h_out) *h_out = H / bi.ds;
    if (w_out) *w_out = W / bi.ds;
    return 0;
}

int cddpm_load_weights(cddpm_handle h, const char* const* names, const float* const* host_ptrs, const int64_t* numels,
                       int n) {
    if (!h) return -1;
    h->gen++;
    if (h->weights_loaded) return fail(h, "weights already loaded for this handle (create a new handle)");
    HIPCHECK(h, hipSetDevice(h->device));
    h->weight_allocs_begin = h->allocs.size();
    HostWeights hw;
    for (int i = 0; i < n; ++i) hw.m[names[i]] = {host_ptrs[i], numels[i]};
    for (const WeightSpec& w : h->wspecs) {
        auto it = hw.m.find(w.name);
        if (it == hw.m.end()) return fail(h, "missing weight '%s'", w.name.c_str());
        if (it->second.second != w.numel)
            return fail(h, "weight '%s' has %lld elements, expected %lld", w.name.c_str(), (long long)it->second.second,
                        (long long)w.numel);
        if (!it->second.first) return fail(h, "weight '%s' has a NULL pointer", w.name.c_str());
    }
    const int C = h->d.model_channels;
    // embedding MLPs
    if (h->d.cond_dim > 0) {
        if (upload(h, &h->le0_w, hw.get("label_emb.0.weight"), (size_t)h->half * h->d.cond_dim)) return -1;
        if (upload(h, &h->le0_b, hw.get("label_emb.0.bias"), h->half)) return -1;
        if (upload(h, &h->le2_w, hw.get("label_emb.2.weight"), (size_t)h->half * h->half)) return -1;
        if (upload(h, &h->le2_b, hw.get("label_emb.2.bias"), h->half)) return -1;
    }
    if (upload(h, &h->te0_w, hw.get("time_embed.0.weight"), (size_t)h->half * C)) return -1;
    if (upload(h, &h->te0_b, hw.get("time_embed.0.bias"), h->half)) return -1;
    if (upload(h, &h->te2_w, hw.get("time_embed.2.weight"), (size_t)h->half * h->half)) return -1;
    if (upload(h, &h->te2_b, hw.get("time_embed.2.bias"), h->half)) return -1;
    // input conv [C][1][3][3] is already [C][9]
    if (upload(h, &h->in_w, hw.get("input_blocks.0.0.weight"), (size_t)C * 9)) return -1;
    if (upload(h, &h->in_b, hw.get("input_blocks.0.0.bias"), C)) return -1;
    // ResBlocks
    std::vector<float> embw((size_t)h->sumE * h->E), embb(h->sumE);
    for (ResW& r : h->res) {
        if (upload_norm(h, hw, r.prefix + ".in_layers.0", r.Cin, &r.gn1)) return -1;
        if (r.up) {
            // the upsampled tensor is never built: Upsample(nearest x2) + Conv3x3 (OpenAI_Unet.py:118-128, :289-293) is
            // evaluated as four 2x2-tap convolutions of the low-resolution input (4/9 of the multiplies)
            r.conv1.Cin = r.Cin; r.conv1.Cout = r.Cout; r.conv1.taps = 4;
            std::vector<float> pk(4 * packed_conv_floats(r.Cout, r.Cin, 4, h->family));
            r.conv1.wexp = pack_conv_weights_up2(hw.get(r.prefix + ".in_layers.2.weight"), r.Cout, r.Cin, pk.data(), h->family);
            if (upload(h, &r.conv1_up2, pk.data(), pk.size())) return -1;
            if (upload(h, &r.conv1.bias, hw.get(r.prefix + ".in_layers.2.bias"), r.Cout)) return -1;
        } else if (upload_conv(h, hw, r.prefix + ".in_layers.2", r.Cin, r.Cout, 9, &r.conv1)) return -1;
        if (upload_norm(h, hw, r.prefix + ".out_layers.0", r.Cout, &r.gn2)) return -1;
        // conv2 and the fused 1x1 skip_connection accumulate into the same tile: one pre-scale exponent for both
        int e2 = conv_weight_exp(hw.get(r.prefix + ".out_layers.3.weight"), (size_t)r.Cout * r.Cout * 9, h->family);
        if (r.has_skip) e2 = std::min(e2, conv_weight_exp(hw.get(r.prefix + ".skip_connection.weight"), (size_t)r.Cout * r.Cin, h->family));
        if (upload_conv(h, hw, r.prefix + ".out_layers.3", r.Cout, r.Cout, 9, &r.conv2, false, e2)) return -1;
        std::vector<float> b2(hw.get(r.prefix + ".out_layers.3.bias"), hw.get(r.prefix + ".out_layers.3.bias") + r.Cout);
        if (r.has_skip) {
            if (upload_conv(h, hw, r.prefix + ".skip_connection", r.Cin, r.Cout, 1, &r.skip, false, e2)) return -1;
            const float* bs = hw.get(r.prefix + ".skip_connection.bias");
            for (int i = 0; i < r.Cout; ++i) b2[i] += bs[i];
        }
        if (upload(h, &r.bias2, b2.data(), r.Cout)) return -1;
        memcpy(&embw[(size_t)r.eoff * h->E], hw.get(r.prefix + ".emb_layers.1.weight"), (size_t)2 * r.Cout * h->E * sizeof(float));
        memcpy(&embb[r.eoff], hw.get(r.prefix + ".emb_layers.1.bias"), (size_t)2 * r.Cout * sizeof(float));
    }
    if (upload(h, &h->emb_w, embw.data(), embw.size())) return -1;
    if (upload(h, &h->emb_b, embb.data(), embb.size())) return -1;
    for (AttnW& a : h->attn) {
        if (upload_norm(h, hw, a.prefix + ".norm", a.C, &a.norm)) return -1;
        if (upload_conv(h, hw, a.prefix + ".qkv", a.C, 3 * a.C, 1, &a.qkv)) return -1;
        if (upload_conv(h, hw, a.prefix + ".proj_out", a.C, a.C, 1, &a.proj)) return -1;
    }
    // head: out.2.weight [1][C][3][3] -> [9][C]
    {
        const int Ch = h->blocks[h->prog[h->prog.size() - 2].block].C;
        if (upload_norm(h, hw, "out.0", Ch, &h->out_norm)) return -1;
        const float* w = hw.get("out.2.weight");
        std::vector<float> w9((size_t)9 * Ch);
        for (int c = 0; c < Ch; ++c)
            for (int t = 0; t < 9; ++t) w9[(size_t)t * Ch + c] = w[(size_t)c * 9 + t];
        if (upload(h, &h->head_w9, w9.data(), w9.size())) return -1;
        h->head_bias = hw.get("out.2.bias")[0];
    }
    h->weights_loaded = true;
    h->weights_dropped = false;
    return 0;
}

int cddpm_set_schedule(cddpm_handle h, const float* coef1, const float* coef2, const float* logvar,
                       const float* sqrt_recip, const float* sqrt_recipm1, int T, int objective) {
    if (!h) return -1;
    h->gen++;
    if (!h->weights_loaded) return fail(h, "load weights before cddpm_set_schedule (it builds the embedding tables)");
    if (T != h->d.timesteps) return fail(h, "T=%d does not match the handle's timesteps=%d", T, h->d.timesteps);
    if (objective != CDDPM_PRED_X0 && objective != CDDPM_PRED_NOISE) return fail(h, "unknown objective %d", objective);
    if (!coef1 || !coef2 || !logvar) return fail(h, "coef1/coef2/logvar must not be NULL");
    if (!sqrt_recip || !sqrt_recipm1)      // read by pred_noise steps and by every DDIM step (also under pred_x0)
        return fail(h, "sqrt_recip_alphas_cumprod and sqrt_recipm1_alphas_cumprod must not be NULL");
    HIPCHECK(h, hipSetDevice(h->device));
    const float* src[5] = {coef1, coef2, logvar, sqrt_recip, sqrt_recipm1};
    for (int i = 0; i < 5; ++i) HIPCHECK(h, hipMemcpy(h->sched[i], src[i], (size_t)T * sizeof(float), hipMemcpyHostToDevice));
    h->objective = objective;
    // time-embedding table: timestep_embedding (util.py:151-171) -> time_embed MLP (OpenAI_Unet.py:598-602)
    // -> time half of every ResBlock's emb_layers (OpenAI_Unet.py:201-207, :300)
    const int C = h->d.model_channels, halfdim = C / 2;
    std::vector<float> temb((size_t)T * C, 0.f);
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < halfdim; ++i) {
            float a = (float)(-std::log(10000.0)) * (float)i;   // float32 arithmetic as torch does
            a = a / (float)halfdim;
            const float f = (float)std::exp((double)a);
            const float arg = (float)t * f;
            temb[(size_t)t * C + i] = (float)std::cos((double)arg);
            temb[(size_t)t * C + halfdim + i] = (float)std::sin((double)arg);
        }
    hipStream_t s = nullptr;
    HIPCHECK(h, hipMemcpy(h->scratch0, temb.data(), temb.size() * sizeof(float), hipMemcpyHostToDevice));
    launch_linear(h->scratch0, C, h->te0_w, C, 0, h->te0_b, h->scratch1, h->half, T, h->half, C, 0, s);
    launch_linear(h->scratch1, h->half, h->te2_w, h->half, 0, h->te2_b, h->scratch0, h->half, T, h->half, h->half, 1, s);
    launch_linear(h->scratch0, h->half, h->emb_w, h->E, 0, nullptr, h->tab, h->sumE, T, h->sumE, h->half, 1, s);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipDeviceSynchronize());
    h->schedule_set = true;
    return 0;
}

int cddpm_prepare_cond(cddpm_handle h, const float* cond_dev, int B, void* stream) {
    if (!h) return -1;
    if (!h->weights_loaded) return h->weights_dropped ? weights_missing(h) : fail(h, "weights not loaded");
    if (B < 1 || B > h->d.max_batch) return fail(h, "B=%d outside [1, %d]", B, h->d.max_batch);
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    if (h->d.cond_dim > 0) {
        if (!cond_dev) return fail(h, "cond_dev is NULL but the model is conditional (cond_dim=%d)", h->d.cond_dim);
        launch_linear(cond_dev, h->d.cond_dim, h->le0_w, h->d.cond_dim, 0, h->le0_b, h->scratch1, h->half, B, h->half,
                      h->d.cond_dim, 0, s);
        launch_linear(h->scratch1, h->half, h->le2_w, h->half, 0, h->le2_b, h->scratch0, h->half, B, h->half, h->half, 1, s);
        launch_linear(h->scratch0, h->half, h->emb_w, h->E, h->half, h->emb_b, h->cpart, h->sumE, B, h->sumE, h->half, 1, s);
    } else {
        launch_linear(h->scratch0, h->half, h->emb_w, h->E, 0, h->emb_b, h->cpart, h->sumE, B, h->sumE, 0, 0, s);
    }
    HIPCHECK(h, hipGetLastError());
    h->cond_B = B;
    return 0;
}

int cddpm_unet_forward(cddpm_handle h, const float* x_dev, const int32_t* t_dev, int t_uniform, float* out_dev, int B,
                       int H, int W, void* stream) {
    if (check_call(h, B, H, W)) return -1;
    if (!x_dev || !out_dev) return fail(h, "x_dev/out_dev must not be NULL");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    if (t_dev) {
        launch_copy_clamp_int(h->d_t, t_dev, B, 0, h->d.timesteps - 1, s);   // per-sample t index device tables: kept inside [0, T)
    } else {
        if (t_uniform < 0 || t_uniform >= h->d.timesteps) return fail(h, "t=%d outside [0, %d)", t_uniform, h->d.timesteps);
        launch_fill_int(h->d_t, B, t_uniform, s);
    }
    return forward_impl(h, x_dev, out_dev, B, H, W, s);
}

static int step_once(cddpm_ctx* h, float* img, const float* z_dev, uint64_t seed, uint64_t slice0, int t, int finalize,
                     int B, int H, int W, hipStream_t s) {
    launch_fill_int(h->d_t, B, t, s);
    h->nb2_now = (t >= h->nb2_tmin) ? 1 : 0;        // the step's accumulation plan: a function of t alone
    const int rc_fwd = forward_impl(h, img, h->model_out, B, H, W, s);
    h->nb2_now = 0;
    if (rc_fwd) return -1;
    StepArgs a;
    a.x = img; a.model_out = h->model_out; a.t_dev = h->d_t;
    a.coef1 = h->sched[0]; a.coef2 = h->sched[1]; a.logvar = h->sched[2];
    a.sqrt_recip = h->sched[3]; a.sqrt_recipm1 = h->sched[4];
    a.objective = h->objective;
    a.noise = z_dev; a.noise_t_stride = 0;
    a.seed = seed; a.slice0 = slice0; a.t_for_rng = t;
    a.B = B; a.HW = H * W; a.finalize = finalize; a.clip = h->clip_denoised;
    launch_step(a, s);
    return 0;
}

static void drop_step_graph(cddpm_ctx* h) {
    if (h->gstream) (void)hipStreamSynchronize(h->gstream);
    if (h->sg.exec) (void)hipGraphExecDestroy(h->sg.exec);
    if (h->sg.graph) (void)hipGraphDestroy(h->sg.graph);
    h->sg = cddpm_ctx::StepGraph();
}

// steps t_hi, t_hi - 1, ..., t_lo as replays of one captured step (the step maps to [0,1] exactly when its t is 0). The caller has run at least one eager step of this
// geometry before (one-time function attributes are set outside the capture).
static int reverse_by_graph(cddpm_ctx* h, float* img, const float* noise_dev, uint64_t seed, uint64_t slice0, int t_hi,
                            int t_lo, int B, int H, int W, hipStream_t s) {
    if (!h->gstream) {
        HIPCHECK(h, hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
        HIPCHECK(h, hipEventCreateWithFlags(&h->gev_in, hipEventDisableTiming));
        HIPCHECK(h, hipEventCreateWithFlags(&h->gev_out, hipEventDisableTiming));
    }
    cddpm_ctx::StepGraph& g = h->sg;
    if (t_hi >= h->nb2_tmin && t_lo < h->nb2_tmin) {       // the plan switches inside the range: two replays, one graph each
        if (reverse_by_graph(h, img, noise_dev, seed, slice0, t_hi, h->nb2_tmin, B, H, W, s)) return -1;
        return reverse_by_graph(h, img, noise_dev, seed, slice0, h->nb2_tmin - 1, t_lo, B, H, W, s);
    }
    const int plan = (t_lo >= h->nb2_tmin) ? 1 : 0;
    const bool hit = g.exec && g.img == img && g.noise == noise_dev && g.seed == seed && g.slice0 == slice0 && g.B == B &&
                     g.H == H && g.W == W && g.gen == h->gen && g.nb2 == plan;
    if (!hit) {
        drop_step_graph(h);
        HIPCHECK(h, hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal));
        h->nb2_now = plan;
        int rc = forward_impl(h, img, h->model_out, B, H, W, h->gstream);
        h->nb2_now = 0;
        StepArgs a;
        a.x = img; a.model_out = h->model_out; a.t_dev = h->d_t;
        a.coef1 = h->sched[0]; a.coef2 = h->sched[1]; a.logvar = h->sched[2];
        a.sqrt_recip = h->sched[3]; a.sqrt_recipm1 = h->sched[4];
        a.objective = h->objective;
        a.noise = noise_dev; a.noise_t_stride = (size_t)B * H * W;
        a.seed = seed; a.slice0 = slice0; a.t_for_rng = 0;
        a.B = B; a.HW = H * W; a.finalize = -1; a.clip = h->clip_denoised;
        launch_step(a, h->gstream);
        launch_add_int(h->d_t, B, -1, h->gstream);
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(h->gstream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return -1; }
        if (ec != hipSuccess) return fail(h, "hipStreamEndCapture: %s", hipGetErrorString(ec));
        g.graph = graph;
        HIPCHECK(h, hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
        g.img = img; g.noise = noise_dev; g.seed = seed; g.slice0 = slice0; g.B = B; g.H = H; g.W = W; g.gen = h->gen; g.nb2 = plan;
    }
    HIPCHECK(h, hipEventRecord(h->gev_in, s));
    HIPCHECK(h, hipStreamWaitEvent(h->gstream, h->gev_in, 0));
    launch_fill_int(h->d_t, B, t_hi, h->gstream);
    for (int t = t_hi; t >= t_lo; --t) HIPCHECK(h, hipGraphLaunch(g.exec, h->gstream));
    HIPCHECK(h, hipEventRecord(h->gev_out, h->gstream));
    HIPCHECK(h, hipStreamWaitEvent(s, h->gev_out, 0));
    return 0;
}

// Opt-in (CDDPM_GRAPH=1): measured on MI355X the replay is no faster than launching -- 45.4 vs 45.6 ms per step at B=64,
// 5.73 vs 5.63 at B=1 (tools/graph_time.py): the step is not launch-bound, the queue already runs ahead of the GPU.
static bool graph_replay_enabled() {
    const char* e = getenv("CDDPM_GRAPH");
    return e && e[0] == '1';
}

int cddpm_p_sample(cddpm_handle h, float* img, const float* z_dev, uint64_t seed, uint64_t slice0, int t, int B, int H,
                   int W, void* stream) {
    if (check_call(h, B, H, W)) return -1;
    if (!img) return fail(h, "img_inout_dev is NULL");
    if (t < 0 || t >= h->d.timesteps) return fail(h, "t=%d outside [0, %d)", t, h->d.timesteps);
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    if (step_once(h, img, z_dev, seed, slice0, t, 0, B, H, W, s)) return -1;
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_ddim_step(cddpm_handle h, float* img, const float* z_dev, uint64_t seed, uint64_t slice0, int t, float coef_x0,
                    float coef_eps, float sigma, int add_noise, int finalize, int B, int H, int W, void* stream) {
    if (check_call(h, B, H, W)) return -1;
    if (!img) return fail(h, "img_inout_dev is NULL");
    if (t < 0 || t >= h->d.timesteps) return fail(h, "t=%d outside [0, %d)", t, h->d.timesteps);
    if (!(coef_x0 == coef_x0) || !(coef_eps == coef_eps) || !(sigma == sigma))
        return fail(h, "cddpm_ddim_step: NaN coefficient (time pair outside the schedule?)");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    launch_fill_int(h->d_t, B, t, s);
    if (forward_impl(h, img, h->model_out, B, H, W, s)) return -1;
    DdimArgs a;
    a.x = img; a.model_out = h->model_out; a.t_dev = h->d_t;
    a.sqrt_recip = h->sched[3]; a.sqrt_recipm1 = h->sched[4];
    a.objective = h->objective;
    a.coef_x0 = coef_x0; a.coef_eps = coef_eps; a.sigma = sigma; a.add_noise = add_noise ? 1 : 0;
    a.noise = z_dev; a.seed = seed; a.slice0 = slice0;
    a.B = B; a.HW = H * W; a.finalize = finalize ? 1 : 0; a.clip = h->clip_denoised;
    launch_ddim_step(a, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_reverse_range(cddpm_handle h, float* img, const float* noise_dev, uint64_t seed, uint64_t slice0, int t_hi,
                        int t_lo, int B, int H, int W, void* stream) {
    if (check_call(h, B, H, W)) return -1;
    if (!img) return fail(h, "img_inout_dev is NULL");
    if (t_lo < 0 || t_hi < t_lo || t_hi >= h->d.timesteps)
        return fail(h, "steps t_hi=%d .. t_lo=%d outside 0 <= t_lo <= t_hi < %d", t_hi, t_lo, h->d.timesteps);
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t HW = (size_t)H * W;
    int t = t_hi;
    bool tapped = false;
    for (float* p : h->taps) tapped = tapped || (p != nullptr);
    // CDDPM_GRAPH=1: the first step runs eagerly; with four or more to go the rest is replayed from a captured graph of one
    // step (per-launch profiling and block taps need eager launches)
    const bool by_graph = graph_replay_enabled() && !h->profiling && !tapped && (t_hi - t_lo + 1) >= 5;
    for (; t >= t_lo; --t) {
        if (step_once(h, img, noise_dev ? noise_dev + (size_t)t * B * HW : nullptr, seed, slice0, t, t == 0, B, H, W, s))
            return -1;
        if (by_graph) { --t; break; }
    }
    if (by_graph && t >= t_lo && reverse_by_graph(h, img, noise_dev, seed, slice0, t, t_lo, B, H, W, s)) return -1;
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_reverse(cddpm_handle h, float* img, const float* noise_dev, uint64_t seed, uint64_t slice0, int t_start, int B,
                  int H, int W, void* stream) {
    if (!h) return -1;
    if (t_start < 1 || t_start > h->d.timesteps) return fail(h, "t_start=%d outside [1, %d]", t_start, h->d.timesteps);
    return cddpm_reverse_range(h, img, noise_dev, seed, slice0, t_start - 1, 0, B, H, W, stream);
}

int cddpm_noise_fill(cddpm_handle h, float* out_dev, uint64_t seed, uint32_t stream_id, int t, uint64_t slice0, int B,
                     int H, int W, void* stream) {
    if (!h) return -1;
    if (!out_dev || B < 1 || H < 1 || W < 1 || (H * W) % 4) return fail(h, "bad arguments to cddpm_noise_fill");
    HIPCHECK(h, hipSetDevice(h->device));
    launch_noise_fill(out_dev, seed, stream_id, t, slice0, B, H * W, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_simplex_fill(cddpm_handle h, uint16_t* out_f16_dev, int64_t seed, int B, int H, int W, int octaves,
                       double persistence, double frequency, void* stream) {
    if (!h) return -1;
    if (!out_f16_dev || B < 1 || H < 1 || W < 1 || octaves < 1 || !(frequency > 0))
        return fail(h, "bad arguments to cddpm_simplex_fill");
    if (H != W)
        return fail(h, "simplex noise is defined for square fields only (the reference's _noise2a index assumes H == W), got %dx%d", H, W);
    HIPCHECK(h, hipSetDevice(h->device));
    launch_simplex(out_f16_dev, (long long)seed, B, H, W, octaves, persistence, frequency, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_residual_postprocess(cddpm_handle h, const float* orig_dev, const float* recon_dev, const float* mask_dev,
                               int S, int H, int W, int squared, int erode_iterations, int median_k, float* tmp_dev,
                               float* out_dev, void* stream) {
    if (!h) return -1;
    if (!orig_dev || !out_dev) return fail(h, "cddpm_residual_postprocess: NULL volume");
    if (S < 1 || H < 1 || W < 1 || (long long)S * H * W >= (1ll << 31)) return fail(h, "cddpm_residual_postprocess: bad S/H/W");
    if (erode_iterations < 0) return fail(h, "erode_iterations must be >= 0");
    if (median_k != 0 && median_k != 3 && median_k != 5) return fail(h, "median_k must be 0, 3 or 5, got %d", median_k);
    if (median_k && !tmp_dev) return fail(h, "cddpm_residual_postprocess: tmp_dev is NULL but median_k != 0");
    if (out_dev == orig_dev || out_dev == recon_dev || out_dev == mask_dev || (median_k && tmp_dev == out_dev))
        return fail(h, "cddpm_residual_postprocess: out_dev aliases an input");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    launch_residual_mask(orig_dev, recon_dev, mask_dev, median_k ? tmp_dev : out_dev, S, H, W, squared ? 1 : 0,
                         erode_iterations, s);
    if (median_k) launch_median3d(tmp_dev, out_dev, S, H, W, median_k, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

size_t cddpm_eval_workspace_bytes(int64_t n, int rows) {
    if (n < 1 || n >= (1ll << 31) || rows < 0) return 0;
    return eval_workspace_bytes((int)n, rows);
}

int cddpm_eval_volume(cddpm_handle h, const float* recon_dev, const float* orig_dev, const float* seg_dev, const float* mask_dev,
                      const float* diff_dev, int R, int D1, int D2, int flags, double threshold, void* ws_dev, size_t ws_bytes,
                      double* record_dev, float* row_score_dev, int32_t* row_label_dev, int32_t* row_counts_dev,
                      uint8_t* pred_dev, void* stream) {
    if (!h) return -1;
    if (!recon_dev || !orig_dev || !seg_dev || !mask_dev || !diff_dev || !ws_dev || !record_dev || !row_score_dev ||
        !row_label_dev || !row_counts_dev)
        return fail(h, "cddpm_eval_volume: NULL argument");
    if (R < 1 || D1 < 1 || D2 < 1 || (long long)R * D1 * D2 >= (1ll << 31)) return fail(h, "cddpm_eval_volume: bad R/D1/D2");
    if (flags & ~(CDDPM_EVAL_VOXEL_METRICS | CDDPM_EVAL_COMPONENT_FILTER | CDDPM_EVAL_ROW_CURVE | CDDPM_EVAL_THRESHOLD_OVERRIDE))
        return fail(h, "cddpm_eval_volume: unknown flags 0x%x", flags);
    const size_t need = eval_workspace_bytes(R * D1 * D2, R);
    if (ws_bytes < need) return fail(h, "cddpm_eval_volume: workspace of %zu bytes, need %zu", ws_bytes, need);
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, launch_eval_volume(recon_dev, orig_dev, seg_dev, mask_dev, diff_dev, R, D1, D2, flags, threshold, ws_dev,
                                   ws_bytes, record_dev, row_score_dev, row_label_dev, row_counts_dev, pred_dev,
                                   (hipStream_t)stream));
    return 0;
}

int cddpm_eval_set(cddpm_handle h, const float* x_dev, const int8_t* y_dev, int64_t n, int healthy, void* ws_dev,
                   size_t ws_bytes, double* out_dev, void* stream) {
    if (!h) return -1;
    if (!x_dev || !y_dev || !ws_dev || !out_dev) return fail(h, "cddpm_eval_set: NULL argument");
    if (n < 1 || n >= (1ll << 31)) return fail(h, "cddpm_eval_set: n = %lld outside [1, 2^31)", (long long)n);
    const size_t need = eval_workspace_bytes((int)n, 0);
    if (ws_bytes < need) return fail(h, "cddpm_eval_set: workspace of %zu bytes, need %zu", ws_bytes, need);
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, launch_eval_set(x_dev, y_dev, (int)n, healthy ? 1 : 0, ws_dev, ws_bytes, out_dev, (hipStream_t)stream));
    return 0;
}

int cddpm_q_sample(cddpm_handle h, const float* x01_dev, const float* noise_dev, const int32_t* t_dev, int t_uniform,
                   const float* sqrt_ac_host, const float* sqrt_1mac_host, int T, float* out_dev, int B, int H, int W,
                   void* stream) {
    if (!h) return -1;
    if (T != h->d.timesteps) return fail(h, "T mismatch");
    if (B < 1 || B > h->d.max_batch || (H * W) % 4) return fail(h, "bad B/H/W");
    if (!x01_dev || !noise_dev || !out_dev || !sqrt_ac_host || !sqrt_1mac_host) return fail(h, "cddpm_q_sample: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipMemcpyAsync(h->qs_sa, sqrt_ac_host, (size_t)T * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHECK(h, hipMemcpyAsync(h->qs_s1, sqrt_1mac_host, (size_t)T * sizeof(float), hipMemcpyHostToDevice, s));
    if (t_dev) launch_copy_clamp_int(h->d_t, t_dev, B, 0, T - 1, s);
    else {
        if (t_uniform < 0 || t_uniform >= T) return fail(h, "t=%d outside [0, %d)", t_uniform, T);
        launch_fill_int(h->d_t, B, t_uniform, s);
    }
    launch_q_sample(x01_dev, noise_dev, h->d_t, h->qs_sa, h->qs_s1, out_dev, B, H * W, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_set_accumulation_switch(cddpm_handle h, int t_switch) {
    if (!h) return -1;
    if (t_switch < 0) return fail(h, "cddpm_set_accumulation_switch: t_switch must be >= 0 (>= timesteps: three-level accumulation on every step)");
    h->nb2_tmin = t_switch;
    return 0;
}

int cddpm_set_clip_denoised(cddpm_handle h, int on) {
    if (!h) return -1;
    h->gen++;                            // a captured step graph has the flag baked in
    h->clip_denoised = on ? 1 : 0;
    return 0;
}

int cddpm_get_conv_family(cddpm_handle h) { return h ? h->family : -1; }

int cddpm_set_conv_family(cddpm_handle h, int family) {
    if (!h) return -1;
    if (family < 0 || family > 2) return fail(h, "cddpm_set_conv_family: unknown family %d (2 = h3, 1 = x6, 0 = f32)", family);
    if (family == h->family) return 0;
    HIPCHECK(h, hipSetDevice(h->device));
    if (h->weights_loaded) {
        // the packed images are in the previous family's format: free everything cddpm_load_weights uploaded (work in flight
        // may still read it) and ask for the weights again
        HIPCHECK(h, hipDeviceSynchronize());
        drop_step_graph(h);
        for (size_t i = h->weight_allocs_begin; i < h->allocs.size(); ++i) (void)hipFree(h->allocs[i]);
        h->allocs.resize(h->weight_allocs_begin);
        for (ResW& r : h->res) { r.gn1 = r.gn2 = NormW(); r.conv1 = r.conv2 = r.skip = ConvW(); r.conv1_up2 = nullptr; r.bias2 = nullptr; }
        for (AttnW& a : h->attn) { a.norm = NormW(); a.qkv = a.proj = ConvW(); }
        h->weights_loaded = false;
        h->schedule_set = false;         // the embedding tables are rebuilt from the reloaded weights
        h->cond_B = -1;
        h->weights_dropped = true;
    }
    h->gen++;                            // a captured step graph has the family's kernels baked in
    h->family = family;
    return 0;
}

int cddpm_slice_status(cddpm_handle h, const float* x_dev, int B, int H, int W, int* status_dev, void* stream) {
    if (!h) return -1;
    if (!x_dev || !status_dev) return fail(h, "cddpm_slice_status: NULL argument");
    if (B < 1 || H < 1 || W < 1 || (long long)H * W >= (1ll << 31) || ((long long)H * W) % 4)
        return fail(h, "cddpm_slice_status: B=%d H=%d W=%d unsupported (H * W must be a multiple of 4)", B, H, W);
    if (reinterpret_cast<uintptr_t>(x_dev) % 16) return fail(h, "cddpm_slice_status: x_dev must be 16-byte aligned");
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_OTHER, 0.0, 4.0 * B * (double)H * W, (hipStream_t)stream);
    launch_slice_status(x_dev, B, H * W, status_dev, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_set_profiling(cddpm_handle h, int on) {
    if (!h) return -1;
    h->profiling = on != 0;
    h->prof_last = nullptr;
    return 0;
}

int cddpm_get_profile(cddpm_handle h, int ncls, double* ms, double* flops, double* bytes, int64_t* launches) {
    if (!h) return -1;
    if (ncls != PC_COUNT) return fail(h, "cddpm_get_profile: ncls must be %d", (int)PC_COUNT);
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipDeviceSynchronize());
    for (int i = 0; i < PC_COUNT; ++i) { ms[i] = 0; flops[i] = 0; bytes[i] = 0; launches[i] = 0; }
    hipEvent_t shared = nullptr;
    for (auto& r : h->prof) {
        float t = 0.f;
        HIPCHECK(h, hipEventElapsedTime(&t, r.a, r.b));
        ms[r.cls] += t; flops[r.cls] += r.flops; bytes[r.cls] += r.bytes; launches[r.cls] += 1;
        if (r.a != shared) h->ev_pool.push_back(r.a);      // (a shared begin event is the previous record's end event)
        h->ev_pool.push_back(r.b);
        shared = r.b;
    }
    h->prof.clear();
    h->prof_last = nullptr;
    return 0;
}

int cddpm_op_set_scratch(cddpm_handle h, size_t bytes) {
    if (!h) return -1;
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipDeviceSynchronize());
    if (h->arena) { (void)hipFree(h->arena); h->arena = nullptr; h->arena_bytes = 0; }
    if (bytes) { HIPCHECK(h, hipMalloc(&h->arena, bytes)); h->arena_bytes = bytes; }
    return 0;
}

static int need_zero_bias(cddpm_ctx* h) {
    if (h->zero_bias) return 0;
    HIPCHECK(h, hipMalloc((void**)&h->zero_bias, 4096 * sizeof(float)));
    HIPCHECK(h, hipMemset(h->zero_bias, 0, 4096 * sizeof(float)));
    return 0;
}

int cddpm_op_absmax(cddpm_handle h, const float* x_dev, int64_t n, float* out_dev, void* stream) {
    if (!h) return -1;
    if (!x_dev || !out_dev || n < 1) return fail(h, "cddpm_op_absmax: bad arguments");
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_OPT, 0.0, 0.0, (hipStream_t)stream);
    launch_absmax(x_dev, n, out_dev, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_pack_conv(cddpm_handle h, const float* w_dev, int Cout, int Cin, int ksize, int mode, int scale_exp, void* packed_dev,
                       void* stream) {
    if (!h) return -1;
    if (h->family != 2) return fail(h, "cddpm_op_pack_conv: the device packer serves the default convolution family (CDDPM_CONV=h3) only");
    // O / I: output / input channels of the PACKED operator (mode 1 swaps the roles of the forward tensor's dimensions)
    const int O = mode == 1 ? Cin : Cout, I = mode == 1 ? Cout : Cin;
    if (!w_dev || !packed_dev || (ksize != 1 && ksize != 3) || mode < 0 || mode > 2 || (mode == 2 && ksize != 3) || O <= 0 || I <= 0 ||
        O % 128 || I % 32 || scale_exp < 0 || scale_exp > 24)
        return fail(h, "cddpm_op_pack_conv: unsupported arguments (Cout %d, Cin %d, k %d, mode %d, exponent %d)", Cout, Cin, ksize, mode, scale_exp);
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_OPT, 0.0, 0.0, (hipStream_t)stream);
    launch_pack_conv_split(w_dev, O, I, mode == 2 ? 4 : ksize * ksize, mode, scale_exp, packed_dev, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_pack_conv_batch(cddpm_handle h, const cddpm_pack_job* jobs_dev, int njobs, int64_t max_units, void* stream) {
    if (!h) return -1;
    if (h->family != 2) return fail(h, "cddpm_op_pack_conv_batch: the device packer serves the default convolution family (CDDPM_CONV=h3) only");
    if (!jobs_dev || njobs < 1 || njobs > 65535 || max_units < 1) return fail(h, "cddpm_op_pack_conv_batch: bad arguments");
    static_assert(sizeof(cddpm_pack_job) == sizeof(PackJob), "job table layout");
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_OPT, 0.0, 0.0, (hipStream_t)stream);
    launch_pack_conv_split_batch(reinterpret_cast<const PackJob*>(jobs_dev), njobs, max_units, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_conv_packed(cddpm_handle h, const float* src0, int C0, const float* src1, int C1, const float* coef_dev, int silu, int folded_up,
                         const void* packed_dev, int scale_exp, const float* bias_dev, int Cout, int ksize, const float* res_dev,
                         int res_upsample, const float* skip_dev, int S0, const float* skip1_dev, int S1, const void* skip_packed_dev,
                         float* out_dev, float* stats_dev, int B, int H, int W, void* stream) {
    if (!h) return -1;
    if (h->family != 2) return fail(h, "cddpm_op_conv_packed: default convolution family (CDDPM_CONV=h3) only");
    if ((ksize != 1 && ksize != 3) || C0 <= 0 || C0 % 32 || C1 < 0 || C1 % 32 || Cout <= 0 || Cout % 128 || Cout > 4096 || B < 1 || H < 1 || W < 1 ||
        (folded_up && (ksize != 3 || C1 || H % 2 || W % 2)) || (skip_dev && (S0 <= 0 || S0 % 32 || !skip_packed_dev || ksize != 3 || S1 < 0 || S1 % 32 || (S1 > 0 && !skip1_dev))) ||
        (C1 && !src1) || scale_exp < 0 || scale_exp > 24)
        return fail(h, "cddpm_op_conv_packed: unsupported shape (k %d, C0 %d, C1 %d, Cout %d, S0 %d)", ksize, C0, C1, Cout, S0);
    if (!src0 || !packed_dev || !out_dev) return fail(h, "cddpm_op_conv_packed: NULL argument");
    HIPCHECK(h, hipSetDevice(h->device));
    if (!bias_dev) { if (need_zero_bias(h)) return -1; bias_dev = h->zero_bias; }
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.src1 = src1; a.C1 = C1;
    a.srcH = folded_up ? H / 2 : H; a.srcW = folded_up ? W / 2 : W;
    a.coef = coef_dev; a.silu = silu; a.wpk = static_cast<const float*>(packed_dev); a.bias = bias_dev; a.res = res_dev; a.res_up = res_upsample;
    a.skip0 = skip_dev; a.S0 = skip_dev ? S0 : 0; a.skip_wpk = static_cast<const float*>(skip_packed_dev);
    a.skip1 = (skip_dev && S1 > 0) ? skip1_dev : nullptr; a.S1 = (skip_dev && S1 > 0) ? S1 : 0;      // the skip input as two concatenated tensors
    a.wscale_inv = ldexpf(1.0f, -scale_exp);
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = folded_up ? 4 : ksize * ksize;
    a.stats = stats_dev;       // [B][cddpm_stat_records(H, W, folded_up ? 1 : 0)][Cout][2]: the output's GroupNorm statistics records, for free
    // CDDPM_TRAIN_PRECISION=16: the training operators multiply plain fp16 operands (hi terms only), as the reference trainer's precision 16 does
    a.hi_only = train_precision() == 16 ? 1 : 0;
    // the training operators plan per call, and DO take the 256-cout workgroups wherever the call fills the chip with them: a gradient's
    // accuracy need (2e-5 of float64 autograd; SGD noise far above that) is not the 1000-step chain's, and +9...12 % per layer is
    a.nb2 = (conv_nb2_env() >= 1 && conv_nb2_ok(a.Cout, conv_workgroups_of_call(a), 1, h->family)) ? 1 : 0;
    Prof prof_(h, a.taps == 1 ? PC_CONV1 : PC_CONV3, conv_flops(a), conv_bytes(a), (hipStream_t)stream);
    launch_conv(a, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_gn_coef_rec(cddpm_handle h, const float* rec0_dev, int n0, int C0, const float* rec1_dev, int n1, int C1, const float* gamma_host,
                         const float* beta_host, const float* film_dev, float* coef_dev, int B, int HW, void* stream) {
    if (!h) return -1;
    const int C = C0 + C1;
    if (C0 % 4 || C1 % 4 || C % 32 || C > MAX_CONCAT_CHANNELS || C0 > 1024 || C1 > 1024 || C0 <= 0 || n0 < 1 || (C1 > 0 && (n1 < 1 || !rec1_dev)))
        return fail(h, "cddpm_op_gn_coef_rec: unsupported channels / record counts");
    if (!rec0_dev || !gamma_host || !beta_host || !coef_dev) return fail(h, "cddpm_op_gn_coef_rec: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_GN, 0.0, 0.0, (hipStream_t)stream);
    OpScratch sc(h, s);
    const float* g = sc.param(gamma_host, C);
    const float* bt = sc.param(beta_host, C);
    SCRATCH_CHECK(sc)
    launch_gn_finalize(rec0_dev, C0, n0, C1 ? rec1_dev : nullptr, C1, C1 ? n1 : 0, B, HW, g, bt, nullptr, nullptr, 0, 0, nullptr, film_dev, coef_dev, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

// ---- standalone ops for kernel tests ---------------------------------------------------------------
int cddpm_op_conv(cddpm_handle h, const float* src0, int C0, const float* src1, int C1, const float* coef_dev, int silu,
                  int upsample, const float* w_host, const float* bias_host, int Cout, int ksize, const float* res_dev,
                  int res_upsample, float* out_dev, int B, int H, int W, void* stream) {
    if (!h) return -1;
    const int Cin = C0 + C1, taps = ksize * ksize;
    if ((ksize != 1 && ksize != 3) || C0 % 32 || C1 % 32 || Cin <= 0 || Cout % 128 || Cout <= 0)
        return fail(h, "cddpm_op_conv: unsupported shape (ksize %d, C0 %d, C1 %d, Cout %d)", ksize, C0, C1, Cout);
    if (upsample && (H % 2 || W % 2)) return fail(h, "upsample needs even H, W");
    const bool folded = (upsample == 2);      // upsample: 1 = gather form, 2 = folded 2x2-tap form (what the UNet uses)
    if (folded && (ksize != 3 || C1 != 0)) return fail(h, "folded upsample needs a 3x3 kernel and a single source");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    const int fam = h->family;
    std::vector<float> pk(folded ? 4 * packed_conv_floats(Cout, Cin, 4, fam) : packed_conv_floats(Cout, Cin, taps, fam));
    int wexp = 0;
    if (folded) wexp = pack_conv_weights_up2(w_host, Cout, Cin, pk.data(), fam);
    else { wexp = conv_weight_exp(w_host, (size_t)Cout * Cin * taps, fam); pack_conv_weights(w_host, Cout, Cin, taps, pk.data(), wexp, fam); }
    float *dw = nullptr, *db = nullptr;
    HIPCHECK(h, hipMalloc((void**)&dw, pk.size() * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&db, (size_t)Cout * sizeof(float)));
    HIPCHECK(h, hipMemcpy(dw, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(db, bias_host, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.src1 = src1; a.C1 = C1;
    a.srcH = upsample ? H / 2 : H; a.srcW = upsample ? W / 2 : W; a.upsample = folded ? 0 : upsample;
    a.coef = coef_dev; a.silu = silu; a.wpk = dw; a.bias = db; a.res = res_dev; a.res_up = res_upsample;
    a.wscale_inv = ldexpf(1.0f, -wexp);
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = folded ? 4 : taps;
    a.nb2 = (conv_nb2_env() == 2 && conv_nb2_ok(a.Cout, conv_workgroups_of_call(a), 1, h->family)) ? 1 : 0;
    launch_conv(a, s);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipStreamSynchronize(s));
    (void)hipFree(dw);
    (void)hipFree(db);
    return 0;
}

int cddpm_op_conv_skip(cddpm_handle h, const float* src0, int C0, const float* coef_dev, int silu, const float* w_host,
                       const float* bias_host, int Cout, const float* skip_dev, int S0, const float* wskip_host,
                       float* out_dev, int B, int H, int W, void* stream) {
    if (!h) return -1;
    if (C0 % 32 || C0 <= 0 || S0 % 32 || S0 <= 0 || Cout % 128 || Cout <= 0)
        return fail(h, "cddpm_op_conv_skip: unsupported shape (C0 %d, S0 %d, Cout %d)", C0, S0, Cout);
    if (!src0 || !skip_dev || !w_host || !wskip_host || !bias_host || !out_dev) return fail(h, "cddpm_op_conv_skip: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    // one pre-scale exponent for both tensors, as cddpm_load_weights chooses it
    const int fam = h->family;
    const int wexp = std::min(conv_weight_exp(w_host, (size_t)Cout * C0 * 9, fam), conv_weight_exp(wskip_host, (size_t)Cout * S0, fam));
    std::vector<float> pk(packed_conv_floats(Cout, C0, 9, fam)), pks(packed_conv_floats(Cout, S0, 1, fam));
    pack_conv_weights(w_host, Cout, C0, 9, pk.data(), wexp, fam);
    pack_conv_weights(wskip_host, Cout, S0, 1, pks.data(), wexp, fam);
    float *dw = nullptr, *dws = nullptr, *db = nullptr;
    HIPCHECK(h, hipMalloc((void**)&dw, pk.size() * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&dws, pks.size() * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&db, (size_t)Cout * sizeof(float)));
    HIPCHECK(h, hipMemcpy(dw, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(dws, pks.data(), pks.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(db, bias_host, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.srcH = H; a.srcW = W; a.coef = coef_dev; a.silu = silu; a.wpk = dw; a.bias = db;
    a.skip0 = skip_dev; a.S0 = S0; a.skip_wpk = dws;
    a.wscale_inv = ldexpf(1.0f, -wexp);
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = 9;
    a.nb2 = (conv_nb2_env() == 2 && conv_nb2_ok(a.Cout, conv_workgroups_of_call(a), 1, h->family)) ? 1 : 0;
    launch_conv(a, s);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipStreamSynchronize(s));
    (void)hipFree(dw); (void)hipFree(dws); (void)hipFree(db);
    return 0;
}

int cddpm_op_conv_gn(cddpm_handle h, const float* src0, int C0, const float* w_host, const float* bias_host, int Cout,
                     const float* gamma_host, const float* beta_host, float* out_dev, float* coef_dev, int B, int H, int W,
                     void* stream) {
    if (!h) return -1;
    if (C0 % 32 || C0 <= 0 || Cout % 128 || Cout <= 0 || Cout > 1024) return fail(h, "cddpm_op_conv_gn: unsupported shape");
    if (!src0 || !w_host || !bias_host || !gamma_host || !beta_host || !out_dev || !coef_dev) return fail(h, "cddpm_op_conv_gn: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    const int wexp = conv_weight_exp(w_host, (size_t)Cout * C0 * 9, h->family);
    std::vector<float> pk(packed_conv_floats(Cout, C0, 9, h->family));
    pack_conv_weights(w_host, Cout, C0, 9, pk.data(), wexp, h->family);
    const int nrec = conv_stat_records(H, W);
    float *dw = nullptr, *db = nullptr, *rec = nullptr, *g = nullptr, *bt = nullptr;
    HIPCHECK(h, hipMalloc((void**)&dw, pk.size() * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&db, (size_t)Cout * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&g, (size_t)Cout * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&bt, (size_t)Cout * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&rec, (size_t)B * nrec * Cout * CDDPM_STAT_FLOATS * sizeof(float)));
    HIPCHECK(h, hipMemcpy(dw, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(db, bias_host, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(g, gamma_host, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(bt, beta_host, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.srcH = H; a.srcW = W; a.wpk = dw; a.bias = db; a.stats = rec;
    a.wscale_inv = ldexpf(1.0f, -wexp);
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = 9;
    a.nb2 = (conv_nb2_env() == 2 && conv_nb2_ok(a.Cout, conv_workgroups_of_call(a), 1, h->family)) ? 1 : 0;
    launch_conv(a, s);
    launch_gn_finalize(rec, Cout, nrec, nullptr, 0, 0, B, H * W, g, bt, nullptr, nullptr, 0, 0, nullptr, nullptr, coef_dev, s);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipStreamSynchronize(s));
    for (void* p : {(void*)dw, (void*)db, (void*)g, (void*)bt, (void*)rec}) (void)hipFree(p);
    return 0;
}

int cddpm_op_gn_coef(cddpm_handle h, const float* src0, int C0, const float* src1, int C1, const float* gamma_host,
                     const float* beta_host, const float* film_dev, float* coef_dev, int B, int HW, void* stream) {
    if (!h) return -1;
    const int C = C0 + C1;
    if (C0 % 4 || C1 % 4 || C % 32 || C > MAX_CONCAT_CHANNELS || C0 > 1024 || C1 > 1024)
        return fail(h, "cddpm_op_gn_coef: unsupported channels (each source <= 1024, together <= %d)", MAX_CONCAT_CHANNELS);
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_GN, 0.0, 0.0, (hipStream_t)stream);
    const int ns = gn_nsplit(B, HW);
    OpScratch sc(h, s);
    float* rec0 = sc.n<float>((size_t)B * ns * C0 * 2);
    float* rec1 = src1 ? sc.n<float>((size_t)B * ns * C1 * 2) : nullptr;
    const float* g = sc.param(gamma_host, C);
    const float* bt = sc.param(beta_host, C);
    SCRATCH_CHECK(sc)
    launch_gn_partial(src0, C0, B, HW, ns, rec0, s);
    if (src1) launch_gn_partial(src1, C1, B, HW, ns, rec1, s);
    launch_gn_finalize(rec0, C0, ns, rec1, C1, src1 ? ns : 0, B, HW, g, bt, nullptr, nullptr, 0, 0, nullptr, film_dev,
                       coef_dev, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_conv_dgrad(cddpm_handle h, const float* dy_dev, int Cout, const float* w_host, int Cin, int ksize, float* dx_dev,
                        int B, int H, int W, void* stream) {
    if (!h) return -1;
    const int taps = ksize * ksize;
    if ((ksize != 1 && ksize != 3) || Cin <= 0 || Cin % 128 || Cout <= 0 || Cout % 32)
        return fail(h, "cddpm_op_conv_dgrad: unsupported shape (ksize %d, Cin %d must be a multiple of 128, Cout %d of 32)", ksize, Cin, Cout);
    if (!dy_dev || !w_host || !dx_dev) return fail(h, "cddpm_op_conv_dgrad: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    // wt[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx]: the gradient of a cross-correlation is a cross-correlation with this tensor
    std::vector<float> wt((size_t)Cin * Cout * taps);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < taps; ++t)
                wt[((size_t)ci * Cout + co) * taps + (taps - 1 - t)] = w_host[((size_t)co * Cin + ci) * taps + t];
    const int wexp = conv_weight_exp(wt.data(), wt.size(), h->family);
    std::vector<float> pk(packed_conv_floats(Cin, Cout, taps, h->family));
    pack_conv_weights(wt.data(), Cin, Cout, taps, pk.data(), wexp, h->family);
    std::vector<float> zb(Cin, 0.f);
    float *dw = nullptr, *db = nullptr;
    HIPCHECK(h, hipMalloc((void**)&dw, pk.size() * sizeof(float)));
    HIPCHECK(h, hipMalloc((void**)&db, (size_t)Cin * sizeof(float)));
    HIPCHECK(h, hipMemcpy(dw, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(db, zb.data(), (size_t)Cin * sizeof(float), hipMemcpyHostToDevice));
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = dy_dev; a.C0 = Cout; a.srcH = H; a.srcW = W; a.wpk = dw; a.bias = db;
    a.wscale_inv = ldexpf(1.0f, -wexp);
    a.out = dx_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cin; a.taps = taps;
    a.nb2 = (conv_nb2_env() == 2 && conv_nb2_ok(a.Cout, conv_workgroups_of_call(a), 1, h->family)) ? 1 : 0;
    launch_conv(a, s);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipStreamSynchronize(s));
    (void)hipFree(dw); (void)hipFree(db);
    return 0;
}

int cddpm_op_bias_grad(cddpm_handle h, const float* dy_dev, int64_t npix, int C, float* db_dev, void* stream) {
    if (!h) return -1;
    if (!dy_dev || !db_dev || npix < 1 || C % 4 || C > 1024) return fail(h, "cddpm_op_bias_grad: bad arguments");
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_OTHER, 0.0, 0.0, (hipStream_t)stream);
    OpScratch sc(h, (hipStream_t)stream);
    double* part = sc.n<double>((size_t)512 * C);
    SCRATCH_CHECK(sc)
    launch_bias_grad(dy_dev, npix, C, db_dev, part, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_conv_wgrad(cddpm_handle h, const float* x0_dev, int C0, const float* x1_dev, int C1, const float* coef_dev, int silu,
                        int upsample, const float* dy_dev, int Cout, int ksize, float* dw_dev, float* db_dev, int B, int H, int W,
                        void* stream) {
    if (!h) return -1;
    const int Cin = C0 + C1, taps = ksize * ksize;
    if ((ksize != 1 && ksize != 3) || C0 <= 0 || C1 < 0 || Cin % 32 || (C1 > 0 && C0 % 32) || Cout <= 0 || Cout % 64 || H < 1 ||
        W < 1 || B < 1 || (C1 > 0 && !x1_dev) || (upsample && (C1 > 0 || (W & 1) || (H & 1))))
        return fail(h, "cddpm_op_conv_wgrad: unsupported shape (k %d, C0 %d, C1 %d, Cout %d, H %d)", ksize, C0, C1, Cout, H);
    if (!x0_dev || !dy_dev || !dw_dev) return fail(h, "cddpm_op_conv_wgrad: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    const int P = conv_wgrad_parts(B, H, W, Cin, Cout, taps);
    OpScratch sc(h, s);
    float* part = sc.n<float>((size_t)P * Cout * Cin * taps);
    const size_t iu = conv_wgrad_image_units(B, H, W, Cin, Cout, taps);
    void* images = iu ? sc.get(iu * 16) : nullptr;
    SCRATCH_CHECK(sc)
    Prof prof_(h, PC_WGRAD, 2.0 * B * H * W * (double)Cout * Cin * taps, 4.0 * B * (double)H * W * (Cin + Cout), s);
    launch_conv_wgrad(x0_dev, C0, x1_dev, C1, coef_dev, silu, upsample ? 1 : 0, dy_dev, B, H, W, Cout, taps, part, P, images, dw_dev, db_dev, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_attention_backward(cddpm_handle h, const float* qkv_dev, const float* da_dev, float* dqkv_dev, int B, int N, int C,
                                void* stream) {
    if (!h) return -1;
    if (C <= 0 || C % 64 || N < 1 || B < 1) return fail(h, "cddpm_op_attention_backward: C must be a multiple of 64");
    if (!qkv_dev || !da_dev || !dqkv_dev) return fail(h, "cddpm_op_attention_backward: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_ATTN, 0.0, 0.0, (hipStream_t)stream);
    OpScratch sc(h, s);
    float* stats = sc.n<float>((size_t)B * (C / 64) * N * 2);
    SCRATCH_CHECK(sc)
    launch_attention_backward_flash(qkv_dev, da_dev, dqkv_dev, stats, B, N, C, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_op_linear_backward(cddpm_handle h, const float* x_dev, const float* w_dev, const float* dy_dev, int M, int N, int K,
                             int silu_in, float* dw_dev, float* db_dev, float* dx_dev, void* stream) {
    if (!h) return -1;
    if (M < 1 || N < 1 || K < 1 || !x_dev || !w_dev || !dy_dev || !dw_dev) return fail(h, "cddpm_op_linear_backward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_OTHER, 0.0, 0.0, (hipStream_t)stream);
    OpScratch sc(h, s);
    const size_t nscr = linear_backward_scratch_floats(M, N, K, silu_in);
    float* a = nscr ? sc.n<float>(nscr) : nullptr;
    SCRATCH_CHECK(sc)
    launch_linear_backward(x_dev, w_dev, dy_dev, M, N, K, silu_in, a, dw_dev, db_dev, dx_dev, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

#define OP_PROLOGUE(cond, msg)                                   \
    if (!h) return -1;                                            \
    if (!(cond)) return fail(h, msg);                             \
    hipStream_t s = (hipStream_t)stream;                          \
    HIPCHECK(h, hipSetDevice(h->device));                         \
    Prof prof_(h, PC_OTHER, 0.0, 0.0, s);
#define OP_CLASS(c, fl) { prof_.r.cls = (c); prof_.r.flops = (fl); }
#define OP_EPILOGUE()                                             \
    HIPCHECK(h, hipGetLastError());                               \
    return 0;

int cddpm_op_linear(cddpm_handle h, const float* x_dev, const float* w_dev, const float* b_dev, int M, int N, int K, int silu_in,
                    float* y_dev, void* stream) {
    OP_PROLOGUE(x_dev && w_dev && y_dev && M > 0 && N > 0 && K > 0, "cddpm_op_linear: bad arguments")
    launch_linear(x_dev, K, w_dev, K, 0, b_dev, y_dev, N, M, N, K, silu_in, s);
    OP_EPILOGUE()
}
int cddpm_op_conv_in1(cddpm_handle h, const float* x_dev, const float* w_dev, const float* b_dev, float* out_dev, int B, int H, int W,
                      int C, void* stream) {
    OP_PROLOGUE(x_dev && w_dev && b_dev && out_dev && C % 64 == 0 && C <= 512, "cddpm_op_conv_in1: bad arguments")
    launch_conv_in1(x_dev, w_dev, b_dev, out_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
int cddpm_op_head(cddpm_handle h, const float* x_dev, const float* coef_dev, const float* w9_dev, float bias, const float* bias_dev,
                  float* out_dev, int B, int H, int W, int C, void* stream) {
    OP_PROLOGUE(x_dev && coef_dev && w9_dev && out_dev && C % 32 == 0, "cddpm_op_head: bad arguments")
    OpScratch sc(h, s);
    float* P = sc.n<float>((size_t)B * H * W * 9);
    SCRATCH_CHECK(sc)
    launch_head_dots(x_dev, coef_dev, w9_dev, P, B, H * W, C, s);
    launch_head_gather(P, bias, bias_dev, out_dev, B, H, W, s);
    OP_EPILOGUE()
}
int cddpm_op_pool_act(cddpm_handle h, const float* x_dev, const float* coef_dev, float* hp_dev, float* xp_dev, int B, int H, int W, int C,
                      void* stream) {
    OP_PROLOGUE(x_dev && coef_dev && hp_dev && xp_dev && H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "cddpm_op_pool_act: bad arguments")
    launch_pool_act(x_dev, coef_dev, hp_dev, xp_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
int cddpm_op_unpool2(cddpm_handle h, const float* dyp_dev, float* dx_dev, int B, int H, int W, int C, float scale, int accumulate, void* stream) {
    OP_PROLOGUE(dyp_dev && dx_dev && H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "cddpm_op_unpool2: bad arguments")
    launch_unpool2(dyp_dev, dx_dev, B, H, W, C, scale, accumulate, s);
    OP_EPILOGUE()
}
int cddpm_op_sumpool2(cddpm_handle h, const float* dy_dev, float* dxp_dev, int B, int H, int W, int C, int accumulate, void* stream) {
    OP_PROLOGUE(dy_dev && dxp_dev && H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "cddpm_op_sumpool2: bad arguments")
    launch_sumpool2(dy_dev, dxp_dev, B, H, W, C, accumulate, s);
    OP_EPILOGUE()
}
int cddpm_op_add_inplace(cddpm_handle h, float* a_dev, const float* b_dev, int64_t n, void* stream) {
    OP_PROLOGUE(a_dev && b_dev && n > 0 && n % 4 == 0, "cddpm_op_add_inplace: bad arguments")
    launch_add_inplace(a_dev, b_dev, n, s);
    OP_EPILOGUE()
}
int cddpm_op_chan_image_corr(cddpm_handle h, const float* t_dev, const float* coef_dev, int silu, const float* s_dev, int sign, float* dw_dev,
                             int B, int H, int W, int C, void* stream) {
    OP_PROLOGUE(t_dev && s_dev && dw_dev && C % 64 == 0 && (sign == 1 || sign == -1), "cddpm_op_chan_image_corr: bad arguments")
    OpScratch sc(h, s);
    double* part = sc.n<double>((size_t)256 * C * 9);
    SCRATCH_CHECK(sc)
    launch_chan_image_corr(t_dev, coef_dev, silu, s_dev, sign, B, H, W, C, part, dw_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_head_dgrad(cddpm_handle h, const float* dout_dev, const float* w9_dev, float* dact_dev, int B, int H, int W, int C, void* stream) {
    OP_PROLOGUE(dout_dev && w9_dev && dact_dev && C % 4 == 0, "cddpm_op_head_dgrad: bad arguments")
    launch_head_dgrad(dout_dev, w9_dev, dact_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
int cddpm_op_loss(cddpm_handle h, const float* out_dev, const float* target_dev, const float* w_b_dev, int l2, int B, int HW, float grad_scale,
                  float* dout_dev, float* loss_b_dev, void* stream) {
    OP_PROLOGUE(out_dev && target_dev && dout_dev && loss_b_dev && B > 0 && HW > 0, "cddpm_op_loss: bad arguments")
    launch_loss(out_dev, target_dev, w_b_dev, l2, B, HW, grad_scale, nullptr, dout_dev, loss_b_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_loss_scaled(cddpm_handle h, const float* out_dev, const float* target_dev, const float* w_b_dev, int l2, int B, int HW,
                         const int32_t* scaler_dev, float* dout_dev, float* loss_b_dev, void* stream) {
    OP_PROLOGUE(out_dev && target_dev && scaler_dev && dout_dev && loss_b_dev && B > 0 && HW > 0, "cddpm_op_loss_scaled: bad arguments")
    launch_loss(out_dev, target_dev, w_b_dev, l2, B, HW, 0.0f, scaler_dev, dout_dev, loss_b_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_adam(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2,
                  float eps, int step, float grad_unscale, void* stream) {
    OP_PROLOGUE(p_dev && g_dev && m_dev && v_dev && n > 0 && step >= 1, "cddpm_op_adam: bad arguments")
    OP_CLASS(PC_OPT, 0.0)
    launch_adam(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, step, grad_unscale, s);
    OP_EPILOGUE()
}
int cddpm_set_train_precision(int bits) {
    if (bits != 16 && bits != 32) return -1;
    return set_train_precision(bits);
}
int cddpm_get_train_precision(void) { return train_precision(); }
int cddpm_op_grad_check(cddpm_handle h, const float* g_dev, int64_t n, int32_t* ctrl_dev, void* stream) {
    OP_PROLOGUE(g_dev && ctrl_dev && n > 0 && ((uintptr_t)g_dev & 15) == 0, "cddpm_op_grad_check: bad arguments (g_dev 16-byte aligned)")
    OP_CLASS(PC_OPT, 0.0)
    launch_grad_check(g_dev, n, ctrl_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_guard_commit(cddpm_handle h, int32_t* ctrl_dev, float beta1, float beta2, void* stream) {
    OP_PROLOGUE(ctrl_dev != nullptr, "cddpm_op_guard_commit: bad arguments")
    OP_CLASS(PC_OPT, 0.0)
    launch_guard_commit(ctrl_dev, beta1, beta2, s);
    OP_EPILOGUE()
}
int cddpm_op_adam_guarded(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1,
                          float beta2, float eps, float grad_unscale, const int32_t* ctrl_dev, void* stream) {
    OP_PROLOGUE(p_dev && g_dev && m_dev && v_dev && ctrl_dev && n > 0, "cddpm_op_adam_guarded: bad arguments")
    OP_CLASS(PC_OPT, 0.0)
    launch_adam_guarded(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, grad_unscale, ctrl_dev, nullptr, s);
    OP_EPILOGUE()
}
int cddpm_op_adam_scaled(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1,
                         float beta2, float eps, float extra_unscale, const int32_t* ctrl_dev, const int32_t* scaler_dev, void* stream) {
    OP_PROLOGUE(p_dev && g_dev && m_dev && v_dev && ctrl_dev && scaler_dev && n > 0, "cddpm_op_adam_scaled: bad arguments")
    OP_CLASS(PC_OPT, 0.0)
    launch_adam_guarded(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, extra_unscale, ctrl_dev, scaler_dev, s);
    OP_EPILOGUE()
}
static bool power_of_two(float x) {
    int e;
    return std::isfinite(x) && x > 0.0f && std::frexp(x, &e) == 0.5f;
}
int cddpm_op_scaler_update(cddpm_handle h, const int32_t* ctrl_dev, int32_t* scaler_dev, float growth, float backoff, int interval,
                           void* stream) {
    OP_PROLOGUE(ctrl_dev && scaler_dev && power_of_two(growth) && growth > 1.0f && power_of_two(backoff) && backoff < 1.0f && interval >= 1,
                "cddpm_op_scaler_update: bad arguments (growth > 1 and backoff < 1 powers of two, interval >= 1)")
    OP_CLASS(PC_OPT, 0.0)
    launch_scaler_update(ctrl_dev, scaler_dev, growth, backoff, interval, s);
    OP_EPILOGUE()
}

// ---- training-mode operators of the context encoder (encoder_train.hip): NHWC fp32 device tensors ---------------------------------------
int cddpm_op_enc_pack_w(cddpm_handle h, const float* w_dev, int Cout, int Cin, int K, float* wf_dev, float* wd_dev, void* stream) {
    OP_PROLOGUE(w_dev && wf_dev && Cout > 0 && Cin > 0 && (K == 1 || K == 3), "cddpm_op_enc_pack_w: bad arguments")
    OP_CLASS(PC_ENC, 0.0)
    launch_enc_pack_w(w_dev, Cout, Cin, K * K, wf_dev, wd_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_conv(cddpm_handle h, const float* src_dev, const float* w_img_dev, float* dst_dev, int B, int H, int W, int Cin, int Cout, int K,
                      int stride, int transposed, void* stream) {
    OP_PROLOGUE(src_dev && w_img_dev && dst_dev && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (K == 1 || K == 3) && (stride == 1 || stride == 2) &&
                    (transposed ? (Cout % 16 == 0 && Cin % 64 == 0) : (Cin % 16 == 0 && Cout % 64 == 0)),
                "cddpm_op_enc_conv: unsupported shape (contraction channels a multiple of 16, produced channels of 64; K 1|3, stride 1|2)")
    OP_CLASS(PC_ENC, 0.0)
    const int Z = enc_conv_split(B, H, W, Cin, Cout, K, stride, transposed);
    OpScratch sc(h, s);
    float* part = nullptr;
    if (Z > 1) {
        const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
        part = sc.n<float>((size_t)Z * B * (transposed ? (size_t)H * W * Cin : (size_t)Ho * Wo * Cout));
        SCRATCH_CHECK(sc)
    }
    launch_enc_conv(src_dev, w_img_dev, dst_dev, B, H, W, Cin, Cout, K, stride, transposed, part, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_conv_wgrad(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, int Cin, int Cout, int K,
                            int stride, void* stream) {
    OP_PROLOGUE(x_dev && dz_dev && dw_dev && B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0 && (K == 1 || K == 3) &&
                    (stride == 1 || stride == 2), "cddpm_op_enc_conv_wgrad: unsupported shape")
    OP_CLASS(PC_ENC, 0.0)
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int P = enc_wgrad_parts(B, Ho, Wo, Cin, Cout, K);
    OpScratch sc(h, s);
    float* part = sc.n<float>((size_t)P * K * K * Cin * Cout);
    SCRATCH_CHECK(sc)
    launch_enc_wgrad(x_dev, dz_dev, part, P, dw_dev, B, H, W, Cin, Cout, K, stride, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_stem(cddpm_handle h, const float* x_dev, const float* w_dev, float* z_dev, int B, int H, int W, void* stream) {
    OP_PROLOGUE(x_dev && w_dev && z_dev && B > 0 && H > 0 && W > 0, "cddpm_op_enc_stem: bad arguments")
    OP_CLASS(PC_ENC, 0.0)
    launch_enc_stem_fwd(x_dev, w_dev, z_dev, B, H, W, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_stem_wgrad(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, void* stream) {
    OP_PROLOGUE(x_dev && dz_dev && dw_dev && B > 0 && H > 0 && W > 0, "cddpm_op_enc_stem_wgrad: bad arguments")
    OP_CLASS(PC_ENC, 0.0)
    OpScratch sc(h, s);
    double* part = sc.n<double>((size_t)32 * 49 * 64);
    SCRATCH_CHECK(sc)
    launch_enc_stem_wgrad(x_dev, dz_dev, part, dw_dev, B, H, W, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_bn_forward(cddpm_handle h, const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* sample_scale_dev,
                            const float* res_dev, int relu, float eps, float momentum, float* run_mean_dev, float* run_var_dev, float* mean_rstd_dev,
                            float* y_dev, int64_t N, int HW, int C, void* stream) {
    OP_PROLOGUE(z_dev && gamma_dev && beta_dev && mean_rstd_dev && y_dev && N > 0 && HW > 0 && C > 0 && C % 64 == 0 && (!run_mean_dev == !run_var_dev),
                "cddpm_op_enc_bn_forward: bad arguments (C a multiple of 64)")
    OP_CLASS(PC_ENC, 0.0)
    OpScratch sc(h, s);
    double* part = sc.n<double>((size_t)enc_bn_chunks(N) * 2 * C);
    SCRATCH_CHECK(sc)
    launch_enc_bn_forward(z_dev, gamma_dev, beta_dev, sample_scale_dev, res_dev, relu, eps, momentum, run_mean_dev, run_var_dev, mean_rstd_dev, y_dev,
                          part, N, HW, C, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_bn_backward(cddpm_handle h, const float* z_dev, const float* y_dev, const float* dy_dev, const float* mean_rstd_dev,
                             const float* gamma_dev, const float* sample_scale_dev, int relu, float* dz_dev, float* dres_dev, float* dgamma_dev,
                             float* dbeta_dev, int64_t N, int HW, int C, void* stream) {
    OP_PROLOGUE(z_dev && dy_dev && mean_rstd_dev && gamma_dev && dz_dev && dgamma_dev && dbeta_dev && (!relu || y_dev) && N > 0 && HW > 0 && C > 0 &&
                    C % 64 == 0, "cddpm_op_enc_bn_backward: bad arguments (C a multiple of 64)")
    OP_CLASS(PC_ENC, 0.0)
    OpScratch sc(h, s);
    double* part = sc.n<double>((size_t)enc_bn_chunks(N) * 2 * C);
    float* k = sc.n<float>((size_t)2 * C);
    SCRATCH_CHECK(sc)
    launch_enc_bn_backward(z_dev, y_dev, dy_dev, mean_rstd_dev, gamma_dev, sample_scale_dev, relu, dz_dev, dres_dev, dgamma_dev, dbeta_dev, k, part, N,
                           HW, C, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_maxpool(cddpm_handle h, const float* x_dev, float* y_dev, int B, int H, int W, int C, int backward, const float* dy_dev, float* dx_dev,
                         void* stream) {
    OP_PROLOGUE(x_dev && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (backward ? (dy_dev && dx_dev) : (y_dev != nullptr)),
                "cddpm_op_enc_maxpool: bad arguments")
    OP_CLASS(PC_ENC, 0.0)
    if (backward) launch_enc_maxpool_backward(x_dev, dy_dev, dx_dev, B, H, W, C, s);
    else launch_enc_maxpool(x_dev, y_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_avgpool(cddpm_handle h, const float* x_dev, float* g_dev, int B, int HW, int C, int backward, void* stream) {
    OP_PROLOGUE(x_dev && g_dev && B > 0 && HW > 0 && C > 0, "cddpm_op_enc_avgpool: bad arguments")
    OP_CLASS(PC_ENC, 0.0)
    if (backward) launch_enc_avgpool_backward(x_dev /* dL/dg [B][C] */, g_dev /* dL/dx [B][HW][C] */, B, HW, C, s);
    else launch_enc_avgpool(x_dev, g_dev, B, HW, C, s);
    OP_EPILOGUE()
}

int cddpm_op_gn_silu_backward(cddpm_handle h, const float* x_dev, const float* x1_dev, int C1, const float* da_dev, const float* gamma_host,
                              const float* beta_host, const float* film_dev, int silu, float* dx_dev, float* dx1_dev, float* dgamma_dev,
                              float* dbeta_dev, float* dfilm_dev, const float* rec_dev, int nrec, const float* add_dev, int B, int HW, int C,
                              void* stream) {
    if (!h) return -1;
    if (C % 32 || C <= 0 || C > 1024 || B < 1 || HW < 1 || (rec_dev && nrec < 1) || C1 < 0 || C1 % 4 || C1 >= C ||
        (C1 > 0 && (!x1_dev || !dx1_dev || !rec_dev)))
        return fail(h, "cddpm_op_gn_silu_backward: unsupported shape (C %d, C1 %d; a two-source input needs its statistics records)", C, C1);
    if (!x_dev || !da_dev || !gamma_host || !beta_host || !dx_dev || !dgamma_dev || !dbeta_dev || (film_dev && !dfilm_dev))
        return fail(h, "cddpm_op_gn_silu_backward: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    const int ns = gn_nsplit(B, HW);
    OpScratch sc(h, s);
    float* rec = rec_dev ? nullptr : sc.n<float>((size_t)B * ns * C * 2);
    const float* g = sc.param(gamma_host, C);
    const float* bt = sc.param(beta_host, C);
    float* planes = sc.n<float>((size_t)4 * B * C);
    float* out_bc = sc.n<float>((size_t)4 * B * C);
    double* part = sc.n<double>((size_t)B * ns * C * 2);
    SCRATCH_CHECK(sc)
    Prof prof_(h, PC_GNBWD, 0.0, 12.0 * B * (double)HW * C, s);       // reads x and da, writes dx
    if (!rec_dev) launch_gn_partial(x_dev, C, B, HW, ns, rec, s);      // statistics records of x: given (kept from the forward pass) or swept here
    launch_gn_bwd_planes(rec_dev ? rec_dev : rec, rec_dev ? nrec : ns, g, bt, film_dev, B, C, HW, planes, s);
    launch_gn_silu_backward(x_dev, C1 ? x1_dev : nullptr, C - C1, C1 ? dx1_dev : nullptr, da_dev, planes, g, bt, film_dev, silu, B, C, HW, ns, part,
                            out_bc, dx_dev, dgamma_dev, dbeta_dev, dfilm_dev, add_dev, s);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

int cddpm_stat_records(int H, int W, int kind) {
    if (H < 1 || W < 1) return -1;
    if (kind == 0) return conv_stat_records(H, W);
    if (kind == 1) return conv_stat_records_up2(H, W);
    if (kind == 2) return gn_nsplit(1, H * W);
    return -1;
}

size_t cddpm_packed_conv_bytes(int Cout, int Cin, int taps) {
    if (Cout <= 0 || Cin <= 0 || Cout % 128 || Cin % 32 || (taps != 1 && taps != 9 && taps != 4)) return 0;
    return packed_conv_floats(Cout, Cin, taps, conv_mode()) * sizeof(float);      // handle-less: the process default family
}

int cddpm_pack_conv_weights(const float* w_host, int Cout, int Cin, int taps, void* dst_host, int* scale_exp_out) {
    if (!w_host || !dst_host || cddpm_packed_conv_bytes(Cout, Cin, taps) == 0) return -1;
    const int wexp = conv_weight_exp(w_host, (size_t)Cout * Cin * taps, conv_mode());     // handle-less: the process default family
    pack_conv_weights(w_host, Cout, Cin, taps, static_cast<float*>(dst_host), wexp, conv_mode());
    if (scale_exp_out) *scale_exp_out = wexp;
    return conv_mode();
}

int cddpm_op_attention(cddpm_handle h, const float* qkv_dev, float* out_dev, int B, int N, int C, void* stream) {
    if (!h) return -1;
    if (C % 64 || N < 1) return fail(h, "cddpm_op_attention: C must be a multiple of 64");
    HIPCHECK(h, hipSetDevice(h->device));
    Prof prof_(h, PC_ATTN, 0.0, 0.0, (hipStream_t)stream);
    launch_attention(qkv_dev, out_dev, B, N, C, (hipStream_t)stream);
    HIPCHECK(h, hipGetLastError());
    return 0;
}

}  // extern "C"
