// C ABI of libcddpm_hip.so (declared in include/cddpm.h): handle, weight packing, embedding tables,
// the UNet forward program and the reverse-diffusion loop driver. Host code only; kernels live in
// conv_mfma.hip, norm_kernels.hip, small_kernels.hip and attention.hip. The standalone operators (cddpm_op_*) are in
// cddpm_ops.hip; what both files share is in cddpm_ctx.h.
//
// Data layout in HBM: every activation is NHWC fp32 ([B][H*W][C], 16-B aligned channel quads); the image
// itself has one channel, so the [B,1,H,W] boundary tensors need no conversion. Skip-stack tensors, three
// ping-pong activation buffers, the qkv/attention buffers, GroupNorm partials and coefficient planes, the
// packed weights and the [T][sumE] time-embedding table are allocated once in cddpm_create.
#include "cddpm_ctx.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

using namespace cddpm;

namespace {
thread_local std::string g_create_error;
}

int cddpm::fail(cddpm_ctx* h, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return -1;
}

namespace {

// workgroups of the 128-cout form at the HANDLE's maximum geometry (the quantity both plans are keyed on): the layer's extent
// scaled by maximum / current image size
long long conv_workgroups_at_max(const cddpm_ctx* h, const ConvArgs& a) {
    if (h->cur_H <= 0) return 0;
    const int Hm = (int)((long long)a.H * h->d.max_h / h->cur_H), Wm = (int)((long long)a.W * h->d.max_w / h->cur_W);
    return conv_workgroups(a, h->d.max_batch, Hm, Wm);
}

// Small-batch plan (fp16-split family). A layer launches B * tiles * (Cout / 128) workgroups of 256 pixels x 128 channels; when the
// HANDLE's largest geometry gives fewer than half the chip's 256 CUs a workgroup, the K loop of that layer is cut into S ranges run
// by S workgroups per tile (plane j of `kpart` each) and conv_reduce_kernel adds the planes in the order of j. S is a property of
// the handle (max_batch, max_h, max_w and the layer), never of the call: a slice's bits do not depend on the batch it is in, as long
// as it is computed on handles of the same maximum geometry (sharded runs: the same engine configuration on every rank).
// The arithmetic is ksplit_rule (below, outside this namespace: the host-only query cddpm_conv_ksplit_plan runs it too).
int plan_ksplit(const cddpm_ctx* h, const ConvArgs& a, short* kbound) {
    if (h->cur_H <= 0) return 1;
    return ksplit_rule(h->family, conv_workgroups_at_max(h, a), a.C0 + a.C1, a.S0 + a.S1, a.taps, kbound);
}

}  // namespace

int cddpm::ksplit_rule(int family, long long nwg, int Cin, int Cskip, int taps, short* kbound) {
    if (family != 2) return 1;
    const int nch_main = Cin / 32, nch_skip = Cskip / 32, nch = nch_main + nch_skip;
    const int units = nch_main * taps + nch_skip;           // taps to multiply per tile
    int S = 1;
    while (S < CDDPM_MAX_KSPLIT && nwg * (S * 2) <= 256 && units / (S * 2) >= 9 && S * 2 <= nch) S *= 2;
    if (S == 1) return 1;
    // consecutive chunk ranges of about units / S taps each, none empty
    int c = 0, acc = 0;
    kbound[0] = 0;
    for (int j = 1; j < S; ++j) {
        const int target = (int)((long long)units * j / S);
        while (c < nch - (S - j) && acc + (c < nch_main ? taps : 1) / 2 < target) { acc += (c < nch_main ? taps : 1); ++c; }
        if (c <= kbound[j - 1]) { acc += (c < nch_main ? taps : 1); ++c; }
        kbound[j] = (short)c;
    }
    kbound[S] = (short)nch;
    return S;
}

int cddpm::conv_launch(cddpm_ctx* h, ConvArgs a, hipStream_t s, ConvPlanTaken* took) {
    auto it = h->stat.find(a.out);           // outputs that can feed a GroupNorm get their statistics for free
    StatBuf* sb = (it != h->stat.end()) ? &it->second : nullptr;
    a.stats = sb ? sb->records : nullptr;
    a.hi_only = (h->precision == 16) ? 1 : 0;      // plain fp16 operands on every convolution of a precision-16 handle, split-K included
    short kb[CDDPM_MAX_KSPLIT + 1] = {0};
    const int S = plan_ksplit(h, a, kb);
    if (took) {
        took->S = S; took->nb2 = 0;
        for (int j = 0; j <= CDDPM_MAX_KSPLIT; ++j) took->kbound[j] = kb[j];
    }
    if (S > 1) {
        if ((size_t)S * a.B * a.H * a.W * a.Cout > (size_t)KSPLIT_PLANE_FLOATS)
            return fail(h, "split-K planes of a %dx%dx%d conv output (B=%d, S=%d) exceed the workspace", a.H, a.W, a.Cout, a.B, S);
        const int nrec_r = conv_reduce_stat_records(a.H, a.W);
        if (sb && (size_t)a.B * nrec_r * a.Cout * 2 > sb->capacity)
            return fail(h, "GroupNorm statistics records of a %dx%dx%d conv output do not fit their buffer", a.H, a.W, a.Cout);
        ConvArgs k = a;
        k.out = h->kpart; k.bias = nullptr; k.res = nullptr; k.stats = nullptr; k.ksplit = S;
        for (int j = 0; j <= S; ++j) k.kbound[j] = kb[j];
        {
            Prof p(h, a.taps == 1 ? PC_CONV1 : PC_CONV3, conv_flops(a), conv_bytes(a), s);
            launch_conv(k, s);
            launch_conv_reduce(h->kpart, S, a.bias, a.res, a.res_up, a.out, a.stats, a.B, a.H, a.W, a.Cout, s);
        }
        if (sb) sb->valid_count = nrec_r;
        return 0;
    }
    conv_set_nb2(a, h, NB2_HANDLE_PLAN, conv_workgroups_at_max(h, a));      // the large-batch plan
    if (took) took->nb2 = (a.nb2 && a.taps != 1) ? 1 : 0;      // the 1x1 loop has no 256-cout form (conv_x6.hip::launch_split)
    const int nrec = (a.taps == 4) ? conv_stat_records_up2(a.H, a.W) : conv_stat_records(a.H, a.W);
    if (sb) {
        // a statically sized buffer against a shape-derived count: refuse to launch rather than write past the end
        const size_t need = (size_t)a.B * nrec * a.Cout * 2;
        if (need > sb->capacity)
            return fail(h, "GroupNorm statistics records of a %dx%dx%d conv output (B=%d, %d records) need %zu floats, the buffer holds %zu",
                        a.H, a.W, a.Cout, a.B, nrec, need, sb->capacity);
    }
    {
        Prof p(h, a.taps == 1 ? PC_CONV1 : PC_CONV3, conv_flops(a), conv_bytes(a), s);   // taps 4 = folded upsample + 3x3
        launch_conv(a, s);
    }
    if (sb) sb->valid_count = nrec;
    return 0;
}

namespace {

template <typename T>
int dev_alloc(cddpm_ctx* h, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(h, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    h->allocs.push_back(q);
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
    for (int i = 0; i < d->num_levels; ++i) {
        if (d->channel_mult[i] < 1) return fail(h, "channel_mult[%d]=%d unsupported: channel_mult must be >= 1", i, d->channel_mult[i]);
        if ((long long)d->channel_mult[i] * d->model_channels > 1024)
            return fail(h, "channel_mult[%d]=%d unsupported: channel_mult[%d] * model_channels = %lld exceeds 1024", i,
                        d->channel_mult[i], i, (long long)d->channel_mult[i] * d->model_channels);
    }
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
// gn_finalize_kernel keeps one fp64 (sum, sum of squares) pair per concatenated channel in LDS: MAX_CONCAT_CHANNELS.
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
    for (const Op& op : h->prog) {
        const BlockInfo& bi = h->blocks[op.block];
        const size_t elems = B * (HW / ((size_t)bi.ds * bi.ds)) * bi.C;
        if (op.kind != OP_HEAD) maxact = std::max(maxact, elems);
        if (op.push) {
            float* p = nullptr;
            want(&p, elems);
            h->hs.push_back(p);
        }
    }
    for (const ResW& r : h->res) maxC = std::max(maxC, (size_t)std::max(r.Cin, r.Cout));
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
                const size_t cap = B * (size_t)nrec_at(bi.ds) * bi.C * 2;
                float* sp = nullptr;
                want(&sp, cap);
                if (do_alloc) h->stat[h->hs[pi]] = {sp, cap, STAT_NONE};
                ++pi;
            }
        size_t maxrc = 0;
        for (const BlockInfo& bi : h->blocks) maxrc = std::max(maxrc, (size_t)nrec_at(bi.ds) * bi.C);
        float* work[3] = {h->bufA, h->bufB, h->bufH};
        for (int i = 0; i < 3; ++i) {
            float* sp = nullptr;
            want(&sp, B * maxrc * 2);
            if (do_alloc) h->stat[work[i]] = {sp, B * maxrc * 2, STAT_NONE};
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
    if (upload(h, &n->gamma, hw.get(p + ".weight"), C)) return -1;
    return upload(h, &n->beta, hw.get(p + ".bias"), C);
}

// wexp < 0: choose the pre-scale exponent from this tensor; >= 0: imposed (tensors accumulated into one output tile share it)
int upload_conv(cddpm_ctx* h, const HostWeights& hw, const std::string& p, int Cin, int Cout, int taps, ConvW* c,
                bool with_bias = true, int wexp = -1) {
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
    StatBuf& sb = h->stat.at(x);
    if (sb.valid_count == STAT_NONE) {
        const int ns = gn_nsplit(B, HW);
        if ((size_t)B * ns * C * 2 > sb.capacity) {
            fail(h, "GroupNorm statistics sweep of a [%d,%d,%d] tensor needs %zu floats, the buffer holds %zu", B, HW, C,
                 (size_t)B * ns * C * 2, sb.capacity);
            return nullptr;
        }
        Prof p(h, PC_GN, 0.0, 4.0 * B * (double)HW * C, s);
        launch_gn_partial(x, C, B, HW, ns, sb.records, s);
        sb.valid_count = ns;
    }
    *n = sb.valid_count;
    return sb.records;
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
        if (h->precision == 16) launch_attention_p16(h->qkvbuf, h->attbuf, B, N, w.C, s);
        else if (h->attn_family == 2) launch_attention_h3(h->qkvbuf, h->attbuf, B, N, w.C, s);
        else launch_attention(h->qkvbuf, h->attbuf, B, N, w.C, s);
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

// The per-sample timesteps of a call, into d_t: t_dev when given (they index device tables: kept inside [0, T)), else t_uniform.
int stage_t(cddpm_ctx* h, const int32_t* t_dev, int t_uniform, int B, hipStream_t s) {
    if (t_dev) {
        launch_copy_clamp_int(h->d_t, t_dev, B, 0, h->d.timesteps - 1, s);
    } else {
        if (t_uniform < 0 || t_uniform >= h->d.timesteps) return fail(h, "t=%d outside [0, %d)", t_uniform, h->d.timesteps);
        launch_fill_int(h->d_t, B, t_uniform, s);
    }
    return 0;
}

// UNetModel.forward (OpenAI_Unet.py:823-1006); d_t must hold the per-sample timesteps.
int forward_impl(cddpm_ctx* h, const float* x, float* out, int B, int H, int W, hipStream_t s) {
    for (auto& kv : h->stat) kv.second.valid_count = STAT_NONE;      // no tensor of this forward has statistics yet
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
    if (stage_t(h, t_dev, t_uniform, B, s)) return -1;
    return forward_impl(h, x_dev, out_dev, B, H, W, s);
}

// the posterior step's arguments that come from the handle and the call's geometry: explicit noise for one step or none (Philox),
// no finalize; the caller sets what differs
static StepArgs step_args(const cddpm_ctx* h, float* img, const float* noise, uint64_t seed, uint64_t slice0, int B, int H, int W) {
    StepArgs a;
    a.x = img; a.model_out = h->model_out; a.t_dev = h->d_t;
    a.coef1 = h->sched[0]; a.coef2 = h->sched[1]; a.logvar = h->sched[2];
    a.sqrt_recip = h->sched[3]; a.sqrt_recipm1 = h->sched[4];
    a.objective = h->objective;
    a.noise = noise; a.noise_t_stride = 0;
    a.seed = seed; a.slice0 = slice0; a.t_for_rng = 0;
    a.B = B; a.HW = H * W; a.finalize = 0; a.clip = h->clip_denoised;
    return a;
}

static int step_once(cddpm_ctx* h, float* img, const float* z_dev, uint64_t seed, uint64_t slice0, int t, int finalize,
                     int B, int H, int W, hipStream_t s) {
    launch_fill_int(h->d_t, B, t, s);
    h->nb2_now = (t >= h->nb2_tmin) ? 1 : 0;        // the step's accumulation plan: a function of t alone (precision 16: of nothing, see conv_set_nb2)
    const int rc_fwd = forward_impl(h, img, h->model_out, B, H, W, s);
    h->nb2_now = 0;
    if (rc_fwd) return -1;
    StepArgs a = step_args(h, img, z_dev, seed, slice0, B, H, W);
    a.t_for_rng = t; a.finalize = finalize;
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
    const int tmin = (h->precision == 16) ? (1 << 30) : h->nb2_tmin;      // precision 16: one plan on every step, the switch has no effect
    if (t_hi >= tmin && t_lo < tmin) {       // the plan switches inside the range: two replays, one graph each
        if (reverse_by_graph(h, img, noise_dev, seed, slice0, t_hi, tmin, B, H, W, s)) return -1;
        return reverse_by_graph(h, img, noise_dev, seed, slice0, tmin - 1, t_lo, B, H, W, s);
    }
    const int plan = (t_lo >= tmin) ? 1 : 0;
    const bool hit = g.exec && g.img == img && g.noise == noise_dev && g.seed == seed && g.slice0 == slice0 && g.B == B &&
                     g.H == H && g.W == W && g.gen == h->gen && g.nb2 == plan;
    if (!hit) {
        drop_step_graph(h);
        HIPCHECK(h, hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal));
        h->nb2_now = plan;
        int rc = forward_impl(h, img, h->model_out, B, H, W, h->gstream);
        h->nb2_now = 0;
        StepArgs a = step_args(h, img, noise_dev, seed, slice0, B, H, W);
        a.noise_t_stride = (size_t)B * H * W; a.finalize = -1;      // `noise` is the [T][B][HW] base; map to [0,1] exactly when t == 0
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
    if (!out_dev) return fail(h, "cddpm_noise_fill: out_dev is NULL");
    if (B < 1 || H < 1 || W < 1 || ((long long)H * W) % 4)
        return fail(h, "cddpm_noise_fill: B=%d H=%d W=%d unsupported (B, H, W >= 1, H * W a multiple of 4)", B, H, W);
    if ((long long)B * H * W >= (1ll << 31)) return fail(h, "cddpm_noise_fill: B * H * W = %lld, must be below 2^31", (long long)B * H * W);
    if (reinterpret_cast<uintptr_t>(out_dev) % 16) return fail(h, "cddpm_noise_fill: out_dev must be 16-byte aligned");
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

static bool hausdorff_in_range(int R, int D1, int D2) {
    return R >= 1 && D1 >= 1 && D2 >= 1 && R <= CDDPM_HAUSDORFF_MAX_AXIS && D1 <= CDDPM_HAUSDORFF_MAX_AXIS && D2 <= CDDPM_HAUSDORFF_MAX_AXIS;
}

size_t cddpm_hausdorff_workspace_bytes(int R, int D1, int D2) {
    if (!hausdorff_in_range(R, D1, D2)) {
        fail(nullptr, "cddpm_hausdorff_workspace_bytes: volume %dx%dx%d outside 1 ... %d per axis", R, D1, D2, CDDPM_HAUSDORFF_MAX_AXIS);
        return 0;
    }
    return hausdorff_workspace_bytes(R, D1, D2);
}

int cddpm_eval_hausdorff(cddpm_handle h, const uint8_t* pred_dev, const float* seg_dev, int R, int D1, int D2, int flags,
                         void* ws_dev, size_t ws_bytes, double* out_dev, uint8_t* edges_dev, int32_t* dist2_dev, void* stream) {
    if (!h) return -1;
    if (!pred_dev || !seg_dev || !ws_dev || !out_dev) return fail(h, "cddpm_eval_hausdorff: NULL argument");
    if (!hausdorff_in_range(R, D1, D2))
        return fail(h, "cddpm_eval_hausdorff: volume %dx%dx%d outside 1 ... %d per axis", R, D1, D2, CDDPM_HAUSDORFF_MAX_AXIS);
    if (flags & ~CDDPM_HAUSDORFF_SQUEEZE) return fail(h, "cddpm_eval_hausdorff: unknown flags 0x%x", flags);
    const size_t need = hausdorff_workspace_bytes(R, D1, D2);
    if (ws_bytes < need) return fail(h, "cddpm_eval_hausdorff: workspace of %zu bytes, need %zu", ws_bytes, need);
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, launch_eval_hausdorff(pred_dev, seg_dev, R, D1, D2, (flags & CDDPM_HAUSDORFF_SQUEEZE) ? 1 : 0, ws_dev, ws_bytes,
                                      out_dev, edges_dev, dist2_dev, (hipStream_t)stream));
    return 0;
}

static bool aug_in_range(int B, int H, int W, int D) {
    return B >= 1 && B <= CDDPM_AUG_MAX_BATCH && H >= 1 && W >= 1 && D >= 1 && H <= CDDPM_AUG_MAX_AXIS && W <= CDDPM_AUG_MAX_AXIS && D <= CDDPM_AUG_MAX_AXIS;
}

size_t cddpm_aug_workspace_bytes(int B, int H, int W, int D) {
    if (!aug_in_range(B, H, W, D)) {
        fail(nullptr, "cddpm_aug_workspace_bytes: B = %d outside 1 ... %d or volume %dx%dx%d outside 1 ... %d per axis", B, CDDPM_AUG_MAX_BATCH, H, W, D,
             CDDPM_AUG_MAX_AXIS);
        return 0;
    }
    return aug_workspace_bytes(B, H, W, D);
}

int cddpm_aug_slices(cddpm_handle h, const float* bank_dev, int N, int H, int W, int D, const int32_t* meta_dev, const float* par_dev,
                     int B, void* ws_dev, size_t ws_bytes, float* out_dev, void* stream) {
    if (!h) return -1;
    if (!bank_dev || !meta_dev || !par_dev || !ws_dev || !out_dev) return fail(h, "cddpm_aug_slices: NULL argument");
    if (N < 1) return fail(h, "cddpm_aug_slices: a bank of %d volumes", N);
    if (!aug_in_range(B, H, W, D))
        return fail(h, "cddpm_aug_slices: B = %d outside 1 ... %d or volume %dx%dx%d outside 1 ... %d per axis", B, CDDPM_AUG_MAX_BATCH, H, W, D,
                    CDDPM_AUG_MAX_AXIS);
    const size_t need = aug_workspace_bytes(B, H, W, D);
    if (ws_bytes < need) return fail(h, "cddpm_aug_slices: workspace of %zu bytes, need %zu", ws_bytes, need);
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, launch_aug_slices(bank_dev, N, H, W, D, meta_dev, par_dev, B, ws_dev, ws_bytes, out_dev, (hipStream_t)stream));
    return 0;
}

size_t cddpm_aug_pipeline_workspace_bytes(int B, int H, int W, int D) {
    if (!aug_in_range(B, H, W, D)) {
        fail(nullptr, "cddpm_aug_pipeline_workspace_bytes: B = %d outside 1 ... %d or volume %dx%dx%d outside 1 ... %d per axis", B, CDDPM_AUG_MAX_BATCH, H, W, D,
             CDDPM_AUG_MAX_AXIS);
        return 0;
    }
    return aug_pipeline_workspace_bytes(B, H, W, D);
}

int cddpm_aug_pipeline(cddpm_handle h, const float* bank_dev, int N, int H, int W, int D, const int32_t* meta_dev, const float* par_dev,
                       int B, void* ws_dev, size_t ws_bytes, float* out_dev, void* stream) {
    if (!h) return -1;
    if (!bank_dev || !meta_dev || !par_dev || !ws_dev || !out_dev) return fail(h, "cddpm_aug_pipeline: NULL argument");
    if (N < 1) return fail(h, "cddpm_aug_pipeline: a bank of %d volumes", N);
    if (!aug_in_range(B, H, W, D))
        return fail(h, "cddpm_aug_pipeline: B = %d outside 1 ... %d or volume %dx%dx%d outside 1 ... %d per axis", B, CDDPM_AUG_MAX_BATCH, H, W, D,
                    CDDPM_AUG_MAX_AXIS);
    const size_t need = aug_pipeline_workspace_bytes(B, H, W, D);
    if (ws_bytes < need) return fail(h, "cddpm_aug_pipeline: workspace of %zu bytes, need %zu", ws_bytes, need);
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, launch_aug_pipeline(bank_dev, N, H, W, D, meta_dev, par_dev, B, ws_dev, ws_bytes, out_dev, (hipStream_t)stream));
    return 0;
}

// what the host can see of a preprocessing geometry; the reason, or NULL
static const char* prep_refusal(int H, int W, int D, int stages, int allowed, int th, int tw, int td, double f) {
    const int M = CDDPM_PREP_MAX_AXIS;
    if (H < 1 || W < 1 || D < 1 || H > M || W > M || D > M) return "volume outside 1 ... 1024 per axis";
    if (stages & ~allowed) return "unknown or unsupported stage bits";
    if ((stages & CDDPM_PREP_CROPPAD) && (th < 1 || tw < 1 || td < 1 || th > M || tw > M || td > M)) return "target outside 1 ... 1024 per axis";
    if (stages & CDDPM_PREP_RESAMPLE) {
        if (!(f >= 1.0) || !std::isfinite(f)) return "resample factor f < 1 or not finite";
        const bool cp = (stages & CDDPM_PREP_CROPPAD) != 0;
        if (f != 1.0 && ((cp ? th : H) == 1 || (cp ? tw : W) == 1 || (cp ? td : D) == 1)) return "an axis of length 1 is not resampled with f != 1";
    }
    return nullptr;
}

size_t cddpm_prep_workspace_bytes(int H, int W, int D, int stages, int th, int tw, int td, double f) {
    if (const char* why = prep_refusal(H, W, D, stages, CDDPM_PREP_ALL, th, tw, td, f)) {
        fail(nullptr, "cddpm_prep_workspace_bytes: %s (volume %dx%dx%d, stages 0x%x, target %dx%dx%d, f %g)", why, H, W, D, stages, th, tw, td, f);
        return 0;
    }
    return prep_workspace_bytes(H, W, D, stages, th, tw, td, f);
}

int cddpm_prep_volume(cddpm_handle h, const float* vol_dev, const uint8_t* mask_dev, int H, int W, int D, int stages, int iterations, int th,
                      int tw, int td, const double* par_host, void* ws_dev, size_t ws_bytes, float* out_dev, uint8_t* mask_out_dev,
                      double* record_dev, void* stream) {
    if (!h) return -1;
    if (!vol_dev || !par_host || !ws_dev || !out_dev || !record_dev) return fail(h, "cddpm_prep_volume: NULL argument");
    const double f = par_host[CDDPM_PREP_PAR_FACTOR], lo = par_host[CDDPM_PREP_PAR_PERC_LO], hi = par_host[CDDPM_PREP_PAR_PERC_HI];
    if (const char* why = prep_refusal(H, W, D, stages, CDDPM_PREP_ALL, th, tw, td, f))
        return fail(h, "cddpm_prep_volume: %s (volume %dx%dx%d, stages 0x%x, target %dx%dx%d, f %g)", why, H, W, D, stages, th, tw, td, f);
    if ((stages & CDDPM_PREP_RESCALE) && !(0.0 <= lo && lo <= hi && hi <= 100.0))
        return fail(h, "cddpm_prep_volume: percentiles (%g, %g) outside 0 <= lo <= hi <= 100", lo, hi);
    if (stages & CDDPM_PREP_SMOOTH) {
        if (iterations < 0 || iterations > CDDPM_PREP_MAX_ITERATIONS)
            return fail(h, "cddpm_prep_volume: %d iterations outside 0 ... %d", iterations, CDDPM_PREP_MAX_ITERATIONS);
        bool ok = std::isfinite(par_host[CDDPM_PREP_PAR_DT]);
        for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(par_host[CDDPM_PREP_PAR_SPACING + a]) && par_host[CDDPM_PREP_PAR_SPACING + a] > 0.0;
        if (!ok) return fail(h, "cddpm_prep_volume: dt not finite or a spacing not positive and finite");
    }
    if ((const void*)out_dev == (const void*)vol_dev) return fail(h, "cddpm_prep_volume: output equal to input");
    if (mask_out_dev && (const void*)mask_out_dev == (const void*)mask_dev) return fail(h, "cddpm_prep_volume: mask output equal to mask input");
    const size_t need = prep_workspace_bytes(H, W, D, stages, th, tw, td, f);
    if (ws_bytes < need) return fail(h, "cddpm_prep_volume: workspace of %zu bytes, need %zu", ws_bytes, need);
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, launch_prep_volume(vol_dev, mask_dev, H, W, D, stages, iterations, th, tw, td, par_host, ws_dev, ws_bytes, out_dev, mask_out_dev,
                                   record_dev, (hipStream_t)stream));
    return 0;
}

int cddpm_prep_labels(cddpm_handle h, const uint8_t* lab_dev, int H, int W, int D, int stages, int th, int tw, int td, double f, uint8_t* out_dev,
                      void* stream) {
    if (!h) return -1;
    if (!lab_dev || !out_dev) return fail(h, "cddpm_prep_labels: NULL argument");
    if (const char* why = prep_refusal(H, W, D, stages, CDDPM_PREP_CROPPAD | CDDPM_PREP_RESAMPLE, th, tw, td, f))
        return fail(h, "cddpm_prep_labels: %s (volume %dx%dx%d, stages 0x%x, target %dx%dx%d, f %g)", why, H, W, D, stages, th, tw, td, f);
    if (out_dev == lab_dev) return fail(h, "cddpm_prep_labels: output equal to input");
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, launch_prep_labels(lab_dev, H, W, D, stages, th, tw, td, f, out_dev, (hipStream_t)stream));
    return 0;
}

int cddpm_q_sample(cddpm_handle h, const float* x01_dev, const float* noise_dev, const int32_t* t_dev, int t_uniform,
                   const float* sqrt_ac_host, const float* sqrt_1mac_host, int T, float* out_dev, int B, int H, int W,
                   void* stream) {
    if (!h) return -1;
    if (T != h->d.timesteps) return fail(h, "T mismatch");
    if (B < 1 || B > h->d.max_batch || H < 1 || W < 1 || ((long long)H * W) % 4 || (long long)B * H * W >= (1ll << 31))
        return fail(h, "cddpm_q_sample: B=%d H=%d W=%d unsupported (1 <= B <= max_batch=%d, H * W a multiple of 4, B * H * W below 2^31)", B, H, W,
                    h->d.max_batch);
    if (!x01_dev || !noise_dev || !out_dev || !sqrt_ac_host || !sqrt_1mac_host) return fail(h, "cddpm_q_sample: NULL argument");
    if (reinterpret_cast<uintptr_t>(x01_dev) % 16 || reinterpret_cast<uintptr_t>(noise_dev) % 16 || reinterpret_cast<uintptr_t>(out_dev) % 16)
        return fail(h, "cddpm_q_sample: x01_dev, noise_dev and out_dev must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(h, hipSetDevice(h->device));
    if (stage_t(h, t_dev, t_uniform, B, s)) return -1;      // first: a bad t_uniform is refused before anything is enqueued
    HIPCHECK(h, hipMemcpyAsync(h->qs_sa, sqrt_ac_host, (size_t)T * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHECK(h, hipMemcpyAsync(h->qs_s1, sqrt_1mac_host, (size_t)T * sizeof(float), hipMemcpyHostToDevice, s));
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
    if (family != 2 && h->precision == 16)
        return fail(h, "cddpm_set_conv_family: the handle is at precision 16, which only the h3 family has (cddpm_set_precision(h, 32) first)");
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

int cddpm_get_attention_family(cddpm_handle h) { return h ? h->attn_family : -1; }

int cddpm_set_attention_family(cddpm_handle h, int family) {
    if (!h) return -1;
    if (family == 1)
        return fail(h, "cddpm_set_attention_family: there is no x6 attention (2 = h3: fp32-grade fp16 splits, 0 = f32: exact fp32 MFMA)");
    if (family != 0 && family != 2) return fail(h, "cddpm_set_attention_family: unknown family %d (2 = h3, 0 = f32)", family);
    if (family == h->attn_family) return 0;
    h->gen++;                            // a captured step graph has the family's kernel baked in
    h->attn_family = family;             // nothing to repack: the attention core has no weights
    return 0;
}

int cddpm_get_precision(cddpm_handle h) { return h ? h->precision : -1; }

int cddpm_set_precision(cddpm_handle h, int bits) {
    if (!h) return -1;
    if (bits != 16 && bits != 32) return fail(h, "cddpm_set_precision: precision must be 32 or 16, got %d", bits);
    if (bits == 16 && h->family != 2)
        return fail(h, "cddpm_set_precision: precision 16 needs the h3 convolution family (the handle's family is %s)", h->family == 1 ? "x6" : "f32");
    if (bits == h->precision) return 0;
    h->gen++;                            // a captured step graph has the precision's kernels baked in
    h->precision = bits;                 // no repack: the hi-only kernels read the hi plane of the h3 weight image
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

}  // extern "C"
