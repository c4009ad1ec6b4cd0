// The standalone operators of libcddpm_hip.so's C ABI (cddpm_op_* of include/cddpm.h): single kernels and small kernel groups behind
// argument checks, what the training step (training.py, encoder_training.py) is sequenced from and what the kernel tests call. Host
// code only. Every operator has one form: OP_CHECK (once per message), OP_PROLOGUE, temporaries from an OpScratch, launches,
// OP_EPILOGUE (cddpm_ctx.h). An operator with shape-dependent temporaries states them ONCE, in a static *_scratch function over an
// OpScratch: the operator runs it on its real scratch and gets the pointers, its exported size query (cddpm_op_*_scratch) runs it on a
// counting scratch and returns the bytes. The handle, the forward program and the reverse loop are in cddpm_api.hip.
#include "cddpm_ctx.h"

#include <cmath>

using namespace cddpm;

// a size query: the operator's own request function, run on a scratch that only counts
template <class Request> static size_t counted(Request&& request) {
    OpScratch sc;
    request(sc);
    return sc.off;
}

extern "C" {

int cddpm_op_set_scratch(cddpm_handle h, size_t bytes) {      // the arena's setter: no stream, nothing to launch
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
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, x_dev && out_dev && n >= 1, "cddpm_op_absmax: bad arguments")
    launch_absmax(x_dev, n, out_dev, s);
    OP_EPILOGUE()
}

int cddpm_op_pack_conv(cddpm_handle h, const float* w_dev, int Cout, int Cin, int ksize, int mode, int scale_exp, void* packed_dev,
                       void* stream) {
    OP_CHECK(h->family == 2, "cddpm_op_pack_conv: the device packer serves the default convolution family (CDDPM_CONV=h3) only")
    // O / I: output / input channels of the PACKED operator (mode 1 swaps the roles of the forward tensor's dimensions)
    const int O = mode == 1 ? Cin : Cout, I = mode == 1 ? Cout : Cin;
    OP_PROLOGUE(PC_OPT, 0.0, 0.0,
                w_dev && packed_dev && (ksize == 1 || ksize == 3) && mode >= 0 && mode <= 2 && (mode != 2 || ksize == 3) && O > 0 && I > 0 &&
                    O % 128 == 0 && I % 32 == 0 && scale_exp >= 0 && scale_exp <= 24,
                "cddpm_op_pack_conv: unsupported arguments (Cout %d, Cin %d, k %d, mode %d, exponent %d)", Cout, Cin, ksize, mode, scale_exp)
    launch_pack_conv_split(w_dev, O, I, mode == 2 ? 4 : ksize * ksize, mode, scale_exp, packed_dev, s);
    OP_EPILOGUE()
}

int cddpm_op_pack_conv_batch(cddpm_handle h, const cddpm_pack_job* jobs_dev, int njobs, int64_t max_units, void* stream) {
    OP_CHECK(h->family == 2, "cddpm_op_pack_conv_batch: the device packer serves the default convolution family (CDDPM_CONV=h3) only")
    static_assert(sizeof(cddpm_pack_job) == sizeof(PackJob), "job table layout");
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, jobs_dev && njobs >= 1 && njobs <= 65535 && max_units >= 1, "cddpm_op_pack_conv_batch: bad arguments")
    launch_pack_conv_split_batch(reinterpret_cast<const PackJob*>(jobs_dev), njobs, max_units, s);
    OP_EPILOGUE()
}

int cddpm_op_conv_packed(cddpm_handle h, const float* src0, int C0, const float* src1, int C1, const float* coef_dev, int silu, int folded_up,
                         const void* packed_dev, int scale_exp, const float* bias_dev, int Cout, int ksize, const float* res_dev,
                         int res_upsample, const float* skip_dev, int S0, const float* skip1_dev, int S1, const void* skip_packed_dev,
                         float* out_dev, float* stats_dev, int B, int H, int W, void* stream) {
    OP_CHECK(h->family == 2, "cddpm_op_conv_packed: default convolution family (CDDPM_CONV=h3) only")
    OP_CHECK(!((ksize != 1 && ksize != 3) || C0 <= 0 || C0 % 32 || C1 < 0 || C1 % 32 || Cout <= 0 || Cout % 128 || Cout > 4096 || B < 1 || H < 1 || W < 1 ||
               (folded_up && (ksize != 3 || C1 || H % 2 || W % 2)) ||
               (skip_dev && (S0 <= 0 || S0 % 32 || !skip_packed_dev || ksize != 3 || S1 < 0 || S1 % 32 || (S1 > 0 && !skip1_dev))) ||
               (C1 && !src1) || scale_exp < 0 || scale_exp > 24),
             "cddpm_op_conv_packed: unsupported shape (k %d, C0 %d, C1 %d, Cout %d, S0 %d)", ksize, C0, C1, Cout, S0)
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.src1 = src1; a.C1 = C1;
    a.srcH = folded_up ? H / 2 : H; a.srcW = folded_up ? W / 2 : W;
    a.coef = coef_dev; a.silu = silu; a.wpk = static_cast<const float*>(packed_dev); a.res = res_dev; a.res_up = res_upsample;
    a.skip0 = skip_dev; a.S0 = skip_dev ? S0 : 0; a.skip_wpk = static_cast<const float*>(skip_packed_dev);
    a.skip1 = (skip_dev && S1 > 0) ? skip1_dev : nullptr; a.S1 = (skip_dev && S1 > 0) ? S1 : 0;      // the skip input as two concatenated tensors
    a.wscale_inv = ldexpf(1.0f, -scale_exp);
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = folded_up ? 4 : ksize * ksize;
    a.stats = stats_dev;       // [B][cddpm_stat_records(H, W, folded_up ? 1 : 0)][Cout][2]: the output's GroupNorm statistics records, for free
    // CDDPM_TRAIN_PRECISION=16: the training operators multiply plain fp16 operands (hi terms only), as the reference trainer's precision 16 does
    a.hi_only = train_precision() == 16 ? 1 : 0;
    conv_set_nb2(a, h, NB2_CALL_PLAN, conv_workgroups(a, B, H, W));
    OP_PROLOGUE(a.taps == 1 ? PC_CONV1 : PC_CONV3, conv_flops(a), conv_bytes(a), src0 && packed_dev && out_dev, "cddpm_op_conv_packed: NULL argument")
    if (!bias_dev && need_zero_bias(h)) return -1;
    a.bias = bias_dev ? bias_dev : h->zero_bias;
    launch_conv(a, s);
    OP_EPILOGUE()
}

int cddpm_op_gn_coef_rec(cddpm_handle h, const float* rec0_dev, int n0, int C0, const float* rec1_dev, int n1, int C1, const float* gamma_host,
                         const float* beta_host, const float* film_dev, float* coef_dev, int B, int HW, void* stream) {
    const int C = C0 + C1;
    OP_CHECK(!(C0 % 4 || C1 % 4 || C % 32 || C > MAX_CONCAT_CHANNELS || C0 > 1024 || C1 > 1024 || C0 <= 0 || n0 < 1 || (C1 > 0 && (n1 < 1 || !rec1_dev))),
             "cddpm_op_gn_coef_rec: unsupported channels / record counts")
    OP_PROLOGUE(PC_GN, 0.0, 0.0, rec0_dev && gamma_host && beta_host && coef_dev, "cddpm_op_gn_coef_rec: NULL argument")
    OpScratch sc(h, s);
    const float* g = sc.param(gamma_host, C);
    const float* bt = sc.param(beta_host, C);
    SCRATCH_CHECK(sc)
    launch_gn_finalize(rec0_dev, C0, n0, C1 ? rec1_dev : nullptr, C1, C1 ? n1 : 0, B, HW, g, bt, nullptr, nullptr, 0, 0, nullptr, film_dev, coef_dev, s);
    OP_EPILOGUE()
}

// ---- standalone ops for kernel tests ---------------------------------------------------------------
// The four convolutions below take their weights from HOST memory. One path: pack on the host for the handle's family (host_pack),
// stage the image and the bias through a scratch of the call (never the arena: a trainer sizes that for its own operators), fill the
// rest of ConvArgs and launch (test_conv_launch), synchronise (OP_EPILOGUE_SYNC): the copies read the packed image and the caller's
// host arrays until the stream has run them, so every host image is declared BEFORE the OpScratch, whose destructor waits for the
// stream on every path before it frees.
static std::vector<float> host_pack(const cddpm_ctx* h, const float* w, int Cout, int Cin, int taps, int wexp) {
    std::vector<float> pk(packed_conv_floats(Cout, Cin, taps, h->family));
    pack_conv_weights(w, Cout, Cin, taps, pk.data(), wexp, h->family);
    return pk;
}
static int test_conv_launch(cddpm_ctx* h, OpScratch& sc, ConvArgs& a, const std::vector<float>& pk, const float* bias_host, int wexp) {
    a.wpk = sc.param(pk.data(), pk.size());
    a.bias = sc.param(bias_host, a.Cout);
    SCRATCH_CHECK(sc)
    a.wscale_inv = ldexpf(1.0f, -wexp);
    conv_set_nb2(a, h, NB2_FORCED_ONLY, conv_workgroups(a, a.B, a.H, a.W));
    launch_conv(a, sc.s);
    return 0;
}
#define OP_EPILOGUE_SYNC()                                        \
    HIPCHECK(h, hipGetLastError());                               \
    HIPCHECK(h, hipStreamSynchronize(s));                         \
    return 0;

int cddpm_op_conv(cddpm_handle h, const float* src0, int C0, const float* src1, int C1, const float* coef_dev, int silu,
                  int upsample, const float* w_host, const float* bias_host, int Cout, int ksize, const float* res_dev,
                  int res_upsample, float* out_dev, int B, int H, int W, void* stream) {
    const int Cin = C0 + C1, taps = ksize * ksize;
    OP_CHECK(!((ksize != 1 && ksize != 3) || C0 % 32 || C1 % 32 || Cin <= 0 || Cout % 128 || Cout <= 0),
             "cddpm_op_conv: unsupported shape (ksize %d, C0 %d, C1 %d, Cout %d)", ksize, C0, C1, Cout)
    OP_CHECK(!(upsample && (H % 2 || W % 2)), "upsample needs even H, W")
    const bool folded = (upsample == 2);      // upsample: 1 = gather form, 2 = folded 2x2-tap form (what the UNet uses)
    OP_PROLOGUE(PC_NONE, 0.0, 0.0, !(folded && (ksize != 3 || C1 != 0)), "folded upsample needs a 3x3 kernel and a single source")
    std::vector<float> pk(folded ? 4 * packed_conv_floats(Cout, Cin, 4, h->family) : 0);
    const int wexp = folded ? pack_conv_weights_up2(w_host, Cout, Cin, pk.data(), h->family)
                            : conv_weight_exp(w_host, (size_t)Cout * Cin * taps, h->family);
    if (!folded) pk = host_pack(h, w_host, Cout, Cin, taps, wexp);
    OpScratch sc(h, s, true);
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.src1 = src1; a.C1 = C1;
    a.srcH = upsample ? H / 2 : H; a.srcW = upsample ? W / 2 : W; a.upsample = folded ? 0 : upsample;
    a.coef = coef_dev; a.silu = silu; a.res = res_dev; a.res_up = res_upsample;
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = folded ? 4 : taps;
    if (test_conv_launch(h, sc, a, pk, bias_host, wexp)) return -1;
    OP_EPILOGUE_SYNC()
}

int cddpm_op_conv_skip(cddpm_handle h, const float* src0, int C0, const float* coef_dev, int silu, const float* w_host,
                       const float* bias_host, int Cout, const float* skip_dev, int S0, const float* wskip_host,
                       float* out_dev, int B, int H, int W, void* stream) {
    OP_CHECK(!(C0 % 32 || C0 <= 0 || S0 % 32 || S0 <= 0 || Cout % 128 || Cout <= 0),
             "cddpm_op_conv_skip: unsupported shape (C0 %d, S0 %d, Cout %d)", C0, S0, Cout)
    OP_PROLOGUE(PC_NONE, 0.0, 0.0, src0 && skip_dev && w_host && wskip_host && bias_host && out_dev, "cddpm_op_conv_skip: NULL argument")
    // one pre-scale exponent for both tensors, as cddpm_load_weights chooses it
    const int fam = h->family;
    const int wexp = std::min(conv_weight_exp(w_host, (size_t)Cout * C0 * 9, fam), conv_weight_exp(wskip_host, (size_t)Cout * S0, fam));
    const std::vector<float> pk = host_pack(h, w_host, Cout, C0, 9, wexp), pks = host_pack(h, wskip_host, Cout, S0, 1, wexp);
    OpScratch sc(h, s, true);
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.srcH = H; a.srcW = W; a.coef = coef_dev; a.silu = silu;
    a.skip0 = skip_dev; a.S0 = S0; a.skip_wpk = sc.param(pks.data(), pks.size());
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = 9;
    if (test_conv_launch(h, sc, a, pk, bias_host, wexp)) return -1;
    OP_EPILOGUE_SYNC()
}

int cddpm_op_conv_gn(cddpm_handle h, const float* src0, int C0, const float* w_host, const float* bias_host, int Cout,
                     const float* gamma_host, const float* beta_host, float* out_dev, float* coef_dev, int B, int H, int W,
                     void* stream) {
    OP_CHECK(!(C0 % 32 || C0 <= 0 || Cout % 128 || Cout <= 0 || Cout > 1024), "cddpm_op_conv_gn: unsupported shape")
    OP_PROLOGUE(PC_NONE, 0.0, 0.0, src0 && w_host && bias_host && gamma_host && beta_host && out_dev && coef_dev, "cddpm_op_conv_gn: NULL argument")
    const int wexp = conv_weight_exp(w_host, (size_t)Cout * C0 * 9, h->family);
    const std::vector<float> pk = host_pack(h, w_host, Cout, C0, 9, wexp);
    const int nrec = conv_stat_records(H, W);
    OpScratch sc(h, s, true);
    const float* g = sc.param(gamma_host, Cout);
    const float* bt = sc.param(beta_host, Cout);
    float* rec = sc.n<float>((size_t)B * nrec * Cout * CDDPM_STAT_FLOATS);
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.srcH = H; a.srcW = W; a.stats = rec;
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = 9;
    if (test_conv_launch(h, sc, a, pk, bias_host, wexp)) return -1;
    launch_gn_finalize(rec, Cout, nrec, nullptr, 0, 0, B, H * W, g, bt, nullptr, nullptr, 0, 0, nullptr, nullptr, coef_dev, s);
    OP_EPILOGUE_SYNC()
}

// One convolution through conv_launch -- the plan of the handle, not of the call: for the duration of the call the handle is "inside a
// forward at img_H x img_W" (cur_H / cur_W) on a step of accumulation plan t (nb2_now), and out_dev has a statistics buffer when the
// GroupNorm coefficients are asked for, as every activation buffer of the forward program has. All of it is put back on every path.
namespace {
struct PlannedCallScope {
    cddpm_ctx* h; int H, W, nb2; const float* stat_key;
    ~PlannedCallScope() {
        h->cur_H = H; h->cur_W = W; h->nb2_now = nb2;
        if (stat_key) h->stat.erase(stat_key);
    }
};
}
int cddpm_op_conv_planned(cddpm_handle h, const float* src0, int C0, const float* src1, int C1, const float* coef_dev, int silu, int folded_up,
                          const float* w_host, const float* bias_host, int Cout, int ksize, const float* res_dev, int res_upsample,
                          const float* skip0_dev, int S0, const float* skip1_dev, int S1, const float* wskip_host, const float* gamma_host,
                          const float* beta_host, float* coef_out_dev, float* out_dev, int B, int H, int W, int img_H, int img_W, int t,
                          int* ksplit_out, int* kbound_out, int* nb2_out, int* scale_exp_out, void* stream) {
    const int Cin = C0 + C1, taps = ksize * ksize;
    const bool skip = skip0_dev != nullptr, gn = gamma_host || beta_host || coef_out_dev;
    OP_CHECK(!((ksize != 1 && ksize != 3) || C0 <= 0 || C0 % 32 || C1 < 0 || C1 % 32 || Cin > MAX_CONCAT_CHANNELS || Cout <= 0 || Cout % 128 ||
               Cout > 4096 || (C1 && !src1) || (folded_up && (ksize != 3 || C1 || H % 2 || W % 2 || skip)) ||
               (skip && (ksize != 3 || S0 <= 0 || S0 % 32 || S1 < 0 || S1 % 32 || S0 + S1 > MAX_CONCAT_CHANNELS || !wskip_host ||
                         (S1 > 0 && !skip1_dev) || res_dev)) ||
               (res_upsample && (!res_dev || H % 2 || W % 2)) || (gn && (!gamma_host || !beta_host || !coef_out_dev || Cout > 1024))),
             "cddpm_op_conv_planned: unsupported shape (k %d, C0 %d, C1 %d, Cout %d, S0 %d, S1 %d)", ksize, C0, C1, Cout, S0, S1)
    OP_CHECK(B >= 1 && B <= h->d.max_batch && img_H >= 1 && img_H <= h->d.max_h && img_W >= 1 && img_W <= h->d.max_w && H >= 1 && H <= img_H &&
                 W >= 1 && W <= img_W,
             "cddpm_op_conv_planned: a %d x %d layer of a %d x %d x %d forward is outside the handle's geometry (%d x %d x %d)", H, W, B, img_H, img_W,
             h->d.max_batch, h->d.max_h, h->d.max_w)
    OP_CHECK(h->stat.find(out_dev) == h->stat.end(), "cddpm_op_conv_planned: out_dev is a buffer of the handle")
    OP_PROLOGUE(PC_NONE, 0.0, 0.0, src0 && w_host && bias_host && out_dev, "cddpm_op_conv_planned: NULL argument")
    // one pre-scale exponent for the main and the skip tensor, as cddpm_load_weights chooses it; the folded classes choose their own
    const int fam = h->family;
    std::vector<float> pk(folded_up ? 4 * packed_conv_floats(Cout, Cin, 4, fam) : 0), pks;
    int wexp = folded_up ? pack_conv_weights_up2(w_host, Cout, Cin, pk.data(), fam) : conv_weight_exp(w_host, (size_t)Cout * Cin * taps, fam);
    if (skip) wexp = std::min(wexp, conv_weight_exp(wskip_host, (size_t)Cout * (S0 + S1), fam));
    if (!folded_up) pk = host_pack(h, w_host, Cout, Cin, taps, wexp);
    if (skip) pks = host_pack(h, wskip_host, Cout, S0 + S1, 1, wexp);
    // records of either epilogue: the convolution's own (per wave tile) or the combine's (per 64 consecutive pixels)
    const int nrec_cap = std::max(conv_reduce_stat_records(H, W), folded_up ? conv_stat_records_up2(H, W) : conv_stat_records(H, W));
    OpScratch sc(h, s, true);
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = src0; a.C0 = C0; a.src1 = C1 ? src1 : nullptr; a.C1 = C1;
    a.srcH = folded_up ? H / 2 : H; a.srcW = folded_up ? W / 2 : W;
    a.coef = coef_dev; a.silu = silu; a.res = res_dev; a.res_up = res_dev ? res_upsample : 0;
    if (skip) {
        a.skip0 = skip0_dev; a.S0 = S0; a.skip1 = S1 > 0 ? skip1_dev : nullptr; a.S1 = S1;
        a.skip_wpk = sc.param(pks.data(), pks.size());
    }
    a.out = out_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cout; a.taps = folded_up ? 4 : taps;
    a.wpk = sc.param(pk.data(), pk.size());
    a.bias = sc.param(bias_host, Cout);
    a.wscale_inv = ldexpf(1.0f, -wexp);
    const float *g = nullptr, *bt = nullptr;
    float* rec = nullptr;
    if (gn) {
        g = sc.param(gamma_host, Cout);
        bt = sc.param(beta_host, Cout);
        rec = sc.n<float>((size_t)B * nrec_cap * Cout * CDDPM_STAT_FLOATS);
    }
    SCRATCH_CHECK(sc)
    PlannedCallScope scope{h, h->cur_H, h->cur_W, h->nb2_now, nullptr};
    h->cur_H = img_H; h->cur_W = img_W;
    h->nb2_now = (t >= 0 && t >= h->nb2_tmin) ? 1 : 0;      // as step_once of cddpm_api.hip sets it; t < 0: a single forward
    if (gn) {
        h->stat[out_dev] = StatBuf{rec, (size_t)B * nrec_cap * Cout * CDDPM_STAT_FLOATS, STAT_NONE};
        scope.stat_key = out_dev;
    }
    ConvPlanTaken took;
    if (conv_launch(h, a, s, &took)) return -1;
    if (ksplit_out) *ksplit_out = took.S;
    if (kbound_out) {
        if (took.S == 1) { took.kbound[0] = 0; took.kbound[1] = (short)((Cin + a.S0 + a.S1) / 32); }
        for (int j = 0; j <= CDDPM_MAX_KSPLIT; ++j) kbound_out[j] = j <= took.S ? took.kbound[j] : 0;
    }
    if (nb2_out) *nb2_out = took.nb2;
    if (scale_exp_out) *scale_exp_out = wexp;
    if (gn) launch_gn_finalize(rec, Cout, h->stat[out_dev].valid_count, nullptr, 0, 0, B, H * W, g, bt, nullptr, nullptr, 0, 0, nullptr, nullptr, coef_out_dev, s);
    OP_EPILOGUE_SYNC()
}

static void gn_coef_scratch(OpScratch& sc, int C0, bool two, int C1, int B, int HW, float*& rec0, float*& rec1) {
    const int ns = gn_nsplit(B, HW);
    rec0 = sc.n<float>((size_t)B * ns * C0 * 2);
    rec1 = two ? sc.n<float>((size_t)B * ns * C1 * 2) : nullptr;
}
size_t cddpm_op_gn_coef_scratch(int C0, int has_src1, int C1, int B, int HW) {
    float *rec0, *rec1;
    return counted([&](OpScratch& sc) { gn_coef_scratch(sc, C0, has_src1 != 0, C1, B, HW, rec0, rec1); });
}
int cddpm_op_gn_coef(cddpm_handle h, const float* src0, int C0, const float* src1, int C1, const float* gamma_host,
                     const float* beta_host, const float* film_dev, float* coef_dev, int B, int HW, void* stream) {
    const int C = C0 + C1;
    OP_PROLOGUE(PC_GN, 0.0, 0.0, !(C0 % 4 || C1 % 4 || C % 32 || C > MAX_CONCAT_CHANNELS || C0 > 1024 || C1 > 1024),
                "cddpm_op_gn_coef: unsupported channels (each source <= 1024, together <= %d)", MAX_CONCAT_CHANNELS)
    const int ns = gn_nsplit(B, HW);
    OpScratch sc(h, s);
    float *rec0, *rec1;
    gn_coef_scratch(sc, C0, src1 != nullptr, C1, B, HW, rec0, rec1);
    const float* g = sc.param(gamma_host, C);
    const float* bt = sc.param(beta_host, C);
    SCRATCH_CHECK(sc)
    launch_gn_partial(src0, C0, B, HW, ns, rec0, s);
    if (src1) launch_gn_partial(src1, C1, B, HW, ns, rec1, s);
    launch_gn_finalize(rec0, C0, ns, rec1, C1, src1 ? ns : 0, B, HW, g, bt, nullptr, nullptr, 0, 0, nullptr, film_dev,
                       coef_dev, s);
    OP_EPILOGUE()
}

int cddpm_op_conv_dgrad(cddpm_handle h, const float* dy_dev, int Cout, const float* w_host, int Cin, int ksize, float* dx_dev,
                        int B, int H, int W, void* stream) {
    const int taps = ksize * ksize;
    OP_CHECK(!((ksize != 1 && ksize != 3) || Cin <= 0 || Cin % 128 || Cout <= 0 || Cout % 32),
             "cddpm_op_conv_dgrad: unsupported shape (ksize %d, Cin %d must be a multiple of 128, Cout %d of 32)", ksize, Cin, Cout)
    OP_PROLOGUE(PC_NONE, 0.0, 0.0, dy_dev && w_host && dx_dev, "cddpm_op_conv_dgrad: NULL argument")
    // wt[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx]: the gradient of a cross-correlation is a cross-correlation with this tensor
    std::vector<float> wt((size_t)Cin * Cout * taps);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < taps; ++t)
                wt[((size_t)ci * Cout + co) * taps + (taps - 1 - t)] = w_host[((size_t)co * Cin + ci) * taps + t];
    const int wexp = conv_weight_exp(wt.data(), wt.size(), h->family);
    const std::vector<float> pk = host_pack(h, wt.data(), Cin, Cout, taps, wexp), zb(Cin, 0.f);
    OpScratch sc(h, s, true);
    ConvArgs a;
    zero_conv_args(a, h);
    a.src0 = dy_dev; a.C0 = Cout; a.srcH = H; a.srcW = W;
    a.out = dx_dev; a.B = B; a.H = H; a.W = W; a.Cout = Cin; a.taps = taps;
    if (test_conv_launch(h, sc, a, pk, zb.data(), wexp)) return -1;
    OP_EPILOGUE_SYNC()
}

static double* bias_grad_scratch(OpScratch& sc, int C) { return sc.n<double>((size_t)512 * C); }
size_t cddpm_op_bias_grad_scratch(int64_t, int C) { return counted([&](OpScratch& sc) { bias_grad_scratch(sc, C); }); }
int cddpm_op_bias_grad(cddpm_handle h, const float* dy_dev, int64_t npix, int C, float* db_dev, void* stream) {
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, !(!dy_dev || !db_dev || npix < 1 || C % 4 || C > 1024), "cddpm_op_bias_grad: bad arguments")
    OpScratch sc(h, s);
    double* part = bias_grad_scratch(sc, C);
    SCRATCH_CHECK(sc)
    launch_bias_grad(dy_dev, npix, C, db_dev, part, s);
    OP_EPILOGUE()
}

static bool wgrad_shape_ok(int C0, int C1, int upsample, int Cout, int ksize, int B, int H, int W) {
    const int Cin = C0 + C1;
    return !((ksize != 1 && ksize != 3) || C0 <= 0 || C1 < 0 || Cin % 32 || (C1 > 0 && C0 % 32) || Cout <= 0 || Cout % 64 || H < 1 || W < 1 || B < 1 ||
             (upsample && (C1 > 0 || (W & 1) || (H & 1))));
}
static float* wgrad_scratch(OpScratch& sc, const WgradPlan& pl, void*& images) {
    float* part = sc.n<float>(pl.part_floats);
    images = pl.image_units ? sc.get(pl.image_units * 16) : nullptr;
    return part;
}
size_t cddpm_op_conv_wgrad_scratch(int C0, int C1, int upsample, int Cout, int ksize, int B, int H, int W, int precision) {
    if (!wgrad_shape_ok(C0, C1, upsample, Cout, ksize, B, H, W) || (precision != 0 && precision != 16 && precision != 32)) return 0;
    void* images;
    const WgradPlan pl = conv_wgrad_plan(B, H, W, C0 + C1, Cout, ksize * ksize, precision ? precision : train_precision());
    return counted([&](OpScratch& sc) { wgrad_scratch(sc, pl, images); });
}
int cddpm_op_conv_wgrad(cddpm_handle h, const float* x0_dev, int C0, const float* x1_dev, int C1, const float* coef_dev, int silu,
                        int upsample, const float* dy_dev, int Cout, int ksize, float* dw_dev, float* db_dev, int B, int H, int W,
                        void* stream) {
    const int Cin = C0 + C1, taps = ksize * ksize;
    OP_CHECK(wgrad_shape_ok(C0, C1, upsample, Cout, ksize, B, H, W) && !(C1 > 0 && !x1_dev),
             "cddpm_op_conv_wgrad: unsupported shape (k %d, C0 %d, C1 %d, Cout %d, H %d)", ksize, C0, C1, Cout, H)
    OP_PROLOGUE(PC_WGRAD, 2.0 * B * H * W * (double)Cout * Cin * taps, 4.0 * B * (double)H * W * (Cin + Cout), x0_dev && dy_dev && dw_dev,
                "cddpm_op_conv_wgrad: NULL argument")
    const WgradPlan pl = conv_wgrad_plan(B, H, W, Cin, Cout, taps, train_precision());
    OpScratch sc(h, s);
    void* images;
    float* part = wgrad_scratch(sc, pl, images);
    SCRATCH_CHECK(sc)
    launch_conv_wgrad(x0_dev, C0, x1_dev, C1, coef_dev, silu, upsample ? 1 : 0, dy_dev, B, H, W, Cout, taps, pl, part, images, dw_dev, db_dev, s);
    OP_EPILOGUE()
}

static float* attention_backward_scratch(OpScratch& sc, int B, int N, int C) { return sc.n<float>((size_t)B * (C / 64) * N * 2); }
size_t cddpm_op_attention_backward_scratch(int B, int N, int C) { return counted([&](OpScratch& sc) { attention_backward_scratch(sc, B, N, C); }); }
int cddpm_op_attention_backward(cddpm_handle h, const float* qkv_dev, const float* da_dev, float* dqkv_dev, int B, int N, int C,
                                void* stream) {
    OP_CHECK(!(C <= 0 || C % 64 || N < 1 || B < 1), "cddpm_op_attention_backward: C must be a multiple of 64")
    OP_PROLOGUE(PC_ATTN, 0.0, 0.0, qkv_dev && da_dev && dqkv_dev, "cddpm_op_attention_backward: NULL argument")
    OpScratch sc(h, s);
    float* stats = attention_backward_scratch(sc, B, N, C);
    SCRATCH_CHECK(sc)
    launch_attention_backward_flash(qkv_dev, da_dev, dqkv_dev, stats, B, N, C, s);
    OP_EPILOGUE()
}

int cddpm_op_attention_backward_p16(cddpm_handle h, const float* qkv_dev, const float* da_dev, float* dqkv_dev, int B, int N, int C,
                                    void* stream) {
    OP_CHECK(!(C <= 0 || C % 64 || N < 1 || B < 1), "cddpm_op_attention_backward_p16: C must be a multiple of 64")
    OP_PROLOGUE(PC_ATTN, 0.0, 0.0, qkv_dev && da_dev && dqkv_dev, "cddpm_op_attention_backward_p16: NULL argument")
    OpScratch sc(h, s);
    float* stats = attention_backward_scratch(sc, B, N, C);
    SCRATCH_CHECK(sc)
    launch_attention_backward_p16(qkv_dev, da_dev, dqkv_dev, stats, B, N, C, s);
    OP_EPILOGUE()
}

// the h3 backward: the row statistics, then one uint32 per sample for the largest magnitude of its dA
static float* attention_backward_h3_scratch(OpScratch& sc, int B, int N, int C, unsigned*& amax) {
    float* stats = attention_backward_scratch(sc, B, N, C);
    amax = sc.n<unsigned>((size_t)B);
    return stats;
}
size_t cddpm_op_attention_backward_h3_scratch(int B, int N, int C) {
    return counted([&](OpScratch& sc) { unsigned* amax; attention_backward_h3_scratch(sc, B, N, C, amax); });
}
int cddpm_op_attention_backward_h3(cddpm_handle h, const float* qkv_dev, const float* da_dev, float* dqkv_dev, int B, int N, int C,
                                   void* stream) {
    OP_CHECK(!(C <= 0 || C % 64 || N < 1 || B < 1), "cddpm_op_attention_backward_h3: C must be a multiple of 64")
    OP_PROLOGUE(PC_ATTN, 0.0, 0.0, qkv_dev && da_dev && dqkv_dev, "cddpm_op_attention_backward_h3: NULL argument")
    OpScratch sc(h, s);
    unsigned* amax;
    float* stats = attention_backward_h3_scratch(sc, B, N, C, amax);
    SCRATCH_CHECK(sc)
    launch_attention_backward_h3(qkv_dev, da_dev, dqkv_dev, stats, amax, B, N, C, s);
    OP_EPILOGUE()
}

static float* linear_backward_scratch(OpScratch& sc, int M, int N, int K, int silu_in) {
    const size_t nscr = linear_backward_scratch_floats(M, N, K, silu_in);
    return nscr ? sc.n<float>(nscr) : nullptr;
}
size_t cddpm_op_linear_backward_scratch(int M, int N, int K, int silu_in) {
    return counted([&](OpScratch& sc) { linear_backward_scratch(sc, M, N, K, silu_in); });
}
int cddpm_op_linear_backward(cddpm_handle h, const float* x_dev, const float* w_dev, const float* dy_dev, int M, int N, int K,
                             int silu_in, float* dw_dev, float* db_dev, float* dx_dev, void* stream) {
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, M >= 1 && N >= 1 && K >= 1 && x_dev && w_dev && dy_dev && dw_dev, "cddpm_op_linear_backward: bad arguments")
    OpScratch sc(h, s);
    float* a = linear_backward_scratch(sc, M, N, K, silu_in);
    SCRATCH_CHECK(sc)
    launch_linear_backward(x_dev, w_dev, dy_dev, M, N, K, silu_in, a, dw_dev, db_dev, dx_dev, s);
    OP_EPILOGUE()
}

int cddpm_op_linear(cddpm_handle h, const float* x_dev, const float* w_dev, const float* b_dev, int M, int N, int K, int silu_in,
                    float* y_dev, void* stream) {
    // linear_kernel reads x and w in quads of K (float4 at k = 4 * lane while k < K): a K that is no multiple of 4 would read the last quad
    // of a row out of the next row, or past the end of the last one, and leave the rows unaligned
    OP_CHECK(M >= 1 && N >= 1 && K >= 1 && K % 4 == 0, "cddpm_op_linear: unsupported shape (M %d, N %d, K %d: all >= 1, K a multiple of 4)", M, N, K)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, x_dev && w_dev && y_dev && !(((uintptr_t)x_dev | (uintptr_t)w_dev) & 15),
                "cddpm_op_linear: NULL argument, or x_dev / w_dev not 16-byte aligned")
    launch_linear(x_dev, K, w_dev, K, 0, b_dev, y_dev, N, M, N, K, silu_in, s);
    OP_EPILOGUE()
}
int cddpm_op_conv_in1(cddpm_handle h, const float* x_dev, const float* w_dev, const float* b_dev, float* out_dev, int B, int H, int W,
                      int C, void* stream) {
    // conv_in1_kernel walks the B * H * W pixels as one flat 32-bit range
    OP_CHECK(B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1ll << 31) && C >= 64 && C % 64 == 0 && C <= 512,
             "cddpm_op_conv_in1: unsupported shape (B %d, H %d, W %d: all >= 1, B * H * W < 2^31; C %d: a multiple of 64, at most 512)", B, H, W, C)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, x_dev && w_dev && b_dev && out_dev, "cddpm_op_conv_in1: NULL argument")
    launch_conv_in1(x_dev, w_dev, b_dev, out_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
static float* head_scratch(OpScratch& sc, int B, int H, int W) { return sc.n<float>((size_t)B * H * W * 9); }
size_t cddpm_op_head_scratch(int B, int H, int W, int) { return counted([&](OpScratch& sc) { head_scratch(sc, B, H, W); }); }
int cddpm_op_head(cddpm_handle h, const float* x_dev, const float* coef_dev, const float* w9_dev, float bias, const float* bias_dev,
                  float* out_dev, int B, int H, int W, int C, void* stream) {
    // head_dots_kernel keeps 64 pixel rows and the weight image in LDS (head_dots_lds_bytes, kernels.h): C is bounded by a workgroup's LDS
    static_assert(head_dots_lds_bytes(head_max_channels()) <= LDS_BYTES_PER_WORKGROUP && head_dots_lds_bytes(head_max_channels() + 32) > LDS_BYTES_PER_WORKGROUP,
                  "the widest head");
    OP_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0 && C <= head_max_channels(),
             "cddpm_op_head: unsupported shape (B %d, H %d, W %d: all >= 1; C %d: a multiple of 32, at most %d)", B, H, W, C, head_max_channels())
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, x_dev && coef_dev && w9_dev && out_dev, "cddpm_op_head: NULL argument")
    OpScratch sc(h, s);
    float* P = head_scratch(sc, B, H, W);
    SCRATCH_CHECK(sc)
    launch_head_dots(x_dev, coef_dev, w9_dev, P, B, H * W, C, s);
    launch_head_gather(P, bias, bias_dev, out_dev, B, H, W, s);
    OP_EPILOGUE()
}
// the 2x2 resampling operators: a full-resolution [B,H,W,C] tensor next to its [B,H/2,W/2,C] half (an empty grid is a launch error)
static bool resample_shape_ok(int B, int H, int W, int C) { return B >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C >= 4 && C % 4 == 0; }
int cddpm_op_pool_act(cddpm_handle h, const float* x_dev, const float* coef_dev, float* hp_dev, float* xp_dev, int B, int H, int W, int C,
                      void* stream) {
    OP_CHECK(resample_shape_ok(B, H, W, C), "cddpm_op_pool_act: unsupported shape (B %d >= 1; H %d, W %d: even, >= 2; C %d: a multiple of 4, >= 4)", B, H, W, C)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, x_dev && coef_dev && hp_dev && xp_dev, "cddpm_op_pool_act: NULL argument")
    launch_pool_act(x_dev, coef_dev, hp_dev, xp_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
int cddpm_op_unpool2(cddpm_handle h, const float* dyp_dev, float* dx_dev, int B, int H, int W, int C, float scale, int accumulate, void* stream) {
    OP_CHECK(resample_shape_ok(B, H, W, C), "cddpm_op_unpool2: unsupported shape (B %d >= 1; H %d, W %d: even, >= 2; C %d: a multiple of 4, >= 4)", B, H, W, C)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, dyp_dev && dx_dev, "cddpm_op_unpool2: NULL argument")
    launch_unpool2(dyp_dev, dx_dev, B, H, W, C, scale, accumulate, s);
    OP_EPILOGUE()
}
int cddpm_op_sumpool2(cddpm_handle h, const float* dy_dev, float* dxp_dev, int B, int H, int W, int C, int accumulate, void* stream) {
    OP_CHECK(resample_shape_ok(B, H, W, C), "cddpm_op_sumpool2: unsupported shape (B %d >= 1; H %d, W %d: even, >= 2; C %d: a multiple of 4, >= 4)", B, H, W, C)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, dy_dev && dxp_dev, "cddpm_op_sumpool2: NULL argument")
    launch_sumpool2(dy_dev, dxp_dev, B, H, W, C, accumulate, s);
    OP_EPILOGUE()
}
int cddpm_op_add_inplace(cddpm_handle h, float* a_dev, const float* b_dev, int64_t n, void* stream) {
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, a_dev && b_dev && n > 0 && n % 4 == 0, "cddpm_op_add_inplace: bad arguments")
    launch_add_inplace(a_dev, b_dev, n, s);
    OP_EPILOGUE()
}
// nn.Dropout(p) of the ResBlocks' out_layers (OpenAI_Unet.py:255): the mask is drawn from (seed, step, slice0 + b, stream_id), never stored
static bool dropout_shape_ok(int B, int HW, int C) {
    return B >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && (long long)HW * C / 4 <= 0xFFFFFFFFLL && (long long)B * HW * C / 1024 < 0x7FFFFFFFLL;
}
int cddpm_op_act_dropout(cddpm_handle h, const float* x_dev, const float* coef_dev, int silu, float* out_dev, uint64_t seed, uint32_t step,
                         uint64_t slice0, uint32_t stream_id, double p, int B, int HW, int C, void* stream) {
    OP_CHECK(p >= 0.0 && p < 1.0, "cddpm_op_act_dropout: the drop probability must lie in [0, 1), got %g", p)
    OP_CHECK(dropout_shape_ok(B, HW, C) && (coef_dev || !silu), "cddpm_op_act_dropout: unsupported arguments (B %d, HW %d, C %d, silu %d without coefficients)",
             B, HW, C, silu)
    OP_PROLOGUE(PC_OTHER, 0.0, 8.0 * B * (double)HW * C, x_dev && out_dev && !(((uintptr_t)x_dev | (uintptr_t)out_dev | (uintptr_t)coef_dev) & 15),
                "cddpm_op_act_dropout: NULL argument or a pointer that is not 16-byte aligned")
    launch_act_dropout(x_dev, coef_dev, silu, out_dev, seed, step, slice0, stream_id, p, B, HW, C, s);
    OP_EPILOGUE()
}

int cddpm_op_dropout_scale(cddpm_handle h, float* da_dev, uint64_t seed, uint32_t step, uint64_t slice0, uint32_t stream_id, double p, int B, int HW,
                           int C, void* stream) {
    OP_CHECK(p >= 0.0 && p < 1.0, "cddpm_op_dropout_scale: the drop probability must lie in [0, 1), got %g", p)
    OP_CHECK(dropout_shape_ok(B, HW, C), "cddpm_op_dropout_scale: unsupported shape (B %d, HW %d, C %d)", B, HW, C)
    OP_PROLOGUE(PC_OTHER, 0.0, 8.0 * B * (double)HW * C, da_dev && !((uintptr_t)da_dev & 15),
                "cddpm_op_dropout_scale: NULL argument or a pointer that is not 16-byte aligned")
    launch_dropout_scale(da_dev, seed, step, slice0, stream_id, p, B, HW, C, s);
    OP_EPILOGUE()
}

static double* chan_image_corr_scratch(OpScratch& sc, int C) { return sc.n<double>((size_t)256 * C * 9); }
size_t cddpm_op_chan_image_corr_scratch(int, int, int, int C) { return counted([&](OpScratch& sc) { chan_image_corr_scratch(sc, C); }); }
int cddpm_op_chan_image_corr(cddpm_handle h, const float* t_dev, const float* coef_dev, int silu, const float* s_dev, int sign, float* dw_dev,
                             int B, int H, int W, int C, void* stream) {
    OP_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 64 && C % 64 == 0 && (sign == 1 || sign == -1),
             "cddpm_op_chan_image_corr: unsupported arguments (B %d, H %d, W %d: all >= 1; C %d: a multiple of 64; sign %d: +1 or -1)", B, H, W, C, sign)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, t_dev && s_dev && dw_dev, "cddpm_op_chan_image_corr: NULL argument")
    OpScratch sc(h, s);
    double* part = chan_image_corr_scratch(sc, C);
    SCRATCH_CHECK(sc)
    launch_chan_image_corr(t_dev, coef_dev, silu, s_dev, sign, B, H, W, C, part, dw_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_head_dgrad(cddpm_handle h, const float* dout_dev, const float* w9_dev, float* dact_dev, int B, int H, int W, int C, void* stream) {
    OP_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "cddpm_op_head_dgrad: unsupported shape (B %d, H %d, W %d: all >= 1; C %d: a multiple of 4)", B, H, W, C)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, dout_dev && w9_dev && dact_dev, "cddpm_op_head_dgrad: NULL argument")
    launch_head_dgrad(dout_dev, w9_dev, dact_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
int cddpm_op_loss(cddpm_handle h, const float* out_dev, const float* target_dev, const float* w_b_dev, int l2, int B, int HW, float grad_scale,
                  float* dout_dev, float* loss_b_dev, void* stream) {
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, out_dev && target_dev && dout_dev && loss_b_dev && B > 0 && HW > 0, "cddpm_op_loss: bad arguments")
    launch_loss(out_dev, target_dev, w_b_dev, l2, B, HW, grad_scale, nullptr, dout_dev, loss_b_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_loss_scaled(cddpm_handle h, const float* out_dev, const float* target_dev, const float* w_b_dev, int l2, int B, int HW,
                         const int32_t* scaler_dev, float* dout_dev, float* loss_b_dev, void* stream) {
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, out_dev && target_dev && scaler_dev && dout_dev && loss_b_dev && B > 0 && HW > 0, "cddpm_op_loss_scaled: bad arguments")
    launch_loss(out_dev, target_dev, w_b_dev, l2, B, HW, 0.0f, scaler_dev, dout_dev, loss_b_dev, s);
    OP_EPILOGUE()
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int cddpm_op_loss_box(cddpm_handle h, const float* out_dev, const float* x0_dev, const float* noise_dev, const int32_t* box_dev,
                      const float* w_b_dev, int pred_noise, int inpaint, int l2, int B, int H, int W, float grad_scale,
                      const int32_t* scaler_dev, float* dout_dev, float* loss_b_dev, void* stream) {
    OP_CHECK(B > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "cddpm_op_loss_box: bad B/H/W (%d, %d, %d)", B, H, W)
    OP_CHECK(out_dev && x0_dev && box_dev && loss_b_dev && (noise_dev || !pred_noise), "cddpm_op_loss_box: NULL argument")
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0,
                aligned16(box_dev) && (W % 4 || (aligned16(out_dev) && aligned16(x0_dev) && aligned16(noise_dev) && aligned16(dout_dev))),
                "cddpm_op_loss_box: box_dev (and, for W a multiple of 4, every image) must be 16-byte aligned")
    launch_loss_box(out_dev, x0_dev, noise_dev, box_dev, w_b_dev, pred_noise ? 1 : 0, inpaint ? 1 : 0, l2 ? 1 : 0, B, H, W, grad_scale, scaler_dev,
                    dout_dev, loss_b_dev, s);
    OP_EPILOGUE()
}
int cddpm_box_q_sample(cddpm_handle h, const float* x01_dev, const float* noise_dev, const int32_t* t_dev, int t_uniform,
                       const float* sqrt_ac_dev, const float* sqrt_1mac_dev, int T, const int32_t* box_dev, float* out_dev, int S, int N, int H,
                       int W, void* stream) {
    OP_CHECK(S > 0 && N > 0 && N % S == 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "cddpm_box_q_sample: bad S/N/H/W (%d, %d, %d, %d)", S, N, H, W)
    OP_CHECK(T > 0 && (t_dev || (t_uniform >= 0 && t_uniform < T)), "cddpm_box_q_sample: t=%d outside [0, %d)", t_uniform, T)
    OP_CHECK(x01_dev && noise_dev && sqrt_ac_dev && sqrt_1mac_dev && box_dev && out_dev, "cddpm_box_q_sample: NULL argument")
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, aligned16(box_dev) && (W % 4 || (aligned16(x01_dev) && aligned16(noise_dev) && aligned16(out_dev))),
                "cddpm_box_q_sample: box_dev (and, for W a multiple of 4, every image) must be 16-byte aligned")
    launch_box_q_sample(x01_dev, noise_dev, t_dev, t_uniform, sqrt_ac_dev, sqrt_1mac_dev, T, box_dev, out_dev, S, N, H, W, s);
    OP_EPILOGUE()
}
int cddpm_box_stitch(cddpm_handle h, const float* reco_dev, const int32_t* box_dev, const int32_t* cut_dev, int mode, float* out_dev, int S, int K,
                     int H, int W, void* stream) {
    OP_CHECK(S > 0 && K > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "cddpm_box_stitch: bad S/K/H/W (%d, %d, %d, %d)", S, K, H, W)
    OP_CHECK(mode == CDDPM_STITCH_PASTE || mode == CDDPM_STITCH_CUT || mode == CDDPM_STITCH_AVG, "cddpm_box_stitch: unknown mode %d", mode)
    const int32_t* rows = mode == CDDPM_STITCH_CUT ? cut_dev : box_dev;
    OP_CHECK(reco_dev && box_dev && out_dev && rows, "cddpm_box_stitch: NULL argument (CDDPM_STITCH_CUT needs cut_dev)")
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, aligned16(rows) && (W % 4 || (aligned16(reco_dev) && aligned16(out_dev))),
                "cddpm_box_stitch: the box rows (and, for W a multiple of 4, every image) must be 16-byte aligned")
    launch_box_stitch(reco_dev, rows, mode, out_dev, S, K, H, W, s);
    OP_EPILOGUE()
}
int cddpm_op_adam(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2,
                  float eps, int step, float grad_unscale, void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, p_dev && g_dev && m_dev && v_dev && n > 0 && step >= 1, "cddpm_op_adam: bad arguments")
    launch_adam(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, step, grad_unscale, s);
    OP_EPILOGUE()
}
int cddpm_set_train_precision(int bits) {
    if (bits != 16 && bits != 32) return -1;
    return set_train_precision(bits);
}
int cddpm_get_train_precision(void) { return train_precision(); }
int cddpm_op_grad_check(cddpm_handle h, const float* g_dev, int64_t n, int32_t* ctrl_dev, void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, g_dev && ctrl_dev && n > 0 && ((uintptr_t)g_dev & 15) == 0, "cddpm_op_grad_check: bad arguments (g_dev 16-byte aligned)")
    launch_grad_check(g_dev, n, ctrl_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_guard_commit(cddpm_handle h, int32_t* ctrl_dev, float beta1, float beta2, void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, ctrl_dev != nullptr, "cddpm_op_guard_commit: bad arguments")
    launch_guard_commit(ctrl_dev, beta1, beta2, s);
    OP_EPILOGUE()
}
int cddpm_op_adam_guarded(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1,
                          float beta2, float eps, float grad_unscale, const int32_t* ctrl_dev, void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, p_dev && g_dev && m_dev && v_dev && ctrl_dev && n > 0, "cddpm_op_adam_guarded: bad arguments")
    launch_adam_guarded(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, grad_unscale, 0.0f, ctrl_dev, nullptr, s);
    OP_EPILOGUE()
}
int cddpm_op_adam_scaled(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1,
                         float beta2, float eps, float extra_unscale, const int32_t* ctrl_dev, const int32_t* scaler_dev, void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, p_dev && g_dev && m_dev && v_dev && ctrl_dev && scaler_dev && n > 0, "cddpm_op_adam_scaled: bad arguments")
    launch_adam_guarded(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, extra_unscale, 0.0f, ctrl_dev, scaler_dev, s);
    OP_EPILOGUE()
}
static bool power_of_two(float x) {
    int e;
    return std::isfinite(x) && x > 0.0f && std::frexp(x, &e) == 0.5f;
}
int cddpm_op_scaler_update(cddpm_handle h, const int32_t* ctrl_dev, int32_t* scaler_dev, float growth, float backoff, int interval,
                           void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, ctrl_dev && scaler_dev && power_of_two(growth) && growth > 1.0f && power_of_two(backoff) && backoff < 1.0f && interval >= 1,
                "cddpm_op_scaler_update: bad arguments (growth > 1 and backoff < 1 powers of two, interval >= 1)")
    launch_scaler_update(ctrl_dev, scaler_dev, growth, backoff, interval, s);
    OP_EPILOGUE()
}

// ---- training-mode operators of the context encoder (encoder_train.hip): NHWC fp32 device tensors ---------------------------------------
int cddpm_op_enc_pack_w(cddpm_handle h, const float* w_dev, int Cout, int Cin, int K, float* wf_dev, float* wd_dev, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, w_dev && wf_dev && Cout > 0 && Cin > 0 && (K == 1 || K == 3), "cddpm_op_enc_pack_w: bad arguments")
    launch_enc_pack_w(w_dev, Cout, Cin, K * K, wf_dev, wd_dev, s);
    OP_EPILOGUE()
}
static bool enc_conv_shape_ok(int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed) {
    return B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (K == 1 || K == 3) && (stride == 1 || stride == 2) &&
           (transposed ? (Cout % 16 == 0 && Cin % 64 == 0) : (Cin % 16 == 0 && Cout % 64 == 0));
}
static float* enc_conv_scratch(OpScratch& sc, int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed) {
    const int Z = enc_conv_split(B, H, W, Cin, Cout, K, stride, transposed);      // split-K planes (1: the kernel writes dst itself)
    if (Z == 1) return nullptr;
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    return sc.n<float>((size_t)Z * B * (transposed ? (size_t)H * W * Cin : (size_t)Ho * Wo * Cout));
}
size_t cddpm_op_enc_conv_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed) {
    if (!enc_conv_shape_ok(B, H, W, Cin, Cout, K, stride, transposed)) return 0;
    return counted([&](OpScratch& sc) { enc_conv_scratch(sc, B, H, W, Cin, Cout, K, stride, transposed); });
}
int cddpm_op_enc_conv(cddpm_handle h, const float* src_dev, const float* w_img_dev, float* dst_dev, int B, int H, int W, int Cin, int Cout, int K,
                      int stride, int transposed, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0,
                src_dev && w_img_dev && dst_dev && enc_conv_shape_ok(B, H, W, Cin, Cout, K, stride, transposed),
                "cddpm_op_enc_conv: unsupported shape (contraction channels a multiple of 16, produced channels of 64; K 1|3, stride 1|2)")
    OpScratch sc(h, s);
    float* part = enc_conv_scratch(sc, B, H, W, Cin, Cout, K, stride, transposed);
    SCRATCH_CHECK(sc)
    launch_enc_conv(src_dev, w_img_dev, dst_dev, B, H, W, Cin, Cout, K, stride, transposed, part, s);
    OP_EPILOGUE()
}
static bool enc_wgrad_shape_ok(int B, int H, int W, int Cin, int Cout, int K, int stride) {
    return B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0 && (K == 1 || K == 3) && (stride == 1 || stride == 2);
}
static float* enc_wgrad_scratch(OpScratch& sc, int B, int H, int W, int Cin, int Cout, int K, int stride, int& P) {
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    P = enc_wgrad_parts(B, Ho, Wo, Cin, Cout, K);
    return sc.n<float>((size_t)P * K * K * Cin * Cout);
}
size_t cddpm_op_enc_conv_wgrad_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride) {
    if (!enc_wgrad_shape_ok(B, H, W, Cin, Cout, K, stride)) return 0;
    int P;
    return counted([&](OpScratch& sc) { enc_wgrad_scratch(sc, B, H, W, Cin, Cout, K, stride, P); });
}
int cddpm_op_enc_conv_wgrad(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, int Cin, int Cout, int K,
                            int stride, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && dz_dev && dw_dev && enc_wgrad_shape_ok(B, H, W, Cin, Cout, K, stride), "cddpm_op_enc_conv_wgrad: unsupported shape")
    OpScratch sc(h, s);
    int P;
    float* part = enc_wgrad_scratch(sc, B, H, W, Cin, Cout, K, stride, P);
    SCRATCH_CHECK(sc)
    launch_enc_wgrad(x_dev, dz_dev, part, P, dw_dev, B, H, W, Cin, Cout, K, stride, s);
    OP_EPILOGUE()
}
// the same three operators in precision 16 (encoder_train_p16.hip): what configs/trainer/default.yaml:7 makes of self.encoder's convolutions
// (src/models/DDPM_2D.py:114-135) -- fp16 operands rounded to nearest, fp32 accumulation, fp32 NHWC results
int cddpm_op_enc_pack_w_p16(cddpm_handle h, const float* w_dev, int Cout, int Cin, int K, void* wf16_dev, void* wd16_dev, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, w_dev && (wf16_dev || wd16_dev) && Cout > 0 && Cout % 64 == 0 && Cin > 0 && Cin % 64 == 0 && (K == 1 || K == 3),
                "cddpm_op_enc_pack_w_p16: bad arguments (Cin, Cout multiples of 64; K 1|3)")
    launch_enc_pack_w_p16(w_dev, Cout, Cin, K * K, wf16_dev, wd16_dev, s);
    OP_EPILOGUE()
}
static bool enc_conv_p16_shape_ok(int B, int H, int W, int Cin, int Cout, int K, int stride) {
    return B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 64 == 0 && Cin <= 2048 && Cout > 0 && Cout % 64 == 0 && Cout <= 2048 && (K == 1 || K == 3) &&
           (stride == 1 || stride == 2);
}
static float* enc_conv_p16_scratch(OpScratch& sc, int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed) {
    const int Z = enc_conv_p16_split(B, H, W, Cin, Cout, K, stride, transposed);      // split-K planes (1: the kernel writes dst itself)
    if (Z == 1) return nullptr;
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    return sc.n<float>((size_t)Z * B * (transposed ? (size_t)H * W * Cin : (size_t)Ho * Wo * Cout));
}
size_t cddpm_op_enc_conv_p16_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed) {
    if (!enc_conv_p16_shape_ok(B, H, W, Cin, Cout, K, stride)) return 0;
    return counted([&](OpScratch& sc) { enc_conv_p16_scratch(sc, B, H, W, Cin, Cout, K, stride, transposed ? 1 : 0); });
}
int cddpm_op_enc_conv_p16(cddpm_handle h, const float* src_dev, const void* w_img16_dev, float* dst_dev, int B, int H, int W, int Cin, int Cout,
                          int K, int stride, int transposed, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, src_dev && w_img16_dev && dst_dev && enc_conv_p16_shape_ok(B, H, W, Cin, Cout, K, stride),
                "cddpm_op_enc_conv_p16: unsupported shape (Cin, Cout multiples of 64 up to 2048; K 1|3, stride 1|2)")
    OpScratch sc(h, s);
    float* part = enc_conv_p16_scratch(sc, B, H, W, Cin, Cout, K, stride, transposed ? 1 : 0);
    SCRATCH_CHECK(sc)
    launch_enc_conv_p16(src_dev, w_img16_dev, dst_dev, B, H, W, Cin, Cout, K, stride, transposed ? 1 : 0, part, s);
    OP_EPILOGUE()
}
static float* enc_wgrad_p16_scratch(OpScratch& sc, int B, int H, int W, int Cin, int Cout, int K, int stride, int& P) {
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    P = enc_wgrad_p16_parts(B, Ho, Wo, Cin, Cout, K);
    if (K == 1 && P == 1) return nullptr;             // one pixel range of a 1x1: the kernel writes dw itself
    return sc.n<float>((size_t)P * K * K * Cin * Cout);
}
size_t cddpm_op_enc_conv_wgrad_p16_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride) {
    if (!enc_conv_p16_shape_ok(B, H, W, Cin, Cout, K, stride)) return 0;
    int P;
    return counted([&](OpScratch& sc) { enc_wgrad_p16_scratch(sc, B, H, W, Cin, Cout, K, stride, P); });
}
int cddpm_op_enc_conv_wgrad_p16(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, int Cin, int Cout,
                                int K, int stride, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && dz_dev && dw_dev && enc_conv_p16_shape_ok(B, H, W, Cin, Cout, K, stride),
                "cddpm_op_enc_conv_wgrad_p16: unsupported shape (Cin, Cout multiples of 64 up to 2048; K 1|3, stride 1|2)")
    OpScratch sc(h, s);
    int P;
    float* part = enc_wgrad_p16_scratch(sc, B, H, W, Cin, Cout, K, stride, P);
    SCRATCH_CHECK(sc)
    launch_enc_wgrad_p16(x_dev, dz_dev, part, P, dw_dev, B, H, W, Cin, Cout, K, stride, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_stem(cddpm_handle h, const float* x_dev, const float* w_dev, float* z_dev, int B, int H, int W, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && w_dev && z_dev && B > 0 && H > 0 && W > 0, "cddpm_op_enc_stem: bad arguments")
    launch_enc_stem_fwd(x_dev, w_dev, z_dev, B, H, W, s);
    OP_EPILOGUE()
}
static double* enc_stem_wgrad_scratch(OpScratch& sc) { return sc.n<double>((size_t)32 * 49 * 64); }
size_t cddpm_op_enc_stem_wgrad_scratch(int, int, int) { return counted([](OpScratch& sc) { enc_stem_wgrad_scratch(sc); }); }
int cddpm_op_enc_stem_wgrad(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && dz_dev && dw_dev && B > 0 && H > 0 && W > 0, "cddpm_op_enc_stem_wgrad: bad arguments")
    OpScratch sc(h, s);
    double* part = enc_stem_wgrad_scratch(sc);
    SCRATCH_CHECK(sc)
    launch_enc_stem_wgrad(x_dev, dz_dev, part, dw_dev, B, H, W, s);
    OP_EPILOGUE()
}
// BatchNorm of the dense ResNet-50: batchnorm_train.hip without a mask, on this entry's own plan -- N / 256 pixel chunks (it fixes the order
// of the fp64 sums and the grid), 2 planes per chunk in the backward (no inactive pixels, no dfill), C a multiple of 64, and N = 1 accepted
// (the biased variance folds into run_var: no status word)
static int enc_bn_chunks(int64_t N) {
    int64_t n = N / 256;            // >= 16 pixels per pixel lane of a chunk; the folds read the chunks serially
    if (n > 32) n = 32;
    return n < 1 ? 1 : (int)n;
}
static BnShape enc_bn_shape(int64_t N, int HW, int C) {
    BnShape g;
    g.N = N; g.HW = HW; g.C = C; g.active = nullptr; g.f = 1; g.H = g.W = 0;
    return g;
}
static double* enc_bn_scratch(OpScratch& sc, int64_t N, int C, bool backward, float*& k) {
    double* part = sc.n<double>((size_t)enc_bn_chunks(N) * 2 * C);
    k = backward ? sc.n<float>((size_t)2 * C) : nullptr;
    return part;
}
size_t cddpm_op_enc_bn_forward_scratch(int64_t N, int, int C) { float* k; return counted([&](OpScratch& sc) { enc_bn_scratch(sc, N, C, false, k); }); }
size_t cddpm_op_enc_bn_backward_scratch(int64_t N, int, int C) { float* k; return counted([&](OpScratch& sc) { enc_bn_scratch(sc, N, C, true, k); }); }
int cddpm_op_enc_bn_forward(cddpm_handle h, const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* sample_scale_dev,
                            const float* res_dev, int relu, float eps, float momentum, float* run_mean_dev, float* run_var_dev, float* mean_rstd_dev,
                            float* y_dev, int64_t N, int HW, int C, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, z_dev && gamma_dev && beta_dev && mean_rstd_dev && y_dev && N > 0 && HW > 0 && C > 0 && C % 64 == 0 && (!run_mean_dev == !run_var_dev),
                "cddpm_op_enc_bn_forward: bad arguments (C a multiple of 64)")
    OpScratch sc(h, s);
    float* k;
    double* part = enc_bn_scratch(sc, N, C, false, k);
    SCRATCH_CHECK(sc)
    const BnShape g = enc_bn_shape(N, HW, C);
    launch_bn_train_stats(g, z_dev, enc_bn_chunks(N), eps, momentum, run_mean_dev, run_var_dev, mean_rstd_dev, part, nullptr, s);
    launch_bn_train_act(g, z_dev, mean_rstd_dev, gamma_dev, beta_dev, sample_scale_dev, res_dev, nullptr, relu != 0, y_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_bn_backward(cddpm_handle h, const float* z_dev, const float* y_dev, const float* dy_dev, const float* mean_rstd_dev,
                             const float* gamma_dev, const float* sample_scale_dev, int relu, float* dz_dev, float* dres_dev, float* dgamma_dev,
                             float* dbeta_dev, int64_t N, int HW, int C, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, z_dev && dy_dev && mean_rstd_dev && gamma_dev && dz_dev && dgamma_dev && dbeta_dev && (!relu || y_dev) && N > 0 && HW > 0 && C > 0 &&
                    C % 64 == 0, "cddpm_op_enc_bn_backward: bad arguments (C a multiple of 64)")
    OpScratch sc(h, s);
    float* k;
    double* part = enc_bn_scratch(sc, N, C, true, k);
    SCRATCH_CHECK(sc)
    launch_bn_train_backward(enc_bn_shape(N, HW, C), z_dev, y_dev, dy_dev, mean_rstd_dev, gamma_dev, sample_scale_dev, relu != 0, 1, enc_bn_chunks(N), 2,
                             dz_dev, dres_dev, dgamma_dev, dbeta_dev, nullptr, k, part, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_maxpool(cddpm_handle h, const float* x_dev, float* y_dev, int B, int H, int W, int C, int backward, const float* dy_dev, float* dx_dev,
                         void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (backward ? (dy_dev && dx_dev) : (y_dev != nullptr)),
                "cddpm_op_enc_maxpool: bad arguments")
    if (backward) launch_enc_maxpool_backward(x_dev, dy_dev, dx_dev, B, H, W, C, s);
    else launch_enc_maxpool(x_dev, y_dev, B, H, W, C, s);
    OP_EPILOGUE()
}
int cddpm_op_enc_avgpool(cddpm_handle h, const float* x_dev, float* g_dev, int B, int HW, int C, int backward, void* stream) {
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && g_dev && B > 0 && HW > 0 && C > 0, "cddpm_op_enc_avgpool: bad arguments")
    if (backward) launch_enc_avgpool_backward(x_dev /* dL/dg [B][C] */, g_dev /* dL/dx [B][HW][C] */, B, HW, C, s);
    else launch_enc_avgpool(x_dev, g_dev, B, HW, C, s);
    OP_EPILOGUE()
}

// the statistics records of x (swept here when the call brings none), the parameter vectors when they come from the host, planes,
// per-(sample, channel) sums, fp64 partial sums
static void gn_silu_backward_scratch(OpScratch& sc, bool has_rec, int B, int HW, int C, const float*& gamma, const float*& beta, float*& rec,
                                     float*& planes, float*& out_bc, double*& part) {
    const int ns = gn_nsplit(B, HW);
    rec = has_rec ? nullptr : sc.n<float>((size_t)B * ns * C * 2);
    gamma = sc.param(gamma, C);
    beta = sc.param(beta, C);
    planes = sc.n<float>((size_t)4 * B * C);
    out_bc = sc.n<float>((size_t)4 * B * C);
    part = sc.n<double>((size_t)B * ns * C * 2);
}
size_t cddpm_op_gn_silu_backward_scratch(int has_rec, int B, int HW, int C) {
    const float *g = nullptr, *bt = nullptr;
    float *rec, *planes, *out_bc;
    double* part;
    return counted([&](OpScratch& sc) { gn_silu_backward_scratch(sc, has_rec != 0, B, HW, C, g, bt, rec, planes, out_bc, part); });
}
int cddpm_op_gn_silu_backward(cddpm_handle h, const float* x_dev, const float* x1_dev, int C1, const float* da_dev, const float* gamma_host,
                              const float* beta_host, const float* film_dev, int silu, float* dx_dev, float* dx1_dev, float* dgamma_dev,
                              float* dbeta_dev, float* dfilm_dev, const float* rec_dev, int nrec, const float* add_dev, int B, int HW, int C,
                              void* stream) {
    OP_CHECK(!(C % 32 || C <= 0 || C > 1024 || B < 1 || HW < 1 || (rec_dev && nrec < 1) || C1 < 0 || C1 % 4 || C1 >= C ||
               (C1 > 0 && (!x1_dev || !dx1_dev || !rec_dev))),
             "cddpm_op_gn_silu_backward: unsupported shape (C %d, C1 %d; a two-source input needs its statistics records)", C, C1)
    OP_PROLOGUE(PC_GNBWD, 0.0, 12.0 * B * (double)HW * C,      // reads x and da, writes dx
                !(!x_dev || !da_dev || !gamma_host || !beta_host || !dx_dev || !dgamma_dev || !dbeta_dev || (film_dev && !dfilm_dev)),
                "cddpm_op_gn_silu_backward: NULL argument")
    const int ns = gn_nsplit(B, HW);
    OpScratch sc(h, s);
    const float *g = gamma_host, *bt = beta_host;
    float *rec, *planes, *out_bc;
    double* part;
    gn_silu_backward_scratch(sc, rec_dev != nullptr, B, HW, C, g, bt, rec, planes, out_bc, part);
    SCRATCH_CHECK(sc)
    if (!rec_dev) launch_gn_partial(x_dev, C, B, HW, ns, rec, s);      // statistics records of x: given (kept from the forward pass) or swept here
    launch_gn_bwd_planes(rec_dev ? rec_dev : rec, rec_dev ? nrec : ns, g, bt, film_dev, B, C, HW, planes, s);
    launch_gn_silu_backward(x_dev, C1 ? x1_dev : nullptr, C - C1, C1 ? dx1_dev : nullptr, da_dev, planes, g, bt, film_dev, silu, B, C, HW, ns, part,
                            out_bc, dx_dev, dgamma_dev, dbeta_dev, dfilm_dev, add_dev, s);
    OP_EPILOGUE()
}

int cddpm_stat_records(int H, int W, int kind) {
    if (H < 1 || W < 1) return -1;
    if (kind == 0) return conv_stat_records(H, W);
    if (kind == 1) return conv_stat_records_up2(H, W);
    if (kind == 2) return gn_nsplit(1, H * W);
    return -1;
}

int cddpm_conv_ksplit_plan(int family, long long workgroups_at_max, int Cin, int Cskip, int taps, int* kbound_out) {
    if (!kbound_out || family < 0 || family > 2 || workgroups_at_max < 1 || Cin <= 0 || Cin % 32 || Cskip < 0 || Cskip % 32 ||
        (Cin + Cskip) / 32 > 32767 || (taps != 1 && taps != 4 && taps != 9))
        return -1;
    short kb[CDDPM_MAX_KSPLIT + 1] = {0};
    const int S = ksplit_rule(family, workgroups_at_max, Cin, Cskip, taps, kb);
    if (S == 1) kb[1] = (short)((Cin + Cskip) / 32);      // unsplit: the one range is the whole K loop
    for (int j = 0; j <= CDDPM_MAX_KSPLIT; ++j) kbound_out[j] = j <= S ? kb[j] : 0;
    return S;
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

int cddpm_op_attention_p16(cddpm_handle h, const float* qkv_dev, float* out_dev, int B, int N, int C, void* stream) {
    OP_CHECK(!(C <= 0 || C % 64 || N < 1 || B < 1), "cddpm_op_attention_p16: C must be a multiple of 64")
    OP_PROLOGUE(PC_ATTN, 0.0, 0.0, qkv_dev && out_dev, "cddpm_op_attention_p16: NULL argument")
    launch_attention_p16(qkv_dev, out_dev, B, N, C, s);
    OP_EPILOGUE()
}

int cddpm_op_attention_h3(cddpm_handle h, const float* qkv_dev, float* out_dev, int B, int N, int C, void* stream) {
    OP_CHECK(!(C <= 0 || C % 64 || N < 1 || B < 1), "cddpm_op_attention_h3: C must be a multiple of 64")
    OP_PROLOGUE(PC_ATTN, 0.0, 0.0, qkv_dev && out_dev, "cddpm_op_attention_h3: NULL argument")
    launch_attention_h3(qkv_dev, out_dev, B, N, C, s);
    OP_EPILOGUE()
}

int cddpm_op_attention(cddpm_handle h, const float* qkv_dev, float* out_dev, int B, int N, int C, void* stream) {
    OP_CHECK(!(C <= 0 || C % 64 || N < 1 || B < 1), "cddpm_op_attention: C must be a multiple of 64")
    OP_PROLOGUE(PC_ATTN, 0.0, 0.0, qkv_dev && out_dev, "cddpm_op_attention: NULL argument")
    launch_attention(qkv_dev, out_dev, B, N, C, s);
    OP_EPILOGUE()
}

// ---- SparK masked pre-training (spark_train.hip; reference src/models/Spark_2D.py, src/models/modules/spark/): NHWC fp32 device tensors ----
static bool spark_aligned(std::initializer_list<const void*> ps) {
    uintptr_t u = 0;
    for (const void* p : ps) u |= (uintptr_t)p;
    return (u & 15) == 0;
}
static bool spark_bn_shape_ok(int64_t N, int HW, int C, bool masked, int f, int H, int W) {
    return N > 0 && N <= 0x7FFFFFFF && H > 0 && W > 0 && HW > 0 && (int64_t)H * W == HW && N % HW == 0 && C >= 4 && C % 4 == 0 && C <= 65536 &&
           (!masked || (f >= 1 && H % f == 0 && W % f == 0 && (N / HW) * f * f <= 0x7FFFFFFF));
}
// sparse / dense BatchNorm of SparK pre-training: batchnorm_train.hip on this entry's own plan -- N C / 16384 pixel chunks, 3 planes per chunk
// in the backward (the third: the sums over inactive pixels, dfill), C a multiple of 4, and fewer than two values per channel reported
// through the status words with nothing written
static int spark_bn_chunks(int64_t N, int C) {
    int64_t n = N * C / 16384;            // >= 16 K elements per chunk; the folds read the chunks serially
    if (n > 128) n = 128;
    return n < 1 ? 1 : (int)n;
}
static BnShape spark_bn_shape(int64_t N, int HW, int C, const uint8_t* active, int f, int H, int W) {
    BnShape g;
    g.N = N; g.HW = HW; g.C = C; g.active = active; g.f = f; g.H = H; g.W = W;
    return g;
}
static double* spark_bn_scratch(OpScratch& sc, int64_t N, int C, bool backward, float*& k, int*& status) {
    double* part = sc.n<double>((size_t)spark_bn_chunks(N, C) * (backward ? 3 : 2) * C);
    k = backward ? sc.n<float>((size_t)2 * C) : nullptr;
    status = backward ? nullptr : sc.n<int>(2);
    return part;
}
size_t cddpm_op_spark_bn_forward_scratch(int64_t N, int HW, int C) {
    if (N <= 0 || N > 0x7FFFFFFF || HW <= 0 || N % HW || C < 4 || C % 4 || C > 65536) return 0;
    float* k; int* st;
    return counted([&](OpScratch& sc) { spark_bn_scratch(sc, N, C, false, k, st); });
}
size_t cddpm_op_spark_bn_backward_scratch(int64_t N, int HW, int C) {
    if (N <= 0 || N > 0x7FFFFFFF || HW <= 0 || N % HW || C < 4 || C % 4 || C > 65536) return 0;
    float* k; int* st;
    return counted([&](OpScratch& sc) { spark_bn_scratch(sc, N, C, true, k, st); });
}
int cddpm_op_spark_bn_forward(cddpm_handle h, const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* sample_scale_dev,
                              const float* res_dev, int act, float eps, float momentum, float* run_mean_dev, float* run_var_dev, float* mean_rstd_dev,
                              float* y_dev, int64_t N, int HW, int C, const uint8_t* active_dev, int f, int H, int W, const float* fill_dev, int training,
                              void* stream) {
    OP_CHECK(spark_bn_shape_ok(N, HW, C, active_dev != nullptr, f, H, W) && act >= 0 && act <= 2,
             "cddpm_op_spark_bn_forward: unsupported arguments (N %lld = B H W, HW %d = H %d x W %d, C %d a multiple of 4, f %d dividing H and W, act %d in 0..2)",
             (long long)N, HW, H, W, C, f, act)
    OP_CHECK(training ? (!run_mean_dev == !run_var_dev) : (run_mean_dev && run_var_dev),
             "cddpm_op_spark_bn_forward: running statistics come as a pair, and evaluation mode (training = 0) needs them")
    OP_CHECK(!training || active_dev || N >= 2, "cddpm_op_spark_bn_forward: training-mode BatchNorm needs more than one value per channel (N = %lld)", (long long)N)
    OP_PROLOGUE(PC_ENC, 0.0, 0.0,
                z_dev && gamma_dev && beta_dev && mean_rstd_dev && y_dev && spark_aligned({z_dev, gamma_dev, beta_dev, res_dev, mean_rstd_dev, y_dev, fill_dev}),
                "cddpm_op_spark_bn_forward: NULL argument or a tensor that is not 16-byte aligned")
    const BnShape g = spark_bn_shape(N, HW, C, active_dev, f, H, W);
    OpScratch sc(h, s);
    float* k; int* status;
    double* part = spark_bn_scratch(sc, N, C, false, k, status);
    SCRATCH_CHECK(sc)
    if (training) {
        launch_bn_train_stats(g, z_dev, spark_bn_chunks(N, C), eps, momentum, run_mean_dev, run_var_dev, mean_rstd_dev, part, status, s);
        if (active_dev) {        // n_act is the device's count: read its verdict back before anything is written from statistics of one row
            int st[2] = {0, 0};
            HIPCHECK(h, hipMemcpyAsync(st, status, sizeof st, hipMemcpyDeviceToHost, s));
            HIPCHECK(h, hipStreamSynchronize(s));
            if (st[0])
                return fail(h, "cddpm_op_spark_bn_forward: %d active pixel(s): training-mode BatchNorm needs more than one value per channel "
                               "(torch's BatchNorm1d raises here)", st[1]);
        }
    } else {
        launch_bn_eval_stats(run_mean_dev, run_var_dev, eps, C, mean_rstd_dev, s);
    }
    launch_bn_train_act(g, z_dev, mean_rstd_dev, gamma_dev, beta_dev, sample_scale_dev, res_dev, fill_dev, act, y_dev, s);
    OP_EPILOGUE()
}
int cddpm_op_spark_bn_backward(cddpm_handle h, const float* z_dev, const float* y_dev, const float* dy_dev, const float* mean_rstd_dev,
                               const float* gamma_dev, const float* sample_scale_dev, int act, float* dz_dev, float* dres_dev, float* dgamma_dev,
                               float* dbeta_dev, int64_t N, int HW, int C, const uint8_t* active_dev, int f, int H, int W, float* dfill_dev, int training,
                               void* stream) {
    OP_CHECK(spark_bn_shape_ok(N, HW, C, active_dev != nullptr, f, H, W) && act >= 0 && act <= 2,
             "cddpm_op_spark_bn_backward: unsupported arguments (N %lld = B H W, HW %d = H %d x W %d, C %d a multiple of 4, f %d dividing H and W, act %d in 0..2)",
             (long long)N, HW, H, W, C, f, act)
    OP_PROLOGUE(PC_ENC, 0.0, 0.0,
                z_dev && dy_dev && mean_rstd_dev && gamma_dev && dz_dev && dgamma_dev && dbeta_dev && (!act || y_dev) &&
                    spark_aligned({z_dev, y_dev, dy_dev, mean_rstd_dev, gamma_dev, dz_dev, dres_dev}),
                "cddpm_op_spark_bn_backward: NULL argument (y_dev is needed with an activation) or a tensor that is not 16-byte aligned")
    OpScratch sc(h, s);
    float* k; int* status;
    double* part = spark_bn_scratch(sc, N, C, true, k, status);
    SCRATCH_CHECK(sc)
    launch_bn_train_backward(spark_bn_shape(N, HW, C, active_dev, f, H, W), z_dev, y_dev, dy_dev, mean_rstd_dev, gamma_dev, sample_scale_dev, act, training,
                             spark_bn_chunks(N, C), 3, dz_dev, dres_dev, dgamma_dev, dbeta_dev, dfill_dev, k, part, s);
    OP_EPILOGUE()
}
int cddpm_op_spark_mask_mul(cddpm_handle h, const float* x_dev, const uint8_t* active_dev, float* y_dev, int B, int H, int W, int C, int f, void* stream) {
    OP_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1 && f >= 1 && H % f == 0 && W % f == 0 && (int64_t)B * H * W <= 0x7FFFFFFF,
             "cddpm_op_spark_mask_mul: unsupported shape (B %d, H %d, W %d, C %d, f %d dividing H and W)", B, H, W, C, f)
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && active_dev && y_dev, "cddpm_op_spark_mask_mul: NULL argument")
    launch_spark_mask_mul(x_dev, active_dev, y_dev, B, H, W, C, f, s);
    OP_EPILOGUE()
}

// Conv2d (K 1 | 3, stride 1, pad K / 2) and ConvTranspose2d (K 4, stride 2, pad 1), forward and input gradient, as one gather over the layer's
// own weight tensor. H, W: the LAYER's input size (a ConvTranspose2d's output is 2H x 2W)
static bool spark_conv_geom(int B, int H, int W, int Cin, int Cout, int K, int tconv, int backward, SparkConv& a) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || Cin > 65536 || Cout > 65536 || (int64_t)B * H * W * 4 > 0x7FFFFFFF) return false;
    if (tconv ? K != 4 : (K != 1 && K != 3)) return false;
    const long long KK = (long long)K * K;
    a.B = B; a.K = K; a.stride = tconv ? 2 : 1; a.pad = tconv ? 1 : K / 2;
    const int Ho = tconv ? 2 * H : H, Wo = tconv ? 2 * W : W;
    if (!backward) { a.Hs = H; a.Ws = W; a.Hd = Ho; a.Wd = Wo; a.Cs = Cin; a.Cd = Cout; }
    else { a.Hs = Ho; a.Ws = Wo; a.Hd = H; a.Wd = W; a.Cs = Cout; a.Cd = Cin; }
    a.form = (tconv != 0) == (backward != 0) ? 0 : 1;
    // Conv2d [Cout][Cin][K][K]; ConvTranspose2d [Cin][Cout][K][K]
    const long long s_in = tconv ? Cout * KK : KK, s_out = tconv ? KK : Cin * KK;
    a.wsd = backward ? s_in : s_out; a.wss = backward ? s_out : s_in;
    return true;
}
static float* spark_conv_scratch(OpScratch& sc, const SparkConv& a) {
    const long long M = (long long)a.B * a.Hd * a.Wd;
    const int Z = spark_conv_split(M, a.Cd, a.Cs, a.K);
    return Z == 1 ? nullptr : sc.n<float>((size_t)Z * M * a.Cd);
}
size_t cddpm_op_spark_conv_scratch(int B, int H, int W, int Cin, int Cout, int K, int transposed_conv, int backward) {
    SparkConv a;
    if (!spark_conv_geom(B, H, W, Cin, Cout, K, transposed_conv, backward, a)) return 0;
    return counted([&](OpScratch& sc) { spark_conv_scratch(sc, a); });
}
int cddpm_op_spark_conv(cddpm_handle h, const float* src_dev, const float* w_dev, const float* bias_dev, float* dst_dev, int B, int H, int W, int Cin,
                        int Cout, int K, int transposed_conv, int backward, void* stream) {
    SparkConv a;
    OP_CHECK(spark_conv_geom(B, H, W, Cin, Cout, K, transposed_conv, backward, a),
             "cddpm_op_spark_conv: unsupported shape (B %d, H %d, W %d, Cin %d, Cout %d; K %d: 1 | 3 for a convolution, 4 for a transposed one)", B, H, W, Cin,
             Cout, K)
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, src_dev && w_dev && dst_dev && src_dev != dst_dev && spark_aligned({src_dev, dst_dev}),
                "cddpm_op_spark_conv: NULL argument, src = dst, or a tensor that is not 16-byte aligned")
    OpScratch sc(h, s);
    a.part = spark_conv_scratch(sc, a);
    SCRATCH_CHECK(sc)
    a.src = src_dev; a.w = w_dev; a.bias = bias_dev; a.dst = dst_dev;
    launch_spark_conv(a, s);
    OP_EPILOGUE()
}
static bool spark_wgrad_geom(int B, int H, int W, int Cin, int Cout, int K, int tconv, SparkWgrad& a) {
    SparkConv c;
    if (!spark_conv_geom(B, H, W, Cin, Cout, K, tconv, 0, c)) return false;
    a.B = B; a.Hq = H; a.Wq = W; a.Hg = tconv ? 2 * H : H; a.Wg = tconv ? 2 * W : W; a.K = K; a.stride = c.stride; a.pad = c.pad;
    a.Cd = tconv ? Cin : Cout; a.Cg = tconv ? Cout : Cin;
    a.P = spark_wgrad_parts((long long)B * H * W, a.Cd, a.Cg, K);
    return true;
}
static float* spark_wgrad_scratch(OpScratch& sc, const SparkWgrad& a, bool has_db, int Cout, long long Mdy, double*& bpart) {
    float* part = sc.n<float>((size_t)a.P * a.Cd * a.Cg * a.K * a.K);
    bpart = has_db ? sc.n<double>((size_t)spark_chan_sum_chunks(Mdy, Cout) * Cout) : nullptr;
    return part;
}
size_t cddpm_op_spark_conv_wgrad_scratch(int B, int H, int W, int Cin, int Cout, int K, int transposed_conv, int has_db) {
    SparkWgrad a;
    if (!spark_wgrad_geom(B, H, W, Cin, Cout, K, transposed_conv, a) || (has_db && Cout > 256)) return 0;
    double* bpart;
    return counted([&](OpScratch& sc) { spark_wgrad_scratch(sc, a, has_db != 0, Cout, (long long)B * a.Hg * a.Wg, bpart); });
}
int cddpm_op_spark_conv_wgrad(cddpm_handle h, const float* x_dev, const float* dy_dev, float* dw_dev, float* db_dev, int B, int H, int W, int Cin, int Cout,
                              int K, int transposed_conv, void* stream) {
    SparkWgrad a;
    OP_CHECK(spark_wgrad_geom(B, H, W, Cin, Cout, K, transposed_conv, a) && (!db_dev || Cout <= 256),
             "cddpm_op_spark_conv_wgrad: unsupported shape (B %d, H %d, W %d, Cin %d, Cout %d (<= 256 with a bias gradient); K %d: 1 | 3, or 4 transposed)", B,
             H, W, Cin, Cout, K)
    OP_PROLOGUE(PC_ENC, 0.0, 0.0, x_dev && dy_dev && dw_dev && spark_aligned({x_dev, dy_dev}),
                "cddpm_op_spark_conv_wgrad: NULL argument or a tensor that is not 16-byte aligned")
    OpScratch sc(h, s);
    double* bpart;
    const long long Mdy = (long long)B * a.Hg * a.Wg;          // pixels of dy: the layer's output
    a.part = spark_wgrad_scratch(sc, a, db_dev != nullptr, Cout, Mdy, bpart);
    SCRATCH_CHECK(sc)
    a.d = transposed_conv ? x_dev : dy_dev; a.g = transposed_conv ? dy_dev : x_dev;
    launch_spark_wgrad(a, dw_dev, s);
    if (db_dev) launch_spark_chan_sum(dy_dev, Mdy, Cout, bpart, db_dev, s);
    OP_EPILOGUE()
}
static bool spark_loss_shape_ok(int B, int H, int W, int f) {
    return B >= 1 && H >= 1 && W >= 1 && f >= 1 && H % f == 0 && W % f == 0 && (int64_t)B * H * W <= 0x7FFFFFFF;
}
static double* spark_loss_scratch(OpScratch& sc, int B, int H, int W) { return sc.n<double>((size_t)spark_loss_chunks((long long)B * H * W) * 2); }
size_t cddpm_op_spark_loss_scratch(int B, int H, int W, int f) {
    if (!spark_loss_shape_ok(B, H, W, f)) return 0;
    return counted([&](OpScratch& sc) { spark_loss_scratch(sc, B, H, W); });
}
int cddpm_op_spark_loss(cddpm_handle h, const float* rec_dev, const float* inp_dev, const uint8_t* active_dev, int f, int B, int H, int W, float w_mask,
                        float w_l1, float* loss_dev, float* drec_dev, void* stream) {
    OP_CHECK(spark_loss_shape_ok(B, H, W, f), "cddpm_op_spark_loss: unsupported shape (B %d, H %d, W %d, f %d dividing H and W)", B, H, W, f)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, rec_dev && inp_dev && active_dev && loss_dev, "cddpm_op_spark_loss: NULL argument")
    OpScratch sc(h, s);
    double* part = spark_loss_scratch(sc, B, H, W);
    SCRATCH_CHECK(sc)
    launch_spark_loss(rec_dev, inp_dev, active_dev, f, B, H, W, w_mask, w_l1, nullptr, loss_dev, drec_dev, part, s);
    OP_EPILOGUE()
}
// cddpm_op_spark_loss under the dynamic loss scale: drec carries the device scale, the two terms do not (step (a) of "Dynamic loss scaling")
int cddpm_op_spark_loss_scaled(cddpm_handle h, const float* rec_dev, const float* inp_dev, const uint8_t* active_dev, int f, int B, int H, int W,
                               float w_mask, float w_l1, const int32_t* scaler_dev, float* loss_dev, float* drec_dev, void* stream) {
    OP_CHECK(spark_loss_shape_ok(B, H, W, f), "cddpm_op_spark_loss_scaled: unsupported shape (B %d, H %d, W %d, f %d dividing H and W)", B, H, W, f)
    OP_PROLOGUE(PC_OTHER, 0.0, 0.0, rec_dev && inp_dev && active_dev && loss_dev && scaler_dev, "cddpm_op_spark_loss_scaled: NULL argument")
    OpScratch sc(h, s);
    double* part = spark_loss_scratch(sc, B, H, W);
    SCRATCH_CHECK(sc)
    launch_spark_loss(rec_dev, inp_dev, active_dev, f, B, H, W, w_mask, w_l1, scaler_dev, loss_dev, drec_dev, part, s);
    OP_EPILOGUE()
}
// torch.optim.AdamW (src/models/Spark_2D.py:123-124): cddpm_op_adam_guarded with the decoupled decay p <- p (1 - lr weight_decay) before the update
int cddpm_op_adamw_guarded(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, float grad_unscale, const int32_t* ctrl_dev, void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, p_dev && g_dev && m_dev && v_dev && ctrl_dev && n > 0 && weight_decay >= 0.0f, "cddpm_op_adamw_guarded: bad arguments")
    launch_adam_guarded(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, grad_unscale, weight_decay, ctrl_dev, nullptr, s);
    OP_EPILOGUE()
}
// cddpm_op_adamw_guarded under the dynamic loss scale, in the form of cddpm_op_adam_scaled: gradient = g extra_unscale / the device scale
int cddpm_op_adamw_scaled(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, float extra_unscale, const int32_t* ctrl_dev, const int32_t* scaler_dev, void* stream) {
    OP_PROLOGUE(PC_OPT, 0.0, 0.0, p_dev && g_dev && m_dev && v_dev && ctrl_dev && scaler_dev && n > 0 && weight_decay >= 0.0f,
                "cddpm_op_adamw_scaled: bad arguments")
    launch_adam_guarded(p_dev, g_dev, m_dev, v_dev, n, lr, beta1, beta2, eps, extra_unscale, weight_decay, ctrl_dev, scaler_dev, s);
    OP_EPILOGUE()
}

}  // extern "C"
