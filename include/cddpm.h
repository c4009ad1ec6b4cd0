/*
 * cddpm.h -- C ABI of libcddpm_hip.so: the MI355X (gfx950) implementation of the cDDPM
 * reverse-diffusion reconstruction path.
 *
 * The reference (raymondfdavey/Conditioned-Diffusion-Models-UAD) is pure Python/PyTorch and has no
 * native interface; each entry point below names the reference Python code it replaces
 * (paths relative to the reference root). Plain pointers and sizes only: no torch types.
 *
 * Conventions
 *   - return value: 0 = ok, negative = error; text via cddpm_last_error().
 *   - "dev" pointers are device (HIP) pointers to contiguous fp32; "host" pointers are host memory.
 *   - images are [B,1,H,W] fp32 (single channel, so NCHW == NHWC); H and W multiples of 4.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued on it, nothing synchronises with the host inside forward/reverse calls.
 *   - one handle per device; a handle is not thread-safe.
 *
 * Environment variables the library reads
 *   - CDDPM_CONV: the PROCESS DEFAULT convolution family and packed weight format: what a new handle starts with and what the
 *     handle-less helpers (cddpm_pack_conv_weights, cddpm_packed_conv_bytes) use. h3 or unset = fp16 two-term split (default),
 *     x6 = bf16 three-term split, f32 = fp32 MFMA (see cddpm_pack_conv_weights). A handle overrides it: cddpm_set_conv_family.
 *   - CDDPM_NB2: 256-cout workgroups of the default family. Unset = where the plan takes them (cddpm_set_accumulation_switch,
 *     cddpm_op_conv_packed); 0 = never; force = wherever the kernel can, in every entry point and at any geometry.
 *   - CDDPM_GRAPH: 1 = cddpm_reverse / cddpm_reverse_range (>= 5 steps, not while profiling) replay each step as a captured
 *     hipGraph instead of launching its kernels: bit-identical, not faster.
 *   - CDDPM_TRAIN_PRECISION: 16 = initial training arithmetic plain fp16 operands; unset = 32 (cddpm_set_train_precision).
 */
#ifndef CDDPM_H
#define CDDPM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cddpm_ctx* cddpm_handle;

#define CDDPM_MAX_LEVELS 8

/* Shape contract of the denoiser: the constructor arguments of UNetModel
 * (src/models/modules/OpenAI_Unet.py:513-539) as DDPM_2D passes them (src/models/DDPM_2D.py:37-59):
 * resblock_updown=True, use_scale_shift_norm=True, use_new_attention_order=True, dims=2, dropout=0. */
typedef struct cddpm_unet_desc {
    int32_t in_channels;                               /* 1 */
    int32_t out_channels;                              /* 1 */
    int32_t model_channels;                            /* cfg.unet_dim = 128 (multiple of 128) */
    int32_t num_levels;                                /* len(channel_mult) */
    int32_t channel_mult[CDDPM_MAX_LEVELS];            /* cfg.dim_mults = [1,2,2] */
    int32_t num_res_blocks;                            /* 3 */
    int32_t num_attention_resolutions;                 /* len(attention_resolutions) */
    int32_t attention_resolutions[CDDPM_MAX_LEVELS];   /* (3,6,12): never matches ds in {1,2,4} */
    int32_t head_channels;                             /* num_head_channels = 64 */
    int32_t cond_dim;                                  /* num_classes slot = context width 128; 0 = unconditional */
    int32_t timesteps;                                 /* GaussianDiffusion timesteps T */
    int32_t max_batch;                                 /* largest B of any later call */
    int32_t max_h, max_w;                              /* largest H, W of any later call */
} cddpm_unet_desc;

/* objective values for cddpm_set_schedule (src/models/modules/cond_DDPM.py:318) */
#define CDDPM_PRED_X0 0
#define CDDPM_PRED_NOISE 1

/* Replaces UNetModel.__init__ + GaussianDiffusion.__init__ buffer allocation. Allocates packed-weight
 * storage, embedding tables and the activation workspace once; no hipMalloc happens later. */
int cddpm_create(cddpm_handle* out, const cddpm_unet_desc* desc, int device);
void cddpm_destroy(cddpm_handle h);
/* message of the last failing call on h (h == NULL: last failing cddpm_create) */
const char* cddpm_last_error(cddpm_handle h);
/* device bytes cddpm_create will allocate for this descriptor */
size_t cddpm_workspace_bytes(const cddpm_unet_desc* desc);

/* The state_dict entries the library consumes, in the reference's naming
 * (`diffusion.model.` prefix stripped): time_embed.0.weight, input_blocks.1.0.in_layers.2.weight, ...
 * (SURVEY.md 8a 'State-dict naming'; src/models/modules/OpenAI_Unet.py:583-797). */
int cddpm_num_weights(cddpm_handle h);
const char* cddpm_weight_name(cddpm_handle h, int i);
int64_t cddpm_weight_numel(cddpm_handle h, int i);

/* Replaces model.load_state_dict (src/train.py:161). `host_ptrs[i]` is the fp32 tensor `names[i]` in
 * PyTorch layout (Conv2d [Cout,Cin,kh,kw], Linear [out,in], Conv1d [Cout,Cin,1]); the library re-packs
 * into its own MFMA tile images and uploads. The caller keeps ownership. Every name reported by
 * cddpm_weight_name must be present; extra names are ignored. */
int cddpm_load_weights(cddpm_handle h, const char* const* names, const float* const* host_ptrs,
                       const int64_t* numels, int n);

/* Replaces the registered schedule buffers GaussianDiffusion reads in q_posterior / p_sample
 * (src/models/modules/cond_DDPM.py:366-371, :391-398, :444). Host arrays of length T:
 * posterior_mean_coef1, posterior_mean_coef2, posterior_log_variance_clipped,
 * sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod (the last two are read by CDDPM_PRED_NOISE steps and by every
 * DDIM step, cond_DDPM.py:385-389, :491; all five are required).
 * Also (re)builds the per-ResBlock time-embedding tables, so weights must be loaded first. */
int cddpm_set_schedule(cddpm_handle h, const float* coef1, const float* coef2, const float* logvar,
                       const float* sqrt_recip, const float* sqrt_recipm1, int T, int objective);

/* Replaces label_emb(cond) and the cond half of every ResBlock's emb_layers
 * (src/models/modules/OpenAI_Unet.py:583-590, :849-852, :300): computed once per batch, not per step.
 * cond_dev: [B, cond_dim]. */
int cddpm_prepare_cond(cddpm_handle h, const float* cond_dev, int B, void* stream);

/* Replaces UNetModel.forward / forward_with_cond_scale (src/models/modules/OpenAI_Unet.py:814-1006).
 * x_dev [B,1,H,W] -> out_dev [B,1,H,W]. t_dev: int32 [B] per-sample timesteps on the device, or NULL to
 * use t_uniform for every sample. Uses the context prepared by cddpm_prepare_cond for the same B. */
int cddpm_unet_forward(cddpm_handle h, const float* x_dev, const int32_t* t_dev, int t_uniform,
                       float* out_dev, int B, int H, int W, void* stream);

/* Replaces GaussianDiffusion.p_sample_loop, Gaussian branch (src/models/modules/cond_DDPM.py:446-464)
 * including p_sample / p_mean_variance / model_predictions / q_posterior (:391-444):
 * img_inout_dev holds x_T on entry ([B,1,H,W], N(0,1)) and the reconstruction in [0,1] on return.
 * Runs steps t = t_start-1 .. 0 (the reference's T = num_timesteps if start_t == 0 else start_t, :449,
 * is resolved by the caller). noise_dev: z_t at noise_dev + t*B*H*W for t in [1, t_start) (slot 0 unused),
 * or NULL to draw z_t on the device with Philox4x32-10 keyed (seed; quad, t, slice0 + b, stream)
 * -- see conditioned-diffusion-models-uad_amd/synth.py. */
int cddpm_reverse(cddpm_handle h, float* img_inout_dev, const float* noise_dev, uint64_t seed,
                  uint64_t slice0, int t_start, int B, int H, int W, void* stream);

/* Accumulation plan of the reverse steps (cddpm_p_sample / cddpm_reverse / cddpm_reverse_range; default family, handles whose maximum
 * geometry gives every Cout = 256 convolution >= 512 workgroups -- i.e. large batches). OPT-IN speed / accuracy trade, off by default
 * (t_switch = 2^30). Steps t >= t_switch multiply those convolutions on 256-cout workgroups that share the chunk's transformed patch
 * between two cout blocks and accumulate in two levels: +9...12 % per layer, +6 % per reverse step at B = 64; a convolution's rounding
 * noise ~6e-7 of rms instead of 1.9e-7 (the reference's CPU fmaf chain: 1.2e-6). Steps t < t_switch use the three-level kernel.
 * Measured on the full-length parity chain (B = 2 x 128 x 128 x T = 1000, final image vs the reference; tools/accum_switch_sweep.py):
 *   t_switch   off      500      300      200      0
 *   max        1.49e-4  1.32e-4  1.59e-4  2.69e-4  1.99e-4
 *   rms        6.95e-6  8.02e-6  9.08e-6  1.09e-5  1.02e-5        (the reference against itself: 1.02e-4 / 5.6e-6)
 * -- the extra rounding noise of ANY part of the chain survives to the end (there is no late switch step that hides it), which is why
 * the default keeps three-level accumulation on every step. A function of t alone: a slice's bits do not depend on its batch.
 * Single forwards (cddpm_unet_forward, cddpm_ddim_step) use the three-level kernel. cddpm_op_conv_packed plans per call instead: it
 * takes the 256-cout form wherever the call itself has >= 512 workgroups of the 128-cout form (CDDPM_NB2=0 disables it).
 * No effect on a handle at precision 16 (cddpm_set_precision): it takes the 256-cout form on every step and in single forwards. */
int cddpm_set_accumulation_switch(cddpm_handle h, int t_switch);

/* Convolution family of a handle. family: CDDPM_CONV_H3 = fp16 two-term split (needs |activation| < 65504; the fastest),
 * CDDPM_CONV_X6 = bf16 three-term split (exact products, no range limit), CDDPM_CONV_F32 = fp32 MFMA; any other value is an error.
 * A new handle starts with the process default (CDDPM_CONV, else h3). Every launch of the handle and every weight image it packs
 * is in its family, so handles of different families work side by side in one process, interleaved on one stream.
 * Packed weights belong to a family: setting a DIFFERENT family after cddpm_load_weights waits for the device, frees the packed
 * images, and cddpm_unet_forward / cddpm_reverse / cddpm_reverse_range / cddpm_p_sample / cddpm_ddim_step fail with a message
 * saying so until cddpm_load_weights and cddpm_set_schedule have run again. Setting the current family does nothing.
 * The device packer and cddpm_op_conv_packed (the training step) serve h3 handles only. */
#define CDDPM_CONV_F32 0
#define CDDPM_CONV_X6 1
#define CDDPM_CONV_H3 2
int cddpm_set_conv_family(cddpm_handle h, int family);
int cddpm_get_conv_family(cddpm_handle h);      /* the family, or -1 for a NULL handle */

/* Precision of a handle's reconstruction path: the arithmetic of the reference's evaluation under the Trainer's `precision: 16`, i.e.
 * fp16 autocast over ResBlock._forward (src/models/modules/OpenAI_Unet.py:284-338) and QKVAttention.forward (:457-476).
 * bits: 32 (what a handle starts with: fp32-grade products, fp32 attention) or 16; any other value is an error, and so is 16 on a
 * handle whose family is not CDDPM_CONV_H3. On a precision-16 handle cddpm_set_conv_family(h, CDDPM_CONV_X6 | CDDPM_CONV_F32) fails
 * with "cddpm_set_conv_family: the handle is at precision 16, which only the h3 family has (cddpm_set_precision(h, 32) first)".
 * At 16, cddpm_unet_forward / cddpm_p_sample / cddpm_reverse / cddpm_reverse_range / cddpm_ddim_step
 *   - multiply plain fp16 operands (fp32 accumulation) in every convolution planned through the split family: 3x3, folded
 *     upsample, 1x1, the 1x1 skip segment and the split-K small-batch plan -- one MFMA per product group instead of three;
 *   - run every attention block, middle and in-level, on the fp16-MFMA kernel of cddpm_op_attention_p16;
 *   - take the 256-cout workgroup form wherever the handle's MAXIMUM geometry allows it (>= 512 workgroups of the 128-cout form;
 *     CDDPM_NB2=0 disables it), on every step and in single forwards: a function of the handle, never of the batch in the call, so
 *     a slice's bits still do not depend on the batch it is computed in. cddpm_set_accumulation_switch has no effect.
 * The one-channel input convolution, the head, GroupNorm, the embedding linears and the step kernels stay fp32.
 * Accuracy: that of fp16 autocast (operand rounding 2^-11, not 2^-24) -- NOT the 1e-4 full-length chain of precision 32; the
 * measured ratios against the reference under autocast are in DESIGN.md section 7.4. Range: as for every h3 handle an activation
 * beyond +-65504 gives a non-finite slice (cddpm_slice_status finds it; re-run it on a handle of an exact family).
 * No repack: the packed h3 weight image is read hi-term only. A change invalidates a captured step graph. The cddpm_op_*
 * operators and the process-wide cddpm_set_train_precision neither read nor change a handle's precision. */
int cddpm_set_precision(cddpm_handle h, int bits);
int cddpm_get_precision(cddpm_handle h);        /* 32 or 16, or -1 for a NULL handle */

/* Attention family of a handle: the arithmetic of every attention block, middle and in-level, of cddpm_unet_forward / cddpm_p_sample /
 * cddpm_reverse / cddpm_reverse_range / cddpm_ddim_step at precision 32, in the convolution families' numbering.
 *   CDDPM_CONV_F32 (what a handle starts with, whatever CDDPM_CONV says): exact fp32 products, the kernel of cddpm_op_attention;
 *   CDDPM_CONV_H3: fp32-grade products from two-term fp16 splits on the 16-bit matrix pipe, the kernel of cddpm_op_attention_h3, with
 *                  its range contract (|q / 8|, |k|, |v| < 65504; outside it that slice is non-finite, which cddpm_slice_status finds);
 *   CDDPM_CONV_X6: refused with "cddpm_set_attention_family: there is no x6 attention (...)"; any other value is an error too.
 * Rule: a precision-16 handle runs the kernel of cddpm_op_attention_p16 WHATEVER its attention family is; the family is kept and takes
 * effect when the handle returns to precision 32. Independent of the convolution family; nothing is repacked (the attention core has
 * no weights); a change invalidates a captured step graph. The cddpm_op_* operators neither read nor change it. */
int cddpm_set_attention_family(cddpm_handle h, int family);
int cddpm_get_attention_family(cddpm_handle h);      /* the family, or -1 for a NULL handle */

/* Per-slice status of x_dev [B,1,H,W] (16-byte aligned, H * W a multiple of 4): status_dev[b] (int32 [B]) = 1 if slice b holds an
 * inf or a NaN, else 0. One kernel launch for the whole batch on `stream`, no host synchronisation: the caller copies the B flags.
 * What a caller uses to find the slices of a reconstruction that left the fp16 range of an h3 handle and re-run only those on a
 * handle of an exact family. Not part of the reverse step: cddpm_reverse and its kin never launch it. */
int cddpm_slice_status(cddpm_handle h, const float* x_dev, int B, int H, int W, int* status_dev, void* stream);

/* `clip_denoised` of p_sample / ddim_sample (src/models/modules/cond_DDPM.py:433, :467): on (the reference's default, and the
 * handle's) clamps the x0 estimate to [-1,1] before the posterior mean / the DDIM update; off uses it as predicted.
 * Applies to every later cddpm_p_sample / cddpm_reverse / cddpm_reverse_range / cddpm_ddim_step on the handle. */
int cddpm_set_clip_denoised(cddpm_handle h, int on);

/* A segment of the same chain: steps t = t_hi, t_hi - 1, ..., t_lo (0 <= t_lo <= t_hi < T) of p_sample_loop's recurrence
 * (cond_DDPM.py:460-461) on img_inout_dev (values in [-1,1]); the map to [0,1] (:463) is applied exactly when t_lo == 0.
 * cddpm_reverse(t_start) == cddpm_reverse_range(t_start - 1, 0); cutting a chain into consecutive segments gives
 * bit-identical results (progress reporting, checkpoints of x_t, bench segments). noise_dev is indexed by the absolute t. */
int cddpm_reverse_range(cddpm_handle h, float* img_inout_dev, const float* noise_dev, uint64_t seed, uint64_t slice0,
                        int t_hi, int t_lo, int B, int H, int W, void* stream);

/* Replaces one GaussianDiffusion.p_sample call (src/models/modules/cond_DDPM.py:432-444): img <- x_{t-1} from x_t,
 * still in [-1,1]. z_dev: the step's N(0,1) draw [B,1,H,W], or NULL for the device Philox (ignored at t == 0). */
int cddpm_p_sample(cddpm_handle h, float* img_inout_dev, const float* z_dev, uint64_t seed, uint64_t slice0,
                   int t, int B, int H, int W, void* stream);

/* Replaces one iteration of GaussianDiffusion.ddim_sample's loop (src/models/modules/cond_DDPM.py:487-511): UNet at
 * t = `time`, eps from the UNCLIPPED x0 (model_predictions :400-420, clip_x_start = False), x0 clamped to [-1,1] (:496),
 * img <- x0 * coef_x0 + coef_eps * eps + sigma * z. The caller supplies what the reference computes from
 * alphas_cumprod_prev[time], alphas_cumprod_prev[time_next] in fp32 (:489-499): coef_x0 = sqrt(alpha_next),
 * sigma = eta sqrt((1 - alpha/alpha_next)(1 - alpha_next)/(1 - alpha)), coef_eps = sqrt(1 - alpha_next - sigma^2);
 * add_noise = (time_next > 0); z_dev = the step's N(0,1) draw or NULL for the device Philox keyed by t;
 * finalize != 0 on the last pair also maps the result to [0,1] (:513). */
int cddpm_ddim_step(cddpm_handle h, float* img_inout_dev, const float* z_dev, uint64_t seed, uint64_t slice0,
                    int t, float coef_x0, float coef_eps, float sigma, int add_noise, int finalize,
                    int B, int H, int W, void* stream);

/* Replaces torch.randn(shape) / torch.randn_like (src/models/modules/cond_DDPM.py:454, :440) with the
 * counter RNG: out_dev [B,1,H,W] ~ N(0,1); stream_id 0x1001 = x_T, 0x1002 = z_t. Philox4x32-10, key = the two 32-bit halves of
 * `seed`, counter = (element quad within the slice, t, slice0 + b, stream_id) with t and slice0 + b taken modulo 2^32: slice b of a
 * batch holds the bits a one-slice call at slice0 + b gives. Not bound by the handle's max_batch.
 * Preconditions, each refused with a message before anything is launched: out_dev not NULL and 16-byte aligned; B, H, W >= 1;
 * H * W a multiple of 4; B * H * W < 2^31. */
int cddpm_noise_fill(cddpm_handle h, float* out_dev, uint64_t seed, uint32_t stream_id, int t,
                     uint64_t slice0, int B, int H, int W, void* stream);

/* Replaces gen_noise(cfg, shape) for noisetype 'simplex' (src/utils/generate_noise.py:8-52: Simplex_CLASS, _init :214-232,
 * rand_2d_octaves :97-114, _noise2 :252-352; numba CPU code + H2D copy on every step in the reference). out_f16_dev
 * receives [B,1,H,W] IEEE half bit patterns: the SAME field for every batch item, float64 arithmetic rounded to float16
 * as torch's .half() does -- bit-exact with the reference for a given `seed` (the value Simplex_CLASS.newSeed draws with
 * np.random.randint). Square fields only, like the reference. Reference parameters: octaves 6, persistence 0.8, frequency 64. */
int cddpm_simplex_fill(cddpm_handle h, uint16_t* out_f16_dev, int64_t seed, int B, int H, int W, int octaves,
                       double persistence, double frequency, void* stream);

/* Replaces the residual-map post-processing of _test_step (src/utils/utils_eval.py:29-33 residual, :64-66 +
 * apply_brainmask_volume :447-460, :69-71 + apply_3d_median_filter :462-464), which the reference runs in scipy on the CPU
 * after copying the volume to the host. Volumes are [S][H][W] fp32 on the device (the reference indexes [H][W][S]; the
 * filters are symmetric under that permutation):
 *   out = |orig - recon| (squared = 0) or (orig - recon)^2 (squared = 1); recon_dev == NULL: out = orig (the volume
 *     already is a residual: apply_brainmask_volume / apply_3d_median_filter on their own);
 *   mask_dev != NULL: out *= erosion of (mask > 0), per slice, by the 4-connected cross applied erode_iterations times
 *     (scipy.ndimage.binary_erosion(structure = generate_binary_structure(2, 1), border_value = 0); the reference passes
 *     iterations = W / 25); erode_iterations = 0 multiplies by the mask as it is;
 *   median_k = 3 or 5: out = scipy.ndimage.median_filter(out, (k, k, k)), boundary mode 'reflect'; 0 = no filter.
 * Exact: the results equal scipy's bit for bit (a selection and a product with 0/1). tmp_dev: [S][H][W] scratch, needed
 * only when median_k != 0 (may be NULL otherwise); out_dev must not alias orig/recon/mask. */
int cddpm_residual_postprocess(cddpm_handle h, const float* orig_dev, const float* recon_dev, const float* mask_dev,
                               int S, int H, int W, int squared, int erode_iterations, int median_k, float* tmp_dev,
                               float* out_dev, void* stream);

/* ---- evaluation metrics (csrc/eval_metrics.hip) -------------------------------------------------------
 * Replace the metric half of _test_step / _test_end (src/utils/utils_eval.py:18-194, :196-297), which the reference runs in
 * sklearn / skimage / numpy on the CPU. Volumes are flat [R][D1][D2] fp32 on the device, R = axis 0 of the reference's
 * [H, W, D] volume (the axis its per-slice loop walks). The caller provides the workspace (cddpm_eval_workspace_bytes);
 * nothing allocates or synchronises inside; results stay on the device. */
#define CDDPM_EVAL_VOXEL_METRICS 1       /* AUROC / AUPRC / find_best_val / threshold / confusion counts (:78-139) */
#define CDDPM_EVAL_COMPONENT_FILTER 2    /* remove 26-connected components of <= 7 voxels (:98-99, :485-499) */
#define CDDPM_EVAL_ROW_CURVE 4           /* AUROC / AUPRC of the per-row anomaly scores (:175-178) */
#define CDDPM_EVAL_THRESHOLD_OVERRIDE 8  /* threshold the volume at `threshold` instead of the search's value (:92-93) */
/* slots of the volume record (float64; NaN where not computed) */
#define CDDPM_EVAL_L1_ALL 0              /* l1 / l2 reconstruction errors over all voxels, seg > 0, seg == 0 (fp32 values, :36-41) */
#define CDDPM_EVAL_L1_LESION 1
#define CDDPM_EVAL_L1_HEALTHY 2
#define CDDPM_EVAL_L2_ALL 3
#define CDDPM_EVAL_L2_LESION 4
#define CDDPM_EVAL_L2_HEALTHY 5
#define CDDPM_EVAL_SCORE_VOL 6           /* mean residual over mask > 0 (fp32 value, :153) */
#define CDDPM_EVAL_LESION 7              /* #(seg > 0) */
#define CDDPM_EVAL_VOXELS 8
#define CDDPM_EVAL_AUROC 9               /* roc_curve + auc (:80, :549-552) */
#define CDDPM_EVAL_AUPRC 10              /* average_precision_score (:81, :555-558) */
#define CDDPM_EVAL_BEST_DICE 11          /* find_best_val(max_steps = 10) (:84-90) */
#define CDDPM_EVAL_BEST_THRESHOLD 12
#define CDDPM_EVAL_THRESHOLD 13          /* the threshold applied: the search's, or the override */
#define CDDPM_EVAL_MAX 14                /* max of the residual */
#define CDDPM_EVAL_PRED1_SEG0 15         /* filtered prediction 1, seg 0 */
#define CDDPM_EVAL_PRED1_SEG1 16         /* filtered prediction 1, seg 1 */
#define CDDPM_EVAL_ROW_AUROC 17
#define CDDPM_EVAL_ROW_AUPRC 18
#define CDDPM_EVAL_RECORD 24
/* slots of the set result (float64) */
#define CDDPM_EVAL_SET_AUROC 0
#define CDDPM_EVAL_SET_AUPRC 1
#define CDDPM_EVAL_SET_T1P 2             /* threshold at the first point roc_curve retains with fpr > 0.01 (:280-283) */
#define CDDPM_EVAL_SET_T5P 3
#define CDDPM_EVAL_SET_T10P 4
#define CDDPM_EVAL_SET_BEST_DICE 5
#define CDDPM_EVAL_SET_BEST_THRESHOLD 6  /* find_best_val over the set: threshold['total'] (:247-254) */
#define CDDPM_EVAL_SET_MAX 7
#define CDDPM_EVAL_SET_RESULT 8

/* workspace bytes for n voxels in `rows` rows (rows = 0: a set search); host arithmetic, callable without a GPU */
size_t cddpm_eval_workspace_bytes(int64_t n, int rows);

/* One volume's metric record (_test_step :36-41, :78-139, :146-178). recon_dev: the squeezed final_volume; orig_dev,
 * seg_dev, mask_dev: data_orig / data_seg / data_mask (raw, binarised inside as > 0); diff_dev: the post-processed residual
 * (cddpm_residual_postprocess). Outputs: record_dev [CDDPM_EVAL_RECORD] float64; row_score_dev [R] fp32 (masked mean per
 * row, 0 for a row without mask); row_label_dev [R] int32 (row has lesion); row_counts_dev [R][3] int32 (#pred, #pred & seg,
 * #seg per row on the UNFILTERED prediction, with CDDPM_EVAL_VOXEL_METRICS); pred_dev [R*D1*D2] uint8: the filtered
 * prediction (may be NULL). Counts are exact (integer atomics), float sums are fixed-order float64: bitwise reproducible. */
int cddpm_eval_volume(cddpm_handle h, const float* recon_dev, const float* orig_dev, const float* seg_dev, const float* mask_dev,
                      const float* diff_dev, int R, int D1, int D2, int flags, double threshold, void* ws_dev, size_t ws_bytes,
                      double* record_dev, float* row_score_dev, int32_t* row_label_dev, int32_t* row_counts_dev,
                      uint8_t* pred_dev, void* stream);

/* Over an accumulated set x_dev [n] fp32 with labels y_dev [n] int8 (_test_end :247-286): healthy = 0: find_best_val ->
 * threshold['total'], plus AUROC / AUPRC; healthy = 1: labels taken as all zero, the t_1p / t_5p / t_10p thresholds.
 * out_dev [CDDPM_EVAL_SET_RESULT] float64. */
int cddpm_eval_set(cddpm_handle h, const float* x_dev, const int8_t* y_dev, int64_t n, int healthy, void* ws_dev,
                   size_t ws_bytes, double* out_dev, void* stream);

/* ---- Hausdorff distance (csrc/eval_hausdorff.hip) -------------------------------------------------------
 * Replaces the HausPerVol entry of _test_step (src/utils/utils_eval.py:131-135; aggregated :240-241), which the reference
 * takes from monai.metrics.compute_hausdorff_distance(diffs_thresholded, data_seg, include_background=False,
 * distance_metric='euclidean', percentile=None, directed=False) on the CPU. Status: PINNED TO SCIPY, UNPINNED TO MONAI. The
 * rules below restate monai 1.0.1's get_mask_edges / get_surface_distance / compute_hausdorff_distance; monai itself was not
 * available to compare with, scipy was, and every result equals the scipy restatement bit for bit.
 * Volumes are flat [R][D1][D2] (R = axis 0 of the reference's [H, W, D]), unit spacing.
 *   masks    P = pred != 0 (uint8: the pred_dev of cddpm_eval_volume, which is what the reference hands to monai);
 *            G = seg != 0 (raw fp32 data_seg). monai, as recalled, reads a non-boolean ground truth as == 1: the two agree
 *            on binary segmentations and differ where a label map holds other values.
 *   axes     U = P | G. With CDDPM_HAUSDORFF_SQUEEZE the ACTIVE axes are those along which U's bounding box is wider than
 *            one voxel (monai crops to the box and np.squeeze's it, so a flat union is eroded with a 2-D cross); without
 *            the flag all three are active.
 *   edges    edge(M) = M & ~erode(M); erode keeps a voxel only if both neighbours along every active axis are in M, and a
 *            neighbour outside the volume is not in M (scipy.ndimage.binary_erosion, border_value = 0). A non-empty mask
 *            always has an edge: when no axis is active (U is one voxel) that voxel is its own edge.
 *   d2       d2(v, E) = min over e in E of the squared index distance (an exact integer);
 *            directed(A -> B) = max over a in edge(A) of d2(a, edge(B)).
 *   result   NaN when both masks are empty, +inf when exactly one is, otherwise
 *            sqrt((double) max(directed(P -> G), directed(G -> P))): equal to
 *            scipy.ndimage.distance_transform_edt(~edge)[other_edge].max() bit for bit.
 * Supported range: every axis 1 ... CDDPM_HAUSDORFF_MAX_AXIS (3 * 1023^2 + CDDPM_HAUSDORFF_FAR fits an int32). */
#define CDDPM_HAUSDORFF_SQUEEZE 1        /* flags: derive the active axes from the bounding box of U (what the mirrors set) */
#define CDDPM_HAUSDORFF_MAX_AXIS 1024
#define CDDPM_HAUSDORFF_FAR (1 << 28)    /* dist2_dev of an EMPTY edge set holds this value at every voxel */
/* slots of the result (float64) */
#define CDDPM_HAUSDORFF_DISTANCE 0
#define CDDPM_HAUSDORFF_D2_PRED_TO_SEG 1 /* directed(P -> G) and directed(G -> P), squared; NaN unless both masks are non-empty */
#define CDDPM_HAUSDORFF_D2_SEG_TO_PRED 2
#define CDDPM_HAUSDORFF_EDGES_PRED 3     /* #edge(P), #edge(G) */
#define CDDPM_HAUSDORFF_EDGES_SEG 4
#define CDDPM_HAUSDORFF_ACTIVE_AXIS0 5   /* 1.0 / 0.0 per axis (R, D1, D2); with the flag all 0.0 when U is empty or one voxel */
#define CDDPM_HAUSDORFF_ACTIVE_AXIS1 6
#define CDDPM_HAUSDORFF_ACTIVE_AXIS2 7
#define CDDPM_HAUSDORFF_RESULT 8

/* workspace bytes of cddpm_eval_hausdorff; host arithmetic, callable without a GPU. Outside the supported range: 0, with the
 * reason in cddpm_last_error(NULL). */
size_t cddpm_hausdorff_workspace_bytes(int R, int D1, int D2);

/* out_dev [CDDPM_HAUSDORFF_RESULT] float64. edges_dev [R*D1*D2] uint8 (may be NULL): bit 0 = edge(P), bit 1 = edge(G).
 * dist2_dev [2][R*D1*D2] int32 (may be NULL): the squared distance of every voxel of the VOLUME to edge(P) ([0]) and to
 * edge(G) ([1]). The two exist for tests: the distance is a maximum, which a transform that is wrong at most voxels can
 * still get right. Integer arithmetic and integer atomics throughout: bitwise reproducible. Nothing allocates or
 * synchronises inside; the bounding box and the active axes stay on the device. */
int cddpm_eval_hausdorff(cddpm_handle h, const uint8_t* pred_dev, const float* seg_dev, int R, int D1, int D2, int flags,
                         void* ws_dev, size_t ws_bytes, double* out_dev, uint8_t* edges_dev, int32_t* dist2_dev, void* stream);

/* ---- Augmented training slices (csrc/augment.hip) -------------------------------------------------------
 * Replaces, for `aug_intensity: True`, the per-item work of the reference's training datamodule: get_augment
 * (src/datamodules/create_dataset.py:220-250) = Compose(RandomGamma(p=.5), RandomBiasField(p=.25), RandomBlur(p=.25),
 * RandomGhosting(p=.5)) of torchio on the whole preloaded volume, then vol2slice (:143-193), which keeps one slice. Status:
 * PINNED TO NUMPY / SCIPY, UNPINNED TO TORCHIO. The rules below restate torchio 0.18.9x's transforms; torchio itself was not
 * available to compare with, numpy and scipy were (tests/augment_reference.py). The random draws are the caller's
 * (augment.IntensityAugment.draw); this entry applies one table row per output slice.
 * The bank is [N][D][H][W] fp32, slice-major: torchio's [1, H, W, D] volume permuted once, so a slice is a contiguous [H][W]
 * image. Axis numbers keep torchio's meaning: 0 = H, 1 = W, 2 = D. Every extent is 1 ... CDDPM_AUG_MAX_AXIS.
 *   meta_dev [B][CDDPM_AUG_META] int32: {volume, z, flags, g | axis << 8} -- bank volume, output slice, the stage bits below,
 *            the ghosting's num_ghosts g (0 ... 255) and axis.
 *   par_dev  [B][CDDPM_AUG_PAR] fp32: {gamma, sigma0, sigma1, sigma2, I, c[20], 3 unused} -- the exponent, the blur's sigma per
 *            axis in VOXELS (std / spacing), the ghosting's intensity, the bias field's coefficients.
 * Stages, in Compose's order; a sample with flags = 0 is a bit-exact copy of its slice:
 *   CDDPM_AUG_GAMMA  y = sign(x) |x|^gamma (torchio's rule for data with negatives; x^gamma otherwise).
 *   CDDPM_AUG_BIAS   y = x exp(sum_i c_i X^a Y^b Z^c), i counting a in 0..3, then b in 0..3-a, then c in 0..3-a-b; X, Y, Z the
 *                    coordinates along axes 0, 1, 2: u(i) = (2 i - L + 1) / (L - 1), 0 where L = 1, and 0^0 = 1.
 *                    Gamma and bias are evaluated together in double and rounded to fp32 once.
 *   CDDPM_AUG_BLUR   scipy.ndimage.gaussian_filter(vol, sigma) with its defaults: separable, axis 0, 1, 2; radius
 *                    int(4 sigma + 0.5); weights exp(-k^2 / (2 sigma^2)) normalised; boundary `reflect` (d c b a | a b c d |
 *                    d c b a) by repeated reflection, so a radius may exceed the axis; an axis with sigma <= 1e-15 is skipped;
 *                    line sums in double, fp32 between the passes.
 *   CDDPM_AUG_GHOST  torchio scales the planes s = 0, g, 2 g, ... of the fft-shifted spectrum along the axis by 1 - I, restores
 *                    the plane s = L / 2, inverts and keeps the real part. The mask depends on the axis frequency alone, so this
 *                    is y = x - I (c (*) x), a circular convolution along the axis with
 *                    c[d] = (1 / L) sum over s = 0, g, 2 g, ... < L, s != L / 2 of cos(2 pi (s - L / 2) d / L),
 *                    built in double with the argument reduced in integers, accumulated in double and evaluated at the output
 *                    slice only. g = 0 or I = 0: the identity (torchio's early return).
 * Errors: -1 with the reason in cddpm_last_error(h) for what the host can see -- a NULL pointer, N < 1, an extent outside
 * 1 ... CDDPM_AUG_MAX_AXIS, B outside 1 ... CDDPM_AUG_MAX_BATCH, a short workspace -- before anything is enqueued. The two tables
 * live on the device: the first kernel reads them alone, and a row with volume outside [0, N), z outside [0, D), axis > 2,
 * unknown flag bits, a sigma outside [0, CDDPM_AUG_MAX_SIGMA] or a non-finite parameter is flagged: no kernel reads the bank
 * or writes the output for that sample, and its CDDPM_AUG_BAD_* bits stand in the status word. After the call the first B int32
 * of ws_dev are the status words of the B samples (0: done). Callers with host tables check them before the copy
 * (CddpmEngine.augment_slices). */
#define CDDPM_AUG_GAMMA 1
#define CDDPM_AUG_BIAS 2
#define CDDPM_AUG_BLUR 4
#define CDDPM_AUG_GHOST 8
#define CDDPM_AUG_ALL 15
#define CDDPM_AUG_META 4
#define CDDPM_AUG_PAR 28
#define CDDPM_AUG_PAR_GAMMA 0
#define CDDPM_AUG_PAR_SIGMA 1            /* 1, 2, 3: axes 0, 1, 2 */
#define CDDPM_AUG_PAR_INTENSITY 4
#define CDDPM_AUG_PAR_COEF 5
#define CDDPM_AUG_BIAS_COEFS 20
#define CDDPM_AUG_MAX_AXIS 1024
#define CDDPM_AUG_MAX_BATCH 65535
#define CDDPM_AUG_MAX_SIGMA 8            /* in voxels: radius 32 */
#define CDDPM_AUG_MAX_RADIUS 32
#define CDDPM_AUG_BAD_VOLUME 1           /* status bits of a sample */
#define CDDPM_AUG_BAD_Z 2
#define CDDPM_AUG_BAD_AXIS 4
#define CDDPM_AUG_BAD_SIGMA 8
#define CDDPM_AUG_BAD_FLAGS 16
#define CDDPM_AUG_BAD_VALUE 32

/* workspace bytes of cddpm_aug_slices for B samples of an H x W x D bank: the status words, the per-sample weight tables and two
 * work volumes per sample. Host arithmetic, callable without a GPU. Outside the supported range: 0, with the reason in
 * cddpm_last_error(NULL). */
size_t cddpm_aug_workspace_bytes(int B, int H, int W, int D);

/* out_dev [B][H][W] fp32: sample b is slice z_b of volume_b after the stages its flags select. Runs on `stream`; nothing
 * allocates or synchronises inside. A sample's result depends on its own table row alone and its arithmetic runs in a fixed
 * order: bitwise reproducible, and independent of the batch it is computed in. */
int cddpm_aug_slices(cddpm_handle h, const float* bank_dev, int N, int H, int W, int D, const int32_t* meta_dev, const float* par_dev,
                     int B, void* ws_dev, size_t ws_bytes, float* out_dev /* [B][H][W] */, void* stream);

/* ---- The augmentation pipeline (csrc/augment.hip) -------------------------------------------------------
 * get_augment (src/datamodules/create_dataset.py:220-250) composes its transforms in one fixed order, the individual keys first,
 * then the `aug_intensity` policy group. This entry is that order as ELEVEN STAGE SLOTS, each gated per sample by one flag bit and
 * with parameters of its own (the reference's probabilities in brackets; the draws are the caller's, augment.SliceAugment.draw):
 *   random_bias (.25) . random_noise (.5) . random_ghosting (.5) . random_blur (.5) . random_gamma (.5) . random_affine (.5) .
 *   random_flip (.5) . policy gamma (.5) . policy bias (.25) . policy blur (.25) . policy ghosting (.5)
 * then vol2slice's one slice. random_motion (before the noise) and random_elastic (before the affine) are NOT built: their rules
 * live in a k-space composite and in SimpleITK's B-spline transform. Mask and label volumes are not transformed: the training step
 * reads `vol` only. Status: PINNED TO NUMPY / SCIPY, UNPINNED TO TORCHIO AND SIMPLEITK (tests/augment_pipeline_reference.py).
 * Bank, axis numbers, extents, the stream and the allocation rule, the status words at the head of the workspace and the -1
 * errors are those of cddpm_aug_slices above; a flagged sample's output is never written.
 *   meta_dev [B][CDDPM_PIPE_META] int32: {volume, z, flags, g | axis << 8 of the ghosting slot, g | axis << 8 of the policy
 *            ghosting, key0, key1, unused} -- key0 and key1 are the two Philox key words of the noise stage.
 *   par_dev  [B][CDDPM_PIPE_PAR] fp32: {slot set [25], policy set [25], noise std, M[9], 4 unused}. A set is the 25 columns
 *            {gamma, sigma0, sigma1, sigma2, I, c[20]} of cddpm_aug_slices' par (CDDPM_AUG_PAR_* from the set's first column):
 *            the slot set at CDDPM_PIPE_PAR_SLOT serves the individual bias, ghosting, blur and gamma, the policy set at
 *            CDDPM_PIPE_PAR_POLICY the policy group. M is the affine's row-major 3 x 3 matrix over the axes (H, W, D).
 * Stages. Every one computes in double and rounds to fp32 once; flags = 0 is a bit-exact copy of the slice.
 *   CDDPM_PIPE_BIAS, _BLUR, _GAMMA   the rules of CDDPM_AUG_BIAS, _BLUR, _GAMMA with the slot set; bias and gamma are passes of
 *                    their own here (the noise, ghosting and blur slots lie between them).
 *   CDDPM_PIPE_GHOST the rule of CDDPM_AUG_GHOST with the slot set, evaluated at EVERY voxel, since later stages read them all:
 *                    about n L double multiply-adds per sample for n voxels and an axis of L.
 *   CDDPM_PIPE_NOISE y = x + std n(v), mean 0 (torchio's RandomNoise draws std from U(0, 0.25)). v is the voxel's index in the
 *                    bank's memory order, (d H + h) W + w. Philox4x32-10 keyed by (key0, key1) at the counter
 *                    (v / 4, 0, 0, 0x6002) gives four words; u = ((word >> 9) + 0.5) 2^-23; the quad's four normals are
 *                    r_a cos(2 pi u_1), r_a sin(2 pi u_1), r_b cos(2 pi u_3), r_b sin(2 pi u_3) with r_a = sqrt(-2 ln u_0),
 *                    r_b = sqrt(-2 ln u_2) (the order of synth.normal_quads), and voxel v takes number v % 4. The rule is the
 *                    real-number function of the two uniforms, evaluated in double. std = 0 leaves the volume bit for bit.
 *   CDDPM_PIPE_AFFINE torchio's RandomAffine with its defaults: scales U(0.9, 1.1) and degrees U(-10, 10) per axis, no
 *                    translation, centre of the image, linear interpolation, default_pad_value = 'minimum'. The caller builds
 *                    R = Rz Rx Ry (ITK's Euler3DTransform order) in float64 and the output-to-source voxel matrix
 *                    M = diag(1 / s) diag(1 / scales) R^T diag(s), s the voxel spacing, and rounds M to fp32 into the table. For
 *                    the output voxel p the source point is q = c + M (p - c) in double, c = (L - 1) / 2 per axis. q is inside
 *                    iff -0.5 <= q_a <= L_a - 0.5 on all three axes. Inside: trilinear interpolation in double over floor(q)
 *                    and floor(q) + 1, both clamped to [0, L - 1]. Outside: the minimum of the volume being transformed (the
 *                    sample's volume after the earlier slots), an exact reduction computed only when the bit is set; volumes are
 *                    taken to be finite. Whether a positive angle turns as torchio's does (RAS against LPS) cannot be pinned
 *                    here; the draw is symmetric about 0, so either sign has the same distribution.
 *   CDDPM_PIPE_FLIP  RandomFlip(axes = 0): y[h] = x[H - 1 - h], exact. One gather serves affine and flip: with both bits set the
 *                    output voxel p takes the affine's sample at flip(p), which is the flip applied to the affine's output.
 *   CDDPM_PIPE_POLICY_GAMMA, _BIAS, _BLUR, _GHOST   cddpm_aug_slices' four stages with the policy set: a row with only these bits
 *                    gives that entry's output for the corresponding four-bit row, bit for bit.
 * A row is flagged as there (CDDPM_AUG_BAD_* bits; the axis and sigma checks cover both sets, the value check also the std and M). */
#define CDDPM_PIPE_BIAS 1
#define CDDPM_PIPE_NOISE 2
#define CDDPM_PIPE_GHOST 4
#define CDDPM_PIPE_BLUR 8
#define CDDPM_PIPE_GAMMA 16
#define CDDPM_PIPE_AFFINE 32
#define CDDPM_PIPE_FLIP 64
#define CDDPM_PIPE_POLICY_GAMMA 128
#define CDDPM_PIPE_POLICY_BIAS 256
#define CDDPM_PIPE_POLICY_BLUR 512
#define CDDPM_PIPE_POLICY_GHOST 1024
#define CDDPM_PIPE_ALL 2047
#define CDDPM_PIPE_META 8
#define CDDPM_PIPE_META_GHOST 3
#define CDDPM_PIPE_META_POLICY_GHOST 4
#define CDDPM_PIPE_META_KEY 5            /* 5, 6 */
#define CDDPM_PIPE_PAR 64
#define CDDPM_PIPE_PAR_SLOT 0
#define CDDPM_PIPE_PAR_POLICY 25
#define CDDPM_PIPE_PAR_NOISE_STD 50
#define CDDPM_PIPE_PAR_MATRIX 51         /* 51 ... 59 */

/* workspace bytes of cddpm_aug_pipeline: as cddpm_aug_workspace_bytes, with the tables of two parameter sets. Host arithmetic,
 * callable without a GPU; outside the supported range: 0, with the reason in cddpm_last_error(NULL). */
size_t cddpm_aug_pipeline_workspace_bytes(int B, int H, int W, int D);

/* out_dev [B][H][W] fp32: sample b is slice z_b of volume_b after the slots its flags select. Runs on `stream`; nothing allocates
 * or synchronises inside. A sample's result depends on its own table row alone and its arithmetic runs in a fixed order: bitwise
 * reproducible, and independent of the batch it is computed in. */
int cddpm_aug_pipeline(cddpm_handle h, const float* bank_dev, int N, int H, int W, int D, const int32_t* meta_dev, const float* par_dev,
                       int B, void* ws_dev, size_t ws_bytes, float* out_dev /* [B][H][W] */, void* stream);

/* ---- Preprocessed volumes (csrc/preprocess.hip) ------------------------------------------------------------
 * Replaces what the reference's datamodule does to a volume on the CPU before it is cached (Train) or handed to test_step (Eval,
 * which has no cache, src/datamodules/create_dataset.py:52-92): sitk_reader's CurvatureFlow (:252-258) and get_transform's
 * CropOrPad, RescaleIntensity and Resample (:196-218). Status: PINNED TO NUMPY / SCIPY, UNPINNED TO TORCHIO AND SIMPLEITK. The
 * rules below restate torchio >=0.18.90,<0.19 and ITK from recollection; neither was available to compare with, numpy and scipy
 * were (tests/preprocess_reference.py). Reading NIfTI files is not built.
 * The input is a C-contiguous [H][W][D] fp32 volume (torchio's layout), label volumes are uint8 of the same shape. Axis numbers
 * keep torchio's meaning: 0 = H, 1 = W, 2 = D. The output is slice-major [D'][H'][W'] (the layout of augment.VolumeBank), labels
 * uint8 in the same layout, written directly at the destination the caller names. Every extent is 1 ... CDDPM_PREP_MAX_AXIS.
 * Stages, in the reference's order; a call with no stage set is a bit-exact copy into the output layout:
 *   CDDPM_PREP_SMOOTH    sitk.CurvatureFlow(timeStep = dt, numberOfIterations): per iteration v <- v + dt u, stored as fp32. With
 *                        s_i = 1 / spacing_i, central differences and neighbours clamped to the edge:
 *                        dx_i = (v+i - v-i) s_i / 2, dxx_i = (v+i - 2 v + v-i) s_i^2, dxy_ij = (v++ - v+- - v-+ + v--) s_i s_j / 4,
 *                        m = sum dx_i^2, u = 0 where m < 1e-9, else
 *                        u = (sum_i dxx_i sum_{j != i} dx_j^2 - 2 sum_{i<j} dx_i dx_j dxy_ij) / m, evaluated in double.
 *                        Images only, never label volumes.
 *   CDDPM_PREP_CROPPAD   tio.CropOrPad((th, tw, td), padding_mode = 0): per axis delta = target - size; padding |delta| puts
 *                        ceil(|delta| / 2) zeros in front and floor(|delta| / 2) behind, cropping removes voxels in the same split.
 *                        The same bounds for image and labels.
 *   CDDPM_PREP_RESCALE   tio.RescaleIntensity((0, 1), percentiles = (lo, hi), masking_method = mask): values = vol[mask > 0] (n of
 *                        them, after the stages above; a NULL mask is vol > 0); per percentile p, v = p (n - 1) / 100, k = floor(v):
 *                        cutoff = numpy's linear interpolation between the order statistics k and min(k + 1, n - 1) at v - k, an
 *                        exact selection on the device; the whole volume is clipped to the cutoffs and [min, max] of the clipped
 *                        volume mapped to [0, 1], y = (clip(x) - min) / (max - min), in double. An empty mask or max == min leaves
 *                        the volume unchanged (torchio warns and returns) and sets CDDPM_PREP_UNCHANGED with its reason.
 *   CDDPM_PREP_RESAMPLE  tio.Resample(f, image_interpolation = 'bspline') at input spacing 1: output size ceil(N / f) per axis,
 *                        output voxel i samples x = (i + 1/2) f - 1/2. Images: scipy.ndimage.map_coordinates(order = 3,
 *                        mode = 'mirror') with its prefilter (pole sqrt(3) - 2, axes 0, 1, 2), coefficients and the 64 taps in
 *                        double, rounded once. Labels: the nearest voxel floor(x + 1/2). A sample point outside [-1/2, N - 1/2)
 *                        gives 0 (ITK's default pixel). f = 1 skips the stage.
 * par_host [CDDPM_PREP_PAR] float64, a HOST array: {dt, spacing0, spacing1, spacing2, perc_lo, perc_hi, f, unused}.
 * record_dev [CDDPM_PREP_RECORD] float64 is written by every call that is enqueued: the status bits, the mask count, the four
 * order statistics (low k, low k + 1, high k, high k + 1; -0.0 is reported as +0.0), both cutoffs, min and max of the clipped volume;
 * slots the call's stages do not compute are 0. A non-finite input value sets CDDPM_PREP_BAD_VALUE: no output is then written.
 * Errors: -1 with the reason in cddpm_last_error(h), before anything is enqueued, for what the host can see -- a NULL pointer,
 * an extent or target outside 1 ... CDDPM_PREP_MAX_AXIS, unknown stage bits, percentiles outside 0 <= lo <= hi <= 100, f < 1,
 * RESAMPLE with f != 1 on an axis of length 1 (its rule is not recalled with confidence), dt, spacing or f not finite, spacing
 * <= 0, iterations outside 0 ... CDDPM_PREP_MAX_ITERATIONS, a short workspace, output equal to input. */
#define CDDPM_PREP_SMOOTH 1
#define CDDPM_PREP_CROPPAD 2
#define CDDPM_PREP_RESCALE 4
#define CDDPM_PREP_RESAMPLE 8
#define CDDPM_PREP_ALL 15
#define CDDPM_PREP_MAX_AXIS 1024
#define CDDPM_PREP_MAX_ITERATIONS 64
#define CDDPM_PREP_PAR 8
#define CDDPM_PREP_PAR_DT 0
#define CDDPM_PREP_PAR_SPACING 1         /* 1, 2, 3: axes 0, 1, 2 */
#define CDDPM_PREP_PAR_PERC_LO 4
#define CDDPM_PREP_PAR_PERC_HI 5
#define CDDPM_PREP_PAR_FACTOR 6
#define CDDPM_PREP_BAD_VALUE 1           /* status bits: a non-finite input value (the output is not written) */
#define CDDPM_PREP_BAD_MASK 2            /* rescale: the mask is empty */
#define CDDPM_PREP_BAD_RANGE 4           /* rescale: max == min after clipping */
#define CDDPM_PREP_UNCHANGED 8           /* rescale: the volume went on unchanged (set with BAD_MASK or BAD_RANGE) */
#define CDDPM_PREP_RECORD 16             /* slots of the record (float64) */
#define CDDPM_PREP_REC_STATUS 0
#define CDDPM_PREP_REC_COUNT 1
#define CDDPM_PREP_REC_STAT 2            /* 2 ... 5 */
#define CDDPM_PREP_REC_CUT_LO 6
#define CDDPM_PREP_REC_CUT_HI 7
#define CDDPM_PREP_REC_MIN 8
#define CDDPM_PREP_REC_MAX 9

/* workspace bytes of cddpm_prep_volume for an H x W x D input, these stages, target (th, tw, td) (read under CROPPAD) and factor f
 * (read under RESAMPLE): state words, tap tables, two fp32 work volumes under SMOOTH, one float64 coefficient volume under
 * RESAMPLE with f != 1. Host arithmetic, callable without a GPU. Outside the supported range: 0, with the reason in
 * cddpm_last_error(NULL). */
size_t cddpm_prep_workspace_bytes(int H, int W, int D, int stages, int th, int tw, int td, double f);

/* out_dev [D'][H'][W'] fp32; mask_dev [H][W][D] uint8 or NULL (vol > 0 after SMOOTH); mask_out_dev [D'][H'][W'] uint8 or NULL: the
 * mask through CROPPAD and RESAMPLE. Runs on `stream`; nothing allocates or synchronises inside; reductions across workgroups
 * are integer atomics: bitwise reproducible. */
int cddpm_prep_volume(cddpm_handle h, const float* vol_dev, const uint8_t* mask_dev, int H, int W, int D, int stages, int iterations,
                      int th, int tw, int td, const double* par_host, void* ws_dev, size_t ws_bytes, float* out_dev,
                      uint8_t* mask_out_dev, double* record_dev, void* stream);

/* a label volume (mask, segmentation) through CROPPAD and RESAMPLE alone (other stage bits are refused): out_dev [D'][H'][W'] uint8 */
int cddpm_prep_labels(cddpm_handle h, const uint8_t* lab_dev, int H, int W, int D, int stages, int th, int tw, int td, double f,
                      uint8_t* out_dev, void* stream);

/* Replaces q_sample (src/models/modules/cond_DDPM.py:548-554) fused with normalize_to_neg_one_to_one (:75):
 * out = sqrt_ac[t_b] * (2 x01 - 1) + sqrt_1mac[t_b] * noise; coefficient tables are host arrays [T]
 * uploaded on first use. Used by the single-step reconstruction (GaussianDiffusion.forward, :647-655). t_b = t_dev[b] kept inside
 * [0, T) when t_dev is given, else t_uniform for every slice. One fused multiply-add over the rounded second product per element.
 * Preconditions, each refused with a message before anything is enqueued: T the handle's timesteps; 1 <= B <= max_batch; H, W >= 1;
 * H * W a multiple of 4; B * H * W < 2^31; no NULL argument; x01_dev, noise_dev and out_dev 16-byte aligned; t_uniform inside
 * [0, T) when t_dev is NULL. */
int cddpm_q_sample(cddpm_handle h, const float* x01_dev, const float* noise_dev, const int32_t* t_dev, int t_uniform,
                   const float* sqrt_ac_host, const float* sqrt_1mac_host, int T,
                   float* out_dev, int B, int H, int W, void* stream);

/* ---- the patched DDPM (src/models/DDPM_2D_patched.py, src/utils/patch_sampling.py) ----------------
 * Boxes are device int32 rows (x0, y1, x2, y3): columns [x0, x2) and rows [y1, y3), the reference's convention, 16-byte aligned.
 * They are clipped to the image as Python slicing clips a non-negative range (sample_single_box yields boxes that run past the
 * right and bottom edge); a box that is empty after clipping is legal and selects nothing. Coordinates are not negative.
 * All three entries only enqueue work on `stream`: no allocation, no synchronisation, fixed-order arithmetic (bitwise reproducible).
 *
 * q_sample of the box alone (cond_DDPM.py:587-604) for N output slices over S source slices, N % S == 0: out_dev [N][H][W], slice n
 * reads x01_dev / noise_dev [S][H][W] at slice n % S. Outside its box it is 2 x01 - 1, inside sqrt_ac[t] (2 x01 - 1) + sqrt_1mac[t]
 * noise with the arithmetic of the q_sample entry above, to the bit. t as there: t_dev [S] int32 (slice n: t_dev[n % S], kept
 * inside [0, T)) or NULL for t_uniform. The coefficient tables are DEVICE arrays [T]: nothing is staged through the handle, so N is
 * not bound by max_batch and the call serves the training step (whose handle has no schedule). */
int cddpm_box_q_sample(cddpm_handle h, const float* x01_dev, const float* noise_dev, const int32_t* t_dev, int t_uniform,
                       const float* sqrt_ac_dev, const float* sqrt_1mac_dev, int T, const int32_t* box_dev, float* out_dev,
                       int S, int N, int H, int W, void* stream);
/* The stitching of DDPM_2D_patched.test_step (:175-215) after its last box, as written: reco_dev [K S][H][W] box-major (n = k S + s),
 * box_dev [K S][4], cut_dev [K S][4] (the sample_grid_cut rows; read by CDDPM_STITCH_CUT only, NULL otherwise) -> out_dev [S][H][W].
 * Every pixel walks k = 0 .. K - 1 in order from 0. PASTE: the value becomes reco_k where box k covers the pixel; CUT: the same with
 * the cut rows; a pixel in no box stays 0. AVG: v <- (v + [pixel in box k] reco_k) / count after EVERY box, count = the number of
 * boxes covering the pixel -- the reference divides the running image by the full mask inside its loop over boxes, so K boxes divide
 * K times (pinned by tests/golden/patched); a pixel in no box is 0 / 0, as torch gives it. */
#define CDDPM_STITCH_PASTE 0
#define CDDPM_STITCH_CUT 1
#define CDDPM_STITCH_AVG 2
int cddpm_box_stitch(cddpm_handle h, const float* reco_dev, const int32_t* box_dev, const int32_t* cut_dev, int mode, float* out_dev,
                     int S, int K, int H, int W, void* stream);

/* ---- measurement ------------------------------------------------------------------------------- */
/* Per-kernel-class timing with HIP events recorded on the launch stream around every kernel (bench.py's
 * roofline leg). Classes: 0 = fused 3x3 conv (MFMA), 1 = 1x1 conv (MFMA), 2 = attention core,
 * 3 = GroupNorm statistics+coefficients, 4 = other (input conv, head, pooling). cddpm_get_profile
 * synchronises, sums elapsed ms / algorithmic FLOPs / algorithmic bytes / launch counts per class since the
 * last call, and clears the records. */
#define CDDPM_PROF_CLASSES 5
int cddpm_set_profiling(cddpm_handle h, int on);
int cddpm_get_profile(cddpm_handle h, int ncls, double* ms, double* flops, double* bytes, int64_t* launches);

/* ---- test / debug surface (used by tests/ only) ------------------------------------------------- */

/* number of blocks in the forward program and their names ("input_blocks.3", "middle_block.1", ...) */
int cddpm_num_blocks(cddpm_handle h);
const char* cddpm_block_name(cddpm_handle h, int i);
/* ask the next cddpm_unet_forward calls to copy block i's output (NHWC [B,h,w,C] fp32) to dst_dev
 * (NULL clears); channels/height/width of that output for the given input size via cddpm_block_shape */
int cddpm_set_tap(cddpm_handle h, int block, float* dst_dev);
int cddpm_block_shape(cddpm_handle h, int block, int H, int W, int* C, int* h_out, int* w_out);

/* standalone fused convolution on NHWC tensors (the kernel behind every ResBlock conv), for kernel tests:
 * out[B,H,W,Cout] = conv_k(act(cat[src0,src1])) + bias (+ res), k in {1,3}, zero padding k/2, optional
 * nearest x2 upsampling of the sources (srcs are then [B,H/2,W/2,*]; upsample = 1: gather form, 2: the folded form the
 * UNet uses -- four 2x2-tap convolutions of the low-resolution input with pre-summed weights) and of the residual.
 * act(v) = silu?( (v - mean[b,c]) * a[b,c] + d[b,c] ) when coef_dev != NULL (coef_dev = [3][B][Cin]: mean, a, d).
 * w_host is PyTorch layout [Cout,Cin,k,k]. */
int cddpm_op_conv(cddpm_handle h, const float* src0_dev, int C0, const float* src1_dev, int C1,
                  const float* coef_dev, int silu, int upsample,
                  const float* w_host, const float* bias_host, int Cout, int ksize,
                  const float* res_dev, int res_upsample,
                  float* out_dev, int B, int H, int W, void* stream);

/* the ResBlock output convolution with its fused 1x1 skip_connection (OpenAI_Unet.py:261-268, :338): out = conv3x3(
 * act(src)) + conv1x1(skip) + bias, the skip operand RAW (un-normalised residual stream), both weight tensors packed
 * under one pre-scale exponent as cddpm_load_weights does. skip_dev [B,H,W,S0], wskip_host [Cout,S0,1,1]. Kernel tests. */
int cddpm_op_conv_skip(cddpm_handle h, const float* src0_dev, int C0, const float* coef_dev, int silu,
                       const float* w_host, const float* bias_host, int Cout, const float* skip_dev, int S0,
                       const float* wskip_host, float* out_dev, int B, int H, int W, void* stream);

/* a 3x3 convolution whose epilogue writes the GroupNorm statistics records of its output, followed by gn_finalize:
 * out_dev [B,H,W,Cout] = conv3x3(src) + bias and coef_dev [3][B][Cout] = (mean, a, d) of GroupNorm32(out) with
 * gamma/beta -- the statistics path every ResBlock uses (records from the producer, never a re-read). Kernel tests. */
int cddpm_op_conv_gn(cddpm_handle h, const float* src0_dev, int C0, const float* w_host, const float* bias_host, int Cout,
                     const float* gamma_host, const float* beta_host, float* out_dev, float* coef_dev, int B, int H, int W,
                     void* stream);

/* host-only (no GPU): the split-K rule of the small-batch plan as a function of its inputs -- the convolution family (CDDPM_CONV_*),
 * the layer's workgroup count of the 128-cout form at the HANDLE's maximum geometry (max_batch x [4 parity classes of the folded
 * upsample] x ceil(w / 32) x ceil(h / 8) x Cout / 128, w x h the layer's extent at max_h x max_w, halved for the folded form), the
 * channels of the main segment (Cin = C0 + C1) and of the 1x1 skip segment (Cskip = S0 + S1, or 0; multiples of 32) and the taps per
 * main chunk (1, 9, or 4 = folded upsample). Returns S, the number of consecutive ranges the K loop's 32-channel chunks (main
 * segment first, then skip) are cut into: a power of two <= CDDPM_MAX_KSPLIT with S * workgroups <= 256, 1 = not split and always 1
 * outside CDDPM_CONV_H3. kbound_out [CDDPM_MAX_KSPLIT + 1]: range j is chunks kbound_out[j] .. kbound_out[j + 1] - 1, with
 * kbound_out[0] = 0 and kbound_out[S] = (Cin + Cskip) / 32; entries beyond S are 0. -1 on bad arguments. The code every convolution of
 * cddpm_unet_forward / cddpm_reverse is planned with. */
#define CDDPM_MAX_KSPLIT 8
int cddpm_conv_ksplit_plan(int family, long long workgroups_at_max, int Cin, int Cskip, int taps, int* kbound_out);

/* one fused convolution launched as the HANDLE plans it inside its forward program -- the union of cddpm_op_conv, cddpm_op_conv_skip
 * and cddpm_op_conv_gn, but through the planning path of cddpm_unet_forward / cddpm_reverse instead of a direct kernel launch: split-K
 * ranges + the fixed-order combine (bias, residual and statistics records then come from the combine kernel) at small maximum
 * geometries, the 128- or 256-cout workgroup form otherwise, plain fp16 operands on a handle at precision 16. Kernel tests.
 *   out[B,H,W,Cout] = conv_k(act(cat[src0, src1])) + bias + (res | conv1x1(cat[skip0, skip1])),  k in {1, 3}
 * folded_up: the folded nearest-x2-upsample form (sources [B,H/2,W/2,C0]; k = 3, single source, no skip segment). res_dev at the
 * output's resolution, or half of it with res_upsample. The skip segment (k = 3 only, instead of a residual) reads two RAW tensors
 * skip0_dev [B,H,W,S0] and skip1_dev [B,H,W,S1] (S1 = 0: one) under ONE weight tensor wskip_host [Cout, S0 + S1, 1, 1], packed with
 * the main tensor's pre-scale exponent as cddpm_load_weights does. gamma_host / beta_host / coef_out_dev (all three or none; Cout <=
 * 1024): coef_out_dev [3][B][Cout] = (mean, a, d) of GroupNorm32(out) from the statistics records of whichever epilogue the plan used.
 * The plan is that of a layer of H x W inside a forward of B <= max_batch slices at img_H x img_W <= max_h x max_w; t >= 0: the
 * accumulation plan of reverse step t (cddpm_set_accumulation_switch), t < 0: that of a single forward. The handle's state is
 * restored before the call returns. The plan taken comes back through (each may be NULL) ksplit_out = S, kbound_out
 * [CDDPM_MAX_KSPLIT + 1] as cddpm_conv_ksplit_plan fills it, nb2_out = 1 when 256-cout workgroups ran, scale_exp_out = the pre-scale
 * exponent of the packed weights (0 outside CDDPM_CONV_H3). Synchronises the stream. */
int cddpm_op_conv_planned(cddpm_handle h, const float* src0_dev, int C0, const float* src1_dev, int C1, const float* coef_dev, int silu,
                          int folded_up, const float* w_host, const float* bias_host, int Cout, int ksize, const float* res_dev,
                          int res_upsample, const float* skip0_dev, int S0, const float* skip1_dev, int S1, const float* wskip_host,
                          const float* gamma_host, const float* beta_host, float* coef_out_dev, float* out_dev, int B, int H, int W,
                          int img_H, int img_W, int t, int* ksplit_out, int* kbound_out, int* nb2_out, int* scale_exp_out, void* stream);

/* standalone GroupNorm(32) statistics + coefficient kernel pair: coef_dev [3][B][C] (mean, a, d) with
 * a = rstd*gamma*(1+scale), d = beta*(1+scale)+shift; film_dev = [B][2C] (scale | shift) or NULL. */
int cddpm_op_gn_coef(cddpm_handle h, const float* src0_dev, int C0, const float* src1_dev, int C1,
                     const float* gamma_host, const float* beta_host, const float* film_dev,
                     float* coef_dev, int B, int HW, void* stream);

/* host-only: the packed weight image of one convolution as the process default family (CDDPM_CONV) expects it (no GPU needed; handle-less,
 * so a handle's own family does not enter).
 * format = 2: conv_x6.hip, fp16 split (default) -- w * 2^e (e = *scale_exp_out, the largest exponent <= 24 that keeps
 *   max|w| * 2^e below 2^14) split into two fp16 terms, hi + mid == w * 2^e to within 2^-23 relative (rms 0.73 x 2^-24);
 *   [Cout/128][Cin/32][taps][128 rows][8 slots of 8 fp16], slot (split s, u = channel/8 in the 32-channel chunk) of
 *   row j at (4 s + u) ^ ((j >> 1) & 7); 4 bytes per weight.
 * format = 1: conv_x6.hip, bf16 split (CDDPM_CONV=x6) -- three bf16 terms, hi + mid + lo == w exactly in fp32;
 *   [..][128 rows][12 slots of 8 bf16], slot (s, u) of row j at 4 s + (u ^ ((j >> 2) & 3)); 6 bytes per weight.
 * format = 0: conv_mfma.hip (CDDPM_CONV=f32) -- fp32, [..][128 rows][8 slots of 4 floats], slot s of row j at
 *   s ^ ((j >> 1) & 7); 4 bytes per weight.
 * cddpm_packed_conv_bytes returns the image size; cddpm_pack_conv_weights fills dst_host (that many bytes) from
 * PyTorch-layout w_host [Cout][Cin][k][k] (taps = k*k in {1, 9}; the size query also takes 4, one folded-upsample class) and returns
 * the format, or -1 on a bad shape. */
size_t cddpm_packed_conv_bytes(int Cout, int Cin, int taps);
int cddpm_pack_conv_weights(const float* w_host, int Cout, int Cin, int taps, void* dst_host, int* scale_exp_out);

/* ---- the training step (csrc/train_kernels.hip, csrc/encoder_train.hip, csrc/batchnorm_train.hip): the operators that the host
 *      sequencing of the package (training.py, encoder_training.py) strings into src/models/DDPM_2D.py:114-135 -> cond_DDPM.py:565-645
 *      with gradients, Adam (:305-306) and the gradient all-reduce. Host-pointer variants (w_host ...) serve the kernel tests; the step
 *      itself runs on the device-resident calls further down (cddpm_op_pack_conv, cddpm_op_conv_packed, scratch arena). */
/* dL/d(input) of Conv2d(k in {1,3}, padding k/2): dx[B,H,W,Cin] = conv_k(dy[B,H,W,Cout], w transposed in (Cout,Cin) and flipped in
 * (ky,kx)) -- the fused forward convolution kernel on host-repacked weights. w_host is the FORWARD weight [Cout,Cin,k,k];
 * Cin must be a multiple of 128 and Cout of 32 (true for every convolution inside the UNet). */
int cddpm_op_conv_dgrad(cddpm_handle h, const float* dy_dev, int Cout, const float* w_host, int Cin, int ksize, float* dx_dev,
                        int B, int H, int W, void* stream);
/* dL/d(weight), dL/d(bias) of y = Conv2d(k in {1,3}, padding k/2) applied to a = act(cat[x0, x1]) with act(v) = silu?((v - mean) *
 * a + d) as in cddpm_op_conv (coef_dev [3][B][C0 + C1] or NULL): dw_dev [Cout,Cin,k,k] (PyTorch layout) = sum over batch and pixels of
 * dy (x) a, db_dev [Cout] = sum of dy (may be NULL). x0_dev [B,H,W,C0], x1_dev [B,H,W,C1] or NULL (C1 = 0), dy_dev [B,H,W,Cout];
 * C0 + C1 a multiple of 32, C0 of 32 when C1 > 0, Cout of 64. upsample != 0:
 * the conv input is the nearest x2 upsampling of act(x0) (up ResBlocks, OpenAI_Unet.py:289-293): x0_dev is [B,H/2,W/2,C0], H and W even.
 * Arithmetic (cddpm_set_train_precision): 32 = products from two-term fp16 splits of both operands on v_mfma_f32_16x16x32_f16, fp32
 * accumulation -- the forward kernel's arithmetic; 16 = plain fp16 operands. */
int cddpm_op_conv_wgrad(cddpm_handle h, const float* x0_dev, int C0, const float* x1_dev, int C1, const float* coef_dev, int silu,
                        int upsample, const float* dy_dev, int Cout, int ksize, float* dw_dev, float* db_dev, int B, int H, int W,
                        void* stream);
/* db_dev[C] = sum over the npix rows of dy_dev [npix][C] (bias gradient of a convolution) */
int cddpm_op_bias_grad(cddpm_handle h, const float* dy_dev, int64_t npix, int C, float* db_dev, void* stream);
/* backward of the attention core QKVAttention (src/models/modules/OpenAI_Unet.py:457-476): qkv_dev [B,N,3C] (q | k | v, heads of 64
 * channels), da_dev [B,N,C] = dL/d(output) -> dqkv_dev [B,N,3C]. The probabilities are recomputed (flash-style: B x C/64 x N x 2
 * floats of scratch for the row statistics; nothing of size N x N is stored). C: a multiple of 64 (heads of 64 channels).
 * Tested against float64 autograd: C = 128 and 256, N = 16 ... 1536, multiples of neither the 128-query workgroup nor the 64-key tile
 * included (N = 240, 576; tests/test_gpu_train_ops.py, tests/test_gpu_attention_shapes.py), and inside the training step at N = 15 ... 1024
 * (tests/test_gpu_training*.py). Expected to hold, not checked against a reference: any N >= 1 with B x C/64 x ceil(N / 128) < 2^31
 * (the one-dimensional grid) -- tails are masked and every row offset is formed in 64 bits; N = 16384 (B 16, C 128) has been run and
 * timed only. */
int cddpm_op_attention_backward(cddpm_handle h, const float* qkv_dev, const float* da_dev, float* dqkv_dev, int B, int N, int C,
                                void* stream);
/* the same contract (arguments, scratch, errors, profiling class 2) in the arithmetic of fp16 autocast over QKVAttention.forward and
 * its backward, the backward of cddpm_op_attention_p16: q / 8, k, v and da are rounded to fp16 (RNE, gradual underflow) once; every
 * product runs on v_mfma_f32_32x32x16_f16 with fp32 accumulators (S, dP, dq, dk, dv); the running max / sum, P = exp(S - lse),
 * D_i = sum_c da_ic a_ic (rounded da, fp32 a) and dS = P (dP - D) are fp32; P and dS are rounded to fp16 only as MFMA operands; dqkv is
 * fp32. Range: |da| >= 65504 rounds to +-inf as under autocast and makes that sample's dqkv non-finite (what the training step's device
 * guard and the dynamic loss scale catch: da carries the loss scale), never a finite wrong number; other samples are unaffected.
 * Tested against float64 autograd by the rule of tests/precision16_cases.py (no further from it than torch's fp16 autocast is):
 * C = 64, 128, 256, N = 15 ... 1536, multiples of neither the 128-row workgroup nor the 64-row tile included (N = 130, 240;
 * tests/test_gpu_attention_backward_p16.py). Expected to hold as for cddpm_op_attention_backward: tails are masked and every row
 * offset is formed in 64 bits; N = 16384 (B 4, C 128) has been run and timed only. */
int cddpm_op_attention_backward_p16(cddpm_handle h, const float* qkv_dev, const float* da_dev, float* dqkv_dev, int B, int N, int C,
                                    void* stream);
/* the same contract (arguments, errors, profiling class 2) at fp32 accuracy on v_mfma_f32_32x32x16_f16, the backward of
 * cddpm_op_attention_h3 and in its arithmetic: all seven N x N x 64 products and the recomputed forward's two are three-term split
 * products (hi . hi + hi . lo + lo . hi), fp32 accumulators; the running max / sum, P, D and dS = P (dP - D) are fp32 VALU work; P
 * (lifted by 2^15) and dS (by 2^10) are split only as MFMA operands; dqkv is fp32.
 * da is normalised per SAMPLE: a pass in front takes the largest |da| of each sample as an integer maximum of the magnitude bits (no
 * float atomics: two calls give the same bits, and a sample's bits do not depend on its batch), the kernels work on da 2^-e with that
 * maximum in [1, 2), and 2^e returns in the stores -- the result is the same function of da 2^k for every k, loss scales included.
 * Scratch: cddpm_op_attention_backward_h3_scratch (the row statistics of cddpm_op_attention_backward_scratch and one uint32 per sample).
 * Range: as cddpm_op_attention_h3 for q, k, v; a non-finite da makes ALL of that sample's dqkv NaN; the lifted dS must stay below
 * 65504, i.e. |P (dP - D)| < 63 for the normalised da (|v| of order 1 gives at most ~10) -- beyond it that sample's dq and dk are
 * non-finite. Never a finite wrong number, never another sample.
 * Tested against float64 autograd under the rule of the exact operator (tests/test_gpu_attention_h3.py): its shapes and regimes,
 * da scaled by 2^-30 ... 2^10, and N = 16384 (C 64) on a subset of rows. */
int cddpm_op_attention_backward_h3(cddpm_handle h, const float* qkv_dev, const float* da_dev, float* dqkv_dev, int B, int N, int C,
                                   void* stream);
/* backward of torch.nn.Linear behind an optional SiLU, y = [SiLU](x) W^T + b (emb_layers / time_embed / label_emb,
 * OpenAI_Unet.py:201-207, :583-602): x_dev [M,K], w_dev [N,K], dy_dev [M,N] -> dw_dev [N,K], db_dev [N] (may be NULL), dx_dev [M,K]
 * (may be NULL). */
int cddpm_op_linear_backward(cddpm_handle h, const float* x_dev, const float* w_dev, const float* dy_dev, int M, int N, int K,
                             int silu_in, float* dw_dev, float* db_dev, float* dx_dev, void* stream);
/* small forward operators of the UNet as stand-alone entry points (the training step's host code sequences them; every pointer is a
 * device pointer, NHWC fp32): y[M,N] = [SiLU](x[M,K]) w[N,K]^T + b (torch.nn.Linear); input_blocks.0 Conv2d(1 -> C, 3x3) with w [C][9];
 * the head out.2 Conv2d(C -> 1, 3x3) on act(x) with w9 [9][C]; the down-ResBlock front end (hp = avgpool2(act(x)), xp = avgpool2(x)).
 * Each entry refuses, with a message (cddpm_last_error) and before anything is launched, what its kernel cannot compute:
 *   cddpm_op_linear   : M, N, K >= 1; K a multiple of 4 and x_dev, w_dev 16-byte aligned (the rows are read in quads of K);
 *   cddpm_op_conv_in1 : B, H, W >= 1 and B * H * W < 2^31 (one flat 32-bit pixel range); C a multiple of 64, at most 512;
 *   cddpm_op_head     : B, H, W >= 1; C a multiple of 32, at most the C whose 64 (C + 4) + 9 C staged floats fit a gfx950 workgroup's
 *                       160 KB of LDS (544);
 *   cddpm_op_pool_act : B >= 1; H, W even and >= 2; C a multiple of 4. */
int cddpm_op_linear(cddpm_handle h, const float* x_dev, const float* w_dev, const float* b_dev, int M, int N, int K, int silu_in,
                    float* y_dev, void* stream);
int cddpm_op_conv_in1(cddpm_handle h, const float* x_dev, const float* w_dev, const float* b_dev, float* out_dev, int B, int H, int W,
                      int C, void* stream);
int cddpm_op_head(cddpm_handle h, const float* x_dev, const float* coef_dev, const float* w9_dev, float bias, const float* bias_dev,
                  float* out_dev, int B, int H, int W, int C, void* stream);   /* bias_dev (device, 1 float) overrides bias when given */
int cddpm_op_pool_act(cddpm_handle h, const float* x_dev, const float* coef_dev, float* hp_dev, float* xp_dev, int B, int H, int W, int C,
                      void* stream);
/* resampling backward and accumulation: dx[B,H,W,C] (+)= scale * dyp[B,H/2,W/2,C] at (y/2, x/2) (AvgPool2d(2) backward: scale 1/4);
 * dxp[B,H/2,W/2,C] (+)= 2x2 block sums of dy (nearest x2 upsample backward); a += b (n floats, multiple of 4).
 * unpool2 / sumpool2: B >= 1, H and W even and >= 2, C a multiple of 4; anything else is refused with a message. */
int cddpm_op_unpool2(cddpm_handle h, const float* dyp_dev, float* dx_dev, int B, int H, int W, int C, float scale, int accumulate, void* stream);
int cddpm_op_sumpool2(cddpm_handle h, const float* dy_dev, float* dxp_dev, int B, int H, int W, int C, int accumulate, void* stream);
int cddpm_op_add_inplace(cddpm_handle h, float* a_dev, const float* b_dev, int64_t n, void* stream);
/* nn.Dropout(p) between the SiLU and the second convolution of every ResBlock (OpenAI_Unet.py:255), for training with dropout_unet > 0.
 * The mask is a pure function of its counters and is never stored: Philox4x32-10 (the generator of cddpm_noise_fill), key = seed, counter =
 * (element quad within the slice's [HW][C] tensor, step, global slice index slice0 + b, stream_id); word i of a quad's draw decides element
 * 4 quad + i, which is dropped iff word < floor(p 2^32); kept elements are multiplied by fp32(1 / (1 - p)). A slice's mask depends on its
 * global index only, never on the batch or the rank it is trained in. stream_id: synth.STREAM_DROPOUT + the ResBlock's ordinal.
 *   act_dropout:   out[b,q,c] = mask / (1 - p) * [SiLU]((x[b,q,c] - mean[b,c]) a[b,c] + d[b,c]) with coef_dev [3][B][C] = (mean, a, d) as
 *                  cddpm_op_gn_coef writes it; coef_dev NULL (silu must be 0): mask / (1 - p) * x. out_dev may be x_dev.
 *   dropout_scale: da *= mask / (1 - p) in place -- the backward, the mask drawn again from the same counters.
 * p outside [0, 1), NULL or not 16-byte aligned pointers, C % 4 != 0 or HW * C / 4 >= 2^32 are refused with a message. */
int cddpm_op_act_dropout(cddpm_handle h, const float* x_dev, const float* coef_dev, int silu, float* out_dev, uint64_t seed, uint32_t step,
                         uint64_t slice0, uint32_t stream_id, double p, int B, int HW, int C, void* stream);
int cddpm_op_dropout_scale(cddpm_handle h, float* da_dev, uint64_t seed, uint32_t step, uint64_t slice0, uint32_t stream_id, double p, int B,
                           int HW, int C, void* stream);
/* weight gradients of the two single-channel convolutions: dw_dev [C][9] = sum_{b,q} act(T)[b,q,c] * s[b, q + sign * tap]
 * (input conv: T = dL/d(output), s = the image, sign +1; head conv: T = the head's input, act = its GroupNorm + SiLU, s = dL/d(out),
 * sign -1), and the head's input gradient dact[b,q,c] = sum_tap w9[tap][c] dout[b, q - tap].
 * Both refuse B, H or W < 1 with a message; chan_image_corr: C a multiple of 64, sign +1 or -1; head_dgrad: C a multiple of 4. */
int cddpm_op_chan_image_corr(cddpm_handle h, const float* t_dev, const float* coef_dev, int silu, const float* s_dev, int sign, float* dw_dev,
                             int B, int H, int W, int C, void* stream);
int cddpm_op_head_dgrad(cddpm_handle h, const float* dout_dev, const float* w9_dev, float* dact_dev, int B, int H, int W, int C, void* stream);
/* p_losses' loss (cond_DDPM.py:636-645): loss_b_dev[b] = p2w[b] * mean_p |out - target|^(1|2) (their mean is the loss), dout_dev =
 * grad_scale * dL/d(out). grad_scale (a power of two, e.g. B * HW rounded) is the loss scale of the backward pass: the convolution
 * input-gradient kernels form their products from fp16 operand splits whose absolute floor is 2^-25, so the gradient tensors are carried
 * at O(1) magnitude (every backward operator is linear in them, the scaling is exact) and cddpm_op_adam divides it out again. */
int cddpm_op_loss(cddpm_handle h, const float* out_dev, const float* target_dev, const float* w_b_dev, int l2, int B, int HW, float grad_scale,
                  float* dout_dev, float* loss_b_dev, void* stream);
/* The loss of p_losses with a box (cond_DDPM.py:612-645), one box per slice (box_dev [B][4], the patched DDPM's rows above): x0_dev
 * is the image in [-1, 1]. The target is x0 (pred_noise = 0) or the noise inside the box and 0 outside (pred_noise = 1; noise_dev is
 * read then only). Under `inpaint` the compared tensor is out inside the box and x0 outside, so dout is 0 outside the box -- under
 * pred_noise the outside still adds |x0| or x0^2 to the value. The mean is over all H W pixels, times w_b. The loss scale is
 * grad_scale, or the device scale when scaler_dev is given (the scaled entry's block below). dout_dev may be NULL: the loss only. */
int cddpm_op_loss_box(cddpm_handle h, const float* out_dev, const float* x0_dev, const float* noise_dev, const int32_t* box_dev,
                      const float* w_b_dev, int pred_noise, int inpaint, int l2, int B, int H, int W, float grad_scale,
                      const int32_t* scaler_dev, float* dout_dev, float* loss_b_dev, void* stream);
/* one Adam update (DDPM_2D.py:305-306: lr 1e-4, torch defaults) of a flat parameter vector; step counts from 1; the gradient used is
 * g_dev * grad_unscale (1 / the loss scale) */
int cddpm_op_adam(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2,
                  float eps, int step, float grad_unscale, void* stream);
/* The guarded form of the update, entirely on the device: a step whose gradients hold inf / NaN is skipped and does not count. With a
 * fixed loss scale this is only the skip half of torch's GradScaler (the reference trainer's `precision: 16`,
 * configs/trainer/default.yaml:7); the dynamic scale is the scaler form below.
 * ctrl_dev: int32[8], zero-initialised by the caller once = {non-finite flag, optimizer step, skip, skipped so far, bits of
 * 1 - beta1^step, bits of 1 - beta2^step, 0, 0}. Per optimisation step: cddpm_op_grad_check on every gradient buffer (ORs the flag),
 * ONE cddpm_op_guard_commit (flag set: skip = 1, skipped += 1; else skip = 0, step += 1, bias corrections refreshed; flag cleared),
 * then cddpm_op_adam_guarded on every parameter buffer (a no-op when skip is set; step and bias corrections come from ctrl_dev).
 *
 * Dynamic loss scaling (torch's GradScaler: the scale backs off on a skipped step and grows after `interval` clean ones), the scale on the
 * device: scaler_dev = int32[4] = {bits of the fp32 loss scale, growth tracker, consecutive skipped steps, 0}, initialised by the caller
 * (scale a power of two; tracker and skips 0 for a fresh run). Per optimisation step, in this order:
 *   (a) cddpm_op_loss_scaled: cddpm_op_loss with the loss scale read from scaler_dev (dout_dev = scale * dL/d(out));
 *   (b) the backward pass, then cddpm_op_grad_check on every gradient buffer and ONE cddpm_op_guard_commit, as above;
 *   (c) cddpm_op_adam_scaled on every parameter buffer (UNet and encoder): cddpm_op_adam_guarded with gradient
 *       g_dev * extra_unscale / scale (extra_unscale: e.g. 1 / ranks for the mean over data-parallel ranks), the scale (a) was formed with;
 *   (d) ONE cddpm_op_scaler_update: torch._amp_update_scale_ from ctrl_dev's skip decision -- skipped: scale *= backoff, tracker = 0,
 *       skips += 1; else skips = 0, tracker += 1, and when it reaches `interval`: scale *= growth (kept only if finite), tracker = 0.
 * growth > 1 and backoff < 1 must be powers of two (refused otherwise): the scale stays one, 1 / scale is exact, and a step at scale S is
 * bit-identical to the fixed-scale calls with grad_scale = S and grad_unscale = extra_unscale / S. */
/* Arithmetic of the training operators, process-wide: 32 (default) = fp32-grade products from two-term fp16 splits; 16 = plain fp16
 * operands with fp32 accumulation in cddpm_op_conv_packed and cddpm_op_conv_wgrad -- what the reference trainer's `precision: 16`
 * (configs/trainer/default.yaml:7) computes under autocast; GroupNorm, embeddings, Adam and the master weights stay fp32 in both, and so
 * does attention unless the trainer asks otherwise: the training step calls cddpm_op_attention / cddpm_op_attention_backward at either
 * value, and cddpm_op_attention_p16 / cddpm_op_attention_backward_p16 only where its caller selects them (UNetTrainer's
 * attention_precision=16), independently of this setting. The context encoder's convolutions likewise: cddpm_op_enc_conv /
 * cddpm_op_enc_conv_wgrad are fp32 at either value, and cddpm_op_enc_conv_p16 / cddpm_op_enc_conv_wgrad_p16 run only where the caller
 * selects them (EncoderTrainer's precision=16).
 * Precision 16 rounds each operand to fp16 to nearest even with gradual underflow, as torch's .half(): measured on gfx950, the 16-bit
 * MFMA inputs keep fp16 subnormals (|x| < 2^-14 is carried to 2^-25, not flushed), in both operators and on either operand
 * (tests/test_gpu_train_ops_edges.py::test_precision16_keeps_fp16_subnormals).
 * Initial value: environment CDDPM_TRAIN_PRECISION (16 | unset). set returns the previous value, -1 for an unsupported `bits`.
 * The reconstruction entry points are not affected. */
int cddpm_set_train_precision(int bits);
int cddpm_get_train_precision(void);
int cddpm_op_grad_check(cddpm_handle h, const float* g_dev, int64_t n, int32_t* ctrl_dev, void* stream);
int cddpm_op_guard_commit(cddpm_handle h, int32_t* ctrl_dev, float beta1, float beta2, void* stream);
int cddpm_op_adam_guarded(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1,
                          float beta2, float eps, float grad_unscale, const int32_t* ctrl_dev, void* stream);
int cddpm_op_loss_scaled(cddpm_handle h, const float* out_dev, const float* target_dev, const float* w_b_dev, int l2, int B, int HW,
                         const int32_t* scaler_dev, float* dout_dev, float* loss_b_dev, void* stream);
int cddpm_op_adam_scaled(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1,
                         float beta2, float eps, float extra_unscale, const int32_t* ctrl_dev, const int32_t* scaler_dev, void* stream);
int cddpm_op_scaler_update(cddpm_handle h, const int32_t* ctrl_dev, int32_t* scaler_dev, float growth, float backoff, int interval,
                           void* stream);
/* ---- device-resident operator calls (what the training step runs on: no host staging, no synchronisation) ----
 * cddpm_op_set_scratch gives the handle an arena of `bytes` (0: release it) from which the operators of this header take their
 * temporaries instead of a hipMalloc / synchronise / hipFree per call; calls then only enqueue work on `stream` (one stream).
 * An operator that needs more than the arena holds fails with the size in cddpm_last_error.
 * Parameter vectors documented as *_host (GroupNorm gamma / beta) may be device pointers: they are then used where they lie.
 * cddpm_op_absmax: out_dev[0] = max |x| (the caller derives a tensor's power-of-two pre-scale from it: the largest e in [0, 24] with
 * max|w| 2^e < 2^14). cddpm_op_pack_conv: the packed image of cddpm_pack_conv_weights (format 2), written by a kernel from the device
 * tensor w_dev [Cout][Cin][k][k]; mode 0 = forward operator, 1 = the input-gradient operator (transposed, taps flipped: Cin outputs,
 * Cout inputs; cddpm_packed_conv_bytes(Cin, Cout, k*k) bytes), 2 = the four folded classes of "nearest x2 upsample -> conv3x3"
 * (4 * cddpm_packed_conv_bytes(Cout, Cin, 4) bytes; the class sums can reach 4 max|w|). Bit-identical to the host packer for the same
 * exponent. Default convolution family only.
 * Environment CDDPM_TRAIN_PRECISION=16 (read once per process): cddpm_op_conv_packed multiplies plain fp16 operands (the hi terms of the
 * images only, fp32 accumulation) and so does cddpm_op_conv_wgrad -- the arithmetic of the reference trainer's precision 16.
 * The reconstruction entry points (cddpm_reverse, cddpm_unet_forward, ...) are not affected.
 * cddpm_op_conv_packed: cddpm_op_conv / cddpm_op_conv_skip on such images: out = conv_k(act(cat[src0, src1])) [+ conv1x1(skip)] + bias
 * [+ res]; bias_dev NULL = none; skip_dev NULL = no skip segment (its image shares scale_exp); folded_up: src0 is at H/2 x W/2. */
int cddpm_op_set_scratch(cddpm_handle h, size_t bytes);
/* What ONE call of an operator takes from the arena, in bytes (every temporary rounded up to 256): host functions without a handle, a
 * stream or a device, run by the very code through which the operator takes its temporaries, so a caller sizes the arena as the
 * largest of them over the calls it will make on the handle. Arguments: the operator's own shape arguments, in the operator's order;
 * where a NULL pointer of the operator changes what it takes, a flag stands in for the pointer (has_src1: src1 given; has_rec: rec_dev
 * given). GroupNorm parameter vectors are taken to be on the device, as the trainers pass them (a vector given in HOST memory is
 * staged through the arena: 256-byte-rounded C floats more for each). A shape the operator refuses gives 0.
 * cddpm_op_conv_wgrad_scratch: precision 16 | 32 = the process-wide training precision to plan for, 0 = the current one
 * (cddpm_get_train_precision); 32 takes the most, so an arena sized for it serves either. db_dev does not change the request.
 * cddpm_op_attention_backward_scratch serves cddpm_op_attention_backward and cddpm_op_attention_backward_p16;
 * cddpm_op_attention_backward_h3 has a query of its own, cddpm_op_attention_backward_h3_scratch. */
size_t cddpm_op_conv_wgrad_scratch(int C0, int C1, int upsample, int Cout, int ksize, int B, int H, int W, int precision);
size_t cddpm_op_gn_coef_scratch(int C0, int has_src1, int C1, int B, int HW);
size_t cddpm_op_gn_silu_backward_scratch(int has_rec, int B, int HW, int C);
size_t cddpm_op_attention_backward_scratch(int B, int N, int C);
size_t cddpm_op_attention_backward_h3_scratch(int B, int N, int C);
size_t cddpm_op_linear_backward_scratch(int M, int N, int K, int silu_in);
size_t cddpm_op_head_scratch(int B, int H, int W, int C);
size_t cddpm_op_bias_grad_scratch(int64_t npix, int C);
size_t cddpm_op_chan_image_corr_scratch(int B, int H, int W, int C);
size_t cddpm_op_enc_conv_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed);
size_t cddpm_op_enc_conv_wgrad_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride);
size_t cddpm_op_enc_conv_p16_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride, int transposed);
size_t cddpm_op_enc_conv_wgrad_p16_scratch(int B, int H, int W, int Cin, int Cout, int K, int stride);
size_t cddpm_op_enc_stem_wgrad_scratch(int B, int H, int W);
size_t cddpm_op_enc_bn_forward_scratch(int64_t N, int HW, int C);
size_t cddpm_op_enc_bn_backward_scratch(int64_t N, int HW, int C);
int cddpm_op_absmax(cddpm_handle h, const float* x_dev, int64_t n, float* out_dev, void* stream);
int cddpm_op_pack_conv(cddpm_handle h, const float* w_dev, int Cout, int Cin, int ksize, int mode, int scale_exp, void* packed_dev,
                       void* stream);
/* The same packer for MANY images in one launch (the training step re-packs 69 convolutions x 2 operators after every update): a device
 * table of jobs, each the arguments of cddpm_op_pack_conv with the operator's dimensions resolved -- O / I = output / input channels of
 * the PACKED operator (mode 1: the forward tensor's Cin / Cout), taps = 1 | 9 (mode 2: 4), cls = the folded-upsample class 0..3 (mode 2:
 * one job per class, dst the image base; else 0). max_units = the largest O / 128 * I / 32 * taps * 512 over the jobs. */
typedef struct cddpm_pack_job { const float* w_dev; void* packed_dev; int32_t O, I, taps, mode, scale_exp, cls; } cddpm_pack_job;
int cddpm_op_pack_conv_batch(cddpm_handle h, const cddpm_pack_job* jobs_dev, int njobs, int64_t max_units, void* stream);
int cddpm_op_conv_packed(cddpm_handle h, const float* src0_dev, int C0, const float* src1_dev, int C1, const float* coef_dev, int silu,
                         int folded_up, const void* packed_dev, int scale_exp, const float* bias_dev, int Cout, int ksize,
                         const float* res_dev, int res_upsample, const float* skip_dev, int S0, const float* skip1_dev, int S1,
                         const void* skip_packed_dev, float* out_dev, float* stats_dev, int B, int H, int W, void* stream);
/* skip1_dev / S1 (0: none): the 1x1 skip segment's input as the concatenation of two tensors (its image covers S0 + S1 channels). */
/* stats_dev (or NULL): the output's GroupNorm statistics records [B][cddpm_stat_records(H, W, folded_up ? 1 : 0)][Cout][2], written by the
 * convolution's epilogue; cddpm_op_gn_coef_rec is cddpm_op_gn_coef on such records (no sweep over the tensors), and
 * cddpm_op_gn_silu_backward takes them through rec_dev / nrec. */
int cddpm_op_gn_coef_rec(cddpm_handle h, const float* rec0_dev, int n0, int C0, const float* rec1_dev, int n1, int C1, const float* gamma_host,
                         const float* beta_host, const float* film_dev, float* coef_dev, int B, int HW, void* stream);
/* ---- training-mode operators of the context encoder (timm ResNet-50, in_chans = 1; reference src/models/modules/DDPM_encoder.py:21-23,
 * trained jointly with the UNet by src/models/DDPM_2D.py:114-135 / :305-306). NHWC fp32 device tensors. The convolutions come in two
 * arithmetics: plain fp32 FMA kernels (cddpm_op_enc_pack_w / _conv / _conv_wgrad: the default), and precision 16 on the matrix pipe
 * (the *_p16 entry points below), chosen per call by the caller (EncoderTrainer's precision). Strided operators map n -> ceil(n / stride).
 * cddpm_op_enc_pack_w: PyTorch weight [Cout][Cin][K][K] -> the images the convolution reads: wf [K*K][Cin][Cout] (forward) and, when wd_dev is
 *   given, wd [K*K][Cout][Cin] (input gradient).
 * cddpm_op_enc_conv: transposed = 0: z [B,Ho,Wo,Cout] = conv_K,stride,pad K/2 (x [B,H,W,Cin]) with wf; transposed = 1: dx [B,H,W,Cin] from
 *   dz [B,Ho,Wo,Cout] with wd (H, W are always the convolution's INPUT size). No bias (ResNet convolutions have none).
 * cddpm_op_enc_conv_wgrad: dw [Cout][Cin][K][K] (PyTorch layout) from x and dz.  cddpm_op_enc_stem / _stem_wgrad: the 7x7 / 2 single-channel stem
 *   (x [B,H,W] -> z [B,ceil(H/2),ceil(W/2),64], weight [64][49]).
 * cddpm_op_enc_bn_forward: BatchNorm2d in TRAINING mode + optional shortcut + optional ReLU:
 *   y = relu(((z - mean_c) rstd_c gamma_c + beta_c) s_b + res), batch statistics over the N = B * HW pixels (fp64 sums), mean_rstd_dev [2][C] kept
 *   for the backward, running statistics updated as torch does (momentum, unbiased variance) when given; s_b (sample_scale_dev [B] or NULL = 1) is
 *   the stochastic-depth scale of the residual branch (timm drop_path).  cddpm_op_enc_bn_backward: dz, dgamma, dbeta and (dres_dev given) the
 *   shortcut operand's gradient dy [y > 0].
 *   There is ONE training BatchNorm in the library (csrc/batchnorm_train.hip); this pair and cddpm_op_spark_bn_forward / _backward below are
 *   two callers of it. What this pair fixes: no mask, no fill value, ReLU or none, training mode; C a multiple of 64; the pixels are summed
 *   in clamp(N / 256, 1, 32) chunks (the order of the fp64 sums, hence the bits, and the grid); 2 planes of partial sums per chunk in the
 *   backward's scratch; N = 1 is accepted (the biased variance then goes into the running variance).
 * cddpm_op_enc_maxpool: 3x3 / 2 pad 1 forward (backward = 0) or its backward in gather form (first maximum in row-major order, as torch;
 *   deterministic).  cddpm_op_enc_avgpool: global average pool x [B,HW,C] -> g [B,C], or (backward = 1) dL/dg [B,C] (first pointer) -> dL/dx (second). */
int cddpm_op_enc_pack_w(cddpm_handle h, const float* w_dev, int Cout, int Cin, int K, float* wf_dev, float* wd_dev, void* stream);
int cddpm_op_enc_conv(cddpm_handle h, const float* src_dev, const float* w_img_dev, float* dst_dev, int B, int H, int W, int Cin, int Cout, int K,
                      int stride, int transposed, void* stream);
int cddpm_op_enc_conv_wgrad(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, int Cin, int Cout, int K,
                            int stride, void* stream);
/* Precision 16 of the three convolution operators: what the reference trainer's `precision: 16` (configs/trainer/default.yaml:7) computes for
 * self.encoder, whose forward and backward lie inside the LightningModule's autocast (src/models/DDPM_2D.py:114-135). The convention of
 * "Arithmetic of the training operators" above: every operand element (forward x, w; input gradient dz, w; weight gradient x, dz) is rounded to
 * fp16 to nearest even with gradual underflow, as torch's .half() (|v| > 65504 -> inf: the result is then non-finite, which cddpm_op_grad_check
 * sees in the gradient buffer; range is the loss scaler's job, there are no pre-scales), products are accumulated in fp32
 * (v_mfma_f32_16x16x32_f16), results are fp32 NHWC / PyTorch layout as the fp32 operators'. Bit-identical from run to run (contraction splits
 * are folded in a fixed order). BatchNorm, ReLU, pooling, fc, the 7x7 stem (K = 49), Adam and the master weights have no precision-16 form.
 * Shapes: Cin and Cout multiples of 64 up to 2048, K 1|3, stride 1|2, B, H, W >= 1; anything else is refused with a message.
 * cddpm_op_enc_pack_w_p16: PyTorch weight [Cout][Cin][K][K] (fp32) -> fp16 images, rounded once here; either pointer may be NULL:
 *   wf16 [K*K][Cin / 32][Cout][32]: element (t, ci, co) at ((t (Cin / 32) + ci / 32) Cout + co) 32 + ci % 32   (forward, transposed = 0)
 *   wd16 [K*K][Cout / 32][Cin][32]: element (t, ci, co) at ((t (Cout / 32) + co / 32) Cin + ci) 32 + co % 32   (input gradient, transposed = 1)
 *   i.e. [tap][32-chunk of the contraction][produced channel][position in the chunk], Cout Cin K K 2 bytes each; taps in the weight's own order.
 * cddpm_op_enc_conv_p16 / cddpm_op_enc_conv_wgrad_p16: cddpm_op_enc_conv / cddpm_op_enc_conv_wgrad with those images and that arithmetic. */
int cddpm_op_enc_pack_w_p16(cddpm_handle h, const float* w_dev, int Cout, int Cin, int K, void* wf16_dev, void* wd16_dev, void* stream);
int cddpm_op_enc_conv_p16(cddpm_handle h, const float* src_dev, const void* w_img16_dev, float* dst_dev, int B, int H, int W, int Cin, int Cout,
                          int K, int stride, int transposed, void* stream);
int cddpm_op_enc_conv_wgrad_p16(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, int Cin, int Cout,
                                int K, int stride, void* stream);
int cddpm_op_enc_stem(cddpm_handle h, const float* x_dev, const float* w_dev, float* z_dev, int B, int H, int W, void* stream);
int cddpm_op_enc_stem_wgrad(cddpm_handle h, const float* x_dev, const float* dz_dev, float* dw_dev, int B, int H, int W, void* stream);
int cddpm_op_enc_bn_forward(cddpm_handle h, const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* sample_scale_dev,
                            const float* res_dev, int relu, float eps, float momentum, float* run_mean_dev, float* run_var_dev, float* mean_rstd_dev,
                            float* y_dev, int64_t N, int HW, int C, void* stream);
int cddpm_op_enc_bn_backward(cddpm_handle h, const float* z_dev, const float* y_dev, const float* dy_dev, const float* mean_rstd_dev,
                             const float* gamma_dev, const float* sample_scale_dev, int relu, float* dz_dev, float* dres_dev, float* dgamma_dev,
                             float* dbeta_dev, int64_t N, int HW, int C, void* stream);
int cddpm_op_enc_maxpool(cddpm_handle h, const float* x_dev, float* y_dev, int B, int H, int W, int C, int backward, const float* dy_dev, float* dx_dev,
                         void* stream);
int cddpm_op_enc_avgpool(cddpm_handle h, const float* x_dev, float* g_dev, int B, int HW, int C, int backward, void* stream);

/* ---- operators of SparK masked pre-training (csrc/spark_train.hip, csrc/batchnorm_train.hip): what reference src/models/Spark_2D.py trains beside the ResNet-50 --
 * the sparse BatchNorm of the converted encoder (src/models/modules/spark/encoder.py:25-35, :183-190), densify (spark/Spark_2D.py:157-171),
 * the LightDecoder (spark/decoder.py:17-76), spatial_loss (spark/Spark_2D.py:180-199) and AdamW (src/models/Spark_2D.py:123-124). NHWC fp32
 * device tensors; nothing uses float atomics, two calls give the same bits.
 * The cell mask active_dev: uint8 [B][f][f]; pixel (b, y, x) of an H x W tensor is active iff active[b][y f / H][x f / W] (H and W multiples
 * of f: the mask dilated to the tensor's resolution, encoder.py:13-16).
 * cddpm_op_spark_bn_forward / _backward: the BatchNorm of cddpm_op_enc_bn_forward / _backward (one implementation, csrc/batchnorm_train.hip)
 *   with all of its options -- sparse or dense, a fill value, ReLU6, evaluation mode -- on this pair's own plan: C a multiple of 4, the
 *   pixels summed in clamp(N C / 16384, 1, 128) chunks, 3 planes of partial sums per chunk in the backward's scratch (the third: dfill),
 *   fewer than two values per channel refused. Where both chunk rules give the same count (C = 64, N <= 8192) the two pairs return the
 *   same bits for the same dense call.
 *   y = act((active ? ((z - mean_c) rstd_c gamma_c + beta_c) : fill_c) s_b + res), act 0 none | 1 ReLU | 2 ReLU6 (decoder.py:26).
 *   active_dev NULL = dense (nn.BatchNorm2d); given = BatchNorm1d over the active pixels only (sp_bn_forward): batch statistics in fp64 over the
 *   n_act active pixels, n_act counted on the device, running mean / unbiased variance updated with n_act. fill_dev [C] or NULL = 0: what
 *   inactive pixels get -- the mask token of densify (torch.where, spark/Spark_2D.py:165-168), 0 in the encoder. training = 0: the running
 *   statistics are used and left alone. Training with fewer than 2 values per channel is refused (torch's BatchNorm1d raises); with a mask
 *   the operator reads the device's count back to say so, which synchronises the stream once per call.
 *   Backward: dz = 0 at inactive pixels; dgamma, dbeta sum over the active pixels; dfill_dev (or NULL) [C] = sum over the inactive pixels
 *   of dy act' s_b; dres_dev (or NULL) = dy act'; ReLU6's gradient flows where 0 < y < 6. training = 0: the backward of the evaluation form.
 *   C: a multiple of 4, >= 4; N = B H W, HW = H W.
 * cddpm_op_spark_mask_mul: y = x * active_ex on [B,H,W,C], C >= 1; y_dev may be x_dev (Spark_2D.py:150-151; encoder.py:19-22).
 * cddpm_op_spark_conv: the small-channel convolution family on the layer's own PyTorch weight tensor, read in place:
 *   transposed_conv 0: nn.Conv2d(Cin, Cout, K, 1, K / 2), K 1 | 3, weight [Cout][Cin][K][K]  (en_de_lins, decoder.py:26-27, proj :66)
 *   transposed_conv 1: nn.ConvTranspose2d(Cin, Cout, 4, 2, 1), weight [Cin][Cout][4][4]       (DecoderConv.up, decoder.py:37)
 *   backward 0: dst = layer(src) + bias (bias_dev [Cout] or NULL); backward 1: dst = the input gradient from src = dy (bias_dev NULL).
 *   H, W: the LAYER's input size; a transposed convolution's output is [B,2H,2W,Cout]. Any Cin, Cout >= 1.
 * cddpm_op_spark_conv_wgrad: dw_dev in the weight's own layout and (db_dev given, Cout <= 256) the bias gradient, from the layer's input
 *   x_dev [B,H,W,Cin] and its output gradient dy_dev. Pixel ranges are folded in a fixed order.
 * cddpm_op_spark_loss: rec_dev, inp_dev [B][H][W] (one channel). loss_dev[0] = sum over the pixels of masked (not active) cells of
 *   (rec - inp)^2 / (p^2 (n_masked + 1e-8)), p^2 = (H / f)(W / f) (spatial_loss, pix_norm 0; 0 when nothing is masked); loss_dev[1] = mean |rec - inp|
 *   (L1_AE's recon_error); drec_dev (or NULL) = the gradient of w_mask loss[0] + w_l1 loss[1].
 * cddpm_op_adamw_guarded: cddpm_op_adam_guarded with torch.optim.AdamW's decoupled decay, p <- p (1 - lr weight_decay) before the update;
 *   the same control block, so a skipped step decays nothing.
 * Under "Dynamic loss scaling" above (scaler_dev: that int32[4] block, required), the pre-training step's forms of steps (a) and (c):
 * cddpm_op_spark_loss_scaled: cddpm_op_spark_loss whose drec_dev is the gradient of w_mask loss[0] + w_l1 loss[1] TIMES the device scale;
 *   loss_dev[0..1] are the unscaled terms. With the scale a power of two S and no under- or overflow it is bit-identical to
 *   cddpm_op_spark_loss called with S w_mask, S w_l1. Temporaries: cddpm_op_spark_loss_scratch.
 * cddpm_op_adamw_scaled: cddpm_op_adamw_guarded with gradient g_dev * extra_unscale / scale, in the form of cddpm_op_adam_scaled:
 *   bit-identical to cddpm_op_adamw_guarded with grad_unscale = extra_unscale / S.
 * Precision 16 of the pre-training step (SparKTrainer's precision=16; the trainer's own choice, cddpm_set_train_precision is neither read
 * nor set): the rule of "Precision 16 of the three convolution operators" -- every convolution of the sparse ResNet-50 but the 7x7 stem,
 * forward, input gradient and weight gradient, runs on cddpm_op_enc_conv_p16 / cddpm_op_enc_conv_wgrad_p16 and the images of
 * cddpm_op_enc_pack_w_p16 (operands rounded as .half(), fp32 accumulation). The sparse and dense BatchNorms, the mask multiply and max
 * pool, the stem, the densify convolutions (en_de_lins), the LightDecoder, the loss, AdamW and the master weights are fp32 at either
 * precision: those layers are launch- and memory-bound at 4 to 128 channels, fp16 operands buy nothing there. */
int cddpm_op_spark_bn_forward(cddpm_handle h, const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* sample_scale_dev,
                              const float* res_dev, int act, float eps, float momentum, float* run_mean_dev, float* run_var_dev, float* mean_rstd_dev,
                              float* y_dev, int64_t N, int HW, int C, const uint8_t* active_dev, int f, int H, int W, const float* fill_dev, int training,
                              void* stream);
int cddpm_op_spark_bn_backward(cddpm_handle h, const float* z_dev, const float* y_dev, const float* dy_dev, const float* mean_rstd_dev,
                               const float* gamma_dev, const float* sample_scale_dev, int act, float* dz_dev, float* dres_dev, float* dgamma_dev,
                               float* dbeta_dev, int64_t N, int HW, int C, const uint8_t* active_dev, int f, int H, int W, float* dfill_dev, int training,
                               void* stream);
int cddpm_op_spark_mask_mul(cddpm_handle h, const float* x_dev, const uint8_t* active_dev, float* y_dev, int B, int H, int W, int C, int f, void* stream);
int cddpm_op_spark_conv(cddpm_handle h, const float* src_dev, const float* w_dev, const float* bias_dev, float* dst_dev, int B, int H, int W, int Cin,
                        int Cout, int K, int transposed_conv, int backward, void* stream);
int cddpm_op_spark_conv_wgrad(cddpm_handle h, const float* x_dev, const float* dy_dev, float* dw_dev, float* db_dev, int B, int H, int W, int Cin, int Cout,
                              int K, int transposed_conv, void* stream);
int cddpm_op_spark_loss(cddpm_handle h, const float* rec_dev, const float* inp_dev, const uint8_t* active_dev, int f, int B, int H, int W, float w_mask,
                        float w_l1, float* loss_dev, float* drec_dev, void* stream);
int cddpm_op_adamw_guarded(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, float grad_unscale, const int32_t* ctrl_dev, void* stream);
int cddpm_op_spark_loss_scaled(cddpm_handle h, const float* rec_dev, const float* inp_dev, const uint8_t* active_dev, int f, int B, int H, int W,
                               float w_mask, float w_l1, const int32_t* scaler_dev, float* loss_dev, float* drec_dev, void* stream);
int cddpm_op_adamw_scaled(cddpm_handle h, float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, float extra_unscale, const int32_t* ctrl_dev, const int32_t* scaler_dev, void* stream);
/* their size queries (the convention of cddpm_op_set_scratch above; has_db: db_dev given) */
size_t cddpm_op_spark_bn_forward_scratch(int64_t N, int HW, int C);
size_t cddpm_op_spark_bn_backward_scratch(int64_t N, int HW, int C);
size_t cddpm_op_spark_conv_scratch(int B, int H, int W, int Cin, int Cout, int K, int transposed_conv, int backward);
size_t cddpm_op_spark_conv_wgrad_scratch(int B, int H, int W, int Cin, int Cout, int K, int transposed_conv, int has_db);
size_t cddpm_op_spark_loss_scratch(int B, int H, int W, int f);

/* backward of a = act(GroupNorm32(x) * (1 + scale) + shift), act = SiLU (silu != 0) or identity (OpenAI_Unet.py:284-338, :325-330):
 * given da_dev [B,HW,C] writes dx_dev [B,HW,C] (with x1_dev: x = cat[x_dev [.., C - C1], x1_dev [.., C1]], the input gradient split the same
 * way into dx_dev / dx1_dev; needs rec_dev), dgamma_dev / dbeta_dev [C] and, when film_dev ([B][2C] scale | shift) is given,
 * dfilm_dev [B][2C]. The forward statistics are recomputed from x_dev. Everything NHWC fp32. */
int cddpm_op_gn_silu_backward(cddpm_handle h, const float* x_dev, const float* x1_dev /* second tensor of a concatenated input, or NULL */, int C1,
                              const float* da_dev, const float* gamma_host,
                              const float* beta_host, const float* film_dev, int silu, float* dx_dev, float* dx1_dev /* [B,HW,C1] */, float* dgamma_dev,
                              float* dbeta_dev, float* dfilm_dev, const float* rec_dev /* x's statistics records or NULL */, int nrec,
                              const float* add_dev /* [B,HW,C] added to dx (the gradient of a parallel skip path), or NULL */, int B, int HW, int C,
                              void* stream);

/* GroupNorm statistics record counts per sample for an H x W tensor (host arithmetic, callable without a GPU):
 * kind 0 = records the fused convolution's epilogue writes, 1 = the folded-upsample convolution's, 2 = the stand-alone
 * sweep's pixel-range split. cddpm_create sizes every records buffer for the largest of the three at max_h x max_w, and
 * every producer launch is refused if its count would not fit (tests/test_host_logic.py checks the counts are monotone). */
int cddpm_stat_records(int H, int W, int kind);

/* standalone attention core on qkv NHWC [B,N,3C] (q | k | v, heads = contiguous groups of head_channels = 64):
 * out [B,N,C] = softmax(q k^T / sqrt(head_channels)) v  (QKVAttention, OpenAI_Unet.py:457-476). C: a multiple of 64; tested and
 * expected ranges of N as for cddpm_op_attention_backward. */
int cddpm_op_attention(cddpm_handle h, const float* qkv_dev, float* out_dev, int B, int N, int C, void* stream);
/* the same contract in the arithmetic of fp16 autocast over QKVAttention.forward (OpenAI_Unet.py:457-476): q / 8, k and v rounded to
 * fp16 (RNE) once, products on v_mfma_f32_32x32x16_f16 with fp32 accumulators, the running max / sum softmax in fp32, P rounded to
 * fp16 only as an MFMA operand, fp32 output. The attention kernel of a precision-16 handle (cddpm_set_precision); any handle may call it. */
int cddpm_op_attention_p16(cddpm_handle h, const float* qkv_dev, float* out_dev, int B, int N, int C, void* stream);
/* the same contract at fp32 accuracy on the fp16 matrix pipe (v_mfma_f32_32x32x16_f16), the attention member of the h3 family: q / 8,
 * k and v are carried as hi = fp16(x), lo = fp16((x - hi) 2^11), P (against the running maximum, lifted by 2^15) as fp16(P),
 * fp16(P - fp16(P)) and fp16(P 2^-11); each product is hi . hi + hi . lo + lo . hi with fp32 accumulation, lo . lo (2^-22) is dropped;
 * the softmax is fp32 VALU work as in the other two kernels; input and output are fp32. 48 MFMAs of 32 cycles per wave and 64-key tile
 * where cddpm_op_attention issues 128 of 64.
 * Range contract, as for the h3 convolutions: it holds for |q / 8|, |k|, |v| < 65504. An element outside it (or non-finite) gives
 * non-finite outputs for that sample only -- never a finite wrong number, never another sample.
 * What a handle of attention family h3 runs (cddpm_set_attention_family); any handle may call it. */
int cddpm_op_attention_h3(cddpm_handle h, const float* qkv_dev, float* out_dev, int B, int N, int C, void* stream);

/* ---- context encoder ---------------------------------------------------------------
 * Replaces the module get_encoder builds (src/models/modules/DDPM_encoder.py:6-29): timm resnet50(in_chans=1,
 * num_classes=cond_dim) in eval mode, called once per slice batch by DDPM_2D.forward (src/models/DDPM_2D.py:98-104).
 * PARITY UNPINNED: timm is not installed in the build image; the network follows timm's published ResNet-50 v1.5 and
 * its state_dict names and is checked against a torch restatement of that description (oracle/encoder_oracle.py).
 * load_weights takes host pointers under timm's key names (conv1.weight, bn1.{weight,bias,running_mean,running_var},
 * layer{1..4}.{i}.{conv1,bn1,conv2,bn2,conv3,bn3,downsample.0,downsample.1}.*, fc.{weight,bias}); BatchNorm is folded.
 * forward: x_dev [B,1,H,W] fp32 in [0,1] (H, W >= 32) -> out_dev [B, num_classes] on the caller's stream. */
typedef struct cddpm_encoder_ctx* cddpm_encoder_handle;
int cddpm_encoder_create(cddpm_encoder_handle* out, int num_classes, int max_batch, int max_h, int max_w, int device);
void cddpm_encoder_destroy(cddpm_encoder_handle h);
const char* cddpm_encoder_last_error(cddpm_encoder_handle h);
int cddpm_encoder_num_weights(void);
int cddpm_encoder_load_weights(cddpm_encoder_handle h, const char* const* names, const float* const* host_ptrs,
                               const int64_t* numels, int n);
int cddpm_encoder_forward(cddpm_encoder_handle h, const float* x_dev, float* out_dev, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDDPM_H */
