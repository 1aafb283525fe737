/* uad_hip.h — C-ABI of libuad_hip.so: the MI355X (gfx950) conv autoencoder train / reconstruct hot path.
 *
 * This is the drop-in boundary for the reference's TF-1.15 `sess.run` calls (the reference has no native code and
 * no FFI of its own; every entry below names the reference lines whose device work it replaces):
 *
 *   uad_forward / uad_backward / uad_adam_step / uad_train_step
 *       <- trainers/VAE.py:83-96, trainers/AE.py:70-83  (one sess.run({reconstruction, **losses, optimizer}))
 *          (+ trainers/ceVAE.py:86-117 on models/context_encoder_variational_autoencoder.py:9-59, losses
 *          trainers/ceVAE.py:38-51)
 *          graph = models/variational_autoencoder.py:9-47 | models/autoencoder.py:9-40 on
 *                  models/customlayers.py:16-38; losses trainers/VAE.py:36-42 | AE.py:28-29;
 *                  optimizer trainers/DLMODEL.py:112-131 (tf.train.AdamOptimizer, beta1 from
 *                  utils/default_config_setup.py:257)
 *   uad_forward(want_backward = 0)
 *       <- trainers/VAE.py:105-118, AE.py:92-105 (reconstruct: sess.run({'reconstruction'})) and the VAL pass
 *   uad_restore_step
 *       <- trainers/GMVAE_spatial.py:178-190 (150 x sess.run({'grads'}) + host `restored -= restore_lr * grads`), graph
 *          models/gaussian_mixture_variational_autoencoder_spatial.py:9-65, losses trainers/GMVAE_spatial.py:61-92
 *   uad_residual
 *       <- utils/Evaluation.py:282-289 (residual map, brain mask, hyper-intensity prior) and
 *          trainers/VAE.py:120 (l1err)
 *   uad_cc_label / uad_detection_rate / uad_scores_threshold_at_precision
 *       <- utils/Evaluation.py:130-172 (skimage label + regionprops: lesion-wise TP / FP / FN), :439 (threshold at 70 % precision)
 *   uad_erode_cross / uad_median3d / uad_scores_*
 *       <- utils/Evaluation.py:84-89 (scipy binary_erosion), :108-110 (scipy median_filter), trainers/Metrics.py:17-19,45-47,
 *          67-72,138-162 (sklearn AUPRC / AUROC, Dice threshold sweep)
 *   uad_curvature_flow
 *       <- utils/NII.py:85-87 (nii.denoise(): sitk.CurvatureFlow, called by dataloaders/MSLUB.py:242 and its siblings)
 *   uad_resize2d / uad_mask_by_label
 *       <- dataloaders/BRAINWEB.py:140-142 (cv2.resize of slices larger than sliceResolution), :266-289 (skull map from the tissue classes)
 *   uad_cc_props / uad_crop2d
 *       <- dataloaders/MSLUB.py:200-222 (cropType 'lesions': regionprops centroids, one crop per component), BRAINWEB.py:166-173 ('random')
 *   uad_brain_boxes / uad_brain_boxes_f32 / uad_assemble_batch
 *       <- trainers/CE.py:123-139 (retrieve_masked_batch: np.argwhere boxes, the 20x20 squares, batch * mask; called by CE.py:77, ceVAE.py:93),
 *          dataloaders/BRAINWEB.py:459, MSLUB.py:468 (Options.addInstanceNoise in next_batch)
 *   uad_render_minmax_u8 / uad_render_heatmap / uad_render_overlay
 *       <- utils/Evaluation.py:302-321 (the per-slice PNGs: normalize_and_squeeze :368, squash_intensities + add_colorbar + utils.apply_colormap),
 *          :501-507 with utils/image_utils.py:22-45 (the TP / FP / FN overlay)
 *   uad_set_params / uad_get_params / uad_tensor_info
 *       <- tf.global_variables_initializer / tf.train.Saver variable access (trainers/DLMODEL.py:63-110)
 *   uad_op_*  — single-kernel entry points used by the parity tests (no reference counterpart).
 *
 * Conventions: plain C, no torch types.  All tensor arguments are DEVICE pointers to fp32 NHWC buffers owned by the
 * caller unless stated otherwise; `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 * asynchronous on `stream` except the ones documented as synchronous.  Every function returns 0 on success or a
 * UAD_ERR_* code; uad_last_error() returns the thread-local message of the last failure.  A handle is not thread-safe.
 */
#ifndef UAD_HIP_H
#define UAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libuad_hip.so is built with -fvisibility=hidden (build.py): everything declared between this push and the pop at the end of the file -- and
 * nothing else -- is exported, so `nm -D --defined-only libuad_hip.so` lists exactly this header's functions (tests/test_host_cpu.py). */
#pragma GCC visibility push(default)

enum { UAD_OK = 0, UAD_ERR_INVALID = 1, UAD_ERR_HIP = 2, UAD_ERR_UNSUPPORTED = 3 };
enum { UAD_ARCH_AE = 0, UAD_ARCH_VAE = 1, UAD_ARCH_CEVAE = 2, UAD_ARCH_GMVAE_SPATIAL = 3,
       UAD_ARCH_AE_SPATIAL = 4 };   /* models/autoencoder_spatial.py:7-27: no dense bottleneck; the latent is the encoder feature map
                                       [n,r,r,C]: io.mask_mu is its dropout keep-mask and io.z_mu receives it (both that shape) */
enum { UAD_BUF_PARAMS = 0, UAD_BUF_GRADS = 1, UAD_BUF_ADAM_M = 2, UAD_BUF_ADAM_V = 3 };
/* ENCODER_HI + ENCODER_LO partition ENCODER: HI = the deep blocks' variables (complete after the blocks >= 2 are back-propagated: ~93 % of the
 * segment at the default depth), LO = the first two blocks' kernels -- the data-parallel layer's last, exposed all-reduce then moves 0.2 MB
 * instead of 2.7 MB */
enum { UAD_SEG_DECODER = 0, UAD_SEG_BOTTLENECK = 1, UAD_SEG_ENCODER = 2, UAD_SEG_ENCODER_HI = 3, UAD_SEG_ENCODER_LO = 4, UAD_SEG_ALL = -1 };
/* arithmetic of the k5 s2 forward / data-gradient contractions: exact fp32 MFMA (default), or split-bf16 (x = hi + lo,
 * hi*hi + hi*lo + lo*hi on the bf16 matrix cores, fp32 accumulate: ~2^-17 relative error per product) */
enum { UAD_MATH_F32 = 0, UAD_MATH_BF16X3 = 1,
       UAD_MATH_BF16X3_ALL = 2 };   /* uad_gan_* only: also the generic k3 / k1 contractions of the ResNet graph in bf16x3.  Each
                                       contraction stays inside 1e-4, but through the 20-layer ResNet critic the penalty scalar
                                       drifts to ~3e-4 of its value, so for THAT graph this mode is opt-in and not parity-rated.
                                       The shorter generic-kernel graphs (aae_kind 4-6: Zimmerer VAE / ceVAE, GMVAE (You)) pass the
                                       same 1e-4 gradient checks in this mode as in fp32; their trainers default to it */
enum { UAD_MATH_BF16X6 = 3 };       /* uad_create handles (AE / VAE / ceVAE / spatial GMVAE) only, round 6: THREE bf16 planes per operand (x = h + m + l),
                                       six products per multiply on the bf16 matrix cores, fp32 accumulate -- fp32-grade results (the dropped terms are
                                       below 2^-26 of a product; tests hold 1e-5 against the fp64 oracle) at 6 x 32 instead of 8 x 64 matrix-pipe cycles
                                       per K = 16 of an fp32 MFMA.  The k5 s2 spatial kernels carry it; launches they do not take run exact fp32 */

typedef struct uad_model uad_model_t;

typedef struct {
    int arch;       /* UAD_ARCH_*                                              */
    int height;     /* config.outputHeight  (trainers/AEMODEL.py:18-19)         */
    int width;      /* config.outputWidth   (must equal height; power of two)   */
    int channels;   /* config.numChannels   (1 supported)                       */
    int inter_res;  /* config.intermediateResolutions[0]                        */
    int zdim;       /* config.zDim                                              */
    int max_batch;  /* largest n any later call will pass                       */
    /* spatial GMVAE only (trainers/GMVAE_spatial.py:12-21); ignored otherwise */
    int dim_c;      /* config.dim_c  mixture components                         */
    int dim_z;      /* config.dim_z                                             */
    int dim_w;      /* config.dim_w                                             */
    float c_lambda; /* config.c_lambda                                          */
} uad_config_t;

typedef struct {
    const float* x;          /* in  [n,H,W,C]                                                        */
    const float* eps;        /* in  [n,zdim] N(0,1) noise (VAE); NULL = 0                            */
    const float* mask_mu;    /* in  [n,zdim] keep-mask pre-scaled by 1/(1-rate), NULL = no dropout.
                                     VAE: on z_mu (variational_autoencoder.py:31); AE: on z (autoencoder.py:29) */
    const float* mask_sigma; /* in  [n,zdim] VAE: on z_log_sigma (:32)                               */
    const float* mask_dec;   /* in  [n,flat] VAE: on dec_dense output (:35); ignored for AE (autoencoder.py:30) */
    float* x_hat;            /* out [n,H,W,C] reconstruction                                         */
    float* l1_map;           /* out [n,H,W,C] |x_hat - x|, may be NULL                               */
    float* z_mu;             /* out [n,zdim] (AE: z), may be NULL                                    */
    float* z_log_sigma;      /* out [n,zdim] VAE, may be NULL                                        */
    float* z_sigma;          /* out [n,zdim] VAE, may be NULL                                        */
    float* scalars;          /* out [8] reconstructionLoss, kl, loss, 0, Rec_vae, Rec_ce, loss_vae, 0
                                     (means over the n samples; [4..6] are written for ceVAE only)       */
    float* rec_per_sample;   /* out [n] sum_hwc L1 (ceVAE: [2n], VAE branch then context branch), may be NULL */
    /* ---- ceVAE only (models/context_encoder_variational_autoencoder.py:9-59); NULL / ignored otherwise ---- */
    const float* x_ce;       /* in  [n,H,W,C] context-masked input (trainers/CE.py:123-139); NULL = x.  ceVAE: the second branch's input.
                                AE handles (dense / spatial): context-encoder training (trainers/CE.py:19-21,87-92): the network reads x_ce, the L1
                                term compares x_hat with x */
    const float* mask_mu_ce; /* in  [n,zdim] keep-mask on z_mu_ce (:37); given iff mask_mu is         */
    const float* mask_dec_ce;/* in  [n,flat] keep-mask on dec_dense(z_mu_ce) (:43); given iff mask_dec is */
    float* x_hat_ce;         /* out [n,H,W,C] reconstruction of the context branch, may be NULL      */
    float* l1_map_ce;        /* out [n,H,W,C] |x_hat_ce - x_ce|, may be NULL                         */
    float* anomaly;          /* out [n,H,W,C] L1_vae * |d loss_vae / d x| (trainers/ceVAE.py:51); written by
                                     uad_backward's ENCODER segment, may be NULL                          */
    /* ---- spatial GMVAE only (models/gaussian_mixture_variational_autoencoder_spatial.py:9-65) ----
     * x_hat = xz_mu; z_mu / z_log_sigma are the [n,r,r,dim_z] maps (r = inter_res); scalars = {mean_p_loss
     * (= reconstructionLoss), conditional_prior_loss, loss, w_prior_loss, c_prior_loss, 0, 0, 0} */
    const float* eps_w;      /* in  [n,r,r,dim_w] N(0,1) noise of w_sampled (:27); NULL = 0          */
    const float* eps_z;      /* in  [n,r,r,dim_z] N(0,1) noise of z_sampled (:32); NULL = 0          */
    float* w_mu;             /* out [n,r,r,dim_w], may be NULL                                       */
    float* w_log_sigma;      /* out [n,r,r,dim_w], may be NULL                                       */
    float* pc;               /* out [n,r,r,dim_c] softmax mixture posterior (:63), may be NULL       */
} uad_io_t;

const char* uad_last_error(void);
const char* uad_version(void);

int uad_create(const uad_config_t* cfg, uad_model_t** out);
int uad_destroy(uad_model_t* m);

long long uad_param_count(const uad_model_t* m);
int uad_num_tensors(const uad_model_t* m);
/* name (NUL-terminated, truncated to name_cap), flat offset, rank and shape (padded with 1s to 4) of tensor idx,
 * in TF variable-creation order (Encoder, Bottleneck, Decoder). */
int uad_tensor_info(const uad_model_t* m, int idx, char* name, int name_cap, long long* offset, int* rank, int* shape4);
/* device pointer to a handle-owned flat fp32 buffer of uad_param_count() elements (UAD_BUF_*) */
float* uad_buffer(uad_model_t* m, int which);
/* flat [offset, offset+count) range of one gradient segment; segments complete in the order DECODER, BOTTLENECK,
 * ENCODER (= ENCODER_HI, then ENCODER_LO) during uad_backward — the data-parallel layer all-reduces each as soon as it is done.
 * A segment may be empty (count 0). */
int uad_grad_segment(const uad_model_t* m, int segment, long long* offset, long long* count);

/* synchronous host<->device copies of the flat parameter vector */
int uad_set_params(uad_model_t* m, const float* host, long long count);
int uad_get_params(uad_model_t* m, float* host, long long count);
int uad_get_buffer(uad_model_t* m, int which, float* host, long long count);
int uad_set_buffer(uad_model_t* m, int which, const float* host, long long count);
int uad_reset_optimizer(uad_model_t* m);            /* zero Adam slots, t = 0 (synchronous) */
long long uad_get_step(const uad_model_t* m);
int uad_set_step(uad_model_t* m, long long t);

/* forward pass + losses.  want_backward != 0 additionally keeps what uad_backward needs and starts the backward
 * (d loss / d c of the last decoder block is produced by the fused loss kernel).  want_backward == 2 asks for the
 * data-gradient chain only (ceVAE validation / reconstruct: the anomaly map needs d loss_vae / d x but no parameter
 * gradient); the following uad_backward then leaves UAD_BUF_GRADS untouched.
 * ceVAE runs both branches as one 2n-sample pass through the shared layers (VAE-branch samples first). */
int uad_forward(uad_model_t* m, const uad_io_t* io, int n, int want_backward, void* stream);
/* gradient of `loss` w.r.t. every parameter into the UAD_BUF_GRADS buffer; segment = UAD_SEG_* (call DECODER,
 * BOTTLENECK, ENCODER in that order -- ENCODER may be given as ENCODER_HI followed by ENCODER_LO -- or UAD_SEG_ALL). */
int uad_backward(uad_model_t* m, int segment, void* stream);
/* Data-parallel form of a segmented uad_backward: the same launches, but a segment whose parameter gradients are all written on the handle's
 * own side stream (DECODER, BOTTLENECK where it runs fused, ENCODER_HI) returns WITHOUT making `stream` wait for that side stream -- three stalls of
 * `stream` per step (each exposing the tail of a slab reduction) that only the collective needs, not the next segment's kernels.  *ready_stream
 * receives the stream in whose order the segment's gradient slice is complete: the side stream where the join was skipped, else `stream`.  The caller
 * issues the slice's all-reduce in THAT stream's order (torch: dist.all_reduce under torch.cuda.stream(ExternalStream(ready))) and goes on with the
 * next segment on `stream`.  The last segment (ENCODER / ENCODER_LO) always joins: after it every gradient is complete in `stream`'s order too.
 * The reference has no counterpart (single process); parallel.DataParallelStep is the caller. */
int uad_backward_deferred(uad_model_t* m, int segment, void* stream, void** ready_stream);
/* ---- library-issued gradient all-reduce (RCCL over xGMI) -------------------------------------------------------------
 * SURVEY.md section 8b's `allreduce_attach(comm)`.  The reference is single-process; under slice-batch data parallelism (one process per GPU) the
 * flat fp32 gradient buffer is summed over the ranks once per step.  With a communicator attached the LIBRARY enqueues ncclAllReduce itself --
 * in place on its own gradient buffer, on its side stream right behind the slab reductions that complete the bucket (the last bucket: on the
 * caller's stream in front of the optimizer step) -- while the caller's stream runs on with the next backward segment: no process-group hand-off per collective (torch.distributed costs an event
 * record + wait on both sides of every all-reduce, 40-80 us per step at four buckets).  librccl.so.1 is bound at run time (dlopen; the copy the
 * process already holds, e.g. PyTorch-ROCm's, else the loader path or UAD_RCCL_LIB): libuad_hip.so does not link it.
 *   uad_rccl_unique_id      rank 0: a fresh ncclUniqueId (128 bytes) -- hand it to the other ranks by any channel (parallel.py: one broadcast over
 *                           the existing torch.distributed group)
 *   uad_rccl_comm_create    every rank, on its own device: ncclCommInitRank(world, id, rank) -> opaque communicator (collective call)
 *   uad_rccl_allreduce      in-place float sum over the ranks of any device buffer, enqueued on `stream` (the GAN handle's per-phase group gradient)
 *   uad_allreduce_attach    comm + bucket plan: bucket i = gradient elements [offset[i], offset[i] + count[i]), all-reduced right after backward segment
 *                           after_segment[i] (UAD_SEG_DECODER | BOTTLENECK | ENCODER_HI | ENCODER_LO); comm == NULL detaches.  The caller applies
 *                           grad_scale = 1 / world in uad_adam_step (the sum of per-rank batch-mean gradients / world = the global batch mean).
 *   uad_backward_allreduce  one backward segment (as uad_backward_deferred: DECODER, BOTTLENECK, ENCODER_HI, ENCODER_LO in this order) + its buckets'
 *                           all-reduces; after ENCODER_LO `stream` has been made to wait for every bucket, so the optimizer step can follow on it. */
int uad_rccl_unique_id(void* id_out, int cap);
int uad_rccl_comm_create(const void* id_bytes, int world, int rank, void** comm_out);
int uad_rccl_comm_destroy(void* comm);
int uad_rccl_allreduce(void* comm, float* buf, long long count, void* stream);
int uad_allreduce_attach(uad_model_t* m, void* comm, int world, int nbuckets, const int* after_segment, const long long* offset, const long long* count);
int uad_backward_allreduce(uad_model_t* m, int segment, void* stream);
/* TF-1.15 Adam: t += 1; lr_t = lr*sqrt(1-b2^t)/(1-b1^t); p -= lr_t*m/(sqrt(v)+eps); grads scaled by grad_scale first */
int uad_adam_step(uad_model_t* m, float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* the other optimizers of DLMODEL.create_optimizer (trainers/DLMODEL.py:113-123) with TF-1.15's update rules; the two slot buffers are the
 * Adam slots' storage (UAD_BUF_ADAM_M = Momentum's accumulator / RMSProp's `momentum` slot, UAD_BUF_ADAM_V = RMSProp's `rms` slot, which
 * TensorFlow initialises to ONE: set it before the first UAD_OPT_RMS step).  RMSProp: decay 0.9, eps 1e-10 are TF's defaults. */
enum { UAD_OPT_SGD = 1, UAD_OPT_MOMENTUM = 2, UAD_OPT_RMS = 3 };
int uad_optimizer_step(uad_model_t* m, int kind, float lr, float momentum, float decay, float eps, float grad_scale, void* stream);
/* Fault word of the fused bottleneck kernels (their sibling-workgroup exchange is bounded: uad_bott.hip).  A fault makes every optimizer launch
 * behind it a no-op ON THE DEVICE (parameters and slots stay those of the last good step) and is reported -- once, with the step counter rolled
 * back by the number of skipped updates (every optimizer call since the FIRST faulted launch) -- by the next uad_forward / uad_get_buffer /
 * uad_check_fault on the handle.  synchronize != 0 waits
 * for `stream` first (call it so at the end of an epoch, before a checkpoint, and -- under data parallelism -- before agreeing on the flag
 * across ranks: trainers/AEMODEL.py).  Returns UAD_OK when no fault is pending. */
int uad_check_fault(uad_model_t* m, int synchronize, void* stream);
/* on != 0: uad_forward / uad_get_buffer no longer report a pending fault -- only uad_check_fault does.  For data-parallel runs: a rank that raised
 * alone in the middle of an epoch would leave the other ranks blocked in the next gradient all-reduce; with deferred reporting every rank keeps
 * issuing the epoch's collectives (the faulted rank's optimizer launches stay no-ops on the device), all ranks agree on the word in the epoch's
 * scalar all-reduce (trainers/AEMODEL.py: process) and raise TOGETHER; the run restarts from the last checkpoint.  Default off. */
int uad_set_fault_deferred(uad_model_t* m, int on);
/* uad_forward(want_backward=1) + uad_backward(ALL) + uad_adam_step */
int uad_train_step(uad_model_t* m, const uad_io_t* io, int n, float lr, float beta1, float beta2, float eps,
                   void* stream);

/* spatial GMVAE restoration (trainers/GMVAE_spatial.py:178-190): one `sess.run(grads)` + host update, on device.
 * grads = d( n * loss + sum_n tv_lambda * TV_n(x - xz_mu) ) / d x  at the current x_restored (tf.gradients of the [n]-shaped
 * `loss + restore` sums its elements: each slice sees its own loss terms with weight 1, as if restored alone); then
 * x_restored -= restore_lr * grads in place.  grads_out (may be NULL) receives the gradient.  No parameter gradient is
 * computed and no host synchronisation happens: the caller enqueues restore_steps calls back to back.
 * On a UAD_ARCH_VAE handle this is trainers/VAE_You.py:52-53,133-144 instead: grads = d( rec_n + kl_n + tv_lambda * TV_n(x - x_hat) ) / d x
 * per sample (no 1/n: `pixel_loss` is not averaged), eps_z is the [n,zDim] reparameterisation noise, eps_w is ignored. */
int uad_restore_step(uad_model_t* m, float* x_restored, const float* eps_w, const float* eps_z, int n, float tv_lambda,
                     float restore_lr, float* grads_out, void* stream);

int uad_set_math_mode(uad_model_t* m, int mode);   /* UAD_MATH_* ; takes effect at the next uad_forward */
int uad_get_math_mode(const uad_model_t* m);
/* tests: device pointer + element count (for the batch of the last uad_forward; 2n rows inside a ceVAE handle) of a named
 * intermediate: "enc_c<i>" / "dec_c<i>" = pre-BN output of encoder / decoder block i (the activation pattern of the step is
 * sign(gamma' c + beta); the last decoder block's is not written when its epilogue is fused -- read "G0" = d loss / d c of that block
 * right after a want_backward forward instead -- or, when the step keeps that gradient in its compressed form, "fin_bits" = one
 * 32-bit word per output pixel (bit ch = channel ch's BN output > 0; read the floats' bit patterns) and "fin_dxhat" =
 * sign(x_hat - x) / n per pixel; both report count 0 otherwise), "dec_in" = the decoder's pre-BN input, "G0" / "G1" = gradient
 * ping-pong buffers, "fused_final" = flag in *count. */
int uad_debug_buffer(uad_model_t* m, const char* name, float** ptr, long long* count);
/* tests: what the handle WOULD launch for one 5x5 block (or the dense bottleneck: side 2) at batch n (1 .. max_batch) in its current math mode; nothing is launched and no state changes.
 * side 0 = encoder block `layer` (>= 1; block 0 runs the one-channel first-layer kernels: only its 'W' is answered, kernel 3, with the slab floats it needs),
 * side 1 = decoder block `layer`; kind 'F' | 'D' | 'W' after
 * the launchers (encoder: F forward, D data gradient; decoder: D forward, F data gradient; W filter gradient).  out[12]:
 *   F / D: 0 path (0 generic implicit GEMM | 1 spatial | 2 split-K generic), 1 splits, 2 slabs reduced inside the kernel (ticket counters), 3 column-block
 *          instance (64 | 32), 4 column-partial tiles, 5 bf16x6 three-plane route (1 taken | 0 refused: exact-fp32 fall-back | -1 other math modes),
 *          (a training step's operand forms are assumed), 6 fused final epilogue (1 | 0; -1 unless the decoder's last D), 7 0, 8 slab-workspace floats needed, 9 ... allocated,
 *          10 BN column-partial floats a data gradient writes (0 for a forward), 11 ... allocated per slot;
 *   W:     0 kernel (0 generic | 1 k5 s2 tile kernel | 2 k3 tap-list kernel | 3 first-layer kernel), 1 splits, 2 last split short, 3 32-channel cs blocks per workgroup (k5: 1 | 2),
 *          4 work units (8 x 8 output tiles; generic: 32-position K steps), 5 bf16x6 three-plane kernel (1 | 0 | -1), 6 -1, 7 units per split,
 *          8 filter-gradient slab floats needed, 9 ... allocated per slot, 10 0, 11 as above.
 * side 2 = the dense bottleneck between encoder and decoder (AE / VAE / ceVAE handles; UAD_ERR_INVALID on the others), layer 0, kind 'B'.  out[12]:
 *   B:     0 fused forward / backward, one kernel each (1 | 0: the chain of generic 1x1 / dense launches), 1 workgroups per sample (1 | 4: partial vectors exchanged
 *          through global memory), 2 parameter gradients in one fused launch (1 | 0: four filter-gradient GEMMs + column sums | -1 when 0 is unfused: the GEMMs
 *          are the only way), 3 k-groups the 1024 threads form over a workgroup's feature slice (1024 / slice width when the slice is narrower, else 1; the slice
 *          is all of inter_res^2 * cmid features with one workgroup per sample; on an unfused handle 1 and 3 are what uad_bottleneck_group chose before
 *          uad_bottleneck_fused_ok refused, i.e. the split the slice rule was tested against), 4 dynamic LDS bytes of the forward kernel, 5 ... of the backward kernel (0 when
 *          unfused; the cap is 150 KiB), 6 64-sample chunks the fused parameter-gradient kernel stages at this batch (n, 2n inside a ceVAE handle), 7 rows in
 *          the last chunk, 8 largest filter-gradient slab floats any of the four bottleneck filter-gradient GEMMs needs at this batch, 9 ... allocated per slot,
 *          10 largest scratch floats any of the bottleneck's bias column sums needs at this batch (row chunks x columns; 0 when every sum is one chunk, which
 *          writes its output directly), 11 ... allocated.  8 - 11 are reported on every route: UAD_NO_FUSED_BOTT / _WGRAD move a handle onto the GEMMs. */
int uad_debug_plan(uad_model_t* m, int side, int layer, int kind, int n, long long* out);

/* per-launch-group HIP-event profiler (bench.py's roofline leg).  While enabled, every launch group of
 * uad_forward / uad_backward / uad_adam_step is bracketed by hipEventRecord on the caller's stream.
 * uad_profile_report synchronises the device and writes lines "tag count total_ms\n" into buf, then clears. */
int uad_profile_enable(uad_model_t* m, int on);
int uad_profile_report(uad_model_t* m, char* buf, int cap);

/* residual anomaly map: out = mask * (pos_only ? max(x - xr, 0) : |x - xr|), zero where x < prior_thresh
 * (pass -INFINITY to disable); l1err[n] = sum |x - xr| per sample (may be NULL); mask may be NULL. hw = H*W*C. */
int uad_residual(const float* x, const float* xr, const float* mask, int n, int hw, int pos_only, float prior_thresh,
                 float* out, float* l1err, void* stream);

/* ---- residual-map scoring on the device (utils/Evaluation.py:84-127, 238-312; trainers/Metrics.py) ----------------------
 * uad_erode_cross: scipy.ndimage.binary_erosion(mask, generate_binary_structure(2,1), iterations) per [H,W] slice, zero
 *   border (utils/Evaluation.py:84-89 with iterations = 12); mask/out are fp32 [n,H,W], out = 1.0 where the pixel survives.
 * uad_median3d: scipy.ndimage.median_filter(vol, (5,5,5)) with the default 'reflect' boundary (utils/Evaluation.py:108-110).
 * uad_scores_*: every threshold metric of trainers/Metrics.py from ONE descending device sort of the n voxel scores:
 *   AUROC (sklearn roc_curve + auc, Metrics.py:45-47), AUPRC (sklearn average_precision_score, :17-19) and
 *   dice(score > t, label) for batches of thresholds (the inner step of compute_dice_curve_recursive, :138-162).
 *   label: fp32, nonzero = positive.  create is synchronous (allocates; one 32-bit radix sort + scans).
 *   Single-class labels give what the reference's numpy divisions give: no positive label -> AUROC = AUPRC = nan; no negative
 *   label -> AUROC = nan, AUPRC = 1; dice with nothing predicted and nothing labelled -> nan (0/0).  Thresholds are the distinct
 *   scores under numpy's `diff != 0`: -0.0 and +0.0 are one threshold, every +-inf score is one of its own (inf - inf is nan);
 *   nan scores are undefined. */
typedef struct uad_scores uad_scores_t;
int uad_erode_cross(const float* mask, int n, int H, int W, int iterations, float* out, void* stream);
int uad_median3d(const float* vol, int D, int H, int W, int ksize, float* out, void* stream);
/* Monte-Carlo dropout statistics of K reconstructions (utils/Evaluation.py:238-266 with numMonteCarloSamples > 1): recs [K, total],
 * optional mask [total] (the eroded brain mask is applied to every sample first, as the reference does); mean [total] = E[mask*rec],
 * var [total] (may be NULL) = E[(mask*rec)^2] - E[mask*rec]^2 = Metrics.combined_predictive_uncertainty(x_recs, 0) (:170-173) */
int uad_mc_stats(const float* recs, const float* mask, int K, long long total, float* mean, float* var, void* stream);
/* utils/Evaluation.py:113-127 filter_3d_connected_components: out = vol with every 26-connected component of non-zero voxels that has
 * at most max_voxels (reference: 7) voxels set to 0 (bounded flood fill per voxel, exact; max_voxels < 16; not in place) */
int uad_cc_filter(const float* vol, int D, int H, int W, int max_voxels, float* out, void* stream);
int uad_scores_create(const float* pred, const float* label, long long n, uad_scores_t** out, void* stream);
int uad_scores_auc(const uad_scores_t* s, double* auroc, double* auprc, double* positives);
int uad_scores_dice(uad_scores_t* s, const double* thresholds_host, int k, double* dice_host, void* stream);
int uad_scores_destroy(uad_scores_t* s);
/* trainers/Metrics.py:17-19 + utils/Evaluation.py:439 (`np.argmax(_precisions <= 0.7)` on sklearn's precision_recall_curve): the threshold at
 * the first point of that curve's ordering (increasing threshold) whose precision is <= `precision`; the smallest threshold when no point
 * qualifies (argmax of all-False is 0).  The result is one of the sorted fp32 scores.  Synchronous, on the stream uad_scores_create ran on. */
int uad_scores_threshold_at_precision(const uad_scores_t* s, double precision, double* threshold);
/* 26-connected component labelling of a binary [D,H,W] volume (non-zero = foreground), the device form of skimage.measure.label(volume) as
 * utils/Evaluation.py:113-127,130-172 call it.  labels [D,H,W] int32 (device): 0 = background, otherwise 1 + the smallest linear index
 * (z*H + y)*W + x of the voxel's component -- unique, and the component's first voxel in raster order (regionprops' coords[0]).
 * slab: groups of `slab` consecutive slices are labelled independently (<= 0 or >= D: the whole volume); the reference labels in chunks of 20.
 * *n_components (device, or NULL) = number of distinct labels.  Union-find: tiles in LDS, tile borders by atomicMin, one flattening pass;
 * asynchronous, no workspace.  D*H*W < 2^31. */
int uad_cc_label(const float* vol, int D, int H, int W, int slab, int* labels, int* n_components, void* stream);
/* utils/Evaluation.py:130-172 compute_detection_rate: per slab, TPs = components of pred & gt; a predicted component of at least min_voxels
 * (reference: 8) voxels that contains the first voxel of no intersection component is a FP; a ground-truth component that contains none is a
 * FN.  counts3 (device, 3 x long long) = { TPs, FPs, FNs } summed over the slabs (reference: slab = 20).  The workspace (16 bytes per voxel)
 * is allocated and freed inside the call, which is therefore synchronous. */
int uad_detection_rate(const float* pred, const float* gt, int D, int H, int W, int slab, int min_voxels, long long* counts3, void* stream);

/* ---- noise of one step, drawn on the device --------------------------------------------------------------------
 * The reference draws eps (tf.random_normal, models/variational_autoencoder.py:34) and the dropout masks (keras Dropout(rate)(x, training),
 * e.g. :28-30) inside the graph on every sess.run; here they are explicit inputs of uad_forward, and this call fills them without a host
 * round trip.  Philox4x32-10, key = seed, counter = (element / 4, GLOBAL sample index sample0 + i, step, stream id): sample i of the
 * call gets the same numbers whichever rank / batch split draws it (data-parallel runs reproduce the single-process run).
 *   kind UAD_RNG_NORMAL:    out[i][e] ~ N(0, 1) (Box-Muller on 24-bit uniforms)
 *   kind UAD_RNG_KEEP_MASK: out[i][e] = u >= rate ? 1 / (1 - rate) : 0        (nn.dropout's rule, pre-scaled)
 * jobs: up to 8 arrays [n, per_sample] filled by ONE launch; `stream` tells independent arrays of a step apart (mu / sigma / dec masks). */
enum { UAD_RNG_NORMAL = 0, UAD_RNG_KEEP_MASK = 1 };
typedef struct { float* out; int per_sample; int kind; float rate; int stream; } uad_rng_job_t;
int uad_rng_fill(const uad_rng_job_t* jobs, int njobs, int n, unsigned long long seed, unsigned long long step, long long sample0, void* stream);

/* ---- measurement: the shader clock under load ---------------------------------------------------------------------
 * One wave, launched on `stream` (give it a stream of its own, beside the workload), samples s_memtime (shader cycles) and s_memrealtime
 * (100 MHz) for ticks_100mhz ticks and writes out2[0] = shader cycles, out2[1] = 100 MHz ticks (device memory): clock [GHz] =
 * out2[0] / out2[1] / 10.  bench.py prices `roofline.frac` at the 2.4 GHz spec clock and reports `frac_at_measured_clock` beside it. */
int uad_clock_probe(unsigned long long* out2, unsigned long long ticks_100mhz, void* stream);

/* ---- batch assembly from an HBM-resident slice cache ------------------------------------------------------------
 * Replaces the host-side batch slicing of dataloaders/BRAINWEB.py:411-478 (`next_batch`: images[images_in_set[start:end]], the label
 * -> brain-mask mapping :466-476) when the whole slice set lives in device memory (288 GB HBM): no H2D copy per step.
 *   uad_gather_slices: out[b] = src[idx[b]]                      src [N, slice_elems] fp32, idx device int32 [n]
 *   uad_gather_mask:   out[b][p] = lut256[labels[idx[b]][p]]     labels [N, slice_px] u8; lut256 NULL = the label value as float */
int uad_gather_slices(const float* src, const int* idx, int n, long long slice_elems, float* out, void* stream);
int uad_gather_mask(const unsigned char* labels, const int* idx, int n, long long slice_px, const unsigned char* lut256, float* out,
                    void* stream);

/* ---- context masking and instance noise of a batch (csrc/uad_batch.hip) --------------------------------------------------------
 * uad_brain_boxes / uad_brain_boxes_f32  <- trainers/CE.py:124-126 (np.argwhere(brainmask): min / max row and column of the brain):
 *   boxes[i] (DEVICE int32 [n,4]) = (row_min, row_max, col_min, col_max), both ends inclusive, of the non-zero pixels of slice i;
 *   (-1, -1, -1, -1) for a slice that has none.  labels: DEVICE u8 [n, H*W] read through lut256 (DEVICE u8 [256]; NULL = the label value,
 *   the uad_gather_mask convention), any base alignment; masks: DEVICE fp32 [n,H,W], non-zero = set (NaN counts, -0.0 does not).  One
 *   launch, one workgroup a slice, integers only: the result does not depend on the order of execution.  UAD_ERR_INVALID: a non-positive
 *   size, a NULL input / boxes.  UAD_ERR_UNSUPPORTED: H * W >= 2^31.
 * uad_assemble_batch  <- dataloaders/BRAINWEB.py:411-459 (next_batch: the slice gather, :459 + numpy.random.normal(0, 0.01) under
 *   Options.addInstanceNoise; MSLUB.py:468 and the other loaders alike) and trainers/CE.py:128-139 (the squares zeroed, batch * mask):
 *     out_x[b]  = src[idx ? idx[b] : b]  (+ sigma * N(0,1) when sigma != 0)
 *     out_ce[b] = out_x[b] * m_b
 *   src: DEVICE fp32 [N,H,W,C]; idx: DEVICE int32 [n] or NULL (entries outside [0, N) are the caller's error); out_x / out_ce: DEVICE fp32
 *   [n,H,W,C], either may be NULL but not both.  rects: DEVICE int32 [n,3,4], up to three windows (row, col, height, width) a sample,
 *   height == 0 = unused; given exactly when out_ce is.  m_b is 0.0f inside any window of sample b (all channels), 1.0f elsewhere, and the
 *   product is an fp32 multiply as the host's batch * mask: -x under a window gives -0.0, NaN stays NaN.  Windows that leave the slice are
 *   the caller's error (DeviceOps.assemble_batch validates them on the host); they are only compared with, never used as addresses.
 *   Noise: the numbers uad_rng_fill writes for kind UAD_RNG_NORMAL, per_sample = H*W*C and the same (seed, step, sample0, stream id =
 *   rng_stream), element for element, added as x + (sigma * n) in fp32 without a fused multiply-add; sample b is GLOBAL sample sample0 + b.
 *   With sigma == 0 out_x holds the source words.  One launch, no workspace, no atomics, nothing written outside out_x / out_ce.
 *   UAD_ERR_INVALID: a non-positive size, H*W*C not a multiple of 4, sigma negative or not finite, sample0 < 0, NULL src, no output, out_ce
 *   without rects or rects without out_ce, an output aliasing src or the other output.  UAD_ERR_UNSUPPORTED: n > 65535. */
int uad_brain_boxes(const unsigned char* labels, int n, int H, int W, const unsigned char* lut256, int* boxes, void* stream);
int uad_brain_boxes_f32(const float* masks, int n, int H, int W, int* boxes, void* stream);
int uad_assemble_batch(const float* src, const int* idx, int n, int H, int W, int C, const int* rects, float sigma, unsigned long long seed,
                       unsigned long long step, long long sample0, int rng_stream, float* out_x, float* out_ce, void* stream);

/* ---- cubic-spline slice resampling (utils/Evaluation.py:223-232, 323-334; the slice ingestion of the dataloaders) ------------
 * uad_zoom_spline3: scipy.ndimage.zoom(a, (H/h, W/w), order=3, mode=..., prefilter=True, grid_mode=False) of every [h,w] slice of an
 *   fp32 [n,h,w] batch -> [n,H,W].  The CALLER fixes the output shape (scipy: round(h * zoom)); output sample o reads input coordinate
 *   o (h-1)/(H-1) (0 when H == 1).  boundary UAD_ZOOM_CONSTANT = scipy mode 'constant' with cval 0: no padding, the prefilter and the
 *   taps that step over the edge use the mirror extension (c[-1] = c[1]); UAD_ZOOM_NEAREST = scipy mode 'nearest': every line is extended
 *   by 12 edge-replicated samples on each side, filtered with the mirror recursion, and the taps read the padded coefficients.
 *   out_kind UAD_ZOOM_F32: fp32 [n,H,W]; UAD_ZOOM_I32: int32 [n,H,W], t > 0 ? (int)(t + 0.5) : (int)(t - 0.5) -- what scipy does to an
 *   integer-typed input (label / skull maps): the same spline, rounded half away from zero, NOT nearest-neighbour sampling.
 *   Coefficients (pole sqrt(3) - 2, gain 6 per axis) and interpolation are fp64 so that the integer maps round as scipy rounds them.
 *   A 3-D zoom of [S,h,w] with factor 1 on axis 0 is this call with n = S (the coefficients of a factor-1 axis evaluated at its
 *   knots are the samples), so one entry serves ingestion and the exportVolumes de-zoom.  h, w >= 2.  No atomics: a slice's result
 *   does not depend on n.  workspace: device memory of at least uad_zoom_spline3_workspace(n, h, w, boundary) bytes (the fp64
 *   coefficient planes), 16-byte aligned, owned by the caller and free for reuse once the call's work on `stream` is done. */
enum { UAD_ZOOM_CONSTANT = 0, UAD_ZOOM_NEAREST = 1 };
enum { UAD_ZOOM_F32 = 0, UAD_ZOOM_I32 = 1 };
size_t uad_zoom_spline3_workspace(int n, int h, int w, int boundary);
int uad_zoom_spline3(const float* in, int n, int h, int w, int H, int W, int boundary, int out_kind, void* out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- cubic-spline affine transforms: the rotation augmentation (dataloaders/BRAINWEB.py:156-162, MSLUB.py / MSISBI2015.py alike) ----
 * uad_affine_spline3: scipy.ndimage.affine_transform(a, M, offset, output_shape=(H,W), order=3, mode=..., prefilter=True) of every [h,w]
 *   slice of an fp32 [n,h,w] batch under K transforms that share one prefilter -> [n,K,H,W].  xf: HOST array of K x 6 doubles
 *   (m00 m01 m10 m11 off0 off1), 1 <= K <= UAD_AFFINE_MAX_K, all finite; output pixel (Y,X) reads the input coordinate
 *   ((Y m00 + X m01) + off0, (Y m10 + X m11) + off1) in fp64 without fused multiply-adds -- scipy's order, so its coordinates bit for bit.
 *   scipy.ndimage.rotate(a, angle, reshape=False) (the reference's call, once per slice and angle, and again with mode='nearest' for the
 *   label map) is this with M = [[c, s], [-s, c]], c / s = cosdg / sindg(angle) and offset = (shape-1)/2 - M @ (shape-1)/2.
 *   boundary UAD_ZOOM_CONSTANT = mode 'constant', cval 0: mirror prefilter, no padding; a pixel whose coordinate lies outside [0, h-1] x
 *   [0, w-1] is 0, otherwise taps that step over the edge are mirror-folded.  UAD_ZOOM_NEAREST = mode 'nearest': every line is extended by
 *   12 edge-replicated samples a side and filtered with scipy's REFLECT initial values (unlike uad_zoom_spline3, whose coordinates never
 *   reach the outer padding); the coordinate moves by 12 and is not clamped, the four tap INDICES are clamped to the padded line.
 *   out_kind as uad_zoom_spline3 (fp32, or int32 rounded half away from zero).  Transform k of a K-call has the bits of the K = 1 call, and a
 *   slice's bits do not depend on n (no atomics).  h, w >= 2.  workspace: device memory of at least uad_affine_spline3_workspace(n, h, w,
 *   boundary) bytes (the fp64 coefficient planes), 16-byte aligned, owned by the caller, free once the call's work on `stream` is done. */
enum { UAD_AFFINE_MAX_K = 16 };
size_t uad_affine_spline3_workspace(int n, int h, int w, int boundary);
int uad_affine_spline3(const float* in, int n, int h, int w, int H, int W, const double* xf, int K, int boundary, int out_kind, void* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- curvature-flow denoising of a volume (csrc/uad_flow.hip) <- utils/NII.py:85-87, nii.denoise() ------------------------------
 * uad_curvature_flow: sitk.CurvatureFlow(image, timeStep = time_step, numberOfIterations = iterations) of one [nz,ny,nx] volume as
 *   utils/curvature_flow.py states it from ITK's CurvatureFlowFunction::ComputeUpdate (that statement has not been compared with
 *   SimpleITK's own output): per iteration one Jacobi sweep of a 19-point fp64 stencil, differences of dimension i scaled by
 *   1 / spacing_xyz[i] (HOST array, x y z), neighbours clamped per axis, update 0 where the squared gradient is below 1e-9.  Every
 *   operation is one IEEE fp64 add, multiply or divide in the host statement's order without fused multiply-adds: the result equals the
 *   host statement's bit for bit.  in: DEVICE fp64, or fp32 (in_is_f32 != 0; widened exactly); out: DEVICE fp64, may not alias in.
 *   iterations = 0 copies.  One launch per iteration; iterations >= 2 ping-pong between out and workspace: device memory of at least
 *   uad_curvature_flow_workspace(nz, ny, nx) bytes (one fp64 volume), owned by the caller, free once the call's work on `stream` is
 *   done; it may be NULL for iterations < 2.  UAD_ERR_INVALID: a non-positive dimension, a non-positive or non-finite spacing,
 *   negative iterations, NULL or aliased pointers. */
size_t uad_curvature_flow_workspace(int nz, int ny, int nx);
int uad_curvature_flow(const void* in, int in_is_f32, int nz, int ny, int nx, const double spacing_xyz[3], double time_step, int iterations,
                       double* out, void* workspace, void* stream);

/* ---- bilinear / nearest resize of slices and tissue-class masking (csrc/uad_resize.hip) <- dataloaders/BRAINWEB.py:140-142, 266-289 ----
 * uad_resize2d: cv2.resize(a, (W, H)) with INTER_LINEAR (UAD_RESIZE_LINEAR) or INTER_NEAREST (UAD_RESIZE_NEAREST) of [h,w] fp32 slices as
 *   utils/resize.py states it from OpenCV 4.2's resize.cpp (that statement has not been compared with OpenCV's own output).  Per axis
 *   scale = 1.0 / ((double)dst / (double)src).  Linear: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= (float)s in fp32, s < 0 ->
 *   (0, 0), s >= src - 1 -> (src - 1, 0), taps s and min(s + 1, src - 1) weighted (1.0f - f, f); the horizontal pass first, then the vertical
 *   one, every multiply and add one fp32 operation without fused multiply-adds.  Nearest: min(floor(d * scale), src - 1) in fp64 -- not
 *   d * src / dst (22 -> 18: output 9 reads input 10) -- and the value's bits are copied.  The result equals the host statement's bit for bit.
 *   in: DEVICE fp32 [n_in,h,w]; out: DEVICE fp32 [n,H,W], may not alias in.  Output slice j is the resize of input slice slice_idx[j]
 *   (DEVICE int32 [n], any order, repeats allowed: the kept slices of a resident slice-major volume are resized where they lie); NULL =
 *   identity, which needs n == n_in.  Entries outside [0, n_in) are the caller's error (engine.resize validates them on the host).
 *   One launch, no workspace, no atomics, no host synchronisation: the per-axis tables are formed in the kernel, once per workgroup in LDS;
 *   a slice's bits depend on neither n nor its position in the batch.  h, w, H, W, n, n_in >= 1.  UAD_ERR_INVALID: a non-positive size, an
 *   unknown mode, NULL in / out, out aliasing in, NULL slice_idx with n != n_in.
 *   UAD_ERR_UNSUPPORTED: more than one grid holds -- n > 65535 output slices or H > 524280 output rows (65535 row tiles of 8); split the call.
 * uad_mask_by_label: out[i] = lut256[labels[i]] ? vol[i] : 0 (out may alias vol) and, unless lesion_out is NULL, lesion_out[i] =
 *   labels[i] == lesion_label ? 1 : 0 -- load_volume_and_groundtruth's skull-map multiply and lesion binarisation (BRAINWEB.py:266-289) in
 *   one pass over a tissue-class volume; the LUT idea of uad_gather_mask.  vol / out / lesion_out: DEVICE fp32 [n]; labels: DEVICE u8 [n];
 *   lut256: DEVICE u8 [256].  A masked element is +0 whatever its sign was. */
enum { UAD_RESIZE_LINEAR = 0, UAD_RESIZE_NEAREST = 1 };
int uad_resize2d(const float* in, int n_in, int h, int w, const int* slice_idx, int n, int H, int W, int mode, float* out, void* stream);
int uad_mask_by_label(const float* vol, const unsigned char* labels, long long n, const unsigned char* lut256, float* out, float* lesion_out,
                      int lesion_label, void* stream);

/* ---- component measurements and crop windows (csrc/uad_crops.hip) <- dataloaders/MSLUB.py:200-222 (MSISBI2015.py / MSSEG2008.py alike),
 *      dataloaders/BRAINWEB.py:166-173, utils/image_utils.py:15-16 --------------------------------------------------------------
 * uad_cc_props: the `regionprops` half of cropType 'lesions' (MSLUB.py:201-206: label, regionprops, prop['centroid']) as utils/crops.py's
 *   component_props states it (skimage is not a dependency; that statement has not been compared with skimage's own output).
 *   labels: DEVICE int32 [D,H,W], the output of uad_cc_label with any slab (with slab = 1 every slice is labelled on its own: skimage's
 *   8-connectivity on a 2-D slice).  props: DEVICE int64 [max_components,5], one row per component -- first (its smallest linear index
 *   (z*H + y)*W + x), area, sum_z, sum_y, sum_x -- ordered by `first`, ascending: slice-major for slab = 1 and regionprops' order inside a
 *   slice; the centroid is (sum_z, sum_y, sum_x) / area.  *n_components (DEVICE) = the true number of components, also when it exceeds
 *   max_components: then only the first max_components rows are written and nothing is written past them.
 *   Roots (labels[v] == v + 1) are counted per tile and ranked in index order by a scan, then every foreground voxel adds to its root's row:
 *   integers only -- 64-bit LDS atomics per tile, 64-bit global atomics for the rest -- so the result does not depend on the order of
 *   execution.  Four launches, no host synchronisation.  workspace: device memory of at least uad_cc_props_workspace(D, H, W) bytes (the
 *   tile counts and one int32 per voxel), 16-byte aligned, owned by the caller, any contents, free once the call's work on `stream` is
 *   done.  UAD_ERR_INVALID: a non-positive size (the workspace query returns 0), max_components < 1, a NULL pointer, D*H*W >= 2^31.
 * uad_crop2d: image_utils.crop (img[y:y + height, x:x + width]; MSLUB.py:215-218, BRAINWEB.py:172-173) for k windows at once: out[j] (DEVICE
 *   fp32 [k,ch,cw]) = the ch x cw window of slice origins[j][0] of in (DEVICE fp32 [n_in,h,w]) with its top-left corner at row origins[j][1],
 *   column origins[j][2].  origins: DEVICE int32 [k,3] of (slice, top, left), any order, repeats allowed.  The words are copied: +-0,
 *   denormals and NaN payloads survive.  One launch, no workspace, no atomics; 16-byte stores where cw is a multiple of four and out is
 *   16-byte aligned.  A slice outside [0, n_in) or a window that leaves the slice is the caller's error (engine.crop validates the origins on
 *   the host).  UAD_ERR_INVALID: a non-positive size, ch > h or cw > w, a NULL pointer, out aliasing in.  UAD_ERR_UNSUPPORTED: more than one
 *   grid holds -- k > 65535 windows; split the call. */
size_t uad_cc_props_workspace(int D, int H, int W);
int uad_cc_props(const int* labels, int D, int H, int W, long long* props, int max_components, int* n_components, void* workspace, void* stream);
int uad_crop2d(const float* in, int n_in, int h, int w, const int* origins, int k, int ch, int cw, float* out, void* stream);

/* ---- 8-bit rendering of the evaluation sample images (csrc/uad_render.hip) <- utils/Evaluation.py:302-321, 368, 501-507,
 *      utils/image_utils.py:22-45, utils/utils.py:21-26 ---------------------------------------------------------------------------
 * The arithmetic is utils/render.py's, operation for operation, and the result equals that statement's bit for bit (the heat map up to the
 * last place of exp()).  Inputs are finite; what a NaN gives is unspecified.  One launch each, no workspace, no atomics, no host
 * synchronisation; a slice's bytes depend on neither n nor its place in the batch.
 * uad_render_minmax_u8: normalize_and_squeeze (:368) = cv2.normalize(x, None, 0, 255, NORM_MINMAX) + astype('uint8') of every [hw] slice as
 *   the statement restates OpenCV's documented arithmetic (it has not been compared with OpenCV's own output, which may fuse the
 *   multiply-add): smin, smax in fp32; in fp64 scale = smax - smin > DBL_EPSILON ? 255 / (smax - smin) : 0, shift = -smin * scale; per pixel
 *   in fp32 v = fl(fl(x * (float)scale) + (float)shift); the byte is v truncated toward zero, clamped to 0 .. 255.  A constant slice gives
 *   zeros.  x: DEVICE fp32 [n,hw]; out: DEVICE u8 [n,hw].
 * uad_render_heatmap: `_heatmap.png` (:319-321) of every [h,w] slice of d: in fp64 q = 2 * (1 / (1 + exp(-100 d)) - 0.5), the colour bar
 *   q[i][w-1] = i / h, q -= min q, q /= max q unless that is 0, index = min((int)(q * 256), 255), out = lut256x4[index].  d: DEVICE fp32
 *   [n,h,w]; lut256x4: DEVICE u8 [256,4] (any table; the jet table is data of the package); out_rgba: DEVICE u8 [n,h,w,4], 4-byte aligned.
 * uad_render_overlay: augment_prediction_and_groundtruth_to_image (image_utils.py:22-45): grey max(x, 0) on three channels; where pred != 0
 *   or gt != 0 the colour of TP (0, 1, 0), FP (1, 0.5, 0) or FN (1, 0, 0); the bytes are (uint8)(clip(v, 0, 1) * 255) in fp32, truncated
 *   (0.5 -> 127).  Stated deviation: the reference's cv2.normalize(tmp, None, 0, 255) with the default norm type and alpha = 0 scales every
 *   image to zero.  x, pred: DEVICE fp32 [n,hw]; gt: DEVICE u8 [n,hw]; out_rgb: DEVICE u8 [n,hw,3].
 * One workgroup renders a slice of the two normalising ops: up to 256 x 256 pixels (heat map: 128 x 128) the slice is read once and kept in
 * registers between the reduction and the map, larger slices are read twice.  n == 0: UAD_OK, nothing is launched.  UAD_ERR_INVALID: n < 0, a non-positive
 * size, a NULL pointer, out aliasing an input, out_rgba not 4-byte aligned.  UAD_ERR_UNSUPPORTED: a slice of more than 2^31 - 5 pixels. */
int uad_render_minmax_u8(const float* x, int n, int hw, uint8_t* out, void* stream);
int uad_render_heatmap(const float* d, int n, int h, int w, const uint8_t* lut256x4, uint8_t* out_rgba, void* stream);
int uad_render_overlay(const float* x, const float* pred, const uint8_t* gt, int n, int hw, uint8_t* out_rgb, void* stream);

/* ---- order statistics without a sort (csrc/uad_select.hip) ----------------------------------------------------
 * uad_select_quantiles: segmented radix select over fp32 `in` [n_seg, n_per_seg] (device, contiguous).  For each segment: m = the number
 *   of values that pass `filter` (UAD_SELECT_ALL | UAD_SELECT_NONNEG: v >= 0) -> m_out[seg] (int64), and for each of the k <=
 *   UAD_SELECT_MAX_Q fractions q[j] (host doubles in [0, 1]) the two order statistics of the passing values that bracket the virtual index
 *   v = (m - 1) * q[j] of numpy's 'linear' method -- lo = x_(floor v), hi = x_(min(floor v + 1, m - 1)) -> bracket_out[seg][2 j], [2 j + 1]
 *   (fp32 [n_seg, 2 k]).  Both are values of the input, bit for bit: no arithmetic touches a value; the caller finishes the interpolation.
 *   The index is ONE multiply on the device in the float type numpy forms it in: double, or -- bit j of f32_index_mask -- float32, which
 *   is what np.percentile / np.quantile of a float32 array with a Python-scalar q do ((n - 1) * float32(q), next = float32(floor v) + 1).
 *   This is np.percentile(v, 0 / 99.8) + max of utils/NII.py:50-66 in one call (q = {lower, upper, 1}), np.percentile(slice, 90) of
 *   dataloaders/MSLUB.py:161 with one segment per slice, np.quantile(volume, 0.9) of utils/Evaluation.py:205, and, with UAD_SELECT_NONNEG,
 *   np.percentile(var[var >= 0], 99.8) of utils/Evaluation.py:404-408.  m == 0: the brackets are NaN.
 *   PRECONDITION: the input holds no NaN (the NIfTI reader zeroes them, utils/NII.py:12-16); a NaN is ordered by its bit pattern.  -0 and +0
 *   compare equal as in numpy; +0 is returned for either.  +-inf are ordinary values.
 *   Four passes over the 8-bit digits of the order-preserving key, most significant first, four launches, no host synchronisation, no
 *   second copy of the data: 4 x 4 B x n of HBM reads.  Grid = (tiles of UAD_SELECT_TILE values per segment, segments).  Integer atomics only:
 *   results are bit-reproducible and a segment's result does not depend on the other segments.
 *   workspace: device memory of at least uad_select_workspace(n_seg) bytes, 16-byte aligned, owned by the caller, any contents, free for
 *   reuse once the call's work on `stream` is done.  n_seg <= 65535, n_per_seg <= 2^31 - 1.
 * uad_histogram_edges: counts[i] (int64 [bins], device) = the number of values with edges[i] <= v < edges[i + 1], the last bin closed
 *   (v <= edges[bins]); values outside [edges[0], edges[bins]] and NaNs are dropped.  edges: bins + 1 fp32 on the device, non-decreasing, bins <=
 *   UAD_HISTOGRAM_MAX_BINS.  With the table np.histogram_bin_edges gives this is np.histogram (utils/Evaluation.py:404-408: 50 bins).
 * uad_clamp_scale: out[i] = (v < lo ? lo : v > hi ? hi : v) * scale, the clamp-and-scale tail of utils/NII.py:57-66; out may alias in.
 * uad_select_quantiles_masked: uad_select_quantiles of ONE segment of n values restricted to the values with labels[i] == class_id (labels:
 *   u8 [n], device) and lo <= v <= hi (fp32 bounds from the host, formed so that the fp32 test equals the caller's fp64 one) -- the
 *   `data[labels == classes[0]]` of utils/utils.py:49 cut to the histogram range as np.histogram's bins='auto' cuts it (utils/Evaluation.py:
 *   399-402).  q = {0, 0.25, 0.75, 1} gives what numpy's 'auto' width needs: m, min, max and the brackets of both quartiles.  Same kernels
 *   (a template parameter), same contract: m, the bracketing order statistics per fraction, integer atomics only, bit-reproducible, no host
 *   synchronisation, workspace of uad_select_workspace(1) bytes.  n <= 2^31 - 1.
 * uad_histogram_by_class (csrc/uad_hist.hip): plot_histogram_with_labels (utils/utils.py:44-71, called at utils/Evaluation.py:400-402 and
 *   :409-411) in one pass over `in` (fp32 [n], device) and `labels` (u8 [n] class ids 0 .. n_classes - 1, n_classes <=
 *   UAD_HISTOGRAM_MAX_CLASSES; ids at or above n_classes are dropped):
 *   counts[c][i] (int64 [n_classes, bins], device) on ONE shared edge table with the bin rule of uad_histogram_edges (last bin closed, NaN
 *   and out-of-table values dropped; a non-monotone table is the caller's error), bins <= UAD_HISTOGRAM_MAX_BINS a call -- a longer table is
 *   counted in chunks, one call each, every chunk but the last with its last edge lowered by one fp32 ulp; bins == 0: no histogram (edges
 *   and counts may be NULL);
 *   class_count[c] (int64 [n_classes]) and sums[c] (fp64 [n_classes]) over ALL values of class c, in the table or not: sum of v with centre
 *   == NULL, else sum of (v - centre[c])^2 (centre: fp64 [n_classes], device).  Two calls give the two-pass np.mean / np.var of :53: the
 *   first without a table, the second with the means as centres.  class_count == sums == NULL: counts only (no workspace needed).
 *   Counters are privatised in LDS per workgroup and added to the global ones with integer atomics.  The fp64 sums use NO floating-point
 *   atomic: a thread adds 32 values, the workgroup adds its 256 runs as a tree in a fixed order, one partial per tile of UAD_SELECT_TILE
 *   values goes to the workspace, one workgroup adds the partials (256 strided runs, the same tree).  Bit-identical from run to run and
 *   independent of the grid.  The longest chain of dependent additions is 32 + 8 + ceil(tiles / 256) + 8 <= UAD_HISTOGRAM_SUM_CHAIN for every
 *   accepted n, so a sum errs by at most UAD_HISTOGRAM_SUM_CHAIN * 2^-53 * sum |terms|.
 *   workspace: device memory of at least uad_histogram_by_class_workspace(n) bytes (64 per tile), 16-byte aligned, owned by the caller, any
 *   contents.  n == 0: UAD_OK, nothing launched, outputs zeroed.  UAD_ERR_INVALID: a NULL pointer that is needed, a negative size, n_classes
 *   outside 1 .. 4, bins above the limit, a short or misaligned workspace.  UAD_ERR_UNSUPPORTED: n > 2^31 - 1. */
enum { UAD_SELECT_ALL = 0, UAD_SELECT_NONNEG = 1 };
enum { UAD_SELECT_MAX_Q = 4, UAD_SELECT_TILE = 8192, UAD_HISTOGRAM_MAX_BINS = 1024 };
enum { UAD_HISTOGRAM_MAX_CLASSES = 4, UAD_HISTOGRAM_SUM_CHAIN = 1073 };
size_t uad_select_workspace(int n_seg);
int uad_select_quantiles(const float* in, int n_seg, long long n_per_seg, const double* q, int k, unsigned f32_index_mask, int filter,
                         long long* m_out, float* bracket_out, void* workspace, size_t workspace_bytes, void* stream);
int uad_histogram_edges(const float* in, long long n, const float* edges, int bins, long long* counts, void* stream);
int uad_clamp_scale(const float* in, long long n, float lo, float hi, float scale, float* out, void* stream);
int uad_select_quantiles_masked(const float* in, const uint8_t* labels, long long n, int class_id, float lo, float hi, const double* q, int k,
                                unsigned f32_index_mask, long long* m_out, float* bracket_out, void* workspace, size_t workspace_bytes, void* stream);
size_t uad_histogram_by_class_workspace(long long n);
int uad_histogram_by_class(const float* in, const uint8_t* labels, long long n, int n_classes, const float* edges, int bins, const double* centre,
                           long long* counts, long long* class_count, double* sums, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-segment voxel confusion counts (csrc/uad_confusion.hip) -------------------------------------------------
 * Metrics.confusion_matrix / dice / precision / recall / tpr / vd of trainers/Metrics.py as utils/Evaluation.py:452-500 calls them, per
 * patient and over the whole test set: each of those scalars is a function of four integers per patient (utils/confusion.py states both
 * halves in numpy).
 * uad_confusion_by_segment: for each of n_segments contiguous segments of a flat voxel array, counts[s] = {TP, FP, FN, TN} (int64
 *   [n_segments, 4], device, 8-byte aligned) of pred[i] > thr against gt[i] != 0 over i in [seg_offsets[s], seg_offsets[s + 1]).
 *   pred: fp32 [n], device, 4-byte aligned (the output of uad_cc_filter, or raw residuals).  thr: the comparison is an ordered `>`, so a NaN
 *   is not a prediction, as in numpy.  gt: u8 [n], device, any byte alignment, non-zero = lesion.  seg_offsets: int64 [n_segments + 1], device,
 *   8-byte aligned, non-decreasing, 0 <= seg_offsets[0] and seg_offsets[n_segments] <= n (the kernels cut an entry outside [0, n] to that
 *   range); empty segments are legal, voxels outside every segment are not counted.  max_seg_len: at least every segment's length; it sizes
 *   the grid only.  counts is zeroed in-stream by the call; TN is formed as length - TP - FP - FN.  Asynchronous, no workspace.
 *   Grid = (a quarter of the tiles of UAD_SELECT_TILE values of the longest segment, segments), held to 2048 workgroups but one per segment at least, which stride over
 *   a segment's tiles.
 *   16-byte loads of the values and dword loads of the labels counted from the 16-byte boundary below the segment's first value, guarded
 *   value-by-value head and tail; three 32-bit counters per thread (a thread sees fewer than 2^23 voxels), one tree reduction in LDS and
 *   three 64-bit integer atomics per workgroup.  Integer atomics only: the counts depend on neither the order of arrival nor the grid.
 *   Reads 4 + 1 B per voxel of a segment, once.
 *   n_segments == 0 or n == 0: UAD_OK, counts zeroed, nothing launched.  UAD_ERR_INVALID: a NULL pointer that is needed, a negative size,
 *   n_segments > 65535, a misaligned pred / seg_offsets / counts.  UAD_ERR_UNSUPPORTED: n > 2^31 - 1. */
int uad_confusion_by_segment(const float* pred, float thr, const uint8_t* gt, long long n, const long long* seg_offsets, int n_segments,
                             long long max_seg_len, long long* counts, void* stream);

/* ---- sums in a defined order and the standardization map (csrc/uad_moments.hip) ---------------------------------
 * NII.normalize(method='standardization') of utils/NII.py:53-75 (and its copy dataloaders/NRRD.py:39-60) on a resident volume: clamp to the
 * percentiles, c = v - mean(v), out = c / std(c), where np.std subtracts the float32 mean of c again before it squares.  Three
 * uad_shifted_sums calls and one uad_clamp_standardize call do it; the caller reads the 16 bytes of sums back between them and rounds
 * each scalar to float32 once (utils/standardize.py states the whole in numpy, same bits):
 *   (shift 0, centre 0) -> sum v          mean32 = f32(sum / n)
 *   (mean32, 0)         -> sum c          m2_32  = f32(sum / n)
 *   (mean32, m2_32)     -> sum e^2        var32  = f32(sum / n), std32 = sqrtf(var32)
 * numpy adds in float32 in an order of its own; these sums are fp64 in the order below -- a stated deviation.
 * uad_shifted_sums: for t_i = f32(f32(clamp(in[i])) - shift) and u_i = f32(t_i - centre), clamp(v) = (v < clamp_lo ? clamp_lo : v >
 *   clamp_hi ? clamp_hi : v) as uad_clamp_scale (-inf / +inf = no bound), sums_out[0] = sum u_i and sums_out[1] = sum f32(u_i * u_i), both
 *   fp64 on the device (8-byte aligned), in ONE pass over `in` (fp32 [n], device, 4-byte aligned) and with NO floating-point atomic.  Order:
 *   tile T is in[T * UAD_SELECT_TILE ..); thread t of the tile adds the values T * UAD_SELECT_TILE + (r * 256 + t) * 4 + e, r = 0 .. 7, e =
 *   0 .. 3, that lie below n -- 32 values, eight 16-byte chunks -- in that order to +0.0; the workgroup adds its 256 runs as a tree (level d
 *   = 128, 64, ... 1: run t + d onto run t); one partial per tile goes to the workspace; one workgroup adds the partials t, t + 256, ... per
 *   thread and its 256 runs with the same tree.  This is the order of uad_histogram_by_class's sums, except that the tiles are counted from
 *   `in` and not from the 16-byte boundary below it: the order is a function of n alone, the result is bit-identical from run to run,
 *   independent of the grid and of the alignment of `in`.  The longest chain of dependent additions is 32 + 8 + ceil(tiles / 256) + 8 <=
 *   UAD_SHIFTED_SUMS_CHAIN for every accepted n, so a sum errs by at most UAD_SHIFTED_SUMS_CHAIN * 2^-53 * sum |terms| (to first order in
 *   2^-53) against the exact sum of the same fp32 terms.  The terms themselves are fp32, unfused.
 *   workspace: device memory of at least uad_shifted_sums_workspace(n) bytes (16 per tile), 16-byte aligned, owned by the caller, any
 *   contents.  n == 0: UAD_OK, nothing launched, sums zeroed.  UAD_ERR_INVALID: a NULL pointer, a negative size, a misaligned pointer, a short
 *   or misaligned workspace.  UAD_ERR_UNSUPPORTED: n > 2^31 - 1.
 * uad_clamp_standardize: out[i] = f32(f32(clamp(in[i]) - mean) / std), a true fp32 division (std == 0 gives NaN / +-inf as numpy's does);
 *   out may alias in.  UAD_ERR_INVALID: a NULL pointer with n > 0, a negative size, a pointer that is not 4-byte aligned. */
enum { UAD_SHIFTED_SUMS_CHAIN = 1072 };
size_t uad_shifted_sums_workspace(long long n);
int uad_shifted_sums(const float* in, long long n, float clamp_lo, float clamp_hi, float shift, float centre, double* sums_out, void* workspace,
                     size_t workspace_bytes, void* stream);
int uad_clamp_standardize(const float* in, long long n, float clamp_lo, float clamp_hi, float mean, float std, float* out, void* stream);

/* ---- f-AnoGAN (unified graph) ------------------------------------------------------------------------------
 * Replaces models/fanogan.py:11-84 (encoder + generator + critic graph) and the three optimisation phases of
 * trainers/fAnoGAN.py:45-77 (losses :50-66, the WGAN-GP penalty's tf.gradients :55-57, three Adams :71-77);
 * uad_gan_reconstruct replaces fAnoGAN.reconstruct :220-239.  One handle owns one flat fp32 parameter buffer in TF
 * variable-creation order (Encoder, Generator, Discriminator groups), its gradient and Adam slots.
 * A phase runs the forward graph the reference's sess.run of that phase needs, the phase's loss, and (want_backward)
 * the gradient of that loss w.r.t. the phase's variable group into the gradient buffer; uad_gan_adam then applies
 * TF-Adam to that group only (each group keeps its own step counter).  All calls are asynchronous on `stream`. */
enum { UAD_GAN_ENCODER = 0, UAD_GAN_GENERATOR = 1, UAD_GAN_DISCRIMINATOR = 2 };
enum { UAD_GAN_UNIFIED = 0, UAD_GAN_RESNET = 1,
       UAD_GAN_ANOVAEGAN = 2 };   /* models/anovaegan.py:10-80 + trainers/AnoVAEGAN.py:45-86 on the unified blocks: the encoder ends in mu /
                                     log-sigma heads (io.mask_z / io.mask_sigma, io.eps), the generator decodes z_vae with a linear output and
                                     the critic judges the reconstruction.  Phases: UAD_GAN_ENCODER = optim_vae (reconstructionLoss +
                                     kl_weight * kl over Encoder + Generator variables; uad_gan_adam(UAD_GAN_ENCODER) steps both, the
                                     Generator with its own second pair of slots, UAD_BUF_ADAM_M2 / _V2), UAD_GAN_GENERATOR = optim_gen,
                                     UAD_GAN_DISCRIMINATOR = optim_dis; io.z is unused */
enum { UAD_GAN_AAE = 3 };        /* dense-bottleneck BN autoencoder + re-encoding constraint and / or latent WGAN-GP critic; cfg.aae_kind:
                                     0 = models/constrained_autoencoder.py:9-48 + trainers/ConstrainedAE.py:36-45,
                                     1 = models/adversarial_autoencoder.py:10-72 + trainers/AAE.py:40-67,
                                     2 = models/constrained_adversarial_autoencoder.py:10-79 + trainers/ConstrainedAAE.py:44-70.
                                     Phases / groups: UAD_GAN_GENERATOR (1) = optim_ae (loss = mean(L2 [+ rho Rec_z]), every autoencoder variable),
                                     UAD_GAN_DISCRIMINATOR (2) = optim_dis (io.z = prior sample, io.alpha = eps of z_hat = z + eps (z - z_)),
                                     UAD_GAN_ENCODER (0) = optim_gen (-mean d_, the variables named 'Encoder/...', own Adam slots);
                                     io.mask_z / mask_g / mask_sigma = dropout masks of z_, dec_dense, z_rec.
                                     3 = the dense GMVAE, models/gaussian_mixture_variational_autoencoder.py:11-76 + trainers/GMVAE.py:56-101:
                                     cfg.zdim = dim_z, cfg.dim = dim_c, cfg.dim_w, cfg.c_lambda; one phase, UAD_GAN_GENERATOR = the optimizer over every
                                     variable (group 1); io.eps_w [n,dim_w] / io.eps [n,dim_z] = reparameterisation noise, io.mask_w_mu / mask_w_ls [n,dim_w],
                                     io.mask_z [n,dim_z] (z_mu; z_log_sigma has no dropout, model :42), io.mask_g [n,flat] (dec_dense);
                                     scalars: UAD_GAN_S_GM_*; restoration through uad_gan_restore_step.
                                     4 = the Zimmerer VAE, models/variational_autoencoder_Zimmerer.py:7-32 under trainers/VAE.py:36-42 (k4 s2 convolutions
                                     16-64-256-1024 + leaky_relu 0.2, no normalisation / dropout; inter_res must be height / 16); one phase,
                                     UAD_GAN_GENERATOR; io.eps [n,zDim]; scalars UAD_GAN_S_REC_LOSS, UAD_GAN_S_KL, UAD_GAN_S_ENC_LOSS (= loss).
                                     5 = the context-encoding VAE on the same stack, models/context_encoder_variational_autoencoder_Zimmerer.py:8-45 under
                                     trainers/ceVAE.py:38-51: io.x_ce, both branches as one 2n-sample pass; want_backward 2 = data-gradient chain only
                                     (io.anomaly without parameter gradients); scalars UAD_GAN_S_LOSS_IMG = Rec_vae, UAD_GAN_S_LOSS_FTS = Rec_ce, UAD_GAN_S_KL,
                                     UAD_GAN_S_REC_LOSS, UAD_GAN_S_ENC_LOSS = loss, UAD_GAN_S_GM_LOSS = loss_vae.
                                     6 = the original-architecture spatial GMVAE, models/gaussian_mixture_variational_autoencoder_You.py:8-85 under
                                     trainers/GMVAE_spatial.py: inter_res = height / 4 (the latent map), cfg as for kind 3, io.eps_w / io.eps =
                                     [n,r,r,dim_w] / [n,r,r,dim_z], no masks; scalars UAD_GAN_S_GM_*; uad_gan_restore_step.
                                     7 = the constrained adversarial autoencoder on residual blocks, models/constrained_adversarial_autoencoder_Chen.py:11-162
                                     under trainers/ConstrainedAAE.py:44-70: cfg.dim (32 | 64), height = 8 * inter_res; phases / groups / io as kind 2
                                     (no dropout masks; io.alpha = the run's scalar eps repeated n times, z_hat = eps z + (1 - eps) z_) */
enum { UAD_GAN_GROUP_VAE = 3 };   /* uad_gan_group only: the contiguous Encoder + Generator slice (AnoVAE-GAN's optim_vae) */
enum { UAD_BUF_ADAM_M2 = 4, UAD_BUF_ADAM_V2 = 5 };
/* scalars[16] written by uad_gan_phase (entries a phase does not compute are left untouched) */
enum { UAD_GAN_S_GEN_LOSS = 0, UAD_GAN_S_DISC_FAKE = 1, UAD_GAN_S_DISC_REAL = 2, UAD_GAN_S_PENALTY = 3, UAD_GAN_S_DISC_LOSS = 4,
       UAD_GAN_S_LOSS_IMG = 5, UAD_GAN_S_LOSS_FTS = 6, UAD_GAN_S_ENC_LOSS = 7, UAD_GAN_S_REC_LOSS = 8, UAD_GAN_S_KL = 9,
       UAD_GAN_S_GM_LOSS = 10, UAD_GAN_S_GM_CON = 11, UAD_GAN_S_GM_W = 12, UAD_GAN_S_GM_C = 13 };   /* dense GMVAE: loss, conditional_prior_loss,
                                                                                                       w_prior_loss, c_prior_loss (mean_p_loss = S_REC_LOSS) */
typedef struct uad_gan uad_gan_t;
typedef struct {
    int height, width, channels;   /* square power-of-two slices, 1 channel */
    int inter_res;                 /* config.intermediateResolutions[0] */
    int zdim;                      /* config.zDim */
    int max_batch;
    float scale, kappa;            /* fAnoGAN.Config :15-16 (gradient-penalty weight, feature-loss weight) */
    int variant;                   /* UAD_GAN_UNIFIED: models/fanogan.py:11-84; UAD_GAN_RESNET: models/fanogan_schlegl.py:11-161
                                      (pre-activation residual blocks, k3 convolutions, avg-pool / k1 s2 shortcuts, tanh output;
                                      height must be 8 * inter_res; no dropout in that graph: mask_z / mask_g are ignored) */
    int dim;                       /* RESNET only: base width (fanogan_schlegl.py:13: 64); 0 = 64 */
    float kl_weight;               /* ANOVAEGAN only: AnoVAEGAN.Config.kl_weight (:17) */
    int aae_kind;                  /* AAE only: 0 constrained AE, 1 AAE, 2 constrained AAE, 3 dense GMVAE, 4 Zimmerer VAE, 5 Zimmerer ceVAE, 6 GMVAE (You), 7 constrained AAE (Chen) */
    float rho;                     /* AAE only: weight of the latent re-encoding term (ConstrainedAE.Config.rho :15) */
    int dim_w;                     /* dense GMVAE only: GMVAE.Config.dim_w (:17); dim_z = zdim, dim_c = dim */
    float c_lambda;                /* dense GMVAE only: GMVAE.Config.c_lambda (:18) */
} uad_gan_config_t;
typedef struct {
    const float* x;                /* [n,H,W,1] batch (critic and encoder phases, reconstruct) */
    const float* z;                /* [n,zDim] sample_z() (generator and critic phases) */
    const float* alpha;            /* [n] the critic phase's interpolation coefficients (tf.random_uniform, fanogan.py:67) */
    const float* mask_z;           /* optional [n,zDim] inverted-dropout keep mask on the encoder's latent (fanogan.py:30) */
    const float* mask_g;           /* optional [n,flat] mask on the generator's dense output (fanogan.py:39,44) */
    float* generated;              /* optional out [n,H,W,1]: x_ (generator / critic phases) */
    float* reconstruction;         /* optional out [n,H,W,1]: x_enc (encoder phase, reconstruct) */
    float* z_enc;                  /* optional out [n,zDim] */
    float* l1_map;                 /* optional out [n,H,W,1]: |x - x_enc| (losses['L1']) */
    float* scalars;                /* optional out [16], UAD_GAN_S_* */
    const float* eps;              /* ANOVAEGAN: [n,zDim] N(0,1) reparameterisation noise (NULL = 0) */
    const float* mask_sigma;       /* ANOVAEGAN: optional keep mask of the log-sigma head (mask_z is the mu head's) */
    const float* eps_w;            /* dense GMVAE: [n,dim_w] N(0,1) noise of w_sampled (NULL = 0); io.eps is z_sampled's */
    const float* mask_w_mu;        /* dense GMVAE: optional [n,dim_w] keep masks of the w_mu / w_log_sigma heads */
    const float* mask_w_ls;
    const float* x_ce;             /* ceVAE on the Zimmerer stack (aae_kind 5): [n,H,W,1] context-masked input (NULL = x) */
    float* l1_map_ce;              /* ... optional out [n,H,W,1]: |x_ce - x_hat_ce| (io.l1_map is the VAE branch's, io.generated = x_hat_ce) */
    float* anomaly;                /* ... optional out [n,H,W,1]: L1_vae * |d loss_vae / d x| (written when want_backward != 0) */
} uad_gan_io_t;
int uad_gan_create(const uad_gan_config_t* cfg, uad_gan_t** out);
int uad_gan_destroy(uad_gan_t* g);
long long uad_gan_param_count(const uad_gan_t* g);
int uad_gan_num_tensors(const uad_gan_t* g);
int uad_gan_tensor_info(const uad_gan_t* g, int idx, char* name, int name_cap, long long* offset, int* rank, int* shape4);
float* uad_gan_buffer(uad_gan_t* g, int which);                         /* UAD_BUF_* device pointers */
int uad_gan_group(const uad_gan_t* g, int group, long long* offset, long long* count);   /* UAD_GAN_* slice of the buffers */
int uad_gan_set_buffer(uad_gan_t* g, int which, const float* host, long long count);
int uad_gan_get_buffer(uad_gan_t* g, int which, float* host, long long count);
int uad_gan_set_math_mode(uad_gan_t* g, int mode);                      /* UAD_MATH_* */
long long uad_gan_get_step(const uad_gan_t* g, int group);
int uad_gan_set_step(uad_gan_t* g, int group, long long t);
/* phase = the variable group being trained: GENERATOR (gen_loss), DISCRIMINATOR (disc_loss incl. penalty), ENCODER (enc_loss) */
int uad_gan_phase(uad_gan_t* g, int phase, const uad_gan_io_t* io, int n, int want_backward, void* stream);
int uad_gan_adam(uad_gan_t* g, int group, float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* Data parallelism of the GAN handles, library-issued (round 6; the reference is single-process: trainers/fAnoGAN.py:70-77,96-129 run one sess.run per phase).
 * With a communicator attached (uad_rccl_comm_create) uad_gan_phase(..., want_backward = 1) all-reduces the TRAINED group's gradient slice itself: the slice is
 * cut into up to four buckets on tensor boundaries and a bucket's ncclAllReduce is enqueued on a collective stream as soon as the last kernel that writes one of
 * its tensors is enqueued -- i.e. while the backward of the earlier layers still runs (ResNet graph: per residual block; the other f-AnoGAN graphs: at the end
 * of the phase) -- and the phase's stream waits for the last bucket before the call returns to the caller, whose next launch is uad_gan_adam with
 * grad_scale = 1 / world.  comm == NULL detaches.  AAE-family handles (aae_kind != 0): UAD_ERR_UNSUPPORTED -- the caller all-reduces the slice with
 * uad_rccl_allreduce as before. */
int uad_gan_allreduce_attach(uad_gan_t* g, void* comm, int world);
int uad_gan_reconstruct(uad_gan_t* g, const uad_gan_io_t* io, int n, void* stream);
/* dense GMVAE restoration (trainers/GMVAE.py:172-184): one `sess.run(grads)` + the host update, on device.  grads = d( n * loss +
 * sum_n tv_lambda * TV_n(x - xz_mu) ) / d x at the current x_restored (= io->x is ignored; tf.gradients sums the [n]-shaped `loss + restore`,
 * so every slice sees its own loss terms with weight 1); then x_restored -= restore_lr * grads in place.  grads_out may be NULL.
 * io supplies the noise / dropout masks of this run.  No parameter gradient is produced. */
int uad_gan_restore_step(uad_gan_t* g, float* x_restored, const uad_gan_io_t* io, int n, float tv_lambda, float restore_lr, float* grads_out,
                         void* stream);
/* HIP-event profiler of the k3 spatial kernels of the ResNet graph (csrc/uad_convk16.inc; process-wide, bench.py's roofline leg for BASELINE
 * configs[3]): while enabled every launch is bracketed by two events on its stream.  uad_k3_profile_read synchronises the device and writes one
 * text line per launch shape -- "kind p1 p2 ntaps planes N MH MW CA Nn calls total_ms" (kind 0: tap-list F / D kernel, p1 = input stride, p2 =
 * halo extent, MH x MW = iteration grid, CA -> Nn channels; kind 1: filter gradient, p1 = stride, MH x MW = small grid, CA = CB, Nn = CS) --
 * and returns the bytes the whole table needs. */
int uad_k3_profile_enable(int on);
int uad_k3_profile_read(char* buf, int cap);
/* tests: device pointer + element count of a named intermediate of the last phase (NULL name table entry -> error) */
int uad_gan_debug_buffer(uad_gan_t* g, const char* name, float** ptr, long long* count);

/* ---- single-kernel entry points (parity tests) ------------------------------------------------------------
 * geometry of one strided-conv relation: big pixel (S*i-P+ky, S*j-P+kx) <-> small pixel (i,j); weights W[tap][cb][cs]
 * (= HWIO for Conv2D with big=input, [kh,kw,Cout,Cin] for Conv2DTranspose with big=output). */
typedef struct { int N, HB, WB, CB, HS, WS, CS, KS, S, P; } uad_conv_desc_t;
/* activation-on-load v -> lrelu_alpha(scale[c]*v + shift[c]); scale == NULL = identity */
typedef struct { const float* scale; const float* shift; float alpha; } uad_xform_t;

int uad_op_conv_f(const uad_conv_desc_t* d, const float* big_in, const uad_xform_t* xf, const float* W,
                  const float* bias, const float* mul, const float* add, float* small_out, void* stream);
int uad_op_conv_d(const uad_conv_desc_t* d, const float* small_in, const uad_xform_t* xf, const float* W,
                  const float* bias, const float* mul, const float* add, float* big_out, void* stream);
/* data-gradient forms with the fused activation backward: out = acc*lrelu'(es*cprev+eh)*es; s1[c]=sum d_bn,
 * s2[c]=sum d_bn*cprev (synchronous: allocates scratch) */
int uad_op_conv_f_bwdact(const uad_conv_desc_t* d, const float* big_in, const float* W, const float* cprev,
                         const uad_xform_t* act, float* small_out, float* s1, float* s2, void* stream);
int uad_op_conv_d_bwdact(const uad_conv_desc_t* d, const float* small_in, const float* W, const float* cprev,
                         const uad_xform_t* act, float* big_out, float* s1, float* s2, void* stream);
int uad_op_conv_w(const uad_conv_desc_t* d, const float* big, const uad_xform_t* xfb, const float* small_,
                  const uad_xform_t* xfs, float* dW, void* stream);
/* Math mode of the op entry points: environment variable UAD_MATH, read per call.  Unset / "f32": exact fp32; "bf16x3": two bf16 planes; "bf16x6": a k5 s2
 * launch runs on the three-plane spatial kernels wherever the library's own decision functions take it (three planes packed here), and on the exact-fp32 route with
 * the fp32 pack everywhere else -- a refused three-plane route is a normal outcome, reported by uad_op_conv_plan, and never an abort.
 *
 * uad_op_conv_plan: host only, nothing is launched.  What the op entry point of `kind` ('F' | 'D' | 'W') would run for this descriptor in the current UAD_MATH.
 * epi: UAD_OP_EPI_* (F / D).  xf_flags: UAD_OP_XF_* (F / D: activation on load of the input; W: of big / of small; F: final backward on load).  out[12]:
 *   F / D: 0 .. 5 and 8 as uad_debug_plan (path, splits, slabs reduced in the kernel, column block, column-partial tiles, three-plane route 1 | 0 | -1, slab floats),
 *          6 D-kind kernel generation of a spatial launch (1 lane = pixel | 2 class-sequential conv5_d16 | 3 conv5_bf16<KIND_D> fallback | 4 exact-fp32 conv5_d_kernel;
 *          0: F kind or no spatial launch), 7 channel range per workgroup `cst` of generations 1 .. 3 (else 0), 9 1 when the entry point would answer
 *          UAD_ERR_UNSUPPORTED (a fused final the shape or mode has no kernel for, a final backward on load outside its instances), 10 math mode (0 f32 | 1 bf16x3 |
 *          3 bf16x6), 11 the fused final's tile: 16 (16 x 16 training instance) | 8 (8 x 16) | 0 (not a fused final);
 *   W:     0 .. 5, 7, 8 as uad_debug_plan, 10 math mode, the rest 0. */
enum { UAD_OP_EPI_BIAS = 0, UAD_OP_EPI_BWD_ACT = 1, UAD_OP_EPI_FINAL = 2, UAD_OP_EPI_FINAL_TRAIN = 3, UAD_OP_EPI_FINAL_DC = 4 };
enum { UAD_OP_XF_IN = 1, UAD_OP_XF_SMALL = 2, UAD_OP_XF_FINAL_BWD = 4 };
int uad_op_conv_plan(const uad_conv_desc_t* d, int kind, int epi, int xf_flags, long long* out);
/* One D-kind launch with the fused final epilogue (the last decoder block): c = ConvT(xf(small_in)) + bias, a = lrelu_alpha(bn.scale * c + bn.shift), x_hat = a . wf + bf[0],
 * l1 = |x_hat - x|.  x_hat [N,HB,WB] and rec_sum[1] = sum l1 are always written, l1 when non-null.  Forms: forward only (bits, dxhat, dc, red null); training, compressed
 * (bits [N,HB,WB] words with bit ch = (BN output of channel ch > 0), dxhat = sign(x_hat - x) * inv_batch, red[3 CB + 1] = {d wf, S1 = sum d bn, S2 = sum d bn * c, d bf} summed
 * over the tiles by the library's slab reduction; split-bf16 modes only); training, uncompressed (dc [N,HB,WB,CB] = d loss / d c, and red).  UAD_ERR_UNSUPPORTED where
 * uad_op_conv_plan reports out[9] = 1.  Synchronous. */
int uad_op_conv_d_final(const uad_conv_desc_t* d, const float* small_in, const uad_xform_t* xf, const float* W, const float* bias, const uad_xform_t* bn,
                        const float* wf, const float* bf, const float* x, float inv_batch, float* x_hat, float* l1, float* rec_sum,
                        unsigned* bits, float* dxhat, float* dc, float* red, void* stream);
/* uad_op_conv_f with final backward on load: the big operand is the compressed loss gradient of uad_op_conv_d_final (bits, dxhat) expanded while it is staged,
 * d loss / d c[pixel][ch] = dxhat[pixel] * wf[ch] * lrelu'(bit ch) * bn.scale[ch]; bias / mul / add as uad_op_conv_f.  Split-bf16 modes, CB <= 32. */
int uad_op_conv_f_final_bwd(const uad_conv_desc_t* d, const unsigned* bits, const float* dxhat, const float* wf, const uad_xform_t* bn, const float* W,
                            const float* bias, const float* mul, const float* add, float* small_out, void* stream);
int uad_op_conv_first_fwd(const uad_conv_desc_t* d, const float* x, const float* W, const float* bias, float* out,
                          void* stream);
int uad_op_conv_first_wgrad(const uad_conv_desc_t* d, const float* x, const float* g, float* dW, void* stream);
int uad_op_adam(float* p, const float* g, float* m, float* v, long long n, float lr_t, float beta1, float beta2,
                float eps, float gscale, void* stream);
/* A layer's parameter-gradient tail as the train step's side stream runs it.  Parts (one whose input pointer is null is left out):
 *   slabs[S][L] -> dW[L] (fixed-order sum);  colpart[T][2][C] -> dbeta = S1, dgamma = rstd S2, dbias = gamma rstd S1 (null outputs skipped);
 *   fin_partial[fin_T][3 fin_C + 1] = rows of {dwf[fin_C], S1[fin_C], S2[fin_C], dbf} -> dwf, dbf and fin_dbeta / fin_dgamma / fin_dbias as above.
 * fused = 1: one launch (C <= 512, fin_C <= 64); fused = 0: the separate launches (fin_red: 3 fin_C + 1 floats of scratch for them).  Both give the same bits.
 * scratch: uad_op_grad_finish_scratch_floats() floats, zero before the first call, reusable by later calls on the same stream.  Asynchronous on `stream`. */
typedef struct {
    const float* slabs; int S, L; float* dW;
    const float* colpart; int T, C; const float* gamma; float rstd; float *dgamma, *dbeta, *dbias;
    const float* fin_partial; int fin_T, fin_C; const float* fin_gamma; float *dwf, *dbf, *fin_dgamma, *fin_dbeta, *fin_dbias, *fin_red;
} uad_grad_finish_t;
long long uad_op_grad_finish_scratch_floats(void);
int uad_op_grad_finish(const uad_grad_finish_t* a, int fused, float* scratch, void* stream);

/* ---- the step's small kernels, ONE launch each on caller-supplied tensors (csrc/uad_loss.hip; the first-layer data gradient: csrc/uad_conv_first.hip;
 * uad_op_optim: csrc/uad_optim.hip; uad_op_colsum: csrc/uad_reduce.hip; uad_op_tv_dxhat: csrc/uad_gmvae.hip) ----
 * Each entry runs the launcher the engines run, asynchronously on `stream`, and allocates nothing.  Outside the kernel's domain (stated per entry) it
 * launches nothing and returns UAD_ERR_INVALID (a NULL pointer that is needed, a size below 1, a misaligned vector operand) or UAD_ERR_UNSUPPORTED (a
 * width or count no kernel form takes).
 *
 * uad_op_final: last 1x1 conv (C -> 1) + L1 loss on c_last [N,H,W,C] (pre-BN output of the last decoder block): a = lrelu_alpha(scale * mult * c + shift),
 *   x_hat = a . wf + bf[0], l1_map = |x_hat - x| (optional), rec_partial[N][B] = per-block sums of |x_hat - x|, B = uad_op_final_blocks(H, W).
 *   d_c == NULL: forward only.  Otherwise s = dxhat_in ? dxhat_in[pixel] : sign(x_hat - x) * inv_batch (sign(0) = 0), d_c = s wf lrelu'(bn) scale mult, and
 *   red_partial[N * B][3 C + 1] = per-block sums of {d wf = s a, S1 = d bn, S2 = d bn * c, d bf = s}.  Domain: C in {4, 8, 16, 32, 64} (C / 4 lanes of a
 *   wave share a pixel; 3 C + 2 partials fit the kernel's 200 LDS floats), N <= 65535, c_last / d_c / scale / shift / wf 16-byte aligned. */
typedef struct {
    int N, H, W, C;
    const float *c_last, *scale, *shift; float alpha, mult;
    const float *wf, *bf, *x;
    float *x_hat, *l1_map, *rec_partial;
    float *d_c, *red_partial; float inv_batch; const float* dxhat_in;
} uad_final_t;
int uad_op_final_blocks(int H, int W);
int uad_op_final(const uad_final_t* a, void* stream);
/* Reparameterisation and KL, one wave per sample, [n, zdim] tensors.  Samples [0, n_vae): m = mu_raw * mask_mu, l = ls_raw * mask_ls, sigma = exp(l),
 *   z = m + eps * sigma, kl[i] = 0.5 sum (m^2 + sigma^2 - 2 l - 1).  Samples [n_vae, n) (ceVAE context branch): m = mu_raw * mask_mu_ce[i - n_vae], z = m,
 *   ls = 0, sigma = 1, kl = 0.  Backward: dmu_raw = (dz + mu * inv_batch) * mask_mu, dls_raw = (dz * eps * sigma + (sigma^2 - 1) * inv_batch) * mask_ls;
 *   context samples: dmu_raw = dz * mask_mu_ce, dls_raw = 0.  Every mask and eps may be NULL (ones / zeros).  Domain: 0 <= n_vae <= n, zdim >= 1; ls_raw,
 *   mu and sigma may be NULL only when n_vae == 0. */
int uad_op_reparam_fwd(int n, int n_vae, int zdim, const float* mu_raw, const float* ls_raw, const float* mask_mu, const float* mask_ls,
                       const float* mask_mu_ce, const float* eps, float* mu, float* ls, float* sigma, float* z, float* kl, void* stream);
int uad_op_reparam_bwd(int n, int n_vae, int zdim, const float* dz, const float* mu, const float* sigma, const float* eps, const float* mask_mu,
                       const float* mask_ls, const float* mask_mu_ce, float inv_batch, float* dmu_raw, float* dls_raw, void* stream);
/* rec_per_sample[i] = sum_b rec_partial[i][b]; scalars[8] = {rec_scale (Rv + Rc), K, Rv + K + Rc, 0, Rv, Rc, Rv + K, 0} * inv_batch with Rv / Rc the sums over
 * samples [0, n_vae) / [n_vae, n) and K = sum kl[0 .. n_vae) (kl NULL: 0).  One workgroup. */
int uad_op_loss_finalize(const float* rec_partial, int n, int n_vae, int bps, const float* kl, float inv_batch, float rec_scale, float* rec_per_sample,
                         float* scalars, void* stream);
/* Data gradient of the first conv layer (CB = 1): acc[pixel] = sum g[n, i, j, :] . W[ky, kx, 0, :] over the small pixels whose window covers it.  Epilogues:
 *   plain       (x, dxhat NULL):  dx = acc;
 *   anomaly map (x, x_hat given): gx = acc + sign(x - x_hat) * inv_batch (sign(0) = 0), dx = gx, anomaly = |x - x_hat| |gx| (either may be NULL, not both);
 *   restoration (dxhat given):    gx = acc - dxhat, dx = gx (optional), x_upd -= restore_lr * gx in place (optional, not both NULL).
 * form 0: the launcher's choice; form 1: the one-thread-per-pixel kernel even where the tiled kernel takes the shape.  uad_op_conv_first_dgrad_form returns
 * the kernel that runs: 2 tiled (k5 s2 P 1, CS 32, HB = 2 HS and WB = 2 WS multiples of 16, N <= 65535), 1 generic (CS a multiple of 8, its KS KS CS
 * weights within 64 KiB of LDS), 0 neither (the entry then returns UAD_ERR_UNSUPPORTED). */
int uad_op_conv_first_dgrad_form(const uad_conv_desc_t* d, int form);
int uad_op_conv_first_dgrad(const uad_conv_desc_t* d, const float* g, const float* W, const float* x, const float* x_hat, float inv_batch, float* anomaly,
                            float* dx, const float* dxhat, float* x_upd, float restore_lr, int form, void* stream);
/* dxhat = -sign(r) * inv_batch - tv_lambda * dTV/dr at r = x - xh, TV = sum of |r - r_up| + |r - r_left| over [N,H,W] single-channel images; sign(0) = 0. */
int uad_op_tv_dxhat(const float* x, const float* xh, int N, int H, int W, float inv_batch, float tv_lambda, float* dxhat, void* stream);
/* TF-1.15 update rules on g * gscale.  kind 1: p -= lr g.  kind 2: s1 = momentum s1 + g, p -= lr s1.  kind 3: s2 = decay s2 + (1 - decay) g^2,
 * s1 = momentum s1 + lr g / sqrt(s2 + eps), p -= s1.  fault (optional device word): non-zero leaves p, s1 and s2 untouched. */
int uad_op_optim(int kind, float* p, const float* g, float* s1, float* s2, long long n, float lr, float momentum, float decay, float eps, float gscale,
                 const unsigned* fault, void* stream);
/* Spatial latent on [rows, C]: z = mask * lrelu_alpha(gamma * rs0 * c + beta); backward dc = dz * mask * lrelu' * gamma * rs0 and
 * colpart[B][2][C] = per-block column sums of {d bn, d bn * c}, B = uad_op_spatial_z_bwd_blocks(rows).  Domain: forward C a multiple of 4; backward C / 4 a
 * power of two <= 256 (its lanes tile a 256-thread workgroup); 16-byte aligned operands. */
int uad_op_spatial_z_fwd(const float* c, const float* gamma, const float* beta, float rs0, float alpha, const float* mask, int rows, int C, float* z,
                         void* stream);
int uad_op_spatial_z_bwd_blocks(int rows);
int uad_op_spatial_z_bwd(const float* dz, const float* c, const float* gamma, const float* beta, float rs0, float alpha, const float* mask, int rows, int C,
                         float* dc, float* colpart, void* stream);
/* out[c] = sum_r g[r][c].  scratch: uad_op_colsum_scratch_floats(rows, C) floats = row chunks x C; one chunk: a single launch writes out and scratch may
 * be NULL; more: per-chunk sums into scratch, then the library's slab sum. */
long long uad_op_colsum_scratch_floats(int rows, int C);
int uad_op_colsum(const float* g, int rows, int C, float* out, float* scratch, void* stream);

/* ---- the small kernels of the materialised-graph engine (csrc/uad_gan_kernels.inc; entries in csrc/uad_gan_ops.inc), ONE launch each on caller-supplied
 * tensors through the launch helper the uad_gan_* phases use.  Asynchronous on `stream`, nothing is allocated.  Outside the kernel's domain an entry launches
 * nothing and returns UAD_ERR_INVALID (a NULL tensor that is needed, an extent below 1, a misaligned float4 operand, an unknown kind / mode / rule) or
 * UAD_ERR_UNSUPPORTED (a width or count the kernel does not take).  Tensors are row-major [rows, C] unless stated; "float4 operand" = 16-byte aligned.
 *
 * Row-split kernels (bn_act_bwd, coef_colsum, gfinal_bwd): `rows` rows go to B = uad_op_gan_rows_blocks(rows, max_blocks) workgroups of ceil(rows /
 *   max_blocks) consecutive rows; max_blocks is one of the engine's rules 256 (coef_colsum), 512 (bn_act_bwd), 1024 (gfinal_bwd).  Each of the C / 4 channel
 *   quads gets 256 / (C / 4) row lanes: C / 4 must divide 256 and C <= 1024.
 * uad_op_gan_bn_act_fwd: a = lrelu_alpha(c * (gamma * rs0) + beta).  C a multiple of 4.
 * uad_op_gan_bn_act_bwd: dn = da * lrelu'(c * (gamma * rs0) + beta), dc = dn * (gamma * rs0), colpart[B][2][C] = per-workgroup column sums of {dn, dn * c}.
 *   C <= 256 in addition (one thread per channel writes the partials).
 * uad_op_gan_rowdot: out[row] = act(feat[row, :] . w + b[0]), act 0 none | 1 sigmoid | 2 tanh.  min(C / 4, 64) lanes per row, a power of two.
 * uad_op_gan_topgrad: out[row, :] = coef4[row / rows_per_group] * w.  rows <= 4 rows_per_group, C a multiple of 4.
 * uad_op_gan_coef_colsum: partial[B][C] = per-workgroup sums of coef4[row / rows_per_group] * feat[row, :].  rows <= 4 rows_per_group.
 * uad_op_gan_gfinal_bwd: dv = dx[row] * (act 0: x (1 - x) | 1: 1 - x^2 | 2: 1), da[row, :] = dv * wf; with partial: partial[B][C + 1] = per-workgroup sums of
 *   {dv * a[row, :], dv}, and then C <= 256. */
int uad_op_gan_rows_blocks(int rows, int max_blocks);
int uad_op_gan_bn_act_fwd(const float* c, const float* gamma, const float* beta, float rs0, float alpha, long long rows, int C, float* a, void* stream);
int uad_op_gan_bn_act_bwd(const float* da, const float* c, const float* gamma, const float* beta, float rs0, float alpha, int rows, int C, int max_blocks,
                          float* dc, float* colpart, void* stream);
int uad_op_gan_rowdot(int act, const float* feat, const float* w, const float* b, int rows, int C, float* out, void* stream);
int uad_op_gan_topgrad(const float* w, long long rows, int rows_per_group, int C, const float* coef4, float* out, void* stream);
int uad_op_gan_coef_colsum(const float* feat, int rows, int rows_per_group, int C, const float* coef4, int max_blocks, float* partial, void* stream);
int uad_op_gan_gfinal_bwd(const float* dx, const float* x, const float* a, const float* wf, int rows, int C, int act, int max_blocks, float* da,
                          float* partial, void* stream);
/* din [3][n, HW] = {xg, x, x + alpha[sample] * (xg - x)}. */
int uad_op_gan_interp(const float* xg, const float* x, const float* alpha, int n, int HW, float* din, void* stream);
/* Elementwise kernels over n floats.  TANH: out = tanh(a).  TANH_BWD: out = a * (1 - b^2) * (c ? c : 1)  (a = dz, b = z, c = optional mask).
 * DIFF_SCALE: out = coef * (a - b); _ACC: out += coef * (a - b).  SIGN_SCALE: out = coef * sign(a - b), sign(0) = 0.  ADD: out += a.  ADD_SCALAR: out += b[0].
 * LRELU_FWD: out = a > 0 ? a : coef * a.  LRELU_BWD: out = b > 0 ? a : coef * a  (a = d / d activation, b = pre-activation); both: n a multiple of 4,
 * float4 operands. */
enum { UAD_GAN_FLAT_TANH = 0, UAD_GAN_FLAT_TANH_BWD = 1, UAD_GAN_FLAT_DIFF_SCALE = 2, UAD_GAN_FLAT_DIFF_SCALE_ACC = 3, UAD_GAN_FLAT_SIGN_SCALE = 4,
       UAD_GAN_FLAT_ADD = 5, UAD_GAN_FLAT_ADD_SCALAR = 6, UAD_GAN_FLAT_LRELU_FWD = 7, UAD_GAN_FLAT_LRELU_BWD = 8 };
int uad_op_gan_flat(int kind, const float* a, const float* b, const float* c, float coef, long long n, float* out, void* stream);
/* partial[uad_op_gan_sum_blocks()] = per-workgroup sums (fixed grid, grid-stride) of mode 0: a | 1: (a - b)^2 | 2: |a - b|, mode 2 also writing map = |a - b|
 * when map is given. */
int uad_op_gan_sum_blocks(void);
int uad_op_gan_sum(int mode, const float* a, const float* b, long long n, float* map, float* partial, void* stream);
/* WGAN-GP slope penalty on g [n, H, W]: s[n, W] = sqrt(sum_h g^2), partial[uad_op_gan_pen_col_blocks(n, W)] = per-workgroup sums of (s - 1)^2;
 * uad_op_gan_pen_grad: out = coef * (s - 1) / s * g. */
int uad_op_gan_pen_col_blocks(int n, int W);
int uad_op_gan_pen_col(const float* g, int n, int H, int W, float* s, float* partial, void* stream);
int uad_op_gan_pen_grad(const float* g, const float* s, float coef, int n, int H, int W, float* out, void* stream);
/* NHWC square maps, C a multiple of 4, float4 operands.  AVG_FWD: in [N,H,H,C] -> out [N,H/2,H/2,C], 0.25 ((a + b) + (c + d)); AVG_BWD: in [N,H/2,H/2,C] ->
 * out [N,H,H,C] = 0.25 in; both need an even H.  UP2_FWD: in [N,H,H,C] -> out [N,2H,2H,C] nearest neighbour; UP2_BWD: in [N,2H,2H,C] -> out [N,H,H,C],
 * (a + b) + (c + d). */
enum { UAD_GAN_POOL_AVG_FWD = 0, UAD_GAN_POOL_AVG_BWD = 1, UAD_GAN_POOL_UP2_FWD = 2, UAD_GAN_POOL_UP2_BWD = 3 };
int uad_op_gan_pool(int kind, const float* in, int N, int H, int C, float* out, void* stream);
/* out[(T - 1 - t) * C + c] = w[t * C + c]; out must not alias w. */
int uad_op_gan_flip_taps(const float* w, int T, int C, float* out, void* stream);
/* the derived UAD_GAN_S_* scalars of a phase from its raw means (combine_kernel); phase 0 .. 7, out [16]; scalars the phase does not define are not written. */
int uad_op_gan_combine(int phase, const float* raw, float kappa, float* out, void* stream);
/* Latent critic zd -> h1 -> h2 -> 1 (leaky_relu 0.2), one workgroup per sample.  mode 0 (critic step): d_fake, d_real, pen [n] and slab [n][zd h1 + h1 +
 * h1 h2 + h2 + h2 + 1] = the sample's gradient of d_fake / n - d_real / n + pen; mode 1 (generator step): d_fake and dz_fake [n, zd] = -inv_n d d_fake / d zf,
 * nothing else is written.  hat_mode 0: z_hat = zr + eps (zr - zf); 1: z_hat = zf + eps (zr - zf).  Domain: zd <= 512, h1, h2 <= 400 (LDS arrays). */
typedef struct {
    int zd, h1, h2, mode, hat_mode;
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    const float *zf, *zr, *eps;
    float inv_n, scale;
    float *d_fake, *d_real, *pen, *slab, *dz_fake;
} uad_gan_critic_t;
int uad_op_gan_critic(const uad_gan_critic_t* c, int n, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* UAD_HIP_H */
