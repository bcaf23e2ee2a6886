/*
 * cad.h — C ABI of libcad_hip.so, the MI355X (gfx950) implementation of the camera-aware depth
 * training step of RyoK3N/Camera-Aware-Neural-Networks-for-Few-View-Depth-Estimation.
 *
 * Boundary.  Each entry point replaces one reference interface on the hot path
 * (paths relative to the reference checkout):
 *   cad_unet_create / destroy       BaselineUNetImpl(in_channels, init_features, max_depth)
 *                                   src/models/baseline_unet.h:144-166 (+ TORCH_MODULE holder :208)
 *   cad_unet_count_parameters       BaselineUNetImpl::count_parameters        baseline_unet.h:200-206
 *   cad_unet_tensor_info/get/set    torch::nn::Module::named_parameters()/named_buffers() order and
 *                                   shapes (registration order, baseline_unet.h:20-30,53-56,79-81,
 *                                   147-165); used by torch::save / load and the trainer
 *   cad_unet_train                  Module::train()/eval()  (enhanced.h:259, :341)
 *   cad_unet_forward                BaselineUNetImpl::forward                 baseline_unet.h:174-195
 *   cad_unet_create_model           IntrinsicsConditionedUNetImpl(in, f, 4, max_depth)
 *                                   src/models/intrinsics_unet.h:137-200 (FiLMLayerImpl(4, C) per
 *                                   DoubleConv, src/layers/film_layer.h:47-72); CAD_MODEL_RAY_FILM =
 *                                   the config-3 composite with enc1 = RayEnhancedConv(3, f, 4, true)
 *                                   (src/models/geometry_aware_network.h:17-65)
 *   cad_unet_forward_cam            IntrinsicsConditionedUNetImpl::forward(x, intrinsics (B,4))
 *                                   intrinsics_unet.h:204-228 (+ RayEnhancedConvImpl::forward's
 *                                   cat(x, rays), geometry_aware_network.h:47-52)
 *   cad_camera_from_K               K (B,3,3) -> (B,4) [fx, fy, cx, cy] (the reference
 *                                   has no such code; train_main never builds camera vectors)
 *   cad_loss_create/forward_backward CombinedDepthLoss(si,grad,smooth,reproj) + forwardWithIntrinsics
 *                                   + the autograd backward of the loss       src/loss/depth_loss.h:366-433
 *   cad_loss_get_components         getComponentsWithIntrinsics               depth_loss.h:454-467
 *   cad_unet_backward[_stage]       loss.backward() through the U-Net         enhanced.h:297
 *   cad_clip_grad_norm              torch::nn::utils::clip_grad_norm_         enhanced.h:300-302
 *   cad_adam_create/step            torch::optim::Adam(AdamOptions(lr).weight_decay(wd)) / step()
 *                                   enhanced.h:97-101, :304
 *   cad_optim_create/step           Trainer::createOptimizer: torch::optim::Adam / AdamW / SGD by
 *   cad_geonet_optim_step           TrainingConfig::optimizer      src/training/trainer.h:388-414, step :348
 *   cad_optim_set_lr / cad_lr_at    createScheduler (StepLR / CosineAnnealingLR) and the epoch loop's warmup
 *                                   and scheduler.step()           trainer.h:416-431, :262-308
 *   cad_optim_attach_ema/ema_swap   exponential moving average of the weights (new: no reference counterpart)
 *   cad_unet_flat                   flat gradient slab for the data-parallel RCCL all-reduce (new:
 *                                   the reference is single-device)
 *   cad_comm_* / cad_grad_allreduce / cad_unet_backward_allreduce
 *                                   data-parallel replicas over RCCL (new; SURVEY.md §8(b) proposal
 *                                   cad_grad_allreduce, §8(e) semantics; hardware.num_gpus /
 *                                   distributed keys of configs/train_config.yaml:178-183, which the
 *                                   reference parses but never uses)
 *   cad_loss_forward_backward_masked forwardWithIntrinsics(pred, gt, image, K, valid_mask)
 *                                   depth_loss.h:416-433 with the optional mask
 *   cad_depth_metrics               computeDepthMetrics (abs_rel ...)          enhanced.h:400-439
 *   cad_evaluator_create/destroy/reset/update/count/sums/metrics, cad_eval_finish
 *                                   DepthMetrics::compute / computePerSample / average
 *                                   src/evaluation/depth_metrics.h:40-141 (validity mask :147-164,
 *                                   the metric formulas :169-233, getZeroMetrics :238-253) and the
 *                                   mean / std / median of Evaluator::computeStatistics,
 *                                   src/evaluation/evaluator.h:385-397, on a device-resident table of
 *                                   per-sample sums (the reference's evaluation target does not build;
 *                                   its metric definitions are the contract)
 *   cad_evaluator_set_strata/update_k/strata_bins/strata_sums, cad_eval_strata_finish
 *                                   the same sums per depth-range and ray-angle stratum (no reference
 *                                   counterpart)
 *   cad_evaluator_set_alignment/get_alignment/alignment/aligned, cad_valid_medians,
 *   cad_eval_solve_alignment        per-sample median / log-mean / least-squares alignment of the
 *                                   prediction before the metrics (new: no reference counterpart; the
 *                                   reference scores raw predictions only)
 *   cad_ray_directions              RayDirectionComputer::computeRayDirections
 *                                   src/preprocessing/ray_direction_computer.cpp:17-62
 *   cad_batcher_create/assemble     SunRGBDLoader::getSample's resizeSample + augmentSample
 *                                   (src/data/sunrgbd_loader.cpp:158-166, 352-489) and the trainer's
 *                                   batch torch::stack + .to(device) (enhanced.h:277-289), on device
 *   cad_aug_sampler_create/draw     augmentSample's random draws (sunrgbd_loader.cpp:352-443;
 *                                   AugmentationConfig sunrgbd_loader.h:30-42, rng_ seed :185)
 *   cad_color_matrix                the declared saturation / hue / gamma stages (new: the reference parses
 *                                   data.augmentation saturation, hue, random_gamma and applies none of
 *                                   them; off unless a cad_sample / cad_aug_config asks: "batch assembly")
 *   cad_exporter_* / cad_colormap_lut / cad_png_encode / cad_png_decode / cad_ply_write / cad_hflip /
 *   cad_flip_mean                   DepthVisualizer (src/visualization/depth_viz.h:23-148,
 *                                   depth_visualizer.h) on the device, 16-bit depth PNGs, point clouds
 *                                   and flip test-time augmentation ("inference export" below)
 *   cad_op_*                        single operators of the step (conv, convT, BN, pool, ...), the
 *                                   ATen calls the reference dispatches
 *
 * Conventions: all tensor pointers are DEVICE pointers owned by the caller unless a handle owns
 * them; tensors crossing the boundary use the reference's NCHW fp32 layout (rgb (B,3,H,W), depth
 * (B,1,H,W), K (B,3,3) row-major).  Every call that launches work takes an explicit stream
 * (a hipStream_t passed as void*; NULL = default stream) and is asynchronous unless documented.
 * Status codes replace exceptions; cad_last_error() returns the thread-local message of the last
 * failing call.  Handles are not thread-safe: one handle per device per host thread.
 */
#ifndef CAD_CAD_H
#define CAD_CAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAD_ABI_VERSION 1

typedef enum {
    CAD_OK = 0,
    CAD_ERR_INVALID = 1, /* bad argument / shape */
    CAD_ERR_HIP = 2,     /* HIP runtime error */
    CAD_ERR_OOM = 3,     /* device allocation failed */
    CAD_ERR_STATE = 4    /* call out of order (e.g. backward before a train-mode forward) */
} cad_status;

typedef struct cad_unet cad_unet;
typedef struct cad_loss cad_loss;
typedef struct cad_adam cad_adam;

/* model families (cad_unet_create_model) */
#define CAD_MODEL_BASELINE 0        /* BaselineUNetImpl */
#define CAD_MODEL_INTRINSICS_FILM 1 /* IntrinsicsConditionedUNetImpl (camera_dim 4) */
#define CAD_MODEL_RAY_FILM 2        /* enc1 = RayEnhancedConv(3, f, 4, use_rays), FiLM blocks after */
/* IntrinsicsAttentionUNetImpl (intrinsics_unet.h:278-385): INTRINSICS_FILM with a CBAM (att4 .. att1,
 * spatial_attention.h:142-191) after every decoder block.  named_parameters() keeps the reference's
 * registration order (att4.* .. att1.* between dec1.* and out_conv.*); in the flat slab att<k> follows
 * dec<k>, so each backward stage's gradient range stays contiguous (stage k = dec<k> + att<k>) */
#define CAD_MODEL_INTRINSICS_ATTN 3

typedef struct {
    int in_channels;   /* 3 */
    int init_features; /* f (64 default, 96 in train_config_production.yaml) */
    float max_depth;   /* 10.0 */
    int max_batch;     /* activation workspace is sized for this batch */
    int height;        /* H, W: must be divisible by 16 (the reference's pad branch is then a no-op) */
    int width;
} cad_unet_desc;

typedef struct {
    float lr;           /* optimization.learning_rate (1e-4) */
    float beta1, beta2; /* 0.9, 0.999 */
    float eps;          /* 1e-8 */
    float weight_decay; /* coupled L2 (torch::optim::Adam), 1e-5 */
} cad_adam_opts;

/* ---- library ---- */
int cad_abi_version(void);
/* GEMM engine of the conv3x3 / ConvTranspose contractions (forward, dgrad, wgrad):
 * CAD_GEMM_F32 = v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chains); CAD_GEMM_S3 = fp32 operands split
 * exactly into three bf16 terms on the bf16 matrix cores, six products accumulated in fp32 (error
 * < 2^-23 |a b| per product: fp32 accuracy); CAD_GEMM_BF16 = operands rounded to bf16 (nearest
 * even), one product, fp32 accumulation — the bf16 arithmetic of BASELINE configs 3-5 (activations,
 * BatchNorm, loss and optimizer stay fp32).  Process-wide, default CAD_GEMM_S3; the env var
 * CAD_GEMM=f32|s3|bf16 sets the initial value. */
#define CAD_GEMM_F32 0
#define CAD_GEMM_S3 1
#define CAD_GEMM_BF16 2
cad_status cad_set_gemm_engine(int engine);
int cad_get_gemm_engine(void);
const char* cad_last_error(void);
/* Launch-level aliasing guard (csrc/host/alias.cpp): with mode 1 every instrumented launcher (the conv /
 * ConvT / dense GEMMs on every engine, the MX-fp8 GEMMs and quantiser, the BN / residual / pool / twin
 * passes) refuses a launch whose output byte range overlaps one of its inputs — CAD_ERR_INVALID, the
 * operands named in cad_last_error() — unless that pair is declared in place.  Default: the environment
 * (CAD_ALIAS_CHECK=1; tests/conftest.py sets it), else off.  Returns the previous mode. */
int cad_set_alias_check(int mode);
/* The guard's overlap rule on two row views (rows of ld elements of es bytes, columns [coff, coff+cols)):
 * 1 when they share a byte.  Host arithmetic only (no device). */
int cad_alias_views_overlap(const void* a, int64_t arows, int64_t ald, int64_t acoff, int64_t acols, int aes,
                            const void* b, int64_t brows, int64_t bld, int64_t bcoff, int64_t bcols, int bes);
cad_status cad_device_count(int* n);
cad_status cad_set_device(int device);
cad_status cad_stream_synchronize(void* stream);
/* timing events for callers without HIP headers (the C++ evaluator's forward time): record on a stream;
 * elapsed_ms waits for `stop` and returns the time between the two records */
typedef struct cad_event cad_event;
cad_status cad_event_create(cad_event** out);
void cad_event_destroy(cad_event* ev);
cad_status cad_event_record(cad_event* ev, void* stream);
cad_status cad_event_elapsed_ms(cad_event* start, cad_event* stop, float* ms);
/* device memory for callers without HIP headers (the C++ drop-in, the train CLI) */
cad_status cad_malloc(int device, int64_t bytes, void** out);
void cad_free(void* p);
/* kind: 0 host->device, 1 device->host, 2 device->device; synchronous when stream is NULL */
cad_status cad_memcpy(void* dst, const void* src, int64_t bytes, int kind, void* stream);

/* ---- model: BaselineUNetImpl ---- */
cad_status cad_unet_create(const cad_unet_desc* desc, int device, cad_unet** out); /* baseline */
cad_status cad_unet_create_model(const cad_unet_desc* desc, int model, int device, cad_unet** out);
int cad_unet_model(const cad_unet* h);
void cad_unet_destroy(cad_unet* h);
int64_t cad_unet_count_parameters(const cad_unet* h);
int cad_unet_num_params(const cad_unet* h);  /* tensors in named_parameters() */
int cad_unet_num_buffers(const cad_unet* h); /* float tensors in named_buffers() */
/* kind: 0 = parameter, 1 = buffer.  shape has up to 4 entries (reference layout). */
cad_status cad_unet_tensor_info(const cad_unet* h, int kind, int idx, const char** name, int* ndim,
                                int64_t shape[4]);
/* host <-> device copies in the REFERENCE layout (OIHW conv, (Cin,Cout,2,2) convT); synchronous */
cad_status cad_unet_set_tensor(cad_unet* h, int kind, int idx, const float* host, int64_t numel);
cad_status cad_unet_get_tensor(const cad_unet* h, int kind, int idx, float* host, int64_t numel);
cad_status cad_unet_get_grad(const cad_unet* h, int idx, float* host, int64_t numel);
cad_status cad_unet_train(cad_unet* h, int train); /* 1 = train(), 0 = eval() */
/* Fused eval forward (off by default): with on != 0 every eval-mode forward applies each block's
 * BatchNorm + ReLU (+ FiLM) in its 3 x 3 convolutions' GEMM epilogues instead of a second pass over the pre-BN
 * output, which is then never written ("enc<l>.y1|y2" debug buffers go stale).  Train-mode forwards ignore the
 * switch.  fp32 engines: the same bits as the two-pass forward; bf16 engine: the activation is rounded to bf16
 * once instead of twice.  The convolution feeding a fused level-0 head stays two-pass.
 * cad_unet_fused_eval_convs: of the last forward's `total` 3 x 3 convolutions, `fused` ran the fused epilogue
 * (either pointer may be NULL).  The ResNet-50 and geometry-aware handles have no such switch. */
cad_status cad_unet_set_fused_eval(cad_unet* h, int on);
int cad_unet_get_fused_eval(const cad_unet* h); /* 0 for a NULL handle */
cad_status cad_unet_fused_eval_convs(const cad_unet* h, int* fused, int* total);
/* flat parameter / gradient slabs (internal packed layout; n = elements incl. alignment padding) */
cad_status cad_unet_flat(cad_unet* h, float** params, float** grads, int64_t* n);
/* switch the flat slabs to caller-owned device memory of cad_unet_flat()'s n floats each (e.g.
 * buffers a collective library registers); current parameter values are copied over.  The caller
 * keeps them alive for the handle's lifetime. */
cad_status cad_unet_use_external_slabs(cad_unet* h, float* params, float* grads);

/* forward: rgb (B,3,H,W) -> depth (B,1,H,W) in (0, max_depth).  B <= max_batch.
 * cad_unet_forward serves CAD_MODEL_BASELINE; the camera-conditioned models take cam4 (B,4)
 * [fx, fy, cx, cy] in pixels of the H x W input (normalised on device, intrinsics_unet.h:252-268;
 * RAY_FILM also derives the per-pixel rays from it).  Note FiLM's BatchNorm1d runs only for B > 1
 * (film_layer.h:85,91), in train and eval mode alike. */
cad_status cad_unet_forward(cad_unet* h, const float* rgb, float* depth, int B, void* stream);
cad_status cad_unet_forward_cam(cad_unet* h, const float* rgb, const float* cam4, float* depth, int B,
                                void* stream);
/* K (B,3,3) row-major -> cam4 (B,4) = [K00, K11, K02, K12] */
cad_status cad_camera_from_K(const float* K, int B, float* cam4, void* stream);

/* backward of the last train-mode forward given dL/ddepth; writes every parameter gradient.
 * Stage form (stage 0 .. cad_unet_num_stages()-1, in order) lets a caller overlap the gradient
 * all-reduce of finished stages with the rest of the backward. */
cad_status cad_unet_backward(cad_unet* h, const float* ddepth, void* stream);
int cad_unet_num_stages(const cad_unet* h);
cad_status cad_unet_backward_stage(cad_unet* h, int stage, const float* ddepth, void* stream);
/* [offset, offset+count) of the flat gradient slab completed by `stage` */
cad_status cad_unet_stage_grad_range(const cad_unet* h, int stage, int64_t* offset, int64_t* count);

/* clip_grad_norm_: total = ||prescale * g||_2; g *= prescale * min(1, max_norm / (total + 1e-6))
 * (the scaling is applied inside cad_adam_step; prescale = 1/world after a SUM all-reduce).
 * The total norm stays on device; cad_unet_last_grad_norm() fetches it (synchronises). */
cad_status cad_clip_grad_norm(cad_unet* h, float max_norm, float prescale, void* stream);
cad_status cad_unet_last_grad_norm(cad_unet* h, float* total_norm, void* stream);

/* ---- optimizer: torch::optim::Adam (coupled L2) over the model's flat slab ---- */
cad_status cad_adam_create(cad_unet* model, const cad_adam_opts* opts, cad_adam** out);
void cad_adam_destroy(cad_adam* a);
cad_status cad_adam_step(cad_adam* a, void* stream); /* consumes the clip coefficient */
cad_status cad_adam_set_lr(cad_adam* a, float lr);
int64_t cad_adam_step_count(const cad_adam* a);
/* optimizer state for checkpoint / resume: device pointers to the m and v slabs (cad_unet_flat's n
 * floats each, same packed layout as the parameters) and the step counter */
cad_status cad_adam_state(cad_adam* a, float** m, float** v);
cad_status cad_adam_set_step_count(cad_adam* a, int64_t step);

/* ---- the declared training recipe (trainer.h:24-92, :388-431): Adam / AdamW / SGD over the model's flat
 * slab in one pass, an optional exponential moving average of the weights fused into it (ours: the
 * reference has none), and the per-epoch learning-rate schedule.  cad_adam_* above is unchanged;
 * CAD_OPTIM_ADAM without an EMA gives its bits. ----
 *   CAD_OPTIM_ADAM   torch::optim::Adam, coupled L2 (g += wd p)
 *   CAD_OPTIM_ADAMW  torch::optim::AdamW: p *= 1 - lr wd, then Adam on the bare gradient (decay uniform over
 *                    the slab, as AdamW over parameters(); zero padding stays zero)
 *   CAD_OPTIM_SGD    torch::optim::SGD(lr).momentum(mu).weight_decay(wd): g += wd p; buf = mu buf + g (zero-
 *                    initialised: the first step gives buf = g; dampening 0, no Nesterov); p -= lr buf.
 *                    buf lives in the m slab; there is no v slab. */
#define CAD_OPTIM_ADAM 0
#define CAD_OPTIM_ADAMW 1
#define CAD_OPTIM_SGD 2
typedef struct {
    int rule;           /* CAD_OPTIM_* */
    float lr;
    float beta1, beta2; /* Adam / AdamW */
    float eps;
    float weight_decay;
    float momentum;     /* SGD */
    float ema_decay;    /* d in [0, 1): ema = d ema + (1 - d) p after every step; 0 = no EMA slab */
} cad_optim_opts;
typedef struct cad_optim cad_optim;
cad_status cad_optim_create(cad_unet* model, const cad_optim_opts* opts, cad_optim** out);
void cad_optim_destroy(cad_optim* o);
cad_status cad_optim_step(cad_optim* o, void* stream); /* consumes the clip coefficient, as cad_adam_step */
cad_status cad_optim_set_lr(cad_optim* o, float lr);
float cad_optim_lr(const cad_optim* o);
int cad_optim_rule(const cad_optim* o);
int64_t cad_optim_step_count(const cad_optim* o);
cad_status cad_optim_set_step_count(cad_optim* o, int64_t step);
/* device pointers to the state slabs (cad_unet_flat's n floats each): m (SGD: the momentum buffer), v (null
 * for SGD) and ema (null without one) */
cad_status cad_optim_state(cad_optim* o, float** m, float** v, float** ema);
/* (re)start the average: allocates the slab on first use and copies the current parameters into it */
cad_status cad_optim_attach_ema(cad_optim* o, float decay, void* stream);
/* exchange the contents of the parameter and EMA slabs in place.  Validation, panels and checkpoints of the
 * averaged model run between two swaps; two swaps restore both slabs bit for bit.  The U-Net rebuilds its
 * prepared weights at every forward, so nothing else needs invalidating.  cad_optim_step while swapped is
 * CAD_ERR_INVALID. */
cad_status cad_optim_ema_swap(cad_optim* o, void* stream);
int cad_optim_swapped(const cad_optim* o);

/* The learning rate of 0-based epoch `epoch0` out of `num_epochs` (host only, pure).  W = warmup_epochs,
 * t = epoch0 - W, computed in double and rounded to float:
 *   epoch0 < W: lr (epoch0 + 1) / W;  "none": lr;  "step": lr gamma^floor(t / step_size);
 *   "cosine": lr_min + (lr - lr_min) (1 + cos(pi t / max(1, num_epochs - W))) / 2.
 * These equal the reference's loop (trainer.h:262-308: the warmup rate set directly, scheduler.step() after
 * each epoch >= W) over StepLR / CosineAnnealingLR(T_max = num_epochs - W, eta_min = lr_min).  "plateau" and
 * unknown names: CAD_ERR_INVALID, the value named in cad_last_error(). */
typedef struct {
    float lr;
    const char* scheduler; /* "none" | "step" | "cosine" (NULL = "none") */
    int step_size;
    float gamma;
    int warmup_epochs;
    float lr_min;
} cad_lr_opts;
cad_status cad_lr_at(const cad_lr_opts* opts, int epoch0, int num_epochs, float* lr);

/* ---- checkpoints in the reference's format: torch::save(model_, path) / torch::load(model, path)
 * (tensorboard_trainer_enhanced.h:656-662; production_trainer.h:323-330 writes final_model.pt).
 * cad_unet_save_torch writes the TorchScript zip archive LibTorch's OutputArchive produces for the
 * module (every parameter and buffer under its named_parameters()/named_buffers() name, BatchNorm
 * num_batches_tracked included, parameterless submodules such as the encoders' MaxPool2d kept), so
 * torch::load of the reference model reads it; cad_unet_load_torch reads such an archive (from the
 * reference or from us) into the model: every model tensor must be present with its shape (extra
 * archive entries are ignored, as torch::load ignores them).  Synchronous. */
cad_status cad_unet_save_torch(cad_unet* h, const char* path);
cad_status cad_unet_load_torch(cad_unet* h, const char* path);
/* BatchNorm num_batches_tracked: train-mode forwards since creation (or the loaded value) */
int64_t cad_unet_num_batches_tracked(const cad_unet* h);

/* host-only archive I/O underneath (no device needed).  Entries are written in the order given:
 * a module's parameters (kind 0), then its buffers (kind 1), then its children in first-appearance
 * order; kind 2 declares a parameterless submodule (e.g. "enc2.pool") at its registration position. */
#define CAD_DTYPE_F32 0
#define CAD_DTYPE_I64 1
#define CAD_DTYPE_F64 2
#define CAD_DTYPE_F16 3
#define CAD_DTYPE_BF16 4
#define CAD_DTYPE_I32 5
typedef struct {
    const char* name;  /* dotted path, e.g. "enc1.bn1.running_mean" */
    int kind;          /* 0 parameter, 1 buffer, 2 empty submodule */
    int dtype;         /* CAD_DTYPE_* */
    int ndim;          /* 0..8 (0 = scalar) */
    int64_t shape[8];
    const void* data;  /* contiguous host data */
} cad_archive_entry;
cad_status cad_archive_write(const char* path, const cad_archive_entry* entries, int n);
/* reader: a data-only pickle interpreter (nothing named in the file is executed) over torch::save
 * module archives and Python torch.save state dicts; tensors are listed under dotted names */
typedef struct cad_archive cad_archive;
cad_status cad_archive_open(const char* path, cad_archive** out);
void cad_archive_close(cad_archive* a);
int cad_archive_count(const cad_archive* a);
int cad_archive_find(const cad_archive* a, const char* name); /* -1 if absent */
cad_status cad_archive_info(const cad_archive* a, int i, const char** name, int* dtype, int* ndim, int64_t shape[8]);
cad_status cad_archive_read(const cad_archive* a, int i, void* dst, int64_t bytes); /* raw, in its dtype */

/* ---- data-parallel gradient exchange: RCCL over xGMI, one process per GPU (new: the reference is
 * single-device).  Semantics: every replica runs the same step on
 * its own shard of the global batch (BN statistics and loss masks per replica); the gradient slab is
 * SUM-all-reduced and the 1/world mean folded into cad_clip_grad_norm(.., prescale = 1/world);
 * clip and Adam are then identical on every replica. ---- */
typedef struct cad_comm cad_comm;
#define CAD_COMM_ID_BYTES 128
#define CAD_REDUCE_SUM 0
#define CAD_REDUCE_MAX 1
/* rank 0 draws the communicator id (ncclGetUniqueId) and hands its bytes to every rank */
cad_status cad_comm_get_unique_id(uint8_t id[CAD_COMM_ID_BYTES]);
/* collective: every rank of the job calls it with the same id (ncclCommInitRank) */
cad_status cad_comm_create(const uint8_t id[CAD_COMM_ID_BYTES], int nranks, int rank, int device, cad_comm** out);
void cad_comm_destroy(cad_comm* c);
int cad_comm_rank(const cad_comm* c);
int cad_comm_size(const cad_comm* c);
/* in-place fp32 all-reduce / broadcast on `stream` (e.g. loss and metric scalars, initial weights) */
cad_status cad_comm_allreduce(cad_comm* c, float* buf, int64_t count, int op, void* stream);
cad_status cad_comm_broadcast(cad_comm* c, float* buf, int64_t count, int root, void* stream);
/* the flat parameter slab of `h` from rank `root` (identical replicas at start / after a resume) */
cad_status cad_comm_broadcast_params(cad_unet* h, cad_comm* c, int root, void* stream);
/* SUM all-reduce of the whole gradient slab after a backward (no overlap; SURVEY §8(b)'s proposal) */
cad_status cad_grad_allreduce(cad_unet* h, cad_comm* c, void* stream);
/* loss.backward() with the exchange overlapped: every backward stage is enqueued on `stream`; as soon
 * as the stages of a bucket (>= bucket_elems floats, decoder first, cad_plan_grad_buckets) are
 * enqueued, its SUM all-reduce is issued on the communicator's stream behind an event, so RCCL runs
 * while the remaining dgrad/wgrad kernels do; `stream` finally waits for every all-reduce. */
cad_status cad_unet_backward_allreduce(cad_unet* h, cad_comm* c, const float* ddepth, int64_t bucket_elems,
                                       void* stream);
/* Exchange accounting of the *_backward_allreduce calls (new; no reference counterpart).  With timing
 * on, each call records HIP timing events: on the compute stream after its last backward kernel and
 * again once that stream has waited for the last all-reduce (the difference is the exposed, i.e.
 * non-overlapped, exchange time), and on the communicator's stream around its all-reduces (the span
 * from the first bucket's start to the last bucket's end).  cad_comm_stats waits for the recorded
 * events, returns the sums since the last read (or since timing was enabled) and resets them.  At most
 * 256 calls are timed between reads (later ones are counted in `calls`/`bytes` only). */
typedef struct cad_comm_stats {
    int64_t calls;          /* backward_allreduce calls */
    int64_t timed_calls;    /* calls whose events were recorded */
    int64_t buckets;        /* all-reduces issued */
    int64_t bytes;          /* bytes all-reduced (fp32 SUM, in place) */
    double exposed_ms;      /* sum over timed calls: last backward kernel -> compute stream released */
    double span_ms;         /* sum over timed calls: first all-reduce start -> last all-reduce end */
} cad_comm_stats;
cad_status cad_comm_set_timing(cad_comm* c, int enable);
cad_status cad_comm_stats_read(cad_comm* c, cad_comm_stats* out);
/* the bucket plan (host only): consecutive backward stages [stage_off, +stage_cnt) grouped greedily
 * into contiguous buckets of >= bucket_elems floats (the last takes the rest).  Writes up to nstages
 * buckets (nullable outputs); returns the bucket count, or -1 on bad input. */
int cad_plan_grad_buckets(const int64_t* stage_off, const int64_t* stage_cnt, int nstages, int64_t bucket_elems,
                          int64_t* bucket_off, int64_t* bucket_cnt, int* bucket_last_stage);
/* host only (no device): the flat gradient slab layout of a model family — backward stage count (at
 * most 16) and each stage's [offset, offset+count) — as cad_unet_stage_grad_range reports it */
cad_status cad_model_grad_layout(int model, int in_channels, int init_features, int* nstages, int64_t stage_off[16],
                                 int64_t stage_cnt[16], int64_t* n_flat);

/* ---- loss: CombinedDepthLoss ----
 * height and width must be at least 16 (CAD_ERR_INVALID otherwise, the message names the value): below
 * that the coarsest gradient-matching scale (avg_pool2d k = 8) has no horizontal or vertical difference
 * and the loss is 0/0.  One handle serves every batch 1..max_batch. */
cad_status cad_loss_create(float si_weight, float grad_weight, float smooth_weight, float reproj_weight,
                           int max_batch, int height, int width, int device, cad_loss** out);
void cad_loss_destroy(cad_loss* l);
/* forwardWithIntrinsics + backward: loss5 (device, 5 floats) = {total, si, grad, smooth, reproj};
 * dpred (device, B*H*W) = dL/dpred.  K (B,3,3) row-major. */
cad_status cad_loss_forward_backward(cad_loss* l, const float* pred, const float* gt, const float* rgb,
                                     const float* K, int B, float* loss5, float* dpred, void* stream);
/* the same with forwardWithIntrinsics' optional valid_mask (depth_loss.h:416-433): mask (device,
 * B*H*W bytes, nonzero = valid) replaces the default gt > 1e-6 mask of the scale-invariant and
 * reprojection terms (:38-40, :320-322); the gradient-matching term ignores it like the reference
 * (:137) and smoothness never takes one (:189).  mask == NULL: cad_loss_forward_backward. */
cad_status cad_loss_forward_backward_masked(cad_loss* l, const float* pred, const float* gt, const float* rgb,
                                            const float* K, const uint8_t* mask, int B, float* loss5, float* dpred,
                                            void* stream);
/* getComponentsWithIntrinsics: host copy of {total, si, grad, smooth, reproj} of the last call */
cad_status cad_loss_get_components(cad_loss* l, float out5[5], void* stream);

/* ---- metrics (computeDepthMetrics) on host-visible results: abs_rel etc. per sample, averaged */
cad_status cad_depth_metrics(const float* pred, const float* gt, int B, int H, int W, float out7[7],
                             void* stream);

/* ---- offline evaluation: DepthMetrics::compute (src/evaluation/depth_metrics.h:40-88) per sample over
 * a whole split.  The evaluator owns a device table of `capacity` rows of twelve double sums
 * {n, sum|p-g|/g, sum(p-g)^2/g, sum(p-g)^2, sum(ln p - ln g)^2, sum|p-g|, sum|log10 p - log10 g|,
 *  #(r < 1.25), #(r < 1.25^2), #(r < 1.25^3), sum p, sum g},  r = max(p/g, g/p), over the valid pixels
 * gt > min_depth && gt < max_depth (strict) [&& mask != 0], p = clamp(pred, min_depth, max_depth) when
 * clamp_pred.  fp32 per-pixel terms, double accumulation in a fixed order: a sample's row is the same
 * bits on every run, in whichever batch it arrives, from aligned or unaligned tensors.
 * Metric order (CAD_EVAL_METRICS values per sample): abs_rel, sq_rel, rmse, rmse_log, mae, log10,
 * delta_1.25, delta_1.25^2, delta_1.25^3, num_valid_pixels, mean_pred_depth, mean_gt_depth; a sample
 * without a valid pixel yields twelve zeros and is counted (getZeroMetrics + average, :122-141,238). */
#define CAD_EVAL_METRICS 12
typedef struct {
    float min_depth; /* 0.1 */
    float max_depth; /* 10.0 */
    int clamp_pred;  /* 1 */
} cad_eval_config;
typedef struct {
    int64_t count;                   /* samples */
    float mean[CAD_EVAL_METRICS];    /* over samples */
    float std[CAD_EVAL_METRICS];     /* population standard deviation (/ N), evaluator.h:385-397 */
    float median[CAD_EVAL_METRICS];  /* mean of the two middle values for even N */
    float min[CAD_EVAL_METRICS];
    float max[CAD_EVAL_METRICS];
    float pooled[CAD_EVAL_METRICS];  /* the twelve sums added over all samples, finished once: what
                                        DepthMetrics::compute returns for all samples as one batch */
} cad_eval_summary;
typedef struct cad_evaluator cad_evaluator;
/* allocates everything the evaluator will ever need (table, partials for max_batch samples of H x W);
 * cfg NULL: the defaults.  Arguments are checked before any device call. */
cad_status cad_evaluator_create(int64_t capacity, int max_batch, int H, int W, const cad_eval_config* cfg, int device,
                                cad_evaluator** out);
void cad_evaluator_destroy(cad_evaluator* e);
cad_status cad_evaluator_reset(cad_evaluator* e); /* count = 0 (host counter only) */
/* appends B rows: pred, gt (B,1,H,W) device fp32, mask (device, B*H*W bytes, nonzero = valid) or NULL.
 * Two kernels on `stream` (the alignment kernels before them with an alignment mode, below); no allocation,
 * no host synchronisation, no host copy.  count + B > capacity
 * or B > max_batch: CAD_ERR_INVALID, table and count unchanged.  Successive updates share the partials
 * buffer: issue them on one stream (or order the streams yourself). */
cad_status cad_evaluator_update(cad_evaluator* e, const float* pred, const float* gt, const uint8_t* mask, int B,
                                void* stream);
int64_t cad_evaluator_count(const cad_evaluator* e); /* samples so far */
/* host copy of the table's first count rows (count x 12 doubles); one synchronous copy on `stream` */
cad_status cad_evaluator_sums(cad_evaluator* e, double* out, void* stream);
/* cad_evaluator_sums on the stream of the last update, then cad_eval_finish; per_sample may be NULL */
cad_status cad_evaluator_metrics(cad_evaluator* e, float* per_sample, cad_eval_summary* s);
/* host only (no device): n rows of twelve sums -> per-sample metrics (n x 12, nullable) and the summary
 * (nullable), in double, rounded to fp32 at the end */
cad_status cad_eval_finish(const double* sums, int64_t n, float* per_sample, cad_eval_summary* s);

/* ---- scale-aligned evaluation.  With an alignment mode set, update first computes a per-sample
 * (scale s, shift t) on the device, stores it in a table of capacity x 2 floats, and the metrics pass
 * scores s * pred + t (one fp32 multiply, one fp32 add, then the clamp_pred clamp).  The statistics run
 * over the evaluator's valid pixels and use the raw pred, before the clamp; finite pred is a precondition.
 *   CAD_ALIGN_NONE         s = 1, t = 0: the unaligned code path, bit-identical rows
 *   CAD_ALIGN_MEDIAN       s = med(gt) / med(pred) as one fp32 division; med(v) = (v_sorted[(n-1)/2] +
 *                          v_sorted[n/2]) * 0.5f in fp32, found exactly by radix select on the device
 *   CAD_ALIGN_LOG_MEAN     s = exp(mean(ln gt - ln pred)) over the valid pixels with pred > 0 (double)
 *   CAD_ALIGN_SCALE_SHIFT  the (s, t) minimising sum (s pred + t - gt)^2, closed form in double from
 *                          n, sum p, sum g, sum p^2, sum pg
 * Fallbacks: no valid pixel, med(pred) <= 0, or no valid pixel with pred > 0: (1, 0); scale_shift with
 * n sum p^2 - (sum p)^2 <= 0: scale only, s = sum pg / sum p^2 (1 when sum p^2 = 0), t = 0.  A sample's
 * (s, t) is the same bits on every run, in whichever batch it arrives, from aligned or unaligned tensors. */
typedef enum { CAD_ALIGN_NONE = 0, CAD_ALIGN_MEDIAN = 1, CAD_ALIGN_LOG_MEAN = 2, CAD_ALIGN_SCALE_SHIFT = 3 } cad_eval_align;
/* allowed only while count == 0 (after create or reset); allocates the alignment workspace here, so that
 * update still allocates nothing.  Unknown mode or count > 0: CAD_ERR_INVALID, nothing changed. */
cad_status cad_evaluator_set_alignment(cad_evaluator* e, int mode);
int cad_evaluator_get_alignment(const cad_evaluator* e);
/* host copy of the first count rows of (scale, shift): count x 2 floats, one synchronous copy on `stream`
 * ((1, 0) rows with CAD_ALIGN_NONE, without a device call) */
cad_status cad_evaluator_alignment(cad_evaluator* e, float* out, void* stream);
/* count bytes beside cad_evaluator_alignment: 1 where the mode's own formula gave the row, 0 where a
 * fallback applied (all 0 with CAD_ALIGN_NONE) */
cad_status cad_evaluator_aligned(cad_evaluator* e, uint8_t* out, void* stream);
/* stand-alone: medians of pred and gt over each sample's valid pixels -> out (device, B x 2 floats
 * {med_pred, med_gt}; 0, 0 without a valid pixel).  Allocates and frees its own workspace and waits for
 * `stream`.  Arguments are checked before any device call. */
cad_status cad_valid_medians(const float* pred, const float* gt, const uint8_t* mask, int B, int H, int W,
                             float min_depth, float max_depth, float* out, void* stream);
/* host only (no device): stats = {n, n_pos, sum p, sum g, sum p^2, sum pg, sum(ln g - ln p)},
 * med = {med_pred, med_gt} (read for CAD_ALIGN_MEDIAN only, may be NULL otherwise) -> out2 = {scale, shift}.
 * The code the device solve kernel runs. */
cad_status cad_eval_solve_alignment(int mode, const double stats[7], const float med[2], float out2[2]);

/* ---- stratified evaluation.  With strata set, update keeps the same twelve sums per sample and per
 * stratum on two per-pixel axes, computed on the device in the pass that fills the sample's total row (the
 * total row keeps its bits; the pixel terms, the valid set and the alignment, which stays per sample over all
 * its valid pixels, are those of the unstratified evaluator).
 *   depth axis  cuts c_0 < ... < c_{m-1}, fp32, finite, strictly inside (min_depth, max_depth), 1 <= m <= 15.
 *               A valid pixel's bin is the number of cuts with c_j <= gt (fp32 comparison): m + 1 bins
 *               [min, c_0), [c_0, c_1), ..., [c_{m-1}, max).
 *   angle axis  cuts th_0 < ... < th_{m-1} in degrees, inside (0, 90), 1 <= m <= 15; the host forms
 *               t_j = (float)(tan(th_j pi / 180)^2), tangent and square in double, rounded once.  With
 *               u = column, v = row as fp32 values of the integer pixel index and fx = K[0], cx = K[2],
 *               fy = K[4], cy = K[5] of the sample's row-major K (the K of the H x W batch):
 *               x = (u - cx) / fx, y = (v - cy) / fy, rho2 = x x + y y, every operation an individually
 *               rounded fp32 operation, no epsilon.  The bin is the number of cuts with t_j <= rho2 (a NaN
 *               rho2: bin 0): m + 1 bins, the last one ending at 90 degrees.
 * On each axis every valid pixel lies in exactly one bin: per sample n and the three delta counts add over
 * the bins to the total row exactly, the eight real sums within double rounding.  A sample's stratum rows
 * are the same bits on every run, in whichever batch it arrives, from aligned or unaligned tensors (no
 * floating-point atomics; fixed reduction order). */
#define CAD_STRATA_MAX_BINS 16
#define CAD_STRATA_DEPTH 0
#define CAD_STRATA_ANGLE 1
typedef struct {
    int n_depth_cuts;                              /* 0: the depth axis is off */
    float depth_cuts[CAD_STRATA_MAX_BINS - 1];     /* metres */
    int n_angle_cuts;                              /* 0: the angle axis is off */
    float angle_cuts_deg[CAD_STRATA_MAX_BINS - 1]; /* degrees off the optical axis */
} cad_strata_config;
/* allowed only while count == 0; every rule above is checked before any device call and the message names
 * the offending value.  Allocates the strata table (capacity x bins x 12 doubles per axis) and the partials
 * here, so that update still allocates nothing.  cfg NULL or both axes with 0 cuts: strata off.  On an
 * error nothing changes. */
cad_status cad_evaluator_set_strata(cad_evaluator* e, const cad_strata_config* cfg);
/* cad_evaluator_update with the batch's K (B,3,3) device fp32: the required form while the angle axis is on
 * (cad_evaluator_update is then CAD_ERR_INVALID, table and count unchanged).  K may be NULL while the angle
 * axis is off.  With strata set three kernels on `stream` instead of two; no allocation, no synchronisation. */
cad_status cad_evaluator_update_k(cad_evaluator* e, const float* pred, const float* gt, const uint8_t* mask,
                                  const float* K, int B, void* stream);
/* bins on an axis (cuts + 1), 0 when the axis is off */
int cad_evaluator_strata_bins(const cad_evaluator* e, int axis);
/* host copy of the axis's first count rows: count x bins x 12 doubles; one synchronous copy on `stream` */
cad_status cad_evaluator_strata_sums(cad_evaluator* e, int axis, double* out, void* stream);
/* host only: the tan^2 thresholds t_j of n angle cuts in degrees, as the evaluator forms them */
cad_status cad_strata_angle_thresholds(const float* cuts_deg, int n, float* out);
/* host only: n x bins rows of twelve sums -> per-sample, per-bin metrics (n x bins x 12, nullable) and one
 * summary per bin (bins, nullable), the formulas of cad_eval_finish with one difference: a bin's mean / std /
 * median / min / max run over the samples with at least one valid pixel in that bin, and count is their
 * number (an image without a pixel in the stratum says nothing about it); pooled adds all samples' sums.
 * A bin no sample reaches: count 0 and zeros. */
cad_status cad_eval_strata_finish(const double* sums, int64_t n, int bins, float* per_sample, cad_eval_summary* per_bin);

/* ---- geometric evaluation: surface-normal and 3-D point metrics from K.  With geometry on, update_k also
 * scores, per sample, quantities computed in camera space.  With fx = K[0], cx = K[2], fy = K[4], cy = K[5] of
 * the sample's row-major K (the K of the H x W batch), u = column, v = row as fp32 values of the integer pixel
 * index, x = (u - cx) / fx, y = (v - cy) / fy.  Per-pixel arithmetic is individually rounded fp32, accumulation
 * is double in a fixed order, no floating-point atomics.
 *   depths   ground truth g; prediction p = clamp(s pred + t), the value the metrics pass scores (the
 *            sample's alignment, then the clamp_pred clamp); the valid set is the evaluator's.
 *   normal   of a depth map d at (u, v), central differences of the back-projected points P = (x d, y d, d),
 *            (P(u+1,v) - P(u-1,v)) x (P(u,v+1) - P(u,v-1)), in the cancellation-free closed form
 *              a = d(u+1,v) - d(u-1,v)   A = (d(u+1,v) + d(u-1,v)) / fx
 *              b = d(u,v+1) - d(u,v-1)   B = (d(u,v+1) + d(u,v-1)) / fy
 *              c = (-a B, -A b, (A B + (x a) B) + (y A) b),   n = -c / |c|   (n_z < 0 for a frontal wall)
 *   normal-valid  1 <= u <= W-2, 1 <= v <= H-2, the pixel and its four neighbours in the valid set, c_p and
 *            c_g finite with |c| > 0.  No such pixel when H < 3 or W < 3.
 *   theta    atan2f(|n_p x n_g|, n_p . n_g) * (float)(180 / pi), degrees in [0, 180]
 *   e        |p - g| * sqrtf((1 + x x) + y y), the distance between the pixel's two back-projected points,
 *            over the valid set (its count is the total row's n)
 * Per sample a row of CAD_GEOM_SUMS doubles {n_normal, sum theta, sum theta^2, #(theta < 11.25f),
 * #(theta < 22.5f), #(theta < 30.0f), sum e, sum e^2} and one fp32 median of theta over the normal-valid
 * pixels, (theta_sorted[(n-1)/2] + theta_sorted[n/2]) * 0.5f, found exactly by CAD_ALIGN_MEDIAN's radix
 * select (0 without a normal-valid pixel).  Metric order (CAD_GEOM_METRICS values per sample): normal_mean,
 * normal_median, normal_rmse, normal_11.25, normal_22.5, normal_30, num_normal_pixels, point_mae, point_rmse.
 * A sample's row and median are the same bits on every run, in whichever batch it arrives, from 16-byte
 * aligned or unaligned tensors.  Per-stratum geometry is not kept: the strata rows are unaffected. */
#define CAD_GEOM_SUMS 8
#define CAD_GEOM_METRICS 9
typedef struct {
    int64_t count;         /* samples */
    int64_t count_normal;  /* samples with n_normal > 0: the set of columns 0..6 */
    int64_t count_point;   /* samples with a valid pixel: the set of columns 7, 8 */
    float mean[CAD_GEOM_METRICS]; /* the strata's rule: over the samples of the column's set */
    float std[CAD_GEOM_METRICS];
    float median[CAD_GEOM_METRICS];
    float min[CAD_GEOM_METRICS];
    float max[CAD_GEOM_METRICS];
    float pooled[CAD_GEOM_METRICS]; /* all samples' sums added, finished once; normal_median: NaN (not defined) */
} cad_geom_summary;
/* allowed only while count == 0.  on != 0 allocates the geometry table (capacity x 8 doubles), the medians,
 * the theta and normal-valid maps (max_batch x H x W), the partials and a select workspace here, so that
 * update still allocates nothing and never synchronises; needs H * W < 2^31.  While geometry is on
 * cad_evaluator_update_k with a non-NULL K is the required form (cad_evaluator_update, or a NULL K:
 * CAD_ERR_INVALID, table and count unchanged), and it issues the stencil pass, its finalise and the select's
 * eight kernels after the metrics pass.  On an error nothing changes. */
cad_status cad_evaluator_set_geometry(cad_evaluator* e, int on);
int cad_evaluator_get_geometry(const cad_evaluator* e);
/* host copies of the first count rows: count x 8 doubles / count floats; one synchronous copy on `stream`.
 * CAD_ERR_INVALID while geometry is off. */
cad_status cad_evaluator_geom_sums(cad_evaluator* e, double* out, void* stream);
cad_status cad_evaluator_geom_medians(cad_evaluator* e, float* out, void* stream);
/* host only (no device): n geometry rows, their n medians and the samples' total rows (n x 12 sums of
 * cad_evaluator_sums; column 0, the valid count, is the n of the point statistics) -> per-sample metrics
 * (n x 9, nullable; zeros for a sample outside a column's set) and the summary (nullable), in double, rounded
 * to fp32 at the end.  A set no sample reaches: count 0 and zeros. */
cad_status cad_eval_geom_finish(const double* sums, const float* medians, const double* total_sums, int64_t n,
                                float* per_sample, cad_geom_summary* summary);
/* stand-alone: normals of depth (B,1,H,W) device fp32 from K (B,3,3) by the closed form above.  A pixel is
 * valid when it and its four neighbours are finite, min_depth < d < max_depth (strict) and mask != 0 (mask:
 * B*H*W device bytes or NULL).  normals: (B,3,H,W) device fp32, zeros where invalid; valid: B*H*W device bytes;
 * either may be NULL, not both.  One kernel on `stream`, no allocation, no synchronisation. */
cad_status cad_depth_normals(const float* depth, const float* K, const uint8_t* mask, int B, int H, int W,
                             float min_depth, float max_depth, float* normals, uint8_t* valid, void* stream);

/* ---- conditioning: per-pixel unit ray directions (B,3,H,W) from K (B,3,3) ---- */
cad_status cad_ray_directions(const float* K, int B, int H, int W, float* rays, void* stream);

/* ---- virtual cameras: the sample a camera with other intrinsics, or rotated about its centre, would have
 * recorded.  Neither change has parallax, so the image follows from the recorded one by a homography and the
 * ground-truth depth by the same homography and a per-pixel rescale of Z; no reference counterpart.
 *
 * Conventions: pixel centres at integer coordinates, depth is Z along the optical axis, x right, y down,
 * z forward, skew ignored.  A view changes a sample's K (fx, fy, cx, cy) into K' and rotates the camera by R
 * (row-major 3x3, P' = R P):
 *   fx' = zoom_x fx, fy' = zoom_y fy, cx' = cx + shift_x W, cy' = cy + shift_y H     (fp32, on the device)
 *   R = Rz(roll) Rx(pitch) Ry(yaw), Ry(t) = [[c,0,-s],[0,1,0],[s,0,c]] (a positive yaw turns the camera right:
 *   the scene moves left), Rx(t) = [[1,0,0],[0,c,-s],[0,s,c]], Rz(t) = [[c,-s,0],[s,c,0],[0,0,1]]; computed
 *   once on the host in double and rounded to fp32.
 * Per output pixel (u', v'): d' = ((u' - cx') / fx', (v' - cy') / fy', 1), d = R^T d', source coordinate
 * u = (fx d.x) / d.z + cx, v = (fy d.y) / d.z + cy.
 *   rgb    bilinear between floor and floor + 1 of the coordinate clamped to [0, W-1] x [0, H-1] (edge
 *          replicate); 0 where d.z <= 0 or the coordinate is not finite
 *   depth  nearest (iu = floor(u + 0.5), iv = floor(v + 0.5)): Z' = Z(iv, iu) / d.z where the tap is inside
 *          the image, d.z > 0, Z(iv, iu) is finite and positive and the source mask, if any, is non-zero
 *          there; 0 otherwise (every loss and metric treats 0 as a hole)
 *   valid  that predicate
 * A sample whose R is the identity and whose K' equals K bit for bit is copied: rgb and depth keep their
 * bits.  With R the identity alone d.z == 1 and Z' keeps the bits of the sampled Z.  The fp32 operations of
 * the coordinates are individually rounded in the order written, so a fp32 restatement reproduces them. */
typedef struct cad_view {
    float zoom_x, zoom_y;                /* neutral: 1, 1 */
    float shift_x, shift_y;              /* in image widths / heights; neutral: 0, 0 */
    float yaw_deg, pitch_deg, roll_deg;  /* neutral: 0, 0, 0 */
} cad_view;
/* host only: CAD_ERR_INVALID, with a message naming the value, for a non-finite field, a non-positive zoom or
 * an angle of magnitude >= 80 degrees */
cad_status cad_view_check(const cad_view* view);
/* host only: the view's R (9 floats, row-major) */
cad_status cad_view_rotation(const cad_view* view, float* R9);
/* view: host; K (B,3,3) device -> K_new (B,3,3) and R (B,3,3) device: every sample's K' and the view's R.
 * Entries of K other than fx, fy, cx, cy are carried over.  One kernel on `stream`, one thread per sample.
 * Refuses what cad_view_check refuses and B, H or W <= 0. */
cad_status cad_view_resolve(const cad_view* view, const float* K, int B, int H, int W, float* K_new, float* R, void* stream);
/* rgb (B,3,H,W), depth (B,1,H,W) device fp32, mask B*H*W device bytes or NULL, K, K_new, R (B,3,3) device fp32
 * (per sample: a batch may mix views) -> rgb_out, depth_out, valid_out (B*H*W device bytes or NULL).  One
 * kernel on `stream`, no allocation, no synchronisation.  Outputs must not overlap the inputs or each other
 * (the alias check refuses that). */
cad_status cad_camera_view(const float* rgb, const float* depth, const uint8_t* mask, const float* K, const float* K_new,
                           const float* R, int B, int H, int W, float* rgb_out, float* depth_out, uint8_t* valid_out,
                           void* stream);

/* ---- batch assembly on device: decoded samples -> the step's (B,3,H,W) rgb, (B,1,H,W) depth,
 * (B,3,3) K.  Per sample: rgb = u8/255, depth = u16 * depth_scale, resized to H x W (rgb bilinear,
 * align_corners = false; depth nearest; K scaled), then — when aug is set — crop (window clamped to
 * the image like a torch Slice, K's principal point shifted), horizontal flip (cx = W - cx - 1),
 * colour jitter clamp(rgb * contrast + brightness - 1, 0, 1), and the resize back to H x W.
 *
 * The declared colour stages (data.augmentation saturation / hue / random_gamma, which the reference parses
 * and never applies; all-zero fields = the behaviour above).  They act on rgb only, per source tap of the
 * resize back, after the jitter: with `color`, c' = clamp((M[c][0] r + M[c][1] g) + M[c][2] b, 0, 1) in
 * unfused fp32 with M = cad_color_matrix(saturation, hue); with `gamma_on`, v' = powf(v, gamma), gamma > 0,
 * finite.  Depth and K are those of the same sample without them. */
typedef struct {
    const uint8_t* rgb;     /* device: decoded image, HWC u8, h0 x w0 x 3 */
    const uint16_t* depth;  /* device: decoded depth, HW u16 */
    int h0, w0;
    int bgr;                /* 1: rgb is in OpenCV BGR order (loadRGB's cvtColor happens here) */
    float depth_scale;      /* metres per unit: 1/1000 (loadDepth) */
    float K[9];             /* host: the sample's intrinsics, 3x3 row-major */
    int aug;                /* 0: resize only (validation / augmentation off) */
    int crop;               /* applyCrop with crop_scale, crop_x, crop_y (on the resized image) */
    float crop_scale;
    int crop_x, crop_y;
    int flip;               /* applyHorizontalFlip */
    int jitter;             /* applyColorJitter with brightness, contrast */
    float brightness, contrast;
    int dh0, dw0;           /* depth map size when it differs from the image's (0: h0 x w0) */
    int color;              /* saturation / hue matrix cad_color_matrix(saturation, hue) (needs aug) */
    float saturation, hue;  /* blend factor around 1; fraction of the colour circle */
    int gamma_on;           /* powf(v, gamma) (needs aug) */
    float gamma;
} cad_sample;
typedef struct cad_batcher cad_batcher;
cad_status cad_batcher_create(int max_batch, int height, int width, int device, cad_batcher** out);
void cad_batcher_destroy(cad_batcher* b);
/* asynchronous on `stream`; samples[] is read before the call returns */
cad_status cad_batcher_assemble(cad_batcher* b, const cad_sample* samples, int B, float* rgb, float* depth,
                                float* K, void* stream);

typedef struct { /* AugmentationConfig (sunrgbd_loader.h:30-42) */
    int enable_random_crop;
    float crop_scale_min, crop_scale_max; /* 0.7, 1.0 */
    int enable_horizontal_flip;
    float horizontal_flip_prob; /* 0.5 */
    int enable_color_jitter;
    float brightness_delta, contrast_delta; /* 0.2, 0.2 */
    /* the declared stages (0 / off: augmentSample's draws, bit for bit) */
    float saturation_delta, hue_delta; /* in [0, 1] and [0, 0.5]; drawn when enable_color_jitter */
    int enable_random_gamma;
    float gamma_min, gamma_max; /* 0 < min <= max */
} cad_aug_config;
typedef struct cad_aug_sampler cad_aug_sampler;
/* std::mt19937 seeded like the loader's rng_ (config.random_seed); a bad range fails with a message
 * naming the field */
cad_status cad_aug_sampler_create(const cad_aug_config* cfg, uint32_t seed, cad_aug_sampler** out);
void cad_aug_sampler_destroy(cad_aug_sampler* s);
/* fills sample->aug/crop/flip/jitter fields with augmentSample's draws, in its order, for an image
 * already resized to height x width; then, from the same engine through uniform_real_distribution<float>:
 * saturation ~ U[1 - ds, 1 + ds] (enable_color_jitter and ds > 0), hue ~ U[-dh, dh] (enable_color_jitter
 * and dh > 0), gamma ~ U[gamma_min, gamma_max] (enable_random_gamma) */
cad_status cad_aug_sampler_draw(cad_aug_sampler* s, int height, int width, cad_sample* sample);
/* host only: the fp32 matrix the batcher applies for (saturation, hue), row-major.  M = T^-1 D T, T the NTSC
 * RGB -> YIQ matrix, D = diag(1, s R(2 pi hue)), evaluated in double as I + T^-1 (D - I) T (so that (1, 0) is
 * exactly the identity) and rounded; rows sum to 1 (grey stays grey) */
cad_status cad_color_matrix(float saturation, float hue, float out[9]);

/* ---- the loader: SunRGBDLoader's manifest + decoding (src/data/sunrgbd_loader.cpp:39-102, 221-275)
 * and a prefetch ring into the batcher.  cad_dataset_open reads the JSON manifest: "images" entries
 * with valid == true, a sensor_type in sensors[] (NULL/0: kv1, kv2, realsense, xtion — the loader's
 * default) and an existing <path>/intrinsics.txt, in manifest order (paths relative to the working
 * directory, as in the reference).  A sample decodes <path>/image/<first .jpg|.png|.ppm> as RGB u8
 * and <path>/depth/<first .png|.pgm> as u16 (16-bit: metres = value / 1000; 8-bit: value), PNG and
 * binary PNM, and baseline / extended-sequential / progressive Huffman JPEG (csrc/host/jpeg.cpp:
 * libjpeg-turbo's default decompression — ISLOW IDCT, fancy upsampling, jdcolor.c YCbCr->RGB —
 * restated bit for bit; arithmetic / lossless / 12-bit / CMYK JPEGs and progressions cut short (which
 * libjpeg-turbo block-smooths) fail with a message). */
typedef struct cad_dataset cad_dataset;
/* decode a JPEG file held in memory (what cv::imread(IMREAD_COLOR) decodes for the loader,
 * sunrgbd_loader.cpp:86,222, before its BGR order): height x width x channels u8 samples (channels 1
 * gray or 3 RGB) into out (out == NULL: dimensions only) */
cad_status cad_jpeg_decode(const uint8_t* data, int64_t size, uint8_t* out, int64_t cap, int* height, int* width,
                           int* channels);
typedef struct {
    int h0, w0;        /* rgb size */
    int dh0, dw0;      /* depth size */
    float depth_scale; /* metres per depth unit */
    float K[9];        /* intrinsics.txt, row-major */
} cad_decoded_info;
cad_status cad_dataset_open(const char* manifest_path, const char* const* sensors, int n_sensors, cad_dataset** out);
/* n procedurally generated decoded samples of height x width (the synthetic dataset) */
cad_status cad_dataset_synthetic(int64_t n, int height, int width, uint32_t seed, cad_dataset** out);
void cad_dataset_destroy(cad_dataset* d);
int64_t cad_dataset_size(const cad_dataset* d);
const char* cad_dataset_image_dir(const cad_dataset* d, int64_t i); /* NULL for synthetic */
/* the sample's manifest sensor_type ("synthetic" for the synthetic dataset); NULL out of range */
const char* cad_dataset_sensor(const cad_dataset* d, int64_t i);
/* host decode of sample i into rgb (h0*w0*3 bytes) and depth (dh0*dw0 u16); either may be NULL to
 * query info only */
cad_status cad_dataset_read(const cad_dataset* d, int64_t i, uint8_t* rgb, int64_t rgb_cap, uint16_t* depth,
                            int64_t depth_cap, cad_decoded_info* info);
/* Prefetch ring: `threads` host workers decode up to `slots` (>= 2) batches ahead into pinned
 * buffers; each batch is uploaded on the loader's copy stream and assembled on the caller's stream
 * by a cad_batcher (resize; with aug != NULL, augmentSample's draws from a mt19937 seeded `seed`,
 * drawn in sample order).  The dataset must outlive the loader. */
typedef struct cad_loader cad_loader;
cad_status cad_loader_create(const cad_dataset* ds, int batch, int height, int width, const cad_aug_config* aug,
                             uint32_t seed, int threads, int slots, int device, cad_loader** out);
void cad_loader_destroy(cad_loader* L);
/* the epoch's sample order (NULL: 0..n-1); batches of `batch`, the last one partial (trainEpoch) */
cad_status cad_loader_start_epoch(cad_loader* L, const int64_t* order, int64_t n);
/* the next batch into rgb (B,3,H,W), depth (B,1,H,W), K (B,3,3) device fp32, asynchronously on
 * `stream`; returns its size B (0 at the end of the epoch, -1 on error: cad_last_error()) */
int cad_loader_next(cad_loader* L, float* rgb, float* depth, float* K, void* stream);

/* ---- debugging: synchronous host copy of an internal NHWC activation buffer by name
 * ("x0", "cat<l>", "dcat<l>", "pool<l>", "dout<l>", "bott", "Sa", "Sb", "Sc",
 *  "enc<l>.y1|a1|y2", "dec<l>.y1|a1|y2"); numel = rows*channels of the last forward's batch.
 * CAD_MODEL_INTRINSICS_ATTN adds the CBAM state of att<l+1>: "att<l>" [B][C] channel attention, "sa<l>"
 * [B*H_l*W_l] spatial attention, and the two argmax decisions "amax<l>" [B][C] (pixel within the sample) and
 * "sidx<l>" [B*H_l*W_l] (channel), int32 bit-copied into the float buffer.
 * Returns the element count (host may be NULL to query), or -1 for an unknown name — and, on the
 * bf16 engine (pre-split operands), for the buffers whose fp32 copy that path does not write
 * ("Sb", "bott", "pool<l>", "dout1..3", every block's a1); cad_last_error() says which. */
int64_t cad_unet_debug_buffer(cad_unet* h, const char* name, float* host, int64_t numel);

/* ---- launch profiler: HIP events around every MFMA GEMM launch on its own stream ---- */
cad_status cad_profile_enable(int on);
cad_status cad_profile_reset(void);
/* time only the launches of the kernel named kernel_name (as the report names it); NULL or "": all */
cad_status cad_profile_only(const char* kernel_name);
/* writes a JSON array [{"name","launches","ms","gflop"}...] into buf (synchronises); returns the
 * length needed including the terminator */
int cad_profile_report(char* buf, int cap);

/* ---- operator-level entry points (NHWC fp32; ld = floats between pixels, coff = channel offset) */
cad_status cad_op_conv3x3_fwd(const float* x, int64_t ldx, int xcoff, int cin, const float* w_ohwi,
                              int cout, float* y, int64_t ldy, int ycoff, int B, int H, int W,
                              void* stream);
cad_status cad_op_conv3x3_dgrad(const float* dz, int cout, const float* w_ohwi, int cin, float* dx,
                                int64_t lddx, int B, int H, int W, void* stream);
cad_status cad_op_conv3x3_wgrad(const float* dz, int cout, const float* x, int64_t ldx, int xcoff, int cin,
                                float* dw_ohwi, int B, int H, int W, void* stream);
/* the bf16 engine's weight gradient on pre-split bf16 NHWC operands (the twins the engine stores):
 * dz rows of lddz bf16, x rows of ldx bf16 at channel offset xcoff (% 8); fp32 OHWI result.  Window
 * kernel when cout, cin % 64 == 0 and W % 16 == 0, the im2col GEMM otherwise.  Requires
 * cad_set_gemm_engine(CAD_GEMM_BF16). */
cad_status cad_op_conv3x3_wgrad_bf16(const void* dz, int64_t lddz, int cout, const void* x, int64_t ldx, int xcoff,
                                     int cin, float* dw_ohwi, int B, int H, int W, void* stream);
/* the bf16 engine's 3x3 convolution forward / input gradient on pre-split bf16 NHWC operands (the twins
 * the engine stores), fp32 OHWI weights rounded to bf16 inside (the dgrad repacks them first):
 * window kernels (gemm_win.hpp) when the shape allows, the im2col GEMM otherwise.  y / dx: fp32 rows, or
 * bf16 rows with y_bf16 / dx_bf16.  with_stats: the forward also forms its BN tile partials (the
 * EpiStoreStats epilogue; the partials are discarded — timing and coverage).  Requires
 * cad_set_gemm_engine(CAD_GEMM_BF16); the bf16 forms of baseline_unet.h:32-42 DoubleConv's convs. */
cad_status cad_op_conv3x3_fwd_bf16(const void* x, int64_t ldx, int xcoff, int cin, const float* w_ohwi, int cout,
                                   void* y, int64_t ldy, int ycoff, int y_bf16, int with_stats, int B, int H, int W,
                                   void* stream);
cad_status cad_op_conv3x3_dgrad_bf16(const void* dz, int64_t lddz, int cout, const float* w_ohwi, int cin, void* dx,
                                     int64_t lddx, int dx_bf16, int B, int H, int W, void* stream);
/* The fused eval forward's convolutions (cad_unet_set_fused_eval): cad_op_conv3x3_fwd / _fwd_bf16 with the
 * block's eval-mode BatchNorm + ReLU and, with gam / bet, its FiLM modulation applied to the accumulator in the
 * GEMM epilogue (EpiStoreAct), so the pre-BN output never reaches memory:
 *   y[p][n] = max(fma(conv[p][n], scale[n], shift[n]), 0)                       gam == bet == NULL
 *   y[p][n] = gam[b][n] * max(conv[p][n] * scale[n] + shift[n], 0) + bet[b][n]   b = p / (H W)
 * scale / shift: cout floats; gam / bet: B x cout floats, both or neither.  H * W must be a multiple of 4.
 * y_bf16: y holds bf16 rows (the activation rounded once, to nearest even) — the pre-split entry only; the
 * fp32-operand entry stores fp32 and rejects y_bf16 != 0.  On CAD_GEMM_F32 the fp32 entry runs the same
 * epilogue on the f32 im2col kernel. */
cad_status cad_op_conv3x3_fwd_act(const float* x, int64_t ldx, int xcoff, int cin, const float* w_ohwi, int cout,
                                  const float* scale, const float* shift, const float* gam, const float* bet, void* y,
                                  int64_t ldy, int ycoff, int y_bf16, int B, int H, int W, void* stream);
cad_status cad_op_conv3x3_fwd_act_bf16(const void* x, int64_t ldx, int xcoff, int cin, const float* w_ohwi, int cout,
                                       const float* scale, const float* shift, const float* gam, const float* bet,
                                       void* y, int64_t ldy, int ycoff, int y_bf16, int B, int H, int W, void* stream);
cad_status cad_op_convT_fwd(const float* x, int cin, const float* w_iqo, const float* bias, int cout,
                            float* y, int64_t ldy, int ycoff, int B, int H, int W, void* stream);
/* the bf16 engine's ConvTranspose2d(k2, s2) forward (baseline_unet.h:91 `up`) on a pre-split bf16 NHWC
 * input (rows of ldx, channel offset xcoff), fp32 [ci][dy][dx][co] weights rounded to bf16 inside:
 * y (bf16 rows of ldy at channel offset ycoff, the decoder concat's up half) = x * w + bias, pixel-
 * shuffled.  Requires cad_set_gemm_engine(CAD_GEMM_BF16). */
cad_status cad_op_convT_fwd_bf16(const void* x, int64_t ldx, int xcoff, int cin, const float* w_iqo,
                                 const float* bias, int cout, void* y, int64_t ldy, int ycoff, int B, int H, int W,
                                 void* stream);
cad_status cad_op_convT_dgrad(const float* g, int64_t ldg, int gcoff, int cout, const float* w_iqo, int cin,
                              float* dx, int B, int H, int W, void* stream);
cad_status cad_op_convT_wgrad(const float* x, int cin, const float* g, int64_t ldg, int gcoff, int cout,
                              float* dw_iqo, int B, int H, int W, void* stream);
cad_status cad_op_maxpool_fwd(const float* x, int64_t ldx, int C, int B, int H, int W, float* out,
                              uint8_t* idx, void* stream);

/* MX-fp8 operands (OCP MXFP8 E4M3, one E8M0 scale per 32 consecutive k; the config-5 network's forward
 * conv-GEMMs, kernels.hpp Mx8): q = element bytes [rows][ldq], s = scale bytes [rows][ldq / 32],
 * ldq % 128 == 0.  quantize: rows [qcoff, qcoff + C) of (q, s) from src rows [scoff, scoff + C)
 * (fp32, or bf16 when src_bf16), C % 32 == 0. */
cad_status cad_op_mx8_quantize(const void* src, int src_bf16, int64_t lds, int scoff, int C, int64_t M, void* q,
                               void* s, int64_t ldq, int qcoff, void* stream);
/* y[m][n] (fp32, dense [M][N]) = sum_k x[m][k] w[n][k] on MX operands; K % 128 == 0, N % 64 == 0 */
cad_status cad_op_dense_x8(const void* xq, const void* xs, int64_t ldx, int K, const void* wq, const void* ws,
                           int64_t ldw, int N, float* y, int64_t M, void* stream);
/* y[pix][co] (fp32, dense [B*H*W][cout]) = conv3x3(x) on MX operands: x rows [pix][ldx] (cin channels),
 * w rows [cout][ldw] in (tap, ci) order (ldw >= 9 cin); cin % 64, cout % 64 and a window block width
 * dividing W (the window kernel), else CAD_ERR_INVALID */
cad_status cad_op_conv3x3_x8(const void* xq, const void* xs, int64_t ldx, int cin, const void* wq, const void* ws,
                             int64_t ldw, int cout, float* y, int B, int H, int W, void* stream);

/* ---- the config-5 network's operators, one launcher per call (tests, timing).  Rows are NHWC pixels;
 * a twin is plain row-major bf16 (ld / coff in elements, multiples of 8).  The dense GEMMs require
 * cad_set_gemm_engine(CAD_GEMM_BF16). */
/* y[m][ycoff + n] = sum_k x[m][xcoff + k] w[n][wcoff + k] on bf16 twins (K % 8 == 0): fp32 rows of ldy, or
 * bf16 rows with y_bf16.  add (nullable, fp32): y = x w^T + add, rows as y's when ldadd == 0 (add == y:
 * in place) or dense rows of their own stride ldadd >= N (then no mask and ycoff == 0); mask (nullable,
 * fp32, rows as y's, needs add): then y = 0 where mask is not > 0.  add takes fp32 y and no statistics.
 * mean / invstd (nullable, together, N floats; N % 4 == 0): the BatchNorm batch statistics (eps 1e-5) of
 * the stored y, from the GEMM epilogue's per-tile partials. */
cad_status cad_op_dense_fwd_bf16(const void* x, int64_t ldx, int xcoff, int K, const void* w, int64_t ldw, int wcoff,
                                 int N, void* y, int64_t ldy, int ycoff, int y_bf16, const float* add, int64_t ldadd,
                                 const float* mask, float* mean, float* invstd, int64_t M, void* stream);
/* dw[n][k] (fp32, ldw == K) = sum_m dz[m][dzcoff + n] x[m][xcoff + k] on bf16 twins; slab_max > 0 caps the
 * split-K slab (floats), 0: the launcher's own size */
cad_status cad_op_dense_wgrad_bf16(const void* dz, int64_t lddz, int dzcoff, int N, const void* x, int64_t ldx, int xcoff,
                                   int K, float* dw, int64_t ldw, int64_t M, int64_t slab_max, void* stream);
/* col[pix_out][k] (bf16 rows of Kp % 8 == 0) = x[pix_in][xcoff + c], k = (ky KW + kx) C + c; zero outside the
 * image and for k >= KH KW C.  x: fp32 rows, or bf16 rows with x_bf16. */
cad_status cad_op_im2col(const void* x, int x_bf16, int64_t ldx, int xcoff, int C, int B, int H, int W, int KH, int KW,
                         int stride, int pad, void* col, int Kp, void* stream);
/* dx[pix_in][c] (fp32 rows of lddx, overwritten) = sum over the taps reading pix_in of dcol[pix_out][tap C + c]
 * (fp32 rows of Kc >= KH KW C); C % 4 == 0 */
cad_status cad_op_col2im(const float* dcol, int Kc, int C, int B, int H, int W, int KH, int KW, int stride, int pad,
                         float* dx, int64_t lddx, void* stream);
/* MaxPool2d(3, 2, 1) on dense fp32 rows of C % 4 == 0: out (nullable) and its bf16 twin (nullable), idx =
 * ky 3 + kx of the first maximum in scan order (NaN propagates); the backward gathers dout through idx
 * into dx (overwritten), plus add rows of ldadd (nullable) */
cad_status cad_op_maxpool3s2_fwd(const float* x, int C, int B, int H, int W, float* out, uint8_t* idx, void* out_twin,
                                 void* stream);
cad_status cad_op_maxpool3s2_bwd(const float* dout, const uint8_t* idx, int C, int B, int H, int W, float* dx,
                                 const float* add, int64_t ldadd, void* stream);
/* out[m][c] = relu(y scale + shift + r), r = yd dscale + dshift (projection: yd != NULL) or x rows of ldx
 * (identity); y / yd dense fp32 rows, or bf16 with y_bf16; out dense fp32 [M][C], out_twin (nullable) its bf16
 * twin, q / s (nullable, together; C % 32 == 0, ldq % 128 == 0) the twin's MX-fp8 copy */
cad_status cad_op_bn_add_relu(const void* y, int y_bf16, const float* scale, const float* shift, const void* yd,
                              const float* dscale, const float* dshift, const float* x, int64_t ldx, int C, int64_t M,
                              float* out, void* out_twin, void* q, void* s, int64_t ldq, void* stream);
/* gs[m][c] (dense) = g[m][gcoff + c] where out[m][c] > 0, else 0 (gs == g allowed for dense g) */
cad_status cad_op_relu_mask(const float* g, int64_t ldg, int gcoff, const float* out, int C, int64_t M, float* gs,
                            void* stream);
/* y[m][ycoff + c] = 0 where mask[m][ycoff + c] (same rows) is not > 0 */
cad_status cad_op_mask_inplace(float* y, int64_t ldy, int ycoff, const float* mask, int C, int64_t M, void* stream);
/* dst[(b, s oy, s ox)][c] += src[(b, oy, ox)][scoff + c] over the ((H-1)/s + 1) x ((W-1)/s + 1) grid; s = 1, 2 */
cad_status cad_op_add_strided(float* dst, int64_t lddst, const float* src, int64_t ldsrc, int scoff, int C, int B, int H,
                              int W, int stride, void* stream);
/* bf16 rows dst[(b, oy, ox)][dcoff + c] = src[(b, s oy, s ox)][scoff + c]; C % 8 == 0 */
cad_status cad_op_copy_twin(const void* src, int64_t lds, int scoff, int C, int B, int H, int W, int stride, void* dst,
                            int64_t ldd, int dcoff, void* stream);
/* wt[k][n] (bf16, dense rows of N) = w[n][k] (fp32 rows of ldw), round-to-nearest-even */
cad_status cad_op_transpose_split(const float* w, int64_t ldw, int N, int K, void* wt, void* stream);

/* ---- config-5 network (BASELINE configs[4]): ResNet-50 encoder + U-Net decoder, bf16 operands ----
 * No reference counterpart: architecture in resunet.cpp / DESIGN.md §9;
 * torchvision ResNet-50 parameter names under "encoder.", decoder "dec4".."dec0", "out_conv".
 * Same life cycle as cad_unet: forward (train: BN batch statistics), backward (dL/ddepth), clip,
 * Adam (moments owned by the model). height / width multiples of 32. */
typedef struct cad_resunet cad_resunet;
typedef struct {
    int in_channels;   /* 3 */
    int max_batch;
    int height, width;
    float max_depth;
} cad_resunet_desc;
cad_status cad_resunet_create(const cad_resunet_desc* d, int device, cad_resunet** out);
void cad_resunet_destroy(cad_resunet* h);
int64_t cad_resunet_count_parameters(const cad_resunet* h);
int cad_resunet_num_tensors(const cad_resunet* h, int kind);   /* 0 parameters, 1 buffers */
cad_status cad_resunet_tensor_info(const cad_resunet* h, int kind, int idx, const char** name, int* ndim,
                                   int64_t shape[4]);
cad_status cad_resunet_set_tensor(cad_resunet* h, int kind, int idx, const float* host, int64_t numel);
cad_status cad_resunet_get_tensor(const cad_resunet* h, int kind, int idx, float* host, int64_t numel);
cad_status cad_resunet_get_grad(const cad_resunet* h, int idx, float* host, int64_t numel);
cad_status cad_resunet_train(cad_resunet* h, int train);
/* MX-fp8 forward conv-GEMMs (configs[4] "bf16 with fp8 MFMA conv-GEMM"): on = 1 runs
 * every eligible forward contraction (the 1x1 / im2col GEMMs with K % 128 == 0, the 3x3 window
 * convolutions with cin % 64 == 0) on OCP MXFP8 E4M3 operands with one E8M0 scale per 32 channels
 * (v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulation); the stem, ConvTs, the backward (dgrad,
 * wgrad) and everything else stay as on 0 (bf16 operands).  Default 0.  fp8_units: how many
 * convolutions are eligible. */
cad_status cad_resunet_set_fp8(cad_resunet* h, int on);
int cad_resunet_fp8_units(const cad_resunet* h);
cad_status cad_resunet_flat(cad_resunet* h, float** params, float** grads, int64_t* n);
cad_status cad_resunet_forward(cad_resunet* h, const float* rgb, float* depth, int B, void* stream);
cad_status cad_resunet_backward(cad_resunet* h, const float* ddepth, void* stream);
/* staged backward (decoder first; stage s writes only the gradients in its flat-slab range, ranges
 * decreasing with s) and the overlapped data-parallel exchange over it (cad_unet_backward_allreduce's
 * semantics: SUM buckets of >= bucket_elems floats on the communicator's stream) */
/* Test hook: a buffer of the last train-mode forward as fp32 rows — "y:<conv>" (stored pre-BN output,
   bf16 widened), "scale:<bn>" / "shift:<bn>" (BN-apply coefficients), "out:<block>" (block output:
   "encoder.layer<L>.<i>", "encoder.stem", "dec<l>"), "cat:dec<l>" (a decoder's bf16 input [skip, up]).
   Returns the element count, -1 if unknown. */
int64_t cad_resunet_debug_buffer(cad_resunet* h, const char* name, float* host, int64_t numel);
int cad_resunet_num_stages(const cad_resunet* h);
/* host only (no device): the stage count (23) and each stage's [offset, offset+count), as
 * cad_resunet_stage_grad_range reports them, and the slab size */
cad_status cad_resunet_grad_layout(int* nstages, int64_t stage_off[32], int64_t stage_cnt[32], int64_t* n_flat);
cad_status cad_resunet_stage_grad_range(const cad_resunet* h, int stage, int64_t* offset, int64_t* count);
cad_status cad_resunet_backward_stage(cad_resunet* h, int stage, const float* ddepth, void* stream);
cad_status cad_resunet_backward_allreduce(cad_resunet* h, cad_comm* c, const float* ddepth, int64_t bucket_elems,
                                          void* stream);
cad_status cad_resunet_clip_grad_norm(cad_resunet* h, float max_norm, float prescale, void* stream);
cad_status cad_resunet_last_grad_norm(cad_resunet* h, float* total_norm, void* stream);
cad_status cad_resunet_adam_step(cad_resunet* h, float lr, float beta1, float beta2, float eps, float weight_decay,
                                 void* stream);

/* ---- geometry-aware family, src/models/geometry_aware_network.h ----
 *   cad_geonet_create (CAD_GEONET_FULL)   GeometryAwareNetworkImpl(3, f, 4, max_depth, use_pcl,
 *                                         use_attention)  geometry_aware_network.h:201-278
 *   cad_geonet_create (CAD_GEONET_LIGHT)  LightweightGeometryNetworkImpl(3, f, 4, max_depth)  :355-383
 *   cad_geonet_forward                    GeometryAwareNetworkImpl::forward(rgb, ray_directions,
 *                                         camera_intrinsics (B,4) [fx, fy, cx, cy])  :289-318 / :385-402
 *     (RayEnhancedConvImpl :17-65, GeometryEncoderBlockImpl :74-104, GeometryDecoderBlockImpl
 *      :112-170, CBAMImpl spatial_attention.h:142-191, PerspectiveCorrectionLayerImpl pcl_layer.h:29-181)
 * rgb, rays (B,3,H,W) NCHW device fp32; depth (B,1,H,W).  Parameter / buffer names and order are the
 * reference module's named_parameters() / named_buffers() (float buffers).  Same life cycle as
 * cad_resunet.  H, W multiples of 32 (FULL, 5 pools) or 16 (LIGHT). */
#define CAD_GEONET_FULL 0
#define CAD_GEONET_LIGHT 1
typedef struct cad_geonet cad_geonet;
typedef struct {
    int variant;        /* CAD_GEONET_FULL / CAD_GEONET_LIGHT */
    int in_channels;    /* 3 */
    int init_features;  /* 64 (FULL default), 32 (LIGHT default) */
    int camera_dim;     /* 4 */
    float max_depth;    /* 10.0 */
    int use_pcl;        /* FULL only (LIGHT: always 1) */
    int use_attention;  /* FULL only (LIGHT: always 1) */
    int max_batch;
    int height, width;
} cad_geonet_desc;
cad_status cad_geonet_create(const cad_geonet_desc* d, int device, cad_geonet** out);
void cad_geonet_destroy(cad_geonet* h);
int64_t cad_geonet_count_parameters(const cad_geonet* h);
int cad_geonet_num_tensors(const cad_geonet* h, int kind);   /* 0 parameters, 1 buffers */
cad_status cad_geonet_tensor_info(const cad_geonet* h, int kind, int idx, const char** name, int* ndim,
                                  int64_t shape[4]);
cad_status cad_geonet_set_tensor(cad_geonet* h, int kind, int idx, const float* host, int64_t numel);
cad_status cad_geonet_get_tensor(const cad_geonet* h, int kind, int idx, float* host, int64_t numel);
cad_status cad_geonet_get_grad(const cad_geonet* h, int idx, float* host, int64_t numel);
cad_status cad_geonet_train(cad_geonet* h, int train);
cad_status cad_geonet_flat(cad_geonet* h, float** params, float** grads, int64_t* n);
cad_status cad_geonet_forward(cad_geonet* h, const float* rgb, const float* rays, const float* cam4, float* depth,
                              int B, void* stream);
cad_status cad_geonet_backward(cad_geonet* h, const float* ddepth, void* stream);
/* staged backward and the overlapped data-parallel exchange (as cad_resunet_*) */
int cad_geonet_num_stages(const cad_geonet* h);
/* host only (no device): the stage layout of the network `d` describes (as cad_resunet_grad_layout) */
cad_status cad_geonet_grad_layout(const cad_geonet_desc* d, int* nstages, int64_t stage_off[16], int64_t stage_cnt[16],
                                  int64_t* n_flat);
cad_status cad_geonet_stage_grad_range(const cad_geonet* h, int stage, int64_t* offset, int64_t* count);
cad_status cad_geonet_backward_stage(cad_geonet* h, int stage, const float* ddepth, void* stream);
cad_status cad_geonet_backward_allreduce(cad_geonet* h, cad_comm* c, const float* ddepth, int64_t bucket_elems,
                                         void* stream);
cad_status cad_geonet_clip_grad_norm(cad_geonet* h, float max_norm, float prescale, void* stream);
cad_status cad_geonet_last_grad_norm(cad_geonet* h, float* total_norm, void* stream);
cad_status cad_geonet_adam_step(cad_geonet* h, float lr, float beta1, float beta2, float eps, float weight_decay,
                                void* stream);
/* one step of opts->rule (CAD_OPTIM_*) at opts->lr on the in-handle moments (SGD's buffer in the first-moment
 * slab); keep to one rule per handle.  The EMA is U-Net-family only: opts->ema_decay != 0 is CAD_ERR_INVALID */
cad_status cad_geonet_optim_step(cad_geonet* h, const cad_optim_opts* opts, void* stream);
/* BatchNorm num_batches_tracked: film = 0 the BatchNorm2d layers, 1 FiLM's BatchNorm1d (B > 1 only) */
int64_t cad_geonet_num_batches_tracked(const cad_geonet* h, int film);
/* operator-level entry points (tests; state allocated per call): one CBAMImpl forward + backward
 * (spatial_attention.h:142-191) / one PerspectiveCorrectionLayerImpl forward + backward (pcl_layer.h:
 * 76-178) on device NHWC tensors [B*H*W][C]; params / grads packed in registration order
 * (CBAM: fc1.w [C/16][C], fc1.b, fc2.w [C][C/16], fc2.b, spatial conv.w [2][7][7]; PCL: loc_fc1.w
 * [128][C+4], loc_fc1.b, loc_fc2.w [128][128], loc_fc2.b, fc_transform.w [6][128], fc_transform.b);
 * g = gradient of the output; camn (B,4) the normalised intrinsics; theta (nullable) <- (B,2,3) */
cad_status cad_op_cbam(const float* x, const float* g, const float* params, int B, int H, int W, int C, float* out,
                       float* dx, float* grads, void* stream);
cad_status cad_op_pcl(const float* u, const float* camn, const float* g, const float* params, int B, int H, int W,
                      int C, float* out, float* du, float* grads, float* theta, void* stream);
/* level 0 of CAD_MODEL_INTRINSICS_ATTN, forward + backward, on device tensors (tests and A/B timing; state
 * allocated per call):  z = relu(y * scale + shift),  pred = max_depth * sigmoid(head_w . CBAM(z) + head_b).
 * y [B*H*W][C] fp32, or bf16 values when y_bf16; scale / shift [C]; cbam_params / cbam_grads packed as
 * cad_op_cbam's; head_w [C], head_b [1]; head_grads [C + 1] = {d head_w, d head_b}; dpred, pred [B*H*W];
 * dz [B*H*W][C] = dL/dz (not yet masked by the ReLU).  fused = 1: the fused attention head (C / 4 a power
 * of two <= 32), which stores neither z nor CBAM's output; fused = 0: bn_relu_fwd, cbam_fwd, head_fwd,
 * head_bwd, cbam_bwd.  sidx_out [B*H*W] / amax_out [B*C] (nullable, device int32): CBAM's two argmax
 * decisions.  elapsed_ms (nullable, host): the forward + backward is run a second time between two device
 * events and their distance stored (the first run warms up) */
cad_status cad_op_cbam_head(const float* y, int y_bf16, const float* scale, const float* shift, const float* cbam_params,
                            const float* head_w, const float* head_b, float max_depth, const float* dpred, int B, int H,
                            int W, int C, int fused, float* pred, float* dz, float* cbam_grads, float* head_grads,
                            int* sidx_out, int* amax_out, float* elapsed_ms, void* stream);
/* test hook: buffer of the last step ("cat<l>", "dcat<l>", "x<l>", "u<l>", "z<l>"; NHWC rows) -> host;
 * returns the element count (host NULL: count only) or -1 */
int64_t cad_geonet_debug_buffer(cad_geonet* h, const char* name, float* host, int64_t numel);

/* ---- inference export: depth renders, 16-bit depth, point clouds, PNG / PLY files.
 *   cad_exporter_range / _render / _image   DepthVisualizer::normalizeDepth, applyColormap and the panes of
 *                                   createComparisonViz, src/visualization/depth_viz.h:23-148 (and
 *                                   depth_visualizer.h), on the device instead of through cv::Mat
 *   cad_colormap_lut                cv::applyColorMap's tables (depth_viz.h:126-132), restated in integers
 *   cad_png_encode / cad_png_decode cv::imwrite / cv::imread of depth_viz.h:81, sunrgbd_loader.cpp:221-259
 *   cad_exporter_points, cad_ply_write, cad_hflip, cad_flip_mean
 *                                   new: no reference counterpart (the mirrored intrinsics of flip
 *                                   augmentation are applyHorizontalFlip's, sunrgbd_loader.cpp:416-430)
 * The device calls run on the caller's stream, allocate nothing, never synchronise and never copy to the
 * host; no floating-point atomics: an image's output is the same bits on every run, in whichever batch it
 * arrives, from 16-byte aligned or unaligned tensors. */

/* built-in colour tables, 256 x 3 bytes (r, g, b of index i), `/` floor division, clamped to [0, 255]:
 *   gray (i, i, i);   jet (383 - |4i - 765|, 383 - |4i - 510|, 383 - |4i - 255|);
 *   hot  (8i / 3, 8 max(i - 96, 0) / 3, max(0, 4 (i - 191) - 1)) */
#define CAD_CMAP_GRAY 0
#define CAD_CMAP_JET 1
#define CAD_CMAP_HOT 2
#define CAD_CMAP_CUSTOM 3 /* the table of cad_exporter_set_lut */
/* host only (no device): name "gray" | "jet" | "hot" -> out768; another name: CAD_ERR_INVALID */
cad_status cad_colormap_lut(const char* name, uint8_t* out768);

typedef struct cad_exporter cad_exporter;
/* owns every workspace (range table and partials, tile counts and scan space, the colour tables) for up to
 * max_batch images of H x W.  Arguments are checked before any device call. */
cad_status cad_exporter_create(int max_batch, int H, int W, int device, cad_exporter** out);
void cad_exporter_destroy(cad_exporter* e);
/* a caller's 768-byte table into the CAD_CMAP_CUSTOM slot (one synchronous upload) */
cad_status cad_exporter_set_lut(cad_exporter* e, const uint8_t* lut768);
/* per image (min, max) of v = sub ? |depth - sub| : depth over its valid pixels — isfinite(v), depth > 0
 * (and sub > 0), mask != 0 — into the exporter's range table and, when out != NULL, into out (device, B x 2
 * floats); (0, 0) without a valid pixel.  depth, sub: (B,1,H,W) device fp32; mask: B*H*W device bytes;
 * sub and mask nullable. */
cad_status cad_exporter_range(cad_exporter* e, const float* depth, const float* sub, const uint8_t* mask, int B, float* out,
                              void* stream);
typedef struct {
    int colormap;          /* CAD_CMAP_* */
    int fixed_range;       /* 0: each image's (lo, hi) from the range table (the last cad_exporter_range); 1: lo, hi */
    float lo, hi;
    uint8_t invalid[3];    /* colour of invalid pixels */
    int64_t row_stride;    /* destination pixels per row; 0: W */
    int64_t col_offset;    /* the pane's first column inside a destination row */
    int64_t image_stride;  /* destination pixels between images; 0: H * row_stride */
    float units_per_metre; /* of the 16-bit output: 1000 = SUN RGB-D's depth PNGs */
} cad_render_opts;
/* one pass over depth, two nullable outputs.  rgb_out: RGB8 HWC, pixel = LUT[idx] with t = (v - lo) / (hi - lo)
 * (fp32 subtract, subtract, IEEE divide) clamped to [0, 1], idx = rintf(t * 255) (half to even); hi - lo < 1e-6:
 * idx 0; invalid pixels (cad_exporter_range's rule): opts->invalid.  u16_out: (B,H,W) uint16,
 * rintf(depth * units_per_metre) as one fp32 multiply, clamped to [0, 65535]; non-finite or depth <= 0: 0
 * (sub and mask do not apply). */
cad_status cad_exporter_render(cad_exporter* e, const float* depth, const float* sub, const uint8_t* mask, int B,
                               const cad_render_opts* opts, uint8_t* rgb_out, uint16_t* u16_out, void* stream);
/* rgb (B,3,H,W) fp32 -> RGB8 HWC pane, rintf(clamp(c, 0, 1) * 255); opts' strides and offset as above */
cad_status cad_exporter_image(cad_exporter* e, const float* rgb, int B, const cad_render_opts* opts, uint8_t* rgb_out,
                              void* stream);
/* surface normals of depth (B,1,H,W) from K (B,3,3) (the closed form of "geometric evaluation") -> RGB8 HWC
 * pane, (r, g, b) = rintf(255 ((n_x + 1) / 2, (1 - n_y) / 2, (1 - n_z) / 2)): a frontal wall is (128, 128, 255).
 * A pixel is valid when it and its four neighbours are (cad_exporter_range's rule: finite, depth > 0,
 * mask != 0); the others, the image border included, are opts->invalid.  opts' strides and offset as above. */
cad_status cad_exporter_normals(cad_exporter* e, const float* depth, const float* K, const uint8_t* mask, int B,
                                const cad_render_opts* opts, uint8_t* rgb_out, void* stream);
/* point cloud: pixel (y, x) of image b is emitted iff y % stride == 0, x % stride == 0, isfinite(Z),
 * min_depth < Z < max_depth (strict) and mask != 0; its 16-byte record {float X, Y, Z; uint8 r, g, b, a} has
 * X = (x - cx) / fx * Z, Y = (y - cy) / fy * Z (fp32 subtract, divide, multiply), Z the depth's bits,
 * r g b = rintf(clamp(c, 0, 1) * 255) from rgb (B,3,H,W) or 255 without it, a = 255.  Records are in
 * row-major pixel order; image b's start at records + b * cap * 16, cap = ceil(H/stride) * ceil(W/stride)
 * (16-byte aligned, B * cap records); counts: device int32[B].  Bytes past an image's count stay untouched.
 * K: (B,3,3) device.  rgb and mask nullable. */
cad_status cad_exporter_points(cad_exporter* e, const float* depth, const float* K, const float* rgb, const uint8_t* mask,
                               int B, int stride, float min_depth, float max_depth, void* records, int32_t* counts,
                               void* stream);
/* flip test-time augmentation: out[p][y][x] = in[p][y][W-1-x] (out must not overlap in), and
 * out[p][y][x] = 0.5f * (a[p][y][x] + b[p][y][W-1-x]) (out may be a); planes * H * W < 2^31 */
cad_status cad_hflip(const float* in, float* out, int64_t planes, int H, int W, void* stream);
cad_status cad_flip_mean(const float* a, const float* b, float* out, int64_t planes, int H, int W, void* stream);

/* host only.  PNG: non-interlaced, channels 1 (gray) or 3 (RGB), bits 8 (uint8 samples) or 16 (host-order
 * uint16 samples, stored big-endian), h x w x channels samples in row-major order.  out == NULL: *size = an
 * upper bound of the file size; else the file is written into out (cap bytes) and *size = its length. */
cad_status cad_png_encode(const void* pixels, int h, int w, int channels, int bits, uint8_t* out, int64_t cap, int64_t* size);
/* the loader's PNG decoder on a file held in memory: 8- or 16-bit gray, gray + alpha, RGB, RGBA, 8-bit
 * palette (as RGB); samples as above into out (cap bytes; out == NULL: dimensions only) */
cad_status cad_png_decode(const uint8_t* data, int64_t size, void* out, int64_t cap, int* height, int* width, int* channels,
                          int* bits);
/* binary_little_endian 1.0 PLY: properties float x y z, uchar red green blue alpha; the body is the n x 16
 * record bytes of cad_exporter_points (host copy) */
cad_status cad_ply_write(const char* path, const void* records, int64_t n);

/* ---- TensorBoard event files (host only, csrc/host/tfevents.cpp): what the reference sends through
 * tensorboard_logger_v2.h -> scripts/tensorboard_writer.py, written natively.
 * File: <logdir>/events.out.tfevents.<unix seconds>.<hostname>.<pid>.<k>, k a per-process counter (0 for the
 * first writer), the directory created; every writer opens a new file and never appends to an old one.
 * Record: uint64 LE length, uint32 masked CRC-32C of those 8 bytes, payload, uint32 masked CRC-32C of the
 * payload; mask(c) = ((c >> 15 | c << 17) + 0xa282ead8) mod 2^32.  Payloads are hand-encoded protobuf wire
 * format (Event / Summary / HistogramProto / TensorProto and the text, custom_scalars and hparams plugin
 * messages).  The file-version, scalar, text, custom_scalars and hparams records are byte for byte what
 * TensorBoard's own writer produces for the same content (pinned by the files under tests/golden/tfevents);
 * histogram and image records are valid for every parser but not pinned to its bytes (a proto3 serializer
 * leaves out a statistic that is 0.0, cad_tb_histogram always writes all five).  The first record is
 * Event{wall_time, file_version "brain.Event:2", source_metadata}; a step of 0 is left out as proto3 does. */
uint32_t cad_crc32c(const void* data, int64_t size);          /* Castagnoli; "123456789" -> 0xE3069283 */
uint32_t cad_crc32c_masked(const void* data, int64_t size);
typedef struct cad_tb_writer cad_tb_writer;
cad_status cad_tb_open(const char* logdir, cad_tb_writer** out);
void cad_tb_close(cad_tb_writer* w);                          /* flushes; also closes the hparams sub-run */
cad_status cad_tb_flush(cad_tb_writer* w);
const char* cad_tb_path(const cad_tb_writer* w);              /* the event file */
cad_status cad_tb_scalar(cad_tb_writer* w, const char* tag, float value, int64_t step);
/* stats: {min, max, num, sum, sum_squares}; limits: n right bucket edges; buckets: n counts (doubles) */
cad_status cad_tb_histogram(cad_tb_writer* w, const char* tag, int64_t step, const double stats[5], const double* limits,
                            const double* buckets, int n);
/* png: an encoded PNG (cad_png_encode); colorspace 3 = RGB, 1 = gray */
cad_status cad_tb_image(cad_tb_writer* w, const char* tag, int64_t step, int height, int width, int colorspace,
                        const void* png, int64_t bytes);
/* text plugin record under tag + "/text_summary" */
cad_status cad_tb_text(cad_tb_writer* w, const char* tag, int64_t step, const char* text);
/* custom-scalars layout: n rows (category, chart, tag) in display order; consecutive rows sharing a category
 * (and chart) are grouped; every chart is a multiline chart */
cad_status cad_tb_custom_scalars(cad_tb_writer* w, const char* const* categories, const char* const* charts,
                                 const char* const* tags, int n);
/* hyper-parameters (all float64, written sorted by name) into the sub-run <logdir>/<subdir> (NULL: the wall
 * clock as seconds.microseconds) with its own event file: _hparams_/experiment, _hparams_/session_start_info,
 * _hparams_/session_end_info, then the metric scalars at step 0 */
cad_status cad_tb_hparams(cad_tb_writer* w, const char* const* names, const double* values, int n,
                          const char* const* metric_tags, const float* metric_values, int nmetrics, const char* subdir);
const char* cad_tb_hparams_path(const cad_tb_writer* w);      /* the sub-run's event file ("" before cad_tb_hparams) */

/* TensorBoard's default histogram buckets as torch.utils.tensorboard builds them, in double: v = 1e-12;
 * while v < 1e20: append v, v *= 1.1; edges = the negated list reversed, 0, the list.  Returns the number of
 * edges (CAD_HIST_BINS + 1) and writes min(cap, that) of them (edges NULL: count only). */
#define CAD_HIST_BINS 1548
int cad_tb_default_bins(double* edges, int cap);
/* make_histogram's trimming (torch/utils/tensorboard/summary.py): first through last non-empty bucket plus one
 * empty bucket on the left; limits are the right edges.  counts: nbins; edges: nbins + 1; limits / buckets:
 * room for nbins + 1.  No non-empty bucket: the single pair (0, 0). */
cad_status cad_tb_trim_histogram(const uint32_t* counts, int nbins, const double* edges, double* limits, double* buckets,
                                 int* n);

/* ---- device histograms over a base pointer and a segment table (csrc/kernels/hist_kernels.hip).
 * Element i of a segment (base[offset + i], i < count) is counted iff i % period < keep.  Buckets are
 * cad_tb_default_bins' with numpy.histogram's rule on the values widened to double: half-open [a, b), the last
 * bin closed, values outside [edges[0], edges[last]] in no bucket, -0.0 with 0.0 in [0, 1e-12); the bucket is
 * found by exact integer comparison against "the smallest fp32 not below edge k".  Per segment
 * {num, min, max, sum, sum_squares, nonfinite}: non-finite values count in nonfinite only; num is the number
 * of counted finite values (in a bucket or not); sums are double (products formed in double), reduced in a
 * fixed order without floating-point atomics: a row is the same bits on every run.  num == 0: min = max = 0. */
typedef struct {
    int64_t offset, count, period, keep;
    /* optional second rule inside a period, for rows that are padded twice (a convolution row of `period` floats
     * whose first `keep` hold taps of inner_period channels, inner_keep of them real): with r = i % period the
     * element counts iff r < keep && r % inner_period < inner_keep.  0, 0: no inner rule. */
    int64_t inner_period, inner_keep;
} cad_hist_segment;
#define CAD_HIST_STATS 6
typedef struct cad_hist cad_hist;
cad_status cad_hist_create(const cad_hist_segment* segments, int nseg, int device, cad_hist** out);
void cad_hist_destroy(cad_hist* h);
int cad_hist_num_segments(const cad_hist* h);
/* asynchronous on stream, allocates nothing, never synchronises, clears its own bins */
cad_status cad_hist_run(cad_hist* h, const float* base, void* stream);
/* one synchronous copy of the last run: stats [nseg][CAD_HIST_STATS] doubles, counts [nseg][CAD_HIST_BINS]
 * (either nullable) */
cad_status cad_hist_read(cad_hist* h, double* stats, uint32_t* counts);
/* the pass over a U-Net's parameter (which = 0) or gradient (1) slab: one segment per named_parameters()
 * entry, in that order, counting exactly the values cad_unet_get_tensor / cad_unet_get_grad return (the
 * zero-padded input channels of enc1.conv1 and the alignment gaps are skipped).  The handle is created on
 * the first call and owned by the model; read it with cad_hist_read. */
cad_status cad_unet_histograms(cad_unet* h, int which, void* stream, cad_hist** hist);
/* the same for the ResNet-50-encoder U-Net and the geometry-aware networks: one slab, one segment per
 * named_parameters() entry (a ResNet convolution row is padded to a multiple of 8 floats and the stem's
 * three input channels to four: both skipped) */
cad_status cad_resunet_histograms(cad_resunet* h, int which, void* stream, cad_hist** hist);
cad_status cad_geonet_histograms(cad_geonet* h, int which, void* stream, cad_hist** hist);

#ifdef __cplusplus
}
#endif
#endif /* CAD_CAD_H */
