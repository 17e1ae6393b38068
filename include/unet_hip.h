/* unet_hip.h — C ABI of libunet_hip.so, the MI355X (gfx950) U-Net training path.
 *
 * Drop-in boundary for the reference's hot path (SwagMag1213/image-segmentation-
 * project, /root/reference).  The reference is pure Python over PyTorch, so its
 * "FFI" is the Python API; each entry point below replaces the compute under one
 * reference call (file:line in /root/reference):
 *
 *   unet_forward         UNetWithBackbone.forward (advanced_models.py:264-357),
 *                        resnet34 encoder (:72-100), use_attention=False
 *   unet_backward        loss.backward() through that graph (train.py:48)
 *   unet_bucket_wait     DDP gradient reduction insertion point between
 *                        loss.backward() and optimizer.step() (train.py:48-49)
 *   unet_loss_forward    BCELoss / DiceLoss / ComboLoss forward (losses.py:13-37,161-171)
 *   unet_loss_backward   their gradient wrt the logits
 *   unet_mask_metrics    calculate_metrics tp/fp/fn/tn counts (utils.py:120-151)
 *   unet_softmax_loss_forward / _backward   softmax CE / multi-class Dice on integer label maps
 *   unet_confusion_matrix                    argmax confusion matrix of the same inputs
 *   unet_label_instances connected-component instances of a predicted mask (scipy.ndimage
 *                        definitions; the reference's host-side post-processing is not ported)
 *   unet_distance_transform / unet_grow_instances   exact Euclidean distance and nearest-site
 *                        transform of masks and label maps, nearest-label growth of instances
 *   unet_geodesic_grow / unet_watershed   growth of a label map along allowed pixels (shortest
 *                        paths) and marker watershed by levels; these synchronise with the host
 *   unet_match_instances IoU tables of predicted instances against a ground truth label map
 *   unet_measure_instances / unet_select_instances   per-instance shape, contact and intensity
 *                        tables of a label map; dropping and renumbering of instances
 *   unet_link_instances  track ids, lineage table and relabelled stack of a sequence of label
 *                        maps (time lapse or z-stack) by mutually best IoU partners
 *   unet_two_nearest_instances / unet_border_weights / unet_boundary_targets   training targets
 *                        for touching cells from a ground-truth instance map; unet_softmax_loss_*_pw
 *                        take the weight map as per-pixel weights of the cross-entropy
 *   unet_adam_step       optimizer.step() of torch.optim.Adam(model.parameters(),
 *                        lr, weight_decay) (train.py:49,331-335)
 *   unet_conv_* / unet_maxpool_* / unet_bn_*   single ops of the graph above
 *                        (torchvision BasicBlock, advanced_models.py:197-205) for tests
 *
 * Conventions: every pointer is a DEVICE pointer owned by the caller (PyTorch's
 * caching allocator); the library never allocates or frees on the hot path.
 * Activations are bf16 NHWC; parameters / grads fp32 in torch layouts.  All work
 * is enqueued asynchronously on the given hipStream_t.  Every function returns
 * 0 on success or a non-zero hipError_t-style code; unet_last_error() gives a
 * thread-local message.  No C++ exception crosses the ABI.
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct unet_plan unet_plan;

typedef struct unet_config {
  int N, H, W;       /* batch and input size (H, W multiples of 32)            */
  int width;         /* channel multiplier: 1 = resnet34 U-Net (64..512)       */
  int n_classes;     /* 1..16: conv_final's output channels (advanced_models.py:160), */
                     /*    independent sigmoid channels; logits are [N,n_classes,H,W]  */
  float bn_eps;      /* 1e-5  (torch.nn.BatchNorm2d default)                   */
  float bn_momentum; /* 0.1                                                    */
  int attention;     /* 1: AttentionGate + ChannelAttention decoder            */
                     /*    (use_attention=True, advanced_models.py:7-61,163-172) */
  int backbone;      /* 34: resnet34 (BasicBlock encoder, advanced_models.py:72-100);     */
                     /* 50: resnet50 (Bottleneck encoder 256..2048, :102-130,158-159)     */
  int fp8;           /* 1: forward convs with >= 128 input channels in fp8 e4m3 (per-tensor */
                     /*    delayed scaling, block-scaled MFMA); backward stays bf16.        */
                     /*    Build extension for BASELINE configs[4] (Wide fp8); resnet34,   */
                     /*    no attention.  The reference trains in fp32 only.               */
} unet_config;

const char* unet_last_error(void);
const char* unet_version(void);

/* ---- plan: layer graph, parameter table, workspace layout ---- */
int unet_plan_create(const unet_config* cfg, unet_plan** out);
void unet_plan_destroy(unet_plan* p);
int64_t unet_plan_workspace_bytes(const unet_plan* p);
int unet_plan_num_params(const unet_plan* p);
int unet_plan_param_name(const unet_plan* p, int i, char* buf, int buflen);
int unet_plan_param_shape(const unet_plan* p, int i, int64_t shape[4]); /* returns ndim */
int64_t unet_plan_param_offset(const unet_plan* p, int i);             /* in flat grads */
int64_t unet_plan_grad_numel(const unet_plan* p);
int unet_plan_num_bn(const unet_plan* p);
int unet_plan_num_buckets(const unet_plan* p);
int unet_plan_bucket_range(const unet_plan* p, int b, int64_t* begin, int64_t* end);
double unet_plan_flops(const unet_plan* p, int training); /* algorithmic FLOPs per step */
/* named workspace views (tests): info = {byte offset, ld, C, H, W} of a bf16 NHWC tensor */
int unet_plan_num_tensors(const unet_plan* p);
int unet_plan_tensor_info(const unet_plan* p, int i, char* name, int namelen, int64_t info[5]);

/* params[i]: fp32 tensors in unet_plan_param_name order (== reference
 * state_dict parameter order); buffers[3*k+0/1/2]: running_mean/var (fp32) and
 * num_batches_tracked (int64) of BN k in named_buffers order.  A training
 * forward updates the running statistics and adds 1 to num_batches_tracked,
 * as torch.nn.BatchNorm2d.train() does.
 * image: [N,1,H,W] fp32; logits: [N, n_classes, H, W] fp32 (NCHW, contiguous). */
int unet_forward(unet_plan* p, const float* image, const float* const* params, float* const* buffers,
                 void* workspace, float* logits, int training, hipStream_t stream);
/* dlogits: [N, n_classes, H, W] fp32, the logits' layout.
 * grads: flat fp32 [unet_plan_grad_numel], param i at unet_plan_param_offset(i).
 * Ordering contract: unet_backward differentiates the LAST training
 * unet_forward of the same plan and workspace (its saved activations and BN
 * statistics).  A training forward also zeroes the backward's accumulators
 * inside its first launch; if the workspace differs, or an eval forward came in
 * between, unet_backward zeroes them itself (one memset), so a mismatched call
 * order is never silently wrong about the accumulators -- but the gradients
 * are only meaningful for the pairing above.
 * unet_plan_create queries the current device's CU count (HIP runtime init);
 * use the plan on that device. */
int unet_backward(unet_plan* p, const float* image, const float* dlogits, const float* const* params,
                  void* workspace, float* grads, hipStream_t stream);
/* record one hipEvent per gradient bucket in every unet_backward (DDP overlap) */
int unet_plan_use_bucket_events(unet_plan* p, int on);
/* make `waiter` wait until bucket b of the last unet_backward is final */
int unet_bucket_wait(unet_plan* p, int bucket, hipStream_t waiter);
/* per-launch hipEvent profiler: enable (clears records), then report lines
 * "name\tms\tflops\n" for every launch since; returns bytes needed (incl. NUL). */
/* In-kernel phase timing of the conv launches (a debug aid; the stamps are
 * written only by a library built with -DUNET_TIMING, `make timing`): enable
 * zeroes a device buffer of kTimLaunches x 1024 blocks x 32 u64 stamps and gives
 * every following conv launch of the plan the next slot; read copies the slots
 * used so far to `host` (max_launches slots) and the launch names (one per
 * line) to `names`, and returns the number of slots used. */
int unet_timing_enable(unet_plan* p, int on);
int64_t unet_timing_read(unet_plan* p, unsigned long long* host, int64_t max_launches, char* names, int64_t nlen);
int unet_profile_enable(unet_plan* p, int on);
int unet_profile_report(unet_plan* p, char* buf, int64_t buflen);

/* ---- loss + metrics (kind: 0 bce, 1 dice, 2 combo) ---- */
/* sums8: exactly 8 doubles out, the sums (bce, sigma*y, sigma, y, tp, fp, fn, tn).
 * scratch: caller-owned device scratch of scratch_len >= UNET_LOSS_SCRATCH_LEN
 * doubles for the per-block partials, which the library reduces in a fixed
 * order (no atomics: the sums are bit-reproducible); a shorter or null scratch
 * is rejected with an error before anything is launched.  Nothing needs to be
 * zeroed beforehand.  (Round 5 wrote the partials behind sums8; the separate,
 * length-checked scratch makes an 8-double sums8 buffer safe again.) */
#define UNET_LOSS_SCRATCH_LEN (8 * 256)
int unet_loss_forward(const float* logits, const float* target, int64_t n, int kind, float alpha,
                      float smooth, double* sums8, double* scratch, int64_t scratch_len, float* loss_out,
                      hipStream_t stream);
int unet_loss_backward(const float* logits, const float* target, int64_t n, int kind, float alpha,
                       float smooth, const double* sums8, const float* grad_scale, float* dlogits,
                       hipStream_t stream);
/* sums8[4..8) = tp, fp, fn, tn.  values_are_prob=0: logits (mask = sigmoid>0.5
 * evaluated bit-exactly as logit >= 0x33C00001); 1: probabilities (p > 0.5).
 * scratch / scratch_len as for unet_loss_forward. */
int unet_mask_metrics(const float* values, const float* target, int64_t n, int values_are_prob,
                      double* sums8, double* scratch, int64_t scratch_len, hipStream_t stream);

/* ---- softmax multi-class loss + confusion matrix (mutually exclusive classes) ---- */
/* logits: fp32, contiguous NCHW [N][K][HW] (the U-Net's multi-channel output),
 *   K = 2..UNET_SOFTMAX_MAX_CLASSES.  Any 4-B aligned base is accepted: the
 *   gradient and confusion kernels use 16-B accesses when HW % 4 == 0, logits
 *   (and dlogits) are 16-B aligned and labels are aligned to 4 B (uint8) / 16 B
 *   (int32, int64), and scalar ones otherwise; the results are bit-identical.
 * labels: one integer per pixel, [N][HW], of label_dtype 0 = uint8, 1 = int32,
 *   2 = int64 (read as they are: no conversion pass).  A pixel is valid when
 *   0 <= label < K and label != ignore_index.  A label equal to ignore_index is
 *   ignored; any other label outside [0, K) is ignored too and counted in
 *   sums[3], so bad data can be detected (nothing faults).
 * class_weights: K floats on the device, or null (all 1).  Not allowed with kind 1.
 * kind: 0 CE   = ce_num / w_den  (F.cross_entropy(weight, ignore_index, "mean"))
 *       1 Dice = 1 - (1/K) sum_k (2 I_k + smooth) / (P_k + Y_k + smooth): one
 *                global Dice per class over the valid pixels of the batch
 *       2 alpha * CE + (1 - alpha) * Dice
 *   With no valid pixel (w_den == 0) CE contributes 0 and its gradient is 0
 *   (torch returns NaN there, which would poison a replayed optimizer step).
 * sums: UNET_SOFTMAX_SUMS_LEN doubles out:
 *   [0] ce_num = sum w[y] nll   [1] w_den = sum w[y]   [2] valid pixels
 *   [3] labels outside [0, K) other than ignore_index
 *   [4 + k] I_k = sum p_k [y = k]   [20 + k] P_k = sum p_k   [36 + k] Y_k = sum [y = k]
 *   (k < K; the entries of k >= K are written as 0), all over valid pixels.
 * scratch: caller-owned device memory of scratch_len >= UNET_SOFTMAX_SCRATCH_LEN
 *   doubles (8-B aligned) for per-block partials, added in block order by a
 *   second launch: no atomics on memory, the results are bit-reproducible.
 *   Nothing needs zeroing.  The sums kernel uses at most UNET_SOFTMAX_MAX_BLOCKS
 *   blocks of UNET_SOFTMAX_THREADS threads, one pixel per thread and stride.
 * Every call validates its arguments (K, label_dtype, kind, null pointers,
 * scratch_len, N / HW > 0, weights with kind 1) before launching anything, and
 * allocates and synchronises nothing: all three are graph-capturable. */
#define UNET_SOFTMAX_MAX_CLASSES 16
#define UNET_SOFTMAX_SUMS_LEN 52
#define UNET_SOFTMAX_MAX_BLOCKS 1024
#define UNET_SOFTMAX_THREADS 256
#define UNET_SOFTMAX_SCRATCH_LEN (UNET_SOFTMAX_SUMS_LEN * UNET_SOFTMAX_MAX_BLOCKS)
int unet_softmax_loss_forward(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                              const float* class_weights, int ignore_index, int kind, float alpha, float smooth,
                              double* sums, double* scratch, int64_t scratch_len, float* loss_out,
                              hipStream_t stream);
/* dlogits [N][K][HW] = grad_scale[0] * dL/dlogits (grad_scale: device scalar, or
 * null for 1), from the sums of the forward call on the same inputs.  Every
 * element is written; all channels of an ignored pixel get an exact 0. */
int unet_softmax_loss_backward(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                               const float* class_weights, int ignore_index, int kind, float alpha, float smooth,
                               const double* sums, const float* grad_scale, float* dlogits, hipStream_t stream);
/* The same pair with per-pixel weights: pixel_weights is float [N][HW] on the
 * device (any 4-B aligned base; 16-B accesses in the gradient kernel under the
 * condition above when it is 16-B aligned too), or null.  A valid pixel then
 * weighs class_weights[y] * pixel_weights[p] in ce_num, w_den and the CE part of
 * the gradient; the valid / invalid counts, the Dice sums, the Dice gradient and
 * the w_den == 0 rule are unchanged.  Weights must be finite and >= 0 (not
 * checked).  Not allowed with kind 1.  With pixel_weights null both return the
 * bits of the entries above. */
int unet_softmax_loss_forward_pw(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                                 const float* class_weights, const float* pixel_weights, int ignore_index, int kind,
                                 float alpha, float smooth, double* sums, double* scratch, int64_t scratch_len,
                                 float* loss_out, hipStream_t stream);
int unet_softmax_loss_backward_pw(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                                  const float* class_weights, const float* pixel_weights, int ignore_index, int kind,
                                  float alpha, float smooth, const double* sums, const float* grad_scale,
                                  float* dlogits, hipStream_t stream);
/* cm: int64 [K][K] out, cm[t][p] = valid pixels of true class t whose first
 * maximum logit is channel p (lowest index on ties).  Exact integer counts. */
int unet_confusion_matrix(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                          int ignore_index, long long* cm, double* scratch, int64_t scratch_len,
                          hipStream_t stream);

/* ---- optimizer ---- */
/* One Adam step (coupled L2 weight decay, torch.optim.Adam semantics) over n
 * fp32 elements of four flat buffers.  step_coef[3] is device memory:
 * step_coef[0] is the step count (incremented on device, so the call is
 * graph-capturable) when advance_step != 0, and [1], [2] then receive
 * step_size = lr/(1-b1^t) and sqrt(1-b2^t); advance_step = 0 reuses them
 * (several slices updated in one optimizer step).  exp_avg / exp_avg_sq must
 * be zero before the first step. */
int unet_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_coef,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int advance_step, hipStream_t stream);

/* ---- DDP gradient reduction over RCCL (non-Python hosts) ----
 * The reference trains in one process; these sit at its DDP insertion point,
 * between loss.backward() and optimizer.step() (train.py:48-49), and replace
 * torch.distributed for a C / C++ / FFI host.  RCCL (the
 * process's own, else /opt/rocm's librccl.so.1) is resolved at run time.
 * Rank 0 calls unet_allreduce_unique_id and ships the UNET_UNIQUE_ID_BYTES blob
 * to every rank out of band; each rank (one process per GPU, its device
 * current) calls unet_allreduce_init -- collective over the world.
 * unet_allreduce_bucket: mean all-reduce, in place in the flat fp32 gradient
 * buffer, of bucket `bucket` (unet_plan_bucket_range) of the last
 * unet_backward, enqueued on comm_stream after that bucket's hipEvent when
 * unet_plan_use_bucket_events(p, 1) was on during that backward (the
 * all-reduce then overlaps the rest of the backward); otherwise the caller
 * orders comm_stream after the backward.  The caller orders its compute
 * stream after comm_stream before optimizer.step().  Graph-capturable. */
#define UNET_UNIQUE_ID_BYTES 128
typedef struct unet_comm unet_comm;
int unet_allreduce_unique_id(void* id);
int unet_allreduce_init(const void* id, int rank, int world, unet_comm** out);
void unet_allreduce_destroy(unet_comm* c);
int unet_allreduce_bucket(unet_comm* c, unet_plan* p, float* grads, int bucket, hipStream_t comm_stream);
/* mean all-reduce of n floats in place (any flat buffer) */
int unet_allreduce_mean(unet_comm* c, float* buf, int64_t n, hipStream_t stream);

/* ---- bf16 gradient exchange (opt-in DDP compression) ----
 * Replace nothing in the reference (it trains in one process); they sit at
 * the DDP insertion point train.py:48-49, around each bucket's all-reduce:
 * dst[i] = bf16_rne(src[i]) before it, dst[i] = float(src[i]) * scale after
 * it (scale = 1/world for a SUM collective).  n elements; any alignment (16-B
 * aligned buffers take the 8-wide path). */
int unet_grad_to_bf16(const float* src, void* dst, int64_t n, hipStream_t stream);
int unet_grad_from_bf16(const void* src, float* dst, int64_t n, float scale, hipStream_t stream);

/* ---- single ops (tests / custom graphs) ---- */
/* mode 0: conv  y = conv(x, w) [stride, pad]           (w packed [Cout][R][S][C])
 * mode 1: transposed gather (conv dgrad / ConvTranspose2d forward)
 * mode 2: 7x7 stem on an fp32 single-channel image     (w packed [64][64] per
 *         64-channel output group; Cout % 64 == 0, any other width is refused
 *         with a message and nothing is launched) */
int unet_conv_fwd(const void* x, int ldx, const void* w, void* y, int ldy, const float* bias,
                  const void* addend, int ldadd, double* stats, int N, int H, int W, int C, int P,
                  int Q, int Cout, int R, int S, int stride, int pad, int mode, hipStream_t stream);
/* stem != 0 (here and in unet_conv_wgrad_slab): the 7x7 stem's weight gradient,
 * x the fp32 image; Cout % 64 == 0, refused like unet_conv_fwd mode 2 otherwise. */
int unet_conv_wgrad(const void* dy, int lddy, const void* x, int ldx, float* dw_acc, int N, int H,
                    int W, int C, int P, int Q, int Cout, int R, int S, int stride, int pad, int stem,
                    hipStream_t stream);
/* the same with the executor's deterministic split-K: partials in the caller's
 * 16-B aligned `slab` scratch, summed in a fixed split order; every element of
 * dw is WRITTEN (no zeroing needed, bit-reproducible).  The convT form computes
 * ConvTranspose2d(k2, s2) dW [Ci][Co][2][2]-packed as [Ci][4*Co] from
 * x [N,H,W,Ci] and dy [N,2H,2W,Co]. */
int unet_conv_wgrad_slab(const void* dy, int lddy, const void* x, int ldx, float* dw, void* slab,
                         int64_t slab_bytes, int N, int H, int W, int C, int P, int Q, int Cout, int R,
                         int S, int stride, int pad, int stem, hipStream_t stream);
int unet_convt_wgrad_slab(const void* dy, int lddy, const void* x, int ldx, float* dw, void* slab,
                          int64_t slab_bytes, int N, int H, int W, int Ci, int Co, hipStream_t stream);
/* The full-line halo conv (conv3x3_fl_kernel: every 3x3 / stride-1 conv with
 * C >= 128 that fills the chip, i.e. the enc2 / enc3 BasicBlocks and decoder4 /
 * decoder3 of the reference, advanced_models.py:84-87,197-205) as a single op.
 * C % 128 == 0, Cout % 64 == 0, H % 16 == 0, W % 16 == 0 (here C = the op's
 * input channels, Cout its output channels).  wch: the chunk-major pack of
 * unet_pack_weight kind 5 (mode 0, forward weight [Cout][C][3][3]) or kind 6
 * (mode 1, data gradient of a forward conv whose weight is [C][Cout][3][3]).
 * mode 0: y = conv3x3(x) (+bias)(+addend); stats != null: BN sums of y into
 *   stats[16][2][Cout] (fp64 atomics, caller zeroes).
 * mode 1: y = conv3x3_transpose(x) (+addend); bsums != null: the fused BN(+ReLU)
 *   backward epilogue: y := dZ = dA * (act > 0) and bsums[16][2][Cout] +=
 *   (sum dZ, sum dZ * (yraw - mean) * invstd); yraw2 != null (downsample blocks,
 *   two BNs): bsums2[16][1][Cout] (the second half of each replica) +=
 *   sum dZ * (yraw2 - mean2) * invstd2.
 * grid: 0 = the production persistent grid (one block per CU); > 0 caps it
 * (rounded down to a multiple of Cout / 64) so blocks run several work items. */
int unet_conv3x3_fl(const void* x, int ldx, const void* wch, void* y, int ldy, const float* bias,
                    const void* addend, int ldadd, double* stats, const void* act, int ldact, const void* yraw,
                    int ldyraw, const float* mean, const float* invstd, const void* yraw2, int ldyraw2,
                    const float* mean2, const float* invstd2, double* bsums, double* bsums2, int N, int H,
                    int W, int C, int Cout, int mode, int grid, hipStream_t stream);
/* The weight-stationary ConvTranspose2d(k2, s2) (convt2x2_kernel: the narrow
 * decoder up-convs, advanced_models.py:96-99 upconv2 / upconv1, applied at
 * :305,315) as a single op.  N, H, W = the INPUT-resolution grid; (Ci, Co) in
 * {(64, 32), (64, 64), (128, 64)}; N*H*W % 32 == 0; 16-B aligned x / w, 8-B
 * aligned y, ldx % 8 == 0, ldy % 4 == 0.
 * mode 0 (forward): x = X [N,H,W] (ld ldx >= Ci), w = unet_pack_weight kind 2
 *   of the [Ci][Co][2][2] weight, y = Y [N,2H,2W] (ld ldy) = convT(X) + bias.
 * mode 1 (data gradient): x = dY [N,2H,2W] (ld ldx >= Co), w = kind 3 pack,
 *   y = dX [N,H,W] (ld ldy); bsums != null: the fused BN(+ReLU) backward as
 *   unet_conv3x3_fl mode 1 (act, yraw, mean, invstd over Ci channels,
 *   bsums[16][2][Ci]); bias_acc != null: bias_acc[16][Co] += the bias
 *   gradient sum of dY (fp64, caller zeroes).
 * grid: 0 = the production persistent grid; > 0 caps it. */
int unet_convt2x2(const void* x, int ldx, const void* w, void* y, int ldy, const float* bias, const void* act,
                  int ldact, const void* yraw, int ldyraw, const float* mean, const float* invstd, double* bsums,
                  double* bias_acc, int N, int H, int W, int Ci, int Co, int mode, int grid, hipStream_t stream);
/* One conv launch with the WHOLE epilogue of the training / eval step, for
 * single-op tests: the launch the executor's conv forward (mode 0) or conv data
 * gradient (mode 1) would make, selected by the same dispatch.  The reference
 * ops underneath are the torchvision BasicBlock convs and the decoder convs
 * (advanced_models.py:72-100,197-205) with their BatchNorm2d folded in (eval) or
 * differentiated (training backward).
 * size = sizeof(unet_conv_ex_args) (checked).  A zero / null field switches the
 * feature off; inconsistent combinations are rejected with a message before
 * anything is launched, nothing is silently ignored.
 *   w: the standard pack (unet_pack_weight kind 0 forward / kind 1 data
 *      gradient); chunk_major != 0: the chunk-major pack (kind 5 / 6) and the
 *      launch is conv3x3_fl_kernel's (unet_conv3x3_fl's shape rules).
 *   N, H, W, C: the op's input grid and reduction channels (data gradient: dY);
 *   P, Q, Cout: its output grid and channels (data gradient: dX).
 *   mode 0: bias, addend, stats as unet_conv_fwd; gamma != null: the eval-mode
 *      BN fold y = act((conv + bias) * scale + shift [+ addend]), scale = gamma /
 *      sqrt(running_var + eps), shift = beta - running_mean * scale, act = ReLU
 *      when relu != 0; wds != null: the block's 1x1 / stride-2 downsample folded
 *      into this 3x3 / stride-2 forward, yds = conv1x1s2(x, wds) and its BN sums
 *      stats_ds from the same launch (an error where the launcher does not fold).
 *   mode 1: addend; bsums != null: the fused BN(+ReLU) backward as
 *      unet_conv3x3_fl mode 1 (act, yraw, mean, invstd; yraw2, mean2, invstd2,
 *      bsums2 for the two-BN form); x2 != null: the folded 1x1 / stride-2
 *      downsample data gradient, output pixels (2p, 2q) += x2[n,p,q,:C2] . w2
 *      (w2: kind-1 pack of the 1x1 weight); ysplit != null: output channels >=
 *      csplit go to ysplit[pix * ldysplit + co - csplit].
 *   grid_cap: 0 = the production grid; > 0 caps the grid of the kernels whose
 *      blocks walk several tiles, rounded down to a whole number of output-
 *      channel blocks and never below one tile slot: conv3x3_fl_kernel,
 *      conv3x3_ws2_kernel, conv3x3_ws_kernel, conv1x1_kernel and the forward
 *      conv3x3_hs_kernel.  The one-tile-per-block kernels have no grid to cap
 *      and launch their full grid whatever grid_cap says: the data-gradient
 *      conv3x3_hs_kernel, conv3x3s2_dgrad_kernel and the implicit GEMM
 *      conv_glds_kernel (unet_last_kernel_tag tells which one ran).
 * BN sums are only accumulated (no last-block finalisation), as in the other
 * single-op entries. */
typedef struct unet_conv_ex_args {
  int size, mode, chunk_major, grid_cap;
  int N, H, W, C, P, Q, Cout, R, S, stride, pad;
  int ldx, ldy, ldadd, ldact, ldyraw, ldyraw2, ldx2, C2, ldysplit, csplit, ldyds, relu;
  float eps;
  const void* x; const void* w; void* y;
  const float* bias; const void* addend; double* stats;
  const void* act; const void* yraw; const float* mean; const float* invstd;
  const void* yraw2; const float* mean2; const float* invstd2; double* bsums; double* bsums2;
  const void* x2; const void* w2;
  void* ysplit;
  const float* gamma; const float* beta; const float* running_mean; const float* running_var;
  const void* wds; void* yds; double* stats_ds;
} unet_conv_ex_args;
int unet_conv_ex(const unet_conv_ex_args* args, hipStream_t stream);
/* the kernel template instance of the calling thread's last conv launch
 * ("conv3x3_hs_kernel<2, 16, 8, true, false, false>", ...): tests assert which
 * instance the dispatch selected */
const char* unet_last_kernel_tag(void);
/* ---- attention decoder as single ops (advanced_models.py:7-61), for tests ----
 * One call runs ONE pass of the AttentionGate (psi conv1x1 + BN(1) + sigmoid +
 * x * psi, advanced_models.py:28-40) or of the ChannelAttention (avg / first-
 * argmax max pooling, the shared C -> Cr -> C MLP, sigmoid, channel scale,
 * advanced_models.py:56-61): the launch the executor makes for that pass, with
 * the launchers' own pass numbers.  size = sizeof(the struct) (checked).  The
 * caller owns every buffer, the accumulators included, and zeroes them; nothing
 * is allocated, zeroed or finalised here.  Everything is checked before any
 * launch (unet_last_error names the field): a null buffer that the chosen pass
 * reads or writes, a misaligned (16 B) bf16 buffer, a leading dimension that is
 * not a multiple of 8 or is smaller than the width, a refused width, a fused
 * BN backward that is only partly given.  Buffers and leading dimensions that
 * the chosen pass does not use are not examined, so one filled struct serves
 * all passes; the fused fields are examined in the pass that fuses (gate 3,
 * channel attention 5) and must be null / 0 to switch the fusion off.
 * bf16 tensors are NHWC with the given channel stride; pixel counts: npix = N H W,
 * HW per image.
 *
 * unet_att_gate_op; Fi, Fl in {8, 16, 32, 64, 128, 256, 512} (F / 8 lanes share
 * a pixel and must tile a wave), npix > 0, BN(1) count = npix.  Per pass:
 *   0  p = psi_b + s . psi_w.  Reads s (lds, Fi), psi_w [Fi], psi_b [1]; writes
 *      p [npix]; training: adds sum p, sum p^2 into pst [2] (fp64, ZEROED).
 *   1  psi = sigmoid(BN(p)), xatt = x * psi.  Reads p, x (ldx, Fl), gamma, beta
 *      [1], eps > 0; training: pst (of pass 0), writes save [2] = mean, invstd,
 *      updates run_mean / run_var [1] (momentum, unbiased variance) and nbt += 1
 *      (int64; null: untouched); eval: reads run_mean / run_var, touches neither
 *      pst, save, the running statistics nor nbt.  Writes psi [npix], xatt (ldxatt).
 *   2  Reads save, psi, p, x, dxatt (lddxatt); writes dxpsi = dxatt * psi
 *      (lddxpsi), dbnp [npix] = dZ of the BN, adds sum dZ, sum dZ phat into pbs
 *      [2] (fp64, ZEROED).
 *   3  Reads save, pbs (of pass 2), gamma, psi_w, p, dbnp, s; writes dS (lddS,
 *      Fi) = dp * psi_w, ggamma, gbeta [1]; adds the psi weight gradient into
 *      gpsi_acc (fp64 [16][Fi], ZEROED) and writes its replica sum to gpsi_w
 *      [Fi].  Fused (bsums != null; all of yraw, yraw2 (ldyraw, ldyraw2 >= Fi),
 *      mean, invstd, mean2, invstd2 [Fi], bsums, bsums2): dS is stored as dZ =
 *      dS * (s > 0) and sum dZ, sum dZ xhat go to rows 0, 1 of bsums, sum dZ
 *      xhat2 to row 1 of bsums2 (fp64 [16][2][Fi] replicas, ZEROED; row 0 of
 *      bsums2 is not written: both BNs share sum dZ).
 *
 * unet_ch_att_op; C in {8, 16, 32, 64, 128, 256, 512, 1024, 2048} (C / 8 must
 * divide 256), Cr > 0, N > 0, 0 < HW <= 2^32 - 2.  Per pass:
 *   0  Reads y (ldy); adds the per-(n, c) sums into psum (fp64 [N][C], ZEROED)
 *      and merges pkey (u64 [N][C], ZEROED) = (order-preserving key of the
 *      maximum) << 32 | (2^32 - 1 - first pixel index of the maximum).
 *   1  Reads psum, pkey, w1 [Cr][C], w2 [C][Cr]; writes am [N][2][C] = avg | max,
 *      h [N][2][Cr], gate [N][C].
 *   2  Reads y, gate; writes out = y * gate (ldo).
 *   3  Reads dout2 (lddo2), y; adds sum_hw dout2 * y into dgate (fp64 [N][C], ZEROED).
 *   4  Reads gate, dgate, w1, w2, h, am; writes dam [N][2][C]; adds the weight
 *      gradients into gw_acc (fp64 [16][2][C Cr]: fc.2 | fc.0, ZEROED) and writes
 *      their replica sums to gw2 [C][Cr], gw1 [Cr][C].
 *   5  Reads gate, dam, pkey, dout2; writes dout (lddo) = dout2 * gate + davg / HW
 *      + [hw == argmax] dmax.  Fused (bsums != null; all of act, yraw (ldact,
 *      ldyraw >= C), mean, invstd [C], bsums): dout is stored as dZ = dout *
 *      (act > 0) and sum dZ, sum dZ xhat go to bsums (fp64 [16][2][C], ZEROED). */
typedef struct unet_att_gate_args {
  int size, pass, training, Fi, Fl;
  int lds, ldx, ldxatt, lddxatt, lddxpsi, lddS, ldyraw, ldyraw2;
  float eps, momentum;
  int64_t npix;
  const void* s; const float* psi_w; const float* psi_b;
  float* p; float* psi; float* dbnp;
  double* pst; double* pbs; float* save;
  const float* gamma; const float* beta; float* run_mean; float* run_var; long long* nbt;
  const void* x; void* xatt; const void* dxatt; void* dxpsi; void* dS;
  float* gpsi_w; float* ggamma; float* gbeta; double* gpsi_acc;
  const void* yraw; const void* yraw2; const float* mean; const float* invstd;
  const float* mean2; const float* invstd2; double* bsums; double* bsums2;
} unet_att_gate_args;
int unet_att_gate_op(const unet_att_gate_args* args, hipStream_t stream);
typedef struct unet_ch_att_args {
  int size, pass, N, C, Cr;
  int ldy, ldo, lddo2, lddo, ldact, ldyraw;
  int64_t HW;
  const void* y; void* out;
  double* psum; unsigned long long* pkey;
  const float* w1; const float* w2;
  float* am; float* h; float* gate;
  const void* dout2; double* dgate; float* dam;
  float* gw1; float* gw2; double* gw_acc;
  void* dout;
  const void* act; const void* yraw; const float* mean; const float* invstd; double* bsums;
} unet_ch_att_args;
int unet_ch_att_op(const unet_ch_att_args* args, hipStream_t stream);
/* ---- fp8 e4m3 forward conv (BASELINE.json configs[4]; no reference counterpart:
 * the reference's convs are fp32 torch.nn.Conv2d, advanced_models.py:72-100) ----
 * state: 16-B scale state {amax prev (float bits), amax this step, e8m0 code,
 * pad}, zeroed before first use; calibrate flags: 1 measures amax before
 * quantizing, 2 ("frozen", eval forwards) quantizes with the scale in use and
 * does not accumulate this call's amax into the state.
 * q = sat448(v * 2^e) with 2 * amax_prev * 2^e <= 448, code = 127 - e.
 * unet_f8_quantize: bf16 [npix][C] (stride ld) -> dense e4m3 [npix][C].
 * unet_f8_pack_weight: fp32 [Co][Ci][R][S] -> e4m3 [Co][R][S][Ci].
 * unet_f8_roll: prev <- this step's amax (if any), this step's amax <- 0.
 * unet_conv_fwd_f8: y = conv(dequant(xq), dequant(wq)) (+bias, +addend, BN
 * sums) as unet_conv_fwd mode 0, K = R*S*C in e4m3 on the block-scaled MFMA. */
int unet_f8_quantize(const void* x, int ld, int C, int64_t npix, void* q, void* state, int calibrate,
                     hipStream_t stream);
int unet_f8_pack_weight(const float* w, int Co, int Ci, int R, int S, void* dst, void* state, int calibrate,
                        hipStream_t stream);
int unet_f8_roll(void* states, int n, hipStream_t stream);
int unet_conv_fwd_f8(const void* xq, int ldx, const void* wq, const void* state_x, const void* state_w, void* y,
                     int ldy, const float* bias, const void* addend, int ldadd, double* stats, int N, int H,
                     int W, int C, int P, int Q, int Cout, int R, int S, int stride, int pad,
                     hipStream_t stream);
/* tile configuration of the implicit-GEMM conv kernels: 0 automatic (default),
 * >0 a fixed configuration from the tuning table (scripts/tune_conv.py) */
int unet_set_conv_config(int cfg);
/* kind: 0 conv fwd, 1 conv dgrad, 2 convT fwd, 3 convT dgrad, 4 stem,
 * 5 conv fwd chunk-major [Ci/32][3*3][Co][32], 6 conv dgrad chunk-major
 * [Co/32][3*3][Ci][32] (3x3 only; unet_conv3x3_fl) */
int unet_pack_weight(const float* src, void* dst, int kind, int Co, int Ci, int R, int S,
                     hipStream_t stream);
/* kind: 0 conv [Co][R][S][Ci] -> [Co][Ci][R][S], 1 convT, 2 stem */
int unet_unpack_grad(const float* acc, float* dst, int kind, int Co, int Ci, int R, int S,
                     hipStream_t stream);
/* BatchNorm2d (+identity residual)(+ReLU) forward from fp64 sums
 * stats[16][2][C] (16 atomic-spreading replicas of (sum, sumsq) over npix
 * pixels, summed by the kernel; training) or running stats (eval); save[2C] =
 * batch mean | invstd.  res_mode: 0 none, 1 out = act(bn(y) + res).
 * unet_conv_fwd's `stats` output has the same [16][2][Cout] layout. */
int unet_bn_forward(const void* y, int ldy, void* out, int ldo, const void* res, int ldr, int res_mode,
                    const double* stats, const float* gamma, const float* beta, float* run_mean,
                    float* run_var, float* save, int64_t npix, int C, int relu, int training,
                    hipStream_t stream);
/* backward of out = relu(bn(y)[+res]): dY, optional dres (= dZ), dgamma/dbeta;
 * sums[16][2][C] must be zero on entry. */
int unet_bn_backward(const void* dout, int ldd, const void* out, int ldo, const void* y, int ldy,
                     const float* save, const float* gamma, double* sums, void* dy, int lddy, void* dres,
                     float* dgamma, float* dbeta, int64_t npix, int C, hipStream_t stream);
int unet_maxpool_fwd(const void* x, int ldx, void* y, uint8_t* idx, int N, int H, int W, int C,
                     hipStream_t stream);
int unet_maxpool_bwd(const void* dy, const uint8_t* idx, const void* addend, int ldadd, void* dx,
                     int N, int H, int W, int C, hipStream_t stream);

/* ---- on-GPU data pipeline (CellSegmentationDataset / CellAugmenter,
 * dataset.py:30-66,147-151) over N decoded uint8 frames [N][H][W] ---- */
/* cv2.resize(..., INTER_AREA) downscale to [N][oh][ow] uint8 (dataset.py:51) */
int unet_resize_area_u8(const uint8_t* src, int N, int H, int W, uint8_t* dst, int oh, int ow, hipStream_t stream);
/* cv2.resize(..., INTER_NEAREST) then (mask > 0) -> float32 [N][oh][ow] (dataset.py:52,61) */
int unet_mask_prep(const uint8_t* src, int N, int H, int W, float* dst, int oh, int ow, hipStream_t stream);
/* normalize_microscopy_image (dataset.py:30-42: 2/98 percentile clip, CLAHE(2.0, 8x8),
 * min-max) -> float32 [N][H][W]; normalize = 0: x / 255 (dataset.py:56) */
int unet_normalize_microscopy(const uint8_t* src, int N, int H, int W, float* dst, int normalize,
                              hipStream_t stream);
/* A.RandomRotate90 + A.VerticalFlip (dataset.py:147,150): dst[n] = vflip?(rot90(src[n], k[n]));
 * k, vflip: device int32 [N]; frames square when any k is odd */
int unet_rot90_vflip_u8(const uint8_t* src, int N, int H, int W, const int* k, const int* vflip, uint8_t* dst,
                        hipStream_t stream);

/* A.Affine (dataset.py:150-151; albumentations 2.0 -> cv2.warpAffine, fixed-point
 * INTER_LINEAR for images / INTER_NEAREST for masks, BORDER_CONSTANT 0) with the
 * pipeline's following A.VerticalFlip folded in.  minv: device double [N][6],
 * the dst -> src map (cv::invertAffineTransform of the forward matrix);
 * active[n] == 0 copies frame n (still flipped when vflip[n]). */
int unet_warp_affine_u8(const uint8_t* src, int N, int H, int W, const double* minv, const int* active,
                        const int* vflip, int nearest, uint8_t* dst, hipStream_t stream);
/* A.AdvancedBlur (dataset.py:153) = cv2.filter2D(img, -1, kernel), BORDER_REFLECT_101.
 * kernels: device float32 [N][7][7] (top-left ksize[n]^2 used, odd ksize <= 7);
 * ksize[n] == 0 copies frame n. */
int unet_filter2d_u8(const uint8_t* src, int N, int H, int W, const float* kernels, const int* ksize, uint8_t* dst,
                     hipStream_t stream);

/* ---- tiled whole-frame inference (no reference counterpart: the reference
 * predicts at the training size only) ----
 * Geometry shared by the three entries.  Square tiles T x T (1..UNET_TILE_MAX),
 * overlap 0 <= overlap <= T/2, stride S = T - overlap.  Per axis of length L:
 *   L <= T: one tile at origin -((T - L) / 2); the footprint outside the image
 *           reads BORDER_REFLECT_101 (L == 1: index 0);
 *   L >  T: n = ceil((L - T) / S) + 1 tiles at j S (j < n - 1) and L - T.
 * At most 3 tiles cover a pixel per axis.  Blend weight of footprint position
 * (u, v): the integer w1(u) w1(v), w1(i) = min(i + 1, T - i, overlap + 1).
 * tta: non-zero 8-bit mask of dihedral transforms d = k + 4 flip, "np.rot90(a, k),
 * then [::-1] if flip" (unet_rot90_vflip_u8's convention) applied to the tile
 * content; M = popcount(tta), m = rank of d among the set bits.  Flat tile index
 * t = ((n M + m) ny + jy) nx + jx, total = N M ny nx.  T need not be a multiple
 * of 32 (that is the model's constraint). */
#define UNET_TILE_MAX 1024        /* keeps the int32 weight sum <= 72 * 513^2 */
#define UNET_TILE_MAX_CLASSES 16
/* host-only: tiles per axis for the geometry above; error on T <= 0, overlap < 0 or > T/2 */
int unet_tile_grid(int H, int W, int T, int overlap, int* ny, int* nx);
/* image fp32 [N][H][W] -> tiles fp32 [count][T][T] for the flat indices
 * [first, first + count); slots with t >= total are written as zeros (the
 * zero-filled tail of a fixed-size batch).  16-B aligned `tiles` with T % 4 == 0
 * stores 16 B per lane. */
int unet_tile_gather(const float* image, int N, int H, int W, int T, int overlap, unsigned tta,
                     int64_t first, int64_t count, float* tiles, hipStream_t stream);
/* tile_logits fp32 [total][K][T][T] (K = 1..UNET_TILE_MAX_CLASSES) -> per image
 * pixel and class  out = (sum_t w_t v_t) / (float)(sum_t w_t)  over the covering
 * tiles in ascending t, v_t read back through the inverse transform; fp32
 * multiply and add kept apart, from 0; int32 weight sum; correctly rounded
 * division: bit-reproducible, no atomics.  Outputs of the one pass, each may be
 * null (not all three): logits fp32 [N][K][H][W]; mask uint8 [N][K][H][W] =
 * bits(out) >= 0x33C00001 for non-negative out (unet_mask_metrics' predicate);
 * labels uint8 [N][H][W] = argmax over K, lowest class on ties
 * (unet_confusion_matrix' rule; needs K >= 2). */
int unet_tile_blend(const float* tile_logits, int N, int K, int H, int W, int T, int overlap, unsigned tta,
                    float* logits, uint8_t* mask, uint8_t* labels, hipStream_t stream);

/* ---- instance labelling of masks (no reference counterpart; the definitions
 * are scipy.ndimage's: label, binary_fill_holes, find_objects) ----
 * mask uint8 [N][H][W]; a pixel is foreground when it is nonzero (fg_value = -1)
 * or equals fg_value (0..255).  Frames are independent.  H W < 2^31.
 * Order of operations: fill holes, then label, then min_area.
 *   fill_holes: a hole is a 4-connected component of the background that touches
 *     no frame edge (binary_fill_holes with its default structure); holes become
 *     foreground.  filled (nullable) receives the filled mask as 0 / 1; it is
 *     written only when fill_holes is set.
 *   labels int32 [N][H][W]: 0 for background, otherwise the instance id.  The
 *     instances of a frame (connectivity 1: 4-neighbour, 2: 8-neighbour) are
 *     numbered 1..counts[n] in raster order of their first pixel, i.e. by
 *     ascending minimum flat index y W + x (scipy.ndimage.label's numbering).
 *   min_area: components with fewer pixels are removed (label 0) before the
 *     numbering, so the ids stay consecutive.
 *   counts int32 [N]: the true number of instances of each frame, also above
 *     max_instances; the label map is always complete.
 *   stats (nullable) int64 [N][max_instances][UNET_INSTANCE_STATS]: row id - 1 =
 *     {area, sum_y, sum_x, y0, x0, y1, x1} with the half-open bounding box
 *     [y0, y1) x [x0, x1) of find_objects; centroid = sums / area.  Only ids <=
 *     max_instances have a row; rows at and beyond min(counts[n], max_instances)
 *     are zero.
 * Integer arithmetic throughout: the outputs are bit-reproducible.  The passes
 * work on tiles of UNET_INSTANCE_TILE_H x UNET_INSTANCE_TILE_W pixels.
 * workspace: at least unet_instances_workspace_bytes(N, H, W) bytes of device
 * memory, 256-B aligned as an allocator returns it; it need not be initialised
 * and holds nothing between calls.  A short workspace is an error with nothing
 * launched. */
#define UNET_INSTANCE_STATS 7
#define UNET_INSTANCE_TILE_H 32
#define UNET_INSTANCE_TILE_W 64
/* host only; 0 (with unet_last_error) for N, H, W <= 0 or H W >= 2^31 */
int64_t unet_instances_workspace_bytes(int N, int H, int W);
int unet_label_instances(const uint8_t* mask, int N, int H, int W,
                         int fg_value /* -1: nonzero; 0..255: == value */,
                         int connectivity /* 1: 4-neighbour, 2: 8-neighbour */,
                         int fill_holes, int min_area, int max_instances,
                         int32_t* labels, int32_t* counts /* [N] */,
                         int64_t* stats /* nullable */, uint8_t* filled /* nullable */,
                         void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- exact Euclidean distance transform, nearest-site transform and growth of
 * instances (no reference counterpart) ----
 * Frames [N][H][W] are independent.  H, W <= 32768 and H W < 2^31, so every
 * squared distance fits an int32.  A set of pixels of each frame are sites; for
 * every pixel p = (py, px):
 *   dist2[p]   = min over the sites s of (py - sy)^2 + (px - sx)^2, exact; 0 at a site.
 *   nearest[p] = the per-frame flat index sy W + sx of a site at that distance;
 *                among equidistant sites the smallest flat index; at a site its
 *                own index.
 *   A frame without a site gives dist2 = UNET_DISTANCE_NONE and nearest = -1.
 * dist2 equals rint(scipy.ndimage.distance_transform_edt(~site) ** 2); scipy's
 * return_indices chooses differently among equidistant sites.
 * unet_distance_transform: src is uint8 (src_dtype 0) or int32 (1).  A pixel is
 *   foreground when it is nonzero (fg_value = -1) or equals fg_value (>= 0; <=
 *   255 for uint8).  sites = 0: the pixels that are not foreground are the sites
 *   (the distance of every foreground pixel to the background, scipy's edt of
 *   the foreground); sites = 1: the foreground pixels are the sites.  dist2 and
 *   nearest are each optional, not both null.
 * unet_grow_instances: nearest-label growth (skimage.segmentation.expand_labels).
 *   The sites are the pixels with labels != 0.  out[p] = labels[p] where that is
 *   nonzero; otherwise labels[nearest[p]] when dist2[p] <= max_dist2 (max_dist2
 *   < 0: no limit) and, if within is given, p is allowed (within[p] nonzero for
 *   within_value = -1, within[p] == within_value for 0..255); otherwise 0.
 *   "Nearest" is Euclidean over the whole frame, not geodesic: a label can grow
 *   across pixels that are not allowed.  The set of ids is unchanged.  out must
 *   not alias labels.
 * Integer arithmetic throughout, no atomics: the outputs are bit-reproducible.
 * workspace: at least unet_distance_workspace_bytes(N, H, W) bytes of device
 * memory; it need not be initialised and holds nothing between calls.  Every
 * bad argument (sizes, src_dtype, sites, fg_value, within_value out of range,
 * a null buffer, both outputs null, out == labels, a short or null workspace)
 * is an error with nothing launched. */
#define UNET_DISTANCE_NONE 2147483647
#define UNET_DISTANCE_MAX_DIM 32768
/* host only; 0 (with unet_last_error) for N, H, W <= 0, H or W > 32768 or H W >= 2^31 */
int64_t unet_distance_workspace_bytes(int N, int H, int W);
int unet_distance_transform(const void* src, int src_dtype /* 0 uint8, 1 int32 */, int N, int H, int W,
                            int fg_value /* -1: nonzero is foreground; >= 0: == value */,
                            int sites /* 0: non-foreground pixels are sites; 1: foreground pixels are sites */,
                            int32_t* dist2 /* nullable */, int32_t* nearest /* nullable */,
                            void* workspace, int64_t workspace_bytes, hipStream_t stream);
int unet_grow_instances(const int32_t* labels, int N, int H, int W,
                        int64_t max_dist2 /* < 0: unlimited */,
                        const uint8_t* within /* nullable [N][H][W] */, int within_value /* -1: nonzero; 0..255: == */,
                        int32_t* out /* must not alias labels */,
                        void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- geodesic growth of a label map and marker watershed by levels (no
 * reference counterpart) ----
 * Frames [N][H][W] are independent.  H, W <= UNET_DISTANCE_MAX_DIM and H W <=
 * UNET_GEODESIC_MAX_HW = 2^28, so that no cost overflows an int32.
 * metric 0 (cityblock): 4 neighbours, a step costs 1.  metric 1 (chamfer): 8
 *   neighbours, an axial step costs 3 and a diagonal step 4; a diagonal step is
 *   allowed whatever the two axial neighbours are.
 * unet_geodesic_grow: labels != 0 are labelled (positive ids; a negative value is a
 *   caller error that is copied like an id, ids are never used as indices).  A
 *   pixel is free when it is unlabelled and allowed (within null: every pixel;
 *   else within[p] nonzero for within_value = -1, within[p] == within_value for
 *   0..255).  A path runs from a free pixel p to a labelled pixel s by steps of the
 *   metric through free pixels only; d(p) is the least cost of such a path with
 *   d(p) <= max_cost (max_cost < 0: unlimited), and out[p] is the smallest id among
 *   the labelled pixels that reach p at cost d(p).  Labelled pixels are copied,
 *   pixels without a path stay 0.  cost (optional): 0 at labelled pixels, d(p) at
 *   reached ones, -1 elsewhere.  Equals Dijkstra from all labelled pixels at once
 *   with the key (cost, id), relaxing into free pixels only.
 * unet_watershed: flooding by levels.  For every value h of relief (uint8) that
 *   occurs under the mask, ascending: markers <- unet_geodesic_grow(markers, within
 *   = mask and relief <= h), unlimited; the predicate is evaluated in the kernel.
 *   Marker pixels keep their id whatever relief and mask say; unreached pixels
 *   stay 0.  mask / mask_value as within / within_value.
 * Both SYNCHRONISE with the host: relaxation passes run until one changes
 *   nothing, which the host learns by reading 4-byte words back on the caller's
 *   stream (the watershed also reads a 256-bin histogram once).  They cannot be
 *   captured into a graph: on a capturing stream they fail with an error and
 *   enqueue nothing.  unet_geodesic_last_counts: passes launched, passes that
 *   changed a tile border and host readbacks of the calling thread's last call.
 * Integer arithmetic, a unique fixed point: the outputs are bit-reproducible.
 * Inputs are never modified; out must not alias labels / markers.  workspace: at
 * least unet_geodesic_workspace_bytes(N, H, W) bytes of device memory (8 bytes
 * per pixel and a little); it need not be initialised and holds nothing between
 * calls.  Every bad argument is an error with nothing launched. */
#define UNET_GEODESIC_MAX_HW 268435456
/* host only; 0 (with unet_last_error) for N, H, W <= 0, H or W > 32768 or H W > 2^28 */
int64_t unet_geodesic_workspace_bytes(int N, int H, int W);
int unet_geodesic_grow(const int32_t* labels, int N, int H, int W, int metric /* 0 cityblock, 1 chamfer */,
                       int64_t max_cost /* < 0: unlimited */,
                       const uint8_t* within /* nullable [N][H][W] */, int within_value /* -1: nonzero; 0..255: == */,
                       int32_t* out /* must not alias labels */, int32_t* cost /* nullable */,
                       void* workspace, int64_t workspace_bytes, hipStream_t stream);
int unet_watershed(const uint8_t* relief, const int32_t* markers, int N, int H, int W, int metric,
                   const uint8_t* mask /* nullable [N][H][W] */, int mask_value /* -1: nonzero; 0..255: == */,
                   int32_t* out /* must not alias markers */,
                   void* workspace, int64_t workspace_bytes, hipStream_t stream);
int unet_geodesic_last_counts(int* passes, int* changing_passes, int* readbacks);

/* ---- training targets for touching cells: the two nearest distinct instances,
 * the border weight map and the interior / boundary targets (no reference
 * counterpart) ----
 * labels are int32 [N][H][W] of independent frames; the sites are the pixels with
 * labels > 0 (any positive id; values <= 0 are unlabelled).
 * unet_two_nearest_instances: for every pixel p the first site s1 minimises the
 *   key (|p - s|^2, flat index of s) over all sites, compared lexicographically
 *   (the key of unet_distance_transform); the second site s2 minimises the same
 *   key over the sites whose label differs from labels[s1].
 *     dist2 int32 [N][2][H][W]: |p - s1|^2 and |p - s2|^2, exact.
 *     ids   int32 [N][2][H][W]: labels[s1] and labels[s2].
 *   Where there is no such site, or it lies beyond max_dist2 (< 0: unlimited),
 *   dist2 = UNET_DISTANCE_NONE and ids = 0.  A labelled pixel has dist2[0] = 0 and
 *   its own id first.  Both squared distances are independent of the tie rule:
 *   they are the two smallest entries of rint(distance_transform_edt(labels != i)
 *   ** 2) over the ids i.  dist2 and ids are each optional, not both null.
 *   H, W <= UNET_TWO_NEAREST_MAX_DIM (a row with two candidates and their labels
 *   per column is staged in 12 W bytes of LDS).
 * unet_border_weights: out[p] = base(p) + border(p), float [N][H][W].
 *   base(p) = class_weights[classes[p]] when classes (uint8 [N][H][W]) and
 *   class_weights (K floats on the device) are given (both or neither; a class >=
 *   K gives 0), else 1.  border(p) = w0 exp(-(sqrt(d1) + sqrt(d2))^2 / (2 sigma^2))
 *   on unlabelled pixels whose second instance exists within max_dist2, with d1,
 *   d2 the squared distances above; 0 elsewhere (the weight map of the U-Net
 *   paper).  The square roots and the exponential are taken in double and the sum
 *   is rounded to float once.  w0 >= 0, sigma > 0.  Labelled pixels skip the scan;
 *   d1 and d2 never go to memory.
 * unet_boundary_targets: classes[p] = 0 where labels[p] <= 0 (background), 2 where
 *   a labelled pixel has a neighbour inside the frame of another value (boundary;
 *   connectivity 1: 4 neighbours, 2: 8), 1 at every other labelled pixel
 *   (interior).  H, W <= UNET_DISTANCE_MAX_DIM, H W < 2^31.  No workspace.
 * Integer arithmetic up to the weight, no atomics, one writer per output word: the
 * outputs are bit-reproducible.  Plain launches on the caller's stream, no memset
 * node: graph-capturable.  workspace: at least unet_two_nearest_workspace_bytes(N,
 * H, W) bytes of device memory; it need not be initialised and holds nothing
 * between calls.  Every bad argument (sizes, a null buffer, both outputs null, one
 * of classes / class_weights alone, w0, sigma, connectivity, a short or null
 * workspace) is an error with nothing launched. */
#define UNET_TWO_NEAREST_MAX_DIM 4096
/* host only; 0 (with unet_last_error) for N, H, W <= 0 or H, W > UNET_TWO_NEAREST_MAX_DIM */
int64_t unet_two_nearest_workspace_bytes(int N, int H, int W);
int unet_two_nearest_instances(const int32_t* labels, int N, int H, int W,
                               int64_t max_dist2 /* < 0: unlimited */,
                               int32_t* dist2 /* nullable [N][2][H][W] */, int32_t* ids /* nullable [N][2][H][W] */,
                               void* workspace, int64_t workspace_bytes, hipStream_t stream);
int unet_border_weights(const int32_t* labels, int N, int H, int W, float w0, float sigma,
                        int64_t max_dist2 /* < 0: unlimited */,
                        const uint8_t* classes /* nullable [N][H][W] */,
                        const float* class_weights /* nullable, K floats on the device */, int K,
                        float* out /* [N][H][W] */, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int unet_boundary_targets(const int32_t* labels, int N, int H, int W,
                          int connectivity /* 1: 4-neighbour, 2: 8-neighbour */,
                          uint8_t* classes /* [N][H][W] */, hipStream_t stream);

/* ---- matching of predicted instances to a ground truth (no reference
 * counterpart) ----
 * gt and pred are int32 label maps [N][H][W] of independent frames, H W < 2^31:
 * 0 is background, the instances carry ids 1..max_gt and 1..max_pred (both caps
 * in 1..65535; the ids need not be compact).  The pair histogram c(g, p) = the
 * number of pixels with gt == g and pred == p gives, per frame,
 *   gt_table int64 [N][max_gt][UNET_MATCH_COLS], row id - 1: area, partner,
 *     intersection, partner_area.  partner is the instance of pred that overlaps
 *     the id with the highest IoU = c / (area + partner_area - c), compared
 *     exactly in integers; among equal IoUs the smaller id.  An id that is absent
 *     (area 0) or overlaps nothing has partner, intersection and partner_area 0.
 *   pred_table int64 [N][max_pred][UNET_MATCH_COLS]: the same for the ids of
 *     pred, with partners among the ids of gt.
 *   status int64 [N][UNET_MATCH_STATUS]: n_gt and n_pred (the ids with area >
 *     0), n_pairs (the pairs (g, p), both nonzero, with c > 0), dropped (the
 *     pixels whose pair found no room in the pair table) and out_of_range (the
 *     pixels with an id below 0 or above its cap; they take no part).  The
 *     tables describe the maps exactly when dropped and out_of_range are 0.
 *   pairs (nullable) int64 [N][max_pairs][3]: gt, pred, intersection of the
 *     first n_pairs pairs, in no particular order (the set is deterministic when
 *     n_pairs <= max_pairs; beyond that an unspecified max_pairs of them); the
 *     remaining rows are 0.
 * The pair table of a frame has the smallest power of two >= 2 max_pairs slots
 * and holds the pairs with one id 0 (instance against background) as well;
 * max_pairs outside 1..2^24 is an error.
 * Integer arithmetic and integer atomics throughout: the outputs are
 * bit-reproducible.  gt and pred are only read.
 * workspace: at least unet_match_workspace_bytes(...) bytes of device memory; it
 * need not be initialised and holds nothing between calls.  It begins with the
 * pair table of the call: uint32 keys [N][slots] (g << 16 | p, 0 = empty), then
 * int32 counts [N][slots].  Every bad argument (a null buffer other than pairs,
 * N, H or W <= 0, H W >= 2^31, a cap or max_pairs out of range, a short or null
 * workspace) is an error with nothing launched. */
#define UNET_MATCH_COLS 4     /* area, partner, intersection, partner_area */
#define UNET_MATCH_STATUS 5   /* n_gt, n_pred, n_pairs, dropped, out_of_range */
/* host only; 0 (with unet_last_error) for a bad argument */
int64_t unet_match_workspace_bytes(int N, int max_gt, int max_pred, int max_pairs);
int unet_match_instances(const int32_t* gt, const int32_t* pred, int N, int H, int W,
                         int max_gt, int max_pred, int max_pairs,
                         int64_t* gt_table,    /* [N][max_gt][4]   row id - 1 */
                         int64_t* pred_table,  /* [N][max_pred][4] */
                         int64_t* status,      /* [N][5] */
                         int64_t* pairs,       /* nullable [N][max_pairs][3]: gt, pred, intersection */
                         void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- measuring the instances of a label map, selecting among them (no reference
 * counterpart) ----
 * labels is an int32 label map [N][H][W] of independent frames, H, W <=
 * UNET_DISTANCE_MAX_DIM and H W <= UNET_GEODESIC_MAX_HW (2^28): 0 is background,
 * the instances carry ids 1..max_instances (in 1..65535; the ids need not be
 * compact).  A pixel with a value below 0 or above max_instances belongs to no
 * instance; as a neighbour it is another nonzero value.  Per frame:
 *   table int64 [N][max_instances][UNET_MEASURE_COLS], row id - 1, over the pixels
 *     (y, x) of value id: area; sum_y, sum_x; y0, x0, y1, x1 (the half-open box;
 *     these seven as the stats of unet_label_instances); sum_yy, sum_xx, sum_xy
 *     (sums of y y, x x, y x); edges (the pixel sides up, down, left, right whose
 *     other side lies outside the frame or holds a different value: the
 *     crack-length perimeter); frame_edges (those on the frame's border);
 *     contact_edges (those whose other side is inside the frame and nonzero).  The
 *     row of an id that does not occur is all zero.
 *   status int64 [N][UNET_MEASURE_STATUS]: n_present (the ids in 1..max_instances
 *     that occur), max_id (the largest of them, 0 if none), out_of_range (the
 *     pixels with a value outside 0..max_instances).
 *   intensity (with image; both null otherwise) [N][max_instances][channels]
 *     [UNET_MEASURE_ICOLS]: sum, sum_sq, min, max of the image over the pixels of
 *     the id; image is [N][channels][H][W], channels in 1..4, of image_dtype 0
 *     (uint8), 1 (uint16) or 2 (float32, finite values; not checked).  Integer
 *     images give an int64 table of exact sums, a float image a double table with
 *     exact min and max.  Rows of absent ids are zero.  Without an image channels
 *     and image_dtype must be 0.
 * Everything but sum and sum_sq of a float image is a sum, minimum or maximum of
 * integers through integer atomics and bit-reproducible; those two are fp64
 * atomic sums and depend on the order of arrival in their last bits.  labels and
 * image are only read.
 * workspace: at least unet_measure_workspace_bytes(...) bytes of device memory
 * (the accumulators: 8 (13 + 4 channels) bytes per row of the table); it need not
 * be initialised and holds nothing between calls.
 *
 * unet_select_instances: keep is uint8 [N][M], M in 1..65535; entry id - 1 nonzero
 * = id survives.  new_ids int32 [N][M]: the 1-based rank of a kept id among the
 * kept ids in ascending order, 0 for a dropped id; counts int32 [N]: the number of
 * kept ids; labels_out int32 [N][H][W] (not labels itself): new_ids[id - 1] for
 * the values 1..M of labels, 0 for every other value.
 * Every bad argument (a null buffer, image without intensity or the reverse, sizes,
 * caps, channels, image_dtype, a short or null workspace) is an error with nothing
 * launched. */
#define UNET_MEASURE_COLS 13   /* area, sum_y, sum_x, y0, x0, y1, x1, sum_yy, sum_xx, sum_xy, edges, frame_edges, contact_edges */
#define UNET_MEASURE_STATUS 3  /* n_present, max_id, out_of_range */
#define UNET_MEASURE_ICOLS 4   /* sum, sum_sq, min, max */
/* host only; 0 (with unet_last_error) for a bad argument */
int64_t unet_measure_workspace_bytes(int N, int H, int W, int max_instances, int channels);
int unet_measure_instances(const int32_t* labels, const void* image /* nullable */,
                           int image_dtype /* 0: uint8, 1: uint16, 2: float32 */, int channels,
                           int N, int H, int W, int max_instances,
                           int64_t* table,   /* [N][max_instances][13] row id - 1 */
                           int64_t* status,  /* [N][3] */
                           void* intensity,  /* nullable with image: [N][max_instances][channels][4] int64 / double */
                           void* workspace, int64_t workspace_bytes, hipStream_t stream);
int unet_select_instances(const int32_t* labels, const uint8_t* keep /* [N][M] */, int N, int H, int W, int M,
                          int32_t* labels_out /* [N][H][W] */, int32_t* counts /* [N] */,
                          int32_t* new_ids /* [N][M] */, hipStream_t stream);

/* ---- linking instances across the frames of a sequence: tracks and z-stacks (no
 * reference counterpart) ----
 * labels is an int32 label map [B][T][H][W]: B independent sequences of T frames
 * (time points, or the slices of a z-stack), T in 1..65535, H, W <=
 * UNET_DISTANCE_MAX_DIM and H W <= UNET_GEODESIC_MAX_HW.  Within a frame 0 is
 * background and the instances carry ids 1..max_instances (in 1..65535; not
 * necessarily compact, and without meaning across frames).  With IoU threshold
 * iou_num / iou_den (0 <= iou_num < iou_den), instance b of frame t >= 1 (area A_b)
 * and its partner a of highest IoU in frame t - 1 as unet_match_instances(gt = frame
 * t - 1, pred = frame t) defines it (intersection I, area A_a):
 *   b continues the track of a iff a exists, the best partner of a in frame t is b,
 *     and I iou_den > iou_num (A_a + A_b - I), i.e. IoU strictly above the threshold;
 *   otherwise b starts a track, whose parent is the track of a iff a exists and
 *     2 I > A_b, else 0.
 * Every instance of frame 0 starts a track with parent 0.  There is no gap closing.
 * Tracks are numbered 1..n_tracks in the order (first frame, original id).
 *   tracks int32 [B][T][H][W] (not labels itself): the track id of every pixel with
 *     a value in 1..max_instances, 0 for every other value.
 *   table int64 [B][max_tracks][UNET_LINK_COLS], row track - 1: first, last (frame
 *     indices), parent (a track id or 0), volume (the sum of the areas over the
 *     frames).  Rows of absent tracks are zero; tracks above max_tracks have no row.
 *   status int64 [B][UNET_LINK_STATUS]: n_tracks (the true count, also above
 *     max_tracks; tracks carries the true ids), n_links (instances that continue a
 *     track), dropped and out_of_range (those of unet_match_instances summed over the
 *     T - 1 frame pairs of the sequence, so a pixel of an inner frame counts twice;
 *     T == 1 matches frame 0 against itself and reports that call's).  When dropped or
 *     out_of_range is nonzero only status is specified.
 * T min(max_instances, H W) must not exceed 2^31 - 1 (track ids are int32).
 * Integer arithmetic throughout; every output is bit-reproducible.  labels is only read.
 * workspace: at least unet_link_workspace_bytes(...) bytes of device memory (the
 * match tables of every frame pair, one int32 LUT row of max_instances + 1 entries per
 * frame, one match workspace); it need not be initialised and holds nothing between
 * calls.  table and status need not be initialised either.  Every bad argument (a
 * null buffer, tracks == labels, sizes, caps, max_tracks < 1, the threshold, a short
 * or null workspace) is an error with nothing launched.  All launches are ordinary
 * kernels on the stream.
 * UNET_LINK_BLOCK: the ids of a frame are resolved in chunks of this many;
 * UNET_LINK_LDS_IDS: up to this max_instances the relabelling pass keeps a frame's LUT
 * row in LDS, above it the row is read through L2. */
#define UNET_LINK_COLS 4        /* first, last, parent, volume */
#define UNET_LINK_STATUS 4      /* n_tracks, n_links, dropped, out_of_range */
#define UNET_LINK_BLOCK 1024
#define UNET_LINK_LDS_IDS 8191
/* host only; 0 (with unet_last_error) for a bad argument */
int64_t unet_link_workspace_bytes(int B, int T, int max_instances, int max_pairs);
int unet_link_instances(const int32_t* labels, int B, int T, int H, int W,
                        int max_instances, int max_pairs, int max_tracks, int iou_num, int iou_den,
                        int32_t* tracks_out,  /* [B][T][H][W] */
                        int64_t* table,       /* [B][max_tracks][4] row track - 1 */
                        int64_t* status,      /* [B][4] */
                        void* workspace, int64_t workspace_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
