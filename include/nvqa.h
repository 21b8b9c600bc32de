/*
 * nvqa.h -- C ABI of libnvqa, the MI355X (gfx950) implementation of the VQA
 * training step of srama2512/novel-vqa.
 *
 * Every entry point below replaces one piece of the reference's Lua/Torch7
 * interface for the hot path (paths relative to the reference checkout):
 *
 *   nvqa_create / nvqa_destroy     net construction + :cuda()
 *                                  002_train_vqa_arch1/002_train_baseline.lua:141-171
 *                                  003_train_vqa_arch2/002_train_baseline.lua:138-177
 *   nvqa_param_count / _segments   sizes={...}; join_vector({...})
 *                                  002_train_baseline.lua:183,190 (arch2 :189,198)
 *   nvqa_init_params               *_w:uniform(-0.08,0.08)        002_train_baseline.lua:174-181
 *   nvqa_set_params/_get_params    split_vector + :copy            002_train_baseline.lua:273-286,
 *                                  004_eval_model.lua:154-163
 *   nvqa_step                      the optim closure JdJ(x)        002_train_baseline.lua:272-335
 *                                  (arch2 :277-333); batch = dataset:next_batch() :195-222
 *   nvqa_get_grads                 `gradients` returned by JdJ incl. clamp :328-329
 *   nvqa_rmsprop_update            optim.rmsprop(JdJ, x, config, state) :408,
 *                                  formula misc/rmsprop_lrscale.lua:13-34
 *   nvqa_forward                   eval-mode forward + argmax      004_eval_model.lua:202-233
 *   nvqa_optim_update              sgd / sgdm / sgdmom / adagrad / rmsprop / adam of 001_train_autoencoder/misc/optim_updates.lua
 *   nvqa_dataset_load /            dataset[...] tensors + dataset:next_batch() gather
 *   nvqa_step_indices              002_train_baseline.lua:93-121,195-222
 *   nvqa_ae_corpus_load /          the label tensors of misc/DataLoader.lua + its linear walk (getBatch): the text
 *   nvqa_ae_step_rows /            auto-encoders' corpus resident in HBM, a step named by B row ids
 *   nvqa_ae_evaluate_rows          001_train_autoencoder/misc/DataLoader.lua
 *   nvqa_comm_*                    (absent in the reference: data-parallel gradient all-reduce)
 *
 * Conventions: plain C, POD arguments only.  All pointers are caller-owned
 * host memory borrowed for the duration of the call; device buffers, streams,
 * optimiser state and the RCCL communicator are owned by the context.  No
 * entry point throws or longjmps: 0 = success, negative = error, message via
 * nvqa_last_error() (thread-local).  Indices follow the reference's data
 * files: tokens 1..V (0 = padding), labels 1..A, image positions 1..N_img.
 */
#ifndef NVQA_H
#define NVQA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVQA_ARCH1 1 /* 002_train_vqa_arch1: Linear(V,E) embedding, n-layer LSTM, AxB fusion */
#define NVQA_ARCH2 2 /* 003_train_vqa_arch2: image-as-first-token nn.Encoder, Linear(R,A) head */
#define NVQA_ARCH_AE1 3 /* 001_train_autoencoder/001_train_arch1_text_autoencoder.lua: LSTM text auto-encoder
                         * (misc/AutoEncoder_text_nostart.lua); dims T = seq_length D, I = C = A = 0 */
#define NVQA_ARCH_AE2 4 /* 001_train_autoencoder/001_train_arch2_text_autoencoder.lua: image-first-token LSTM auto-encoder
                         * (misc/AutoEncoder.lua); dims as NVQA_ARCH_AE1, the image row is E wide */
#define NVQA_ARCH_AE2_WP 5 /* 001_train_autoencoder/004_train_arch2_weakpaired_autoencoder_{vgg,inc}.lua: the AE2 model fed
                            * L2Normalize(features) W_p^T + b_p as its image row, with a frozen lookup table
                            * (misc/AutoEncoderNull.lua); dims B, T = seq_length, V, E, R, L, I = feature width; C = A = 0 */
#define NVQA_ARCH_AE1_WP 6 /* 001_train_autoencoder/004_train_arch1_weakpaired_autoencoder_{vgg,inc}.lua: the AE1 model whose
                            * decoder starts from the encoder's final state plus a multimodal correction of that state and the
                            * image (misc/AutoEncoder_vqa_arch.lua); dims B, T = seq_length, V, E, R, L = 1, I = feature width,
                            * C = 2R, A = 0 */

/* Model dimensions (SURVEY.md symbol table). */
typedef struct nvqa_dims {
    int32_t arch; /* NVQA_ARCH1 | NVQA_ARCH2 | NVQA_ARCH_AE1 | NVQA_ARCH_AE2 | NVQA_ARCH_AE2_WP | NVQA_ARCH_AE1_WP */
    int32_t B;    /* minibatch (QA pairs) per device             -batch_size          */
    int32_t T;    /* question buffer length (columns of ques_*)  buffer_size_q        */
    int32_t V;    /* question vocabulary size                    vocabulary_size_q    */
    int32_t E;    /* word embedding width                        -input_encoding_size */
    int32_t R;    /* LSTM hidden size                            -rnn_size            */
    int32_t L;    /* LSTM layers                                 -rnn_layer/-num_layers */
    int32_t I;    /* image feature width                         -nhimage             */
    int32_t C;    /* common embedding width (arch1 only)         -common_embedding_size */
    int32_t A;    /* answer classes                              -num_output          */
} nvqa_dims;

/* Dropout control.  Torch7's MT19937 bernoulli stream cannot be reproduced, so
 * masks come from the counter-based generator of nvqa_rng.h, identical on the
 * CPU oracle and on the device.  mode 0 = every D_* = 1 (gradient/logit parity
 * runs); mode 1 = Bernoulli(1-p) masks scaled by 1/(1-p), keyed by
 * (seed, step, site, element). */
typedef struct nvqa_dropout {
    int32_t mode;  /* 0 off, 1 seeded */
    float p;       /* drop probability, reference value 0.5 */
    uint64_t seed; /* reference default -seed 123 */
    uint64_t step; /* iteration counter, mixed into every mask */
} nvqa_dropout;

/* Decoding options of nvqa_ae_sample / nvqa_ae_sample_rows: the opt table of sample(sents, opt)
 * (001_train_autoencoder/misc/AutoEncoder_text_nostart.lua:134-139).  32 bytes. */
typedef struct nvqa_sample_opts {
    int32_t mode;        /* 0 = argmax (sample_max = 1), 1 = multinomial (sample_max = 0), 2 = beam (beam_size > 1) */
    int32_t beam_size;   /* mode 2: 1..8; ignored otherwise */
    float temperature;   /* mode 1: > 0; ignored otherwise */
    int32_t pad_;        /* 0 */
    uint64_t seed, step; /* mode 1: keys of the counter-based generator (nvqa_rng.h, NVQA_SITE_AE_SAMPLE) */
} nvqa_sample_opts;

typedef struct nvqa_ctx nvqa_ctx;

/* ---- lifetime ------------------------------------------------------- */
int nvqa_create(const nvqa_dims *dims, int device, nvqa_ctx **out);
int nvqa_destroy(nvqa_ctx *ctx);
const char *nvqa_last_error(void);
int nvqa_sync(nvqa_ctx *ctx); /* wait for all enqueued work (loss_out becomes valid) */

/* ---- parameters: one flat fp32 vector, reference segment order ------- */
/* arch1: [encoder | embedding | multimodal]; arch2: [cnn | encoder | multimodal].
 * Intra-segment order (documented in DESIGN.md):
 *  arch1 encoder   : per layer W_i2h[4R x in], b_i2h[4R], W_h2h[4R x R], b_h2h[4R]
 *  arch1 embedding : W_e[E x V] (Torch nn.Linear layout), b_e[E]
 *  arch1 multimodal: W_q[C x 2RL], b_q[C], W_v[C x I], b_v[C], W_o[A x C], b_o[A]
 *  arch2 cnn       : W_p[E x I], b_p[E]
 *  arch2 encoder   : LSTM layers as above, then lookup W_lk[(V+1) x E]
 *  arch2 multimodal: W_o[A x R], b_o[A]
 *  ae1 encoder     : LSTM layers as above (AutoEncoder_text_nostart.lua:89-110 parameters() order)
 *  ae1 decoder     : LSTM layers as above, then W_proj[(V+1) x R], b_proj[V+1]
 *  ae1 lookup      : W_lk[(V+1) x E] (row V+1 = the START / END token)
 *  ae2             : as ae1 (AutoEncoder.lua:86-107 parameters() order)
 *  ae2_wp          : as ae2; the image projection W_p [E x I], b_p [E] lives outside the vector (nvqa_ae_wp_*)  */
size_t nvqa_param_count(const nvqa_ctx *ctx);
int nvqa_segments(const nvqa_ctx *ctx, size_t sizes_out[3]);
int nvqa_init_params(nvqa_ctx *ctx, uint64_t seed, float lo, float hi);
int nvqa_set_params(nvqa_ctx *ctx, const float *params);
int nvqa_get_params(nvqa_ctx *ctx, float *params_out);
/* Gradient of the last step, reference layout; clamp > 0 applies
 * clamp(-clamp, clamp) on the way out (JdJ returns clamped gradients). */
int nvqa_get_grads(nvqa_ctx *ctx, float *grads_out, float clamp);

/* ---- the hot path ---------------------------------------------------- */
/* One forward+backward over a host-resident minibatch (the body of JdJ).
 *  arch1: tokens [B x T] right-aligned, 0 = left padding (right_align,
 *         misc/RNNUtils.lua:54-61); lengths [B] >= 1.
 *  arch2: tokens [B x T] left-aligned, 0 = null token (the library forms the
 *         reference's [T x B] transpose itself); lengths may be NULL.
 *  img [B x I] (already L2-normalised, 002_train_baseline.lua:117-121);
 *  labels [B], 1-based.  The mean cross-entropy is written to *loss_out once
 *  the work has drained (nvqa_sync or the next call). Gradients stay on the
 *  device for nvqa_rmsprop_update / nvqa_get_grads. */
int nvqa_step(nvqa_ctx *ctx, const int32_t *tokens, const int32_t *lengths, const float *img,
              const int32_t *labels, const nvqa_dropout *dropout, float *loss_out);

/* Loss of the last step (waits for the stream). With loss_out == NULL nvqa_step only
 * enqueues work; with a non-NULL loss_out it blocks like the reference's JdJ does. */
int nvqa_get_loss(nvqa_ctx *ctx, float *loss_out);

/* Evaluate-mode forward (all dropout = identity): scores [n x A] and/or
 * 1-based argmax [n] (either may be NULL), n <= B rows. */
int nvqa_forward(nvqa_ctx *ctx, int32_t n, const int32_t *tokens, const int32_t *lengths,
                 const float *img, float *scores_out, int32_t *argmax_out);

/* Evaluate-mode forward with everything the reference's validation and test loops take from it, on the device:
 *  labels [n] (optional, 1-based): *loss_out = mean cross-entropy over the n rows -- validate(),
 *         002_train_baseline.lua:337-381 (arch2: 003_.../002_train_baseline.lua:335-378);
 *  mc_ans [n x n_mc] (optional; 1-based answer ids, 0 = empty slot, n_mc <= 64): mc_argmax_out[i] = the candidate
 *         with the highest score, first one on ties, as torch.max over the candidates in slot order gives it --
 *         multiple-choice answers of 004_eval_model.lua:259-271 (MC_ans_test has 18 slots); rows without any
 *         candidate return 0;
 *  scores_out [n x A], argmax_out [n]: as nvqa_forward.  Every output pointer may be NULL. */
int nvqa_evaluate(nvqa_ctx *ctx, int32_t n, const int32_t *tokens, const int32_t *lengths, const float *img,
                  const int32_t *labels, const int32_t *mc_ans, int32_t n_mc, float *scores_out,
                  int32_t *argmax_out, int32_t *mc_argmax_out, float *loss_out);

/* clamp -> (+ wd * x) -> m = alpha m + (1-alpha) g^2 -> x -= lr g / (sqrt(m) + eps).
 * With a communicator (nvqa_comm_init) nvqa_step itself sums the gradient over the ranks,
 * one all-reduce per parameter segment overlapped with the backward pass; the update then
 * divides by the world size and the clamp acts on that average.  nvqa_get_grads returns the
 * same average. */
int nvqa_rmsprop_update(nvqa_ctx *ctx, float lr, float alpha, float eps, float wd, float clamp);

/* ---- model variants of the reference's other training scripts -------------- */
/* The fusion module in front of the classifier (002_train_vqa_arch1/misc/netdef.lua), arch1 only:
 *   mode 0  netdef.AxB    (:6-14)   qc (*) ic                      -- what every training script of the reference uses
 *   mode 1  netdef.AskipB (:16-25)  qc + qc (*) ic                 -- 003_train_ae_based_wp.lua:151
 *   mode 2  netdef.A_B    (:27-35)  JoinTable(2)({qc, ic}): the classifier reads 2C values, so W_o becomes [A x 2C]:
 *           nvqa_param_count / nvqa_segments / include/nvqa_layout.h (nvqa_layout_init_fusion) change.  Switching to or
 *           from mode 2 is only accepted on a context that has not been given parameters yet (right after nvqa_create). */
int nvqa_set_fusion(nvqa_ctx *ctx, int mode);
/* BASELINE config "arch2 ... bf16": bf16 = 1 runs every dense product of the step (forward, dgrad, wgrad)
 * on the bf16 matrix cores: both operands rounded to bf16 (round-to-nearest-even) as they are read,
 * products accumulated in f32.  Parameters, activations, gradients, the optimiser and everything at this
 * ABI stay f32 (SURVEY.md 8b "numerics contract").  Default 0 = the reference's f32 arithmetic
 * (torch.setdefaulttensortype('torch.FloatTensor'), 002_train_baseline.lua:54). */
int nvqa_set_precision(nvqa_ctx *ctx, int bf16);
/* arch2 only: reproduce, on request, two things the reference's nn.Encoder does that are artefacts of its Lua code
 * (flags = OR of the bits; default 0 = the model as designed):
 *  NVQA_QUIRK_H0      misc/Encoder_lstm.lua:238-239 with :30-47,:164 -- backward aliases the table of initial-state
 *                     tensors and stores gradOutput in its last slot, so from the second iteration on (training and
 *                     validation forwards alike) the top layer starts from h0 = dL/d(encoder output) of the previous
 *                     backward, and the step-1 weight gradient of the top layer's W_h2h is taken against the CURRENT
 *                     step's dL/d(encoder output).
 *  NVQA_QUIRK_LOOKUP  misc/Encoder_lstm.lua:49-58 with 002_train_baseline.lua:186,273 -- getParameters() runs before
 *                     createClones(), whose lookup-table clones share the weight but not gradWeight with the flattened
 *                     module: the lookup slice of encoder_dw_q stays zero, W_lk only sees weightDecay.
 * Setting the flags also clears the carried h0 state. */
#define NVQA_QUIRK_H0 1
#define NVQA_QUIRK_LOOKUP 2
int nvqa_set_ref_quirks(nvqa_ctx *ctx, int flags);
/* torch.norm(cnn_w), torch.norm(encoder_w_q), torch.norm(multimodal_w) of 003_train_vqa_arch2/002_train_baseline.lua:402-404
 * (arch1: encoder_w_q, embedding_w_q, multimodal_w): the L2 norm of each of the three parameter segments in
 * nvqa_segments order, reduced on the device.  Synchronises the context's stream. */
int nvqa_param_norms(nvqa_ctx *ctx, float out[3]);
/* out[0] / out[1] = 1 when the next training step runs the LSTM forward unroll / the BPTT as ONE persistent launch
 * (R = 512, E in {200, 512}; BPTT: L <= 2), 0 when it takes the per-level kernels (other shapes, NVQA_PERSIST=0, or after a
 * reported time-out). */
int nvqa_persistent_state(const nvqa_ctx *ctx, int out[2]);
/* How many f32-mode weight-gradient products this context has launched so far, by route: out[0] the f32 MFMA chain
 * (NVQA_WGRAD_SPLIT=0, or a shape the six-term kernels do not take), out[1] k_wgrad_split (NVQA_WGRAD_KERNEL=1), out[2]
 * k_wgrad_split2 (the default).  The two six-term kernels give the same bits; the counters say which one ran. */
int nvqa_wgrad_routes(const nvqa_ctx *ctx, int64_t out[3]);
/* How many f32-mode d(layer-0 input) products this context has launched so far, by route: out[0] the f32 MFMA GEMM
 * (NVQA_DX0_KERNEL=1, or a shape k_dx0_split does not take), out[1] k_dx0_split (six bf16 MFMA terms per product, the
 * default).  NVQA_DX0_KERNEL is independent of NVQA_WGRAD_SPLIT. */
int nvqa_dx0_routes(const nvqa_ctx *ctx, int64_t out[2]);
/* Per-segment gradient scale applied before the clamp: {lr_scale, lr_scale, 1} reproduces
 * -lr_scale of 003_train_ae_based_wp.lua:30,344. */
int nvqa_set_grad_scales(nvqa_ctx *ctx, const float scales[3]);

/* ---- HBM-resident dataset (the tensors of 002_train_baseline.lua:93-121) ---- */
/* questions [N x T] (aligned as nvqa_step expects), lengths [N], img_pos [N]
 * (1-based rows of feats), answers [N] (1-based), feats [N_img x I].
 * l2_normalize: 0 = keep, 1 = row L2 norm (002_train_baseline.lua:117-121), n > 1 = the two blocks
 * [0,n) and [n,I) normalised separately (early fusion, 003_train_ae_based_ef.lua:115-119, n = 2048). */
int nvqa_dataset_load(nvqa_ctx *ctx, int64_t n_q, const int32_t *questions, const int32_t *lengths,
                      const int32_t *img_pos, const int32_t *answers, int64_t n_img,
                      const float *feats, int l2_normalize);
/* JdJ with dataset:next_batch() done on the device: qinds [B], 0-based rows. */
int nvqa_step_indices(nvqa_ctx *ctx, const int64_t *qinds, const nvqa_dropout *dropout,
                      float *loss_out);

/* ---- data parallel (new functionality; the reference is single-GPU) --- */
#define NVQA_COMM_ID_BYTES 128
int nvqa_comm_unique_id(void *id_out /* NVQA_COMM_ID_BYTES */);
int nvqa_comm_init(nvqa_ctx *ctx, int rank, int world, const void *id);
/* Path of the collective library the nvqa_comm_* entries run on (loads it if that has not happened yet; NULL +
 * nvqa_last_error() when none can be loaded).  The rule: NVQA_RCCL_LIB if set; else the librccl that sits beside the HIP
 * runtime image mapped into this process, opened RTLD_LOCAL. */
const char *nvqa_comm_library(void);

/* ---- VGG-16 fc7 feature extractor (002_train_vqa_arch1/001_prepro_img_vgg.lua) ---- */
/* Forward only.  width_div = 1 and input_hw = 224 is the real 16-layer VGG (channels
 * 64..512, fc 4096); other values shrink it for tests.  Replaces loadcaffe.load +
 * net:forward + net.modules[38].output (:36-37,109-110). */
typedef struct nvqa_vgg nvqa_vgg;
int nvqa_vgg16_create(int device, int width_div, int input_hw, int max_batch, nvqa_vgg **out);
int nvqa_vgg16_destroy(nvqa_vgg *vgg);
size_t nvqa_vgg16_weight_count(const nvqa_vgg *vgg);
int nvqa_vgg16_feature_dim(const nvqa_vgg *vgg);
/* One flat vector in Caffe order and layout: per conv W [Cout][Cin][3][3], b [Cout];
 * fc6 W [F][C5*S*S] (CHW-flattened input), b [F]; fc7 W [F][F], b [F]. */
int nvqa_vgg16_set_weights(nvqa_vgg *vgg, const float *flat);
/* images: n x 3 x hw x hw as loadim returns them (BGR planes, mean-subtracted, :65-70);
 * feats_out: n x F = post-ReLU fc7. */
int nvqa_vgg16_fc7(nvqa_vgg *vgg, const float *images, int n, float *feats_out);
/* 1: the operands of every convolution / fc product are rounded to bf16 (bf16 matrix cores, f32 accumulate; weights,
 * activations and the features at the ABI stay f32), as nvqa_set_precision does for the training step.  The reference
 * extracts in fp32 (001_prepro_img_vgg.lua:36,109-110): 0 is the default. */
int nvqa_vgg16_set_precision(nvqa_vgg *vgg, int bf16);
/* loadim's arithmetic (:50,65-69): bilinear scale of RGB [0,1] planes n x 3 x H x W to hw x hw,
 * x255, RGB->BGR, mean subtraction.  out: n x 3 x hw x hw. */
int nvqa_vgg16_preprocess(nvqa_vgg *vgg, const float *rgb, int n, int H, int W, float *out);
/* The raw-image route of the weak-paired scripts (004_train_arch{1,2}_weakpaired_autoencoder_vgg.lua with net_utils.prepro):
 * images = n x 3 x S x S uint8 planar RGB as /images/<split> stores them.  One fused kernel cuts the hw x hw window whose
 * 0-based origin is (xoff, yoff), 0 <= off <= S - hw (one origin for the batch; S == hw: no crop), converts to float, subtracts
 * the RGB mean {123.68, 116.779, 103.939} and writes the network's input; the bytes the convolutions read are those
 * nvqa_vgg16_fc7 reads from the same crop prepared on the host (BGR planes, mean-subtracted, float32).  body_dropout NULL or
 * mode 0: evaluate mode, the bits of nvqa_vgg16_fc7.  mode 1: drop6 and drop7 (modules 35 and 38) are live, masks of
 * nvqa_rng.h's NVQA_SITE_VGG_FC6 / NVQA_SITE_VGG_FC7 applied to the f32 value.  feats_out: n x F = module 38's output.
 * An error, before anything is launched: S < hw, an origin outside 0..S-hw, n outside 1..max_batch or above the extractor's
 * chunk size (NVQA_VGG_CHUNK, 256), no weights loaded, p outside [0, 1). */
int nvqa_vgg16_fc7_raw(nvqa_vgg *vgg, const uint8_t *images, int n, int S, int xoff, int yoff,
                       const nvqa_dropout *body_dropout, float *feats_out);

/* Fine-tuning the f32 body (protos.cnn:backward and the cnn update of 004_train_arch{1,2}_weakpaired_autoencoder_vgg.lua,
 * arch2 :307-310, :457-466; arch1 :329, :477-484).
 * nvqa_vgg16_train_enable(vgg, 1) allocates the training state -- every layer's output of a training forward, two gradient
 * buffers, the gradients, the tap-flipped weight images of d(input), the split-K workspace; about 60 MB per image of max_batch
 * at full width and 224 x 224 -- and (vgg, 0) or destroy frees it; an extractor that never trains pays nothing.  Refused on a
 * bf16 extractor, and nvqa_vgg16_set_precision(vgg, 1) is refused while it is enabled.
 * nvqa_vgg16_train_forward_raw: nvqa_vgg16_fc7_raw's arguments, launches and bits, every layer kept; feats_out may be NULL.
 * nvqa_vgg16_train_activation: the saved output of layer which = 0..12 (convolution, post-ReLU, NCHW, true channels), 13 (fc6),
 * 14 (fc7: post-ReLU, post-dropout) of the last training forward.
 * nvqa_vgg16_backward: dfeats [n x F] on the host = d(loss)/d(features); through_l2norm = 1: dfeats is d/d(f^) of the
 * row-normalised features and nn.L2Normalize's backward (misc/L2Normalize.lua:22-40, from the saved features; a row of norm zero
 * gives NaN there as in the forward) runs first.  Bit-reproducible: no atomics, split-K slabs summed in a fixed order.
 * nvqa_vgg16_get_grads / nvqa_vgg16_get_weights: one flat vector in nvqa_vgg16_set_weights' layout (get_weights is its exact inverse).
 * nvqa_vgg16_update: rule NVQA_OPT_SGD, NVQA_OPT_SGDM or NVQA_OPT_ADAM in the lrs forms of misc/optim_updates.lua with
 * cnnFinalLearningScales = scale everywhere (arch2: 0.01, arch1: 1): g += wd scale x (wd != 0), clamp (clamp > 0), the rule with
 * every step times scale.  stats_out (may be NULL) = {|x|_2, count(|lr g| >= 0.01 |x|)} over the true weights, of x before the
 * update and g after wd and clamp.
 * An error before anything is launched: training not enabled, bf16, backward without a training forward or with another n,
 * n outside 1..max_batch, any other rule. */
int nvqa_vgg16_train_enable(nvqa_vgg *vgg, int on);
int nvqa_vgg16_train_forward_raw(nvqa_vgg *vgg, const uint8_t *images, int n, int S, int xoff, int yoff,
                                 const nvqa_dropout *dropout, float *feats_out);
int nvqa_vgg16_train_activation(nvqa_vgg *vgg, int which, float *out);
int nvqa_vgg16_backward(nvqa_vgg *vgg, const float *dfeats, int n, int through_l2norm);
int nvqa_vgg16_get_grads(nvqa_vgg *vgg, float *flat_out);
int nvqa_vgg16_get_weights(nvqa_vgg *vgg, float *flat_out);
int nvqa_vgg16_update(nvqa_vgg *vgg, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                      float scale, float stats_out[2]);

/* The extractor run on the fly in front of the training step (BASELINE config "end-to-end"):
 * images [B x 3 x hw x hw] as loadim returns them -> fc7 -> row L2 norm (002_train_baseline.lua:117-121)
 * -> the JdJ body of nvqa_step.  The extractor's feature width must equal dims.I; the features
 * never leave the device. */
int nvqa_step_images(nvqa_ctx *ctx, nvqa_vgg *vgg, const float *images, const int32_t *tokens,
                     const int32_t *lengths, const int32_t *labels, const nvqa_dropout *dropout,
                     float *loss_out);

/* ---- text auto-encoder (NVQA_ARCH_AE1 / NVQA_ARCH_AE2 contexts) ---- */
/* On an auto-encoder context nvqa_step*, nvqa_forward, nvqa_evaluate, nvqa_set_fusion, nvqa_set_ref_quirks,
 * nvqa_dataset_load (the resident corpus: nvqa_ae_corpus_load, below), nvqa_comm_init (data parallel: nvqa_ae_comm_init, below) and nvqa_set_precision(ctx, 1) return an error.
 * One training forward + LanguageModelCriterion + backward (lossFun of 001_train_arch1_text_autoencoder.lua:212-245):
 * tokens [B x D] left-aligned, 1..V, 0 = null.  Gradients stay on the device (nvqa_get_grads, nvqa_adam_update,
 * nvqa_rmsprop_update); *loss_out (may be NULL) = the criterion's mean over the positions that carry a loss. */
int nvqa_ae_step(nvqa_ctx *ctx, const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out);
/* Evaluate-mode (dropout = identity) loss of n <= B rows (eval_split, :148-194) and, if samples_out [n x D] is not NULL,
 * greedy decoding (sample() with sample_max = 1, AutoEncoder_text_nostart.lua:134-210): 1-based tokens, V+1 = END.
 * The encoder sees the tokens as the training forward does (0 -> 1, up to the batch's last non-null column). */
int nvqa_ae_evaluate(nvqa_ctx *ctx, int32_t n, const int32_t *tokens, float *loss_out, int32_t *samples_out);
/* NVQA_ARCH_AE2 (misc/AutoEncoder.lua): the encoder runs image row, START, then the tokens; the decoder is AE1's.
 * On an AE2 context nvqa_ae_step / nvqa_ae_evaluate are the calls below with images = NULL (the text script's zero rows);
 * on an AE1 context the calls below return an error.  images [B x E] (evaluate: [n x E]) or NULL = zeros.
 * dimages_out [B x E] (may be NULL) = d(loss)/d(images), the encoder's step-1 input gradient (updateGradInput, :405-414). */
int nvqa_ae_step_images(nvqa_ctx *ctx, const float *images, const int32_t *tokens, const nvqa_dropout *dropout,
                        float *loss_out, float *dimages_out);
int nvqa_ae_evaluate_images(nvqa_ctx *ctx, int32_t n, const float *images, const int32_t *tokens, float *loss_out,
                            int32_t *samples_out);
/* The bf16 operand mode of the NVQA_ARCH_AE1 / NVQA_ARCH_AE2 step: bf16 = 1 rounds both operands of
 * every dense product -- the time-batched i2h and the recurrent h2h products, their d(input) / d(h) counterparts in BPTT, all
 * LSTM weight gradients, the vocabulary projection, its dH_top and dW_proj -- to bf16 (round-to-nearest-even) and accumulates
 * in f32, in nvqa_ae_step* and nvqa_ae_evaluate* alike.  Parameters, activations, the logits the softmax reads, the cell, the
 * lookup, the dropout masks (applied before the rounding), bias sums, the lookup gradient, Adam and everything at this ABI
 * stay f32.  May be switched between any two steps; 0 (the default) is the f32 path, bit for bit.
 * A switch of its own on purpose: nvqa_set_precision(ctx, 1) stays an error on every auto-encoder context (above), and this
 * call is an error on a VQA context (use nvqa_set_precision there) and on the weak-paired contexts below (at the scripts'
 * batch sizes of 10 - 20 rows their step is bound by its launches; the image projection and the state bridge stay f32). */
int nvqa_ae_set_precision(nvqa_ctx *ctx, int bf16);
/* Data parallel for NVQA_ARCH_AE1 / NVQA_ARCH_AE2 contexts (f32 and the bf16 operand mode).  Same id /
 * rank / world contract and the same collective-library rule as nvqa_comm_init (nvqa_comm_unique_id, nvqa_comm_library,
 * NVQA_RCCL_LIB).  A call of its own on purpose, as nvqa_ae_set_precision is: nvqa_comm_init stays an error on every auto-encoder
 * context.  An error on a VQA context, on the weak-paired contexts (batches of 16 - 20 rows, steps bound by their launches), on
 * a context that already has a communicator, and for a bad rank / world.
 * With a communicator nvqa_ae_step / nvqa_ae_step_images end with the gradient of the GLOBAL batch: with n_r the criterion's
 * count on rank r (predictions that carry a loss) and N = sum n_r, nvqa_get_grads returns sum_r (n_r / N) G_r on every rank --
 * the ranks' counts differ, so the plain mean of their gradients is not that -- and nvqa_adam_update / nvqa_rmsprop_update clamp
 * and apply that value (the clamp after the mean), with the same stats_out on every rank.  N is formed on the device (a one-float
 * all-reduce under the forward pass); the gradient travels as one all-reduce per bucket behind the kernels that finish it, in
 * the same order on every rank: W_proj | b_proj first (under the whole BPTT chain), then per layer, top down, the decoder's and
 * the encoder's LSTM slice, then the lookup table; a two-float exchange closes the step.  loss_out / nvqa_get_loss return the
 * global batch's loss sum n_r loss_r / N once that has drained.  dimages_out is this rank's rows of d(loss_r)/d(images) times
 * n_r world / N: scaled as the rank's own gradient is BEFORE the exchange, so that whatever the caller back-propagates from it
 * and then averages over the ranks is again the global batch's gradient (d(global loss)/d(own rows) = dimages_out / world).
 * tmax stays rank-local: the reference's model depends on the batch (the encoder runs to the batch's last non-null column and
 * feeds 0 -> 1 before it), so every rank runs its own rows exactly as a single-GPU step would, and the exchange forms the
 * count-weighted mean.  That equals the step on the concatenated batch whenever all ranks have the same tmax.
 * nvqa_ae_evaluate* issue no collective: they are rank-local, and one rank may evaluate while the others do not.  Dropout masks
 * stay keyed by (seed, step, site, rank-local element): distinct seeds per rank are the caller's job.
 * A step is collective: every rank must call it the same number of times.  When nvqa_ae_step* returns an error on one rank
 * before its collectives were issued (an all-null batch, a token outside 0..V), the other ranks block in the count's
 * all-reduce: treat a step error on any rank as fatal for the whole job. */
int nvqa_ae_comm_init(nvqa_ctx *ctx, int rank, int world, const void *id);
/* The resident corpus of NVQA_ARCH_AE1 / NVQA_ARCH_AE2 contexts: the text scripts walk a corpus that
 * never changes, so it lives in HBM and a step is named by B row ids.  An error on a VQA context and on the weak-paired contexts.
 * nvqa_ae_corpus_load: tokens [n_rows x D], 0..V, 0 = null, left-aligned as nvqa_ae_step takes them; every token is checked
 * before any device state is touched.  A failed load leaves a previously loaded corpus in place; a successful one replaces it
 * (after the context's stream has drained). */
int nvqa_ae_corpus_load(nvqa_ctx *ctx, int64_t n_rows, const int32_t *tokens);
/* nvqa_ae_step on rows[0..B) of the corpus (0-based; any order, repeats allowed): the same kernels on the same lookup index, which
 * is built on the device, so loss, gradients and updates equal nvqa_ae_step on the gathered rows bit for bit.  AE2: zero image
 * rows, as the text script feeds.  With loss_out = NULL and no communicator the call only enqueues: it waits for nothing on the
 * device.  With a communicator (nvqa_ae_comm_init) it is nvqa_ae_step's collective step, and the two may be mixed freely. */
int nvqa_ae_step_rows(nvqa_ctx *ctx, const int64_t *rows, const nvqa_dropout *dropout, float *loss_out);
/* nvqa_ae_evaluate on rows[0..n) of the corpus, n <= B */
int nvqa_ae_evaluate_rows(nvqa_ctx *ctx, int32_t n, const int64_t *rows, float *loss_out, int32_t *samples_out);
/* out[0] = training steps fed from host tokens so far (nvqa_ae_step*), out[1] = training steps fed from the resident corpus */
int nvqa_ae_step_routes(const nvqa_ctx *ctx, int64_t out[2]);
/* Decoding of NVQA_ARCH_AE1 / NVQA_ARCH_AE2 contexts: sample(sents, opt) of
 * misc/AutoEncoder_text_nostart.lua:134-210 (and the same block of misc/AutoEncoder.lua) with its second result, seqLogprobs.
 * Evaluate mode; the encoder is fed as nvqa_ae_evaluate feeds it (0 -> 1, up to the batch's last non-null column), the decoder
 * START and then its own picks.  n in 1..B rows; tokens [n x D]; images [n x E] or NULL (NVQA_ARCH_AE2; must be NULL on
 * NVQA_ARCH_AE1); seq_out [n x D] 1-based tokens, V+1 = END; logprobs_out [n x D] (may be NULL); opts = NULL is mode 0.  f32 and
 * the bf16 operand mode (the products are nvqa_ae_evaluate's; the selection always reads the f32 logits).  No collective is
 * issued: rank-local on a data-parallel context.  Every bad argument -- mode outside 0..2, temperature <= 0 or not finite in
 * mode 1, beam_size outside 1..8 or above V+1 or n beam_size > B in mode 2, n outside 1..B, images on NVQA_ARCH_AE1, V+1 > 16384
 * or R not a multiple of 4 -- is an error before anything is launched, as is a weak-paired context (their *_evaluate decodes
 * greedily).  No other entry point changes: nvqa_ae_evaluate* keeps its own argmax.
 * With z the f32 logits row of a decoder step and l = z - logsumexp(z):
 *   mode 0: the pick is the first maximum of z (the tokens equal nvqa_ae_evaluate's samples_out); logprobs_out = l[pick].
 *   mode 1: w_c = exp((z_c - max z) / temperature); u = (h >> 8) 2^-24, h = nvqa_hash32 of (seed, step, NVQA_SITE_AE_SAMPLE, b D + s), b
 *     the row in the caller's order and s = 0..D-1 the position; the pick is the smallest c with sum_{j<=c} w_j > u sum_j w_j
 *     (the last c with w_c > 0 if rounding leaves none); logprobs_out = l[pick], untempered (logprobs:gather, :195).  The sums
 *     run in a fixed order of the kernel's own: same input, same bits.
 *   mode 2: a plain beam search, the library's own definition (the reference names sample_beam at :138 and does not ship it).
 *     Each sentence keeps K = beam_size hypotheses on n K <= B decoder rows; a hypothesis' score is the sum of its tokens' l, no
 *     length normalisation.  At position 0 only hypothesis 0 is expanded; from then on a live hypothesis k offers (k, c) with
 *     score S_k + l_kc and a finished one (last token END) offers itself once, score unchanged, ranked as (k, END).  The K best
 *     survive, ties to the smaller k (V+1) + c, ordered best first; a survivor takes its parent's state, tokens and log-probs.
 *     After D positions seq_out / logprobs_out are hypothesis 0's tokens and their l, END included, zeros behind it.  With
 *     K = 1 the tokens equal mode 0's up to and including the first END (mode 0, like the reference, decodes on behind it). */
int nvqa_ae_sample(nvqa_ctx *ctx, int32_t n, const float *images, const int32_t *tokens, const nvqa_sample_opts *opts,
                   int32_t *seq_out, float *logprobs_out);
/* nvqa_ae_sample on rows[0..n) of the resident corpus (nvqa_ae_corpus_load; AE2: zero image rows) */
int nvqa_ae_sample_rows(nvqa_ctx *ctx, int32_t n, const int64_t *rows, const nvqa_sample_opts *opts, int32_t *seq_out,
                        float *logprobs_out);
/* ---- weak-paired auto-encoder (NVQA_ARCH_AE2_WP contexts) ---- */
/* 004_train_arch2_weakpaired_autoencoder_{vgg,inc}.lua with misc/AutoEncoderNull.lua.  The CNN body is frozen and runs
 * outside: feats [B x I] are its output (vgg: post-ReLU fc7 as nvqa_vgg16_fc7 returns it, I = 4096; inc: I = 2048).  The
 * library L2-normalises them (in place on its copy, the caller's rows only) and forms the encoder's step-0 input
 * x0 = f^ W_p^T + b_p.  The encoder then runs START and enc_tokens (0 -> 1) for 2 + tmax(enc_tokens) steps; enc_tokens =
 * NULL is the null sentence (2 steps).  The decoder and the criterion read tokens, for tmax(tokens) + 1 steps.  The lookup
 * table is frozen: its slice of nvqa_get_grads is zero, and nvqa_adam_update clamps, decays, updates and takes its
 * statistics over [encoder | decoder] only.  nvqa_ae_step*, nvqa_ae_evaluate* and nvqa_rmsprop_update return an error on
 * such a context; the calls below return an error on every other context.
 * nvqa_ae_wp_step: one training forward + criterion + backward; the projection's gradient is kept for
 * nvqa_ae_wp_get_projection_grads / nvqa_ae_wp_projection_adam. */
int nvqa_ae_wp_step(nvqa_ctx *ctx, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                    const nvqa_dropout *dropout, float *loss_out);
/* Evaluate-mode loss and (samples_out not NULL) greedy decoding of n <= B rows; feats [n x I], enc_tokens [n x D] or NULL,
 * tokens [n x D].  eval_split feeds enc_tokens = tokens (forward{feats, labels, labels}). */
int nvqa_ae_wp_evaluate(nvqa_ctx *ctx, int32_t n, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                        float *loss_out, int32_t *samples_out);
/* The projection Linear(I, E) (build_cnn's last module): w [E x I] (Torch layout), b [E].  nvqa_init_params sets
 * w = uniform(lo, hi) from its seed and b = 0, as build_cnn does, and resets the projection's Adam state. */
int nvqa_ae_wp_set_projection(nvqa_ctx *ctx, const float *w, const float *b);
int nvqa_ae_wp_get_projection(nvqa_ctx *ctx, float *w_out, float *b_out);
/* dW_p = dx0^T f^ and db_p = colsum(dx0) of the last step, dx0 = d(loss)/d(x0) */
int nvqa_ae_wp_get_projection_grads(nvqa_ctx *ctx, float *w_out, float *b_out);
/* The projection's own update (the cnn branch of the script, :318-325, :456-467): g += wd * x (wd != 0), then
 * g = clamp(g, -clamp, clamp) (clamp > 0) -- the reverse of nvqa_adam_update's order -- then adam() with a step counter of
 * its own.  stats_out (may be NULL; synchronises) = {||W_p||_2 (weight only), count(|lr g| >= 0.01 |x|) over W_p and b_p}
 * of x before the update. */
int nvqa_ae_wp_projection_adam(nvqa_ctx *ctx, float lr, float beta1, float beta2, float eps, float wd, float clamp,
                               float stats_out[2]);
/* The same update with the three rules of the scripts' -cnn_optim: rule = NVQA_OPT_SGD | NVQA_OPT_SGDM | NVQA_OPT_ADAM (further
 * down; any other rule is an error).  The order (wd, then clamp), stats_out and the contexts are those of
 * nvqa_ae_wp_projection_adam.  ADAM shares that call's state and step counter and gives the same bits; SGDM owns a velocity
 * buffer (allocated and zeroed on first use, zeroed again by nvqa_init_params); cnnFinalLearningScales is 1 on this Linear. */
int nvqa_ae_wp_projection_update(nvqa_ctx *ctx, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                                 float stats_out[2]);
/* ---- arch1 weak-paired auto-encoder (NVQA_ARCH_AE1_WP contexts) ---- */
/* 004_train_arch1_weakpaired_autoencoder_{vgg,inc}.lua with misc/AutoEncoder_vqa_arch.lua.  The flat vector is
 * [encoder | decoder | multimodal] with multimodal = W_q [2R x 2R], b_q [2R], W_v [2R x I], b_v [2R] (netdef.AxB(2R, I, 2R));
 * the lookup table LookupTable -> Tanh is frozen, evaluates without its Dropout even in training, and lives outside the vector
 * (the two calls at the end).  feats [B x I] are the frozen CNN body's output; the library L2-normalises its copy (the
 * caller's rows only) into f^.  With j = [c_T | h_T] the encoder's final state (enc_tokens, 0 -> 1, tmax(enc_tokens) steps) or
 * the caller's enc_state [B x 2R] (encoder_skip_flag = 1: the encoder does not run and its gradient segment is zero):
 *   m = D_Z (tanh(W_q (D_Q j) + b_q) * tanh(W_v (D_V f^) + b_v)),  decoder state (c, h) = (c_T + m[:, :R], h_T + m[:, R:]),
 * then AE1's decoder, projection and criterion over tokens.  Every other step / evaluate entry point, nvqa_comm_init,
 * nvqa_set_precision(ctx, 1) and nvqa_rmsprop_update return an error on such a context; the calls below return an error on
 * every other context.  nvqa_adam_update runs over the whole vector.
 * nvqa_ae1_wp_step: exactly one of enc_tokens [B x D] and enc_state [B x 2R] is non-NULL; dfeats_out [B x I] (may be NULL) =
 * d(loss)/d(f^), the module's gradInput for the features. */
int nvqa_ae1_wp_step(nvqa_ctx *ctx, const float *feats, const int32_t *enc_tokens, const float *enc_state,
                     const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out);
/* Evaluate-mode loss and (samples_out [n x D] not NULL) greedy decoding of n <= B rows, the encoder run on enc_tokens [n x D]
 * (eval_split feeds enc_tokens = tokens with the flag at 0); feats [n x I], tokens [n x D]. */
int nvqa_ae1_wp_evaluate(nvqa_ctx *ctx, int32_t n, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                         float *loss_out, int32_t *samples_out);
/* Evaluate-mode encoder only: state_out [n x 2R] = [c_T | h_T] of n <= B rows (the sentence vectors whose corpus mean the skip
 * mode is fed). */
int nvqa_ae1_wp_encode(nvqa_ctx *ctx, int32_t n, const int32_t *enc_tokens, float *state_out);
/* The frozen lookup table W_lk [(V+1) x E] (row V = START); no update ever touches it. */
int nvqa_ae1_wp_set_lookup(nvqa_ctx *ctx, const float *w);
int nvqa_ae1_wp_get_lookup(nvqa_ctx *ctx, float *w_out);
/* ---- the weak-paired steps with the VGG-16 body in the loop ---- */
/* The `cnn` forward of the weak-paired scripts in front of the step: images_u8 [B x 3 x S x S] (evaluate: [n x ...]), window
 * origin and body_dropout as nvqa_vgg16_fc7_raw takes them.  The body runs on the extractor's stream; the context's stream
 * waits for it and L2-normalises the features into the slot the host-fed call fills, and from there on the call IS
 * nvqa_ae_wp_step / nvqa_ae_wp_evaluate / nvqa_ae1_wp_step / nvqa_ae1_wp_evaluate: the results are bit-equal to those calls
 * given nvqa_vgg16_fc7_raw's features.  The features never visit the host; with loss_out = NULL (and dfeats_out = NULL) a step
 * waits for nothing but the previous batch's host-to-device copies.  The body is frozen: dfeats_out stays d(loss)/d(f^).
 * An error before anything is launched: what the host-fed call refuses, what nvqa_vgg16_fc7_raw refuses, a context of the
 * other arch, an extractor whose feature width is not dims.I or that lives on another device. */
int nvqa_ae_wp_step_images(nvqa_ctx *ctx, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                           const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                           const nvqa_dropout *dropout, float *loss_out);
int nvqa_ae_wp_evaluate_images(nvqa_ctx *ctx, nvqa_vgg *vgg, int32_t n, const uint8_t *images_u8, int S, int xoff, int yoff,
                               const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                               float *loss_out, int32_t *samples_out);
int nvqa_ae1_wp_step_images(nvqa_ctx *ctx, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                            const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const float *enc_state,
                            const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out);
int nvqa_ae1_wp_evaluate_images(nvqa_ctx *ctx, nvqa_vgg *vgg, int32_t n, const uint8_t *images_u8, int S, int xoff, int yoff,
                                const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                                float *loss_out, int32_t *samples_out);
/* The weak-paired steps with the body fine-tuning.  nvqa_ae_wp_step_dfeats: nvqa_ae_wp_step that also
 * returns d(loss)/d(f^) = dx0 W_p [B x I] (one more product; loss and gradients keep nvqa_ae_wp_step's bits).  The two
 * *_finetune steps take a training-enabled extractor and run its training forward, the step of the same name without the
 * suffix, nn.L2Normalize's backward and the body's backward; d f^ goes from the context's stream to the extractor's on the
 * device and the extractor's stream waits for it.  The result -- loss, nvqa_get_grads, the projection's gradients,
 * nvqa_vgg16_get_grads -- is bit-equal to nvqa_vgg16_train_forward_raw, the host-fed step with dfeats_out, then
 * nvqa_vgg16_backward(vgg, dfeats, B, 1).  Errors before anything is launched: those of the step without the suffix, and an
 * extractor that is not training-enabled. */
int nvqa_ae_wp_step_dfeats(nvqa_ctx *ctx, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                           const nvqa_dropout *dropout, float *loss_out, float *dfeats_out);
int nvqa_ae_wp_step_images_finetune(nvqa_ctx *ctx, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                    const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                                    const nvqa_dropout *dropout, float *loss_out);
int nvqa_ae1_wp_step_images_finetune(nvqa_ctx *ctx, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                     const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const float *enc_state,
                                     const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out);
/* Valid on every context.  One pass over the flat vector: g = clamp(g, -clamp, clamp) (clamp > 0), g += wd * x, then
 * adam() of misc/optim_updates.lua:78-111 (step counter held by the context, reset by nvqa_init_params).
 * stats_out (may be NULL; synchronises) = {||x||_2, count(|lr g| >= 0.01 |x|)} of x before the update, g after clamp + wd
 * (the log line of 001_train_arch1_text_autoencoder.lua:266-268). */
int nvqa_adam_update(nvqa_ctx *ctx, float lr, float beta1, float beta2, float eps, float wd, float clamp,
                     float stats_out[2]);
/* The six update rules of misc/optim_updates.lua (-optim rmsprop|adagrad|sgd|sgdm|sgdmom|adam of the seven scripts of
 * 001_train_autoencoder), each one fused pass over the flat vector.  Valid on every context, with nvqa_adam_update's contract
 * for every rule: per-segment gradient scale (nvqa_set_grad_scales x 1/world), then g = clamp(g, -clamp, clamp) (clamp > 0), then
 * g += wd * x (wd != 0), then the rule; stats_out (may be NULL; synchronises) = {||x||_2, count(|lr g| >= 0.01 |x|)} of x before
 * the update, g after clamp + wd; NVQA_ARCH_AE2_WP: [encoder | decoder] only, the frozen lookup table keeps its bits and the
 * statistics leave it out; the step-skip words and the data-parallel status word are handled as there, and with a communicator
 * the global batch's gradient is applied.  Arguments a rule does not use are ignored.  An error for an unknown rule and before
 * any step.
 * State: SGD has none.  SGDM, SGDMOM and ADAGRAD own one buffer each, allocated and zeroed on first use and zeroed again by
 * nvqa_init_params.  RMSPROP uses the buffer of nvqa_rmsprop_update, ADAM the buffers and the step counter of nvqa_adam_update:
 * with equal arguments the old and the new entry point give the same bits and may be interleaved on one context.  Through this
 * call RMSPROP runs on the weak-paired contexts and with per-segment scales on an auto-encoder context too
 * (nvqa_rmsprop_update itself keeps both refusals).
 * HBM traffic per parameter: 12 B (SGD), 20 B (the four one-buffer rules), 28 B (ADAM). */
#define NVQA_OPT_SGD     0  /* sgd()     optim_updates.lua:4-10            x -= lr g                   */
#define NVQA_OPT_SGDM    1  /* sgdm()    :12-24  v = a v + lr g;            x -= v                      */
#define NVQA_OPT_SGDMOM  2  /* sgdmom()  :26-40  m' = a m - lr g;           x += -a m + (1 + a) m'      */
#define NVQA_OPT_ADAGRAD 3  /* adagrad() :42-57  m += g g;                  x -= lr g / (sqrt(m) + eps) */
#define NVQA_OPT_RMSPROP 4  /* rmsprop() :60-76  m = a m + (1 - a) g g;     x -= lr g / (sqrt(m) + eps) */
#define NVQA_OPT_ADAM    5  /* adam()    :78-111 as nvqa_adam_update (alpha = beta1, beta = beta2)      */
int nvqa_optim_update(nvqa_ctx *ctx, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                      float stats_out[2]);

/* ---- measurement ------------------------------------------------------ */
/* HIP-event timing of kernel groups on the stream they are launched on.
 * enable=1 brackets every launch with events (slows the step; bench.py uses a
 * separate timed pass for it). Names: see nvqa_profile_name(). */
int nvqa_profile_enable(nvqa_ctx *ctx, int enable);
int nvqa_profile_reset(nvqa_ctx *ctx);
int nvqa_profile_count(const nvqa_ctx *ctx);
const char *nvqa_profile_name(const nvqa_ctx *ctx, int idx);
/* total_ms and launches accumulated since reset; flops = algorithmic FLOPs issued */
int nvqa_profile_get(nvqa_ctx *ctx, int idx, double *total_ms, int64_t *launches, double *flops,
                     double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* NVQA_H */
