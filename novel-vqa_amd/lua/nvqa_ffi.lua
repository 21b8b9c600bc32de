--[[
nvqa_ffi.lua -- LuaJIT FFI binding of libnvqa.so (include/nvqa.h).

This is the reference-side stub a maintainer drops next to misc/RNNUtils.lua: the Torch7
scripts keep their CmdLine flags and data loading and replace the body of JdJ (and the
optim.rmsprop call) with calls into the library.  The cdef below mirrors include/nvqa.h
one to one; novel-vqa_amd/host/binding.py is the same binding for Python/ctypes and is the
twin that the test-suite actually executes (no LuaJIT in the build image).
]]--
local ffi = require 'ffi'

ffi.cdef[[
typedef struct nvqa_dims { int32_t arch, B, T, V, E, R, L, I, C, A; } nvqa_dims;
typedef struct nvqa_dropout { int32_t mode; float p; uint64_t seed; uint64_t step; } nvqa_dropout;
typedef struct nvqa_sample_opts { int32_t mode; int32_t beam_size; float temperature; int32_t pad_; uint64_t seed, step; } nvqa_sample_opts;
typedef struct nvqa_ctx nvqa_ctx;
int nvqa_create(const nvqa_dims *dims, int device, nvqa_ctx **out);
int nvqa_destroy(nvqa_ctx *ctx);
const char *nvqa_last_error(void);
int nvqa_sync(nvqa_ctx *ctx);
size_t nvqa_param_count(const nvqa_ctx *ctx);
int nvqa_segments(const nvqa_ctx *ctx, size_t sizes_out[3]);
int nvqa_init_params(nvqa_ctx *ctx, uint64_t seed, float lo, float hi);
int nvqa_set_params(nvqa_ctx *ctx, const float *params);
int nvqa_get_params(nvqa_ctx *ctx, float *params_out);
int nvqa_get_grads(nvqa_ctx *ctx, float *grads_out, float clamp);
int nvqa_step(nvqa_ctx *ctx, const int32_t *tokens, const int32_t *lengths, const float *img,
              const int32_t *labels, const nvqa_dropout *dropout, float *loss_out);
int nvqa_get_loss(nvqa_ctx *ctx, float *loss_out);
int nvqa_forward(nvqa_ctx *ctx, int32_t n, const int32_t *tokens, const int32_t *lengths,
                 const float *img, float *scores_out, int32_t *argmax_out);
int nvqa_evaluate(nvqa_ctx *ctx, int32_t n, const int32_t *tokens, const int32_t *lengths, const float *img,
                  const int32_t *labels, const int32_t *mc_ans, int32_t n_mc, float *scores_out,
                  int32_t *argmax_out, int32_t *mc_argmax_out, float *loss_out);
int nvqa_rmsprop_update(nvqa_ctx *ctx, float lr, float alpha, float eps, float wd, float clamp);
int nvqa_set_fusion(nvqa_ctx *ctx, int mode);
int nvqa_set_precision(nvqa_ctx *ctx, int bf16);
int nvqa_set_ref_quirks(nvqa_ctx *ctx, int flags);
int nvqa_param_norms(nvqa_ctx *ctx, float out[3]);
int nvqa_persistent_state(const nvqa_ctx *ctx, int out[2]);
int nvqa_wgrad_routes(const nvqa_ctx *ctx, int64_t out[3]);
int nvqa_dx0_routes(const nvqa_ctx *ctx, int64_t out[2]);
int nvqa_set_grad_scales(nvqa_ctx *ctx, const float scales[3]);
int nvqa_dataset_load(nvqa_ctx *ctx, int64_t n_q, const int32_t *questions, const int32_t *lengths,
                      const int32_t *img_pos, const int32_t *answers, int64_t n_img,
                      const float *feats, int l2_normalize);
int nvqa_step_indices(nvqa_ctx *ctx, const int64_t *qinds, const nvqa_dropout *dropout, float *loss_out);
int nvqa_comm_unique_id(void *id_out);
int nvqa_comm_init(nvqa_ctx *ctx, int rank, int world, const void *id);
const char *nvqa_comm_library(void);
typedef struct nvqa_vgg nvqa_vgg;
int nvqa_vgg16_create(int device, int width_div, int input_hw, int max_batch, nvqa_vgg **out);
int nvqa_vgg16_destroy(nvqa_vgg *vgg);
size_t nvqa_vgg16_weight_count(const nvqa_vgg *vgg);
int nvqa_vgg16_feature_dim(const nvqa_vgg *vgg);
int nvqa_vgg16_set_weights(nvqa_vgg *vgg, const float *flat);
int nvqa_vgg16_fc7(nvqa_vgg *vgg, const float *images, int n, float *feats_out);
int nvqa_vgg16_set_precision(nvqa_vgg *vgg, int bf16);
int nvqa_vgg16_preprocess(nvqa_vgg *vgg, const float *rgb, int n, int H, int W, float *out);
int nvqa_vgg16_fc7_raw(nvqa_vgg *vgg, const uint8_t *images, int n, int S, int xoff, int yoff,
                       const nvqa_dropout *body_dropout, float *feats_out);
int nvqa_vgg16_train_enable(nvqa_vgg *vgg, int on);
int nvqa_vgg16_train_forward_raw(nvqa_vgg *vgg, const uint8_t *images, int n, int S, int xoff, int yoff,
                                 const nvqa_dropout *dropout, float *feats_out);
int nvqa_vgg16_train_activation(nvqa_vgg *vgg, int which, float *out);
int nvqa_vgg16_backward(nvqa_vgg *vgg, const float *dfeats, int n, int through_l2norm);
int nvqa_vgg16_get_grads(nvqa_vgg *vgg, float *flat_out);
int nvqa_vgg16_get_weights(nvqa_vgg *vgg, float *flat_out);
int nvqa_vgg16_update(nvqa_vgg *vgg, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                      float scale, float stats_out[2]);
int nvqa_step_images(nvqa_ctx *ctx, nvqa_vgg *vgg, const float *images, const int32_t *tokens,
                     const int32_t *lengths, const int32_t *labels, const nvqa_dropout *dropout, float *loss_out);
int nvqa_ae_step(nvqa_ctx *ctx, const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out);
int nvqa_ae_evaluate(nvqa_ctx *ctx, int32_t n, const int32_t *tokens, float *loss_out, int32_t *samples_out);
int nvqa_ae_step_images(nvqa_ctx *ctx, const float *images, const int32_t *tokens, const nvqa_dropout *dropout,
                        float *loss_out, float *dimages_out);
int nvqa_ae_evaluate_images(nvqa_ctx *ctx, int32_t n, const float *images, const int32_t *tokens, float *loss_out,
                            int32_t *samples_out);
int nvqa_ae_set_precision(nvqa_ctx *ctx, int bf16);
int nvqa_ae_comm_init(nvqa_ctx *ctx, int rank, int world, const void *id);
int nvqa_ae_corpus_load(nvqa_ctx *ctx, int64_t n_rows, const int32_t *tokens);
int nvqa_ae_step_rows(nvqa_ctx *ctx, const int64_t *rows, const nvqa_dropout *dropout, float *loss_out);
int nvqa_ae_evaluate_rows(nvqa_ctx *ctx, int32_t n, const int64_t *rows, float *loss_out, int32_t *samples_out);
int nvqa_ae_step_routes(const nvqa_ctx *ctx, int64_t out[2]);
int nvqa_ae_sample(nvqa_ctx *ctx, int32_t n, const float *images, const int32_t *tokens, const nvqa_sample_opts *opts,
                   int32_t *seq_out, float *logprobs_out);
int nvqa_ae_sample_rows(nvqa_ctx *ctx, int32_t n, const int64_t *rows, const nvqa_sample_opts *opts, int32_t *seq_out,
                        float *logprobs_out);
int nvqa_adam_update(nvqa_ctx *ctx, float lr, float beta1, float beta2, float eps, float wd, float clamp,
                     float stats_out[2]);
int nvqa_optim_update(nvqa_ctx *ctx, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                      float stats_out[2]);
int nvqa_ae_wp_step(nvqa_ctx *ctx, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                    const nvqa_dropout *dropout, float *loss_out);
int nvqa_ae_wp_evaluate(nvqa_ctx *ctx, int32_t n, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                        float *loss_out, int32_t *samples_out);
int nvqa_ae_wp_set_projection(nvqa_ctx *ctx, const float *w, const float *b);
int nvqa_ae_wp_get_projection(nvqa_ctx *ctx, float *w_out, float *b_out);
int nvqa_ae_wp_get_projection_grads(nvqa_ctx *ctx, float *w_out, float *b_out);
int nvqa_ae_wp_projection_adam(nvqa_ctx *ctx, float lr, float beta1, float beta2, float eps, float wd, float clamp,
                               float stats_out[2]);
int nvqa_ae_wp_projection_update(nvqa_ctx *ctx, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                                 float stats_out[2]);
int nvqa_ae1_wp_step(nvqa_ctx *ctx, const float *feats, const int32_t *enc_tokens, const float *enc_state,
                     const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out);
int nvqa_ae1_wp_evaluate(nvqa_ctx *ctx, int32_t n, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                         float *loss_out, int32_t *samples_out);
int nvqa_ae1_wp_encode(nvqa_ctx *ctx, int32_t n, const int32_t *enc_tokens, float *state_out);
int nvqa_ae1_wp_set_lookup(nvqa_ctx *ctx, const float *w);
int nvqa_ae1_wp_get_lookup(nvqa_ctx *ctx, float *w_out);
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
int nvqa_ae_wp_step_dfeats(nvqa_ctx *ctx, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                           const nvqa_dropout *dropout, float *loss_out, float *dfeats_out);
int nvqa_ae_wp_step_images_finetune(nvqa_ctx *ctx, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                    const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                                    const nvqa_dropout *dropout, float *loss_out);
int nvqa_ae1_wp_step_images_finetune(nvqa_ctx *ctx, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                     const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const float *enc_state,
                                     const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out);
int nvqa_profile_enable(nvqa_ctx *ctx, int enable);
int nvqa_profile_reset(nvqa_ctx *ctx);
int nvqa_profile_count(const nvqa_ctx *ctx);
const char *nvqa_profile_name(const nvqa_ctx *ctx, int idx);
int nvqa_profile_get(nvqa_ctx *ctx, int idx, double *total_ms, int64_t *launches, double *flops, double *bytes);
]]

local M = {}
M.lib = ffi.load(os.getenv('NVQA_LIB') or 'nvqa')   -- libnvqa.so on the loader path

-- Torch raises Lua errors on misuse and the scripts never pcall: keep that fail-fast behaviour.
local function check(rc)
  if rc ~= 0 then error('libnvqa: ' .. ffi.string(M.lib.nvqa_last_error()), 2) end
end
M.check = check

function M.create(arch, opt, vocabulary_size, buffer_size, device)
  local d = ffi.new('nvqa_dims')
  d.arch = arch; d.B = opt.batch_size; d.T = buffer_size; d.V = vocabulary_size
  d.E = opt.input_encoding_size; d.R = opt.rnn_size
  d.L = (arch == 1) and opt.rnn_layer or opt.num_layers
  d.I = opt.nhimage; d.C = opt.common_embedding_size; d.A = opt.num_output
  local out = ffi.new('nvqa_ctx*[1]')
  check(M.lib.nvqa_create(d, device or 0, out))
  return ffi.gc(out[0], M.lib.nvqa_destroy), d
end

-- pointers to the storage of contiguous torch tensors (IntTensor / FloatTensor / LongTensor)
function M.iptr(t) return ffi.cast('const int32_t*', t:data()) end
function M.fptr(t) return ffi.cast('float*', t:data()) end
function M.lptr(t) return ffi.cast('const int64_t*', t:data()) end
function M.bptr(t) return ffi.cast('const uint8_t*', t:data()) end   -- ByteTensor: the raw images of /images/<split>

function M.dropout(mode, p, seed, step)
  local d = ffi.new('nvqa_dropout'); d.mode = mode; d.p = p; d.seed = seed; d.step = step
  return d
end

-- sample(sents, opt) of misc/AutoEncoder_text_nostart.lua:134-210 on the library: opt.sample_max (default 1), opt.beam_size
-- (default 1), opt.temperature (default 1.0) as there; opt.seed / opt.step key the multinomial draws.  sample_max = 1 with
-- beam_size > 1 is the beam (:138).  sents: IntTensor [n x D]; imgs: FloatTensor [n x E] or nil (arch2 only).  Returns
-- seq IntTensor [n x D] and seqLogprobs FloatTensor [n x D].
function M.sample_opts(opt)
  opt = opt or {}
  local o = ffi.new('nvqa_sample_opts')
  local sample_max, beam_size = opt.sample_max or 1, opt.beam_size or 1
  o.mode = (sample_max == 1) and ((beam_size > 1) and 2 or 0) or 1
  o.beam_size = beam_size; o.temperature = opt.temperature or 1.0; o.pad_ = 0
  o.seed = opt.seed or 0; o.step = opt.step or 0
  return o
end

function M.ae_sample(ctx, sents, opt, imgs)
  local n, D = sents:size(1), sents:size(2)
  local seq, lp = torch.IntTensor(n, D), torch.FloatTensor(n, D)
  check(M.lib.nvqa_ae_sample(ctx, n, imgs and M.fptr(imgs) or nil, M.iptr(sents), M.sample_opts(opt), ffi.cast('int32_t*', seq:data()),
                             M.fptr(lp)))
  return seq, lp
end

function M.ae_sample_rows(ctx, rows, D, opt)
  local n = rows:size(1)
  local seq, lp = torch.IntTensor(n, D), torch.FloatTensor(n, D)
  check(M.lib.nvqa_ae_sample_rows(ctx, n, M.lptr(rows), M.sample_opts(opt), ffi.cast('int32_t*', seq:data()), M.fptr(lp)))
  return seq, lp
end

-- -body_in_loop 1 of train_arch{1,2}_wp_ae.lua: the VGG-16 body (full width, 224 x 224 input) on opt.gpuid with the weights of
-- opt.cnn_weights, a flat float32 file in nvqa_vgg16_set_weights order (the caffemodel's blobs, layer by layer)
function M.body_open(opt)
  local out = ffi.new('nvqa_vgg*[1]')
  check(M.lib.nvqa_vgg16_create(opt.gpuid or 0, 1, 224, opt.batch_size, out))
  local vgg = ffi.gc(out[0], M.lib.nvqa_vgg16_destroy)
  local w = torch.FloatTensor(torch.FloatStorage(opt.cnn_weights))
  assert(w:nElement() == tonumber(M.lib.nvqa_vgg16_weight_count(vgg)), '-cnn_weights does not hold the VGG-16 weight vector')
  assert(M.lib.nvqa_vgg16_feature_dim(vgg) == opt.nhimage, 'the body\'s feature width does not match -nhimage')
  check(M.lib.nvqa_vgg16_set_weights(vgg, M.fptr(w)))
  return vgg
end

-- net_utils.prepro's window origin, 0-based: training torch.random(S - 224) per axis (x first, as there), evaluation the centre
function M.crop_origin(S, train)
  if S <= 224 then return 0, 0 end
  if train then
    local xoff = torch.random(S - 224) - 1
    return xoff, torch.random(S - 224) - 1
  end
  local c = math.max(0, math.ceil((S - 224) / 2) - 1)
  return c, c
end

-- the body's dropout (drop6 / drop7, p = 0.5) of iteration `step`; on = false: the body in evaluate mode
function M.body_dropout(on, seed, step)
  if not on then return nil end
  return M.dropout(1, 0.5, seed, step)
end

-- -optim / -cnn_optim of the scripts of 001_train_autoencoder -> NVQA_OPT_* (misc/optim_updates.lua)
M.OPT = {sgd = 0, sgdm = 1, sgdmom = 2, adagrad = 3, rmsprop = 4, adam = 5}
M.CNN_OPT = {sgd = 0, sgdm = 1, adam = 5}

-- The scripts' `perform a parameter update` block as one call: clamp, weight decay and the -optim rule in one pass, with the
-- log line's statistics in stats = {paramsNorm, # updates}.  learning_rate is the decayed rate; sgd takes the undecayed
-- opt.learning_rate, as every reference script passes it (sgd(params, grad_params, opt.learning_rate)).
function M.optim_update(ctx, opt, learning_rate, stats)
  local rule = M.OPT[opt.optim]
  if rule == nil then error('bad option opt.optim (rmsprop | adagrad | sgd | sgdm | sgdmom | adam)') end
  local lr = (opt.optim == 'sgd') and opt.learning_rate or learning_rate
  check(M.lib.nvqa_optim_update(ctx, rule, lr, opt.optim_alpha, opt.optim_beta, opt.optim_epsilon, opt.weight_decay,
                                opt.grad_clip, stats))
end

return M
