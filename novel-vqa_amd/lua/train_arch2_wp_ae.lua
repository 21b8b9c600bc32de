--[[
train_arch2_wp_ae.lua -- 001_train_autoencoder/004_train_arch2_weakpaired_autoencoder_vgg.lua (and _inc.lua: -nhimage 2048,
-learning_rate 3e-5) with the hot path on libnvqa.

Same command-line options (:27-74, minus -backend / -language_eval / -cnn_proto / -cnn_model), same log line
(:302-306), learning-rate decay (:443-451), updates (:453-467) and stopping rules (:470-478).  What changed:
  * The CNN body is frozen (-finetune_cnn_after only starts the update of its final Linear, the projection) and runs outside:
    -input_feats_h5 holds its output per caption, /feats/train and /feats/val [N x I] (vgg: post-ReLU fc7 as nvqa_vgg16_fc7
    returns it), row i belonging to /labels/<split> row i.  DataLoaderWeakPaired's lockstep walk and wrap rule are kept.
    With -body_in_loop 1 the body runs inside the step instead, as in the reference: uint8 images from /images/<split> of
    -input_h5 (only a batch's rows are read), a random 224 window per training batch, the central one in eval_split, the RGB
    mean, VGG-16 up to module 38 with the weights of -cnn_weights, all on the device (nvqa_ae_wp_step_images; DESIGN.md
    section 9.10).  drop6 / drop7 are live in training; -body_dropout_in_eval 1 keeps them live in eval_split too, which is
    what the reference script does (it never calls cnn:evaluate()); the default evaluates the model as designed.
  * AutoEncoderNull, L2Normalize + Linear and LanguageModelCriterion are one library context of arch NVQA_ARCH_AE2_WP;
    protos.ae's parameters come from -start_from_text, the flat-vector table AETrainer.export_params writes for a text
    auto-encoder of arch NVQA_ARCH_AE2 (the reference loads the whole protos.ae, :127-129).
  * The null-sentence draw (:289-295) uses torch.uniform() under torch.manualSeed(-seed), not Lua's math.random.
  * Instead of the thin nn checkpoints it writes what 003_train_ae_based_wp_{vgg,inc}.lua take from them: {encoder,
    lookup_table, cnn_w = [W_p | b_p], layout = 'nvqa'}, read by train_arch2_ae.lua -ae_cnn 1 and
    VQATrainer.init_from_autoencoder(..., with_cnn=True).
Needs LuaJIT + torch + hdf5 + cjson; NOT executable in the build image, where novel-vqa_amd/host/ae.py (WeakPairedAETrainer)
is the executed twin.
]]--
require 'torch'
require 'hdf5'
local cjson = require 'cjson'
local ffi = require 'ffi'
local nvqa = require 'nvqa_ffi'

cmd = torch.CmdLine()
cmd:option('-input_h5','data/data.h5','path to the h5file containing the preprocessed dataset (/labels/<split>)')
cmd:option('-input_feats_h5','data/feats.h5','path to the h5file with the frozen CNN body\'s features (/feats/<split>)')
cmd:option('-input_json','data/data.json','path to the json file containing additional info and vocab')
cmd:option('-start_from_text', '', 'flat-vector table of the arch2 text auto-encoder (AETrainer.export_params)')
cmd:option('-body_in_loop', 0, '1: run the VGG-16 body inside the step on the raw images /images/<split> of -input_h5 (needs -cnn_weights)')
cmd:option('-cnn_weights', '', 'flat float32 file of the VGG-16 weights in nvqa_vgg16_set_weights order (-body_in_loop 1)')
cmd:option('-finetune_body', 0, '1: from -finetune_cnn_after on the VGG-16 body learns too (-body_in_loop 1): its backward inside the step, -cnn_optim on all its weights at scale 0.01')
cmd:option('-body_dropout_in_eval', 0, '1: drop6 / drop7 stay live in eval_split, as in the reference script (-body_in_loop 1)')
cmd:option('-rnn_size',512,'size of the rnn in number of hidden nodes in each layer')
cmd:option('-input_encoding_size',512,'the encoding size of each token in the vocabulary, and the image.')
cmd:option('-nhimage', 4096, 'feature width of the CNN body (vgg fc7 4096, inception 2048)')
cmd:option('-max_iters', 22501, 'max number of iterations to run for (-1 = run forever)')
cmd:option('-batch_size',20,'what is the batch size in number of sentences per batch?')
cmd:option('-grad_clip',0.1,'clip gradients at this value')
cmd:option('-drop_prob_ae', 0.5, 'strength of dropout in the AutoEncoder RNN')
cmd:option('-optim','adam','what update to use? rmsprop|adagrad|sgd|sgdm|sgdmom|adam')
cmd:option('-learning_rate',1e-5,'learning rate')
cmd:option('-learning_rate_decay_start', -1, 'at what iteration to start decaying learning rate? (-1 = dont)')
cmd:option('-learning_rate_decay_every', 50000, 'every how many iterations thereafter to drop LR by half?')
cmd:option('-optim_alpha',0.8,'alpha for adagrad/rmsprop/momentum/adam')
cmd:option('-optim_beta',0.999,'beta used for adam')
cmd:option('-optim_epsilon',1e-8,'epsilon that goes into denominator for smoothing')
cmd:option('-weight_decay', 1e-6, 'L2 regularization parameter')
cmd:option('-finetune_cnn_after', -1, 'After what iteration do we start updating the projection? (-1 = never)')
cmd:option('-rand_val', 0.5, 'probability of feeding the null sentence to the encoder')
cmd:option('-cnn_optim','adam','optimization to use for the projection: sgd|sgdm|adam')
cmd:option('-cnn_optim_alpha',0.8,'alpha for momentum / adam of the projection')
cmd:option('-cnn_optim_beta',0.999,'beta for adam of the projection')
cmd:option('-cnn_learning_rate',1e-5,'learning rate for the projection')
cmd:option('-cnn_weight_decay', 0, 'L2 weight decay just for the projection')
cmd:option('-val_sentences_use', 30000, 'how many sentences to use when periodically evaluating the validation loss?')
cmd:option('-save_checkpoint_every', 10000, 'how often to evaluate and save the best export table?')
cmd:option('-save_model_every', 22500, 'how often to save an export table regardless of the validation loss?')
cmd:option('-checkpoint_path', '', 'folder to save checkpoints into (empty = this folder)')
cmd:option('-id', '', 'an id identifying this run/job')
cmd:option('-seed', 123, 'random number generator seed to use')
cmd:option('-gpuid', 0, 'which MI355X to use')
opt = cmd:parse(arg)
torch.manualSeed(opt.seed)

-- data (misc/DataLoaderWeakPaired.lua) ---------------------------------------------------------------------------------
local f = io.open(opt.input_json, 'r'); local info = cjson.decode(f:read('*a')); f:close()
local vocab_size = 0
for _ in pairs(info.ix_to_word) do vocab_size = vocab_size + 1 end
local h5 = hdf5.open(opt.input_h5, 'r')
local labels = {train = h5:read('/labels/train'):all():int(), val = h5:read('/labels/val'):all():int()}
h5:close()
local feats, images, body, img_size = nil, nil, nil, 0
if opt.body_in_loop == 1 then                        -- the reference's stage: raw images, the VGG-16 body inside the step
  assert(string.len(opt.cnn_weights) > 0, '-body_in_loop 1 needs -cnn_weights')
  local h5i = hdf5.open(opt.input_h5, 'r')           -- stays open: a batch reads its own rows
  images = {train = h5i:read('/images/train'), val = h5i:read('/images/val')}
  img_size = images.train:dataspaceSize()[3]
  body = nvqa.body_open(opt)
  if opt.finetune_body == 1 then nvqa.check(nvqa.lib.nvqa_vgg16_train_enable(body, 1)) end
else
  assert(opt.finetune_body ~= 1, '-finetune_body 1 needs -body_in_loop 1')
  h5 = hdf5.open(opt.input_feats_h5, 'r')
  feats = {train = h5:read('/feats/train'):all():float(), val = h5:read('/feats/val'):all():float()}
  h5:close()
  assert(feats.train:size(2) == opt.nhimage, 'feature width does not match -nhimage')
end
local seq_length = labels.train:size(2)
local iterators = {train = 1, val = 1}

local function getBatch(split, batch_size)          -- DataLoaderWeakPaired:getBatch (:58-103): captions and images in lockstep
  local data, max_index, it = labels[split], labels[split]:size(1), iterators[split]
  local ranges, wrapped = nil, false                  -- the rows of the batch, 1-based inclusive, in batch order
  if it + batch_size - 1 > max_index then
    wrapped = true
    if it < max_index then
      ranges = {{it, max_index}, {1, batch_size - (max_index - it + 1)}}
    else
      ranges = {{1, batch_size}}
    end
    iterators[split] = 1
  else
    ranges = {{it, it + batch_size - 1}}
    iterators[split] = it + batch_size
  end
  local batch = torch.IntTensor(batch_size, seq_length)
  local fb = body and torch.ByteTensor(batch_size, 3, img_size, img_size) or torch.FloatTensor(batch_size, opt.nhimage)
  local at = 1
  for _, r in ipairs(ranges) do
    local n = r[2] - r[1] + 1
    batch:narrow(1, at, n):copy(data:narrow(1, r[1], n))
    if body then                                      -- only the batch's rows of /images/<split> are ever read
      fb:narrow(1, at, n):copy(images[split]:partial({r[1], r[2]}, {1, 3}, {1, img_size}, {1, img_size}))
    else
      fb:narrow(1, at, n):copy(feats[split]:narrow(1, r[1], n))
    end
    at = at + n
  end
  return batch, fb, wrapped
end

-- the context: [encoder | decoder | lookup] from the text model; W_p uniform(-0.08, 0.08), b_p = 0 (build_cnn) -----------
opt.num_layers = 1
opt.common_embedding_size, opt.num_output = 0, 0
local ctx = nvqa.create(5, opt, vocab_size, seq_length, opt.gpuid)
nvqa.check(nvqa.lib.nvqa_init_params(ctx, opt.seed, -0.08, 0.08))
local n_params = tonumber(nvqa.lib.nvqa_param_count(ctx))
do
  local t = torch.load(opt.start_from_text)
  assert(t.layout == 'nvqa' and t.params:nElement() == n_params, 'the text model does not match this auto-encoder')
  nvqa.check(nvqa.lib.nvqa_set_params(ctx, nvqa.fptr(t.params:float():contiguous())))
end
local E, I = opt.input_encoding_size, opt.nhimage

local function eval_split(split)                    -- eval_split (:199-260): forward{feats, labels, labels}
  iterators[split] = 1
  local loss_sum, evals, n = 0, 0, 0
  local loss = ffi.new('float[1]')
  while true do
    local batch, fb, wrapped = getBatch(split, opt.batch_size)
    if body then
      local xoff, yoff = nvqa.crop_origin(img_size, false)
      nvqa.check(nvqa.lib.nvqa_ae_wp_evaluate_images(ctx, body, opt.batch_size, nvqa.bptr(fb), img_size, xoff, yoff,
                                                     nvqa.body_dropout(opt.body_dropout_in_eval == 1, opt.seed, 0),
                                                     nvqa.iptr(batch), nvqa.iptr(batch), loss, nil))
    else
      nvqa.check(nvqa.lib.nvqa_ae_wp_evaluate(ctx, opt.batch_size, nvqa.fptr(fb), nvqa.iptr(batch), nvqa.iptr(batch), loss, nil))
    end
    loss_sum = loss_sum + loss[0]; evals = evals + 1
    n = n + opt.batch_size
    if wrapped then break end
    if n >= opt.val_sentences_use then break end
  end
  return loss_sum / evals
end

local function export(path)                          -- what 003_train_ae_based_wp_*.lua take from the checkpoint
  local x = torch.FloatTensor(n_params)
  nvqa.check(nvqa.lib.nvqa_get_params(ctx, nvqa.fptr(x)))
  local seg = ffi.new('size_t[3]'); nvqa.check(nvqa.lib.nvqa_segments(ctx, seg))
  local s0, s1 = tonumber(seg[0]), tonumber(seg[1])
  local lookup = x:narrow(1, s0 + s1 + 1, tonumber(seg[2])):view(vocab_size + 1, E)
  local cnn_w = torch.FloatTensor(E * I + E)
  nvqa.check(nvqa.lib.nvqa_ae_wp_get_projection(ctx, nvqa.fptr(cnn_w), nvqa.fptr(cnn_w:narrow(1, E * I + 1, E))))
  torch.save(path, {encoder = x:narrow(1, 1, s0):clone(), lookup_table = lookup:clone(), cnn_w = cnn_w, layout = 'nvqa'})
end

-- main loop (:292-478) ------------------------------------------------------------------------------------------------
local iter, loss0, best_score = 1, nil, nil
local loss, stats, cnn_stats = ffi.new('float[1]'), ffi.new('float[2]'), ffi.new('float[2]')
local frozen_stats = nil
local checkpoint_path = paths.concat(opt.checkpoint_path, 'model_id' .. opt.id)
while true do
  local batch, fb = getBatch('train', opt.batch_size)
  local enc = batch
  if torch.uniform() <= opt.rand_val then enc = nil end                          -- the null sentence (:289-295)
  local body_learns = opt.finetune_body == 1 and opt.finetune_cnn_after >= 0 and iter >= opt.finetune_cnn_after
  if body_learns then                                                            -- ... + cnn:backward(data.imgs, dfeats) (:307-310)
    local xoff, yoff = nvqa.crop_origin(img_size, true)
    nvqa.check(nvqa.lib.nvqa_ae_wp_step_images_finetune(ctx, body, nvqa.bptr(fb), img_size, xoff, yoff,
                                                        nvqa.body_dropout(true, opt.seed, iter), enc and nvqa.iptr(enc) or nil,
                                                        nvqa.iptr(batch), nvqa.dropout(1, opt.drop_prob_ae, opt.seed, iter), loss))
  elseif body then                                                               -- prepro(data.images, true, ...) + cnn:forward
    local xoff, yoff = nvqa.crop_origin(img_size, true)
    nvqa.check(nvqa.lib.nvqa_ae_wp_step_images(ctx, body, nvqa.bptr(fb), img_size, xoff, yoff,
                                               nvqa.body_dropout(true, opt.seed, iter), enc and nvqa.iptr(enc) or nil,
                                               nvqa.iptr(batch), nvqa.dropout(1, opt.drop_prob_ae, opt.seed, iter), loss))
  else
    nvqa.check(nvqa.lib.nvqa_ae_wp_step(ctx, nvqa.fptr(fb), enc and nvqa.iptr(enc) or nil, nvqa.iptr(batch),
                                        nvqa.dropout(1, opt.drop_prob_ae, opt.seed, iter), loss))
  end
  local learning_rate, cnn_learning_rate = opt.learning_rate, opt.cnn_learning_rate
  if iter > opt.learning_rate_decay_start and opt.learning_rate_decay_start >= 0 then
    local decay_factor = math.pow(0.5, (iter - opt.learning_rate_decay_start) / opt.learning_rate_decay_every)
    learning_rate = learning_rate * decay_factor
    cnn_learning_rate = cnn_learning_rate * decay_factor
  end
  if opt.optim == 'adam' then  -- the script's default keeps its own entry point: the same kernel, state and bits as the rule
    nvqa.check(nvqa.lib.nvqa_adam_update(ctx, learning_rate, opt.optim_alpha, opt.optim_beta, opt.optim_epsilon,
                                         opt.weight_decay, opt.grad_clip, stats))
  else
    nvqa.optim_update(ctx, opt, learning_rate, stats)
  end
  if opt.finetune_cnn_after >= 0 and iter >= opt.finetune_cnn_after then
    local clamp = 0
    if opt.cnn_weight_decay > 0 then clamp = opt.grad_clip end                   -- wd, then clamp, as lossFun (:318-322)
    local cnn_rule = nvqa.CNN_OPT[opt.cnn_optim]
    if cnn_rule == nil then error('bad option for opt.cnn_optim (sgd | sgdm | adam)') end
    if opt.cnn_optim == 'adam' then  -- as for -optim: the default keeps its own entry point
      nvqa.check(nvqa.lib.nvqa_ae_wp_projection_adam(ctx, cnn_learning_rate, opt.cnn_optim_alpha, opt.cnn_optim_beta,
                                                     opt.optim_epsilon, opt.cnn_weight_decay, clamp, cnn_stats))
    else
      nvqa.check(nvqa.lib.nvqa_ae_wp_projection_update(ctx, cnn_rule, cnn_learning_rate, opt.cnn_optim_alpha, opt.cnn_optim_beta,
                                                       opt.optim_epsilon, opt.cnn_weight_decay, clamp, cnn_stats))
    end
    frozen_stats = nil
    if body_learns then                                                          -- the whole cnn vector, cnnFinalLearningScales 0.01 (:194, :457-466)
      nvqa.check(nvqa.lib.nvqa_vgg16_update(body, cnn_rule, cnn_learning_rate, opt.cnn_optim_alpha, opt.cnn_optim_beta,
                                            opt.optim_epsilon, opt.cnn_weight_decay, clamp, 0.01, nil))
    end
  else
    if frozen_stats == nil then                                                  -- a zero gradient: the zero entries count
      local w = torch.FloatTensor(E * I + E)
      nvqa.check(nvqa.lib.nvqa_ae_wp_get_projection(ctx, nvqa.fptr(w), nvqa.fptr(w:narrow(1, E * I + 1, E))))
      frozen_stats = {w:narrow(1, 1, E * I):norm(), w:eq(0):sum()}
    end
    cnn_stats[0], cnn_stats[1] = frozen_stats[1], frozen_stats[2]
  end
  print(string.format('iter %d: loss: %.3f | # updates: %4d | paramsNorm: %.4f | # cnn updates: %4d | cnnParamsNorm: %.4f',
                      iter, loss[0], stats[1], stats[0], cnn_stats[1], cnn_stats[0]))
  if iter % opt.save_checkpoint_every == 0 or iter == opt.max_iters then
    local val_loss = eval_split('val')
    print('validation loss: ', val_loss)
    if best_score == nil or -val_loss > best_score then
      best_score = -val_loss
      export(checkpoint_path .. '_vqa.t7')
      print('wrote BEST export table to ' .. checkpoint_path .. '_vqa.t7')
    end
  end
  if iter % opt.save_model_every == 0 then
    export(checkpoint_path .. iter .. '_vqa.t7')
    print('wrote export table to ' .. checkpoint_path .. iter .. '_vqa.t7')
  end
  iter = iter + 1
  if loss0 == nil then loss0 = loss[0] end
  if loss[0] > loss0 * 20 then print('loss seems to be exploding, quitting.'); break end
  if opt.max_iters > 0 and iter >= opt.max_iters then break end
end
