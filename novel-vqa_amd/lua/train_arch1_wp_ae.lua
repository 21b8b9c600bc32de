--[[
train_arch1_wp_ae.lua -- 001_train_autoencoder/004_train_arch1_weakpaired_autoencoder_vgg.lua (and _inc.lua: -nhimage 2048,
-batch_size 10) with the hot path on libnvqa.

Same command-line options (:27-78, minus -backend / -language_eval / -cnn_proto / -cnn_model and the cnn optimiser's, whose
body is frozen here; -img_average_path is dropped: the script loads that vector and never uses it), same learning-rate decay,
update (clamp, then weight decay, :335-341, then the -optim rule) and stopping rules.  What changed:
  * The CNN body is frozen and runs outside: -input_feats_h5 holds its output per caption, /feats/train and /feats/val
    [N x I], row i belonging to /labels/<split> row i.  DataLoaderWeakPaired's lockstep walk and wrap rule are kept.
    With -body_in_loop 1 the body runs inside the step instead, as in the reference: uint8 images from /images/<split> of
    -input_h5 (only a batch's rows are read), a random 224 window per training batch, the central one in eval_split, the RGB
    mean, VGG-16 up to module 38 with the weights of -cnn_weights, all on the device (nvqa_ae1_wp_step_images; DESIGN.md
    section 9.10).  drop6 / drop7 are live in training and off in eval_split, as the script's cnn:training() / cnn:evaluate().
  * AutoEncoder_vqa (misc/AutoEncoder_vqa_arch.lua), L2Normalize and LanguageModelCriterion are one library context of arch
    NVQA_ARCH_AE1_WP.  Encoder, decoder and the frozen lookup table come from -start_from_text, the flat-vector table
    AETrainer.export_params writes for a text auto-encoder of arch NVQA_ARCH_AE1; the script's ae_temp.multimodal_net:clone()
    (:150) takes a module the text model does not have, so the bridge starts from nn.Linear's default, uniform +-1/sqrt(fan_in).
  * -lstm_average_path's /mean_vector [2R] is what the skipped encoder is replaced by (:299-301); without the option it is
    computed here, the mean of nvqa_ae1_wp_encode over the training sentences.
  * The skip draw (:299) uses torch.uniform() under torch.manualSeed(-seed), not Lua's math.random.
  * The log line ends with paramsNorm: the script's two cnn figures describe the body that is not here.
  * Instead of the thin nn checkpoints it writes what 005_convert_weakpaired_model_arch1.lua makes of them: {lookup = W_lk^T,
    encoder, multimodal, layout = 'nvqa'}, read by train_arch1_ae.lua -variant wp and
    VQATrainer.init_from_autoencoder(..., with_multimodal=True).
Needs LuaJIT + torch + hdf5 + cjson; NOT executable in the build image, where novel-vqa_amd/host/ae.py (WeakPairedAE1Trainer)
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
cmd:option('-start_from_text', '', 'flat-vector table of the arch1 text auto-encoder (AETrainer.export_params)')
cmd:option('-lstm_average_path', '', 'path to h5 file containing average lstm sentence vector (empty: computed from the training sentences)')
cmd:option('-body_in_loop', 0, '1: run the VGG-16 body inside the step on the raw images /images/<split> of -input_h5 (needs -cnn_weights)')
cmd:option('-cnn_weights', '', 'flat float32 file of the VGG-16 weights in nvqa_vgg16_set_weights order (-body_in_loop 1)')
cmd:option('-rnn_size',512,'size of the rnn in number of hidden nodes in each layer')
cmd:option('-input_encoding_size',512,'the encoding size of each token in the vocabulary')
cmd:option('-nhimage', 4096, 'feature width of the CNN body (vgg fc7 4096, inception 2048)')
cmd:option('-max_iters', -1, 'max number of iterations to run for (-1 = run forever)')
cmd:option('-batch_size',16,'what is the batch size in number of sentences per batch?')
cmd:option('-grad_clip',0.1,'clip gradients at this value')
cmd:option('-drop_prob_ae', 0.5, 'strength of dropout in the AutoEncoder RNN')
cmd:option('-optim','adam','what update to use? rmsprop|adagrad|sgd|sgdm|sgdmom|adam')
cmd:option('-learning_rate',3e-5,'learning rate')
cmd:option('-learning_rate_decay_start', -1, 'at what iteration to start decaying learning rate? (-1 = dont)')
cmd:option('-learning_rate_decay_every', 50000, 'every how many iterations thereafter to drop LR by half?')
cmd:option('-finetune_body', 0, '1: from -finetune_cnn_after on the VGG-16 body learns too (-body_in_loop 1): its backward inside the step, -cnn_optim on all its weights')
cmd:option('-finetune_cnn_after', -1, 'After what iteration do we start finetuning the CNN body? (-1 = never; read with -finetune_body 1)')
cmd:option('-cnn_optim','adam','optimization to use for the CNN body: sgd|sgdm|adam')
cmd:option('-cnn_optim_alpha',0.8,'alpha for momentum / adam of the CNN body')
cmd:option('-cnn_optim_beta',0.999,'beta for adam of the CNN body')
cmd:option('-cnn_learning_rate',1e-5,'learning rate for the CNN body')
cmd:option('-cnn_weight_decay', 0, 'L2 weight decay just for the CNN body')
cmd:option('-optim_alpha',0.8,'alpha for adagrad/rmsprop/momentum/adam')
cmd:option('-optim_beta',0.999,'beta used for adam')
cmd:option('-optim_epsilon',1e-8,'epsilon that goes into denominator for smoothing')
cmd:option('-weight_decay', 1e-6, 'L2 regularization parameter')
cmd:option('-val_sentences_use', 30000, 'how many sentences to use when periodically evaluating the validation loss?')
cmd:option('-save_checkpoint_every', 5000, 'how often to evaluate and save the best export table?')
cmd:option('-save_model_every', 12500, 'how often to save an export table regardless of the validation loss?')
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

-- the context: [encoder | decoder] and the frozen lookup from the text model; the bridge from nn.Linear's default ---------
opt.num_layers = 1                                   -- :137
opt.common_embedding_size, opt.num_output = 2 * opt.rnn_size, 0
local ctx = nvqa.create(6, opt, vocab_size, seq_length, opt.gpuid)
nvqa.check(nvqa.lib.nvqa_init_params(ctx, opt.seed, -0.08, 0.08))
local n_params = tonumber(nvqa.lib.nvqa_param_count(ctx))
local E, R, I = opt.input_encoding_size, opt.rnn_size, opt.nhimage
local seg = ffi.new('size_t[3]'); nvqa.check(nvqa.lib.nvqa_segments(ctx, seg))
local s0, s1, s2 = tonumber(seg[0]), tonumber(seg[1]), tonumber(seg[2])
do
  local t = torch.load(opt.start_from_text)
  local n_lk = (vocab_size + 1) * E
  assert(t.layout == 'nvqa' and t.params:nElement() == s0 + s1 + n_lk, 'the text model does not match this auto-encoder')
  local src = t.params:float():contiguous()
  local x = torch.FloatTensor(n_params)
  x:narrow(1, 1, s0 + s1):copy(src:narrow(1, 1, s0 + s1))
  local off = s0 + s1
  for _, fan_in in ipairs({2 * R, I}) do             -- W_q, b_q, W_v, b_v
    local k = 1 / math.sqrt(fan_in)
    x:narrow(1, off + 1, 2 * R * fan_in + 2 * R):uniform(-k, k)
    off = off + 2 * R * fan_in + 2 * R
  end
  nvqa.check(nvqa.lib.nvqa_set_params(ctx, nvqa.fptr(x)))
  nvqa.check(nvqa.lib.nvqa_ae1_wp_set_lookup(ctx, nvqa.fptr(src:narrow(1, s0 + s1 + 1, n_lk):contiguous())))
end

-- the corpus-mean sentence vector the skipped encoder is replaced by -------------------------------------------------------
local mean_vector
if string.len(opt.lstm_average_path) > 0 then
  local hf = hdf5.open(opt.lstm_average_path, 'r')
  mean_vector = hf:read('/mean_vector'):all():float():view(-1)
  hf:close()
  assert(mean_vector:nElement() == 2 * R, 'mean_vector must hold 2 * rnn_size values')
else
  local acc, used = torch.DoubleTensor(2 * R):zero(), 0
  local state = torch.FloatTensor(opt.batch_size, 2 * R)
  local n_train = labels.train:size(1)
  for i = 1, n_train - opt.batch_size + 1, opt.batch_size do
    local rows = labels.train:narrow(1, i, opt.batch_size):contiguous()
    nvqa.check(nvqa.lib.nvqa_ae1_wp_encode(ctx, opt.batch_size, nvqa.iptr(rows), nvqa.fptr(state)))
    acc:add(state:double():sum(1):view(-1))
    used = used + opt.batch_size
  end
  mean_vector = acc:div(used):float()
end
local mean_rows = torch.repeatTensor(mean_vector:view(1, -1), opt.batch_size, 1):contiguous()   -- :300

local function eval_split(split)                    -- eval_split (:212-275): forward{feats, labels, labels, 0}
  iterators[split] = 1
  local loss_sum, evals, n = 0, 0, 0
  local loss = ffi.new('float[1]')
  while true do
    local batch, fb, wrapped = getBatch(split, opt.batch_size)
    if body then
      local xoff, yoff = nvqa.crop_origin(img_size, false)
      nvqa.check(nvqa.lib.nvqa_ae1_wp_evaluate_images(ctx, body, opt.batch_size, nvqa.bptr(fb), img_size, xoff, yoff, nil,
                                                      nvqa.iptr(batch), nvqa.iptr(batch), loss, nil))
    else
      nvqa.check(nvqa.lib.nvqa_ae1_wp_evaluate(ctx, opt.batch_size, nvqa.fptr(fb), nvqa.iptr(batch), nvqa.iptr(batch), loss, nil))
    end
    loss_sum = loss_sum + loss[0]; evals = evals + 1
    n = n + opt.batch_size
    if wrapped then break end
    if n >= opt.val_sentences_use then break end
  end
  return loss_sum / evals
end

local function export(path)                          -- 005_convert_weakpaired_model_arch1.lua's table
  local x = torch.FloatTensor(n_params)
  nvqa.check(nvqa.lib.nvqa_get_params(ctx, nvqa.fptr(x)))
  local lookup = torch.FloatTensor(vocab_size + 1, E)
  nvqa.check(nvqa.lib.nvqa_ae1_wp_get_lookup(ctx, nvqa.fptr(lookup)))
  torch.save(path, {lookup = lookup:t():clone(), encoder = x:narrow(1, 1, s0):clone(),
                    multimodal = x:narrow(1, s0 + s1 + 1, s2):clone(), layout = 'nvqa'})
end

-- main loop (:359-420) ------------------------------------------------------------------------------------------------
local iter, loss0, best_score = 1, nil, nil
local loss, stats, cnn_stats = ffi.new('float[1]'), ffi.new('float[2]'), ffi.new('float[2]')
local checkpoint_path = paths.concat(opt.checkpoint_path, 'model_id' .. opt.id)
while true do
  local batch, fb = getBatch('train', opt.batch_size)
  local dr = nvqa.dropout(1, opt.drop_prob_ae, opt.seed, iter)
  local skip = torch.uniform() <= 0.5                                              -- encoder_skip_flag = 1 (:299-301)
  local enc_tokens, enc_state = nvqa.iptr(batch), nil
  if skip then enc_tokens, enc_state = nil, nvqa.fptr(mean_rows) end
  local body_learns = body ~= nil and opt.finetune_body == 1 and opt.finetune_cnn_after >= 0 and iter >= opt.finetune_cnn_after
  if body_learns then                                                              -- ... + cnn:backward(data.imgs, dfeats) (:329)
    local xoff, yoff = nvqa.crop_origin(img_size, true)
    nvqa.check(nvqa.lib.nvqa_ae1_wp_step_images_finetune(ctx, body, nvqa.bptr(fb), img_size, xoff, yoff,
                                                         nvqa.body_dropout(true, opt.seed, iter), enc_tokens, enc_state,
                                                         nvqa.iptr(batch), dr, loss, nil))
  elseif body then                                                                 -- prepro(data.images, true, ...) + cnn:forward
    local xoff, yoff = nvqa.crop_origin(img_size, true)
    nvqa.check(nvqa.lib.nvqa_ae1_wp_step_images(ctx, body, nvqa.bptr(fb), img_size, xoff, yoff,
                                                nvqa.body_dropout(true, opt.seed, iter), enc_tokens, enc_state, nvqa.iptr(batch),
                                                dr, loss, nil))
  else
    nvqa.check(nvqa.lib.nvqa_ae1_wp_step(ctx, nvqa.fptr(fb), enc_tokens, enc_state, nvqa.iptr(batch), dr, loss, nil))
  end
  local learning_rate = opt.learning_rate
  if iter > opt.learning_rate_decay_start and opt.learning_rate_decay_start >= 0 then
    learning_rate = learning_rate * math.pow(0.5, (iter - opt.learning_rate_decay_start) / opt.learning_rate_decay_every)
  end
  if opt.optim == 'adam' then  -- the script's default keeps its own entry point: the same kernel, state and bits as the rule
    nvqa.check(nvqa.lib.nvqa_adam_update(ctx, learning_rate, opt.optim_alpha, opt.optim_beta, opt.optim_epsilon,
                                         opt.weight_decay, opt.grad_clip, stats))
  else
    nvqa.optim_update(ctx, opt, learning_rate, stats)
  end
  if body_learns then                                                              -- the cnn vector, scales all 1 (:182, :477-484)
    local clamp = 0
    if opt.cnn_weight_decay > 0 then clamp = opt.grad_clip end
    local cnn_rule = nvqa.CNN_OPT[opt.cnn_optim]
    if cnn_rule == nil then error('bad option for opt.cnn_optim (sgd | sgdm | adam)') end
    nvqa.check(nvqa.lib.nvqa_vgg16_update(body, cnn_rule, opt.cnn_learning_rate * learning_rate / opt.learning_rate, opt.cnn_optim_alpha,
                                          opt.cnn_optim_beta, opt.optim_epsilon, opt.cnn_weight_decay, clamp, 1, cnn_stats))
    print(string.format('iter %d: loss: %.3f | # updates: %4d | paramsNorm: %.4f | # cnn updates: %4d | cnnParamsNorm: %.4f',
                        iter, loss[0], stats[1], stats[0], cnn_stats[1], cnn_stats[0]))
  else
    print(string.format('iter %d: loss: %.3f | # updates: %4d | paramsNorm: %.4f', iter, loss[0], stats[1], stats[0]))
  end
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
