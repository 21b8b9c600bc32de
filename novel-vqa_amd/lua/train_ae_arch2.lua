--[[
train_ae_arch2.lua -- 001_train_autoencoder/001_train_arch2_text_autoencoder.lua with the hot path on libnvqa.

Same command-line options (:22-58, minus -backend / -language_eval), same HDF5/JSON inputs (misc/DataLoader.lua, whose
image rows are zeros, :84), same log line (:271-273), learning-rate decay (:342-348), update (-optim rmsprop | adagrad | sgd | sgdm | sgdmom | adam) and
stopping rules (:367-375); num_layers is 1 as in the script (:104).  eval_split counts the sentences it used and stops at
-val_sentences_use (:192-195).  What changed: the AutoEncoder / LanguageModelCriterion modules, their clones, lossFun and
the optimiser are one library context of arch NVQA_ARCH_AE2 (include/nvqa.h), where nvqa_ae_step feeds the zero image
rows.  Instead of the thin nn checkpoints (best validation loss every -save_checkpoint_every, every -save_model_every) it
writes the table that convert_ae_arch2.lua makes ({encoder, lookup_table}) plus layout = 'nvqa', which train_arch2_ae.lua
and VQATrainer.init_from_autoencoder read without -encoder_perm.  Needs LuaJIT + torch + hdf5 + cjson; NOT executable in
the build image, where novel-vqa_amd/host/ae.py (AETrainer) is the executed twin.

Data parallel (absent in the reference): -world N -rank r -comm_id_file F runs one process per GPU (nvqa_ae_comm_init).
Rank 0 writes the 128-byte communicator id to F, the others wait for it and read it; -batch_size is the batch PER RANK, the
training iterator walks strides of world * batch_size rows of which rank r takes its block, the dropout masks come from
seed + 1000 * rank, and the step ends with the global batch's gradient and loss, so every rank prints the same log line.
Validation is rank-local over the same rows on every rank; rank 0 alone writes the export tables.  -world 1 (the default)
creates no communicator.  F must not exist when the job starts: a rank above 0 reads it as soon as it is there, and an id left by
an earlier run would make ncclCommInitRank wait for ranks that never come.  Rank 0 removes a stale F first thing, before it
loads the data, and removes its own F again when the communicator stands; start rank 0 first, or use a fresh name per job.

-resident 1 (absent in the reference): [train | val] is copied to HBM once (nvqa_ae_corpus_load) and every training and
validation batch is named by its row ids (nvqa_ae_step_rows / nvqa_ae_evaluate_rows): the same rows from the same iterator,
rank stride included, and the same bits (DESIGN.md section 9.7).
]]--
require 'torch'
require 'hdf5'
local cjson = require 'cjson'
local ffi = require 'ffi'
local nvqa = require 'nvqa_ffi'

cmd = torch.CmdLine()
cmd:option('-input_h5','data/data.h5','path to the h5file containing the preprocessed dataset')
cmd:option('-input_json','data/data.json','path to the json file containing additional info and vocab')
cmd:option('-rnn_size',512,'size of the rnn in number of hidden nodes in each layer')
cmd:option('-input_encoding_size',512,'the encoding size of each token in the vocabulary, and the image.')
cmd:option('-max_iters', 40001, 'max number of iterations to run for (-1 = run forever)')
cmd:option('-batch_size',1000,'what is the batch size in number of sentences per batch?')
cmd:option('-grad_clip',0.1,'clip gradients at this value')
cmd:option('-drop_prob_ae', 0.5, 'strength of dropout in the AutoEncoder RNN')
cmd:option('-optim','adam','what update to use? rmsprop|adagrad|sgd|sgdm|sgdmom|adam')
cmd:option('-learning_rate',5e-5,'learning rate')
cmd:option('-learning_rate_decay_start', -1, 'at what iteration to start decaying learning rate? (-1 = dont)')
cmd:option('-learning_rate_decay_every', 50000, 'every how many iterations thereafter to drop LR by half?')
cmd:option('-optim_alpha',0.8,'alpha for adagrad/rmsprop/momentum/adam')
cmd:option('-optim_beta',0.999,'beta used for adam')
cmd:option('-optim_epsilon',1e-8,'epsilon that goes into denominator for smoothing')
cmd:option('-weight_decay', 1e-6, 'L2 regularization parameter')
cmd:option('-val_sentences_use', 30000, 'how many sentences to use when periodically evaluating the validation loss?')
cmd:option('-save_checkpoint_every', 2500, 'how often to evaluate and save the best export table?')
cmd:option('-save_model_every', 40000, 'how often to save an export table regardless of the validation loss?')
cmd:option('-checkpoint_path', '', 'folder to save checkpoints into (empty = this folder)')
cmd:option('-id', '', 'an id identifying this run/job')
cmd:option('-seed', 123, 'random number generator seed to use')
cmd:option('-gpuid', 0, 'which MI355X to use')
cmd:option('-bf16', 0, '1 = bf16 operands for every dense product of the step, f32 accumulate (nvqa_ae_set_precision)')
cmd:option('-resident', 0, '1 = the label sets stay in HBM (nvqa_ae_corpus_load) and every batch is named by its row ids')
cmd:option('-rank', 0, 'data parallel: this process\'s rank, 0 .. world - 1')
cmd:option('-world', 1, 'data parallel: number of processes (1 = no communicator)')
cmd:option('-comm_id_file', '', 'data parallel: file through which rank 0 hands the communicator id to the other ranks')
opt = cmd:parse(arg)
assert(opt.world >= 1 and opt.rank >= 0 and opt.rank < opt.world, 'bad -rank / -world')
if opt.world > 1 and opt.rank == 0 and opt.comm_id_file ~= '' then os.remove(opt.comm_id_file) end  -- a stale id of an earlier run
torch.manualSeed(opt.seed)

-- data (misc/DataLoader.lua:6-31) ------------------------------------------------------------------------------------
local f = io.open(opt.input_json, 'r'); local info = cjson.decode(f:read('*a')); f:close()
local vocab_size = 0
for _ in pairs(info.ix_to_word) do vocab_size = vocab_size + 1 end
local h5 = hdf5.open(opt.input_h5, 'r')
local labels = {train = h5:read('/labels/train'):all():int(), val = h5:read('/labels/val'):all():int()}
h5:close()
local seq_length = labels.train:size(2)
local iterators = {train = 1, val = 1}

local function getBatch(split, batch_size)          -- DataLoader:getBatch (:58-89), wrap-around included
  local data, max_index, it = labels[split], labels[split]:size(1), iterators[split]
  local batch = torch.IntTensor(batch_size, seq_length)
  local wrapped = false
  if it + batch_size - 1 > max_index then
    wrapped = true
    if it < max_index then
      local num_left = max_index - it + 1
      batch[{{1, num_left}, {}}] = data[{{it, max_index}, {}}]
      batch[{{num_left + 1, batch_size}, {}}] = data[{{1, batch_size - num_left}, {}}]
    else
      batch:copy(data[{{1, batch_size}, {}}])
    end
    iterators[split] = 1
  else
    batch:copy(data[{{it, it + batch_size - 1}, {}}])
    iterators[split] = it + batch_size
  end
  return batch:contiguous(), wrapped
end

-- the context: [encoder | decoder | lookup], *_w:uniform(-0.08, 0.08); one LSTM layer (:104) ----------------------------
opt.num_layers = 1
opt.nhimage, opt.common_embedding_size, opt.num_output = 0, 0, 0
local ctx = nvqa.create(4, opt, vocab_size, seq_length, opt.gpuid)
nvqa.check(nvqa.lib.nvqa_init_params(ctx, opt.seed, -0.08, 0.08))
nvqa.check(nvqa.lib.nvqa_ae_set_precision(ctx, opt.bf16))
local n_params = tonumber(nvqa.lib.nvqa_param_count(ctx))
if opt.world > 1 then                               -- the parameters above came from -seed on every rank: identical replicas
  assert(opt.comm_id_file ~= '', '-world > 1 needs -comm_id_file')
  local id = ffi.new('char[128]')
  if opt.rank == 0 then
    nvqa.check(nvqa.lib.nvqa_comm_unique_id(id))
    local fh = assert(io.open(opt.comm_id_file .. '.tmp', 'wb')); fh:write(ffi.string(id, 128)); fh:close()
    assert(os.rename(opt.comm_id_file .. '.tmp', opt.comm_id_file))
  else
    local fh = io.open(opt.comm_id_file, 'rb')
    while not fh do os.execute('sleep 0.1'); fh = io.open(opt.comm_id_file, 'rb') end
    local bytes = fh:read(128); fh:close()
    assert(bytes and #bytes == 128, 'short communicator id in ' .. opt.comm_id_file)
    ffi.copy(id, bytes, 128)
  end
  nvqa.check(nvqa.lib.nvqa_ae_comm_init(ctx, opt.rank, opt.world, id))
  if opt.rank == 0 then os.remove(opt.comm_id_file) end  -- every rank has read it: ncclCommInitRank returns when all have joined
end
-- -resident 1: [train | val] in HBM once; a batch is then getBatch's rows by number (0-based, same iterator, same wrap)
local first_row = {train = 0, val = labels.train:size(1)}
if opt.resident == 1 then
  local corpus = torch.cat(labels.train, labels.val, 1):contiguous()
  nvqa.check(nvqa.lib.nvqa_ae_corpus_load(ctx, corpus:size(1), nvqa.iptr(corpus)))
end
local function getRows(split, batch_size)
  local max_index, it = labels[split]:size(1), iterators[split]
  local rows, wrapped, num_left = torch.LongTensor(batch_size), false, 0
  if it + batch_size - 1 > max_index then
    wrapped = true
    if it < max_index then num_left = max_index - it + 1 end
    for i = 1, batch_size do
      rows[i] = first_row[split] + (i <= num_left and it + i - 2 or i - num_left - 1)
    end
    iterators[split] = 1
  else
    for i = 1, batch_size do rows[i] = first_row[split] + it + i - 2 end
    iterators[split] = it + batch_size
  end
  return rows, wrapped
end
local dropout_seed = opt.seed + 1000 * opt.rank     -- ranks hold different sentences: identical masks would correlate them

local function eval_split(split)                    -- eval_split (:148-204): mean of the per-batch losses
  iterators[split] = 1
  local loss_sum, evals, n = 0, 0, 0
  local loss = ffi.new('float[1]')
  while true do
    local wrapped
    if opt.resident == 1 then
      local rows
      rows, wrapped = getRows(split, opt.batch_size)
      nvqa.check(nvqa.lib.nvqa_ae_evaluate_rows(ctx, opt.batch_size, nvqa.lptr(rows), loss, nil))
    else
      local batch
      batch, wrapped = getBatch(split, opt.batch_size)
      nvqa.check(nvqa.lib.nvqa_ae_evaluate(ctx, opt.batch_size, nvqa.iptr(batch), loss, nil))
    end
    loss_sum = loss_sum + loss[0]; evals = evals + 1
    n = n + opt.batch_size
    if wrapped then break end
    if n >= opt.val_sentences_use then break end
  end
  return loss_sum / evals
end

local function export(path)                          -- convert_ae_arch2.lua's table + layout = 'nvqa'
  if opt.rank ~= 0 then return end                   -- identical replicas: one writer
  local x = torch.FloatTensor(n_params)
  nvqa.check(nvqa.lib.nvqa_get_params(ctx, nvqa.fptr(x)))
  local seg = ffi.new('size_t[3]'); nvqa.check(nvqa.lib.nvqa_segments(ctx, seg))
  local s0, s1 = tonumber(seg[0]), tonumber(seg[1])
  local lookup = x:narrow(1, s0 + s1 + 1, tonumber(seg[2])):view(vocab_size + 1, opt.input_encoding_size)
  torch.save(path, {encoder = x:narrow(1, 1, s0):clone(), lookup_table = lookup:clone(), layout = 'nvqa'})
end

-- main loop (:265-376) ------------------------------------------------------------------------------------------------
local iter, loss0, best_score = 1, nil, nil
local loss, stats = ffi.new('float[1]'), ffi.new('float[2]')
local checkpoint_path = paths.concat(opt.checkpoint_path, 'model_id' .. opt.id)
while true do
  if opt.resident == 1 then
    local rows = getRows('train', opt.batch_size * opt.world)
    if opt.world > 1 then rows = rows:narrow(1, opt.rank * opt.batch_size + 1, opt.batch_size):contiguous() end
    nvqa.check(nvqa.lib.nvqa_ae_step_rows(ctx, nvqa.lptr(rows), nvqa.dropout(1, opt.drop_prob_ae, dropout_seed, iter), loss))
  else
    local batch = getBatch('train', opt.batch_size * opt.world)
    if opt.world > 1 then batch = batch:narrow(1, opt.rank * opt.batch_size + 1, opt.batch_size):contiguous() end
    nvqa.check(nvqa.lib.nvqa_ae_step(ctx, nvqa.iptr(batch), nvqa.dropout(1, opt.drop_prob_ae, dropout_seed, iter), loss))
  end
  local learning_rate = opt.learning_rate
  if iter > opt.learning_rate_decay_start and opt.learning_rate_decay_start >= 0 then
    local frac = (iter - opt.learning_rate_decay_start) / opt.learning_rate_decay_every
    learning_rate = learning_rate * math.pow(0.5, frac)
  end
  if opt.optim == 'adam' then  -- the script's default keeps its own entry point: the same kernel, state and bits as the rule
    nvqa.check(nvqa.lib.nvqa_adam_update(ctx, learning_rate, opt.optim_alpha, opt.optim_beta, opt.optim_epsilon,
                                         opt.weight_decay, opt.grad_clip, stats))
  else
    nvqa.optim_update(ctx, opt, learning_rate, stats)
  end
  print(string.format('iter %d: loss: %.3f | # updates: %4d | paramsNorm: %.4f', iter, loss[0], stats[1], stats[0]))
  if iter % opt.save_checkpoint_every == 0 or iter == opt.max_iters then
    local val_loss = eval_split('val')
    print('validation loss: ', val_loss)
    if best_score == nil or -val_loss > best_score then  -- the negative validation loss decides (:300-322)
      best_score = -val_loss
      export(checkpoint_path .. '_vqa.t7')
      if opt.rank == 0 then print('wrote BEST export table to ' .. checkpoint_path .. '_vqa.t7') end
    end
  end
  if iter % opt.save_model_every == 0 then
    export(checkpoint_path .. iter .. '_vqa.t7')
    if opt.rank == 0 then print('wrote export table to ' .. checkpoint_path .. iter .. '_vqa.t7') end
  end
  iter = iter + 1
  if loss0 == nil then loss0 = loss[0] end
  if loss[0] > loss0 * 20 then print('loss seems to be exploding, quitting.'); break end
  if opt.max_iters > 0 and iter >= opt.max_iters then break end
end
